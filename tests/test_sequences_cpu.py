"""No GPU: what tests/test_gpu_sequences.py rests on.  The table of tests/sequence_cases.py has the properties it is written for -- every
ordered pair of a plan's pure kinds adjacent somewhere, every pure kind compared in every state a twin is built in, batch sizes that rise
and fall, constant random walks -- and its plans are planned as it says: the switchable plan with two full arenas at the smallest
max_batch that gives them, the others with the stream count they name, the exact chains with the kernels they are in the table for.  The
number of twins a plan needs (one engine built per key) stays under the cap written in the table."""
import ctypes as C

import pytest

import poison_cases as P
import sequence_cases as S
import test_gpu_exact as E
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine


def all_sequences(sid):
    return S.sequences_of(sid)


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", S.ALL_PLANS)
def test_calls_are_well_formed(sid):
    pl = S.PLANS[sid]
    mb = S.plan_kw(sid)["max_batch"]
    for name, seq in all_sequences(sid).items():
        for c in seq:
            if c[0] == S.REFUSE:
                assert c[1] in pl["refusals"] and c[1] in S.REFUSALS, (sid, name, c)
            elif S.is_changing(c):
                assert c[0] in S.CHANGING and (pl["train"] or c[0] not in ("train", "train_u8", "head_train_init", "load_weights")), (sid, name, c)
            else:
                assert c[0] in pl["kinds"], (sid, name, c)
                lo, n = c[1], c[2]
                assert 1 <= n <= mb and (n > S.N_IMAGES or (0 <= lo and lo + n <= S.N_IMAGES)), (sid, name, c)
    assert set(pl["kinds"]) <= set(S.FORWARD) | set(S.DETECT) | set(S.LOSS) | {S.REFUSE}
    if "loss" in pl["kinds"]:
        assert P.PLANS[pl["pid"]]["net"].startswith("v2")
    assert max(t[4] for img in S.TRUTHS for t in img) < 20 and max(len(img) for img in S.TRUTHS) <= S.MAX_GT and [] in S.TRUTHS


def test_pure_and_changing_calls_are_the_issue_s():
    assert set(S.CHANGING) == {"train", "train_u8", "head_train_init", "load_weights", "rebind", "set_streams", "autotune", "tune_streams"}
    thresholds = {(m, t) for m, t, _ in S.DETECT.values()}
    assert {("detect", 0.5), ("detect", 0.05), ("detect", 0.9999), ("detect_u8", 0.5), ("detect_frames", 0.5)} <= thresholds
    for t in (0.5, 0.05, 0.9999):       # both NMS modes
        assert {mode for m, thr, mode in S.DETECT.values() if m == "detect" and thr == t} == {_hip.NMS_AGNOSTIC, _hip.NMS_PER_CLASS}
    assert S.is_sparse_detect(("detect@0.5", 0, 1)) and S.is_sparse_detect(("detect@0.05/per-class", 0, 1))
    assert not S.is_sparse_detect(("detect@0.9999", 0, 1)) and not S.is_sparse_detect(("forward", 0, 1))       # inside 1e-4 of 1: the dense branch
    assert 1.0 - 0.9999 <= 1e-4 + 1e-12
    assert set(S.V2_KINDS) == set(S.V3_KINDS) | set(S.LOSS)


# ---- the walks -----------------------------------------------------------------------------------------------------------------------------
def test_euler_walk_covers_every_ordered_pair_once():
    for k in (1, 2, 5, 12, 15):
        kinds = ["k%d" % i for i in range(k)]
        walk = S.euler_kinds(kinds)
        pairs = list(zip(walk, walk[1:]))
        assert len(pairs) == k * k and len(set(pairs)) == k * k and walk[0] == walk[-1], k


@pytest.mark.parametrize("sid", S.MAIN)
def test_every_ordered_pair_of_pure_kinds_is_adjacent(sid):
    kinds = S.PLANS[sid]["kinds"]
    walk = S.SEQUENCES[sid]["cover"]
    pairs = {(a[0], b[0]) for a, b in zip(walk, walk[1:])}
    missing = [(a, b) for a in kinds for b in kinds if (a, b) not in pairs]
    assert not missing, (sid, missing[:5])
    # each step of a kind that has a batch runs at a batch size different from the last call's that had one
    prev = None
    for c in walk:
        n = S.batch_of(c)
        if n is not None:
            assert n != prev, (sid, c, prev)
            prev = n
    # both slices of every kind are used
    for kind in kinds:
        if kind != S.REFUSE:
            assert {(c[1], c[2]) for c in walk if c[0] == kind} >= set(S.variants(kinds, kind)), (sid, kind)
            a, b = S.variants(kinds, kind)
            assert a[1] != b[1]
    assert {c[1] for c in walk if c[0] == S.REFUSE} == set(S.PLANS[sid]["refusals"])


@pytest.mark.parametrize("sid", S.MAIN)
def test_the_named_leaks_are_in_the_covering_walk(sid):
    walk = S.SEQUENCES[sid]["cover"]

    def adjacent(a, b, other_images=False):
        return any(x[0] == a and y[0] == b and x[2] != y[2] and (not other_images or (x[1], x[2]) != (y[1], y[2]) and y[1] + y[2] > x[1] + x[2])
                   for x, y in zip(walk, walk[1:]))
    assert adjacent("detect@0.5", "forward")                              # obj_min_logit
    assert adjacent("detect@0.5", "detect@0.05", other_images=True)       # rows the first did not write, images it did not see
    assert adjacent("detect@0.9999", "detect@0.5") and adjacent("detect@0.5", "detect@0.9999")
    assert adjacent("forward_timed", "detect@0.5")                        # obj_valid, halves
    if "loss" in S.PLANS[sid]["kinds"]:
        assert any(a[0] == "loss" and b[0].startswith("detect") and c[0] == "loss_grad" for a, b, c in zip(walk, walk[1:], walk[2:]))


@pytest.mark.parametrize("sid", S.ALL_PLANS)
def test_batch_sizes_rise_and_fall_in_every_walk(sid):
    for name, seq in all_sequences(sid).items():
        ns = [S.batch_of(c) for c in seq if S.is_pure(c) and S.batch_of(c) is not None]
        steps = [b - a for a, b in zip(ns, ns[1:])]
        assert any(s > 0 for s in steps) and any(s < 0 for s in steps), (sid, name, ns)


def test_random_walks_regenerate_identically():
    for sid in S.MAIN:
        a, b = S.random_walk(sid), S.random_walk(sid)
        assert a == b == S.SEQUENCES[sid]["random"] and len(a) == 24 and all(S.is_pure(c) for c in a), sid
        assert a != S.random_walk(sid, seed=1)
    assert S.SEQUENCES["v3-fp16"]["random"][:3] == [("detect@0.05", 1, 3), ("detect_frames@0.5", 0, 3), ("detect@0.9999/per-class", 0, 1)]     # seed 0, written out


@pytest.mark.parametrize("sid", S.ALL_PLANS)
def test_every_pure_kind_is_compared_in_every_state_a_twin_is_built_in(sid):
    """a state = a tuple of changing calls a twin replays: behind every changing call of the table, before the next one, the plan's
    sequences together compare every pure kind the plan supports"""
    kinds = set(S.PLANS[sid]["kinds"])
    seen = {}
    for prefix, call in S.twin_keys(sid):
        if S.is_pure(call):
            seen.setdefault(prefix, set()).add(call[0])
    changed = {S.twin_key(seq, i + 1)[0] for seq in all_sequences(sid).values() for i, c in enumerate(seq) if S.is_changing(c) and i + 1 < len(seq)
               and S.is_pure(seq[i + 1])}
    assert changed <= set(seen)
    for prefix in sorted(seen):
        assert seen[prefix] == kinds, (sid, prefix, sorted(kinds - seen[prefix]))


def test_twin_keys():
    seq = [("forward", 0, 1), ("head_train_init",), ("train", 0, 3, 1), ("detect@0.5", 0, 2), ("train_u8", 1, 2, 2), ("loss", 0, 1), ("load_weights",),
           ("forward", 0, 1), ("rebind",), ("head_train_init",), ("train", 0, 3, 1), ("forward", 0, 2)]
    assert S.twin_key(seq, 0) == ((), ("forward", 0, 1))
    assert S.twin_key(seq, 2) == ((("head_train_init",),), ("train", 0, 3, 1))
    assert S.twin_key(seq, 3) == ((("head_train_init",), ("train", 0, 3, 1)), ("detect@0.5", 0, 2))
    assert S.twin_key(seq, 5)[0] == (("head_train_init",), ("train", 0, 3, 1), ("train_u8", 1, 2, 2))
    assert S.twin_key(seq, 7) == S.twin_key(seq, 0)                                     # load_weights: the untrained twin
    assert S.twin_key(seq, 10) == ((("rebind",), ("head_train_init",)), ("train", 0, 3, 1))       # the first step again, on a re-bound workspace
    # in the table: the pure calls behind load_weights have the keys of the untrained twins, the step behind the second init the key of the first
    for sid in ("v2-fp16", "v2-fp32"):
        s = S.SEQUENCES[sid]["train-u8-load-init"]
        i = s.index(("load_weights",))
        assert all(S.twin_key(s, j)[0] == () for j in range(i + 1, i + 1 + 2 * len(S.PLANS[sid]["kinds"])))
        j = len(s) - 1 - s[::-1].index(("train", 0, 3, 1))
        assert j > i and S.twin_key(s, j) == S.twin_key(s, 1)
        assert any(c[0] == "train_u8" for c in s)


@pytest.mark.parametrize("sid", S.ALL_PLANS)
def test_the_number_of_twins_stays_under_the_cap(sid):
    n = len(S.twin_keys(sid))
    print("%s: %d twin keys (cap %d)" % (sid, n, S.TWIN_KEY_CAP))
    assert 0 < n <= S.TWIN_KEY_CAP


def test_items():
    assert len(S.ITEMS) == len(set(S.ITEMS)) and {it[0] for it in S.ITEMS} == set(S.ALL_PLANS)
    assert S.ITEMS == S.items()
    parts = {}
    for sid, name, part, start, end in S.ITEMS:
        parts.setdefault((sid, name), []).append((part, start, end))
    assert set(parts) == {(sid, name) for sid in S.ALL_PLANS for name in all_sequences(sid)}
    met = {}
    for (sid, name), ps in parts.items():       # the parts of a sequence, in order, compare every call of it exactly once
        seq = all_sequences(sid)[name]
        assert [p[0] for p in ps] == list(range(1, len(ps) + 1)) and ps[0][1] == 0 and ps[-1][2] == len(seq), (sid, name, ps)
        assert all(a[2] == b[1] and a[1] < a[2] for a, b in zip(ps, ps[1:])), (sid, name, ps)
    for sid, name, part, start, end in S.ITEMS:      # ... and none has more than TWINS_PER_ITEM twins to build
        seq = all_sequences(sid)[name]
        keys = {S.twin_key(seq, i) for i in range(start, end) if not (S.is_changing(seq[i]) and seq[i][0] not in ("train", "train_u8"))}
        new = keys - met.setdefault(sid, set())
        assert len(new) <= S.TWINS_PER_ITEM, (sid, name, part, len(new))
        met[sid] |= keys
    for sid in S.MAIN:
        assert {"cover", "random", "refusals"} <= set(S.SEQUENCES[sid])
    assert sum("rebind" in S.SEQUENCES[sid] for sid in S.MAIN) == 3
    for sid, name in (("v2-fp16", "rebind"), ("v3-fp16", "rebind"), ("v3-tiny-fp32", "rebind")):
        s = S.SEQUENCES[sid][name]
        assert 0 < s.index(("rebind",)) < len(s) - 1
    for sid in S.MAIN:       # every refusal of the plan between two calls that are compared
        s = S.SEQUENCES[sid]["refusals"]
        for w in S.PLANS[sid]["refusals"]:
            i = s.index((S.REFUSE, w))
            assert S.batch_of(s[i - 1]) is not None and S.batch_of(s[i + 1]) is not None
    assert {p for p, _ in S.INTERLEAVED} == set(S.PAIR) and S.PLANS[S.PAIR[0]]["pid"] != S.PLANS[S.PAIR[1]]["pid"]
    assert all(a[0] != b[0] for a, b in zip(S.INTERLEAVED, S.INTERLEAVED[1:]))
    for sid, c in S.INTERLEAVED:
        assert ((), c) in S.twin_keys(sid)
    assert set(S.ASYNC_PLANS) == {"v2-fp16", "v3-fp16"}


# ---- the plans -----------------------------------------------------------------------------------------------------------------------------
def test_the_plans_are_the_issue_s():
    rows = {sid: (P.PLANS[pl["pid"]]["net"], P.PLANS[pl["pid"]]["dtype"]) for sid, pl in S.PLANS.items()}
    assert {rows[s] for s in S.MAIN} == {("v2", "fp16"), ("v2", "fp32"), ("v2-tiny", "fp16"), ("v3", "fp16"), ("v3", "mxfp8"), ("v3-spp", "fp16"), ("v3-tiny", "fp32")}
    assert {s for s in S.PLANS if S.PLANS[s]["train"]} == {"v2-fp16", "v2-fp32"}
    for sid in S.MAIN:
        assert S.PLANS[sid]["more"] == {"streams": 1, "max_batch": 4} and not P.PLANS[S.PLANS[sid]["pid"]]["keep_all"]


@pytest.mark.parametrize("sid", S.MAIN + ("v2-fp16-two-parts",))
def test_plan_runs_the_stream_count_it_names(sid):
    p = S.plan_only(sid)
    assert p.num_streams == S.PLANS[sid]["streams"] >= 1 and p.max_batch == S.MAX_BATCH
    assert p.lib.yolo_net_set_streams(p.handle, 3) == S.REFUSALS["set_streams(3)"][0]
    for s in P.FEATURES.get(S.PLANS[sid]["pid"], ()):       # what the row is in poison_cases for, at this max_batch as well
        names, text = E.kernel_text(p, [E._info(p, k, C, _hip) for k in range(p.num_kernels)])
        assert s in text, (sid, s)
    if sid == "v2-fp16-two-parts":
        assert p.lib.yolo_net_set_streams(p.handle, 1) == S.REFUSALS["set_streams(1)-split-arenas"][0]
        assert S.REFUSALS["set_streams(1)-split-arenas"][1] in p.lib.yolo_last_error().decode()


def test_the_switchable_plan_has_two_full_arenas_at_the_smallest_max_batch():
    mb = S.switch_max_batch()
    p = S.plan_only("v3-fp16-switch")
    assert p.max_batch == mb and p.num_streams == 2
    # two arenas, each sized for the WHOLE batch: every tensor of arena 0 is there again in arena 1 with the same bytes, a multiple of max_batch
    regions = p.workspace_regions()
    a0 = {n[:-len(" arena 0")]: used for n, _, used, _ in regions if n.endswith(" arena 0")}
    a1 = {n[:-len(" arena 1")]: used for n, _, used, _ in regions if n.endswith(" arena 1")}
    assert a0 and a0 == a1 and all(u % mb == 0 for u in a0.values())
    one = engine.Plan(P.create_network("v3"), dtype="fp16", max_batch=mb, streams=1)
    assert {n[:-len(" arena 0")]: used for n, _, used, _ in one.workspace_regions() if n.endswith(" arena 0")} == a0
    # the switch is accepted both ways, and back
    for k in (1, 2, 1):
        assert p.lib.yolo_net_set_streams(p.handle, k) == 0 and p.num_streams == k
    assert p.lib.yolo_net_set_streams(p.handle, 3) == S.ERR_STATE
    # ... and one image fewer is not given two arenas by the rule
    less = engine.Plan(P.create_network("v3"), dtype="fp16", max_batch=mb - 1, streams=0)
    assert less.num_streams == 1 and less.lib.yolo_net_set_streams(less.handle, 2) == S.ERR_STATE
    # the batches of its sequences: two parts for the full batch and for one image more than half, one part for 4, 2 and 3 (2 * b <= max_batch)
    ns = {S.batch_of(c) for seq in S.sequences_of("v3-fp16-switch").values() for c in seq if S.batch_of(c)}
    assert ns == {mb, mb // 2 + 1, 4, 2, 3} and 2 * 4 <= mb < 2 * (mb // 2 + 1)
    seq = S.sequences_of("v3-fp16-switch")["switch"]
    assert [c for c in seq if S.is_changing(c)] == [("set_streams", 2), ("set_streams", 1), ("set_streams", 2)] and S.is_changing(seq[0])


def test_yolov2_is_never_given_two_full_arenas():
    """why the refused train step runs on a streams = 2 plan, which cannot be switched back"""
    for mb in (4, 64, 512):
        p = engine.Plan(P.create_network("v2"), dtype="fp16", max_batch=mb, streams=0)
        assert p.num_streams == 1 and p.lib.yolo_net_set_streams(p.handle, 2) == S.ERR_STATE


@pytest.mark.parametrize("cid", sorted(S.EXACT_CHAINS))
def test_exact_chain_names_its_kernel(cid):
    spec = S.EXACT_CHAINS[cid]
    c = E.CASES[E.IDS.index(cid)]
    assert spec["variant"] in c["variants"] and c["tile"] is None and not c["kw"]
    p = engine.Plan(E.build_graph(c, spec["variant"]), dtype=c["dtype"], max_batch=S.EXACT_BATCH)
    names, text = E.kernel_text(p, [E._info(p, k, C, _hip) for k in range(p.num_kernels)])
    assert spec["feature"] in text, (cid, names)
    E.reference(dict(c, B=S.EXACT_BATCH), spec["variant"])          # the preconditions of the integer reference hold at this batch
    kinds = [s[0] for s in S.EXACT_STEPS]
    assert kinds == ["forward", "autotune", "forward", "tune_streams", "forward", "forward_u8", "forward"]
    assert [s[2] for s in S.EXACT_STEPS] == [1, 3, 3, 3, 2, 3, 3]
    assert {spec["feature"] for spec in S.EXACT_CHAINS.values()} == {",1launch", "conv_stem<f16,3-32-64-32>"}

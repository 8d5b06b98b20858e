"""No GPU: what tests/test_gpu_sequences.py rests on.  The table of tests/sequence_cases.py has the properties it is written for -- every
ordered pair of a plan's pure kinds adjacent somewhere, every pure kind compared in every state a twin is built in, batch sizes that rise
and fall, constant random walks -- and its plans are planned as it says: the switchable plan with two full arenas at the smallest
max_batch that gives them, the others with the stream count they name, the exact chains with the kernels they are in the table for.  The
number of twins a plan needs (one engine built per key) stays under the cap written in the table.  The changing calls a twin does NOT
replay (sequence_cases.twin_key drops them) are held against a model of this file's own of what every changing call reads and writes:
the reduced prefix of every index of every sequence reaches the state of the full one."""
import ctypes as C

import numpy as np
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
        on = False
        for c in seq:
            if c[0] == "set_wgrad_f16":         # only where the library accepts it, and as one of the two calls the table has
                assert sid in S.MODE and c in (S.SET_ON, S.SET_OFF) and (on or c == S.SET_ON), (sid, name, c)
                on = c[1]
            elif c[0] == "poison_extra":        # only while the engine has a buffer
                assert c == ("poison_extra",) and on, (sid, name, c)
            if c[0] == S.REFUSE:
                assert c[1] in pl["refusals"] and c[1] in S.REFUSALS, (sid, name, c)
            elif S.is_changing(c):
                family = S.INITS.get(c[0]) or S.STEPS.get(c[0])         # a training call: of a family the plan trains
                assert c[0] in S.CHANGING and (family is None or family in pl["train"]) and (pl["train"] or c[0] != "load_weights"), (sid, name, c)
                if c[0] in S.STEPS:
                    assert len(c) == 4 and 1 <= c[2] <= min(mb, S.N_IMAGES) and 0 <= c[1] and c[1] + c[2] <= S.N_IMAGES and c[3] in (1, 2, 3, 4), (sid, name, c)
            else:
                assert c[0] in pl["kinds"], (sid, name, c)
                lo, n = c[1], c[2]
                assert 1 <= n <= mb and (n > S.N_IMAGES or (0 <= lo and lo + n <= S.N_IMAGES)), (sid, name, c)
    assert set(pl["kinds"]) <= set(S.FORWARD) | set(S.DETECT) | set(S.LOSS) | set(S.LOSS_V3) | {S.REFUSE}
    if "loss" in pl["kinds"]:
        assert P.PLANS[pl["pid"]]["net"].startswith("v2") and not set(S.LOSS_V3) & set(pl["kinds"])
    if "loss_v3" in pl["kinds"]:
        assert P.PLANS[pl["pid"]]["net"].startswith("v3") and set(S.LOSS_V3) <= set(pl["kinds"])
    assert set(pl["train"]) <= set(S.FAMILIES) and all((f in ("v3", "blocks")) == P.PLANS[pl["pid"]]["net"].startswith("v3") for f in pl["train"])
    # Adam's step numbers of a family count up from 1 behind each of its inits (steps 3 and 4: the `mode` sequences alone)
    for name, seq in all_sequences(sid).items():
        t = {}
        for c in seq:
            if c[0] in S.INITS:
                t[S.INITS[c[0]]] = 0
            elif c[0] in S.STEPS:
                t[S.STEPS[c[0]]] += 1
                assert c[3] == t[S.STEPS[c[0]]] and (c[3] <= 2 or name == "mode"), (sid, name, c)
    assert max(t[4] for img in S.TRUTHS for t in img) < 20 and max(len(img) for img in S.TRUTHS) <= S.MAX_GT and [] in S.TRUTHS


def test_pure_and_changing_calls_are_the_issue_s():
    assert set(S.CHANGING) == {"train", "train_u8", "head_train_init", "load_weights", "rebind", "set_streams", "autotune", "tune_streams",
                               "head_train_v3_init", "train_v3", "train_v3_u8", "tail_train_init", "train_tail", "train_tail_u8",
                               "blocks_train_v3_init", "train_blocks_v3", "train_blocks_v3_u8", "set_wgrad_f16", "poison_extra"}
    assert S.FAMILIES == {"head": ("head_train_init", "train", "train_u8"), "v3": ("head_train_v3_init", "train_v3", "train_v3_u8"),
                          "tail": ("tail_train_init", "train_tail", "train_tail_u8"),
                          "blocks": ("blocks_train_v3_init", "train_blocks_v3", "train_blocks_v3_u8")}
    assert set(S.INITS) | set(S.STEPS) <= set(S.CHANGING) and len(S.INITS) == 4 and len(S.STEPS) == 8
    # the fourth family: it packs the v3 heads, as the `v3` family does, and the v3 blocks, which load_weights alone had written so far
    assert S.PACKED["blocks"] == ("packed v3 heads", "packed v3 blocks") and S.STATE["blocks"] == "blocks state" and "packed v3 blocks" in S.NET
    assert "packed v3 blocks" in S.effects(("load_weights",))[1] and S.effects(("blocks_train_v3_init",)) == (set(), {"blocks state", "packed v3 heads", "packed v3 blocks"})
    # the mode: written by set_wgrad_f16 alone, read by the tail and blocks steps alone; the buffer's bytes: written by poison_extra, read by nobody
    assert S.effects(S.SET_ON) == S.effects(S.SET_OFF) == (set(), {"wgrad mode"}) and S.effects(("poison_extra",)) == (set(), {"wgrad scratch"})
    for kind, family in S.STEPS.items():
        assert ("wgrad mode" in S.effects((kind, 0, 1, 1))[0]) == (family in ("tail", "blocks")), kind
    for c in [(k,) for k in S.INITS] + [("load_weights",), ("rebind",), ("set_streams", 1)] + [(k, 0, 1, 1) for k in S.STEPS]:
        assert not {"wgrad mode", "wgrad scratch"} & S.effects(c)[1], c
    assert not {"wgrad mode", "wgrad scratch"} & S.observes(("forward", 0, 1)) and "wgrad scratch" not in S.observes(("train_tail", 0, 1, 1))
    import blocks_v3_cases
    assert S.step_lr("train_blocks_v3") == S.step_lr("train_blocks_v3_u8") == blocks_v3_cases.TRAIN_LR == 1e-5
    for what in ("train_blocks-on-mxfp8", "set_wgrad_f16-on-fp32", "train_blocks-two-parts"):
        assert S.REFUSALS[what][0] == S.ERR_STATE
    for what in S.SET_REFUSALS:
        assert S.REFUSALS[what][0] == S.ERR_ARG and S.PLANS[S.MODE[0]]["refusals"][:2] == S.SET_REFUSALS
    assert S.LOSS_V3 == ("loss_v3", "loss_v3_u8", "loss_v3_grad") and 0.0 < S.IGNORE_THRESH <= 1.0
    # the four YOLOv3 plans have the three v3 loss kinds, the v2 plans the refusal of the v3 loss; the refusals of the v2 loss stay
    for sid in ("v3-fp16", "v3-mxfp8", "v3-spp-fp16", "v3-tiny-fp32"):
        assert set(S.LOSS_V3) <= set(S.PLANS[sid]["kinds"]) and {"loss-on-v3", "loss_grad-on-v3"} <= set(S.PLANS[sid]["refusals"])
    for sid in ("v2-fp16", "v2-fp32", "v2-tiny-fp16") + S.TRAIN_TAIL + S.HEAD_AND_TAIL:
        assert "loss_v3-on-v2" in S.PLANS[sid]["refusals"] and set(S.LOSS) <= set(S.PLANS[sid]["kinds"])
    assert S.REFUSALS["loss_v3-on-v2"] == (S.ERR_ARG, "the head must be version 3")
    assert S.REFUSALS["train_v3-two-parts"] == (S.ERR_STATE, "call yolo_net_set_streams(net, 1)")
    # the learning rates: the head families at the table's, the tail at the one its own GPU test uses (and for its reason)
    import test_gpu_sequences as G
    import test_gpu_train_tail as TT
    assert S.step_lr("train") == S.step_lr("train_v3_u8") == S.LR == 1e-3 and S.step_lr("train_tail") == S.step_lr("train_tail_u8") == TT.LR == 1e-4
    assert G.TAIL_PARTS == TT.TAIL_PARTS and len(G.TAIL_PARTS) == 16 and G.V3_STATE_KEYS == ("w", "b", "m_w", "v_w", "m_b", "v_b", "dw", "db")
    thresholds = {(m, t) for m, t, _ in S.DETECT.values()}
    assert {("detect", 0.5), ("detect", 0.05), ("detect", 0.9999), ("detect_u8", 0.5), ("detect_frames", 0.5)} <= thresholds
    for t in (0.5, 0.05, 0.9999):       # both NMS modes
        assert {mode for m, thr, mode in S.DETECT.values() if m == "detect" and thr == t} == {_hip.NMS_AGNOSTIC, _hip.NMS_PER_CLASS}
    assert S.is_sparse_detect(("detect@0.5", 0, 1)) and S.is_sparse_detect(("detect@0.05/per-class", 0, 1))
    assert not S.is_sparse_detect(("detect@0.9999", 0, 1)) and not S.is_sparse_detect(("forward", 0, 1))       # inside 1e-4 of 1: the dense branch
    assert 1.0 - 0.9999 <= 1e-4 + 1e-12
    assert set(S.V2_KINDS) - set(S.LOSS) == set(S.V3_KINDS) - set(S.LOSS_V3) and set(S.LOSS) <= set(S.V2_KINDS) and set(S.LOSS_V3) <= set(S.V3_KINDS)


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
    if "loss_v3" in S.PLANS[sid]["kinds"]:
        # loss_v3 -> a SPARSE detect -> loss_v3_grad, each at a batch size different from its predecessor's
        assert any(a[0] == "loss_v3" and b[0] == "detect@0.5" and S.is_sparse_detect(b) and c[0] == "loss_v3_grad" and a[2] != b[2] != c[2]
                   for a, b, c in zip(walk, walk[1:], walk[2:]))
        # rows the sparse detect did not write (more images than it had: batch slots it never touched), images it did not see
        assert any(x[0] == "detect@0.5" and y[0] == "loss_v3" and y[2] > x[2] and not (x[1] <= y[1] and y[1] + y[2] <= x[1] + x[2]) for x, y in zip(walk, walk[1:]))
        assert adjacent("forward_timed", "loss_v3_u8")
    else:
        assert not set(S.LOSS_V3) & {c[0] for c in walk}


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
    # seed 0, written out (drawn from the plan's calls, the three v3 loss kinds among them)
    assert S.SEQUENCES["v3-fp16"]["random"][:3] == [("detect_frames@0.5", 0, 1), ("detect@0.5", 3, 1), ("detect_u8@0.5", 0, 3)]
    for sid in ("v3-fp16", "v3-mxfp8", "v3-spp-fp16", "v3-tiny-fp32"):
        assert set(S.LOSS_V3) <= {c[0] for c in S.all_calls(sid)}


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
    for sid in ("v2-fp16", "v2-fp32") + S.TRAIN_V3 + S.TRAIN_TAIL + S.BLOCKS:
        init, step, step_u8 = S.FAMILIES[S.PLANS[sid]["train"][0]]
        s = S.SEQUENCES[sid]["train-u8-load-init"]
        i = s.index(("load_weights",))
        assert all(S.twin_key(s, j)[0] == () for j in range(i + 1, i + 1 + 2 * len(S.PLANS[sid]["kinds"])))
        j = len(s) - 1 - s[::-1].index((step, 0, 3, 1))
        assert j > i and S.twin_key(s, j) == S.twin_key(s, 1) == (((init,),), (step, 0, 3, 1))
        assert any(c[0] == step_u8 for c in s)
    # two training states on one net.  tail_train_init re-packs the head, so the tail step does not see the head-only step in front of it;
    # the second head-only step reads the state the first left and the block the tail step packed: everything is replayed for it ...
    s = S.SEQUENCES["v2-fp16-tail-and-head"]["head-and-tail"]
    start = (("head_train_init",), ("train", 0, 3, 1), ("tail_train_init",), ("train_tail", 0, 2, 1), ("train", 0, 4, 2))
    assert tuple(s[:5]) == start and all(S.twin_key(s, j)[0] == start[:j] for j in (0, 1, 2, 4, 5))
    assert S.twin_key(s, 3) == ((("tail_train_init",),), ("train_tail", 0, 2, 1))
    # ... and behind the second head_train_init, which overwrites all that is left of the two head-only steps, neither they nor the
    # first init are replayed: the step is the first step on the tail-trained block
    j = 5 + s[5:].index(("head_train_init",))
    assert S.twin_key(s, j + 1) == ((("tail_train_init",), ("train_tail", 0, 2, 1), ("head_train_init",)), ("train", 0, 3, 1))
    assert S.twin_key(s, len(s) - 1)[0] == (("tail_train_init",), ("train_tail", 0, 2, 1), ("head_train_init",), ("train", 0, 3, 1))
    # a tail step that DID run on a head-only step's head (no tail_train_init in between) keeps that step behind a later head_train_init
    s = [("tail_train_init",), ("head_train_init",), ("train", 0, 3, 1), ("train_tail", 0, 2, 1), ("head_train_init",), ("forward", 0, 1)]
    assert S.twin_key(s, 5)[0] == tuple(s[:5])
    # load_weights does not reset a training state: a step behind it without an init keeps the steps in front of it, and load_weights
    s = [("head_train_v3_init",), ("train_v3", 0, 3, 1), ("load_weights",), ("train_v3", 0, 4, 2), ("forward", 0, 1)]
    assert S.twin_key(s, 3)[0] == tuple(s[:3]) and S.twin_key(s, 4)[0] == tuple(s[:4])
    # rebind and set_streams are never dropped, whatever is dropped around them
    s = [("set_streams", 2), ("head_train_v3_init",), ("train_v3", 0, 3, 1), ("rebind",), ("set_streams", 1), ("load_weights",), ("forward", 0, 1)]
    assert S.twin_key(s, 6)[0] == (("set_streams", 2), ("rebind",), ("set_streams", 1))
    # two states on one YOLOv3 net, as head-and-tail: blocks_train_v3_init re-packs the head convs a head-convs step packed ...
    s = S.SEQUENCES["v3-fp16-blocks-and-heads"]["blocks-and-heads"]
    start = (("head_train_v3_init",), ("train_v3", 0, 3, 1), ("blocks_train_v3_init",), ("train_blocks_v3", 0, 2, 1), ("train_v3", 0, 4, 2))
    assert tuple(s[:5]) == start and all(S.twin_key(s, j)[0] == start[:j] for j in (0, 1, 2, 4, 5))
    assert S.twin_key(s, 3) == ((("blocks_train_v3_init",),), ("train_blocks_v3", 0, 2, 1))
    j = 5 + s[5:].index(("head_train_v3_init",))
    assert S.twin_key(s, j + 1) == ((("blocks_train_v3_init",), ("train_blocks_v3", 0, 2, 1), ("head_train_v3_init",)), ("train_v3", 0, 3, 1))
    # ... and a blocks step that DID run on a head-convs step's heads keeps that step
    s = [("blocks_train_v3_init",), ("head_train_v3_init",), ("train_v3", 0, 3, 1), ("train_blocks_v3", 0, 2, 1), ("head_train_v3_init",), ("forward", 0, 1)]
    assert S.twin_key(s, 5)[0] == tuple(s[:5])
    # the mode.  on -> off -> step: the twin never switched; on -> on: one set; a head-only step and a pure call under the mode: no set; an
    # init and load_weights leave it alone: the set in front of them is replayed for the step behind them; poison_extra is nobody's
    init, step, on, off = ("tail_train_init",), ("train_tail", 0, 3, 1), S.SET_ON, S.SET_OFF
    assert S.twin_key([on, off, init, step], 3) == S.twin_key([init, on, off, step], 3) == ((init,), step)
    assert S.twin_key([on, on, init, step], 3) == ((on, init), step) and S.twin_key([init, on, ("poison_extra",), step], 3) == ((init, on), step)
    assert S.twin_key([on, ("head_train_init",), ("train", 0, 3, 1)], 2) == ((("head_train_init",),), ("train", 0, 3, 1))
    assert S.twin_key([on, ("loss", 0, 1)], 1) == ((), ("loss", 0, 1))
    assert S.twin_key([on, init, step, ("load_weights",), init, step], 5) == ((on, init), step)
    assert S.twin_key([init, on, step, off, ("train_tail", 0, 4, 2)], 4)[0] == (init, on, step, off)       # the first step ran under it: both sets stay
    assert S.twin_key([init, off, step], 2) == ((init,), step)
    # ... in the table: the last three steps of `mode` are the uint8 step under the second set(on), step 1 under it behind load_weights and
    # an init, and step 1 of a twin that never switched
    for sid in S.MODE:
        init, step, step_u8 = S.FAMILIES[S.PLANS[sid]["train"][0]]
        s = S.SEQUENCES[sid]["mode"]
        steps = [i for i, c in enumerate(s) if c[0] in S.STEPS]
        assert [s[i] for i in steps] == [(step, 0, 3, 1), (step, 0, 4, 2), (step, 0, 2, 3), (step_u8, 1, 3, 4), (step, 0, 3, 1), (step, 0, 3, 1)]
        assert S.twin_key(s, steps[1])[0] == ((init,), on, (step, 0, 3, 1))                   # (neither the refused set nor the 0xFF is replayed)
        assert S.twin_key(s, steps[2])[0] == ((init,), on, (step, 0, 3, 1), (step, 0, 4, 2), off)
        assert S.twin_key(s, steps[3])[0] == S.twin_key(s, steps[2])[0] + ((step, 0, 2, 3), on)
        assert S.twin_key(s, steps[4]) == ((on, (init,)), (step, 0, 3, 1)) == S.twin_key(S.SEQUENCES[sid]["mode-before-init"], 4)
        assert S.twin_key(s, steps[5]) == (((init,),), (step, 0, 3, 1)) and s[steps[5] - 2:steps[5]] == [off, (init,)]
        i = s.index(("load_weights",))
        assert all(S.twin_key(s, j)[0] == () for j in range(i + 1, steps[4] - 1)) and steps[4] - 2 - i == len(S.PLANS[sid]["kinds"])
        assert S.twin_key(S.SEQUENCES[sid]["mode-before-init"], 1)[0] == ()                 # the loss under the mode: the untrained twin


# ---- the drop rules of twin_key, against a model of what the changing calls do -------------------------------------------------------------
# The model is this file's own (sequence_cases.effects is not used): each piece of state holds a VALUE, a term built from the call that wrote
# it and the values that call read.  Two prefixes that end in equal terms have put the net into the same state as far as the model goes.
PIECES = ("packed head", "packed block", "packed v3 heads", "packed v3 blocks", "head state", "tail state", "v3 state", "blocks state", "workspace", "streams",
          "tiles", "wgrad mode", "wgrad scratch")
MODEL_STATE = {"head": "head state", "tail": "tail state", "v3": "v3 state", "blocks": "blocks state"}
MODEL_PACKS = {"head": ("packed head",), "tail": ("packed head", "packed block"), "v3": ("packed v3 heads",), "blocks": ("packed v3 heads", "packed v3 blocks")}
MODEL_PACKED = ("packed head", "packed block", "packed v3 heads", "packed v3 blocks")
MODEL_MODE_STEPS = ("train_tail", "train_tail_u8", "train_blocks_v3", "train_blocks_v3_u8")     # the steps whose 3 x 3 weight gradient the mode replaces


def model_net(st):
    """what a pass through the net can see: every packed region, the workspace binding, the stream count, the tiles"""
    return tuple(st[k] for k in MODEL_PACKED + ("workspace", "streams", "tiles"))


def model_run(calls):
    st = dict.fromkeys(PIECES, "as built")
    st.update(dict.fromkeys(MODEL_PACKED, "as loaded"))
    st.update(dict.fromkeys(MODEL_STATE.values(), None))
    st.update({"wgrad mode": "off", "wgrad scratch": None})
    for c in calls:
        kind = c[0]
        if kind == "load_weights":                  # the original stream: every packed region as it was loaded; no training state is touched, nor the mode
            st.update(dict.fromkeys(MODEL_PACKED, "as loaded"))
        elif kind in S.INITS:                       # masters from the original stream, zeroed moments; the family's layers packed from the masters
            st[MODEL_STATE[S.INITS[kind]]] = "started"
            st.update(dict.fromkeys(MODEL_PACKS[S.INITS[kind]], "as loaded"))
        elif kind in S.STEPS:                       # forward through the net as it is, the state moved, the family's layers packed from the new masters
            family = S.STEPS[kind]
            assert st[MODEL_STATE[family]] is not None, "a step without its init: %r" % (c,)
            # a tail or a blocks step computes its block's weight gradient by the kernel the mode names; in the mode it writes every byte of
            # the buffer that it reads, so the buffer's bytes are no part of the term -- and they are the step's own scratch afterwards
            mode = (st["wgrad mode"],) if kind in MODEL_MODE_STEPS else ()
            assert not mode or mode[0] == "off" or st["wgrad scratch"] is not None, "a step in the mode without a buffer: %r" % (c,)
            st[MODEL_STATE[family]] = ("step", c, st[MODEL_STATE[family]], model_net(st)) + mode
            st.update({k: ("packed from", k, st[MODEL_STATE[family]]) for k in MODEL_PACKS[family]})
            if mode and mode[0] == "on":
                st["wgrad scratch"] = ("scratch of", c)
        elif kind == "set_wgrad_f16":               # on: a new buffer, whatever it holds; off: no buffer.  Nothing else
            st["wgrad mode"], st["wgrad scratch"] = ("on", "uninitialised") if c[1] else ("off", None)
        elif kind == "poison_extra":
            assert st["wgrad mode"] == "on", "no buffer to poison: %r" % (c,)
            st["wgrad scratch"] = "0xFF"
        elif kind == "rebind":
            st["workspace"] = ("re-bound", st["workspace"])
        elif kind in ("set_streams", "tune_streams"):
            st["streams"] = (c, st["streams"])
        elif kind == "autotune":
            st["tiles"] = (c, st["tiles"])
        else:
            raise ValueError(c)
    return st


def model_result(calls, call):
    """what the call returns, and the state it leaves, behind `calls`: a pure call sees the net; a step its family's state as well and
    leaves a new one; an init, a load or a switch returns nothing"""
    st = model_run(calls)
    if S.is_pure(call):
        return ("result", call, model_net(st))
    after = model_run(list(calls) + [call])
    return ("result", call, model_net(after)) + ((after[MODEL_STATE[S.STEPS[call[0]]]],) if call[0] in S.STEPS else ())


@pytest.mark.parametrize("sid", S.ALL_PLANS)
def test_the_reduced_prefix_reaches_the_state_of_the_full_prefix(sid):
    """for every index of every sequence: the calls twin_key keeps are a subsequence of the changing calls in front of the index, and in
    the model they give the call the same result, and leave the same net, as all of them do.  And the table never steps a family without
    an init of that family between the step and the last load_weights in front of it (load_weights does not reset a training state)."""
    dropped = 0
    for name, seq in all_sequences(sid).items():
        for i, call in enumerate(seq):
            full = [c for c in seq[:i] if S.is_changing(c)]
            kept = list(S.twin_key(seq, i)[0])
            it = iter(full)
            assert all(any(c == f for f in it) for c in kept), (sid, name, i, kept)            # a subsequence, in order
            assert model_result(kept, call) == model_result(full, call), (sid, name, i, call, kept)
            dropped += len(full) - len(kept)
            if call[0] in S.STEPS:
                family = S.STEPS[call[0]]
                behind_load = full[max((j for j, c in enumerate(full) if c[0] == "load_weights"), default=-1) + 1:]
                assert any(c[0] in S.INITS and S.INITS[c[0]] == family for c in behind_load), (sid, name, i, call)
    if any("train-u8-load-init" in n or "head-and-tail" in n or "blocks-and-heads" in n or n.startswith("mode") for n in all_sequences(sid)):
        assert dropped > 0, sid


def test_the_model_tells_a_wrong_drop_from_a_right_one():
    """the proof above is worth what the model can refute"""
    init, step = ("tail_train_init",), ("train_tail", 0, 3, 1)
    head = [("head_train_init",), ("train", 0, 3, 1)]
    fwd = ("forward", 0, 1)
    assert model_result(head + [init, step], fwd) == model_result([init, step], fwd)                 # tail_train_init re-packs the head
    assert model_result([init] + head + [step], fwd) != model_result([init, step], fwd)             # ... a head-only step behind it is seen
    assert model_result([init, step, ("load_weights",)], fwd) == model_result([], fwd)
    assert model_result([init, step, ("load_weights",)], step) != model_result([init], step)        # the state outlives load_weights
    assert model_result([init, step, ("load_weights",), init], step) == model_result([init], step)
    assert model_result([("rebind",)], fwd) != model_result([], fwd) and model_result([("set_streams", 2), ("set_streams", 1)], fwd) != model_result([("set_streams", 1)], fwd)
    assert model_result([("head_train_v3_init",), ("train_v3", 0, 3, 1)], ("train_v3", 0, 4, 2)) != model_result([("head_train_v3_init",)], ("train_v3", 0, 4, 2))
    # a set_wgrad_f16 that a retained tail or blocks step read: dropping it is seen in that step, in the step behind it and in a forward behind both
    on, off, step2 = S.SET_ON, S.SET_OFF, ("train_tail", 0, 4, 2)
    assert model_result([init, on], step) != model_result([init], step)
    assert model_result([init, on, step], step2) != model_result([init, step], step2) and model_result([init, on, step, off], step2) != model_result([init, step], step2)
    assert model_result([init, on, step, off], fwd) != model_result([init, step], fwd)
    assert model_result([on, off, init], step) == model_result([init], step) and model_result([on, on, init], step) == model_result([on, init], step)
    assert model_result([on, init, step, ("load_weights",), init], step) == model_result([on, init], step) != model_result([init], step)      # nothing but a set writes the mode
    assert model_result([init, on, ("poison_extra",)], step) == model_result([init, on], step)
    assert model_result([on] + head, ("train", 0, 4, 2)) == model_result(head, ("train", 0, 4, 2)) and model_result([on], fwd) == model_result([], fwd)
    b_init, b_step, b_fwd = ("blocks_train_v3_init",), ("train_blocks_v3", 0, 2, 1), ("forward", 0, 1)
    assert model_result([b_init, on], b_step) != model_result([b_init], b_step)
    # a v3 step that a retained blocks step ran on (no blocks_train_v3_init in between re-packed the heads): dropping it is seen
    v3 = [("head_train_v3_init",), ("train_v3", 0, 3, 1)]
    assert model_result([b_init] + v3, b_step) != model_result([b_init], b_step)
    assert model_result([b_init] + v3 + [b_step, v3[0]], b_fwd) != model_result([b_init, b_step, v3[0]], b_fwd)
    assert model_result(v3 + [b_init], b_step) == model_result([b_init], b_step)                     # blocks_train_v3_init re-packs the heads
    assert model_result(v3 + [b_init, b_step], v3[1]) != model_result([v3[0]], v3[1])               # ... and a blocks step is seen by the next v3 step
    assert model_result([b_init, b_step, ("load_weights",)], b_fwd) == model_result([], b_fwd)


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
        keys = {S.twin_key(seq, i) for i in range(start, end) if S.is_pure(seq[i]) or seq[i][0] in S.STEPS}
        first = sid not in met          # the plan's first item builds the second twins of the newer controls as well
        new = keys - met.setdefault(sid, set())
        assert len(new) + (S.control_engines(sid) if first else 0) <= S.TWINS_PER_ITEM, (sid, name, part, len(new))
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
    # the covering walks as before, and the train-2 sequence of one plan of each training family
    assert set(S.ASYNC_PLANS) == {"v2-fp16", "v3-fp16", "v3-tiny-fp32-train", "v2-tiny-fp16-tail", "v3-tiny-fp16-blocks", "v3-tiny-fp16-blocks-f16"}
    assert {s for s in S.ASYNC_PLANS if "cover" in S.SEQUENCES[s]} == {"v2-fp16", "v3-fp16"}
    assert sorted(S.PLANS[s]["train"][0] for s in S.ASYNC_PLANS if "train-2" in S.SEQUENCES[s]) == ["blocks", "blocks", "head", "tail", "v3"]
    # ... of a MODE plan train-2 with a set(on) in front of the first step, and no set(off), which waits for the device
    assert S.MODE_ASYNC in S.MODE and [s for s in S.MODE if "train-2" in S.SEQUENCES[s]] == [S.MODE_ASYNC]
    s, form = S.SEQUENCES[S.MODE_ASYNC]["train-2"], S.training_sequences(S.MODE_ASYNC, "blocks")["train-2"]
    assert s == form[:1] + [S.SET_ON] + form[1:] and S.SET_OFF not in s
    # the training sequences of every training plan, and what they are made of
    for sid in S.TRAIN_V3 + S.TRAIN_TAIL + S.BLOCKS:
        init, step, step_u8 = S.FAMILIES[S.PLANS[sid]["train"][0]]
        seqs, pure0, pure1 = S.SEQUENCES[sid], S.each_pure(sid, 0), S.each_pure(sid, 1)
        assert set(seqs) == {"train-1", "train-2", "train-u8-load-init", "rebind-train"}
        assert [c[0] for c in pure0] == list(S.PLANS[sid]["kinds"]) == [c[0] for c in pure1]
        assert seqs["train-1"] == [(init,), (step, 0, 3, 1)] + pure0
        assert seqs["train-2"] == [(init,), (step, 0, 3, 1), ("forward", 0, 2), (step, 0, 4, 2)] + pure1
        assert seqs["train-u8-load-init"] == ([(init,), (step, 0, 3, 1), ("detect@0.5", 0, 2), (step_u8, 1, 2, 2)] + pure0 + [("load_weights",)] + pure0 + pure1
                                              + [(init,), (step, 0, 3, 1)] + pure0)
        assert S.is_sparse_detect(("detect@0.5", 0, 2))
        s = seqs["rebind-train"]
        assert s[:3] == [(init,), (step, 0, 3, 1), ("rebind",)] and s[3][0] == step and s[3][3] == 2 and s[4:] == pure1
    for sid in S.HEAD_AND_TAIL:
        assert S.SEQUENCES[sid] == {"head-and-tail": [("head_train_init",), ("train", 0, 3, 1), ("tail_train_init",), ("train_tail", 0, 2, 1), ("train", 0, 4, 2)]
                                    + S.each_pure(sid, 0) + [("head_train_init",), ("train", 0, 3, 1)] + S.each_pure(sid, 1)}
    # the second interleaved pair: both engines train, calls alternate, each engine's calls are the start of its train-2 sequence
    assert S.PAIR_TRAIN == ("v2-tiny-fp16-tail", "v3-tiny-fp32-train") and all(a[0] != b[0] for a, b in zip(S.INTERLEAVED_TRAIN, S.INTERLEAVED_TRAIN[1:]))
    for sid in S.PAIR_TRAIN:
        own = [c for s, c in S.INTERLEAVED_TRAIN if s == sid]
        assert own == S.SEQUENCES[sid]["train-2"][:len(own)] and sum(c[0] in S.STEPS for c in own) == 2 and sum(S.is_pure(c) for c in own) >= 8
    # the two states on one YOLOv3 net: the form of head-and-tail
    for sid in S.BLOCKS_AND_HEADS:
        assert S.SEQUENCES[sid] == {"blocks-and-heads": [("head_train_v3_init",), ("train_v3", 0, 3, 1), ("blocks_train_v3_init",), ("train_blocks_v3", 0, 2, 1),
                                                         ("train_v3", 0, 4, 2)] + S.each_pure(sid, 0) + [("head_train_v3_init",), ("train_v3", 0, 3, 1)] + S.each_pure(sid, 1)}
    # the mode sequences, call by call
    on, off, refused = S.SET_ON, S.SET_OFF, (S.REFUSE, "set_wgrad_f16-too-small")
    for sid in S.MODE:
        init, step, step_u8 = S.FAMILIES[S.PLANS[sid]["train"][0]]
        seqs, pure0, pure1 = S.SEQUENCES[sid], S.each_pure(sid, 0), S.each_pure(sid, 1)
        tail = sid.endswith("-tail-f16")
        assert set(seqs) == {"mode", "mode-before-init"} | ({"mode-and-head"} if tail else set()) | ({"train-2"} if sid == S.MODE_ASYNC else set())
        assert seqs["mode"] == ([(init,), on, (step, 0, 3, 1)] + pure0 + [("poison_extra",), (step, 0, 4, 2)] + [off, (step, 0, 2, 3)] + pure1
                                + [on, refused, (step_u8, 1, 3, 4)] + [("load_weights",)] + pure0 + [(init,), (step, 0, 3, 1)] + [off, (init,), (step, 0, 3, 1)])
        # the refused set under the mode stands among the pure kinds in front of the 0xFF and step 2, the unaligned one among those behind set(off)
        assert refused in pure0 and (S.REFUSE, "set_wgrad_f16-unaligned") in pure1
        loss = ("loss" if tail else "loss_v3",) + S.variants(S.PLANS[sid]["kinds"], "loss" if tail else "loss_v3")[0]
        assert seqs["mode-before-init"] == [on, loss, on, (init,), (step, 0, 3, 1), ("rebind",), (step, 1, 3, 2)] + pure1
        if tail:
            assert seqs["mode-and-head"] == [(init,), on, (step, 0, 3, 1), ("head_train_init",), ("train", 0, 2, 1), (step, 0, 4, 2)] + pure0
    # the third interleaved pair: a blocks engine and a tail engine in the fp16 mode, each engine's calls the start of its `mode` sequence
    # up to the step behind the 0xFF in its own buffer
    assert S.PAIR_MODE == ("v3-tiny-fp16-blocks-f16", "v2-tiny-fp16-tail-f16") and all(a[0] != b[0] for a, b in zip(S.INTERLEAVED_MODE, S.INTERLEAVED_MODE[1:]))
    assert [S.PLANS[s]["train"][0] for s in S.PAIR_MODE] == ["blocks", "tail"] and set(S.PAIR_MODE) <= set(S.MODE)
    for sid in S.PAIR_MODE:
        own = [c for s, c in S.INTERLEAVED_MODE if s == sid]
        assert own == S.SEQUENCES[sid]["mode"][:len(own)] and own[1] == on and own[-2] == ("poison_extra",) and own[-1][0] in S.STEPS and own[-1][3] == 2
    # the new refusals where the issue puts them: in the refusal sequence of the MXFP8 plan, between two compared calls; in switch-train at two parts
    s = S.SEQUENCES["v3-mxfp8"]["refusals"]
    i = s.index((S.REFUSE, "train_blocks-on-mxfp8"))
    assert S.batch_of(s[i - 1]) is not None and S.batch_of(s[i + 1]) is not None
    assert "set_wgrad_f16-on-fp32" in {c[1] for c in S.SEQUENCES["v3-tiny-fp32-blocks"]["train-1"] if c[0] == S.REFUSE}


# ---- the plans -----------------------------------------------------------------------------------------------------------------------------
def test_the_plans_are_the_issue_s():
    rows = {sid: (P.PLANS[pl["pid"]]["net"], P.PLANS[pl["pid"]]["dtype"]) for sid, pl in S.PLANS.items()}
    assert {rows[s] for s in S.MAIN} == {("v2", "fp16"), ("v2", "fp32"), ("v2-tiny", "fp16"), ("v3", "fp16"), ("v3", "mxfp8"), ("v3-spp", "fp16"), ("v3-tiny", "fp32")}
    assert {s: S.PLANS[s]["train"] for s in S.PLANS if S.PLANS[s]["train"]} == dict(
        [("v2-fp16", ("head",)), ("v2-fp32", ("head",)), ("v3-fp16-switch", ("v3",))] + [(s, ("v3",)) for s in S.TRAIN_V3] + [(s, ("tail",)) for s in S.TRAIN_TAIL]
        + [(s, ("tail", "head")) for s in S.HEAD_AND_TAIL] + [(s, ("blocks",)) for s in S.BLOCKS] + [(s, ("blocks", "v3")) for s in S.BLOCKS_AND_HEADS]
        + [(s, ("tail", "head") if s.startswith("v2") else ("blocks",)) for s in S.MODE])
    assert S.BLOCKS == ("v3-fp16-blocks", "v3-tiny-fp16-blocks", "v3-tiny-fp32-blocks")
    assert S.BLOCKS_AND_HEADS == ("v3-tiny-fp16-blocks-and-heads", "v3-fp16-blocks-and-heads")
    assert S.MODE == ("v2-fp16-tail-f16", "v2-tiny-fp16-tail-f16", "v3-tiny-fp16-blocks-f16", "v3-fp16-blocks-f16")
    assert [S.PLANS[s]["pid"] for s in S.BLOCKS + S.BLOCKS_AND_HEADS + S.MODE] == [
        "v3-fp16-plan", "v3-tiny-fp16-plan", "v3-tiny-fp32-plan", "v3-tiny-fp16-plan", "v3-fp16-plan", "v2-fp16-plan", "v2-tiny-fp16-plan", "v3-tiny-fp16-plan",
        "v3-fp16-plan"]
    assert S.TRAINING_PLANS == S.TRAIN_V3 + S.TRAIN_TAIL + S.HEAD_AND_TAIL + S.BLOCKS + S.BLOCKS_AND_HEADS + S.MODE and len(set(S.ALL_PLANS)) == len(S.ALL_PLANS)
    for sid in S.BLOCKS + S.BLOCKS_AND_HEADS + S.MODE:
        v3 = P.PLANS[S.PLANS[sid]["pid"]]["net"].startswith("v3")
        assert S.PLANS[sid]["kinds"] == (S.V3_KINDS if v3 else S.V2_KINDS) and set(S.V3_REFUSALS if v3 else S.V2_REFUSALS) <= set(S.PLANS[sid]["refusals"])
        assert S.PLANS[sid]["more"] == {"streams": 1, "max_batch": 4} and not P.PLANS[S.PLANS[sid]["pid"]]["keep_all"]
    assert S.PLANS["v3-mxfp8"]["refusals"] == S.V3_REFUSALS + ("train_blocks-on-mxfp8",) and "train_blocks-two-parts" in S.PLANS["v3-fp16-switch"]["refusals"]
    assert S.TRAIN_V3 == ("v3-fp16-train", "v3-tiny-fp32-train", "v3-mxfp8-train") and S.TRAIN_TAIL == ("v2-fp16-tail", "v2-fp32-tail", "v2-tiny-fp16-tail")
    assert [S.PLANS[s]["pid"] for s in S.TRAIN_V3 + S.TRAIN_TAIL] == ["v3-fp16-plan", "v3-tiny-fp32-plan", "v3-mxfp8-plan", "v2-fp16-plan", "v2-fp32-plan",
                                                                     "v2-tiny-fp16-plan"]
    assert [S.PLANS[s]["pid"] for s in S.HEAD_AND_TAIL] == [S.PLANS[s]["pid"] for s in S.TRAIN_TAIL]
    for sid in S.TRAIN_V3:          # their pure kinds are the plan's ordinary ones
        assert S.PLANS[sid]["kinds"] == S.V3_KINDS == S.PLANS["v3-fp16"]["kinds"]
    for sid in S.TRAIN_TAIL + S.HEAD_AND_TAIL:
        assert S.PLANS[sid]["kinds"] == S.V2_KINDS == S.PLANS["v2-fp16"]["kinds"]
    for sid in S.MAIN + S.TRAIN_V3 + S.TRAIN_TAIL + S.HEAD_AND_TAIL:
        assert S.PLANS[sid]["more"] == {"streams": 1, "max_batch": 4} and not P.PLANS[S.PLANS[sid]["pid"]]["keep_all"]


@pytest.mark.parametrize("sid", S.TRAINING_PLANS)
def test_the_library_accepts_the_training_plans(sid):
    """the entry points that refuse a plan they cannot train (a fused-away input, an MXFP8 conv, a reused buffer) accept these, and the
    activations a step reads out of the workspace lie inside it"""
    p = S.plan_only(sid)
    assert p.num_streams == 1 and p.max_batch == S.MAX_BATCH
    views = []
    if "v3" in S.PLANS[sid]["train"]:
        lay, views = p.head_train_layout_v3(), p.head_inputs_v3()
        assert lay.n_scales == len(views) == p.head.n_scales >= 2 and lay.total_bytes > 0        # (the mutation test flips a bit of scale 1)
    if "tail" in S.PLANS[sid]["train"]:
        cls, anchors, names, _ = P.NETS[P.PLANS[S.PLANS[sid]["pid"]]["net"]]
        h, w, _ = p.output_shape            # (a model sets the YOLOv2 head when it builds its engine)
        p.set_head(engine.head_desc_v2(h, w, np.reshape(anchors, [-1, 2]), len(names)))
        lay, views = p.tail_train_layout(), list(p.tail_inputs())
        assert lay.total_bytes > 0 and (views[1].cin, views[0].cin) == (lay.cin, lay.cin3)
    if "head" in S.PLANS[sid]["train"]:
        assert p.head_train_layout().total_bytes > 0 and p.head_input().offset == views[1].offset
    if "blocks" in S.PLANS[sid]["train"]:
        lay, (block_in, head_in) = p.blocks_train_layout_v3(), p.block_inputs_v3()
        assert lay.n_scales == len(block_in) == len(head_in) == p.head.n_scales >= 2 and lay.total_bytes > 0     # (the mutation test flips a bit of scale 1)
        assert [v.cin for v in block_in] == list(lay.cin3[:lay.n_scales]) and [v.cin for v in head_in] == list(lay.cout3[:lay.n_scales]) == list(lay.cin[:lay.n_scales])
        if "v3" in S.PLANS[sid]["train"]:       # the same head convs, read from the same place
            assert [v.offset for v in head_in] == [v.offset for v in views]
        views = views + block_in + head_in
    for v in views:
        assert 0 <= v.offset and v.offset + S.MAX_BATCH * v.image_stride * (2 if v.dtype == _hip.DTYPE_F16 else 4) <= p.workspace_bytes, (sid, v.offset)
    # the mode: a buffer size on every MODE plan, the float32 refusal on a float32 plan with a trainable block
    need = int(p.lib.yolo_net_train_wgrad_f16_bytes(p.handle))
    if sid in S.MODE:
        assert need > 0 and need % 256 == 0, (sid, need)
        # the refused sets, on the host (no device: the pointers are never followed) -- and an accepted one, cleared again
        for what, args in (("set_wgrad_f16-too-small", (4096, need - 1)), ("set_wgrad_f16-unaligned", (4096 + 128, need))):
            assert p.lib.yolo_net_train_set_wgrad_f16(p.handle, *args) == S.REFUSALS[what][0] and S.REFUSALS[what][1] in p.lib.yolo_last_error().decode(), what
        assert p.lib.yolo_net_train_set_wgrad_f16(p.handle, 4096, need) == 0 and p.lib.yolo_net_train_set_wgrad_f16(p.handle, None, 0) == 0
    elif P.PLANS[S.PLANS[sid]["pid"]]["dtype"] == "fp32" and set(S.PLANS[sid]["train"]) & {"tail", "blocks"}:
        what = "set_wgrad_f16-on-fp32"
        assert need == 0 and S.REFUSALS[what][1] in p.lib.yolo_last_error().decode(), sid
        assert p.lib.yolo_net_train_set_wgrad_f16(p.handle, 4096, 1 << 30) == S.REFUSALS[what][0] and S.REFUSALS[what][1] in p.lib.yolo_last_error().decode()
        assert (what in S.PLANS[sid]["refusals"]) == (sid in S.BLOCKS)


def test_what_must_leave_the_mode_alone_is_compared_across_twin_keys():
    """A twin that replays the suspect call behind the same set(on) cannot see that call clear the mode: in the model, an init that did
    would give engine and twin the same term.  MODE_SURVIVES therefore pairs keys that differ in WHERE the set stands, or in whether it
    is there at all, and the model -- in which nothing but a set writes the mode -- says which pairs are equal and which differ."""
    on = S.SET_ON
    for sid in S.MODE:
        init, step, _ = S.FAMILIES[S.PLANS[sid]["train"][0]]
        table, first = S.MODE_SURVIVES[sid], (step, 0, 3, 1)
        assert set(table) == {"equal", "differ"}
        assert table["equal"][0] == ((((init,), on), first), ((on, (init,)), first))
        # both keys of the init pair are the sequences' own: the first step of `mode` and the step behind load_weights and an init in it
        seq = S.SEQUENCES[sid]["mode"]
        assert {S.twin_key(seq, i) for i, c in enumerate(seq) if c == first} >= set(table["equal"][0])
        assert (len(table["equal"]) == 2) == ("head" in S.PLANS[sid]["train"])
        if "head" in S.PLANS[sid]["train"]:
            assert table["equal"][1] == ((((init,), on), first), (((init,), on, ("head_train_init",)), first))
        assert table["differ"] == [((((init,), on, ("rebind",)), first), (((init,), ("rebind",)), first))]
        for a, b in table["equal"]:         # in the model: the same step term but for the ORDER of what the prefix wrote, the same mode
            ra, rb = model_run(list(a[0])), model_run(list(b[0]))
            assert ra["wgrad mode"] == rb["wgrad mode"] == "on" and all(ra[k] == rb[k] for k in MODEL_PACKED) and a[1] == b[1]
            assert model_result(list(a[0]), a[1]) == model_result(list(b[0]), b[1])
        for a, b in table["differ"]:
            assert model_result(list(a[0]), a[1]) != model_result(list(b[0]), b[1]) and [c for c in a[0] if c != on] == list(b[0])
        assert {k for pairs in table.values() for pair in pairs for k in pair} <= S.twin_keys(sid)      # counted against the cap
    # why a sequence alone cannot hold the claim: the keys of row 6 of `mode` and of mode-before-init carry the init behind the set
    s = S.SEQUENCES[S.MODE[0]]["mode-before-init"]
    assert S.twin_key(s, 4)[0] == (on, ("tail_train_init",)) and s[4][0] in S.STEPS


def test_the_library_refuses_the_blocks_of_the_mxfp8_plan():
    """why no blocks plan stands over the MXFP8 row: the conv behind each head conv is an MXFP8 conv there, and the entry points say so"""
    what = "train_blocks-on-mxfp8"
    for sid in ("v3-mxfp8", "v3-mxfp8-train"):
        p = S.plan_only(sid)
        blocks, heads, n = (_hip.TensorView * _hip.MAX_SCALES)(), (_hip.TensorView * _hip.MAX_SCALES)(), C.c_int32(0)
        assert p.lib.yolo_net_block_inputs_v3(p.handle, blocks, heads, C.byref(n)) == S.REFUSALS[what][0] and S.REFUSALS[what][1] in p.lib.yolo_last_error().decode()
        assert p.lib.yolo_net_blocks_train_v3_layout(p.handle, C.byref(_hip.BlocksTrainV3Layout())) == S.REFUSALS[what][0]
        assert S.REFUSALS[what][1] in p.lib.yolo_last_error().decode()
        assert p.head_train_layout_v3().n_scales == 3           # (its head convs are fp16 convs and train: v3-mxfp8-train)
    assert (S.REFUSE, what) in S.SEQUENCES["v3-mxfp8"]["refusals"] and not any("mxfp8" in s for s in S.BLOCKS + S.BLOCKS_AND_HEADS + S.MODE)


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
    # the YOLOv3 train step on this plan: refused at two parts, accepted after set_streams(1), seen by both arenas, refused again, a second step
    seq = S.sequences_of("v3-fp16-switch")["switch-train"]
    refused = (S.REFUSE, "train_v3-two-parts")
    assert seq[:7] == [("set_streams", 2), ("forward", 0, mb), refused, ("set_streams", 1), ("head_train_v3_init",), ("train_v3", 0, 4, 1), ("set_streams", 2)]
    assert seq[7:9] == [("detect@0.5", 0, mb), ("forward", 0, mb)] and S.is_sparse_detect(seq[7])
    assert [c for c in seq if S.is_changing(c)] == [("set_streams", 2), ("set_streams", 1), ("head_train_v3_init",), ("train_v3", 0, 4, 1), ("set_streams", 2),
                                                    ("set_streams", 1), ("train_v3", 0, 3, 2)]
    j = len(seq) - 1 - seq[::-1].index(("set_streams", 1))
    assert seq[j - 1] == refused and seq[j + 1] == ("train_v3", 0, 3, 2) and seq[j + 2] == ("forward", 0, mb)
    refused_blocks = (S.REFUSE, "train_blocks-two-parts")       # the blocks step in front of it: refused as the head step is, by the same check
    assert seq[j - 2] == refused_blocks and seq.count(refused_blocks) == 1 and S.batch_of(seq[j - 3]) is not None
    assert S.REFUSALS["train_blocks-two-parts"] == S.REFUSALS["train_v3-two-parts"]
    streams = 0
    for c in seq:           # the refusal only ever at two parts, the steps only at one
        streams = c[1] if c[0] == "set_streams" else streams
        assert (c not in (refused, refused_blocks) or streams == 2) and (c[0] not in S.STEPS or streams == 1), c
    assert S.twin_key(seq, len(seq) - 1)[0] == tuple(c for c in seq if S.is_changing(c))
    lay = p.head_train_layout_v3()          # at one part (the loop above left it there) the layout is accepted ...
    assert lay.n_scales == 3
    assert p.lib.yolo_net_set_streams(p.handle, 2) == 0 and p.lib.yolo_net_head_train_v3_layout(p.handle, C.byref(lay)) == S.REFUSALS["train_v3-two-parts"][0]
    assert S.REFUSALS["train_v3-two-parts"][1] in p.lib.yolo_last_error().decode()      # ... at two parts it is refused with the documented message
    blk = _hip.BlocksTrainV3Layout()        # ... and so is the blocks layout, the first thing a blocks step asks for
    assert p.lib.yolo_net_blocks_train_v3_layout(p.handle, C.byref(blk)) == S.REFUSALS["train_blocks-two-parts"][0]
    assert S.REFUSALS["train_blocks-two-parts"][1] in p.lib.yolo_last_error().decode()
    assert p.lib.yolo_net_set_streams(p.handle, 1) == 0 and p.lib.yolo_net_blocks_train_v3_layout(p.handle, C.byref(blk)) == 0 and blk.n_scales == 3


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

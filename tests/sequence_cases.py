"""The call sequences of tests/test_gpu_sequences.py, as a table that needs no GPU (tests/test_sequences_cpu.py keeps it honest).

The rule under test: the result of call i of a sequence equals, bit for bit, the result of the same call on a TWIN -- an engine built the
same way that has executed only the CHANGING calls in front of i, in order, and then this call.  PURE calls (forward, forward_u8,
forward_timed, detect / detect_u8 at 0.5, 0.05 and 0.9999 in both NMS modes, detect_frames, loss, loss_u8, loss_grad, loss_v3, loss_v3_u8,
loss_v3_grad, a refused call) must leave nothing behind that a later call can observe; changing calls (a train step of any of the four
families -- the YOLOv2 head, the YOLOv3 head convs, the YOLOv2 tail, the YOLOv3 head convs with the 3 x 3 blocks behind them --, their
inits, load_weights, a re-bind onto a poisoned buffer, set_streams, autotune, tune_streams, set_wgrad_f16 -- the mode bit of the tail and
blocks steps --, poison_extra -- 0xFF into the buffer that mode runs in) are what a twin replays.  twin_key(sequence, i) is the key a twin's result is cached under.

A call is a tuple: (kind, lo, n) runs on images lo .. lo + n - 1 of the plan's four distinct images, ("refuse", what) is a call the library
must refuse (REFUSALS), a changing call is (kind, ...) of CHANGING; a train step is (kind, lo, n, t), Adam's step t = 1, 2, ...  Every list
below is a constant: the walks are generated at import by a fixed algorithm and a fixed seed, nothing is drawn while the tests run.

A twin need not replay a changing call whose every effect is gone: twin_key drops it (the rules are in its docstring, EFFECTS is what they
are computed from, tests/test_sequences_cpu.py proves them on a model of its own).  Every drop is a claim, asserted by every comparison
behind it: yolo_net_load_weights of the ORIGINAL stream takes the net back to the bytes of a net that never trained; an init of a family
starts that family's training state again and packs its layers as load_weights does (a step behind it equals the first step), whatever a
step of ANOTHER family on the same net had packed there."""
import functools
import random

import blocks_v3_cases
import poison_cases as P
from tensorflow_yolo_amd import _hip

MAX_BATCH = 4
N_IMAGES = 4
IOU = 0.6
TWIN_KEY_CAP = 112           # distinct twin keys per plan, over all its sequences: each is one engine built and one call (GPU time)

# ---- call kinds --------------------------------------------------------------------------------------------------------------------------
# kind -> (engine method, threshold, NMS mode)
DETECT = {"detect@0.5": ("detect", 0.5, _hip.NMS_AGNOSTIC), "detect@0.5/per-class": ("detect", 0.5, _hip.NMS_PER_CLASS),
          "detect@0.05": ("detect", 0.05, _hip.NMS_AGNOSTIC), "detect@0.05/per-class": ("detect", 0.05, _hip.NMS_PER_CLASS),
          "detect@0.9999": ("detect", 0.9999, _hip.NMS_AGNOSTIC), "detect@0.9999/per-class": ("detect", 0.9999, _hip.NMS_PER_CLASS),
          "detect_u8@0.5": ("detect_u8", 0.5, _hip.NMS_AGNOSTIC), "detect_frames@0.5": ("detect_frames", 0.5, _hip.NMS_AGNOSTIC)}
FORWARD = ("forward", "forward_u8", "forward_timed")
LOSS = ("loss", "loss_u8", "loss_grad")
LOSS_V3 = ("loss_v3", "loss_v3_u8", "loss_v3_grad")
# ignore_thresh of every YOLOv3 loss call and train step of the table.  Not the engine's default of 0.7: on the calibrated synthetic weights
# no row of the four images overlaps a truth by more than 0.5 on YOLOv3 fp16 and mxfp8 (0.7, 0.6: no ignored row on any plan; 0.5: one
# on YOLOv3-SPP and YOLOv3-tiny, none on the other two), and a loss without an ignored row (-2 in `assign`) leaves that branch unrun.  At
# 0.4: 1 (fp16), 3 (mxfp8), 1 (SPP), 4 (tiny) ignored rows and 6 truth rows; the control of tests/test_gpu_sequences.py asserts both kinds.
IGNORE_THRESH = 0.4
REFUSE = "refuse"
# the four training families: the YOLOv2 detection layer, the head convs of a YOLOv3 network, the last 3 x 3 block and the detection layer
# of a YOLOv2 network, the head convs of a YOLOv3 network and the 3 x 3 block behind each.  family -> (init kind, step kind, uint8 step kind)
FAMILIES = {"head": ("head_train_init", "train", "train_u8"),
            "v3": ("head_train_v3_init", "train_v3", "train_v3_u8"),
            "tail": ("tail_train_init", "train_tail", "train_tail_u8"),
            "blocks": ("blocks_train_v3_init", "train_blocks_v3", "train_blocks_v3_u8")}
MODE_FAMILIES = ("tail", "blocks")      # the families whose steps look at the mode yolo_net_train_set_wgrad_f16 sets (csrc/train_api.cpp: block_wgrad_check)
SET_ON, SET_OFF = ("set_wgrad_f16", True), ("set_wgrad_f16", False)
INITS = {f[0]: name for name, f in FAMILIES.items()}                        # init kind -> family
STEPS = {k: name for name, f in FAMILIES.items() for k in f[1:]}            # step kind -> family
CHANGING = ("train", "train_u8", "head_train_init", "load_weights", "rebind", "set_streams", "autotune", "tune_streams",
            "head_train_v3_init", "train_v3", "train_v3_u8", "tail_train_init", "train_tail", "train_tail_u8",
            "blocks_train_v3_init", "train_blocks_v3", "train_blocks_v3_u8", "set_wgrad_f16", "poison_extra")
V3_KINDS = FORWARD + tuple(DETECT) + LOSS_V3 + (REFUSE,)
V2_KINDS = FORWARD + tuple(DETECT) + LOSS + (REFUSE,)
SWITCH_KINDS = ("forward", "forward_u8", "forward_timed", "detect@0.5", "detect@0.05/per-class", "detect@0.9999", REFUSE)

# what -> (status code, a part of yolo_last_error): include/yolo_hip.h, csrc/api.cpp, csrc/train_api.cpp, csrc/loss3_host.cpp
ERR_ARG, ERR_STATE = 1, 5
REFUSALS = {"batch+1": (ERR_ARG, "batch outside 1..max_batch"),
            "loss-on-v3": (ERR_ARG, "the head must be version 2"),
            "loss_grad-on-v3": (ERR_ARG, "the head must be version 2"),
            "loss_v3-on-v2": (ERR_ARG, "the head must be version 3"),
            "set_streams(3)": (ERR_STATE, "yolo_net_set_streams"),
            "train-null-state": (ERR_ARG, "null state"),
            "train-two-parts": (ERR_STATE, "call yolo_net_set_streams(net, 1)"),
            "train_v3-two-parts": (ERR_STATE, "call yolo_net_set_streams(net, 1)"),
            "set_streams(1)-split-arenas": (ERR_STATE, "part(s) only"),
            "train_blocks-on-mxfp8": (ERR_STATE, "the plan runs the conv behind the head conv as an MXFP8 conv"),
            "train_blocks-two-parts": (ERR_STATE, "call yolo_net_set_streams(net, 1)"),
            "set_wgrad_f16-on-fp32": (ERR_STATE, "a float32 plan stores float32 activations"),
            "set_wgrad_f16-too-small": (ERR_ARG, "buffer too small (yolo_net_train_wgrad_f16_bytes)"),      # bytes: one less than ..._wgrad_f16_bytes
            "set_wgrad_f16-unaligned": (ERR_ARG, "the buffer must be 256-byte aligned")}
V3_REFUSALS = ("batch+1", "loss-on-v3", "set_streams(3)", "loss_grad-on-v3")
V2_REFUSALS = ("batch+1", "set_streams(3)", "train-null-state", "loss_v3-on-v2")
# the refused sets come first in a MODE plan's refusals: each_pure(sid, 0) then makes the too-small one, each_pure(sid, 1) the unaligned one
SET_REFUSALS = ("set_wgrad_f16-too-small", "set_wgrad_f16-unaligned")

# truths of the four images (x, y, w, h, class): one image has none
TRUTHS = [[(0.3, 0.4, 0.2, 0.5, 1), (0.8, 0.2, 0.3, 0.3, 2)], [], [(0.5, 0.5, 0.6, 0.4, 7)],
          [(0.2, 0.7, 0.15, 0.25, 3), (0.6, 0.3, 0.4, 0.5, 0), (0.9, 0.9, 0.1, 0.1, 12)]]
MAX_GT = 3
FRAME_SIZES = ((120, 90), (75, 200), (64, 64), (50, 131))     # detect_frames: frame i of the plan's four, letterboxed
LR = 1e-3
TAIL_LR = 1e-4      # tests/test_gpu_train_tail.py: the block's weights all move by lr in Adam's first step, at 1e-3 the second step's logits overflow exp()
BLOCKS_LR = blocks_v3_cases.TRAIN_LR        # 1e-5, the rate tests/test_gpu_train_blocks_v3.py trains twenty steps with: every weight of three blocks moves by lr in step 1


def step_lr(kind):
    """the learning rate of a train step of the table"""
    return {"tail": TAIL_LR, "blocks": BLOCKS_LR}.get(STEPS[kind], LR)


def is_changing(call):
    return call[0] in CHANGING


def is_pure(call):
    return not is_changing(call)


def is_sparse_detect(call):
    """a detect whose head convs skip rows below the threshold's logit (api.cpp detect_any: thresholds inside (0, 1 - 1e-4))"""
    return call[0] in DETECT and 0.0 < DETECT[call[0]][1] < 1.0 - 1e-4


def batch_of(call):
    """images of a call, None where it has none (a refusal, a call that takes no batch)"""
    return call[2] if call[0] != REFUSE and len(call) >= 3 else None


# What a changing call reads and writes of the state a net and its engine carry between calls, as the drop rules of twin_key see it.  A
# write replaces the whole of what it names.  PACKED: the regions of the device weights a family's init and steps re-pack.
# "wgrad mode": net->wgrad_f16_dev / wgrad_f16_bytes, read by the steps of MODE_FAMILIES alone; "wgrad scratch": the bytes of the engine's
# buffer behind that pointer, which nobody reads -- every byte a step reads of it is one the same step wrote --, so a poison_extra is
# dropped from every twin.
PACKED = {"head": ("packed head",), "v3": ("packed v3 heads",), "tail": ("packed head", "packed block"), "blocks": ("packed v3 heads", "packed v3 blocks")}
STATE = {"head": "head state", "v3": "v3 state", "tail": "tail state", "blocks": "blocks state"}
NET = ("packed head", "packed block", "packed v3 heads", "packed v3 blocks", "workspace", "streams", "tiles")     # what every call that runs the net reads


def effects(call):
    """(what the changing call reads, what it writes)"""
    kind = call[0]
    if kind == "load_weights":
        return set(), {"packed head", "packed block", "packed v3 heads", "packed v3 blocks"}
    if kind == "set_wgrad_f16":
        return set(), {"wgrad mode"}
    if kind == "poison_extra":
        return set(), {"wgrad scratch"}
    if kind in INITS:
        return set(), {STATE[INITS[kind]]} | set(PACKED[INITS[kind]])
    if kind in STEPS:       # forward through all packed weights, the family's state updated, its layers re-packed from it
        mode = {"wgrad mode"} if STEPS[kind] in MODE_FAMILIES else set()
        return set(NET) | {STATE[STEPS[kind]]} | mode, {STATE[STEPS[kind]]} | set(PACKED[STEPS[kind]])
    # a re-bind, a stream count, tuned tiles: each is the history of its own piece of state (the very thing a sequence is about), so it
    # reads what it writes and is never dropped
    if kind == "rebind":
        return {"workspace"}, {"workspace"}
    if kind == "set_streams":
        return {"streams"}, {"streams"}
    if kind == "autotune":
        return set(NET), {"tiles"}
    if kind == "tune_streams":
        return set(NET), {"streams"}
    raise ValueError(call)


def observes(call):
    """what the result of a call may depend on: the net; for a train step its family's training state as well, and for a tail or a
    blocks step the mode.  No call but a step of its family reads a training state (a pure call has no access to one), and no pure call
    and no head-only step looks at the mode."""
    return set(NET) | (effects(call)[0] if is_changing(call) else set())


def twin_key(sequence, i):
    """(the changing calls a twin executes first, in order; the call itself).

    Replaying every changing call in front of i is always a correct twin.  A call is dropped only when everything it wrote has since been
    overwritten and no retained call in between read it -- dead-store elimination, backwards from what call i observes (observes), over
    effects:
      * a train step, or an init, is dropped behind a later init of its family or a load_weights that overwrite all it wrote, unless a
        retained step in between (of any family: each runs the whole net) read it.  With two training states on one net both are
        followed: tail_train_init re-packs the head that a head-only step packed, so that step is dropped where nothing read it, while a
        tail step that ran on the head-only step's weights keeps it;
      * load_weights does not reset a training state.  A step behind it with no init of its family in between reads the state the
        earlier steps left, and they are retained (the table has no such step: tests/test_sequences_cpu.py);
      * load_weights itself is dropped where no train step is retained in front of it: an init packs what load_weights packs, the net
        is as it was loaded;
      * set_wgrad_f16 writes the mode and reads nothing: of on -> on the first is dropped (the second replaces the buffer and nothing
        else), of on -> off the `on` where no retained tail or blocks step ran under it; no init and no load_weights writes the mode, so
        a set is retained through them (which keeps the twin right and asserts nothing about an init: the twin replays it behind the same
        set; MODE_SURVIVES compares across keys for that).  A set(off) with no set(on) retained in front of it is dropped as well, as load_weights is: the
        net is as it was built, and the twin is one that never switched;
      * poison_extra writes what nobody reads and is always dropped;
      * rebind, set_streams, autotune and tune_streams are never dropped."""
    calls = [c for c in sequence[:i] if is_changing(c)]
    while True:
        live, kept = observes(sequence[i]), []
        for c in reversed(calls):
            reads, writes = effects(c)
            if writes & live:
                kept.append(c)
                live = (live - writes) | reads
        kept.reverse()
        kept = [c for j, c in enumerate(kept) if c[0] != "load_weights" or any(p[0] in STEPS for p in kept[:j])]
        kept = [c for j, c in enumerate(kept) if c != SET_OFF or SET_ON in kept[:j]]
        if kept == calls:
            return tuple(calls), sequence[i]
        calls = kept


# ---- plans -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def switch_max_batch(net="v3", dtype="fp16"):
    """the smallest max_batch at which streams = 0 (the library's rule) plans two full arenas for the network at the table's input size:
    read from engine.Plan (yolo_net_set_streams(net, 1) is accepted only by such a plan), found by doubling and bisection"""
    from tensorflow_yolo_amd.net import engine

    def two(mb):
        p = engine.Plan(P.create_network(net), dtype=dtype, max_batch=mb, streams=0)
        ok = p.num_streams == 2 and p.lib.yolo_net_set_streams(p.handle, 1) == 0
        p.close()
        return ok
    hi = 2
    while not two(hi):
        hi *= 2
        assert hi <= 4096, "the rule never plans two full arenas for %s %s" % (net, dtype)
    lo = hi // 2            # (not two, or hi == 2)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if two(mid) else (mid, hi)
    return hi


PLANS = {}      # id -> dict(pid = row of poison_cases.PLANS, more = engine options over that row's, kinds, refusals, train, streams)


def _plan(sid, pid, kinds, refusals, train=(), streams=1, max_batch=MAX_BATCH):
    """train: the families (FAMILIES) the plan's sequences train, the first one the plan's own"""
    PLANS[sid] = dict(pid=pid, more={"streams": streams, "max_batch": max_batch}, kinds=kinds, refusals=refusals, train=tuple(train), streams=streams)


_plan("v2-fp16", "v2-fp16-plan", V2_KINDS, V2_REFUSALS, train=("head",))
_plan("v2-fp32", "v2-fp32-plan", V2_KINDS, V2_REFUSALS, train=("head",))
_plan("v2-tiny-fp16", "v2-tiny-fp16-plan", V2_KINDS, V2_REFUSALS)
_plan("v3-fp16", "v3-fp16-plan", V3_KINDS, V3_REFUSALS)
_plan("v3-mxfp8", "v3-mxfp8-plan", V3_KINDS, V3_REFUSALS + ("train_blocks-on-mxfp8",))      # (the conv behind each head conv is an MXFP8 conv there)
_plan("v3-spp-fp16", "v3-spp-fp16-plan", V3_KINDS, V3_REFUSALS)
_plan("v3-tiny-fp32", "v3-tiny-fp32-plan", V3_KINDS, V3_REFUSALS)
# streams = 0 at the smallest max_batch where the rule plans two full arenas: the plan yolo_net_set_streams can switch (max_batch: None
# until asked for -- plan_kw -- since finding it plans the network a dozen times)
_plan("v3-fp16-switch", "v3-fp16-plan", SWITCH_KINDS, ("batch+1", "set_streams(3)", "train_v3-two-parts", "train_blocks-two-parts"), train=("v3",), streams=0,
      max_batch=None)
# YOLOv2 is never given two arenas by the rule (fewer than 40 conv launches), so its two-part plan is one with streams = 2: split arenas,
# which yolo_net_set_streams cannot switch.  The train step is refused there; that it is accepted after set_streams(1) cannot be shown
# on a YOLOv2 plan (v3-fp16-switch shows it for the YOLOv3 step).
_plan("v2-fp16-two-parts", "v2-fp16-plan", ("forward", "detect@0.5", "loss", REFUSE), ("train-two-parts", "set_streams(1)-split-arenas"), streams=2)
# Training plans, over rows the table has already (a plan id of its own each: the cap on twin keys is per plan id).  The head convs of
# the MXFP8 plan are fp16 convs and trainable; yolo_net_tail_inputs accepts the three YOLOv2 rows at 160 x 160 (test_sequences_cpu.py).
TRAIN_V3 = ("v3-fp16-train", "v3-tiny-fp32-train", "v3-mxfp8-train")
TRAIN_TAIL = ("v2-fp16-tail", "v2-fp32-tail", "v2-tiny-fp16-tail")
for _sid in TRAIN_V3:
    _plan(_sid, _sid[:-len("-train")] + "-plan", V3_KINDS, V3_REFUSALS, train=("v3",))
for _sid in TRAIN_TAIL:
    _plan(_sid, _sid[:-len("-tail")] + "-plan", V2_KINDS, V2_REFUSALS, train=("tail",))
# Two training states on one net, head-only and tail: the `head-and-tail` sequence of the tail rows, under ids of its own -- with the four
# training sequences a tail plan has 99 twin keys, this one needs 37 more, and the cap is 112.
HEAD_AND_TAIL = tuple(s + "-and-head" for s in TRAIN_TAIL)
for _sid in HEAD_AND_TAIL:
    _plan(_sid, PLANS[_sid[:-len("-and-head")]]["pid"], V2_KINDS, V2_REFUSALS, train=("tail", "head"))
# The fourth family, the YOLOv3 head convs and the 3 x 3 block behind each: the rows yolo_net_block_inputs_v3 accepts (test_sequences_cpu.py;
# the MXFP8 row is refused, which is a refusal of `v3-mxfp8`).  The float32 row refuses the fp16 mode: that refusal is among its pure kinds.
BLOCKS = ("v3-fp16-blocks", "v3-tiny-fp16-blocks", "v3-tiny-fp32-blocks")
for _sid in BLOCKS:
    _plan(_sid, _sid[:-len("-blocks")] + "-plan", V3_KINDS, (("set_wgrad_f16-on-fp32",) if "fp32" in _sid else ()) + V3_REFUSALS, train=("blocks",))
# Two training states on one YOLOv3 net, head convs only and blocks, both packing the head convs: the analogue of HEAD_AND_TAIL
BLOCKS_AND_HEADS = ("v3-tiny-fp16-blocks-and-heads", "v3-fp16-blocks-and-heads")
for _sid in BLOCKS_AND_HEADS:
    _plan(_sid, _sid[:-len("-blocks-and-heads")] + "-plan", V3_KINDS, V3_REFUSALS, train=("blocks", "v3"))
# The fp16 mode of the tail and blocks steps, on the rows where yolo_net_train_wgrad_f16_bytes is not 0 (the fp16 rows).  The two tail rows
# also train the head alone (`mode-and-head`): a step that does not look at the mode.
MODE = ("v2-fp16-tail-f16", "v2-tiny-fp16-tail-f16", "v3-tiny-fp16-blocks-f16", "v3-fp16-blocks-f16")
for _sid in MODE:
    if _sid.endswith("-tail-f16"):
        _plan(_sid, _sid[:-len("-tail-f16")] + "-plan", V2_KINDS, SET_REFUSALS + V2_REFUSALS, train=("tail", "head"))
    else:
        _plan(_sid, _sid[:-len("-blocks-f16")] + "-plan", V3_KINDS, SET_REFUSALS + V3_REFUSALS, train=("blocks",))
TRAINING_PLANS = TRAIN_V3 + TRAIN_TAIL + HEAD_AND_TAIL + BLOCKS + BLOCKS_AND_HEADS + MODE      # the ids whose first sequence begins with an init and a step


def plan_kw(sid):
    """engine options of a plan over its poison_cases row"""
    more = dict(PLANS[sid]["more"])
    if more["max_batch"] is None:
        more["max_batch"] = switch_max_batch()
    return more


def build_model(sid, weights=None, **more):
    return P.build_model(PLANS[sid]["pid"], weights=weights, **dict(plan_kw(sid), **more))


def plan_only(sid):
    from tensorflow_yolo_amd.net import engine
    p = P.PLANS[PLANS[sid]["pid"]]
    kw = plan_kw(sid)
    return engine.Plan(P.create_network(p["net"]), dtype=p["dtype"], max_batch=kw["max_batch"], keep_all=p["keep_all"], streams=kw["streams"])


# ---- batches: slices of the four images ---------------------------------------------------------------------------------------------------
SLICES = ((0, 1), (0, 2), (0, 3), (0, 4), (2, 2), (1, 3), (3, 1), (1, 2))


def variants(kinds, kind):
    """the two slices a kind runs on in the walks: different batch sizes, spread over the table by the kind's place in the plan's list"""
    j = kinds.index(kind)
    a = SLICES[j % len(SLICES)]
    b = next(s for k in range(1, len(SLICES)) for s in [SLICES[(j + 3 * k) % len(SLICES)]] if s[1] != a[1])
    return a, b


def _call(sid, kind, which):
    pl = PLANS[sid]
    if kind == REFUSE:
        return (REFUSE, pl["refusals"][which % len(pl["refusals"])])
    lo, n = variants(pl["kinds"], kind)[which % 2]
    return (kind, lo, n)


def euler_kinds(kinds):
    """a closed walk over the kinds in which every ordered pair (a, b), a == b included, is adjacent exactly once: an Euler circuit of the
    complete directed graph with loops (Hierholzer, edges taken in the order of the list)"""
    k = len(kinds)
    nxt = [0] * k
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            stack.append((v + 1 + nxt[v]) % k)      # (the loop edge v -> v comes last)
            nxt[v] += 1
        else:
            out.append(stack.pop())
    out.reverse()
    return [kinds[v] for v in out]


def _with_batches(sid, kind_walk, prev_n=None):
    """kinds -> calls: of a kind's two slices the one whose batch differs from its predecessor's (both differ: the two in turn)"""
    pl = PLANS[sid]
    used, out = {}, []
    for kind in kind_walk:
        if kind == REFUSE:
            out.append(_call(sid, kind, used.get(kind, 0)))
            used[kind] = used.get(kind, 0) + 1
            continue
        a, b = variants(pl["kinds"], kind)
        ok = [s for s in (a, b) if s[1] != prev_n]
        s = ok[used.get(kind, 0) % len(ok)]
        used[kind] = used.get(kind, 0) + 1
        out.append((kind, s[0], s[1]))
        prev_n = s[1]
    return out


def _next(sid, kind, prev, other_images=False, small=False):
    """a call of `kind` at a batch size different from prev's (other_images: on images prev's call did not see as well): one of the kind's
    two slices where one fits -- no twin of its own then --, else the first slice of the table that does"""
    fits = lambda v: v[1] != prev[2] and (not other_images or not (prev[1] <= v[0] and v[0] + v[1] <= prev[1] + prev[2]))
    own = [v for v in variants(PLANS[sid]["kinds"], kind) if fits(v)]
    if small:       # (the call in front of an `other_images` step: not the whole set of images)
        own = [v for v in sorted(own, key=lambda v: v[1]) if v[1] < N_IMAGES]
    return (kind,) + (own + [v for v in SLICES if fits(v) and v[1] < N_IMAGES])[0]


def named_prologue(sid):
    """the leaks the issue names, each at a batch size different from its predecessor's: detect at 0.5 -> forward (obj_min_logit);
    detect at 0.5 -> detect at 0.05 on OTHER images (rows the first did not write); 0.9999 <-> 0.5; loss -> detect -> loss_grad;
    forward_timed -> detect (obj_valid, halves); on a YOLOv3 plan loss_v3 -> detect at 0.5 -> loss_v3_grad (rows the sparse detect left
    unwritten in front of a dense pass), detect at 0.5 -> loss_v3 on OTHER images, forward_timed -> loss_v3_u8"""
    kinds = PLANS[sid]["kinds"]
    chain = [("detect@0.5", False), ("forward", False), ("detect@0.5", "small"), ("detect@0.05", True), ("detect@0.9999", False), ("detect@0.5", False),
             ("detect@0.9999", False)]
    if "loss" in kinds:
        chain += [("loss", False), ("detect@0.5", False), ("loss_grad", False)]
    chain += [("forward_timed", False), ("detect@0.5", False)]
    if "loss_v3" in kinds:
        chain += [("loss_v3", False), ("detect@0.5", False), ("loss_v3_grad", False), ("detect@0.5", "small"), ("loss_v3", True), ("forward_timed", False),
                  ("loss_v3_u8", False)]
    out = [("detect@0.5",) + variants(kinds, "detect@0.5")[0]]
    for kind, other in chain[1:]:
        out.append(_next(sid, kind, out[-1], other is True, other == "small"))
    return out


def cover_walk(sid):
    pro = named_prologue(sid)
    return pro + _with_batches(sid, euler_kinds(list(PLANS[sid]["kinds"])), prev_n=pro[-1][2] if pro else None)


def all_calls(sid):
    """every (kind, slice) of a plan's pure calls, and its refusals"""
    pl = PLANS[sid]
    out = []
    for kind in pl["kinds"]:
        if kind == REFUSE:
            out += [(REFUSE, w) for w in pl["refusals"]]
        else:
            out += [(kind, lo, n) for lo, n in variants(pl["kinds"], kind)]
    return out


def random_walk(sid, seed=0, length=24):
    rng = random.Random("%s/%d" % (sid, seed))
    pool = all_calls(sid)
    return [pool[rng.randrange(len(pool))] for _ in range(length)]


def each_pure(sid, which):
    """every pure kind of the plan once, on its slice `which`"""
    return [_call(sid, kind, which) for kind in PLANS[sid]["kinds"]]


SEQUENCES = {}      # plan id -> {name: [calls]}
MAIN = ("v2-fp16", "v2-fp32", "v2-tiny-fp16", "v3-fp16", "v3-mxfp8", "v3-spp-fp16", "v3-tiny-fp32")
for _sid in MAIN:
    SEQUENCES[_sid] = {"cover": cover_walk(_sid), "random": random_walk(_sid)}

# 3. training, every family with its own init and step, in three sequences so that no item builds more than one round of twins
def training_sequences(sid, family):
    init, step, step_u8 = FAMILIES[family]
    start = [(init,), (step, 0, 3, 1)]
    return {"train-1": start + each_pure(sid, 0),
            "train-2": start + [("forward", 0, 2), (step, 0, 4, 2)] + each_pure(sid, 1),
            "train-u8-load-init": (start + [("detect@0.5", 0, 2), (step_u8, 1, 2, 2)] + each_pure(sid, 0)
                                   + [("load_weights",)] + each_pure(sid, 0) + each_pure(sid, 1)       # back to the untrained twins
                                   + [(init,), (step, 0, 3, 1)] + each_pure(sid, 0))}                  # the first step again


for _sid in ("v2-fp16", "v2-fp32"):
    SEQUENCES[_sid].update(training_sequences(_sid, "head"))
# 3b. the YOLOv3 head convs and the YOLOv2 tail; rebind-train: nothing the second step reads out of the workspace (the head convs' inputs,
# the block's input, split-K slabs, ticket counters, the logits) may survive from the first -- the workspace is 0xFF in between
for _sid in TRAIN_V3 + TRAIN_TAIL + BLOCKS:
    _init, _step, _ = FAMILIES[PLANS[_sid]["train"][0]]
    SEQUENCES[_sid] = training_sequences(_sid, PLANS[_sid]["train"][0])
    SEQUENCES[_sid]["rebind-train"] = [(_init,), (_step, 0, 3, 1), ("rebind",), (_step, 1, 3, 2)] + each_pure(_sid, 1)
# 3c. two training states on one net, both packing the head: a head-only step, a tail step on the head it packed, a head-only step on the
# block the tail step packed; then head_train_init again, behind which the head-only step is the first step on the TAIL-trained block
for _sid in HEAD_AND_TAIL:
    SEQUENCES[_sid] = {"head-and-tail": [("head_train_init",), ("train", 0, 3, 1), ("tail_train_init",), ("train_tail", 0, 2, 1), ("train", 0, 4, 2)]
                       + each_pure(_sid, 0) + [("head_train_init",), ("train", 0, 3, 1)] + each_pure(_sid, 1)}
# 3d. ... and on a YOLOv3 net, both packing the head convs: a head-convs step, a blocks step on the heads blocks_train_v3_init packed again
# (its twin ran that init alone), a head-convs step on the blocks the blocks step packed; then head_train_v3_init again
for _sid in BLOCKS_AND_HEADS:
    SEQUENCES[_sid] = {"blocks-and-heads": [("head_train_v3_init",), ("train_v3", 0, 3, 1), ("blocks_train_v3_init",), ("train_blocks_v3", 0, 2, 1), ("train_v3", 0, 4, 2)]
                       + each_pure(_sid, 0) + [("head_train_v3_init",), ("train_v3", 0, 3, 1)] + each_pure(_sid, 1)}


# 3e. the fp16 mode of the tail and blocks steps, a bit on the net and a buffer of the engine's
def mode_sequences(sid):
    """mode: (1) init, set(on), step 1, every pure kind -- the refused too-small set among them, under the mode; (2) 0xFF into the
    engine's buffer, step 2 at another batch size: what it reads of the buffer it wrote itself, and the refused set left the mode on;
    (3) set(off), step 3, every pure kind on the other slice; (4) set(on), the too-small set refused once more, a uint8 step 4; (5)
    load_weights, every pure kind: the untrained twins; (6) init and step 1 again: load_weights does not touch the mode (that the init does not is MODE_SURVIVES' to hold), the twin
    is [set(on), init, step]; (7) set(off), init, step 1: the twin is the one that never switched.  A twin of (3) replays on and off
    itself, so a set(off) that clears nothing shows at (7) alone.
    mode-before-init: set(on), a loss under it (no pure call looks at the mode), set(on) again (it replaces the buffer and nothing else), init, step 1, re-bind onto 0xFF, step 2, every pure
    kind.  mode-and-head, where the plan trains the head alone as well: tail init, set(on), tail step, head init, head-only step (it does
    not look at the mode), tail step, every pure kind."""
    init, step, step_u8 = FAMILIES[PLANS[sid]["train"][0]]
    refused = (REFUSE, "set_wgrad_f16-too-small")
    under = _call(sid, "loss_v3" if "loss_v3" in PLANS[sid]["kinds"] else "loss", 0)        # its twin: the untrained one, which never set the mode
    out = {"mode": ([(init,), SET_ON, (step, 0, 3, 1)] + each_pure(sid, 0) + [("poison_extra",), (step, 0, 4, 2)]
                    + [SET_OFF, (step, 0, 2, 3)] + each_pure(sid, 1) + [SET_ON, refused, (step_u8, 1, 3, 4)]
                    + [("load_weights",)] + each_pure(sid, 0) + [(init,), (step, 0, 3, 1)] + [SET_OFF, (init,), (step, 0, 3, 1)]),
           "mode-before-init": [SET_ON, under, SET_ON, (init,), (step, 0, 3, 1), ("rebind",), (step, 1, 3, 2)] + each_pure(sid, 1)}
    if "head" in PLANS[sid]["train"]:
        out["mode-and-head"] = ([(init,), SET_ON, (step, 0, 3, 1), ("head_train_init",), ("train", 0, 2, 1), (step, 0, 4, 2)] + each_pure(sid, 0))
    return out


for _sid in MODE:
    SEQUENCES[_sid] = mode_sequences(_sid)
# (the plan of the unsynchronised run below: train-2 under the mode, also run item by item so that its twins count against the cap)
MODE_ASYNC = "v3-tiny-fp16-blocks-f16"
_init, _step, _ = FAMILIES[PLANS[MODE_ASYNC]["train"][0]]
SEQUENCES[MODE_ASYNC]["train-2"] = [(_init,), SET_ON, (_step, 0, 3, 1), ("forward", 0, 2), (_step, 0, 4, 2)] + each_pure(MODE_ASYNC, 1)



# 3f. what must leave the mode alone.  A twin that replays the suspect call behind the same set(on) cannot see it clear the mode -- engine
# and twin would both run float32 steps -- so these are comparisons ACROSS twin keys, not of a sequence with its twin:
#   equal:  two keys whose first steps must be byte-equal.  The family's own init behind set(on) against in front of it (the mode bit is
#           all that could differ: both keys are the sequences' own, row 6 of `mode` and its first step); on a tail plan head_train_init
#           between set(on) and the tail step against the key without it (it packs the head tail_train_init packed, from the same values).
#   differ: two keys whose first steps must differ in dw3 -- the same prefix with and without set(on), with a re-bind onto 0xFF between
#           the set and the step: the mode is still on behind yolo_net_bind_workspace.  (Equality with the key that has no re-bind would
#           claim more than the mode: twin_key never drops a re-bind.)
# yolo_net_set_streams is not here: on these plans it returns before it does anything, and the plan it can switch has 196 images a batch.
def mode_survives(sid):
    init, step, _ = FAMILIES[PLANS[sid]["train"][0]]
    first = (step, 0, 3, 1)
    equal = [(((init,), SET_ON), (SET_ON, (init,)))]
    if "head" in PLANS[sid]["train"]:
        equal.append((((init,), SET_ON), ((init,), SET_ON, ("head_train_init",))))
    differ = [(((init,), SET_ON, ("rebind",)), ((init,), ("rebind",)))]
    return {"equal": [((a, first), (b, first)) for a, b in equal], "differ": [((a, first), (b, first)) for a, b in differ]}


MODE_SURVIVES = {_sid: mode_survives(_sid) for _sid in MODE}

# 5. a re-bind onto an 0xFF-filled buffer in the middle of a walk
for _sid in ("v2-fp16", "v3-fp16", "v3-tiny-fp32"):
    SEQUENCES[_sid]["rebind"] = SEQUENCES[_sid]["random"][:8] + [("rebind",)] + each_pure(_sid, 1) + [("detect@0.05", 0, 4), ("forward", 0, 1)]

# 6. refusals in the middle of a walk: every refusal of the plan between two calls of the covering walk's set
for _sid in MAIN:
    _seq = []
    for _i, _w in enumerate(PLANS[_sid]["refusals"]):
        _seq += [_call(_sid, ("detect@0.5", "forward", "detect@0.05/per-class")[_i % 3], _i), (REFUSE, _w), _call(_sid, ("forward", "detect@0.5", "forward_u8")[_i % 3], _i + 1)]
    SEQUENCES[_sid]["refusals"] = _seq


# 4. the plan yolo_net_set_streams can switch: a full batch and one image more than half of it run as two parts, 4, 2 and 3 images as one
def switch_sequence(mb):
    body = [("forward", 0, mb), ("detect@0.5", 0, mb // 2 + 1), ("forward", 0, 4), ("detect@0.5", 0, 2), ("detect@0.05/per-class", 0, 3), ("forward_timed", 0, 2),
            (REFUSE, "set_streams(3)"), ("forward_u8", 0, 4), ("detect@0.9999", 0, 3)]
    return [("set_streams", 2)] + body + [("set_streams", 1)] + body + [("set_streams", 2)] + body


def switch_body(mb):
    """every pure kind of the switchable plan: the full batch and one image more than half of it as two parts, 4, 2 and 3 images as one"""
    return switch_sequence(mb)[1:10]


def switch_train_sequence(mb):
    """the train step of the YOLOv3 head convs on the plan yolo_net_set_streams can switch: refused at two parts (each part has its own
    arena: which one would the head convs' inputs be read from), accepted after set_streams(1); back at two parts both arenas see the
    trained heads; refused again; a second step after the next switch.  yolo_net_set_streams changes which arena a head input lives in."""
    refused = (REFUSE, "train_v3-two-parts")
    return ([("set_streams", 2), ("forward", 0, mb), refused, ("set_streams", 1), ("head_train_v3_init",), ("train_v3", 0, 4, 1), ("set_streams", 2),
             ("detect@0.5", 0, mb)] + switch_body(mb) + [(REFUSE, "train_blocks-two-parts"), refused, ("set_streams", 1), ("train_v3", 0, 3, 2)]
            + switch_body(mb))     # (a body begins with the full batch; the blocks step is refused at two parts as the head step is, with or without a state)


SEQUENCES["v2-fp16-two-parts"] = {"refused-train": [("forward", 0, 4), (REFUSE, "train-two-parts"), ("forward", 0, 4), ("detect@0.5", 0, 3),
                                                    (REFUSE, "set_streams(1)-split-arenas"), ("detect@0.5", 0, 3), ("loss", 0, 4), (REFUSE, "train-two-parts"),
                                                    ("loss", 0, 4), ("forward", 0, 1)]}
ALL_PLANS = MAIN + ("v3-fp16-switch", "v2-fp16-two-parts") + TRAINING_PLANS


def sequences_of(sid):
    if sid == "v3-fp16-switch" and sid not in SEQUENCES:        # (planned a dozen times to find its max_batch: when first asked for)
        SEQUENCES[sid] = {"switch": switch_sequence(switch_max_batch()), "switch-train": switch_train_sequence(switch_max_batch())}
    return SEQUENCES[sid]


# One pytest item per (plan, sequence, part).  A part runs its sequence from the start to its own end and compares the calls from its own
# start on: the parts of a sequence together compare every call of it, and each part meets at most TWINS_PER_ITEM twin keys that no part
# in front of it (in the order of this list) has met -- the twins it has to build, which is where an item's time goes.
TWINS_PER_ITEM = 8


def builds_twin(call):
    """a call whose result is compared with a twin's: a pure call, a train step (the other changing calls return nothing)"""
    return is_pure(call) or call[0] in STEPS


def control_engines(sid):
    """the engines the plan's first item builds for the controls that came with the YOLOv3 loss and the training families, beyond the twins
    its sequences cache: the second twin of each controlled call (tests/test_gpu_sequences.py: control) -- a loss_v3 call on a YOLOv3
    plan; on a training plan id a forward, a detect and the first step as well, and for head-and-tail the forward behind that step, which
    is no call of the sequence; the same for blocks-and-heads; on a MODE plan the first step with the mode off as well, which the one with
    the mode on must differ from (it is also the twin of the last step of `mode`, where it is counted once more: the count is an upper
    bound, the item that meets it there is cut one twin short).  They count against the first item's twins, so that it costs what any
    other item costs."""
    kinds = PLANS[sid]["kinds"]
    if sid in TRAINING_PLANS:
        return 3 + ("loss_v3" in kinds) + (sid in HEAD_AND_TAIL + BLOCKS_AND_HEADS + MODE)
    return int("loss_v3" in kinds)


def items():
    out = []
    for sid in ALL_PLANS:
        met = set()
        for k, (name, seq) in enumerate(sequences_of(sid).items()):
            start, new, part = 0, control_engines(sid) if k == 0 else 0, 1
            for i in range(len(seq)):
                key = twin_key(seq, i)
                fresh = key not in met and builds_twin(seq[i])
                if fresh and new == TWINS_PER_ITEM:
                    out.append((sid, name, part, start, i))
                    start, new, part = i, 0, part + 1
                if fresh:
                    met.add(key)
                    new += 1
            out.append((sid, name, part, start, len(seq)))
    return out


ITEMS = items()

# 8. two engines of different plans alive at once, their calls interleaved on one stream: (plan, call)
PAIR = ("v3-fp16", "v2-tiny-fp16")
INTERLEAVED = [(PAIR[i % 2], c) for i, c in enumerate(
    x for pair in zip(SEQUENCES[PAIR[0]]["random"][:12], SEQUENCES[PAIR[1]]["random"][:12]) for x in pair)]

# 8b. ... and two engines that both TRAIN, a YOLOv2 tail and the YOLOv3 head convs: (plan, call), each engine's calls the start of its
# train-2 sequence (init, step, forward, step, pure kinds), so that every twin is one of that sequence's
PAIR_TRAIN = ("v2-tiny-fp16-tail", "v3-tiny-fp32-train")
INTERLEAVED_TRAIN_CALLS = 12
INTERLEAVED_TRAIN = [(PAIR_TRAIN[i % 2], c) for i, c in enumerate(
    x for pair in zip(SEQUENCES[PAIR_TRAIN[0]]["train-2"][:INTERLEAVED_TRAIN_CALLS], SEQUENCES[PAIR_TRAIN[1]]["train-2"][:INTERLEAVED_TRAIN_CALLS]) for x in pair)]

# 8c. ... and a blocks engine and a tail engine that both train in the fp16 mode, each in a buffer of its own: each engine's calls the start
# of its `mode` sequence, up to the second step -- the one behind the 0xFF in its buffer
PAIR_MODE = ("v3-tiny-fp16-blocks-f16", "v2-tiny-fp16-tail-f16")
INTERLEAVED_MODE_CALLS = 20
INTERLEAVED_MODE = [(PAIR_MODE[i % 2], c) for i, c in enumerate(
    x for pair in zip(SEQUENCES[PAIR_MODE[0]]["mode"][:INTERLEAVED_MODE_CALLS], SEQUENCES[PAIR_MODE[1]]["mode"][:INTERLEAVED_MODE_CALLS]) for x in pair)]

# 9. the covering walk without any host synchronisation between the calls (the plans that have one), and the train-2 sequence of one
# plan of each training family (the plans that train); of a MODE plan train-2 with a set(on) in front of the first step -- set(off) waits
# for the device inside the engine and stays out of this run
ASYNC_PLANS = ("v2-fp16", "v3-fp16", "v3-tiny-fp32-train", "v2-tiny-fp16-tail", "v3-tiny-fp16-blocks", MODE_ASYNC)

# 7. exact chains (tests/test_gpu_exact.py's list; integer data: every tile and every split must give the integer reference), each run as
# forward (1 image) -> autotune -> forward (3) -> tune_streams -> forward (2) -> forward_u8 -> forward (3) at max_batch 3
EXACT_CHAINS = {"conv-c256to512_linear_bias-fp16-tdef": dict(variant="pool", feature=",1launch"),         # a ticketed split-K conv
                "stem-3-32-64-32-3x40x56": dict(variant=None, feature="conv_stem<f16,3-32-64-32>")}       # the stem
EXACT_BATCH = 3
EXACT_STEPS = (("forward", 0, 1), ("autotune", 0, 3), ("forward", 0, 3), ("tune_streams", 0, 3), ("forward", 0, 2), ("forward_u8", 0, 3), ("forward", 0, 3))


def twin_keys(sid):
    """the distinct twin keys of all sequences of a plan (the interleaved and the unsynchronised walks use calls of these sequences), and
    of a MODE plan the keys MODE_SURVIVES compares"""
    keys = {k for pairs in MODE_SURVIVES.get(sid, {}).values() for pair in pairs for k in pair}
    for seq in sequences_of(sid).values():
        keys.update(twin_key(seq, i) for i in range(len(seq)))
    return keys

"""GPU: a net's answers must not depend on the calls before them.

A yolo_net carries state from one call to the next -- on the host (obj_min_logit, obj_valid, cand_clean, side_ok, parts / halves, the
tiles autotune chose) and on the device (the packed weights of the layers a train step re-packs, split-K ticket counters, candidate
counters, the logits region with rows a sparse detect did not write, the compact objectness array, split-K slabs, the lifetime-packed
arenas a train step reads activations out of, the fork / join events); an engine adds up to four training states (the YOLOv2 head, the
YOLOv3 head convs, the YOLOv2 tail, the YOLOv3 head convs with the blocks behind them), the buffer of the fp16 weight-gradient mode -- a
bit on the net that yolo_net_train_set_wgrad_f16 sets -- and torch.empty scratch, assign and parts tensors per call.  Every other GPU test asks its question of
a freshly built engine.  Here whole sequences of calls run on ONE engine (tests/sequence_cases.py has the table and the rule,
tests/test_sequences_cpu.py its properties), and the result of every call is compared, bit for bit, with the result of the same call on a
TWIN: a fresh engine that has executed only the changing calls in front of it that still matter (sequence_cases.twin_key).  Twins are
cached per module by that key (the largest ones, the states of tail steps, only while memory allows: an evicted twin is built again);
every twin is closed as soon as its one result is on the host, every other engine when the module ends.

What is compared: logits and gradients as bytes; counts, status and the first counts[n] records of every image of a detect; the named
fields of the loss records (`images`, `result`) of the YOLOv2 and the YOLOv3 loss, `assign` and `grad` as bytes; of a YOLOv2 head step the
result and the six state arrays; of a YOLOv3 head step the result and per scale s the masters w[s], b[s], the moments m_w[s], v_w[s],
m_b[s], v_b[s] and the gradients dw[s], db[s] of the engine's state; of a tail step the result and the sixteen parts of the tail state
(TAIL_PARTS: the head's eight and the block's eight); of a blocks step the result and per scale s those sixteen (`dw3[1]`: the weight
gradient of the block behind head conv 1); the status code and message of a refused call.  There is no tolerance anywhere.

Controls come first, per plan: two fresh twins making the same call give the same bytes -- a forward and a detect, a loss_v3 call where
the plan has one, the first train step where the plan's sequences train.  If one fails the finding is NON-DETERMINISM, not call order,
and the plan's sequences stop there.  The controls also hold the fixture to exercising the code: boxes are found, loss_v3 assigns truth
rows and ignores rows, the first step's weight gradients (dw; dw3 of every trained block where the plan's first step is a tail or a blocks
step -- on the blocks-and-heads ids it is a head-convs step, and their blocks step is held by the same rows under the blocks ids) are
non-zero on every scale and the forward behind it differs from the untrained one; on a plan of the fp16 mode the first step's dw3 with the mode on differs from the one with it off.

How to read a failure: it names the plan and the sequence, the index and the call, the call in front of it (and whether that was a sparse
detect: head rows below the threshold's logit not written) and the last changing call, the changing calls the twin replayed, and the
first differing (image, row, column), record or state array (`m_w[1]`: the first moment of the kernel of scale 1).  The call in front is
the suspect; the state it may have left is listed in DESIGN.md section 5, "Call order".  A state array that differs while `result` does not
points at the state (an init that did not start it again, a part another family's step wrote); `result` or `dw` differing points at the
forward behind the step: packed weights, or what the step read out of the workspace."""
import ctypes as C
import functools

import numpy as np
import pytest

import exact_ref as X
import poison_cases as P
import sequence_cases as S
import test_gpu_exact as E
from helpers import poison_and_bind, poisoned_out
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth, train as ytrain

pytestmark = pytest.mark.gpu

CALIBRATION = {"v2": 1, "v2-tiny": 1, "v3": 8, "v3-spp": 8, "v3-tiny": 10}        # x synth.HEAD_DEFAULTS' fraction, as the detect tests of these sizes use
RIGS, TWINS, CONTROL, ENGINES = {}, {}, {}, []
STATE_KEYS = ("w", "b", "m_w", "v_w", "m_b", "v_b")
V3_STATE_KEYS = STATE_KEYS + ("dw", "db")
TAIL_PARTS = ("w", "b", "m_w", "v_w", "m_b", "v_b", "dw", "db", "w3", "beta", "m_w3", "v_w3", "m_beta", "v_beta", "dw3", "dbeta")     # tests/test_gpu_train_tail.py
TWIN_CACHE_BYTES = 1 << 30      # of cached LARGE twin results; what goes over it: the oldest of OTHER plans are dropped (and built again if asked for)
LARGE_RESULT_BYTES = 32 << 20   # the state of a tail step (150 - 200 MB); the logits of the switchable plan's full batch (105 MB); the state of a
                                # blocks step on YOLOv3 (about 100 MB: four arrays of 24.8 MB over its three blocks).  A plan's own results are
                                # never dropped, only other plans': the budget need not hold a plan's working set (7 blocks steps, 8 tail steps)


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    import torch
    torch.cuda.synchronize()
    for eng in ENGINES:
        eng.close()
    del ENGINES[:]
    RIGS.clear()
    TWINS.clear()


# ---- a plan's data: weights, the four images, truths, frames -----------------------------------------------------------------------------
class Rig(object):
    def __init__(self, sid):
        import torch
        pl = S.PLANS[sid]
        row = P.PLANS[pl["pid"]]
        self.sid, self.net = sid, row["net"]
        cls, anchors, names, (h, w) = P.NETS[self.net]
        rng = np.random.RandomState(45)
        self.x8 = rng.randint(0, 256, size=(S.N_IMAGES, h, w, 3)).astype(np.uint8)
        self.xf = (self.x8 / 255.).astype(np.float32)
        self.weights = calibrated(pl["pid"])
        self.max_batch = S.plan_kw(sid)["max_batch"]
        self.xd, self.x8d = torch.from_numpy(self.xf).cuda(), torch.from_numpy(self.x8).cuda()
        gt, counts = yeval.pack_gts(S.TRUTHS, S.MAX_GT)
        self.gt_dev = torch.from_numpy(np.ascontiguousarray(gt).view(np.uint8).reshape(S.N_IMAGES, -1)).cuda()
        self.gc_dev = torch.from_numpy(counts).cuda()
        self.frames = [torch.from_numpy(rng.randint(0, 256, size=s + (3,)).astype(np.uint8)).cuda() for s in S.FRAME_SIZES]
        self.big = {}
        self.dummy = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")     # arguments of refused calls: never read or written
        # what the inits of the plan's training families start from: the layers' own values in the rig's stream
        layers = P.create_network(self.net) if pl["train"] else None
        if "head" in pl["train"]:
            cout, cin = ytrain.head_counts(layers)[:2]
            self.head = ytrain.split_head(self.weights, cout, cin)
        if "tail" in pl["train"]:
            self.tail = ytrain.split_tail(self.weights, layers)
        if "v3" in pl["train"]:
            self.heads_v3 = ytrain.split_heads(self.weights, ytrain.head_convs_v3(layers))
        if "blocks" in pl["train"]:
            self.blocks_v3 = (ytrain.split_blocks(self.weights, ytrain.block_convs_v3(layers)),) + ytrain.split_heads(self.weights, ytrain.head_convs_v3(layers))

    def images(self, lo, n, u8=False):
        """images lo .. lo + n - 1 on the device; more than the four distinct ones (the switchable plan): image i is distinct image i mod 4"""
        import torch
        src = self.x8d if u8 else self.xd
        if lo + n <= S.N_IMAGES:
            return src[lo:lo + n]
        if (n, u8) not in self.big:
            self.big[(n, u8)] = src[torch.arange(n, device=src.device) % S.N_IMAGES].contiguous()
        return self.big[(n, u8)]

    def gts(self, lo, n):
        return self.gt_dev[lo:lo + n], self.gc_dev[lo:lo + n]


@functools.lru_cache(maxsize=None)
def calibrated(pid):
    """the synthetic stream of the row's network with its objectness biases re-centred on the four images (synth.calibrate_model), so that
    the detect calls find boxes to compare (control); a pure function of the row"""
    row = P.PLANS[pid]
    cls, anchors, names, (h, w) = P.NETS[row["net"]]
    x8 = np.random.RandomState(45).randint(0, 256, size=(S.N_IMAGES, h, w, 3)).astype(np.uint8)
    model = P.build_model(pid, weights=P.weights_of(row["net"]), max_batch=S.MAX_BATCH, streams=1)
    w_ = synth.calibrate_model(model, (x8 / 255.).astype(np.float32), CALIBRATION[row["net"]] * synth.HEAD_DEFAULTS[cls.version][1])
    model.net.engine.close()
    w_.setflags(write=False)
    return w_


def rig(sid):
    if sid not in RIGS:
        RIGS[sid] = Rig(sid)
    return RIGS[sid]


def new_engine(sid, keep=True):
    """a fresh engine of the plan with the rig's weights.  The stream count never comes from a measurement here: the one-off tuning of a
    streams = 0 engine is switched off, the sequences call yolo_net_set_streams themselves"""
    model = S.build_model(sid, weights=rig(sid).weights)
    eng = model.net.engine
    eng._streams_tuned = True
    eng.sid = sid
    if keep:
        ENGINES.append(eng)
    return eng


# ---- running a call ------------------------------------------------------------------------------------------------------------------------
def refuse(r, eng, what):
    """a call the library must refuse, through the C ABI -> (status, message).  Every one of them is refused on the host before any device
    call (api.cpp), so the buffers behind the pointers are never touched; they are large enough all the same."""
    import torch
    lib, h, st = eng.lib, eng.handle, eng._stream()
    d = r.dummy.data_ptr()
    x1 = r.images(0, 1)
    gt, gc = r.gts(0, 1)
    if what == "batch+1":
        n = r.max_batch + 1
        out = torch.empty((n,) + tuple(eng.output_shape), dtype=torch.float32, device="cuda")
        rc = lib.yolo_net_forward(h, r.images(0, n).data_ptr(), n, out.data_ptr(), st)
    elif what == "loss-on-v3":
        rc = lib.yolo_net_loss(h, x1.data_ptr(), 1, gt.data_ptr(), gc.data_ptr(), S.MAX_GT, d, None, d + 4096, st)
    elif what == "loss_grad-on-v3":
        rc = lib.yolo_v2_loss_grad(C.byref(eng.head), d, 1, gt.data_ptr(), gc.data_ptr(), S.MAX_GT, d + 4096, d + 8192, d + 12288, d + 16384, st)
    elif what == "set_streams(3)":
        rc = lib.yolo_net_set_streams(h, 3)
    elif what == "set_streams(1)-split-arenas":
        rc = lib.yolo_net_set_streams(h, 1)
    elif what in ("train-null-state", "train-two-parts"):
        state = None if what == "train-null-state" else d + 256 - d % 256
        rc = lib.yolo_net_train_head_step(h, x1.data_ptr(), 1, gt.data_ptr(), gc.data_ptr(), S.MAX_GT, state, float(S.LR), d + 32768, st)
    elif what == "loss_v3-on-v2":       # (net_loss_v3_any: the head's version is looked at before the net is, nothing is launched)
        rc = lib.yolo_net_loss_v3(h, x1.data_ptr(), 1, gt.data_ptr(), gc.data_ptr(), S.MAX_GT, S.IGNORE_THRESH, d, d + 4096, d + 8192, d + 12288, st)
    elif what == "train_v3-two-parts":  # (head_convs_v3, the first thing the step does: refused whether or not a state exists)
        rc = lib.yolo_net_train_head_step_v3(h, x1.data_ptr(), 1, gt.data_ptr(), gc.data_ptr(), S.MAX_GT, S.IGNORE_THRESH, d + 256 - d % 256, float(S.LR),
                                             d + 32768, st)
    elif what in ("train_blocks-on-mxfp8", "train_blocks-two-parts"):       # (blocks_train_v3_layout, the first thing the step does, as above)
        rc = lib.yolo_net_train_blocks_step_v3(h, x1.data_ptr(), 1, gt.data_ptr(), gc.data_ptr(), S.MAX_GT, S.IGNORE_THRESH, d + 256 - d % 256,
                                               float(S.BLOCKS_LR), d + 32768, st)
    elif what == "set_wgrad_f16-on-fp32":       # (wgrad_f16_need refuses the plan before it looks at the buffer)
        assert lib.yolo_net_train_wgrad_f16_bytes(h) == 0
        rc = lib.yolo_net_train_set_wgrad_f16(h, d + 256 - d % 256, 32768)
    elif what in ("set_wgrad_f16-too-small", "set_wgrad_f16-unaligned"):
        # a buffer of the full size all the same, so that a set that is NOT refused leaves the net a pointer it may write through
        need = int(lib.yolo_net_train_wgrad_f16_bytes(h))
        assert need > 256, (what, need)
        buf = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
        at = buf.data_ptr() + 256 - buf.data_ptr() % 256
        rc = lib.yolo_net_train_set_wgrad_f16(h, at, need - 1) if what.endswith("too-small") else lib.yolo_net_train_set_wgrad_f16(h, at - 128, need)
        if rc == 0:     # (not refused: the pointer must not outlive `buf`; the assertion behind this call reports it)
            lib.yolo_net_train_set_wgrad_f16(h, None, 0)
    else:
        raise ValueError(what)
    return int(rc), (lib.yolo_last_error() or b"").decode()


def enqueue(r, eng, call):
    """one pure call or one train step on the current stream, nothing else: no host synchronisation, results that live in engine-held
    tensors (records, a training state) cloned on the stream -> {name: device tensor | host value}"""
    import torch
    kind = call[0]
    if kind in S.STEPS:
        return enqueue_step(r, eng, call)
    if kind == S.REFUSE:
        rc, msg = refuse(r, eng, call[1])
        want = S.REFUSALS[call[1]]
        assert rc == want[0] and want[1] in msg, "%r: status %d (%r), the documented refusal is status %d with %r" % (call, rc, msg, want[0], want[1])
        return {"status": np.array([rc], np.int32)}
    lo, n = call[1], call[2]
    if kind in ("forward", "forward_u8", "forward_timed"):
        x = r.images(lo, n, kind == "forward_u8")
        # an output tensor of 0xFF (NaN): a row the pass does not write must not show up as what the allocator's recycled block held --
        # the right logits of an earlier call, more often than not
        out = poisoned_out(eng, n)
        getattr(eng, kind)(x, out=out)      # (forward_timed synchronises inside the library: it reads its events)
        return {"logits": out}
    if kind in S.DETECT:
        method, thr, mode = S.DETECT[kind]
        if method == "detect_frames":
            got = eng.detect_frames([r.frames[i % S.N_IMAGES] for i in range(lo, lo + n)], thr, S.IOU, mode, _hip.RESIZE_LETTERBOX)
        else:
            got = getattr(eng, method)(r.images(lo, n, method == "detect_u8"), thr, S.IOU, mode)
        return dict(zip(("boxes", "counts", "status"), (t.clone() for t in got)))
    if kind in ("loss", "loss_u8"):
        images, result = getattr(eng, kind)(r.images(lo, n, kind == "loss_u8"), r.gts(lo, n))
        return {"images": images, "result": result}
    if kind == "loss_grad":
        return dict(zip(("images", "result", "assign", "grad"), eng.loss_grad(r.images(lo, n), r.gts(lo, n))))
    if kind in ("loss_v3", "loss_v3_u8"):
        return dict(zip(("images", "result", "assign"), getattr(eng, kind)(r.images(lo, n, kind == "loss_v3_u8"), r.gts(lo, n), S.IGNORE_THRESH)))
    if kind == "loss_v3_grad":
        return dict(zip(("images", "result", "assign", "grad"), eng.loss_v3_grad(r.images(lo, n), r.gts(lo, n), S.IGNORE_THRESH)))
    raise ValueError(call)


def state_slices(eng, family):
    """{name: (the engine's state tensor of the family, byte offset, bytes)} of the parts of a training state that a step is compared on"""
    if family == "head":
        lay = eng.train_layout
        nw, nb = lay.cout * lay.cin * 4, lay.cout * 4
        return {k: (eng._train_state, int(getattr(lay, k + "_offset")), n) for k, n in zip(STATE_KEYS, (nw, nb, nw, nw, nb, nb))}
    if family == "v3":
        lay = eng.train_layout_v3
        out = {}
        for s in range(lay.n_scales):
            nw, nb = lay.cout[s] * lay.cin[s] * 4, lay.cout[s] * 4
            for k, n in zip(V3_STATE_KEYS, (nw, nb, nw, nw, nb, nb, nw, nb)):
                out["%s[%d]" % (k, s)] = (eng._train_state_v3, int(getattr(lay, k + "_offset")[s]), n)
        return out
    if family == "blocks":      # per scale the head conv's eight arrays and the block's eight: TAIL_PARTS, `w3[1]` the block's master kernel of scale 1
        lay = eng.blocks_layout_v3
        out = {}
        for s in range(lay.n_scales):
            nw, nb, nw3, nb3 = lay.cout[s] * lay.cin[s] * 4, lay.cout[s] * 4, lay.cout3[s] * 9 * lay.cin3[s] * 4, lay.cout3[s] * 4
            for k, n in zip(TAIL_PARTS, (nw, nb, nw, nw, nb, nb, nw, nb, nw3, nb3, nw3, nw3, nb3, nb3, nw3, nb3)):
                out["%s[%d]" % (k, s)] = (eng._blocks_state_v3, int(getattr(lay, k + "_offset")[s]), n)
        return out
    assert family == "tail", family
    lay = eng.tail_layout
    nw, nb, nw3, nb3 = lay.cout * lay.cin * 4, lay.cout * 4, lay.cout3 * 9 * lay.cin3 * 4, lay.cout3 * 4
    return {k: (eng._tail_state, int(getattr(lay, k + "_offset")), n) for k, n in zip(TAIL_PARTS, (nw, nb, nw, nw, nb, nb, nw, nb, nw3, nb3, nw3, nw3, nb3, nb3, nw3, nb3))}


def enqueue_step(r, eng, call):
    """a train step of any family into a result tensor of the test's, and clones of the state's parts behind it on the stream"""
    import torch
    kind, lo, n, t = call
    family, u8 = S.STEPS[kind], kind.endswith("_u8")
    x, gts, lr_t = r.images(lo, n, u8), r.gts(lo, n), engine.adam_lr_t(S.step_lr(kind), t)
    result = torch.full((yeval.LOSS_RESULT_DTYPE.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
    if family == "head":
        (eng.train_head_step_u8 if u8 else eng.train_head_step)(x, gts, lr_t, result=result)
    elif family == "v3":
        (eng.train_head_step_v3_u8 if u8 else eng.train_head_step_v3)(x, gts, lr_t, S.IGNORE_THRESH, result=result)
    elif family == "blocks":
        (eng.train_blocks_step_v3_u8 if u8 else eng.train_blocks_step_v3)(x, gts, lr_t, S.IGNORE_THRESH, result=result)
    else:
        (eng.train_tail_step_u8 if u8 else eng.train_tail_step)(x, gts, lr_t, result=result)
    res = {"result": result}
    for k, (state, at, nbytes) in state_slices(eng, family).items():
        part = state[at:at + nbytes].clone()
        res[k] = part if family == "head" else part.view(torch.float32)     # (the head family's parts stay the bytes they have always been here)
    return res


def named_fields(raw, dtype):
    """the bytes of a record array without its trailing pad word, which is nobody's output"""
    rec = np.ascontiguousarray(raw).view(dtype)
    return np.concatenate([np.ascontiguousarray(rec[k]).view(np.uint8).reshape(-1) for k in dtype.names if k != "pad_"])


def to_host(res):
    out = {}
    for k, v in res.items():
        a = v if isinstance(v, np.ndarray) else v.cpu().numpy()
        if k == "images":
            a = named_fields(a, yeval.LOSS_IMAGE_DTYPE)
        elif k == "result":
            a = named_fields(a, yeval.LOSS_RESULT_DTYPE)
        out[k] = a
    return out


def issue(r, eng, call):
    """a call of either kind, as the engine issues it -> enqueue's device results, None for a changing call that returns nothing (the inits
    and load_weights are synchronous by nature: the library waits for the device before it copies)"""
    kind = call[0]
    if S.builds_twin(call):
        return enqueue(r, eng, call)
    if kind == "head_train_init":
        eng.head_train_init(*r.head)
    elif kind == "tail_train_init":
        eng.tail_train_init(*r.tail)
    elif kind == "head_train_v3_init":
        eng.head_train_init_v3(*r.heads_v3)
    elif kind == "blocks_train_v3_init":
        eng.blocks_train_init_v3(*r.blocks_v3)
    elif kind == "set_wgrad_f16":       # (on: a new buffer of the engine's, no synchronisation; off waits for the device inside the engine)
        eng.set_wgrad_f16(call[1])
        assert (eng._wgrad_f16_buf is not None) == call[1]
    elif kind == "poison_extra":        # 0xFF into the buffer the fp16 weight gradient runs in: slabs, the m / k record, the partial sums of db
        assert getattr(eng, "_wgrad_f16_buf", None) is not None, "poison_extra outside the mode"
        eng._wgrad_f16_buf.fill_(0xFF)
    elif kind == "load_weights":
        eng.load_weights(r.weights)
    elif kind == "rebind":
        poison_and_bind(eng, "ones")
    elif kind == "set_streams":
        _hip.check(eng.lib.yolo_net_set_streams(eng.handle, call[1]), "yolo_net_set_streams")
        assert eng.num_streams == call[1]
    else:
        raise ValueError(call)
    return None


def execute(r, eng, call, fetch=True):
    """a call of either kind, synchronously -> its result on the host, None for a changing call that returns nothing (fetch = False: for
    any call; the device has finished it all the same)"""
    import torch
    res = issue(r, eng, call)
    if res is None or not fetch:
        torch.cuda.synchronize()
        return None
    return to_host(res)


def done(eng):
    """close an engine whose sequence is over and let go of its memory (what is still open when the module ends: close_engines)"""
    eng.close()
    if eng in ENGINES:
        ENGINES.remove(eng)


def twin(sid, key, cache=True):
    """the result of key's call on a fresh engine that has executed only key's changing calls"""
    if cache and (sid, key) in TWINS:
        return TWINS[(sid, key)]
    import torch
    prefix, call = key
    r = rig(sid)
    eng = new_engine(sid, keep=False)
    try:
        for c in prefix:
            execute(r, eng, c, fetch=False)
        res = execute(r, eng, call)
        torch.cuda.synchronize()
    finally:
        eng.close()
    if cache:
        TWINS[(sid, key)] = res
        # the states of the tail steps are hundreds of megabytes each: over the budget the oldest LARGE results of other plans go
        large = [k for k, v in TWINS.items() if result_bytes(v) > LARGE_RESULT_BYTES]
        held = sum(result_bytes(TWINS[k]) for k in large)
        for old in [k for k in large if k[0] != sid]:
            if held <= TWIN_CACHE_BYTES:
                break
            held -= result_bytes(TWINS.pop(old))
    return res


def result_bytes(res):
    return sum(v.nbytes for v in res.values()) if res else 0


# ---- comparing -----------------------------------------------------------------------------------------------------------------------------
def first_difference(got, want):
    """None, or what differed first between two results of one call"""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    if "counts" in got:
        for k in ("counts", "status"):
            if not np.array_equal(got[k], want[k]):
                return "%s: %s against the twin's %s" % (k, got[k].tolist(), want[k].tolist())
        for i, n in enumerate(want["counts"]):
            a, b = got["boxes"][i, :n].view(np.uint32), want["boxes"][i, :n].view(np.uint32)
            if not np.array_equal(a, b):
                rec, col = (int(v) for v in np.argwhere(a != b)[0])
                return "image %d, record %d of %d, field %d: %r against the twin's %r" % (i, rec, n, col, got["boxes"][i, rec].tolist(), want["boxes"][i, rec].tolist())
        return None
    # of a training state the weight gradients come first, the block's in front of the head's, then the bias gradients: they are what
    # the step's kernels wrote from the forward, and the masters and moments behind them in the alphabet only follow them
    for k in sorted(want, key=lambda k: (0 if k.startswith("dw") else 1 if k.startswith("db") else 2, k)):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            return "%s: shape / type %s %s against the twin's %s %s" % (k, a.shape, a.dtype, b.shape, b.dtype)
        if a.tobytes() == b.tobytes():
            continue
        bits = {4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}[a.dtype.itemsize]
        bad = np.argwhere(a.view(bits) != b.view(bits))
        idx = tuple(int(v) for v in bad[0])
        where = "(image, row, column%s) = %s" % (", channel" if a.ndim == 4 else "", idx) if a.ndim >= 3 else "element %s" % (idx,)
        # (every array that differs, by name: the first in the alphabet is seldom the cause -- `beta` moves because `dbeta` did, `dw3` is the kernel's)
        others = [o for o in sorted(want) if o != k and np.ascontiguousarray(got[o]).tobytes() != np.ascontiguousarray(want[o]).tobytes()]
        return "%s: %d of %d elements differ, first at %s: %r against the twin's %r%s" % (
            k, len(bad), a.size, where, a[idx].item(), b[idx].item(), "; differing as well: " + ", ".join(others) if others else "")
    return None


def describe_failure(sid, name, seq, i, diff):
    ran = [c for c in seq[:i] if c[0] != S.REFUSE]          # (a refused call launches nothing: the suspect is the call in front of it)
    prev = ran[-1] if ran else None
    changing = [c for c in seq[:i] if S.is_changing(c)]
    return ("plan %s, sequence %s, call %d %r: the result differs from its twin's (a fresh engine that ran only %r and this call)\n  %s\n"
            "  the call in front of it: %r%s%s\n  the last changing call in front of it: %r"
            % (sid, name, i, seq[i], list(S.twin_key(seq, i)[0]), diff, prev,
               " (a SPARSE detect: head rows below the threshold's logit were not written)" if prev and S.is_sparse_detect(prev) else "",
               ", then the refused %r" % (seq[i - 1],) if i and seq[i - 1][0] == S.REFUSE else "", changing[-1] if changing else None))


def control(sid):
    """two fresh twins, the same call, the same bytes -- else what a sequence would show is non-determinism, not call order"""
    if sid not in CONTROL:
        CONTROL[sid] = None
        kinds = S.PLANS[sid]["kinds"]
        # (calls of the covering walk's own set, so that the cached twin of each serves the sequences as well)
        detect = min((k for k in kinds if k in S.DETECT and S.DETECT[k][0] == "detect"), key=lambda k: S.DETECT[k][1:])     # the lowest threshold
        first = next(iter(S.sequences_of(sid).values()))
        trains = sid in S.TRAINING_PLANS        # (the plans that came with the later training families and the fp16 mode)
        keys = [((), (k,) + S.variants(kinds, k)[0]) for k in ("forward", detect) + (("loss_v3",) if "loss_v3" in kinds else ())]
        if trains:
            at = 2 if sid in S.MODE else 1      # (a MODE plan sets the mode between the init and the step)
            assert first[0][0] in S.INITS and first[at][0] in S.STEPS and first[at][3] == 1 and (at == 1 or first[1] == S.SET_ON), first[:3]
            keys.append((tuple(first[:at]), first[at]))         # the first training step
        for key in keys:
            call = key[1]
            want = twin(sid, key)
            diff = first_difference(twin(sid, key, cache=False), want)
            if diff:
                CONTROL[sid] = "%r behind %r: %s" % (call, list(key[0]), diff)
                break
            # the fixture itself: finite, non-zero logits, and boxes to compare
            assert "counts" not in want or int(want["counts"].sum()) > 0, "plan %s: %r finds no box: the fixture detects nothing" % (sid, call)
            assert "logits" not in want or (np.isfinite(want["logits"]).all() and np.any(want["logits"] != 0)), (sid, call)
            if call[0] == "loss_v3":        # ... truth rows and ignored rows in the loss
                assert (want["assign"] >= 0).any() and (want["assign"] == -2).any(), (
                    "plan %s: %r at ignore_thresh %r assigns %d truth rows and ignores %d rows: the fixture leaves a branch of the loss unrun"
                    % (sid, call, S.IGNORE_THRESH, int((want["assign"] >= 0).sum()), int((want["assign"] == -2).sum())))
            if call[0] in S.STEPS:          # ... a weight gradient on every scale / layer, and a forward that sees the update
                grads = [k for k in want if k.startswith("dw")]
                assert grads or S.STEPS[call[0]] == "head", sorted(want)
                for k in grads:
                    assert np.isfinite(want[k]).all() and np.any(want[k] != 0), "plan %s: %r leaves %s zero or not finite: the fixture trains nothing there" % (sid, call, k)
                fwd = S.each_pure(sid, 0)[0]
                assert fwd[0] == "forward"
                trained, untrained = twin(sid, (key[0] + (call,), fwd)), twin(sid, ((), fwd))
                assert np.isfinite(trained["logits"]).all() and first_difference(trained, untrained) is not None, (
                    "plan %s: the forward behind %r equals the untrained twin's: the step changed nothing a forward sees" % (sid, call))
                if sid in S.MODE:       # ... and a mode that shows: the block's weight gradient with the mode on is not the one with it off
                    off = twin(sid, ((first[0],), call))
                    dw3 = [k for k in want if k.startswith("dw3")]
                    assert dw3 and any(want[k].tobytes() != off[k].tobytes() for k in dw3), (
                        "plan %s: %r leaves the same %s with the fp16 mode on and off: the mode sequences would test nothing" % (sid, call, dw3))
    if CONTROL[sid]:
        pytest.fail("plan %s: CONTROL failed -- two fresh engines, the same single call, different bytes.  This is non-determinism, not call "
                    "order; the plan's sequences are not run.  %s" % (sid, CONTROL[sid]))


def run_sequence(sid, name, seq, start=0, end=None):
    """the calls of seq[:end] on one engine, those from `start` on compared with their twins"""
    control(sid)
    r = rig(sid)
    eng = new_engine(sid)
    boxes = 0
    seq = seq[:end]
    for i, call in enumerate(seq):
        got = execute(r, eng, call, fetch=i >= start)      # (a part's calls in front of its start are another part's to compare)
        if got is None:
            continue
        diff = first_difference(got, twin(sid, S.twin_key(seq, i)))
        assert diff is None, describe_failure(sid, name, seq, i, diff)
        boxes += int(got["counts"].sum()) if "counts" in got else 0
    done(eng)
    print("%s/%s: calls %d .. %d equal to their twins (%d twins cached for the module), %d boxes" % (sid, name, start, len(seq) - 1, len(TWINS), boxes))


# ---- 1 - 6: one item per (plan, sequence, part) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid,name,part,start,end", S.ITEMS, ids=["%s/%s/%d" % it[:3] for it in S.ITEMS])
def test_sequence(sid, name, part, start, end):
    run_sequence(sid, name, S.sequences_of(sid)[name], start, end)


# ---- 8: two engines of different plans alive at once, calls interleaved on one stream --------------------------------------------------------
def test_two_engines_interleaved():
    for sid in S.PAIR:
        control(sid)
    engines = {sid: new_engine(sid) for sid in S.PAIR}
    for i, (sid, call) in enumerate(S.INTERLEAVED):
        got = execute(rig(sid), engines[sid], call)
        diff = first_difference(got, twin(sid, ((), call)))
        assert diff is None, "interleaved call %d, %r on plan %s, behind %r on the other engine: %s" % (i, call, sid, S.INTERLEAVED[i - 1] if i else None, diff)
    for eng in engines.values():
        done(eng)


def test_two_training_engines_interleaved():
    """a YOLOv2 tail and the YOLOv3 head convs training side by side: init, step, forward, step and pure calls of each, alternating on one
    stream; every result equals its twin's in the engine's OWN sequence (the other engine's calls are nobody's changing calls)"""
    run_interleaved_training(S.PAIR_TRAIN, S.INTERLEAVED_TRAIN)


def run_interleaved_training(pair, interleaved):
    own = {sid: [c for s, c in interleaved if s == sid] for sid in pair}
    for sid in pair:
        control(sid)
    engines = {sid: new_engine(sid) for sid in pair}
    at = dict.fromkeys(pair, 0)
    for i, (sid, call) in enumerate(interleaved):
        got = execute(rig(sid), engines[sid], call)
        at[sid] += 1
        if got is None:
            continue
        diff = first_difference(got, twin(sid, S.twin_key(own[sid], at[sid] - 1)))
        assert diff is None, "interleaved call %d, %r on plan %s, behind %r on the other engine: %s" % (i, call, sid, interleaved[i - 1] if i else None, diff)
    for eng in engines.values():
        done(eng)


def test_two_engines_training_in_the_fp16_mode_interleaved():
    """the blocks of YOLOv3-tiny and a tiny-YOLOv2 tail training side by side, both in the fp16 mode, each in a buffer of its own: init,
    set(on), step, every pure kind, 0xFF into the engine's OWN buffer, second step, alternating on one stream -- the other engine's
    weight gradient ran in between each step's and the next, and every result equals its twin's in the engine's own `mode` sequence"""
    run_interleaved_training(S.PAIR_MODE, S.INTERLEAVED_MODE)


# ---- 3f: what must leave the mode alone, compared ACROSS twin keys -------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", S.MODE)
def test_an_init_and_a_rebind_leave_the_mode_on(sid):
    """A sequence whose twin replays the same init behind the same set(on) passes with an init that clears the mode: both run float32
    steps.  So here two DIFFERENT prefixes are compared (sequence_cases.MODE_SURVIVES): the first step behind [set(on), init] equals the
    one behind [init, set(on)], byte for byte, and differs in dw3 from the one with no set -- an init that cleared the mode would make
    the first pair differ; head_train_init between set(on) and a tail step changes nothing; and behind a re-bind onto 0xFF the step's
    dw3 still differs from the one of the same prefix without set(on)."""
    control(sid)
    table = S.MODE_SURVIVES[sid]
    for a, b in table["equal"]:
        diff = first_difference(twin(sid, a), twin(sid, b))
        assert diff is None, "plan %s: %r behind %r differs from the same step behind %r -- the mode did not survive, or more than the mode moved: %s" % (
            sid, a[1], list(a[0]), list(b[0]), diff)
    behind_init = table["equal"][0][1]      # [set(on), init]: against [init], the control's mode-off first step
    for a, b in table["differ"] + [(behind_init, off_key(behind_init))]:
        got, want = twin(sid, a), twin(sid, b)
        dw3 = [k for k in got if k.startswith("dw3")]
        assert dw3 and any(got[k].tobytes() != want[k].tobytes() for k in dw3), (
            "plan %s: %r behind %r leaves the dw3 of the same step behind %r: the mode is off there" % (sid, a[1], list(a[0]), list(b[0])))


def off_key(key):
    """the key without its set(on)"""
    return tuple(c for c in key[0] if c != S.SET_ON), key[1]


# ---- 9: the covering walk without host synchronisation between the calls -----------------------------------------------------------------------
@pytest.mark.parametrize("sid", [s for s in S.ASYNC_PLANS if "cover" in S.SEQUENCES[s]])
def test_covering_walk_enqueued_without_synchronisation(sid):
    """every call of the walk is only enqueued (inputs, truths and frames are on the device already; results that live in the engine's
    record buffer are cloned on the stream); ONE synchronisation at the end, then every result is compared.  forward_timed is the
    exception by its nature: it reads its own events and so waits for the stream inside the library."""
    import torch
    control(sid)
    seq = S.SEQUENCES[sid]["cover"]
    r = rig(sid)
    eng = new_engine(sid)
    torch.cuda.synchronize()
    pending = [enqueue(r, eng, call) for call in seq]
    torch.cuda.synchronize()
    for i, res in enumerate(pending):
        diff = first_difference(to_host(res), twin(sid, S.twin_key(seq, i)))
        assert diff is None, "enqueued without synchronisation: " + describe_failure(sid, "cover", seq, i, diff)
    done(eng)


@pytest.mark.parametrize("sid", [s for s in S.ASYNC_PLANS if "train-2" in S.SEQUENCES[s]])
def test_train_2_enqueued_without_synchronisation(sid):
    """init (synchronous by nature), step, forward, step, every pure kind: the steps write their records into tensors of the test's, the
    parts of the training state are cloned on the stream behind each step; ONE synchronisation at the end, then every result is compared.
    Each step's forward, loss, weight gradient and update are ordered against the calls around them by the stream alone."""
    import torch
    control(sid)
    seq = S.SEQUENCES[sid]["train-2"]
    r = rig(sid)
    eng = new_engine(sid)
    torch.cuda.synchronize()
    pending = [issue(r, eng, call) for call in seq]
    torch.cuda.synchronize()
    assert sum(c[0] in S.STEPS for c in seq) == 2 and all((res is None) == (not S.builds_twin(c)) for c, res in zip(seq, pending))
    for i, res in enumerate(pending):
        if res is not None:
            diff = first_difference(to_host(res), twin(sid, S.twin_key(seq, i)))
            assert diff is None, "enqueued without synchronisation: " + describe_failure(sid, "train-2", seq, i, diff)
    done(eng)


# ---- the harness itself: a flipped bit of a training state is found and named ------------------------------------------------------------------
def test_a_flipped_bit_of_the_first_moment_is_found_and_named():
    """Nothing in the library is mutated.  Behind a correct train_v3 step on a sequence engine, one bit of one word of m_w of scale 1 is
    flipped in the engine's state tensor: the next step's comparison must fail and name m_w of that scale; with the state and the packed
    weights as they were in front of that step and the bit flipped back, the comparison passes again."""
    flip_a_bit_of_the_state("v3-tiny-fp32-train", "v3", "m_w[1]")


def test_a_flipped_bit_of_a_block_s_first_moment_is_found_and_named():
    """the same for the fourth family: one bit of m_w3 of scale 1, the first moment of the kernel of the block behind the second head conv,
    in the blocks state of a YOLOv3-tiny engine -- found by the next blocks step's comparison and named, gone with the bit flipped back"""
    flip_a_bit_of_the_state("v3-tiny-fp16-blocks", "blocks", "m_w3[1]")


def flip_a_bit_of_the_state(sid, family, part):
    import torch
    control(sid)
    seq = S.SEQUENCES[sid]["train-2"]
    steps = [i for i, c in enumerate(seq) if c[0] in S.STEPS]
    r = rig(sid)
    eng = new_engine(sid)
    for i in range(steps[1]):
        got = execute(r, eng, seq[i])
        assert got is None or first_difference(got, twin(sid, S.twin_key(seq, i))) is None, describe_failure(sid, "train-2", seq, i, "before the flip")
    state, at, nbytes = state_slices(eng, family)[part]
    words = state[at:at + nbytes].view(torch.int32)
    word = int(torch.nonzero(words)[0])             # a moment the first step moved
    flip = lambda: words[word:word + 1].bitwise_xor_(1 << 22)       # the top bit of the mantissa
    flip()
    kept_state, kept_weights = state.clone(), eng._weights.clone()
    want = twin(sid, S.twin_key(seq, steps[1]))
    diff = first_difference(execute(r, eng, seq[steps[1]]), want)
    assert diff is not None and diff.startswith(part + ": "), "a flipped bit of %s (word %d) in front of %r was not found, or not named: %r" % (part, word, seq[steps[1]], diff)
    state.copy_(kept_state)
    eng._weights.copy_(kept_weights)
    flip()
    diff = first_difference(execute(r, eng, seq[steps[1]]), want)
    assert diff is None, "with the bit flipped back: " + describe_failure(sid, "train-2", seq, steps[1], diff)
    done(eng)


# ---- 7: exact chains through autotune and tune_streams -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(S.EXACT_CHAINS))
def test_exact_chain_through_autotune_and_tune_streams(cid):
    """autotune and tune_streams decide by timing, so two twins may end up with different tiles: on integer data every tile and every
    split must give the integer reference, which is what each forward of the chain is compared with"""
    import torch
    spec = S.EXACT_CHAINS[cid]
    c = dict(E.CASES[E.IDS.index(cid)], B=S.EXACT_BATCH)
    variant = spec["variant"]
    L, d, want, kept, rep = E.reference(c, variant)             # (asserts exact_ref's preconditions for this batch)
    x8 = (np.random.RandomState(7).randint(0, 2, size=d["x"].shape) * 255).astype(np.uint8)
    want8 = X.check_preconditions(L, dict(d, x=(x8 / 255.).astype(np.float32)), c["dtype"], keep=set())["out"]
    assert np.array_equal((x8 / 255.).astype(np.float32), (x8 > 0).astype(np.float32))
    eng = engine.HipNetwork(E.build_graph(c, variant), dtype=c["dtype"], max_batch=S.EXACT_BATCH)
    ENGINES.append(eng)
    eng.load_weights(d["stream"])
    names, text = E.kernel_text(eng, eng.kernel_infos())
    assert spec["feature"] in text, (cid, names)
    xd = torch.from_numpy(d["x"]).cuda()
    for i, (kind, lo, n) in enumerate(S.EXACT_STEPS):
        what = "%s step %d %s at batch %d (kernels now: %s)" % (cid, i, kind, n, [ki.name.decode() for ki in eng.kernel_infos()])
        if kind == "autotune":
            eng.autotune(xd[lo:lo + n])
        elif kind == "tune_streams":
            _hip.check(eng.lib.yolo_net_tune_streams(eng.handle, xd[lo:lo + n].data_ptr(), n, eng._stream()), "yolo_net_tune_streams")
        elif kind == "forward_u8":
            E.assert_equal(eng.forward_u8(x8[lo:lo + n]).cpu().numpy(), want8[lo:lo + n], what)
        else:
            E.assert_equal(eng.forward(xd[lo:lo + n]).cpu().numpy(), want[lo:lo + n], what)
    done(eng)

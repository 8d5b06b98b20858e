"""Shared test helpers: bridge between the product's layer objects and the oracle's tuples."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tensorflow_yolo_amd  # noqa: E402,F401  (shim -> tensorflow-yolo_amd/)
from tensorflow_yolo_amd.net import engine, layers as PL, synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def to_oracle(net):
    """Product layer objects -> oracle/topology tuples (same indices)."""
    engine.number_layers(net)
    out = []
    for l in net:
        src = [s.index for s in l.inputs]
        if isinstance(l, PL.input_layer):
            out.append(("input",) + tuple(l.out.hwc))
        elif isinstance(l, PL.conv2d_bn_act):
            out.append(("conv", src[0], l.filters, l.ksize, l.stride, l.batch_norm, l.activation))
        elif isinstance(l, PL.max_pool2d):
            out.append(("maxpool", src[0], l.ksize, l.stride))
        elif isinstance(l, PL.route):
            out.append(("route", src))
        elif isinstance(l, PL.reorg):
            out.append(("reorg", src[0], l.stride))
        elif isinstance(l, PL.shortcut):
            out.append(("shortcut", src[0], src[1]))
        elif isinstance(l, PL.upsample):
            out.append(("upsample", src[0], l.stride))
        elif isinstance(l, PL.yolo_layer):
            out.append(("yolo", src[0], [tuple(a) for a in l.anchors]))
        elif isinstance(l, PL.detection_layer):
            out.append(("detection", src))
        else:
            raise TypeError(l)
    return out


class Graph(list):
    """A free-form layer list for operator tests."""
    engine = None
    darknet_weights = None


def new_graph(h, w, c):
    PL.conv2d_bn_act.reset()
    g = Graph()
    g.append(PL.input_layer([None, h, w, c]))
    return g


def run_hip(net, weights, x, dtype, keep_all=False, max_batch=None, force_tile=None, **engine_kw):
    eng = engine.HipNetwork(net, dtype=dtype, max_batch=max_batch or x.shape[0], keep_all=keep_all, force_tile=force_tile, **engine_kw)
    eng.load_weights(weights)
    out = eng.forward(x).cpu().numpy()
    return out, eng


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-6, float(np.max(np.abs(b)))))


def match_boxes(got, want, atol_xy=2e-5, atol_p=2e-6):
    """got/want: lists of (x,y,w,h,cls,prob) in output order.  Exact order, class and count; coordinates/prob to float32
    rounding.  Order: up to boxes whose scores tie within 4 float32 ulps -- the reference's score is float32 arithmetic on
    NumPy's float32 exp (net/base.py:171-172), a few ulp accurate and not the same function as the GPU's expf, so two rows
    whose exact scores are closer than that may be sorted either way (oracle/parity.py: kTieUlps).  A non-finite value
    (an infinite box: expf overflow) matches only its exact equal."""
    assert len(got) == len(want), "count %d vs %d" % (len(got), len(want))

    def close(g, w, atol):
        if not (np.isfinite(g) and np.isfinite(w)):
            return g == w
        return abs(g - w) <= atol

    def same(g, w):
        return (int(g[4]) == int(w[4]) and close(g[5], w[5], atol_p) and
                all(close(g[i], w[i], atol_xy * max(1.0, abs(w[i]))) for i in range(4)))

    tie = 4 * 2.0 ** -24
    used = [False] * len(want)
    for k, g in enumerate(got):
        if not used[k] and same(g, want[k]):
            used[k] = True
            continue
        lo = k
        while lo > 0 and abs(want[lo - 1][5] - want[lo][5]) <= tie:
            lo -= 1
        hi = k
        while hi + 1 < len(want) and abs(want[hi + 1][5] - want[hi][5]) <= tie:
            hi += 1
        j = next((j for j in range(lo, hi + 1) if not used[j] and same(g, want[j])), None)
        w = want[k]
        assert j is not None, "box %d: %r vs %r (no box of the tied-score run %d..%d matches)" % (k, tuple(g), tuple(w), lo, hi)
        used[j] = True


def guarded_run(net, w, x, dtype, tile=None, keep_all=True, detect=False, guard=4096):
    """Plan with `guard` never-used bytes behind every tensor, fill the WHOLE workspace with a pattern, run, and require every byte no
    plan region claims as payload to still hold the pattern: the slack + guard behind each tensor / candidate list / counter block /
    scratch slab (yolo_net_workspace_regions).  With keep_all no two tensors share bytes; without it (the fused production plan:
    lifetime-packed arenas) only slack that no other region's payload overlaps can be checked."""
    import torch
    from tensorflow_yolo_amd import _hip
    eng = engine.HipNetwork(net, dtype=dtype, max_batch=x.shape[0], keep_all=keep_all, force_tile=tile, guard_bytes=guard)
    eng.load_weights(w)
    ws = eng._workspace
    ws.fill_(0xA5)
    _hip.check(eng.lib.yolo_net_bind_workspace(eng.handle, ws.data_ptr(), ws.numel()), "yolo_net_bind_workspace")   # (zeroes the tickets)
    eng.forward(x)
    if detect:
        eng.detect(x, 0.3, 0.6)
    torch.cuda.synchronize()
    regions = eng.workspace_regions()
    payload = sorted((off, off + used) for _, off, used, _ in regions if used)
    checked = 0
    for name, off, used, region in regions:
        lo, hi = off + used, off + region
        if hi <= lo:
            continue
        # cut out what another region's payload covers (lifetime-packed arenas)
        spans, cur = [], lo
        for a, b in payload:
            if b <= cur or a >= hi:
                continue
            if a > cur:
                spans.append((cur, a))
            cur = max(cur, b)
            if cur >= hi:
                break
        if cur < hi:
            spans.append((cur, hi))
        for a, b in spans:
            bad = (ws[a:b] != 0xA5).nonzero()
            assert bad.numel() == 0, "%s (tile %s, %s): byte %d behind the payload of a %d-byte region was written\n%s" % (
                name, tile, dtype, int(bad[0]) + a - lo, used, eng.describe())
            checked += b - a
    assert checked >= guard, "nothing to check"
    return eng, checked


# ---- a poisoned workspace -----------------------------------------------------------------------------------------------------------
# INTEGRATION.md lets a C-ABI caller bind a workspace it never zeroed; engine.HipNetwork allocates torch.zeros, so without these helpers
# every test starts from zero bytes, where a kernel that reads what no kernel of the pass wrote gets 0 (or, later, stale FINITE data).
#   "ones": every byte 0xFF -- NaN as fp16, float32 and float64, -1 / 4 294 967 295 as any integer;
#   "inf":  +inf of the plan's storage type through a typed view -- 0x7C00 per 16 bits (fp16 and mxfp8 plans), 0x7F800000 per 32 bits
#           (fp32 plans).  On an fp16 plan the float32 regions then read 2.66e36: finite, but wrong wherever it is used.
# A NaN poisons every sum it enters and is dropped by max; +inf wins every max and turns sums into inf or NaN.
POISONS = ("ones", "inf")


def poison_fill(t, poison, f32_storage):
    """fill a device tensor of bytes with a poison pattern (the whole tensor: its size is a multiple of 4)"""
    import torch
    assert t.dtype == torch.uint8 and t.is_contiguous() and t.numel() % 4 == 0, (t.dtype, t.numel())
    if poison == "ones":
        t.fill_(0xFF)
    elif poison == "inf":
        if f32_storage:
            t.view(torch.int32).fill_(0x7F800000)
        else:
            t.view(torch.int16).fill_(0x7C00)
    else:
        raise ValueError(poison)


def poison_and_bind(eng, poison):
    """Fill the WHOLE workspace of an engine with the poison, the record buffer detect() writes (boxes, counts, status) with 0xFF, and bind
    the workspace again: the documented contract (bind after allocation; yolo_net_bind_workspace clears what the library counts on).
    The fills are complete before the bind, whose clears would otherwise be overwritten."""
    import torch
    from tensorflow_yolo_amd import _hip
    torch.cuda.synchronize()
    poison_fill(eng._workspace, poison, eng.dtype == _hip.DTYPE_F32)
    eng.records.fill_(-1)
    torch.cuda.synchronize()
    _hip.check(eng.lib.yolo_net_bind_workspace(eng.handle, eng._workspace.data_ptr(), eng._workspace.numel()), "yolo_net_bind_workspace")


def poisoned_out(eng, batch):
    """a caller's output tensor of `batch` images with every byte 0xFF (NaN): an element the pass does not write stays NaN"""
    import torch
    out = torch.empty((batch,) + tuple(eng.output_shape), dtype=torch.float32, device=eng.device)
    out.view(torch.int32).fill_(-1)
    return out


def forward_poisoned(eng, x, poison, u8=False):
    """poison + bind, then ONE forward of x into a poisoned output tensor -> the output on the host"""
    poison_and_bind(eng, poison)
    out = poisoned_out(eng, x.shape[0])
    (eng.forward_u8 if u8 else eng.forward)(x, out=out)
    return out.cpu().numpy()


def run_hip_poisoned(net, weights, x, dtype, poison, before_pass=None, **engine_kw):
    """run_hip on memory nobody zeroed: construct the engine, fill the weight buffer with 0xFF and load the weights, fill the whole workspace
    with the poison, bind, fill the output tensor with 0xFF, forward.  before_pass(eng): called between the bind and the pass (the
    sensitivity check of tests/test_gpu_poison.py reads every layer there).  Uses the engine's own buffers and the C ABI's bind only."""
    import torch
    engine_kw.setdefault("max_batch", x.shape[0])
    eng = engine.HipNetwork(net, dtype=dtype, **engine_kw)
    eng._weights.fill_(0xFF)
    torch.cuda.synchronize()
    eng.load_weights(weights)
    poison_and_bind(eng, poison)
    if before_pass is not None:
        before_pass(eng)
    out = poisoned_out(eng, x.shape[0])
    eng.forward(x, out=out)
    return out.cpu().numpy(), eng

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


# ---- tensors at and past the 2 GiB line (tests/large_cases.py, test_large_cpu.py, test_gpu_large.py) ---------------------------------------
# Where a planned tensor lies: yolo_net_describe prints every kernel with its views ("out=b1[252x266x128 ld128+0]": buffer 1, H x W x C,
# row pitch ld, first channel coff), yolo_net_workspace_regions the bytes of every buffer ("tensor 1 arena 0").  Both need no GPU.
_VIEW_RE = r"b(-?\d+)\[(\d+)x(\d+)x(\d+) ld(\d+)\+(\d+)( f32)?\]"


def plan_kernels(p):
    """the kernels of a Plan from its description -> [dict(kernel, kind, layer, in=view | None, out=view, text)], a view being
    dict(buf, h, w, c, ld, coff, f32); buf < 0: a caller's tensor"""
    import re
    out = []
    for line in p.describe().splitlines():
        m = re.match(r"\s*\[(\d+)\] (\w+) layer (\d+)", line)
        if not m:
            continue
        k = dict(kernel=int(m.group(1)), kind=m.group(2), layer=int(m.group(3)), text=line.strip())
        k["in"] = k["out"] = None
        for key in ("in", "out"):
            v = re.search(r"\b%s=%s" % (key, _VIEW_RE), line)
            if v:
                k[key] = dict(zip(("buf", "h", "w", "c", "ld", "coff"), (int(t) for t in v.groups()[:6])), f32=v.group(7) is not None)
        out.append(k)
    assert len(out) == p.num_kernels, (len(out), p.num_kernels)
    return out


def layer_view(p, layer):
    """the view a layer's values are stored in: the output view of the (last) kernel that writes for it"""
    ks = [k for k in plan_kernels(p) if k["layer"] == layer and k["out"] is not None and k["out"]["buf"] >= 0]
    assert ks, "layer %r has no kernel that writes it into the workspace in this plan\n%s" % (layer, p.describe())
    return ks[-1]["out"]


def buffer_region(p, buf, arena=0):
    """(offset, used bytes, region bytes) of a planned buffer in the workspace"""
    name = "tensor %d arena %d" % (buf, arena)
    found = [(off, used, region) for n, off, used, region in p.workspace_regions() if n == name]
    assert len(found) == 1, (name, found)
    return found[0]


def view_esize(p, view):
    from tensorflow_yolo_amd import _hip
    return 4 if view["f32"] or p.dtype == _hip.DTYPE_F32 else 2


def view_image_bytes(p, view):
    """S of a planned tensor: bytes from one image to the next (the WHOLE buffer's pitch where the view is a channel slice); every
    buffer of a plan is sized for max_batch images (per arena: plans of one part only)"""
    off, used, region = buffer_region(p, view["buf"])
    assert used % p.max_batch == 0, (used, p.max_batch)
    return used // p.max_batch


def buffer_is_alone(p, buf):
    """no other region's payload overlaps this buffer's (always so under keep_all; in a lifetime-packed plan only for some): only then do its
    bytes still hold after the pass what its kernel wrote"""
    off, used, _ = buffer_region(p, buf)
    name = "tensor %d arena 0" % buf
    return all(n == name or not u or o + u <= off or o >= off + used for n, o, u, _ in p.workspace_regions())


def layer_tensor(eng, layer, batch, side="out"):
    """a typed, strided view [batch, H, W, C] of a layer's values in the engine's workspace (no copy) and where it lies: dict(image_bytes,
    ld, coff, esize, w).  side = "in": what the layer's kernel READS instead (the whole concat buffer behind a route)"""
    import torch
    v = layer_view(eng, layer) if side == "out" else [k for k in plan_kernels(eng) if k["layer"] == layer][0]["in"]
    assert v["buf"] >= 0 and buffer_is_alone(eng, v["buf"]), "layer %d: no view possible\n%s" % (layer, eng.describe())
    off, used, _ = buffer_region(eng, v["buf"])
    es = view_esize(eng, v)
    isb = view_image_bytes(eng, v)
    assert isb % es == 0 and v["h"] * v["w"] * v["ld"] * es <= isb and v["coff"] + v["c"] <= v["ld"], (v, isb)
    t = eng._workspace[off:off + batch * isb].view(torch.float32 if es == 4 else torch.float16).view(batch, isb // es)
    t = t[:, :v["h"] * v["w"] * v["ld"]].view(batch, v["h"], v["w"], v["ld"])[..., v["coff"]:v["coff"] + v["c"]]
    return t, dict(image_bytes=isb, ld=v["ld"], coff=v["coff"], esize=es, w=v["w"])


def large_batch(x, batch):
    """distinct images [D, ...] (NumPy) -> the batch on the device by an index gather: image n is distinct image n mod D"""
    import torch
    xd = torch.tensor(np.asarray(x)).cuda()                 # (a copy: the reference's arrays are read-only)
    return xd[torch.arange(batch, device=xd.device) % xd.shape[0]]


LARGE_CHUNK = 1 << 25       # elements compared at a time: the comparison holds a few hundred MB beside the tensors


def large_difference(got, want):
    """got: a device tensor [B, H, W, C] of any strides; want: the D expected images as a NumPy float32 array [D, H, W, C].  Element (n, y, x, c)
    must equal want[n mod D, y, x, c] BIT for bit (compared as integers: a NaN that nothing overwrote differs, -0 differs from 0).  Runs on the device
    in chunks of whole images, over the whole tensor, torch.equal per chunk.  None when equal, else the FIRST differing element in
    memory order: dict(index=(n, y, x, c), got, want, differing = how many of its chunk differ, chunk = (first image, images))."""
    import torch
    assert got.dim() == 4 and tuple(got.shape[1:]) == tuple(want.shape[1:]), (tuple(got.shape), want.shape)
    D = want.shape[0]
    wd = torch.tensor(np.asarray(want, np.float32)).to(got.device)
    if got.dtype == torch.float16:
        w16 = wd.to(torch.float16)
        assert torch.equal(w16.to(torch.float32), wd), "the expected values are not fp16 values"
        wd = w16
    bits = torch.int16 if got.dtype == torch.float16 else torch.int32
    gi, wi = got.view(bits), wd.view(bits)
    per = int(np.prod(got.shape[1:]))
    step = max(1, LARGE_CHUNK // per)
    for n0 in range(0, got.shape[0], step):
        n1 = min(got.shape[0], n0 + step)
        e = wi[torch.arange(n0, n1, device=got.device) % D]
        g = gi[n0:n1]
        if torch.equal(g, e):
            continue
        ne = g != e
        flat = int(ne.view(-1).to(torch.int32).argmax())         # (the first maximum: the first differing element)
        n, y, x, c = (int(v) for v in np.unravel_index(flat, tuple(ne.shape)))
        return dict(index=(n0 + n, y, x, c), got=float(got[n0 + n, y, x, c]), want=float(want[(n0 + n) % D, y, x, c]),
                    differing=int(ne.sum()), chunk=(n0, n1 - n0))
    return None


def large_offset(index, where, shape):
    """byte offset of element (n, y, x, c) inside its tensor: from the first byte of the planned buffer (where = layer_tensor's dict), or of
    the caller's dense float32 tensor (where = None)"""
    n, y, x, c = index
    if where is None:
        return int(np.ravel_multi_index((n, y, x, c), shape)) * 4
    return n * where["image_bytes"] + ((y * where["w"] + x) * where["ld"] + where["coff"] + c) * where["esize"]


def large_report(diff, what, where, shape, kernel):
    """what a failed comparison says: the case and layer, the first differing element, its byte offset and which lines it is past, the kernel"""
    off = large_offset(diff["index"], where, shape)
    return ("%s: first difference at (image, y, x, channel) = %s: got %r, want %r; byte offset %d inside the tensor (%s 2^31, %s 2^32); %d of the "
            "elements of images %d..%d differ; written by kernel %s [%s]"
            % (what, diff["index"], diff["got"], diff["want"], off, "AT OR PAST" if off >= 1 << 31 else "below", "AT OR PAST" if off >= 1 << 32 else "below",
               diff["differing"], diff["chunk"][0], diff["chunk"][0] + diff["chunk"][1] - 1, kernel[0], kernel[1]))


def assert_large_equal(got, want, what, where, kernel):
    diff = large_difference(got, want)
    assert diff is None, large_report(diff, what, where, tuple(got.shape), kernel)


def kernel_of_layer(infos, layer):
    """(name, symbol) of the kernel that computes a layer, from yolo_net_kernel_info records: the first with a launch of its own (the
    conversion of the last layer to float32 comes behind it under the same layer)"""
    ks = [(ki.name.decode(), ki.symbol.decode()) for ki in infos if ki.layer == layer]
    assert ks, layer
    launched = [k for k in ks if k[1]]
    return (launched or ks)[0]


def assert_slack_intact(eng, value, what):
    """guarded_run's check for a workspace filled with `value` bytes: every byte no plan region claims as payload still holds it"""
    regions = eng.workspace_regions()
    payload = sorted((off, off + used) for _, off, used, _ in regions if used)
    checked = 0
    for name, off, used, region in regions:
        lo, hi = off + used, off + region
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
            bad = (eng._workspace[a:b] != value).nonzero()
            assert bad.numel() == 0, "%s: %s: byte %d behind the payload of a %d-byte region was written" % (what, name, int(bad[0]) + a - lo, used)
            checked += b - a
    return checked

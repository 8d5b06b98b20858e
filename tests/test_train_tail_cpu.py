"""CPU: the host side of the data gradient and the 3 x 3 weight gradient -- the yardstick of tests/tail_ref.py against torch.autograd,
yolo_conv3x3_wgrad_plan and the case table of tests/tail_cases.py against each other, every refusal that needs no device, the layout
round trip of the block's kernel, and the sanitizer run of the host code as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tail_cases
import tail_ref
from helpers import ROOT, new_graph
from oracle import cases
from tensorflow_yolo_amd import _hip, launcher
from tensorflow_yolo_amd.net import engine, layers as PL, train as ytrain, v2, v3


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def _block(seed, B, h, w, cin, cmid, cout):
    """random parameters and inputs of the block and the head with no pre-activation within 1e-6 of 0"""
    rng = np.random.RandomState(seed)
    X3 = rng.randn(B, h, w, cin)
    W3 = rng.randn(cmid, 9, cin) / np.sqrt(9 * cin)
    scale = rng.uniform(0.5, 2.0, size=cmid) * rng.choice([-1.0, 1.0], size=cmid)
    bias = rng.randn(cmid) * 0.1
    W = rng.randn(cout, cmid) / np.sqrt(cmid)
    b = rng.randn(cout) * 0.1
    G = rng.randn(B * h * w, cout)
    z, Y, L = tail_ref.tail_forward(X3, W3, scale, bias, W, b)
    assert np.min(np.abs(z)) > 1e-6, "an input on the kink of the leaky ReLU: the slope branch could differ"
    return X3, W3, scale, bias, W, b, G, Y


@pytest.mark.parametrize("shape", [(1, 1, 1, 8, 8, 1), (2, 3, 5, 8, 16, 30), (3, 5, 7, 16, 24, 10), (2, 13, 13, 8, 16, 6)])
def test_float64_yardstick_equals_autograd(shape):
    """conv2d + affine + leaky_relu + 1 x 1 conv2d in float64 under torch.autograd, loss = sum(L * G) so that dloss / dL = G.  Bound, set
    before anything here ran: 1e-12 of the largest gradient of its kind, the margin of the Adam yardstick (test_train_cpu.py).  Measured:
    at most 1.6e-15 of the largest gradient (dbeta at 13 x 13, batch 2), on every shape and every gradient."""
    import torch
    import torch.nn.functional as F
    B, h, w, cin, cmid, cout = shape
    X3, W3, scale, bias, W, b, G, Y = _block(sum(shape), *shape)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    # W3 [o][t][c] -> torch's [out][in][kh][kw]; beta enters z as b' = beta - mean s, so dloss / dbeta = dloss / db'
    k3 = t(W3.reshape(cmid, 3, 3, cin).transpose(0, 3, 1, 2)).requires_grad_()
    bt, Wt, bh = t(bias).requires_grad_(), t(W).requires_grad_(), t(b).requires_grad_()
    x = t(X3.transpose(0, 3, 1, 2))
    u = F.conv2d(x, k3, padding=1)
    z = u * t(scale)[None, :, None, None] + bt[None, :, None, None]
    y = F.leaky_relu(z, tail_ref.SLOPE)
    y.retain_grad()
    L = F.conv2d(y, Wt[:, :, None, None], bias=bh)
    (L * t(G.reshape(B, h, w, cout).transpose(0, 3, 1, 2))).sum().backward()
    want = {"dW": Wt.grad.numpy(), "db": bh.grad.numpy(), "dbeta": bt.grad.numpy(),
            "dW3": k3.grad.numpy().transpose(0, 2, 3, 1).reshape(cmid, 9, cin),
            # autograd's dloss / dY, times the activation's derivative at the stored Y, is the D of the definition
            "D": (y.grad.numpy() * np.where(y.detach().numpy() > 0, 1.0, tail_ref.SLOPE)).transpose(0, 2, 3, 1).reshape(B * h * w, cmid)}
    got = tail_ref.tail_grads64(X3, Y, W, scale, G)
    for name in sorted(want):
        gap, top = float(np.max(np.abs(got[name] - want[name]))), float(np.max(np.abs(want[name])))
        print("shape %s %s: max|ref - autograd| = %.3e = %.3e of max|g| = %.6g" % (shape, name, gap, gap / top, top))
        assert gap <= 1e-12 * top, (shape, name)


def test_float32_mode_is_sequential_and_close_to_float64():
    """the float32 mode of the yardstick rounds every operation to float32 and stays inside the bound the header states"""
    rng = np.random.RandomState(3)
    X3, D = rng.randn(2, 5, 7, 8), rng.randn(70, 6)
    scale = rng.uniform(0.5, 2.0, size=6)
    r32, b32 = tail_ref.wgrad3x3(X3.astype(np.float32), D.astype(np.float32), scale.astype(np.float32), mode="float32")
    r64, b64, bound_w, bound_b = tail_ref.wgrad3x3_ref64(X3.astype(np.float32), D.astype(np.float32), scale.astype(np.float32))
    assert r32.dtype == np.float32 and np.all(np.abs(r32 - r64) <= bound_w) and np.all(np.abs(b32 - b64) <= bound_b)
    s64, _ = tail_ref.wgrad3x3(X3, D, scale, mode="float64")
    assert np.max(np.abs(s64 - tail_ref.wgrad3x3_ref64(X3, D, scale)[0])) <= 1e-12 * np.max(np.abs(s64))
    G, W, Y = rng.randn(9, 5), rng.randn(5, 8), rng.randn(9, 8)
    d32, d64 = tail_ref.dgrad(G, W, Y, mode="float32"), tail_ref.dgrad(G, W, Y, mode="float64")
    assert d32.dtype == np.float32 and np.max(np.abs(d32 - d64)) <= 8 * 2.0 ** -24 * np.max(np.abs(G) @ np.abs(W))


def test_slope_branch_is_decided_by_the_stored_value():
    G, W = np.ones((1, 1)), np.ones((1, 8))
    Y = np.array([[0.0, -0.0, -1.0, 1.0, np.nan, 6e-8, -6e-8, np.inf]])
    want = np.array([[0.1, 0.1, 0.1, 1.0, 0.1, 1.0, 0.1, 1.0]], dtype=np.float32)
    assert np.array_equal(tail_ref.dgrad(G, W, Y, mode="float32"), want)
    assert np.array_equal(tail_ref.dgrad(G, W, None, mode="float32"), np.ones((1, 8), dtype=np.float32))


def test_taps_are_zero_outside_the_image_and_never_cross_rows_or_images():
    X3 = np.arange(1, 2 * 2 * 3 + 1, dtype=np.float64).reshape(2, 2, 3, 1)      # 1 .. 12, nothing is 0
    T = tail_ref.taps(X3)[:, :, 0]
    assert T.shape == (12, 9) and np.array_equal(T[:, 4], np.arange(1, 13))
    assert np.array_equal(T[2], [0, 0, 0, 2, 3, 0, 5, 6, 0])                  # the end of row 0: no tap reads the start of row 1
    assert np.array_equal(T[5], [2, 3, 0, 5, 6, 0, 0, 0, 0])                  # the last position of image 0: nothing of image 1
    assert np.array_equal(T[6], [0, 0, 0, 0, 7, 8, 0, 10, 11])                # the first position of image 1: nothing of image 0


def test_kernel_layout_round_trip():
    """the Darknet stream's [out][in][kh][kw] <-> [o][t = 3 ky + kx][c], the K order of the packed rows (weights.cpp: pack_weights)"""
    cout, cin = 5, 8
    stream = np.arange(cout * cin * 9, dtype=np.float32)
    otc = tail_ref.stream_to_otc(stream, cout, cin)
    assert otc.shape == (cout, 9, cin)
    for o, c, ky, kx in ((0, 0, 0, 0), (1, 2, 0, 1), (4, 7, 2, 2), (3, 5, 1, 0)):
        assert otc[o, 3 * ky + kx, c] == stream[((o * cin + c) * 3 + ky) * 3 + kx]
    assert np.array_equal(tail_ref.otc_to_stream(otc), stream)


# ---- yolo_conv3x3_wgrad_plan and the case table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [_hip.DTYPE_F16, _hip.DTYPE_F32])
def test_plan_properties_for_every_shape_of_the_case_table(dtype):
    shapes = tail_cases.wgrad_shapes()
    assert {s[:2] for s in shapes} == set(tail_cases.WGRAD_HW) and {s[2] for s in shapes} == set(tail_cases.WGRAD_BATCHES)
    assert {s[3] for s in shapes} == set(tail_cases.WGRAD_CINS) and {s[4] for s in shapes} == set(tail_cases.WGRAD_COUTS)
    for hw in tail_cases.WGRAD_HW:          # every map size with every batch
        assert {s[2] for s in shapes if s[:2] == hw} == set(tail_cases.WGRAD_BATCHES)
    for h, w, b, cin, cout in shapes:
        pl = _hip.conv3x3_wgrad_plan(h, w, b, cin, cout, dtype)
        P = h * w * b
        assert (pl["tile_cout"], pl["tile_cin"], pl["tile_positions"]) == (64, 64, 32)
        assert pl["tiles_cout"] == -(-cout // 64) and pl["tiles_cin"] == -(-cin // 64)
        ppc = pl["positions_per_chunk"]
        assert ppc % pl["tile_positions"] == 0
        # the chunks [k * ppc, min(P, (k + 1) * ppc)) cover [0, P) exactly once and none is empty
        chunks = [(k * ppc, min(P, (k + 1) * ppc)) for k in range(pl["n_chunks"])]
        assert chunks[0][0] == 0 and chunks[-1][1] == P and all(a < e for a, e in chunks)
        assert all(chunks[k][1] == chunks[k + 1][0] for k in range(len(chunks) - 1))
        assert pl["halo_rows"] == pl["tile_positions"] + 2 * w + 2
        assert pl["scratch_bytes"] == pl["n_chunks"] * cout * (9 * cin + 1) * 4
        assert P <= 4096 and 64 * P < 2 ** 24          # |values| <= 8: every sum of the exact tests is an integer below 2^24


def test_case_table_really_crosses_chunk_tile_and_image_boundaries():
    """a changed split must fail here, not silently shrink what the GPU tests cover"""
    h, w, b = tail_cases.CHUNK_CASE
    for cin in tail_cases.WGRAD_CINS:
        for cout in tail_cases.WGRAD_COUTS:
            assert (h, w, b, cin, cout) in tail_cases.wgrad_shapes()
            pl = _hip.conv3x3_wgrad_plan(h, w, b, cin, cout)
            P, ppc = h * w * b, pl["positions_per_chunk"]
            assert pl["n_chunks"] >= 3 and P % ppc != 0                              # three chunks or more, the last one partial
            ends = [k * ppc for k in range(1, pl["n_chunks"])]
            assert any(e % (h * w) % w != 0 for e in ends)                           # a chunk boundary inside an image row
            assert any(e < h * w < e + ppc for e in [0] + ends)                      # an image boundary inside a chunk
    # tile boundaries: a partial cin tile, a cout tile of one row, several tiles of both
    assert 136 in tail_cases.WGRAD_CINS and 65 in tail_cases.WGRAD_COUTS and 64 in tail_cases.WGRAD_COUTS
    plan = lambda h_, w_, b_: _hip.conv3x3_wgrad_plan(h_, w_, b_, 8, 1)
    sized = tail_cases.wgrad_plan_shapes(plan)
    assert [plan(h_, w_, b_)["n_chunks"] for h_, w_, b_, _ in sized] == [c for _, _, _, c in sized] == [1, 1, 2, 3]
    c = plan(1, 1, 1)["positions_per_chunk"]
    assert [h_ * w_ * b_ for h_, w_, b_, _ in sized] == [c - 1, c, c + 1, 2 * c + 5]
    # the dgrad table against its tile
    counts = [b_ * ppi for b_, ppi in tail_cases.DGRAD_POSITIONS]
    assert 1 in counts and 17 in counts and any(P > tail_cases.DGRAD_TILE_POSITIONS and P % tail_cases.DGRAD_TILE_POSITIONS for P in counts)


def test_plan_fills_the_chip_at_the_flagship_shape():
    """YOLOv2-416 at batch 16 and 64: the block is 1280 -> 1024 on 13 x 13"""
    for batch in (16, 64):
        pl = _hip.conv3x3_wgrad_plan(13, 13, batch, 1280, 1024)
        grid = pl["tiles_cout"] * pl["tiles_cin"] * pl["n_chunks"]
        assert 256 <= grid <= 1024 and pl["scratch_bytes"] <= 128 << 20, pl


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def last_error():
    return _hip.lib().yolo_last_error().decode()


def test_plan_refusals_have_messages():
    lib = _hip.lib()
    pl = _hip.Conv3x3WgradPlan()
    for args, text in (((0, 5, 1, 8, 1, _hip.DTYPE_F16), "at least 1"), ((5, 81, 1, 8, 1, _hip.DTYPE_F16), "does not fit LDS"),
                       ((5, 5, 1, 12, 1, _hip.DTYPE_F16), "multiple of 8"), ((5, 5, 1, 8, 0, _hip.DTYPE_F16), "cout must be at least 1"),
                       ((5, 5, 1, 8, 1, 7), "x_dtype"), ((1 << 20, 64, 32, 8, 1, _hip.DTYPE_F16), "2^30"),
                       ((5, 5, 1, 1 << 16, 1 << 16, _hip.DTYPE_F16), "31 bits")):
        assert lib.yolo_conv3x3_wgrad_plan(*args, C.byref(pl)) == 1 and text in last_error(), (args, last_error())
        assert last_error().startswith("yolo_conv3x3_wgrad_plan: ")
    assert lib.yolo_conv3x3_wgrad_plan(5, 5, 1, 8, 1, _hip.DTYPE_F16, None) == 1


def test_entry_refusals_need_no_device():
    """the checks run in front of any HIP call: host pointers stand in, nothing is launched"""
    lib = _hip.lib()
    buf = (C.c_float * 64)()
    q = C.addressof(buf) + (-C.addressof(buf)) % 16
    need = _hip.conv3x3_wgrad_plan(13, 13, 3, 40, 30)["scratch_bytes"]
    wg = lambda **kw: lib.yolo_conv3x3_wgrad(*[kw.get(k, v) for k, v in (("x", q), ("dt", _hip.DTYPE_F16), ("ld", 48), ("coff", 8), ("istride", 169 * 48), ("h", 13),
                                                                         ("w", 13), ("b", 3), ("cin", 40), ("d", q), ("cout", 30), ("scale", None), ("dw", q), ("db", q),
                                                                         ("scratch", q), ("bytes", need), ("stream", None))])
    for kw, text in (({"x": None}, "null"), ({"d": None}, "null"), ({"dw": None}, "null"), ({"db": None}, "null"), ({"scratch": None}, "null"),
                     ({"cin": 36}, "multiple of 8"), ({"ld": 40}, "inside the pixel stride"), ({"coff": -8}, "inside the pixel stride"),
                     ({"istride": 168 * 48}, "image_stride"), ({"bytes": need - 1}, "scratch too small"), ({"x": q + 1}, "aligned"),
                     ({"w": 81}, "LDS"), ({"dt": _hip.DTYPE_MXF8}, "x_dtype")):
        assert wg(**kw) == 1 and text in last_error(), (kw, last_error())
        assert last_error().startswith("yolo_conv3x3_wgrad: ")
    dg = lambda **kw: lib.yolo_conv1x1_dgrad(*[kw.get(k, v) for k, v in (("g", q), ("cout", 30), ("w", q), ("cin", 40), ("y", q), ("dt", _hip.DTYPE_F16), ("ld", 48),
                                                                         ("coff", 8), ("istride", 17 * 48), ("ppi", 17), ("b", 2), ("slope", 0.1), ("d", q),
                                                                         ("stream", None))])
    for kw, text in (({"g": None}, "null"), ({"w": None}, "null"), ({"d": None}, "null"), ({"cout": 0}, "cout must be at least 1"),
                     ({"cin": 36}, "multiple of 8"), ({"ppi": 0}, "at least 1"), ({"b": 0}, "at least 1"), ({"ppi": 1 << 20, "b": 1 << 11}, "2^30"),
                     ({"cout": 1 << 16, "cin": 1 << 16}, "31 bits"), ({"w": q + 4}, "16-byte"), ({"d": q + 8}, "16-byte"),
                     ({"ld": 40}, "inside the pixel stride"), ({"istride": 16 * 48}, "image_stride"), ({"dt": _hip.DTYPE_MXF8}, "dtype"),
                     ({"y": q + 1}, "aligned")):
        assert dg(**kw) == 1 and text in last_error(), (kw, last_error())
        assert last_error().startswith("yolo_conv1x1_dgrad: ")


# ---- the tail of a net: views, layout, refusals (host only) ---------------------------------------------------------------------------------
V2_ANCHORS = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071]
NAMES3 = ["a", "b", "c"]


def _plan(net, hw=None, **kw):
    p = engine.Plan(net, **kw)
    if hw:
        p.set_head(engine.head_desc_v2(hw[0], hw[1], np.reshape(V2_ANCHORS, [-1, 2]), len(NAMES3)))
    return p


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_tail_inputs_and_layout_of_the_v2_networks(dtype):
    anchors = np.reshape(V2_ANCHORS, [-1, 2])
    for make, shape, cin3, cmid in ((v2.create_full_network, (64, 64, 3), 1280, 1024), (v2.create_full_network, (96, 160, 3), 1280, 1024),
                                    (v2.create_tiny_network, (64, 64, 3), 1024, 1024), (tail_cases.small_tail_network, (64, 64, 3), 128, 128)):
        net = make(anchors, NAMES3, False, input_shape=shape)
        h, w, cout = net[-1].out.hwc
        p = _plan(net, (h, w), dtype=dtype, max_batch=3, streams=1)
        block_in, head_in = p.tail_inputs()
        want_dt = _hip.DTYPE_F16 if dtype == "fp16" else _hip.DTYPE_F32
        assert (block_in.cin, block_in.h, block_in.w, block_in.dtype) == (cin3, h, w, want_dt)
        assert (head_in.cin, head_in.h, head_in.w, head_in.dtype) == (cmid, h, w, want_dt)
        hv = p.head_input()
        assert (hv.offset, hv.image_stride, hv.ld, hv.coff) == (head_in.offset, head_in.image_stride, head_in.ld, head_in.coff)
        esz = 2 if dtype == "fp16" else 4
        for v in (block_in, head_in):       # inside the workspace, and the two tensors do not share a byte
            assert v.coff + v.cin <= v.ld and v.image_stride >= (h * w - 1) * v.ld + v.coff + v.cin
            assert v.offset + esz * 3 * v.image_stride <= p.workspace_bytes
        a0, a1 = block_in.offset, block_in.offset + esz * 3 * block_in.image_stride
        b0, b1 = head_in.offset, head_in.offset + esz * 3 * head_in.image_stride
        assert a1 <= b0 or b1 <= a0
        lay = p.tail_train_layout()
        assert (lay.cin, lay.cout, lay.cin3, lay.cout3) == (cmid, cout, cin3, cmid)
        cout3, cin3_, pos, n_block = ytrain.tail_counts(net)
        assert (cout3, cin3_) == (cmid, cin3) and lay.block_src == pos and lay.head_src == pos + n_block
        offs = [int(getattr(lay, n)) for n, _ in _hip.TailTrainLayout._fields_ if n.endswith("_offset")]
        assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and len(set(offs)) == len(offs)
        assert lay.total_bytes == p.lib.yolo_net_tail_train_bytes(p.handle) >= lay.scratch_offset + lay.scratch_bytes
        need = max(max(_hip.conv3x3_wgrad_plan(h, w, b, cin3, cmid, _hip.DTYPE_F32)["scratch_bytes"],
                       _hip.wgrad_plan(b * h * w, cmid, cout, _hip.DTYPE_F32)["scratch_bytes"]) for b in (1, 2, 3))
        assert lay.scratch_bytes == need
        assert lay.grad_offset - lay.d_offset >= 3 * h * w * cmid * 4


def test_tail_refusals_name_what_is_in_the_way():
    anchors = np.reshape(V2_ANCHORS, [-1, 2])
    lib = _hip.lib()
    views = (_hip.TensorView(), _hip.TensorView())
    call = lambda p: lib.yolo_net_tail_inputs(p.handle, C.byref(views[0]), C.byref(views[1]))
    # a v3 network: no detection layer at the end (YOLO_ERR_ARG)
    p = engine.Plan(v3.create_tiny_network(np.reshape(cases.COCO_V3_ANCHORS[:12], [-1, 2]), NAMES3, False, input_shape=(64, 64, 3)), dtype="fp16", max_batch=2, streams=1)
    assert call(p) == 1 and "a v3 network has no tail of this kind" in last_error() and "heads" in last_error()
    # an MXFP8 plan whose block is an MX conv (YOLO_ERR_STATE)
    full = v2.create_full_network(anchors, NAMES3, False, input_shape=(64, 64, 3))
    p = engine.Plan(full, dtype="mxfp8", max_batch=2, streams=1)
    assert call(p) == 5 and "MXFP8 conv" in last_error()
    assert lib.yolo_net_tail_train_bytes(p.handle) == 0 and "MXFP8 conv" in last_error()
    # two stream parts (YOLO_ERR_STATE)
    p = engine.Plan(full, dtype="fp16", max_batch=4, streams=2)
    assert call(p) == 5 and "stream parts" in last_error() and "yolo_net_set_streams(net, 1)" in last_error()
    # a hand-built layer list whose penultimate conv carries a residual (YOLO_ERR_ARG)
    p = engine.Plan(tail_cases.small_tail_network(anchors, NAMES3, False, residual=True), dtype="fp16", max_batch=2, streams=1)
    assert call(p) == 1 and "residual" in last_error(), last_error()
    # a 1 x 1 conv behind the detection layer; a block whose output passes a pool first
    g = new_graph(16, 16, 16)
    g.append(PL.conv2d_bn_act(g[-1].out, 32, 1, 1))
    g.append(PL.conv2d_bn_act(g[-1].out, 24, 1, 1, use_batch_normalization=False, activation_fn="linear"))
    assert call(engine.Plan(g, dtype="fp16", max_batch=2, streams=1)) == 1 and "3 x 3 / stride 1" in last_error()
    g = new_graph(16, 16, 16)
    g.append(PL.conv2d_bn_act(g[-1].out, 32, 3, 1))
    g.append(PL.max_pool2d(g[-1].out, 2, 2))
    g.append(PL.conv2d_bn_act(g[-1].out, 24, 1, 1, use_batch_normalization=False, activation_fn="linear"))
    assert call(engine.Plan(g, dtype="fp16", max_batch=2, streams=1)) != 0 and last_error().startswith("yolo_net_tail_inputs: ")
    # null arguments; the step entries check the net's tail before anything else, and a null state
    good = _plan(tail_cases.small_tail_network(anchors, NAMES3, False), (4, 4), dtype="fp16", max_batch=2, streams=1)
    assert lib.yolo_net_tail_inputs(good.handle, None, C.byref(views[1])) == 1 and lib.yolo_net_tail_inputs(None, C.byref(views[0]), C.byref(views[1])) == 1
    assert call(good) == 0
    for name in ("yolo_net_train_tail_step", "yolo_net_train_tail_step_u8"):
        fn = getattr(lib, name)
        assert fn(p.handle, 4096, 1, 4096, 4096, 1, 4096, 1e-3, 4096, None) == 1 and last_error().startswith(name + ": ") and "residual" in last_error()
        assert fn(good.handle, 4096, 1, 4096, 4096, 1, None, 1e-3, 4096, None) == 1 and "null state" in last_error()
        assert fn(good.handle, 4096, 1, 4096, 4096, 1, 4096 + 8, 1e-3, 4096, None) == 1 and "256-byte aligned" in last_error()
        assert fn(good.handle, 4096, 1, 4096, 4096, 1, 4096, 1e-3, 4096, None) == 5 and "weights not loaded" in last_error()
    assert lib.yolo_net_tail_train_init(good.handle, 4096, 1 << 30, 4096, 4096, 4096) == 5 and "weights not loaded" in last_error()
    assert lib.yolo_net_tail_train_init(good.handle, 4096, 16, 4096, 4096, 4096) == 1 and "state too small" in last_error()
    assert lib.yolo_net_tail_train_init(good.handle, None, 1 << 30, 4096, 4096, 4096) == 1


# ---- train mode: parsing, the shipped file, the stream --------------------------------------------------------------------------------------
def test_train_layers_tail_parsing_and_refusals(tmp_path):
    assert ytrain.train_layers({"train_layers": " Tail "}) == "tail" and ytrain.train_option({"train_layers": "tail"}) is True
    assert ytrain.train_layers({"train_layers": "head"}) == "head" and ytrain.train_layers({"train_layers": "heads"}) == "heads"       # as they were
    with pytest.raises(ValueError, match="^train_layers must be head "):
        ytrain.train_option({"train_layers": "tails"})
    for version in ("v2", "v2-tiny"):
        assert ytrain.check_params({"train_layers": "tail"}, version) == 0.0
    for version in ("v3", "v3-tiny", "v3-spp"):
        with pytest.raises(ValueError, match="takes train_layers = heads"):
            ytrain.check_params({"train_layers": "tail"}, version)
    with pytest.raises(ValueError, match="augment_probability must be 0"):
        ytrain.check_params({"train_layers": "tail", "augment_probability": "0.5"}, "v2")
    assert ytrain.check_params({"train_layers": "tail", "augment": "device", "augment_probability": "0.5"}, "v2") == 0.5
    ini = tmp_path / "cfg.ini"
    ini.write_text("[COMMON]\nversion = v3\n[TRAIN]\ntrain_layers = tail\naugment_probability = 0\n")
    with pytest.raises(ValueError, match="a v3 network takes train_layers = heads"):
        launcher.run(launcher.read_config(str(ini)), "train")


def test_shipped_tail_train_config():
    cfg = launcher.read_config(os.path.join(ROOT, "tensorflow-yolo_amd", "config", "yolo_2_tail_train.ini"))
    params = dict(cfg["TRAIN"])
    params.update(cfg["COMMON"])
    assert ytrain.train_layers(params) == "tail" and float(params["augment_probability"]) == 0 and params["version"] == "v2"
    ytrain.check_params(params, params["version"])
    for key in ("image_dir", "annotation_dir", "val_image_dir", "val_annotation_dir", "batch_size", "learning_rate", "epochs", "max_step",
                "checkpoint_dir", "checkpoint_step", "checkpoint_prefix", "pretrained_weights_path", "anchors", "class_names", "seed"):
        assert key in params, key


def test_stream_split_and_replace_of_the_tail():
    anchors = np.reshape(V2_ANCHORS, [-1, 2])
    net = tail_cases.small_tail_network(anchors, NAMES3, False)
    cout, cin, n_head, need = ytrain.head_counts(net)
    cout3, cin3, pos, n_block = ytrain.tail_counts(net)
    assert (cout3, cin3, n_block) == (128, 128, 128 * (4 + 9 * 128)) and pos + n_block + n_head == need
    body = np.arange(need, dtype=np.float32)
    block, w, b = ytrain.split_tail(body, net)
    assert block[0] == pos and block[-1] == pos + n_block - 1 and b[0] == pos + n_block and w[-1, -1] == need - 1
    # the block's kernel in the library's order and back
    otc = tail_ref.stream_to_otc(block[4 * cout3:], cout3, cin3)
    assert otc[2, 3 * 1 + 2, 5] == block[4 * cout3 + ((2 * cin3 + 5) * 3 + 1) * 3 + 2]
    k3 = tail_ref.otc_to_stream(otc).reshape(cout3, cin3, 3, 3)
    assert k3.tobytes() == block[4 * cout3:].tobytes()
    same = ytrain.replace_tail(body, net, k3, block[:cout3], w, b)
    assert same.tobytes() == body.tobytes() and same is not body
    new = ytrain.replace_tail(body, net, -k3, block[:cout3] + 0.5, w * 2, b - 1)
    changed = np.flatnonzero(new != body)
    # beta, the kernel and the head change; gamma and the moving statistics and everything in front stay
    assert changed.min() >= pos and not ((changed >= pos + cout3) & (changed < pos + 4 * cout3)).any()
    assert new[pos] == body[pos] + 0.5 and new[pos + 4 * cout3 + 7] == -body[pos + 4 * cout3 + 7] and new[-1] == 2 * body[-1]
    g = new_graph(16, 16, 16)           # a 1 x 1 conv in front of the detection layer is no block
    g.append(PL.conv2d_bn_act(g[-1].out, 32, 1, 1))
    g.append(PL.conv2d_bn_act(g[-1].out, 24, 1, 1, use_batch_normalization=False, activation_fn="linear"))
    with pytest.raises(ValueError, match="not a 3 x 3 conv with batch norm"):
        ytrain.tail_counts(g)


def test_yardstick_loop_packs_like_the_weight_loader_and_lowers_the_loss():
    """pack_block against a direct restatement of weights.cpp, and six steps of the float64 and the float32 loop on a tiny tail"""
    rng = np.random.RandomState(5)
    cout3, cin3, cout, h, w, B = 8, 8, 7, 2, 3, 2
    beta, gamma, mean, var = rng.randn(cout3), rng.uniform(0.5, 2, cout3), rng.randn(cout3) * 0.1, rng.uniform(0.5, 2, cout3)
    block = [a.astype(np.float32) for a in (beta, gamma, mean, var)] + [(rng.randn(cout3, 9, cin3) / 8).astype(np.float32)]
    scale64, bfold = tail_ref.fold(*block[:4])
    pack, bp = tail_ref.pack_block(block[4], block[0], block[2], scale64, np.float16)
    assert pack.dtype == np.float16 and bp.tobytes() == bfold.tobytes()
    o, t, c = 3, 5, 2
    want = np.float16(np.float64(block[4][o, t, c]) * (np.float64(block[1][o]) / np.sqrt(np.float64(block[3][o]) + 1e-5)))      # one rounding
    assert pack[o, t, c] == want
    import loss_grad_cases
    _, gt, counts = loss_grad_cases.random_case((h, w, 1, 2, B), 7)
    W, b = (rng.randn(cout, cout3) / 3).astype(np.float32), np.zeros(cout, dtype=np.float32)
    X3 = rng.randn(B, h, w, cin3).astype(np.float16)
    args = (X3, block, W, b, h, w, V2_ANCHORS[:2], 2, gt, counts, 1e-2, 6, np.float16)
    l64 = tail_ref.tail_train_loop(*args, mode="float64")[0]
    l32 = tail_ref.tail_train_loop(*args, mode="float32")[0]
    assert all(a > c for a, c in zip(l64, l64[1:])) and np.allclose(l32, l64, rtol=1e-3)


# ---- host code under sanitizers -----------------------------------------------------------------------------------------------------------
def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """train_tail_host.cpp (yolo_conv3x3_wgrad_plan and every argument check in front of a launch) with train_tail_host_check.cpp, a program
    with its own main, built with -fsanitize=address,undefined and run on the CPU"""
    csrc = os.path.join(ROOT, "tensorflow-yolo_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc, "san-tail", "OBJDIR=" + str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "train_tail_host_check OK" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr

"""GPU: the stride-1 SAME max-pools and the fused SPP kernel through the C ABI, bit for bit (max never rounds), and the two nets that
use them or share their trunk -- YOLOv3-SPP and YOLOv3-tiny -- against the fp32 oracle with the general pool of tests/spp_ref.py."""
import functools

import numpy as np
import pytest

import spp_ref
from helpers import new_graph, to_oracle
from oracle import forward_ref as FR
from oracle import cases, parity
from tensorflow_yolo_amd import YoloV3SPP, YoloV3Tiny
from tensorflow_yolo_amd.net import engine, layers as PL, synth

pytestmark = pytest.mark.gpu

NAMES80 = ["c%d" % i for i in range(80)]
SPP_SYMBOL = "void yolo::spp_pool_kernel<2>(yolo::SppParams)"


def same_symbol(f32, vec):
    return "void yolo::pool_same_kernel<%s, %s>(yolo::PoolParams)" % ("true" if f32 else "false", "true" if vec else "false")


# ---- the SPP block, bit-exact ------------------------------------------------------------------------------------------------------
X, P5, P9, P13, CAT = 2, 3, 5, 7, 8         # layers of spp_graph


def spp_graph(H, W, C, dtype, negative):
    """input -> 3x3 conv -> 1x1 conv (x) -> pool 5 / route x / pool 9 / route x / pool 13 -> route [p13, p9, p5, x] -> 1x1 conv.
    negative: x is a linear conv with a large negative bias (every value below zero: a zero-padded pool would show).
    Where the conv tiling does not take 4 C input channels (C = 24, 264, 20: the implicit GEMM wants 1, 2, 4 or a multiple of 8 chunks),
    the last conv reads route [concat, filler] with a filler conv that rounds the channel count up to a multiple of 64."""
    g = new_graph(H, W, 3)
    g.append(PL.conv2d_bn_act(g[-1].out, 64, 3, 1))                                                         # 1
    stem = g[-1]
    if negative:
        g.append(PL.conv2d_bn_act(g[-1].out, C, 1, 1, use_batch_normalization=False, activation_fn="linear"))   # 2 = x
    else:
        g.append(PL.conv2d_bn_act(g[-1].out, C, 1, 1))
    x = g[-1]
    g.append(PL.max_pool2d(x.out, 5, stride=1))                                                             # 3
    g.append(PL.route([x.out]))
    g.append(PL.max_pool2d(g[-1].out, 9, stride=1))                                                         # 5
    g.append(PL.route([x.out]))
    g.append(PL.max_pool2d(g[-1].out, 13, stride=1))                                                        # 7
    g.append(PL.route([g[P13].out, g[P9].out, g[P5].out, x.out]))                                           # 8
    chunks = 4 * C * (2 if dtype == "fp16" else 4) // 16
    if (4 * C) % (8 if dtype == "fp16" else 4) or not (chunks % 8 == 0 or chunks in (1, 2, 4)):
        cat = g[-1]
        g.append(PL.conv2d_bn_act(stem.out, -(4 * C) % 64 or 64, 1, 1))
        g.append(PL.route([cat.out, g[-1].out]))
    g.append(PL.conv2d_bn_act(g[-1].out, 16, 1, 1))
    w = synth.darknet_stream(g, seed=11)
    if negative:
        pos, n = synth.head_bias_offsets(g)[0]
        assert n == C
        w[pos:pos + n] = -20.0 - np.arange(n, dtype=np.float32) % 7
    return g, w


def run_block(H, W, C, dtype, fuse, negative, monkeypatch, batches=(1, 3)):
    if fuse:
        monkeypatch.delenv("YOLO_NO_SPP_FUSE", raising=False)
    else:
        monkeypatch.setenv("YOLO_NO_SPP_FUSE", "1")
    g, w = spp_graph(H, W, C, dtype, negative)
    eng = engine.HipNetwork(g, dtype=dtype, max_batch=max(batches), keep_all=True)
    eng.load_weights(w)
    # which kernel runs
    f32 = dtype == "fp32"
    fused = fuse and not f32 and H <= 32 and W <= 32 and C % 8 == 0
    syms = [ki.symbol.decode() for ki in eng.kernel_infos() if ki.kind == 2]
    if fused:
        assert syms == [SPP_SYMBOL], syms
    else:
        assert syms == [same_symbol(f32, C % (4 if f32 else 8) == 0)] * 3, syms
    for b in batches:
        xin = synth.synthetic_input(b, H, W, 3, seed=20 + b)
        eng.forward(xin)
        x = eng.read_layer(X, b)
        if negative:
            assert (x < 0).all() and x.max() < -1.0
        else:
            assert (x < 0).any() and (x > 0).any()
        pools = {}
        for layer, k in ((P5, 5), (P9, 9), (P13, 13)):
            pools[k] = eng.read_layer(layer, b)
            want = spp_ref.maxpool_nhwc(x, k)
            assert np.array_equal(pools[k], want), "%dx%d C%d b%d %s fuse=%s: pool %d differs at %s" % (
                H, W, C, b, dtype, fuse, k, np.argwhere(pools[k] != want)[:4].tolist())
        assert np.array_equal(eng.read_layer(CAT, b), np.concatenate([pools[13], pools[9], pools[5], x], axis=-1))
    return eng


MAPS = [(2, 2), (5, 5), (7, 4), (12, 12), (13, 13), (19, 19), (32, 32), (33, 33)]


@pytest.mark.parametrize("C", [8, 24, 264, 20])
@pytest.mark.parametrize("hw", MAPS, ids=["%dx%d" % m for m in MAPS])
def test_spp_block_bit_exact(hw, C, monkeypatch):
    """every pool of the block equals the clipped-window pool of the x that was read back, and the concat is [p13, p9, p5, x]: fp16 and
    float32, batch 1 and 3, the fused kernel (maps up to 32 x 32, C a multiple of 8) and the three plain launches (33 x 33, C = 20, float32,
    YOLO_NO_SPP_FUSE=1); x with both signs, and entirely negative for C = 24 and C = 20 (a fused and a fallback case)"""
    for dtype in ("fp16", "fp32"):
        for fuse in (True, False):
            for negative in ((False, True) if C in (24, 20) else (False,)):
                run_block(hw[0], hw[1], C, dtype, fuse, negative, monkeypatch)


@pytest.mark.parametrize("fuse", [True, False])
def test_spp_block_writes_only_its_tensors(fuse, monkeypatch):
    """guard bytes behind every tensor and a pattern-filled workspace: every byte outside the regions' payloads stays intact (19 x 19 with a
    ragged last slab of chunks, and a 2 x 2 map whose windows all exceed it)"""
    from helpers import guarded_run
    if fuse:
        monkeypatch.delenv("YOLO_NO_SPP_FUSE", raising=False)
    else:
        monkeypatch.setenv("YOLO_NO_SPP_FUSE", "1")
    total = 0
    for H, W, C in ((19, 19, 264), (2, 2, 24), (32, 32, 8)):
        g, w = spp_graph(H, W, C, "fp16", False)
        for keep_all in (True, False):
            eng, checked = guarded_run(g, w, synth.synthetic_input(3, H, W, 3, seed=5), "fp16", keep_all=keep_all)
            syms = [ki.symbol.decode() for ki in eng.kernel_infos() if ki.kind == 2]
            assert syms == ([SPP_SYMBOL] if fuse else [same_symbol(False, True)] * 3), syms
            total += checked
    print("fuse=%s: %d guard / slack bytes intact" % (fuse, total))


# ---- whole nets against the fp32 oracle with the general pool ------------------------------------------------------------------------
NETS = {"tiny": (YoloV3Tiny, spp_ref.TINY_V3_ANCHORS, "v3-tiny"), "spp": (YoloV3SPP, cases.COCO_V3_ANCHORS, "v3-spp")}
WHOLE = [("tiny", 96, 3), ("tiny", 416, 2), ("spp", 64, 2), ("spp", 160, 2)]
THR, IOU = 0.5, 0.6


def build_model(kind, size, batch, dtype, w, **kw):
    cls, anchors, _ = NETS[kind]
    m = cls()
    m.build(anchors, NAMES80, (size, size, 3), dtype=dtype, max_batch=batch, weights=w, **kw)
    return m


@functools.lru_cache(maxsize=None)
def reference(kind, size, batch):
    """calibrated synthetic weights, the images, and the oracle's logits (fp32, and with fp16 storage) -- computed once per net"""
    cls, anchors, key = NETS[kind]
    hg, frac = synth.HEAD_DEFAULTS[key]
    net = cls.create_network(np.reshape(anchors, [-1, 2]), NAMES80, False, input_shape=(size, size, 3))
    w = synth.darknet_stream(net, seed=5, num_classes=80, head_gain=hg, obj_bias=0.0)
    x = synth.synthetic_input(batch, size, size, 3, seed=6)
    m = build_model(kind, size, batch, "fp32", w)
    w = synth.calibrate_model(m, x, 4 * frac if size < 200 else frac)       # (small maps: a few dozen candidates all the same)
    L = to_oracle(net)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(FR, "_maxpool", spp_ref.maxpool)
        want32 = FR.forward(L, w, x)
        want16 = FR.forward(L, w, x, storage="fp16")
    for a in (want32, want16):                   # (shared among the tests: read-only)
        a.setflags(write=False)
    scales = [(y.h, y.w, y.anchors) for y in net[-1].yolos]
    return w, x, want32, want16, scales, L


def boxes_of(model, x):
    return [[(b.x, b.y, b.w, b.h, b.class_idx, b.prob) for b in img] for img in model.predict(x, THR, IOU)]


@pytest.mark.parametrize("kind,size,batch", WHOLE)
def test_whole_net_fp32_within_1e4(kind, size, batch):
    w, x, want32, _, scales, _ = reference(kind, size, batch)
    m = build_model(kind, size, batch, "fp32", w)
    got = m.forward(x)
    assert got.shape == want32.shape
    err = float(np.max(np.abs(got.astype(np.float64) - want32)))
    rep = parity.check(want32, got, boxes_of(m, x), 3, THR, IOU, scales=scales, abs_bound=1e-4)
    print("%s-%d b%d fp32: max|logit| %.2f, max abs err %.3e, boxes %d, unexplained %d"
          % (kind, size, batch, np.abs(want32).max(), err, rep["boxes_ref"], rep["boxes_unexplained"]))
    assert err <= 1e-4, err                     # absolute
    parity.assert_ok(rep)
    assert rep["boxes_unexplained"] == 0 and rep["boxes_ref"] > 0, rep


@pytest.mark.parametrize("kind,size,batch", WHOLE)
def test_whole_net_fp16_within_e_ref(kind, size, batch):
    w, x, want32, want16, scales, _ = reference(kind, size, batch)
    e_ref = float(np.max(np.abs(want16.astype(np.float64) - want32)))      # what fp16 storage alone does to these logits
    m = build_model(kind, size, batch, "fp16", w)
    got = m.forward(x)
    err = float(np.max(np.abs(got.astype(np.float64) - want32)))
    rep = parity.check(want32, got, boxes_of(m, x), 3, THR, IOU, scales=scales, e_ref=e_ref)
    names = [ki.name.decode() for ki in m.net.engine.kernel_infos()]
    print("%s-%d b%d fp16: e_hip %.3e, e_ref %.3e (ratio %.2f), boxes %d, unexplained %d"
          % (kind, size, batch, err, e_ref, err / e_ref, rep["boxes_ref"], rep["boxes_unexplained"]))
    assert err <= 1.5 * e_ref, (err, e_ref)
    parity.assert_ok(rep)
    assert rep["boxes_unexplained"] == 0 and rep["boxes_ref"] > 0, rep
    if kind == "spp":
        assert names.count("spp_pool<f16,5-9-13>") == 1 and not any(n.startswith("pool_same") for n in names), names
    else:
        assert any(n.startswith("conv_first_pool") for n in names), names


def test_spp_net_mxfp8_runs():
    """the MXFP8 plan of YOLOv3-SPP: runs, its boxes pass the gate with the MX restatement's own error as the bound, and the SPP kernel's
    three outputs are the pools of its input bit for bit"""
    import mx_ref
    w, x, want32, _, scales, L = reference("spp", 160, 2)
    m = build_model("spp", 160, 2, "mxfp8", w)
    eng = m.net.engine
    assert any(ki.name.decode().startswith("conv_mx") for ki in eng.kernel_infos())
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(FR, "_maxpool", spp_ref.maxpool)
        want_mx = mx_ref.forward(L, w, x, mx_ref.mx_conv_layers(L, eng))
    e_ref_mx = float(np.max(np.abs(want_mx.astype(np.float64) - want32)))
    got = m.forward(x)
    rep = parity.check(want32, got, boxes_of(m, x), 3, THR, IOU, scales=scales, e_ref=e_ref_mx)
    print("spp-160 b2 mxfp8: max|logit - fp32 oracle| %.3e, e_ref_mx %.3e, unexplained %d" % (rep["max_abs_logit_err"], e_ref_mx, rep["boxes_unexplained"]))
    assert rep["boxes_unexplained"] == 0, rep
    keep = build_model("spp", 160, 2, "mxfp8", w, keep_all=True).net.engine
    assert [ki.symbol.decode() for ki in keep.kernel_infos() if ki.kind == 2] == [SPP_SYMBOL]
    keep.forward(x)
    xs = keep.read_layer(78, 2)
    for layer, k in ((79, 5), (81, 9), (83, 13)):
        assert np.array_equal(keep.read_layer(layer, 2), spp_ref.maxpool_nhwc(xs, k)), k


@pytest.mark.parametrize("kind,size", [("tiny", 96), ("spp", 160)])
def test_predict_u8_equals_predict(kind, size):
    batch = 3 if kind == "tiny" else 2
    w, x, _, _, _, _ = reference(kind, size, batch)
    m = build_model(kind, size, batch, "fp16", w)
    u = np.rint(x * 255.).astype(np.uint8)
    xf = (u / 255.).astype(np.float32)
    tup = lambda boxes: [[(q.x, q.y, q.w, q.h, q.class_idx, q.prob) for q in img] for img in boxes]
    a, b = tup(m.predict(xf, THR, IOU)), tup(m.predict_u8(u, THR, IOU))
    assert a == b and sum(len(i) for i in a) > 0
    assert np.array_equal(m.forward_u8(u).view(np.uint32), m.forward(xf).view(np.uint32))

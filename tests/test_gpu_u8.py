"""GPU: the uint8 input path (ABI 7).  Contract: for a uint8 batch U the *_u8 entry points return BIT-IDENTICAL logits / box records /
counts / status to the float32 entry points fed X = float32(U / 255.) (division in float64) -- for every dtype, every stream mode and
every kernel that reads the network input.  No tolerance anywhere in this file: np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from helpers import new_graph
from oracle import cases, preprocess_ref
from tensorflow_yolo_amd import YoloV2Tiny, YoloV3, _hip
from tensorflow_yolo_amd.net import engine, layers as PL, synth, v2, v3

pytestmark = pytest.mark.gpu

NAMES80 = ["c%d" % i for i in range(80)]


def _v3(size=96):
    return v3.create_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(size, size, 3))


def _v2(size=96):
    return v2.create_full_network(np.reshape(cases.COCO_V2_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(size, size, 3))


def _tiny(size=96):
    return v2.create_tiny_network(np.reshape(cases.VOC_TINY_ANCHORS, [-1, 2]), NAMES80[:20], False, input_shape=(size, size, 3))


def _stem_no_1x1():
    g = new_graph(64, 96, 3)
    g.append(PL.conv2d_bn_act(g[-1].out, 32, 3, 1))
    g.append(PL.conv2d_bn_act(g[-1].out, 64, 3, 2))
    g.append(PL.conv2d_bn_act(g[-1].out, 64, 3, 1))          # not the 1x1 64 -> 32 of Darknet-53: the stem runs without its phase 3
    return g


def _odd(cout):
    g = new_graph(149, 151, 3)
    g.append(PL.conv2d_bn_act(g[-1].out, cout, 3, 1))
    g.append(PL.conv2d_bn_act(g[-1].out, 32, 1, 1))
    return g


def _fallback():
    """the graph of tests/test_abi.py::test_fallback_graph_plans: 16 input channels, so the input goes through prep_kernel"""
    g = new_graph(8, 8, 16)
    g.append(PL.conv2d_bn_act(g[-1].out, 32, 3, 1))
    g.append(PL.max_pool2d(g[-1].out, 2, 1))
    g.append(PL.shortcut(g[1].out, g[2].out))
    g.append(PL.upsample(g[-1].out, 2))
    g.append(PL.reorg(g[-1].out, 2))
    g.append(PL.route([g[-1].out, g[3].out]))
    return g


# name: (graph, dtype, engine keywords, name of the input kernel in yolo_kernel_info, its float32 symbol)
NETS = {
    "v3_fp16_stem_1x1": (_v3, "fp16", {}, "conv_stem<f16,3-32-64-32>", "yolo::stem_v3_kernel(yolo::StemParams)"),
    "stem_without_1x1": (_stem_no_1x1, "fp16", {}, "conv_stem<f16,3-32-64>", "yolo::stem_v3_kernel(yolo::StemParams)"),
    "v3_mxfp8_stem": (_v3, "mxfp8", {}, "conv_stem<f16,3-32-64-32>", "yolo::stem_v3_kernel(yolo::StemParams)"),
    "v3_fp16_keep_all": (_v3, "fp16", {"keep_all": True}, "conv_first<f16,32>", "void yolo::conv_first_kernel<false, 32, false>(yolo::FirstParams)"),
    "v3_fp32": (_v3, "fp32", {}, "conv_first<f32,32>", "void yolo::conv_first_kernel<true, 32, false>(yolo::FirstParams)"),
    "v2_fp16": (_v2, "fp16", {}, "conv_first_pool<f16,32>", "yolo::first_pool_mfma_kernel(yolo::FirstParams)"),
    "tiny_fp32": (_tiny, "fp32", {}, "conv_first_pool<f32,16>", "void yolo::first_pool_mfma_f32_kernel<1>(yolo::FirstParams)"),
    "v2_fp32": (_v2, "fp32", {}, "conv_first_pool<f32,32>", "void yolo::first_pool_mfma_f32_kernel<2>(yolo::FirstParams)"),
    "tiny_fp16": (_tiny, "fp16", {}, "conv_first_pool<f16,16>", "void yolo::conv_first_kernel<false, 16, true>(yolo::FirstParams)"),
    "odd_149x151_fp16": (lambda: _odd(32), "fp16", {}, "conv_first<f16,32>", "void yolo::conv_first_kernel<false, 32, false>(yolo::FirstParams)"),
    "odd_149x151_fp32_16": (lambda: _odd(16), "fp32", {}, "conv_first<f32,16>", "void yolo::conv_first_kernel<true, 16, false>(yolo::FirstParams)"),
    "fallback_prep_fp16": (_fallback, "fp16", {"keep_all": True}, "prep<f16>", "void yolo::prep_kernel<false>(yolo::PrepParams)"),
    "fallback_prep_fp32": (_fallback, "fp32", {"keep_all": True}, "prep<f32>", "void yolo::prep_kernel<true>(yolo::PrepParams)"),
}
MAX_BATCH = 4


def to_f32(u):
    return (u.astype(np.float64) / 255.).astype(np.float32)


def make_engine(name, **kw):
    graph, dtype, ekw, kname, sym = NETS[name]
    net = graph()
    opts = dict(ekw)
    opts.update(kw)
    eng = engine.HipNetwork(net, dtype=dtype, max_batch=MAX_BATCH, **opts)
    eng.load_weights(synth.darknet_stream(net, seed=11))
    # which kernel reads the input: asserted, so that no case passes on another path than the one it is named for
    infos = [(k.name.decode(), k.symbol.decode()) for k in eng.kernel_infos()]
    readers = [i for i in infos if i[0].startswith(("conv_stem", "conv_first", "prep")) and "fused into" not in i[0]]
    assert readers == [(kname, sym)], (name, infos[:4])
    if dtype == "mxfp8":
        assert "dtype=mxf8" in eng.describe()
    return eng


def images(eng, batch, seed):
    """random bytes; image 0 all 0 / image 1 all 255 / image 2 covering 0..255 where the batch has them"""
    h, w, c = eng.input_hwc
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 256, size=(batch, h, w, c), dtype=np.uint8)
    if batch >= 3:
        u[0] = 0
        u[1] = 255
        u[2] = (np.arange(h * w * c) % 256).astype(np.uint8).reshape(h, w, c)
    elif batch == 1:
        u[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return u


@pytest.mark.parametrize("name", sorted(NETS))
def test_forward_u8_is_bit_identical_to_forward(name):
    """forward_u8(U) == forward(float32(U / 255.)) bit for bit: batch 1, an odd batch, a full batch; then the same bytes starting 1, 2 and
    3 bytes into their allocation (no alignment beyond one byte may be assumed)."""
    import torch
    eng = make_engine(name)
    for batch in (1, 3, 4):
        u = images(eng, batch, seed=batch)
        want = eng.forward(to_f32(u)).cpu().numpy()
        got = eng.forward_u8(u).cpu().numpy()
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, batch, float(np.abs(got - want).max()))
        if batch == 3:
            for off in (1, 2, 3):
                flat = torch.zeros(u.size + 8, dtype=torch.uint8, device=eng.device)
                view = flat[off:off + u.size].view(u.shape)
                view.copy_(torch.from_numpy(u))
                assert view.data_ptr() == flat.data_ptr() + off and view.is_contiguous()
                got = eng.forward_u8(view).cpu().numpy()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, "offset", off)
    assert eng.u8_calls == 3 + 3


@pytest.mark.parametrize("name", ["v3_fp16_stem_1x1", "v3_mxfp8_stem", "v2_fp16", "v3_fp32"])
def test_forward_u8_two_halves(name):
    """streams = 2: the batch runs as two halves on two streams, the second half's input offset is img0 * H*W*3 BYTES for uint8"""
    eng = make_engine(name, streams=2)
    assert eng.num_streams == 2
    for batch in (4, 3):
        u = images(eng, batch, seed=20 + batch)
        want = eng.forward(to_f32(u)).cpu().numpy()
        got = eng.forward_u8(u).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, batch)
        assert not np.array_equal(want[0], want[batch - 1])         # (the halves really hold different images)


def test_forward_timed_u8_runs_the_same_plan():
    eng = make_engine("v3_fp16_stem_1x1")
    u = images(eng, 4, seed=5)
    ms = eng.forward_timed_u8(u)
    ms32 = eng.forward_timed(to_f32(u))
    assert ms.shape == ms32.shape == (eng.num_kernels,) and ((ms > 0) == (ms32 > 0)).all() and ms.sum() > 0


def _calibrated(cls, anchors, names, size, dtype, kind, batch, **kw):
    model = cls()
    net = cls.create_network(np.reshape(anchors, [-1, 2]), names, False, input_shape=(size, size, 3))
    hg, frac = synth.HEAD_DEFAULTS[kind]
    w = synth.darknet_stream(net, seed=1, num_classes=len(names), head_gain=hg, obj_bias=0.0)
    model.build(anchors, names, (size, size, 3), dtype=dtype, max_batch=batch, weights=w, **kw)
    u = np.rint(synth.synthetic_input(batch, size, size, 3, seed=2) * 255.).astype(np.uint8)
    synth.calibrate_model(model, to_f32(u), 4 * frac)
    return model, u


@pytest.mark.parametrize("kind, dtype", [("v3", "fp16"), ("v3", "fp32"), ("v2-tiny", "fp16"), ("v3", "mxfp8")])
def test_detect_u8_and_predict_u8_equal_their_float32_twins(kind, dtype):
    """box records as raw bytes, counts and status of detect_u8 against detect (class-agnostic and per-class NMS), and the BoundingBox
    lists of predict_u8 against predict"""
    if kind == "v3":
        model, u = _calibrated(YoloV3, cases.COCO_V3_ANCHORS, NAMES80, 160, dtype, "v3", 3)
    else:
        model, u = _calibrated(YoloV2Tiny, cases.VOC_TINY_ANCHORS, NAMES80[:20], 160, dtype, "v2-tiny", 3)
    eng = model.net.engine
    x = to_f32(u)
    for mode in (_hip.NMS_AGNOSTIC, _hip.NMS_PER_CLASS):
        want = [t.cpu().numpy().copy() for t in eng.detect(x, 0.5, 0.6, mode)]
        got = [t.cpu().numpy().copy() for t in eng.detect_u8(u, 0.5, 0.6, mode)]
        assert want[1].sum() > 0, "no boxes: the comparison would be empty"
        for i in range(len(u)):         # (records behind count[i] are not written by either call)
            n = int(want[1][i])
            assert np.array_equal(got[0][i, :n].view(np.uint32), want[0][i, :n].view(np.uint32)), (mode, i)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    a = model.predict(x, 0.5, 0.6)
    b = model.predict_u8(u, 0.5, 0.6)
    tup = lambda boxes: [[(q.x, q.y, q.w, q.h, q.class_idx, q.prob) for q in img] for img in boxes]
    assert tup(a) == tup(b) and sum(len(i) for i in a) > 0
    assert np.array_equal(model.forward_u8(u).view(np.uint32), model.forward(x).view(np.uint32))
    with pytest.raises(ValueError, match="uint8"):
        model.predict_u8(x, 0.5, 0.6)
    # a uint8 array through the float32 entry keeps its old meaning: cast, unscaled (0..255)
    assert np.array_equal(model.forward(u[:1]), model.forward(u[:1].astype(np.float32)))


@pytest.mark.parametrize("src_hw, dst_hw, pad", [((48, 64), (160, 160), 0), ((300, 200), (96, 128), 5), ((33, 47), (33, 47), 3), ((17, 301), (64, 32), 1)])
@pytest.mark.parametrize("swap", [0, 1])
def test_resize_u8_equals_the_oracle_and_the_float32_resize(src_hw, dst_hw, pad, swap):
    """yolo_preprocess_resize_u8 == oracle/preprocess_ref.resize_linear_u8 exactly (up- and down-scaling, non-square, same size, swap_rb, a
    padded source pitch), and yolo_preprocess_resize of the same source == float32(that / 255.) exactly"""
    import torch
    lib = _hip.lib()
    rng = np.random.default_rng(src_hw[0] * 1000 + dst_hw[1] + swap)
    (sh, sw), (dh, dw) = src_hw, dst_hw
    img = rng.integers(0, 256, size=(sh, sw, 3), dtype=np.uint8)
    pitch = sw * 3 + pad
    padded = np.full((sh, pitch), 0xA5, dtype=np.uint8)
    padded[:, :sw * 3] = img.reshape(sh, sw * 3)
    src = torch.from_numpy(padded).cuda()
    dst8 = torch.full((dh * dw * 3 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    dst32 = torch.zeros((dh, dw, 3), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _hip.check(lib.yolo_preprocess_resize_u8(src.data_ptr(), sh, sw, pitch, dst8.data_ptr() + 1, dh, dw, swap, s), "yolo_preprocess_resize_u8")
    _hip.check(lib.yolo_preprocess_resize(src.data_ptr(), sh, sw, pitch, dst32.data_ptr(), dh, dw, swap, s), "yolo_preprocess_resize")
    torch.cuda.synchronize()
    want = preprocess_ref.resize_linear_u8(img[:, :, ::-1] if swap else img, dh, dw)
    got = dst8.cpu().numpy()
    assert np.array_equal(got[1:1 + dh * dw * 3].reshape(dh, dw, 3), want)
    assert (got[0] == 0x5A) and (got[1 + dh * dw * 3:] == 0x5A).all()         # nothing written outside the image
    assert np.array_equal(dst32.cpu().numpy().view(np.uint32), to_f32(want).view(np.uint32))


def test_pipelined_test_loop_stages_uint8(tmp_path, capsys):
    """Yolo.test's pipeline with `staging = u8` keeps the resized batch as uint8 and goes through detect_u8; without the key it stages
    float32 as before: the same console lines either way"""
    import json
    import os
    from PIL import Image
    from tensorflow_yolo_amd import launcher
    from tensorflow_yolo_amd.net import base
    rng = np.random.RandomState(3)
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    for i in range(5):
        Image.fromarray(rng.randint(0, 256, size=(40 + i, 50, 3)).astype(np.uint8)).save(str(img_dir / ("f%d.png" % i)))
    names = NAMES80[:20]
    net = _tiny(160)
    hg, frac = synth.HEAD_DEFAULTS["v2-tiny"]
    wpath = str(tmp_path / "tiny.weights")
    base.write_darknet_weights(wpath, synth.darknet_stream(net, seed=3, num_classes=20, head_gain=hg, obj_bias=2.0), "v2")
    lines = {}
    for staging in ("u8", "f32"):
        out_dir = tmp_path / ("out_" + staging)
        params = dict(image_dir=str(img_dir), out_dir=str(out_dir), batch_size=2, threshold=0.3, iou_threshold=0.5, anchors=list(cases.VOC_TINY_ANCHORS),
                      class_names=names, input_h=160, input_w=160, input_c=3, checkpoint_path="", pretrained_weights_path=wpath,
                      cpu_only="False", dtype="fp16", pipeline="True", workers=2)
        if staging == "u8":
            params["staging"] = "u8"
        model = launcher.pick_model("v2-tiny")
        model.test(params)
        text = capsys.readouterr().out
        lines[staging] = [l.replace(str(out_dir), "OUT") for l in text.splitlines() if ": Found " in l]
        assert len(lines[staging]) == 5 and model.timing["mode"] == "pipelined" and model.timing["staging"] == staging
        assert model.net.engine.u8_calls == (3 if staging == "u8" else 0)
    assert lines["u8"] == lines["f32"]

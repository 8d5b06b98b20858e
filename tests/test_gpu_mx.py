"""GPU: the MXFP8 plan (dtype="mxfp8") -- the kernel's quantizer bit for bit against the torch restatement (tests/mx_ref.py),
single MX convs and whole networks against the restatement and the fp32 oracle, and guard-band canaries around its launches."""
import numpy as np
import pytest
import torch

import mx_ref
from helpers import new_graph, rel_err, run_hip, to_oracle
from oracle import cases, decode_ref, forward_ref as FR, parity
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import layers as PL, synth, v2, v3

pytestmark = pytest.mark.gpu

NAMES80 = ["c%d" % i for i in range(80)]


def test_quantizer_is_bit_identical_to_the_restatement():
    rng = np.random.RandomState(7)
    rows, ch = 300, 256
    v = (rng.standard_normal((rows, ch)) * np.exp2(rng.randint(-20, 12, (rows, 1)))).astype(np.float16)
    # engineered blocks: zero, a power-of-two amax, the 448 / 464 boundary, saturation, subnormal results, negatives, fp16 extremes
    v[0, :32] = 0
    v[1, :32] = np.float16(1.0); v[1, 3] = np.float16(2.0)
    v[2, :3] = [448 / 256, 464 / 256, 1.0]
    v[3, :2] = [1.9375, -1.99]
    v[4, :4] = [1.0, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -17]
    v[5, :3] = [1.0, 2.0 ** -18, 3 * 2.0 ** -18]
    v[6, :32] = -np.abs(v[6, :32])
    v[7, :2] = [65504.0, -6e-8]
    v[8, :2] = [6e-8, 0.0]
    src = torch.from_numpy(v).cuda()
    q = torch.empty((rows, ch), dtype=torch.uint8, device="cuda")
    s = torch.empty((rows, ch // 32), dtype=torch.uint8, device="cuda")
    _hip.check(_hip.lib().yolo_mx_quantize(src.data_ptr(), rows, ch, q.data_ptr(), s.data_ptr(), None), "yolo_mx_quantize")
    torch.cuda.synchronize()
    wq, ws = mx_ref.quantize(torch.from_numpy(v.astype(np.float32)))
    assert torch.equal(s.cpu(), ws), np.argwhere((s.cpu() != ws).numpy())[:8]
    bad = np.argwhere((q.cpu() != wq).numpy())
    assert len(bad) == 0, [(tuple(i), v[tuple(i)], int(q.cpu()[tuple(i)]), int(wq[tuple(i)])) for i in bad[:8]]


def _single(cin, cout, H, W, residual=False, concat=False, linear=False):
    g = new_graph(H, W, cin)
    g.append(PL.conv2d_bn_act(g[-1].out, cout, 3, 1, use_batch_normalization=not linear, activation_fn=None if linear else "leaky"))
    if residual:
        assert cin == cout
        g.append(PL.shortcut(g[-1].out, g[0].out))
    if concat:
        g.append(PL.conv2d_bn_act(g[0].out, 128, 1, 1))
        g.append(PL.route([g[1].out, g[-1].out]))
    g.append(PL.conv2d_bn_act(g[-1].out, 48, 1, 1))      # the head stays an fp16 1x1 conv: float32 out
    return g


def _check_against_restatement(g, x, **kw):
    w = synth.darknet_stream(g, seed=11)
    got, eng = run_hip(g, w, x, "mxfp8", **kw)
    L = to_oracle(g)
    mx = mx_ref.mx_conv_layers(L, eng)
    assert mx, eng.describe()
    want = mx_ref.forward(L, w, x, mx)
    e = rel_err(got, want)
    print("MX single conv %s: rel err vs restatement %.2e (MX layers %s)" % (x.shape, e, sorted(mx)))
    assert e <= 2.5e-3, e
    return eng


@pytest.mark.parametrize("cin,cout,H,W,B", [(128, 256, 17, 23, 2), (256, 128, 9, 11, 3), (512, 256, 13, 13, 1), (1024, 192, 7, 5, 2),
                                            (128, 128, 76, 76, 1), (256, 128, 3, 100, 2)])     # W = 100: the widest map the patch takes
def test_single_mx_conv(cin, cout, H, W, B):
    g = _single(cin, cout, H, W)
    _check_against_restatement(g, synth.synthetic_input(B, H, W, cin, seed=3))


@pytest.mark.parametrize("case", ["residual", "concat", "linear", "forced"])
def test_single_mx_conv_epilogues(case):
    H, W, B = 19, 21, 2
    g = _single(256, 256, H, W, residual=case == "residual", concat=case == "concat", linear=case == "linear")
    eng = _check_against_restatement(g, synth.synthetic_input(B, H, W, 256, seed=4), force_tile=24 if case == "forced" else None)
    names = [ki.name.decode() for ki in eng.kernel_infos()]
    assert sum(n.startswith("conv_mx") for n in names) == 1, names


def _net(kind):
    if kind == "v3":
        return v3.create_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(416, 416, 3))
    return v2.create_full_network(np.reshape(cases.COCO_V2_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(416, 416, 3))


@pytest.mark.parametrize("kind", ["v3", "v2"])
def test_whole_net_mxfp8_against_the_fp32_oracle(kind):
    from tensorflow_yolo_amd import YoloV2, YoloV3
    net = _net(kind)
    hg, frac = synth.HEAD_DEFAULTS[kind]
    w = synth.darknet_stream(net, seed=5, num_classes=80, head_gain=hg, obj_bias=0.0)
    x = synth.synthetic_input(2, 416, 416, 3, seed=6)
    model = YoloV3() if kind == "v3" else YoloV2()
    anchors = cases.COCO_V3_ANCHORS if kind == "v3" else cases.COCO_V2_ANCHORS
    model.build(anchors, NAMES80, (416, 416, 3), dtype="fp16", max_batch=2, weights=w)
    w = synth.calibrate_model(model, x, frac)
    model = YoloV3() if kind == "v3" else YoloV2()
    model.build(anchors, NAMES80, (416, 416, 3), dtype="mxfp8", max_batch=2, weights=w)
    eng = model.net.engine
    L = to_oracle(model.net)
    t = torch.get_num_threads()
    torch.set_num_threads(min(32, t))
    try:
        want32 = FR.forward(L, w, x)
        want_mx = mx_ref.forward(L, w, x, mx_ref.mx_conv_layers(L, eng))
        want16 = FR.forward(L, w, x, storage="fp16")
    finally:
        torch.set_num_threads(t)
    got = model.forward(x)
    e_ref_mx = float(np.max(np.abs(want_mx.astype(np.float64) - want32)))
    e_ref16 = float(np.max(np.abs(want16.astype(np.float64) - want32)))
    err = float(np.max(np.abs(got.astype(np.float64) - want32)))
    print("%s-416 b2 mxfp8: max|logit - fp32 oracle| %.3e, e_ref_mx %.3e (fp16 storage alone: %.3e), rel vs restatement %.2e"
          % (kind, err, e_ref_mx, e_ref16, rel_err(got, want_mx)))
    assert err <= 1.5 * e_ref_mx, (err, e_ref_mx)
    boxes = model.predict(x, 0.5, 0.6)
    got_boxes = [[(b.x, b.y, b.w, b.h, b.class_idx, b.prob) for b in img] for img in boxes]
    if kind == "v3":
        rep = parity.check(want32, got, got_boxes, 3, 0.5, 0.6, scales=decode_ref.v3_scales(cases.COCO_V3_ANCHORS, (416, 416)), e_ref=e_ref_mx)
    else:
        rep = parity.check(want32, got, got_boxes, 2, 0.5, 0.6, anchors=cases.COCO_V2_ANCHORS, num_classes=80, e_ref=e_ref_mx)
    print(rep)
    assert rep["boxes_unexplained"] == 0, rep


def test_mx_launches_write_only_their_tensors():
    from helpers import guarded_run
    g = new_graph(19, 21, 256)
    g.append(PL.conv2d_bn_act(g[-1].out, 256, 3, 1))
    g.append(PL.shortcut(g[-1].out, g[0].out))           # MX conv + fused residual add
    g.append(PL.conv2d_bn_act(g[-1].out, 128, 3, 1))      # a second MX conv
    g.append(PL.conv2d_bn_act(g[-1].out, 16, 1, 1))
    guarded_run(g, synth.darknet_stream(g, seed=2), synth.synthetic_input(3, 19, 21, 256, seed=2), "mxfp8")

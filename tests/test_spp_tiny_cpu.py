"""CPU: YOLOv3-tiny and YOLOv3-SPP (upstream Darknet yolov3-tiny.cfg / yolov3-spp.cfg in the reference's layer vocabulary) -- layer lists,
weight counts, plans of the three dtypes, the fused SPP kernel and its fallback in the plan, the max-pool sizes the planner takes, and the
pool reference the GPU tests compare with (tests/spp_ref.py).  No compute calls."""
import ctypes as C

import numpy as np
import pytest
import torch

import spp_ref
from helpers import new_graph, to_oracle
from oracle import cases, forward_ref, topology
from tensorflow_yolo_amd import _hip, launcher
from tensorflow_yolo_amd.net import engine, layers as PL, v3

NAMES80 = ["c%d" % i for i in range(80)]
SPP_SYMBOL = "void yolo::spp_pool_kernel<2>(yolo::SppParams)"


def make(kind, size, names=NAMES80):
    if kind == "tiny":
        return v3.create_tiny_network(np.reshape(spp_ref.TINY_V3_ANCHORS, [-1, 2]), names, False, input_shape=(size, size, 3))
    return v3.create_spp_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), names, False, input_shape=(size, size, 3))


def oracle_list(kind, size, nc=80):
    if kind == "tiny":
        return spp_ref.yolov3_tiny(spp_ref.TINY_V3_ANCHORS, nc, (size, size, 3))
    return spp_ref.yolov3_spp(cases.COCO_V3_ANCHORS, nc, (size, size, 3))


def infos(plan):
    out = []
    for k in range(plan.num_kernels):
        ki = _hip.KernelInfo()
        _hip.check(plan.lib.yolo_net_kernel_info(plan.handle, k, C.byref(ki)), "yolo_net_kernel_info")
        out.append(ki)
    return out


@pytest.mark.parametrize("size", [416, 608])
def test_tiny_layer_list(size):
    net = make("tiny", size)
    L = to_oracle(net)
    want = oracle_list("tiny", size)
    assert len(L) == len(want) == 1 + 24 + 1           # input + Darknet layers 0..23 + detection_layer
    for got, ref in zip(L, want):
        assert got[:2] == ref[:2] and (got == ref or got[0] == "yolo" and len(got[2]) == len(ref[2]) == 3), (got, ref)
    S = topology.shapes(L)
    g = size // 32
    assert [l.out.hwc for l in net[:-1]] == S[:-1]
    assert L[12] == ("maxpool", 11, 2, 1) and S[12] == (g, g, 512)                 # Darknet 11: pool 2 / 1
    assert L[18] == ("route", [14]) and L[21] == ("route", [20, 9])                # route [13], route [19, 8]
    assert S[17] == (g, g, 255) and S[24] == (2 * g, 2 * g, 255) and S[21] == (2 * g, 2 * g, 384)
    assert L[25] == ("detection", [17, 24])
    yolos = net[-1].yolos
    assert [(y.h, y.w, y.b) for y in yolos] == [(g, g, 3), (2 * g, 2 * g, 3)]
    # anchors 3, 4, 5 at stride 32, anchors 0, 1, 2 at stride 16, in grid units
    assert np.allclose(yolos[0].anchors, np.reshape(spp_ref.TINY_V3_ANCHORS, [-1, 2])[3:] / 32.)
    assert np.allclose(yolos[1].anchors, np.reshape(spp_ref.TINY_V3_ANCHORS, [-1, 2])[:3] / 16.)
    assert net[-1].out.hwc == (3 * (g * g + 4 * g * g), 1, 85)


@pytest.mark.parametrize("size", [416, 608])
def test_spp_layer_list(size):
    net = make("spp", size)
    L = to_oracle(net)
    want = oracle_list("spp", size)
    base = to_oracle(v3.create_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(size, size, 3)))
    assert len(L) == len(want) == len(base) + 7        # 3 pools, 2 routes back to x, the concat, one more conv
    for got, ref in zip(L, want):
        assert got[:2] == ref[:2] and (got == ref or got[0] == "yolo" and len(got[2]) == len(ref[2]) == 3), (got, ref)
    assert L[:76] == base[:76]                          # the trunk is Darknet-53's
    S = topology.shapes(L)
    assert [l.out.hwc for l in net[:-1]] == S[:-1]
    g = size // 32
    x = 78
    assert L[x] == ("conv", 77, 512, 1, 1, True, "leaky")
    assert L[79:85] == [("maxpool", x, 5, 1), ("route", [x]), ("maxpool", 80, 9, 1), ("route", [x]), ("maxpool", 82, 13, 1),
                        ("route", [83, 81, 79, x])]
    assert all(S[i] == (g, g, 512) for i in (78, 79, 81, 83)) and S[84] == (g, g, 2048)
    assert [op[2:4] for op in L[85:90]] == [(512, 1), (1024, 3), (512, 1), (1024, 3), (255, 1)] and L[90][0] == "yolo"
    assert L[91] == ("route", [87])                     # the lateral reads the 1x1 two convs before the head conv
    assert L[94] == ("route", [93, 62]) and L[106] == ("route", [105, 37])
    assert L[-1] == ("detection", [90, 102, 114])
    assert [(y.h, y.w) for y in net[-1].yolos] == [(g, g), (2 * g, 2 * g), (4 * g, 4 * g)]


@pytest.mark.parametrize("kind, known", [("tiny", 8858734), ("spp", 63052381)])
def test_weight_counts(kind, known):
    """sum over convs of k^2 Cin Cout + (4 if BN else 1) Cout -- and the float counts of upstream's yolov3-tiny.weights /
    yolov3-spp.weights ((file bytes - 20) / 4)"""
    net = make(kind, 416)
    L = oracle_list(kind, 416)
    want = spp_ref.conv_weight_count(L, topology.shapes(L))
    assert want == known
    assert sum(l.weight_count() for l in net if isinstance(l, PL.conv2d_bn_act)) == want
    p = engine.Plan(net, dtype="fp16", max_batch=2)
    assert p.weight_count == want == p.lib.yolo_net_weight_count(p.handle)


@pytest.mark.parametrize("dtype", ["fp16", "fp32", "mxfp8"])
@pytest.mark.parametrize("kind", ["tiny", "spp"])
def test_both_nets_plan_in_every_dtype(kind, dtype):
    net = make(kind, 416)
    p = engine.Plan(net, dtype=dtype, max_batch=4)
    n_scales = 2 if kind == "tiny" else 3
    assert p.head.version == 3 and p.head.n_scales == n_scales and p.head.n_classes == 80
    assert p.output_count == net[-1].out.hwc[0] * 85
    d = p.describe()
    assert d.count("head logits") == n_scales
    if kind == "tiny":      # the trunk is tiny-YOLOv2's: first conv + pool in one kernel, the plain 2x2 pools elsewhere
        assert "conv_first" in d and "fused 2x2/2 max-pool (layer 2)" in d and "spp_pool" not in d and "pool_same" not in d
        assert d.count("concat slice") == 2 and "fused: upsample x2" in d
    else:
        assert d.count("fused: +shortcut") == 23 and d.count("fused: upsample x2") == 2


def test_spp_plan_fuses_the_three_pools(monkeypatch):
    net = make("spp", 608)
    p = engine.Plan(net, dtype="fp16", max_batch=32)
    d = p.describe()
    assert d.count("spp_pool layer 79") == 1 and d.count("pool_same") == 0 and "fused SPP block: pools 5 / 9 / 13" in d
    line = [l for l in d.splitlines() if "spp_pool" in l][0]
    # one input view, three output views: channel slices of the 2048-channel concat buffer, [p13, p9, p5, x]
    assert "in=b0[19x19x512 ld2048+1536]" in line
    assert all("out=b0[19x19x512 ld2048+%d]" % off in line for off in (1024, 512, 0))
    ks = [ki for ki in infos(p) if ki.name.decode().startswith("spp_pool")]
    assert len(ks) == 1 and ks[0].name.decode() == "spp_pool<f16,5-9-13>" and ks[0].symbol.decode() == SPP_SYMBOL
    assert ks[0].bytes == 4 * 19 * 19 * 512 * 2 and ks[0].kind == 2 and ks[0].layer == 79         # 1 read + 3 writes
    assert p.num_kernels == engine.Plan(v3.create_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(608, 608, 3)),
                                        dtype="fp16", max_batch=32).num_kernels + 2                  # + the SPP kernel and one conv
    # keep_all keeps the fusion: nothing is elided
    assert engine.Plan(net, dtype="fp16", max_batch=2, keep_all=True).describe().count("spp_pool layer 79") == 1
    assert engine.Plan(net, dtype="mxfp8", max_batch=2).describe().count("spp_pool layer 79") == 1
    # fp32: three launches of the plain kernel
    p32 = engine.Plan(net, dtype="fp32", max_batch=2)
    d32 = p32.describe()
    assert d32.count("pool_same") == 3 and "spp_pool" not in d32
    k32 = [ki for ki in infos(p32) if ki.name.decode().startswith("pool_same")]
    assert [ki.name.decode() for ki in k32] == ["pool_same<f32,5x5>", "pool_same<f32,9x9>", "pool_same<f32,13x13>"]
    assert all(ki.symbol.decode() == "void yolo::pool_same_kernel<true, true>(yolo::PoolParams)" and ki.bytes == 2 * 19 * 19 * 512 * 4 for ki in k32)
    # ... and under YOLO_NO_SPP_FUSE=1
    monkeypatch.setenv("YOLO_NO_SPP_FUSE", "1")
    pn = engine.Plan(net, dtype="fp16", max_batch=32)
    dn = pn.describe()
    assert dn.count("pool_same") == 3 and "spp_pool" not in dn and pn.num_kernels == p.num_kernels + 2
    kn = [ki for ki in infos(pn) if ki.name.decode().startswith("pool_same")]
    assert [ki.symbol.decode() for ki in kn] == ["void yolo::pool_same_kernel<false, true>(yolo::PoolParams)"] * 3
    assert pn.workspace_bytes == p.workspace_bytes


def test_new_kernel_symbols_are_kernels_of_the_library():
    import subprocess
    exported = {line.split(" ", 2)[2].strip() for line in subprocess.check_output(["nm", "-DC", _hip.LIB_PATH], text=True).splitlines()
                if len(line.split(" ", 2)) == 3}
    for sym in [SPP_SYMBOL, "void yolo::spp_pool_kernel<1>(yolo::SppParams)"] + \
               ["void yolo::pool_same_kernel<%s, %s>(yolo::PoolParams)" % (a, b) for a in ("false", "true") for b in ("false", "true")]:
        assert sym in exported, sym


def test_workspace_regions_cover_the_spp_tensors():
    net = make("spp", 416)
    p = engine.Plan(net, dtype="fp16", max_batch=2, keep_all=True, guard_bytes=4096)
    concat = 2 * 13 * 13 * 2048 * 2
    assert sum(1 for _, _, used, region in p.workspace_regions() if used == concat and region >= used + 4096) >= 1


def _pool_graph(ksize, stride):
    g = new_graph(8, 8, 8)
    g.append(PL.max_pool2d(g[-1].out, ksize, stride=stride))
    g.append(PL.conv2d_bn_act(g[-1].out, 16, 1, 1))
    return g


@pytest.mark.parametrize("ksize, stride", [(4, 1), (15, 1), (5, 2), (3, 2), (1, 1)])
def test_unsupported_pools_fail_to_plan(ksize, stride):
    descs = engine.to_descs(_pool_graph(ksize, stride))
    o = _hip.NetOptions(dtype=_hip.DTYPE_F16, max_batch=1)
    h = C.c_void_p()
    rc = _hip.lib().yolo_net_create(descs, 3, C.byref(o), C.byref(h))
    assert rc == 2                                      # YOLO_ERR_PLAN
    msg = _hip.lib().yolo_last_error()
    assert b"maxpool supports ksize 2" in msg and b"odd ksize 3..13 with stride 1" in msg


@pytest.mark.parametrize("ksize", [3, 5, 7, 9, 11, 13])
def test_odd_stride1_pools_plan_and_keep_the_shape(ksize):
    g = _pool_graph(ksize, 1)
    assert g[1].out.hwc == (8, 8, 8)
    for dtype in ("fp16", "fp32"):
        d = engine.Plan(g, dtype=dtype, max_batch=2).describe()
        assert "pool_same layer 1" in d and "SAME max-pool %dx%d/1" % (ksize, ksize) in d


def test_spp_fusion_needs_the_block_and_aligned_views():
    def block(h, w, c, sizes=(5, 9, 13)):
        g = new_graph(h, w, 8)
        g.append(PL.conv2d_bn_act(g[-1].out, c, 1, 1))
        x = g[-1]
        pools = []
        for k in sizes:
            g.append(PL.max_pool2d(x.out, k, stride=1))
            pools.append(g[-1])
        g.append(PL.route([p.out for p in reversed(pools)] + [x.out]))
        g.append(PL.conv2d_bn_act(g[-1].out, 16, 1, 1))
        return g
    count = lambda g, dtype="fp16": engine.Plan(g, dtype=dtype, max_batch=2).describe().count("spp_pool")
    assert count(block(32, 32, 64)) == 1 and count(block(2, 2, 8)) == 1 and count(block(7, 4, 16)) == 1
    assert count(block(9, 9, 16, sizes=(3, 5, 7))) == 1            # the same relation at radius 1
    assert count(block(33, 33, 64)) == 0 and count(block(32, 33, 64)) == 0          # larger than the LDS planes
    assert count(block(19, 19, 64), "fp32") == 0
    assert count(block(9, 9, 16, sizes=(5, 9, 11))) == 0 and count(block(9, 9, 16, sizes=(5, 7, 13))) == 0
    assert count(block(9, 9, 16, sizes=(5, 9, 9))) == 0


# ---- the pool reference of the GPU tests -------------------------------------------------------------------------------------------
def test_general_pool_equals_the_oracle_pool_for_k2():
    rng = np.random.RandomState(3)
    for h, w in ((6, 6), (7, 5), (13, 13)):
        x = torch.from_numpy(rng.randn(2, 5, h, w).astype(np.float32))
        for s in (1, 2):
            assert torch.equal(spp_ref.maxpool(x, 2, s), forward_ref._maxpool(x, 2, s))


@pytest.mark.parametrize("hw", [(5, 5), (7, 4), (13, 13)])
def test_general_pool_equals_a_clipped_window_loop(hw):
    rng = np.random.RandomState(4)
    x = rng.randn(2, hw[0], hw[1], 3).astype(np.float32)
    neg = -np.abs(x) - 1.0                               # all negative: zero padding would show
    for k in (5, 9, 13):
        assert np.array_equal(spp_ref.maxpool_nhwc(x, k), spp_ref.maxpool_naive(x, k))
        got = spp_ref.maxpool_nhwc(neg, k)
        assert np.array_equal(got, spp_ref.maxpool_naive(neg, k)) and (got < 0).all()


@pytest.mark.parametrize("hw", [(2, 2), (5, 5), (7, 4), (13, 13), (19, 19)])
def test_pools_cascade(hw):
    """what the fused kernel rests on: with clipped windows and no padding value pool9 = pool5 o pool5 and pool13 = pool5 o pool9"""
    x = np.random.RandomState(5).randn(2, hw[0], hw[1], 4).astype(np.float32)
    p5 = spp_ref.maxpool_nhwc(x, 5)
    p9 = spp_ref.maxpool_nhwc(x, 9)
    assert np.array_equal(spp_ref.maxpool_nhwc(p5, 5), p9)
    assert np.array_equal(spp_ref.maxpool_nhwc(p9, 5), spp_ref.maxpool_nhwc(x, 13))
    assert np.array_equal(spp_ref.maxpool_nhwc(spp_ref.maxpool_nhwc(x, 3), 3), p5)


def test_oracle_forward_runs_the_spp_list_with_the_patched_pool(monkeypatch):
    from tensorflow_yolo_amd.net import synth
    net = make("spp", 64, NAMES80[:2])
    L = to_oracle(net)
    w = synth.darknet_stream(net, seed=1, num_classes=2)
    x = synth.synthetic_input(1, 64, 64, 3, seed=2)
    _, plain = forward_ref.forward(L, w, x, keep={78, 83})
    assert not np.array_equal(plain[83], spp_ref.maxpool_naive(plain[78], 13))        # the k = 2 form pads only after: another window
    monkeypatch.setattr(forward_ref, "_maxpool", spp_ref.maxpool)
    out, kept = forward_ref.forward(L, w, x, keep={78, 79, 81, 83, 84})
    assert out.shape == (1, 3 * (4 + 16 + 64), 7)
    assert np.array_equal(kept[84], np.concatenate([kept[83], kept[81], kept[79], kept[78]], axis=-1))
    assert np.array_equal(kept[83], spp_ref.maxpool_naive(kept[78], 13))


# ---- public surface ----------------------------------------------------------------------------------------------------------------
def test_launcher_knows_the_new_versions(tmp_path):
    from tensorflow_yolo_amd import YoloV3SPP, YoloV3Tiny
    assert isinstance(launcher.pick_model("v3-tiny"), YoloV3Tiny) and isinstance(launcher.pick_model("v3-spp"), YoloV3SPP)
    with pytest.raises(ValueError, match="Unsupported version"):
        launcher.pick_model("v3-huge")
    import os
    cfg_dir = os.path.join(os.path.dirname(launcher.__file__), "config")
    for name, ver, n_anchors in (("yolo_3_tiny.ini", "v3-tiny", 12), ("yolo_3_spp.ini", "v3-spp", 18)):
        cfg = launcher.read_config(os.path.join(cfg_dir, name))
        assert cfg["COMMON"]["version"] == ver and len(cfg["TEST"]["anchors"]) == n_anchors and len(cfg["TEST"]["class_names"]) == 80


def test_launcher_v3_tiny_reaches_the_engine(tmp_path, monkeypatch):
    """`version = v3-tiny` gets as far as the engine: on a machine without a GPU that is HipNetwork's "no GPU" error"""
    from PIL import Image
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    (tmp_path / "imgs").mkdir()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(str(tmp_path / "imgs" / "a.png"))
    ini = tmp_path / "t.ini"
    ini.write_text("[COMMON]\nversion = v3-tiny\ninput_h = 96\ninput_w = 96\ninput_c = 3\n[TEST]\nimage_dir = imgs\nout_dir = out\n"
                   "batch_size = 1\nthreshold = 0.5\niou_threshold = 0.6\nanchors = %r\nclass_names = %r\n"
                   "checkpoint_path =\npretrained_weights_path = none.weights\n" % (spp_ref.TINY_V3_ANCHORS, NAMES80[:3]))
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        launcher.run(launcher.read_config(str(ini)), "test")

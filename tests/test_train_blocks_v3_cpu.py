"""CPU: the host side of the sparse data gradient of a YOLOv3 head conv -- the yardstick of tests/blocks_v3_ref.py against torch.autograd,
yolo_v3_head_dgrad_plan and the case table of tests/blocks_v3_cases.py against each other, every refusal that needs no device, the wide
shapes of the 3 x 3 weight gradient against its plan, yolo_net_block_inputs_v3 and the state layout on the v3 networks with their
refusals, the `head_blocks` train mode's host logic, and the sanitizer run of the host code as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import blocks_v3_cases as cases
import blocks_v3_ref as ref
import tail_ref
import train_v3_ref
from helpers import ROOT
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine


def head_of(grids, A, n_classes):
    return engine.head_desc_v3(grids, [[(1. + a, 2. + a) for a in range(A)] for _ in grids], n_classes)


def plan(grids, A, n_classes, scale, cin, batch):
    return _hip.head_dgrad_plan(head_of(grids, A, n_classes), scale, cin, batch)


def all_cases():
    return cases.DGRAD_CASES + (cases.loop_case(plan),)


def last_error():
    return _hip.lib().yolo_last_error().decode()


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.DGRAD_CASES[:6], ids=lambda c: c[0])
def test_float64_yardstick_equals_autograd(case):
    """Y = leaky(z), L_s = Y W_s^T in float64 under torch.autograd with loss = sum(L_s * G_s), G_s the gathered gradient with +0 in its
    structural zeros: dloss / dz is the D of the definition.  Bound, set before anything here ran: 1e-12 of the largest |D|, the margin of
    the other yardsticks (test_train_tail_cpu.py)."""
    import torch
    import torch.nn.functional as F
    _, grids, A, n_classes, scale, cin, batch = case
    rng = np.random.RandomState(len(case[0]) + cin)
    R, scales = train_v3_ref.scales_of(grids, A)
    width = 5 + n_classes
    table = cases.make_table("full-image", grids, A, batch, rng, scale)
    table[0, scales[scale][0]:scales[scale][0] + A] = (0, cases.MAX_GT, -2)[:A]      # a winner, an entry that names no truth, an ignored row
    G = rng.randn(batch, R, width)
    G[~train_v3_ref.terms(table, width, cases.MAX_GT)] = np.nan                      # the structural zeros are never looked at
    P = batch * scales[scale][1] * scales[scale][2]
    W, z = rng.randn(A * width, cin), rng.randn(P, cin)
    assert np.min(np.abs(z)) > 1e-9
    Gs, _ = ref.gathered(G, table, scales[scale], cases.MAX_GT)
    zt, Wt = torch.from_numpy(z).requires_grad_(), torch.from_numpy(W)
    y = F.leaky_relu(zt, ref.SLOPE)
    ((y @ Wt.T) * torch.from_numpy(Gs)).sum().backward()
    want = zt.grad.numpy()
    got = ref.head_dgrad(G, table, W, scales[scale], cases.MAX_GT, y.detach().numpy(), mode="float64")
    gap, top = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    print("%s: max|ref - autograd| = %.3e = %.3e of max|D| = %.6g" % (case[0], gap, gap / top, top))
    assert gap <= 1e-12 * top
    # the bound's reference is the same function with the slope the device multiplies by: the float32 value of 0.1
    d64, bound = ref.head_dgrad_ref64(G, table, W, scales[scale], cases.MAX_GT, y.detach().numpy())
    same = ref.head_dgrad(G, table, W, scales[scale], cases.MAX_GT, y.detach().numpy(), float(np.float32(ref.SLOPE)), mode="float64")
    assert np.max(np.abs(d64 - same)) <= 1e-12 * top
    # the float32 mode is the same chain rounded per operation, inside the header's bound
    G32, W32 = G.astype(np.float32), W.astype(np.float32)
    d32 = ref.head_dgrad(G32, table, W32, scales[scale], cases.MAX_GT, y.detach().numpy(), mode="float32")
    r64, bound = ref.head_dgrad_ref64(G32, table, W32, scales[scale], cases.MAX_GT, y.detach().numpy())
    assert d32.dtype == np.float32 and np.all(np.abs(d32 - r64) <= bound)


def test_yardstick_skips_structural_zeros_and_multiplies_once():
    grids, A, width = ((1, 1),), 2, 6
    _, scales = train_v3_ref.scales_of(grids, A)
    W = np.arange(1, A * width * 8 + 1, dtype=np.float32).reshape(A * width, 8)
    G = np.full((1, 2, width), np.nan, dtype=np.float32)
    G[0, :, 4] = (2, 3)
    table = np.array([[-1, -2]], dtype=np.int32)
    want = 2 * W[4] + 3 * W[width + 4]
    assert np.array_equal(ref.head_dgrad(G, table, W, scales[0], 8), want[None])
    table[0, 1] = 8                                 # an entry >= max_gt names no truth
    assert np.array_equal(ref.head_dgrad(G, table, W, scales[0], 8), want[None])
    table[0, 1] = 7
    G[0, 1] = 1
    assert np.array_equal(ref.head_dgrad(G, table, W, scales[0], 8), (2 * W[4] + W[width:].sum(axis=0))[None])
    Y = np.array([[0.0, -0.0, -1.0, 1.0, np.nan, 6e-8, -6e-8, np.inf]])
    got = ref.head_dgrad(G, table, W, scales[0], 8, Y)
    plain = ref.head_dgrad(G, table, W, scales[0], 8)
    assert np.array_equal(got, plain * np.array([0.1, 0.1, 0.1, 1, 0.1, 1, 0.1, 1], dtype=np.float32))


# ---- yolo_v3_head_dgrad_plan and the case table --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", all_cases(), ids=lambda c: c[0])
def test_plan_properties(case):
    _, grids, A, n_classes, scale, cin, batch = case
    pl = plan(grids, A, n_classes, scale, cin, batch)
    h, w = grids[scale]
    assert pl["positions"] == batch * h * w and pl["threads"] % 64 == 0 and pl["channels_per_thread"] == 8
    assert pl["tile_cin"] == min(cin, pl["tile_cin"]) and pl["tiles_cin"] == -(-cin // pl["tile_cin"])
    assert pl["threads_per_position"] * pl["channels_per_thread"] == pl["tile_cin"]
    assert pl["positions_per_round"] == pl["threads"] // pl["threads_per_position"] >= 1
    assert pl["positions_per_workgroup"] == pl["rounds"] * pl["positions_per_round"] and pl["loops"] == int(pl["rounds"] > 1)
    assert (pl["workgroups"] - 1) * pl["positions_per_workgroup"] < pl["positions"] <= pl["workgroups"] * pl["positions_per_workgroup"]
    assert pl["lds_bytes"] == A * pl["tile_cin"] * 4 <= 64 * 1024


def test_case_table_crosses_what_it_claims():
    """asserted from the plan, so that a changed constant fails here: a workgroup boundary, a second round of a looping workgroup, a
    second channel tile, an idle thread, every cin / A / C / grid / batch the tests promise, scale 0, a middle and the last scale"""
    table = all_cases()
    plans = {c[0]: plan(*c[1:]) for c in table}
    assert sum(pl["workgroups"] > 1 for pl in plans.values()) >= 6
    loop = plans["cin1024-second-round"]
    assert loop["loops"] == 1 and loop["rounds"] == 2 and loop["workgroups"] > 1
    assert not plan(*cases.loop_case(plan)[1:-1], cases.loop_case(plan)[-1] - 1)["loops"]      # the smallest such batch
    assert plans["cin1032-last-of-2"]["tiles_cin"] == 2 and plans["cin1024-last-of-3"]["tiles_cin"] == 1
    assert plans["cin40-only-scale"]["positions_per_round"] * plans["cin40-only-scale"]["threads_per_position"] < plans["cin40-only-scale"]["threads"]
    assert {c[5] for c in table} == {8, 40, 136, 1024, 1032} and {c[2] for c in table} == {2, 3} and {c[3] for c in table} == {1, 3, 80}
    assert {c[6] for c in cases.DGRAD_CASES} == {1, 2, 3}
    assert {c[1][c[4]] for c in table} == {(1, 1), (3, 5), (13, 13)}
    assert {(c[4], len(c[1])) for c in table} >= {(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3)}
    for c in table:         # a position whose A rows are all winners, in the scale under test; rows beyond max_gt in it
        _, grids, A, _, scale, _, batch = c
        _, scales = train_v3_ref.scales_of(grids, A)
        row0, h, w, na = scales[scale]
        t = cases.make_table("all-anchors", grids, A, batch, np.random.RandomState(1), scale)[:, row0:row0 + h * w * na].reshape(batch, h * w, na)
        assert (((t >= 0) & (t < cases.MAX_GT)).all(axis=2)).sum() == 1
        t = cases.make_table("beyond-max-gt", grids, A, batch, np.random.RandomState(1), scale)[:, row0:row0 + h * w * na]
        assert (t >= cases.MAX_GT).sum() == na and not ((t >= 0) & (t < cases.MAX_GT)).any()
        t = cases.make_table("edges", grids, A, batch, np.random.RandomState(1))
        assert 0 <= t[batch - 1, row0 + h * w * na - 1] < cases.MAX_GT                      # the last row of the last image


def test_plan_at_the_flagship_shapes():
    hd = head_of(((19, 19), (38, 38), (76, 76)), 3, 80)
    for s, cin in enumerate((1024, 512, 256)):
        for batch in (16, 32):
            pl = _hip.head_dgrad_plan(hd, s, cin, batch)
            assert pl["tiles_cin"] == 1 and pl["lds_bytes"] == 3 * cin * 4 <= 12 * 1024 and pl["workgroups"] <= 2048
            assert pl["loops"] == int(pl["positions"] > 2048 * pl["positions_per_round"])


def test_plan_refusals_have_messages():
    lib = _hip.lib()
    pl = _hip.V3DgradPlan()
    hd = head_of(cases.GRIDS3, 3, 3)
    v2 = head_of(cases.GRIDS3, 3, 3)
    v2.version = 2
    for args, text in (((hd, -1, 8, 1), "scale must be 0..2"), ((hd, 3, 8, 1), "scale must be 0..2"), ((hd, 0, 12, 1), "multiple of 8"),
                       ((hd, 0, 0, 1), "multiple of 8"), ((hd, 0, 8, 0), "batch must be at least 1"), ((hd, 2, 8, 1 << 24), "2^30"),
                       ((v2, 0, 8, 1), "the head must be version 3")):
        assert lib.yolo_v3_head_dgrad_plan(C.byref(args[0]), *args[1:], C.byref(pl)) == 1 and text in last_error(), (args[1:], last_error())
        assert last_error().startswith("yolo_v3_head_dgrad_plan: ")
    assert lib.yolo_v3_head_dgrad_plan(C.byref(hd), 0, 8, 1, None) == 1 and lib.yolo_v3_head_dgrad_plan(None, 0, 8, 1, C.byref(pl)) == 1


def test_entry_refusals_need_no_device():
    """the checks run in front of any HIP call: host pointers stand in, nothing is launched"""
    lib = _hip.lib()
    buf = (C.c_float * 64)()
    q = (C.addressof(buf) + 255) & ~255
    hd = head_of(cases.GRIDS3, 3, 3)
    v2 = head_of(cases.GRIDS3, 3, 3)
    v2.version = 2
    names = (("head", hd), ("scale", 1), ("g", q), ("assign", q), ("max_gt", 8), ("b", 2), ("w", q), ("cin", 40), ("y", q), ("dt", _hip.DTYPE_F16),
             ("ld", 48), ("coff", 8), ("istride", 15 * 48), ("slope", 0.1), ("d", q), ("stream", None))

    def dg(**kw):
        args = [kw.get(k, v) for k, v in names]
        return lib.yolo_v3_head_dgrad(C.byref(args[0]), *args[1:])
    for kw, text in (({"g": None}, "null"), ({"assign": None}, "null"), ({"w": None}, "null"), ({"d": None}, "null"),
                     ({"head": v2}, "the head must be version 3"), ({"scale": 3}, "scale must be 0..2"), ({"scale": -1}, "scale must be 0..2"),
                     ({"cin": 36}, "multiple of 8"), ({"max_gt": 0}, "max_gt must be 1..1024"), ({"max_gt": 1025}, "max_gt must be 1..1024"),
                     ({"b": 0}, "batch must be at least 1"), ({"scale": 2, "b": 1 << 24}, "2^30"), ({"w": q + 4}, "16-byte"), ({"d": q + 8}, "16-byte"),
                     ({"g": q + 2}, "not aligned"), ({"ld": 40}, "pixel stride"), ({"coff": -1}, "pixel stride"), ({"istride": 15 * 48 - 9}, "image_stride"),
                     ({"dt": _hip.DTYPE_MXF8}, "dtype"), ({"y": q + 1}, "not aligned")):
        assert dg(**kw) == 1 and text in last_error(), (kw, last_error())
        assert last_error().startswith("yolo_v3_head_dgrad: ")


# ---- yolo_conv3x3_wgrad on wide maps: the shapes against its plan -------------------------------------------------------------------------------
def test_wide_wgrad_shapes_cross_a_chunk_inside_a_row():
    for h, w, batch, cin, cout in cases.WIDE_WGRAD_SHAPES:
        pl = _hip.conv3x3_wgrad_plan(h, w, batch, cin, cout)
        assert pl["n_chunks"] > 1 and pl["positions_per_chunk"] % w, (h, w, pl)       # a chunk ends in the middle of a row
        assert pl["halo_rows"] == pl["tile_positions"] + 2 * w + 2
        # |values| <= 8: every sum of the exact tests stays below 2^24
        assert batch * h * w * 64 < 2 ** 24
    assert {s[1] for s in cases.WIDE_WGRAD_SHAPES} == {26, 38, 76, 80} and {s[2] for s in cases.WIDE_WGRAD_SHAPES} == {1, 2}
    assert {s[3:] for s in cases.WIDE_WGRAD_SHAPES} == {(8, 8), (8, 64), (64, 8), (64, 64)}
    h, w, batch, cin, cout = cases.WIDE_WGRAD_REFUSED
    pl = _hip.Conv3x3WgradPlan()
    assert _hip.lib().yolo_conv3x3_wgrad_plan(h, w, batch, cin, cout, _hip.DTYPE_F16, C.byref(pl)) == 1 and "does not fit LDS" in last_error()


def test_head_block_shapes_have_plans():
    """the 3 x 3 blocks behind the heads of YOLOv3-608 and YOLOv3-tiny-416, at batch 16 and 32"""
    for h, cin, cout in ((19, 512, 1024), (38, 256, 512), (76, 128, 256), (13, 256, 512), (26, 384, 256)):
        for batch in (16, 32):
            pl = _hip.conv3x3_wgrad_plan(h, h, batch, cin, cout)
            assert pl["halo_rows"] == 34 + 2 * h and pl["scratch_bytes"] == pl["n_chunks"] * cout * (9 * cin + 1) * 4


# ---- the whole step: the yardstick's float64 loop chooses the learning rate ---------------------------------------------------------------------
def test_float64_loop_lowers_the_loss_at_every_step_at_the_rate_the_gpu_test_runs():
    """blocks_v3_ref.blocks_train_loop in float64 on the case of the GPU test's twenty steps (YOLOv3 at 64 x 64, float32 storage, batch 3),
    the block inputs from the oracle's forward pass: the loss falls at every step at cases.TRAIN_LR, which is why the GPU test runs at that
    rate.  (At ten times the rate, the shipped config's 1e-4, the same loop reaches 11.3 in sixteen steps and then rises for two: Adam's
    first steps move every one of a block's 4.7 M weights by about lr whatever its gradient.  Not asserted here: it is a second 5 s loop.)"""
    from helpers import to_oracle
    from oracle import forward_ref
    from tensorflow_yolo_amd.net import evaluate as yeval, synth
    net = v3.create_network(np.reshape(cases.TRAIN_ANCHORS, [-1, 2]), cases.TRAIN_NAMES, False, input_shape=cases.TRAIN_HW + (3,))
    weights = synth.darknet_stream(net, seed=cases.TRAIN_WEIGHT_SEED, num_classes=len(cases.TRAIN_NAMES))
    x = synth.synthetic_input(cases.TRAIN_BATCH, cases.TRAIN_HW[0], cases.TRAIN_HW[1], 3, seed=cases.TRAIN_INPUT_SEED)
    layers = to_oracle(net)
    # the input of the conv in front of each head conv
    idx = [net[i - 1].inputs[0].index for i, l in enumerate(net) if isinstance(l, PL.conv2d_bn_act) and i + 1 < len(net) and isinstance(net[i + 1], PL.yolo_layer)]
    _, kept = forward_ref.forward(layers, weights, x, keep=set(idx))
    X3s = [kept[i] for i in idx]
    assert [a.shape for a in X3s] == [(3, 2, 2, 512), (3, 4, 4, 256), (3, 8, 8, 128)]
    gt, counts = yeval.pack_gts(cases.TRAIN_TRUTHS, 3)
    args = cases.train_loop_args(net, weights, X3s, engine.head_desc_v3(net[-1].yolos))
    l64 = ref.blocks_train_loop(*args, gt, counts, cases.TRAIN_LR, cases.TRAIN_STEPS, np.float32, mode="float64")[0]
    print("float64:", " ".join("%.4f" % v for v in l64))
    assert np.isfinite(l64).all() and all(b < a for a, b in zip(l64, l64[1:])), l64
    assert l64[-1] < 0.6 * l64[0]


# ---- the sanitizer run ----------------------------------------------------------------------------------------------------------------------
def test_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    """train3_tail_host.cpp with a program of its own (train3_tail_host_check.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: no
    HIP, no device, nothing preloaded"""
    csrc = os.path.join(ROOT, "tensorflow-yolo_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc, "san-blocks", "OBJDIR=" + str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "train3_tail_host_check OK" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


# ---- the blocks behind the heads of a net: views, layout, refusals (host only) ----------------------------------------------------------------
from tensorflow_yolo_amd import launcher                                                      # noqa: E402
from tensorflow_yolo_amd.net import layers as PL, train as ytrain, v2, v3                     # noqa: E402
from helpers import new_graph                                                                 # noqa: E402

NAMES3 = ["a", "b", "c"]
TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
V2_ANCHORS = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071]
# (maker, anchors, input, grid of scale 0, (cin3, cout3) per scale): the five shapes the blocks were probed on
SHAPES = {"v3-608": (v3.create_network, V3_ANCHORS, (608, 608), (19, 19), ((512, 1024), (256, 512), (128, 256))),
          "v3-64": (v3.create_network, V3_ANCHORS, (64, 64), (2, 2), ((512, 1024), (256, 512), (128, 256))),
          "v3-spp-608": (v3.create_spp_network, V3_ANCHORS, (608, 608), (19, 19), ((512, 1024), (256, 512), (128, 256))),
          "v3-tiny-416": (v3.create_tiny_network, TINY_ANCHORS, (416, 416), (13, 13), ((256, 512), (384, 256))),
          "v3-tiny-96x160": (v3.create_tiny_network, TINY_ANCHORS, (96, 160), (3, 5), ((256, 512), (384, 256)))}
BLOCK_FIELDS = ("w", "b", "m_w", "v_w", "m_b", "v_b", "dw", "db", "w3", "beta", "m_w3", "v_w3", "m_beta", "v_beta", "dw3", "dbeta", "scale64", "scale32", "mean")


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_block_inputs_and_state_layout_of_the_v3_networks(name, dtype):
    make, anchors, hw, g0, chans = SHAPES[name]
    mb = 2
    net = make(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=hw + (3,))
    p = engine.Plan(net, dtype=dtype, max_batch=mb, streams=1)
    bviews, hviews = p.block_inputs_v3()
    ns = len(chans)
    grids = [(g0[0] << s, g0[1] << s) for s in range(ns)]
    assert [(v.cin, v.h, v.w) for v in bviews] == [(c3,) + g for (c3, _), g in zip(chans, grids)]
    assert [(v.cin, v.h, v.w) for v in hviews] == [(o3,) + g for (_, o3), g in zip(chans, grids)]
    assert [(v.cin, v.h, v.w, v.offset) for v in hviews] == [(v.cin, v.h, v.w, v.offset) for v in p.head_inputs_v3()]
    esz = 4 if dtype == "fp32" else 2
    spans = []
    for v, (h, w) in zip(list(bviews) + list(hviews), grids + grids):
        assert v.dtype == (_hip.DTYPE_F32 if dtype == "fp32" else _hip.DTYPE_F16)
        assert v.ld >= v.coff + v.cin and v.image_stride >= h * w * v.ld and v.offset % 256 == 0
        assert v.offset + esz * mb * v.image_stride <= p.workspace_bytes                 # inside the workspace
        spans.append((v.offset, v.offset + esz * mb * v.image_stride))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                             # no two of them share bytes
    lay = p.blocks_train_layout_v3()
    heads, blocks = ytrain.head_convs_v3(net), ytrain.block_convs_v3(net)
    assert lay.n_scales == ns and [(lay.cin3[s], lay.cout3[s]) for s in range(ns)] == list(chans)
    assert [lay.cin[s] for s in range(ns)] == [o3 for _, o3 in chans] and [lay.cout[s] for s in range(ns)] == [24] * ns
    assert [int(lay.bias_src[s]) for s in range(ns)] == [pos for pos, _, _ in heads]        # the stream positions of the Python layer list
    assert [int(lay.block_src[s]) for s in range(ns)] == [pos for pos, _, _ in blocks]
    assert [(c3, i3) for _, c3, i3 in blocks] == [(o3, c3) for c3, o3 in chans]
    offs = [int(getattr(lay, k + "_offset")[s]) for s in range(ns) for k in BLOCK_FIELDS]
    offs += [int(lay.d_offset), int(lay.grad_offset), int(lay.assign_offset), int(lay.parts_offset), int(lay.images_offset), int(lay.scratch_offset)]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and offs[0] == 0 and len(set(offs)) == len(offs)
    R, parts = engine.v3_loss_rows(p.head)
    # D holds the largest scale at the full batch
    assert lay.grad_offset - lay.d_offset >= mb * max(h * w * o3 for (h, w), (_, o3) in zip(grids, chans)) * 4
    assert lay.assign_offset - lay.grad_offset >= mb * R * 8 * 4 and lay.parts_offset - lay.assign_offset >= mb * R * 4
    assert lay.images_offset - lay.parts_offset >= mb * parts * 56 and lay.scratch_offset - lay.images_offset >= mb * 56
    # the scratch holds the largest split of any batch up to max_batch, of the heads' plan and of every block's
    want = max([_hip.v3_head_wgrad_plan(p.head, [o3 for _, o3 in chans], b)["scratch_bytes"] for b in range(1, mb + 1)] +
               [_hip.conv3x3_wgrad_plan(h, w, b, c3, o3)["scratch_bytes"] for b in range(1, mb + 1) for (h, w), (c3, o3) in zip(grids, chans)])
    assert lay.scratch_bytes == want
    assert lay.total_bytes >= lay.scratch_offset + lay.scratch_bytes and lay.total_bytes == _hip.lib().yolo_net_blocks_train_v3_bytes(p.handle)


def test_blocks_net_refusals_without_a_device():
    lib = _hip.lib()
    bv, hv, n = (_hip.TensorView * 4)(), (_hip.TensorView * 4)(), C.c_int32(0)
    call = lambda p: lib.yolo_net_block_inputs_v3(p.handle, bv, hv, C.byref(n))
    net = v3.create_tiny_network(np.reshape(TINY_ANCHORS, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3))
    # an MXFP8 plan whose blocks are MX convs (YOLO_ERR_STATE)
    p = engine.Plan(net, dtype="mxfp8", max_batch=2, streams=1)
    assert call(p) == 5 and "MXFP8 conv" in last_error() and last_error().startswith("yolo_net_block_inputs_v3: scale 0: ")
    assert lib.yolo_net_blocks_train_v3_bytes(p.handle) == 0 and "MXFP8 conv" in last_error()
    assert len(p.head_inputs_v3()) == 2                                                    # head-only training still takes this plan
    # two stream parts (YOLO_ERR_STATE)
    p2 = engine.Plan(net, dtype="fp16", max_batch=4, streams=2)
    assert call(p2) == 5 and "stream parts" in last_error() and "yolo_net_set_streams(net, 1)" in last_error()
    # a v2 net: no head set, then a version 2 head (YOLO_ERR_ARG); yolo_net_tail_inputs keeps refusing a v3 net with its message
    pv2 = engine.Plan(v2.create_tiny_network(np.reshape(V2_ANCHORS, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3)), dtype="fp16", max_batch=1, streams=1)
    assert call(pv2) == 5 and "head geometry not set" in last_error()
    pv2.set_head(engine.head_desc_v2(3, 5, V2_ANCHORS, 3))
    assert call(pv2) == 1 and "yolo_net_block_inputs_v3: the head must be version 3" in last_error()
    good = engine.Plan(net, dtype="fp16", max_batch=2, streams=1)
    views = [_hip.TensorView(), _hip.TensorView()]
    assert lib.yolo_net_tail_inputs(good.handle, C.byref(views[0]), C.byref(views[1])) == 1 and "a v3 network has no tail of this kind" in last_error()
    # hand-built v3-style graphs: the block behind the head conv carries a residual; is 1 x 1
    for kind, word in (("residual", "scale 0: the conv behind the head conv carries a residual"),
                       ("1x1", "scale 0: the conv behind the head conv must be 3 x 3 / stride 1")):
        g = new_graph(16, 16, 16)
        g.append(PL.conv2d_bn_act(g[-1].out, 16, 3, 1))
        before = g[-1]
        g.append(PL.conv2d_bn_act(g[-1].out, 16, 1 if kind == "1x1" else 3, 1))
        if kind == "residual":
            g.append(PL.shortcut(g[-1].out, before.out))
        g.append(PL.conv2d_bn_act(g[-1].out, 24, 1, 1, use_batch_normalization=False, activation_fn="linear"))
        g.append(PL.yolo_layer(g[-1].out, np.reshape([10, 14, 23, 27, 37, 58], [-1, 2]), 3, (16, 16)))
        g.append(PL.detection_layer([g[-1]]))
        pg = engine.Plan(g, dtype="fp16", max_batch=2, streams=1)
        assert call(pg) == 1 and word in last_error(), (kind, last_error())
    # null arguments; the step entries check the net's blocks before anything else, and a null state
    assert lib.yolo_net_block_inputs_v3(good.handle, None, hv, C.byref(n)) == 1 and lib.yolo_net_block_inputs_v3(None, bv, hv, C.byref(n)) == 1
    assert call(good) == 0 and n.value == 2
    for name in ("yolo_net_train_blocks_step_v3", "yolo_net_train_blocks_step_v3_u8"):
        fn = getattr(lib, name)
        assert fn(p.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096, 1e-3, 4096, None) == 5 and last_error().startswith(name + ": ") and "MXFP8 conv" in last_error()
        assert fn(good.handle, 4096, 1, 4096, 4096, 1, 0.7, None, 1e-3, 4096, None) == 1 and "null state (yolo_net_blocks_train_v3_init)" in last_error()
        assert fn(good.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096 + 8, 1e-3, 4096, None) == 1 and "256-byte aligned" in last_error()
        assert fn(good.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096, 1e-3, 4096, None) == 5 and "weights not loaded" in last_error()
    ptrs = (C.c_void_p * 4)(4096, 4096, 4096, 4096)
    assert lib.yolo_net_blocks_train_v3_init(good.handle, 4096, 1 << 30, ptrs, ptrs, ptrs) == 5 and "weights not loaded" in last_error()
    assert lib.yolo_net_blocks_train_v3_init(good.handle, 4096, 16, ptrs, ptrs, ptrs) == 1 and "state too small" in last_error()
    assert lib.yolo_net_blocks_train_v3_init(good.handle, None, 1 << 30, ptrs, ptrs, ptrs) == 1


# ---- train mode: parsing, the shipped file, the stream --------------------------------------------------------------------------------------
def test_train_layers_head_blocks_parsing_and_refusals():
    assert ytrain.train_layers({"train_layers": " Head_Blocks "}) == "head_blocks" and ytrain.train_option({"train_layers": "head_blocks"}) is True
    for word in ("tails", "all", "blocks"):
        with pytest.raises(ValueError, match="^train_layers must be head .*head_blocks"):
            ytrain.train_layers({"train_layers": word})
    for version in ("v3", "v3-spp", "v3-tiny"):
        assert ytrain.check_params({"train_layers": "head_blocks"}, version) == 0.0
    for version in ("v2", "v2-tiny"):
        with pytest.raises(ValueError, match="train_layers = head_blocks trains .* a %s network takes train_layers = tail" % version):
            ytrain.check_params({"train_layers": "head_blocks"}, version)
    with pytest.raises(ValueError, match="ignore_thresh must be in"):
        ytrain.check_params({"train_layers": "head_blocks", "ignore_thresh": "0"}, "v3")
    with pytest.raises(ValueError, match="augment_probability must be 0"):
        ytrain.check_params({"train_layers": "head_blocks", "augment_probability": "0.5"}, "v3")
    assert ytrain.check_params({"train_layers": "head_blocks", "augment_probability": "0.5", "augment": "device"}, "v3") == 0.5


def test_shipped_head_blocks_config():
    cfg = launcher.read_config(os.path.join(ROOT, "tensorflow-yolo_amd", "config", "yolo_3_head_blocks_train.ini"))
    params = dict(cfg["COMMON"], **cfg["TRAIN"])
    assert ytrain.train_layers(params) == "head_blocks" and ytrain.check_params(params, params["version"]) == 0.0
    assert params["version"] == "v3" and params["dtype"] == "fp16" and int(params["pretrained_classes"]) == 80
    assert "yolo_3_head_blocks_train.ini" in open(os.path.join(ROOT, "README.md")).read()


def test_block_stream_split_and_replace_round_trip():
    for make, anchors, want in ((v3.create_tiny_network, TINY_ANCHORS, [(512, 256), (256, 384)]),
                                (v3.create_network, V3_ANCHORS, [(1024, 512), (512, 256), (256, 128)])):
        net = make(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3))
        heads, blocks = ytrain.head_convs_v3(net), ytrain.block_convs_v3(net)
        need = sum(l.weight_count() for l in net if hasattr(l, "weight_count"))
        assert [(c3, i3) for _, c3, i3 in blocks] == want
        # a block ends exactly where its head conv begins
        assert [pos + c3 * (4 + 9 * i3) for pos, c3, i3 in blocks] == [pos for pos, _, _ in heads]
        body = np.random.RandomState(8).randn(need).astype(np.float32)
        pieces = ytrain.split_blocks(body, blocks)
        ws, bs = ytrain.split_heads(body, heads)
        for (pos, c3, i3), piece in zip(blocks, pieces):
            assert piece.size == c3 * (4 + 9 * i3) and piece.tobytes() == body[pos:pos + piece.size].tobytes()
        k3 = [piece[4 * c3:].reshape(c3, i3, 3, 3) for (_, c3, i3), piece in zip(blocks, pieces)]
        betas = [piece[:c3] for (_, c3, _), piece in zip(blocks, pieces)]
        assert ytrain.replace_head_blocks(body, blocks, heads, k3, betas, ws, bs).tobytes() == body.tobytes()
        # the master order [o][t][c] and back is the conversion of the v2 tail
        otc = tail_ref.stream_to_otc(pieces[0][4 * blocks[0][1]:], blocks[0][1], blocks[0][2])
        assert tail_ref.otc_to_stream(otc).tobytes() == pieces[0][4 * blocks[0][1]:].tobytes()
        out = ytrain.replace_blocks(body, blocks, [k + 1 for k in k3], [b + 2 for b in betas])
        changed = np.flatnonzero(out != body)
        for pos, c3, i3 in blocks:          # gamma and the moving statistics stay
            assert not ((changed >= pos + c3) & (changed < pos + 4 * c3)).any()
        assert len(changed) == sum(c3 * (1 + 9 * i3) for _, c3, i3 in blocks)

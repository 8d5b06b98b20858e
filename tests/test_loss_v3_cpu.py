"""CPU: the YOLOv3 loss (include/yolo_hip.h: yolo_v3_loss, yolo_v3_loss_grad).  The yardstick tests/loss_v3_ref.py against torch autograd
and central differences; the properties the GPU cases of tests/loss_v3_cases.py must have for the device tests to be allowed to compare
tables as integers (no IoU near the threshold) and values by the project's rules (non-degenerate groups); every argument error and its
message through the library without a device; yolo_v3_loss_rows on the networks' heads; the sanitizer run of the host code as a program of
its own; and the refusals of the YOLOv2 entries for a version 3 head, which stay."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loss_v3_cases as cases
import loss_v3_ref
from helpers import ROOT
from oracle import cases as ocases
from tensorflow_yolo_amd import _hip, yolo_v3_loss
from tensorflow_yolo_amd.net import engine, v2, v3

NAMES3 = ["a", "b", "c"]
NAMES80 = ["c%d" % i for i in range(80)]
TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]


def last_error():
    return _hip.lib().yolo_last_error().decode()


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def torch_loss(x, ref, grids, anchors, C_, gt):
    """the definition's total as a float64 torch expression of the logits x [B, R, 5 + C], on the table and targets of the yardstick"""
    import torch
    import torch.nn.functional as F
    R, scales = loss_v3_ref.rows_of(grids, anchors)
    B = x.shape[0]
    total = x.new_zeros(())
    for b in range(B):
        for r in range(R):
            g = int(ref["table"][b, r])
            if g == -2:
                continue
            t = x[b, r]
            if g == -1:
                total = total + F.softplus(t[4])
                continue
            s, cr, cc, a = loss_v3_ref.locate(scales, r)
            tx, ty, tw, th, m = loss_v3_ref.targets(gt[b, g], scales[s], cr, cc, anchors[s][a], np.float64)
            onehot = torch.zeros(C_, dtype=torch.float64)
            onehot[int(gt[b, g]["class_idx"])] = 1
            total = total + m * (F.softplus(t[0]) - tx * t[0] + F.softplus(t[1]) - ty * t[1]) + m * 0.5 * ((t[2] - tw) ** 2 + (t[3] - th) ** 2)
            total = total + F.softplus(t[4]) - t[4] + (F.softplus(t[5:]) - onehot * t[5:]).sum()
    return total / B


def test_yardstick_gradient_is_autograd_of_its_loss():
    import torch
    logits, gt, counts, grids, anchors, C_ = cases.make_case("three-scales")
    r64 = cases.yardsticks("three-scales")[0]
    x = torch.from_numpy(logits.astype(np.float64)).requires_grad_()
    total = torch_loss(x, r64, grids, anchors, C_, gt)
    assert abs(float(total.detach()) - r64["totals"]["loss"]) <= 1e-12 * abs(r64["totals"]["loss"])
    total.backward()
    got, want = x.grad.numpy(), r64["grad"]
    scale = np.abs(want).max()
    print("largest |autograd - closed form| / max|G| = %.3e" % (np.abs(got - want).max() / scale))
    assert np.abs(got - want).max() <= 1e-12 * scale
    assert (want[r64["table"] == -2] == 0).all()


def test_yardstick_gradient_against_central_differences():
    """on the smallest three-scale case, 60 elements of winner, plain and ignored rows: (L(t + e) - L(t - e)) / 2e with e = 1e-5 in float64,
    relative to the largest gradient element"""
    logits, gt, counts, grids, anchors, C_ = cases.make_case("three-scales")
    r64 = cases.yardsticks("three-scales")[0]
    table, grad = r64["table"], r64["grad"]
    rng = np.random.RandomState(3)
    picks = []
    for kind in (lambda v: v >= 0, lambda v: v == -1, lambda v: v == -2):
        rows = np.argwhere(kind(table))
        for i in rng.choice(len(rows), size=min(20, len(rows)), replace=False):
            picks.append((int(rows[i][0]), int(rows[i][1]), int(rng.randint(0, 5 + C_))))
    x = logits.astype(np.float64)
    scale, eps, worst = np.abs(grad).max(), 1e-5, 0.0
    import torch
    for b, r, j in picks:
        vals = []
        for sign in (1., -1.):
            y = x.copy()
            y[b, r, j] += sign * eps
            vals.append(float(torch_loss(torch.from_numpy(y[b:b + 1]), {"table": table[b:b + 1]}, grids, anchors, C_, gt[b:b + 1])) / x.shape[0])
        worst = max(worst, abs((vals[0] - vals[1]) / (2 * eps) - grad[b, r, j]) / scale)
    print("largest |central difference - G| / max|G| = %.3e over %d elements" % (worst, len(picks)))
    assert worst <= 1e-5


# ---- the properties of the GPU cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.GPU_CASES))
def test_case_properties(name):
    r64, r32 = cases.yardsticks(name)
    # no (row, truth) IoU of either mode near the threshold -- every row, winners included; so both modes, and the device, agree on the table
    print("%s: smallest |iou - thresh| float64 %.3e float32 %.3e" % (name, r64["margin"], r32["margin"]))
    assert r64["margin"] > cases.MARGIN and r32["margin"] > cases.MARGIN
    assert np.array_equal(r64["table"], r32["table"])
    table = r32["table"]
    kinds = ((table >= 0).sum(), (table == -1).sum(), (table == -2).sum())
    if table.shape[1] >= 3:         # (the smallest case has ONE row, a winner: it cannot hold the three kinds)
        assert all(k > 0 for k in kinds), kinds
    else:
        assert kinds == (1, 0, 0)
    for group, fig in cases.group_figures(r64["grad"], r32["grad"]).items():
        if fig["M"] > 0:
            assert fig["E_32"] >= 0.25 * fig["ulp"], (name, group, fig)
    assert np.isfinite(r32["grad"]).all() and np.isfinite(r32["sums"]).all()


def test_case_shapes_are_what_they_are_for():
    lib = _hip.lib()
    rows, parts = C.c_int64(), C.c_int32()
    grids, A, C_, B, _, _ = cases.GPU_CASES["parts"]
    hd = engine.head_desc_v3(grids, cases.anchors_for(grids, A), C_)
    assert lib.yolo_v3_loss_rows(C.byref(hd), C.byref(rows), C.byref(parts)) == 0
    assert parts.value >= 3 and rows.value == cases.rows_for(grids, A)
    assert rows.value > (parts.value - 1) * 1024 and rows.value < parts.value * 1024        # the last part is partial
    assert cases.GPU_CASES["long-class-row"][2] > 128 and cases.GPU_CASES["batch-65"][3] == 65
    assert (5 + cases.GPU_CASES["row-of-85"][2]) % 4 != 0
    logits, gt, counts, _, _, _ = cases.make_case("truth-edges")
    assert counts.tolist() == [0, 1, 1024] and gt.shape[1] == _hip.EVAL_MAX_GT


def test_descent_losses_are_the_yardsticks():
    got = cases.descent_losses(steps=2)
    assert np.allclose(got, cases.DESCENT_LOSSES[:3], rtol=0, atol=5e-5), got
    assert len(cases.DESCENT_LOSSES) == cases.DESCENT_STEPS + 1 and all(b < a for a, b in zip(cases.DESCENT_LOSSES, cases.DESCENT_LOSSES[1:]))


# ---- the library without a device -----------------------------------------------------------------------------------------------------------
def v3_heads():
    a3 = np.reshape(ocases.COCO_V3_ANCHORS, [-1, 2])
    return {"v3-608": v3.create_network(a3, NAMES80, False, input_shape=(608, 608, 3)),
            "v3-416": v3.create_network(a3, NAMES80, False, input_shape=(416, 416, 3)),
            "v3-spp-608": v3.create_spp_network(a3, NAMES80, False, input_shape=(608, 608, 3)),
            "v3-tiny-416": v3.create_tiny_network(np.reshape(TINY_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(416, 416, 3))}


def test_rows_and_parts_of_the_networks():
    lib = _hip.lib()
    want = {"v3-608": (22743, 23), "v3-416": (10647, 11), "v3-spp-608": (22743, 23), "v3-tiny-416": (2535, 3)}
    for name, net in v3_heads().items():
        hd = engine.head_desc_v3(net[-1].yolos)
        assert engine.v3_loss_rows(hd) == want[name], name
    v2_head = engine.head_desc_v2(13, 13, [1, 1, 2, 2, 3, 3, 4, 4, 5, 5], 80)      # the fifth network, YOLOv2: refused
    rows, parts = C.c_int64(), C.c_int32()
    assert lib.yolo_v3_loss_rows(C.byref(v2_head), C.byref(rows), C.byref(parts)) == 1
    assert last_error() == "yolo_v3_loss_rows: the head must be version 3"
    assert lib.yolo_v3_loss_rows(None, C.byref(rows), C.byref(parts)) == 1 and "null argument" in last_error()
    # plain numbers give the same head as the layers
    net = v3_heads()["v3-tiny-416"]
    a = engine.head_desc_v3(net[-1].yolos)
    b = engine.head_desc_v3([(y.h, y.w) for y in net[-1].yolos], [y.anchors for y in net[-1].yolos], 80)
    assert bytes(a) == bytes(b)


def test_argument_errors_and_their_messages():
    lib = _hip.lib()
    grids = ((2, 3), (4, 6))
    hd = engine.head_desc_v3(grids, cases.anchors_for(grids, 3), 3)
    p, q = 4096, 8192
    good = [C.byref(hd), p, 2, p, p, 8, 0.7, p, p, p, p, None]
    for entry, args in (("yolo_v3_loss", good), ("yolo_v3_loss_grad", good[:11] + [q, None])):
        fn = getattr(lib, entry)

        def call(at, value):
            a = list(args)
            a[at] = value
            return fn(*a)
        for at in [0, 1, 3, 4, 7, 8, 9, 10] + ([11] if entry.endswith("grad") else []):
            assert call(at, None) == 1 and last_error() == entry + ": null argument", (entry, at, last_error())
        assert call(2, 0) == 1 and last_error() == entry + ": batch must be at least 1"
        for bad in (0, _hip.EVAL_MAX_GT + 1):
            assert call(5, bad) == 1 and last_error() == entry + ": max_gt must be 1..1024"
        for bad in (0.0, -0.1, 1.5, float("nan")):
            assert call(6, bad) == 1 and last_error() == entry + ": ignore_thresh must be in (0, 1]"
        v2_head = engine.head_desc_v2(4, 4, [1, 1, 2, 2], 3)
        assert call(0, C.byref(v2_head)) == 1 and last_error() == entry + ": the head must be version 3"
        for field in ("h", "w", "n_anchors"):
            bad = engine.head_desc_v3(grids, cases.anchors_for(grids, 3), 3)
            getattr(bad, field)[1] = 0
            assert call(0, C.byref(bad)) == 1 and last_error().startswith(entry + ": scale 1: h, w and n_anchors must be at least 1"), last_error()
        bad = engine.head_desc_v3(grids, cases.anchors_for(grids, 3), 3)
        bad.n_scales = 5
        assert call(0, C.byref(bad)) == 1 and "n_scales must be 1..4" in last_error()
        bad.n_scales, bad.n_classes = 2, 0
        assert call(0, C.byref(bad)) == 1 and "n_classes must be at least 1" in last_error()
    assert lib.yolo_v3_loss_grad(*(good[:11] + [p, None])) == 1
    assert last_error() == "yolo_v3_loss_grad: grad_dev must not be logits_dev (the gradient is not computed in place)"


def test_net_entries_without_a_device():
    lib = _hip.lib()
    p3 = engine.Plan(v3.create_tiny_network(np.reshape(TINY_ANCHORS, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3)), dtype="fp16", max_batch=1,
                     streams=1)
    for entry in ("yolo_net_loss_v3", "yolo_net_loss_v3_u8"):
        fn = getattr(lib, entry)
        assert fn(None, 4096, 1, 4096, 4096, 1, 0.7, 4096, 4096, 4096, 4096, None) == 1 and last_error() == entry + ": null argument"
        assert fn(p3.handle, 4096, 1, 4096, 4096, 1, 0.7, None, 4096, 4096, 4096, None) == 1 and last_error() == entry + ": null argument"
        assert fn(p3.handle, 4096, 1, 4096, 4096, 1, 0.0, 4096, 4096, 4096, 4096, None) == 1 and "ignore_thresh" in last_error()
        assert fn(p3.handle, 4096, 0, 4096, 4096, 1, 0.7, 4096, 4096, 4096, 4096, None) == 1 and "batch must be at least 1" in last_error()
        assert fn(p3.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096, 4096, 4096, 4096, None) == 5 and "weights not loaded" in last_error()
        # a v2 net is refused with the new message; a net whose head was never set is told so first
        anchors = [1.3221, 1.73145, 3.19275, 4.00944]
        net = v2.create_tiny_network(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3))
        unset = engine.Plan(net, dtype="fp16", max_batch=1, streams=1)
        assert fn(unset.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096, 4096, 4096, 4096, None) == 5 and "head geometry not set" in last_error()
        unset.set_head(engine.head_desc_v2(3, 5, anchors, 3))
        assert fn(unset.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096, 4096, 4096, 4096, None) == 1
        assert last_error() == entry + ": the head must be version 3"


def test_the_old_entries_still_refuse_a_v3_head():
    lib = _hip.lib()
    grids = ((2, 3), (4, 6))
    hd = engine.head_desc_v3(grids, cases.anchors_for(grids, 3), 3)
    assert lib.yolo_v2_loss(C.byref(hd), 4096, 1, 4096, 4096, 1, 4096, None, 4096, None) == 1
    assert "the reference has a loss for YOLOv2 only" in last_error()
    assert lib.yolo_v2_loss_grad(C.byref(hd), 4096, 1, 4096, 4096, 1, 4096, 4096, 4096, 8192, None) == 1
    assert "the reference has a loss for YOLOv2 only" in last_error()
    p3 = engine.Plan(v3.create_tiny_network(np.reshape(TINY_ANCHORS, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3)), dtype="fp16", max_batch=1,
                     streams=1)
    for entry in ("yolo_net_loss", "yolo_net_loss_u8"):
        assert getattr(lib, entry)(p3.handle, 4096, 1, 4096, 4096, 1, 4096, None, 4096, None) == 1
        assert "the reference has a loss for YOLOv2 only" in last_error()
    assert lib.yolo_net_train_head_step(p3.handle, 4096, 1, 4096, 4096, 1, 4096, 1e-3, 4096, None) == 1


def test_the_op_validates_its_arguments():
    import torch
    grids = ((2, 3), (4, 6))
    anchors = cases.anchors_for(grids, 3)
    x = torch.zeros((1, 90, 8))
    with pytest.raises(ValueError, match="float32 device tensor"):
        yolo_v3_loss(x, [[]], grids, anchors, 3)
    with pytest.raises(ValueError, match="float32 device tensor"):
        yolo_v3_loss(x.numpy(), [[]], grids, anchors, 3)
    with pytest.raises(ValueError, match=r"expected \[B, 90, 8\]"):
        yolo_v3_loss(torch.zeros((1, 89, 8)), [[]], grids, anchors, 3)
    with pytest.raises(ValueError, match="as many anchor lists"):
        yolo_v3_loss(x, [[]], grids, anchors[:1], 3)


def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """loss3_host.cpp (the geometry and every argument check in front of a launch) with loss3_host_check.cpp, a program with its own main,
    built with -fsanitize=address,undefined and run on the CPU"""
    csrc = os.path.join(ROOT, "tensorflow-yolo_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc, "san-loss3", "OBJDIR=" + str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "loss3_host_check OK" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr

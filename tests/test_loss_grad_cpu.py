"""CPU: the yardstick of the loss gradient (tests/loss_grad_ref.py) against torch autograd on an independent float64 restatement of the
loss, against central differences of loss_ref.loss, and on engineered cases (a perfect match: every tie bracket; touching boxes; disjoint
boxes; structural zeros); the host-side argument checks of yolo_v2_loss_grad; the argument checks of lossfn.yolo_v2_loss.  No device call
is made.

Bounds, set before anything here was written: autograd max|g_ref - g_autograd| <= 1e-6 * max|g| (random inputs have no ties; measured
here at most 1.9e-16 of max|g| on the five shapes, seed 7); the restated loss within 1e-9 relative of
loss_ref.loss; central differences (step 2^-10, the six largest elements of each shape) within 1e-4 relative (measured at most 2.2e-6); the hand values of the
engineered cases within 1e-12 relative.

One structural zero cannot hold in float64 as it does in float32: at t4 = -100 float32 has po = 1 / (1 + inf) = 0, float64 has
po = 3.7e-44, so G[4] = 2 po^2 (1 - po) / B = 2.8e-87 / B there.  That element is compared with its closed form in float64 mode and with
0 in float32 mode (where the device arithmetic lives); t4 = +100 is 0 in both."""
import ctypes as C
import functools

import numpy as np
import pytest

import loss_grad_cases
import loss_grad_ref
import loss_ref
from loss_grad_cases import ANCHORS8, random_case, raw_gts
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine, lossfn

SHAPES = [(1, 1, 1, 1, 1), (4, 4, 5, 20, 3), (3, 5, 2, 3, 2), (13, 13, 5, 80, 2), (7, 7, 8, 1, 9)]       # (h, w, A, C, B)
IDS = lambda s: "x".join(str(v) for v in s)


@functools.lru_cache(maxsize=None)
def yardstick(shape, mode="float64"):
    """computed once per shape and mode, shared, left unchanged"""
    h, w, A, n_classes, _ = shape
    logits, gt, counts = random_case(shape, 7)
    g = loss_grad_ref.grad(logits, h, w, ANCHORS8[:2 * A], n_classes, gt, counts, mode=mode)
    g.setflags(write=False)
    return g


def torch_loss(logits, h, w, anchors, n_classes, gt, counts):
    """an independent restatement of the loss for autograd: dense float64 torch tensors, masks from the winner table, one expression
    per term.  -> (loss tensor, the leaf it depends on)"""
    import torch
    anchors = np.reshape(np.asarray(anchors, dtype=np.float64), [-1, 2])
    A = len(anchors)
    logits = np.asarray(logits, dtype=np.float32).reshape(-1, h, w, A, 5 + n_classes)
    B = logits.shape[0]
    table, _, _ = loss_ref.assign(h, w, anchors, n_classes, gt, counts)
    on_slot = np.zeros((B, h, w, A), dtype=bool)
    truth = np.ones((B, h, w, A, 4))
    label = np.zeros((B, h, w, A), dtype=np.int64)
    for b, r, c in zip(*np.nonzero(table >= 0)):
        win = int(table[b, r, c])
        g, a = gt[b, win >> 3], win & 7
        on_slot[b, r, c, a] = True
        truth[b, r, c, a] = [np.float32(np.float64(g["x"]) * w), np.float32(np.float64(g["y"]) * h), np.float32(np.float64(g["w"]) * w),
                             np.float32(np.float64(g["h"]) * h)]
        label[b, r, c, a] = int(g["class_idx"])
    t = torch.tensor(logits.astype(np.float64), requires_grad=True)
    prior = torch.tensor(anchors.astype(np.float32).astype(np.float64))
    tr, m = torch.tensor(truth), torch.tensor(on_slot)
    on_cell = torch.tensor(np.broadcast_to((table >= 0)[..., None], on_slot.shape).copy())
    col = torch.arange(w, dtype=torch.float64).view(1, 1, w, 1)
    row = torch.arange(h, dtype=torch.float64).view(1, h, 1, 1)
    ctr = torch.stack([torch.sigmoid(t[..., 0]) + col, torch.sigmoid(t[..., 1]) + row], dim=-1)
    size = torch.exp(t[..., 2:4]) * prior
    conf = torch.sigmoid(t[..., 4])
    lo = torch.maximum(ctr - size / 2, tr[..., 0:2] - tr[..., 2:4] / 2)
    hi = torch.minimum(ctr + size / 2, tr[..., 0:2] + tr[..., 2:4] / 2)
    ov = torch.clamp(hi - lo, min=0)
    shared = ov[..., 0] * ov[..., 1]
    iou = shared / (size[..., 0] * size[..., 1] + tr[..., 2] * tr[..., 3] - shared)
    xy = ((tr[..., 0:2] - ctr) ** 2).sum(-1)[m].sum()
    wh = ((torch.sqrt(tr[..., 2:4]) - torch.sqrt(size)) ** 2).sum(-1)[m].sum()
    obj = ((iou - conf) ** 2)[m].sum()
    noobj = (conf ** 2)[~m].sum()
    ce = torch.nn.functional.cross_entropy(t[..., 5:].reshape(-1, n_classes), torch.tensor(label).reshape(-1), reduction="none")
    cls = ce.reshape(B, h, w, A)[on_cell].sum()
    return (xy + wh + 5. * obj + noobj) / B + cls, t


# ---- the yardstick against autograd and against differences ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_float64_yardstick_equals_autograd(shape):
    h, w, A, n_classes, _ = shape
    logits, gt, counts = random_case(shape, 7)
    loss, leaf = torch_loss(logits, h, w, ANCHORS8[:2 * A], n_classes, gt, counts)
    loss.backward()
    got = float(loss.detach())
    want = loss_ref.loss(logits, h, w, ANCHORS8[:2 * A], n_classes, gt, counts, mode="float64")["loss"]
    print("shape %s: restated loss %.17g, loss_ref %.17g, relative gap %.3e" % (shape, got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-9 * abs(want)
    g_auto, g_ref = leaf.grad.numpy(), yardstick(shape)
    scale = float(np.max(np.abs(g_ref)))
    gap = float(np.max(np.abs(g_ref - g_auto)))
    print("shape %s: max|g_ref - g_autograd| = %.3e = %.3e of max|g| = %.6g" % (shape, gap, gap / scale, scale))
    assert np.isfinite(g_ref).all() and scale > 0 and gap <= 1e-6 * scale


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_float64_yardstick_equals_central_differences(shape):
    h, w, A, n_classes, _ = shape
    logits, gt, counts = random_case(shape, 7)
    g_ref = yardstick(shape)
    f = lambda x: loss_ref.loss(x, h, w, ANCHORS8[:2 * A], n_classes, gt, counts, mode="float64")["loss"]
    order = np.argsort(-np.abs(g_ref).reshape(-1), kind="stable")[:6]
    for flat in order:
        idx = np.unravel_index(int(flat), g_ref.shape)
        up, down = logits.copy(), logits.copy()
        up[idx] = np.float32(np.float64(logits[idx]) + 2. ** -10)
        down[idx] = np.float32(np.float64(logits[idx]) - 2. ** -10)
        step = np.float64(up[idx]) - np.float64(down[idx])          # (the float32 values actually fed)
        diff = (f(up) - f(down)) / step
        if g_ref[idx] == 0:             # (the 1 x 1 x 1 head has six elements, and its one class element is exactly 0 at C = 1)
            assert diff == 0, (idx, diff)
            continue
        rel = abs(diff - g_ref[idx]) / abs(g_ref[idx])
        print("shape %s element %s: yardstick %.12g, central difference %.12g, relative gap %.3e" % (shape, idx, g_ref[idx], diff, rel))
        assert rel <= 1e-4, (idx, g_ref[idx], diff)


@pytest.mark.parametrize("shape,seed", loss_grad_cases.GPU_CASES, ids=[IDS(s) for s, _ in loss_grad_cases.GPU_CASES])
def test_device_cases_are_not_degenerate(shape, seed):
    """the seeds of the device test: the float32 yardstick is off the float64 one by at least a quarter ulp of the group's largest
    element in every group that is not identically zero -- otherwise FACTOR * E_32 would bound nothing but the ulp"""
    r64, r32 = loss_grad_cases.yardsticks(shape, seed)
    figures = loss_grad_cases.group_figures(r64, r32)
    print("shape %s seed %d: E_32 / ulp32(M) = %s" % (shape, seed, {k: round(v["E_32"] / v["ulp"], 2) if v["M"] > 0 else None
                                                                     for k, v in figures.items()}))
    assert np.isfinite(r64).all() and np.isfinite(r32).all() and set(figures) == {"xy", "wh", "obj", "cls"}
    for name, fig in figures.items():
        if fig["M"] > 0:
            assert fig["E_32"] >= 0.25 * fig["ulp"], (name, fig)
        else:
            assert name == "cls" and shape[3] == 1 and fig["E_32"] == 0         # softmax of one class: 1 - 1


# ---- engineered cases: the tie rules -----------------------------------------------------------------------------------------------------
def one_truth_case(anchor, truth, t4=0.0):
    """a 4 x 4 grid, one anchor, one truth (grid units), all logits 0 except t4 on slot (1, 1, 0).  -> float64 gradient [4, 4, 6]"""
    gt, counts = raw_gts([[(truth[0] / 4., truth[1] / 4., truth[2] / 4., truth[3] / 4., 0)]], 2)
    logits = np.zeros((1, 4, 4, 1, 6), dtype=np.float32)
    logits[0, 1, 1, 0, 4] = t4
    table, _, _ = loss_ref.assign(4, 4, anchor, 1, gt, counts)
    assert table[0, 1, 1] == 0 and (table >= 0).sum() == 1
    return loss_grad_ref.grad(logits, 4, 4, anchor, 1, gt, counts, mode="float64")[0, :, :, 0, :], (logits, gt, counts)


def close(got, want):
    return abs(got - want) <= 1e-12 * max(abs(want), 1e-300) if want else got == 0


def test_perfect_match_takes_every_tie_bracket():
    """the prediction equals the truth: px1 == gx1, px2 == gx2, rw == gw -- every bracket is 1, dI/dpx = 0 and dI/dpw = 1 / gw"""
    G, _ = one_truth_case([2, 2], (1.5, 1.5, 2., 2.), t4=1.0)
    po = 1. / (1. + np.exp(-1.))
    assert G[1, 1, 0] == 0 and G[1, 1, 1] == 0
    assert close(G[1, 1, 2], 10. * (1. - po)) and close(G[1, 1, 3], 10. * (1. - po)) and abs(G[1, 1, 2] - 2.68941421) < 1e-8
    assert close(G[1, 1, 4], -10. * (1. - po) * po * (1. - po)) and abs(G[1, 1, 4] + 0.52877093) < 1e-8
    assert G[1, 1, 5] == 0                                              # C = 1: softmax - onehot
    others = np.ones((4, 4), dtype=bool)
    others[1, 1] = False
    assert (G[others][:, 4] == 0.25).all() and (G[others][:, :4] == 0).all() and (G[others][:, 5] == 0).all()
    # torch splits each of these ties in half: it is NOT the yardstick here (dI/dpw = 1 / (2 gw) there)
    logits = np.zeros((1, 4, 4, 1, 6), dtype=np.float32)
    logits[0, 1, 1, 0, 4] = 1.0
    gt, counts = raw_gts([[(0.375, 0.375, 0.5, 0.5, 0)]], 2)
    loss, leaf = torch_loss(logits, 4, 4, [2, 2], 1, gt, counts)
    loss.backward()
    assert abs(float(leaf.grad[0, 1, 1, 0, 2]) - G[1, 1, 2]) > 0.1


def test_touching_boxes_pass_the_gradient_and_disjoint_boxes_do_not():
    """anchor (0.5, 1), logits 0: the prediction at cell (1, 1) spans x 1.25 .. 1.75, y 1 .. 2 (all exact)"""
    # touching: the truth spans x 1.75 .. 2: rw == 0, [rw >= 0] = 1, [px2 <= gx2] = 1, [px1 >= gx1] = 0; iou = 0, uni = 0.75, ih = 1
    G, _ = one_truth_case([0.5, 1], (1.875, 1.5, 0.25, 1.))
    k = 5. * 2. * (0. - 0.5)
    assert close(G[1, 1, 0], (2. * (1.5 - 1.875) + k * (1. / 0.75)) * 0.25)
    assert close(G[1, 1, 2], ((np.sqrt(0.5) - np.sqrt(0.25)) / np.sqrt(0.5) + k * (0.5 * 0.75 / 0.75 ** 2)) * 0.5)
    assert G[1, 1, 1] == 0 and G[1, 1, 3] == 0                          # y: a perfect match with iw = 0: dinter/dph = iw = 0
    assert close(G[1, 1, 4], -k * 0.25)
    # disjoint: the truth spans x 1.875 .. 2: rw < 0, the IoU path contributes exactly 0 to x, y, w, h
    G, _ = one_truth_case([0.5, 1], (1.9375, 1.5, 0.125, 1.))
    assert G[1, 1, 0] == 2. * (1.5 - 1.9375) * 0.25
    assert close(G[1, 1, 2], (np.sqrt(0.5) - np.sqrt(0.125)) / np.sqrt(0.5) * 0.5)
    assert G[1, 1, 1] == 0 and G[1, 1, 3] == 0 and close(G[1, 1, 4], -k * 0.25)


# ---- structural zeros ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["float64", "float32"])
def test_structural_zeros(mode):
    shape = SHAPES[1]
    h, w, A, n_classes, B = shape
    logits, gt, counts = random_case(shape, 7)
    logits = logits.copy()
    table, _, _ = loss_ref.assign(h, w, ANCHORS8[:2 * A], n_classes, gt, counts)
    b, r, c = [int(v[0]) for v in np.nonzero(table >= 0)]
    a = int(table[b, r, c]) & 7
    other = (a + 1) % A
    logits[b, r, c, other, 2] = 100.            # a non-winner slot of a winner's cell: exp overflows in float32, its terms are never formed
    logits[b, r, c, other, 4] = 100.            # po = 1 exactly in both modes
    rr, cc = [int(v[0]) for v in np.nonzero(table[b] < 0)]
    logits[b, rr, cc, 0, 3] = 100.
    logits[b, rr, cc, 0, 4] = -100.             # po = 0 in float32, 3.7e-44 in float64
    logits[b, rr, cc, 1, 4] = 100.
    G = loss_grad_ref.grad(logits, h, w, ANCHORS8[:2 * A], n_classes, gt, counts, mode=mode)
    assert G.dtype == np.dtype(mode) and np.isfinite(G).all()
    on_slot = np.zeros((B, h, w, A), dtype=bool)
    for bb, r2, c2 in zip(*np.nonzero(table >= 0)):
        on_slot[bb, r2, c2, int(table[bb, r2, c2]) & 7] = True
    assert on_slot.sum() == (table >= 0).sum() > 0 and (table[1] < 0).all()
    assert (G[~on_slot][:, :4] == 0).all() and not np.signbit(G[~on_slot][:, :4]).any()
    assert (G[table < 0][:, :, 5:] == 0).all() and (G[1, ..., 5:] == 0).all()
    assert (G[table >= 0][:, :, 5:] != 0).any(axis=-1).all()            # ... and every slot of a winner's cell has a class row
    assert (G[b, r, c, other, :5] == 0).all() and (G[b, rr, cc, 0, :4] == 0).all() and G[b, rr, cc, 1, 4] == 0
    if mode == "float32":
        assert G[b, rr, cc, 0, 4] == 0
    else:
        po = 1. / (1. + np.exp(100.))
        assert G[b, rr, cc, 0, 4] == (1. / B * 2. * po) * (po * (1. - po)) and 0 < G[b, rr, cc, 0, 4] < 1e-86
    # nothing else moved
    base = yardstick(shape, mode)
    touched = np.zeros(G.shape, dtype=bool)
    touched[b, r, c, other, :5] = touched[b, rr, cc, 0, :5] = touched[b, rr, cc, 1, :5] = True
    assert np.array_equal(G[~touched], base[~touched])


# ---- C ABI: host-side checks, before any device call -------------------------------------------------------------------------------------
def last_error():
    return (_hip.lib().yolo_last_error() or b"").decode()


def head(version=2, n_scales=1, h=13, w=13, a=5, c=20):
    hd = engine.head_desc_v2(h, w, ANCHORS8[:2 * a], c)
    hd.version, hd.n_scales = version, n_scales
    for s in range(1, n_scales):
        hd.h[s], hd.w[s], hd.n_anchors[s] = h, w, a
    return hd


def test_export_and_signature():
    lib = _hip.lib()
    assert lib.yolo_hip_abi_version() == 7 == _hip.ABI_VERSION
    res, args = _hip.SIGNATURES["yolo_v2_loss_grad"]
    assert res is C.c_int and args == [C.POINTER(_hip.HeadDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.yolo_v2_loss_grad.argtypes == args and lib.yolo_v2_loss_grad.restype is C.c_int
    assert args[:9] + args[10:] == _hip.SIGNATURES["yolo_v2_loss"][1]      # yolo_v2_loss's, with grad_dev in front of the stream
    assert not hasattr(lib, "yolo_net_loss_grad") and "yolo_net_loss_grad" not in _hip.SIGNATURES        # (no consumer yet)


def test_v2_loss_grad_refuses_bad_arguments():
    lib = _hip.lib()
    P, Q = 4096, 8192           # non-null pointers that are never used: the checks come first
    ok = head()
    call = lambda hd=ok, logits=P, batch=1, gt=P, gc=P, max_gt=8, images=P, assign=P, result=P, grad=Q: lib.yolo_v2_loss_grad(
        C.byref(hd) if hd is not None else None, logits, batch, gt, gc, max_gt, images, assign, result, grad, None)
    for kw in (dict(hd=None), dict(logits=None), dict(gt=None), dict(gc=None), dict(images=None), dict(result=None), dict(assign=None),
               dict(grad=None)):
        assert call(**kw) == 1 and "yolo_v2_loss_grad: null argument" in last_error(), kw
    assert call(grad=P) == 1 and "yolo_v2_loss_grad: grad_dev must not be logits_dev" in last_error()
    assert call(hd=head(version=3)) == 1 and "the reference has a loss for YOLOv2 only" in last_error()
    assert call(hd=head(n_scales=2)) == 1 and "yolo_v2_loss_grad: the head must be version 2 with one scale" in last_error()
    for m in (0, 1025):
        assert call(max_gt=m) == 1 and "yolo_v2_loss_grad: max_gt must be 1..1024" in last_error()
    assert call(batch=0) == 1 and "yolo_v2_loss_grad: batch must be at least 1" in last_error()
    assert call(hd=head(h=65, w=65)) == 1 and "yolo_v2_loss_grad: h * w must be at most 4096" in last_error()
    assert call(hd=head(a=0)) == 1 and "yolo_v2_loss_grad: bad head scale" in last_error()


# ---- the torch op's own checks -------------------------------------------------------------------------------------------------------------
def test_lossfn_refuses_what_it_cannot_take():
    import torch
    import tensorflow_yolo_amd
    assert tensorflow_yolo_amd.yolo_v2_loss is lossfn.yolo_v2_loss
    anchors = ANCHORS8[:4]
    with pytest.raises(ValueError, match="expected a float32 device tensor, got torch.float64"):
        lossfn.yolo_v2_loss(torch.zeros((1, 2, 2, 2 * 8), dtype=torch.float64), [[]], anchors, 3)
    with pytest.raises(ValueError, match="expected a float32 device tensor, got torch.float32 on cpu"):
        lossfn.yolo_v2_loss(torch.zeros((1, 2, 2, 2, 8), dtype=torch.float32), [[]], anchors, 3)
    with pytest.raises(ValueError, match="expected a float32 device tensor, got ndarray"):
        lossfn.yolo_v2_loss(np.zeros((1, 2, 2, 16), dtype=np.float32), [[]], anchors, 3)
    for shape in ((1, 2, 2, 15), (1, 2, 2, 2, 7), (1, 2, 2, 8, 2), (2, 2, 16), (1, 2, 2, 2, 4, 2)):
        with pytest.raises(ValueError, match=r"expected \[B, h, w, 16\] or \[B, h, w, 2, 8\]"):
            lossfn.yolo_v2_loss(torch.zeros(shape, dtype=torch.float32), [[]], anchors, 3)

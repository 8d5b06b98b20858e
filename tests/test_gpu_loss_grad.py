"""GPU: the gradient of the YOLOv2 loss with respect to the logits (yolo_v2_loss_grad through the C ABI, the torch op of net/lossfn.py,
HipNetwork.loss_grad / Yolo.loss_grad) against the sequential yardstick tests/loss_grad_ref.py.

Every device output -- images, result, assign and grad -- is a 0xA5-filled buffer with a 256-byte guard band on both sides; a gradient
without a single 0xA5A5A5A5 word left (-2.3e-16 as a float, which no case here produces) has had every element written.

Values are compared per call and per group of elements (xy = 0-1, wh = 2-3, obj = 4, cls = 5 and up; loss_grad_cases.group_figures):
E_dev = max|device - ref64| <= FACTOR * E_32 + ulp32(M), E_32 = max|ref32 - ref64|, M = max|ref64|, FACTOR = 4 -- the margin
tests/test_gpu_loss.py gives the same sigmoid / expf / sqrt arithmetic, set before the gradient was measured.  A group with M == 0 is
exactly zero on the device.  Where the float32 yardstick is not finite the device is not finite either, and nowhere else.

Measured on an MI355X, the largest (E_dev - ulp32(M)) / E_32 over the groups of each of the fourteen shapes of
loss_grad_cases.GPU_CASES, in their order: 0.959, 0.869, 0.917, 0.658, 0.836, 0.952, 0.939, 0.794, 0.968, 0.769, 0.998, 0.941, 0.878 and
0.870.  The engineered cases: 0.853 (rules), 0.937 (overflow).  In most groups E_dev equals E_32 to the digits printed: the kernel rounds
every operation on its own and in the yardstick's order, so it lands on the float32 yardstick's values except where the device's expf
differs from NumPy's or a row's sum is added in another order."""
import ctypes as C

import numpy as np
import pytest

import loss_grad_cases as cases
import loss_grad_ref
import loss_ref
from loss_grad_cases import ANCHORS8, FACTOR, raw_gts
from tensorflow_yolo_amd import YoloV2Tiny, YoloV3Tiny, _hip, yolo_v2_loss
from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 256, 0xA5
IDS = ["x".join(str(v) for v in s) for s, _ in cases.GPU_CASES]


def guarded(nbytes):
    import torch
    t = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + GUARD


def check_guards(bufs):
    for t, _ in bufs:
        assert bool((t[:GUARD] == PATTERN).all()) and bool((t[-GUARD:] == PATTERN).all()), "a guard band was written"


def upload(logits, gt, counts):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)).cuda(),
            torch.from_numpy(np.ascontiguousarray(gt).view(np.uint8).reshape(-1)).cuda(),
            torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda())


def run_grad(h, w, anchors, n_classes, logits, gt, counts, calls=1):
    """yolo_v2_loss_grad through the C ABI, every output in a pattern-filled buffer with a guard band on both sides.
    -> (images LOSS_IMAGE_DTYPE [B], result record, table int32 [B, h, w], grad float32 [B, h, w, A, 5 + C])"""
    import torch
    lib = _hip.lib()
    shape = tuple(np.asarray(logits).shape)
    B, n = shape[0], int(np.prod(shape))
    hd = engine.head_desc_v2(h, w, anchors, n_classes)
    d_logits, d_gt, d_gc = upload(logits, gt, counts)
    bufs = [guarded(B * 56), guarded(64), guarded(B * h * w * 4), guarded(n * 4)]
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(calls):
        _hip.check(lib.yolo_v2_loss_grad(C.byref(hd), d_logits.data_ptr(), B, d_gt.data_ptr(), d_gc.data_ptr(), gt.shape[1], bufs[0][1],
                                         bufs[2][1], bufs[1][1], bufs[3][1], st), "yolo_v2_loss_grad")
    torch.cuda.synchronize()
    check_guards(bufs)
    body = [t[GUARD:-GUARD].cpu().numpy() for t, _ in bufs]
    images = body[0].view(yeval.LOSS_IMAGE_DTYPE).copy()
    result = body[1].view(yeval.LOSS_RESULT_DTYPE)[0].copy()
    table = body[2].view(np.int32).reshape(B, h, w).copy()
    assert not (body[3].view(np.uint32) == 0xA5A5A5A5).any(), "an element of grad was not written"
    return images, result, table, body[3].view(np.float32).reshape(shape).copy()


def run_loss(h, w, anchors, n_classes, logits, gt, counts):
    """yolo_v2_loss on the same inputs -> the bytes of (images, result, assign)"""
    import torch
    lib = _hip.lib()
    B = int(np.asarray(logits).shape[0])
    hd = engine.head_desc_v2(h, w, anchors, n_classes)
    d_logits, d_gt, d_gc = upload(logits, gt, counts)
    bufs = [guarded(B * 56), guarded(64), guarded(B * h * w * 4)]
    _hip.check(lib.yolo_v2_loss(C.byref(hd), d_logits.data_ptr(), B, d_gt.data_ptr(), d_gc.data_ptr(), gt.shape[1], bufs[0][1], bufs[2][1],
                                bufs[1][1], torch.cuda.current_stream().cuda_stream), "yolo_v2_loss")
    torch.cuda.synchronize()
    check_guards(bufs)
    return [t[GUARD:-GUARD].cpu().numpy().tobytes() for t, _ in bufs]


def winner_slots(table, A):
    on = np.zeros(table.shape + (A,), dtype=bool)
    for b, r, c in zip(*np.nonzero(table >= 0)):
        on[b, r, c, int(table[b, r, c]) & 7] = True
    return on


def check_structure(grad, table):
    """the structural zeros, on the device: G[0..3] of every slot that is not a winner, G[5:] of every cell without a winner"""
    on = winner_slots(table, grad.shape[3])
    assert (grad[~on][:, :4] == 0).all(), "a coordinate element of a slot that is not a winner"
    assert (grad[table < 0][:, :, 5:] == 0).all(), "a class element of a cell without a winner"


def compare_groups(tag, grad, r64, r32):
    """the bound of the module docstring, per call and per group; prints every figure, and per image when a group fails.
    -> the largest (E_dev - ulp) / E_32"""
    bad = ~np.isfinite(r32)
    assert np.array_equal(~np.isfinite(grad), bad), "%s: the device is not finite exactly where the float32 yardstick is not" % tag
    worst = 0.0
    for name, fig in cases.group_figures(r64, r32, grad).items():
        print("%s %s: M %.6g E_32 %.3e E_dev %.3e ulp %.3e (E_dev - ulp) / E_32 = %.3f (bound %.1f)"
              % (tag, name, fig["M"], fig["E_32"], fig["E_dev"], fig["ulp"], fig["ratio"], FACTOR))
        if fig["M"] == 0:
            assert fig["E_dev"] == 0, (tag, name, "must be exactly zero")
            continue
        worst = max(worst, fig["ratio"])
        if not fig["E_dev"] <= FACTOR * fig["E_32"] + fig["ulp"]:
            sl = dict(cases.GROUPS)[name]
            for b in range(grad.shape[0]):
                with np.errstate(invalid="ignore"):
                    gap = np.where(bad[b][..., sl], 0.0, np.abs(grad[b][..., sl].astype(np.float64) - r64[b][..., sl]))
                at = np.unravel_index(int(np.argmax(gap)), gap.shape)
                print("  image %d: largest |device - ref64| %.3e at (row, col, anchor, element) %s: device %.9g ref64 %.17g ref32 %.9g"
                      % (b, gap[at], at, grad[b][..., sl][at], r64[b][..., sl][at], r32[b][..., sl][at]))
            raise AssertionError((tag, name, fig))
    print("%s: largest (E_dev - ulp) / E_32 = %.3f" % (tag, worst))
    return worst


# ---- values -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", cases.GPU_CASES, ids=IDS)
def test_values_against_the_yardstick(shape, seed):
    h, w, A, n_classes, B = shape
    logits, gt, counts = cases.random_case(shape, seed)
    r64, r32 = cases.yardsticks(shape, seed)
    images, result, table, grad = run_grad(h, w, ANCHORS8[:2 * A], n_classes, logits, gt, counts)
    want, _, _ = loss_ref.assign(h, w, ANCHORS8[:2 * A], n_classes, gt, counts)
    assert np.array_equal(table, want)
    check_structure(grad, table)
    compare_groups("shape %s" % (shape,), grad, r64, r32)


@pytest.mark.parametrize("k", [1, 3, 4], ids=[IDS[1], IDS[3], IDS[4]])
def test_loss_side_is_unchanged_and_two_calls_give_the_same_bytes(k):
    shape, seed = cases.GPU_CASES[k]
    h, w, A, n_classes, B = shape
    logits, gt, counts = cases.random_case(shape, seed)
    images, result, table, grad = run_grad(h, w, ANCHORS8[:2 * A], n_classes, logits, gt, counts)
    plain = run_loss(h, w, ANCHORS8[:2 * A], n_classes, logits, gt, counts)
    assert images.tobytes() == plain[0] and result.tobytes() == plain[1] and table.tobytes() == plain[2]
    again = run_grad(h, w, ANCHORS8[:2 * A], n_classes, logits, gt, counts, calls=2)       # twice into the same buffers
    assert again[3].tobytes() == grad.tobytes() and again[0].tobytes() == images.tobytes() and again[1].tobytes() == result.tobytes()


# ---- rules ------------------------------------------------------------------------------------------------------------------------------
def test_rules():
    """one call on a 4 x 4 grid with one anchor (2, 2) and three classes: image 0 is the perfect match of the issue (every tie bracket),
    1 is empty, 2 has skipped truths (out of grid, bad box, bad class) between good ones, 3 has a clamped count (max_gt + 1), 4 has two
    truths in one cell; the records behind every count are 0xFF bytes"""
    h, w, anchors, n_classes, max_gt = 4, 4, [2, 2], 3, 5
    g = lambda x, y, bw, bh, c: (x / 4., y / 4., bw / 4., bh / 4., c)
    lists = [[g(1.5, 1.5, 2, 2, 0)],
             [],
             [g(0.5, 0.5, 1, 1, 1), (1.0, 0.5, 0.2, 0.2, 1), (0.5, 0.5, -0.2, 0.2, 1), (0.5, 0.5, 0.2, 0.2, 3), g(3.5, 2.5, 3, 1, 2)],
             [g(0.5, 3.5, 1, 1, 0), g(1.5, 3.5, 1, 2, 1), g(2.5, 3.5, 2, 1, 2), g(3.5, 3.5, 2, 2, 0), g(3.5, 0.5, 4, 4, 1)],
             [g(2.25, 1.25, 0.5, 0.5, 1), g(2.75, 1.75, 2, 2.5, 2)]]
    gt, counts = raw_gts(lists, max_gt)
    counts[3] = max_gt + 1
    logits = np.random.RandomState(21).uniform(-6, 6, size=(5, h, w, 1, 5 + n_classes)).astype(np.float32)
    logits[0] = 0
    logits[0, 1, 1, 0, 4] = 1.0
    want, status, n_truths = loss_ref.assign(h, w, anchors, n_classes, gt, counts)
    # the yardstick itself hits every rule
    assert (want[0] >= 0).sum() == 1 and want[0, 1, 1] == 0 and (want[1] == -1).all()
    assert status.tolist() == [0, 0, 7, 8, 0] and n_truths.tolist() == [1, 0, 2, 5, 2] and (want[2] >= 0).sum() == 2 and want[2, 2, 3] == 4 * 8
    assert (want[3] >= 0).sum() == 5 and (want[4] >= 0).sum() == 1 and want[4, 1, 2] == 1 * 8
    images, result, table, grad = run_grad(h, w, anchors, n_classes, logits, gt, counts)
    assert np.array_equal(table, want) and images["status"].tolist() == status.tolist() and images["n_truths"].tolist() == n_truths.tolist()
    check_structure(grad, table)
    r64, r32 = (loss_grad_ref.grad(logits, h, w, anchors, n_classes, gt, counts, mode=m) for m in ("float64", "float32"))
    compare_groups("rules", grad, r64, r32)
    # the perfect match at B = 5: dI/dpx = 0 exactly, dI/dpw = 1 / gw.  16 float32 ulp: po carries an expf and a division, 1 - po
    # amplifies its error by po / (1 - po) = 2.7, and four more roundings follow
    po = 1. / (1. + np.exp(-1.))
    tie, tol = grad[0, 1, 1, 0], 16 * 2. ** -24
    assert tie[0] == 0 and tie[1] == 0
    assert abs(tie[2] - 2. * (1. - po)) <= tol * 2. * (1. - po) and tie[3] == tie[2]
    assert abs(tie[4] + 2. * (1. - po) * po * (1. - po)) <= tol * 2. * (1. - po) * po * (1. - po)
    assert abs(tie[5] + 2. / 3.) <= tol and abs(tie[6] - 1. / 3.) <= tol and tie[6] == tie[7]
    others = np.ones((4, 4), dtype=bool)
    others[1, 1] = False
    assert (grad[0, :, :, 0, 4][others] == np.float32(0.25 / 5)).all()
    assert (grad[1, ..., :4] == 0).all() and (grad[1, ..., 5:] == 0).all() and (grad[1, ..., 4] > 0).all()


# ---- overflow ---------------------------------------------------------------------------------------------------------------------------
def test_overflow_stays_on_its_slot():
    h, w, A, n_classes = 4, 4, 5, 20
    rng = np.random.RandomState(4)
    logits = rng.uniform(-6, 6, size=(2, h, w, A, 5 + n_classes)).astype(np.float32)
    lists = [[(0.3, 0.3, 0.2, 0.3, 1)], [(0.3, 0.3, 0.2, 0.3, 1), (0.8, 0.6, 0.5, 0.5, 7)]]
    gt, counts = raw_gts(lists, 2)
    table, _, _ = loss_ref.assign(h, w, ANCHORS8[:10], n_classes, gt, counts)
    a = int(table[0, 1, 1]) & 7
    logits[0, 1, 1, (a + 1) % A, 2] = 100.      # image 0: t2 = 100 on a slot of the winner's CELL that is not the winner, and on a far cell
    logits[0, 3, 3, 0, 3] = 100.
    logits[0, 3, 3, 1, 4] = 100.                # ... and saturated objectness: po = 1 and po = 0 exactly
    logits[0, 3, 3, 2, 4] = -100.
    logits[1, 1, 1, a, 2] = 100.                # image 1: on the winner slot itself
    r64, r32 = (loss_grad_ref.grad(logits, h, w, ANCHORS8[:10], n_classes, gt, counts, mode=m) for m in ("float64", "float32"))
    bad = ~np.isfinite(r32)
    assert bad.any() and not bad[0].any() and np.array_equal(np.argwhere(bad)[:, :4], np.repeat([[1, 1, 1, a]], bad.sum(), axis=0))
    images, result, got, grad = run_grad(h, w, ANCHORS8[:10], n_classes, logits, gt, counts)
    assert np.array_equal(got, table)
    check_structure(grad, table)
    compare_groups("overflow", grad, r64, r32)          # (asserts: not finite exactly where ref32 is not; everything else within the bound)
    assert (grad[0, 1, 1, (a + 1) % A, :4] == 0).all() and (grad[0, 3, 3, 0, :4] == 0).all()
    assert grad[0, 3, 3, 1, 4] == 0 and grad[0, 3, 3, 2, 4] == 0


# ---- the torch op -----------------------------------------------------------------------------------------------------------------------
def test_autograd_op_is_the_abi_gradient():
    import torch
    shape, seed = cases.GPU_CASES[1]
    h, w, A, n_classes, B = shape
    anchors = ANCHORS8[:2 * A]
    logits, gt, counts = cases.random_case(shape, seed)
    images, result, table, grad = run_grad(h, w, anchors, n_classes, logits, gt, counts)
    x = torch.from_numpy(logits.reshape(B, h, w, A * (5 + n_classes))).cuda().requires_grad_()
    loss, record = yolo_v2_loss(x, (gt, counts), anchors, n_classes, return_record=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad and not record.requires_grad
    assert record.cpu().numpy().tobytes() == result.tobytes()
    assert loss.item() == float(np.float32(result["loss"]))
    loss.backward()
    assert x.grad.shape == x.shape and x.grad.cpu().numpy().tobytes() == grad.tobytes()
    x2 = x.detach().clone().requires_grad_()
    (2 * yolo_v2_loss(x2, (gt, counts), anchors, n_classes)).backward()
    assert x2.grad.cpu().numpy().tobytes() == (np.float32(2) * grad).tobytes()
    # a non-contiguous [B, h, w, A, 5 + C] view: the last two axes of a tensor stored [B, h, w, 5 + C, A]
    stored = torch.from_numpy(np.ascontiguousarray(logits.transpose(0, 1, 2, 4, 3))).cuda().requires_grad_()
    view = stored.transpose(3, 4)
    assert not view.is_contiguous() and tuple(view.shape) == logits.shape
    yolo_v2_loss(view, (gt, counts), anchors, n_classes).backward()
    assert stored.grad.cpu().numpy().tobytes() == np.ascontiguousarray(grad.transpose(0, 1, 2, 4, 3)).tobytes()
    # lists of truths, and device tensors of truths, are the same truths
    lists = [[tuple(gt[b, g])[:5] for g in range(counts[b])] for b in range(B)]
    x3 = x.detach().clone().requires_grad_()
    yolo_v2_loss(x3, lists, anchors, n_classes).backward()
    assert x3.grad.cpu().numpy().tobytes() == grad.tobytes()


def test_descent():
    """end to end through the op: 20 steps of plain SGD on the logits themselves, the loss lower after every step (the float64 yardstick
    goes 789.69 -> 578.47 -> ... -> 475.92 on the same loop, at least 4.3 per step: far above float32 noise)"""
    import torch
    shape = (4, 4, 5, 20, 3)
    h, w, A, n_classes, B = shape
    logits, gt, counts = cases.random_case(shape, 7)
    param = torch.nn.Parameter(torch.from_numpy(logits).cuda())
    opt = torch.optim.SGD([param], lr=0.05)
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(B, -1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
    losses = []
    for _ in range(21):
        opt.zero_grad()
        loss = yolo_v2_loss(param, (d_gt, d_gc), ANCHORS8[:2 * A], n_classes)
        loss.backward()
        opt.step()
        losses.append(loss)
    losses = [float(v) for v in torch.stack(losses).detach().cpu()]          # the one read
    print("descent:", " ".join("%.2f" % v for v in losses))
    assert abs(losses[0] - 789.69) < 0.01 and all(b < a for a, b in zip(losses, losses[1:])), losses


# ---- through a network ------------------------------------------------------------------------------------------------------------------
HW = (32, 32)
NAMES3 = ["a", "b", "c"]
V2_ANCHORS = ANCHORS8[:10]


def test_yolo_loss_grad_is_forward_then_the_abi_gradient():
    """tiny-YOLOv2 at 32 x 32 (a 1 x 1 grid: its five stride-2 pools take nothing smaller), float and uint8 batches"""
    import torch
    lib = _hip.lib()
    m = YoloV2Tiny()
    net = YoloV2Tiny.create_network(np.reshape(V2_ANCHORS, [-1, 2]), NAMES3, False, input_shape=HW + (3,))
    weights = synth.darknet_stream(net, seed=31, num_classes=3, head_gain=synth.HEAD_DEFAULTS["v2-tiny"][0], obj_bias=0.0)
    m.build(V2_ANCHORS, NAMES3, HW + (3,), dtype="fp32", max_batch=2, weights=weights)
    eng = m.net.engine
    x8 = np.random.RandomState(32).randint(0, 256, size=(2,) + HW + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    truths = [[(0.3, 0.4, 0.2, 0.5, 1), (0.8, 0.2, 0.3, 0.3, 2)], []]
    gt, counts = yeval.pack_gts(truths, 2)
    st = torch.cuda.current_stream().cuda_stream
    for x, fwd in ((xf, eng.forward), (x8, eng.forward_u8)):
        logits = fwd(x)
        assert tuple(logits.shape) == (2, 1, 1, 5 * 8)
        d_logits, d_gt, d_gc = upload(logits.cpu().numpy(), gt, counts)
        bufs = [guarded(2 * 56), guarded(64), guarded(2 * 4), guarded(logits.numel() * 4)]
        _hip.check(lib.yolo_v2_loss_grad(C.byref(eng.head), d_logits.data_ptr(), 2, d_gt.data_ptr(), d_gc.data_ptr(), 2, bufs[0][1], bufs[2][1],
                                         bufs[1][1], bufs[3][1], st), "yolo_v2_loss_grad")
        torch.cuda.synchronize()
        check_guards(bufs)
        out = m.loss_grad(x, truths)
        grad = out.pop("grad")
        assert grad.is_cuda and grad.dtype == torch.float32 and tuple(grad.shape) == (2, 1, 1, 5 * 8)
        assert grad.cpu().numpy().tobytes() == bufs[3][0][GUARD:-GUARD].cpu().numpy().tobytes()
        plain = m.loss(x, truths)
        assert set(out) == set(plain) and out["n_assigned"] == 1 and out["status"] == 0 and np.isfinite(out["loss"]) and out["loss"] > 0
        for k in plain:
            assert (out[k].tobytes() == plain[k].tobytes()) if k == "images" else (out[k] == plain[k]), k
        images, result, assign, g2 = (eng.loss_grad_u8 if x is x8 else eng.loss_grad)(x, (gt, counts))
        assert torch.equal(g2, grad) and int((assign >= 0).sum()) == 1


def test_loss_grad_refuses_a_v3_net():
    anchors = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
    m = YoloV3Tiny()
    net = YoloV3Tiny.create_network(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3))
    m.build(anchors, NAMES3, (96, 160, 3), dtype="fp16", max_batch=1, weights=synth.darknet_stream(net, seed=33, num_classes=3))
    with pytest.raises(ValueError, match="YOLOv2 heads only"):
        m.loss_grad(np.zeros((1, 96, 160, 3), dtype=np.float32), [[]])

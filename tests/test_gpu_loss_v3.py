"""GPU: the YOLOv3 loss and its gradient (yolo_v3_loss, yolo_v3_loss_grad, yolo_net_loss_v3[_u8] through the C ABI; the torch op of
net/lossfn.py; HipNetwork.loss_v3* / Yolo.loss_v3*) against the sequential yardstick tests/loss_v3_ref.py.

Every device buffer has a 256-byte guard band of 0xA5 on both sides.  Scratch (the part records), images, result, table and gradient are
pre-filled with 0x00 and, in a second run, with 0xFF: the two runs must return the same bytes, so every byte of every output is written by
every call and nothing depends on what the buffers held.

Shapes (tests/loss_v3_cases.py), the smallest at which something can go wrong:
    smallest         one scale 1 x 1 x 1, C = 1, B = 1                       a single row
    three-scales     2 x 3 / 4 x 6 / 8 x 12, A = 3, C = 3, B = 3             non-square, a wave's rows straddle scales
    tiny             3 x 3 / 6 x 6, A = 3, C = 20, B = 2                     the tiny geometry
    row-of-85        4 x 4 / 8 x 8 / 16 x 16, C = 80, B = 2                  rows that are not 16-byte aligned
    parts            13^2 / 26^2 / 52^2, C = 1, B = 2                        eleven parts per image, the last one partial
    long-class-row   2 x 2 / 4 x 4, C = 150                                  a class row longer than two passes of a wave
    batch-65         2 x 2 / 4 x 4, B = 65                                   more images than one pass of the finish kernel's waves
    truth-edges      4 x 4 / 8 x 8, images with 0, 1 and 1024 truths         max_gt = YOLO_EVAL_MAX_GT

Assertions per shape: the table EQUALS the float32 yardstick's (tests/test_loss_v3_cpu.py guarantees that no IoU lies within 1e-5 of the
threshold); n_assigned, n_truths and status are equal; each of the five sums, per image and in total, is within 4 d + 1 ulp of the float64
yardstick, d = the yardstick's own float32-against-float64 gap (the rule of tests/test_gpu_loss.py); the gradient has exact structural zeros
and every group (xy, wh, obj, cls) holds E_dev <= 4 E_32 + ulp32(M) (the rule and FACTOR of tests/loss_grad_cases.py), and is non-finite
exactly where the float32 yardstick is.

Measured on an MI355X, the largest (|device - ref64| - ulp) / d over the sums of each of the eight shapes, in their order: 0.964, 0.173,
0.600, 0.000, 0.000, 0.000, 0.959 and 0.590; the rules batch 0.244.  In every gradient group of every shape E_dev equals E_32 to the
digits printed (largest (E_dev - ulp) / E_32 = 0.972): expf and log1pf of the terms and of the gradient's sigmoid are correctly rounded
on both sides, so the device lands on the float32 yardstick's values.  Every test prints its figures (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

import loss_v3_cases as cases
import loss_v3_ref
from loss_grad_cases import raw_gts
from tensorflow_yolo_amd import YoloV2Tiny, YoloV3, YoloV3Tiny, _hip, yolo_v3_loss
from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 256, 0xA5
KEYS = ("xy", "wh", "obj", "noobj", "cls")


def guarded(nbytes, fill):
    import torch
    t = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    t[GUARD:GUARD + nbytes] = fill
    return t, t.data_ptr() + GUARD


def check_guards(bufs):
    for t, _ in bufs:
        assert bool((t[:GUARD] == PATTERN).all()) and bool((t[-GUARD:] == PATTERN).all()), "a guard band was written"


def upload(logits, gt, counts):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)).cuda(),
            torch.from_numpy(np.ascontiguousarray(gt).view(np.uint8).reshape(-1)).cuda(),
            torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda())


def run(hd, logits, gt, counts, thresh=cases.IGNORE, fill=0x00, grad=True, calls=1, grad_shift=0):
    """yolo_v3_loss_grad (or yolo_v3_loss) through the C ABI into guarded, pre-filled buffers -> dict of host arrays and their bytes"""
    import torch
    lib = _hip.lib()
    B = int(np.asarray(logits).shape[0])
    R, P = engine.v3_loss_rows(hd)
    n = B * R * (5 + hd.n_classes)
    assert np.asarray(logits).size == n
    d_logits, d_gt, d_gc = upload(logits, gt, counts)
    bufs = [guarded(B * P * 56, fill), guarded(B * 56, fill), guarded(64, fill), guarded(B * R * 4, fill)] + ([guarded(n * 4 + 16, fill)] if grad else [])
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(calls):
        if grad:
            _hip.check(lib.yolo_v3_loss_grad(C.byref(hd), d_logits.data_ptr(), B, d_gt.data_ptr(), d_gc.data_ptr(), gt.shape[1], thresh, bufs[0][1],
                                             bufs[1][1], bufs[3][1], bufs[2][1], bufs[4][1] + grad_shift, st), "yolo_v3_loss_grad")
        else:
            _hip.check(lib.yolo_v3_loss(C.byref(hd), d_logits.data_ptr(), B, d_gt.data_ptr(), d_gc.data_ptr(), gt.shape[1], thresh, bufs[0][1],
                                        bufs[1][1], bufs[3][1], bufs[2][1], st), "yolo_v3_loss")
    torch.cuda.synchronize()
    check_guards(bufs)
    body = [t[GUARD:-GUARD].cpu().numpy() for t, _ in bufs]
    if grad:        # the gradient sits grad_shift bytes into a buffer 16 bytes longer: nothing around it is written
        assert (body[4][:grad_shift] == fill).all() and (body[4][grad_shift + n * 4:] == fill).all(), "a byte next to the gradient was written"
        body[4] = body[4][grad_shift:grad_shift + n * 4].copy()
    out = {"parts": body[0].view(yeval.LOSS_IMAGE_DTYPE).reshape(B, P).copy(), "images": body[1].view(yeval.LOSS_IMAGE_DTYPE).copy(),
           "result": body[2].view(yeval.LOSS_RESULT_DTYPE)[0].copy(), "table": body[3].view(np.int32).reshape(B, R).copy()}
    if grad:
        out["grad"] = body[4].view(np.float32).reshape(B, R, 5 + hd.n_classes).copy()
    out["bytes"] = [b.tobytes() for b in body]
    return out


def compare(tag, out, r64, r32):
    """every assertion of the module docstring on one call's outputs; prints the figures"""
    images, result, table = out["images"], out["result"], out["table"]
    assert np.array_equal(table, r32["table"]), "%s: the table differs at %s" % (tag, np.argwhere(table != r32["table"])[:8].tolist())
    assert images["n_assigned"].tolist() == r32["n_assigned"].tolist() and images["n_truths"].tolist() == r32["n_truths"].tolist()
    assert images["status"].tolist() == r32["status"].tolist() and (images["pad_"] == 0).all() and result["pad_"] == 0
    assert result["n_assigned"] == r32["n_assigned"].sum() and result["n_truths"] == r32["n_truths"].sum()
    assert result["status"] == np.bitwise_or.reduce(r32["status"])
    worst = 0.0
    for b in range(len(images)):
        for i, k in enumerate(KEYS):
            worst = max(worst, cases.check_value("%s image %d %s" % (tag, b, k), float(images[k][b]), r64["sums"][b, i], r32["sums"][b, i]))
    for k in yeval.LOSS_KEYS:
        worst = max(worst, cases.check_value("%s total %s" % (tag, k), float(result[k]), r64["totals"][k], r32["totals"][k]))
    print("%s: sums, largest (|device - ref64| - ulp) / d = %.3f (bound %.1f)" % (tag, worst, cases.FACTOR))
    # the parts add up to the images, in part order
    for b in range(len(images)):
        for k in KEYS:
            s = 0.0
            for v in out["parts"][k][b]:
                s += float(v)
            assert s == float(images[k][b]), (tag, b, k)
        assert out["parts"]["n_assigned"][b].sum() == images["n_assigned"][b]
    if "grad" not in out:
        return
    grad, g64, g32 = out["grad"], r64["grad"], r32["grad"]
    assert (grad[table == -2] == 0).all(), "an element of an ignored row"
    assert (grad[table < 0][:, :4] == 0).all() and (grad[table < 0][:, 5:] == 0).all(), "a box or class element of a row that is not a winner"
    assert not np.signbit(grad[table < 0][:, :4]).any() and not np.signbit(grad[table == -2]).any(), "a structural zero must be +0"
    assert np.array_equal(~np.isfinite(grad), ~np.isfinite(g32)), "%s: the device is not finite exactly where the float32 yardstick is not" % tag
    for name, fig in cases.group_figures(g64, g32, grad).items():
        print("%s %s: M %.6g E_32 %.3e E_dev %.3e ulp %.3e (E_dev - ulp) / E_32 = %.3f (bound %.1f)"
              % (tag, name, fig["M"], fig["E_32"], fig["E_dev"], fig["ulp"], fig["ratio"], cases.FACTOR))
        if fig["M"] == 0:
            assert fig["E_dev"] == 0, (tag, name, "must be exactly zero")
            continue
        assert fig["E_dev"] <= cases.FACTOR * fig["E_32"] + fig["ulp"], (tag, name, fig)


def head_of(grids, anchors, n_classes):
    return engine.head_desc_v3(grids, anchors, n_classes)


# ---- values -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.GPU_CASES))
def test_values_against_the_yardstick(name):
    logits, gt, counts, grids, anchors, n_classes = cases.make_case(name)
    r64, r32 = cases.yardsticks(name)
    hd = head_of(grids, anchors, n_classes)
    zero = run(hd, logits, gt, counts, fill=0x00)
    compare(name, zero, r64, r32)
    ones = run(hd, logits, gt, counts, fill=0xFF)
    assert ones["bytes"] == zero["bytes"], "an output depends on what its buffer held: not every byte is written"


@pytest.mark.parametrize("name", ["three-scales", "parts", "batch-65"])
def test_determinism_and_the_loss_side(name):
    logits, gt, counts, grids, anchors, n_classes = cases.make_case(name)
    hd = head_of(grids, anchors, n_classes)
    once = run(hd, logits, gt, counts, fill=0xFF)
    twice = run(hd, logits, gt, counts, fill=0x00, calls=2)        # twice into the same buffers
    assert twice["bytes"] == once["bytes"]
    plain = run(hd, logits, gt, counts, fill=0xFF, grad=False)      # yolo_v3_loss alone: the same parts, images, result and table
    assert plain["bytes"] == once["bytes"][:4]


def test_a_gradient_that_is_not_16_byte_aligned():
    """the gradient kernel stores 16 bytes per lane where grad_dev allows it; 4, 8 and 12 bytes off that it must write the same values"""
    logits, gt, counts, grids, anchors, n_classes = cases.make_case("three-scales")
    hd = head_of(grids, anchors, n_classes)
    want = run(hd, logits, gt, counts, fill=0xFF)
    for shift in (4, 8, 12):
        assert run(hd, logits, gt, counts, fill=0xFF, grad_shift=shift)["bytes"] == want["bytes"], shift


# ---- rules ------------------------------------------------------------------------------------------------------------------------------
RULE_GRIDS = ((4, 4), (8, 8))
RULE_ANCHORS = [[(2., 2.)], [(4., 4.)]]         # the same anchor in the units of either scale: every truth ties, the first scale wins


def rules_batch():
    n_classes, max_gt = 3, 5
    lists = [[(0.3, 0.3, 0.5, 0.5, 0), (0.35, 0.35, 0.4, 0.4, 1)],                   # 0: two truths on one slot
             [],                                                                    # 1: no truths: nothing is ignored
             [(0.1, 0.1, 0.3, 0.3, 1), (1.0, 0.5, 0.2, 0.2, 1), (0.5, -0.1, 0.2, 0.2, 1), (0.5, 0.5, 0.0, 0.2, 1), (0.5, 0.5, 0.2, 0.2, 3)],
             [(0.1, 0.9, 0.2, 0.2, 0), (0.4, 0.9, 0.2, 0.4, 1), (0.6, 0.9, 0.4, 0.2, 2), (0.9, 0.9, 0.4, 0.4, 0), (0.9, 0.1, 0.9, 0.9, 1)],
             [(0.55, 0.55, 0.5, 0.5, 2)],                                           # 4: all-zero logits: the threshold tie
             [(0.7, 0.2, 0.3, 0.3, 0)]]                                             # 5: a NaN and an overflow on rows that are not winners
    gt, counts = raw_gts(lists, max_gt)
    counts[3] = max_gt + 1
    R = 16 + 64
    rng = np.random.RandomState(23)
    logits = rng.uniform(-4, 4, size=(6, R, 5 + n_classes)).astype(np.float32)
    # image 1: every row decodes to the box that image 0's first truth would make it ignore
    logits[1, :, :4] = 0
    logits[4] = 0
    logits[5, 3, 0] = np.nan            # scale 0, cell (0, 3): the truth's own cell is (0, 2)
    logits[5, 40, 2] = 100.             # expf overflows: an infinite box, IoU 0
    return logits, gt, counts, n_classes


def test_rules():
    logits, gt, counts, n_classes = rules_batch()
    hd = head_of(RULE_GRIDS, RULE_ANCHORS, n_classes)
    r64, r32 = (loss_v3_ref.loss(logits, RULE_GRIDS, RULE_ANCHORS, n_classes, gt, counts, cases.IGNORE, mode=m) for m in ("float64", "float32"))
    want = r32["table"]
    # the yardstick itself hits every rule
    assert r32["n_truths"].tolist() == [2, 0, 1, 5, 1, 1] and r32["n_assigned"].tolist() == [1, 0, 1, 5, 1, 1]
    assert r32["status"].tolist() == [0, 0, 7, 8, 0, 0]
    assert want[0, 1 * 4 + 1] == 1 and (want[0] >= 0).sum() == 1            # the last truth of the slot; scale 0 although scale 1 ties
    assert (want[:, 16:] < 0).all()                                           # no winner on the second scale: the first wins every tie
    assert (want[1] == -1).all() and (want[4] == -2).sum() >= 1
    assert want[5, 3] == -1 and want[5, 40] == -1 and np.isfinite(r32["sums"]).all()
    assert r32["margin"] > cases.MARGIN and np.array_equal(want, r64["table"])
    out = run(hd, logits, gt, counts)
    compare("rules", out, r64, r32)
    grad = out["grad"]
    assert (grad[5, 3, :4] == 0).all() and np.isfinite(grad[5, 3]).all() and np.isfinite(grad[5, 40]).all() and np.isfinite(out["images"]["noobj"]).all()
    # the threshold tie on image 4: scale 1, cell (4, 4) decodes exactly (sigmoid(0) = 0.5, exp(0) = 1) to (0.5625, 0.5625, 0.5, 0.5)
    row = 16 + 4 * 8 + 4
    tie = float(r32["best_iou"][4, row])
    assert tie == float(loss_v3_ref.iou64(0.5625, 0.5625, 0.5, 0.5, np.float32(0.55), np.float32(0.55), 0.5, 0.5)) and 0.7 < tie < 1
    for thresh, ignored in ((tie, False), (float(np.nextafter(tie, 0.)), True)):
        ref = loss_v3_ref.loss(logits, RULE_GRIDS, RULE_ANCHORS, n_classes, gt, counts, thresh, mode="float32")
        near = np.argwhere(np.abs(ref["best_iou"] - thresh) <= cases.MARGIN)
        assert all(int(b) == 4 for b, _ in near), near          # only rows of the all-zero image (exact decodes) sit at the threshold
        got = run(hd, logits, gt, counts, thresh=thresh)
        assert np.array_equal(got["table"], ref["table"]) and (got["table"][4, row] == -2) == ignored
        assert (got["grad"][4, row, 4] == 0) == ignored


# ---- through the nets -----------------------------------------------------------------------------------------------------------------------
HW = (96, 160)
NAMES3 = ["a", "b", "c"]
TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("model", ["v3-tiny", "v3"])
def test_net_loss_is_forward_then_the_abi(model, dtype):
    import torch
    cls, anchors = (YoloV3Tiny, TINY_ANCHORS) if model == "v3-tiny" else (YoloV3, V3_ANCHORS)
    m = cls()
    net = cls.create_network(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=HW + (3,))
    m.build(anchors, NAMES3, HW + (3,), dtype=dtype, max_batch=2, weights=synth.darknet_stream(net, seed=41, num_classes=3))
    eng = m.net.engine
    x8 = np.random.RandomState(42).randint(0, 256, size=(2,) + HW + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    truths = [[(0.3, 0.4, 0.2, 0.5, 1), (0.8, 0.2, 0.3, 0.3, 2), (0.5, 0.5, 0.9, 0.9, 0)], [(0.6, 0.6, 0.1, 0.15, 0)]]
    gt, counts = yeval.pack_gts(truths, 3)
    before = m.predict(xf, 0.3, 0.5)
    logits = eng.forward(xf).cpu().numpy()
    R, P = engine.v3_loss_rows(eng.head)
    assert logits.shape == (2, R, 8)
    want = run(eng.head, logits, gt, counts, fill=0xFF)
    for x, fn in ((xf, eng.loss_v3), (x8, eng.loss_v3_u8)):
        images, result, assign = fn(x, (gt, counts))
        got = [t.cpu().numpy().tobytes() for t in (images, result, assign)]
        assert got == want["bytes"][1:4], "yolo_net_loss_v3%s is not forward + yolo_v3_loss" % ("_u8" if x is x8 else "")
    after = m.predict(xf, 0.3, 0.5)
    key = lambda boxes: [[(b.x, b.y, b.w, b.h, b.class_idx, b.prob) for b in img] for img in boxes]
    assert key(after) == key(before), "a detect after the loss sees stale logits"
    for x in (xf, x8):
        out = m.loss_v3_grad(x, truths)
        grad = out.pop("grad")
        assert grad.is_cuda and grad.dtype == torch.float32 and grad.cpu().numpy().tobytes() == want["bytes"][4]
        plain = m.loss_v3(x, truths)
        assert set(out) == set(plain) and out["n_truths"] == 4 and out["status"] == 0 and np.isfinite(out["loss"]) and out["loss"] > 0
        for k in plain:
            assert (out[k].tobytes() == plain[k].tobytes()) if k == "images" else (out[k] == plain[k]), k
        assert out["loss"] == float(want["result"]["loss"]) and out["images"].tobytes() == want["bytes"][1]
    images, result, assign, g2 = eng.loss_v3_grad_u8(x8, (gt, counts))
    assert g2.cpu().numpy().tobytes() == want["bytes"][4] and assign.cpu().numpy().tobytes() == want["bytes"][3]


def test_a_v2_net_is_refused():
    anchors = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071]
    m = YoloV2Tiny()
    net = YoloV2Tiny.create_network(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=(32, 32, 3))
    m.build(anchors, NAMES3, (32, 32, 3), dtype="fp32", max_batch=1, weights=synth.darknet_stream(net, seed=31, num_classes=3))
    x = np.zeros((1, 32, 32, 3), dtype=np.float32)
    for fn in (m.loss_v3, m.loss_v3_grad):
        with pytest.raises(ValueError, match="version 3 heads only"):
            fn(x, [[]])


# ---- the torch op -----------------------------------------------------------------------------------------------------------------------
def test_autograd_op_is_the_abi_gradient():
    import torch
    logits, gt, counts, grids, anchors, n_classes = cases.make_case("three-scales")
    out = run(head_of(grids, anchors, n_classes), logits, gt, counts)
    x = torch.from_numpy(logits).cuda().requires_grad_()
    loss, record = yolo_v3_loss(x, (gt, counts), grids, anchors, n_classes, return_record=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad and not record.requires_grad
    assert record.cpu().numpy().tobytes() == out["bytes"][2]
    assert loss.item() == float(np.float32(out["result"]["loss"]))
    loss.backward()
    assert x.grad.shape == x.shape and x.grad.cpu().numpy().tobytes() == out["bytes"][4]
    x2 = x.detach().clone().requires_grad_()
    (2 * yolo_v3_loss(x2, (gt, counts), grids, anchors, n_classes, ignore_thresh=cases.IGNORE)).backward()
    assert x2.grad.cpu().numpy().tobytes() == (np.float32(2) * out["grad"]).tobytes()
    # lists of truths are the same truths
    lists = [[tuple(gt[b, g])[:5] for g in range(counts[b])] for b in range(len(counts))]
    x3 = x.detach().clone().requires_grad_()
    yolo_v3_loss(x3, lists, grids, anchors, n_classes).backward()
    assert x3.grad.cpu().numpy().tobytes() == out["bytes"][4]
    with pytest.raises(ValueError, match="ignore_thresh"):
        yolo_v3_loss(x3, lists, grids, anchors, n_classes, ignore_thresh=0.)


def test_descent():
    """end to end through the op: twenty steps of plain SGD on the logits themselves, the loss lower after every step and equal to four
    digits to the float64 yardstick's on the same loop (loss_v3_cases.DESCENT_LOSSES; the step size was chosen there, on the CPU)"""
    import torch
    logits, gt, counts, grids, anchors, n_classes = cases.make_case(cases.DESCENT_CASE)
    param = torch.nn.Parameter(torch.from_numpy(logits).cuda())
    opt = torch.optim.SGD([param], lr=cases.DESCENT_LR)
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(len(counts), -1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
    losses = []
    for _ in range(cases.DESCENT_STEPS + 1):
        opt.zero_grad()
        loss = yolo_v3_loss(param, (d_gt, d_gc), grids, anchors, n_classes)
        loss.backward()
        opt.step()
        losses.append(loss)
    losses = [float(v) for v in torch.stack(losses).detach().cpu()]          # the one read
    print("descent:", " ".join("%.4f" % v for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert all(abs(a - b) <= 1e-4 * b for a, b in zip(losses, cases.DESCENT_LOSSES)), (losses, cases.DESCENT_LOSSES)

"""GPU: the YOLOv2 loss entries (yolo_v2_loss, yolo_net_loss[_u8], yolo_loss_reduce, through the C ABI; Yolo.evaluate with loss = true)
against the sequential yardstick tests/loss_ref.py.

Assignment tables are compared as integers (EQUAL).  Values, per component, per image and in total: the yardstick is loss_ref in float64
mode, d = |ref_float32 - ref_float64| on the same inputs measures what float32 elementwise arithmetic costs, and the device may be off
the float64 value by FACTOR * d plus one float32 ulp of the component (device expf / sigmoid differ from NumPy's by an ulp or so per
call, the order of the float32 rounding itself).  FACTOR = 4, set by the issue before anything was measured.  Where the float32
yardstick is not finite (an overflowing exp on a winner slot) the device must return the same non-finite value.

Measured on an MI355X, (|device - ref_float64| - ulp) / d, the largest over all components, images and totals of each of the five
SHAPES: 0.000, 0.000, 1.000, 0.796 and 3.707.  The last is `wh` of image 19 of the 13 x 13 x 8 x 1 batch of 65: one winner term of 782.66
(exp(t) * anchor of some thousands), the device 1.7 float32 ulp of it from the float64 value where NumPy's float32 route happens to land
0.18 ulp away -- the device's expf against NumPy's, on a term whose own ulp is 6e-5; the next largest is 1.452.  The engineered cases:
0.686 (rules), 0.728 (overflow), 0.278 (Yolo.evaluate)."""
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest

import loss_ref
from helpers import GOLDEN
from tensorflow_yolo_amd import YoloV2, YoloV2Tiny, YoloV3Tiny, _hip
from tensorflow_yolo_amd.net import base, engine, evaluate as yeval, synth

pytestmark = pytest.mark.gpu
GUARD, PATTERN, FACTOR = 256, 0xA5, 4.0
ANCHORS8 = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071, 0.57273, 0.677385, 1.87446, 2.06253,
            3.33843, 5.47434]
SHAPES = [(1, 1, 1, 1, 1), (4, 4, 5, 20, 3), (3, 5, 2, 3, 2), (13, 13, 5, 80, 2), (13, 13, 8, 1, 65)]
COMPONENTS = (("loss_xy", "xy"), ("loss_wh", "wh"), ("loss_obj", "obj"), ("loss_noobj", "noobj"), ("loss_class", "cls"))


def guarded(nbytes):
    import torch
    t = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + GUARD


def check_guards(bufs):
    for t, _ in bufs:
        assert bool((t[:GUARD] == PATTERN).all()) and bool((t[-GUARD:] == PATTERN).all()), "a guard band was written"


def raw_gts(lists, max_gt, counts=None):
    """yolo_gt records [B, max_gt]; the records behind each list are garbage (0xFF bytes: NaN floats, class -1) that must not matter"""
    arr = np.frombuffer(b"\xff" * (len(lists) * max_gt * yeval.GT_DTYPE.itemsize), dtype=yeval.GT_DTYPE).reshape(len(lists), max_gt).copy()
    for i, img in enumerate(lists):
        for g, t in enumerate(img):
            arr[i, g] = (t[0], t[1], t[2], t[3], int(t[4]), 0)
    return arr, np.asarray([len(l) for l in lists] if counts is None else counts, dtype=np.int32)


def run_loss(h, w, anchors, n_classes, logits, gt, counts, assign=True, calls=1):
    """yolo_v2_loss through the C ABI, every output in a pattern-filled buffer with a guard band on both sides.
    -> (images LOSS_IMAGE_DTYPE [B], result record, table int32 [B, h, w] | None)"""
    import torch
    lib = _hip.lib()
    B = int(np.asarray(logits).shape[0])
    hd = engine.head_desc_v2(h, w, anchors, n_classes)
    d_logits = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)).cuda()
    d_gt = torch.from_numpy(np.ascontiguousarray(gt).view(np.uint8).reshape(-1)).cuda()
    d_gc = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).cuda()
    bufs = [guarded(B * 56), guarded(64)] + ([guarded(B * h * w * 4)] if assign else [])
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(calls):
        _hip.check(lib.yolo_v2_loss(C.byref(hd), d_logits.data_ptr(), B, d_gt.data_ptr(), d_gc.data_ptr(), gt.shape[1], bufs[0][1],
                                    bufs[2][1] if assign else None, bufs[1][1], st), "yolo_v2_loss")
    torch.cuda.synchronize()
    check_guards(bufs)
    images = bufs[0][0][GUARD:-GUARD].cpu().numpy().view(yeval.LOSS_IMAGE_DTYPE).copy()
    result = bufs[1][0][GUARD:-GUARD].cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0].copy()
    table = bufs[2][0][GUARD:-GUARD].cpu().numpy().view(np.int32).reshape(B, h, w).copy() if assign else None
    return images, result, table


def ulp32(v):
    return float(np.spacing(np.float32(abs(v)))) if np.isfinite(v) else 0.0


def compare(label, dev, r64, r32, worst):
    """one value against the yardstick: prints the figures, returns nothing, asserts the bound of the module docstring"""
    if not np.isfinite(r32):
        print("%s: device %r, float32 yardstick %r (not finite: must be the same)" % (label, dev, r32))
        assert dev == r32 or (np.isnan(dev) and np.isnan(r32)), label
        return
    d, err, ulp = abs(r32 - r64), abs(dev - r64), ulp32(r64)
    ratio = max(0.0, err - ulp) / d if d > 0 else (0.0 if err <= ulp else float("inf"))
    worst[0] = max(worst[0], ratio)
    if ratio > 1.0:
        print("%s: device %.17g ref64 %.17g ref32 %.17g |dev - ref64| %.3e d %.3e ulp %.3e ratio %.3f" % (label, dev, r64, r32, err, d, ulp, ratio))
    assert err <= FACTOR * d + ulp, (label, dev, r64, r32, ratio)


def compare_all(tag, images, result, r64, r32):
    worst = [0.0]
    try:
        for i in range(len(images)):
            for _, k in COMPONENTS:
                compare("%s image %d %s" % (tag, i, k), float(images[i][k]), r64["images"][i][k], r32["images"][i][k], worst)
            assert int(images[i]["n_assigned"]) == r64["images"][i]["n_assigned"] and int(images[i]["n_truths"]) == r64["images"][i]["n_truths"]
            assert int(images[i]["status"]) == r64["images"][i]["status"]
        for k, _ in COMPONENTS + (("loss", None),):
            compare("%s total %s" % (tag, k), float(result[k]), r64[k], r32[k], worst)
        for k in ("n_assigned", "n_truths", "status"):
            assert int(result[k]) == r64[k], k
    finally:
        print("%s: largest (|device - ref64| - ulp) / d = %.3f (bound %.1f)" % (tag, worst[0], FACTOR))
    return worst[0]


def random_case(shape, seed):
    h, w, A, n_classes, B = shape
    rng = np.random.RandomState(seed)
    logits = rng.uniform(-6, 6, size=(B, h, w, A, 5 + n_classes)).astype(np.float32)
    lists = []
    for b in range(B):
        n = 0 if (b == 1 and B > 1) else 1 + rng.randint(0, 12)
        lists.append([(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), rng.randint(0, n_classes))
                      for _ in range(n)])
    gt, counts = raw_gts(lists, 13)
    return logits, gt, counts


@functools.lru_cache(maxsize=None)
def yardstick(shape, seed):
    """computed once per shape, shared, left unchanged"""
    h, w, A, n_classes, _ = shape
    logits, gt, counts = random_case(shape, seed)
    return tuple(loss_ref.loss(logits, h, w, ANCHORS8[:2 * A], n_classes, gt, counts, mode=m) for m in ("float64", "float32"))


# ---- assignment -------------------------------------------------------------------------------------------------------------------------
RULE_ANCHORS = [1, 2, 2, 1, 0.5, 0.5, 3, 3, 1, 1]


def rule_lists():
    g = lambda x, y, bw, bh, c: (x / 4., y / 4., bw / 4., bh / 4., c)       # grid units -> normalised on the 4 x 4 grid (exact)
    return [[],                                                               # an image with no truths
            [g(0.5, 0.5, 1.125, 1.875, 3), g(0.25, 0.75, 1, 2, 4),          # cell (0, 0): the later truth fits anchor 0 exactly and wins
             g(2.5, 2.5, 2.5, 2.5, 5), g(2.25, 2.75, 0.4375, 0.5, 6), g(2.75, 2.25, 1, 1, 7)],       # cell (2, 2): three, the last wins
            [g(1.5, 3.5, 0.75, 0.75, 8), g(1.5, 3.5, 0.75, 0.75, 9),        # two identical truths: the first wins
             g(3.5, 0.5, 1.5, 1.5, 10)],                                     # equal IoU with anchors 0 (1 x 2) and 1 (2 x 1): anchor 0
            [g(2, 1, 1, 1, 11), g(0, 0, 3, 3, 12),                           # centres exactly on cell boundaries: cells (1, 2) and (0, 0)
             g(3.25, 3.25, 0, 0, 13)]]                                       # a zero-size truth takes anchor 0


def test_assignment_rules_equal_the_yardstick():
    lists = rule_lists()
    gt, counts = raw_gts(lists, 6)
    logits = np.random.RandomState(1).uniform(-6, 6, size=(4, 4, 4, 5, 25)).astype(np.float32)
    want, status, n_truths = loss_ref.assign(4, 4, RULE_ANCHORS, 20, gt, counts)
    # the yardstick itself hits every rule (truth * 8 + anchor)
    assert (want[0] == -1).all() and want[1, 0, 0] == 1 * 8 + 0 and want[1, 2, 2] == 4 * 8 + 4 and (want[1] >= 0).sum() == 2
    assert want[2, 3, 1] == 0 * 8 + 4 and want[2, 0, 3] == 2 * 8 + 0
    assert want[3, 1, 2] == 0 * 8 + 4 and want[3, 0, 0] == 1 * 8 + 3 and want[3, 3, 3] == 2 * 8 + 0
    images, result, table = run_loss(4, 4, RULE_ANCHORS, 20, logits, gt, counts)
    assert np.array_equal(table, want)
    assert images["n_assigned"].tolist() == [0, 2, 2, 3] and images["n_truths"].tolist() == [0, 5, 3, 3] and not images["status"].any()
    assert int(result["n_assigned"]) == 7 and int(result["n_truths"]) == 11 and int(result["status"]) == 0
    r64, r32 = (loss_ref.loss(logits, 4, 4, RULE_ANCHORS, 20, gt, counts, mode=m) for m in ("float64", "float32"))
    compare_all("rules", images, result, r64, r32)


def test_1024_truths_in_one_image():
    rng = np.random.RandomState(2)
    crowd = [(rng.uniform(0.25, 0.5), rng.uniform(0.5, 0.75), rng.uniform(0.01, 1.0), rng.uniform(0.01, 1.0), rng.randint(0, 20)) for _ in range(900)]
    rest = [(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.01, 1.0), rng.uniform(0.01, 1.0), rng.randint(0, 20)) for _ in range(124)]
    lists = [crowd[:500] + rest + crowd[500:], [(0.1, 0.1, 0.2, 0.2, 1), (0.9, 0.9, 0.3, 0.1, 2), (0.12, 0.1, 0.4, 0.5, 3)]]
    gt, counts = raw_gts(lists, 1024)
    logits = rng.uniform(-6, 6, size=(2, 4, 4, 5, 25)).astype(np.float32)
    want, status, n_truths = loss_ref.assign(4, 4, ANCHORS8[:10], 20, gt, counts)
    images, result, table = run_loss(4, 4, ANCHORS8[:10], 20, logits, gt, counts)
    assert np.array_equal(table, want) and (want[0] >= 0).all() and want[0].max() >> 3 > 512
    assert images["n_truths"].tolist() == [1024, 3] and images["n_assigned"].tolist() == [16, int((want[1] >= 0).sum())] and not images["status"].any()


@pytest.mark.parametrize("name,bad,count,bit", [
    ("x_is_one", (1.0, 0.5, 0.2, 0.2, 1), None, loss_ref.OUT_OF_GRID), ("y_negative", (0.5, -0.01, 0.2, 0.2, 1), None, loss_ref.OUT_OF_GRID),
    ("negative_width", (0.5, 0.5, -0.2, 0.2, 1), None, loss_ref.BAD_BOX), ("nan_height", (0.5, 0.5, 0.2, float("nan"), 1), None, loss_ref.BAD_BOX),
    ("class_minus_one", (0.5, 0.5, 0.2, 0.2, -1), None, loss_ref.BAD_CLASS), ("class_c", (0.5, 0.5, 0.2, 0.2, 20), None, loss_ref.BAD_CLASS),
    ("count_minus_one", None, -1, loss_ref.BAD_COUNT), ("count_above_max_gt", None, 9, loss_ref.BAD_COUNT)])
def test_skipped_truths_set_their_bit_and_disturb_nothing(name, bad, count, bit):
    rng = np.random.RandomState(3)
    clean = [[(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.05, 0.9), rng.uniform(0.05, 0.9), rng.randint(0, 20)) for _ in range(n)]
             for n in (7, 8, 3)]
    logits = rng.uniform(-6, 6, size=(3, 4, 4, 5, 25)).astype(np.float32)
    gt0, counts0 = raw_gts(clean, 8)
    images0, result0, table0 = run_loss(4, 4, ANCHORS8[:10], 20, logits, gt0, counts0)
    assert int(result0["status"]) == 0
    lists, counts = [list(l) for l in clean], counts0.copy()
    if bad is not None:
        lists[0].append(bad)            # behind the image's clean truths: indices, winners and sums of a correct kernel stay as they are
        counts[0] += 1
    else:
        counts[1] = count               # image 1 holds max_gt truths: clamping max_gt + 1 changes nothing; -1 empties the image
    gt, _ = raw_gts(lists, 8)
    images, result, table = run_loss(4, 4, ANCHORS8[:10], 20, logits, gt, counts)
    want, status, n_truths = loss_ref.assign(4, 4, ANCHORS8[:10], 20, gt, counts)
    assert np.array_equal(table, want) and images["status"].tolist() == status.tolist() and int(result["status"]) == bit
    assert images["n_truths"].tolist() == n_truths.tolist()
    same = [0, 1, 2] if count != -1 else [0, 2]
    assert np.array_equal(table[same], table0[same])
    for k in ("xy", "wh", "obj", "noobj", "cls", "n_assigned", "n_truths"):
        assert images[k][same].tobytes() == images0[k][same].tobytes(), k
    if count == -1:
        assert (table[1] == -1).all() and images["n_assigned"][1] == 0 and images["xy"][1] == 0 and images["cls"][1] == 0
    else:
        assert [float(result[k]) for k in yeval.LOSS_KEYS] == [float(result0[k]) for k in yeval.LOSS_KEYS]


# ---- values -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes", [1, 4])
def test_exact_case(n_classes):
    """all logits zero, anchors powers of two, B a power of two, truths at cell centres with the size of an anchor: px = c + 0.5,
    pw = aw, po = 0.5, iou = 1 exactly -- no term dropped, duplicated or taken from a neighbour"""
    h, w, anchors, B = 4, 4, [1, 1, 2, 4], 2
    lists = [[(0.5 / 4, 0.5 / 4, 1 / 4., 1 / 4., 0), (1.5 / 4, 2.5 / 4, 2 / 4., 4 / 4., n_classes - 1)], [(3.5 / 4, 3.5 / 4, 2 / 4., 4 / 4., 0)]]
    gt, counts = raw_gts(lists, 2)
    logits = np.zeros((B, h, w, 2, 5 + n_classes), dtype=np.float32)
    images, result, table = run_loss(h, w, anchors, n_classes, logits, gt, counts)
    n = 3
    assert table[0, 0, 0] == 0 and table[0, 2, 1] == 8 + 1 and table[1, 3, 3] == 1 and (table >= 0).sum() == n
    assert float(result["loss_xy"]) == 0.0 and float(result["loss_wh"]) == 0.0
    assert float(result["loss_obj"]) == 1.25 * n / B and float(result["loss_noobj"]) == 0.25 * (h * w * 2 * B - n) / B
    assert images["obj"].tolist() == [0.5, 0.25] and images["noobj"].tolist() == [0.25 * 30, 0.25 * 31]
    if n_classes == 1:
        assert float(result["loss_class"]) == 0.0 and float(result["loss"]) == 1.25 * n / B + 0.25 * (h * w * 2 * B - n) / B
    else:
        r64, r32 = (loss_ref.loss(logits, h, w, anchors, n_classes, gt, counts, mode=m) for m in ("float64", "float32"))
        assert abs(r64["loss_class"] - n * 2 * np.log(4.0)) < 1e-12
        compare_all("exact C=4", images, result, r64, r32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_values_against_the_yardstick(shape):
    h, w, A, n_classes, B = shape
    logits, gt, counts = random_case(shape, 11)
    r64, r32 = yardstick(shape, 11)
    images, result, table = run_loss(h, w, ANCHORS8[:2 * A], n_classes, logits, gt, counts)
    assert np.array_equal(table, r64["table"])
    compare_all("shape %s" % (shape,), images, result, r64, r32)


def test_overflow_and_saturation():
    """difference (b): exp overflow on a masked-out slot leaves every sum finite; on a winner slot loss_wh is inf, as in float32"""
    h, w, A, n_classes = 4, 4, 5, 20
    rng = np.random.RandomState(4)
    logits = rng.uniform(-6, 6, size=(3, h, w, A, 5 + n_classes)).astype(np.float32)
    lists = [[(0.3, 0.3, 0.2, 0.3, 1)], [(0.3, 0.3, 0.2, 0.3, 1)], [(0.6, 0.1, 0.5, 0.5, 2), (0.1, 0.9, 0.05, 0.05, 3)]]
    gt, counts = raw_gts(lists, 2)
    table, _, _ = loss_ref.assign(h, w, ANCHORS8[:10], n_classes, gt, counts)
    a = int(table[0, 1, 1]) & 7
    logits[0, 1, 1, (a + 1) % A, 2] = 100.      # image 0: t2 = 100 on a slot of the winner's CELL that is not the winner, and on a far cell
    logits[0, 3, 3, 0, 3] = 100.
    logits[1, 1, 1, a, 2] = 100.                # image 1: on the winner slot itself
    logits[2, 0, 2, :, 4] = 40.                 # image 2: saturated objectness, winner cell and elsewhere
    logits[2, 3, 0, :, 4] = -40.
    logits[2, 2, 2, :, 4] = 40.
    r64, r32 = (loss_ref.loss(logits, h, w, ANCHORS8[:10], n_classes, gt, counts, mode=m) for m in ("float64", "float32"))
    assert np.isinf(r32["images"][1]["wh"]) and np.isinf(r32["loss_wh"]) and all(np.isfinite(r32["images"][0][k]) for k in loss_ref.TERMS)
    images, result, _ = run_loss(h, w, ANCHORS8[:10], n_classes, logits, gt, counts)
    assert all(np.isfinite(float(images[0][k])) for k in loss_ref.TERMS)
    assert np.isinf(images["wh"][1]) and np.isinf(float(result["loss_wh"])) and np.isinf(float(result["loss"]))
    compare_all("overflow", images, result, r64, r32)


def test_two_calls_and_null_assign_give_identical_bits():
    shape = SHAPES[3]
    h, w, A, n_classes, B = shape
    logits, gt, counts = random_case(shape, 11)
    first = run_loss(h, w, ANCHORS8[:2 * A], n_classes, logits, gt, counts)
    again = run_loss(h, w, ANCHORS8[:2 * A], n_classes, logits, gt, counts, calls=2)        # twice into the same buffers
    plain = run_loss(h, w, ANCHORS8[:2 * A], n_classes, logits, gt, counts, assign=False)
    for other in (again, plain):
        assert other[0].tobytes() == first[0].tobytes() and other[1].tobytes() == first[1].tobytes()
    assert np.array_equal(again[2], first[2]) and plain[2] is None


def test_loss_reduce_adds_in_order_with_the_repeat():
    import torch
    rng = np.random.RandomState(6)
    n = 300                             # more than one chunk of 256
    rec = np.zeros(n, dtype=yeval.LOSS_IMAGE_DTYPE)
    for k in loss_ref.TERMS:
        rec[k] = rng.uniform(0, 10, size=n)
    rec["n_assigned"], rec["n_truths"] = rng.randint(0, 9, size=n), rng.randint(0, 20, size=n)
    rec["status"][270] = 4
    dev = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
    for repeat, bs in ((0, 300), (20, 64), (300, 8)):
        out = guarded(64)
        _hip.check(_hip.lib().yolo_loss_reduce(dev.data_ptr(), n, repeat, bs, out[1], torch.cuda.current_stream().cuda_stream), "yolo_loss_reduce")
        torch.cuda.synchronize()
        check_guards([out])
        got = out[0][GUARD:-GUARD].cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]
        want = loss_ref.totals(rec, bs, repeat)         # the same sequential float64 additions: the same bits
        for k in yeval.LOSS_KEYS + ("n_assigned", "n_truths", "status"):
            assert got[k] == want[k], (repeat, k)


# ---- through a network ------------------------------------------------------------------------------------------------------------------
HW = (96, 160)
NAMES3 = ["a", "b", "c"]
V2_ANCHORS = ANCHORS8[:10]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("cls", [YoloV2Tiny, YoloV2], ids=["v2-tiny", "v2"])
def test_net_loss_is_forward_then_loss(cls, dtype):
    import torch
    lib = _hip.lib()
    m = cls()
    net = cls.create_network(np.reshape(V2_ANCHORS, [-1, 2]), NAMES3, False, input_shape=HW + (3,))
    hg, _ = synth.HEAD_DEFAULTS[cls.version]
    weights = synth.darknet_stream(net, seed=31, num_classes=3, head_gain=hg, obj_bias=0.0)
    m.build(V2_ANCHORS, NAMES3, HW + (3,), dtype=dtype, max_batch=2, weights=weights)
    eng = m.net.engine
    x8 = np.random.RandomState(32).randint(0, 256, size=(2,) + HW + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    truths = [[(0.3, 0.4, 0.2, 0.5, 1), (0.8, 0.2, 0.3, 0.3, 2)], [(0.5, 0.5, 0.9, 0.9, 0)]]
    gt, counts = yeval.pack_gts(truths, 2)
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(-1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
    st = torch.cuda.current_stream().cuda_stream
    before = [t.clone() for t in eng.detect(xf, 0.1, 0.6)]
    assert int(before[1].sum()) > 0
    for x, fwd, loss in ((xf, eng.forward, eng.loss), (x8, eng.forward_u8, eng.loss_u8)):
        logits = fwd(x)
        bufs = [guarded(2 * 56), guarded(64)]
        _hip.check(lib.yolo_v2_loss(C.byref(eng.head), logits.data_ptr(), 2, d_gt.data_ptr(), d_gc.data_ptr(), 2, bufs[0][1], None, bufs[1][1], st),
                   "yolo_v2_loss")
        images, result, table = loss(x, truths, assign=True)
        torch.cuda.synchronize()
        check_guards(bufs)
        assert bytes(images.cpu().numpy().tobytes()) == bytes(bufs[0][0][GUARD:-GUARD].cpu().numpy().tobytes())
        assert bytes(result.cpu().numpy().tobytes()) == bytes(bufs[1][0][GUARD:-GUARD].cpu().numpy().tobytes())
        host = yeval.loss_to_host(images, result)
        assert host["n_assigned"] == 3 and host["status"] == 0 and np.isfinite(host["loss"]) and host["loss"] > 0
        assert int((table >= 0).sum()) == 3
        # ... and the pair form of the truths, and Yolo.loss, give the same record
        images2, result2 = loss(x, (gt, counts))
        assert bytes(images2.cpu().numpy().tobytes()) == bytes(images.cpu().numpy().tobytes())
        assert m.loss(x, truths)["loss"] == host["loss"]
    after = eng.detect(xf, 0.1, 0.6)        # the workspace logits / objectness bookkeeping are not left stale
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_net_loss_refuses_a_v3_net():
    import torch
    anchors = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
    m = YoloV3Tiny()
    net = YoloV3Tiny.create_network(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=HW + (3,))
    m.build(anchors, NAMES3, HW + (3,), dtype="fp16", max_batch=1, weights=synth.darknet_stream(net, seed=33, num_classes=3))
    x = np.zeros((1,) + HW + (3,), dtype=np.float32)
    with pytest.raises(ValueError, match="YOLOv2 heads only"):
        m.net.engine.loss(x, [[]])
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    rc = _hip.lib().yolo_net_loss(m.net.engine.handle, m.net.engine.to_device(x).data_ptr(), 1, p, p, 1, p, None, p, None)
    assert rc == 1 and "the reference has a loss for YOLOv2 only" in (_hip.lib().yolo_last_error() or b"").decode()


# ---- Yolo.evaluate with loss = true -------------------------------------------------------------------------------------------------------
NAMES4 = ["bicycle", "car", "dog", "tower"]


def eval_setup(tmp_path):
    img_dir, ann_dir = tmp_path / "img", tmp_path / "ann"
    img_dir.mkdir()
    ann_dir.mkdir()
    shutil.copy(os.path.join(GOLDEN, "eval", "dog", "dog_576x768.xml"), str(ann_dir))
    shutil.copy(os.path.join(GOLDEN, "dog_576x768.jpg"), str(img_dir))
    for k in (11, 12, 13):              # the tower annotations over the dog's pixels (the XML's own <size> normalises the truths)
        shutil.copy(os.path.join(GOLDEN, "eval", "eiffel", "tower%d.xml" % k), str(ann_dir))
        shutil.copy(os.path.join(GOLDEN, "dog_576x768.jpg"), str(img_dir / ("tower%d.jpg" % k)))
    return {"annotation_dir": str(ann_dir), "image_dir": str(img_dir), "batch_size": "3", "threshold": "0.1", "iou_threshold": "0.6",
            "anchors": V2_ANCHORS, "class_names": NAMES4, "input_h": str(HW[0]), "input_w": str(HW[1]), "input_c": "3", "dtype": "fp32",
            "pretrained_weights_path": ""}


def test_evaluate_with_loss(tmp_path, capsys):
    params = eval_setup(tmp_path)
    net = YoloV2Tiny.create_network(np.reshape(V2_ANCHORS, [-1, 2]), NAMES4, False, input_shape=HW + (3,))
    weights = synth.darknet_stream(net, seed=41, num_classes=4, head_gain=synth.HEAD_DEFAULTS["v2-tiny"][0], obj_bias=0.0)

    def run(extra, out):
        m = YoloV2Tiny()
        m.build(V2_ANCHORS, NAMES4, HW + (3,), dtype="fp32", max_batch=3, weights=weights, max_boxes=1024)
        m.evaluate(dict(params, out_dir=str(tmp_path / out), **extra))
        return m, json.load(open(str(tmp_path / out / "eval.json"))), capsys.readouterr().out.splitlines()

    _, plain, plain_lines = run({}, "plain")
    m, report, lines = run({"loss": "true"}, "loss")
    added = {"validation_loss", "loss_xy", "loss_wh", "loss_obj", "loss_noobj", "loss_class", "loss_batches", "loss_batch_size", "loss_status"}
    assert set(report) - set(plain) == added and {k: report[k] for k in plain} == plain and plain["images"] == 4
    assert lines[:-1] == plain_lines and lines[-1] == "validation loss: {}".format(report["validation_loss"])
    assert not any("validation loss" in l for l in plain_lines)
    assert report["loss_batches"] == 2 and report["loss_batch_size"] == 3 and report["loss_status"] == []
    # the yardstick on the logits of forward_u8 on the same resized batches, padding (2 of the first annotations) included
    eng = m.net.engine
    ann, _ = yeval.parse_voc_annotations(params["annotation_dir"], params["image_dir"], NAMES4)
    partials = {"float64": [], "float32": []}
    for start in (0, 3):
        chunk = ann[start:start + 3]
        descs, keep = eng.frame_descs(base.decode_frames([p for p, _ in chunk]))
        x = eng.preprocess_frames(descs, len(chunk), _hip.RESIZE_STRETCH, u8=True)
        logits = eng.forward_u8(x).cpu().numpy()
        gt, counts = yeval.pack_gts([t for _, t in chunk], 3)
        for mode in partials:
            partials[mode] += loss_ref.loss(logits, 3, 5, V2_ANCHORS, 4, gt, counts, mode=mode)["images"]
    want = {mode: yeval.validation_loss(np.array([tuple(r[k] for k in loss_ref.TERMS) + (0, 0, 0, 0) for r in recs], dtype=yeval.LOSS_IMAGE_DTYPE), 3)
            for mode, recs in partials.items()}
    worst = [0.0]
    for k in yeval.LOSS_KEYS:
        compare("evaluate %s" % k, report["validation_loss" if k == "loss" else k], want["float64"][k], want["float32"][k], worst)
    print("evaluate: largest ratio %.3f" % worst[0])
    assert report["validation_loss"] > 0 and m.last_loss["loss"] == report["validation_loss"]

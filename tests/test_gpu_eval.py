"""GPU: the evaluation entries (yolo_eval_reset / add / finish, through the C ABI and through net.evaluate.Evaluator) against the
sequential yardstick tests/eval_ref.py: verdicts, best truths, IoU bits, sorted order and the integer scans EQUAL, the APs within the
rounding of their sums (|dAP_voc12| <= n_tp * 2^-52: at most n_tp additions of terms in [0, 1], each rounding by at most 2^-53 of a
partial sum <= 1, on each side; |dAP_voc07| <= 11 * 2^-52; the means likewise)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import eval_ref
import spp_ref
from helpers import GOLDEN
from tensorflow_yolo_amd import YoloV3Tiny, _hip, launcher
from tensorflow_yolo_amd.net import base, evaluate as yeval, synth

pytestmark = pytest.mark.gpu
GUARD = 4096
PATTERN = 0xA5
TP, FP, IGNORED = eval_ref.TP, eval_ref.FP, eval_ref.IGNORED


def pack_boxes(dets, max_boxes):
    """list per image of (x, y, w, h, prob, class_idx) -> (float32 [B, max_boxes, 6] with the class as int32 bits, int32 counts)"""
    boxes = np.full((len(dets), max_boxes, 6), 7.0, dtype=np.float32)         # (slots behind the count hold junk that must not be read)
    counts = np.zeros(len(dets), dtype=np.int32)
    for i, img in enumerate(dets):
        counts[i] = len(img)
        for r, d in enumerate(img):
            boxes[i, r, :5] = d[:5]
            boxes[i, r, 5:6].view(np.int32)[0] = int(d[5])
    return boxes, counts


def run_eval(dets, gts, n_classes, max_boxes, det_capacity=None, max_gt=None, match_iou=0.5, calls=None, raw_counts=None, raw_gt_counts=None):
    """the dataset through the C ABI in `calls` add calls [(first image, end)], state and result in pattern-filled buffers with a 4 KiB
    guard behind each; returns (header, classes, sorted records, ctp, cfp, n_gt) as host arrays.  raw_counts / raw_gt_counts: the count
    words to pass instead of the lists' lengths (the slots are filled from the lists all the same)"""
    import torch
    lib = _hip.lib()
    total = sum(len(d) for d in dets)
    det_capacity = det_capacity or max(1, total)
    max_gt = max_gt or max(1, max(len(g) for g in gts))
    d = yeval.eval_desc(n_classes, det_capacity, max_gt, match_iou)
    sbytes, rbytes = lib.yolo_eval_state_bytes(C.byref(d)), lib.yolo_eval_result_bytes(C.byref(d))
    assert sbytes and rbytes, lib.yolo_last_error()
    lay = _hip.EvalLayout()
    _hip.check(lib.yolo_eval_state_layout(C.byref(d), C.byref(lay)))
    state = torch.full((sbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    result = torch.full((rbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _hip.check(lib.yolo_eval_reset(C.byref(d), state.data_ptr(), sbytes, st), "yolo_eval_reset")
    keep = []
    for lo, hi in calls or [(0, len(dets))]:
        boxes, counts = pack_boxes(dets[lo:hi], max_boxes)
        garr, gcounts = yeval.pack_gts(gts[lo:hi], max_gt)
        if raw_counts is not None:
            counts = np.asarray(raw_counts[lo:hi], dtype=np.int32)
        if raw_gt_counts is not None:
            gcounts = np.asarray(raw_gt_counts[lo:hi], dtype=np.int32)
        t = [torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda() for a in (boxes, counts, garr, gcounts)]
        keep.append(t)
        _hip.check(lib.yolo_eval_add(C.byref(d), state.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), hi - lo, max_boxes, t[2].data_ptr(),
                                     t[3].data_ptr(), lo, st), "yolo_eval_add")
    _hip.check(lib.yolo_eval_finish(C.byref(d), state.data_ptr(), result.data_ptr(), st), "yolo_eval_finish")
    torch.cuda.synchronize()
    assert bool((state[sbytes:] == PATTERN).all()) and bool((result[rbytes:] == PATTERN).all()), "a guard band was written"
    raw, s = result[:rbytes].cpu().numpy(), state[:sbytes].cpu().numpy()
    header = raw[:32].view(yeval.HEADER_DTYPE)[0]
    classes = raw[32:].view(yeval.CLASS_DTYPE)
    n = int(header["n_records"])
    part = lambda off, dt, m: s[int(off):int(off) + m * np.dtype(dt).itemsize].view(dt)
    assert int(part(lay.status_offset, np.uint32, 1)[0]) == int(header["status"])
    return (header, classes, part(lay.sorted_offset, yeval.RECORD_DTYPE, n), part(lay.ctp_offset, np.uint32, n),
            part(lay.cfp_offset, np.uint32, n), part(lay.n_gt_offset, np.int32, n_classes))


def same_as_ref(got, ref, status=0):
    header, classes, rec, ctp, cfp, n_gt = got
    want = ref["records"]
    assert int(header["status"]) == status and int(header["n_records"]) == len(want)
    for f in ("seq", "class_idx", "verdict", "best_gt"):
        assert np.array_equal(rec[f], want[f]), f
    assert np.array_equal(rec["prob"].view(np.uint32), want["prob"].view(np.uint32))
    assert np.array_equal(rec["best_iou"].view(np.uint64), want["best_iou"].view(np.uint64)), "IoU bits"
    assert np.array_equal(ctp, ref["ctp"]) and np.array_equal(cfp, ref["cfp"])
    assert np.array_equal(n_gt, ref["n_gt"]) and np.array_equal(classes["n_gt"], ref["n_gt"])
    for f in ("n_det", "tp", "fp", "ignored"):
        assert np.array_equal(classes[f], ref[f]), f
    worst12 = worst07 = 0.
    for c in range(len(n_gt)):
        if ref["n_gt"][c] == 0:
            assert np.isnan(classes["ap_voc12"][c]) and np.isnan(classes["ap_voc07"][c])
            continue
        e12, e07 = abs(classes["ap_voc12"][c] - ref["ap_voc12"][c]), abs(classes["ap_voc07"][c] - ref["ap_voc07"][c])
        worst12, worst07 = max(worst12, e12), max(worst07, e07)
        assert e12 <= max(1, int(ref["tp"][c])) * 2.0 ** -52 and e07 <= 11 * 2.0 ** -52, (c, e12, e07)
    n_tp = max(1, int(ref["tp"].sum()))
    if (ref["n_gt"] > 0).any():
        e12, e07 = abs(float(header["map_voc12"]) - ref["map_voc12"]), abs(float(header["map_voc07"]) - ref["map_voc07"])
        print("records %d, tp %d: max |dAP12| %.3e (bound %.3e), |dAP07| %.3e, |dmAP12| %.3e, |dmAP07| %.3e"
              % (len(want), n_tp, worst12, n_tp * 2.0 ** -52, worst07, e12, e07))
        assert e12 <= n_tp * 2.0 ** -52 and e07 <= 11 * 2.0 ** -52
    else:
        assert np.isnan(header["map_voc12"]) and np.isnan(header["map_voc07"])


# ---- 1. engineered images -----------------------------------------------------------------------------------------------------------
T = (0.5, 0.5, 0.5, 0.5)
ENGINEERED_GTS = [
    [(0.5, 0.5, 0.2, 0.2, 0, 0)],                                   # 0: two detections claim one truth
    [(0.3, 0.3, 0.2, 0.2, 1, 0), (0.3, 0.3, 0.2, 0.2, 1, 0)],       # 1: identical truths: the lowest index wins
    [T + (0, 0)],                                                   # 2: a detection inside the truth with half its area: IoU 0.5 exactly
    [(0.5, 0.5, 0.2, 0.2, 0, 1), (0.2, 0.2, 0.1, 0.1, 0, 0)],       # 3: a difficult truth
    [(0.5, 0.5, 0.2, 0.2, 1, 0)],                                   # 4: class mismatch
    [],                                                             # 5: an empty image
    [(0.5, 0.5, 0.2, 0.2, 2, 0), (0.1, 0.1, 0.1, 0.1, 0, 1)],       # 6: truths, no detections
    [(0.5, 0.5, 0.2, 0.2, 0, 0)],                                   # 7: the same prob as image 0's first: seq decides
    [(0.4, 0.4, 0., 0., 2, 0)],                                     # 8: zero-area boxes: the union floor applies
    [(0.5, 0.5, 0.2, 0.2, 0, 0)],                                   # 9: infinite w: IoU NaN (h = 0) or 0
]
ENGINEERED_DETS = [
    [(0.5, 0.5, 0.2, 0.2, 0.875, 0), (0.51, 0.5, 0.2, 0.2, 0.75, 0)],
    [(0.3, 0.3, 0.2, 0.2, 0.5, 1), (0.3, 0.3, 0.2, 0.2, 0.25, 1), (0.3, 0.3, 0.2, 0.2, 0.125, 1)],
    [(0.5, 0.5, 0.25, 0.5, 0.625, 0)],
    [(0.5, 0.5, 0.2, 0.2, 0.9375, 0), (0.5, 0.5, 0.21, 0.2, 0.5, 0), (0.2, 0.2, 0.1, 0.1, 0.25, 0)],
    [(0.5, 0.5, 0.2, 0.2, 0.5, 2)],
    [],
    [],
    [(0.5, 0.5, 0.2, 0.2, 0.875, 0)],
    [(0.4, 0.4, 0., 0., 0.5, 2)],
    [(0.5, 0.5, np.inf, 0., 0.75, 0), (0.5, 0.5, np.inf, 0.2, 0.5, 0)],
]


@pytest.mark.parametrize("match_iou", [0.5, float(np.nextafter(0.5, 0))])
def test_engineered_images_field_by_field(match_iou):
    ref = eval_ref.evaluate(ENGINEERED_DETS, ENGINEERED_GTS, 3, match_iou=match_iou, max_boxes=4)
    got = run_eval(ENGINEERED_DETS, ENGINEERED_GTS, 3, 4, det_capacity=64, match_iou=match_iou)
    same_as_ref(got, ref)
    rec = {int(r["seq"]): r for r in got[2]}
    v = lambda image, rank: (int(rec[4 * image + rank]["verdict"]), int(rec[4 * image + rank]["best_gt"]))
    assert v(0, 0) == (TP, 0) and v(0, 1) == (FP, 0)                            # the second claim is a false positive
    assert [v(1, r) for r in range(3)] == [(TP, 0), (FP, 0), (FP, 0)]           # never truth 1
    assert rec[8]["best_iou"] == 0.5 and v(2, 0) == ((FP if match_iou == 0.5 else TP), 0)      # strict comparison
    assert [v(3, r) for r in range(3)] == [(IGNORED, 0), (IGNORED, 0), (TP, 1)]
    assert v(4, 0) == (FP, -1) and rec[16]["best_iou"] == 0.0
    assert v(8, 0) == (FP, 0) and rec[32]["best_iou"] == 0.0
    assert v(9, 0) == (FP, -1) and v(9, 1) == (FP, 0)
    # equal probs: image 0 (seq 0) sorts in front of image 7 (seq 28)
    c0 = got[2][got[2]["class_idx"] == 0]
    assert c0["seq"][:3].tolist() == [12, 0, 28] and got[5].tolist() == [5, 3, 2]


# ---- 1b. boxes at a frame edge: iw * ih is NOT exact there ----------------------------------------------------------------------------
def iou_contracted(b1, b2):
    """What the IoU would be with the union contracted into one FMA: w1 * h1 + w2 * h2 (exact products, one rounding) minus the
    UNROUNDED iw * ih, rounded once -- in exact rationals.  NumPy subtracts the rounded product; this is the value that must NOT come out."""
    from fractions import Fraction as F
    x1, y1, w1, h1 = (float(np.float32(v)) for v in b1)
    x2, y2, w2, h2 = (float(np.float32(v)) for v in b2)
    iw = max(min(x1 + w1 / 2., x2 + w2 / 2.) - max(x1 - w1 / 2., x2 - w2 / 2.), 0.)
    ih = max(min(y1 + h1 / 2., y2 + h2 / 2.) - max(y1 - h1 / 2., y2 - h2 / 2.), 0.)
    s = float(F(w1) * F(h1) + F(w2) * F(h2))
    return iw * ih / max(float(F(s) - F(iw) * F(ih)), 1e-8)


# (detection, truth) with centre << extent, found by search: the contracted union gives ...b7a / ...81c / ...755 in the last digits
EDGE_PAIRS = [
    ((-0.007388080470263958, 0.008312931284308434, 0.9170951247215271, 0.5401189923286438),
     (0.0012111872201785445, 0.014179239980876446, 0.9093872904777527, 0.5450735092163086), "0x1.ebd0f1db12b7cp-1"),
    ((-0.0152154341340065, 0.02837260067462921, 0.4805592894554138, 1.0097441673278809),
     (0.0005491248448379338, 0.02689935639500618, 0.48880496621131897, 0.9966958165168762), "0x1.d9c96f795081bp-1"),
    ((-0.017515262588858604, 0.035231828689575195, 0.6917782425880432, 0.353610098361969),
     (0.004820519592612982, 0.046991389244794846, 0.700301468372345, 0.3541354537010193), "0x1.c22c0bdd1c753p-1"),
]


def test_engineered_boxes_at_the_frame_edge_iou_bits():
    dets = [[d + (0.5, 0)] for d, _, _ in EDGE_PAIRS]
    gts = [[t + (0, 0)] for _, t, _ in EDGE_PAIRS]
    for d, t, want in EDGE_PAIRS:
        assert float(eval_ref.iou([np.float64(np.float32(v)) for v in d], [np.float64(np.float32(v)) for v in t])).hex() == want
        assert iou_contracted(d, t).hex() != want                   # the case can tell the two roundings apart
    got = run_eval(dets, gts, 1, 2, det_capacity=8)
    same_as_ref(got, eval_ref.evaluate(dets, gts, 1, max_boxes=2))
    assert [float(v).hex() for v in got[2]["best_iou"]] == [want for _, _, want in EDGE_PAIRS]


def edge_dataset(seed, images, n_classes, per_image):
    """truths with centre in [0, 0.06] and extent in [0.3, 1] (large objects in the frame's corner), detections = jittered copies"""
    rng = np.random.default_rng(seed)
    dets, gts = [], []
    for _ in range(images):
        g = [(float(rng.uniform(0, .06)), float(rng.uniform(0, .06)), float(rng.uniform(.3, 1.)), float(rng.uniform(.3, 1.)),
              int(rng.integers(0, n_classes)), int(rng.random() < 0.1)) for _ in range(per_image)]
        d = []
        for t in g:
            for _ in range(2):
                j = rng.normal(0, 0.01, 4)
                d.append((t[0] + j[0], t[1] + j[1], abs(t[2] + j[2]), abs(t[3] + j[3]), int(rng.integers(1, 65)) / 64., t[4]))
        d.sort(key=lambda r: -r[4])
        dets.append(d)
        gts.append(g)
    return dets, gts


def test_random_boxes_at_the_frame_edge():
    dets, gts = edge_dataset(11, 16, 4, 24)
    # the data can tell: among the same-class pairs of the first images some IoUs differ under contraction
    pairs = [(d[:4], t[:4]) for img_d, img_t in zip(dets[:4], gts[:4]) for d in img_d for t in img_t if d[5] == t[4]]
    plain = [float(eval_ref.iou([np.float64(np.float32(v)) for v in d], [np.float64(np.float32(v)) for v in t])) for d, t in pairs]
    n_diff = sum(a != iou_contracted(d, t) for a, (d, t) in zip(plain, pairs))
    print("edge pairs %d, differing under contraction %d" % (len(pairs), n_diff))
    assert n_diff >= 3
    same_as_ref(run_eval(dets, gts, 4, 64, det_capacity=1024, max_gt=24), eval_ref.evaluate(dets, gts, 4, max_boxes=64))


# ---- 2. random accumulation ---------------------------------------------------------------------------------------------------------
def random_dataset(seed, images, n_classes, max_gts, noise, max_boxes):
    rng = np.random.default_rng(seed)
    dets, gts = [], []
    for _ in range(images):
        ng = int(rng.integers(0, max_gts + 1))
        g = [(float(rng.uniform(0.1, 0.9)), float(rng.uniform(0.1, 0.9)), float(rng.uniform(0.05, 0.4)), float(rng.uniform(0.05, 0.4)),
              int(rng.integers(0, n_classes)), int(rng.random() < 0.15)) for _ in range(ng)]
        d = []
        for t in g:
            for _ in range(int(rng.integers(0, 3))):                # jittered copies: good, poor and double claims
                j = rng.normal(0, 0.03, 4)
                d.append((t[0] + j[0], t[1] + j[1], abs(t[2] + j[2]), abs(t[3] + j[3]), int(rng.integers(1, 65)) / 64., t[4]))
        for _ in range(int(rng.integers(0, noise + 1))):
            d.append((float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0.02, 0.5)), float(rng.uniform(0.02, 0.5)),
                      int(rng.integers(1, 65)) / 64., int(rng.integers(0, n_classes))))
        d = d[:max_boxes]
        d.sort(key=lambda r: -r[4])                                 # (stable) the order yolo_net_detect* guarantees
        dets.append(d)
        gts.append(g)
    return dets, gts


def test_random_accumulation_in_two_calls():
    dets, gts = random_dataset(3, 64, 20, 40, 30, 128)
    ref = eval_ref.evaluate(dets, gts, 20, max_boxes=128)
    assert ref["tp"].sum() > 300 and ref["fp"].sum() > 300 and ref["ignored"].sum() > 20
    same_as_ref(run_eval(dets, gts, 20, 128, det_capacity=1 << 13, max_gt=40, calls=[(0, 32), (32, 64)]), ref)


# ---- 3. boundaries ------------------------------------------------------------------------------------------------------------------
def boundary_dataset():
    rng = np.random.default_rng(5)
    n_dets, n_gts = [0, 1, 63, 64, 65, 512, 513, 520], [0, 1, 64, 65, 70, 1, 64, 65]
    dets, gts = [], []
    for nd, ng in zip(n_dets, n_gts):
        g = [(float(rng.uniform(0.1, 0.9)), float(rng.uniform(0.1, 0.9)), 0.1, 0.1, int(rng.integers(0, 2)), int(k % 7 == 3)) for k in range(ng)]
        d = []
        for k in range(nd):
            if g and k % 3 == 0:
                t = g[int(rng.integers(0, len(g)))]
                d.append((t[0] + 0.01, t[1], t[2], t[3], 1.0 - (k // 4) / 256., t[4]))
            else:
                d.append((float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), 0.1, 0.1, 1.0 - (k // 4) / 256., int(rng.integers(0, 2))))
        dets.append(d)
        gts.append(g)
    return dets, gts


def test_boundaries_of_counts_and_capacity():
    dets, gts = boundary_dataset()
    total = sum(len(d) for d in dets)
    ref = eval_ref.evaluate(dets, gts, 2, max_boxes=520)
    same_as_ref(run_eval(dets, gts, 2, 520, det_capacity=total, max_gt=70), ref)       # exactly full: ok
    header, classes, rec, _, _, n_gt = run_eval(dets, gts, 2, 520, det_capacity=total - 1, max_gt=70)
    assert int(header["status"]) == _hip.EVAL_OVERFLOW and int(header["n_records"]) == total - 1
    assert int(classes["n_det"].sum()) == total - 1 and np.array_equal(n_gt, ref["n_gt"])
    assert len(np.unique(rec["seq"])) == total - 1 and set(rec["seq"].tolist()) <= set(ref["records"]["seq"].tolist())


def test_unsorted_list_and_classes_out_of_range_are_flagged():
    gts = [[(0.5, 0.5, 0.2, 0.2, 0, 0), (0.2, 0.2, 0.1, 0.1, 3, 0), (0.8, 0.8, 0.1, 0.1, -1, 0)]]
    dets = [[(0.5, 0.5, 0.2, 0.2, 0.75, 0), (0.2, 0.2, 0.1, 0.1, 0.5, 3), (0.8, 0.8, 0.1, 0.1, 0.5, -1), (0.5, 0.5, 0.2, 0.2, 0.25, 0)]]
    ref = eval_ref.evaluate(dets, gts, 3, max_boxes=4)
    assert len(ref["records"]) == 2 and ref["n_gt"].tolist() == [1, 0, 0]
    same_as_ref(run_eval(dets, gts, 3, 4, det_capacity=16), ref, status=_hip.EVAL_BAD_CLASS)
    ok = [[(0.5, 0.5, 0.2, 0.2, 0.5, 0), (0.5, 0.5, 0.2, 0.2, 0.5, 0)]]
    assert int(run_eval(ok, gts[:1], 4, 4)[0]["status"]) == _hip.EVAL_BAD_CLASS        # equal probs are in order; the truth of class -1 is not
    bad = [[(0.5, 0.5, 0.2, 0.2, 0.5, 0), (0.5, 0.5, 0.2, 0.2, 0.75, 0)]]
    assert int(run_eval(bad, [gts[0][:1]], 3, 4)[0]["status"]) == _hip.EVAL_UNSORTED


def test_max_gt_at_the_cap():
    """1024 truths in one image (the LDS cap the match kernel is sized for), 1 in the other; detections claim the first, a middle and
    the last truth"""
    cap = _hip.EVAL_MAX_GT
    rng = np.random.default_rng(17)
    g0 = [(0.03 + 0.03 * (k % 32), 0.03 + 0.03 * (k // 32), 0.02, 0.02, k % 3, int(k % 11 == 5)) for k in range(cap)]
    picks = [0, 1, 2, 511, 512, 1021, 1022, 1023] + [int(v) for v in rng.integers(0, cap, 56)]
    d0 = [(g0[k][0] + 0.001, g0[k][1], 0.02, 0.02, 1.0 - i / 128., g0[k][4]) for i, k in enumerate(picks)]
    dets, gts = [d0, [(0.5, 0.5, 0.2, 0.2, 0.5, 1)]], [g0, [(0.5, 0.5, 0.2, 0.2, 1, 0)]]
    ref = eval_ref.evaluate(dets, gts, 3, max_boxes=64)
    assert ref["tp"].sum() > 40 and ref["ignored"].sum() > 0 and 1023 in ref["records"]["best_gt"]
    same_as_ref(run_eval(dets, gts, 3, 64, det_capacity=128, max_gt=cap), ref)
    assert _hip.lib().yolo_eval_state_bytes(C.byref(yeval.eval_desc(3, 128, cap + 1, 0.5))) == 0        # refused above the cap


def test_counts_out_of_range_are_clamped_and_flagged():
    """a count above max_boxes / above max_gt is taken as the cap, one below 0 as 0, and YOLO_EVAL_BAD_COUNT is set: the kernel never
    reads or writes outside the image's slots (the guards in run_eval, and the records, say so)"""
    full_d = [(0.5, 0.5, 0.2, 0.2, 1.0 - r / 8., r % 2) for r in range(4)]
    full_g = [(0.5, 0.5, 0.2, 0.2, 0, 0), (0.5, 0.5, 0.21, 0.2, 1, 0), (0.1, 0.1, 0.1, 0.1, 1, 1)]
    dets, gts = [full_d, full_d, full_d, full_d[:2]], [full_g, full_g, full_g, full_g[:1]]
    clean = eval_ref.evaluate(dets, gts, 2, max_boxes=4)
    same_as_ref(run_eval(dets, gts, 2, 4, det_capacity=32, max_gt=3), clean)
    # detections: 4 + 5 -> 4, -1 -> 0
    want = eval_ref.evaluate([full_d, [], full_d, full_d[:2]], gts, 2, max_boxes=4)
    same_as_ref(run_eval(dets, gts, 2, 4, det_capacity=32, max_gt=3, raw_counts=[9, -1, 4, 2]), want, status=_hip.EVAL_BAD_COUNT)
    # truths: 3 + 1000 -> 3, -7 -> 0
    want = eval_ref.evaluate(dets, [full_g, [], full_g, full_g[:1]], 2, max_boxes=4)
    same_as_ref(run_eval(dets, gts, 2, 4, det_capacity=32, max_gt=3, raw_gt_counts=[1003, -7, 3, 1]), want, status=_hip.EVAL_BAD_COUNT)


# ---- 4. finish at size --------------------------------------------------------------------------------------------------------------
def test_finish_at_65536_records():
    rng = np.random.default_rng(8)
    dets, gts = [], []
    for i in range(64):
        g = [(0.1 + 0.1 * k, 0.5, 0.08, 0.3, k % 3, int(k == 7)) for k in range(8)]
        cls = np.where(rng.random(1024) < 0.9, 0, rng.integers(1, 3, 1024))
        prob = np.sort(rng.integers(1, 4096, 1024))[::-1] / 4096.
        d = []
        for r in range(1024):
            c = int(cls[r])
            p = 0.5 if c == 1 else float(prob[r])                   # class 1: one prob for all -- a pure seq sort
            if r % 16 == 0:
                t = g[int(rng.integers(0, 8))]
                d.append((t[0] + 0.005, t[1], t[2], t[3], p, c))
            else:
                d.append((float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), 0.1, 0.2, p, c))
        # class 1's constant prob must not break the order of the list: put its records where 0.5 belongs
        d.sort(key=lambda r: -r[4])
        dets.append(d)
        gts.append(g)
    ref = eval_ref.evaluate(dets, gts, 3, max_boxes=1024)
    assert len(ref["records"]) == 65536 and ref["n_det"][0] > 0.88 * 65536 and len(np.unique(ref["records"]["prob"][ref["records"]["class_idx"] == 1])) == 1
    same_as_ref(run_eval(dets, gts, 3, 1024, det_capacity=65536, max_gt=8, calls=[(0, 32), (32, 64)]), ref)


def test_finish_above_65536_records_in_a_capacity_of_2_to_the_20():
    """77 881 records (no power of two) sorted by the full 2^20 network, its padding included; few truths, so that the sequential
    yardstick stays quick -- the sort order and the scans are what this checks"""
    rng = np.random.default_rng(9)
    images, K = 80, 1024
    total = (1 << 16) + 12345
    n_dets = [total // images + (1 if i < total % images else 0) for i in range(images)]
    for j in range(0, images, 2):                                   # uneven lists, one of them full, the same total
        shift = 50 if j == 0 else int(rng.integers(0, 51))
        n_dets[j], n_dets[j + 1] = n_dets[j] + shift, n_dets[j + 1] - shift
    assert sum(n_dets) == total and max(n_dets) == K
    dets, gts = [], []
    for i, nd in enumerate(n_dets):
        g = [(0.3, 0.3, 0.2, 0.2, 0, 0), (0.7, 0.7, 0.2, 0.2, 0, int(i % 2))] if i < 6 else []
        prob = np.sort(rng.integers(1, 512, nd))[::-1] / 512.        # ties across and inside images
        cls = rng.integers(0, 4, nd)
        xy = rng.uniform(0.2, 0.8, (nd, 2))
        dets.append([(float(xy[r, 0]), float(xy[r, 1]), 0.2, 0.2, float(prob[r]), int(cls[r])) for r in range(nd)])
        gts.append(g)
    ref = eval_ref.evaluate(dets, gts, 4, max_boxes=K)
    assert len(ref["records"]) == (1 << 16) + 12345 and ref["tp"][0] >= 6
    same_as_ref(run_eval(dets, gts, 4, K, det_capacity=1 << 20, max_gt=2, calls=[(0, 32), (32, 64), (64, 80)]), ref)


# ---- 5. end to end on a small network -----------------------------------------------------------------------------------------------
NAMES3 = ["bicycle", "car", "dog"]
HW = (96, 160)
BATCH = 4


@functools.lru_cache(maxsize=None)
def net_weights():
    hg, frac = synth.HEAD_DEFAULTS["v3-tiny"]
    net = YoloV3Tiny.create_network(np.reshape(spp_ref.TINY_V3_ANCHORS, [-1, 2]), NAMES3, False, input_shape=HW + (3,))
    w = synth.darknet_stream(net, seed=21, num_classes=3, head_gain=hg, obj_bias=0.0)
    m = YoloV3Tiny()
    m.build(spp_ref.TINY_V3_ANCHORS, NAMES3, HW + (3,), dtype="fp32", max_batch=BATCH, weights=w)
    w = synth.calibrate_model(m, synth.synthetic_input(BATCH, HW[0], HW[1], 3, seed=22), 0.2)
    w.setflags(write=False)
    return w


def build_model(max_boxes=256):
    m = YoloV3Tiny()
    m.build(spp_ref.TINY_V3_ANCHORS, NAMES3, HW + (3,), dtype="fp32", max_batch=BATCH, weights=net_weights(), max_boxes=max_boxes)
    return m


def host_lists(boxes, counts):
    b, c = boxes.cpu().numpy(), counts.cpu().numpy()
    cls = b[..., 5].view(np.int32)
    return [[tuple(b[i, r, :5]) + (int(cls[i, r]),) for r in range(int(c[i]))] for i in range(len(c))]


def check_own_boxes_then_low_threshold(detect, max_boxes):
    """truths = the boxes of detect(0.5); the same boxes score 1; detect(0.1) against them equals the yardstick"""
    boxes, counts, status = detect(0.5)
    truth_lists = host_lists(boxes, counts)
    gts = [[d[:4] + (d[5], 0) for d in img] for img in truth_lists]
    n_truths = sum(len(g) for g in gts)
    assert n_truths >= 8 and int(status.cpu().max()) == 0
    ev = yeval.Evaluator(3, det_capacity=4096, max_gt=max(len(g) for g in gts))
    ev.add(boxes, counts, gts, status)
    res = ev.finish()
    assert res.status == 0 and res.n_records == n_truths and ev.images_truncated == 0
    assert np.array_equal(res.tp, res.n_gt) and not res.fp.any() and not res.ignored.any()
    for c in range(3):
        if res.n_gt[c]:
            assert abs(res.ap_voc12[c] - 1.) <= res.tp[c] * 2.0 ** -52 and abs(res.ap_voc07[c] - 1.) <= 11 * 2.0 ** -52
            prec, rec = res.precision_recall(c)
            assert np.all(prec == 1.) and rec[-1] == 1.
    assert abs(res.map_voc12 - 1.) <= n_truths * 2.0 ** -52
    # a lower threshold: more detections against the same truths
    ev.reset()
    boxes, counts, status = detect(0.1)
    dets = host_lists(boxes, counts)
    assert sum(len(d) for d in dets) > n_truths
    ev.add(boxes, counts, gts, status)
    res = ev.finish()
    ref = eval_ref.evaluate(dets, gts, 3, max_boxes=max_boxes)
    header = {"status": res.status, "n_records": res.n_records, "map_voc12": res.map_voc12, "map_voc07": res.map_voc07}
    classes = {k: getattr(res, k) for k in ("ap_voc12", "ap_voc07", "n_gt", "n_det", "tp", "fp", "ignored")}
    same_as_ref((header, classes, res.records, res.ctp, res.cfp, res.n_gt), ref)
    arrival = ev.records()
    assert sorted(arrival["seq"].tolist()) == sorted(res.records["seq"].tolist())


def test_end_to_end_small_network():
    m = build_model()
    x = synth.synthetic_input(BATCH, HW[0], HW[1], 3, seed=22)
    check_own_boxes_then_low_threshold(lambda thr: m.net.engine.detect(x, thr, 0.6), 256)


def test_end_to_end_frames_letterbox():
    rng = np.random.default_rng(23)
    frames = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in ((120, 90), (75, 200))]
    m = build_model()
    check_own_boxes_then_low_threshold(lambda thr: m.net.engine.detect_frames(frames, thr, 0.6, _hip.NMS_AGNOSTIC, _hip.RESIZE_LETTERBOX), 256)


# ---- 6. launcher --------------------------------------------------------------------------------------------------------------------
def test_launcher_mode_eval(tmp_path, capsys):
    import shutil
    img_dir, ann_dir, out_dir = tmp_path / "img", tmp_path / "ann", tmp_path / "out"
    img_dir.mkdir()
    ann_dir.mkdir()
    shutil.copy(os.path.join(GOLDEN, "dog_576x768.jpg"), str(img_dir))
    shutil.copy(os.path.join(GOLDEN, "eval", "dog", "dog_576x768.xml"), str(ann_dir))
    base.write_darknet_weights(str(tmp_path / "tiny.weights"), net_weights(), "v3")
    (tmp_path / "cfg.ini").write_text(
        "[COMMON]\nversion = v3-tiny\ninput_h = %d\ninput_w = %d\ninput_c = 3\n"
        "[TEST]\nimage_dir = img/\nout_dir = out/\nbatch_size = 2\nthreshold = 0.5\niou_threshold = 0.6\nanchors = %s\nclass_names = %s\n"
        "checkpoint_path =\npretrained_weights_path = tiny.weights\ndtype = fp32\n"
        "[EVAL]\nannotation_dir = ann/\nimage_dir = img/\nresize = letterbox\nmatch_iou = 0.3\n"
        % (HW[0], HW[1], list(spp_ref.TINY_V3_ANCHORS), json.dumps(NAMES3)))
    launcher.run(launcher.read_config(str(tmp_path / "cfg.ini")), "eval")
    lines = [l for l in capsys.readouterr().out.splitlines() if "AP12" in l or l.startswith("images_truncated")]
    report = json.load(open(str(out_dir / "eval.json")))
    # the same frames through the engine and an Evaluator of our own
    ann, skipped = yeval.parse_voc_annotations(str(ann_dir), str(img_dir), NAMES3)
    m = build_model(max_boxes=1024)
    boxes, counts, status = m.net.engine.detect_frames(base.decode_frames([ann[0][0]]), 0.005, 0.6, _hip.NMS_AGNOSTIC, _hip.RESIZE_LETTERBOX)
    ev = yeval.Evaluator(3, max_gt=3, match_iou=0.3)
    ev.add(boxes, counts, [ann[0][1]], status)
    res = ev.finish()
    want = res.to_json(NAMES3)
    assert report["n_records"] == want["n_records"] == int(counts.cpu().sum()) and report["n_records"] > 10
    for k in ("map_voc12", "map_voc07", "status", "classes"):
        assert report[k] == want[k], k
    assert report["images"] == 1 and report["names_skipped"] == {"tree": 1} and report["match_iou"] == 0.3 and report["threshold"] == 0.005
    assert [c["n_gt"] for c in report["classes"]] == [1, 0, 1]              # the car is difficult
    want.update(images=1, images_truncated=ev.images_truncated, names_skipped=skipped)
    from tensorflow_yolo_amd.net.yolo import eval_lines
    assert lines == eval_lines(want) and len(lines) >= 3

"""The yardstick of the evaluation tests: a plain sequential NumPy / Python VOC evaluator, written as VOCdevkit's voc_eval walks the
data -- ONE global sort of all detections, then one pass over them -- and not as the device kernel does it (per image, in parallel).
Agreement with it therefore also checks that the per-image matching equals the global sequential rule.

Definitions (restated from include/yolo_hip.h):

  IoU         the reference's net/base.py:180-192 in float64, all eight float32 fields promoted, union floored at 1e-8 (np.maximum).
  best truth  of a detection: among the truths of the SAME image and SAME class_idx, difficult ones included, the one of largest IoU;
              ties go to the lowest index (np.argmax); an IoU that is NaN never wins.  None: best_gt = -1, best_iou = 0, verdict FP.
  verdict     detections in the global order (prob descending, then seq ascending; seq = image_index * max_boxes + rank in the image's
              list).  best_iou > match_iou (STRICT, as VOCdevkit and Darknet) and the best truth difficult: IGNORED, the truth is not
              taken.  best_iou > match_iou and the best truth not yet taken: TP, and it is taken.  Otherwise FP.
  per class   n_gt = non-difficult truths; records sorted by (prob descending, seq ascending); ctp / cfp integer cumulative counts over
              the records that are not IGNORED; recall = ctp / n_gt, precision = ctp / max(ctp + cfp, eps) in float64;
              ap_voc12 = sum over the TPs of (precision envelope at that TP) / n_gt; ap_voc07 = sum over i = 0..10 of
              (max precision at recall >= i / 10.0, else 0) / 11.  n_gt == 0: NaN, the class is left out of the mean.
  mAP         mean over the classes with truths, NaN if there are none.
"""
import numpy as np

FP, TP, IGNORED = 0, 1, 2
EPS = np.finfo(np.float64).eps


def iou(box1, box2):
    """net/base.py:180-192 on float64 (x, y, w, h); the fields of box2 may be arrays (one IoU per truth: the same elementwise operations)"""
    x1, y1, w1, h1 = (np.float64(v) for v in box1)
    x2, y2, w2, h2 = (np.asarray(v, dtype=np.float64) for v in box2)
    with np.errstate(invalid="ignore", over="ignore"):
        box1_min, box1_max = (x1 - w1 / 2., y1 - h1 / 2.), (x1 + w1 / 2., y1 + h1 / 2.)
        box2_min, box2_max = (x2 - w2 / 2., y2 - h2 / 2.), (x2 + w2 / 2., y2 + h2 / 2.)
        intersect_w = np.maximum(np.minimum(box1_max[0], box2_max[0]) - np.maximum(box1_min[0], box2_min[0]), 0)
        intersect_h = np.maximum(np.minimum(box1_max[1], box2_max[1]) - np.maximum(box1_min[1], box2_min[1]), 0)
        intersect_area = intersect_w * intersect_h
        union_area = np.maximum(w1 * h1 + w2 * h2 - intersect_area, 1e-8)
        return intersect_area / union_area


def _f32(v):
    return np.float64(np.float32(v))


def evaluate(dets, gts, n_classes, match_iou=0.5, max_boxes=1024, image_base=0):
    """dets[i]: list of (x, y, w, h, prob, class_idx) of image i in list order; gts[i]: list of (x, y, w, h, class_idx, difficult).
    Values are taken as float32.  Returns a dict:
      records   structured array in the SORTED order (class ascending, prob descending, seq ascending) with fields
                best_iou f8, prob f4, class_idx i4, seq u4, verdict i4, best_gt i4
      ctp, cfp  uint32 per sorted position (IGNORED records repeat the counts in front of them)
      n_gt, n_det, tp, fp, ignored   int arrays [n_classes];  ap_voc12, ap_voc07 float64 [n_classes];  map_voc12, map_voc07
    Detections and truths with a class outside [0, n_classes) are skipped."""
    n_gt = np.zeros(n_classes, dtype=np.int64)
    for img in gts:
        for g in img:
            if 0 <= int(g[4]) < n_classes and not int(g[5]):
                n_gt[int(g[4])] += 1
    # every detection of the dataset, then the ONE global sort
    flat = []
    for i, img in enumerate(dets):
        for r, d in enumerate(img):
            c = int(d[5])
            if 0 <= c < n_classes:
                flat.append((np.float32(d[4]), (image_base + i) * max_boxes + r, i, c, d))
    flat.sort(key=lambda t: (-float(t[0]), t[1]))
    taken = [np.zeros(len(img), dtype=bool) for img in gts]
    gt_f64 = [np.array([[np.float32(v) for v in g[:4]] for g in img], dtype=np.float64).reshape(-1, 4) for img in gts]
    gt_cls = [np.array([int(g[4]) for g in img], dtype=np.int64) for img in gts]
    out = []
    for prob, seq, i, c, d in flat:
        cand = np.nonzero(gt_cls[i] == c)[0]
        best_gt, best_iou, verdict = -1, np.float64(0.), FP
        if len(cand):
            t = gt_f64[i][cand]
            ious = np.asarray(iou([_f32(v) for v in d[:4]], (t[:, 0], t[:, 1], t[:, 2], t[:, 3])), dtype=np.float64)
            v = np.where(np.isnan(ious), -1., ious)
            j = int(np.argmax(v))
            if v[j] >= 0.:
                best_gt, best_iou = int(cand[j]), ious[j]
        if best_gt >= 0 and best_iou > match_iou:
            if int(gts[i][best_gt][5]):
                verdict = IGNORED
            elif not taken[i][best_gt]:
                taken[i][best_gt] = True
                verdict = TP
        out.append((best_iou, prob, c, seq, verdict, best_gt))
    dt = np.dtype([("best_iou", "f8"), ("prob", "f4"), ("class_idx", "i4"), ("seq", "u4"), ("verdict", "i4"), ("best_gt", "i4")])
    rec = np.array(out, dtype=dt) if out else np.zeros(0, dtype=dt)
    # class ascending; inside a class the global order is kept (the sort is stable)
    rec = rec[np.argsort(rec["class_idx"], kind="stable")]
    res = {"records": rec, "n_gt": n_gt, "ctp": np.zeros(len(rec), dtype=np.uint32), "cfp": np.zeros(len(rec), dtype=np.uint32)}
    for k in ("n_det", "tp", "fp", "ignored"):
        res[k] = np.zeros(n_classes, dtype=np.int64)
    res["ap_voc12"] = np.full(n_classes, np.nan)
    res["ap_voc07"] = np.full(n_classes, np.nan)
    for c in range(n_classes):
        sel = np.nonzero(rec["class_idx"] == c)[0]
        verdict = rec["verdict"][sel]
        ctp_all = np.cumsum(verdict == TP)
        cfp_all = np.cumsum(verdict == FP)
        res["ctp"][sel] = ctp_all
        res["cfp"][sel] = cfp_all
        res["n_det"][c], res["tp"][c], res["fp"][c] = len(sel), int((verdict == TP).sum()), int((verdict == FP).sum())
        res["ignored"][c] = int((verdict == IGNORED).sum())
        if n_gt[c] == 0:
            continue
        keep = verdict != IGNORED                   # the devkit drops them before it accumulates
        res["ap_voc12"][c], res["ap_voc07"][c] = average_precision(verdict[keep] == TP, int(n_gt[c]))
    have = n_gt > 0
    res["map_voc12"] = _mean(res["ap_voc12"][have])
    res["map_voc07"] = _mean(res["ap_voc07"][have])
    return res


def _mean(values):
    if len(values) == 0:
        return float("nan")
    s = np.float64(0.)
    for v in values:
        s = s + v
    return float(s / np.float64(len(values)))


def average_precision(is_tp, n_gt):
    """(ap_voc12, ap_voc07) of one class: is_tp = bool per detection in (prob descending, seq ascending) order, IGNORED ones removed"""
    is_tp = np.asarray(is_tp, dtype=bool)
    tp = np.cumsum(is_tp).astype(np.float64)
    fp = np.cumsum(~is_tp).astype(np.float64)
    rec = tp / np.float64(n_gt)
    prec = tp / np.maximum(tp + fp, EPS)
    # monotone envelope, from the end
    env = prec.copy()
    for k in range(len(env) - 2, -1, -1):
        env[k] = max(env[k], env[k + 1])
    ap12 = np.float64(0.)
    for k in np.nonzero(is_tp)[0]:
        ap12 = ap12 + env[k] / np.float64(n_gt)
    ap07 = np.float64(0.)
    for i in range(11):
        at = rec >= i / 10.0
        p = np.max(prec[at]) if at.any() else np.float64(0.)
        ap07 = ap07 + p / 11.
    return float(ap12), float(ap07)

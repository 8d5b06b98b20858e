"""The oracle's greedy NMS with the inner loop vectorised, for inputs too large for the pure-Python restatement.

Same semantics as oracle/decode_ref.py non_maximum_suppression / non_maximum_suppression_per_class (stable sort by prob
descending, float64 IoU with the NaN-propagating 1e-8 union floor, suppress at IoU >= thr); checked against those pinned
restatements by tests/test_host_logic.py: test_vector_nms_equals_the_pinned_restatements."""
import numpy as np


def vector_nms(x, y, w, h, prob, thr, cls=None, per_class=False):
    """indices of the kept boxes, in output order.  per_class: only a kept box of the SAME class suppresses."""
    order = np.argsort(-prob.astype(np.float64), kind="stable")
    x = x.astype(np.float64)[order]; y = y.astype(np.float64)[order]; w = w.astype(np.float64)[order]; h = h.astype(np.float64)[order]
    x1, y1, x2, y2 = (x - w / 2.) * 1., (y - h / 2.) * 1., (x + w / 2.) * 1., (y + h / 2.) * 1.
    area = w * h
    if per_class:
        cls = np.asarray(cls)[order]
    alive = np.ones(len(order), bool)
    keep = []
    with np.errstate(invalid="ignore"):
        for i in range(len(order)):
            if not alive[i]:
                continue
            keep.append(order[i])
            iw = np.maximum(np.minimum(x2[i], x2[i + 1:]) - np.maximum(x1[i], x1[i + 1:]), 0)
            ih = np.maximum(np.minimum(y2[i], y2[i + 1:]) - np.maximum(y1[i], y1[i + 1:]), 0)
            inter = iw * ih
            union = np.maximum(area[i] + area[i + 1:] - inter, 1e-8)
            hit = inter / union >= thr
            if per_class:
                hit &= cls[i + 1:] == cls[i]
            alive[i + 1:] &= ~hit
    return keep


def random_boxes(rng, n):
    """n random boxes; probabilities rounded to three decimals: exact ties, so the stable order matters"""
    xy = rng.uniform(0.05, 0.95, size=(n, 2)).astype(np.float32)
    wh = rng.uniform(0.02, 0.25, size=(n, 2))
    prob = np.round(rng.uniform(0.3, 1.0, size=n), 3).astype(np.float32)
    return xy, wh, prob, rng.randint(0, 80, size=n)


def clustered_boxes(rng, n, centres=300):
    """n boxes around a few hundred centres, sizes near 0.05: greedy NMS keeps a few per centre however large n is"""
    c = rng.uniform(0.05, 0.95, size=(centres, 2))
    xy = (c[rng.randint(0, centres, size=n)] + rng.normal(0, 0.004, size=(n, 2))).astype(np.float32)
    wh = rng.uniform(0.045, 0.055, size=(n, 2))
    prob = np.round(rng.uniform(0.3, 1.0, size=n), 3).astype(np.float32)
    return xy, wh, prob, rng.randint(0, 4, size=n)

"""Inputs and figures that the CPU and the GPU tests of the YOLOv3 loss share: the shapes with the seed each one uses, the generator that
plants predictions near the truths (so that the ignore branch fires), the two yardsticks of every case (computed once, read-only) and
the comparisons.

A case is (grids, A, C, B, truths): grids = ((h, w), ...) in head order, A anchors per scale, C classes, B images, truths = how many
truths every image gets (an int -> 1 + randint(0, n) per image and none in image 1; a tuple -> exactly those counts).

The comparisons are the project's rules: a sum may be off the float64 yardstick by FACTOR * d + one float32 ulp of it, d being the
yardstick's own float32-against-float64 gap (tests/test_gpu_loss.py); a group of gradient elements by FACTOR * E_32 + ulp32(M)
(tests/loss_grad_cases.py, whose group_figures and FACTOR are used as they are)."""
import functools

import numpy as np

import loss_v3_ref
from loss_grad_cases import FACTOR, group_figures, raw_gts, ulp32      # noqa: F401  (re-exported: one rule, one place)

IGNORE = 0.7
MARGIN = 1e-5           # no (row, truth) IoU of a case may lie this close to IGNORE: the device's expf differs from NumPy's by a few float32
#                         ulps, which moves an IoU by less than 1e-6; this is ten times that
# anchors as fractions of the image, coarse scale first (the COCO anchors of yolov3.cfg over 416, rounded); in grid units: times (w_s, h_s)
ANCHORS_NORM = (((0.28, 0.22), (0.375, 0.476), (0.897, 0.784)), ((0.072, 0.147), (0.149, 0.108), (0.142, 0.286)),
                ((0.024, 0.031), (0.038, 0.072), (0.079, 0.055)), ((0.012, 0.016), (0.02, 0.04), (0.045, 0.03)))


def anchors_for(grids, A):
    return [[(ANCHORS_NORM[s][a][0] * w, ANCHORS_NORM[s][a][1] * h) for a in range(A)] for s, (h, w) in enumerate(grids)]


def rows_for(grids, A):
    return sum(h * w * A for h, w in grids)


# name -> (grids, A, C, B, truths, seed).  What each shape is for: see the table of tests/test_gpu_loss_v3.py.  Seed 7 unless the yardstick
# is degenerate there by the rule of loss_grad_cases.py (E_32 / ulp32(M) of the wh group: 0.17 at "tiny", 0.23 at "parts"); then the next
# seed that is not.
GPU_CASES = {
    "smallest": (((1, 1),), 1, 1, 1, (1,), 7),
    "three-scales": (((2, 3), (4, 6), (8, 12)), 3, 3, 3, 12, 7),
    "tiny": (((3, 3), (6, 6)), 3, 20, 2, 12, 8),
    "row-of-85": (((4, 4), (8, 8), (16, 16)), 3, 80, 2, 12, 7),
    "parts": (((13, 13), (26, 26), (52, 52)), 3, 1, 2, (9, 4), 8),
    "long-class-row": (((2, 2), (4, 4)), 3, 150, 2, 12, 7),
    "batch-65": (((2, 2), (4, 4)), 3, 2, 65, 3, 7),
    "truth-edges": (((4, 4), (8, 8)), 3, 3, 3, (0, 1, 1024), 7),
}
DESCENT_CASE, DESCENT_LR, DESCENT_STEPS = "three-scales", 1.0, 20
# the float64 yardstick's losses on that loop (tests/test_loss_v3_cpu.py recomputes the first three): descent_losses() printed them; lr 2 descends as well, lr 4 diverges
DESCENT_LOSSES = (490.0298, 435.4023, 389.3160, 347.5860, 309.7126, 275.5989, 245.1559, 218.2508, 194.6987, 174.2627, 156.6619, 141.5853,
                  128.7112, 117.7252, 108.3363, 100.2857, 93.3505, 87.3432, 82.1088, 77.5198, 73.4722)


def logit(p):
    return float(np.log(p / (1. - p)))


def make_case(name):
    """-> (logits float32 [B, R, 5 + C], gt, counts, grids, anchors, C)"""
    grids, A, C, B, truths, seed = GPU_CASES[name]
    anchors = anchors_for(grids, A)
    R, scales = loss_v3_ref.rows_of(grids, anchors)
    rng = np.random.RandomState(seed)
    logits = rng.uniform(-4, 4, size=(B, R, 5 + C)).astype(np.float32)
    lists = []
    for b in range(B):
        n = truths[b] if isinstance(truths, tuple) else (0 if (b == 1 and B > 1) else 1 + rng.randint(0, truths))
        lists.append([(rng.uniform(0.02, 0.98), rng.uniform(0.02, 0.98), rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.6), rng.randint(0, C))
                      for _ in range(n)])
    max_gt = max(1, max(len(l) for l in lists))
    gt, counts = raw_gts(lists, max_gt)
    # planted predictions: for the first truths of an image, every row of the truth's cell at every scale gets box logits that decode
    # to the truth with a jitter of up to +-0.35 in the log of the size -- IoUs on both sides of IGNORE.  Winner rows are planted too
    # (they are never ignored).
    for b in range(B):
        for t in lists[b][:8]:
            x, y, w, h = (float(np.float32(v)) for v in t[:4])
            for s, (row0, hs, ws, na) in enumerate(scales):
                cc, cr = int(np.floor(x * ws)), int(np.floor(y * hs))
                for a in range(na):
                    r = row0 + (cr * ws + cc) * na + a
                    fx, fy = min(max(x * ws - cc, 0.02), 0.98), min(max(y * hs - cr, 0.02), 0.98)
                    logits[b, r, 0] = logit(fx) + rng.uniform(-0.1, 0.1)
                    logits[b, r, 1] = logit(fy) + rng.uniform(-0.1, 0.1)
                    logits[b, r, 2] = np.log(w * ws / anchors[s][a][0]) + rng.uniform(-0.35, 0.35)
                    logits[b, r, 3] = np.log(h * hs / anchors[s][a][1]) + rng.uniform(-0.35, 0.35)
    return logits, gt, counts, grids, anchors, C


@functools.lru_cache(maxsize=None)
def yardsticks(name):
    """(ref64, ref32) of make_case(name): loss_v3_ref.loss dicts, computed once, shared, read-only"""
    logits, gt, counts, grids, anchors, C = make_case(name)
    out = tuple(loss_v3_ref.loss(logits, grids, anchors, C, gt, counts, IGNORE, mode=m) for m in ("float64", "float32"))
    for r in out:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def check_value(label, dev, r64, r32, factor=FACTOR):
    """the rule of tests/test_gpu_loss.py: |dev - ref64| <= factor * |ref32 - ref64| + ulp32(ref64); prints, asserts, -> the ratio"""
    if not np.isfinite(r32):
        assert (np.isnan(dev) and np.isnan(r32)) or dev == r32, (label, dev, r32)
        return 0.0
    d, err, ulp = abs(r32 - r64), abs(dev - r64), ulp32(r64)
    ratio = max(0.0, err - ulp) / d if d > 0 else (0.0 if err <= ulp else float("inf"))
    if ratio > 1.0:
        print("%s: device %.17g ref64 %.17g ref32 %.17g |dev - ref64| %.3e d %.3e ulp %.3e ratio %.3f" % (label, dev, r64, r32, err, d, ulp, ratio))
    assert err <= factor * d + ulp, (label, dev, r64, r32, ratio)
    return ratio


def descent_losses(steps=DESCENT_STEPS, lr=DESCENT_LR, name=DESCENT_CASE):
    """plain SGD on the logits with the float64 yardstick: the losses of steps + 1 evaluations"""
    logits, gt, counts, grids, anchors, C = make_case(name)
    x = logits.astype(np.float64)
    out = []
    for _ in range(steps + 1):
        r = loss_v3_ref.loss(x.astype(np.float32), grids, anchors, C, gt, counts, IGNORE, mode="float64")
        out.append(r["totals"]["loss"])
        x = (x.astype(np.float32) - np.float32(lr) * r["grad"].astype(np.float32)).astype(np.float64)
    return out

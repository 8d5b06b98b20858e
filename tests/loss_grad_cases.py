"""Inputs and figures that the CPU and the GPU tests of the loss gradient share: the random cases (as test_gpu_loss.random_case), the
shapes of the device test with the seed each one uses, and the per-group comparison of a gradient against the two yardsticks.

Groups of elements of a row: xy = 0-1, wh = 2-3, obj = 4, cls = 5 and up.  Per call and per group, over the elements where the float32
yardstick is finite:  E_dev = max|device - ref64|,  E_32 = max|ref32 - ref64|,  M = max|ref64|;  the bound is
E_dev <= FACTOR * E_32 + ulp32(M).  A seed is usable for a shape when the yardstick alone is non-degenerate there: every group with
M > 0 has E_32 >= 0.25 * ulp32(M) (test_loss_grad_cpu.py asserts it for every entry of GPU_CASES)."""
import functools

import numpy as np

import loss_grad_ref
from tensorflow_yolo_amd.net import evaluate as yeval

ANCHORS8 = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071, 0.57273, 0.677385, 1.87446, 2.06253,
            3.33843, 5.47434]
FACTOR = 4.0
GROUPS = (("xy", slice(0, 2)), ("wh", slice(2, 4)), ("obj", slice(4, 5)), ("cls", slice(5, None)))
# (h, w, A, C, B) -> seed.  What each shape is for: a single slot with a 6-float row; a general small case; a non-square grid; the real
# head (an 85-float row is more than one wave pass); 8 anchors (the full `win & 7` range) and a batch above any chunking; rows of exactly
# 64 and 65 floats; three passes over a row; YOLO_LOSS_MAX_CELLS cells.
# Seed 7 unless the yardstick is degenerate there (E_32 / ulp32(M) of the wh group: 0.24 at (1, 1, 1, 1, 1), 0.15 at (2, 2, 1, 150, 2), 0.08 at
# (64, 64, 1, 1, 1)); then the next seed that is not.
GPU_CASES = (((1, 1, 1, 1, 1), 9), ((4, 4, 5, 20, 3), 7), ((3, 5, 2, 3, 2), 7), ((13, 13, 5, 80, 2), 7), ((13, 13, 8, 1, 65), 7),
             ((2, 3, 2, 59, 2), 7), ((2, 3, 2, 60, 2), 7), ((2, 2, 1, 150, 2), 8), ((64, 64, 1, 1, 1), 8),
             # ... and where loss_grad_kernel takes another path: three and four anchors (lane groups of 16, one group idle at three); the
             # longest row a lane group of 8 keeps in registers (128 floats) and the first that takes three passes over memory; the same
             # step for a group of 64 (1024 floats in registers, 1025 not)
             ((2, 2, 3, 7, 2), 7), ((2, 2, 4, 7, 2), 7), ((1, 2, 5, 123, 2), 7), ((1, 2, 5, 124, 2), 7), ((1, 1, 1, 1020, 2), 10))


def raw_gts(lists, max_gt, counts=None):
    """yolo_gt records [B, max_gt]; the records behind each list are garbage (0xFF bytes: NaN floats, class -1) that must not matter"""
    arr = np.frombuffer(b"\xff" * (len(lists) * max_gt * yeval.GT_DTYPE.itemsize), dtype=yeval.GT_DTYPE).reshape(len(lists), max_gt).copy()
    for i, img in enumerate(lists):
        for g, t in enumerate(img):
            arr[i, g] = (t[0], t[1], t[2], t[3], int(t[4]), 0)
    return arr, np.asarray([len(l) for l in lists] if counts is None else counts, dtype=np.int32)


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
def yardsticks(shape, seed):
    """(ref64, ref32) of random_case(shape, seed): computed once, shared, read-only"""
    h, w, A, n_classes, _ = shape
    logits, gt, counts = random_case(shape, seed)
    out = tuple(loss_grad_ref.grad(logits, h, w, ANCHORS8[:2 * A], n_classes, gt, counts, mode=m) for m in ("float64", "float32"))
    for g in out:
        g.setflags(write=False)
    return out


def ulp32(v):
    return float(np.spacing(np.float32(abs(v)))) if np.isfinite(v) else 0.0


def group_figures(r64, r32, dev=None):
    """-> {group: dict(M, E_32, ulp[, E_dev, ratio = (E_dev - ulp) / E_32])} over the elements where ref32 is finite"""
    out = {}
    for name, sl in GROUPS:
        a64, a32 = r64[..., sl].astype(np.float64), r32[..., sl].astype(np.float64)
        ok = np.isfinite(a32)
        if not ok.any():
            continue
        fig = {"M": float(np.max(np.abs(a64[ok]))), "E_32": float(np.max(np.abs(a32[ok] - a64[ok])))}
        fig["ulp"] = ulp32(fig["M"])
        if dev is not None:
            d = dev[..., sl].astype(np.float64)[ok]
            with np.errstate(invalid="ignore"):
                gap = np.abs(d - a64[ok])
            fig["E_dev"] = float(np.max(gap)) if np.isfinite(d).all() else float("inf")
            over = max(0.0, fig["E_dev"] - fig["ulp"])
            fig["ratio"] = over / fig["E_32"] if fig["E_32"] > 0 else (0.0 if over == 0 else float("inf"))
        out[name] = fig
    return out

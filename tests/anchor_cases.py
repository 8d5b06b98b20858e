"""The cases the anchor k-means tests share: the data, the starting centres, and the lists the CPU tests (which check on the yardstick that a
case shows what it is there for) and the GPU tests (which compare the library with the yardstick, bit for bit) both walk.  CHUNK is the
library's chunk of boxes per workgroup; tests/test_anchors_cpu.py pins it against yolo_anchor_plan."""
import numpy as np

CHUNK = 1024
LLOYD_N = [1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
LLOYD_K = [1, 2, 5, 9, 32]
DISTANCES = ["euclidean", "iou"]
SEEDS = [0, 1, 2 ** 63]


def boxes(n, seed):
    """log-normal(-1.5, 0.8) sizes clipped to [0.01, 1]: float64 [n, 2], not quantised"""
    rng = np.random.default_rng(seed)
    return np.clip(rng.lognormal(-1.5, 0.8, size=(n, 2)), 0.01, 1.0)


def start(wh, k, seed):
    """k starting centres: boxes of the data where there are enough (different ones), else drawn like them"""
    rng = np.random.default_rng(1000 + seed)
    if len(wh) >= k:
        return wh[rng.choice(len(wh), size=k, replace=False)].copy()
    return np.clip(rng.lognormal(-1.5, 0.8, size=(k, 2)), 0.01, 1.0)


def duplicates(n, distinct, seed):
    """n boxes drawn from `distinct` different ones"""
    rng = np.random.default_rng(seed)
    return boxes(distinct, seed)[rng.integers(0, distinct, size=n)]


def with_bad_boxes(wh):
    """the data with one box of every invalid kind put in (and two that are just valid): -> (data, indices of the invalid ones)"""
    wh = np.array(wh, dtype=np.float64)
    bad = [(3, (0.0, 0.5)), (7, (0.5, -0.25)), (11, (1.0000001, 0.5)), (12, (np.nan, 0.5)), (20, (0.5, np.inf)), (21, (-np.inf, 0.5)),
           (30, (2.0 ** -42, 0.5)), (31, (0.5, 2.0 ** -41))]               # 2^-41 * 2^40 = 0.5 rounds to the even 0
    for i, v in bad:
        wh[i] = v
    wh[40] = (1.5 * 2.0 ** -41, 1.0)                                       # 0.75 rounds to 1: valid, as is exactly 1
    wh[41] = (2.0 ** -40, 2.0 ** -40)
    return wh, [i for i, _ in bad]


# name -> (data, k, keyword arguments of the yardstick / of kmeans_anchors): Lloyd from given centres
def stop_cases():
    wh = boxes(700, 5)
    c = start(wh, 5, 5)
    out = {}
    for tol in (0.0, 0.005, 1e9):
        out["tolerate_%g" % tol] = (wh, 5, dict(init=c, tolerate=tol, n_init=1))
    for m in (1, 2):
        out["max_iter_%d" % m] = (wh, 5, dict(init=c, tolerate=0.0, max_iter=m, n_init=1))
    out["labels_first"] = (boxes(40, 6), 3, dict(init=start(boxes(40, 6), 3, 6), tolerate=1e-12, n_init=1))
    out["tolerance_first"] = (boxes(2000, 7), 9, dict(init=start(boxes(2000, 7), 9, 7), tolerate=0.005, n_init=1))
    return out


def tie_cases():
    out = {}
    d = duplicates(500, 12, 8)
    out["duplicates"] = (d, 4, dict(init=start(boxes(12, 8), 4, 8), n_init=1))
    wh = boxes(100, 9)
    c = start(wh, 3, 9)
    c[2] = c[0]
    out["identical_centres"] = (wh, 3, dict(init=c, n_init=1, max_iter=1, tolerate=0.0))
    # (0.5, 0.5) is exactly as far from (0.25, 0.5) as from (0.75, 0.5): the first takes it
    out["equidistant"] = (np.array([[0.5, 0.5], [0.25, 0.5], [0.75, 0.5], [0.25, 0.5]]), 2,
                          dict(init=np.array([[0.25, 0.5], [0.75, 0.5]]), n_init=1, max_iter=1, tolerate=0.0))
    return out

"""The yardstick of the anchor k-means tests: a sequential NumPy / Python-int restatement of "Anchor k-means on the device" in
include/yolo_hip.h, written from the definition and sharing no code with the library or with net/anchors.py.  Sums are Python ints (exact,
any size), float64 operations are single NumPy operations (each rounded on its own), restarts run one after the other, and Philox is
tests/augment_ref.py's (whose known answers tests/test_anchors_cpu.py checks again)."""
import numpy as np

from augment_ref import philox4x32_10

EUCLIDEAN, IOU = 0, 1
BAD_BOX, EMPTY_CLUSTER, DEGENERATE, MAX_ITER = 1, 2, 4, 8
MAX_K = 32
TWO40 = float(2 ** 40)


def quantise(wh):
    """float64 [n, 2] -> (q int64 [n, 2], valid bool [n]); q is 0 where the box is not valid"""
    wh = np.asarray(wh, dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(wh) & (wh > 0.0) & (wh <= 1.0)
        q = np.where(ok, np.rint(np.where(ok, wh, 0.0) * TWO40), 0.0).astype(np.int64)
    valid = (q >= 1).all(axis=1)
    q[~valid] = 0
    return q, valid


def iou(w, h, cw, ch):
    """i / (w * h + cw * ch - i), arrays or scalars, every operation rounded on its own"""
    i = np.minimum(w, cw) * np.minimum(h, ch)
    s = w * h + cw * ch
    return i / (s - i)


def dist(distance, w, h, cw, ch):
    if distance == IOU:
        return 1.0 - iou(w, h, cw, ch)
    dw, dh = w - cw, h - ch
    return dw * dw + dh * dh


def fixed40(d):
    """floor(d * 2^40) as int64 (d >= 0, at most 2)"""
    return np.floor(np.asarray(d, dtype=np.float64) * TWO40).astype(np.int64)


def draw(seed, restart, rnd):
    """u of (restart, round): the first two words of Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32) and the counter (restart, round, 0, 0)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    o = philox4x32_10(restart, rnd, 0, 0, seed & 0xFFFFFFFF, seed >> 32)
    return (int(o[0]) << 32) | int(o[1])


def threshold(q, valid, tolerate):
    """tolerate * mean of the two population variances of the quantised data, from exact integer sums"""
    n = int(valid.sum())
    if n == 0:
        return 0.0
    var = []
    for c in range(2):
        col = [int(v) for v in q[valid, c]]
        N = n * sum(v * v for v in col) - sum(col) ** 2
        var.append(np.float64(float(N)) / (np.float64(n) * np.float64(n)) * np.float64(2.0 ** -80))     # float(int): correctly rounded
    return float(np.float64(tolerate) * ((var[0] + var[1]) / np.float64(2.0)))


def seeding(q, valid, k, distance, seed, restart):
    """-> (seed indices list (shorter than k when degenerate), degenerate)"""
    idx = np.flatnonzero(valid)
    w, h = q[:, 0].astype(np.float64) / TWO40, q[:, 1].astype(np.float64) / TWO40
    picks = []
    D = None
    for rnd in range(k):
        if rnd == 0:
            D = np.where(valid, 1, 0).astype(np.int64)
        else:
            s = picks[-1]
            d = np.where(valid, fixed40(dist(distance, w, h, w[s], h[s])), 0)
            D = d if rnd == 1 else np.minimum(D, d)
        T = sum(int(v) for v in D)
        if T == 0:
            return picks, True
        t = (draw(seed, restart, rnd) * T) >> 64
        run = 0
        pick = None
        for i in idx:
            run += int(D[i])
            if run > t:
                pick = int(i)
                break
        assert pick is not None
        picks.append(pick)
    return picks, False


def assign(q, valid, centres, distance):
    """labels int64 [n] (-1 where not valid) and the distances [n] to the label's centre: the first k with the smallest d"""
    w, h = q[:, 0].astype(np.float64) / TWO40, q[:, 1].astype(np.float64) / TWO40
    with np.errstate(invalid="ignore", divide="ignore"):
        best = dist(distance, w, h, centres[0][0], centres[0][1])
        labels = np.zeros(len(w), dtype=np.int64)
        for c in range(1, len(centres)):
            d = dist(distance, w, h, centres[c][0], centres[c][1])
            better = d < best
            best = np.where(better, d, best)
            labels[better] = c
    labels[~valid] = -1
    return labels, best


def cluster_sums(q, labels, k):
    """[(sum q_w, sum q_h, count)] as Python ints"""
    out = []
    for c in range(k):
        m = labels == c
        out.append((int(q[m, 0].sum()), int(q[m, 1].sum()), int(m.sum())))     # int64 is exact here: at most 2^22 values of at most 2^40
    return out


def lloyd(q, valid, centres, distance, thr, max_iter, trace=None):
    """One restart from `centres` -> dict(centres, labels, sums, n_iter, status, inertia_q, iou_q).  trace: a list that receives, per
    iteration, (labels, the centres they were assigned with)."""
    k = len(centres)
    centres = [[np.float64(c[0]), np.float64(c[1])] for c in centres]
    prev = np.full(len(q), -1, dtype=np.int64)
    status, n_iter, stop = 0, 0, None
    while True:
        labels, _ = assign(q, valid, centres, distance)
        if trace is not None:
            trace.append((labels.copy(), [list(c) for c in centres]))
        changed = int(((labels != prev) & valid).sum())
        prev = labels
        shift = np.float64(0.0)
        for c, (sw, sh, cnt) in enumerate(cluster_sums(q, labels, k)):
            if cnt == 0:
                status |= EMPTY_CLUSTER
                continue
            den = np.float64(cnt) * np.float64(TWO40)
            nw, nh = np.float64(float(sw)) / den, np.float64(float(sh)) / den
            dw, dh = nw - centres[c][0], nh - centres[c][1]
            shift = shift + (dw * dw + dh * dh)
            centres[c] = [nw, nh]
        n_iter += 1
        if n_iter >= 2 and changed == 0:
            stop = "labels"
        elif distance == EUCLIDEAN and shift <= thr:
            stop = "tolerance"
        elif n_iter >= max_iter:
            status |= MAX_ITER
            stop = "max_iter"
        if stop:
            break
    labels, best = assign(q, valid, centres, distance)
    sums = cluster_sums(q, labels, k)
    if any(s[2] == 0 for s in sums):
        status |= EMPTY_CLUSTER
    w, h = q[:, 0].astype(np.float64) / TWO40, q[:, 1].astype(np.float64) / TWO40
    with np.errstate(invalid="ignore", divide="ignore"):
        top = iou(w, h, centres[0][0], centres[0][1])
        for c in range(1, k):
            v = iou(w, h, centres[c][0], centres[c][1])
            top = np.where(v > top, v, top)
    inertia_q = int(fixed40(best[valid]).sum())
    iou_q = int(fixed40(top[valid]).sum())
    return dict(centres=centres, labels=labels, sums=sums, n_iter=n_iter, status=status, inertia_q=inertia_q, iou_q=iou_q, stop=stop)


def kmeans(wh, k, distance=EUCLIDEAN, tolerate=0.005, n_init=10, max_iter=300, seed=0, init=None):
    """The whole definition -> dict with the fields of the result block (header, restart table, best block) and labels"""
    q, valid = quantise(wh)
    n_valid = int(valid.sum())
    thr = threshold(q, valid, tolerate)
    if init is not None:
        assert n_init == 1
        init = np.asarray(init, dtype=np.float64).reshape(k, 2)
    rows, runs = [], []
    for r in range(n_init):
        if init is not None:
            with np.errstate(invalid="ignore"):
                bad = n_valid == 0 or not bool(((init > 0.0) & (init <= 1.0)).all())
            seeds, start = [], init
        else:
            seeds, bad = seeding(q, valid, k, distance, seed, r)
            start = [(np.float64(q[s, 0]) / TWO40, np.float64(q[s, 1]) / TWO40) for s in seeds]
        row_seeds = seeds + [-1] * (MAX_K - len(seeds))
        if bad:
            rows.append(dict(n_iter=0, status=DEGENERATE, inertia_q=0, iou_q=0, seeds=row_seeds, stop=None))
            runs.append(None)
            continue
        run = lloyd(q, valid, start, distance, thr, max_iter)
        rows.append(dict(n_iter=run["n_iter"], status=run["status"], inertia_q=run["inertia_q"], iou_q=run["iou_q"], seeds=row_seeds,
                         stop=run["stop"]))
        runs.append(run)
    best = -1
    for r, run in enumerate(runs):
        if run is not None and (best < 0 or run["inertia_q"] < runs[best]["inertia_q"]):
            best = r
    n_bad = len(q) - n_valid
    out = dict(restarts=rows, best_restart=best, n_valid=n_valid, n_bad=n_bad, k=k, n_init=n_init, distance=distance,
               status=(BAD_BOX if n_bad else 0) | (DEGENERATE if best < 0 else rows[best]["status"]),
               centres=np.zeros((MAX_K, 2)), counts=np.zeros(MAX_K, dtype=np.int64), sum_q=np.zeros((MAX_K, 2), dtype=np.uint64),
               inertia_q=0, iou_q=0, inertia=0.0, avg_iou=0.0, labels=np.full(len(q), -1, dtype=np.int32), q=q, valid=valid, threshold=thr)
    if best < 0:
        return out
    run = runs[best]
    order = sorted(range(k), key=lambda c: (float(run["centres"][c][0] * run["centres"][c][1]), float(run["centres"][c][0]), c))
    rank = np.full(k + 1, -1, dtype=np.int32)
    for j, c in enumerate(order):
        rank[c] = j
        out["centres"][j] = run["centres"][c]
        out["counts"][j] = run["sums"][c][2]
        out["sum_q"][j] = run["sums"][c][:2]
    out["labels"] = rank[run["labels"]].astype(np.int32)          # (-1 indexes the last entry: -1)
    out["inertia_q"], out["iou_q"] = run["inertia_q"], run["iou_q"]
    out["inertia"] = float(np.float64(float(run["inertia_q"])) * np.float64(2.0 ** -40))
    out["avg_iou"] = float(np.float64(float(run["iou_q"])) / (np.float64(n_valid) * np.float64(TWO40)))
    return out

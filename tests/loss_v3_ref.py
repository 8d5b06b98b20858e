"""The sequential yardstick of the YOLOv3 loss and its gradient (include/yolo_hip.h: yolo_v3_loss, yolo_v3_loss_grad): one truth, one row
and one term at a time, in NumPy scalars.  Two modes: "float32" is the definition as it is written (float32 terms, every operation rounded
on its own -- exp and log1p of the terms and of the gradient's sigmoid correctly rounded, through float64 --, float32 decode in the
ignore test, targets rounded once to float32); "float64" is the same mathematics with no float32
rounding after the inputs.  Assignment (float64 in the definition) is the same in both.  Sums are float64, rows ascending, in both.

A head is given as grids = [(h, w), ...] and anchors = [[(aw, ah), ...], ...] in the grid units of their scale."""
import numpy as np

OUT_OF_GRID, BAD_BOX, BAD_CLASS, BAD_COUNT = 1, 2, 4, 8
KEYS = ("xy", "wh", "obj", "noobj", "cls")


def rows_of(grids, anchors):
    """-> (R, [(row0, h, w, A)] per scale)"""
    out, row0 = [], 0
    for (h, w), anc in zip(grids, anchors):
        out.append((row0, int(h), int(w), len(anc)))
        row0 += int(h) * int(w) * len(anc)
    return row0, out


def locate(scales, r):
    """row -> (scale, cell row, cell column, anchor)"""
    s = 0
    while s + 1 < len(scales) and r >= scales[s + 1][0]:
        s += 1
    row0, h, w, na = scales[s]
    cell, a = divmod(r - row0, na)
    cr, cc = divmod(cell, w)
    return s, cr, cc, a


def iou64(x1, y1, w1, h1, x2, y2, w2, h2):
    """net/base.py:180-192 in float64 (the evaluation's IoU): union floored at 1e-8; NaN propagates through np.maximum / np.minimum"""
    f = np.float64
    x1, y1, w1, h1, x2, y2, w2, h2 = (np.asarray(v, dtype=f) for v in (x1, y1, w1, h1, x2, y2, w2, h2))
    with np.errstate(all="ignore"):
        ax1, ay1, ax2, ay2 = x1 - w1 / 2., y1 - h1 / 2., x1 + w1 / 2., y1 + h1 / 2.
        bx1, by1, bx2, by2 = x2 - w2 / 2., y2 - h2 / 2., x2 + w2 / 2., y2 + h2 / 2.
        iw = np.maximum(np.minimum(ax2, bx2) - np.maximum(ax1, bx1), 0.)
        ih = np.maximum(np.minimum(ay2, by2) - np.maximum(ay1, by1), 0.)
        inter = iw * ih
        uni = np.maximum(w1 * h1 + w2 * h2 - inter, 1e-8)
        return inter / uni


def truth_flags(t, n_classes):
    x, y, w, h, cls = np.float32(t[0]), np.float32(t[1]), np.float32(t[2]), np.float32(t[3]), int(t[4])
    bad = 0
    if not (x >= 0 and x < 1 and y >= 0 and y < 1):
        bad |= OUT_OF_GRID
    if not (w > 0) or not (h > 0):
        bad |= BAD_BOX
    if cls < 0 or cls >= n_classes:
        bad |= BAD_CLASS
    return bad


def assign(grids, anchors, n_classes, gt, counts):
    """-> (table int32 [B, R] of truth index | -1, status [B], n_truths [B], valid: per image the list of truth indices that take part)"""
    R, scales = rows_of(grids, anchors)
    B, max_gt = gt.shape
    table = np.full((B, R), -1, dtype=np.int32)
    status, n_truths, valid = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), []
    for b in range(B):
        ng = int(counts[b])
        if ng < 0 or ng > max_gt:
            status[b] |= BAD_COUNT
            ng = 0 if ng < 0 else max_gt
        ok = []
        for g in range(ng):
            t = gt[b, g]
            bad = truth_flags((t["x"], t["y"], t["w"], t["h"], t["class_idx"]), n_classes)
            status[b] |= bad
            if bad:
                continue
            x, y, w, h = (np.float64(t[k]) for k in ("x", "y", "w", "h"))
            best, bs, ba = -1., 0, 0
            for s, (row0, hs, ws, na) in enumerate(scales):
                for a in range(na):
                    aw, ah = anchors[s][a]
                    iou = float(iou64(0., 0., w * ws, h * hs, 0., 0., np.float64(aw), np.float64(ah)))
                    if best < iou:
                        best, bs, ba = iou, s, a
            row0, hs, ws, na = scales[bs]
            cx, cy = int(np.floor(x * ws)), int(np.floor(y * hs))
            table[b, row0 + (cy * ws + cx) * na + ba] = g           # in list order: the last truth of a slot owns it
            n_truths[b] += 1
            ok.append(g)
        valid.append(ok)
    return table, status, n_truths, valid


def _exp(t):
    """exp in t's dtype, CORRECTLY rounded: evaluated in float64 and rounded once (NumPy's own float32 exp is off by up to 2.5 ulp)"""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(t, dtype=np.float64)).astype(t.dtype)[()]


def _sp(t):
    with np.errstate(all="ignore"):
        e = _exp(-np.abs(t))
        return np.maximum(t, t.dtype.type(0)) + np.log1p(np.asarray(e, dtype=np.float64)).astype(t.dtype)[()]


def _sig(t):
    """the sigmoid of the gradient: 1 / (1 + exp(-t)) with the correctly rounded exp"""
    with np.errstate(all="ignore"):
        return t.dtype.type(1) / (t.dtype.type(1) + _exp(-t))


def _sig_decode(t):
    """the sigmoid of the decode (the ignore test): the library's exp in t's dtype"""
    with np.errstate(all="ignore"):
        return t.dtype.type(1) / (t.dtype.type(1) + np.exp(-t))


def targets(t, scale, cr, cc, anchor, dt):
    """(tx, ty, tw, th, m) of a winner row: float64, rounded once to dt"""
    _, hs, ws, _ = scale
    x, y, w, h = (np.float64(t[k]) for k in ("x", "y", "w", "h"))
    with np.errstate(all="ignore"):
        vals = (x * ws - cc, y * hs - cr, np.log(w * ws / np.float64(anchor[0])), np.log(h * hs / np.float64(anchor[1])), 2. - w * h)
    return tuple(dt(v) for v in vals)


def loss(logits, grids, anchors, n_classes, gt, counts, ignore_thresh=0.7, mode="float64"):
    """-> dict: table [B, R] (truth index | -1 | -2), status, n_truths, n_assigned [B], sums float64 [B, 5] in KEYS order, totals (the
    yolo_loss_result values), grad [B, R, 5 + C] of dtype `mode`, best_iou [B, R] (the ignore test's value, -1 where no truth; computed
    for EVERY row, winners too), margin = the smallest |iou - ignore_thresh| over every (row, valid truth) pair"""
    dt = {"float64": np.float64, "float32": np.float32}[mode]
    R, scales = rows_of(grids, anchors)
    B = logits.shape[0]
    width = 5 + n_classes
    logits = np.asarray(logits, dtype=np.float32).reshape(B, R, width)
    table, status, n_truths, valid = assign(grids, anchors, n_classes, gt, counts)
    sums = np.zeros((B, 5), dtype=np.float64)
    n_assigned = np.zeros(B, dtype=np.int32)
    grad = np.zeros((B, R, width), dtype=dt)
    best_iou = np.full((B, R), -1., dtype=np.float64)
    margin = np.inf
    Bd = dt(B)
    for b in range(B):
        ok = valid[b]
        tx_, ty_, tw_, th_ = (np.asarray([np.float64(gt[b, g][k]) for g in ok], dtype=np.float64) for k in ("x", "y", "w", "h"))
        for r in range(R):
            s, cr, cc, a = locate(scales, r)
            _, hs, ws, _ = scales[s]
            t = logits[b, r].astype(dt)
            with np.errstate(all="ignore"):
                # the ignore test's value (the device forms it on rows that are not winners; here on every row, for the margins)
                bx = (_sig_decode(t[0]) + dt(cc)) / dt(ws)
                by = (_sig_decode(t[1]) + dt(cr)) / dt(hs)
                bw = np.exp(t[2]) * dt(anchors[s][a][0]) / dt(ws)
                bh = np.exp(t[3]) * dt(anchors[s][a][1]) / dt(hs)
                if ok:
                    ious = iou64(bx, by, bw, bh, tx_, ty_, tw_, th_)
                    good = ious[~np.isnan(ious)]
                    if good.size:
                        best_iou[b, r] = max(-1., float(good.max()))
                        margin = min(margin, float(np.min(np.abs(good - ignore_thresh))))
                g = int(table[b, r])
                if g >= 0:
                    tx, ty, tw, th, m = targets(gt[b, g], scales[s], cr, cc, anchors[s][a], dt)
                    xy = m * (_sp(t[0]) - tx * t[0] + _sp(t[1]) - ty * t[1])
                    d2, d3 = t[2] - tw, t[3] - th
                    wh = m * dt(0.5) * (d2 * d2 + d3 * d3)
                    obj = _sp(t[4]) - t[4]
                    cls = int(gt[b, g]["class_idx"])
                    c = np.float64(0)
                    for k in range(n_classes):
                        v = t[5 + k]
                        c += np.float64(_sp(v) - v if k == cls else _sp(v))
                    sums[b, 0] += np.float64(xy); sums[b, 1] += np.float64(wh); sums[b, 2] += np.float64(obj); sums[b, 4] += c
                    n_assigned[b] += 1
                    grad[b, r, 0] = m * (_sig(t[0]) - tx) / Bd
                    grad[b, r, 1] = m * (_sig(t[1]) - ty) / Bd
                    grad[b, r, 2] = m * d2 / Bd
                    grad[b, r, 3] = m * d3 / Bd
                    grad[b, r, 4] = (_sig(t[4]) - dt(1)) / Bd
                    onehot = np.zeros(n_classes, dtype=dt)
                    onehot[cls] = 1
                    grad[b, r, 5:] = (_sig(t[5:]) - onehot) / Bd
                elif best_iou[b, r] > ignore_thresh:
                    table[b, r] = -2
                else:
                    sums[b, 3] += np.float64(_sp(t[4]))
                    grad[b, r, 4] = _sig(t[4]) / Bd
    totals = {"loss_" + ("class" if k == "cls" else k): _ordered(sums[:, i]) / B for i, k in enumerate(KEYS)}
    totals["loss"] = totals["loss_xy"] + totals["loss_wh"] + totals["loss_obj"] + totals["loss_noobj"] + totals["loss_class"]
    return {"table": table, "status": status, "n_truths": n_truths, "n_assigned": n_assigned, "sums": sums, "totals": totals, "grad": grad,
            "best_iou": best_iou, "margin": margin}


def _ordered(v):
    s = 0.0
    for x in v:         # in image order
        s += float(x)
    return s

"""The yardstick of the YOLOv2 loss-gradient tests: a sequential NumPy restatement of the gradient defined in include/yolo_hip.h
(yolo_v2_loss_grad), G = d loss / d logits with `loss` as loss_ref.loss computes it.

`grad` takes what the device entry takes: float32 logits [B, h, w, A, 5 + C], anchors in grid units, yolo_gt records with int32 counts.
The winner table is loss_ref.assign's.  Every element of G is written, slot by slot:

  not a winner   G[0..3] = +0 (the terms of a masked-out slot are never formed);  G[4] = (1/B) * 2 po * po (1 - po)
  class rows     every anchor slot of a cell WITH a winner: softmax(t[5:]) - onehot(label), label = the winner's class on the winner slot,
                 0 on the others; not divided by B.  A cell without a winner: +0
  winner         k = (5/B) * 2 (iou - po);  dL/dpx = (1/B) * 2 (px - gx) + k * dI/dpx;  dL/dpw = (1/B) * (sqrt pw - sqrt gw) / sqrt pw + k * dI/dpw
                 G[0] = dL/dpx * sx (1 - sx), G[2] = dL/dpw * pw, G[4] = -k * po (1 - po); y / h alike
  IoU partials   rw = min(px2, gx2) - max(px1, gx1), iw = max(rw, 0), TensorFlow's tie rules as 0/1 brackets:
                 diw/dpx = [rw >= 0] ([px2 <= gx2] - [px1 >= gx1]),  diw/dpw = [rw >= 0] ([px2 <= gx2] + [px1 >= gx1]) / 2
                 dI/dv = (dinter/dv * (uni + inter) - inter * d(pw ph)/dv) / uni^2

mode "float32": every elementwise operation in float32; mode "float64": everything in float64 from the float32 logits, the
float32-rounded anchors and the float32-rounded truths (as loss_ref.loss).  Returns an array of the mode's dtype, [B, h, w, A, 5 + C].
"""
import numpy as np

import loss_ref


def _iou_and_partials(gx, gy, gw, gh, px, py, pw, ph, T):
    """-> (iou, dI/dpx, dI/dpy, dI/dpw, dI/dph) in dtype T"""
    two, zero = T(2), T(0)
    gx1, gy1, gx2, gy2 = gx - gw / two, gy - gh / two, gx + gw / two, gy + gh / two
    px1, py1, px2, py2 = px - pw / two, py - ph / two, px + pw / two, py + ph / two
    rw = np.minimum(px2, gx2) - np.maximum(px1, gx1)
    rh = np.minimum(py2, gy2) - np.maximum(py1, gy1)
    iw, ih = np.maximum(rw, zero), np.maximum(rh, zero)
    inter = iw * ih
    uni = pw * ph + gw * gh - inter
    iou = inter / uni
    hi_x, lo_x, hi_y, lo_y = T(px2 <= gx2), T(px1 >= gx1), T(py2 <= gy2), T(py1 >= gy1)
    on_w, on_h = T(rw >= zero), T(rh >= zero)
    diw_dpx, diw_dpw = on_w * (hi_x - lo_x), on_w * (hi_x + lo_x) / two
    dih_dpy, dih_dph = on_h * (hi_y - lo_y), on_h * (hi_y + lo_y) / two
    both, uni2 = uni + inter, uni * uni
    di_dpx = ih * diw_dpx * both / uni2
    di_dpy = iw * dih_dpy * both / uni2
    di_dpw = (ih * diw_dpw * both - inter * ph) / uni2
    di_dph = (iw * dih_dph * both - inter * pw) / uni2
    return iou, di_dpx, di_dpy, di_dpw, di_dph


def _winner(tt, c, r, aw, ah, gx, gy, gw, gh, po, lam, lam_obj, T):
    """the five box elements of a winner slot"""
    one, two = T(1), T(2)
    sx, sy = loss_ref._sigmoid(tt[0], T), loss_ref._sigmoid(tt[1], T)
    px, py = sx + T(c), sy + T(r)
    pw, ph = np.exp(tt[2]) * aw, np.exp(tt[3]) * ah
    iou, di_dpx, di_dpy, di_dpw, di_dph = _iou_and_partials(gx, gy, gw, gh, px, py, pw, ph, T)
    k = lam_obj * (two * (iou - po))
    dl_dpx = lam * (two * (px - gx)) + k * di_dpx
    dl_dpy = lam * (two * (py - gy)) + k * di_dpy
    rpw, rph = np.sqrt(pw), np.sqrt(ph)
    dl_dpw = lam * ((rpw - np.sqrt(gw)) / rpw) + k * di_dpw
    dl_dph = lam * ((rph - np.sqrt(gh)) / rph) + k * di_dph
    return (dl_dpx * (sx * (one - sx)), dl_dpy * (sy * (one - sy)), dl_dpw * pw, dl_dph * ph, -k * (po * (one - po)))


def _class_row(t, label, T):
    m = np.max(t)
    e = np.exp(t - m)
    p = e / np.sum(e, dtype=T)
    p[label] = p[label] - T(1)
    return p


def grad(logits, h, w, anchors, n_classes, gt, counts, mode="float64"):
    T = {"float32": np.float32, "float64": np.float64}[mode]
    anchors = np.reshape(np.asarray(anchors, dtype=np.float64), [-1, 2])
    A = len(anchors)
    anc = anchors.astype(np.float32).astype(T)
    logits = np.asarray(logits, dtype=np.float32).reshape(-1, h, w, A, 5 + n_classes)
    B = logits.shape[0]
    table, _, _ = loss_ref.assign(h, w, anchors, n_classes, gt, counts)
    one, two = T(1), T(2)
    lam, lam_obj = one / T(B), T(5) / T(B)
    G = np.zeros(logits.shape, dtype=T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for b in range(B):
            t = logits[b].astype(T)
            po = loss_ref._sigmoid(t[..., 4], T)
            G[b, ..., 4] = (lam * two * po) * (po * (one - po))
            for r in range(h):
                for c in range(w):
                    win = int(table[b, r, c])
                    if win < 0:
                        continue
                    g, a = gt[b, win >> 3], win & 7
                    gx, gy = T(np.float32(np.float64(g["x"]) * w)), T(np.float32(np.float64(g["y"]) * h))
                    gw, gh = T(np.float32(np.float64(g["w"]) * w)), T(np.float32(np.float64(g["h"]) * h))
                    G[b, r, c, a, :5] = _winner(t[r, c, a], c, r, anc[a, 0], anc[a, 1], gx, gy, gw, gh, po[r, c, a], lam, lam_obj, T)
                    for k in range(A):
                        G[b, r, c, k, 5:] = _class_row(t[r, c, k, 5:], int(g["class_idx"]) if k == a else 0, T)
    return G

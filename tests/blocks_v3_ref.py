"""The yardstick of the tests of the sparse data gradient of a YOLOv3 head conv: sequential NumPy restatements of the definition in
include/yolo_hip.h ("The sparse data gradient of one YOLOv3 head conv", "Training the 3 x 3 blocks behind the YOLOv3 heads").  The term
mask, the gather of one scale and the tables come from tests/train_v3_ref.py; the taps, the fold, the packed form of a block and the Adam
restatement from tests/tail_ref.py; the loss and its gradient from tests/loss_v3_ref.py.

head_dgrad        D_s[p][c] = (S_o G_s[p][o] W_s[o][c]) * (Y_s[p][c] > 0 ? 1 : slope): one chain per element from +0, o ascending over the terms
                  the table does not declare a structural zero; a structural zero is never looked at, whatever G holds there.  mode "float32"
                  restates the device's fmaf chain (the product exact in float64, the sum rounded to float32 -- for the integer operands
                  of the exact tests nothing is rounded before the factor, which is ONE float32 multiply), mode "float64" does everything in
                  float64
head_dgrad_ref64  the float64 result with the bound (T + 2) 2^-24 |factor| S |G| |W| per element, T the terms of the position
gathered          G_s [P_s, cout_s] with its structural zeros set to +0: the operand of the dense route (yolo_conv1x1_dgrad)
blocks_train_loop the whole step, `steps` times on fixed block inputs: forward of every block and head conv, the YOLOv3 loss and its gradient,
                  the heads' weight gradient over the terms, head_dgrad, the 3 x 3 weight gradient with the fold's float32 scale, Adam on
                  the four arrays of every scale, the re-pack with the batch norm folded in float64 -- in float64 or float32
"""
import numpy as np

import loss_v3_ref
import tail_ref
import train_v3_ref

SLOPE = 0.1


def _f(mode):
    assert mode in ("float32", "float64")
    return np.float32 if mode == "float32" else np.float64


def gathered(G, table, scale, max_gt):
    """-> (G_s float [P_s, cout_s] with +0 in its structural zeros, mask_s bool alike); scale = (row0, h, w, A)"""
    G = np.asarray(G)
    mask = train_v3_ref.terms(table, G.shape[2], max_gt)
    Gs, Ms = train_v3_ref.scale_operands(G, mask, scale)
    return np.where(Ms, Gs, 0).astype(G.dtype), Ms


def factor_of(Y, slope, f):
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(Y) > 0, f(1), f(slope)).astype(f)      # +0, -0, negatives and NaN take the slope


def head_dgrad(G, table, W, scale, max_gt, Y=None, slope=SLOPE, mode="float32"):
    """G [B, R, 5 + C], table [B, R], W [cout_s, cin], scale = (row0, h, w, A), Y [P_s, cin] (the stored values) or None -> D [P_s, cin]"""
    f = _f(mode)
    Gs, Ms = gathered(G, table, scale, max_gt)
    Gs, W = Gs.astype(f), np.asarray(W, dtype=f)
    assert W.shape[0] == Gs.shape[1]
    acc = np.zeros((Gs.shape[0], W.shape[1]), dtype=f)
    for o in range(W.shape[0]):                 # o ascending; a position without the term keeps its sum untouched
        rows = np.nonzero(Ms[:, o])[0]
        if rows.size:
            # fmaf: the product of two float32 values is exact in float64
            acc[rows] = (Gs[rows, o:o + 1].astype(np.float64) * W[o:o + 1, :].astype(np.float64) + acc[rows].astype(np.float64)).astype(f)
    if Y is None:
        return acc
    out = acc * factor_of(Y, slope, f)
    assert out.dtype == f
    return out


def head_dgrad_ref64(G, table, W, scale, max_gt, Y=None, slope=SLOPE):
    """-> (D, bound) in float64; bound = (T + 2) 2^-24 |factor| S |G| |W| per element"""
    Gs, Ms = gathered(np.asarray(G, dtype=np.float64), table, scale, max_gt)
    W64 = np.asarray(W, dtype=np.float64)
    factor = np.ones((Gs.shape[0], W64.shape[1])) if Y is None else factor_of(Y, np.float32(slope), np.float64)
    T = Ms.sum(axis=1).astype(np.float64)
    return (Gs @ W64) * factor, ((T + 2) * 2.0 ** -24)[:, None] * np.abs(factor) * (np.abs(Gs) @ np.abs(W64))


def blocks_train_loop(X3s, blocks, Ws, bs, grids, anchors, n_classes, gt, counts, lr, steps, storage, mode="float64", ignore_thresh=0.7,
                      slope=SLOPE):
    """`steps` Adam steps of the head convs and the 3 x 3 blocks behind them on the fixed block inputs X3s[s] [B, h_s, w_s, cin3_s] (the
    stored values) -> (losses before each update, [W3_s [cout3, 9, cin3]], [beta_s], [W_s], [b_s]).  blocks[s] = (beta, gamma, mean, var,
    W3 [cout3, 9, cin3]); anchors[s] = [(w, h)] in grid units.  The arithmetic runs in the mode's dtype; what is PART OF THE FUNCTION
    is restated in either mode, as in tail_ref.tail_train_loop: the packed weights of both convs and the stored Y are rounded to `storage`
    (np.float16 | np.float32) and b' to float32, the fold's scale is float64 and its float32 rounding multiplies dW3, the logits pass
    through float32 into the loss yardstick, and the masters are float32 on the device (float32 mode) or the ideal float64 ones."""
    f = _f(mode)
    R, scales = loss_v3_ref.rows_of(grids, anchors)
    ns, width, max_gt = len(scales), 5 + n_classes, np.asarray(gt).shape[1]
    B = np.asarray(X3s[0]).shape[0]
    Tms, folds, par, mom = [], [], [], []
    for s in range(ns):
        beta0, gamma, mean, var, W3_0 = blocks[s]
        scale64, _ = tail_ref.fold(beta0, gamma, mean, var)
        folds.append((scale64, scale64.astype(np.float32), np.asarray(mean)))
        T = tail_ref.taps(np.asarray(X3s[s], dtype=f))
        Tms.append(T.reshape(T.shape[0], -1))
        par.append([np.array(a, dtype=f) for a in (W3_0, beta0, Ws[s], bs[s])])
        mom.append([[np.zeros_like(a), np.zeros_like(a)] for a in par[s]])
    losses = []
    for t in range(1, steps + 1):
        Ys, parts = [], []
        for s in range(ns):
            W3, beta, Wh, bh = par[s]
            scale64, _, mean = folds[s]
            pack, bp = tail_ref.pack_block(W3, beta, mean, scale64, storage)
            z = Tms[s] @ pack.reshape(pack.shape[0], -1).astype(f).T + bp.astype(f)
            Y = np.where(z > 0, z, f(slope) * z).astype(storage)            # the stored activation
            Ys.append(Y)
            L = (Y.astype(f) @ Wh.astype(storage).astype(f).T + bh.astype(np.float32).astype(f)).astype(np.float32)
            parts.append(L.reshape(B, -1, width))
        logits = np.concatenate(parts, axis=1)
        r = loss_v3_ref.loss(logits, grids, anchors, n_classes, gt, counts, ignore_thresh, mode=mode)
        losses.append(float(r["totals"]["loss"]))
        G, table = np.asarray(r["grad"]).astype(f), r["table"]
        lr_t = f(np.float32(float(lr) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)))
        for s in range(ns):
            W3, beta, Wh, bh = par[s]
            Gs, _ = gathered(G, table, scales[s], max_gt)
            Yf = Ys[s].astype(f)
            D = head_dgrad(G, table, Wh, scales[s], max_gt, Ys[s], slope, mode=mode)
            grads = [folds[s][1].astype(f)[:, None, None] * (D.T @ Tms[s]).reshape(W3.shape), D.sum(axis=0), Gs.T @ Yf, Gs.sum(axis=0)]
            for i in range(4):
                par[s][i], mom[s][i][0], mom[s][i][1] = tail_ref.adam(par[s][i], mom[s][i][0], mom[s][i][1], grads[i], lr_t)
                assert par[s][i].dtype == f
    return (losses, [p[0] for p in par], [p[1] for p in par], [p[2] for p in par], [p[3] for p in par])

"""The yardstick of the tail-training tests: sequential NumPy restatements of the definitions in include/yolo_hip.h ("The data gradient of
the detection layer and the weight gradient of a 3 x 3 conv").

The block is  u = conv3x3_same(W3, X3);  z = s (.) u + b';  Y = leaky_0.1(z);  L = W Y + b.

dgrad                 D[p][c] = (S_o G[p][o] W[o][c]) * (Y[p][c] > 0 ? 1 : slope): o ascending; mode "float32" rounds every product and
                      every sum to float32 (for the integer operands of the exact tests nothing is rounded before the slope multiply, which
                      is ONE float32 multiply), mode "float64" does everything in float64
taps                  X3 [B, h, w, cin] -> [P, 9, cin]: tap t = 3 ky + kx of position (n, r, x) is X3[n, r + ky - 1, x + kx - 1], zeros outside
wgrad3x3              R[o][t][c] = S_p D[p][o] taps[p][t][c], db[o] = S_p D[p][o], dW3 = s R: p ascending in both modes
wgrad3x3_exact        the same in int64 for integer operands
wgrad3x3_bound        (P + 3) 2^-24 |s| S_p |D| |X3| per element (|X3| = 1, |s| = 1 for db)
stream_to_otc / otc_to_stream   the Darknet stream's kernel [out][in][kh][kw] <-> [o][t][c]
tail_forward          the block and the head from their parameters (float64)
tail_grads64          every gradient of a scalar loss given G = dloss / dL, in float64 (checked against torch.autograd: test_train_tail_cpu.py)
"""
import numpy as np

SLOPE = 0.1
BN_EPS = 1e-5


def _f(mode):
    assert mode in ("float32", "float64")
    return np.float32 if mode == "float32" else np.float64


def dgrad(G, W, Y=None, slope=SLOPE, mode="float32"):
    """G [P, cout], W [cout, cin], Y [P, cin] (any float dtype: the stored values) or None -> D [P, cin] in the mode's dtype"""
    f = _f(mode)
    G, W = np.asarray(G, dtype=f), np.asarray(W, dtype=f)
    acc = np.zeros((G.shape[0], W.shape[1]), dtype=f)
    for o in range(W.shape[0]):                         # o ascending, every product and every sum rounded to the mode's dtype
        acc = acc + G[:, o:o + 1] * W[o:o + 1, :]
    assert acc.dtype == f
    if Y is None:
        return acc
    with np.errstate(invalid="ignore"):
        factor = np.where(np.asarray(Y) > 0, f(1), f(slope)).astype(f)       # +0, -0, negatives and NaN take the slope
    out = acc * factor
    assert out.dtype == f
    return out


def taps(X3):
    """X3 [B, h, w, cin] -> [B * h * w, 9, cin]; taps outside the image are zeros"""
    X3 = np.asarray(X3)
    B, h, w, cin = X3.shape
    pad = np.zeros((B, h + 2, w + 2, cin), dtype=X3.dtype)
    pad[:, 1:h + 1, 1:w + 1] = X3
    out = np.empty((B, h, w, 9, cin), dtype=X3.dtype)
    for ky in range(3):
        for kx in range(3):
            out[:, :, :, 3 * ky + kx] = pad[:, ky:ky + h, kx:kx + w]
    return out.reshape(B * h * w, 9, cin)


def wgrad3x3(X3, D, scale=None, mode="float32"):
    """X3 [B, h, w, cin], D [P, cout], scale [cout] or None -> (dW3 [cout, 9, cin], db [cout]) in the mode's dtype, p ascending"""
    f = _f(mode)
    T = taps(np.asarray(X3, dtype=f))
    D = np.asarray(D, dtype=f)
    R = np.zeros((D.shape[1],) + T.shape[1:], dtype=f)
    db = np.zeros(D.shape[1], dtype=f)
    for p in range(D.shape[0]):
        R = R + D[p][:, None, None] * T[p][None]
        db = db + D[p]
    if scale is not None:
        R = np.asarray(scale, dtype=f)[:, None, None] * R
    assert R.dtype == f and db.dtype == f
    return R, db


def wgrad3x3_exact(X3, D, scale=None):
    """integer operands (and an integer or power-of-two scale) -> (dW3 float64 [cout, 9, cin], db int64 [cout]), exact"""
    Xi, Di = np.asarray(X3).astype(np.int64), np.asarray(D).astype(np.int64)
    assert np.array_equal(Xi, X3) and np.array_equal(Di, D), "the exact reference takes integers"
    T = taps(Xi).astype(np.float64)
    # float64 products and sums of integers: exact while every sum of magnitudes stays below 2^53; below 2^24 float32 holds them too
    assert (np.abs(Di).astype(np.float64).T @ np.abs(T).reshape(T.shape[0], -1)).max(initial=0) < 2 ** 24
    R = (Di.astype(np.float64).T @ T.reshape(T.shape[0], -1)).reshape((Di.shape[1],) + T.shape[1:])
    if scale is not None:
        R = np.asarray(scale, dtype=np.float64)[:, None, None] * R
    return R, Di.sum(axis=0)


def wgrad3x3_ref64(X3, D, scale=None):
    """-> (dW3, db, bound_dW3, bound_db) in float64; bound = (P + 3) 2^-24 |s| S_p |D| |X3| per element"""
    X64, D64 = np.asarray(X3, dtype=np.float64), np.asarray(D, dtype=np.float64)
    T = taps(X64)
    P = D64.shape[0]
    s = np.ones(D64.shape[1]) if scale is None else np.asarray(scale, dtype=np.float64)
    k = (P + 3) * 2.0 ** -24
    R = np.einsum("po,ptc->otc", D64, T, optimize=True)
    A = np.einsum("po,ptc->otc", np.abs(D64), np.abs(T), optimize=True)
    return s[:, None, None] * R, D64.sum(axis=0), k * np.abs(s)[:, None, None] * A, k * np.abs(D64).sum(axis=0)


def stream_to_otc(kernel, cout, cin):
    """the Darknet stream's kernel, [out][in][kh][kw] flat -> [o][t = 3 ky + kx][c]"""
    return np.ascontiguousarray(np.asarray(kernel).reshape(cout, cin, 9).transpose(0, 2, 1))


def otc_to_stream(otc):
    """[o][t][c] -> the Darknet stream's [out][in][kh][kw], flat"""
    return np.ascontiguousarray(np.asarray(otc).transpose(0, 2, 1)).reshape(-1)


def fold(beta, gamma, mean, var):
    """weights.cpp: fold_batch_norm -> (scale64 [cout] float64, b' float32 [cout])"""
    scale = np.asarray(gamma, dtype=np.float64) / np.sqrt(np.asarray(var, dtype=np.float64) + BN_EPS)
    return scale, (np.asarray(beta, dtype=np.float64) - np.asarray(mean, dtype=np.float64) * scale).astype(np.float32)


def tail_forward(X3, W3, scale, bias, W, b, slope=SLOPE):
    """float64: X3 [B, h, w, cin], W3 [cout3, 9, cin], scale / bias [cout3], W [cout, cout3], b [cout] -> (z, Y, L), each [P, .]"""
    T = taps(np.asarray(X3, dtype=np.float64))
    u = np.einsum("ptc,otc->po", T, np.asarray(W3, dtype=np.float64), optimize=True)
    z = u * np.asarray(scale, dtype=np.float64) + np.asarray(bias, dtype=np.float64)
    Y = np.where(z > 0, z, slope * z)
    return z, Y, Y @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)


def pack_block(W3, beta, mean, scale64, storage):
    """the block's packed form from its master values, as the weight loader and the step write it: pack = T((double)W3 * scale64[o]),
    ONE rounding from the float64 product, b' = (float)((double)beta - (double)mean * scale64) -> (pack [cout3, 9, cin3] of dtype
    `storage`, b' float32)"""
    W64, s64 = np.asarray(W3, dtype=np.float64), np.asarray(scale64, dtype=np.float64)
    pack = (W64 * s64[:, None, None]).astype(storage)
    return pack, (np.asarray(beta, dtype=np.float64) - np.asarray(mean, dtype=np.float64) * s64).astype(np.float32)


def adam(w, m, v, g, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    """one Adam step in the dtype of w (every array operation rounded once): -> (w, m, v)"""
    f = w.dtype.type
    g = np.asarray(g, dtype=f)
    m = f(beta1) * m + (f(1) - f(beta1)) * g
    v = f(beta2) * v + (f(1) - f(beta2)) * (g * g)
    return w - (f(lr_t) * m) / (np.sqrt(v) + f(eps)), m, v


def tail_train_loop(X3, block, W, b, h, w, anchors, n_classes, gt, counts, lr, steps, storage, mode="float64", slope=SLOPE):
    """`steps` Adam steps of the tail on the fixed block input X3 [B, h, w, cin3] (the device's stored values) -> (losses before each
    update, W3 [cout3, 9, cin3], beta, W, b).  block = (beta, gamma, mean, var, W3 [cout3, 9, cin3]).  The arithmetic runs in the mode's
    dtype; what is PART OF THE FUNCTION is restated in either mode: the packed weights of both layers and the stored Y are rounded to
    `storage` (np.float16 | np.float32) and b' to float32, the fold's scale is float64 and its float32 rounding multiplies dW3, the
    logits pass through float32 into the loss yardsticks, and the master values are float32 on the device (float32 mode) or the ideal
    float64 ones (float64 mode)."""
    import loss_grad_ref
    import loss_ref
    f = _f(mode)
    beta0, gamma, mean, var, W3_0 = block
    scale64, _ = fold(beta0, gamma, mean, var)
    scale32 = scale64.astype(np.float32)
    T = taps(np.asarray(X3, dtype=f))                      # [P, 9, cin3]
    P = T.shape[0]
    Tm = T.reshape(P, -1)
    B = P // (h * w)
    par = [np.array(a, dtype=f) for a in (W3_0, beta0, W, b)]
    mom = [[np.zeros_like(a), np.zeros_like(a)] for a in par]
    losses = []
    for t in range(1, steps + 1):
        W3, beta, Wh, bh = par
        pack, bp = pack_block(W3, beta, mean, scale64, storage)
        z = Tm @ pack.reshape(pack.shape[0], -1).astype(f).T + bp.astype(f)
        Y = np.where(z > 0, z, f(slope) * z).astype(storage)                # the stored activation
        Yf = Y.astype(f)
        logits = (Yf @ Wh.astype(storage).astype(f).T + bh.astype(np.float32).astype(f)).astype(np.float32).reshape(B, h, w, -1)
        losses.append(float(loss_ref.loss(logits, h, w, anchors, n_classes, gt, counts, mode=mode)["loss"]))
        G = np.asarray(loss_grad_ref.grad(logits, h, w, anchors, n_classes, gt, counts, mode=mode)).reshape(P, -1).astype(f)
        D = (G @ Wh) * np.where(Y > 0, f(1), f(slope))
        grads = [scale32.astype(f)[:, None, None] * (D.T @ Tm).reshape(W3.shape), D.sum(axis=0), G.T @ Yf, G.sum(axis=0)]
        lr_t = f(np.float32(float(lr) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)))
        for i in range(4):
            par[i], mom[i][0], mom[i][1] = adam(par[i], mom[i][0], mom[i][1], grads[i], lr_t)
            assert par[i].dtype == f
    return losses, par[0], par[1], par[2], par[3]


def tail_grads64(X3, Y, W, scale, G, slope=SLOPE):
    """float64, from G = dloss / dL [P, cout] and the stored Y -> dict of dW [cout, cout3], db, D [P, cout3], dW3 [cout3, 9, cin], dbeta"""
    G64, Y64 = np.asarray(G, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    D = dgrad(G64, W, Y64, slope, mode="float64")
    dW3, dbeta, _, _ = wgrad3x3_ref64(X3, D, scale)
    return {"dW": G64.T @ Y64, "db": G64.sum(axis=0), "D": D, "dW3": dW3, "dbeta": dbeta}

"""The yardstick of the head-training tests: NumPy restatements of the definitions in include/yolo_hip.h ("Training the detection layer").

wgrad_exact / wgrad_ref64   dW[o][c] = S_p G[p][o] X[p][c], db[o] = S_p G[p][o]: in int64 for the integer operands of the exact tests
                            (any summation order gives these values while every partial sum stays below 2^24), and in float64 with the
                            derived float32 bound (P + 2) 2^-24 S_p |G[p][o]| |X[p][c]|
adam_ref32                  the update in float32, every operation rounded on its own (NumPy rounds each array operation once: there is
                            no fused multiply-add to contract into), what yolo_adam_step must equal bit for bit
adam_ref64                  the same in float64, checked against torch.optim.Adam (tests/test_train_cpu.py)
head_train_loop64           forward of the detection layer, loss, gradient (tests/loss_ref.py, tests/loss_grad_ref.py), weight gradient
                            and Adam in float64 on a fixed batch of features
"""
import numpy as np

import loss_grad_ref
import loss_ref


COUTS = (6, 30, 125, 130)         # below one MFMA tile; not a multiple of any tile; one past 128
CINS = (8, 40, 136, 1024)
VIEWS = ((0, 0), (8, 8))          # (ld - cin, coff): dense, and a slice of a wider pixel


def wgrad_position_cases(plan):
    """The position counts of the exact tests, sized from yolo_wgrad_plan (`plan`: P -> its dict) and not hard-coded, as
    (batch, positions_per_image, image stride beyond positions_per_image * ld, chunks the case must run as): one position; one short of
    a chunk; exactly one chunk; one past it; three chunks, the last ragged; 3 images of 13 x 13 with a gap between the images."""
    c = plan(1)["positions_per_chunk"]
    return ((1, 1, 0, 1), (1, c - 1, 0, 1), (1, c, 0, 1), (1, c + 1, 0, 2), (1, 2 * c + 5, 0, 3), (3, 169, 24, -(-3 * 169 // plan(3 * 169)["positions_per_chunk"])))


def view_positions(x_view, batch, ppi, ld, coff, image_stride, cin):
    """the [P, cin] operand a strided view holds: element (n, q, c) at n * image_stride + q * ld + coff + c of the flat buffer"""
    idx = (np.arange(batch)[:, None, None] * image_stride + np.arange(ppi)[None, :, None] * ld + coff + np.arange(cin)[None, None, :])
    return x_view[idx].reshape(batch * ppi, cin)


def wgrad_exact(X, G):
    """integer operands -> (dW int64 [cout, cin], db int64 [cout])"""
    Xi, Gi = np.asarray(X).astype(np.int64), np.asarray(G).astype(np.int64)
    assert np.array_equal(Xi, X) and np.array_equal(Gi, G), "the exact reference takes integers"
    return Gi.T @ Xi, Gi.sum(axis=0)


def wgrad_ref64(X, G):
    """-> (dW, db, bound_dW, bound_db) in float64; bound = (P + 2) 2^-24 S_p |G| |X| per element (|X| = 1 for db)"""
    X64, G64 = np.asarray(X, dtype=np.float64), np.asarray(G, dtype=np.float64)
    P = X64.shape[0]
    k = (P + 2) * 2.0 ** -24
    return G64.T @ X64, G64.sum(axis=0), k * (np.abs(G64).T @ np.abs(X64)), k * np.abs(G64).sum(axis=0)


def adam_lr_t(lr, t, beta1=0.9, beta2=0.999):
    """float64, rounded to float32 once"""
    return np.float32(float(lr) * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t))


def adam_ref32(w, m, v, g, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    """one step in float32 -> (w, m, v); m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) (g g); w = w - (lr_t m) / (sqrt(v) + eps)"""
    f = np.float32
    w, m, v, g = (np.asarray(a, dtype=f) for a in (w, m, v, g))
    b1, b2, lr_t, eps = f(beta1), f(beta2), f(lr_t), f(eps)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        m = b1 * m + (f(1) - b1) * g
        v = b2 * v + (f(1) - b2) * (g * g)
        w = w - (lr_t * m) / (np.sqrt(v) + eps)
    assert w.dtype == f and m.dtype == f and v.dtype == f
    return w, m, v


def adam_ref64(w, m, v, g, lr_t, beta1=0.9, beta2=0.999, eps=1e-8):
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    return w - (lr_t * m) / (np.sqrt(v) + eps), m, v


def head_train_loop64(X, W, b, h, w, anchors, n_classes, gt, counts, lr, steps):
    """`steps` Adam steps of the detection layer alone on the fixed features X [B * h * w, cin] (float64) -> (losses before each update,
    W, b).  The logits pass through float32 on their way into the loss yardsticks, as the device's do."""
    X = np.asarray(X, dtype=np.float64)
    W, b = np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)
    B = X.shape[0] // (h * w)
    mw, vw, mb, vb = np.zeros_like(W), np.zeros_like(W), np.zeros_like(b), np.zeros_like(b)
    losses = []
    for t in range(1, steps + 1):
        logits = (X @ W.T + b).reshape(B, h, w, -1)
        losses.append(loss_ref.loss(logits, h, w, anchors, n_classes, gt, counts, mode="float64")["loss"])
        G = loss_grad_ref.grad(logits, h, w, anchors, n_classes, gt, counts, mode="float64").reshape(B * h * w, -1).astype(np.float64)
        lr_t = float(lr) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        W, mw, vw = adam_ref64(W, mw, vw, G.T @ X, lr_t)
        b, mb, vb = adam_ref64(b, mb, vb, G.sum(axis=0), lr_t)
    return losses, W, b

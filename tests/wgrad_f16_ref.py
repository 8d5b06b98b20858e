"""The yardstick of the fp16-operand 3 x 3 weight gradient (include/yolo_hip.h: yolo_conv3x3_wgrad_f16): NumPy restatements of the
definition, and the case table of its tests (tests/test_wgrad_f16_cpu.py checks the table against the library's plan,
tests/test_gpu_wgrad_f16.py runs it).  Nothing here touches a device.

max_bits              the integer maximum of the bit patterns of |float32(D)|: the record's first word
scale_k               k from m: 0 for m = 0, Inf and NaN, else clamp(14 - floor(log2 m), -126, 126)
narrow                D16 = fp16_rne(D * 2^k): the scaling exact (float64), ONE conversion, gradual underflow
sums64                dW64 = s 2^-k S_p D16 X3 over the narrowed operands in float64, dWexact = s S_p D X3, db, and the header's two bounds
wgrad3x3_f16_exact    the integer reference: tests/tail_ref.py's, imported
tail_train_loop       tests/tail_ref.py's float64 / float32 training loop of the tail with the narrowing put in (narrow=False: that loop)
"""
import numpy as np

import tail_ref
from tail_ref import wgrad3x3_exact as wgrad3x3_f16_exact       # noqa: F401  (the integer reference is the float32 operator's)

FACTOR = 4          # the margin every device-versus-restatement comparison of this project gets


def max_bits(D):
    """the largest bit pattern of |float32(D)| as a Python int (NaN patterns sort above Inf)"""
    bits = np.ascontiguousarray(D, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return int(bits.max(initial=0))


def scale_k(m):
    """m: the maximum magnitude (any float; NaN stands for a NaN pattern) -> k"""
    m = float(m)
    if m == 0.0 or not np.isfinite(m):
        return 0
    mant, exp = np.frexp(abs(m))            # |m| = mant * 2^exp, mant in [0.5, 1): floor(log2 |m|) = exp - 1, subnormals included
    return int(min(126, max(-126, 14 - (int(exp) - 1))))


def k_of(D):
    """k of a call with the float32 gradient D"""
    return scale_k(np.array([max_bits(D)], dtype=np.uint32).view(np.float32)[0])


def narrow(D, k):
    """D16 [.] float16 = fp16_rne(D * 2^k): float64 holds the scaled value of a float32 (or of a float64 whose bits fit) exactly"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ldexp(np.asarray(D, dtype=np.float64), int(k)).astype(np.float16)


def sums64(X3, D, scale=None):
    """X3 [B, h, w, cin] (fp16 values), D [P, cout] float32, scale [cout] or None -> dict of float64 arrays:
    k; dW64 (narrowed operands), dWexact (un-narrowed), db; bound1 = (P + 4) 2^-24 |s| 2^-k S |D16| |X3|;
    bound2 = bound1 + |s| S (2^-11 |D| + 2^-25 2^-k) |X3|; bound_db = (P + 3) 2^-24 S |D|"""
    D32 = np.asarray(D, dtype=np.float32)
    k = k_of(D32)
    D16 = narrow(D32, k).astype(np.float64)
    D64 = D32.astype(np.float64)
    T = tail_ref.taps(np.asarray(X3, dtype=np.float64))
    P = D64.shape[0]
    s = np.ones(D64.shape[1]) if scale is None else np.asarray(scale, dtype=np.float64)
    sa = np.abs(s)[:, None, None]
    ein = lambda a, b: np.einsum("po,ptc->otc", a, b, optimize=True)
    bound1 = (P + 4) * 2.0 ** -24 * sa * 2.0 ** -k * ein(np.abs(D16), np.abs(T))
    return {"k": k, "dW64": s[:, None, None] * 2.0 ** -k * ein(D16, T), "dWexact": s[:, None, None] * ein(D64, T), "db": D64.sum(axis=0),
            "bound1": bound1, "bound2": bound1 + sa * ein(2.0 ** -11 * np.abs(D64) + 2.0 ** -25 * 2.0 ** -k, np.abs(T)),
            "bound_db": (P + 3) * 2.0 ** -24 * np.abs(D64).sum(axis=0)}


def tail_train_loop(X3, block, W, b, h, w, anchors, n_classes, gt, counts, lr, steps, storage, mode="float64", narrow_d=True, slope=tail_ref.SLOPE):
    """tail_ref.tail_train_loop with the block's weight gradient as yolo_conv3x3_wgrad_f16 defines it: dW3 = s32 (2^-k (D16^T taps)) with k
    and D16 from the step's D (through float32 in either mode: D is a float32 array on the device); dbeta from the un-narrowed D.
    narrow_d=False is tail_ref.tail_train_loop itself.  -> (losses before each update, W3, beta, W, b)"""
    import loss_grad_ref
    import loss_ref
    if not narrow_d:
        return tail_ref.tail_train_loop(X3, block, W, b, h, w, anchors, n_classes, gt, counts, lr, steps, storage, mode=mode, slope=slope)
    f = tail_ref._f(mode)
    beta0, gamma, mean, var, W3_0 = block
    scale64, _ = tail_ref.fold(beta0, gamma, mean, var)
    scale32 = scale64.astype(np.float32)
    T = tail_ref.taps(np.asarray(X3, dtype=f))
    P = T.shape[0]
    Tm = T.reshape(P, -1)
    B = P // (h * w)
    par = [np.array(a, dtype=f) for a in (W3_0, beta0, W, b)]
    mom = [[np.zeros_like(a), np.zeros_like(a)] for a in par]
    losses = []
    for t in range(1, steps + 1):
        W3, beta, Wh, bh = par
        pack, bp = tail_ref.pack_block(W3, beta, mean, scale64, storage)
        z = Tm @ pack.reshape(pack.shape[0], -1).astype(f).T + bp.astype(f)
        Y = np.where(z > 0, z, f(slope) * z).astype(storage)
        Yf = Y.astype(f)
        logits = (Yf @ Wh.astype(storage).astype(f).T + bh.astype(np.float32).astype(f)).astype(np.float32).reshape(B, h, w, -1)
        losses.append(float(loss_ref.loss(logits, h, w, anchors, n_classes, gt, counts, mode=mode)["loss"]))
        G = np.asarray(loss_grad_ref.grad(logits, h, w, anchors, n_classes, gt, counts, mode=mode)).reshape(P, -1).astype(f)
        D = (G @ Wh) * np.where(Y > 0, f(1), f(slope))
        D32 = D.astype(np.float32)
        k = k_of(D32)
        D16 = narrow(D32, k).astype(f)
        dW3 = scale32.astype(f)[:, None, None] * (f(2.0 ** -k) * (D16.T @ Tm).reshape(W3.shape))
        grads = [dW3, D.sum(axis=0), G.T @ Yf, G.sum(axis=0)]
        lr_t = f(np.float32(float(lr) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)))
        for i in range(4):
            par[i], mom[i][0], mom[i][1] = tail_ref.adam(par[i], mom[i][0], mom[i][1], grads[i], lr_t)
            assert par[i].dtype == f
    return losses, par[0], par[1], par[2], par[3]


def dist(a, b):
    """the largest relative distance between the per-step losses of two runs"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def narrowed_loops(args, lr):
    """The float64 loop of the tail with the narrowing and without it on one net and batch (args: tail_train_loop's up to `counts`, then
    steps and storage behind lr) -> (rate, losses narrowed, losses un-narrowed, d_narrow).  The rate starts at `lr` and is halved until both
    loops lower the loss at every step; d_narrow = dist(narrowed, un-narrowed) at that rate."""
    head, tail = args[:10], args[10:]
    falls = lambda v: all(a > c for a, c in zip(v, v[1:]))
    rate = float(lr)
    for _ in range(8):
        narrowed = tail_train_loop(*head, rate, *tail, mode="float64", narrow_d=True)[0]
        plain = tail_train_loop(*head, rate, *tail, mode="float64", narrow_d=False)[0]
        if falls(narrowed) and falls(plain):
            return rate, narrowed, plain, dist(narrowed, plain)
        rate /= 2
    raise AssertionError("no rate down to %g lowers the loss of both float64 loops at every step" % rate)


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
# (h, w, batch, cin, cout).  Maps 1 x 1, 1 x 5, 5 x 1, 3 x 5, 13 x 13; batch 1 - 3 (the images differ); position counts 1, 3, 10, 15, 30, 169,
# 338, 507: no multiple of the MFMA's k (8, 16, 32) or of the 64-position stage but 1 x 5 x ... none at all; cin 8 / 40 / 136 and 72 (one
# 8-channel group past a channel tile; 136: past a second one); cout 1 / 30 / 72 and 136 (past a second cout tile)
SHAPES = ((1, 1, 1, 8, 1), (1, 1, 3, 40, 30), (1, 5, 2, 8, 72), (5, 1, 3, 136, 1), (3, 5, 1, 40, 136), (3, 5, 2, 72, 30), (13, 13, 1, 8, 30),
          (13, 13, 2, 136, 72), (13, 13, 3, 40, 136))
# one case each 26 and 80 wide and one at the widest map of the plan, each with a chunk boundary inside a row (checked against the plan on the CPU)
WIDE_SHAPES = ((5, 26, 1, 8, 1), (2, 80, 1, 8, 30), (2, 96, 1, 16, 1))
MAX_W = 96
REAL_SHAPES = ((13, 13, 2, 136, 64), (3, 5, 1, 1280, 30))


def boundary_inside_a_row(plan, w):
    """does a chunk of `plan` end inside a row of a w-wide map?"""
    return plan["n_chunks"] >= 2 and plan["positions_per_chunk"] % w != 0


def plan_shapes(plan):
    """(h, w, batch, chunks) sized from yolo_conv3x3_wgrad_f16_plan (`plan`: (h, w, batch) -> its dict): one position short of a chunk, exactly
    one chunk, one past it, and two chunks and five positions; w the largest divisor of the count up to 13"""
    c = plan(1, 1, 1)["positions_per_chunk"]
    out = []
    for P, chunks in ((c - 1, 1), (c, 1), (c + 1, 2), (2 * c + 5, 3)):
        w = max(d for d in range(1, 14) if P % d == 0)
        out.append((P // w, w, 1, chunks))
    return out

"""The yardstick of the augmentation tests: a NumPy restatement of "Training augmentation on the device" in include/yolo_hip.h, written
from the definition and sharing no code with the library or with net/augment.py.  Whole-array integer arithmetic in int64; the generator
always runs (the library may skip a call whose result cannot matter: that shows here if it is wrong).  A record is anything with the
fields of yolo_augment_image as attributes."""
import numpy as np

GT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("w", "f4"), ("h", "f4"), ("class_idx", "i4"), ("difficult", "i4")])
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
S_SIGMA = np.sqrt((65536.0 ** 2 - 1.0) / 3.0)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds on arrays of counters (any shape; uint64 holds the 32-bit words) -> four arrays of 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in (c0, c1, c2, c3)]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def flip(S, flip_lr, flip_ud):
    F = S[::-1] if flip_ud else S
    return F[:, ::-1] if flip_lr else F


def blur(F, radius, taps):
    """separable, per channel, border reflect-101; Hs unrounded, B = (V + 32768) >> 16"""
    F = np.asarray(F).astype(np.int64)
    h, w = F.shape[:2]
    r = int(radius)
    t = [int(taps[k]) for k in range(r + 1)]
    assert r < h and r < w and t[0] + 2 * sum(t[1:]) == 256
    P = np.pad(F, ((0, 0), (r, r), (0, 0)), mode="reflect") if r else F
    Hs = sum(t[abs(k)] * P[:, r + k:r + k + w] for k in range(-r, r + 1))
    assert Hs.max() <= 65280
    P = np.pad(Hs, ((r, r), (0, 0), (0, 0)), mode="reflect") if r else Hs
    V = sum(t[abs(k)] * P[r + k:r + k + h] for k in range(-r, r + 1))
    return (V + 32768) >> 16


def halves(word):
    word = word.astype(np.int64)
    return (word & 0xFFFF) + (word >> 16)


def pixel_steps(h, w, p):
    """(dropped [h, w] bool, d0 [h, w] int64, d1 [h, w] int64) of the record's key, threshold and noise multipliers"""
    pos = (np.arange(h, dtype=np.uint64)[:, None] * np.uint64(w) + np.arange(w, dtype=np.uint64)[None, :])
    a = philox4x32_10(pos, 0, 0, 0, p.key[0], p.key[1])
    b = philox4x32_10(pos, 1, 0, 0, p.key[0], p.key[1])
    dropped = a[0] < np.uint64(int(p.drop_thr))
    s0 = halves(a[1]) + halves(a[2]) - 131070
    s1 = halves(b[0]) + halves(b[1]) - 131070
    d0 = (s0 * int(p.noise_q[0]) + (1 << 23)) >> 24
    d1 = (s1 * int(p.noise_q[1]) + (1 << 23)) >> 24
    return dropped, d0, d1


def augment_image(S, p):
    """S uint8 [h, w, 3] -> the augmented uint8 [h, w, 3]"""
    S = np.asarray(S)
    assert S.dtype == np.uint8 and S.ndim == 3 and S.shape[2] == 3
    if not p.enabled:
        return S.copy()
    h, w = S.shape[:2]
    B = blur(flip(S, p.flip_lr, p.flip_ud), p.radius, p.taps)
    dropped, d0, d1 = pixel_steps(h, w, p)
    T = np.where(dropped[:, :, None], 0, B)
    T = np.clip(T + int(p.noise_loc[0]) + d0[:, :, None], 0, 255)
    T = np.clip(T + int(p.noise_loc[1]) + d1[:, :, None], 0, 255)
    O = np.zeros_like(T)
    tx = int(p.tx)
    if abs(tx) < w:
        if tx >= 0:
            O[:, tx:] = T[:, :w - tx]
        else:
            O[:, :w + tx] = T[:, -tx:]
    return O.astype(np.uint8)


def augment_batch(X, params):
    return np.stack([augment_image(x, p) for x, p in zip(X, params)])


def augment_truths(gt, p, h, w):
    """gt: GT_DTYPE array [n] -> the GT_DTYPE array of the truths that are left; float64, every operation on its own"""
    gt = np.asarray(gt, dtype=GT_DTYPE)
    if not p.enabled:
        return gt.copy()
    x, y, bw, bh = (gt[k].astype(np.float64) for k in ("x", "y", "w", "h"))
    with np.errstate(invalid="ignore"):
        x1, x2 = x - bw / 2.0, x + bw / 2.0
        y1, y2 = y - bh / 2.0, y + bh / 2.0
        if p.flip_lr:
            x1, x2 = 1.0 - x2, 1.0 - x1
        if p.flip_ud:
            y1, y2 = 1.0 - y2, 1.0 - y1
        shift = np.float64(int(p.tx)) / np.float64(w)
        x1, x2 = x1 + shift, x2 + shift
        nan = np.isnan(x1) | np.isnan(x2) | np.isnan(y1) | np.isnan(y2)
        keep = ~(nan | (x2 <= 0) | (x1 >= 1) | (y2 <= 0) | (y1 >= 1))
    x1, x2, y1, y2 = (np.clip(v[keep], 0.0, 1.0) for v in (x1, x2, y1, y2))
    out = gt[keep].copy()
    out["x"], out["w"] = ((x1 + x2) / 2.0).astype(np.float32), (x2 - x1).astype(np.float32)
    out["y"], out["h"] = ((y1 + y2) / 2.0).astype(np.float32), (y2 - y1).astype(np.float32)
    return out

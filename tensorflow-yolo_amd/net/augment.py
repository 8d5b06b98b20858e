"""Training augmentation: the parameters of the reference's imgaug pipeline (net/base.py:15-23), drawn on the host, one yolo_augment_image
per image (include/yolo_hip.h "Training augmentation on the device" defines what the device does with it; DESIGN.md lists the deliberate
differences from imgaug).

    Fliplr(0.5), Flipud(0.5)                      flip_lr, flip_ud
    GaussianBlur((0, 3.0))                        sigma ~ U(0, 3) -> gauss_taps: radius and 8-bit fixed-point taps
    Dropout(0.02)                                 drop_thr = round(0.02 * 2^32)
    AdditiveGaussianNoise(scale=0.01 * 255)       noise_q[0] = noise_q(2.55), noise_loc[0] = 0
    AdditiveGaussianNoise(loc=32, scale=0.0255)   noise_q[1] = noise_q(0.0255) = 11 (d == 0 everywhere: exactly + 32), noise_loc[1] = 32
    Affine(translate_px={"x": (-40, 40)})         tx, an integer uniform in [-40, 40]

draw() consumes a random.Random in a fixed order, whatever it draws -- six calls per image:
    random() < prob -> enabled;  random() < 0.5 -> flip_lr;  random() < 0.5 -> flip_ud;  3 * random() -> sigma;
    int(81 * random()) - 40 -> tx;  getrandbits(64) -> key (low word key[0], high word key[1])
so a run is reproducible from the seed of stream().
"""
import math

import numpy as np

from .. import _hip

MAX_RADIUS = 9
DROP_PROBABILITY = 0.02
NOISE_SCALES = (0.01 * 255, 0.0001 * 255)
NOISE_LOCS = (0, 32)
MAX_SHIFT = 40
MAX_SIGMA = 3.0
# standard deviation of s, the sum of four uniform 16-bit numbers less 131070
S_SIGMA = math.sqrt((65536.0 ** 2 - 1.0) / 3.0)


def gauss_taps(sigma):
    """(radius, taps[10]) of a Gaussian of standard deviation sigma: radius min(9, ceil(3 sigma)); the float64 weights
    exp(-k^2 / (2 sigma^2)) / sum are rounded to 1 / 256 for k >= 1, the centre taps[0] takes what is left of 256, and taps that rounded to
    0 at the end shorten the radius (rounding is Python's round: halves to even).  sigma <= 0, and a sigma so small that taps[1] rounds
    to 0 (0.1 for one), gives radius 0, taps[0] = 256: the identity."""
    sigma = float(sigma)
    taps = [0] * (MAX_RADIUS + 1)
    radius = min(MAX_RADIUS, int(math.ceil(3.0 * sigma))) if sigma > 0 else 0
    if radius > 0:
        g = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(radius + 1)]
        total = g[0] + 2.0 * sum(g[1:])
        for k in range(1, radius + 1):
            taps[k] = int(round(256.0 * g[k] / total))
        while radius > 0 and taps[radius] == 0:
            radius -= 1
    taps[0] = 256 - 2 * sum(taps[1:])
    return radius, taps


def noise_q(scale):
    """the 14-bit multiplier of a noise step of standard deviation `scale` (in 8-bit steps): round(scale * 2^24 / 37837.227)"""
    q = int(round(float(scale) * (1 << 24) / S_SIGMA))
    if not 0 <= q <= 16383:
        raise ValueError("noise scale %r is outside what noise_q holds (0 .. %.2f)" % (scale, 16383 * S_SIGMA / (1 << 24)))
    return q


def make(enabled=True, flip_lr=False, flip_ud=False, sigma=0.0, drop=0.0, scales=(0.0, 0.0), locs=(0, 0), tx=0, key=0, taps=None):
    """a yolo_augment_image from plain values: drop is a probability (or an integer threshold), key a 64-bit integer, taps an explicit
    (radius, taps) instead of sigma"""
    p = _hip.AugmentImage()
    p.enabled, p.flip_lr, p.flip_ud = int(bool(enabled)), int(bool(flip_lr)), int(bool(flip_ud))
    radius, t = taps if taps is not None else gauss_taps(sigma)
    p.radius = int(radius)
    for k in range(MAX_RADIUS + 1):
        p.taps[k] = int(t[k]) if k < len(t) else 0
    p.drop_thr = int(drop) if isinstance(drop, int) else min(0xffffffff, int(round(float(drop) * 2.0 ** 32)))
    for i in range(2):
        p.noise_q[i] = noise_q(scales[i])
        p.noise_loc[i] = int(locs[i])
    p.tx = int(tx)
    p.key[0], p.key[1] = int(key) & 0xffffffff, (int(key) >> 32) & 0xffffffff
    return p


def check(p, h, w):
    """yolo_augment_check: raises _hip.YoloHipError with the field's message"""
    _hip.check(_hip.lib().yolo_augment_check(p, int(h), int(w)), "yolo_augment_check")


def stream(seed):
    """the generator the head trainer draws the augmentation from: its own random.Random, so that the shuffle of the batches (seeded with
    `seed` itself) is the same with and without augmentation"""
    import random
    return random.Random("augment-%d" % int(seed))


def draw(rng, prob, h, w):
    """One image's parameters with the reference's distribution, from six calls of `rng` (a random.Random) in the order of the module's
    docstring.  An image that is not enabled still consumes its six calls."""
    enabled = rng.random() < float(prob)
    flip_lr = rng.random() < 0.5
    flip_ud = rng.random() < 0.5
    sigma = MAX_SIGMA * rng.random()
    tx = int((2 * MAX_SHIFT + 1) * rng.random()) - MAX_SHIFT
    key = rng.getrandbits(64)
    radius, taps = gauss_taps(sigma)
    radius = min(radius, int(h) - 1, int(w) - 1)        # (an image smaller than the blur: the taps beyond it go to the centre)
    taps = taps[:radius + 1] + [0] * (MAX_RADIUS - radius)
    taps[0] = 256 - 2 * sum(taps[1:])
    p = make(enabled, flip_lr, flip_ud, drop=DROP_PROBABILITY, scales=NOISE_SCALES, locs=NOISE_LOCS, tx=tx, key=key, taps=(radius, taps))
    check(p, h, w)
    return p


def params_array(params):
    """list of yolo_augment_image -> the ctypes array yolo_augment_u8 takes"""
    arr = (_hip.AugmentImage * max(len(params), 1))()
    for i, p in enumerate(params):
        arr[i] = p
    return arr


def truths(p, gts, h, w):
    """yolo_augment_truths_host on one image's list of (x, y, w, h, class_idx[, difficult]) -> the list of the truths that are left, as
    (x, y, w, h, class_idx, difficult) with the float32 values the device will see"""
    from . import evaluate as yeval
    import ctypes as C
    arr, _ = yeval.pack_gts([gts], max(1, len(gts)))
    rec = np.ascontiguousarray(arr[0])
    out = np.zeros_like(rec)
    n_out = C.c_int32(0)
    _hip.check(_hip.lib().yolo_augment_truths_host(rec.ctypes.data, len(gts), p, int(h), int(w), out.ctypes.data, C.byref(n_out)),
               "yolo_augment_truths_host")
    return [(float(t["x"]), float(t["y"]), float(t["w"]), float(t["h"]), int(t["class_idx"]), int(t["difficult"])) for t in out[:n_out.value]]

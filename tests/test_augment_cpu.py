"""CPU: the host side of the training augmentation (include/yolo_hip.h "Training augmentation on the device") -- the yardstick of
tests/augment_ref.py against the generator's known answers and its own invariants, net/augment.py (taps, draw), yolo_augment_check,
yolo_augment_truths_host bit for bit against float64 NumPy, the [TRAIN] key gate, and the sanitizer run of the host code as a program of
its own."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import augment_ref as ref
from helpers import ROOT
from tensorflow_yolo_amd import YoloV2, _hip, launcher
from tensorflow_yolo_amd.net import augment as yaug, evaluate as yeval, train as ytrain


def last_error():
    return _hip.lib().yolo_last_error().decode()


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
def test_yardstick_reproduces_the_philox_known_answers():
    zero = [int(v) for v in ref.philox4x32_10(0, 0, 0, 0, 0, 0)]
    ones = [int(v) for v in ref.philox4x32_10(*([0xFFFFFFFF] * 6))]
    assert zero == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert ones == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    # arrays of counters are the scalar calls
    got = ref.philox4x32_10(np.array([0, 0xFFFFFFFF, 7]), np.array([0, 0xFFFFFFFF, 1]), np.array([0, 0xFFFFFFFF, 0]), np.array([0, 0xFFFFFFFF, 0]), 0, 0)
    assert [int(g[0]) for g in got] == zero
    seven = [int(v) for v in ref.philox4x32_10(7, 1, 0, 0, 0, 0)]
    assert [int(g[2]) for g in got] == seven and seven != zero


def test_blur_of_a_constant_image_returns_it_and_flips_are_involutions():
    rng = np.random.RandomState(1)
    S = rng.randint(0, 256, size=(21, 24, 3)).astype(np.uint8)
    for sigma in (0.0, 0.4, 1.0, 2.2, 3.0):
        radius, taps = yaug.gauss_taps(sigma)
        for v in (0, 1, 127, 255):
            const = np.full((21, 24, 3), v, dtype=np.uint8)
            assert np.array_equal(ref.blur(const, radius, taps), const), (sigma, v)
    assert np.array_equal(ref.blur(S, 0, [256]), S)
    for lr, ud in ((1, 0), (0, 1), (1, 1)):
        once = ref.flip(S, lr, ud)
        assert not np.array_equal(once, S) and np.array_equal(ref.flip(once, lr, ud), S)
    # a one-hot image shows the taps themselves: the centre row of the blurred image is taps (x) taps, rounded
    one = np.zeros((21, 24, 3), dtype=np.uint8)
    one[10, 12, 1] = 255
    radius, taps = yaug.gauss_taps(1.0)
    B = ref.blur(one, radius, taps)
    assert B[:, :, 0].max() == 0 and B[10, 12, 1] == (255 * taps[0] * taps[0] + 32768) >> 16
    assert B[10, 12 + radius, 1] == (255 * taps[0] * taps[radius] + 32768) >> 16 and B[10 - radius, 12, 1] == B[10, 12 + radius, 1]


# ---- net/augment.py ---------------------------------------------------------------------------------------------------------------------
def test_gauss_taps_add_up_to_256_and_small_sigmas_are_the_identity():
    for sigma in np.linspace(0.0, 3.0, 61):
        radius, taps = yaug.gauss_taps(sigma)
        assert len(taps) == 10 and 0 <= radius <= 9 and radius <= int(np.ceil(3 * sigma))
        assert taps[0] + 2 * sum(taps[1:radius + 1]) == 256 and all(t == 0 for t in taps[radius + 1:])
        assert all(taps[k] >= taps[k + 1] for k in range(9)) and taps[0] > 0 and (radius == 0 or taps[radius] > 0)
        if sigma <= 0.1:
            assert radius == 0 and taps[0] == 256
        yaug.check(yaug.make(taps=(radius, taps)), 32, 32)
    # (sigma = 3: the 9th weight is 0.38 / 256 and rounds to 0, so the radius that is left is 8)
    assert yaug.gauss_taps(3.0)[0] == 8 and yaug.gauss_taps(1.0)[0] == 3 and yaug.gauss_taps(-1.0) == (0, [256] + [0] * 9)
    # against the weights themselves: every tap within half a step of 256 * g, the centre within the steps it absorbs
    radius, taps = yaug.gauss_taps(2.0)
    g = np.exp(-np.arange(-radius, radius + 1) ** 2 / 8.0)
    g = 256 * g / g.sum()
    assert all(abs(taps[abs(k)] - g[k + radius]) <= 0.5 for k in range(-radius, radius + 1) if k) and abs(taps[0] - g[radius]) <= radius


def test_noise_q_and_the_default_record():
    assert yaug.noise_q(2.55) == int(np.rint(2.55 * 2 ** 24 / ref.S_SIGMA)) == 1131 and yaug.noise_q(0.0255) == 11 and yaug.noise_q(0) == 0
    assert 131070 * 11 < 2 ** 23       # the second step has d == 0 everywhere: exactly + 32
    with pytest.raises(ValueError):
        yaug.noise_q(40.0)
    p = yaug.draw(random.Random(5), 1.0, 416, 416)
    assert p.enabled == 1 and p.drop_thr == int(np.rint(0.02 * 2 ** 32)) == 85899346
    assert list(p.noise_q) == [1131, 11] and list(p.noise_loc) == [0, 32] and -40 <= p.tx <= 40
    assert C.sizeof(_hip.AugmentImage) == 68


def test_draw_is_reproducible_from_a_seed_and_has_the_reference_distribution():
    as_tuple = lambda p: (p.enabled, p.flip_lr, p.flip_ud, p.radius, tuple(p.taps), p.drop_thr, tuple(p.noise_q), tuple(p.noise_loc), p.tx, tuple(p.key))
    a = [as_tuple(yaug.draw(r, 0.5, 416, 416)) for r in [yaug.stream(3)] for _ in range(400)]
    b = [as_tuple(yaug.draw(r, 0.5, 416, 416)) for r in [yaug.stream(3)] for _ in range(400)]
    c = [as_tuple(yaug.draw(r, 0.5, 416, 416)) for r in [yaug.stream(4)] for _ in range(400)]
    assert a == b and a != c
    # six calls per image, whatever was drawn: the stream of the 3rd image does not depend on the probability
    r1, r2 = yaug.stream(9), yaug.stream(9)
    for _ in range(2):
        yaug.draw(r1, 0.0, 416, 416), yaug.draw(r2, 1.0, 416, 416)
    assert as_tuple(yaug.draw(r1, 1.0, 416, 416)) == as_tuple(yaug.draw(r2, 1.0, 416, 416))
    r = random.Random(1)
    manual = (r.random() < 0.5, r.random() < 0.5, r.random() < 0.5, 3.0 * r.random(), int(81 * r.random()) - 40, r.getrandbits(64))
    p = yaug.draw(random.Random(1), 0.5, 416, 416)
    assert (p.enabled, p.flip_lr, p.flip_ud, p.tx) == (int(manual[0]), int(manual[1]), int(manual[2]), manual[4])
    assert (p.radius, list(p.taps)) == tuple(yaug.gauss_taps(manual[3])) and p.key[0] | (p.key[1] << 32) == manual[5]
    # shares over 400 draws, 5 binomial sigmas (0.125) around 0.5; the shifts span their range and every radius a sigma below 3 gives occurs
    n = 400.0
    for k in (0, 1, 2):
        assert abs(sum(t[k] for t in a) / n - 0.5) <= 0.125
    assert {t[8] for t in a} <= set(range(-40, 41)) and min(t[8] for t in a) <= -38 and max(t[8] for t in a) >= 38
    assert {t[3] for t in a} == set(range(9))          # (a radius of 9 needs taps of the caller's own: at sigma = 3 the 9th rounds to 0)
    assert all(yaug.draw(yaug.stream(1), 0.0, 416, 416).enabled == 0 for _ in range(3))
    # an image smaller than the blur keeps a record the library accepts
    for _ in range(20):
        p = yaug.draw(r, 1.0, 4, 4)
        assert p.radius <= 3 and p.taps[0] + 2 * sum(p.taps[1:p.radius + 1]) == 256


def test_default_parameters_at_416_have_the_shares_the_header_states():
    """one key: the dropped share within 5 binomial sigmas of 0.02, the first noise step's standard deviation within 2 % of
    sqrt(2.55^2 + 1/12) (the rounding to integers adds the 1/12), the second step identically 0"""
    p = yaug.make(drop=yaug.DROP_PROBABILITY, scales=yaug.NOISE_SCALES, locs=yaug.NOISE_LOCS, key=0x0123456789abcdef)
    dropped, d0, d1 = ref.pixel_steps(416, 416, p)
    share, sd = float(dropped.mean()), float(d0.std())
    five_sigma = 5 * np.sqrt(0.02 * 0.98 / (416 * 416))
    want_sd = np.sqrt(2.55 ** 2 + 1 / 12.0)
    print("dropped share %.5f (0.02 +- %.5f); noise-0 sd %.4f (want %.4f); noise-0 mean %.4f; max |d0| %d" % (share, five_sigma, sd, want_sd, d0.mean(), np.abs(d0).max()))
    assert abs(share - 0.02) <= five_sigma
    assert abs(sd - want_sd) <= 0.02 * want_sd
    assert not d1.any()
    assert np.abs(d0).max() <= int(np.ceil(3.47 * 2.55))       # Irwin-Hall(4): the tails end at 3.46 sigma


# ---- yolo_augment_check -------------------------------------------------------------------------------------------------------------------
def test_check_refuses_each_bad_field_with_its_own_message():
    lib = _hip.lib()
    good = lambda: yaug.make(flip_lr=True, sigma=1.0, drop=0.02, scales=yaug.NOISE_SCALES, locs=yaug.NOISE_LOCS, tx=-40, key=1)
    assert lib.yolo_augment_check(good(), 32, 32) == 0
    cases = [("enabled", 2, "enabled"), ("flip_lr", 2, "flip_lr"), ("flip_ud", -1, "flip_ud"), ("radius", 10, "radius must be 0 .. 9"),
             ("radius", -1, "radius must be 0 .. 9"), ("radius", 2, "taps"), ("tx", (1 << 30) + 1, "tx"), ("tx", -(1 << 31), "tx")]
    seen = set()
    for field, value, word in cases:
        p = good()
        setattr(p, field, value)
        assert lib.yolo_augment_check(p, 32, 32) == 1 and word in last_error(), (field, last_error())
        seen.add(last_error())
    for i in (0, 1):
        for field, value, word in (("noise_q", 16384, "noise_q"), ("noise_q", -1, "noise_q"), ("noise_loc", 256, "noise_loc"), ("noise_loc", -256, "noise_loc")):
            p = good()
            getattr(p, field)[i] = value
            assert lib.yolo_augment_check(p, 32, 32) == 1 and word in last_error(), (field, i, last_error())
            seen.add(last_error())
    p = good()
    p.taps[0] += 1
    assert lib.yolo_augment_check(p, 32, 32) == 1 and "taps" in last_error() and "257" in last_error()
    assert len(seen) == 8           # enabled, flip_lr, flip_ud, radius, taps, tx, noise_q, noise_loc: a message each
    assert lib.yolo_augment_check(None, 32, 32) == 1 and "null" in last_error()
    assert lib.yolo_augment_check(good(), 0, 32) == 1 and "at least 1" in last_error()
    assert lib.yolo_augment_check(good(), 32, 34) == 1 and "multiple of 4" in last_error()
    assert lib.yolo_augment_check(good(), 1 << 16, 1 << 16) == 1 and "31 bits" in last_error()
    assert lib.yolo_augment_check(good(), 3, 32) == 1 and "below h and w" in last_error()       # radius 3
    assert lib.yolo_augment_check(good(), 4, 4) == 0
    p = good()
    p.enabled, p.radius = 0, 77                 # not enabled: nothing else is looked at
    assert lib.yolo_augment_check(p, 32, 32) == 0
    # the launch entry runs the same checks before it touches anything: numbers stand in for device pointers
    arr = yaug.params_array([good(), good(), good()])
    arr[2].radius = 12
    assert lib.yolo_augment_u8(4096, 1 << 20, 3, 32, 32, arr, None) == 1 and "image 2: radius" in last_error()
    arr[2].radius = good().radius
    assert lib.yolo_augment_u8(4096, 4096 + 3 * 32 * 32 * 3 - 1, 3, 32, 32, arr, None) == 1 and "overlap" in last_error()
    assert lib.yolo_augment_u8(None, 4096, 3, 32, 32, arr, None) == 1 and "null" in last_error()
    assert lib.yolo_augment_u8(4096, 1 << 20, 0, 32, 32, arr, None) == 1
    rows, cols, per_launch = _hip.augment_tile()
    assert rows >= 4 and cols >= 4 and cols % 4 == 0 and 1 <= per_launch and per_launch * C.sizeof(_hip.AugmentImage) <= 2 * 4096
    assert lib.yolo_augment_tile(None, None, None) == 0


# ---- truths -----------------------------------------------------------------------------------------------------------------------------
def run_truths(gt, p, h, w):
    """yolo_augment_truths_host on a GT_DTYPE array -> the GT_DTYPE array it wrote"""
    gt = np.ascontiguousarray(gt, dtype=yeval.GT_DTYPE)
    out = np.zeros(max(len(gt), 1), dtype=yeval.GT_DTYPE)
    n_out = C.c_int32(-1)
    rc = _hip.lib().yolo_augment_truths_host(gt.ctypes.data if len(gt) else None, len(gt), p, h, w, out.ctypes.data if len(gt) else None, C.byref(n_out))
    assert rc == 0, last_error()
    return out[:n_out.value]


def edge_boxes(W):
    """boxes inside, across each edge, exactly on each edge, and outside on each side, in units that make the edges exact"""
    px = 1.0 / W
    boxes = [(0.5, 0.5, 0.2, 0.3), (0.3, 0.7, 0.1, 0.1),                                           # inside
             (0.05, 0.5, 0.2, 0.2), (0.95, 0.5, 0.2, 0.2), (0.5, 0.05, 0.2, 0.2), (0.5, 0.95, 0.2, 0.2),     # across each edge
             (0.125, 0.5, 0.25, 0.25), (0.875, 0.5, 0.25, 0.25), (0.5, 0.125, 0.25, 0.25), (0.5, 0.875, 0.25, 0.25),   # exactly on an edge
             (-0.125, 0.5, 0.25, 0.25), (1.125, 0.5, 0.25, 0.25), (0.5, -0.125, 0.25, 0.25), (0.5, 1.125, 0.25, 0.25),  # touching from outside: dropped
             (-0.5, 0.5, 0.2, 0.2), (1.5, 0.5, 0.2, 0.2), (0.5, -0.5, 0.2, 0.2), (0.5, 1.5, 0.2, 0.2),  # outside
             (40 * px, 0.5, 80 * px, 0.5), (1 - 20 * px, 0.5, 40 * px, 0.5),                         # leave exactly at tx = -40 / land on the edge at +40
             (0.5, 0.5, 1.0, 1.0), (0.5, 0.5, 3.0, 3.0), (0.5, 0.5, 0.0, 0.0),                       # the whole image, more, a point
             (np.nan, 0.5, 0.1, 0.1), (0.5, 0.5, 0.1, np.nan), (np.inf, 0.5, 0.1, 0.1)]
    gt = np.zeros(len(boxes), dtype=yeval.GT_DTYPE)
    for i, b in enumerate(boxes):
        gt[i] = b + (i, i % 2)
    return gt


@pytest.mark.parametrize("W", [416, 100, 36])
def test_truths_equal_the_float64_yardstick_bit_for_bit(W):
    gt = edge_boxes(W)
    rng = np.random.RandomState(W)
    rand = np.zeros(200, dtype=yeval.GT_DTYPE)
    rand["x"], rand["y"] = rng.uniform(-0.3, 1.3, 200), rng.uniform(-0.3, 1.3, 200)
    rand["w"], rand["h"] = rng.uniform(0, 0.6, 200), rng.uniform(0, 0.6, 200)
    rand["class_idx"] = np.arange(200)
    total = dropped = cut = 0
    for lr in (0, 1):
        for ud in (0, 1):
            for tx in (0, 1, -1, 40, -40, 17, W, -W - 5, 3 * W):
                p = yaug.make(flip_lr=lr, flip_ud=ud, tx=tx)
                for boxes in (gt, rand):
                    got, want = run_truths(boxes, p, 64, W), ref.augment_truths(boxes, p, 64, W)
                    assert got.tobytes() == want.tobytes(), (lr, ud, tx)
                    total += len(boxes)
                    dropped += len(boxes) - len(got)
                    cut += int(np.sum(got["w"] < boxes["w"][np.isin(boxes["class_idx"], got["class_idx"])]))
                    assert list(got["class_idx"]) == sorted(got["class_idx"])            # the order is kept
                    if len(got):
                        lo_x, hi_x = got["x"].astype(np.float64) - got["w"] / 2.0, got["x"].astype(np.float64) + got["w"] / 2.0
                        assert lo_x.min() >= -1e-6 and hi_x.max() <= 1 + 1e-6
    assert dropped > total // 4 and cut > 100 and total - dropped > total // 4          # the cases reach every branch
    # what a few of them give, stated: both flips of a box, a shift out of the image, a box cut at the left edge
    one = np.array([(0.25, 0.75, 0.25, 0.125, 4, 1)], dtype=yeval.GT_DTYPE)
    got = run_truths(one, yaug.make(flip_lr=1, flip_ud=1), 64, W)
    assert got.tolist() == [(0.75, 0.25, 0.25, 0.125, 4, 1)]
    assert len(run_truths(one, yaug.make(tx=W), 64, W)) == 0 and len(run_truths(one, yaug.make(tx=-W), 64, W)) == 0
    got = run_truths(np.array([(0.0, 0.5, 0.5, 0.5, 0, 0)], dtype=yeval.GT_DTYPE), yaug.make(), 64, W)
    assert got.tolist() == [(0.125, 0.5, 0.25, 0.5, 0, 0)]


def test_truths_disabled_empty_and_many():
    gt = edge_boxes(416)
    off = yaug.make(enabled=False, flip_lr=True, tx=40)
    assert run_truths(gt, off, 416, 416).tobytes() == gt.tobytes() == ref.augment_truths(gt, off, 416, 416).tobytes()     # NaN and all
    p = yaug.make(flip_lr=True, flip_ud=True, tx=-33)
    assert len(run_truths(gt[:0], p, 416, 416)) == 0 and len(ref.augment_truths(gt[:0], p, 416, 416)) == 0
    rng = np.random.RandomState(2)
    many = np.zeros(1024, dtype=yeval.GT_DTYPE)
    many["x"], many["y"], many["w"], many["h"] = rng.uniform(-0.2, 1.2, (4, 1024)) * np.array([[1], [1], [0.4], [0.4]])
    many["class_idx"], many["difficult"] = np.arange(1024), rng.randint(0, 2, 1024)
    got = run_truths(many, p, 416, 416)
    assert 0 < len(got) < 1024 and got.tobytes() == ref.augment_truths(many, p, 416, 416).tobytes()
    # in place
    buf = many.copy()
    n_out = C.c_int32(0)
    assert _hip.lib().yolo_augment_truths_host(buf.ctypes.data, 1024, p, 416, 416, buf.ctypes.data, C.byref(n_out)) == 0
    assert buf[:n_out.value].tobytes() == got.tobytes()
    # the Python wrapper: lists of tuples in, lists of tuples out
    lst = yaug.truths(p, [tuple(t) for t in many[:50].tolist()], 416, 416)
    want = ref.augment_truths(many[:50], p, 416, 416)
    assert yeval.pack_gts([lst], max(1, len(lst)))[0][0][:len(lst)].tobytes() == want.tobytes()
    # refusals
    lib = _hip.lib()
    assert lib.yolo_augment_truths_host(None, 1, p, 416, 416, buf.ctypes.data, C.byref(n_out)) == 1 and "null" in last_error()
    assert lib.yolo_augment_truths_host(buf.ctypes.data, -1, p, 416, 416, buf.ctypes.data, C.byref(n_out)) == 1 and "negative" in last_error()
    assert lib.yolo_augment_truths_host(buf.ctypes.data, 1, p, 416, 416, buf.ctypes.data, None) == 1
    bad = yaug.make()
    bad.radius = 11
    assert lib.yolo_augment_truths_host(buf.ctypes.data, 1, bad, 416, 416, buf.ctypes.data, C.byref(n_out)) == 1 and "radius" in last_error()


# ---- the [TRAIN] key ----------------------------------------------------------------------------------------------------------------------
def test_the_augment_key_gates_the_probability(tmp_path):
    v = "v2-tiny"
    assert ytrain.check_params({"augment_probability": "0.0"}, v) == 0.0 and ytrain.check_params({}, v) == 0.0
    with pytest.raises(ValueError, match="augment_probability must be 0: augmentation is not built"):
        ytrain.check_params({"augment_probability": "0.5"}, v)
    assert ytrain.check_params({"augment": "device", "augment_probability": "0.5"}, v) == 0.5
    assert ytrain.check_params({"augment": " Device ", "augment_probability": "1"}, v) == 1.0
    assert ytrain.check_params({"augment": "device", "augment_probability": "0"}, v) == 0.0
    assert ytrain.check_params({"augment": "device"}, v) == 0.0
    for bad in ("1.5", "-0.1", "nan"):
        with pytest.raises(ValueError, match=r"augment_probability must be in \[0, 1\]"):
            ytrain.check_params({"augment": "device", "augment_probability": bad}, v)
    with pytest.raises(ValueError, match="augment must be device"):
        ytrain.check_params({"augment": "host", "augment_probability": "0.5"}, v)
    with pytest.raises(NotImplementedError):
        ytrain.check_params({"augment": "device", "augment_probability": "0.5"}, "v3")
    # the launcher says so before anything is built; YoloV2.train too
    ini = tmp_path / "t.ini"
    ini.write_text("[COMMON]\nversion = v2\n[TRAIN]\ntrain_layers = head\naugment = device\naugment_probability = 1.5\n")
    with pytest.raises(ValueError, match=r"must be in \[0, 1\]"):
        launcher.run(launcher.read_config(str(ini)), "train")
    ini.write_text("[COMMON]\nversion = v2\n[TRAIN]\ntrain_layers = head\naugment = cpu\naugment_probability = 0.5\n")
    with pytest.raises(ValueError, match="augment must be device"):
        launcher.run(launcher.read_config(str(ini)), "train")
    with pytest.raises(ValueError, match="must be in"):
        YoloV2().train({"train_layers": "head", "augment": "device", "augment_probability": "2"})
    # the shipped configs: the augmenting one passes the gate, the plain one keeps 0
    cfg = launcher.read_config(os.path.join(ROOT, "tensorflow-yolo_amd", "config", "yolo_2_head_train_augment.ini"))
    params = dict(cfg["TRAIN"], **cfg["COMMON"])
    assert ytrain.train_option(params) and 0 < ytrain.check_params(params, params["version"]) <= 1
    cfg = launcher.read_config(os.path.join(ROOT, "tensorflow-yolo_amd", "config", "yolo_2_head_train.ini"))
    params = dict(cfg["TRAIN"], **cfg["COMMON"])
    assert "augment" not in params and ytrain.check_params(params, params["version"]) == 0.0


# ---- the host code under the sanitizers ----------------------------------------------------------------------------------------------------
def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """`make san-augment`: augment_host.cpp with augment_host_check.cpp, a program of its own, on the CPU"""
    csrc = os.path.join(ROOT, "tensorflow-yolo_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc, "san-augment", "OBJDIR=" + str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "augment_host_check OK" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr

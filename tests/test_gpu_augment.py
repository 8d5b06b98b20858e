"""GPU: the training augmentation (include/yolo_hip.h "Training augmentation on the device") through the C ABI, yolo_augment_u8, against the
NumPy yardstick of tests/augment_ref.py with np.array_equal and no tolerance, and the launcher's train mode with `augment = device`.

Every call writes into a destination with a 256-byte 0xA5 guard band on both sides, pre-filled with 0x00 and then with 0xFF bytes: both
results are compared, the bands and the source must be untouched.  The shapes are sized from yolo_augment_tile: 32 x 32 (less than one
tile), three tiles in each direction with a ragged last one, one tile wide and three high, and images_per_launch + 2 images (a second
launch)."""
import ctypes as C
import random

import numpy as np
import pytest

import augment_ref as ref
from tensorflow_yolo_amd import YoloV2Tiny, _hip, launcher
from tensorflow_yolo_amd.net import augment as yaug, base, engine, evaluate as yeval, synth, train as ytrain, v3

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 256, 0xA5
ROWS, COLS, PER_LAUNCH = _hip.augment_tile()
SMALL = (32, 32)
RAGGED = (2 * ROWS + 12, 2 * COLS + 20)         # three tiles in each direction, the last one ragged
TALL = (2 * ROWS + 4, COLS - 24)                # non-square the other way: one ragged tile wide, three high
SHAPES = [SMALL, RAGGED, TALL]
NOISY = dict(drop=0.02, scales=yaug.NOISE_SCALES, locs=yaug.NOISE_LOCS)


def image(shape, seed, n=1):
    return np.random.RandomState(seed).randint(0, 256, size=(n,) + tuple(shape) + (3,)).astype(np.uint8)


def run(X, params, offset=0):
    """yolo_augment_u8 on the batch X [n, h, w, 3] -> the result; the destination starts `offset` bytes behind a 256-byte boundary"""
    import torch
    lib = _hip.lib()
    n, h, w, _ = X.shape
    nbytes = X.size
    src = torch.from_numpy(X).cuda()
    outs = []
    for fill in (0x00, 0xFF):
        buf = torch.full((GUARD + offset + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        buf[GUARD + offset:GUARD + offset + nbytes] = fill
        _hip.check(lib.yolo_augment_u8(src.data_ptr(), buf.data_ptr() + GUARD + offset, n, h, w, yaug.params_array(params),
                                       torch.cuda.current_stream().cuda_stream), "yolo_augment_u8")
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:GUARD + offset] == PATTERN).all() and (host[GUARD + offset + nbytes:] == PATTERN).all(), "a guard band was written"
        outs.append(host[GUARD + offset:GUARD + offset + nbytes].reshape(X.shape))
    assert np.array_equal(src.cpu().numpy(), X), "the source was written"
    assert np.array_equal(outs[0], outs[1]), "the result depends on what the destination held"
    return outs[0]


def check(X, params, offset=0):
    got = run(X, params, offset)
    want = ref.augment_batch(X, params)
    for i in range(len(X)):
        bad = np.argwhere(got[i] != want[i])
        assert len(bad) == 0, "image %d: %d bytes differ, first at (y, x, c) = %s: got %d, want %d" % (
            i, len(bad), tuple(bad[0]), got[i][tuple(bad[0])], want[i][tuple(bad[0])])
    return got


OPS = {
    "flip_lr": dict(flip_lr=True),
    "flip_ud": dict(flip_ud=True),
    "both_flips": dict(flip_lr=True, flip_ud=True),
    "blur": dict(sigma=1.5),
    "dropout": dict(drop=0.3, key=0x1234567890abcdef),
    "noise0": dict(scales=(2.55, 0.0), key=77),
    "noise1_loc": dict(scales=(0.0, 0.0255), locs=(0, 32)),
    "noise1_wide": dict(scales=(0.0, 30.0), locs=(0, -20), key=0xfedcba9876543210),
    "noise_saturates": dict(scales=(36.0, 36.0), locs=(200, -255), key=5),
    "shift": dict(tx=7),
    "identity": dict(),
}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("op", sorted(OPS))
def test_each_operation_alone(op, shape):
    X = image(shape, 11)
    got = check(X, [yaug.make(**OPS[op])])
    if op == "identity":
        assert np.array_equal(got, X)
    else:
        assert not np.array_equal(got, X)


def tent_taps(radius):
    """taps that fall by 2 per step from 2 * radius beside the centre: every one of them is non-zero and different"""
    taps = [0] * 10
    for k in range(1, radius + 1):
        taps[k] = 2 * (radius + 1 - k)
    taps[0] = 256 - 2 * sum(taps)
    return radius, taps


@pytest.mark.parametrize("radius", range(1, 10))
def test_blur_of_every_radius_on_one_hot_and_random_images(radius):
    h, w = RAGGED
    one = np.zeros((4, h, w, 3), dtype=np.uint8)
    one[0, h // 2, w // 2, 0] = 255         # inside a tile
    one[1, 0, 0, 1] = 255                   # a corner: both borders reflect
    one[2, h - 1, w - 1, 2] = 255           # the far corner, in the ragged tiles
    one[3, ROWS, COLS, :] = 255             # where four tiles meet
    p = yaug.make(taps=tent_taps(radius))
    got = check(one, [p] * 4)
    taps = list(p.taps)
    assert got[0, h // 2, w // 2 + radius, 0] == (255 * taps[0] * taps[radius] + 32768) >> 16 and got[0, :, :, 1:].max() == 0
    check(image(RAGGED, 20 + radius), [p])
    check(image(SMALL, 40 + radius), [p])
    check(np.full((1,) + TALL + (3,), 255, dtype=np.uint8), [p])        # the largest sums: Hs = 65280


@pytest.mark.parametrize("thr", [0, 1, 0x7fffffff, 0xfffffffe, 0xffffffff])
def test_dropout_thresholds(thr):
    X = np.maximum(image(RAGGED, 3), 1)
    got = check(X, [yaug.make(drop=thr, key=9)])
    share = float((got == 0).all(axis=-1).mean())        # pixels with all three channels 0 (the image itself has none)
    if thr <= 1:
        assert share == 0
    elif thr >= 0xfffffffe:
        assert share > 0.999
    else:
        assert 0.45 < share < 0.55


def test_shifts():
    for shape in (RAGGED, SMALL):
        h, w = shape
        X = np.maximum(image(shape, 4), 1)
        for tx in (-40, -1, 0, 1, 40, w, -w - 5, w - 1, 1 - w, 1 << 30, -(1 << 30)):
            got = check(X, [yaug.make(tx=tx, **NOISY)])
            lit = (got != 0).any(axis=(0, 1, 3))        # columns with anything in them (the second noise step adds 32 wherever the image is)
            want = np.zeros(w, dtype=bool)
            if abs(tx) < w:
                want[max(tx, 0):w + min(tx, 0)] = True
            assert np.array_equal(lit, want), tx


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_everything_together(shape):
    X = image(shape, 5, n=4)
    params = [yaug.make(flip_lr=i & 1, flip_ud=i >> 1, sigma=(0.7, 1.6, 2.4, 3.0)[i], tx=(-40, 13, 40, -7)[i], key=0x9e3779b97f4a7c15 * (i + 1) & (2 ** 64 - 1),
                        **NOISY) for i in range(4)]
    check(X, params)
    check(X[:1], params[3:], offset=1)          # a destination that is not 4-byte aligned: byte stores
    check(X[:2], params[1:3], offset=2)


def test_batch_of_three_with_one_image_disabled():
    X = image(RAGGED, 6, n=3)
    params = [yaug.make(flip_lr=True, sigma=2.0, tx=21, key=1, **NOISY),
              yaug.make(enabled=False, flip_ud=True, sigma=3.0, tx=-30, key=2, **NOISY),
              yaug.make(flip_ud=True, sigma=0.9, tx=-30, key=3, **NOISY)]
    params[1].radius = 77                       # a record that is not enabled is not looked at
    got = check(X, params)
    assert np.array_equal(got[1], X[1]) and not np.array_equal(got[0], X[0]) and not np.array_equal(got[2], X[2])


def test_more_images_than_one_launch_holds():
    n = PER_LAUNCH + 2
    X = image(SMALL, 7, n=n)
    rng = yaug.stream(7)
    params = [yaug.draw(rng, 0.9, *SMALL) for _ in range(n)]
    assert len({tuple(p.key) for p in params}) == n and sum(p.enabled for p in params) < n
    got = check(X, params)
    assert not np.array_equal(got[n - 1], got[PER_LAUNCH - 1])


def test_the_drawn_parameters_at_the_network_size():
    """416 x 416, what a training step runs: two images drawn with the reference's distribution"""
    X = image((416, 416), 8, n=2)
    rng = yaug.stream(8)
    check(X, [yaug.draw(rng, 1.0, 416, 416) for _ in range(2)])


# ---- the engine and train mode -----------------------------------------------------------------------------------------------------------
HW = (96, 160)
V2_ANCHORS = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071]
VOC_XML = ("<annotation><filename>%s</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>"
           "<object><name>tower</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>"
           "<object><name>tower</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object></annotation>")
SEED, LR = 3, 1e-3


def dataset(root):
    """five training and three validation images of 120 x 200 with two boxes each (one near the left edge: a shift cuts or drops it), a
    backbone-only weight file, and the text of a config without the augmentation keys"""
    from PIL import Image
    rng = np.random.RandomState(52)
    for d in ("train", "val"):
        (root / d).mkdir()
    for d, n in (("train", 5), ("val", 3)):
        for i in range(n):
            name = "im%d.png" % i
            Image.fromarray(rng.randint(0, 256, size=(120, 200, 3)).astype(np.uint8)).save(str(root / d / name))
            x1, y1 = int(rng.randint(0, 100)), int(rng.randint(0, 60))
            (root / d / ("im%d.xml" % i)).write_text(VOC_XML % (name, 200, 120, x1, y1, x1 + int(rng.randint(20, 100)), y1 + int(rng.randint(20, 60)),
                                                                0, 10, int(rng.randint(8, 40)), 100))
    net = YoloV2Tiny.create_network(np.reshape(V2_ANCHORS, [-1, 2]), ["tower"], False, input_shape=HW + (3,))
    full = synth.darknet_stream(net, seed=41, num_classes=1, head_gain=synth.HEAD_DEFAULTS["v2-tiny"][0], obj_bias=0.0)
    base.write_darknet_weights(str(root / "backbone.weights"), full[:len(full) - 30 * 1025], "v2")
    return ("[COMMON]\nversion = v2-tiny\ninput_h = %d\ninput_w = %d\ninput_c = 3\n"
            "[TRAIN]\ntrain_layers = head\nseed = %d\nimage_dir = train/\nannotation_dir = train/\nval_image_dir = val/\nval_annotation_dir = val/\n"
            "batch_size = 2\nlearning_rate = %r\nepochs = 1\nmax_step = -1\ncheckpoint_step = 2\n"
            "checkpoint_prefix = yolo\npretrained_weights_path = backbone.weights\nanchors = %s\nclass_names = [\"tower\"]\n"
            "cpu_only = False\ndtype = fp16\n" % (HW[0], HW[1], SEED, LR, list(V2_ANCHORS)))


def train_run(root, text, out_dir, extra, capsys):
    (root / out_dir).mkdir()
    (root / "cfg.ini").write_text(text + "checkpoint_dir = %s/\n" % out_dir + extra)
    launcher.run(launcher.read_config(str(root / "cfg.ini")), "train")
    out = capsys.readouterr().out.splitlines()
    assert out[-1] == "Done", out[-5:]
    return out


def losses_of(out):
    return [l.split(": ")[1].split(" ")[0] for l in out if l.startswith("step ")] + [l for l in out if l.startswith("validation loss: ")]


def test_train_mode_with_augmentation(tmp_path, capsys):
    """`augment = device` with probability 1 runs to "Done" and its first loss is train_head_step_u8 on the yardstick's batch and truths, bit
    for bit; with probability 0 every printed loss is that of the run without the key"""
    text = dataset(tmp_path)
    plain = train_run(tmp_path, text, "out_plain", "augment_probability = 0.0\n", capsys)
    keyed = train_run(tmp_path, text, "out_keyed", "augment = device\naugment_probability = 0.0\n", capsys)
    full = train_run(tmp_path, text, "out_full", "augment = device\naugment_probability = 1.0\n", capsys)
    assert len(losses_of(plain)) == 3 + 1 and losses_of(keyed) == losses_of(plain)
    assert not any("Augmentation" in l for l in plain + keyed) and any(l == "Augmentation on the device with probability 1.0." for l in full)
    got = losses_of(full)
    assert len(got) == 4 and got[0] != losses_of(plain)[0] and np.isfinite([float(v) for v in got[:3]]).all()
    assert got[3] != losses_of(plain)[3]                # (another head after three other steps; the validation batches are not augmented)

    # the first step again, by hand: the same start, the same first batch, the yardstick's augmentation
    _, body = base.read_darknet_weights(str(tmp_path / "out_full" / "yolo-0.weights"), "v2")
    m = YoloV2Tiny()
    m.build(V2_ANCHORS, ["tower"], HW + (3,), dtype="fp16", max_batch=2, streams=1)
    v3.attach_weights(m.net, body)
    eng = m.net.engine
    cout, cin, _, _ = ytrain.head_counts(m.net)
    eng.head_train_init(*ytrain.split_head(body, cout, cin))
    annotations, _ = yeval.parse_voc_annotations(str(tmp_path / "train"), str(tmp_path / "train"), ["tower"])
    first = ytrain.make_batches(annotations, 2, random.Random(SEED))[0]
    x, truths = ytrain.batch_to_device(eng, first)
    x = x.cpu().numpy()
    rng = yaug.stream(SEED)
    records = [yaug.draw(rng, 1.0, HW[0], HW[1]) for _ in first]
    assert all(p.enabled for p in records)
    xa = ref.augment_batch(x, records)
    ta = []
    for p, t in zip(records, truths):
        rec = ref.augment_truths(yeval.pack_gts([t], len(t))[0][0], p, HW[0], HW[1])
        ta.append([tuple(r) for r in rec.tolist()])
    assert not np.array_equal(xa, x) and ta != [list(t) for t in truths]
    result = eng.train_head_step_u8(xa, ta, engine.adam_lr_t(LR, 1))
    loss = np.float32(result.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]["loss"])
    # (the line prints the float32 through Python's float: the digits of the exact value, which parse back to the same bits)
    assert float(got[0]) == float(loss) and np.float32(float(got[0])).tobytes() == loss.tobytes(), (repr(loss), got[0])
    # and the engine's own entry on the same records is the yardstick's batch
    assert np.array_equal(eng.augment_u8(x, records).cpu().numpy(), xa)
    with pytest.raises(ValueError, match="augmentation records"):
        eng.augment_u8(x, records[:1])

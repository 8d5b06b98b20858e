"""GPU: frames of any size in one call -- the batched resize (stretch / letterbox, uint8 and float32 results), the map of box records
back to frame coordinates, the whole step in one enqueue, and the Python surface (Yolo.predict_frames, the `.ini` key `resize`).
Everything is compared bit for bit (np.array_equal) with tests/frames_ref.py, which builds on oracle/preprocess_ref.py, and with the
entries the project already has (yolo_preprocess_resize_u8, yolo_net_detect_u8)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import frames_ref
import spp_ref
from helpers import GOLDEN
from tensorflow_yolo_amd import YoloV3Tiny, _hip, launcher
from tensorflow_yolo_amd.net import base, synth

pytestmark = pytest.mark.gpu

NAMES80 = ["c%d" % i for i in range(80)]
NETS = [(32, 32), (64, 96), (96, 64)]
N_FRAMES = 70               # one call crosses the 64-frame launch
GUARD = 4096
PATTERN = 0x5A


@functools.lru_cache(maxsize=None)
def dog():
    from PIL import Image
    rgb = np.array(Image.open(os.path.join(GOLDEN, "dog_576x768.jpg")).convert("RGB"), dtype=np.uint8)
    assert rgb.shape == (576, 768, 3)
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def frame_set(H, W):
    """70 seeded random frames cycling through the sizes at which the kernel can go wrong (one pixel, a few, odd, wide, tall, exactly
    the net's size) and the 576 x 768 photograph once; per frame a row pitch (some 3 w + 5), a start offset (some odd) and swap_rb.
    Returns [(pixels, pitch, offset in the device buffer, swap_rb)], the host image of the device buffer."""
    sizes = [(1, 1), (2, 3), (7, 5), (37, 53), (53, 37), (16, 300), (300, 16), (H, W)]
    rng = np.random.default_rng(H * 1000 + W)
    frames, pos = [], 0
    for i in range(N_FRAMES):
        img = dog() if i == 41 else rng.integers(0, 256, size=sizes[i % len(sizes)] + (3,), dtype=np.uint8)
        h, w = img.shape[:2]
        pitch = 3 * w + (5 if i % 3 == 1 else 0)
        pos = (pos + 255) // 256 * 256 + (1 if i % 4 == 2 else 3 if i % 4 == 3 else 0)
        frames.append((img, pitch, pos, 1 if i % 5 == 3 else 0))
        pos += h * pitch
    buf = np.full(pos + 64, 0xA5, dtype=np.uint8)
    for img, pitch, off, _ in frames:
        h, w = img.shape[:2]
        rows = buf[off:off + h * pitch].reshape(h, pitch)
        rows[:, :3 * w] = img.reshape(h, 3 * w)
    buf.setflags(write=False)
    assert any(f[1] != 3 * f[0].shape[1] for f in frames) and any(f[2] % 2 for f in frames) and any(f[3] for f in frames)
    return frames, buf


@functools.lru_cache(maxsize=None)
def want_u8(H, W, mode):
    """the reference batch [70, H, W, 3], computed once per net and mode and shared read-only"""
    out = np.stack([frames_ref.resized_u8(img, H, W, mode, swap_rb=bool(swap)) for img, _, _, swap in frame_set(H, W)[0]])
    out.setflags(write=False)
    return out


def descs_on_device(H, W):
    import torch
    frames, buf = frame_set(H, W)
    dev = torch.from_numpy(np.array(buf)).cuda()
    descs = (_hip.Frame * len(frames))()
    for i, (img, pitch, off, swap) in enumerate(frames):
        descs[i] = _hip.Frame(dev.data_ptr() + off, img.shape[0], img.shape[1], pitch, swap)
    return descs, dev


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("mode", [frames_ref.STRETCH, frames_ref.LETTERBOX], ids=["stretch", "letterbox"])
@pytest.mark.parametrize("H, W", NETS)
def test_batched_resize_equals_the_reference_and_writes_nothing_else(H, W, mode):
    """yolo_preprocess_frames_u8 / yolo_preprocess_frames of 70 frames (two launches) == tests/frames_ref.py, every byte; the 4 KiB
    guards on both sides of the batch tensor keep their pattern; stretch also == yolo_preprocess_resize_u8 called per frame"""
    import torch
    lib = _hip.lib()
    descs, dev = descs_on_device(H, W)
    want = want_u8(H, W, mode)
    n = N_FRAMES
    for u8 in (True, False):
        nbytes = n * H * W * 3 * (1 if u8 else 4)
        buf = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        name = "yolo_preprocess_frames_u8" if u8 else "yolo_preprocess_frames"
        _hip.check(getattr(lib, name)(descs, n, mode, buf.data_ptr() + GUARD, H, W, stream()), name)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:GUARD] == PATTERN).all() and (got[GUARD + nbytes:] == PATTERN).all(), "a write outside the batch tensor"
        body = got[GUARD:GUARD + nbytes]
        if u8:
            body = body.reshape(n, H, W, 3)
            bad = [i for i in range(n) if not np.array_equal(body[i], want[i])]
            assert not bad, (name, "frames", bad)
        else:
            body = body.view(np.uint32).reshape(n, H, W, 3)
            ref = frames_ref.to_f32(want).view(np.uint32)
            bad = [i for i in range(n) if not np.array_equal(body[i], ref[i])]
            assert not bad, (name, "frames", bad)
    if mode == frames_ref.STRETCH:
        one = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        for i in range(n):
            d = descs[i]
            _hip.check(lib.yolo_preprocess_resize_u8(d.pixels_dev, d.h, d.w, d.row_bytes, one[i].data_ptr(), H, W, d.swap_rb, stream()), "yolo_preprocess_resize_u8")
        assert np.array_equal(one.cpu().numpy(), want)
    else:
        assert (want[:, 0, 0] == frames_ref.CANVAS).all(axis=1).sum() >= 40       # (the canvas really shows in most frames)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
def test_batched_resize_into_an_unaligned_tensor(u8):
    """a batch tensor that starts 1 byte (uint8) / 4 bytes (float32) off the alignment of the wide stores: same bytes, same guards"""
    import torch
    lib = _hip.lib()
    H, W, n = 64, 96, 9
    descs, dev = descs_on_device(H, W)
    want = want_u8(H, W, frames_ref.LETTERBOX)[:n]
    es = 1 if u8 else 4
    nbytes = n * H * W * 3 * es
    buf = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    name = "yolo_preprocess_frames_u8" if u8 else "yolo_preprocess_frames"
    _hip.check(getattr(lib, name)(descs, n, frames_ref.LETTERBOX, buf.data_ptr() + GUARD + es, H, W, stream()), name)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD + es] == PATTERN).all() and (got[GUARD + es + nbytes:] == PATTERN).all()
    body = got[GUARD + es:GUARD + es + nbytes]
    if u8:
        assert np.array_equal(body.reshape(n, H, W, 3), want)
    else:
        assert np.array_equal(np.frombuffer(body.tobytes(), dtype=np.uint32).reshape(n, H, W, 3), frames_ref.to_f32(want).view(np.uint32))


def test_boxes_to_frames_equals_the_float64_reference():
    """hand-made records -- the frame's corners and centre and the canvas corners in network coordinates, then seeded random ones --
    for 70 images of cycling sizes, counts from 0 to max_boxes: the valid records equal frames_ref.remap bit for bit, prob, class and
    every record behind the count keep their bits, stretch leaves the whole buffer as it is"""
    import torch
    lib = _hip.lib()
    H, W, K, n = 64, 96, 12, N_FRAMES
    sizes = [(1, 1), (2, 3), (7, 5), (37, 53), (53, 37), (16, 300), (300, 16), (H, W), (576, 768)]
    rng = np.random.default_rng(7)
    descs = (_hip.Frame * n)()
    rec = np.zeros((n, K, 6), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        descs[i] = _hip.Frame(None, h, w, 0, 0)             # (only h and w are read)
        nh, nw, oy, ox = frames_ref.geometry(h, w, H, W, frames_ref.LETTERBOX)
        x0, x1, y0, y1 = ox / W, (ox + nw) / W, oy / H, (oy + nh) / H
        hand = [(x0, y0, nw / W, nh / H), (x1, y1, nw / W, nh / H), (x0, y1, 0., 0.), (x1, y0, 1. / W, 1. / H), ((x0 + x1) / 2, (y0 + y1) / 2, nw / W / 2, nh / H / 2),
                (0., 0., 1., 1.), (1., 1., 1., 1.), (0., 1., .5, .25), (1., 0., .25, .5)]
        rec[i, :len(hand), :4] = np.array(hand, dtype=np.float64).astype(np.float32)
        rec[i, len(hand):, :4] = rng.random((K - len(hand), 4), dtype=np.float32) * 1.5 - 0.25
        rec[i, :, 4] = rng.random(K, dtype=np.float32)
        rec[i, :, 5] = rng.integers(0, 80, size=K).astype(np.int32).view(np.float32)
        counts[i] = (0, K, 1, 9, 5, K - 1)[i % 6]
    assert (counts == 0).any() and (counts == K).any()
    want = rec.copy()
    for i in range(n):
        c = int(counts[i])
        want[i, :c, :4] = frames_ref.remap(rec[i, :c, :4], descs[i].h, descs[i].w, H, W, frames_ref.LETTERBOX)
    # the hand-made records say what they should: the frame's corners land on 0 and 1, its centre on 0.5
    full = [i for i in range(n) if counts[i] >= 5]
    # (to the float32 rounding of the hand-made network coordinates, magnified by net / new: up to 96 * 2^-24)
    assert all(np.allclose(want[i, :2, :2], [[0, 0], [1, 1]], atol=1e-5) and np.allclose(want[i, 0, 2:4], 1, atol=1e-5) for i in full)
    assert all(np.allclose(want[i, 4, :2], 0.5, atol=1e-5) for i in full)
    boxes = torch.from_numpy(rec.copy()).cuda()
    cnt = torch.from_numpy(counts).cuda()
    _hip.check(lib.yolo_boxes_to_frames(boxes.data_ptr(), cnt.data_ptr(), n, K, descs, frames_ref.STRETCH, H, W, stream()), "yolo_boxes_to_frames")
    torch.cuda.synchronize()
    assert np.array_equal(boxes.cpu().numpy().view(np.uint32), rec.view(np.uint32))
    _hip.check(lib.yolo_boxes_to_frames(boxes.data_ptr(), cnt.data_ptr(), n, K, descs, frames_ref.LETTERBOX, H, W, stream()), "yolo_boxes_to_frames")
    torch.cuda.synchronize()
    got = boxes.cpu().numpy()
    bad = [i for i in range(n) if not np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32))]
    assert not bad, bad
    assert np.array_equal(cnt.cpu().numpy(), counts)
    assert not np.array_equal(got.view(np.uint32), rec.view(np.uint32))


# ---- the whole step ---------------------------------------------------------------------------------------------------------------------
STEP_HW = (64, 96)
STEP_SIZES = [(40, 90), (90, 40), (64, 96), (30, 31), (120, 61), (33, 160)]        # wider, taller, the net's, near-square, tall, very wide
THR, IOU = 0.3, 0.6


@functools.lru_cache(maxsize=None)
def step_frames():
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in STEP_SIZES]
    for f in frames:
        f.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def step_weights():
    """synthetic v3-tiny weights whose objectness prior is calibrated on the letterboxed batch: a third of the cells of each anchor pass"""
    H, W = STEP_HW
    hg, _ = synth.HEAD_DEFAULTS["v3-tiny"]
    net = YoloV3Tiny.create_network(np.reshape(spp_ref.TINY_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(H, W, 3))
    w = synth.darknet_stream(net, seed=9, num_classes=80, head_gain=hg, obj_bias=0.0)
    m = build_step_model("fp32", w)
    x = frames_ref.to_f32(np.stack([frames_ref.letterbox_u8(f, H, W) for f in step_frames()]))
    w = synth.calibrate_model(m, x, 0.33)
    w.setflags(write=False)
    return w


def build_step_model(dtype, w):
    m = YoloV3Tiny()
    m.build(spp_ref.TINY_V3_ANCHORS, NAMES80, STEP_HW + (3,), dtype=dtype, max_batch=len(STEP_SIZES), weights=w)
    return m


def host(tensors):
    return [t.cpu().numpy().copy() for t in tensors]


@functools.lru_cache(maxsize=None)
def step_reference(dtype, mode):
    """(records [6, K, 6] with the first count[i] of image i mapped to frame coordinates by NumPy, counts, status) of yolo_net_detect_u8 on
    the batch tests/frames_ref.py builds"""
    H, W = STEP_HW
    m = build_step_model(dtype, step_weights())
    batch = np.stack([frames_ref.resized_u8(f, H, W, mode) for f in step_frames()])
    boxes, counts, status = host(m.net.engine.detect_u8(batch, THR, IOU))
    for i, f in enumerate(step_frames()):
        c = int(counts[i])
        boxes[i, :c, :4] = frames_ref.remap(boxes[i, :c, :4], f.shape[0], f.shape[1], H, W, mode)
    return boxes, counts, status


def same_records(got, want):
    gb, gc, gs = got
    wb, wc, ws = want
    assert np.array_equal(gc, wc) and np.array_equal(gs, ws), (gc, wc, gs, ws)
    for i in range(len(wc)):
        c = int(wc[i])
        assert np.array_equal(gb[i, :c].view(np.uint32), wb[i, :c].view(np.uint32)), i


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_whole_step_equals_detect_u8_on_the_reference_batch_then_the_numpy_map(dtype):
    """yolo_net_detect_frames_u8(letterbox) == yolo_net_detect_u8 on frames_ref.letterbox_u8 of the same frames + the NumPy map: records,
    counts and status bit for bit; stretch == the per-image yolo_preprocess_resize_u8 + yolo_net_detect_u8"""
    import torch
    H, W = STEP_HW
    lib = _hip.lib()
    m = build_step_model(dtype, step_weights())
    eng = m.net.engine
    frames = step_frames()
    want = step_reference(dtype, frames_ref.LETTERBOX)
    print("boxes per image (letterbox, %s): %s, status %s" % (dtype, want[1].tolist(), want[2].tolist()))
    assert int(want[1].sum()) >= 20, "too few boxes for the comparison to mean anything"
    assert (want[2] == 0).all()
    got = host(eng.detect_frames(frames, THR, IOU, _hip.NMS_AGNOSTIC, _hip.RESIZE_LETTERBOX))
    same_records(got, want)
    assert np.array_equal(eng._frames_u8.cpu().numpy(), np.stack([frames_ref.letterbox_u8(f, H, W) for f in frames]))
    # the boxes moved: letterbox is not a no-op on this batch
    plain = host(eng.detect_u8(np.stack([frames_ref.letterbox_u8(f, H, W) for f in frames]), THR, IOU))
    assert not np.array_equal(plain[0].view(np.uint32), got[0].view(np.uint32))
    # stretch: the path the project had -- one resize call per image, then yolo_net_detect_u8
    x = torch.empty((len(frames), H, W, 3), dtype=torch.uint8, device="cuda")
    for i, f in enumerate(frames):
        src = torch.from_numpy(np.array(f)).cuda()
        _hip.check(lib.yolo_preprocess_resize_u8(src.data_ptr(), f.shape[0], f.shape[1], 3 * f.shape[1], x[i].data_ptr(), H, W, 0, stream()), "yolo_preprocess_resize_u8")
    want_s = host(eng.detect_u8(x, THR, IOU))
    assert int(want_s[1].sum()) >= 20 and (want_s[2] == 0).all()
    got_s = host(eng.detect_frames(frames, THR, IOU, _hip.NMS_AGNOSTIC, _hip.RESIZE_STRETCH))
    same_records(got_s, want_s)
    same_records(got_s, step_reference(dtype, frames_ref.STRETCH))
    # frames that already live on the device, one of them a view with a pitch of its own
    wide = torch.zeros((frames[0].shape[0], frames[0].shape[1] + 3, 3), dtype=torch.uint8, device="cuda")
    wide[:, :frames[0].shape[1]] = torch.from_numpy(np.array(frames[0])).cuda()
    on_dev = [wide[:, :frames[0].shape[1]]] + [torch.from_numpy(np.array(f)).cuda() for f in frames[1:3]] + list(frames[3:])
    same_records(host(eng.detect_frames(on_dev, THR, IOU, _hip.NMS_AGNOSTIC, _hip.RESIZE_LETTERBOX)), want)


def tuples(boxes):
    return [[(b.x, b.y, b.w, b.h, b.class_idx, b.prob) for b in img] for img in boxes]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_predict_frames_returns_the_boxes_of_the_step(dtype):
    m = build_step_model(dtype, step_weights())
    for resize, mode in (("letterbox", frames_ref.LETTERBOX), ("stretch", frames_ref.STRETCH)):
        boxes, counts, _ = step_reference(dtype, mode)
        got = tuples(m.predict_frames(step_frames(), THR, IOU, resize=resize))
        want = [[tuple(float(v) for v in boxes[i, k, :4]) + (int(boxes[i, k, 5:6].view(np.int32)[0]), float(boxes[i, k, 4])) for k in range(int(counts[i]))]
                for i in range(len(counts))]
        assert got == want and sum(len(g) for g in got) >= 20
    with pytest.raises(ValueError, match="resize must be stretch or letterbox"):
        m.predict_frames(step_frames(), THR, IOU, resize="crop")
    with pytest.raises(ValueError, match="expected a uint8 array or tensor"):
        m.predict_frames([np.zeros((4, 4, 3), np.float32)], THR, IOU)
    with pytest.raises(ValueError, match="outside 1..6"):
        m.predict_frames(list(step_frames()) + [step_frames()[0]], THR, IOU)


@pytest.mark.parametrize("pipeline, staging", [("True", "u8"), ("True", "f32"), ("False", "f32")])
def test_test_mode_with_resize_letterbox(tmp_path, capsys, pipeline, staging):
    """Yolo.test with `resize = letterbox` on six PNG files of three aspect ratios (lossless: the loop sees the step's frames): one line
    per file with the box counts of the step above, from the pipelined loop (both staging types) and the serial one"""
    from PIL import Image
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    for i, f in enumerate(step_frames()):
        Image.fromarray(np.array(f)).save(str(img_dir / ("f%d.png" % i)))
    wpath = str(tmp_path / "tiny.weights")
    base.write_darknet_weights(wpath, step_weights(), "v3")
    out_dir = tmp_path / "out"
    params = dict(image_dir=str(img_dir), out_dir=str(out_dir), batch_size=6, threshold=THR, iou_threshold=IOU, anchors=list(spp_ref.TINY_V3_ANCHORS),
                  class_names=NAMES80, input_h=STEP_HW[0], input_w=STEP_HW[1], input_c=3, checkpoint_path="", pretrained_weights_path=wpath,
                  cpu_only="False", dtype="fp16", pipeline=pipeline, workers=2, staging=staging, resize="letterbox")
    model = launcher.pick_model("v3-tiny")
    model.test(params)
    text = capsys.readouterr().out
    found = {l.split(":")[0]: int(l.split(": Found ")[1].split(" ")[0]) for l in text.splitlines() if ": Found " in l}
    counts = step_reference("fp16", frames_ref.LETTERBOX)[1]
    assert found == {"f%d" % i: int(counts[i]) for i in range(6)}, (found, counts.tolist())
    assert model.timing["mode"] == ("pipelined" if pipeline == "True" else "serial")
    assert sorted(os.listdir(str(out_dir))) == ["f%d_out.png" % i for i in range(6)]
    # the boxes drawn are the frame-normalised ones: the records of the last batch, as the loop left them on the device
    boxes, cnt, _ = step_reference("fp16", frames_ref.LETTERBOX)
    got = model.net.engine._boxes.cpu().numpy()
    order = [int(os.path.splitext(os.path.basename(p))[0][1:]) for p in base.load_image_paths(str(img_dir))]
    for slot, i in enumerate(order):
        c = int(cnt[i])
        assert np.array_equal(got[slot, :c].view(np.uint32), boxes[i, :c].view(np.uint32)), (slot, i)

"""CPU: the frame entries (batched resize / letterbox / boxes in frame coordinates) as far as they exist without a GPU -- the integer
geometry against tests/frames_ref.py, the argument checks, the `.ini` key, the exports."""
import ctypes as C
import os

import pytest

import frames_ref
from helpers import ROOT, new_graph
from tensorflow_yolo_amd import _hip, launcher
from tensorflow_yolo_amd.net import engine, layers as PL

NETS = [(32, 32), (64, 96), (96, 64)]
FRAME_ENTRIES = ("yolo_letterbox_geometry", "yolo_preprocess_frames", "yolo_preprocess_frames_u8", "yolo_boxes_to_frames",
                 "yolo_net_detect_frames_u8")


def sizes():
    return [(h, w) for h in range(1, 41) for w in range(1, 41)] + [(1, 4000), (4000, 1)]


def test_geometry_equals_the_reference():
    """yolo_letterbox_geometry == frames_ref.geometry for every frame size 1..40 x 1..40 and the two extreme aspect ratios (the max(1, .)
    clamp), three nets, both modes"""
    clamped = 0
    for H, W in NETS:
        for h, w in sizes():
            for mode in (frames_ref.STRETCH, frames_ref.LETTERBOX):
                got = _hip.letterbox_geometry(h, w, H, W, mode)
                assert got == frames_ref.geometry(h, w, H, W, mode), (h, w, H, W, mode, got)
            if (h, w) in ((1, 4000), (4000, 1)):
                new_h, new_w = _hip.letterbox_geometry(h, w, H, W, frames_ref.LETTERBOX)[:2]
                assert min(new_h, new_w) == 1 and (h * W) // w * ((w * H) // h) == 0
                clamped += 1
    assert clamped == 6


def test_geometry_properties():
    """letterbox: the binding side fills its axis, the other does not exceed it, the region lies inside the canvas and the offsets are
    symmetric to within one pixel; the aspect ratio is kept up to the floor.  Stretch: the canvas itself."""
    for H, W in NETS:
        for h, w in sizes():
            assert _hip.letterbox_geometry(h, w, H, W, frames_ref.STRETCH) == (H, W, 0, 0)
            new_h, new_w, oy, ox = _hip.letterbox_geometry(h, w, H, W, frames_ref.LETTERBOX)
            assert 1 <= new_h <= H and 1 <= new_w <= W
            assert new_h == H or new_w == W
            if W * h < H * w:
                assert new_w == W and (new_h == 1 or new_h * w <= h * W < (new_h + 1) * w)
            else:
                assert new_h == H and (new_w == 1 or new_w * h <= w * H < (new_w + 1) * h)
            assert oy >= 0 and ox >= 0 and oy + new_h <= H and ox + new_w <= W
            assert 0 <= (H - new_h - oy) - oy <= 1 and 0 <= (W - new_w - ox) - ox <= 1
    # a frame of the net's aspect ratio fills the canvas, enlarged or reduced
    assert _hip.letterbox_geometry(2, 3, 64, 96, frames_ref.LETTERBOX) == (64, 96, 0, 0)
    assert _hip.letterbox_geometry(640, 960, 64, 96, frames_ref.LETTERBOX) == (64, 96, 0, 0)
    assert _hip.letterbox_geometry(576, 768, 608, 608, frames_ref.LETTERBOX) == (456, 608, 76, 0)


def msg():
    return _hip.lib().yolo_last_error().decode()


def test_bad_arguments_return_err_arg_with_a_message():
    lib = _hip.lib()
    v = [C.c_int32() for _ in range(4)]
    refs = [C.byref(x) for x in v]
    for args in ((0, 4, 8, 8, 1), (4, 0, 8, 8, 1), (4, 4, 0, 8, 0), (4, 4, 8, -1, 1)):
        assert lib.yolo_letterbox_geometry(*(args + tuple(refs))) == 1 and msg() == "yolo_letterbox_geometry: sizes must be at least 1"
    assert lib.yolo_letterbox_geometry(4, 4, 8, 8, 2, *refs) == 1 and "mode must be" in msg()
    assert lib.yolo_letterbox_geometry(4, 4, 8, 8, 1, None, refs[1], refs[2], refs[3]) == 1 and msg() == "yolo_letterbox_geometry: null argument"
    with pytest.raises(_hip.YoloHipError, match="sizes must be at least 1"):
        _hip.letterbox_geometry(0, 1, 8, 8, 1)

    buf = (C.c_uint8 * 4096)()
    ptr = C.addressof(buf)
    good = (_hip.Frame * 2)(_hip.Frame(ptr, 4, 4, 12, 0), _hip.Frame(ptr, 3, 5, 20, 1))
    for name in ("yolo_preprocess_frames_u8", "yolo_preprocess_frames"):
        fn = getattr(lib, name)
        assert fn(None, 2, 0, buf, 8, 8, None) == 1 and msg() == name + ": null argument"
        assert fn(good, 2, 0, None, 8, 8, None) == 1 and msg() == name + ": null argument"
        assert fn(good, 0, 0, buf, 8, 8, None) == 1 and msg() == name + ": frame count must be at least 1"
        assert fn(good, 2, 2, buf, 8, 8, None) == 1 and msg() == name + ": mode must be YOLO_RESIZE_STRETCH or YOLO_RESIZE_LETTERBOX"
        assert fn(good, 2, 1, buf, 0, 8, None) == 1 and msg() == name + ": dst_h and dst_w must be at least 1"
        for bad_w in (6, 9, 30):
            assert fn(good, 2, 1, buf, 8, bad_w, None) == 1 and msg() == name + ": dst_w must be a multiple of 4"
        for bad, text in ((_hip.Frame(ptr, 0, 4, 12, 0), "frame 1 has h or w below 1"), (_hip.Frame(ptr, 4, -1, 12, 0), "frame 1 has h or w below 1"),
                          (_hip.Frame(None, 4, 4, 12, 0), "frame 1 has no pixels"), (_hip.Frame(ptr, 4, 4, 11, 0), "frame 1 has row_bytes below 3 * w")):
            arr = (_hip.Frame * 2)(good[0], bad)
            assert fn(arr, 2, 1, buf, 8, 8, None) == 1 and msg() == name + ": " + text
    name = "yolo_boxes_to_frames"
    assert lib.yolo_boxes_to_frames(None, buf, 2, 8, good, 1, 8, 8, None) == 1 and msg() == name + ": null argument"
    assert lib.yolo_boxes_to_frames(buf, None, 2, 8, good, 1, 8, 8, None) == 1 and msg() == name + ": null argument"
    assert lib.yolo_boxes_to_frames(buf, buf, 2, 8, None, 1, 8, 8, None) == 1 and msg() == name + ": null argument"
    assert lib.yolo_boxes_to_frames(buf, buf, 0, 8, good, 1, 8, 8, None) == 1 and msg() == name + ": frame count must be at least 1"
    assert lib.yolo_boxes_to_frames(buf, buf, 2, 0, good, 1, 8, 8, None) == 1 and "must be at least 1" in msg()
    assert lib.yolo_boxes_to_frames(buf, buf, 2, 8, good, 3, 8, 8, None) == 1 and "mode must be" in msg()
    # stretch: a no-op that launches nothing -- it succeeds without a device (host memory stands in for the record buffer, untouched)
    before = bytes(buf)
    assert lib.yolo_boxes_to_frames(buf, buf, 2, 8, good, 0, 8, 8, None) == 0 and bytes(buf) == before

    # the whole step: the checks of yolo_net_detect_u8 under the new entry's name, then the frames'
    g = new_graph(8, 8, 3)
    g.append(PL.conv2d_bn_act(g[-1].out, 16, 3, 1))
    p = engine.Plan(g, dtype="fp16", max_batch=2)
    name = "yolo_net_detect_frames_u8"
    call = lambda frames, b, dev=buf: lib.yolo_net_detect_frames_u8(p.handle, frames, b, 1, dev, 0.5, 0.5, 0, buf, buf, buf, None)
    assert call(None, 1) == 1 and msg() == name + ": null argument"
    assert call(good, 1, None) == 1 and msg() == name + ": null argument"
    for bad in (0, 3, -1):
        assert call(good, bad) == 1 and msg() == name + ": batch outside 1..max_batch"
    assert call(good, 1) == 5 and msg() == name + ": weights not loaded"
    g2 = new_graph(8, 8, 16)                    # (no weights to load: the call reaches the workspace check)
    g2.append(PL.max_pool2d(g2[-1].out, 2, 2))
    p2 = engine.Plan(g2, dtype="fp16", max_batch=2)
    assert lib.yolo_net_detect_frames_u8(p2.handle, good, 1, 1, buf, 0.5, 0.5, 0, buf, buf, buf, None) == 5 and msg() == name + ": workspace not bound"


def test_ini_key_resize_parses_and_rejects(tmp_path):
    assert _hip.resize_mode("stretch") == _hip.RESIZE_STRETCH == 0 and _hip.resize_mode("letterbox") == _hip.RESIZE_LETTERBOX == 1
    assert _hip.resize_mode(" Letterbox ") == 1
    for bad in ("pad", "", "0", None):
        with pytest.raises(ValueError, match="resize must be stretch or letterbox"):
            _hip.resize_mode(bad)
    text = open(os.path.join(ROOT, "tensorflow-yolo_amd", "config", "yolo_3.ini")).read()
    assert "; resize = letterbox\n" in text
    assert "resize" not in launcher.read_config(os.path.join(ROOT, "tensorflow-yolo_amd", "config", "yolo_3.ini"))["TEST"]      # commented: the default holds
    for value, want in (("letterbox", 1), ("stretch", 0), (None, 0)):
        ini = tmp_path / ("r_%s.ini" % value)
        ini.write_text(text.replace("; resize = letterbox\n", "resize = %s\n" % value if value else ""))
        cfg = launcher.read_config(str(ini))
        params = dict(cfg["TEST"])
        params.update(cfg["COMMON"])
        assert launcher.test_options(params) == {"resize": want}
    ini = tmp_path / "bad.ini"
    ini.write_text(text.replace("; resize = letterbox\n", "resize = crop\n"))
    with pytest.raises(ValueError, match="resize must be stretch or letterbox, got 'crop'"):
        launcher.run(launcher.read_config(str(ini)), "test")          # rejected before a network is built: no GPU needed


def test_abi_is_still_7_and_the_frame_symbols_resolve():
    assert _hip.ABI_VERSION == 7 and _hip.lib().yolo_hip_abi_version() == 7
    raw = C.CDLL(_hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    for name in FRAME_ENTRIES:
        assert hasattr(raw, name) and name in _hip.SIGNATURES and ("int %s(" % name) in header, name
    assert "#define YOLO_HIP_ABI_VERSION 7" in header and "typedef struct yolo_frame {" in header
    assert C.sizeof(_hip.Frame) == 24 and _hip.Frame.pixels_dev.offset == 0 and _hip.Frame.h.offset == 8 and _hip.Frame.swap_rb.offset == 20
    assert _hip.FRAMES_PER_LAUNCH == 64

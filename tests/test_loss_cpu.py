"""CPU: the loss yardstick (tests/loss_ref.py) -- its two restatements against each other --, the host-side argument checks of the
yolo_v2_loss / yolo_net_loss* / yolo_loss_reduce entries, the `loss` key of `--mode eval`, and the padding formula of the validation
loss.  No device call is made."""
import ctypes as C
import os

import numpy as np
import pytest

import loss_ref
from tensorflow_yolo_amd import _hip, launcher
from tensorflow_yolo_amd.net import engine, evaluate as yeval, v2, v3

ANCHORS5 = [1.0, 1.0, 0.5, 2.0, 2.0, 0.5, 3.0, 3.0, 0.25, 0.25]


def last_error():
    return (_hip.lib().yolo_last_error() or b"").decode()


# ---- the two restatements ------------------------------------------------------------------------------------------------------------
def square_case():
    """input 128 x 128 -> a 4 x 4 grid (1 cell = 32 pixels); even integer corners: centre and size are exact in both routes"""
    objects = [[(10, 20, 50, 60, 1), (34, 2, 62, 30, 0), (36, 4, 60, 28, 2), (96, 96, 128, 112, 1)],        # two truths in cell (0, 1)
               [],
               [(0, 0, 64, 64, 2), (2, 66, 30, 126, 0), (2, 66, 30, 126, 1)]]                               # two identical truths: the first wins
    rng = np.random.RandomState(5)
    logits = rng.uniform(-3, 3, size=(3, 4, 4, 5 * (5 + 3))).astype(np.float32)
    return objects, logits


def test_restatements_agree_on_a_square_grid():
    objects, logits = square_case()
    gt, counts = loss_ref.objects_to_gts(objects, (128, 128), 4)
    mine = loss_ref.loss(logits, 4, 4, ANCHORS5, 3, gt, counts, mode="float64")
    lit = loss_ref.literal_loss(logits, objects, (128, 128), ANCHORS5, 3, T=np.float64)
    # the same assignment ...
    want = np.full((3, 4, 4), -1, dtype=np.int32)
    for b, winners in enumerate(lit["winners"]):
        for (cy, cx), (index, a) in winners.items():
            want[b, cy, cx] = index * 8 + a
    assert np.array_equal(mine["table"], want)
    assert want[0, 0, 1] >> 3 in (1, 2) and want[2, 3, 0] >> 3 == 1 and (want >= 0).sum() == 5
    assert mine["status"] == 0 and mine["n_truths"] == 7
    # ... and the same float64 terms: per image, the literal's dense arrays hold exactly the values the sequential route adds up
    for b in range(3):
        for k in loss_ref.TERMS:
            dense = float(np.sum(lit[k][b].astype(np.float64)))
            assert abs(dense - mine["images"][b][k]) <= 1e-12 * max(1.0, abs(dense)), (b, k)
    for k in ("loss", "loss_xy", "loss_wh", "loss_obj", "loss_noobj", "loss_class"):
        assert abs(lit[k] - mine[k]) <= 1e-12 * max(1.0, abs(lit[k])), k
    # a winner slot's terms bit for bit (one slot, no summation order in the way)
    b, (cy, cx) = 0, (0, 1)
    a = want[b, cy, cx] & 7
    one = loss_ref.loss(logits[:1], 4, 4, ANCHORS5, 3, gt[:1, 1:3], np.asarray([2], dtype=np.int32), mode="float64")
    assert one["images"][0]["xy"] == float(lit["xy"][b, cy, cx, a]) and one["images"][0]["wh"] == float(lit["wh"][b, cy, cx, a])
    assert one["images"][0]["obj"] == float(lit["obj"][b, cy, cx, a])


def test_literal_offsets_differ_on_a_non_square_grid():
    """deliberate difference (a): the reference's offset tensor is (k % h, k // h) at k = r * w + c -- (c, r) only where h == w"""
    sq = loss_ref.literal_offsets(4, 4)
    assert all(tuple(sq[r, c]) == (c, r) for r in range(4) for c in range(4))
    off = loss_ref.literal_offsets(3, 5)
    differ = [(r, c) for r in range(3) for c in range(5) if tuple(off[r, c]) != (c, r)]
    assert tuple(off[0, 3]) == (0, 1) and tuple(off[2, 4]) == (2, 4) and tuple(off[1, 0]) == (2, 1)
    assert len(differ) == 12 and all((0, c) not in differ for c in range(3)) and (2, 4) in differ
    # so on a 3 x 5 grid the literal route puts a centred prediction of cell (r=0, c=3) at x = 0.5, not 3.5: the xy term differs
    objects = [[(96 + 4, 4, 96 + 28, 28, 0)]]                  # input 96 x 160 -> 3 x 5 cells of 32: the centre of cell (0, 3)
    logits = np.zeros((1, 3, 5, 2 * 6), dtype=np.float32)
    gt, counts = loss_ref.objects_to_gts(objects, (96, 160), 1)
    mine = loss_ref.loss(logits, 3, 5, [1, 1, 2, 2], 1, gt, counts)
    lit = loss_ref.literal_loss(logits, objects, (96, 160), [1, 1, 2, 2], 1)
    assert mine["table"][0, 0, 3] >= 0 and mine["loss_xy"] == 0.0 and lit["loss_xy"] == 3.0 ** 2 + 1.0 ** 2


# ---- C ABI: host-side checks, before any device call ---------------------------------------------------------------------------------
def head(version=2, n_scales=1, h=13, w=13, a=5, c=20):
    hd = engine.head_desc_v2(h, w, ANCHORS5[:2 * a], c)
    hd.version, hd.n_scales = version, n_scales
    for s in range(1, n_scales):
        hd.h[s], hd.w[s], hd.n_anchors[s] = h, w, a
    return hd


def test_struct_sizes():
    assert C.sizeof(_hip.LossImage) == 56 == yeval.LOSS_IMAGE_DTYPE.itemsize
    assert C.sizeof(_hip.LossResult) == 64 == yeval.LOSS_RESULT_DTYPE.itemsize
    assert [n for n, _ in _hip.LossImage._fields_] == list(yeval.LOSS_IMAGE_DTYPE.names)
    assert [n for n, _ in _hip.LossResult._fields_] == list(yeval.LOSS_RESULT_DTYPE.names)


def test_v2_loss_refuses_bad_arguments():
    lib = _hip.lib()
    P = 4096            # a non-null pointer that is never used: the checks come first
    ok = head()
    call = lambda hd=ok, logits=P, batch=1, gt=P, gc=P, max_gt=8, images=P, assign=None, result=P: lib.yolo_v2_loss(
        C.byref(hd) if hd is not None else None, logits, batch, gt, gc, max_gt, images, assign, result, None)
    for kw in (dict(hd=None), dict(logits=None), dict(gt=None), dict(gc=None), dict(images=None), dict(result=None)):
        assert call(**kw) == 1 and "yolo_v2_loss: null argument" in last_error(), kw
    assert call(hd=head(version=3)) == 1 and "the reference has a loss for YOLOv2 only" in last_error()
    assert call(hd=head(n_scales=2)) == 1 and "yolo_v2_loss: the head must be version 2 with one scale" in last_error()
    for m in (0, 1025):
        assert call(max_gt=m) == 1 and "yolo_v2_loss: max_gt must be 1..1024" in last_error()
    assert call(batch=0) == 1 and "yolo_v2_loss: batch must be at least 1" in last_error()
    assert call(hd=head(h=65, w=65)) == 1 and "yolo_v2_loss: h * w must be at most 4096" in last_error()
    assert call(hd=head(a=0)) == 1 and "yolo_v2_loss: bad head scale" in last_error()


def test_net_loss_and_reduce_refuse_bad_arguments():
    lib = _hip.lib()
    P = 4096
    for name in ("yolo_net_loss", "yolo_net_loss_u8"):
        fn = getattr(lib, name)
        assert fn(None, P, 1, P, P, 8, P, None, P, None) == 1 and name + ": null argument" in last_error()
    names = ["c%d" % i for i in range(3)]
    tiny3 = engine.Plan(v3.create_tiny_network(np.reshape([10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319], [-1, 2]), names, False,
                                               input_shape=(96, 160, 3)), dtype="fp16", max_batch=2)      # (a v3 plan sets its own head)
    assert lib.yolo_net_loss(tiny3.handle, P, 1, P, P, 8, P, None, P, None) == 1 and "the reference has a loss for YOLOv2 only" in last_error()
    anchors = np.reshape(ANCHORS5, [-1, 2])
    tiny2 = engine.Plan(v2.create_tiny_network(anchors, names, False, input_shape=(96, 160, 3)), dtype="fp16", max_batch=2)
    # no head set yet: that is what the message says, whatever the (zeroed) head's version
    assert lib.yolo_net_loss(tiny2.handle, P, 1, P, P, 8, P, None, P, None) == 5 and "yolo_net_loss: head geometry not set" in last_error()
    assert "call yolo_net_set_head" in last_error()
    tiny2.set_head(engine.head_desc_v2(3, 5, anchors, 3))
    for k in (3, 4, 6, 8):
        args = [tiny2.handle, P, 1, P, P, 8, P, None, P, None]
        args[k] = None
        assert lib.yolo_net_loss_u8(*args) == 1 and "yolo_net_loss_u8: null argument" in last_error(), k
    assert lib.yolo_net_loss(tiny2.handle, None, 1, P, P, 8, P, None, P, None) == 1 and "yolo_net_loss: null argument" in last_error()
    assert lib.yolo_net_loss(tiny2.handle, P, 1, P, P, 0, P, None, P, None) == 1 and "yolo_net_loss: max_gt must be 1..1024" in last_error()
    assert lib.yolo_net_loss(tiny2.handle, P, 0, P, P, 8, P, None, P, None) == 1 and "yolo_net_loss: batch must be at least 1" in last_error()
    assert lib.yolo_net_loss(tiny2.handle, P, 3, P, P, 8, P, None, P, None) == 1 and "batch outside 1..max_batch" in last_error()
    assert lib.yolo_net_loss(tiny2.handle, P, 1, P, P, 8, P, None, P, None) == 5 and "weights not loaded" in last_error()
    assert lib.yolo_loss_reduce(None, 1, 0, 1, P, None) == 1 and "yolo_loss_reduce: null argument" in last_error()
    assert lib.yolo_loss_reduce(P, 0, 0, 1, P, None) == 1 and "n_images and batch_size must be at least 1" in last_error()
    assert lib.yolo_loss_reduce(P, 4, 0, 0, P, None) == 1 and "n_images and batch_size must be at least 1" in last_error()
    assert lib.yolo_loss_reduce(P, 4, 5, 4, P, None) == 1 and "n_repeat must be 0..n_images" in last_error()
    assert lib.yolo_loss_reduce(P, 4, -1, 4, P, None) == 1 and "n_repeat must be 0..n_images" in last_error()


# ---- launcher -------------------------------------------------------------------------------------------------------------------------
INI = """[COMMON]
version = %s
input_h = 96
input_w = 160
input_c = 3
[TEST]
image_dir = img/
out_dir = out/
batch_size = 4
threshold = 0.5
iou_threshold = 0.6
anchors = [1, 1, 2, 2]
class_names = ["a", "b"]
pretrained_weights_path = w.weights
[EVAL]
annotation_dir = ann/
image_dir = val/
%s
"""


def params_of(tmp_path, version, tail):
    p = tmp_path / "cfg.ini"
    p.write_text(INI % (version, tail))
    return launcher.eval_params(launcher.read_config(str(p)))


def test_loss_key_is_parsed(tmp_path):
    p = params_of(tmp_path, "v2-tiny", "loss = true\n")
    assert p["loss"] == "true" and launcher.eval_options(p) == {"resize": _hip.RESIZE_STRETCH, "loss": True}
    assert launcher.eval_options(params_of(tmp_path, "v2", "loss = True\nresize = stretch\n"))["loss"] is True
    assert launcher.eval_options(params_of(tmp_path, "v2", "loss = false\nresize = letterbox\n")) == {"resize": _hip.RESIZE_LETTERBOX, "loss": False}
    with pytest.raises(ValueError, match="loss must be true or false"):
        launcher.eval_options(params_of(tmp_path, "v2", "loss = maybe\n"))


def test_loss_key_absent_changes_nothing(tmp_path):
    p = params_of(tmp_path, "v3-tiny", "")
    assert "loss" not in p and launcher.test_options(p) == {"resize": _hip.RESIZE_STRETCH}
    assert launcher.eval_options(p) == {"resize": _hip.RESIZE_STRETCH, "loss": False}
    assert sorted(p) == sorted(["version", "input_h", "input_w", "input_c", "image_dir", "out_dir", "batch_size", "threshold", "iou_threshold",
                                "anchors", "class_names", "pretrained_weights_path", "annotation_dir", "max_boxes", "match_iou"])
    assert (p["threshold"], p["max_boxes"], p["match_iou"], p["batch_size"]) == ("0.005", "1024", "0.5", "4")


def test_loss_refuses_letterbox_and_v3(tmp_path):
    with pytest.raises(ValueError, match="loss = true needs resize = stretch"):
        launcher.eval_options(params_of(tmp_path, "v2", "loss = true\nresize = letterbox\n"))
    for version in ("v3", "v3-tiny", "v3-spp"):
        with pytest.raises(ValueError, match="loss = true needs a YOLOv2 network"):
            launcher.eval_options(params_of(tmp_path, version, "loss = true\n"))
    from tensorflow_yolo_amd.net.yolo import YoloV3Tiny, YoloV2Tiny        # Yolo.evaluate makes the same checks before it builds anything
    with pytest.raises(ValueError, match="loss = true needs a YOLOv2 network"):
        YoloV3Tiny().evaluate(params_of(tmp_path, "v3-tiny", "loss = true\n"))
    with pytest.raises(ValueError, match="loss = true needs resize = stretch"):
        YoloV2Tiny().evaluate(params_of(tmp_path, "v2-tiny", "loss = true\nresize = letterbox\n"))


def test_shipped_configs_say_how_to_ask_for_the_loss():
    cfg_dir = os.path.join(os.path.dirname(os.path.abspath(launcher.__file__)), "config")
    for name in ("yolo_2.ini", "yolov2_tiny_voc.ini"):
        text = open(os.path.join(cfg_dir, name)).read()
        assert "loss = true" in text[text.index("[EVAL]"):], name
        assert launcher.eval_options(launcher.eval_params(launcher.read_config(os.path.join(cfg_dir, name))))["loss"] is False      # off by default


# ---- the validation loss from per-image partials ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 8])
def test_padding_formula_equals_batch_by_batch_averaging(n):
    """net/v2.py:209-217 + net/yolo.py:177-193: wrap the list, average the batch losses"""
    batch_size = 4
    rng = np.random.RandomState(n)
    partials = np.zeros(n, dtype=yeval.LOSS_IMAGE_DTYPE)
    for k in loss_ref.TERMS:
        partials[k] = rng.uniform(0, 10, size=n)
    bs = min(batch_size, n)                                 # v2.py:212-213
    wrapped = list(partials)
    if n % bs:
        wrapped.extend(wrapped[0:bs - n % bs])              # v2.py:216-217
    total_batches = int(np.ceil(n / bs))
    assert yeval.loss_batches(n, batch_size) == (bs, total_batches, len(wrapped) - n)
    val_total, comp = 0.0, dict.fromkeys(yeval.LOSS_KEYS[1:], 0.0)
    for i in range(total_batches):
        one = loss_ref.totals(wrapped[i * bs:(i + 1) * bs], bs)
        val_total += one["loss"]
        for k in comp:
            comp[k] += one[k]
    got = yeval.validation_loss(partials, batch_size)
    assert abs(got["loss"] - val_total / total_batches) <= 1e-13 * val_total
    for k in comp:
        assert abs(got[k] - comp[k] / total_batches) <= 1e-13 * max(1.0, comp[k]), k
    # ... and yolo_loss_reduce's arithmetic (loss_ref.totals with `repeat`) divided by the number of batches is the same number
    red = loss_ref.totals(partials, bs, repeat=len(wrapped) - n)
    assert abs(red["loss"] / total_batches - got["loss"]) <= 1e-13 * val_total

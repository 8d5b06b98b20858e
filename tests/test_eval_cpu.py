"""CPU: the evaluation yardstick (tests/eval_ref.py) on hand-computed cases, the VOC annotation reader, the host-side argument checks
of every yolo_eval_* entry, and `--mode eval` config handling.  No device call is made."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import eval_ref
from helpers import ROOT
from tensorflow_yolo_amd import _hip, launcher
from tensorflow_yolo_amd.net import evaluate as yeval

GOLDEN = os.path.join(ROOT, "tests", "golden", "eval")
FP, TP, IGNORED = eval_ref.FP, eval_ref.TP, eval_ref.IGNORED


def box(i, w=0.05, h=0.05):
    """disjoint boxes on a grid"""
    return (0.1 + 0.1 * (i % 8), 0.1 + 0.1 * (i // 8), w, h)


def test_ten_detections_known_ap():
    # 5 truths, 10 detections of falling prob: TP TP FP TP FP FP TP FP FP FP (a far-away box is an FP)
    gts = [[box(i) + (0, 0) for i in range(5)]]
    pattern = [0, 1, None, 2, None, None, 3, None, None, None]
    dets = [[(box(t) if t is not None else box(40 + k)) + (1.0 - k / 16., 0) for k, t in enumerate(pattern)]]
    r = eval_ref.evaluate(dets, gts, 1)
    assert r["records"]["verdict"].tolist() == [TP, TP, FP, TP, FP, FP, TP, FP, FP, FP]
    assert r["ctp"].tolist() == [1, 2, 2, 3, 3, 3, 4, 4, 4, 4] and r["cfp"].tolist() == [0, 0, 1, 1, 2, 3, 3, 4, 5, 6]
    # envelope at the TPs: 1, 1, 3/4, 4/7 -> AP12 = (1 + 1 + 3/4 + 4/7) / 5; AP07 = (5 * 1 + 2 * 3/4 + 2 * 4/7) / 11
    assert abs(r["ap_voc12"][0] - float(Fraction(93, 140))) <= 4 * 2.0 ** -52
    assert abs(r["ap_voc07"][0] - float(Fraction(107, 154))) <= 11 * 2.0 ** -52
    assert r["map_voc12"] == r["ap_voc12"][0] and r["n_gt"].tolist() == [5]
    assert (r["tp"][0], r["fp"][0], r["ignored"][0], r["n_det"][0]) == (4, 6, 0, 10)


def test_difficult_truth_is_ignored_not_taken_not_counted():
    gts = [[box(0) + (0, 1), box(1) + (0, 0)]]
    dets = [[box(0) + (0.9, 0), box(0) + (0.8, 0), box(1) + (0.7, 0)]]
    r = eval_ref.evaluate(dets, gts, 1)
    assert r["records"]["verdict"].tolist() == [IGNORED, IGNORED, TP]
    assert r["n_gt"].tolist() == [1] and r["ctp"].tolist() == [0, 0, 1] and r["cfp"].tolist() == [0, 0, 0]
    assert r["ap_voc12"][0] == 1.0 and abs(r["ap_voc07"][0] - 1.0) <= 11 * 2.0 ** -52


def test_double_claim_second_is_fp_across_images_by_global_order():
    gts = [[box(0) + (0, 0)], [box(0) + (0, 0)]]
    dets = [[box(0) + (0.5, 0), box(0) + (0.25, 0)], [box(0) + (0.75, 0)]]
    r = eval_ref.evaluate(dets, gts, 1, max_boxes=4)
    assert r["records"]["seq"].tolist() == [4, 0, 1]                 # prob order: image 1's detection first
    assert r["records"]["verdict"].tolist() == [TP, TP, FP]
    assert r["records"]["best_gt"].tolist() == [0, 0, 0] and np.all(r["records"]["best_iou"] == 1.0)
    assert r["ap_voc12"][0] == 1.0


def test_iou_exactly_at_the_threshold_is_not_a_match():
    gts = [[(0.5, 0.5, 0.5, 0.5, 0, 0)]]
    dets = [[(0.5, 0.5, 0.25, 0.5, 0.9, 0)]]                       # inside the truth, half its area
    r = eval_ref.evaluate(dets, gts, 1, match_iou=0.5)
    assert r["records"]["best_iou"][0] == 0.5 and r["records"]["verdict"][0] == FP and r["ap_voc12"][0] == 0.0
    r = eval_ref.evaluate(dets, gts, 1, match_iou=float(np.nextafter(0.5, 0)))
    assert r["records"]["verdict"][0] == TP and r["ap_voc12"][0] == 1.0


def test_class_without_truths_is_nan_and_left_out():
    gts = [[box(0) + (0, 0)]]
    dets = [[box(0) + (0.9, 0), box(0) + (0.8, 1), box(3) + (0.7, 5)]]      # class 5 is out of range: skipped
    r = eval_ref.evaluate(dets, gts, 3)
    assert r["records"]["class_idx"].tolist() == [0, 1] and r["records"]["best_gt"].tolist() == [0, -1]
    assert math.isnan(r["ap_voc12"][1]) and math.isnan(r["ap_voc07"][2]) and r["fp"].tolist() == [0, 1, 0]
    assert r["map_voc12"] == 1.0
    assert math.isnan(eval_ref.evaluate([[]], [[]], 2)["map_voc12"])


def test_iou_follows_numpy_on_degenerate_boxes():
    assert eval_ref.iou((0.5, 0.5, 0., 0.), (0.5, 0.5, 0., 0.)) == 0.0          # union floored at 1e-8
    assert 0.009 < eval_ref.iou((0.5, 0.5, 1e-5, 1e-5), (0.5, 0.5, 1e-5, 1e-5)) < 0.011      # 1e-10 / 1e-8, not 1
    assert math.isnan(eval_ref.iou((0.5, 0.5, np.inf, 0.), (0.5, 0.5, 0.2, 0.2)))


# ---- annotations ------------------------------------------------------------------------------------------------------------------
def test_parse_voc_annotations_eiffel():
    ann, skipped = yeval.parse_voc_annotations(os.path.join(GOLDEN, "eiffel"), "/img", ["tower"])
    assert [os.path.basename(p) for p, _ in ann] == ["tower11.jpg", "tower12.jpg", "tower13.jpg"] and skipped == {}
    assert ann[0][0] == os.path.join("/img", "tower11.jpg")
    assert ann[0][1] == [((222 + 412) / 2. / 640, (101 + 587) / 2. / 800, (412 - 222) / 640., (587 - 101) / 800., 0, 0)]
    assert all(len(t) == 1 and t[0][4] == 0 for _, t in ann)
    none, skipped = yeval.parse_voc_annotations(os.path.join(GOLDEN, "eiffel"), "/img", ["dog"])
    assert skipped == {"tower": 3} and all(t == [] for _, t in none)


def test_parse_voc_annotations_dog_difficult_and_unknown_names():
    ann, skipped = yeval.parse_voc_annotations(os.path.join(GOLDEN, "dog"), os.path.join(ROOT, "tests", "golden"), ["bicycle", "car", "dog"])
    assert len(ann) == 1 and os.path.exists(ann[0][0]) and skipped == {"tree": 1}
    truths = ann[0][1]
    assert [(t[4], t[5]) for t in truths] == [(2, 0), (0, 0), (1, 1)]
    assert truths[0][:4] == ((128 + 314) / 2. / 768, (224 + 537) / 2. / 576, (314 - 128) / 768., (537 - 224) / 576.)
    arr, counts = yeval.pack_gts([truths], 4)
    assert arr.dtype.itemsize == C.sizeof(_hip.Gt) == 24 and counts.tolist() == [3] and arr[0, 2]["difficult"] == 1
    with pytest.raises(ValueError):
        yeval.pack_gts([truths], 2)


# ---- C ABI: host-side checks, before any device call ---------------------------------------------------------------------------------
def desc(n_classes=20, det_capacity=1024, max_gt=64, match_iou=0.5):
    return _hip.EvalDesc(n_classes, det_capacity, max_gt, 0, match_iou)


def last_error():
    return (_hip.lib().yolo_last_error() or b"").decode()


def test_struct_sizes_and_state_layout():
    assert C.sizeof(_hip.EvalDesc) == 24 and C.sizeof(_hip.EvalRecord) == 32 == yeval.RECORD_DTYPE.itemsize
    assert C.sizeof(_hip.EvalClass) == 40 == yeval.CLASS_DTYPE.itemsize and C.sizeof(_hip.EvalResultHeader) == 32 == yeval.HEADER_DTYPE.itemsize
    lib = _hip.lib()
    d = desc()
    lay = _hip.EvalLayout()
    assert lib.yolo_eval_state_layout(C.byref(d), C.byref(lay)) == 0
    assert lay.total_bytes == lib.yolo_eval_state_bytes(C.byref(d))
    assert lay.n_gt_offset >= 256 and lay.records_offset >= lay.n_gt_offset + 4 * 20
    assert lay.sorted_offset >= lay.records_offset + 32 * 1024 and lay.ctp_offset >= lay.sorted_offset + 32 * 1024
    assert lay.cfp_offset >= lay.ctp_offset + 4 * 1024 and lay.total_bytes >= lay.cfp_offset + 4 * 1024
    assert lib.yolo_eval_result_bytes(C.byref(d)) == 32 + 40 * 20
    big = desc(det_capacity=1 << 20)
    assert lib.yolo_eval_state_bytes(C.byref(big)) >= (1 << 20) * (32 + 32 + 4 + 4)


BAD_DESCS = [(dict(n_classes=0), "n_classes must be"), (dict(n_classes=65537), "n_classes must be"),
             (dict(det_capacity=0), "det_capacity must be"), (dict(det_capacity=(1 << 20) + 1), "det_capacity must be"),
             (dict(max_gt=0), "max_gt must be"), (dict(max_gt=1025), "max_gt must be"),
             (dict(match_iou=-0.01), "match_iou must be in [0, 1]"), (dict(match_iou=1.5), "match_iou must be in [0, 1]"),
             (dict(match_iou=float("nan")), "match_iou must be in [0, 1]")]


@pytest.mark.parametrize("kw,msg", BAD_DESCS)
def test_every_eval_entry_refuses_a_bad_descriptor(kw, msg):
    lib = _hip.lib()
    d = desc(**kw)
    P = 4096            # a non-null pointer that is never used: the checks come first
    lay = _hip.EvalLayout()
    assert lib.yolo_eval_state_bytes(C.byref(d)) == 0 and "yolo_eval_state_bytes: " + msg in last_error()
    assert lib.yolo_eval_result_bytes(C.byref(d)) == 0 and "yolo_eval_result_bytes: " + msg in last_error()
    assert lib.yolo_eval_state_layout(C.byref(d), C.byref(lay)) == 1 and "yolo_eval_state_layout: " + msg in last_error()
    assert lib.yolo_eval_reset(C.byref(d), P, 1 << 30, None) == 1 and "yolo_eval_reset: " + msg in last_error()
    assert lib.yolo_eval_add(C.byref(d), P, P, P, 1, 16, P, P, 0, None) == 1 and "yolo_eval_add: " + msg in last_error()
    assert lib.yolo_eval_finish(C.byref(d), P, P, None) == 1 and "yolo_eval_finish: " + msg in last_error()


def test_eval_entries_refuse_null_small_state_and_seq_overflow():
    lib = _hip.lib()
    d = desc()
    P = 4096
    need = lib.yolo_eval_state_bytes(C.byref(d))
    assert lib.yolo_eval_state_bytes(None) == 0 and "null argument" in last_error()
    assert lib.yolo_eval_state_layout(C.byref(d), None) == 1 and "yolo_eval_state_layout: null argument" in last_error()
    assert lib.yolo_eval_reset(None, P, need, None) == 1 and "yolo_eval_reset: null argument" in last_error()
    assert lib.yolo_eval_reset(C.byref(d), None, need, None) == 1 and "yolo_eval_reset: null argument" in last_error()
    assert lib.yolo_eval_reset(C.byref(d), P, need - 1, None) == 1 and "yolo_eval_reset: state too small" in last_error()
    for k in range(5):
        ptrs = [P] * 5
        ptrs[k] = None
        assert lib.yolo_eval_add(C.byref(d), ptrs[0], ptrs[1], ptrs[2], 1, 16, ptrs[3], ptrs[4], 0, None) == 1
        assert "yolo_eval_add: null argument" in last_error()
    assert lib.yolo_eval_add(C.byref(d), P, P, P, 0, 16, P, P, 0, None) == 1 and "batch and max_boxes must be at least 1" in last_error()
    assert lib.yolo_eval_add(C.byref(d), P, P, P, 1, 0, P, P, 0, None) == 1 and "batch and max_boxes must be at least 1" in last_error()
    assert lib.yolo_eval_add(C.byref(d), P, P, P, 1, 16, P, P, -1, None) == 1 and "image_base must not be negative" in last_error()
    # seq = image * max_boxes + rank is a uint32: (image_base + batch) * max_boxes may reach 2^32 and not pass it
    assert lib.yolo_eval_add(C.byref(d), P, P, P, 32, 1024, P, P, (1 << 22) - 31, None) == 1 and "does not fit 32 bits" in last_error()
    assert lib.yolo_eval_add(C.byref(d), P, P, P, 1, 1024, P, P, 1 << 40, None) == 1 and "does not fit 32 bits" in last_error()
    assert lib.yolo_eval_finish(C.byref(d), None, P, None) == 1 and "yolo_eval_finish: null argument" in last_error()
    assert lib.yolo_eval_finish(C.byref(d), P, None, None) == 1 and "yolo_eval_finish: null argument" in last_error()


# ---- launcher -------------------------------------------------------------------------------------------------------------------------
INI = """[COMMON]
version = v3-tiny
input_h = 96
input_w = 160
input_c = 3
[TEST]
image_dir = img/
out_dir = out/
batch_size = 4
threshold = 0.5
iou_threshold = 0.6
anchors = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
class_names = ["a", "b"]
pretrained_weights_path = w.weights
%s
"""


def write_ini(tmp_path, tail):
    p = tmp_path / "cfg.ini"
    p.write_text(INI % tail)
    return str(p)


def test_eval_params_merge_and_defaults(tmp_path):
    cfg = launcher.read_config(write_ini(tmp_path, "[EVAL]\nannotation_dir = ann/\nimage_dir = val/\n"))
    p = launcher.eval_params(cfg)
    assert p["annotation_dir"] == os.path.join(str(tmp_path), "ann/") and p["image_dir"] == os.path.join(str(tmp_path), "val/")
    assert (p["threshold"], p["max_boxes"], p["match_iou"]) == ("0.005", "1024", "0.5")       # not [TEST]'s demo threshold
    assert p["iou_threshold"] == "0.6" and p["class_names"] == ["a", "b"] and p["version"] == "v3-tiny" and p["batch_size"] == "4"
    cfg = launcher.read_config(write_ini(tmp_path, "[EVAL]\nannotation_dir = ann/\nimage_dir = val/\nthreshold = 0.1\nmax_boxes = 64\n"
                                                   "match_iou = 0.75\nresize = letterbox\n"))
    p = launcher.eval_params(cfg)
    assert (p["threshold"], p["max_boxes"], p["match_iou"], p["resize"]) == ("0.1", "64", "0.75", "letterbox")
    assert launcher.test_options(p) == {"resize": _hip.RESIZE_LETTERBOX}


def test_eval_params_errors(tmp_path):
    with pytest.raises(ValueError, match=r"needs an \[EVAL\] section"):
        launcher.eval_params(launcher.read_config(write_ini(tmp_path, "")))
    with pytest.raises(ValueError, match="needs image_dir"):
        launcher.eval_params(launcher.read_config(write_ini(tmp_path, "[EVAL]\nannotation_dir = ann/\n")))
    with pytest.raises(ValueError, match="match_iou must be in"):
        launcher.eval_params(launcher.read_config(write_ini(tmp_path, "[EVAL]\nannotation_dir = a/\nimage_dir = b/\nmatch_iou = 1.5\n")))


def test_other_modes_are_unchanged(tmp_path):
    cfg = launcher.read_config(write_ini(tmp_path, ""))
    for mode in ("train", "anchor"):
        with pytest.raises(SystemExit, match="mode '%s' is not supported by the HIP inference backend" % mode):
            launcher.run(cfg, mode)
    with pytest.raises(ValueError, match="Unsupported mode: bogus"):
        launcher.run(cfg, "bogus")


def test_eval_refuses_more_than_one_process(tmp_path, monkeypatch):
    cfg = launcher.read_config(write_ini(tmp_path, "[EVAL]\nannotation_dir = ann/\nimage_dir = val/\n"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="runs in one process"):
        launcher.run(cfg, "eval")


def test_shipped_configs_have_an_eval_section():
    cfg_dir = os.path.join(ROOT, "tensorflow-yolo_amd", "config")
    for name in sorted(os.listdir(cfg_dir)):
        p = launcher.eval_params(launcher.read_config(os.path.join(cfg_dir, name)))
        assert os.path.isabs(p["annotation_dir"]) and os.path.isabs(p["image_dir"]) and p["threshold"] == "0.005", name

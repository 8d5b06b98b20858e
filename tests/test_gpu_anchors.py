"""GPU: anchor k-means (include/yolo_hip.h "Anchor k-means on the device") through yolo_anchor_kmeans against the sequential yardstick of
tests/anchor_ref.py.  Every comparison is np.array_equal / ==: the definition leaves no tolerance.  Every call runs twice, with scratch,
result and labels pre-filled with 0x00 and then with 0xFF bytes, and both runs must give the same bytes (the second is also the "two calls
give the same bits" check).  The sizes stand around the chunk of boxes a workgroup takes (tests/anchor_cases.py; pinned against
yolo_anchor_plan in tests/test_anchors_cpu.py), the cases that are there to show a property are checked for it on the yardstick."""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

import anchor_cases as ac
import anchor_ref as ref
from helpers import ROOT
from tensorflow_yolo_amd import _hip, launcher
from tensorflow_yolo_amd.net import anchors as yanchors, engine

pytestmark = pytest.mark.gpu
EIFFEL = os.path.join(ROOT, "tests", "golden", "anchor", "eiffel")


def run(wh, k, distance, init=None, labels=True, **kw):
    """yolo_anchor_kmeans twice, everything it writes pre-filled with 0x00 and 0xFF -> (result dict, labels or None)"""
    import torch
    d = _hip.anchor_distance(distance)
    x = torch.from_numpy(np.ascontiguousarray(wh, dtype=np.float64)).cuda()
    c0 = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float64)).cuda() if init is not None else None
    pl = engine.anchor_plan(len(wh), k, d, kw.get("tolerate", 0.005), kw.get("n_init", 10), kw.get("max_iter", 300), kw.get("seed", 0))
    outs = []
    for fill in (0x00, 0xFF):
        scratch = torch.full((pl["scratch_bytes"],), fill, dtype=torch.uint8, device="cuda")
        result = torch.full((pl["result_bytes"],), fill, dtype=torch.uint8, device="cuda")
        lab = torch.full((len(wh),), -1 if fill else 0, dtype=torch.int32, device="cuda") if labels else None
        res, lab = engine.anchor_kmeans(x, k, d, init=c0, scratch=scratch, result=result, labels=lab, **kw)
        outs.append((res, lab.cpu().numpy() if lab is not None else None))
    assert np.array_equal(x.cpu().numpy(), np.asarray(wh, dtype=np.float64), equal_nan=True), "the data were written"
    assert np.array_equal(outs[0][0]["raw"], outs[1][0]["raw"]), "the result depends on what scratch / result held"
    if labels:
        assert np.array_equal(outs[0][1], outs[1][1]), "the labels depend on what scratch / labels held"
    return outs[0]


def compare(got, labels, want):
    for key in ("status", "best_restart", "n_valid", "n_bad", "k", "n_init", "distance", "inertia_q", "iou_q"):
        assert got[key] == want[key], (key, got[key], want[key])
    for r, (g, w) in enumerate(zip(got["restarts"], want["restarts"])):
        for key in ("seeds", "n_iter", "status", "inertia_q", "iou_q"):
            assert g[key] == w[key], ("restart %d" % r, key, g[key], w[key])
    assert len(got["restarts"]) == len(want["restarts"])
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["sum_q"], want["sum_q"])
    assert np.array_equal(got["centres"], want["centres"]), np.abs(got["centres"] - want["centres"]).max()       # the same bits
    assert got["inertia"] == want["inertia"] and got["avg_iou"] == want["avg_iou"], (got["avg_iou"], want["avg_iou"])
    if labels is not None:
        bad = np.flatnonzero(labels != want["labels"])
        assert len(bad) == 0, "%d labels differ, first at %d: got %d, want %d" % (len(bad), bad[0], labels[bad[0]], want["labels"][bad[0]])


def check(wh, k, distance, **kw):
    got, labels = run(wh, k, distance, **kw)
    want = ref.kmeans(wh, k, _hip.anchor_distance(distance), **{"n_init": 10, **kw})
    compare(got, labels, want)
    return got, want


@pytest.mark.parametrize("distance", ac.DISTANCES)
@pytest.mark.parametrize("n", ac.LLOYD_N)
def test_lloyd_from_given_centres(n, distance):
    """labels, counts, integer sums, centres, n_iter, integer inertia and avg_iou for every k at this size"""
    wh = ac.boxes(n, n)
    for k in ac.LLOYD_K:
        check(wh, k, distance, init=ac.start(wh, k, n + k), n_init=1)


@pytest.mark.parametrize("name", sorted(ac.stop_cases()))
def test_stop_rules(name):
    wh, k, kw = ac.stop_cases()[name]
    got, want = check(wh, k, "euclidean", **kw)
    row = got["restarts"][0]
    if name.startswith("max_iter"):
        assert row["n_iter"] == kw["max_iter"] and row["status"] & _hip.ANCHOR_MAX_ITER and got["status"] & _hip.ANCHOR_MAX_ITER
    else:
        assert not row["status"] & _hip.ANCHOR_MAX_ITER
    if name == "tolerate_1e+09":
        assert row["n_iter"] == 1
    # the two cases that are there for the order of the rules show it (on the yardstick, whose figures the library has just equalled)
    if name == "labels_first":
        assert want["restarts"][0]["stop"] == "labels" and kw["tolerate"] > 0
    if name == "tolerance_first":
        assert want["restarts"][0]["stop"] == "tolerance" and row["n_iter"] >= 2


@pytest.mark.parametrize("distance", ac.DISTANCES)
def test_iou_and_euclidean_stop_at_max_iter(distance):
    wh = ac.boxes(700, 5)
    for m in (1, 2):
        got, _ = check(wh, 5, distance, init=ac.start(wh, 5, 5), n_init=1, max_iter=m, tolerate=0.0)
        assert got["restarts"][0]["n_iter"] == m and got["status"] & _hip.ANCHOR_MAX_ITER


@pytest.mark.parametrize("distance", ac.DISTANCES)
@pytest.mark.parametrize("name", sorted(ac.tie_cases()))
def test_ties_and_empty_clusters(name, distance):
    wh, k, kw = ac.tie_cases()[name]
    got, want = check(wh, k, distance, **kw)
    if name == "identical_centres":
        # the first of the two equal centres takes the boxes; the second keeps its centre through the update and says so
        assert got["status"] & _hip.ANCHOR_EMPTY_CLUSTER
        assert any(np.array_equal(c, kw["init"][0]) for c in got["centres"][:k])
    if name == "equidistant" and distance == "euclidean":
        assert got["status"] & _hip.ANCHOR_EMPTY_CLUSTER == 0 and sorted(got["counts"][:2]) == [1, 3]


@pytest.mark.parametrize("distance", ac.DISTANCES)
@pytest.mark.parametrize("n_init,seed,n", [(1, 0, ac.CHUNK - 1), (3, 1, ac.CHUNK), (10, 2 ** 63, ac.CHUNK + 1), (3, 0, 2 * ac.CHUNK + 3),
                                           (10, 1, 300), (3, 2 ** 63, 65)])
def test_seeding_and_restarts(n_init, seed, n, distance):
    """the seed indices of every restart, the per-restart table and the best index"""
    got, want = check(ac.boxes(n, n_init + n), 5, distance, n_init=n_init, seed=seed)
    assert all(s >= 0 for row in got["restarts"] for s in row["seeds"][:5]) and all(s == -1 for row in got["restarts"] for s in row["seeds"][5:])


@pytest.mark.parametrize("distance", ac.DISTANCES)
def test_seeding_heavy_duplicates(distance):
    for seed in ac.SEEDS:
        check(ac.duplicates(2 * ac.CHUNK + 3, 7, 3), 7, distance, n_init=3, seed=seed)
        check(ac.duplicates(ac.CHUNK + 1, 40, 4), 9, distance, n_init=3, seed=seed)


@pytest.mark.parametrize("distance", ac.DISTANCES)
def test_seeding_two_boxes_and_degenerate(distance):
    wh = np.array([[0.25, 0.5], [0.75, 0.125]])
    for seed in ac.SEEDS:
        got, _ = check(wh, 2, distance, n_init=3, seed=seed)
        for row in got["restarts"]:
            assert sorted(row["seeds"][:2]) == [0, 1]               # the second seed is the other box
    same = np.tile([[0.3, 0.4]], (70, 1))
    got, labels = run(same, 2, distance, n_init=3)
    compare(got, labels, ref.kmeans(same, 2, _hip.anchor_distance(distance), n_init=3))
    assert got["status"] == _hip.ANCHOR_DEGENERATE and got["best_restart"] == -1 and (labels == -1).all()
    assert all(row["status"] == _hip.ANCHOR_DEGENERATE and row["n_iter"] == 0 and row["seeds"][0] >= 0 and row["seeds"][1] == -1
               for row in got["restarts"])
    assert not got["centres"].any() and not got["counts"].any()
    # one restart from given centres works on such data, with an empty cluster
    got, _ = check(same, 2, distance, init=np.array([[0.3, 0.4], [0.9, 0.9]]), n_init=1)
    assert got["status"] == _hip.ANCHOR_EMPTY_CLUSTER and list(got["counts"][:2]) == [70, 0]


def test_restarts_finish_at_different_iterations_and_ties_go_to_the_lower_index():
    got, want = check(ac.boxes(300, 2), 5, "iou", n_init=10, seed=1)
    assert len({row["n_iter"] for row in want["restarts"]}) > 2
    # twelve boxes, two clusters: several restarts end in the same partition, the lowest of them is the best
    got, want = check(ac.boxes(12, 12), 2, "euclidean", n_init=10, seed=0)
    low = min(row["inertia_q"] for row in want["restarts"])
    winners = [r for r, row in enumerate(want["restarts"]) if row["inertia_q"] == low]
    assert len(winners) >= 2 and got["best_restart"] == winners[0]


@pytest.mark.parametrize("distance", ac.DISTANCES)
def test_bad_boxes_are_skipped_counted_and_flagged(distance):
    wh, bad = ac.with_bad_boxes(ac.boxes(ac.CHUNK + 77, 13))
    got, labels = run(wh, 5, distance, n_init=3, seed=1)
    compare(got, labels, ref.kmeans(wh, 5, _hip.anchor_distance(distance), n_init=3, seed=1))
    assert got["status"] & _hip.ANCHOR_BAD_BOX and got["n_bad"] == len(bad) and got["n_valid"] == len(wh) - len(bad)
    assert (labels[bad] == -1).all() and (np.delete(labels, bad) >= 0).all() and labels[40] >= 0 and labels[41] >= 0
    # nothing but bad boxes: every restart is degenerate
    none = np.array([[0.0, 0.5], [np.nan, 0.5], [2.0, 2.0]])
    got, labels = run(none, 1, distance, n_init=2)
    compare(got, labels, ref.kmeans(none, 1, _hip.anchor_distance(distance), n_init=2))
    assert got["status"] == _hip.ANCHOR_BAD_BOX | _hip.ANCHOR_DEGENERATE and got["n_valid"] == 0 and (labels == -1).all()


def test_without_labels():
    wh = ac.boxes(ac.CHUNK + 5, 21)
    got, labels = run(wh, 5, "iou", n_init=3, labels=False)
    assert labels is None
    compare(got, None, ref.kmeans(wh, 5, ref.IOU, n_init=3))


def test_kmeans_anchors_and_refusals():
    wh = ac.boxes(500, 31)
    res = yanchors.kmeans_anchors(wh, 9, distance="iou", n_init=4, seed=7)
    want = ref.kmeans(wh, 9, ref.IOU, n_init=4, seed=7)
    assert np.array_equal(res.anchors, want["centres"][:9]) and np.array_equal(res.labels, want["labels"]) and res.avg_iou == want["avg_iou"]
    assert res.best_restart == want["best_restart"] and res.n_iter == want["restarts"][want["best_restart"]]["n_iter"]
    areas = res.anchors[:, 0] * res.anchors[:, 1]
    assert (np.diff(areas) >= 0).all()
    import torch
    x = torch.from_numpy(wh).cuda()
    with pytest.raises(_hip.YoloHipError, match="yolo_anchor_kmeans: n_init must be 1 when init is given"):
        engine.anchor_kmeans(x, 2, n_init=3, init=x[:2].contiguous())
    with pytest.raises(_hip.YoloHipError, match="yolo_anchor_kmeans: scratch of 256 bytes, the plan needs"):
        engine.anchor_kmeans(x, 2, scratch=torch.zeros(256, dtype=torch.uint8, device="cuda"))


def write_ini(path, version, annotation_dir, num_anchors, extra=""):
    path.write_text("[COMMON]\nversion = %s\ninput_h = 416\ninput_w = 416\ninput_c = 3\n\n[ANCHOR]\nkmeans = device\nnum_anchors = %d\n"
                    "image_dir = %s\nannotation_dir = %s\ntolerate = 0.005\nstride = 32\n%s" % (version, num_anchors, annotation_dir, annotation_dir, extra))
    return str(path)


def test_launcher_anchor_mode_on_the_eiffel_annotations(tmp_path):
    """num_anchors = 1, the reference's own [ANCHOR] section: the anchor is the mean of the ten (w, h) times 416 / 32"""
    ini = write_ini(tmp_path / "a.ini", "v2", EIFFEL, 1)
    out = io.StringIO()
    with redirect_stdout(out):
        launcher.main(["--config", ini, "--mode", "anchor"])
    lines = out.getvalue().splitlines()
    at = lines.index("Anchors: ")
    wh, names = yanchors.read_box_sizes(EIFFEL)
    want = ref.kmeans(wh, 1, ref.EUCLIDEAN)
    anchors = np.array([want["centres"][0][0] * 416 / 32, want["centres"][0][1] * 416 / 32])
    assert lines[at + 1] == "\t{}".format(anchors) and lines[at + 2] == "Class names: " and lines[at + 3] == "\t['tower']"
    assert np.abs(anchors - wh.mean(axis=0) * 13).max() <= 13 * 2.0 ** -40
    assert "distance: euclidean" in lines and "boxes used: 10, skipped: 0" in lines and "iterations: %d" % want["restarts"][0]["n_iter"] in lines
    assert lines[-1] == "anchors = {}".format([float(v) for v in anchors])


def test_launcher_anchor_mode_v3(tmp_path):
    """nine anchors in network pixels, ascending by area, equal to kmeans_anchors called directly"""
    wh = ac.boxes(120, 41)
    d = tmp_path / "ann"
    d.mkdir()
    data = []
    for i, (w, h) in enumerate(wh):
        bw, bh = max(1, int(round(w * 640))), max(1, int(round(h * 480)))
        data.append((bw, bh))
        (d / ("img%03d.xml" % i)).write_text(
            "<annotation><filename>img%03d.jpg</filename><size><width>640</width><height>480</height><depth>3</depth></size><object>"
            "<name>%s</name><bndbox><xmin>3</xmin><ymin>2</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object></annotation>"
            % (i, "cat" if i % 3 else "dog", 3 + bw, 2 + bh))
    ini = write_ini(tmp_path / "b.ini", "v3", str(d), 9, "distance = iou\nn_init = 4\nseed = 3\n")
    out = io.StringIO()
    with redirect_stdout(out):
        launcher.main(["--config", ini, "--mode", "anchor"])
    lines = out.getvalue().splitlines()
    boxes, names = yanchors.read_box_sizes(str(d))
    assert names == {"cat", "dog"} and len(boxes) == 120
    res = yanchors.kmeans_anchors(boxes, 9, distance="iou", n_init=4, seed=3)
    anchors = np.reshape([[a[0] * 416, a[1] * 416] for a in res.anchors], [-1])
    assert lines[-1] == "anchors = {}".format([float(v) for v in anchors]) and "\t['cat', 'dog']" in lines and "distance: iou" in lines
    areas = anchors[0::2] * anchors[1::2]
    assert len(anchors) == 18 and (np.diff(areas) >= 0).all()
    assert np.array_equal(res.anchors, ref.kmeans(boxes, 9, ref.IOU, n_init=4, seed=3)["centres"][:9])

"""CPU: the anchor k-means yardstick (tests/anchor_ref.py) against scikit-learn, the data and the random stream of the definition, the host
side of the entries (plan, refusals, the sanitizer program), net/anchors.py's gate, and the behaviour without `kmeans = device`."""
import ctypes as C
import os
import subprocess
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import anchor_cases as ac
import anchor_ref as ref
from augment_ref import philox4x32_10
from helpers import ROOT
from tensorflow_yolo_amd import YoloV2, YoloV3, _hip, launcher
from tensorflow_yolo_amd.net import anchors as yanchors, engine

EIFFEL = os.path.join(ROOT, "tests", "golden", "anchor", "eiffel")
CONFIG = os.path.join(ROOT, "tensorflow-yolo_amd", "config")
# (generator seed, boxes, clusters): log-normal(-1.5, 0.8) clipped to [0.01, 1], not quantised
SKLEARN_CASES = [(0, 37, 3), (1, 200, 5), (2, 1000, 9), (3, 5000, 5), (0, 5000, 9)]


def float64_lloyd(X, init, tol, max_iter=300):
    """sklearn's Lloyd loop restated in plain float64 on the data as given (means by np.mean, no quantisation) -> (centres, n_iter)"""
    c = np.array(init, dtype=np.float64)
    thr = np.mean(np.var(X, axis=0)) * tol
    prev = np.full(len(X), -1)
    for it in range(1, max_iter + 1):
        d = ((X[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
        labels = d.argmin(axis=1)
        new = np.array([X[labels == j].mean(axis=0) if (labels == j).any() else c[j] for j in range(len(c))])
        shift = ((new - c) ** 2).sum()
        c = new
        if np.array_equal(labels, prev) or shift <= thr:
            break
        prev = labels
    return c, it


@pytest.mark.parametrize("tolerate", [0.005, 1e-4, 0.0])
@pytest.mark.parametrize("seed,n,k", SKLEARN_CASES)
def test_yardstick_against_sklearn(seed, n, k, tolerate):
    """With the yardstick's own seeds as `init`, n_init = 1 and algorithm = "lloyd", sklearn's KMeans on the UN-quantised data stops after
    the same number of iterations as the yardstick on the quantised data, and its centres lie within 2^-40 (the quantisation: a centre is a
    mean of values moved by at most 2^-41 each) plus sklearn's own float64 noise.  That noise is measured here, as the distance between
    sklearn and a plain float64 run of the same loop on the same un-quantised data: it was at most 4.5e-16 over these 15 cases (sklearn
    subtracts the data's mean before it iterates and adds it back).  Precondition, asserted: at every iteration of every case the gap
    between a box's best and second-best distance exceeds 1e-10 (measured: 8.3e-8 at the least), so that no label hangs on a rounding;
    and no cluster is ever empty (sklearn would relocate it, the definition keeps it)."""
    cluster = pytest.importorskip("sklearn.cluster")
    X = ac.boxes(n, seed)
    q, valid = ref.quantise(X)
    assert valid.all()
    seeds, degenerate = ref.seeding(q, valid, k, ref.EUCLIDEAN, seed, 0)
    assert not degenerate and len(set(seeds)) == k
    trace = []
    run = ref.lloyd(q, valid, [q[s] / ref.TWO40 for s in seeds], ref.EUCLIDEAN, ref.threshold(q, valid, tolerate), 300, trace=trace)
    assert not run["status"] & ref.EMPTY_CLUSTER and run["n_iter"] <= 100
    w, h = q[:, 0] / ref.TWO40, q[:, 1] / ref.TWO40
    gap = np.inf
    for labels, centres in trace:
        d = np.sort(np.stack([ref.dist(ref.EUCLIDEAN, w, h, c[0], c[1]) for c in centres]), axis=0)
        gap = min(gap, float((d[1] - d[0]).min()))
    assert gap > 1e-10, gap
    km = cluster.KMeans(n_clusters=k, init=X[seeds], n_init=1, tol=tolerate, algorithm="lloyd", max_iter=300).fit(X)
    plain, plain_iter = float64_lloyd(X, X[seeds], tolerate)
    noise = float(np.abs(km.cluster_centers_ - plain).max())
    err = float(np.abs(np.array(run["centres"], dtype=np.float64) - km.cluster_centers_).max())
    print("n %d k %d tolerate %g: n_iter %d (sklearn %d, float64 %d), gap %.3e, |yardstick - sklearn| %.3e, sklearn's noise %.3e"
          % (n, k, tolerate, run["n_iter"], km.n_iter_, plain_iter, gap, err, noise))
    assert km.n_iter_ == run["n_iter"] == plain_iter
    assert noise <= 1e-13
    assert err <= 2.0 ** -40 + noise


# ---- the data and the random stream -----------------------------------------------------------------------------------------------------
def test_box_sizes_are_the_references_arithmetic_on_the_eiffel_annotations():
    wh, names = yanchors.read_box_sizes(EIFFEL)
    files = sorted(os.listdir(EIFFEL))
    assert len(files) == 10 and names == {"tower"} and wh.shape == (10, 2) and wh.dtype == np.float64
    want = []
    for f in files:                     # net/base.py:78-93 with normalize = True, then net/v2.py:315-316
        root = ET.parse(os.path.join(EIFFEL, f)).getroot()
        width, height = int(root.find("size").find("width").text), int(root.find("size").find("height").text)
        for o in root.findall("object"):
            b = o.find("bndbox")
            x1, y1, x2, y2 = (int(b.find(t).text) for t in ("xmin", "ymin", "xmax", "ymax"))
            want.append([float(x2 / width - x1 / width), float(y2 / height - y1 / height)])
    assert np.array_equal(wh, np.array(want))
    assert wh[0, 0] == 952 / 1920 - 595 / 1920 and wh[0, 1] == 905 / 1080 - 103 / 1080          # tower01.xml
    q, valid = ref.quantise(wh)
    assert valid.all() and np.abs(q / ref.TWO40 - wh).max() <= 2.0 ** -41


def test_philox_known_answers_and_the_draw():
    zero = [int(v) for v in philox4x32_10(0, 0, 0, 0, 0, 0)]
    ones = [int(v) for v in philox4x32_10(*([0xFFFFFFFF] * 6))]
    assert zero == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8] and ones == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert ref.draw(0, 0, 0) == (0x6627E8D5 << 32) | 0xE169C58D
    # the key is the seed's two halves, the counter (restart, round, 0, 0)
    o = philox4x32_10(5, 3, 0, 0, 0x89ABCDEF, 0x01234567)
    assert ref.draw(0x0123456789ABCDEF, 5, 3) == (int(o[0]) << 32) | int(o[1])
    assert ref.draw(2 ** 63, 1, 2) != ref.draw(0, 1, 2) and ref.draw(-1, 0, 0) == ref.draw(2 ** 64 - 1, 0, 0)


def mulhi64(a, b):
    """the upper half of a 64 x 64-bit product from 32-bit limbs (what a device's 64-bit multiply-high computes)"""
    m = 0xFFFFFFFF
    a0, a1, b0, b1 = a & m, a >> 32, b & m, b >> 32
    mid = a1 * b0 + ((a0 * b0) >> 32)
    mid2 = a0 * b1 + (mid & m)
    return (a1 * b1 + (mid >> 32) + (mid2 >> 32)) & 0xFFFFFFFFFFFFFFFF


def test_seeding_products_match_python_ints():
    """t = floor(u * T / 2^64): the 128-bit product in limbs equals Python's, t < T always, and the pick follows the prefix sums"""
    rng = np.random.default_rng(0)
    us = [0, 1, 2 ** 64 - 1, 2 ** 63, 2 ** 32, 2 ** 32 - 1] + [int(v) for v in rng.integers(0, 2 ** 64, size=50, dtype=np.uint64)]
    Ts = [1, 2, 2 ** 22, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 2 ** 22 * 2 ** 41] + [int(v) for v in rng.integers(1, 2 ** 63, size=50, dtype=np.uint64)]
    for u in us:
        for T in Ts:
            t = (u * T) >> 64
            assert mulhi64(u, T) == t and 0 <= t < T
    # round 0 picks valid box number floor(u * n_valid / 2^64) in index order, whatever lies between the valid ones
    wh, bad = ac.with_bad_boxes(ac.boxes(200, 3))
    q, valid = ref.quantise(wh)
    idx = np.flatnonzero(valid)
    for restart in range(8):
        seeds, _ = ref.seeding(q, valid, 1, ref.IOU, 11, restart)
        assert seeds == [int(idx[(ref.draw(11, restart, 0) * len(idx)) >> 64])]
    # round j never picks a box that is already a seed (its weight is 0), in either distance
    for distance in (ref.EUCLIDEAN, ref.IOU):
        seeds, degenerate = ref.seeding(q, valid, 20, distance, 5, 0)
        assert not degenerate and len({tuple(q[s]) for s in seeds}) == 20


# ---- the host code ------------------------------------------------------------------------------------------------------------------------
def test_plan_numbers():
    assert C.sizeof(_hip.AnchorDesc) == 32 and C.sizeof(_hip.AnchorHeader) == 32 and C.sizeof(_hip.AnchorRestart) == 152
    assert C.sizeof(_hip.AnchorBest) == 32 * 16 + 32 * 8 + 32 * 16 + 32 and C.sizeof(_hip.AnchorPlan) == 16 + 12 * 8
    for n in ac.LLOYD_N + [1 << 22]:
        for n_init in (1, 10, 64):
            pl = engine.anchor_plan(n, 9, n_init=n_init)
            assert pl["chunk"] == ac.CHUNK == 1024 and pl["threads"] == 256 and pl["period"] == 8
            assert pl["n_chunks"] == -(-n // 1024)
            parts = [pl[key] for key in ("prep_offset", "pick_offset", "state_offset", "q_offset", "label_offset", "sums_offset", "scratch_bytes")]
            assert all(p % 256 == 0 for p in parts) and parts == sorted(set(parts)) and parts[0] == 0
            assert pl["q_offset"] - pl["state_offset"] >= n_init * (32 * 16 + 2 * 32 * 24 + 24 + 32 * 4 + 16)
            assert pl["label_offset"] - pl["q_offset"] >= 16 * n and pl["label_stride"] >= n and pl["label_stride"] % 256 == 0
            assert pl["sums_offset"] - pl["label_offset"] == n_init * pl["label_stride"]
            assert pl["scratch_bytes"] - pl["sums_offset"] >= 8 * n_init * pl["n_chunks"]
            assert (pl["header_offset"], pl["restarts_offset"]) == (0, 256)
            assert pl["best_offset"] == 256 + -(-152 * n_init // 256) * 256 and pl["result_bytes"] == pl["best_offset"] + 1536
    assert engine.anchor_plan(1 << 22, 32, n_init=64)["scratch_bytes"] < 1 << 29


PLAN_REFUSALS = [(dict(k=0), "k must be 1 .. 32, got 0"), (dict(k=33), "k must be 1 .. 32, got 33"), (dict(n_init=0), "n_init must be 1 .. 64, got 0"),
                 (dict(n_init=65), "n_init must be 1 .. 64, got 65"), (dict(max_iter=0), "max_iter must be 1 .. 10000, got 0"),
                 (dict(max_iter=10001), "max_iter must be 1 .. 10000, got 10001"), (dict(distance=2), "distance must be YOLO_ANCHOR_EUCLIDEAN or YOLO_ANCHOR_IOU, got 2"),
                 (dict(tolerate=-0.5), "tolerate must be finite and not negative"), (dict(tolerate=float("nan")), "tolerate must be finite and not negative"),
                 (dict(tolerate=float("inf")), "tolerate must be finite and not negative"), (dict(n=0), "n must be 1 .. 2^22, got 0"),
                 (dict(n=(1 << 22) + 1), "n must be 1 .. 2^22, got 4194305")]


@pytest.mark.parametrize("kw,msg", PLAN_REFUSALS)
def test_plan_and_call_refuse_bad_sizes(kw, msg):
    kw = dict(kw)
    n = kw.pop("n", 100)
    desc = _hip.anchor_desc(**{"k": 5, **kw})
    with pytest.raises(_hip.YoloHipError, match="yolo_anchor_plan: " + msg.replace("^", r"\^")):
        _hip.anchor_plan(desc, n)
    lib = _hip.lib()
    assert lib.yolo_anchor_kmeans(C.byref(desc), 1 << 20, n, None, 2 << 20, 1 << 30, 3 << 20, 1 << 20, None, None) == 1
    assert lib.yolo_last_error().decode() == "yolo_anchor_kmeans: " + msg


def test_call_refuses_bad_arguments():
    """every refusal of anchor_host.cpp in front of a launch: nothing is dereferenced, numbers stand in for device pointers"""
    lib = _hip.lib()
    desc = _hip.anchor_desc(5)
    pl = _hip.anchor_plan(desc, 1500)
    S, R, WH, LAB, INIT = 1 << 30, 2 << 30, 3 << 30, 4 << 30, 5 << 30
    sb, rb = pl["scratch_bytes"], pl["result_bytes"]

    def refused(msg, desc=desc, wh=WH, init=None, scratch=S, scratch_bytes=sb, result=R, result_bytes=rb, labels=LAB):
        assert lib.yolo_anchor_kmeans(C.byref(desc), wh, 1500, init, scratch, scratch_bytes, result, result_bytes, labels, None) == 1
        assert lib.yolo_last_error().decode() == "yolo_anchor_kmeans: " + msg

    refused("null argument", wh=None)
    refused("null argument", scratch=None)
    refused("null argument", result=None)
    assert lib.yolo_anchor_kmeans(None, WH, 1500, None, S, sb, R, rb, LAB, None) == 1 and b"yolo_anchor_kmeans: null argument" == lib.yolo_last_error()
    refused("n_init must be 1 when init is given, got 10", init=INIT)
    refused("wh and init must be 8-byte aligned", wh=WH + 4)
    refused("wh and init must be 8-byte aligned", desc=_hip.anchor_desc(5, n_init=1), init=INIT + 2)
    refused("scratch and result must be 256-byte aligned", scratch=S + 128)
    refused("scratch and result must be 256-byte aligned", result=R + 64)
    refused("labels must be 4-byte aligned", labels=LAB + 2)
    refused("scratch of %d bytes, the plan needs %d" % (sb - 1, sb), scratch_bytes=sb - 1)
    refused("result of %d bytes, the plan needs %d" % (rb - 256, rb), result_bytes=rb - 256)
    refused("wh must not overlap the scratch", wh=S + sb - 8)
    refused("result must not overlap the scratch", result=S + 256)
    refused("labels must not overlap the scratch", labels=S + 4)
    refused("init must not overlap the scratch", desc=_hip.anchor_desc(5, n_init=1), init=S - 8, scratch_bytes=1 << 20)
    assert lib.yolo_anchor_plan(C.byref(desc), 5, None) == 1 and lib.yolo_last_error() == b"yolo_anchor_plan: null argument"


def test_check_params_names_the_problem():
    good = {"num_anchors": "5", "tolerate": "0.005", "stride": "32", "input_w": "416", "input_h": "416", "kmeans": "device"}
    assert yanchors.check_params(good, "v2") == dict(k=5, distance=0, tolerate=0.005, n_init=10, max_iter=300, seed=0)
    assert yanchors.check_params(dict(good, distance="IoU", n_init="3", max_iter="50", seed="9"), "v2-tiny") == dict(
        k=5, distance=1, tolerate=0.005, n_init=3, max_iter=50, seed=9)
    with pytest.raises(ValueError, match="distance must be euclidean or iou, got 'manhattan'"):
        yanchors.check_params(dict(good, distance="manhattan"), "v2")
    for version, scales in (("v3", 3), ("v3-spp", 3), ("v3-tiny", 2)):
        with pytest.raises(ValueError, match="num_anchors must be a multiple of %d for a %s network" % (scales, version)):
            yanchors.check_params(dict(good, num_anchors="7"), version)
        assert yanchors.check_params(dict(good, num_anchors="6"), version)["k"] == 6
    with pytest.raises(ValueError, match="num_anchors must be 1 .. 32, got 33"):
        yanchors.check_params(dict(good, num_anchors="33"), "v3")
    with pytest.raises(ValueError, match="num_anchors must be 1 .. 32, got 0"):
        yanchors.check_params(dict(good, num_anchors="0"), "v2")
    with pytest.raises(ValueError, match="tolerate must be finite and not negative"):
        yanchors.check_params(dict(good, tolerate="-1"), "v2")
    with pytest.raises(ValueError, match="n_init must be 1 .. 64, got 100"):
        yanchors.check_params(dict(good, n_init="100"), "v2")
    with pytest.raises(ValueError, match="max_iter must be 1 .. 10000, got 0"):
        yanchors.check_params(dict(good, max_iter="0"), "v2")
    wh = ac.duplicates(50, 4, 1)
    with pytest.raises(ValueError, match="num_anchors = 5 needs at least as many distinct boxes, the data hold 4"):
        yanchors.check_params(good, "v2", wh)
    assert yanchors.check_params(dict(good, num_anchors="4"), "v2", wh)["k"] == 4
    bad, _ = ac.with_bad_boxes(ac.boxes(50, 2))
    assert yanchors.distinct_boxes(bad) == 42
    with pytest.raises(ValueError, match="kmeans must be device"):
        yanchors.anchor_option({"kmeans": "sklearn"})
    assert yanchors.anchor_option({"kmeans": " Device "}) and not yanchors.anchor_option({})
    # units: grid cells for v2 (the reference's a * input / stride), network pixels for the v3 family
    a = np.array([[0.25, 0.5], [0.5, 0.125]])
    assert list(yanchors.scale_anchors(a, dict(good, input_w="416", input_h="320"), "v2")) == [0.25 * 416 / 32, 0.5 * 320 / 32, 0.5 * 416 / 32, 0.125 * 320 / 32]
    assert list(yanchors.scale_anchors(a, dict(good, input_w="416", input_h="320"), "v3-tiny")) == [104.0, 160.0, 208.0, 40.0]


def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """`make san-anchor`: anchor_host.cpp with anchor_host_check.cpp, a program of its own, on the CPU"""
    csrc = os.path.join(ROOT, "tensorflow-yolo_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc, "san-anchor", "OBJDIR=" + str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "anchor_host_check OK" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


# ---- without the key nothing has changed ---------------------------------------------------------------------------------------------------
def test_without_the_key_the_three_refusals_stand(tmp_path, capsys):
    for model in (YoloV2(), YoloV3()):
        with pytest.raises(NotImplementedError) as e:
            model.generate_anchors({"num_anchors": "5"})
        assert str(e.value) == "anchor mode is not supported by the HIP inference backend"
    ini = tmp_path / "plain.ini"
    ini.write_text("[COMMON]\nversion = v2\ninput_h = 416\ninput_w = 416\ninput_c = 3\n\n[ANCHOR]\nnum_anchors = 1\nannotation_dir = %s\n"
                   "image_dir = %s\ntolerate = 0.005\nstride = 32\n" % (EIFFEL, EIFFEL))
    with pytest.raises(SystemExit) as e:
        launcher.run(launcher.read_config(str(ini)), "anchor")
    assert str(e.value) == "mode 'anchor' is not supported by the HIP inference backend (TEST mode only)"
    with pytest.raises(SystemExit) as e:           # the default config and the default mode
        launcher.main([])
    assert str(e.value) == "mode 'anchor' is not supported by the HIP inference backend (TEST mode only)"
    for name in ("yolo_2.ini", "yolo_3.ini"):
        assert "kmeans" not in launcher.read_config(os.path.join(CONFIG, name)).get("ANCHOR", {})
    # the new configs opt in and pass the gate; a bad value of the key is named before anything runs
    for name, version, k in (("yolo_2_anchor.ini", "v2", 5), ("yolo_3_anchor.ini", "v3", 9)):
        cfg = launcher.read_config(os.path.join(CONFIG, name))
        params = dict(cfg["ANCHOR"], **cfg["COMMON"])
        assert yanchors.anchor_option(params) and params["version"] == version and yanchors.check_params(params, version)["k"] == k
    ini.write_text("[COMMON]\nversion = v2\n[ANCHOR]\nkmeans = host\nnum_anchors = 1\n")
    with pytest.raises(ValueError, match="kmeans must be device"):
        launcher.run(launcher.read_config(str(ini)), "anchor")
    ini.write_text("[COMMON]\nversion = v3\n[ANCHOR]\nkmeans = device\nnum_anchors = 4\n")
    with pytest.raises(ValueError, match="num_anchors must be a multiple of 3 for a v3 network"):
        launcher.run(launcher.read_config(str(ini)), "anchor")

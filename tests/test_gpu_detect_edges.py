"""GPU: nms_kernel at its path and word boundaries, the small path's truncation / overflow branches, per-class mode above
512 and above 4096 candidates -- against the oracle's NMS semantics (tests/nms_ref.py: float64, vectorised, pinned to the
restatement by tests/test_host_logic.py).

nms_kernel (csrc/detect.hip) has three paths: rank sort + 64-bit suppression words for n <= 512, an LDS bitonic sort up to a
capacity of 4096, global-memory slabs up to 65536; yolo_nms_host runs it with capacity = n."""
import functools
import os

import numpy as np
import pytest

from helpers import GOLDEN, match_boxes
from nms_ref import clustered_boxes, vector_nms
from oracle import cases, decode_ref
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import base, engine, v3

pytestmark = pytest.mark.gpu

IOU = 0.45
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4095, 4096, 4097, 65536]
CLUSTERED_FROM = 4095       # from here on: boxes around a few hundred centres, so that few survive however many there are


@functools.lru_cache(maxsize=None)
def boxes_and_reference(n):
    """n boxes with probabilities rounded to three decimals (exact ties: the stable order matters) and three classes, and
    the float64 reference's kept indices in both modes -- computed once per n"""
    rng = np.random.RandomState(1000 + n % 997)
    if n >= CLUSTERED_FROM:
        xy, wh, prob, cls = clustered_boxes(rng, n)
    else:
        xy = rng.uniform(0.1, 0.9, size=(n, 2)).astype(np.float32)
        wh = rng.uniform(0.1, 0.4, size=(n, 2))
        prob = np.round(rng.uniform(0.3, 1.0, size=n), 3).astype(np.float32)
        cls = rng.randint(0, 3, size=n)
    want = {pc: [int(i) for i in vector_nms(xy[:, 0], xy[:, 1], wh[:, 0], wh[:, 1], prob, IOU, cls=cls, per_class=pc)]
            for pc in (False, True)}
    return xy, wh, prob, cls, want


def _boxes(xy, wh, prob, cls):
    return [base.BoundingBox(x=xy[i, 0], y=xy[i, 1], w=wh[i, 0], h=wh[i, 1], class_idx=int(cls[i]), prob=prob[i]) for i in range(len(prob))]


@pytest.mark.parametrize("per_class", [False, True], ids=["agnostic", "per_class"])
@pytest.mark.parametrize("n", SIZES)
def test_nms_at_path_and_word_boundaries(n, per_class):
    xy, wh, prob, cls, want = boxes_and_reference(n)
    want = want[per_class]
    if n >= 63:
        assert 10 < len(want) < n, (n, len(want))           # the fixture has suppression work and survivors
    if n >= CLUSTERED_FROM:
        assert len(want) <= 2000, len(want)                 # (keeps the greedy loop, here and on the device, short)
    boxes = _boxes(xy, wh, prob, cls)
    got = base.non_maximum_suppression(boxes, IOU, per_class=per_class)
    at = {id(b): i for i, b in enumerate(boxes)}
    print("n %d %s: %d kept" % (n, "per class" if per_class else "agnostic", len(want)))
    assert [at[id(b)] for b in got] == want                 # kept indices, in order, exactly


def test_more_boxes_than_the_largest_capacity_is_an_error():
    n = 65537
    z = np.zeros(n)
    boxes = _boxes(np.stack([z, z], 1), np.stack([z, z], 1), z.astype(np.float32), z.astype(int))
    with pytest.raises(_hip.YoloHipError, match="more than 65536 boxes"):
        base.non_maximum_suppression(boxes, IOU)


def _v3_head(name):
    c = cases.CASES[name]
    net = v3.create_network(np.reshape(c["anchors"], [-1, 2]), ["c"] * c["classes"], False, input_shape=cases.input_hw(c) + (3,))
    return c, cases.make_head(name), engine.head_desc_v3(net[-1].yolos)


def test_small_path_truncation_and_overflow():
    """the <= 512-candidate path's own `nk == max_boxes` and `count > cap` branches (the 1069-candidate fixture of
    test_overflow_and_truncation_are_flagged takes the LDS bitonic path): v3_96x160 has about 100 candidates and 70 survivors"""
    c, head, hd = _v3_head("v3_96x160")
    g = np.load(os.path.join(GOLDEN, "decode_v3_96x160.npz"))
    n_pre = [len(g["pre%d" % i]) for i in range(c["batch"])]
    n_post = [len(g["post%d" % i]) for i in range(c["batch"])]
    assert max(n_pre) <= 512 and min(n_post) > 50 and min(n_pre) > 64
    with pytest.raises(_hip.YoloHipError, match="max_boxes"):
        engine.decode_nms(hd, head, c["threshold"], c["iou"], max_boxes=50)
    recs, status = engine.decode_nms(hd, head, c["threshold"], c["iou"], max_boxes=50, allow_truncation=True)
    for i in range(c["batch"]):
        assert len(recs[i]) == 50 and int(status[i]) == 2
        match_boxes(recs[i], [tuple(r) for r in g["post%d" % i][:50]])      # exactly the top-50 prefix of the full list
    recs, status = engine.decode_nms(hd, head, c["threshold"], c["iou"], max_boxes=max(n_post))      # the survivor count itself fits
    assert not status.any() and [len(r) for r in recs] == n_post
    with pytest.raises(_hip.YoloHipError, match="candidate capacity"):
        engine.decode_nms(hd, head, c["threshold"], c["iou"], cand_capacity=64, max_boxes=256)


@pytest.mark.parametrize("size,obj_shift,capacity,more_than", [(160, 0.0, 4096, 512), (320, 1.5, 8192, 4096)])
def test_per_class_mode_on_the_large_paths(size, obj_shift, capacity, more_than):
    """per-class NMS had only run on the <= 512 path: a three-class head with more than 512 candidates (LDS bitonic sort, per-survivor
    loop) and one with more than 4096 (global-memory slabs), decode + NMS against the reference decode followed by the float64 helper;
    the agnostic result of the same head must differ"""
    c = dict(cases.CASES["v3_c3"], input=size, seed=91, obj_shift=obj_shift)
    head = cases.make_head(c)
    net = v3.create_network(np.reshape(c["anchors"], [-1, 2]), ["c"] * 3, False, input_shape=(size, size, 3))
    hd = engine.head_desc_v3(net[-1].yolos)
    cand = decode_ref.find_bounding_boxes_v3(head, 0.5, c["iou"], decode_ref.v3_scales(c["anchors"], (size, size)), nms=False)[0]
    assert more_than < len(cand) <= capacity, len(cand)
    arr = lambda f, t: np.array([f(b) for b in cand], t)
    got = {}
    for mode, pc in ((_hip.NMS_AGNOSTIC, False), (_hip.NMS_PER_CLASS, True)):
        recs, status = engine.decode_nms(hd, head, 0.5, c["iou"], nms_mode=mode, cand_capacity=capacity, max_boxes=capacity)
        assert not status.any()
        k = vector_nms(arr(lambda b: b.x, np.float32), arr(lambda b: b.y, np.float32), arr(lambda b: b.w, np.float64),
                       arr(lambda b: b.h, np.float64), arr(lambda b: b.prob, np.float32), c["iou"],
                       cls=arr(lambda b: int(b.class_idx), np.int64), per_class=pc)
        match_boxes(recs[0], [cand[j].astuple() for j in k])
        got[pc] = recs[0]
    print("%d candidates: %d survivors agnostic, %d per class" % (len(cand), len(got[False]), len(got[True])))
    assert len(got[True]) > len(got[False])

"""Oracle (test infrastructure): seeded synthetic head tensors shared by the fixture
generator (oracle/gen_golden.py, runs the REFERENCE) and the tests (run the oracle /
the HIP path).  Inputs are regenerated from the seed; only outputs are committed.

Value distributions follow SURVEY 8d: randn*scale with the objectness logit shifted so
that tens to hundreds of candidates pass; plus engineered ties (equal prob) and an
empty case.
"""
import numpy as np

COCO_V2_ANCHORS = [0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434,
                   7.88282, 3.52778, 9.77052, 9.16828]            # config/yolo_2.ini:52
VOC_TINY_ANCHORS = [1.08, 1.19, 3.42, 4.41, 6.63, 11.38, 9.42, 5.11, 16.62, 10.52]   # resource/yolov2-tiny-voc.anchors:1
COCO_V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119,
                   116, 90, 156, 198, 373, 326]                    # config/yolo_3.ini:39

# name -> dict(version, input | input_hw, batch, classes, seed, scale, obj_shift, threshold, iou, anchors, ties)
#   input     square network input size; input_hw = (H, W) for a non-square one (input_hw() below reads either)
#   box_scale factor on the four box logits (boxes anchor-sized around their cells: NMS has work)
#   class_ties / saturated: engineered rows, see class_tie_rows() / saturated_rows()
CASES = {
    "v2_416_thr01": dict(version=2, input=416, batch=2, classes=80, seed=11, scale=2.0, obj_shift=0.0,
                         cls_boost=0.0, threshold=0.1, iou=0.6, anchors=COCO_V2_ANCHORS, ties=0),
    "v2_416_thr05": dict(version=2, input=416, batch=2, classes=80, seed=12, scale=1.0, obj_shift=1.0,
                         cls_boost=6.0, threshold=0.5, iou=0.6, anchors=COCO_V2_ANCHORS, ties=6),
    "v2_tinyvoc_416": dict(version=2, input=416, batch=1, classes=20, seed=13, scale=1.5, obj_shift=0.5,
                           cls_boost=4.0, threshold=0.3, iou=0.5, anchors=VOC_TINY_ANCHORS, ties=0),
    "v2_416_empty": dict(version=2, input=416, batch=1, classes=80, seed=14, scale=1.0, obj_shift=-8.0,
                         cls_boost=0.0, threshold=0.5, iou=0.6, anchors=COCO_V2_ANCHORS, ties=0),
    "v3_416": dict(version=3, input=416, batch=2, classes=80, seed=21, scale=2.0, obj_shift=-4.0,
                   cls_boost=0.0, threshold=0.5, iou=0.6, anchors=COCO_V3_ANCHORS, ties=8),
    "v3_608": dict(version=3, input=608, batch=1, classes=80, seed=22, scale=2.0, obj_shift=-5.0,
                   cls_boost=0.0, threshold=0.5, iou=0.6, anchors=COCO_V3_ANCHORS, ties=0),
    "v3_416_empty": dict(version=3, input=416, batch=1, classes=80, seed=23, scale=1.0, obj_shift=-9.0,
                         cls_boost=0.0, threshold=0.5, iou=0.6, anchors=COCO_V3_ANCHORS, ties=0),
    "v3_320_lowthr": dict(version=3, input=320, batch=1, classes=80, seed=24, scale=2.0, obj_shift=-3.0,
                          cls_boost=0.0, threshold=0.25, iou=0.45, anchors=COCO_V3_ANCHORS, ties=4),
    # the headline size WITH suppression work (v3_608 above keeps all of its 141 candidates): box logits scaled down
    # so that boxes are anchor-sized around their cell centres and neighbouring cells / anchors overlap
    "v3_608_dense": dict(version=3, input=608, batch=1, classes=80, seed=25, scale=2.0, obj_shift=-3.9,
                         cls_boost=0.0, threshold=0.5, iou=0.3, anchors=COCO_V3_ANCHORS, ties=3, box_scale=0.1),
    # non-square network inputs: v3 heads 3x5 / 6x10 / 12x20 (and transposed), v2 head 3x5 / 5x3; box_scale so that NMS suppresses
    "v3_96x160": dict(version=3, input_hw=(96, 160), batch=2, classes=80, seed=31, scale=2.0, obj_shift=-2.5,
                      cls_boost=0.0, threshold=0.5, iou=0.3, anchors=COCO_V3_ANCHORS, ties=2, box_scale=0.1),
    "v3_160x96": dict(version=3, input_hw=(160, 96), batch=2, classes=80, seed=32, scale=2.0, obj_shift=-2.5,
                      cls_boost=0.0, threshold=0.5, iou=0.3, anchors=COCO_V3_ANCHORS, ties=2, box_scale=0.1),
    "v2_96x160": dict(version=2, input_hw=(96, 160), batch=2, classes=80, seed=33, scale=1.0, obj_shift=1.0,
                      cls_boost=6.0, threshold=0.3, iou=0.6, anchors=COCO_V2_ANCHORS, ties=0, box_scale=0.1),
    "v2_160x96": dict(version=2, input_hw=(160, 96), batch=2, classes=80, seed=34, scale=1.0, obj_shift=1.0,
                      cls_boost=6.0, threshold=0.3, iou=0.6, anchors=COCO_V2_ANCHORS, ties=0, box_scale=0.1),
}

# class counts of 1, below 16, one more than 16 and above 80 (the decode kernel's 16-lane groups serve "five classes per
# lane" only at 80)
for _i, _nc in enumerate((1, 3, 17, 91)):
    CASES["v3_c%d" % _nc] = dict(version=3, input=160, batch=1, classes=_nc, seed=41 + _i, scale=2.0, obj_shift=-3.0,
                                 cls_boost=0.0, threshold=0.5, iou=0.3, anchors=COCO_V3_ANCHORS, ties=0, box_scale=0.1)
    CASES["v2_c%d" % _nc] = dict(version=2, input=320, batch=1, classes=_nc, seed=55 + _i, scale=1.0, obj_shift=0.0,
                                 cls_boost=6.0, threshold=0.3, iou=0.5, anchors=COCO_V2_ANCHORS, ties=0, box_scale=0.1)

# equal maximal class logits within ONE row (np.argmax returns the first maximum): see class_tie_rows()
CASES["v3_class_ties"] = dict(version=3, input=160, batch=2, classes=80, seed=61, scale=2.0, obj_shift=-4.0,
                              cls_boost=0.0, threshold=0.5, iou=0.6, anchors=COCO_V3_ANCHORS, ties=0, class_ties=True)
# (v2: p = sigmoid(obj) * max softmax, 1/80 on the all-equal row: the threshold lies below that)
CASES["v2_class_ties"] = dict(version=2, input=256, batch=2, classes=80, seed=62, scale=2.0, obj_shift=-6.0,
                              cls_boost=0.0, threshold=0.01, iou=0.6, anchors=COCO_V2_ANCHORS, ties=0, class_ties=True)
# saturated logits: see saturated_rows().  No NaN logits anywhere: the reference orders its candidates with Python's sort,
# and what that does with NaN keys is not a contract worth restating on a GPU.
CASES["v3_saturated"] = dict(version=3, input=160, batch=1, classes=80, seed=71, scale=2.0, obj_shift=-4.0,
                             cls_boost=0.0, threshold=0.5, iou=0.6, anchors=COCO_V3_ANCHORS, ties=0, saturated=True)
CASES["v2_saturated"] = dict(version=2, input=256, batch=1, classes=80, seed=72, scale=1.0, obj_shift=-2.0,
                             cls_boost=6.0, threshold=0.3, iou=0.6, anchors=COCO_V2_ANCHORS, ties=0, saturated=True)

# index pairs of the engineered class ties against the decode kernel's lane layout (class k is read by lane k % 16 of a
# 16-lane group in iteration k // 16): the same lane in different iterations, neighbouring lanes, far lanes
TIE_PAIRS = ((3, 19), (5, 6), (15, 16), (0, 79))


def input_hw(case):
    """(H, W) of the network input: `input_hw`, or the square `input`."""
    c = CASES[case] if isinstance(case, str) else case
    return tuple(c["input_hw"]) if "input_hw" in c else (c["input"], c["input"])


def head_rows(case):
    """Number of (cell, anchor) rows per image and the per-row width."""
    c = CASES[case] if isinstance(case, str) else case
    H, W = input_hw(c)
    if c["version"] == 2:
        return (H // 32) * (W // 32) * (len(c["anchors"]) // 2), 5 + c["classes"]
    return sum((H // s) * (W // s) for s in (32, 16, 8)) * 3, 5 + c["classes"]


def _engineered_rows(c, count):
    """`count` distinct rows per image for the engineered cases, the same in every image (seeded apart from the head's
    own stream, so that the head's draws do not depend on them)."""
    rows, _ = head_rows(c)
    return [int(r) for r in np.random.RandomState(c["seed"] + 1000).choice(rows, size=count, replace=False)]


def class_tie_rows(case):
    """[(row, expected class_idx)] of a class_ties case, per image: row k of the engineered rows carries equal maximal
    class logits at TIE_PAIRS[k]; the last one has ALL classes equal.  Each passes the threshold."""
    c = CASES[case] if isinstance(case, str) else case
    rows = _engineered_rows(c, len(TIE_PAIRS) + 1)
    return [(r, TIE_PAIRS[k][0] if k < len(TIE_PAIRS) else 0) for k, r in enumerate(rows)]


# per engineered row of a saturated case: (objectness, (tx, ty, tw, th), {class: logit}, logit of every other class);
# None keeps the random value.  +-30: sigmoid rounds to 1 / 9e-14; +-104: its exp overflows float32, sigmoid is exactly 1 / 0.
_SATURATED = (
    (30.0, (104.0, -104.0, None, None), {7: 30.0}, -30.0),
    (104.0, (-104.0, 104.0, None, None), {11: 104.0, 12: 104.0}, -104.0),      # two classes tie at prob exactly 1 (v3) / 0.5 (v2)
    (-30.0, (None, None, None, None), {3: 30.0}, -30.0),                        # never a candidate
    (-104.0, (None, None, None, None), {3: 104.0}, -104.0),                     # never a candidate
    (30.0, (None, None, 80.0, 80.0), {20: 30.0}, -30.0),                        # e^80: finite in float32, and as a float32 record
    (104.0, (None, None, -104.0, -104.0), {21: 104.0}, -104.0),                 # w = h = 0
    (30.0, (0.0, 0.0, 100.0, 100.0), {30: 30.0}, -30.0),                        # e^100 overflows: an infinite box ...
    (30.0, (0.5, -0.5, 100.0, 100.0), {31: 30.0}, -30.0),                       # ... and a second one over it
    (30.0, (None, None, None, None), {}, -104.0),                               # every class sigmoid exactly 0 (v3: class 0)
)
SATURATED_INF = (6, 7)      # the two infinite boxes among the engineered rows


def saturated_rows(case):
    """rows of a saturated case, in the order of _SATURATED"""
    c = CASES[case] if isinstance(case, str) else case
    return _engineered_rows(c, len(_SATURATED))


def make_head(case):
    """Seeded head tensor in the reference's layout: v2 [B,g,g,A*(5+C)], v3 [B,rows,5+C]."""
    c = CASES[case] if isinstance(case, str) else case
    rng = np.random.RandomState(c["seed"])
    rows, width = head_rows(c)
    t = (rng.randn(c["batch"], rows, width) * c["scale"]).astype(np.float32)
    t[..., 4] += np.float32(c["obj_shift"])
    if c.get("box_scale"):
        t[..., 0:4] *= np.float32(c["box_scale"])
    if c["cls_boost"]:
        hot = rng.randint(0, c["classes"], size=(c["batch"], rows))
        bi, ri = np.meshgrid(np.arange(c["batch"]), np.arange(rows), indexing="ij")
        t[bi, ri, 5 + hot] += np.float32(c["cls_boost"])
    if c["ties"]:
        # engineered ties: copy the objectness (and for v2 the class logits) of one passing
        # row onto a few others so that several boxes carry bit-identical prob
        for b in range(c["batch"]):
            src = int(np.argmax(t[b, :, 4]))
            dst = rng.choice(rows, size=c["ties"], replace=False)
            for d in dst:
                t[b, d, 4:] = t[b, src, 4:]
    if c.get("class_ties"):
        for k, (r, _) in enumerate(class_tie_rows(c)):
            t[:, r, 4] = np.float32(8.0)
            if k < len(TIE_PAIRS):
                top = t[:, r, 5:].max(axis=-1) + np.float32(1.0)
                for j in TIE_PAIRS[k]:
                    t[:, r, 5 + j] = top
            else:
                t[:, r, 5:] = np.float32(0.5)
    if c.get("saturated"):
        for r, (obj, box, hot, rest) in zip(saturated_rows(c), _SATURATED):
            t[:, r, 4] = np.float32(obj)
            for k, v in enumerate(box):
                if v is not None:
                    t[:, r, k] = np.float32(v)
            t[:, r, 5:] = np.float32(rest)
            for j, v in hot.items():
                t[:, r, 5 + j] = np.float32(v)
    if c["version"] == 2:
        H, W = input_hw(c)
        return t.reshape(c["batch"], H // 32, W // 32, -1)
    return t


# engineered NMS-only cases: list of (x, y, w, h, class_idx, prob), iou threshold
NMS_CASES = {
    "iou_exactly_at_threshold": (
        [(0.5, 0.5, 1.0, 1.0, 0, 0.9), (0.5, 0.25, 1.0, 0.5, 1, 0.8), (3.0, 3.0, 0.5, 0.5, 2, 0.7)], 0.5),
    "iou_just_below_threshold": (
        [(0.5, 0.5, 1.0, 1.0, 0, 0.9), (0.5, 0.25, 1.0, 0.5, 1, 0.8)], 0.5000001),
    "equal_prob_keeps_scan_order": (
        [(0.2, 0.2, 0.1, 0.1, 3, 0.75), (0.8, 0.8, 0.1, 0.1, 4, 0.75), (0.2, 0.2, 0.1, 0.1, 5, 0.75),
         (0.5, 0.5, 0.1, 0.1, 6, 0.75)], 0.6),
    "zero_area_union_floor": (
        [(0.5, 0.5, 0.0, 0.0, 0, 0.9), (0.5, 0.5, 0.0, 0.0, 1, 0.8)], 0.6),
    "chain_suppression": (
        [(0.50, 0.5, 0.4, 0.4, 0, 0.95), (0.60, 0.5, 0.4, 0.4, 0, 0.90), (0.70, 0.5, 0.4, 0.4, 0, 0.85),
         (0.80, 0.5, 0.4, 0.4, 0, 0.80), (0.90, 0.5, 0.4, 0.4, 0, 0.75)], 0.5),
    "single": ([(0.3, 0.3, 0.2, 0.2, 7, 0.6)], 0.6),
    "empty": ([], 0.6),
}

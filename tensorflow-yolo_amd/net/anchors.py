"""Anchor mode: k-means over the (w, h) of a dataset's boxes on the device (include/yolo_hip.h "Anchor k-means on the device").

Counterpart of the reference's `generate_anchors` (net/v2.py:299-323) and `run_kmeans` (net/base.py:49-52): the same data, the same
`num_anchors` / `tolerate` / `stride` keys, sklearn's defaults (n_init 10, max_iter 300, Euclidean distance) -- as a solver whose answer is
the same bits on every call (`seed`), with the distance 1 - IoU as an option.  Opt-in: `kmeans = device` in [ANCHOR]; without the key anchor
mode is what it was, not supported.
"""
import collections
import os
import xml.etree.ElementTree as ET

import numpy as np

from .. import _hip
from . import engine

NOT_SUPPORTED = "anchor mode is not supported by the HIP inference backend"
SCALES = {"v3": 3, "v3-spp": 3, "v3-tiny": 2}        # detection scales of the v3 family: num_anchors is split evenly over them

AnchorResult = collections.namedtuple("AnchorResult", [
    "anchors",          # float64 [k, 2]: the best restart's centres (w, h), normalised, ascending by area
    "labels",           # int32 [n]: the cluster of every box in that order; -1: a box that was skipped
    "counts",           # int64 [k]
    "avg_iou",          # mean over the boxes used of the best IoU with an anchor
    "inertia",          # sum of the distances of the final assignment (floor(d * 2^40) each, times 2^-40)
    "n_iter",           # iterations of the best restart
    "best_restart", "n_valid", "n_bad", "status", "distance",
    "restarts",         # per restart: dict(n_iter, status, inertia_q, iou_q, seeds)
    "raw"])             # the whole result as engine.anchor_result gives it


def anchor_option(params):
    """The [ANCHOR] key `kmeans`: absent -> False (anchor mode keeps raising), `device` -> True, anything else raises ValueError."""
    raw = params.get("kmeans")
    if raw is None:
        return False
    if str(raw).strip().lower() != "device":
        raise ValueError("kmeans must be device (the k-means kernels), got %r" % (raw,))
    return True


def distinct_boxes(wh):
    """How many different valid boxes the library will see: rows of rint(v * 2^40) with both values in 1 .. 2^40"""
    wh = np.asarray(wh, dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        ok = (np.isfinite(wh) & (wh > 0.0) & (wh <= 1.0)).all(axis=1)
    q = np.rint(wh[ok] * float(2 ** 40)).astype(np.int64)
    q = q[(q >= 1).all(axis=1)]
    return len(np.unique(q, axis=0)) if len(q) else 0


def check_params(params, version, wh=None):
    """What anchor mode refuses, naming the problem before anything touches the device: a `distance` that is neither euclidean nor iou;
    `num_anchors` below 1 or above 32; for the v3 family a `num_anchors` that is no multiple of the scale count (3; v3-tiny: 2); n_init,
    max_iter and tolerate outside the library's ranges; with `wh` (the boxes) fewer distinct boxes than num_anchors.
    -> dict(k, distance, tolerate, n_init, max_iter, seed) parsed"""
    out = {"distance": _hip.anchor_distance(params.get("distance", "euclidean"))}
    k = out["k"] = int(params["num_anchors"])
    if k < 1 or k > _hip.ANCHOR_MAX_K:
        raise ValueError("num_anchors must be 1 .. %d, got %d" % (_hip.ANCHOR_MAX_K, k))
    scales = SCALES.get(str(version))
    if scales and k % scales:
        raise ValueError("num_anchors must be a multiple of %d for a %s network (%d detection scales share them evenly), got %d"
                         % (scales, version, scales, k))
    out["tolerate"] = float(params.get("tolerate", 0.005))
    if not 0 <= out["tolerate"] < float("inf"):
        raise ValueError("tolerate must be finite and not negative, got %s" % params.get("tolerate"))
    out["n_init"] = int(params.get("n_init", 10))
    if not 1 <= out["n_init"] <= _hip.ANCHOR_MAX_INIT:
        raise ValueError("n_init must be 1 .. %d, got %d" % (_hip.ANCHOR_MAX_INIT, out["n_init"]))
    out["max_iter"] = int(params.get("max_iter", 300))
    if not 1 <= out["max_iter"] <= _hip.ANCHOR_ITER_LIMIT:
        raise ValueError("max_iter must be 1 .. %d, got %d" % (_hip.ANCHOR_ITER_LIMIT, out["max_iter"]))
    out["seed"] = int(params.get("seed", 0))
    if wh is not None:
        n = len(np.asarray(wh).reshape(-1, 2))
        if n < 1 or n > _hip.ANCHOR_MAX_N:
            raise ValueError("anchor k-means takes 1 .. %d boxes, got %d" % (_hip.ANCHOR_MAX_N, n))
        d = distinct_boxes(wh)
        if d < k:
            raise ValueError("num_anchors = %d needs at least as many distinct boxes, the data hold %d" % (k, d))
    return out


def read_box_sizes(annotation_dir):
    """The data of the reference's generate_anchors: every .xml of the directory, sorted by file name, every object in file order, its
    (w, h) = (xmax / width - xmin / width, ymax / height - ymin / height) in float64 -- the reference's own arithmetic
    (net/base.py:91-93, net/v2.py:315-316).  -> (float64 [n, 2], the set of class names seen)"""
    files = sorted(f for f in os.listdir(annotation_dir) if f.lower().endswith(".xml"))
    data, names = [], set()
    for f in files:
        root = ET.parse(os.path.join(annotation_dir, f)).getroot()
        size = root.find("size")
        width, height = int(size.find("width").text), int(size.find("height").text)
        for obj in root.findall("object"):
            box = obj.find("bndbox")
            x1, y1 = int(box.find("xmin").text), int(box.find("ymin").text)
            x2, y2 = int(box.find("xmax").text), int(box.find("ymax").text)
            x1, x2 = x1 / width, x2 / width
            y1, y2 = y1 / height, y2 / height
            data.append([float(x2 - x1), float(y2 - y1)])
            names.add(obj.find("name").text)
    return np.asarray(data, dtype=np.float64).reshape(-1, 2), names


def kmeans_anchors(wh, k, distance="euclidean", tolerate=0.005, n_init=10, max_iter=300, seed=0, init=None, device=None):
    """k-means over normalised (w, h) on the device -> AnchorResult.  wh: array-like [n, 2] (or a float64 device tensor); distance:
    "euclidean" (the reference) | "iou" (1 - IoU); init: [k, 2] starting centres (one restart from them) or None (seeded k-means++, n_init
    restarts); device: a torch device, default the current one.  The call synchronises with the host.  A result whose status has
    ANCHOR_DEGENERATE holds no anchors (fewer distinct boxes than k)."""
    torch = engine._torch()
    dist = distance if isinstance(distance, int) else _hip.anchor_distance(distance)
    if torch.is_tensor(wh):
        x = wh.to(dtype=torch.float64).contiguous()
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(wh, dtype=np.float64).reshape(-1, 2))).to(dev)
    c0 = None
    if init is not None:
        c0 = torch.from_numpy(np.ascontiguousarray(np.asarray(init, dtype=np.float64).reshape(int(k), 2))).to(x.device)
        n_init = 1
    res, labels = engine.anchor_kmeans(x, k, dist, tolerate, n_init, max_iter, seed, init=c0)
    best = res["best_restart"]
    return AnchorResult(anchors=res["centres"][:int(k)].copy(), labels=labels.cpu().numpy(), counts=res["counts"][:int(k)].copy(),
                        avg_iou=res["avg_iou"], inertia=res["inertia"], n_iter=res["restarts"][best]["n_iter"] if best >= 0 else 0,
                        best_restart=best, n_valid=res["n_valid"], n_bad=res["n_bad"], status=res["status"], distance=dist,
                        restarts=res["restarts"], raw=res)


def scale_anchors(anchors, params, version):
    """Normalised centres -> the unit the network's .ini takes: v2 / v2-tiny grid cells, a_w * input_w / stride and a_h * input_h / stride
    (net/v2.py:320); the v3 family network pixels, a_w * input_w and a_h * input_h (the unit of yolov3-coco.anchors).  -> flat float64"""
    input_w, input_h = int(params["input_w"]), int(params["input_h"])
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 2)
    if str(version).startswith("v3"):
        out = [[c[0] * input_w, c[1] * input_h] for c in a]
    else:
        stride = int(params["stride"])
        out = [[c[0] * input_w / stride, c[1] * input_h / stride] for c in a]
    return np.reshape(out, [-1])


def generate_anchors(params, version):
    """The reference's generate_anchors on the device -> (anchors flat float64 in the network's unit, ascending by area; class names as a
    sorted list; the AnchorResult).  Raises what check_params raises; without `kmeans = device` NotImplementedError, as before."""
    if not anchor_option(params):
        raise NotImplementedError(NOT_SUPPORTED)
    opts = check_params(params, version)
    wh, names = read_box_sizes(params["annotation_dir"])
    print("{} boxes found.".format(len(wh)))
    check_params(params, version, wh)
    res = kmeans_anchors(wh, opts["k"], opts["distance"], opts["tolerate"], opts["n_init"], opts["max_iter"], opts["seed"])
    if res.status & _hip.ANCHOR_DEGENERATE:
        raise ValueError("num_anchors = %d: every restart ran out of distinct boxes while seeding" % opts["k"])
    return scale_anchors(res.anchors, params, version), sorted(names), res

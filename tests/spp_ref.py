"""Test helper for YOLOv3-SPP / YOLOv3-tiny: a max-pool reference that covers the odd stride-1 SAME windows of the SPP block, and the
oracle-style layer lists of the two nets (the tuples of oracle/topology.py; neither net is in the reference, both are upstream Darknet
cfgs -- yolov3-spp.cfg, yolov3-tiny.cfg -- written in its layer vocabulary).

oracle/forward_ref._maxpool is the k = 2 form (it pads only after the map); tests install `maxpool` below in its place for their duration
with `monkeypatch.setattr(forward_ref, "_maxpool", spp_ref.maxpool)` -- forward() looks the name up at call time.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import forward_ref

_maxpool_k2 = forward_ref._maxpool      # the original, whatever a test patches in later

TINY_V3_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]      # yolov3-tiny.cfg, pixels, small -> large


def maxpool(x, k, s):
    """net/layers.py:70-81 on an NCHW torch tensor.  Odd k at stride 1: tf.layers.max_pooling2d(padding="SAME") = the window
    [i - k//2, i + k//2] clipped to the map (torch pads with -inf, so padding never wins); everything else: the oracle's own form."""
    if s == 1 and k % 2 == 1:
        return F.max_pool2d(x, k, 1, padding=k // 2)
    return _maxpool_k2(x, k, s)


def maxpool_nhwc(x_nhwc, k, s=1):
    """`maxpool` on a NumPy NHWC array, float32 out."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x_nhwc, np.float32))).permute(0, 3, 1, 2)
    return maxpool(t, k, s).permute(0, 2, 3, 1).contiguous().numpy()


def maxpool_naive(x_nhwc, k):
    """Clipped-window loop in NumPy (stride 1, odd k): the independent statement of SAME pooling."""
    x = np.asarray(x_nhwc)
    n, h, w, c = x.shape
    r = k // 2
    y = np.empty_like(x)
    for i in range(h):
        for j in range(w):
            y[:, i, j, :] = x[:, max(0, i - r):min(h, i + r + 1), max(0, j - r):min(w, j + r + 1), :].max(axis=(1, 2))
    return y


def _darknet53_trunk(L):
    def conv(f, k, s=1):
        L.append(("conv", len(L) - 1, f, k, s, True, "leaky"))

    def block(f):
        conv(f, 1)
        conv(2 * f, 3)
        L.append(("shortcut", len(L) - 1, len(L) - 3))

    conv(32, 3)
    for f, blocks in ((32, 1), (64, 2), (128, 8), (256, 8), (512, 4)):
        conv(2 * f, 3, 2)
        for _ in range(blocks):
            block(f)


def yolov3_spp(anchors_px, num_classes, input_shape=(416, 416, 3)):
    """yolov3-spp.cfg: Darknet-53, then the coarse head with the SPP block behind its third conv."""
    anc = np.reshape(np.asarray(anchors_px), [3, -1, 2])[::-1, :, :]
    L = [("input",) + tuple(input_shape)]
    _darknet53_trunk(L)

    def conv(f, k, bn=True, act="leaky"):
        L.append(("conv", len(L) - 1, f, k, 1, bn, act))

    def finish(a):
        conv(len(a) * (5 + num_classes), 1, bn=False, act="linear")
        L.append(("yolo", len(L) - 1, [tuple(v) for v in a.tolist()]))
        return len(L) - 1

    def head(f, a):
        for _ in range(3):
            conv(f, 1)
            conv(2 * f, 3)
        return finish(a)

    def lateral(f, skip):
        L.append(("route", [len(L) - 4]))
        conv(f, 1)
        L.append(("upsample", len(L) - 1, 2))
        L.append(("route", [len(L) - 1, skip]))

    conv(512, 1)
    conv(1024, 3)
    conv(512, 1)
    x = len(L) - 1
    L.append(("maxpool", x, 5, 1))
    p5 = len(L) - 1
    L.append(("route", [x]))
    L.append(("maxpool", len(L) - 1, 9, 1))
    p9 = len(L) - 1
    L.append(("route", [x]))
    L.append(("maxpool", len(L) - 1, 13, 1))
    p13 = len(L) - 1
    L.append(("route", [p13, p9, p5, x]))
    conv(512, 1)
    conv(1024, 3)
    conv(512, 1)
    conv(1024, 3)
    y1 = finish(anc[0])
    lateral(256, 61 + 1)
    y2 = head(256, anc[1])
    lateral(128, 36 + 1)
    y3 = head(128, anc[2])
    L.append(("detection", [y1, y2, y3]))
    return L


def yolov3_tiny(anchors_px, num_classes, input_shape=(416, 416, 3)):
    """yolov3-tiny.cfg (Darknet layer d = list entry d + 1); anchors 3, 4, 5 to the stride-32 head, 0, 1, 2 to the stride-16 head."""
    anc = np.reshape(np.asarray(anchors_px), [2, -1, 2])[::-1, :, :]
    L = [("input",) + tuple(input_shape)]

    def conv(f, k, bn=True, act="leaky"):
        L.append(("conv", len(L) - 1, f, k, 1, bn, act))

    def finish(a):
        conv(len(a) * (5 + num_classes), 1, bn=False, act="linear")
        L.append(("yolo", len(L) - 1, [tuple(v) for v in a.tolist()]))
        return len(L) - 1

    for f in (16, 32, 64, 128, 256):
        conv(f, 3)
        L.append(("maxpool", len(L) - 1, 2, 2))
    conv(512, 3)
    L.append(("maxpool", len(L) - 1, 2, 1))
    conv(1024, 3)
    conv(256, 1)
    conv(512, 3)
    y1 = finish(anc[0])
    L.append(("route", [13 + 1]))
    conv(128, 1)
    L.append(("upsample", len(L) - 1, 2))
    L.append(("route", [len(L) - 1, 8 + 1]))
    conv(256, 3)
    y2 = finish(anc[1])
    L.append(("detection", [y1, y2]))
    return L


def conv_weight_count(L, shapes):
    """sum over convs of k^2 Cin Cout + (4 if BN else 1) Cout, from the tuples alone"""
    n = 0
    for op in L:
        if op[0] == "conv":
            _, src, f, k, _, bn, _ = op
            n += k * k * shapes[src][2] * f + (4 if bn else 1) * f
    return n

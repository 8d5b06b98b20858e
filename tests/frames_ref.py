"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the frame entries (yolo_letterbox_geometry, yolo_preprocess_frames[_u8],
yolo_boxes_to_frames): integer geometry, the letterboxed / stretched network input built from oracle.preprocess_ref.resize_linear_u8,
and the float64 map of box records back to frame coordinates.  Everything that compares against this file uses np.array_equal."""
import numpy as np

from oracle import preprocess_ref

STRETCH, LETTERBOX = 0, 1
CANVAS = 128


def geometry(h, w, H, W, mode):
    """(new_h, new_w, off_y, off_x) of an h x w frame in an H x W network input; Python integers are exact"""
    new_h, new_w = H, W
    if mode == LETTERBOX:
        if W * h < H * w:                       # the width binds
            new_h = max(1, (h * W) // w)
        else:
            new_w = max(1, (w * H) // h)
    return new_h, new_w, (H - new_h) // 2, (W - new_w) // 2


def resized_u8(img, H, W, mode, swap_rb=False):
    """uint8 [h, w, 3] -> uint8 [H, W, 3]: the project's 8-bit INTER_LINEAR resize to (new_h, new_w) pasted at the offsets of a canvas
    of 128 (stretch: the resize fills the canvas)"""
    img = np.asarray(img, dtype=np.uint8)
    if swap_rb:
        img = img[:, :, ::-1]
    new_h, new_w, oy, ox = geometry(img.shape[0], img.shape[1], H, W, mode)
    out = np.full((H, W, 3), CANVAS, dtype=np.uint8)
    out[oy:oy + new_h, ox:ox + new_w] = preprocess_ref.resize_linear_u8(img, new_h, new_w)
    return out


def letterbox_u8(img, H, W):
    return resized_u8(img, H, W, LETTERBOX)


def to_f32(u):
    """a byte as the network sees it: float32(u / 255.), the division in float64"""
    return (np.asarray(u).astype(np.float64) / 255.).astype(np.float32)


def remap(xywh, h, w, H, W, mode):
    """float32 [n, 4] (x, y, w, h normalised to the network input) -> float32 [n, 4] normalised to the frame: float64 arithmetic, one
    rounding to float32 each.  Stretch returns the input."""
    b = np.asarray(xywh, dtype=np.float32)
    if mode == STRETCH:
        return b.copy()
    new_h, new_w, oy, ox = geometry(h, w, H, W, mode)
    d = b.astype(np.float64)
    out = np.empty_like(b)
    out[:, 0] = ((d[:, 0] * np.float64(W) - np.float64(ox)) / np.float64(new_w)).astype(np.float32)
    out[:, 1] = ((d[:, 1] * np.float64(H) - np.float64(oy)) / np.float64(new_h)).astype(np.float32)
    out[:, 2] = (d[:, 2] * np.float64(W) / np.float64(new_w)).astype(np.float32)
    out[:, 3] = (d[:, 3] * np.float64(H) / np.float64(new_h)).astype(np.float32)
    return out

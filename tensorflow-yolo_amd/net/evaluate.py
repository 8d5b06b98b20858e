"""VOC-style evaluation on the device: `Evaluator` over the yolo_eval_* entries of libyolo_hip (include/yolo_hip.h has the definitions),
and the annotation reader that feeds it.

No counterpart in the reference beyond its annotation parser (net/base.py:69-97): it never scores a detector.  The detections stay on
the device: `Evaluator.add` takes the record tensors of `HipNetwork.detect*` as they are, in the stream of the step that wrote them.
"""
import ctypes as C
import os
import xml.etree.ElementTree as ET

import numpy as np

from .. import _hip

GT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("w", "f4"), ("h", "f4"), ("class_idx", "i4"), ("difficult", "i4")])
RECORD_DTYPE = np.dtype([("best_iou", "f8"), ("prob", "f4"), ("class_idx", "i4"), ("seq", "u4"), ("verdict", "i4"), ("best_gt", "i4"),
                         ("pad_", "i4")])
CLASS_DTYPE = np.dtype([("ap_voc12", "f8"), ("ap_voc07", "f8"), ("n_gt", "i4"), ("n_det", "i4"), ("tp", "i4"), ("fp", "i4"),
                        ("ignored", "i4"), ("pad_", "i4")])
HEADER_DTYPE = np.dtype([("map_voc12", "f8"), ("map_voc07", "f8"), ("n_records", "i4"), ("status", "i4"), ("n_classes", "i4"), ("pad_", "i4")])
LOSS_IMAGE_DTYPE = np.dtype([("xy", "f8"), ("wh", "f8"), ("obj", "f8"), ("noobj", "f8"), ("cls", "f8"), ("n_assigned", "i4"), ("n_truths", "i4"),
                             ("status", "i4"), ("pad_", "i4")])
LOSS_RESULT_DTYPE = np.dtype([("loss", "f8"), ("loss_xy", "f8"), ("loss_wh", "f8"), ("loss_obj", "f8"), ("loss_noobj", "f8"), ("loss_class", "f8"),
                              ("n_assigned", "i4"), ("n_truths", "i4"), ("status", "i4"), ("pad_", "i4")])
LOSS_KEYS = ("loss", "loss_xy", "loss_wh", "loss_obj", "loss_noobj", "loss_class")
LOSS_STATUS_NAMES = ((_hip.LOSS_OUT_OF_GRID, "out_of_grid"), (_hip.LOSS_BAD_BOX, "bad_box"), (_hip.LOSS_BAD_CLASS, "bad_class"),
                     (_hip.LOSS_BAD_COUNT, "bad_count"))
DEFAULT_MAX_GT = 256
STATUS_NAMES = ((_hip.EVAL_OVERFLOW, "overflow"), (_hip.EVAL_UNSORTED, "unsorted"), (_hip.EVAL_BAD_CLASS, "bad_class"),
                (_hip.EVAL_BAD_COUNT, "bad_count"))


def eval_desc(n_classes, det_capacity, max_gt, match_iou):
    return _hip.EvalDesc(int(n_classes), int(det_capacity), int(max_gt), 0, float(match_iou))


def pack_gts(gts, max_gt):
    """list per image of (x, y, w, h, class_idx, difficult) -> (GT_DTYPE array [B, max_gt], int32 counts [B]); more than max_gt raises"""
    arr = np.zeros((len(gts), int(max_gt)), dtype=GT_DTYPE)
    counts = np.zeros(len(gts), dtype=np.int32)
    for i, img in enumerate(gts):
        if len(img) > max_gt:
            raise ValueError("image %d has %d truths, max_gt is %d" % (i, len(img), max_gt))
        counts[i] = len(img)
        for g, t in enumerate(img):
            arr[i, g] = (t[0], t[1], t[2], t[3], int(t[4]), int(t[5]) if len(t) > 5 else 0)
    return arr, counts


class EvalResult(object):
    """What yolo_eval_finish computed, on the host: per-class arrays (ap_voc12, ap_voc07, n_gt, n_det, tp, fp, ignored), map_voc12,
    map_voc07, n_records, status (yolo_eval_status bits), and the sorted records with their cumulative counts."""

    def __init__(self, header, classes, records, ctp, cfp):
        self.map_voc12, self.map_voc07 = float(header["map_voc12"]), float(header["map_voc07"])
        self.n_records, self.status = int(header["n_records"]), int(header["status"])
        for k in ("ap_voc12", "ap_voc07", "n_gt", "n_det", "tp", "fp", "ignored"):
            setattr(self, k, classes[k].copy())
        self.records, self.ctp, self.cfp = records, ctp, cfp

    @property
    def status_names(self):
        return [name for bit, name in STATUS_NAMES if self.status & bit]

    def precision_recall(self, c):
        """(precision, recall) float64 arrays of class c over its records in (prob descending, seq ascending) order, IGNORED ones
        removed: VOCdevkit's curve, from the device's integer scans"""
        sel = (self.records["class_idx"] == c) & (self.records["verdict"] != _hip.EVAL_IGNORED)
        tp, fp = self.ctp[sel].astype(np.float64), self.cfp[sel].astype(np.float64)
        n = float(self.n_gt[c])
        with np.errstate(invalid="ignore", divide="ignore"):
            return tp / np.maximum(tp + fp, np.finfo(np.float64).eps), tp / n

    def to_json(self, class_names=None):
        def num(v):
            return None if np.isnan(v) else float(v)
        names = list(class_names) if class_names is not None else ["%d" % c for c in range(len(self.n_gt))]
        return {"map_voc12": num(self.map_voc12), "map_voc07": num(self.map_voc07), "n_records": self.n_records, "status": self.status,
                "status_names": self.status_names,
                "classes": [{"name": names[c], "ap_voc12": num(self.ap_voc12[c]), "ap_voc07": num(self.ap_voc07[c]),
                             "n_gt": int(self.n_gt[c]), "n_det": int(self.n_det[c]), "tp": int(self.tp[c]), "fp": int(self.fp[c]),
                             "ignored": int(self.ignored[c])} for c in range(len(self.n_gt))]}


class Evaluator(object):
    """Accumulates the detections of a dataset on the device and scores them.

        ev = Evaluator(n_classes)
        for each step:  boxes, counts, status = engine.detect*(...);  ev.add(boxes, counts, gts, status)
        result = ev.finish()

    match_iou is compared STRICTLY (`best_iou > match_iou`), as VOCdevkit and Darknet's `detector map` do -- unlike NMS, which
    suppresses at `>=` (net/base.py:204)."""

    def __init__(self, n_classes, det_capacity=1 << 18, max_gt=DEFAULT_MAX_GT, match_iou=0.5, device=None):
        import torch
        self.torch = torch
        self.lib = _hip.lib()
        self.desc = eval_desc(n_classes, det_capacity, max_gt, match_iou)
        self.n_classes, self.det_capacity, self.max_gt = int(n_classes), int(det_capacity), int(max_gt)
        nbytes = self.lib.yolo_eval_state_bytes(C.byref(self.desc))
        if not nbytes:
            raise _hip.YoloHipError((self.lib.yolo_last_error() or b"").decode())
        self.layout = _hip.EvalLayout()
        _hip.check(self.lib.yolo_eval_state_layout(C.byref(self.desc), C.byref(self.layout)), "yolo_eval_state_layout")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.result = torch.zeros(self.lib.yolo_eval_result_bytes(C.byref(self.desc)), dtype=torch.uint8, device=self.device)
        self.reset()

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def reset(self):
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_eval_reset(C.byref(self.desc), self.state.data_ptr(), self.state.numel(), self._stream()), "yolo_eval_reset")
            self._truncated = self.torch.zeros(1, dtype=self.torch.int64, device=self.device)
        self.n_images = 0
        self._keep = None

    def upload_gts(self, gts):
        """The truths of a whole dataset (a list per image, or the pair of pack_gts) -> (uint8 [N, max_gt * 24], int32 [N]) on the
        device, packed and copied ONCE; `add` takes the slices [lo:hi] of both."""
        torch = self.torch
        arr, gcounts = gts if isinstance(gts, tuple) else pack_gts(gts, self.max_gt)
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(len(gcounts), -1)
        return torch.from_numpy(raw).to(self.device), torch.from_numpy(np.ascontiguousarray(gcounts, dtype=np.int32)).to(self.device)

    def add(self, boxes, counts, gts, status=None):
        """One step.  boxes [B, max_boxes, 6] float32 and counts [B] int32: the device tensors of HipNetwork.detect* (or host arrays of
        that shape).  gts: the step's slice of what `upload_gts` returned -- truths already on the device, and then nothing here
        touches the host's data or waits for the GPU: the match kernel is enqueued behind the step that wrote the records.  Or, for
        convenience, a list per image of (x, y, w, h, class_idx, difficult) normalised like the boxes, or the pair of host arrays of
        pack_gts: these are packed in a Python loop and copied from pageable memory on every call, which holds the host up until
        the copy is staged -- fine for a test, not for a loop that should keep the GPU busy.  status: the detect call's status tensor;
        images whose list was truncated (bit 1) are counted (`images_truncated`), on the device."""
        torch = self.torch
        if not isinstance(boxes, torch.Tensor):
            boxes = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32))
        if not isinstance(counts, torch.Tensor):
            counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32))
        boxes = boxes.to(self.device).contiguous()
        counts = counts.to(device=self.device, dtype=torch.int32).contiguous()
        if boxes.dim() != 3 or boxes.shape[2] != 6 or boxes.dtype != torch.float32 or counts.numel() != boxes.shape[0]:
            raise ValueError("expected boxes [B, max_boxes, 6] float32 and counts [B]")
        batch, max_boxes = int(boxes.shape[0]), int(boxes.shape[1])
        if isinstance(gts, tuple) and isinstance(gts[0], torch.Tensor):
            gt_dev, gc_dev = gts
            if (gt_dev.device != self.device or gc_dev.device != self.device or gt_dev.dtype != torch.uint8 or gc_dev.dtype != torch.int32
                    or tuple(gt_dev.shape) != (batch, self.max_gt * GT_DTYPE.itemsize) or tuple(gc_dev.shape) != (batch,)
                    or not gt_dev.is_contiguous() or not gc_dev.is_contiguous()):
                raise ValueError("expected the [%d] slice of upload_gts" % batch)
        else:
            arr, gcounts = gts if isinstance(gts, tuple) else pack_gts(gts, self.max_gt)
            if arr.shape != (batch, self.max_gt) or arr.dtype != GT_DTYPE or len(gcounts) != batch:
                raise ValueError("expected truths [%d, %d] of GT_DTYPE with %d counts" % (batch, self.max_gt, batch))
            gt_dev, gc_dev = self.upload_gts((arr, gcounts))
        with torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_eval_add(C.byref(self.desc), self.state.data_ptr(), boxes.data_ptr(), counts.data_ptr(), batch, max_boxes,
                                              gt_dev.data_ptr(), gc_dev.data_ptr(), self.n_images, self._stream()), "yolo_eval_add")
            if status is not None:
                self._truncated += ((status.to(self.device) & 2) != 0).sum()
        self._keep = (boxes, counts, gt_dev, gc_dev)       # (alive until the next call: the work is only enqueued)
        self.n_images += batch

    @property
    def images_truncated(self):
        return int(self._truncated.item())

    def _part(self, offset, dtype, n):
        return self.state[int(offset):int(offset) + n * np.dtype(dtype).itemsize].cpu().numpy().view(dtype)

    def records(self, n=None):
        """the records in ARRIVAL order (before or after finish)"""
        if n is None:
            self.torch.cuda.synchronize(self.device)
            cursor = int(self.state[:8].cpu().numpy().view(np.uint64)[0])
            n = min(cursor, self.det_capacity)
        return self._part(self.layout.records_offset, RECORD_DTYPE, n)

    def finish(self):
        """sort + scans + AP on the device, then the result block and the sorted records to the host"""
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_eval_finish(C.byref(self.desc), self.state.data_ptr(), self.result.data_ptr(), self._stream()), "yolo_eval_finish")
        raw = self.result.cpu().numpy()
        header = raw[:HEADER_DTYPE.itemsize].view(HEADER_DTYPE)[0]
        classes = raw[HEADER_DTYPE.itemsize:].view(CLASS_DTYPE)
        n = int(header["n_records"])
        return EvalResult(header, classes, self._part(self.layout.sorted_offset, RECORD_DTYPE, n),
                          self._part(self.layout.ctp_offset, np.uint32, n), self._part(self.layout.cfp_offset, np.uint32, n))


def loss_option(params, version):
    """The optional [EVAL] key `loss` (true | false, default false): also report the reference's validation loss.  Checked before a
    network is built: it needs a YOLOv2 head (the reference binds no loss to v3) and the stretch resize (under letterbox the truths
    would have to be mapped into the canvas, which is not built); anything else raises ValueError."""
    raw = str(params.get("loss", "false")).strip().lower()
    if raw not in ("true", "false"):
        raise ValueError("loss must be true or false, got %r" % (params.get("loss"),))
    if raw == "false":
        return False
    if not str(version).startswith("v2"):
        raise ValueError("loss = true needs a YOLOv2 network (version v2 or v2-tiny), got %s: the reference has a loss for YOLOv2 only" % version)
    if _hip.resize_mode(params.get("resize", "stretch")) != _hip.RESIZE_STRETCH:
        raise ValueError("loss = true needs resize = stretch: letterboxed truths are not built")
    return True


def loss_batches(n_images, batch_size):
    """How the reference's make_batch (net/v2.py:209-217) groups a set of n_images annotations: (bs, n_batches, pad) -- the batch shrinks
    to the set if the set is smaller, and the last batch is filled with the first `pad` annotations of the set."""
    n, bs = int(n_images), int(batch_size)
    if n < 1 or bs < 1:
        raise ValueError("n_images and batch_size must be at least 1")
    bs = min(bs, n)
    nb = -(-n // bs)
    return bs, nb, nb * bs - n


def validation_loss(partials, batch_size):
    """The reference's `validation loss` (net/yolo.py:177-193) from the per-image partials (LOSS_IMAGE_DTYPE array, one record per
    annotated image in set order): the mean over the batches of make_batch of the batch loss.  With (bs, nb, pad) = loss_batches and
    S_t = sum of term t over ALL records in index order, then over the first `pad` records once more,

        loss_xy = S_xy / bs / nb     loss_wh = S_wh / bs / nb     loss_obj = 5 S_obj / bs / nb     loss_noobj = S_noobj / bs / nb
        loss_class = S_cls / nb      validation_loss = (loss_xy + loss_wh + loss_obj + loss_noobj + loss_class as of one batch) / nb

    Four terms are divided by the batch and the class term is not, in every batch alike, so the result does not depend on how the
    images are grouped: make_batch's shuffle needs no counterpart.  The host mirror of yolo_loss_reduce followed by the division by nb
    (Yolo.evaluate runs that on the device).  Returns a dict of the six LOSS_KEYS."""
    bs, nb, pad = loss_batches(len(partials), batch_size)
    s = {k: 0.0 for k in ("xy", "wh", "obj", "noobj", "cls")}
    for rec in list(partials) + list(partials[:pad]):
        for k in s:
            s[k] += float(rec[k])
    one = {"loss_xy": s["xy"] / bs, "loss_wh": s["wh"] / bs, "loss_obj": 5. * s["obj"] / bs, "loss_noobj": s["noobj"] / bs, "loss_class": s["cls"]}
    one["loss"] = one["loss_xy"] + one["loss_wh"] + one["loss_obj"] + one["loss_noobj"] + one["loss_class"]
    return {k: one[k] / nb for k in LOSS_KEYS}


def loss_to_host(images, result):
    """the device tensors of HipNetwork.loss* -> dict: the six totals, n_assigned, n_truths, status, status_names, and `images`, the
    per-image partials as a LOSS_IMAGE_DTYPE array (synchronises)"""
    rec = result.cpu().numpy().view(LOSS_RESULT_DTYPE)[0]
    out = {k: float(rec[k]) for k in LOSS_KEYS}
    out.update(n_assigned=int(rec["n_assigned"]), n_truths=int(rec["n_truths"]), status=int(rec["status"]),
               status_names=[name for bit, name in LOSS_STATUS_NAMES if int(rec["status"]) & bit],
               images=images.cpu().numpy().reshape(-1).view(LOSS_IMAGE_DTYPE).copy())
    return out


def parse_voc_annotations(annotation_dir, image_dir, class_names):
    """The .xml files of annotation_dir (sorted by name) -> (list of (image_path, truths), names_skipped): truths are
    (x, y, w, h, class_idx, difficult) with centre / size normalised by the XML's own <size> width / height -- so they are
    frame-normalised, like the boxes of the frame entries.  Objects whose <name> is not in class_names are skipped and counted per name
    in names_skipped.  Reads filename, size, and per object name, bndbox and difficult (absent: 0)."""
    index = {name: i for i, name in enumerate(class_names)}
    skipped = {}
    out = []
    for fname in sorted(f for f in os.listdir(annotation_dir) if f.lower().endswith(".xml")):
        root = ET.parse(os.path.join(annotation_dir, fname)).getroot()
        size = root.find("size")
        width, height = float(size.findtext("width")), float(size.findtext("height"))
        truths = []
        for obj in root.findall("object"):
            name = (obj.findtext("name") or "").strip()
            if name not in index:
                skipped[name] = skipped.get(name, 0) + 1
                continue
            bb = obj.find("bndbox")
            x1, y1, x2, y2 = (float(bb.findtext(k)) for k in ("xmin", "ymin", "xmax", "ymax"))
            difficult = int((obj.findtext("difficult") or "0").strip() or 0)
            truths.append(((x1 + x2) / 2. / width, (y1 + y2) / 2. / height, (x2 - x1) / width, (y2 - y1) / height, index[name],
                           1 if difficult else 0))
        out.append((os.path.join(image_dir, (root.findtext("filename") or "").strip()), truths))
    return out, skipped

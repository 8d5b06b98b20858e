"""Driver classes of the HIP backend: `Yolo.test(params)` with the reference's parameter keys,
and the factored-out per-batch body `predict(x_batch)`.

Counterpart of the reference's net/yolo.py (TEST path :41-96; binding classes :198-211).
Training (`create_loss_fn`, batches) is out of scope: those entries raise, so does `generate_anchors` unless [ANCHOR] has
`kmeans = device` -- then the anchors come from k-means on the device (net/anchors.py) -- and so does `train` unless [TRAIN] has
`train_layers = head` -- then the detection layer is trained on the device on a frozen backbone (net/train.py).  The loss itself and its
gradient with respect to the head logits exist (`Yolo.loss`, `Yolo.loss_grad`, net/lossfn.py); a backward pass through the rest of the
network does not.
"""
import os

import numpy as np

from .. import _hip
from . import base, dist as ydist, engine, tfckpt, v2, v3


class Yolo(object):
    version = None
    # plug points, bound per version below (same names as the reference)
    create_network = None
    load_weights = None
    find_bounding_boxes = None

    def __init__(self):
        self.net = None
        self.params = None
        self.last_status = None

    # ---- out of scope for an inference backend (train: but for the detection layer) -----------------
    def train(self, params):
        """The reference's loop (net/yolo.py:98-195) for the detection layer on a frozen backbone, only when [TRAIN] has
        `train_layers = head` (a v2 network) or `train_layers = heads` (the detection convs of a v3 network) (net/train.py); without the
        key train mode is what it was: not supported."""
        from . import train as ytrain
        if not ytrain.train_option(params):
            raise NotImplementedError("train mode is not supported by the HIP inference backend")
        ytrain.train_head(self, params)

    def generate_anchors(self, params):
        """The reference's generate_anchors (net/v2.py:299-323) as k-means on the device, only when [ANCHOR] has `kmeans = device`
        (net/anchors.py); without the key anchor mode is what it was: not supported.  -> (anchors in the unit of the network's .ini,
        ascending by area; class names, sorted); the whole result stays in `last_anchor_result`."""
        from . import anchors as yanchors
        if not yanchors.anchor_option(params):
            raise NotImplementedError("anchor mode is not supported by the HIP inference backend")
        anchors, class_names, self.last_anchor_result = yanchors.generate_anchors(params, self.version)
        return anchors, class_names

    def create_loss_fn(self, batch_size, net, anchors, class_names):
        raise NotImplementedError("training is not supported by the HIP inference backend")

    def make_batch(self, net, annotations, batch_size, anchors, class_names, augment_prob):
        raise NotImplementedError("training is not supported by the HIP inference backend")

    def create_train_optimizer(self, loss_fn, learning_rate):
        raise NotImplementedError("training is not supported by the HIP inference backend")

    # ---- network lifecycle ----------------------------------------------------------------------
    def build(self, anchors, class_names, input_shape=(416, 416, 3), dtype="fp32", max_batch=1,
              weights=None, weights_path=None, **engine_kw):
        """create_network + compile for the GPU + load weights (array or Darknet file)."""
        anchors = np.reshape(anchors, [-1, 2])
        self.anchors, self.class_names = anchors, list(class_names)
        net = type(self).create_network(anchors, class_names, False, input_shape=tuple(input_shape))
        net.engine = engine.HipNetwork(net, dtype=dtype, max_batch=max_batch, **engine_kw)
        if not self.version.startswith("v3"):
            h, w, _ = net[-1].out.hwc
            net.engine.set_head(engine.head_desc_v2(h, w, anchors, len(class_names)))
        if weights is not None:
            v3.attach_weights(net, weights)
        elif weights_path is not None:
            type(self).load_weights(net, weights_path)
        self.net = net
        return net

    def predict(self, x_batch, threshold=0.5, iou_threshold=0.6, nms_mode=_hip.NMS_AGNOSTIC, group=None):
        """One batch: forward + decode + NMS on the GPU (the body of the reference's test loop,
        net/yolo.py:83-86).  x_batch: [B,H,W,C] in [0,1], RGB (NumPy or torch).
        Returns list[B] of list[BoundingBox], each in descending-prob (stable) order.

        Under an initialised `torch.distributed` group of W > 1 ranks (one process per GPU) every rank passes the SAME
        global batch: rank r runs images shard_range(B, r, W), the fixed-size box records are all-gathered (the only
        exchange, net/dist.py) and every rank returns the full list.  `self.last_status` keeps the per-image status
        words (bit 0 candidate overflow, bit 1 more survivors than max_boxes): both raise, the reference has no caps."""
        rank, world = ydist.world(group)
        if world > 1:
            lo, hi = ydist.shard_range(len(x_batch), rank, world)
            return self.predict_shard(x_batch[lo:hi] if hi > lo else None, len(x_batch), threshold, iou_threshold, nms_mode, group)
        return self.predict_shard(x_batch, len(x_batch), threshold, iou_threshold, nms_mode, group)

    def predict_u8(self, x_batch_u8, threshold=0.5, iou_threshold=0.6, nms_mode=_hip.NMS_AGNOSTIC, group=None):
        """predict() for a uint8 batch [B,H,W,C] with values 0..255, RGB -- the pixels net/base.py:115-155 has before its `/ 255.`:
        the bytes go to the device as they are (a quarter of the float32 batch) and the first kernel converts.  Returns exactly
        what predict() returns for float32(x_batch_u8 / 255.); sharding as in predict()."""
        rank, world = ydist.world(group)
        if world > 1:
            lo, hi = ydist.shard_range(len(x_batch_u8), rank, world)
            return self.predict_shard(x_batch_u8[lo:hi] if hi > lo else None, len(x_batch_u8), threshold, iou_threshold, nms_mode, group, u8=True)
        return self.predict_shard(x_batch_u8, len(x_batch_u8), threshold, iou_threshold, nms_mode, group, u8=True)

    def predict_frames(self, frames, threshold=0.5, iou_threshold=0.6, nms_mode=_hip.NMS_AGNOSTIC, resize="stretch", group=None):
        """predict() for frames of ANY sizes: a list of uint8 [h, w, 3] RGB arrays or device tensors.  The whole batch is resized on the
        device in one launch -- resize = "stretch" (the reference, net/base.py:121) or "letterbox" (Darknet's `detector test`: aspect
        ratio kept, grey canvas) -- and the boxes come back normalised to each FRAME, so draw_boxes and every other consumer of
        BoundingBox work as they are.  Stretch returns exactly what predict_u8 returns for the frames resized one by one.  Sharding as
        in predict_u8: each rank resizes, runs and maps back its own shard before the one all-gather."""
        mode = _hip.resize_mode(resize)
        eng = self.net.engine
        if not eng.weights_loaded:
            raise RuntimeError("no weights loaded: call load_weights / build(weights=...) first")
        frames = list(frames)
        rank, world = ydist.world(group)
        if world > 1:
            lo, hi = ydist.shard_range(len(frames), rank, world)
            local = frames[lo:hi]
            if not local:
                return self.predict_shard(None, len(frames), threshold, iou_threshold, nms_mode, group, u8=True)
            descs, keep = eng.frame_descs(local)
            x_local = eng.preprocess_frames(descs, len(local), mode, True)
            return self.predict_shard(x_local, len(frames), threshold, iou_threshold, nms_mode, group, u8=True,
                                      after_detect=lambda: eng.boxes_to_frames(descs, len(local), mode))
        boxes, counts, status = eng.detect_frames(frames, threshold, iou_threshold, nms_mode, mode)
        records, self.last_status = engine.records_to_host(boxes, counts, status)
        return base.boxes_from_records(records)

    def predict_shard(self, x_local, n_global, threshold=0.5, iou_threshold=0.6, nms_mode=_hip.NMS_AGNOSTIC, group=None, u8=False,
                      after_detect=None):
        """predict() for a caller that holds only ITS images of the global batch (Yolo.test under torch.distributed
        preprocesses just the rank's shard): x_local = images shard_range(n_global, rank, world) of the batch, or None
        when the shard is empty.  u8: x_local is uint8 0..255 (predict_u8).  after_detect: called behind the local detect, before the
        records leave the device (predict_frames / Yolo.test: boxes to frame coordinates).  Returns the list for all n_global images on
        every rank."""
        eng = self.net.engine
        if not eng.weights_loaded:
            raise RuntimeError("no weights loaded: call load_weights / build(weights=...) first")
        rank, world = ydist.world(group)
        if world > 1:
            n = int(n_global)
            per = -(-n // world)
            if per > eng.max_batch:
                raise ValueError("global batch %d over %d ranks needs max_batch >= %d (engine has %d)" % (n, world, per, eng.max_batch))
            lo, hi = ydist.shard_range(n, rank, world)
            n_local = 0 if x_local is None else len(x_local)
            if n_local != hi - lo:
                raise ValueError("rank %d holds %d images of a global batch of %d, its shard is [%d, %d)" % (rank, n_local, n, lo, hi))
            extra = {"after_detect": after_detect} if after_detect is not None else {}
            if u8:
                boxes, counts, status = ydist.detect_sharded(eng, x_local if n_local else None, threshold, iou_threshold, nms_mode, group, u8=True, **extra)
            else:
                boxes, counts, status = ydist.detect_sharded(eng, x_local if n_local else None, threshold, iou_threshold, nms_mode, group, **extra)
            keep = [r * eng.max_batch + i for r in range(world) for i in range(per)][:n]     # slot of global image g
            status = status.cpu().numpy().reshape(-1)[keep]
            self.last_status = status
            engine.check_status(status)
            lists = ydist.records_to_lists(boxes, counts)
            return base.boxes_from_records([lists[k] for k in keep])
        boxes, counts, status = (eng.detect_u8 if u8 else eng.detect)(x_local, threshold, iou_threshold, nms_mode)
        if after_detect is not None:
            after_detect()
        records, self.last_status = engine.records_to_host(boxes, counts, status)
        return base.boxes_from_records(records)

    def forward(self, x_batch):
        """Head logits as a NumPy float32 array in the reference's layout (what sess.run returns)."""
        return self.net.engine.forward(x_batch).cpu().numpy()

    def forward_u8(self, x_batch_u8):
        """forward() for a uint8 batch (0..255): the same array as forward(float32(x_batch_u8 / 255.))."""
        return self.net.engine.forward_u8(x_batch_u8).cpu().numpy()

    def loss(self, x_batch, truths):
        """The YOLOv2 loss of one batch, forward only (net/v2.py:123-198 create_loss_fn over net/v2.py:242-295; include/yolo_hip.h has
        the definition): a dense forward pass and the loss kernels in one enqueue.  x_batch: [B,H,W,C] float in [0,1], or uint8 0..255;
        truths: a list per image of (x, y, w, h, class_idx) normalised to the image, the pair of evaluate.pack_gts, or the device
        tensors of Evaluator.upload_gts.  Returns a dict: loss, loss_xy, loss_wh, loss_obj, loss_noobj, loss_class, n_assigned, n_truths,
        status, status_names and `images`, the per-image partial sums.  The create_loss_fn / make_batch stubs above stay: a TensorFlow
        graph and its placeholders cannot be mirrored."""
        from . import evaluate as yeval
        eng = self.net.engine
        if not eng.weights_loaded:
            raise RuntimeError("no weights loaded: call load_weights / build(weights=...) first")
        images, result = (eng.loss_u8 if eng.is_u8(x_batch) else eng.loss)(x_batch, truths)
        return yeval.loss_to_host(images, result)

    def loss_grad(self, x_batch, truths):
        """loss() and the gradient of that loss with respect to the head logits (tf.gradients of net/v2.py:188 with respect to
        net[-1].out; include/yolo_hip.h has the definition): a dense forward pass, the loss kernels and the gradient kernel on one
        stream.  Arguments as loss().  Returns loss()'s dict plus `grad`, a float32 DEVICE tensor [B, h, w, A * (5 + C)].  The gradient
        stops at the logits: there is no backward pass through the network here."""
        from . import evaluate as yeval
        eng = self.net.engine
        if not eng.weights_loaded:
            raise RuntimeError("no weights loaded: call load_weights / build(weights=...) first")
        images, result, _, grad = (eng.loss_grad_u8 if eng.is_u8(x_batch) else eng.loss_grad)(x_batch, truths)
        out = yeval.loss_to_host(images, result)
        out["grad"] = grad
        return out

    def loss_v3(self, x_batch, truths, ignore_thresh=0.7):
        """The YOLOv3 loss of one batch, forward only: the loss of Darknet's [yolo] layer (include/yolo_hip.h has the definition; the
        reference binds no loss to YoloV3).  Arguments and the returned dict as loss(); ignore_thresh: a row whose decoded box overlaps
        a truth by more than this pays no objectness penalty.  ValueError on a YOLOv2 network."""
        from . import evaluate as yeval
        eng = self.net.engine
        if not eng.weights_loaded:
            raise RuntimeError("no weights loaded: call load_weights / build(weights=...) first")
        images, result, _ = (eng.loss_v3_u8 if eng.is_u8(x_batch) else eng.loss_v3)(x_batch, truths, ignore_thresh)
        return yeval.loss_to_host(images, result)

    def loss_v3_grad(self, x_batch, truths, ignore_thresh=0.7):
        """loss_v3() and the gradient of that loss with respect to the head logits.  Returns loss_v3()'s dict plus `grad`, a float32 DEVICE
        tensor [B, R, 5 + C].  The gradient stops at the logits: there is no backward pass through the network here."""
        from . import evaluate as yeval
        eng = self.net.engine
        if not eng.weights_loaded:
            raise RuntimeError("no weights loaded: call load_weights / build(weights=...) first")
        images, result, _, grad = (eng.loss_v3_grad_u8 if eng.is_u8(x_batch) else eng.loss_v3_grad)(x_batch, truths, ignore_thresh)
        out = yeval.loss_to_host(images, result)
        out["grad"] = grad
        return out

    # ---- TEST mode --------------------------------------------------------------------------------
    def test(self, params):
        image_dir = params["image_dir"]
        out_dir = params["out_dir"]
        batch_size = int(params["batch_size"])
        threshold = float(params["threshold"])
        iou_threshold = float(params["iou_threshold"])
        anchors = np.reshape(params["anchors"], [-1, 2])
        class_names = params["class_names"]
        input_shape = (int(params["input_h"]), int(params["input_w"]), int(params["input_c"]))
        checkpoint_path = params.get("checkpoint_path", "")
        pretrained_weights_path = params["pretrained_weights_path"]
        cpu_only = str(params.get("cpu_only", "false")).lower() == "true"
        dtype = params.get("dtype", "fp32")                 # new optional key; fp32 == the reference's arithmetic
        nms_mode = {"agnostic": _hip.NMS_AGNOSTIC, "per_class": _hip.NMS_PER_CLASS}[params.get("nms_mode", "agnostic")]

        image_paths = base.load_image_paths(image_dir)
        if len(image_paths) == 0:
            print("No test images found in {}".format(image_dir))
            return
        if cpu_only:
            print("cpu_only = True is ignored: this backend runs on the MI355X only")

        # one process per GPU (torch.distributed initialised by the launcher, e.g. torchrun): every batch of `batch_size`
        # images shards over the ranks, the box records are all-gathered, rank 0 draws and writes (net/dist.py)
        rank, world = ydist.world()
        # the reference's box lists are unbounded (net/base.py:195-209); the record buffers are not: optional keys raise the caps
        caps = {k: int(params[k]) for k in ("max_boxes", "cand_capacity") if k in params}
        self.build(anchors, class_names, input_shape, dtype=dtype, max_batch=-(-batch_size // world), **caps)
        # same order as the reference (net/yolo.py:71-78, net/base.py:55-61): restore the TensorFlow checkpoint (read without
        # TensorFlow by net/tfckpt.py); when that fails, say so and load the Darknet weights
        restored = False
        if checkpoint_path:
            try:
                v3.attach_weights(self.net, tfckpt.checkpoint_to_darknet(self.net, checkpoint_path))
                restored = True
                print("Checkpoint {} restored.".format(checkpoint_path))
            except Exception as e:
                print("Failed to load {}: {}".format(checkpoint_path, str(e)))
        if not restored:
            type(self).load_weights(self.net, pretrained_weights_path)
            print("Pre-trained weights loaded.")

        if str(params.get("autotune", "false")).lower() == "true":      # new optional key: time every conv tile per layer once, on a
            eng = self.net.engine                                         # full batch of this shape (yolo_net_autotune), instead of the built-in rules
            eng.autotune(np.zeros((eng.max_batch,) + tuple(input_shape), dtype=np.float32))
        # resize / colour order / /255 run on the device with OpenCV's INTER_LINEAR arithmetic (base.preprocess_image_gpu);
        # `preprocess = pillow` (new optional key) keeps the host-side Pillow resampler
        pillow = str(params.get("preprocess", "gpu")).lower() == "pillow"
        # `resize` (new optional key): "stretch", the default, is the reference's geometry (net/base.py:121); "letterbox" is Darknet's
        # `detector test` -- aspect ratio kept, grey canvas, boxes mapped back to the frame on the device (yolo_boxes_to_frames)
        resize = _hip.resize_mode(params.get("resize", "stretch"))
        if pillow and resize != _hip.RESIZE_STRETCH:
            raise ValueError("resize = letterbox needs the device-side preprocessing (preprocess = gpu)")
        # One process: the loop is a three-stage pipeline (new optional key `pipeline`, default True): worker threads decode the files
        # of batch i + 1 and draw / encode / write the images of batch i - 1 while the GPU runs batch i; the box records come back by
        # an asynchronous copy into pinned memory.  Same files, same console lines in the same order as the serial loop.
        import time
        t_loop = time.perf_counter()
        self.timing = {"images": len(image_paths), "batch_size": batch_size}      # (seconds per stage of the loop: tools/e2e_launcher.py)
        if world == 1 and not pillow and str(params.get("pipeline", "true")).lower() == "true":
            self.timing["mode"] = "pipelined"
            # (new optional key `staging`: "u8" keeps the resized batch as 8-bit pixels on the device and runs yolo_net_detect_u8 -- same
            # files, a quarter of the staging memory; "f32", the default until tools/e2e_launcher.py has timed both, the float32 batch)
            self._test_pipelined(image_paths, out_dir, batch_size, input_shape, threshold, iou_threshold, nms_mode, class_names,
                                 workers=int(params.get("workers", 0)), timings=self.timing,
                                 staging=str(params.get("staging", "f32")).lower(), resize=resize)
            self.timing["loop_s"] = time.perf_counter() - t_loop
            print("Done")
            return
        self.timing.update(mode="serial", decode_preprocess=0.0, predict=0.0, draw_save=0.0)
        eng = self.net.engine
        for start in range(0, len(image_paths), batch_size):
            paths = image_paths[start:start + batch_size]
            # every rank decodes / resizes only ITS shard of the batch (one process per GPU)
            lo, hi = ydist.shard_range(len(paths), rank, world)
            t0 = time.perf_counter()
            after = None
            if hi <= lo:
                x_local = None
            elif pillow:
                x_local = next(iter(base.generate_test_batch(paths[lo:hi], batch_size, input_shape)))[0]
            else:
                # the shard's frames in one copy and ONE resize launch (yolo_preprocess_frames) where a launch per image used to be
                descs, keep = eng.frame_descs(base.decode_frames(paths[lo:hi]))
                x_local = eng.preprocess_frames(descs, hi - lo, resize, u8=False)
                if resize != _hip.RESIZE_STRETCH:
                    after = lambda d=descs, n=hi - lo: eng.boxes_to_frames(d, n, resize)
            t1 = time.perf_counter()
            net_boxes = self.predict_shard(x_local, len(paths), threshold, iou_threshold, nms_mode, after_detect=after)
            t2 = time.perf_counter()
            self.timing["decode_preprocess"] += t1 - t0
            self.timing["predict"] += t2 - t1
            if rank != 0:
                continue
            for boxes, path in zip(net_boxes, paths):
                new_img = base.draw_boxes(path, boxes, class_names)
                file_name, file_ext = os.path.splitext(os.path.basename(path))
                out_path = os.path.join(out_dir, "{}_out{}".format(file_name, file_ext))
                base.save_image(new_img, out_path)
                print("{}: Found {} objects. Saved to {}".format(file_name, len(boxes), out_path))
            self.timing["draw_save"] += time.perf_counter() - t2
        self.timing["loop_s"] = time.perf_counter() - t_loop
        if rank == 0:
            print("Done")

    # ---- EVAL mode (no reference counterpart: net/base.py:69-97 parses annotations, nothing scores a detector) ----------------
    def evaluate(self, params):
        """VOC-style mAP of the network on an annotated directory, matched and scored on the device (net/evaluate.py, yolo_eval_*).
        The [TEST] keys plus `annotation_dir`, `image_dir`, `match_iou` (0.5); `threshold` defaults to 0.005 and `max_boxes` to 1024, the
        usual settings of a mAP run.  Frames go through the predict_frames step (`resize` = stretch | letterbox), so boxes and truths
        are both normalised to the frame; the records never leave the device.  Prints one line per class with truths and the two
        means, writes `eval.json` under `out_dir`, returns the EvalResult.  A candidate overflow (detect status 1) raises, as in
        test(); truncated lists (status 2) are counted and reported as `images_truncated`.

        `loss = true` (optional, default off; YOLOv2 and resize = stretch only): every step also enqueues the loss (HipNetwork.loss_frames) on
        the batch tensor the step resized, against the step's slice of the truths; the per-image partials stay on the device, are added
        there once at the end (yolo_loss_reduce) and read once.  The report gains `validation_loss` -- the reference's number
        (net/yolo.py:177-193): the mean over make_batch's batches, the last one padded with the first annotations of the set
        (evaluate.validation_loss has the formula) -- and its five components; one more console line."""
        import json
        from . import evaluate as yeval
        annotation_dir, image_dir = params["annotation_dir"], params["image_dir"]
        out_dir = params["out_dir"]
        batch_size = int(params["batch_size"])
        threshold = float(params.get("threshold", 0.005))
        iou_threshold = float(params["iou_threshold"])
        match_iou = float(params.get("match_iou", 0.5))
        anchors = np.reshape(params["anchors"], [-1, 2])
        class_names = params["class_names"]
        input_shape = (int(params["input_h"]), int(params["input_w"]), int(params["input_c"]))
        nms_mode = {"agnostic": _hip.NMS_AGNOSTIC, "per_class": _hip.NMS_PER_CLASS}[params.get("nms_mode", "agnostic")]
        resize = _hip.resize_mode(params.get("resize", "stretch"))
        want_loss = yeval.loss_option(params, self.version)
        annotations, skipped = yeval.parse_voc_annotations(annotation_dir, image_dir, class_names)
        if not annotations:
            print("No annotations found in {}".format(annotation_dir))
            return None
        caps = {"max_boxes": int(params.get("max_boxes", 1024))}
        if "cand_capacity" in params:
            caps["cand_capacity"] = int(params["cand_capacity"])
        if self.net is None or getattr(self.net, "engine", None) is None:
            self.build(anchors, class_names, input_shape, dtype=params.get("dtype", "fp32"), max_batch=batch_size, **caps)
            type(self).load_weights(self.net, params["pretrained_weights_path"])
            print("Pre-trained weights loaded.")
        eng = self.net.engine
        max_gt = max(1, max(len(t) for _, t in annotations))
        ev = yeval.Evaluator(len(class_names), det_capacity=int(params.get("det_capacity", 1 << 18)), max_gt=max_gt, match_iou=match_iou,
                             device=eng.device)
        overflow = eng.torch.zeros(1, dtype=eng.torch.int32, device=eng.device)
        gt_dev, gt_counts = ev.upload_gts([t for _, t in annotations])     # the truths of the whole set: packed and copied once
        if want_loss:
            loss_images = eng.torch.empty((len(annotations), yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=eng.torch.uint8, device=eng.device)
        for start in range(0, len(annotations), batch_size):
            chunk = annotations[start:start + batch_size]
            frames = base.decode_frames([p for p, _ in chunk])
            boxes, counts, status = eng.detect_frames(frames, threshold, iou_threshold, nms_mode, resize)
            # same stream, no copy of the records to the host, nothing read from the host
            ev.add(boxes, counts, (gt_dev[start:start + len(chunk)], gt_counts[start:start + len(chunk)]), status)
            overflow |= (status & 1).max()
            if want_loss:       # a dense pass on the batch tensor detect_frames resized; the partials go to this step's slice
                eng.loss_frames((gt_dev[start:start + len(chunk)], gt_counts[start:start + len(chunk)]), images=loss_images[start:start + len(chunk)])
        if int(overflow.item()):
            raise _hip.YoloHipError("candidate capacity exceeded during evaluation: raise cand_capacity or the threshold")
        result = ev.finish()
        report = result.to_json(class_names)
        report.update(images=len(annotations), images_truncated=ev.images_truncated, names_skipped=skipped, match_iou=match_iou,
                      threshold=threshold, iou_threshold=iou_threshold, resize=str(params.get("resize", "stretch")))
        for line in eval_lines(report):
            print(line)
        if want_loss:
            bs, nb, pad = yeval.loss_batches(len(annotations), batch_size)
            total = eng.torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=eng.torch.uint8, device=eng.device)
            with eng.torch.cuda.device(eng.device):
                _hip.check(eng.lib.yolo_loss_reduce(loss_images.data_ptr(), len(annotations), pad, bs, total.data_ptr(), eng._stream()),
                           "yolo_loss_reduce")
            rec = total.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]          # the one read
            self.last_loss = {k: float(rec[k]) / nb for k in yeval.LOSS_KEYS}
            report["validation_loss"] = self.last_loss["loss"]
            report.update({k: self.last_loss[k] for k in yeval.LOSS_KEYS[1:]})
            report.update(loss_batches=nb, loss_batch_size=bs, loss_status=[name for bit, name in yeval.LOSS_STATUS_NAMES if int(rec["status"]) & bit])
            print("validation loss: {}".format(report["validation_loss"]))
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "eval.json"), "w") as f:
            json.dump(report, f, indent=1)
        self.last_eval = result
        return result

    def _test_pipelined(self, image_paths, out_dir, batch_size, input_shape, threshold, iou_threshold, nms_mode, class_names, workers=0,
                        timings=None, staging="f32", resize=_hip.RESIZE_STRETCH):
        """The body of the reference's test loop (net/yolo.py:80-95) as a pipeline over batches:

            worker threads   decode_image() of the files of batch i + 1 (Pillow releases the GIL inside its codecs)
            this thread      batch i: uint8 pixels -> pinned staging -> device (async), ONE yolo_preprocess_frames of all its images
                             (stretch or letterbox) straight into the batch tensor, yolo_net_detect (staging = "u8": a uint8 batch
                             tensor through yolo_preprocess_frames_u8 / yolo_net_detect_u8, same records), for letterbox
                             yolo_boxes_to_frames on the survivors, async copy of the record buffer
                             [counts | status | boxes] to pinned memory + an event -- nothing here waits for the GPU
            worker PROCESSES batch i - 1, once its event has fired: records -> BoundingBox lists, draw_boxes on the pixels
                             already decoded (no second read of the file), encode + write `<stem>_out<ext>`
                             (base.draw_save_task; drawing holds the GIL, so threads only for directories of < 64 files)

        The console lines are printed by this thread in image order, a batch's lines when its files are on disk.
        timings: optional dict that receives the summed seconds per stage (tools/e2e_launcher.py)."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        import torch
        eng = self.net.engine
        torch_dev = eng.device
        lib = _hip.lib()
        h, w, c = (int(v) for v in input_shape)
        if workers <= 0:
            workers = max(2, min(16, (os.cpu_count() or 4) - 2))
        t = timings if timings is not None else {}
        for k in ("decode_wait", "upload_resize_enqueue", "detect_enqueue", "records_wait", "boxes", "draw_save_wait"):
            t.setdefault(k, 0.0)
        batches = [image_paths[i:i + batch_size] for i in range(0, len(image_paths), batch_size)]
        pool = ThreadPoolExecutor(max_workers=min(8, workers))          # decoders (Pillow's codecs release the GIL)
        # drawing + encoding hold the GIL, so the writers are PROCESSES (spawned: they import PIL / NumPy / net.base, never torch,
        # never the GPU); a handful of files is not worth their start-up: threads then
        if len(image_paths) >= 64:
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor
            writers = ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn"))
            for _ in range(workers):        # (the processes start now, beside the first batches, not at the first file to write)
                writers.submit(int)
        else:
            writers = pool
        decode = lambda paths: [pool.submit(base.decode_image, p) for p in paths]
        stream = torch.cuda.current_stream(torch_dev)
        # two sets of per-batch resources, used alternately: batch i + 1 is prepared while batch i's records are still in flight
        if staging not in ("u8", "f32"):
            raise ValueError("staging must be u8 or f32, got %r" % (staging,))
        u8 = staging == "u8"
        t["staging"] = staging
        resize_name = "yolo_preprocess_frames_u8" if u8 else "yolo_preprocess_frames"
        resize_frames = getattr(lib, resize_name)
        descs = (_hip.Frame * batch_size)()
        x_dev = [torch.empty((batch_size, h, w, c), dtype=torch.uint8 if u8 else torch.float32, device=torch_dev) for _ in range(2)]
        rec_host = [torch.empty(ydist.record_words(eng.max_batch, eng.max_boxes), dtype=torch.int32).pin_memory() for _ in range(2)]
        stage_host, stage_dev = [None, None], [None, None]
        events = [torch.cuda.Event() for _ in range(2)]

        def finish(job):
            """batch whose GPU work was enqueued earlier: wait for its records, hand the images to the writers"""
            slot, paths, rgbs = job
            t0 = time.perf_counter()
            events[slot].synchronize()
            t["records_wait"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            n = len(paths)
            boxes, counts, status = ydist.split_records(rec_host[slot], eng.max_batch, eng.max_boxes)
            records, self.last_status = engine.records_to_host(boxes[:n], counts[:n], status[:n])
            t["boxes"] += time.perf_counter() - t0
            return [writers.submit(base.draw_save_task, p, rgb, r, list(class_names), out_dir) for p, rgb, r in zip(paths, rgbs, records)]

        from collections import deque
        written = deque()               # futures of the writers, in image order
        max_pending = 4 * workers + 2 * batch_size

        def flush(everything=False):
            """print the lines of the files that are on disk, in image order; wait only when too many writes are queued (or at the end)"""
            t0 = time.perf_counter()
            while written and (everything or len(written) > max_pending or written[0].done()):
                print(written.popleft().result())
            t["draw_save_wait"] += time.perf_counter() - t0

        os.makedirs(out_dir, exist_ok=True)
        ahead = max(2 * batch_size, 32)         # images whose decode is requested ahead of the batch the GPU is given
        decoding, nxt, in_flight = deque(), 0, 0
        job = None
        for bi, paths in enumerate(batches):
            slot = bi & 1
            while nxt < len(batches) and (nxt <= bi or in_flight + len(batches[nxt]) <= ahead):
                decoding.append(decode(batches[nxt]))
                in_flight += len(batches[nxt])
                nxt += 1
            t0 = time.perf_counter()
            rgbs = [f.result() for f in decoding.popleft()]
            in_flight -= len(paths)
            t["decode_wait"] += time.perf_counter() - t0
            for p, rgb in zip(paths, rgbs):
                if rgb is None:
                    raise IOError("cannot read image {}".format(p))
            # ---- batch bi on the GPU (enqueue only) -----------------------------------------------------------------------------------
            t0 = time.perf_counter()
            total = sum((int(r.size) + 255) // 256 * 256 for r in rgbs)     # (every image starts on a 256-byte boundary)
            if stage_host[slot] is None or stage_host[slot].numel() < total:
                stage_host[slot] = torch.empty(int(total * 1.25) + 4096, dtype=torch.uint8).pin_memory()
                stage_dev[slot] = torch.empty(stage_host[slot].numel(), dtype=torch.uint8, device=torch_dev)
            off = 0
            spans = []
            host_np = stage_host[slot].numpy()
            for rgb in rgbs:
                n = int(rgb.size)
                host_np[off:off + n] = rgb.reshape(-1)
                spans.append((off, rgb.shape[0], rgb.shape[1]))
                off += (n + 255) // 256 * 256
            stage_dev[slot][:off].copy_(stage_host[slot][:off], non_blocking=True)
            x = x_dev[slot][:len(paths)]
            base_ptr = stage_dev[slot].data_ptr()
            for i, (o, ih, iw) in enumerate(spans):
                descs[i] = _hip.Frame(base_ptr + o, ih, iw, iw * 3, 0)
            _hip.check(resize_frames(descs, len(spans), resize, x.data_ptr(), h, w, stream.cuda_stream), resize_name)
            t["upload_resize_enqueue"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            (eng.detect_u8 if u8 else eng.detect)(x, threshold, iou_threshold, nms_mode)
            eng.boxes_to_frames(descs, len(spans), resize)        # (stretch: returns at once, nothing is launched)
            rec_host[slot].copy_(eng.records, non_blocking=True)
            events[slot].record(stream)
            t["detect_enqueue"] += time.perf_counter() - t0
            # ---- batch bi - 1: records -> boxes -> writers; the lines of whatever is on disk by now ------------------------------------
            if job is not None:
                written.extend(finish(job))
            flush()
            job = (slot, paths, rgbs)
        if job is not None:
            written.extend(finish(job))
        flush(everything=True)
        pool.shutdown()
        if writers is not pool:
            writers.shutdown()


def eval_lines(report):
    """the console lines of Yolo.evaluate: one per class with truths, then the two means and what was not clean"""
    fmt = lambda v: "nan" if v is None else "%.6f" % v
    lines = ["{}: AP12 {} AP07 {} (truths {}, detections {}, tp {}, fp {}, ignored {})".format(
        c["name"], fmt(c["ap_voc12"]), fmt(c["ap_voc07"]), c["n_gt"], c["n_det"], c["tp"], c["fp"], c["ignored"])
        for c in report["classes"] if c["n_gt"] > 0]
    lines.append("mAP12 {} mAP07 {} over {} images, {} records".format(fmt(report["map_voc12"]), fmt(report["map_voc07"]), report["images"],
                                                                      report["n_records"]))
    if report["images_truncated"] or report["status"] or report["names_skipped"]:
        lines.append("images_truncated {} status {} names_skipped {}".format(report["images_truncated"], report["status_names"],
                                                                             report["names_skipped"]))
    return lines


class YoloV2(Yolo):
    version = "v2"
    create_network = staticmethod(v2.create_full_network)
    load_weights = staticmethod(v2.load_weights)
    find_bounding_boxes = staticmethod(v2.find_bounding_boxes)


class YoloV2Tiny(Yolo):
    """Not in the reference (it ships only the tiny-voc anchors); same plug points."""
    version = "v2-tiny"
    create_network = staticmethod(v2.create_tiny_network)
    load_weights = staticmethod(v2.load_weights)
    find_bounding_boxes = staticmethod(v2.find_bounding_boxes)


class YoloV3(Yolo):
    version = "v3"
    create_network = staticmethod(v3.create_network)
    load_weights = staticmethod(v3.load_weights)
    find_bounding_boxes = staticmethod(v3.find_bounding_boxes)


class YoloV3Tiny(Yolo):
    """Not in the reference: upstream Darknet's yolov3-tiny.cfg (two scales); same plug points."""
    version = "v3-tiny"
    create_network = staticmethod(v3.create_tiny_network)
    load_weights = staticmethod(v3.load_weights)
    find_bounding_boxes = staticmethod(v3.find_bounding_boxes)


class YoloV3SPP(Yolo):
    """Not in the reference: upstream Darknet's yolov3-spp.cfg (Darknet-53 + SPP block in the coarse head); same plug points."""
    version = "v3-spp"
    create_network = staticmethod(v3.create_spp_network)
    load_weights = staticmethod(v3.load_weights)
    find_bounding_boxes = staticmethod(v3.find_bounding_boxes)

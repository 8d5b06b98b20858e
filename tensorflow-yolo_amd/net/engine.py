"""Runtime object behind a layer list: lowers it through the C ABI to a fused kernel plan and
runs it.  Stands where the reference has `tf.Session` + `sess.run(net[-1].out, {net[0].out: x})`
(reference net/yolo.py:67-83).

torch is used for exactly three things: device memory (uint8/float32 tensors whose
`.data_ptr()` goes to the C ABI), the current HIP stream, and host<->device copies.
"""
import ctypes as C

import numpy as np

from .. import _hip
from . import dist as ydist
from . import layers as L


def number_layers(net):
    for i, layer in enumerate(net):
        layer.index = i
    return net


def to_descs(net):
    """Layer objects -> the C ABI's yolo_layer_desc array (one per list element)."""
    number_layers(net)
    descs = (_hip.LayerDesc * len(net))()
    for i, layer in enumerate(net):
        d = descs[i]
        d.op = layer.op
        d.n_src = len(layer.inputs)
        if d.n_src > _hip.MAX_SRC:
            raise ValueError("layer %d has more than %d inputs" % (i, _hip.MAX_SRC))
        for k, src in enumerate(layer.inputs):
            if src.index is None or src.index >= i or net[src.index] is not src:
                raise ValueError("layer %d consumes a layer that is not earlier in the same list" % i)
            d.src[k] = src.index
        layer.fill_desc(d)
    return descs


def head_desc_v2(h, w, anchors, num_classes):
    """YOLOv2 keeps its anchors outside the graph (reference net/v2.py:83-85): one scale."""
    anchors = np.reshape(np.asarray(anchors, dtype=np.float64), [-1, 2])
    hd = _hip.HeadDesc()
    hd.version, hd.n_classes, hd.n_scales = 2, int(num_classes), 1
    hd.h[0], hd.w[0], hd.n_anchors[0] = int(h), int(w), len(anchors)
    for i, (aw, ah) in enumerate(anchors):
        hd.anchors[0][2 * i], hd.anchors[0][2 * i + 1] = float(aw), float(ah)
    return hd


def head_desc_v3(yolos, anchors_per_scale=None, n_classes=None):
    """From the yolo layers of a detection layer (reference net/v3.py:145-149): head_desc_v3(yolos).  Or from plain numbers, for a head
    that belongs to no network of this package: head_desc_v3(grids, anchors_per_scale, n_classes) with grids = [(h, w), ...] in head order
    and anchors_per_scale = [[(aw, ah), ...], ...] in the grid units of their scale."""
    hd = _hip.HeadDesc()
    if anchors_per_scale is None:
        hd.version, hd.n_classes, hd.n_scales = 3, int(yolos[0].no_c), len(yolos)
        for s, y in enumerate(yolos):
            hd.h[s], hd.w[s], hd.n_anchors[s] = y.h, y.w, y.b
            for i, (aw, ah) in enumerate(y.anchors):
                hd.anchors[s][2 * i], hd.anchors[s][2 * i + 1] = float(aw), float(ah)
        return hd
    grids = [(int(h), int(w)) for h, w in yolos]
    if n_classes is None or not 1 <= len(grids) <= _hip.MAX_SCALES or len(anchors_per_scale) != len(grids):
        raise ValueError("head_desc_v3: expected 1..%d grids, as many anchor lists and n_classes" % _hip.MAX_SCALES)
    hd.version, hd.n_classes, hd.n_scales = 3, int(n_classes), len(grids)
    for s, ((h, w), anc) in enumerate(zip(grids, anchors_per_scale)):
        anc = np.reshape(np.asarray(anc, dtype=np.float64), [-1, 2])
        if not 1 <= len(anc) <= _hip.MAX_ANCHORS:
            raise ValueError("head_desc_v3: scale %d: expected 1..%d anchors" % (s, _hip.MAX_ANCHORS))
        hd.h[s], hd.w[s], hd.n_anchors[s] = h, w, len(anc)
        for i, (aw, ah) in enumerate(anc):
            hd.anchors[s][2 * i], hd.anchors[s][2 * i + 1] = float(aw), float(ah)
    return hd


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP backend needs a ROCm GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback in this package")
    return torch


class Plan(object):
    """Device-free part: create the native net object, query sizes, print the plan.
    Works without a GPU (used by the CPU test-suite to check planning)."""

    def __init__(self, net, dtype="fp16", max_batch=1, keep_all=False, cand_capacity=4096, max_boxes=_hip.DEFAULT_MAX_BOXES, streams=0,
                 force_tile=None, guard_bytes=0, f32_products=0):
        self.lib = _hip.lib()
        self.layers = list(net)
        known = {"fp16": _hip.DTYPE_F16, "f16": _hip.DTYPE_F16, "half": _hip.DTYPE_F16,
                 "fp32": _hip.DTYPE_F32, "f32": _hip.DTYPE_F32, "float": _hip.DTYPE_F32,
                 "mxfp8": _hip.DTYPE_MXF8, "mxf8": _hip.DTYPE_MXF8}
        if str(dtype).lower() not in known:
            raise ValueError("dtype must be fp16, fp32 or mxfp8, got %r" % (dtype,))
        self.dtype = known[str(dtype).lower()]
        self.max_batch = int(max_batch)
        self.max_boxes = int(max_boxes)
        self.cand_capacity = int(cand_capacity)
        opt = _hip.NetOptions(dtype=self.dtype, max_batch=self.max_batch, keep_all=int(bool(keep_all)),
                              cand_capacity=self.cand_capacity, max_boxes=self.max_boxes, streams=int(streams),
                              force_tile=0 if force_tile is None else int(force_tile) + 1, guard_bytes=int(guard_bytes),
                              f32_products=int(f32_products))
        descs = to_descs(self.layers)
        handle = C.c_void_p()
        _hip.check(self.lib.yolo_net_create(descs, len(self.layers), C.byref(opt), C.byref(handle)), "yolo_net_create")
        self.handle = handle
        self.weight_count = self.lib.yolo_net_weight_count(handle)
        self.weights_bytes = self.lib.yolo_net_weights_bytes(handle)
        self.workspace_bytes = self.lib.yolo_net_workspace_bytes(handle)
        self.output_count = self.lib.yolo_net_output_count(handle)
        self.flops_per_image = self.lib.yolo_net_flops_per_image(handle)
        self.num_kernels = self.lib.yolo_net_num_kernels(handle)
        self._auto_streams = int(streams) <= 0                          # streams = 0: the library's rule, re-measured on the device
        self._streams_tuned = False                                     # (HipNetwork: at the first full batch)
        self.u8_calls = 0                                               # diagnostic: calls that went through a uint8 entry point (forward_u8 / detect_u8 / forward_timed_u8)
        self.input_hwc = self.layers[0].out.hwc
        last = self.layers[-1]
        if isinstance(last, L.detection_layer):
            self.output_shape = (last.out.hwc[0], last.out.hwc[2])              # [rows, 5+C]
            self.set_head(head_desc_v3(last.yolos))
        else:
            self.output_shape = last.out.hwc                                    # [h, w, c]

    @property
    def num_streams(self):
        """parts / HIP streams a full batch currently runs as (yolo_net_options.streams; 0 = the library's rule, which a
        HipNetwork re-measures on the device at its first full batch: yolo_net_tune_streams)"""
        return self.lib.yolo_net_num_streams(self.handle)

    def workspace_regions(self):
        """[(name, offset, used_bytes, region_bytes)] of the planned workspace (yolo_net_workspace_regions: diagnostic / canary tests)."""
        n = self.lib.yolo_net_workspace_regions(self.handle, None, 0)
        arr = (_hip.WsRegion * n)()
        self.lib.yolo_net_workspace_regions(self.handle, arr, n)
        return [(r.name.decode(), int(r.offset), int(r.used_bytes), int(r.region_bytes)) for r in arr]

    def set_head(self, hd):
        _hip.check(self.lib.yolo_net_set_head(self.handle, C.byref(hd)), "yolo_net_set_head")
        self.head = hd

    def head_input(self):
        """yolo_net_head_input: where the detection layer's input lives in the workspace after a dense forward (a _hip.TensorView; host only)"""
        v = _hip.TensorView()
        _hip.check(self.lib.yolo_net_head_input(self.handle, C.byref(v)), "yolo_net_head_input")
        return v

    def head_train_layout(self):
        """yolo_net_head_train_layout: byte offsets of the parts of the head-training state (a _hip.HeadTrainLayout; host only)"""
        lay = _hip.HeadTrainLayout()
        _hip.check(self.lib.yolo_net_head_train_layout(self.handle, C.byref(lay)), "yolo_net_head_train_layout")
        return lay

    def tail_inputs(self):
        """yolo_net_tail_inputs: where the input of the 3 x 3 block behind the detection layer and the detection layer's input live in the
        workspace after a dense forward (two _hip.TensorView; host only)"""
        block_in, head_in = _hip.TensorView(), _hip.TensorView()
        _hip.check(self.lib.yolo_net_tail_inputs(self.handle, C.byref(block_in), C.byref(head_in)), "yolo_net_tail_inputs")
        return block_in, head_in

    def tail_train_layout(self):
        """yolo_net_tail_train_layout: byte offsets of the parts of the tail-training state (a _hip.TailTrainLayout; host only)"""
        lay = _hip.TailTrainLayout()
        _hip.check(self.lib.yolo_net_tail_train_layout(self.handle, C.byref(lay)), "yolo_net_tail_train_layout")
        return lay

    def head_inputs_v3(self):
        """yolo_net_head_inputs_v3: where the input of every head conv lives in the workspace after a dense forward, in head order (a list of
        _hip.TensorView; host only)"""
        views = (_hip.TensorView * _hip.MAX_SCALES)()
        n = C.c_int32(0)
        _hip.check(self.lib.yolo_net_head_inputs_v3(self.handle, views, C.byref(n)), "yolo_net_head_inputs_v3")
        return [views[s] for s in range(n.value)]

    def head_train_layout_v3(self):
        """yolo_net_head_train_v3_layout: byte offsets of the parts of the YOLOv3 head-training state (a _hip.HeadTrainV3Layout; host only)"""
        lay = _hip.HeadTrainV3Layout()
        _hip.check(self.lib.yolo_net_head_train_v3_layout(self.handle, C.byref(lay)), "yolo_net_head_train_v3_layout")
        return lay

    def block_inputs_v3(self):
        """yolo_net_block_inputs_v3: per scale in head order, where the input of the 3 x 3 block behind the head conv and the head conv's
        input live in the workspace after a dense forward (two lists of _hip.TensorView; host only)"""
        blocks, heads = (_hip.TensorView * _hip.MAX_SCALES)(), (_hip.TensorView * _hip.MAX_SCALES)()
        n = C.c_int32(0)
        _hip.check(self.lib.yolo_net_block_inputs_v3(self.handle, blocks, heads, C.byref(n)), "yolo_net_block_inputs_v3")
        return [blocks[s] for s in range(n.value)], [heads[s] for s in range(n.value)]

    def blocks_train_layout_v3(self):
        """yolo_net_blocks_train_v3_layout: byte offsets of the parts of the state that trains the YOLOv3 head convs and the blocks behind
        them (a _hip.BlocksTrainV3Layout; host only)"""
        lay = _hip.BlocksTrainV3Layout()
        _hip.check(self.lib.yolo_net_blocks_train_v3_layout(self.handle, C.byref(lay)), "yolo_net_blocks_train_v3_layout")
        return lay

    def describe(self):
        n = self.lib.yolo_net_describe(self.handle, None, 0)
        buf = C.create_string_buffer(n)
        self.lib.yolo_net_describe(self.handle, buf, n)
        return buf.value.decode()

    def close(self):
        if getattr(self, "handle", None):
            self.lib.yolo_net_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipNetwork(Plan):
    """Plan + device memory: forward() / detect() on the current torch HIP stream."""

    def __init__(self, net, dtype="fp16", max_batch=1, device=None, **kw):
        super(HipNetwork, self).__init__(net, dtype=dtype, max_batch=max_batch, **kw)
        torch = _torch()
        self.torch = torch
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self._weights = torch.empty(max(self.weights_bytes, 256), dtype=torch.uint8, device=self.device)
            self._workspace = torch.zeros(max(self.workspace_bytes, 256), dtype=torch.uint8, device=self.device)
            # ONE record buffer [counts | status | boxes] (net/dist.py): what a multi-GPU run all-gathers as it is
            self.records = torch.zeros(ydist.record_words(self.max_batch, self.max_boxes), dtype=torch.int32, device=self.device)
            self._boxes, self._counts, self._status = ydist.split_records(self.records, self.max_batch, self.max_boxes)
            _hip.check(self.lib.yolo_net_bind_workspace(self.handle, self._workspace.data_ptr(), self._workspace.numel()),
                       "yolo_net_bind_workspace")
        self.weights_loaded = False

    # -- weights ------------------------------------------------------------------------------
    def load_weights(self, flat):
        """flat: float32 body of a Darknet .weights file, layer-list order (reference net/base.py:26-46)."""
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_load_weights(self.handle, flat.ctypes.data, flat.size,
                                                      self._weights.data_ptr(), self._weights.numel()),
                       "yolo_net_load_weights")
        self.weights_loaded = True

    # -- data ---------------------------------------------------------------------------------
    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def to_device(self, x_batch):
        """Host NumPy [B,H,W,C] (float64 in the reference, net/base.py:153) or a torch tensor ->
        float32 device tensor, the dtype the reference's placeholder casts to (net/layers.py:108)."""
        torch = self.torch
        if isinstance(x_batch, torch.Tensor):
            x = x_batch.to(device=self.device, dtype=torch.float32)
        else:
            x = torch.from_numpy(np.ascontiguousarray(x_batch, dtype=np.float32)).to(self.device)
        x = x.contiguous()
        h, w, c = self.input_hwc
        if x.dim() != 4 or tuple(x.shape[1:]) != (h, w, c):
            raise ValueError("expected input [B,%d,%d,%d], got %s" % (h, w, c, tuple(x.shape)))
        if not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError("batch %d outside 1..%d (max_batch)" % (x.shape[0], self.max_batch))
        return x

    def is_u8(self, x_batch):
        """a torch tensor of torch.uint8 or a NumPy array of np.uint8 (what decides between an entry point and its uint8 twin)"""
        if isinstance(x_batch, self.torch.Tensor):
            return x_batch.dtype == self.torch.uint8
        return getattr(x_batch, "dtype", None) == np.uint8

    def check_u8(self, x_batch):
        """Shape / dtype rule of the uint8 entry points (no GPU needed): a uint8 NumPy array or torch tensor [B,H,W,C] of the net's input
        shape with 1 <= B <= max_batch; anything else raises ValueError (a float array is NOT scaled or cast here: use forward / detect)."""
        dt = str(getattr(x_batch, "dtype", None)).replace("torch.", "")
        if dt != "uint8":
            raise ValueError("the uint8 entry points take a uint8 array or tensor, got %s (%s)" % (type(x_batch).__name__, dt))
        h, w, c = self.input_hwc
        shape = tuple(int(v) for v in x_batch.shape)
        if len(shape) != 4 or shape[1:] != (h, w, c):
            raise ValueError("expected uint8 input [B,%d,%d,%d], got %s" % (h, w, c, shape))
        if not 1 <= shape[0] <= self.max_batch:
            raise ValueError("batch %d outside 1..%d (max_batch)" % (shape[0], self.max_batch))
        return shape[0]

    def to_device_u8(self, x_batch):
        """uint8 [B,H,W,C] (host NumPy / torch, or already on the device) -> dense uint8 device tensor: one copy of B*H*W*C bytes, no
        arithmetic (the / 255. of net/base.py:153 happens inside the first kernel).  A contiguous device view is passed as it is,
        whatever its byte alignment."""
        torch = self.torch
        self.check_u8(x_batch)
        x = x_batch if isinstance(x_batch, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x_batch))
        return x.to(self.device).contiguous()

    def _tune_streams(self, x):
        """streams = 0 and the rule said two halves: time one pass against two halves on THIS device, once, with the first batch
        that is large enough, and keep the faster (yolo_net_tune_streams: the gain is board-dependent, +4 % to -1.5 %)."""
        if self._streams_tuned or not self._auto_streams or not self.weights_loaded:
            return
        if self.lib.yolo_net_num_streams(self.handle) < 2 or 2 * x.shape[0] <= self.max_batch:
            self._streams_tuned = self.lib.yolo_net_num_streams(self.handle) < 2
            return
        name = "yolo_net_tune_streams_u8" if x.dtype == self.torch.uint8 else "yolo_net_tune_streams"
        with self.torch.cuda.device(self.device):
            _hip.check(getattr(self.lib, name)(self.handle, x.data_ptr(), x.shape[0], self._stream()), name)
        self._streams_tuned = True

    def agree_streams(self, x, group=None, u8=False):
        """Ranks of a sharded batch must run the SAME plan: each rank measures for itself where it can, then rank
        0's answer is broadcast and taken by everyone -- one pass and two halves differ in fp16 summation order, and the job's step
        time is the slowest rank's.  A collective: every rank calls it once (net/dist.py does, at its first sharded detect)."""
        torch = self.torch
        if x is not None and x.shape[0] > 0:
            self._tune_streams(self.to_device_u8(x) if u8 else self.to_device(x))
        import torch.distributed as dist
        from . import dist as ydist
        want = ydist.broadcast_rank0_int(self.num_streams, group, self.device if dist.get_backend(group) == "nccl" else "cpu")
        if want != self.num_streams:
            _hip.check(self.lib.yolo_net_set_streams(self.handle, want), "yolo_net_set_streams")
        self._streams_tuned = True
        return want

    def forward(self, x, out=None):
        """Head logits (float32, device) in the reference's layout: v2 [B,h,w,A*(5+C)], v3 [B,rows,5+C]."""
        torch = self.torch
        x = self.to_device(x)
        self._tune_streams(x)
        b = x.shape[0]
        if out is None:
            out = torch.empty((b,) + tuple(self.output_shape), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_forward(self.handle, x.data_ptr(), b, out.data_ptr(), self._stream()),
                       "yolo_net_forward")
        return out

    def detect(self, x, threshold, iou_threshold, nms_mode=_hip.NMS_AGNOSTIC):
        """forward + decode + NMS, one enqueue.  Returns device tensors (boxes [B,K,6] as
        (x,y,w,h,prob,class-as-int32-bits), counts [B], status [B]); no host sync."""
        torch = self.torch
        x = self.to_device(x)
        self._tune_streams(x)
        b = x.shape[0]
        with torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_detect(self.handle, x.data_ptr(), b, float(threshold), float(iou_threshold),
                                                int(nms_mode), self._boxes.data_ptr(), self._counts.data_ptr(),
                                                self._status.data_ptr(), self._stream()), "yolo_net_detect")
        return self._boxes[:b], self._counts[:b], self._status[:b]

    # -- uint8 input (ABI 7): bit-identical to forward / detect / forward_timed fed float32(x / 255.) -----------------------------
    def forward_u8(self, x, out=None):
        """forward() for a uint8 batch [B,H,W,C] (0..255, RGB): the bytes go to the device as they are."""
        torch = self.torch
        x = self.to_device_u8(x)
        self._tune_streams(x)
        b = x.shape[0]
        if out is None:
            out = torch.empty((b,) + tuple(self.output_shape), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_forward_u8(self.handle, x.data_ptr(), b, out.data_ptr(), self._stream()), "yolo_net_forward_u8")
        self.u8_calls += 1
        return out

    def detect_u8(self, x, threshold, iou_threshold, nms_mode=_hip.NMS_AGNOSTIC):
        """detect() for a uint8 batch [B,H,W,C] (0..255, RGB)."""
        x = self.to_device_u8(x)
        self._tune_streams(x)
        b = x.shape[0]
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_detect_u8(self.handle, x.data_ptr(), b, float(threshold), float(iou_threshold),
                                                   int(nms_mode), self._boxes.data_ptr(), self._counts.data_ptr(),
                                                   self._status.data_ptr(), self._stream()), "yolo_net_detect_u8")
        self.u8_calls += 1
        return self._boxes[:b], self._counts[:b], self._status[:b]

    # -- frames of any size: batched resize / letterbox, boxes in frame coordinates -----------------------------------------------
    def frame_descs(self, frames):
        """list of uint8 [h, w, 3] frames of any sizes (NumPy arrays, or torch tensors on any device) -> (yolo_frame array, the device
        tensors it points into).  Host frames travel in ONE copy, each starting on a 256-byte boundary; a device tensor whose pixels are
        dense within a row is described where it lies (any pitch, any alignment)."""
        torch = self.torch
        n = len(frames)
        descs = (_hip.Frame * max(n, 1))()
        keep, host, spans, total = [], [], [], 0
        for i, f in enumerate(frames):
            dt = str(getattr(f, "dtype", None)).replace("torch.", "")
            shape = tuple(int(v) for v in getattr(f, "shape", ()))
            if dt != "uint8" or len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
                raise ValueError("frame %d: expected a uint8 array or tensor [h, w, 3], got %s %s" % (i, dt, shape))
            if isinstance(f, torch.Tensor) and f.device.type != "cpu":
                t = f.to(self.device)
                if t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < 3 * shape[1]:
                    t = t.contiguous()
                keep.append(t)
                descs[i] = _hip.Frame(t.data_ptr(), shape[0], shape[1], t.stride(0), 0)
            else:
                a = f.numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
                host.append((i, np.ascontiguousarray(a).reshape(-1)))
                spans.append((i, total, shape))
                total += (a.size + 255) // 256 * 256
        if host:
            stage = np.empty(total, dtype=np.uint8)
            for (i, flat), (_, off, _) in zip(host, spans):
                stage[off:off + flat.size] = flat
            dev = torch.from_numpy(stage).to(self.device)
            keep.append(dev)
            for i, off, shape in spans:
                descs[i] = _hip.Frame(dev.data_ptr() + off, shape[0], shape[1], 3 * shape[1], 0)
        return descs, keep

    def _frames_batch(self, n, u8=True):
        """the batch tensor the frame entries resize into: [max_batch, H, W, 3], allocated once per type"""
        h, w, c = self.input_hwc
        if c != 3:
            raise ValueError("the frame entries need a network input of 3 channels, this one has %d" % c)
        if not 1 <= n <= self.max_batch:
            raise ValueError("batch %d outside 1..%d (max_batch)" % (n, self.max_batch))
        key = "_frames_u8" if u8 else "_frames_f32"
        if getattr(self, key, None) is None:
            setattr(self, key, self.torch.empty((self.max_batch, h, w, 3), dtype=self.torch.uint8 if u8 else self.torch.float32, device=self.device))
        return getattr(self, key)[:n]

    def preprocess_frames(self, descs, n, resize=_hip.RESIZE_STRETCH, u8=True, out=None):
        """yolo_preprocess_frames[_u8]: the n frames of `descs` (frame_descs) -> the batch tensor [n, H, W, 3] (uint8, or float32 in
        [0, 1]), stretched or letterboxed, one launch per 64 frames.  Enqueued; returns the tensor."""
        x = self._frames_batch(n, u8) if out is None else out
        h, w, _ = self.input_hwc
        name = "yolo_preprocess_frames_u8" if u8 else "yolo_preprocess_frames"
        with self.torch.cuda.device(self.device):
            _hip.check(getattr(self.lib, name)(descs, n, int(resize), x.data_ptr(), h, w, self._stream()), name)
        return x

    def boxes_to_frames(self, descs, n, resize):
        """yolo_boxes_to_frames on the engine's own record buffer: the records of the last detect call, normalised to the network input,
        become normalised to each frame (in place, on the device; nothing happens for stretch)."""
        h, w, _ = self.input_hwc
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_boxes_to_frames(self._boxes.data_ptr(), self._counts.data_ptr(), n, self.max_boxes, descs, int(resize),
                                                     h, w, self._stream()), "yolo_boxes_to_frames")

    def detect_frames(self, frames, threshold, iou_threshold, nms_mode=_hip.NMS_AGNOSTIC, resize=_hip.RESIZE_STRETCH):
        """One enqueue for a whole step (yolo_net_detect_frames_u8): frames of any sizes -> batched resize (stretch | letterbox) into a
        uint8 batch -> forward + decode + NMS -> boxes normalised to each frame.  Returns what detect() returns."""
        n = len(frames)
        x = self._frames_batch(n, True)
        descs, keep = self.frame_descs(frames)
        if self._auto_streams and not self._streams_tuned:         # (the one-off stream measurement wants the batch it would run)
            self._tune_streams(self.preprocess_frames(descs, n, resize, True))
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_detect_frames_u8(self.handle, descs, n, int(resize), x.data_ptr(), float(threshold), float(iou_threshold),
                                                          int(nms_mode), self._boxes.data_ptr(), self._counts.data_ptr(),
                                                          self._status.data_ptr(), self._stream()), "yolo_net_detect_frames_u8")
        self.u8_calls += 1
        self._frames_keep = keep        # (the frames stay allocated until the next call: the work is only enqueued)
        self._frames_last = x           # (the batch this step resized: what loss_frames runs on)
        return self._boxes[:n], self._counts[:n], self._status[:n]

    # -- training augmentation (yolo_augment_u8) ------------------------------------------------------------------------------------------
    def augment_u8(self, x, params, out=None):
        """yolo_augment_u8: a uint8 batch [B, H, W, 3] (the network input; host or device) and one yolo_augment_image per image (a list,
        net/augment.py draws them) -> the augmented batch in `out` (a second buffer of the engine's, allocated once, unless given: the
        source and the result must not overlap).  Enqueued; returns the tensor."""
        from . import augment as yaug
        torch = self.torch
        x = self.to_device_u8(x)
        b, (h, w, c) = x.shape[0], self.input_hwc
        if c != 3:
            raise ValueError("augmentation needs a network input of 3 channels, this one has %d" % c)
        if len(params) != b:
            raise ValueError("expected %d augmentation records, got %d" % (b, len(params)))
        if out is None:
            if getattr(self, "_augment_out", None) is None:
                self._augment_out = torch.empty((self.max_batch, h, w, 3), dtype=torch.uint8, device=self.device)
            out = self._augment_out[:b]
        elif out.device != self.device or out.dtype != torch.uint8 or tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
            raise ValueError("out: expected a contiguous uint8 device tensor %s" % (tuple(x.shape),))
        with torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_augment_u8(x.data_ptr(), out.data_ptr(), b, h, w, yaug.params_array(params), self._stream()),
                       "yolo_augment_u8")
        self._augment_keep = x          # (alive until the next call: the work is only enqueued)
        return out

    # -- YOLOv2 loss, forward only (yolo_net_loss / yolo_net_loss_u8) ------------------------------------------------------------------
    def _loss_gts(self, gts, b):
        return loss_gts(self.torch, self.device, gts, b)

    def _loss_any(self, x, gts, u8, images, assign):
        from . import evaluate as yeval
        torch = self.torch
        if getattr(self, "head", None) is None or self.head.version != 2:
            raise ValueError("the loss is defined for YOLOv2 heads only (the reference has a loss for YOLOv2 only)")
        x = self.to_device_u8(x) if u8 else self.to_device(x)
        self._tune_streams(x)
        b = x.shape[0]
        gt_dev, gc_dev, max_gt = self._loss_gts(gts, b)
        if images is None:
            images = torch.empty((b, yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        elif (images.device != self.device or images.dtype != torch.uint8 or tuple(images.shape) != (b, yeval.LOSS_IMAGE_DTYPE.itemsize)
              or not images.is_contiguous()):
            raise ValueError("images: expected a contiguous uint8 device tensor [%d, %d]" % (b, yeval.LOSS_IMAGE_DTYPE.itemsize))
        result = torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        if assign is True:
            assign = torch.empty((b, self.head.h[0], self.head.w[0]), dtype=torch.int32, device=self.device)
        name = "yolo_net_loss_u8" if u8 else "yolo_net_loss"
        with torch.cuda.device(self.device):
            _hip.check(getattr(self.lib, name)(self.handle, x.data_ptr(), b, gt_dev.data_ptr(), gc_dev.data_ptr(), int(max_gt), images.data_ptr(),
                                               assign.data_ptr() if assign is not None else None, result.data_ptr(), self._stream()), name)
        self.u8_calls += int(u8)
        self._loss_keep = (x, gt_dev, gc_dev)      # (alive until the next call: the work is only enqueued)
        return (images, result) if assign is None else (images, result, assign)

    def loss(self, x, gts, images=None, assign=None):
        """The YOLOv2 loss of a batch against its truths (include/yolo_hip.h has the definition): a dense forward pass and the loss kernels
        in one enqueue, no host sync.  Returns device tensors (images uint8 [B, 56] = yolo_loss_image records, result uint8 [64] =
        yolo_loss_result; evaluate.loss_to_host reads them); `images`: a slice of a caller's record tensor to write into; assign = True
        adds the winner table int32 [B, h, w] (truth_index * 8 + anchor | -1)."""
        return self._loss_any(x, gts, False, images, assign)

    def loss_u8(self, x, gts, images=None, assign=None):
        """loss() for a uint8 batch [B,H,W,C] (0..255, RGB): the same bits as loss(float32(x / 255.))"""
        return self._loss_any(x, gts, True, images, assign)

    def loss_frames(self, gts, images=None):
        """loss_u8() on the uint8 batch the last detect_frames call resized, enqueued behind it on the same stream: the loss of the frames
        that step detected on, without resizing them again.  Stretch only: letterboxed truths are not mapped into the canvas."""
        x = getattr(self, "_frames_last", None)
        if x is None:
            raise RuntimeError("loss_frames follows a detect_frames call")
        return self.loss_u8(x, gts, images=images)

    # -- the gradient of the YOLOv2 loss with respect to the logits (yolo_v2_loss_grad) ---------------------------------------------------
    def _loss_grad_any(self, x, gts, u8):
        if getattr(self, "head", None) is None or self.head.version != 2:
            raise ValueError("the loss is defined for YOLOv2 heads only (the reference has a loss for YOLOv2 only)")
        logits = (self.forward_u8 if u8 else self.forward)(x)
        images, result, assign, grad, keep = v2_loss_grad(self.head, logits, gts)
        self._loss_keep = (logits,) + keep         # (alive until the next call: the work is only enqueued)
        return images, result, assign, grad

    def loss_grad(self, x, gts):
        """The YOLOv2 loss of a batch and its gradient with respect to the head logits (include/yolo_hip.h has the definition): a dense
        forward pass into an output tensor, then the loss kernels and the gradient kernel on it, on the same stream, no host sync.
        Returns device tensors (images, result as loss(); assign int32 [B, h, w]; grad float32 [B, h, w, A * (5 + C)]).  There is no
        backward pass through the network: the gradient stops at the logits."""
        return self._loss_grad_any(x, gts, False)

    def loss_grad_u8(self, x, gts):
        """loss_grad() for a uint8 batch [B,H,W,C] (0..255, RGB): the same bits as loss_grad(float32(x / 255.))"""
        return self._loss_grad_any(x, gts, True)

    # -- the YOLOv3 loss and its gradient (yolo_net_loss_v3 / yolo_net_loss_v3_u8 / yolo_v3_loss_grad) -----------------------------------------
    def _need_v3(self):
        if getattr(self, "head", None) is None or self.head.version != 3:
            raise ValueError("the YOLOv3 loss is defined for version 3 heads only (loss / loss_grad serve a YOLOv2 head)")

    def _loss_v3_any(self, x, gts, ignore_thresh, u8, images):
        from . import evaluate as yeval
        torch = self.torch
        self._need_v3()
        x = self.to_device_u8(x) if u8 else self.to_device(x)
        self._tune_streams(x)
        b = x.shape[0]
        gt_dev, gc_dev, max_gt = self._loss_gts(gts, b)
        rows, parts = v3_loss_rows(self.head)
        if images is None:
            images = torch.empty((b, yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        elif (images.device != self.device or images.dtype != torch.uint8 or tuple(images.shape) != (b, yeval.LOSS_IMAGE_DTYPE.itemsize)
              or not images.is_contiguous()):
            raise ValueError("images: expected a contiguous uint8 device tensor [%d, %d]" % (b, yeval.LOSS_IMAGE_DTYPE.itemsize))
        scratch = torch.empty((b, parts, yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        result = torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        assign = torch.empty((b, rows), dtype=torch.int32, device=self.device)
        name = "yolo_net_loss_v3_u8" if u8 else "yolo_net_loss_v3"
        with torch.cuda.device(self.device):
            _hip.check(getattr(self.lib, name)(self.handle, x.data_ptr(), b, gt_dev.data_ptr(), gc_dev.data_ptr(), int(max_gt), float(ignore_thresh),
                                               scratch.data_ptr(), images.data_ptr(), assign.data_ptr(), result.data_ptr(), self._stream()), name)
        self.u8_calls += int(u8)
        self._loss_keep = (x, gt_dev, gc_dev, scratch)     # (alive until the next call: the work is only enqueued)
        return images, result, assign

    def loss_v3(self, x, gts, ignore_thresh=0.7, images=None):
        """The YOLOv3 loss of a batch against its truths (the loss of Darknet's [yolo] layer; include/yolo_hip.h has the definition): a
        dense forward pass and the loss kernels in one enqueue, no host sync.  Returns device tensors (images uint8 [B, 56], result uint8
        [64] as loss(); assign int32 [B, R]: truth index | -1 | -2 ignored).  ValueError on a YOLOv2 head."""
        return self._loss_v3_any(x, gts, ignore_thresh, False, images)

    def loss_v3_u8(self, x, gts, ignore_thresh=0.7, images=None):
        """loss_v3() for a uint8 batch [B,H,W,C] (0..255, RGB): the same bits as loss_v3(float32(x / 255.))"""
        return self._loss_v3_any(x, gts, ignore_thresh, True, images)

    def _loss_v3_grad_any(self, x, gts, ignore_thresh, u8):
        self._need_v3()
        logits = (self.forward_u8 if u8 else self.forward)(x)
        images, result, assign, grad, keep = v3_loss_grad(self.head, logits, gts, ignore_thresh)
        self._loss_keep = (logits,) + keep         # (alive until the next call: the work is only enqueued)
        return images, result, assign, grad

    def loss_v3_grad(self, x, gts, ignore_thresh=0.7):
        """loss_v3() and its gradient with respect to the head logits: a dense forward pass into an output tensor, then the loss kernels
        and the gradient kernel on it, on the same stream, no host sync.  Returns device tensors (images, result, assign as loss_v3();
        grad float32 of the logits' shape).  The gradient stops at the logits."""
        return self._loss_v3_grad_any(x, gts, ignore_thresh, False)

    def loss_v3_grad_u8(self, x, gts, ignore_thresh=0.7):
        """loss_v3_grad() for a uint8 batch [B,H,W,C] (0..255, RGB)"""
        return self._loss_v3_grad_any(x, gts, ignore_thresh, True)

    # -- what the four training paths share -------------------------------------------------------------------------------------------------
    _TRAIN_ORDER = {"_train_state": "train_head_step follows head_train_init", "_tail_state": "train_tail_step follows tail_train_init",
                    "_train_state_v3": "train_head_step_v3 follows head_train_init_v3",
                    "_blocks_state_v3": "train_blocks_step_v3 follows blocks_train_init_v3"}

    def _train_begin(self):
        """The opening of every *_train_init*: weights are loaded, and a net whose streams = 0 rule runs two halves is set to one pass (each
        part has its own arena; the stream measurement of the first full batch is off from here on).  Returns torch."""
        if not self.weights_loaded:
            raise RuntimeError("no weights loaded: call load_weights first")
        if self._auto_streams and self.num_streams != 1:
            _hip.check(self.lib.yolo_net_set_streams(self.handle, 1), "yolo_net_set_streams")
        self._streams_tuned = True
        return self.torch

    def _train_step(self, name, state, x, gts, lr_t, u8, result, *extra):
        """One yolo_net_train_*_step[_u8] call: `name` the float32 entry, `state` the attribute its *_train_init* left the state in,
        `extra` what the entry takes between max_gt and the state"""
        from . import evaluate as yeval
        torch = self.torch
        if getattr(self, state, None) is None:
            raise RuntimeError(self._TRAIN_ORDER[state])
        x = self.to_device_u8(x) if u8 else self.to_device(x)
        b = x.shape[0]
        gt_dev, gc_dev, max_gt = self._loss_gts(gts, b)
        if result is None:
            result = torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        name += "_u8" if u8 else ""
        with torch.cuda.device(self.device):
            _hip.check(getattr(self.lib, name)(self.handle, x.data_ptr(), b, gt_dev.data_ptr(), gc_dev.data_ptr(), int(max_gt), *extra,
                                               getattr(self, state).data_ptr(), float(lr_t), result.data_ptr(), self._stream()), name)
        self.u8_calls += int(u8)
        self._loss_keep = (x, gt_dev, gc_dev)      # (alive until the next call: the work is only enqueued)
        return result

    def set_wgrad_f16(self, on=True):
        """The weight gradient of the trained 3 x 3 blocks on the fp16 matrix cores (yolo_net_train_set_wgrad_f16): train_tail_step[_u8] and
        train_blocks_step_v3[_u8] then run yolo_conv3x3_wgrad_f16 in place of yolo_conv3x3_wgrad, in a buffer this engine owns.
        on=False: back to the float32 steps, bit for bit.  Before or after a *_train_init*; raises the library's refusal for a float32 plan
        or a net without such a block."""
        torch = self.torch
        with torch.cuda.device(self.device):
            if not on:
                torch.cuda.synchronize(self.device)       # (a step that still runs in the buffer)
                _hip.check(self.lib.yolo_net_train_set_wgrad_f16(self.handle, None, 0), "yolo_net_train_set_wgrad_f16")
                self._wgrad_f16_buf = None
                return
            need = int(self.lib.yolo_net_train_wgrad_f16_bytes(self.handle))
            if not need:
                raise _hip.YoloHipError("yolo_net_train_wgrad_f16_bytes failed: %s" % (self.lib.yolo_last_error() or b"").decode())
            buf = torch.empty(need, dtype=torch.uint8, device=self.device)
            _hip.check(self.lib.yolo_net_train_set_wgrad_f16(self.handle, buf.data_ptr(), buf.numel()), "yolo_net_train_set_wgrad_f16")
            self._wgrad_f16_buf = buf

    # -- training the detection layer (yolo_net_head_train_init / yolo_net_train_head_step / yolo_net_head_train_read) ------------------
    def head_train_init(self, head_w, head_b):
        """Allocate the head-training state and start it from head_w [cout, cin] (the Darknet kernel, [out][in]) and head_b [cout]: master
        values, zeroed moments, and the layer packed into the device weights.  Synchronous.  A net whose streams = 0 rule runs two halves is
        set to one pass first (each part has its own arena)."""
        torch = self._train_begin()
        lay = self.head_train_layout()
        w = np.ascontiguousarray(head_w, dtype=np.float32).reshape(-1)
        b = np.ascontiguousarray(head_b, dtype=np.float32).reshape(-1)
        if w.size != lay.cout * lay.cin or b.size != lay.cout:
            raise ValueError("expected a head kernel of %d x %d values and %d biases, got %d and %d" % (lay.cout, lay.cin, lay.cout, w.size, b.size))
        with torch.cuda.device(self.device):
            self._train_state = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device=self.device)
            _hip.check(self.lib.yolo_net_head_train_init(self.handle, self._train_state.data_ptr(), self._train_state.numel(), w.ctypes.data,
                                                         b.ctypes.data), "yolo_net_head_train_init")
        self.train_layout = lay
        return self._train_state

    def train_head_step(self, x, gts, lr_t, result=None):
        """One training step of the detection layer in one enqueue, no host sync (include/yolo_hip.h: yolo_net_train_head_step): dense
        forward, loss and its gradient, weight gradient, Adam update and re-pack.  lr_t: adam_lr_t(lr, step).  Returns the device record
        (uint8 [64] = yolo_loss_result) of the loss BEFORE the update; `result`: a caller's tensor to write it into."""
        return self._train_step("yolo_net_train_head_step", "_train_state", x, gts, lr_t, False, result)

    def train_head_step_u8(self, x, gts, lr_t, result=None):
        """train_head_step() for a uint8 batch [B,H,W,C] (0..255, RGB): the same bits as train_head_step(float32(x / 255.))"""
        return self._train_step("yolo_net_train_head_step", "_train_state", x, gts, lr_t, True, result)

    def head_train_read(self):
        """The master values of the detection layer (synchronous): (kernel float32 [cout, cin], bias float32 [cout])"""
        lay = self.train_layout
        w = np.empty((lay.cout, lay.cin), dtype=np.float32)
        b = np.empty(lay.cout, dtype=np.float32)
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_head_train_read(self.handle, self._train_state.data_ptr(), w.ctypes.data, b.ctypes.data),
                       "yolo_net_head_train_read")
        return w, b

    # -- training the tail of a YOLOv2 net (yolo_net_tail_train_init / yolo_net_train_tail_step / yolo_net_tail_train_read) -------------
    def tail_train_init(self, block, head_w, head_b):
        """Allocate the tail-training state and start it from `block` -- the 3 x 3 block's piece of the Darknet stream: beta, gamma, moving
        mean, moving variance [cout3 each], then the kernel [out][in][kh][kw] --, head_w [cout, cin] and head_b [cout]: master values,
        zeroed moments, the fold's scale, and both layers packed into the device weights.  Synchronous.  A net whose streams = 0 rule runs
        two halves is set to one pass first (each part has its own arena)."""
        torch = self._train_begin()
        lay = self.tail_train_layout()
        blk = np.ascontiguousarray(block, dtype=np.float32).reshape(-1)
        w = np.ascontiguousarray(head_w, dtype=np.float32).reshape(-1)
        b = np.ascontiguousarray(head_b, dtype=np.float32).reshape(-1)
        if blk.size != lay.cout3 * (4 + 9 * lay.cin3) or w.size != lay.cout * lay.cin or b.size != lay.cout:
            raise ValueError("expected a block of %d values, a head kernel of %d x %d values and %d biases, got %d, %d and %d"
                             % (lay.cout3 * (4 + 9 * lay.cin3), lay.cout, lay.cin, lay.cout, blk.size, w.size, b.size))
        with torch.cuda.device(self.device):
            self._tail_state = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device=self.device)
            _hip.check(self.lib.yolo_net_tail_train_init(self.handle, self._tail_state.data_ptr(), self._tail_state.numel(), blk.ctypes.data,
                                                         w.ctypes.data, b.ctypes.data), "yolo_net_tail_train_init")
        self.tail_layout = lay
        return self._tail_state

    def train_tail_step(self, x, gts, lr_t, result=None):
        """One training step of the last 3 x 3 block and the detection layer in one enqueue, no host sync (include/yolo_hip.h:
        yolo_net_train_tail_step): dense forward, loss and its gradient, the head's weight gradient, the data gradient, the block's weight
        gradient, Adam update and re-pack of both layers.  lr_t: adam_lr_t(lr, step).  Returns the device record (uint8 [64] =
        yolo_loss_result) of the loss BEFORE the update; `result`: a caller's tensor to write it into."""
        return self._train_step("yolo_net_train_tail_step", "_tail_state", x, gts, lr_t, False, result)

    def train_tail_step_u8(self, x, gts, lr_t, result=None):
        """train_tail_step() for a uint8 batch [B,H,W,C] (0..255, RGB): the same bits as train_tail_step(float32(x / 255.))"""
        return self._train_step("yolo_net_train_tail_step", "_tail_state", x, gts, lr_t, True, result)

    def tail_train_read(self):
        """The master values of the tail (synchronous): (block kernel float32 [cout3, cin3, 3, 3] as the Darknet stream holds it, beta
        [cout3], head kernel [cout, cin], head bias [cout])"""
        lay = self.tail_layout
        k3 = np.empty((lay.cout3, lay.cin3, 3, 3), dtype=np.float32)
        beta = np.empty(lay.cout3, dtype=np.float32)
        w = np.empty((lay.cout, lay.cin), dtype=np.float32)
        b = np.empty(lay.cout, dtype=np.float32)
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_tail_train_read(self.handle, self._tail_state.data_ptr(), k3.ctypes.data, beta.ctypes.data,
                                                         w.ctypes.data, b.ctypes.data), "yolo_net_tail_train_read")
        return k3, beta, w, b

    # -- training the YOLOv3 head convs (yolo_net_head_inputs_v3 / yolo_net_head_train_v3_* / yolo_net_train_head_step_v3) ----------------
    def head_train_init_v3(self, head_ws, head_bs):
        """Allocate the YOLOv3 head-training state and start it from head_ws[s] [cout_s, cin_s] (the Darknet kernels, [out][in]) and
        head_bs[s] [cout_s], in head order: master values, zeroed moments, and the convs packed into the device weights.  Synchronous.  A
        net whose streams = 0 rule runs two halves is set to one pass first (each part has its own arena)."""
        torch = self._train_begin()
        lay = self.head_train_layout_v3()
        if len(head_ws) != lay.n_scales or len(head_bs) != lay.n_scales:
            raise ValueError("expected %d head kernels and biases, one per scale" % lay.n_scales)
        ws = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in head_ws]
        bs = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in head_bs]
        for s in range(lay.n_scales):
            if ws[s].size != lay.cout[s] * lay.cin[s] or bs[s].size != lay.cout[s]:
                raise ValueError("scale %d: expected a head kernel of %d x %d values and %d biases, got %d and %d"
                                 % (s, lay.cout[s], lay.cin[s], lay.cout[s], ws[s].size, bs[s].size))
        wp = (C.c_void_p * _hip.MAX_SCALES)(*[w.ctypes.data for w in ws])
        bp = (C.c_void_p * _hip.MAX_SCALES)(*[b.ctypes.data for b in bs])
        with torch.cuda.device(self.device):
            self._train_state_v3 = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device=self.device)
            _hip.check(self.lib.yolo_net_head_train_v3_init(self.handle, self._train_state_v3.data_ptr(), self._train_state_v3.numel(), wp, bp),
                       "yolo_net_head_train_v3_init")
        self.train_layout_v3 = lay
        return self._train_state_v3

    def train_head_step_v3(self, x, gts, lr_t, ignore_thresh=0.7, result=None):
        """One training step of the head convs of a YOLOv3 network in one enqueue, no host sync (include/yolo_hip.h:
        yolo_net_train_head_step_v3): dense forward, the YOLOv3 loss and its gradient, the sparse weight gradient, Adam update and re-pack
        per scale.  lr_t: adam_lr_t(lr, step).  Returns the device record (uint8 [64] = yolo_loss_result) of the loss BEFORE the update."""
        return self._train_step("yolo_net_train_head_step_v3", "_train_state_v3", x, gts, lr_t, False, result, float(ignore_thresh))

    def train_head_step_v3_u8(self, x, gts, lr_t, ignore_thresh=0.7, result=None):
        """train_head_step_v3() for a uint8 batch [B,H,W,C] (0..255, RGB): the same bits as train_head_step_v3(float32(x / 255.))"""
        return self._train_step("yolo_net_train_head_step_v3", "_train_state_v3", x, gts, lr_t, True, result, float(ignore_thresh))

    def head_train_read_v3(self):
        """The master values of the head convs (synchronous): ([kernel float32 [cout_s, cin_s]], [bias float32 [cout_s]]) in head order"""
        lay = self.train_layout_v3
        ws = [np.empty((lay.cout[s], lay.cin[s]), dtype=np.float32) for s in range(lay.n_scales)]
        bs = [np.empty(lay.cout[s], dtype=np.float32) for s in range(lay.n_scales)]
        wp = (C.c_void_p * _hip.MAX_SCALES)(*[w.ctypes.data for w in ws])
        bp = (C.c_void_p * _hip.MAX_SCALES)(*[b.ctypes.data for b in bs])
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_head_train_v3_read(self.handle, self._train_state_v3.data_ptr(), wp, bp), "yolo_net_head_train_v3_read")
        return ws, bs

    # -- training the YOLOv3 head convs and the 3 x 3 blocks behind them (yolo_net_blocks_train_v3_* / yolo_net_train_blocks_step_v3) --------
    def blocks_train_init_v3(self, blocks, head_ws, head_bs):
        """Allocate the state that trains the head convs of a YOLOv3 network and the 3 x 3 block behind each, and start it, in head order,
        from blocks[s] -- block s's piece of the Darknet stream: beta, gamma, moving mean, moving variance [cout3 each], then the kernel
        [out][in][kh][kw] --, head_ws[s] [cout_s, cin_s] and head_bs[s] [cout_s]: master values, zeroed moments, the folds' scales, and
        every conv packed into the device weights.  Synchronous.  A net whose streams = 0 rule runs two halves is set to one pass first."""
        torch = self._train_begin()
        lay = self.blocks_train_layout_v3()
        ns = lay.n_scales
        if len(blocks) != ns or len(head_ws) != ns or len(head_bs) != ns:
            raise ValueError("expected %d blocks, head kernels and biases, one per scale" % ns)
        ks = [np.ascontiguousarray(k, dtype=np.float32).reshape(-1) for k in blocks]
        ws = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in head_ws]
        bs = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in head_bs]
        for s in range(ns):
            if ks[s].size != lay.cout3[s] * (4 + 9 * lay.cin3[s]) or ws[s].size != lay.cout[s] * lay.cin[s] or bs[s].size != lay.cout[s]:
                raise ValueError("scale %d: expected a block of %d values, a head kernel of %d x %d values and %d biases, got %d, %d and %d"
                                 % (s, lay.cout3[s] * (4 + 9 * lay.cin3[s]), lay.cout[s], lay.cin[s], lay.cout[s], ks[s].size, ws[s].size, bs[s].size))
        ptrs = lambda arrs: (C.c_void_p * _hip.MAX_SCALES)(*[a.ctypes.data for a in arrs])
        with torch.cuda.device(self.device):
            self._blocks_state_v3 = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device=self.device)
            _hip.check(self.lib.yolo_net_blocks_train_v3_init(self.handle, self._blocks_state_v3.data_ptr(), self._blocks_state_v3.numel(), ptrs(ks),
                                                              ptrs(ws), ptrs(bs)), "yolo_net_blocks_train_v3_init")
        self.blocks_layout_v3 = lay
        return self._blocks_state_v3

    def train_blocks_step_v3(self, x, gts, lr_t, ignore_thresh=0.7, result=None):
        """One training step of the head convs of a YOLOv3 network and the 3 x 3 blocks behind them in one enqueue, no host sync
        (include/yolo_hip.h: yolo_net_train_blocks_step_v3): dense forward, the YOLOv3 loss and its gradient, the heads' sparse weight
        gradient, per scale the sparse data gradient and the block's weight gradient, Adam update and re-pack of every conv.  lr_t:
        adam_lr_t(lr, step).  Returns the device record (uint8 [64] = yolo_loss_result) of the loss BEFORE the update."""
        return self._train_step("yolo_net_train_blocks_step_v3", "_blocks_state_v3", x, gts, lr_t, False, result, float(ignore_thresh))

    def train_blocks_step_v3_u8(self, x, gts, lr_t, ignore_thresh=0.7, result=None):
        """train_blocks_step_v3() for a uint8 batch [B,H,W,C] (0..255, RGB): the same bits as train_blocks_step_v3(float32(x / 255.))"""
        return self._train_step("yolo_net_train_blocks_step_v3", "_blocks_state_v3", x, gts, lr_t, True, result, float(ignore_thresh))

    def blocks_train_read_v3(self):
        """The master values (synchronous), in head order: ([block kernel float32 [cout3, cin3, 3, 3] as the Darknet stream holds it], [beta
        [cout3]], [head kernel [cout_s, cin_s]], [head bias [cout_s]])"""
        lay = self.blocks_layout_v3
        ns = lay.n_scales
        k3 = [np.empty((lay.cout3[s], lay.cin3[s], 3, 3), dtype=np.float32) for s in range(ns)]
        beta = [np.empty(lay.cout3[s], dtype=np.float32) for s in range(ns)]
        ws = [np.empty((lay.cout[s], lay.cin[s]), dtype=np.float32) for s in range(ns)]
        bs = [np.empty(lay.cout[s], dtype=np.float32) for s in range(ns)]
        ptrs = lambda arrs: (C.c_void_p * _hip.MAX_SCALES)(*[a.ctypes.data for a in arrs])
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_blocks_train_v3_read(self.handle, self._blocks_state_v3.data_ptr(), ptrs(k3), ptrs(beta), ptrs(ws), ptrs(bs)),
                       "yolo_net_blocks_train_v3_read")
        return k3, beta, ws, bs

    def forward_timed_u8(self, x, out=None):
        """forward_timed() for a uint8 batch: the input kernel's entry is the time of its uint8 twin."""
        torch = self.torch
        x = self.to_device_u8(x)
        b = x.shape[0]
        if out is None:
            out = torch.empty((b,) + tuple(self.output_shape), dtype=torch.float32, device=self.device)
        ms = np.zeros(self.num_kernels, dtype=np.float32)
        with torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_forward_timed_u8(self.handle, x.data_ptr(), b, out.data_ptr(), self._stream(),
                                                          ms.ctypes.data), "yolo_net_forward_timed_u8")
        self.u8_calls += 1
        return ms

    def autotune(self, x):
        """Pick the fastest conv tile per layer by timing them on the device (optional, synchronous)."""
        x = self.to_device(x)
        with self.torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_autotune(self.handle, x.data_ptr(), x.shape[0], self._stream()), "yolo_net_autotune")

    def kernel_infos(self):
        out = []
        for k in range(self.num_kernels):
            ki = _hip.KernelInfo()
            _hip.check(self.lib.yolo_net_kernel_info(self.handle, k, C.byref(ki)), "yolo_net_kernel_info")
            out.append(ki)
        return out

    def forward_timed(self, x, out=None):
        """Instrumented forward: device milliseconds of every kernel (hipEvents on the launch stream)."""
        torch = self.torch
        x = self.to_device(x)
        b = x.shape[0]
        if out is None:
            out = torch.empty((b,) + tuple(self.output_shape), dtype=torch.float32, device=self.device)
        ms = np.zeros(self.num_kernels, dtype=np.float32)
        with torch.cuda.device(self.device):
            _hip.check(self.lib.yolo_net_forward_timed(self.handle, x.data_ptr(), b, out.data_ptr(), self._stream(),
                                                       ms.ctypes.data), "yolo_net_forward_timed")
        return ms

    def read_layer(self, index, batch):
        """Dense float32 NHWC copy of one layer's output (needs keep_all=True)."""
        h, w, c = self.layers[index].out.hwc
        host = np.empty((batch, h, w, c), dtype=np.float32)
        _hip.check(self.lib.yolo_net_read_layer(self.handle, index, batch, host.ctypes.data, host.size), "yolo_net_read_layer")
        return host


def adam_lr_t(lr, step, beta1=0.9, beta2=0.999):
    """tf.train.AdamOptimizer's step size for step = 1, 2, ...: lr * sqrt(1 - beta2^t) / (1 - beta1^t), in float64, rounded to float32 once"""
    t = float(step)
    return np.float32(float(lr) * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t))


def loss_gts(torch, device, gts, b):
    """gts -> (gt_dev uint8 [b, max_gt * 24], counts_dev int32 [b], max_gt): a list per image of (x, y, w, h, class_idx[, difficult]),
    the pair of evaluate.pack_gts, or the device tensors of Evaluator.upload_gts (their [lo:hi] slices)"""
    from . import evaluate as yeval
    if isinstance(gts, tuple) and isinstance(gts[0], torch.Tensor):
        gt_dev, gc_dev = gts
        isz = yeval.GT_DTYPE.itemsize
        if (gt_dev.device != device or gc_dev.device != device or gt_dev.dtype != torch.uint8 or gc_dev.dtype != torch.int32
                or gt_dev.dim() != 2 or gt_dev.shape[0] != b or gt_dev.shape[1] % isz or gt_dev.shape[1] == 0 or tuple(gc_dev.shape) != (b,)
                or not gt_dev.is_contiguous() or not gc_dev.is_contiguous()):
            raise ValueError("expected the [%d] slice of upload_gts" % b)
        return gt_dev, gc_dev, gt_dev.shape[1] // isz
    if isinstance(gts, tuple):
        arr, gcounts = gts
    else:
        arr, gcounts = yeval.pack_gts(gts, max(1, max([len(g) for g in gts] or [1])))
    if arr.ndim != 2 or arr.shape[0] != b or arr.dtype != yeval.GT_DTYPE or len(gcounts) != b:
        raise ValueError("expected truths [%d, max_gt] of GT_DTYPE with %d counts" % (b, b))
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(b, -1)
    return (torch.from_numpy(raw).to(device), torch.from_numpy(np.ascontiguousarray(gcounts, dtype=np.int32)).to(device),
            arr.shape[1])


def v2_loss_grad(head, logits, gts):
    """yolo_v2_loss_grad on float32 device logits [B, ...] (contiguous, B * h * w * A * (5 + C) values) with a version 2 head: the loss
    kernels and the gradient kernel in one enqueue on the current stream, no host sync.  gts as HipNetwork.loss takes them.  Returns device
    tensors (images uint8 [B, 56], result uint8 [64], assign int32 [B, h, w], grad float32 of the logits' shape) and the pair of uploaded
    truths, which the caller keeps alive with the logits until the work has run."""
    from . import evaluate as yeval
    torch = _torch()
    dev, b = logits.device, logits.shape[0]
    gt_dev, gc_dev, max_gt = loss_gts(torch, dev, gts, b)
    images = torch.empty((b, yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    result = torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    assign = torch.empty((b, head.h[0], head.w[0]), dtype=torch.int32, device=dev)
    grad = torch.empty_like(logits)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().yolo_v2_loss_grad(C.byref(head), logits.data_ptr(), b, gt_dev.data_ptr(), gc_dev.data_ptr(), int(max_gt),
                                                images.data_ptr(), assign.data_ptr(), result.data_ptr(), grad.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "yolo_v2_loss_grad")
    return images, result, assign, grad, (gt_dev, gc_dev)


def v3_loss_rows(head):
    """yolo_v3_loss_rows: (rows per image R, partial records per image) of a version 3 head"""
    rows, parts = C.c_int64(0), C.c_int32(0)
    _hip.check(_hip.lib().yolo_v3_loss_rows(C.byref(head), C.byref(rows), C.byref(parts)), "yolo_v3_loss_rows")
    return int(rows.value), int(parts.value)


def v3_loss_grad(head, logits, gts, ignore_thresh=0.7):
    """yolo_v3_loss_grad on float32 device logits [B, R, 5 + C] (contiguous) with a version 3 head: the loss kernels and the gradient
    kernel in one enqueue on the current stream, no host sync.  gts as HipNetwork.loss takes them.  Returns device tensors (images uint8
    [B, 56], result uint8 [64], assign int32 [B, R], grad float32 of the logits' shape) and the tensors the caller keeps alive with the
    logits until the work has run."""
    from . import evaluate as yeval
    torch = _torch()
    dev, b = logits.device, logits.shape[0]
    rows, parts = v3_loss_rows(head)
    if logits.numel() != b * rows * (5 + head.n_classes):
        raise ValueError("logits: expected %d x %d x %d values, got %d" % (b, rows, 5 + head.n_classes, logits.numel()))
    gt_dev, gc_dev, max_gt = loss_gts(torch, dev, gts, b)
    scratch = torch.empty((b, parts, yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    images = torch.empty((b, yeval.LOSS_IMAGE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    result = torch.empty(yeval.LOSS_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    assign = torch.empty((b, rows), dtype=torch.int32, device=dev)
    grad = torch.empty_like(logits)
    with torch.cuda.device(dev):
        _hip.check(_hip.lib().yolo_v3_loss_grad(C.byref(head), logits.data_ptr(), b, gt_dev.data_ptr(), gc_dev.data_ptr(), int(max_gt),
                                                float(ignore_thresh), scratch.data_ptr(), images.data_ptr(), assign.data_ptr(), result.data_ptr(),
                                                grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "yolo_v3_loss_grad")
    return images, result, assign, grad, (gt_dev, gc_dev, scratch)


def v3_head_wgrad(head, xs, grad, assign, max_gt, scratch=None, out=None):
    """yolo_v3_head_wgrad: the weight gradient of the head convs of a version 3 head from the gradient and the table of v3_loss_grad
    (float32 [B, R, 5 + C] and int32 [B, R] device tensors), one enqueue on the current stream, no host sync.  xs: per scale, in head
    order, the conv's input -- a contiguous fp16 / float32 device tensor [B, h_s, w_s, cin_s], or (flat tensor, ld, coff, image_stride,
    cin) for a strided view of it (element (n, q, c) at n * image_stride + q * ld + coff + c).  scratch: a uint8 device tensor to run in
    (tests pre-fill it), else one is allocated; out: ([dW_s], [db_s]) to write into.  Returns ([dW_s float32 [cout_s, cin_s]], [db_s
    float32 [cout_s]], scratch); the caller keeps the inputs alive until the work has run."""
    torch = _torch()
    dev, b, ns = grad.device, grad.shape[0], head.n_scales
    if len(xs) != ns:
        raise ValueError("v3_head_wgrad: expected %d inputs, one per scale, got %d" % (ns, len(xs)))
    views = (_hip.V3WgradView * _hip.MAX_SCALES)()
    for s, x in enumerate(xs):
        if isinstance(x, (tuple, list)):
            t, ld, coff, image_stride, cin = x
        else:
            if not x.is_contiguous() or x.dim() != 4 or x.shape[0] != b or tuple(x.shape[1:3]) != (head.h[s], head.w[s]):
                raise ValueError("v3_head_wgrad: scale %d: expected a contiguous [%d, %d, %d, cin] tensor" % (s, b, head.h[s], head.w[s]))
            t, cin = x, x.shape[3]
            ld, coff, image_stride = cin, 0, head.h[s] * head.w[s] * cin
        if t.dtype not in (torch.float16, torch.float32):
            raise ValueError("v3_head_wgrad: scale %d: the input must be fp16 or float32" % s)
        views[s].x_dev, views[s].image_stride, views[s].ld, views[s].coff = t.data_ptr(), int(image_stride), int(ld), int(coff)
        views[s].dtype, views[s].cin = (_hip.DTYPE_F16 if t.dtype == torch.float16 else _hip.DTYPE_F32), int(cin)
    cins = [views[s].cin for s in range(ns)]
    pl = _hip.v3_head_wgrad_plan(head, cins, b, views[0].dtype)
    with torch.cuda.device(dev):
        if scratch is None:
            scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device=dev)
        if out is None:
            couts = [head.n_anchors[s] * (5 + head.n_classes) for s in range(ns)]
            out = ([torch.empty((couts[s], cins[s]), dtype=torch.float32, device=dev) for s in range(ns)],
                   [torch.empty(couts[s], dtype=torch.float32, device=dev) for s in range(ns)])
        dws = (C.c_void_p * _hip.MAX_SCALES)(*[t.data_ptr() for t in out[0]])
        dbs = (C.c_void_p * _hip.MAX_SCALES)(*[t.data_ptr() for t in out[1]])
        _hip.check(_hip.lib().yolo_v3_head_wgrad(C.byref(head), views, b, grad.data_ptr(), assign.data_ptr(), int(max_gt), dws, dbs,
                                                 scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream),
                   "yolo_v3_head_wgrad")
    return out[0], out[1], scratch


def _nhwc_view(torch, x, who):
    """a contiguous fp16 / float32 [B, h, w, c] device tensor, or (flat tensor, ld, coff, image_stride, (B, h, w, c)) for a strided view of
    one (element (n, q, c) at n * image_stride + q * ld + coff + c) -> (tensor, dtype code, ld, coff, image_stride, (B, h, w, c))"""
    if isinstance(x, (tuple, list)):
        t, ld, coff, image_stride, shape = x
    else:
        if x.dim() != 4 or not x.is_contiguous():
            raise ValueError("%s: expected a contiguous [B, h, w, c] tensor or a view tuple" % who)
        t, shape = x, tuple(x.shape)
        ld, coff, image_stride = shape[3], 0, shape[1] * shape[2] * shape[3]
    if t.dtype not in (torch.float16, torch.float32):
        raise ValueError("%s: the view must be fp16 or float32" % who)
    return t, (_hip.DTYPE_F16 if t.dtype == torch.float16 else _hip.DTYPE_F32), int(ld), int(coff), int(image_stride), tuple(int(v) for v in shape)


def conv1x1_dgrad(grad, weight, y=None, slope=0.1, out=None):
    """yolo_conv1x1_dgrad: D[p][c] = (sum_o G[p][o] W[o][c]) * (Y[p][c] > 0 ? 1 : slope), one enqueue on the current stream, no host sync.
    grad: float32 device tensor [B, h, w, cout] (or [P, cout] when y is None); weight: the float32 MASTER kernel [cout, cin]; y: the stored
    output of the block in front -- as _nhwc_view takes it -- or None for no activation factor; out: a float32 [P, cin] tensor to write into
    (tests pre-fill it).  Returns D float32 [P, cin]; the caller keeps the inputs alive until the work has run."""
    torch = _torch()
    dev = grad.device
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if grad.dtype != torch.float32 or weight.dtype != torch.float32 or not grad.is_contiguous() or not weight.is_contiguous() or grad.shape[-1] != cout:
        raise ValueError("conv1x1_dgrad: expected contiguous float32 grad [..., %d] and weight [%d, %d]" % (cout, cout, cin))
    P = grad.numel() // cout
    if y is None:
        yt, ydt, ld, coff, istride, ppi, b = None, 0, 0, 0, 0, P, 1
    else:
        yt, ydt, ld, coff, istride, shape = _nhwc_view(torch, y, "conv1x1_dgrad")
        b, ppi = shape[0], shape[1] * shape[2]
        if b * ppi != P or shape[3] != cin:
            raise ValueError("conv1x1_dgrad: y is %r, expected %d positions of %d channels" % (shape, P, cin))
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((P, cin), dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().yolo_conv1x1_dgrad(grad.data_ptr(), cout, weight.data_ptr(), cin, yt.data_ptr() if yt is not None else None, ydt,
                                                 ld, coff, istride, ppi, b, float(slope), out.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "yolo_conv1x1_dgrad")
    return out


def v3_head_dgrad(head, scale, grad, assign, max_gt, weight, y=None, slope=0.1, out=None):
    """yolo_v3_head_dgrad: D_s[p][c] = (sum_o G_s[p][o] W_s[o][c]) * (Y_s[p][c] > 0 ? 1 : slope) for the head conv of scale `scale` of a
    version 3 head, the sum over the terms the assign table does not declare a structural zero; one enqueue on the current stream, no host
    sync.  grad, assign: the float32 [B, R, 5 + C] gradient and the int32 [B, R] table of v3_loss_grad, read in place; weight: the
    float32 MASTER kernel [cout_s, cin]; y: the stored output of the block in front -- as _nhwc_view takes it -- or None for no
    activation factor; out: a float32 [P_s, cin] tensor to write into (tests pre-fill it).  Returns D float32 [P_s, cin]; the caller keeps
    the inputs alive until the work has run."""
    torch = _torch()
    dev, b = grad.device, int(grad.shape[0])
    if not 0 <= int(scale) < head.n_scales:
        raise ValueError("v3_head_dgrad: scale must be 0..%d" % (head.n_scales - 1))
    scale = int(scale)
    cout, cin = head.n_anchors[scale] * (5 + head.n_classes), int(weight.shape[1])
    if (grad.dtype != torch.float32 or weight.dtype != torch.float32 or assign.dtype != torch.int32 or not grad.is_contiguous()
            or not weight.is_contiguous() or not assign.is_contiguous() or weight.shape[0] != cout):
        raise ValueError("v3_head_dgrad: expected contiguous float32 grad, int32 assign and a float32 weight [%d, cin]" % cout)
    rows, _ = v3_loss_rows(head)
    if grad.numel() != b * rows * (5 + head.n_classes) or assign.numel() != b * rows:
        raise ValueError("v3_head_dgrad: expected grad [%d, %d, %d] and assign [%d, %d]" % (b, rows, 5 + head.n_classes, b, rows))
    P = b * head.h[scale] * head.w[scale]
    if y is None:
        yt, ydt, ld, coff, istride = None, 0, 0, 0, 0
    else:
        yt, ydt, ld, coff, istride, shape = _nhwc_view(torch, y, "v3_head_dgrad")
        if shape != (b, head.h[scale], head.w[scale], cin):
            raise ValueError("v3_head_dgrad: y is %r, expected %r" % (shape, (b, head.h[scale], head.w[scale], cin)))
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((P, cin), dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().yolo_v3_head_dgrad(C.byref(head), scale, grad.data_ptr(), assign.data_ptr(), int(max_gt), b, weight.data_ptr(), cin,
                                                 yt.data_ptr() if yt is not None else None, ydt, ld, coff, istride, float(slope), out.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream), "yolo_v3_head_dgrad")
    return out


def conv3x3_wgrad(x, d, scale=None, scratch=None, out=None):
    """yolo_conv3x3_wgrad: the gradient of a 3 x 3 / stride 1 / SAME conv with respect to its kernel and bias, from the gradient D of its
    output, one enqueue on the current stream, no host sync.  x: the conv's input as _nhwc_view takes it; d: float32 device tensor
    [B * h * w, cout] (contiguous); scale: float32 [cout] (the fold's scale: dW3 = scale * R) or None; scratch: a uint8 device tensor to run
    in (tests pre-fill it), else one is allocated; out: (dW3, db) to write into.  Returns (dW3 float32 [cout, 9, cin], db float32 [cout],
    scratch); the caller keeps the inputs alive until the work has run."""
    torch = _torch()
    dev = d.device
    xt, xdt, ld, coff, istride, (b, h, w, cin) = _nhwc_view(torch, x, "conv3x3_wgrad")
    if d.dtype != torch.float32 or not d.is_contiguous() or d.dim() != 2 or d.shape[0] != b * h * w:
        raise ValueError("conv3x3_wgrad: expected a contiguous float32 gradient [%d, cout]" % (b * h * w))
    cout = int(d.shape[1])
    if scale is not None and (scale.dtype != torch.float32 or not scale.is_contiguous() or scale.numel() != cout):
        raise ValueError("conv3x3_wgrad: expected a contiguous float32 scale [%d]" % cout)
    pl = _hip.conv3x3_wgrad_plan(h, w, b, cin, cout, xdt)
    with torch.cuda.device(dev):
        if scratch is None:
            scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device=dev)
        if out is None:
            out = (torch.empty((cout, 9, cin), dtype=torch.float32, device=dev), torch.empty(cout, dtype=torch.float32, device=dev))
        _hip.check(_hip.lib().yolo_conv3x3_wgrad(xt.data_ptr(), xdt, ld, coff, istride, h, w, b, cin, d.data_ptr(), cout,
                                                 scale.data_ptr() if scale is not None else None, out[0].data_ptr(), out[1].data_ptr(),
                                                 scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream),
                   "yolo_conv3x3_wgrad")
    return out[0], out[1], scratch


def conv3x3_wgrad_f16(x, d, scale=None, scratch=None, out=None):
    """yolo_conv3x3_wgrad_f16: conv3x3_wgrad() with D narrowed to fp16 by one power of two per call, on the fp16 matrix cores (the
    definition: include/yolo_hip.h).  x must be an fp16 view; the other arguments and the result are conv3x3_wgrad()'s.  The scratch ends
    with the call's m / k record, at yolo_conv3x3_wgrad_f16_plan's record_offset."""
    torch = _torch()
    dev = d.device
    xt, xdt, ld, coff, istride, (b, h, w, cin) = _nhwc_view(torch, x, "conv3x3_wgrad_f16")
    if d.dtype != torch.float32 or not d.is_contiguous() or d.dim() != 2 or d.shape[0] != b * h * w:
        raise ValueError("conv3x3_wgrad_f16: expected a contiguous float32 gradient [%d, cout]" % (b * h * w))
    cout = int(d.shape[1])
    if scale is not None and (scale.dtype != torch.float32 or not scale.is_contiguous() or scale.numel() != cout):
        raise ValueError("conv3x3_wgrad_f16: expected a contiguous float32 scale [%d]" % cout)
    with torch.cuda.device(dev):
        if scratch is None:
            scratch = torch.empty(_hip.conv3x3_wgrad_f16_plan(h, w, b, cin, cout)["scratch_bytes"], dtype=torch.uint8, device=dev)
        if out is None:
            out = (torch.empty((cout, 9, cin), dtype=torch.float32, device=dev), torch.empty(cout, dtype=torch.float32, device=dev))
        _hip.check(_hip.lib().yolo_conv3x3_wgrad_f16(xt.data_ptr(), xdt, ld, coff, istride, h, w, b, cin, d.data_ptr(), cout,
                                                     scale.data_ptr() if scale is not None else None, out[0].data_ptr(), out[1].data_ptr(),
                                                     scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream),
                   "yolo_conv3x3_wgrad_f16")
    return out[0], out[1], scratch


def anchor_plan(n, k, distance=_hip.ANCHOR_EUCLIDEAN, tolerate=0.005, n_init=10, max_iter=300, seed=0):
    """yolo_anchor_plan as a dict (host only): chunk, n_chunks, period, the offsets of the scratch's and the result's parts, both sizes"""
    return _hip.anchor_plan(_hip.anchor_desc(k, n_init, max_iter, distance, tolerate, seed), n)


def anchor_result(raw, plan, n_init):
    """The result block of yolo_anchor_kmeans (raw: its bytes on the host, a uint8 array) -> dict: the header's fields, `restarts` (a list
    of dicts: n_iter, status, inertia_q, iou_q, seeds) and the best block's fields as NumPy arrays / ints / floats"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    hdr = _hip.AnchorHeader.from_buffer_copy(raw[plan["header_offset"]:].tobytes()[:C.sizeof(_hip.AnchorHeader)])
    out = {name: int(getattr(hdr, name)) for name, _ in _hip.AnchorHeader._fields_ if name != "pad_"}
    size = C.sizeof(_hip.AnchorRestart)
    table = raw[plan["restarts_offset"]:plan["restarts_offset"] + n_init * size].tobytes()
    out["restarts"] = []
    for r in range(n_init):
        row = _hip.AnchorRestart.from_buffer_copy(table[r * size:(r + 1) * size])
        out["restarts"].append(dict(n_iter=int(row.n_iter), status=int(row.status), inertia_q=int(row.inertia_q), iou_q=int(row.iou_q),
                                    seeds=[int(v) for v in row.seeds]))
    best = _hip.AnchorBest.from_buffer_copy(raw[plan["best_offset"]:].tobytes()[:C.sizeof(_hip.AnchorBest)])
    out["centres"] = np.array([[c[0], c[1]] for c in best.centres], dtype=np.float64)
    out["counts"] = np.array(list(best.counts), dtype=np.int64)
    out["sum_q"] = np.array([[c[0], c[1]] for c in best.sum_q], dtype=np.uint64)
    out["inertia_q"], out["iou_q"] = int(best.inertia_q), int(best.iou_q)
    out["inertia"], out["avg_iou"] = float(best.inertia), float(best.avg_iou)
    return out


def anchor_kmeans(wh, k, distance=_hip.ANCHOR_EUCLIDEAN, tolerate=0.005, n_init=10, max_iter=300, seed=0, init=None, scratch=None,
                  result=None, labels=True):
    """yolo_anchor_kmeans on the device of `wh`: a contiguous float64 device tensor [n, 2] of normalised (w, h).  init: a float64 device
    tensor [k, 2] of starting centres (then n_init must be 1) or None (seeded); scratch / result: uint8 device tensors to run in (tests
    pre-fill them), else allocated; labels: True (an int32 tensor is allocated), a tensor to write into, or False / None (no labels).
    UNLIKE the other operators this call synchronises with the host between batches of iterations.  Returns (dict as anchor_result plus
    "raw": the result block's bytes as a NumPy array, labels tensor or None)."""
    torch = _torch()
    if wh.dtype != torch.float64 or not wh.is_contiguous() or wh.dim() != 2 or wh.shape[1] != 2 or not wh.is_cuda:
        raise ValueError("anchor_kmeans: expected a contiguous float64 device tensor [n, 2]")
    if init is not None and (init.dtype != torch.float64 or not init.is_contiguous() or tuple(init.shape) != (int(k), 2) or init.device != wh.device):
        raise ValueError("anchor_kmeans: expected init as a contiguous float64 tensor [%d, 2] on the device of wh" % int(k))
    dev, n = wh.device, int(wh.shape[0])
    desc = _hip.anchor_desc(k, n_init, max_iter, distance, tolerate, seed)
    pl = _hip.anchor_plan(desc, n)
    with torch.cuda.device(dev):
        if scratch is None:
            scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device=dev)
        if result is None:
            result = torch.empty(pl["result_bytes"], dtype=torch.uint8, device=dev)
        if labels is True:
            labels = torch.empty(n, dtype=torch.int32, device=dev)
        elif labels is False:
            labels = None
        if labels is not None and (labels.dtype != torch.int32 or not labels.is_contiguous() or labels.numel() != n):
            raise ValueError("anchor_kmeans: expected labels as a contiguous int32 tensor [%d]" % n)
        _hip.check(_hip.lib().yolo_anchor_kmeans(C.byref(desc), wh.data_ptr(), n, init.data_ptr() if init is not None else None,
                                                 scratch.data_ptr(), scratch.numel(), result.data_ptr(), result.numel(),
                                                 labels.data_ptr() if labels is not None else None,
                                                 torch.cuda.current_stream(dev).cuda_stream), "yolo_anchor_kmeans")
        raw = result[:pl["result_bytes"]].cpu().numpy()
    out = anchor_result(raw, pl, int(n_init))
    out["raw"] = raw
    return out, labels


def check_status(status, allow_truncation=False):
    """The reference's lists are unbounded (net/base.py:195-209); the record buffers are not.  Both overflow bits mean the
    result would differ from the reference's, so both raise: bit 0 = more candidates than cand_capacity passed the
    threshold, bit 1 = more NMS survivors than max_boxes."""
    status = np.asarray(status).reshape(-1)
    if (status & 1).any():
        raise _hip.YoloHipError("candidate capacity exceeded for image(s) %s: raise cand_capacity or the threshold"
                                % np.nonzero(status & 1)[0].tolist())
    if (status & 2).any() and not allow_truncation:
        raise _hip.YoloHipError("more than max_boxes boxes survive NMS for image(s) %s: the list would be truncated "
                                "(the reference has no cap): raise max_boxes" % np.nonzero(status & 2)[0].tolist())


def records_to_host(boxes, counts, status, allow_truncation=False):
    """Device records -> per-image list of (x, y, w, h, class_idx, prob) tuples (synchronises).
    Raises if a capacity was exceeded (the result would not be the reference's): check_status."""
    boxes = boxes.cpu().numpy()
    counts = counts.cpu().numpy()
    status = status.cpu().numpy()
    check_status(status, allow_truncation)
    out = []
    cls = boxes[..., 5].view(np.int32)
    for i in range(boxes.shape[0]):
        n = int(counts[i])
        b = boxes[i, :n].astype(np.float64).tolist()        # float32 -> the same Python floats as float(np.float32)
        c = cls[i, :n].tolist()
        out.append([(r[0], r[1], r[2], r[3], c[k], r[4]) for k, r in enumerate(b)])
    return out, status


def decode_nms(head, logits, threshold, iou_threshold, nms_mode=_hip.NMS_AGNOSTIC, cand_capacity=4096,
               max_boxes=_hip.DEFAULT_MAX_BOXES, allow_truncation=False):
    """Standalone decode + NMS of a head tensor already on (or copied to) the device:
    the drop-in for find_bounding_boxes (reference net/v2.py:83-90, net/v3.py:140-151)."""
    torch = _torch()
    lib = _hip.lib()
    if not isinstance(logits, torch.Tensor):
        logits = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()
    logits = logits.contiguous().float()
    b = logits.shape[0]
    dev = logits.device
    with torch.cuda.device(dev):
        nbytes = lib.yolo_decode_scratch_bytes(C.byref(head), b, cand_capacity)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        boxes = torch.empty((b, max_boxes, 6), dtype=torch.float32, device=dev)
        counts = torch.zeros((2, b), dtype=torch.int32, device=dev)
        _hip.check(lib.yolo_decode_nms(C.byref(head), logits.data_ptr(), b, float(threshold), float(iou_threshold),
                                       int(nms_mode), cand_capacity, max_boxes, scratch.data_ptr(), nbytes,
                                       boxes.data_ptr(), counts[0].data_ptr(), counts[1].data_ptr(),
                                       torch.cuda.current_stream(dev).cuda_stream), "yolo_decode_nms")
        return records_to_host(boxes, counts[0], counts[1], allow_truncation)

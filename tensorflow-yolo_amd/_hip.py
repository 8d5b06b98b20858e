"""ctypes binding of libyolo_hip.so (C ABI: include/yolo_hip.h).

The HIP library IS the product path: there is no CPU fallback.  Loading fails loudly
(ImportError with the build hint) when the shared object is missing.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (YOLO_HIP_LIB: another build of the SAME library -- the sanitizer build of tests/test_sanitizer.py, A/B builds of tools/; no fallback of any kind)
LIB_PATH = os.environ.get("YOLO_HIP_LIB") or os.path.join(_HERE, "libyolo_hip.so")

ABI_VERSION = 7

# enum yolo_op
OP_INPUT, OP_CONV, OP_MAXPOOL, OP_ROUTE, OP_REORG, OP_SHORTCUT, OP_UPSAMPLE, OP_YOLO, OP_DETECTION = range(9)
DTYPE_F32, DTYPE_F16, DTYPE_MXF8 = 0, 1, 2
NMS_AGNOSTIC, NMS_PER_CLASS = 0, 1
RESIZE_STRETCH, RESIZE_LETTERBOX = 0, 1         # enum yolo_resize_mode
RESIZE_MODES = {"stretch": RESIZE_STRETCH, "letterbox": RESIZE_LETTERBOX}
EVAL_FP, EVAL_TP, EVAL_IGNORED = 0, 1, 2        # enum yolo_eval_verdict
EVAL_OVERFLOW, EVAL_UNSORTED, EVAL_BAD_CLASS, EVAL_BAD_COUNT = 1, 2, 4, 8       # enum yolo_eval_status
EVAL_MAX_GT, EVAL_MAX_DET_CAPACITY, EVAL_MAX_CLASSES = 1024, 1 << 20, 65536
LOSS_OUT_OF_GRID, LOSS_BAD_BOX, LOSS_BAD_CLASS, LOSS_BAD_COUNT = 1, 2, 4, 8     # enum yolo_loss_status
LOSS_MAX_CELLS = 4096
ANCHOR_EUCLIDEAN, ANCHOR_IOU = 0, 1               # enum yolo_anchor_distance
ANCHOR_DISTANCES = {"euclidean": ANCHOR_EUCLIDEAN, "iou": ANCHOR_IOU}
ANCHOR_BAD_BOX, ANCHOR_EMPTY_CLUSTER, ANCHOR_DEGENERATE, ANCHOR_MAX_ITER = 1, 2, 4, 8        # enum yolo_anchor_status
ANCHOR_MAX_K, ANCHOR_MAX_INIT, ANCHOR_MAX_N, ANCHOR_ITER_LIMIT = 32, 64, 1 << 22, 10000
FRAMES_PER_LAUNCH = 64                          # frames one launch of the batched resize covers (larger batches: consecutive launches)
MAX_SRC, MAX_ANCHORS, MAX_SCALES = 4, 8, 4
# Records per image every Python entry point asks for unless told otherwise.  The reference's lists are unbounded
# (net/base.py:195-209); 1024 covers every YOLOv2 head (845 rows) and exceeding it raises (engine.check_status).
DEFAULT_MAX_BOXES = 1024


class LayerDesc(C.Structure):
    _fields_ = [("op", C.c_int32), ("n_src", C.c_int32), ("src", C.c_int32 * MAX_SRC),
                ("filters", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32),
                ("batch_norm", C.c_int32), ("leaky", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32),
                ("n_anchors", C.c_int32), ("anchors", C.c_double * (2 * MAX_ANCHORS))]


class NetOptions(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("max_batch", C.c_int32), ("keep_all", C.c_int32),
                ("cand_capacity", C.c_int32), ("max_boxes", C.c_int32), ("streams", C.c_int32), ("force_tile", C.c_int32), ("guard_bytes", C.c_int32), ("f32_products", C.c_int32)]


class Box(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float),
                ("prob", C.c_float), ("class_idx", C.c_int32)]


class HeadDesc(C.Structure):
    _fields_ = [("version", C.c_int32), ("n_classes", C.c_int32), ("n_scales", C.c_int32),
                ("h", C.c_int32 * MAX_SCALES), ("w", C.c_int32 * MAX_SCALES), ("n_anchors", C.c_int32 * MAX_SCALES),
                ("anchors", (C.c_double * (2 * MAX_ANCHORS)) * MAX_SCALES)]


class Frame(C.Structure):
    """yolo_frame: one decoded uint8 HWC3 frame on the device"""
    _fields_ = [("pixels_dev", C.c_void_p), ("h", C.c_int32), ("w", C.c_int32), ("row_bytes", C.c_int32), ("swap_rb", C.c_int32)]


class Gt(C.Structure):
    """yolo_gt: one ground-truth box (centre / size normalised like Box)"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float), ("class_idx", C.c_int32), ("difficult", C.c_int32)]


class EvalDesc(C.Structure):
    _fields_ = [("n_classes", C.c_int32), ("det_capacity", C.c_int32), ("max_gt", C.c_int32), ("pad_", C.c_int32), ("match_iou", C.c_double)]


class EvalRecord(C.Structure):
    _fields_ = [("best_iou", C.c_double), ("prob", C.c_float), ("class_idx", C.c_int32), ("seq", C.c_uint32), ("verdict", C.c_int32),
                ("best_gt", C.c_int32), ("pad_", C.c_int32)]


class EvalClass(C.Structure):
    _fields_ = [("ap_voc12", C.c_double), ("ap_voc07", C.c_double), ("n_gt", C.c_int32), ("n_det", C.c_int32), ("tp", C.c_int32),
                ("fp", C.c_int32), ("ignored", C.c_int32), ("pad_", C.c_int32)]


class EvalResultHeader(C.Structure):
    """yolo_eval_result: the head of the result block, EvalClass[n_classes] follows"""
    _fields_ = [("map_voc12", C.c_double), ("map_voc07", C.c_double), ("n_records", C.c_int32), ("status", C.c_int32),
                ("n_classes", C.c_int32), ("pad_", C.c_int32)]


class EvalLayout(C.Structure):
    _fields_ = [("status_offset", C.c_uint64), ("n_gt_offset", C.c_uint64), ("records_offset", C.c_uint64), ("sorted_offset", C.c_uint64),
                ("ctp_offset", C.c_uint64), ("cfp_offset", C.c_uint64), ("total_bytes", C.c_uint64)]


class LossImage(C.Structure):
    """yolo_loss_image: one image's float64 sums of the loss terms, before weights and 1 / B"""
    _fields_ = [("xy", C.c_double), ("wh", C.c_double), ("obj", C.c_double), ("noobj", C.c_double), ("cls", C.c_double),
                ("n_assigned", C.c_int32), ("n_truths", C.c_int32), ("status", C.c_int32), ("pad_", C.c_int32)]


class LossResult(C.Structure):
    _fields_ = [("loss", C.c_double), ("loss_xy", C.c_double), ("loss_wh", C.c_double), ("loss_obj", C.c_double), ("loss_noobj", C.c_double),
                ("loss_class", C.c_double), ("n_assigned", C.c_int32), ("n_truths", C.c_int32), ("status", C.c_int32), ("pad_", C.c_int32)]


class LaunchCaps(C.Structure):
    """yolo_launch_caps: how much work one round of the looping kernels holds"""
    _fields_ = [("tap_stream_workgroups", C.c_int32), ("stem_workgroups", C.c_int32), ("first_mfma_workgroups", C.c_int32),
                ("aux_work_items", C.c_int32), ("decode_rows", C.c_int32)]


class WgradPlan(C.Structure):
    """yolo_wgrad_plan: how a weight-gradient call is split (tiles of dW, chunks of positions, scratch)"""
    _fields_ = [("tile_cout", C.c_int32), ("tile_cin", C.c_int32), ("tile_positions", C.c_int32), ("tiles_cout", C.c_int32),
                ("tiles_cin", C.c_int32), ("positions_per_chunk", C.c_int32), ("n_chunks", C.c_int32), ("pad_", C.c_int32),
                ("scratch_bytes", C.c_uint64)]


class Conv3x3WgradPlan(C.Structure):
    """yolo_conv3x3_wgrad_plan: how a 3 x 3 weight-gradient call is split (tiles of dW3, chunks of positions, the halo in LDS, scratch)"""
    _fields_ = [("tile_cout", C.c_int32), ("tile_cin", C.c_int32), ("tile_positions", C.c_int32), ("tiles_cout", C.c_int32),
                ("tiles_cin", C.c_int32), ("positions_per_chunk", C.c_int32), ("n_chunks", C.c_int32), ("halo_rows", C.c_int32),
                ("scratch_bytes", C.c_uint64)]


class Conv3x3WgradF16Plan(C.Structure):
    """yolo_conv3x3_wgrad_f16_plan: the split of a 3 x 3 weight-gradient call on the fp16 matrix cores, and where the m / k record lies"""
    _fields_ = [("tile_cout", C.c_int32), ("tile_cin", C.c_int32), ("tile_positions", C.c_int32), ("tiles_cout", C.c_int32),
                ("tiles_cin", C.c_int32), ("positions_per_chunk", C.c_int32), ("n_chunks", C.c_int32), ("halo_rows", C.c_int32),
                ("db_groups", C.c_int32), ("db_positions", C.c_int32), ("record_offset", C.c_uint64), ("scratch_bytes", C.c_uint64)]


class TensorView(C.Structure):
    """yolo_tensor_view: a strided NHWC tensor inside the bound workspace"""
    _fields_ = [("offset", C.c_uint64), ("image_stride", C.c_int64), ("ld", C.c_int32), ("coff", C.c_int32), ("dtype", C.c_int32),
                ("cin", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


class HeadTrainLayout(C.Structure):
    """yolo_head_train_layout: byte offsets of the parts of the head-training state"""
    _fields_ = [(n, C.c_uint64) for n in ("w_offset", "b_offset", "m_w_offset", "v_w_offset", "m_b_offset", "v_b_offset", "dw_offset",
                                          "db_offset", "grad_offset", "assign_offset", "images_offset", "scratch_offset", "scratch_bytes",
                                          "total_bytes")] + [("cin", C.c_int32), ("cout", C.c_int32)]


class TailTrainLayout(C.Structure):
    """yolo_tail_train_layout: byte offsets of the parts of the tail-training state (the head's parts, then the 3 x 3 block's)"""
    _fields_ = [(n, C.c_uint64) for n in ("w_offset", "b_offset", "m_w_offset", "v_w_offset", "m_b_offset", "v_b_offset", "dw_offset",
                                          "db_offset", "w3_offset", "beta_offset", "m_w3_offset", "v_w3_offset", "m_beta_offset",
                                          "v_beta_offset", "dw3_offset", "dbeta_offset", "scale64_offset", "scale32_offset", "mean_offset",
                                          "d_offset", "grad_offset", "assign_offset", "images_offset", "scratch_offset", "scratch_bytes",
                                          "total_bytes", "block_src", "head_src")] + [(n, C.c_int32) for n in ("cin", "cout", "cin3", "cout3")]


class HeadTrainV3Layout(C.Structure):
    """yolo_head_train_v3_layout: byte offsets of the parts of the YOLOv3 head-training state, per scale where the part is per conv"""
    _fields_ = ([("n_scales", C.c_int32), ("pad_", C.c_int32), ("cin", C.c_int32 * MAX_SCALES), ("cout", C.c_int32 * MAX_SCALES)] +
                [(n, C.c_uint64 * MAX_SCALES) for n in ("w_offset", "b_offset", "m_w_offset", "v_w_offset", "m_b_offset", "v_b_offset",
                                                        "dw_offset", "db_offset", "bias_src")] +
                [(n, C.c_uint64) for n in ("grad_offset", "assign_offset", "parts_offset", "images_offset", "scratch_offset",
                                           "scratch_bytes", "total_bytes")])


class BlocksTrainV3Layout(C.Structure):
    """yolo_blocks_train_v3_layout: byte offsets of the parts of the state that trains the YOLOv3 head convs and the 3 x 3 blocks behind them"""
    _fields_ = ([("n_scales", C.c_int32), ("pad_", C.c_int32)] + [(n, C.c_int32 * MAX_SCALES) for n in ("cin", "cout", "cin3", "cout3")] +
                [(n, C.c_uint64 * MAX_SCALES) for n in ("w_offset", "b_offset", "m_w_offset", "v_w_offset", "m_b_offset", "v_b_offset",
                                                        "dw_offset", "db_offset", "w3_offset", "beta_offset", "m_w3_offset", "v_w3_offset",
                                                        "m_beta_offset", "v_beta_offset", "dw3_offset", "dbeta_offset", "scale64_offset",
                                                        "scale32_offset", "mean_offset", "bias_src", "block_src")] +
                [(n, C.c_uint64) for n in ("d_offset", "grad_offset", "assign_offset", "parts_offset", "images_offset", "scratch_offset",
                                           "scratch_bytes", "total_bytes")])


class V3WgradPlan(C.Structure):
    """yolo_v3_wgrad_plan: how the weight gradient of the YOLOv3 head convs is split (per scale: chunks of positions, slabs; slot; scratch)"""
    _fields_ = ([(n, C.c_int32) for n in ("n_scales", "threads", "channels_per_thread", "min_chunk", "win_tile_cin", "win_tile_rows", "reduce_tile_chunks", "pad_")] +
                [(n, C.c_int32 * MAX_SCALES) for n in ("positions", "positions_per_chunk", "n_chunks", "threads_per_chunk", "obj_workgroups",
                                                       "win_workgroups")] +
                [(n, C.c_uint64 * MAX_SCALES) for n in ("slab_offset", "slab_bytes")] +
                [(n, C.c_uint64) for n in ("slot_offset", "slot_bytes", "scratch_bytes")])


class V3WgradView(C.Structure):
    """yolo_v3_wgrad_view: the input of one head conv, a strided NHWC view behind a device pointer"""
    _fields_ = [("x_dev", C.c_void_p), ("image_stride", C.c_int64), ("ld", C.c_int32), ("coff", C.c_int32), ("dtype", C.c_int32),
                ("cin", C.c_int32)]


class V3DgradPlan(C.Structure):
    """yolo_v3_dgrad_plan: how the sparse data gradient of one YOLOv3 head conv is split (channel tiles, positions per round and workgroup)"""
    _fields_ = [(n, C.c_int32) for n in ("threads", "channels_per_thread", "tile_cin", "tiles_cin", "threads_per_position",
                                         "positions_per_round", "rounds", "positions_per_workgroup", "workgroups", "loops", "positions",
                                         "lds_bytes")]


class AugmentImage(C.Structure):
    """yolo_augment_image: how one image of a training batch is augmented (net/augment.py draws it)"""
    _fields_ = [("enabled", C.c_int32), ("flip_lr", C.c_int32), ("flip_ud", C.c_int32), ("radius", C.c_int32), ("taps", C.c_uint16 * 10),
                ("drop_thr", C.c_uint32), ("noise_q", C.c_int32 * 2), ("noise_loc", C.c_int32 * 2), ("tx", C.c_int32), ("key", C.c_uint32 * 2)]


class AnchorDesc(C.Structure):
    """yolo_anchor_desc: one anchor k-means problem"""
    _fields_ = [("k", C.c_int32), ("n_init", C.c_int32), ("max_iter", C.c_int32), ("distance", C.c_int32), ("tolerate", C.c_double),
                ("seed", C.c_uint64)]


class AnchorPlan(C.Structure):
    """struct yolo_anchor_plan: the split of an anchor k-means call and the layout of its scratch and result"""
    _fields_ = [(n, C.c_int32) for n in ("chunk", "n_chunks", "period", "threads")] + \
               [(n, C.c_uint64) for n in ("prep_offset", "pick_offset", "state_offset", "q_offset", "label_offset", "label_stride",
                                          "sums_offset", "scratch_bytes", "header_offset", "restarts_offset", "best_offset", "result_bytes")]


class AnchorHeader(C.Structure):
    _fields_ = [("status", C.c_uint32)] + [(n, C.c_int32) for n in ("best_restart", "n_valid", "n_bad", "k", "n_init", "distance", "pad_")]


class AnchorRestart(C.Structure):
    _fields_ = [("n_iter", C.c_int32), ("status", C.c_uint32), ("inertia_q", C.c_uint64), ("iou_q", C.c_uint64),
                ("seeds", C.c_int32 * ANCHOR_MAX_K)]


class AnchorBest(C.Structure):
    _fields_ = [("centres", (C.c_double * 2) * ANCHOR_MAX_K), ("counts", C.c_int64 * ANCHOR_MAX_K), ("sum_q", (C.c_uint64 * 2) * ANCHOR_MAX_K),
                ("inertia_q", C.c_uint64), ("iou_q", C.c_uint64), ("inertia", C.c_double), ("avg_iou", C.c_double)]


class WsRegion(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("offset", C.c_uint64), ("used_bytes", C.c_uint64), ("region_bytes", C.c_uint64)]


class KernelInfo(C.Structure):
    _fields_ = [("kind", C.c_int32), ("layer", C.c_int32), ("variant", C.c_int32), ("ksize", C.c_int32),
                ("stride", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("flops", C.c_double), ("bytes", C.c_double), ("weight_bytes", C.c_double), ("name", C.c_char * 64),
                ("symbol", C.c_char * 160)]


# name -> (restype, argtypes); every symbol include/yolo_hip.h declares
SIGNATURES = {
    "yolo_hip_abi_version": (C.c_int, []),
    "yolo_last_error": (C.c_char_p, []),
    "yolo_net_create": (C.c_int, [C.POINTER(LayerDesc), C.c_int, C.POINTER(NetOptions), C.POINTER(C.c_void_p)]),
    "yolo_net_destroy": (None, [C.c_void_p]),
    "yolo_net_weight_count": (C.c_size_t, [C.c_void_p]),
    "yolo_net_weights_bytes": (C.c_size_t, [C.c_void_p]),
    "yolo_net_workspace_bytes": (C.c_size_t, [C.c_void_p]),
    "yolo_net_output_count": (C.c_size_t, [C.c_void_p]),
    "yolo_net_flops_per_image": (C.c_double, [C.c_void_p]),
    "yolo_net_head_desc": (C.c_int, [C.c_void_p, C.POINTER(HeadDesc)]),
    "yolo_net_set_head": (C.c_int, [C.c_void_p, C.POINTER(HeadDesc)]),
    "yolo_net_num_kernels": (C.c_int, [C.c_void_p]),
    "yolo_net_num_streams": (C.c_int, [C.c_void_p]),
    "yolo_net_describe": (C.c_size_t, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "yolo_net_load_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "yolo_net_bind_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "yolo_net_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_net_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # uint8 network input (ABI 7): the float32 entries' signatures, the input pointer holds bytes
    "yolo_net_forward_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_net_detect_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_net_forward_timed_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_net_tune_streams_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_preprocess_resize_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_u8_unit_table": (C.c_int, [C.c_void_p]),
    "yolo_launch_caps": (C.c_int, [C.POINTER(LaunchCaps)]),
    "yolo_net_autotune": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_net_tune_streams": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "yolo_net_set_streams": (C.c_int, [C.c_void_p, C.c_int]),
    "yolo_net_workspace_regions": (C.c_int, [C.c_void_p, C.POINTER(WsRegion), C.c_int]),
    "yolo_net_kernel_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(KernelInfo)]),
    "yolo_net_forward_timed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_net_read_layer": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "yolo_mx_quantize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_mx_quantize_host": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "yolo_decode_scratch_bytes": (C.c_size_t, [C.POINTER(HeadDesc), C.c_int, C.c_int]),
    "yolo_decode_nms": (C.c_int, [C.POINTER(HeadDesc), C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int,
                                  C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "yolo_preprocess_resize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    # frames of any size (added within ABI 7): batched resize / letterbox, boxes back in frame coordinates, the whole step
    "yolo_letterbox_geometry": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "yolo_preprocess_frames_u8": (C.c_int, [C.POINTER(Frame), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yolo_preprocess_frames": (C.c_int, [C.POINTER(Frame), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yolo_boxes_to_frames": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(Frame), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "yolo_net_detect_frames_u8": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # VOC-style evaluation on the device (added within ABI 7)
    "yolo_eval_state_bytes": (C.c_size_t, [C.POINTER(EvalDesc)]),
    "yolo_eval_result_bytes": (C.c_size_t, [C.POINTER(EvalDesc)]),
    "yolo_eval_state_layout": (C.c_int, [C.POINTER(EvalDesc), C.POINTER(EvalLayout)]),
    "yolo_eval_reset": (C.c_int, [C.POINTER(EvalDesc), C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_eval_add": (C.c_int, [C.POINTER(EvalDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_int64, C.c_void_p]),
    "yolo_eval_finish": (C.c_int, [C.POINTER(EvalDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    # YOLOv2 loss, forward only (added within ABI 7)
    "yolo_v2_loss": (C.c_int, [C.POINTER(HeadDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "yolo_net_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "yolo_net_loss_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "yolo_loss_reduce": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # the gradient of the YOLOv2 loss with respect to the logits (added within ABI 7)
    "yolo_v2_loss_grad": (C.c_int, [C.POINTER(HeadDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    # the YOLOv3 loss and its gradient with respect to the logits (added within ABI 7)
    "yolo_v3_loss_rows": (C.c_int, [C.POINTER(HeadDesc), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "yolo_v3_loss": (C.c_int, [C.POINTER(HeadDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_v3_loss_grad": (C.c_int, [C.POINTER(HeadDesc), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_net_loss_v3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_net_loss_v3_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    # training the detection layer (added within ABI 7)
    "yolo_wgrad_plan": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(WgradPlan)]),
    "yolo_conv1x1_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_adam_step": (C.c_int, [C.c_void_p] * 8 + [C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "yolo_net_head_input": (C.c_int, [C.c_void_p, C.POINTER(TensorView)]),
    "yolo_net_head_train_layout": (C.c_int, [C.c_void_p, C.POINTER(HeadTrainLayout)]),
    "yolo_net_head_train_bytes": (C.c_size_t, [C.c_void_p]),
    "yolo_net_head_train_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "yolo_net_head_train_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_net_train_head_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                           C.c_void_p, C.c_void_p]),
    "yolo_net_train_head_step_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                              C.c_void_p, C.c_void_p]),
    # the weight gradient of the YOLOv3 head convs (added within ABI 7)
    "yolo_v3_head_wgrad_plan": (C.c_int, [C.POINTER(HeadDesc), C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(V3WgradPlan)]),
    "yolo_v3_head_wgrad": (C.c_int, [C.POINTER(HeadDesc), C.POINTER(V3WgradView), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]),
    # training the YOLOv3 head convs on a net (added within ABI 7)
    "yolo_net_head_inputs_v3": (C.c_int, [C.c_void_p, C.POINTER(TensorView), C.POINTER(C.c_int32)]),
    "yolo_net_head_train_v3_layout": (C.c_int, [C.c_void_p, C.POINTER(HeadTrainV3Layout)]),
    "yolo_net_head_train_v3_bytes": (C.c_size_t, [C.c_void_p]),
    "yolo_net_head_train_v3_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "yolo_net_head_train_v3_read": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "yolo_net_train_head_step_v3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                              C.c_float, C.c_void_p, C.c_void_p]),
    "yolo_net_train_head_step_v3_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                                 C.c_float, C.c_void_p, C.c_void_p]),
    # the data gradient of the detection layer and the weight gradient of a 3 x 3 conv (added within ABI 7)
    "yolo_conv1x1_dgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int,
                                     C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "yolo_conv3x3_wgrad_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Conv3x3WgradPlan)]),
    "yolo_conv3x3_wgrad": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # the 3 x 3 weight gradient on the fp16 matrix cores and its mode on a net (added within ABI 7)
    "yolo_conv3x3_wgrad_f16_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Conv3x3WgradF16Plan)]),
    "yolo_conv3x3_wgrad_f16": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "yolo_net_train_wgrad_f16_bytes": (C.c_size_t, [C.c_void_p]),
    "yolo_net_train_set_wgrad_f16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    # training the tail of a YOLOv2 net (added within ABI 7)
    "yolo_net_tail_inputs": (C.c_int, [C.c_void_p, C.POINTER(TensorView), C.POINTER(TensorView)]),
    "yolo_net_tail_train_layout": (C.c_int, [C.c_void_p, C.POINTER(TailTrainLayout)]),
    "yolo_net_tail_train_bytes": (C.c_size_t, [C.c_void_p]),
    "yolo_net_tail_train_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_net_tail_train_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "yolo_net_train_tail_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                           C.c_void_p, C.c_void_p]),
    "yolo_net_train_tail_step_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                              C.c_void_p, C.c_void_p]),
    # the sparse data gradient of one YOLOv3 head conv (added within ABI 7)
    "yolo_v3_head_dgrad_plan": (C.c_int, [C.POINTER(HeadDesc), C.c_int, C.c_int, C.c_int, C.POINTER(V3DgradPlan)]),
    "yolo_v3_head_dgrad": (C.c_int, [C.POINTER(HeadDesc), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_int, C.c_int, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    # training the 3 x 3 blocks behind the YOLOv3 heads (added within ABI 7)
    "yolo_net_block_inputs_v3": (C.c_int, [C.c_void_p, C.POINTER(TensorView), C.POINTER(TensorView), C.POINTER(C.c_int32)]),
    "yolo_net_blocks_train_v3_layout": (C.c_int, [C.c_void_p, C.POINTER(BlocksTrainV3Layout)]),
    "yolo_net_blocks_train_v3_bytes": (C.c_size_t, [C.c_void_p]),
    "yolo_net_blocks_train_v3_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_void_p)]),
    "yolo_net_blocks_train_v3_read": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_void_p)]),
    "yolo_net_train_blocks_step_v3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                                C.c_float, C.c_void_p, C.c_void_p]),
    "yolo_net_train_blocks_step_v3_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                                   C.c_float, C.c_void_p, C.c_void_p]),
    # training augmentation (added within ABI 7)
    "yolo_augment_check": (C.c_int, [C.POINTER(AugmentImage), C.c_int, C.c_int]),
    "yolo_augment_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(AugmentImage), C.c_void_p]),
    "yolo_augment_truths_host": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(AugmentImage), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32)]),
    "yolo_augment_tile": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    # anchor k-means (added within ABI 7)
    "yolo_anchor_plan": (C.c_int, [C.POINTER(AnchorDesc), C.c_int64, C.POINTER(AnchorPlan)]),
    "yolo_anchor_kmeans": (C.c_int, [C.POINTER(AnchorDesc), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_void_p]),
    "yolo_nms_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int,
                                C.c_void_p, C.POINTER(C.c_int32)]),
}

_lib = None


class YoloHipError(RuntimeError):
    """A libyolo_hip call returned a non-zero status (message from yolo_last_error)."""


def lib():
    """Load (once) and return the shared library with typed entry points."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libyolo_hip.so not found at %s: the HIP extension is the only compute path of this package "
            "(no CPU fallback). Build it with `python __graft_entry__.py` or `make -C tensorflow-yolo_amd/csrc`."
            % LIB_PATH)
    # torch first: libyolo_hip.so links the system libamdhip64 while torch-ROCm carries its own copy; whichever is loaded first
    # serves both, and a process that loaded the system copy before torch ends up with two HIP runtimes of which ours sees no
    # device ("no ROCm-capable device is detected" from hipMemcpy).  torch is this package's device-memory plumbing anyway.
    import torch  # noqa: F401
    handle = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(handle, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    v = handle.yolo_hip_abi_version()
    if v != ABI_VERSION:
        raise ImportError("libyolo_hip.so ABI version %d, binding expects %d: rebuild the library" % (v, ABI_VERSION))
    _lib = handle
    return _lib


def resize_mode(name):
    """'stretch' | 'letterbox' (the .ini key `resize`, the `resize` argument of predict_frames) -> enum yolo_resize_mode; else ValueError"""
    key = str(name).strip().lower()
    if key not in RESIZE_MODES:
        raise ValueError("resize must be stretch or letterbox, got %r" % (name,))
    return RESIZE_MODES[key]


def letterbox_geometry(src_h, src_w, dst_h, dst_w, mode):
    """(new_h, new_w, off_y, off_x) of a src_h x src_w frame in a dst_h x dst_w network input (yolo_letterbox_geometry: host only)"""
    out = [C.c_int32() for _ in range(4)]
    check(lib().yolo_letterbox_geometry(int(src_h), int(src_w), int(dst_h), int(dst_w), int(mode), *[C.byref(v) for v in out]),
          "yolo_letterbox_geometry")
    return tuple(int(v.value) for v in out)


def launch_caps():
    """yolo_launch_caps as a dict (host only)"""
    caps = LaunchCaps()
    check(lib().yolo_launch_caps(C.byref(caps)), "yolo_launch_caps")
    return {name: int(getattr(caps, name)) for name, _ in LaunchCaps._fields_}


def wgrad_plan(P, cin, cout, x_dtype=DTYPE_F16):
    """yolo_wgrad_plan as a dict (host only)"""
    pl = WgradPlan()
    check(lib().yolo_wgrad_plan(int(P), int(cin), int(cout), int(x_dtype), C.byref(pl)), "yolo_wgrad_plan")
    return {name: int(getattr(pl, name)) for name, _ in WgradPlan._fields_ if name != "pad_"}


def conv3x3_wgrad_plan(h, w, batch, cin, cout, x_dtype=DTYPE_F16):
    """yolo_conv3x3_wgrad_plan as a dict (host only)"""
    pl = Conv3x3WgradPlan()
    check(lib().yolo_conv3x3_wgrad_plan(int(h), int(w), int(batch), int(cin), int(cout), int(x_dtype), C.byref(pl)), "yolo_conv3x3_wgrad_plan")
    return {name: int(getattr(pl, name)) for name, _ in Conv3x3WgradPlan._fields_}


def conv3x3_wgrad_f16_plan(h, w, batch, cin, cout):
    """yolo_conv3x3_wgrad_f16_plan as a dict (host only)"""
    pl = Conv3x3WgradF16Plan()
    check(lib().yolo_conv3x3_wgrad_f16_plan(int(h), int(w), int(batch), int(cin), int(cout), C.byref(pl)), "yolo_conv3x3_wgrad_f16_plan")
    return {name: int(getattr(pl, name)) for name, _ in Conv3x3WgradF16Plan._fields_}


def v3_head_wgrad_plan(head, cins, batch, x_dtype=DTYPE_F16):
    """yolo_v3_head_wgrad_plan as a dict (host only): scalars as ints, per-scale fields as lists of n_scales ints"""
    pl = V3WgradPlan()
    arr = (C.c_int32 * MAX_SCALES)(*[int(c) for c in cins])
    check(lib().yolo_v3_head_wgrad_plan(C.byref(head), arr, int(batch), int(x_dtype), C.byref(pl)), "yolo_v3_head_wgrad_plan")
    out = {}
    for name, kind in V3WgradPlan._fields_:
        if name == "pad_":
            continue
        v = getattr(pl, name)
        out[name] = int(v) if kind in (C.c_int32, C.c_uint64) else [int(x) for x in v[:pl.n_scales]]
    return out


def head_dgrad_plan(head, scale, cin, batch):
    """yolo_v3_head_dgrad_plan as a dict (host only)"""
    pl = V3DgradPlan()
    check(lib().yolo_v3_head_dgrad_plan(C.byref(head), int(scale), int(cin), int(batch), C.byref(pl)), "yolo_v3_head_dgrad_plan")
    return {name: int(getattr(pl, name)) for name, _ in V3DgradPlan._fields_}


def augment_tile():
    """yolo_augment_tile: (rows, cols, images_per_launch) of the augmentation kernel (host only)"""
    out = [C.c_int32() for _ in range(3)]
    check(lib().yolo_augment_tile(*[C.byref(v) for v in out]), "yolo_augment_tile")
    return tuple(int(v.value) for v in out)


def anchor_distance(name):
    """'euclidean' | 'iou' (the .ini key `distance`, the `distance` argument of kmeans_anchors) -> enum yolo_anchor_distance; else ValueError"""
    key = str(name).strip().lower()
    if key not in ANCHOR_DISTANCES:
        raise ValueError("distance must be euclidean or iou, got %r" % (name,))
    return ANCHOR_DISTANCES[key]


def anchor_desc(k, n_init=10, max_iter=300, distance=ANCHOR_EUCLIDEAN, tolerate=0.005, seed=0):
    return AnchorDesc(int(k), int(n_init), int(max_iter), int(distance), float(tolerate), int(seed) & 0xFFFFFFFFFFFFFFFF)


def anchor_plan(desc, n):
    """yolo_anchor_plan as a dict (host only)"""
    pl = AnchorPlan()
    check(lib().yolo_anchor_plan(C.byref(desc), int(n), C.byref(pl)), "yolo_anchor_plan")
    return {name: int(getattr(pl, name)) for name, _ in AnchorPlan._fields_}


def check(rc, what=""):
    if rc != 0:
        msg = lib().yolo_last_error()
        raise YoloHipError("%s failed (status %d): %s" % (what or "libyolo_hip call", rc, (msg or b"").decode()))

/*
 * yolo_hip.h -- C ABI of libyolo_hip.so: MI355X (gfx950) native YOLO v2/v3 TEST-mode hot path.
 *
 * Plain C: pointers, sizes and PODs only.  No torch / C++ types cross this boundary.
 * All device pointers are ordinary HIP device pointers (the Python host passes
 * torch-ROCm tensor .data_ptr() values); `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Every entry returns 0 on success or a YOLO_ERR_* code;
 * yolo_last_error() gives the message.  A yolo_net is used by one host thread at a time.
 * Unless stated otherwise work is ENQUEUED on `stream` and the caller synchronises.
 *
 * What each entry replaces in the reference (wns349/tensorflow-yolo):
 *   yolo_net_create         net/v2.py:11-60 create_full_network, net/v3.py:9-94 create_network
 *                           (the TF graph build: here a layer list -> fused kernel plan)
 *   yolo_net_load_weights   net/base.py:26-46 load_weights + net/v2.py:63-79 / net/v3.py:98-106
 *   yolo_net_forward        net/yolo.py:83  sess.run(net[-1].out, {net[0].out: x_batch})
 *   yolo_decode_nms         net/v2.py:83-119 / net/v3.py:140-151 find_bounding_boxes
 *                           (+ net/base.py:195-209 non_maximum_suppression)
 *   yolo_net_detect         net/yolo.py:83-86 (forward + find_bounding_boxes in one enqueue)
 *   yolo_nms_host           net/base.py:195-209 non_maximum_suppression on a host box list
 *   yolo_preprocess_resize  net/base.py:115-155 preprocess_image (resize + colour order + /255) on the device
 *   yolo_net_forward_u8, yolo_net_detect_u8, yolo_net_forward_timed_u8, yolo_net_tune_streams_u8, yolo_preprocess_resize_u8
 *                           (ABI 7) the same call sites for a caller that holds the 8-bit pixels net/base.py:115-155 starts from:
 *                           the / 255. of net/base.py:153 happens inside the first kernel instead of in a float32 tensor
 *   yolo_preprocess_frames, yolo_preprocess_frames_u8
 *                           net/base.py:158-168 generate_test_batch's loop over net/base.py:115-155 preprocess_image: every frame of a batch,
 *                           whatever its size, in one launch (stretch as there, or Darknet's letterbox, which the reference does not have)
 *   yolo_net_detect_frames_u8
 *                           net/yolo.py:80-86: that loop, the forward pass and find_bounding_boxes in one enqueue
 *   yolo_letterbox_geometry, yolo_boxes_to_frames
 *                           no reference call site: net/base.py:121 only stretches, so its boxes are normalised to the frame as they are
 *                           (net/base.py:212-226 draw_boxes scales them by the frame size)
 *   yolo_eval_reset, yolo_eval_add, yolo_eval_finish (+ yolo_eval_state_bytes, yolo_eval_result_bytes, yolo_eval_state_layout)
 *                           no reference call site: the reference parses annotations (net/base.py:69-97) but never scores a detector;
 *                           VOC average precision with the IoU of net/base.py:180-192
 *   yolo_v2_loss            net/v2.py:123-198 create_loss_fn (the loss graph, forward only) over net/v2.py:242-295 _make_ground_truths
 *   yolo_net_loss, yolo_net_loss_u8
 *                           net/yolo.py:177-193: sess.run(loss, ...) of one validation batch, forward pass included
 *   yolo_loss_reduce        net/yolo.py:185-187: the sums behind `val_total / val_count`, over the per-image records of a whole set
 *   yolo_v2_loss_grad       tf.gradients of net/v2.py:188 with respect to net[-1].out, as AdamOptimizer.minimize (net/v2.py:205) takes it
 *   yolo_conv1x1_wgrad      tf.gradients of net/v2.py:188 with respect to the last conv's kernel and bias (net/v2.py:52-56), from that gradient
 *   yolo_adam_step          the update of tf.train.AdamOptimizer(lr).minimize(loss), net/v2.py:205, on those two variables
 *   yolo_net_train_head_step, yolo_net_train_head_step_u8
 *                           net/yolo.py:161-173: sess.run([optimizer, loss, ...]) of one training batch, for the detection layer alone
 *                           (+ yolo_wgrad_plan, yolo_net_head_input, yolo_net_head_train_bytes / _layout / _init / _read: no reference call site)
 *   yolo_v3_loss, yolo_v3_loss_grad, yolo_net_loss_v3, yolo_net_loss_v3_u8 (+ yolo_v3_loss_rows)
 *                           no reference call site: the reference binds no loss to YoloV3 (net/yolo.py:208-211); the loss of Darknet's
 *                           [yolo] layer and its gradient with respect to the logits
 *   yolo_v3_head_wgrad      no reference call site either: the gradient of that loss with respect to the kernels and biases of the convs in
 *                           front of the [yolo] layers, from that gradient (+ yolo_v3_head_wgrad_plan)
 *   yolo_net_train_head_step_v3, yolo_net_train_head_step_v3_u8
 *                           net/yolo.py:161-173 for the head convs of a YOLOv3 network (+ yolo_net_head_inputs_v3,
 *                           yolo_net_head_train_v3_bytes / _layout / _init / _read: no reference call site)
 *   yolo_conv1x1_dgrad, yolo_conv3x3_wgrad (+ yolo_conv3x3_wgrad_plan)
 *                           tf.gradients of net/v2.py:188 with respect to the detection layer's input (through the leaky ReLU in front of
 *                           it) and, from that, to the kernel and beta of the 3 x 3 conv of net/v2.py:62: standalone operators
 *   yolo_v3_head_dgrad      no reference call site: the gradient of the YOLOv3 loss with respect to the input of one head conv, through the
 *                           leaky ReLU in front of it, from the sparse gradient in place (+ yolo_v3_head_dgrad_plan)
 *   yolo_net_train_blocks_step_v3, yolo_net_train_blocks_step_v3_u8
 *                           net/yolo.py:161-173 for the head convs of a YOLOv3 network and the 3 x 3 blocks behind them
 *                           (+ yolo_net_block_inputs_v3, yolo_net_blocks_train_v3_bytes / _layout / _init / _read: no reference call site)
 *   yolo_conv3x3_wgrad_f16 (+ yolo_conv3x3_wgrad_f16_plan, yolo_net_train_wgrad_f16_bytes, yolo_net_train_set_wgrad_f16)
 *                           no reference call site: yolo_conv3x3_wgrad with D narrowed to fp16 by one power of two per call, on the fp16
 *                           matrix cores, and the mode that puts it into the tail and blocks steps
 *   yolo_augment_u8         net/base.py:15-23, :100-107: seq.to_deterministic().augment_images of a resized batch, on the device
 *   yolo_augment_truths_host
 *                           net/base.py:107-111: augment_bounding_boxes(...).remove_out_of_image().cut_out_of_image()
 *                           (+ yolo_augment_check, yolo_augment_tile: no reference call site)
 *   yolo_anchor_kmeans      net/v2.py:299-323, net/base.py:49-52: generate_anchors / run_kmeans (sklearn's KMeans), on the device
 *                           (+ yolo_anchor_plan: no reference call site)
 */
#ifndef YOLO_HIP_H
#define YOLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YOLO_HIP_ABI_VERSION 7      /* 2: yolo_kernel_info.symbol; 3: yolo_net_num_streams, streams = 0 is the library's rule; 4: yolo_net_tune_streams; 5: yolo_net_set_streams;
                                       6: YOLO_DTYPE_MXF8, yolo_mx_quantize, yolo_mx_quantize_host;
                                       7: uint8 network input -- yolo_net_forward_u8, yolo_net_detect_u8, yolo_net_forward_timed_u8,
                                          yolo_net_tune_streams_u8, yolo_preprocess_resize_u8, yolo_u8_unit_table;
                                          added WITHIN ABI 7 (new exports, struct yolo_frame and enum yolo_resize_mode only: no existing struct or
                                          entry changed) -- the frame entries yolo_letterbox_geometry, yolo_preprocess_frames,
                                          yolo_preprocess_frames_u8, yolo_boxes_to_frames, yolo_net_detect_frames_u8;
                                          added WITHIN ABI 7 in the same way (new exports and the yolo_gt / yolo_eval_* PODs and enums only) -- the evaluation
                                          entries yolo_eval_state_bytes, yolo_eval_result_bytes, yolo_eval_state_layout, yolo_eval_reset, yolo_eval_add,
                                          yolo_eval_finish;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_loss_* PODs and enum only) -- the YOLOv2 loss entries
                                          yolo_v2_loss, yolo_net_loss, yolo_net_loss_u8, yolo_loss_reduce;
                                          added WITHIN ABI 7 in the same way (one new export) -- the loss gradient yolo_v2_loss_grad;
                                          added WITHIN ABI 7 in the same way (one new export, one new POD) -- the test hook yolo_launch_caps;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_wgrad_plan, yolo_tensor_view and yolo_head_train_layout
                                          PODs only) -- training the detection layer: yolo_wgrad_plan, yolo_conv1x1_wgrad, yolo_adam_step,
                                          yolo_net_head_input, yolo_net_head_train_bytes, yolo_net_head_train_layout, yolo_net_head_train_init,
                                          yolo_net_head_train_read, yolo_net_train_head_step, yolo_net_train_head_step_u8;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_augment_image POD only) -- training augmentation:
                                          yolo_augment_u8, yolo_augment_check, yolo_augment_truths_host, yolo_augment_tile;
                                          added WITHIN ABI 7 in the same way (new exports only; the yolo_loss_* PODs are reused unchanged) -- the YOLOv3
                                          loss and its gradient: yolo_v3_loss_rows, yolo_v3_loss, yolo_v3_loss_grad, yolo_net_loss_v3,
                                          yolo_net_loss_v3_u8;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_v3_wgrad_plan and yolo_v3_wgrad_view PODs only) -- the
                                          weight gradient of the YOLOv3 head convs: yolo_v3_head_wgrad_plan, yolo_v3_head_wgrad;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_head_train_v3_layout POD only) -- training the YOLOv3 head
                                          convs: yolo_net_head_inputs_v3, yolo_net_head_train_v3_layout, yolo_net_head_train_v3_bytes,
                                          yolo_net_head_train_v3_init, yolo_net_head_train_v3_read, yolo_net_train_head_step_v3,
                                          yolo_net_train_head_step_v3_u8;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_conv3x3_wgrad_plan POD only) -- the two operators a
                                          backward pass behind the detection layer is built from: yolo_conv1x1_dgrad, yolo_conv3x3_wgrad_plan,
                                          yolo_conv3x3_wgrad;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_tail_train_layout POD only) -- training the last 3 x 3
                                          block and the detection layer of a YOLOv2 net: yolo_net_tail_inputs, yolo_net_tail_train_layout,
                                          yolo_net_tail_train_bytes, yolo_net_tail_train_init, yolo_net_tail_train_read, yolo_net_train_tail_step,
                                          yolo_net_train_tail_step_u8;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_v3_dgrad_plan POD only) -- the sparse data gradient of
                                          one YOLOv3 head conv: yolo_v3_head_dgrad_plan, yolo_v3_head_dgrad;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_blocks_train_v3_layout POD only) -- training the 3 x 3
                                          blocks behind the YOLOv3 heads: yolo_net_block_inputs_v3, yolo_net_blocks_train_v3_layout,
                                          yolo_net_blocks_train_v3_bytes, yolo_net_blocks_train_v3_init, yolo_net_blocks_train_v3_read,
                                          yolo_net_train_blocks_step_v3, yolo_net_train_blocks_step_v3_u8;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_conv3x3_wgrad_f16_plan POD only) -- the 3 x 3 weight
                                          gradient on the fp16 matrix cores and its mode on a net: yolo_conv3x3_wgrad_f16_plan, yolo_conv3x3_wgrad_f16,
                                          yolo_net_train_wgrad_f16_bytes, yolo_net_train_set_wgrad_f16;
                                          added WITHIN ABI 7 in the same way (new exports, the yolo_anchor_* PODs and enums only) -- anchor k-means on the
                                          device: yolo_anchor_plan, yolo_anchor_kmeans */

enum yolo_status {
    YOLO_OK = 0,
    YOLO_ERR_ARG = 1,       /* bad argument                                        */
    YOLO_ERR_PLAN = 2,      /* layer list cannot be planned (unsupported topology) */
    YOLO_ERR_HIP = 3,       /* a HIP runtime call failed                           */
    YOLO_ERR_WEIGHTS = 4,   /* weight stream length != what the layer list needs   */
    YOLO_ERR_STATE = 5,     /* call order (weights / workspace not bound)          */
    YOLO_ERR_OVERFLOW = 6   /* more candidates than the configured capacity        */
};

/* Layer vocabulary == the reference's net/layers.py classes. */
enum yolo_op {
    YOLO_OP_INPUT = 0,      /* layers.py:106-109 input_layer     (h, w, c)                       */
    YOLO_OP_CONV = 1,       /* layers.py:17-67   conv2d_bn_act   (filters,ksize,stride,bn,leaky) */
    YOLO_OP_MAXPOOL = 2,    /* layers.py:70-81   max_pool2d      (ksize 2, stride 1|2; or odd ksize 3..13, stride 1: SAME) */
    YOLO_OP_ROUTE = 3,      /* layers.py:84-87   route           (src[0..n_src))                 */
    YOLO_OP_REORG = 4,      /* layers.py:90-97   reorg           (stride)                        */
    YOLO_OP_SHORTCUT = 5,   /* layers.py:100-103 shortcut        (src[0] = prev, src[1] = skip)  */
    YOLO_OP_UPSAMPLE = 6,   /* layers.py:112-116 upsample        (stride)                        */
    YOLO_OP_YOLO = 7,       /* layers.py:126-134 yolo_layer      (anchors in grid units)         */
    YOLO_OP_DETECTION = 8   /* layers.py:119-123 detection_layer (src = yolo layers)             */
};

/* YOLO_DTYPE_MXF8 (ABI 6): the fp16 plan -- fp16 activations in memory, same kernels, fusions, arenas and streams -- except that every
 * 3x3 / stride-1 conv with Cin % 128 == 0 and a map at most 100 wide (not pool-fused, not a head conv) multiplies on the block-scaled
 * fp8 matrix cores: OCP MXFP8, e4m3fn elements with one E8M0 scale per 32 input channels (weights quantized once at load, activations
 * inside the kernel), float32 accumulation, the fp16 epilogue.  yolo_net_describe() prints dtype=mxf8 and marks those convs. */
enum yolo_dtype { YOLO_DTYPE_F32 = 0, YOLO_DTYPE_F16 = 1, YOLO_DTYPE_MXF8 = 2 };

enum yolo_nms_mode {
    YOLO_NMS_AGNOSTIC = 0,  /* the reference: class_idx never consulted (base.py:195-209) */
    YOLO_NMS_PER_CLASS = 1  /* opt-in: only boxes of the same class suppress each other   */
};

#define YOLO_MAX_SRC 4
#define YOLO_MAX_ANCHORS 8
#define YOLO_MAX_SCALES 4

/* One entry per element of the reference's `layers` list (index 0 = input layer). */
typedef struct yolo_layer_desc {
    int32_t op;                         /* enum yolo_op                                  */
    int32_t n_src;
    int32_t src[YOLO_MAX_SRC];          /* indices into the layer list                   */
    int32_t filters, ksize, stride;     /* conv / maxpool / reorg / upsample             */
    int32_t batch_norm;                 /* conv: 1 -> beta,gamma,mean,var,kernel stream  */
    int32_t leaky;                      /* conv: 1 -> leaky 0.1, 0 -> linear             */
    int32_t h, w, c;                    /* input layer                                   */
    int32_t n_anchors;                  /* yolo layer                                    */
    double anchors[2 * YOLO_MAX_ANCHORS];/* yolo layer: (w,h) pairs in GRID units (float64 like layers.py:131) */
} yolo_layer_desc;

typedef struct yolo_net_options {
    int32_t dtype;          /* enum yolo_dtype: storage/operand type (accumulation is f32)     */
    int32_t max_batch;      /* buffers are planned for this many images                        */
    int32_t keep_all;       /* 1: no activation-buffer reuse, so yolo_net_read_layer works     */
    int32_t cand_capacity;  /* candidates per image the decode stage can hold (0 -> 4096; up to
                             * 4096 sort + NMS run in LDS, up to 65536 on global-memory slabs; an image
                             * with at most 512 candidates always takes the single-wave LDS path)    */
    int32_t max_boxes;      /* records per image written by detect / decode_nms (0 -> 256)     */
    int32_t streams;        /* 1: one pass on the caller's stream; 2..4: the batch runs as that many independent
                             * parts on the caller's + internal streams (overlaps the kernels' tails and launch
                             * boundaries); 0: the library's rule (two parts for fp16 nets of >= 40 conv launches
                             * whose half batch is >= 2.5 M input pixels, e.g. YOLOv3-608 at batch >= 16, else one;
                             * the environment variable YOLO_STREAMS overrides the rule; yolo_net_tune_streams() re-measures
                             * the rule's "two" on the device).  Results do not depend on it up to fp16 summation order.
                             * yolo_net_num_streams() tells what a net runs with.                              */
    int32_t force_tile;     /* 0: per-layer tile choice (cost model / autotune); t + 1: run conv tile id t on every
                             * conv layer that accepts it (0 = 4-wave kernel, 1-7 and 14 LDS-DMA tiles, 8-13 and 15-17
                             * tap-reuse tiles; 24 = the MXFP8 3x3 kernel, accepted only by a YOLO_DTYPE_MXF8 net that has a conv
                             * it takes -- else yolo_net_create fails with YOLO_ERR_ARG): test and tuning hook, any value gives the
                             * same results up to summation order   */
    int32_t guard_bytes;    /* test hook (guard-band canaries): this many extra, never-used bytes behind every planned activation
                             * tensor (rounded into the tensor's 4 KiB-aligned region); with keep_all = 1 no two tensors share bytes, so a
                             * pattern-filled workspace shows any kernel that writes outside its tensor (yolo_net_workspace_regions);
                             * 0 in production                                                                                */
    int32_t f32_products;   /* float32 nets (ABI 5): how the long-K convs of the 4-wave kernel multiply.  0: the library's rule -- whole-K
                             * launches with K >= 4608 and >= 256 workgroups (tiny-YOLOv2's 13 x 13 512 -> 1024 and 1024 -> 1024 layers) run
                             * every float32 product as NINE bf16 x bf16 products on the bf16 matrix cores (a float32 value is exactly the
                             * sum of three bf16 values; each partial product is exact, the sums accumulate in float32: not narrower than
                             * tf.layers.conv2d's float32, net/layers.py:31-39; 16/9 of the float32 matrix rate); 1: native float32 MFMA
                             * everywhere; 2: nine bf16 products wherever the kernel applies.  Ignored by fp16 nets.                   */
} yolo_net_options;

/* Result record; field names follow net/base.py:257-272 BoundingBox. */
typedef struct yolo_box {
    float x, y, w, h;       /* centre / size, normalised to the image */
    float prob;
    int32_t class_idx;
} yolo_box;

/* Head geometry for the standalone decode (the reference reads the same from
 * net[-1].yolos[i].{h,w,b,anchors}, net/v3.py:145-149; v2 has one scale). */
typedef struct yolo_head_desc {
    int32_t version;                    /* 2: p = sigmoid(obj)*max softmax(cls); 3: p = sigmoid(obj) */
    int32_t n_classes;
    int32_t n_scales;
    int32_t h[YOLO_MAX_SCALES], w[YOLO_MAX_SCALES], n_anchors[YOLO_MAX_SCALES];
    double anchors[YOLO_MAX_SCALES][2 * YOLO_MAX_ANCHORS];  /* grid units, (w,h) pairs */
} yolo_head_desc;

typedef struct yolo_net yolo_net;

int yolo_hip_abi_version(void);
const char *yolo_last_error(void);                  /* thread-local message of the last failure */

/* ---- network object ------------------------------------------------------------------ */
int yolo_net_create(const yolo_layer_desc *layers, int n_layers, const yolo_net_options *opt, yolo_net **out);
void yolo_net_destroy(yolo_net *net);

size_t yolo_net_weight_count(const yolo_net *net);      /* float32 values the Darknet stream must hold  */
size_t yolo_net_weights_bytes(const yolo_net *net);     /* device bytes for the packed (BN-folded) weights */
size_t yolo_net_workspace_bytes(const yolo_net *net);   /* device bytes for activations + decode scratch */
size_t yolo_net_output_count(const yolo_net *net);      /* float32 values per image of the head output  */
double yolo_net_flops_per_image(const yolo_net *net);   /* sum 2*Ho*Wo*Cout*k*k*Cin over convs          */
int yolo_net_head_desc(const yolo_net *net, yolo_head_desc *out);
/* nets whose last layer is a plain conv (YOLOv2: the reference keeps anchors outside the graph,
 * net/v2.py:83-85) get their head geometry from the caller before detect() */
int yolo_net_set_head(yolo_net *net, const yolo_head_desc *head);
int yolo_net_num_kernels(const yolo_net *net);
int yolo_net_num_streams(const yolo_net *net);      /* parts / HIP streams a full batch currently runs as (yolo_net_options.streams) */
/* Where streams = 0 picked two halves by rule, both activation arenas hold a FULL batch and this call (optional, once, with a batch
 * above max_batch / 2; synchronous, 30 forward passes) times one pass against two halves on THIS device and keeps two halves where they win by 1.5 %: the same
 * build gains 3-4 % from two halves on one MI355X and loses 1-2 % on another (power-limited clocks differ from board to board).
 * No-op for nets whose streams were given explicitly or whose rule says one.  The Python engine calls it at its first full batch. */
int yolo_net_tune_streams(yolo_net *net, const float *in_dev, int batch, void *stream);
/* The same choice made by the caller instead of a measurement: 1 = one pass, 2 = two halves, for a net whose streams = 0 rule planned both
 * (else only the value it already runs with is accepted: YOLO_ERR_STATE otherwise).  For processes that must all run the SAME plan -- the ranks
 * of a sharded batch (net/dist.py broadcasts rank 0's measurement: fp16 sums of one pass and of two halves differ in order, and the step time of
 * the job is the slowest rank's).  Not a reference call site: net/yolo.py:65-67 is one process, one session. */
int yolo_net_set_streams(yolo_net *net, int parts);
/* Diagnostic (ABI 5; tests/test_gpu_ops.py::test_no_kernel_writes_outside_its_tensor): the regions of the workspace the plan laid out -- every
 * activation tensor of every arena, the head logits of detect(), candidate lists, counters, NMS scratch, the compact objectness array, the
 * split-K slabs.  Bytes [offset, offset + used_bytes) are the region's payload; [offset + used_bytes, offset + region_bytes) belong to it but are
 * never written by any kernel.  Fills at most `cap` records, returns the number of regions.  No reference call site (net/yolo.py holds no buffers). */
typedef struct yolo_ws_region {
    char name[32];
    uint64_t offset, used_bytes, region_bytes;
} yolo_ws_region;
int yolo_net_workspace_regions(const yolo_net *net, yolo_ws_region *out, int cap);
/* human-readable plan (kernels, fusions, buffers); returns bytes needed incl. NUL */
size_t yolo_net_describe(const yolo_net *net, char *buf, size_t cap);

/* host_weights: the float32 body of a Darknet .weights file (header stripped), n values, in
 * layer-list order.  dev_weights: caller-owned device memory of yolo_net_weights_bytes().
 * Folds BN in fp32/fp64 on the host, repacks to the kernel layout, copies H2D (synchronous). */
int yolo_net_load_weights(yolo_net *net, const float *host_weights, size_t n, void *dev_weights, size_t dev_bytes);
int yolo_net_bind_workspace(yolo_net *net, void *dev_workspace, size_t dev_bytes);

/* in_dev: float32 NHWC [batch,h,w,c] in [0,1] RGB (what net/base.py:115-155 produces, as f32).
 * out_dev: float32, reference layout -- v2 [B,h,w,A*(5+C)], v3 [B,sum(h*w*3),5+C] coarse->fine. */
int yolo_net_forward(yolo_net *net, const float *in_dev, int batch, float *out_dev, void *stream);

/* uint8 network input (ABI 7).  in_dev: uint8 NHWC [batch,h,w,c], values 0..255, RGB: the pixels net/base.py:115-155 has BEFORE its
 * `/ 255.` (net/base.py:153), fed where net/yolo.py:83 feeds x_batch.  Dense (h*w*c bytes per image), any byte alignment.  The kernels
 * that read the input -- the Darknet-53 stem, the first-layer kernels, the fallback input cast -- have uint8 twins that turn a byte u into
 * float32(u / 255.) (division in float64 as NumPy does it = the correctly rounded float32 quotient; not u * float32(1 / 255), which differs
 * for 126 of the 256 bytes) and go on as their float32 forms do; every later kernel is the same launch on the same operands.  So each
 * *_u8 entry returns BIT-IDENTICAL results to its float32 twin fed float32(u / 255.), for every dtype and stream mode, with a quarter of
 * the input bytes to produce, copy and read.  The input type is a property of the call: one net serves both.  Argument checks and
 * messages as the float32 twins.  yolo_net_autotune stays float32-only (the tile choice does not depend on the input type), and
 * yolo_net_kernel_info keeps describing the float32 plan: the uint8 twins carry the same names with `_u8_kernel` for `_kernel`
 * (yolo::stem_v3_u8_kernel, yolo::first_pool_mfma_u8_kernel, yolo::first_pool_mfma_f32_u8_kernel<>, yolo::conv_first_u8_kernel<>,
 * yolo::prep_u8_kernel<>). */
int yolo_net_forward_u8(yolo_net *net, const uint8_t *in_dev, int batch, float *out_dev, void *stream);
/* yolo_net_tune_streams on a uint8 batch (net/yolo.py:65-67 is one session: no reference call site) */
int yolo_net_tune_streams_u8(yolo_net *net, const uint8_t *in_dev, int batch, void *stream);
/* The conversion above for u = 0..255, computed on the host by the function the input kernels run on every byte: out256[u] = float32(u / 255.)
 * (test hook; no reference call site beyond net/base.py:153). */
int yolo_u8_unit_table(float *out256);

/* How much work one ROUND of the looping kernels holds (test hook, added within ABI 7: one new export and this POD): the persistent
 * kernels run at most this many workgroups and each walks tiles blockIdx, blockIdx + grid, ...; the grid-stride kernels launch at most this
 * many threads.  Work beyond a cap is what gives a workgroup its second tile (a thread its second item) -- the tests of that hand-over
 * size their cases from these numbers, so a changed cap shows there instead of quietly turning them into one-round tests.
 * tap_stream_workgroups: conv3x3_tap_stream_kernel, tiles of 16 x 16 positions; stem_workgroups: stem_v3_kernel on ONE part (a batch
 * split over n streams runs cap / n per part), tiles of 8 x 16 outputs; first_mfma_workgroups: first_pool_mfma*_kernel, tiles of 8 x 16
 * pooled outputs; aux_work_items: prep / pool / pool_same / eltwise / splitk_reduce; decode_rows: decode_kernel. */
struct yolo_launch_caps {
    int32_t tap_stream_workgroups, stem_workgroups, first_mfma_workgroups, aux_work_items, decode_rows;
};
int yolo_launch_caps(struct yolo_launch_caps *out);

/* Optional: time every valid tile configuration of each heavy conv on the device (synchronous, a few
 * hundred launches) and keep the fastest per layer for later forward/detect calls at this batch. */
int yolo_net_autotune(yolo_net *net, const float *in_dev, int batch, void *stream);

/* forward + decode + NMS.  boxes_dev: [batch][max_boxes] yolo_box, counts_dev: [batch] int32
 * (number of valid records, descending prob, stable); status_dev: [batch] int32
 * (0 ok, 1 candidate overflow, 2 more survivors than max_boxes: list truncated).
 * threshold is compared in float32 (`p < threshold`, net/v2.py:107), iou_threshold in float64
 * (`iou >= iou_threshold`, net/base.py:204), as NumPy does in the reference. */
int yolo_net_detect(yolo_net *net, const float *in_dev, int batch, double threshold, double iou_threshold,
                    int nms_mode, yolo_box *boxes_dev, int32_t *counts_dev, int32_t *status_dev, void *stream);

/* yolo_net_detect on a uint8 batch (net/yolo.py:83-86 with the pixels of net/base.py:115-155 before the / 255.): see yolo_net_forward_u8. */
int yolo_net_detect_u8(yolo_net *net, const uint8_t *in_dev, int batch, double threshold, double iou_threshold,
                       int nms_mode, yolo_box *boxes_dev, int32_t *counts_dev, int32_t *status_dev, void *stream);

/* Per-kernel facts for roofline accounting (bench.py): algorithmic work of ONE image.  Always the plan of the float32 entry points
 * (input bytes counted as float32, float32 kernel symbols), also for a net that is only ever fed uint8. */
typedef struct yolo_kernel_info {
    int32_t kind;               /* 0 prep, 1 conv, 2 maxpool (incl. the fused SPP block: one read, three writes), 3 eltwise */
    int32_t layer;              /* reference layer index the kernel materialises                 */
    int32_t variant;            /* conv: cout-tile config (0 N128, 1 N64, 2 N32) + 4*perchunk    */
    int32_t ksize, stride, cin, cout, out_h, out_w;
    double flops;               /* conv: 2*Ho*Wo*Cout*k*k*Cin, else 0                            */
    double bytes;               /* input + output (+ residual) elements * element size           */
    double weight_bytes;        /* packed weights + bias read once per launch (not per image)    */
    char name[64];              /* readable label of the kernel family, e.g. "conv_igemm_dma<f16,128x256,tap9,x2>" */
    char symbol[160];           /* the kernel's name exactly as rocprofv3 --kernel-trace prints it, e.g.
                                 * "void yolo::conv3x3_tap_kernel<false, 2, 4, 4, 4, 26, 4, 1>(yolo::ConvParams)":
                                 * joins roofline.kernel_symbol of bench.py to the kernel_stats CSVs under profiles/; "" = no launch */
} yolo_kernel_info;
int yolo_net_kernel_info(const yolo_net *net, int kernel, yolo_kernel_info *out);

/* yolo_net_forward with every kernel bracketed by hipEvents recorded on `stream`; synchronises and
 * writes the device time of each kernel in milliseconds to ms_host[yolo_net_num_kernels()].
 * Measurement aid only (the events add bubbles): never used for throughput numbers. */
int yolo_net_forward_timed(yolo_net *net, const float *in_dev, int batch, float *out_dev, void *stream, float *ms_host);

/* yolo_net_forward_timed on a uint8 batch: ms_host[k] of an input kernel is the time of its uint8 twin (net/yolo.py:83). */
int yolo_net_forward_timed_u8(yolo_net *net, const uint8_t *in_dev, int batch, float *out_dev, void *stream, float *ms_host);

/* debug / parity: copy one layer's output to host as dense float32 NHWC (needs keep_all; synchronous) */
int yolo_net_read_layer(yolo_net *net, int layer, int batch, float *host_out, size_t n);

/* MXFP8 quantizer of the MX conv kernel (ABI 6), for testing: `rows` x `channels` fp16 values (device, 16-byte aligned, channels % 32 == 0)
 * -> q_dev[rows][channels] e4m3fn bytes and scale_dev[rows][channels / 32] E8M0 bytes, by the device function the kernel runs on its
 * patches (OCP MX v1.0: e = floor(log2 amax) - 8, elements rounded to nearest even and saturated to +-448, amax 0 -> scale byte 0).
 * stream: a hipStream_t or NULL.  Asynchronous. */
int yolo_mx_quantize(const void *src_f16_dev, int rows, int channels, uint8_t *q_dev, uint8_t *scale_dev, void *stream);
/* The same rule on the host, as yolo_net_load_weights applies it to the folded float32 weights of the MX convs (ABI 6, testing):
 * rows x channels float32 values (host) -> q[rows][channels] e4m3fn bytes, scale[rows][channels / 32] E8M0 bytes. */
int yolo_mx_quantize_host(const float *src, int rows, int channels, uint8_t *q, uint8_t *scale);

/* ---- standalone decode + NMS (drop-in for find_bounding_boxes) --------------------- */
size_t yolo_decode_scratch_bytes(const yolo_head_desc *head, int batch, int cand_capacity);
int yolo_decode_nms(const yolo_head_desc *head, const float *logits_dev, int batch, double threshold,
                    double iou_threshold, int nms_mode, int cand_capacity, int max_boxes, void *scratch_dev,
                    size_t scratch_bytes, yolo_box *boxes_dev, int32_t *counts_dev, int32_t *status_dev,
                    void *stream);

/* Image preprocessing of the TEST loop, replaces net/base.py:115-155 (cv2.resize INTER_LINEAR stretch to the network
 * input, optional BGR<->RGB swap, / 255.): src_dev is a decoded uint8 HWC image with 3 channels on the device
 * (src_row_bytes >= 3*src_w), dst_dev receives float32 [dst_h][dst_w][3] in [0,1].  Bit-exact with OpenCV's published
 * 8-bit INTER_LINEAR algorithm as restated in oracle/preprocess_ref.py (OpenCV itself is not available: unpinned).
 * Enqueued on `stream`. */
int yolo_preprocess_resize(const uint8_t *src_dev, int src_h, int src_w, int src_row_bytes, float *dst_dev, int dst_h, int dst_w,
                           int swap_rb, void *stream);

/* The same resize with the 8-bit value itself as the result (net/base.py:115-155 up to, not including, the / 255. of :153):
 * dst_dev receives uint8 [dst_h][dst_w][3], the image layout of yolo_net_forward_u8 / yolo_net_detect_u8.  yolo_preprocess_resize of the
 * same source is float32(that / 255.) exactly. */
int yolo_preprocess_resize_u8(const uint8_t *src_dev, int src_h, int src_w, int src_row_bytes, uint8_t *dst_dev, int dst_h, int dst_w,
                              int swap_rb, void *stream);

/* ---- frames of any size: batched resize, letterbox, boxes in frame coordinates (added within ABI 7) ------------------------------
 * One decoded frame on the device: uint8 HWC, 3 channels, row_bytes >= 3 * w, any byte alignment.  swap_rb != 0: channels 0 and 2 change
 * places on the way (a BGR frame for an RGB network, net/base.py:152). */
typedef struct yolo_frame {
    const uint8_t *pixels_dev;
    int32_t h, w, row_bytes, swap_rb;
} yolo_frame;

enum yolo_resize_mode {
    YOLO_RESIZE_STRETCH = 0,    /* the reference: cv2.resize to the network input, aspect ratio not kept (net/base.py:121)  */
    YOLO_RESIZE_LETTERBOX = 1   /* Darknet's `detector test`: aspect ratio kept, the rest of the canvas is the byte 128     */
};

/* Where a src_h x src_w frame lands in a dst_h x dst_w network input, in integers (pure host function, no device).  Stretch: new = dst,
 * offsets 0.  Letterbox (Darknet's letterbox_image with its float comparison replaced by the exact cross-multiplied one): if
 * dst_w * src_h < dst_h * src_w the width binds -- new_w = dst_w, new_h = max(1, src_h * dst_w / src_w) -- else new_h = dst_h,
 * new_w = max(1, src_w * dst_h / src_h) (integer division); off_x = (dst_w - new_w) / 2, off_y = (dst_h - new_h) / 2.  Small frames are
 * enlarged, as Darknet does.  All sizes >= 1 (and below 2^31: the products are taken in 64 bits). */
int yolo_letterbox_geometry(int src_h, int src_w, int dst_h, int dst_w, int mode, int32_t *new_h, int32_t *new_w, int32_t *off_y,
                            int32_t *off_x);

/* The resize of a whole batch: frames_host[0..n) (a HOST array; the descriptors travel in the kernel arguments, at most 64 frames per
 * launch, larger n as consecutive launches -- no device table, no copy, nothing in the workspace) -> dst_dev, the dense batch tensor
 * uint8 [n][dst_h][dst_w][3] of yolo_net_forward_u8 / yolo_net_detect_u8.  Frames may differ in size, pitch and alignment.  Inside the
 * new_h x new_w region of yolo_letterbox_geometry every pixel is what yolo_preprocess_resize_u8 gives for that frame resized to
 * (new_h, new_w) -- the project's one resize arithmetic, OpenCV's 8-bit INTER_LINEAR, not Darknet's bilinear; outside it the byte 128
 * (written without touching the source).  Every byte of the n images is written by each call.  A thread produces 4 consecutive pixels
 * of a row and stores them as dwords: dst_w must be a multiple of 4 (every network width is: YOLO_ERR_ARG otherwise); a dst_dev that is
 * not 4-byte aligned (16 for the float32 twin) is served by narrower stores.  Enqueued on `stream`. */
int yolo_preprocess_frames_u8(const yolo_frame *frames_host, int n, int mode, uint8_t *dst_dev, int dst_h, int dst_w, void *stream);
/* The same with float32 [n][dst_h][dst_w][3] results, the batch tensor of yolo_net_forward / yolo_net_detect: float32(u / 255.) of the
 * uint8 result by the conversion of the uint8 input kernels (yolo_u8_unit_table); the canvas is float32(128 / 255.). */
int yolo_preprocess_frames(const yolo_frame *frames_host, int n, int mode, float *dst_dev, int dst_h, int dst_w, void *stream);

/* Box records of a detect call on such a batch (normalised to the net_h x net_w network input) -> normalised to each frame, in place:
 * the first counts_dev[i] (at most max_boxes) records of image i, with (new_h, new_w, off_y, off_x) = yolo_letterbox_geometry of frame i,
 *     x' = float32((double(x) * net_w - off_x) / new_w)      w' = float32(double(w) * net_w / new_w)
 *     y' = float32((double(y) * net_h - off_y) / new_h)      h' = float32(double(h) * net_h / new_h)
 * (the products are exact in float64, then one IEEE division and one narrowing: NumPy's float64 gives the same bits).  prob and class_idx
 * stay; nothing is clipped (net/base.py:212-226 draw_boxes clamps).  Records behind the count are not touched.  NMS has run in network
 * coordinates before: set and order of the boxes are those of the detect call.  YOLO_RESIZE_STRETCH changes nothing and launches
 * nothing.  Only h and w of the frame descriptors are read; the geometry travels in the kernel arguments, 64 images per launch. */
int yolo_boxes_to_frames(yolo_box *boxes_dev, const int32_t *counts_dev, int batch, int max_boxes, const yolo_frame *frames_host, int mode,
                         int net_h, int net_w, void *stream);

/* One enqueue for a whole step: yolo_preprocess_frames_u8 of frames_host[0..batch) into the caller's batch_dev (uint8
 * [batch][H][W][3], H x W the network input, which must have 3 channels), yolo_net_detect_u8 on it, yolo_boxes_to_frames on the
 * survivors.  Records, counts and status are those of yolo_net_detect_u8 on that batch tensor, boxes normalised to each frame.
 * Argument checks and messages as yolo_net_detect_u8, plus the frames' (h, w >= 1, row_bytes >= 3 w). */
int yolo_net_detect_frames_u8(yolo_net *net, const yolo_frame *frames_host, int batch, int mode, uint8_t *batch_dev, double threshold,
                              double iou_threshold, int nms_mode, yolo_box *boxes_dev, int32_t *counts_dev, int32_t *status_dev,
                              void *stream);

/* ---- VOC-style evaluation on the device: match, AP, mAP (added within ABI 7: new exports, new PODs, nothing existing changed) ------
 * Average precision against ground truth as VOCdevkit's voc_eval and Darknet's `detector map` define it, on the records that
 * yolo_net_detect* left on the device.  No reference call site: the reference has parse_annotations (net/base.py:69-97) and nothing
 * that scores a detector; the IoU is its net/base.py:180-192.
 *
 * Definitions.
 *   IoU           net/base.py:180-192 in float64 with all eight float32 fields promoted, union floored at 1e-8 (np.maximum: a NaN
 *                 stays a NaN).  Every operation is rounded on its own, as NumPy rounds it -- the intersection's product of two float64
 *                 differences is not exact in general, so the kernel forbids FMA contraction here: the value equals NumPy's bit for bit.
 *   best truth    of a detection: among the truths of the SAME image and SAME class_idx, difficult ones included, the one of largest IoU;
 *                 ties go to the lowest index; an IoU that is NaN never wins.  No candidate: best_gt = -1, best_iou = 0, verdict FP.
 *   verdict       detections in the global order (prob descending, then seq ascending; seq = image_index * max_boxes + rank in the
 *                 image's list, a uint32).  best_iou > match_iou and the best truth difficult: IGNORED (neither TP nor FP, the truth is
 *                 not taken).  best_iou > match_iou and the best truth not yet taken: TP, the truth is taken.  Otherwise FP.  The
 *                 comparison is STRICT, as in VOCdevkit and Darknet -- a deliberate difference from the `>=` of NMS (net/base.py:204):
 *                 a detection whose IoU is exactly match_iou is a false positive.
 *   per image     a list in non-increasing prob order (yolo_net_detect* guarantees it) decides the global rule per image: the TP of a
 *                 truth is the FIRST detection in list order that claims it.  A list that is not ordered sets YOLO_EVAL_UNSORTED.
 *   per class c   n_gt[c] counts the non-difficult truths; the records of c sorted by (prob descending, seq ascending); ctp[k], cfp[k]
 *                 integer cumulative counts with IGNORED records contributing nothing; in float64 recall = ctp / n_gt and
 *                 precision = ctp / max(ctp + cfp, 2^-52) (VOCdevkit's eps).  ap_voc12 = sum over the TPs of (envelope precision at that
 *                 TP) / n_gt, the area under the monotone precision envelope; ap_voc07 = sum over i = 0..10 of (the envelope at the first
 *                 record with recall >= i / 10.0, else 0) / 11.  n_gt[c] == 0: both NaN, the class is left out of the means.
 *   mAP           the mean over the classes with truths, NaN if there are none. */
typedef struct yolo_gt {
    float x, y, w, h;       /* centre / size, normalised like yolo_box (to the frame where the detections come from the frame entries) */
    int32_t class_idx;
    int32_t difficult;      /* VOC's flag: != 0 -- matching it is IGNORED, it is not counted in n_gt */
} yolo_gt;

enum yolo_eval_verdict { YOLO_EVAL_FP = 0, YOLO_EVAL_TP = 1, YOLO_EVAL_IGNORED = 2 };

/* bits of the status word (yolo_eval_result.status; also readable in the state at yolo_eval_layout.status_offset) */
enum yolo_eval_status {
    YOLO_EVAL_OVERFLOW = 1,     /* more records than det_capacity: nothing was written behind the capacity, the result covers the first ones kept */
    YOLO_EVAL_UNSORTED = 2,     /* an image's list was not in non-increasing prob order                                    */
    YOLO_EVAL_BAD_CLASS = 4,    /* a truth or a detection with class_idx outside [0, n_classes): skipped                  */
    YOLO_EVAL_BAD_COUNT = 8     /* a count below 0 or above max_boxes / max_gt: clamped                                    */
};

#define YOLO_EVAL_MAX_GT 1024               /* truths per image (they live in LDS)  */
#define YOLO_EVAL_MAX_DET_CAPACITY (1 << 20)
#define YOLO_EVAL_MAX_CLASSES 65536

typedef struct yolo_eval_desc {
    int32_t n_classes;      /* 1 .. YOLO_EVAL_MAX_CLASSES                                */
    int32_t det_capacity;   /* records the state holds, 1 .. YOLO_EVAL_MAX_DET_CAPACITY */
    int32_t max_gt;         /* truths per image the caller's arrays hold, 1 .. YOLO_EVAL_MAX_GT */
    int32_t pad_;
    double match_iou;       /* in [0, 1]; VOC: 0.5                                       */
} yolo_eval_desc;

/* one detection after matching (32 bytes) */
typedef struct yolo_eval_record {
    double best_iou;
    float prob;
    int32_t class_idx;
    uint32_t seq;
    int32_t verdict;        /* enum yolo_eval_verdict */
    int32_t best_gt;        /* index into the image's truths or -1 */
    int32_t pad_;
} yolo_eval_record;

typedef struct yolo_eval_class {
    double ap_voc12, ap_voc07;
    int32_t n_gt, n_det, tp, fp, ignored, pad_;
} yolo_eval_class;

/* result block: this header, then yolo_eval_class[n_classes] */
typedef struct yolo_eval_result {
    double map_voc12, map_voc07;
    int32_t n_records;      /* records kept (at most det_capacity) */
    int32_t status;         /* enum yolo_eval_status bits          */
    int32_t n_classes, pad_;
} yolo_eval_result;

/* Where the readable parts of the state are (byte offsets): status word (uint32), n_gt int32[n_classes], the records in arrival order,
 * and after yolo_eval_finish the records in sorted order (class ascending, prob descending, seq ascending) with ctp / cfp uint32 per
 * sorted position; the first yolo_eval_result.n_records entries of each are valid. */
typedef struct yolo_eval_layout {
    uint64_t status_offset, n_gt_offset, records_offset, sorted_offset, ctp_offset, cfp_offset, total_bytes;
} yolo_eval_layout;

/* Device bytes of the caller-owned state / of the result block; 0 for a bad descriptor (yolo_last_error says why).  Replaces nothing. */
size_t yolo_eval_state_bytes(const yolo_eval_desc *desc);
size_t yolo_eval_result_bytes(const yolo_eval_desc *desc);
int yolo_eval_state_layout(const yolo_eval_desc *desc, yolo_eval_layout *out);
/* An empty state: no records, no truths, status 0.  state_bytes >= yolo_eval_state_bytes (YOLO_ERR_ARG otherwise).  Enqueued.  Replaces nothing. */
int yolo_eval_reset(const yolo_eval_desc *desc, void *state_dev, size_t state_bytes, void *stream);
/* One step's detections against its truths: boxes_dev [batch][max_boxes] and counts_dev [batch] as yolo_net_detect* wrote them,
 * gt_dev [batch][max_gt] yolo_gt with gt_counts_dev [batch]; image_base = index of image 0 of this call in the dataset (seq).  One
 * workgroup per image, enqueued on `stream` with no host synchronisation: it can follow yolo_net_detect* directly.  YOLO_ERR_ARG if
 * (image_base + batch) * max_boxes does not fit 32 bits.  Replaces nothing in the reference (there is no evaluation there). */
int yolo_eval_add(const yolo_eval_desc *desc, void *state_dev, const yolo_box *boxes_dev, const int32_t *counts_dev, int batch, int max_boxes,
                  const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int64_t image_base, void *stream);
/* Once per dataset: sorts the records, scans TP / FP per class, computes both APs per class and the means into result_dev
 * (yolo_eval_result_bytes).  Enqueued; the state stays valid and further yolo_eval_add calls may follow.  Replaces nothing. */
int yolo_eval_finish(const yolo_eval_desc *desc, void *state_dev, void *result_dev, void *stream);

/* ---- YOLOv2 loss on the device (added within ABI 7: new exports, new PODs, nothing existing changed) ------------------
 * The number net/yolo.py:177-193 prints as `validation loss`: net/v2.py:123-198 create_loss_fn over the truth tensors of
 * net/v2.py:242-295 _make_ground_truths.  Its gradient: yolo_v2_loss_grad below.  YOLOv2 heads only (the reference binds no loss to YoloV3, net/yolo.py:208-211).
 *
 * Inputs.     logits float32 [B][h][w][A][5 + C], the v2 layout of yolo_net_forward; a yolo_head_desc with version == 2, n_scales == 1 and
 *             anchors (aw, ah) in grid units; truths yolo_gt [B][max_gt] with int32 counts [B], centre / size normalised float32 -- to
 *             the frame, which under the reference's stretch resize (net/base.py:121) is also the network input.  `difficult` is ignored:
 *             the reference's parser does not read it (net/base.py:69-97).
 * Truth to grid (net/v2.py:252-257), in float64: bx = double(x) * w, by = double(y) * h, bw = double(w_) * w, bh = double(h_) * h,
 *             cx = floor(bx), cy = floor(by).  Skipped, with a bit in the status word: a truth whose cx or cy lies outside the grid
 *             (YOLO_LOSS_OUT_OF_GRID; x == 1.0 too, where the reference would index out of range; a NaN centre too), one whose w_ or h_
 *             is negative or NaN (YOLO_LOSS_BAD_BOX), one whose class_idx is outside [0, C) (YOLO_LOSS_BAD_CLASS).  A count outside
 *             [0, max_gt] is clamped (YOLO_LOSS_BAD_COUNT).
 * Assignment (net/v2.py:261-289).  Per grid cell, over its truths in list order and the anchors in index order: the float64 IoU of
 *             net/base.py:180-192 of the box (w / 2, h / 2, bw, bh) against (w / 2, h / 2, aw, ah), every operation rounded on its own
 *             (the arithmetic of the evaluation's IoU, one function for both: union floored at 1e-8, no FMA contraction).  The winner is
 *             the FIRST (truth, anchor) pair that reaches the cell's largest IoU: the reference replaces on strict `best_iou < iou`
 *             starting from -1, so a zero-size truth takes anchor 0 and a NaN never wins (a cell all of whose IoUs are NaN has no winner;
 *             the reference would fail there).  One winner per cell: its anchor slot holds gt = float32(bx, by, bw, bh) and the truth's
 *             class; mask_ij = 1 for that slot, mask_i = 1 for the cell.
 * Terms (net/v2.py:128-188), float32 operations (the graph is float32, the anchors are rounded to float32), each rounded on its own:
 *             px = sigmoid(t0) + c, py = sigmoid(t1) + r, pw = exp(t2) * aw, ph = exp(t3) * ah, po = sigmoid(t4), with the sigmoid and
 *             exp of the decode (1 / (1 + expf(-t)), expf); iou = the float32 IoU of net/v2.py:157-173 of gt against (px, py, pw, ph),
 *             no floor on the union.
 *               winner slot:      xy = (gx - px)^2 + (gy - py)^2;  wh = (sqrt gw - sqrt pw)^2 + (sqrt gh - sqrt ph)^2;  obj = (iou - po)^2
 *               every other slot: noobj = po^2
 *               class:            softmax cross-entropy of t[5:], log(sum_k exp(t_k - m)) - (t_label - m) with m = max_k t_k.
 *                                 REFERENCE BEHAVIOUR, reproduced as it is: it applies to ALL A anchor slots of a cell with mask_i = 1
 *                                 (mask_i broadcasts over the anchors, v2.py:185-186) -- label = the winner's class on the winner slot and
 *                                 0 on the others (the argmax of an all-zero one-hot, v2.py:155);
 *                                 REFERENCE BEHAVIOUR, reproduced as it is: the class sum is NOT divided by the batch (v2.py:185).
 * Totals.     loss_xy = S xy / B, loss_wh = S wh / B, loss_obj = 5 * S obj / B, loss_noobj = S noobj / B, loss_class = S class,
 *             loss = loss_xy + loss_wh + loss_obj + loss_noobj + loss_class (added in this order).
 * Two DELIBERATE DIFFERENCES from the reference:
 *   (a) cell offsets.  The reference's offset tensor (v2.py:128-134) is (k % h, k / h) at k = r * w + c, which is (c, r) only on a
 *       square grid.  Here the offsets are (c, r) on every grid.
 *   (b) masked-out slots.  Their terms are never formed, so an infinite pw on a slot that is not a winner does not turn a sum into NaN
 *       as 0 * inf does in TensorFlow.  The two agree whenever every exp is finite.
 * Sums.       Every float32 term is widened to float64 and added in a FIXED order: a thread's own slots in index order, the lane tree
 *             inside a wave, the waves in index order through LDS, the images in index order.  No floating-point atomics: two calls on
 *             the same input return the same bits. */
enum yolo_loss_status {
    YOLO_LOSS_OUT_OF_GRID = 1,  /* a truth whose cell lies outside the grid: skipped                */
    YOLO_LOSS_BAD_BOX = 2,      /* a truth with a negative or NaN size: skipped                     */
    YOLO_LOSS_BAD_CLASS = 4,    /* a truth with class_idx outside [0, n_classes): skipped           */
    YOLO_LOSS_BAD_COUNT = 8     /* a count below 0 or above max_gt: clamped                         */
};

#define YOLO_LOSS_MAX_CELLS 4096            /* h * w of the head (the winner table lives in LDS) */

/* one image: the float64 sums of its terms, before weights and 1 / B (56 bytes) */
typedef struct yolo_loss_image {
    double xy, wh, obj, noobj, cls;
    int32_t n_assigned;     /* cells with a winner                  */
    int32_t n_truths;       /* truths that were not skipped         */
    int32_t status;         /* enum yolo_loss_status bits           */
    int32_t pad_;
} yolo_loss_image;

typedef struct yolo_loss_result {
    double loss, loss_xy, loss_wh, loss_obj, loss_noobj, loss_class;
    int32_t n_assigned, n_truths;   /* sums over the records added (a repeated record counts twice) */
    int32_t status;                 /* OR of the records' bits                                      */
    int32_t pad_;
} yolo_loss_result;

/* The standalone entry, as yolo_decode_nms is for the decode: logits already on the device.  images_dev [batch] receives the per-image
 * records, result_dev the totals; assign_dev, if not NULL, int32 [batch][h][w], receives the winner of every cell as
 * truth_index * 8 + anchor, or -1.  Two kernels (one workgroup per image; one workgroup that adds the records in image order), enqueued
 * on `stream` with no host synchronisation.  YOLO_ERR_ARG for a null pointer, batch < 1, max_gt outside 1..YOLO_EVAL_MAX_GT, a head
 * that is not version 2 / single-scale, or h * w > YOLO_LOSS_MAX_CELLS. */
int yolo_v2_loss(const yolo_head_desc *head, const float *logits_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev,
                 int max_gt, yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, void *stream);
/* One enqueue for a validation batch: a DENSE forward pass into the workspace logits (yolo_net_detect leaves rows below its threshold
 * unwritten, so its logits cannot be reused), then the kernels of yolo_v2_loss on them with the head of yolo_net_set_head: bit-identical
 * to yolo_net_forward[_u8] followed by yolo_v2_loss.  Checks and messages as yolo_net_forward plus those of yolo_v2_loss; a net whose
 * head was never set is told so first (YOLO_ERR_STATE, "head geometry not set"), before the head's version is looked at. */
int yolo_net_loss(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                  yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, void *stream);
int yolo_net_loss_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                     yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, void *stream);
/* The second kernel alone, over records collected from many calls (a validation set): adds images_dev[0 .. n_images) in index order,
 * then images_dev[0 .. n_repeat) once more (net/v2.py:215-217 pads the last batch with the first annotations of the set), and applies
 * the weights with B = batch_size.  The reference's `validation loss` (net/yolo.py:185-187) is each of the six values divided by the
 * number of batches, (n_images + n_repeat) / batch_size.  0 <= n_repeat <= n_images, n_images and batch_size >= 1.  Enqueued. */
int yolo_loss_reduce(const yolo_loss_image *images_dev, int n_images, int n_repeat, int batch_size, yolo_loss_result *result_dev,
                     void *stream);

/* ---- The gradient of the YOLOv2 loss with respect to the logits (added within ABI 7: one new export, nothing existing changed) ------
 * G = d loss / d logits, `loss` being the total of yolo_v2_loss above for the same call: the same truths to grid, skipped truths and
 * status bits, the same assignment, the same two reference behaviours and two deliberate differences.  Replaces tf.gradients of
 * net/v2.py:188 with respect to net[-1].out, as AdamOptimizer.minimize (net/v2.py:205) takes it; everything behind it (the backward pass
 * of a backbone, an optimizer) is not here.  G is float32 [B][h][w][A][5 + C] like the logits; EVERY element is written by every call,
 * zeros included.  Weights: lxy = lwh = lnoobj = 1 / B, lobj = 5 / B, lcls = 1 (the class term is not divided by the batch, v2.py:185;
 * its gradient is not either).
 *   slot that is not a winner:  G[0..3] = +0 exactly -- the terms of a masked-out slot are never formed (difference (b)), so an infinite
 *                      exp there gives 0, not NaN;  G[4] = lnoobj * 2 po * po (1 - po), po = sigmoid(t4).
 *   class rows:        every anchor slot of a cell WITH a winner (the reference's mask_i broadcast): G[5 + k] = softmax(t[5:])_k -
 *                      [k == label], label = the winner's class on the winner slot and 0 on the others, softmax as
 *                      exp(t_k - m) / sum_j exp(t_j - m), m = max_j t_j.  A cell without a winner: G[5:] = +0 exactly.
 *   winner slot:       in the notation of the terms above, sx = sigmoid(t0), px = sx + c, pw = exp(t2) * aw, gx .. gh the float32 truth,
 *                      iou = I(px, py, pw, ph), e = iou - po, k = lobj * 2 e:
 *                        dL/dpx = lxy * 2 (px - gx) + k * dI/dpx                    G[0] = dL/dpx * sx (1 - sx)      (G[1] likewise with y)
 *                        dL/dpw = lwh * (sqrt pw - sqrt gw) / sqrt pw + k * dI/dpw  G[2] = dL/dpw * pw               (G[3] likewise with h)
 *                        G[4] = -k * po (1 - po)
 *                      REFERENCE BEHAVIOUR, reproduced as it is: the gradient DOES flow through the IoU into x, y, w, h.  The reference
 *                      multiplies iou_score into gt_obj without a stop_gradient (v2.py:173-176), so its Adam step sees that path.
 *                      Darknet treats the IoU of its objectness target as a constant.
 *   IoU partials:      I = inter / uni, inter = iw * ih, uni = pw * ph + gw * gh - inter, rw = min(px2, gx2) - max(px1, gx1),
 *                      iw = max(rw, 0):
 *                        diw/dpx = [rw >= 0] ([px2 <= gx2] - [px1 >= gx1])          diw/dpw = [rw >= 0] ([px2 <= gx2] + [px1 >= gx1]) / 2
 *                        dI/dv = (dinter/dv * (uni + inter) - inter * d(pw ph)/dv) / uni^2, dinter/dpx = ih * diw/dpx,
 *                        dinter/dpw = ih * diw/dpw, d(pw ph)/dpw = ph, d(pw ph)/dpx = 0; y / h alike.
 *   ties:              the brackets are TensorFlow's rules, fixed here as part of the definition: maximum(x, y) gives its gradient to x
 *                      when x >= y, minimum(x, y) to x when x <= y, maximum(rw, 0) passes it when rw >= 0 (torch splits a tie in half).
 *                      A prediction that equals its truth therefore has dI/dpw = 1 / gw and dI/dpx = 0.
 * Arithmetic.   float32, element by element, with the sigmoid and expf of the decode and of the loss.  Nothing here is bit-exact against
 *               anything: an element is a product of several rounded factors.  The tests hold each group of elements (xy, wh, obj, class)
 *               of a call within 4 x the float32-against-float64 gap of a sequential restatement plus one float32 ulp.  Where float32
 *               arithmetic is not finite (an overflowing exp on a winner slot) the element is not finite; no other slot is affected.
 *
 * Runs the two kernels of yolo_v2_loss exactly as yolo_v2_loss does -- images_dev and result_dev receive the same bytes -- then the
 * gradient kernel (a wave per grid cell, grid = chunks of cells x images), all enqueued on `stream` with no host synchronisation.
 * assign_dev is REQUIRED here: the gradient kernel reads the winner table from it; caller-owned like every other buffer.  grad_dev:
 * batch * h * w * A * (5 + C) floats that do not overlap logits_dev.  Checks and messages as yolo_v2_loss, plus YOLO_ERR_ARG for a NULL
 * assign_dev or grad_dev and for grad_dev == logits_dev. */
int yolo_v2_loss_grad(const yolo_head_desc *head, const float *logits_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev,
                      int max_gt, yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, float *grad_dev,
                      void *stream);

/* ---- YOLOv3 loss and its gradient on the device (added WITHIN ABI 7: new exports only, nothing existing changed) ------------------
 * The loss of Darknet's [yolo] layer (forward_yolo_layer), the definition every YOLOv3 .weights file was trained with, and its gradient
 * with respect to the logits.  The reference has no loss for YoloV3 (net/yolo.py:208-211); yolo_v2_loss*, yolo_net_loss* and
 * yolo_net_train_head_step* keep refusing a version 3 head.  This stops at the logits; the weight gradient of the head convs from G is
 * yolo_v3_head_wgrad below.
 *
 * Inputs.     logits float32 [B][R][5 + C], the layout yolo_net_forward writes for a version 3 head: rows scale by scale in head order,
 *             inside a scale [h_s][w_s][A_s]; R = sum_s h_s * w_s * A_s.  A yolo_head_desc with version == 3, 1 <= n_scales <=
 *             YOLO_MAX_SCALES and anchors (aw, ah) in the grid units of their scale.  Truths yolo_gt [B][max_gt] with int32 counts [B],
 *             1 <= max_gt <= YOLO_EVAL_MAX_GT, centre / size normalised to the network input (stretch resize); `difficult` is ignored.
 *             ignore_thresh: a double in (0, 1]; upstream cfgs use 0.7.
 * Truth checks. As for yolo_v2_loss, with the same status bits: skipped are a truth whose centre lies outside [0, 1) in x or y -- its cell
 *             floor(x * w_s) would lie outside the grid, at every scale alike (YOLO_LOSS_OUT_OF_GRID; x == 1.0 too, a NaN too), one with
 *             w <= 0, h <= 0 or a NaN size (YOLO_LOSS_BAD_BOX: it now covers a ZERO size too, because the log of the size is taken), one
 *             whose class_idx is outside [0, C) (YOLO_LOSS_BAD_CLASS).  A count outside [0, max_gt] is clamped (YOLO_LOSS_BAD_COUNT).
 * Assignment. Per valid truth, in float64: the best anchor over ALL anchors of all scales, scales in head order and anchors in index
 *             order, by eval_iou(0, 0, w * w_s, h * h_s, 0, 0, aw, ah) (the evaluation's IoU, net/base.py:180-192); the FIRST anchor to
 *             reach the largest value wins (strict `<` replacement from -1).  The truth's slot is that scale, cell
 *             (floor(y * h_s), floor(x * w_s)) and that anchor.  When several truths of an image claim one slot the LAST in list order owns
 *             it (Darknet overwrites the box and objectness deltas in list order); the others count in n_truths, not in n_assigned.
 * Targets of a winner row, float64, rounded ONCE to float32: tx = x * w_s - c, ty = y * h_s - r, tw = log(w * w_s / aw),
 *             th = log(h * h_s / ah), m = 2 - w * h.
 * Terms.      float32, every operation rounded on its own, sp(t) = fmaxf(t, 0) + log1pf(expf(-fabsf(t))), expf and log1pf CORRECTLY
 *             rounded (evaluated in float64 and rounded once: a term does not depend on the float32 library that evaluates it):
 *               winner row:      xy = m * (sp(t0) - tx * t0 + sp(t1) - ty * t1)      (added left to right)
 *                                wh = m * 0.5 * ((t2 - tw)^2 + (t3 - th)^2)
 *                                obj = sp(t4) - t4
 *                                cls = sum_k (k == class ? sp(t[5 + k]) - t[5 + k] : sp(t[5 + k]))      (the bracket is a selection)
 *               every other row: noobj = sp(t4), UNLESS the row is ignored; an ignored row forms no term at all.
 * Ignore test. The row's box in float32, every operation rounded on its own: bx = (sigmoid(t0) + c) / w_s, by = (sigmoid(t1) + r) / h_s,
 *             bw = expf(t2) * float(aw) / w_s, bh = expf(t3) * float(ah) / h_s, with the sigmoid 1 / (1 + expf(-t)) of the decode (the
 *             decode itself keeps the size in float64; this is a restatement, the decode is untouched).  Widened to float64;
 *             best = max over the image's VALID truths of eval_iou(box, truth) in normalised units; ignored iff best > ignore_thresh.
 *             The comparison is strict, a NaN compares false, an image without truths ignores nothing.  Only rows that are not winners
 *             are tested.
 * Totals.     loss_xy = S xy / B, loss_wh = S wh / B, loss_obj = S obj / B, loss_noobj = S noobj / B, loss_class = S cls / B,
 *             loss = the five added in this order.  yolo_loss_image / yolo_loss_result as for YOLOv2: n_assigned counts winner rows.
 * Gradient.   G = d loss / d logits, float32 [B][R][5 + C], EVERY element written by every call; float32, every operation rounded on its
 *             own, s(t) = 1 / (1 + expf(-t)) with the correctly rounded expf of the terms:
 *               winner row:               G0 = m * (s(t0) - tx) / B, G1 = m * (s(t1) - ty) / B, G2 = m * (t2 - tw) / B, G3 = m * (t3 - th) / B,
 *                                         G4 = (s(t4) - 1) / B, G[5 + k] = (s(t[5 + k]) - [k == class]) / B
 *               not a winner, not ignored: G4 = s(t4) / B, all else +0 exactly
 *               ignored:                  the whole row +0 exactly
 *             This is -1 / B times Darknet's `delta`, so an optimizer fed with G takes Darknet's step.
 * Three DELIBERATE DIFFERENCES from Darknet:
 *   (a) the number returned is the function whose gradient G is (cross-entropies and half squares), not Darknet's printed
 *       mag_array(delta)^2;
 *   (b) the truth_thresh branch is not built: it never fires at the cfgs' value 1;
 *   (c) one truth per slot: Darknet's partial class update when a slot is claimed twice is not kept.
 * Sums.       Every float32 term is widened to float64 and added in a FIXED order: a thread's rows ascending (the class terms of a wave's
 *             winner rows: lanes striding over the classes, a butterfly over the lanes), the lane tree, the waves in index order, the parts
 *             of an image in index order, the images in index order.  A part is a constant number of rows (1024).  No floating-point
 *             atomics: the same bits on every call and every device. */
/* R and the number of partial records an image is summed through -- a function of the head alone, never of the device, because it fixes
 * the summation order.  YOLO_ERR_ARG as below for a bad head. */
int yolo_v3_loss_rows(const yolo_head_desc *head, int64_t *rows_per_image, int32_t *parts_per_image);
/* The standalone entry.  parts_dev: yolo_loss_image [batch][parts], caller-owned scratch; images_dev [batch]; assign_dev int32 [batch][R],
 * REQUIRED and wholly written by every call: a value >= 0 is the index of the truth that owns the row, -1 none, -2 ignored -- the complete
 * description the gradient kernel needs.  Three kernels (one workgroup per image; parts x images; one workgroup), enqueued on `stream`
 * with no host synchronisation.  YOLO_ERR_ARG, with a message that names the entry, for a null pointer, batch < 1, max_gt outside
 * 1..YOLO_EVAL_MAX_GT, ignore_thresh outside (0, 1], a head that is not version 3 ("the head must be version 3"), n_scales or n_classes
 * out of range, a scale with h, w or n_anchors < 1, or an image of 2^31 or more logits. */
int yolo_v3_loss(const yolo_head_desc *head, const float *logits_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                 double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev,
                 void *stream);
/* Runs the kernels of yolo_v3_loss exactly as yolo_v3_loss does -- parts, images, result and assign hold the same bytes -- then the
 * gradient kernel (a lane per element, no LDS, no atomics).  grad_dev: batch * R * (5 + C) floats that do not overlap logits_dev;
 * YOLO_ERR_ARG also for a NULL grad_dev and for grad_dev == logits_dev. */
int yolo_v3_loss_grad(const yolo_head_desc *head, const float *logits_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                      double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev,
                      yolo_loss_result *result_dev, float *grad_dev, void *stream);
/* One enqueue for a validation batch: a DENSE forward pass into the workspace logits, as yolo_net_loss does it, then the kernels of
 * yolo_v3_loss on them with the net's head: bit-identical to yolo_net_forward[_u8] followed by yolo_v3_loss.  Checks and messages as
 * yolo_net_forward plus those of yolo_v3_loss; a net whose head was never set is told so first (YOLO_ERR_STATE). */
int yolo_net_loss_v3(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                     double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev,
                     yolo_loss_result *result_dev, void *stream);
int yolo_net_loss_v3_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                        double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev,
                        yolo_loss_result *result_dev, void *stream);

/* ---- Training the detection layer on the device (added within ABI 7: new exports, the yolo_wgrad_plan and yolo_tensor_view PODs only) ------
 * The detection layer is the last conv of every YOLOv2 network here (net/v2.py:52-56): 1 x 1, stride 1, linear, with bias and no batch
 * norm, so its folded weights are its raw weights.  The entries below are its backward pass with respect to kernel and bias, the update
 * AdamOptimizer.minimize (net/v2.py:205) applies to them, and one enqueue for a whole step of net/yolo.py:161-173 on that layer.
 * Two DELIBERATE DIFFERENCES from the reference's training:
 *   (a) only the last conv's kernel and bias receive updates; the reference's minimize() updates every variable of the graph;
 *   (b) the backbone's batch norms run on their stored statistics (the inference pass); the reference builds its training graph with
 *       is_training = True, normalises with batch statistics and updates the moving averages.
 * What a fine-tune of a pretrained, frozen backbone does.  The step entries of THIS section stop at the last conv's kernel and bias.  The
 * input gradient dX of the last conv and the weight gradient of the 3 x 3 conv in front of it are yolo_conv1x1_dgrad and yolo_conv3x3_wgrad
 * ("The data gradient of the detection layer and the weight gradient of a 3 x 3 conv" below); yolo_net_train_tail_step ("Training the tail
 * of a YOLOv2 net") runs a step on both layers.  Everything in front of that block is not here.
 *
 * Weight gradient.  dW[o][c] = S_p G[p][o] * X[p][c] and db[o] = S_p G[p][o], p over the P = batch * positions_per_image positions.
 *   G   float32 [P][cout], dense: the gradient in the logits' layout (yolo_v2_loss_grad).
 *   X   the conv's input, a strided NHWC view: element (image n, position q, channel c) at n * image_stride + q * ld + coff + c from
 *       x_dev, fp16 (YOLO_DTYPE_F16) or float32 (YOLO_DTYPE_F32).  cin % 8 == 0 (YOLO_ERR_ARG otherwise).
 *   Arithmetic: X is widened to float32 (exact); products and sums on the float32-input matrix cores (v_mfma_f32_32x32x2_f32: every
 *   product rounded once, float32 accumulators); nothing is narrowed to fp16 or bf16.  The positions are split into n_chunks chunks of
 *   positions_per_chunk; a workgroup adds its chunk in ascending position order into a float32 slab of the caller's scratch, a second
 *   kernel adds the slabs in chunk order.  No floating-point atomics: two calls return the same bits.  Every element of dW and db is
 *   written by every call, and nothing depends on what scratch, dW or db held before.  Against exact arithmetic, per element,
 *   |dW - exact| <= (P + 2) 2^-24 S_p |G[p][o]| |X[p][c]| for any split.
 * yolo_wgrad_plan: how a call with these sizes is split (a host-side query: the sizing call for the scratch, and the hook the tests size
 * their cases from -- a changed split shows there).  tiles_cout x tiles_cin tiles of tile_cout x tile_cin elements of dW, each walked
 * tile_positions positions at a time; chunk k holds the positions [k * positions_per_chunk, min(P, (k + 1) * positions_per_chunk));
 * scratch_bytes = n_chunks * cout * (cin + 1) * 4.  P is 1 .. 2^30 and cout * (cin + 1) fits 31 bits (YOLO_ERR_ARG otherwise). */
struct yolo_wgrad_plan {
    int32_t tile_cout, tile_cin, tile_positions;
    int32_t tiles_cout, tiles_cin;
    int32_t positions_per_chunk, n_chunks, pad_;
    uint64_t scratch_bytes;
};
int yolo_wgrad_plan(int64_t P, int cin, int cout, int x_dtype, struct yolo_wgrad_plan *out);
/* The standalone entry, as yolo_v2_loss is for the loss: dw_dev float32 [cout][cin], db_dev float32 [cout], scratch_dev at least
 * yolo_wgrad_plan's scratch_bytes.  Two kernels, enqueued on `stream` with no host synchronisation.  YOLO_ERR_ARG for a null pointer, a
 * dtype that is not F16 / F32, cin % 8 != 0, a view whose channels do not fit ld or whose images overlap, a scratch that is too small. */
int yolo_conv1x1_wgrad(const void *x_dev, int x_dtype, int ld, int coff, int64_t image_stride, int positions_per_image, int batch, int cin,
                       const float *g_dev, int cout, float *dw_dev, float *db_dev, void *scratch_dev, size_t scratch_bytes, void *stream);

/* tf.train.AdamOptimizer's update (net/v2.py:205; its defaults: beta1 = 0.9, beta2 = 0.999, eps = 1e-8) of n_w weights and n_b biases
 * with their moments, in place, every operation float32 and rounded on its own, IEEE division and square root:
 *     m = beta1 * m + (1 - beta1) * g       v = beta2 * v + (1 - beta2) * (g * g)       w = w - (lr_t * m) / (sqrt(v) + eps)
 * lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) for step t = 1, 2, ... is the caller's, computed in float64 and passed as one float32.
 * The standalone update, without the re-pack of yolo_net_train_head_step.  n_b may be 0 (then the bias pointers are not looked at).
 * One kernel, enqueued. */
int yolo_adam_step(float *w, float *b, float *m_w, float *v_w, float *m_b, float *v_b, const float *dw, const float *db, int64_t n_w,
                   int64_t n_b, float lr_t, float beta1, float beta2, float eps, void *stream);

/* Where the detection layer's input lives in the bound workspace after a dense forward (yolo_net_forward*, yolo_net_loss*): element
 * (n, q, c) at byte offset + (n * image_stride + q * ld + coff + c) * (2 for YOLO_DTYPE_F16, 4 for YOLO_DTYPE_F32) of the workspace,
 * q = row * w + column.  Valid until the next call on the net.  YOLO_ERR_ARG unless the last kernel of the plan is a 1 x 1 / stride 1
 * linear conv with bias that writes the logits; YOLO_ERR_STATE when the plan has fused its input away or runs the batch in several
 * stream parts (each part has its own arena: call yolo_net_set_streams(net, 1)). */
typedef struct yolo_tensor_view {
    uint64_t offset;        /* bytes from the start of the workspace to element 0 of the tensor's buffer */
    int64_t image_stride;   /* elements */
    int32_t ld, coff;       /* elements between consecutive positions; first channel inside a position */
    int32_t dtype;          /* YOLO_DTYPE_F16 | YOLO_DTYPE_F32 */
    int32_t cin, h, w;
} yolo_tensor_view;
int yolo_net_head_input(const yolo_net *net, yolo_tensor_view *out);

/* Caller-owned device state of the head training: the float32 master W [cout][cin] and b [cout], their four moment arrays, dW and db, the
 * gradient G of a full batch, the winner table, the per-image loss records and the weight-gradient scratch, every part 256-byte aligned.
 * yolo_net_head_train_bytes: its size, 0 with a message for a net that cannot train its head (a head that is not version 2, a last kernel
 * that is not the 1 x 1 conv above, several stream parts).  yolo_net_head_train_init (synchronous; weights loaded first): copies
 * head_w_host [cout][cin] -- the kernel as the Darknet stream holds it, [out][in] -- and head_b_host [cout] into the master arrays AND,
 * packed, into the net's device weights, and zeroes the moments.  yolo_net_head_train_read: synchronous copy of the master values back
 * (checkpoints, tests).  yolo_net_head_train_layout: where the parts are, as byte offsets into the state (like yolo_eval_state_layout). */
typedef struct yolo_head_train_layout {
    uint64_t w_offset, b_offset, m_w_offset, v_w_offset, m_b_offset, v_b_offset, dw_offset, db_offset;
    uint64_t grad_offset, assign_offset, images_offset, scratch_offset, scratch_bytes, total_bytes;
    int32_t cin, cout;
} yolo_head_train_layout;
int yolo_net_head_train_layout(const yolo_net *net, yolo_head_train_layout *out);
size_t yolo_net_head_train_bytes(const yolo_net *net);
int yolo_net_head_train_init(yolo_net *net, void *state_dev, size_t bytes, const float *head_w_host, const float *head_b_host);
int yolo_net_head_train_read(yolo_net *net, const void *state_dev, float *w_host, float *b_host);
/* ONE enqueue with no host synchronisation for a step of net/yolo.py:161-173 on the detection layer: a dense forward pass into the
 * workspace logits, the kernels of yolo_v2_loss_grad on them (head of yolo_net_set_head), the weight gradient on the view of
 * yolo_net_head_input, the Adam update of the master values -- which in the same pass writes the layer's packed form into the net's device
 * weights: exactly the bytes yolo_net_load_weights would have produced from the master values (an MXFP8 plan keeps its head conv fp16), so
 * the next forward runs on the updated layer with no host round trip.  result_dev receives the yolo_loss_result of the weights BEFORE the
 * update, what the reference prints per step.  Bit-identical to yolo_net_forward[_u8] -> yolo_v2_loss_grad -> yolo_conv1x1_wgrad ->
 * yolo_adam_step on the same buffers.  Checks and messages as yolo_net_loss plus those of yolo_net_head_train_bytes; a null state is
 * YOLO_ERR_ARG. */
int yolo_net_train_head_step(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                             void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream);
int yolo_net_train_head_step_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream);

/* ---- The weight gradient of the YOLOv3 head convs (added within ABI 7: new exports, the yolo_v3_wgrad_plan and yolo_v3_wgrad_view PODs) ------
 * The head convs of a YOLOv3 network are the convs in front of its [yolo] layers, one per scale: 1 x 1, stride 1, linear, with bias and no
 * batch norm, cout_s = A_s * (5 + C).  This is their backward pass with respect to kernel and bias, from the gradient G of
 * yolo_v3_loss_grad.  The entries that run a whole training step on a net: "Training the YOLOv3 head convs on a net" below.
 *
 * Definition.  For scale s with P_s = batch * h_s * w_s positions, position p = (image n, cell q = row * w_s + column):
 *       dW_s[o][c] = S_p G_s[p][o] * X_s[p][c]          db_s[o] = S_p G_s[p][o]          o = a * (5 + C) + k
 *   G_s[p][o] is element k of row row0_s + q * A_s + a of image n of G ([B][R][5 + C], rows scale by scale; row0_s = the rows of the scales
 *   in front).  X_s is the conv's input, a strided NHWC view as for yolo_conv1x1_wgrad: element (n, q, c) at n * image_stride + q * ld +
 *   coff + c from x_dev, fp16 or float32, cin % 8 == 0.
 *   The sums run over exactly those (p, o) that the assign table (assign_dev of yolo_v3_loss_grad: >= 0 winner, -1 none, -2 ignored) does
 *   NOT declare a structural zero.  What remains: k == 4 for every row; every k of a row whose table entry is >= 0.  A structural zero
 *   forms no product and is never read -- a DELIBERATE DIFFERENCE from a dense G^T X: a non-finite X at a position without a winner
 *   reaches only the objectness rows o = a * (5 + C) + 4, and what G holds in its structural zeros does not matter.  A table entry >= max_gt
 *   names no truth: its row counts as one without a winner.  The table must name a truth at most once per image (yolo_v3_loss_grad does).
 * Objectness part (k == 4).  One pass over X_s: X widened to float32 (exact), float32 products and sums on the vector ALU (six flops per
 *   two bytes of X: the matrix cores have nothing to add), column 4 of G read with 4-byte loads.  The positions of a scale are split into
 *   n_chunks chunks of positions_per_chunk; a chunk is summed in ascending position order into a float32 slab of the scratch, a second
 *   kernel adds the slabs in chunk order, reduce_tile_chunks of them staged at a time.  All scales run in one launch.
 * Winner part (k != 4).  slot[n][j] = the row truth j of image n owns, or -1, built from the table; then a workgroup per (scale, anchor,
 *   win_tile_rows elements k, win_tile_cin channels) walks the slots in order, `threads` of them at a time, compacts the winner rows of its scale and anchor in that
 *   order, and adds per element the terms G[row][k] * X[position][c], images ascending, then truth index ascending, into one float32
 *   sum.  A row of dW_s and an element of db_s without a term is +0.
 * Every element of every dW_s and db_s is written by every call; nothing depends on what scratch (slot included), dW or db held before.
 * No floating-point atomics: two calls return the same bits.  Against exact arithmetic, per element, with T <= P_s terms:
 *   |dW - exact| <= (T + 2) 2^-24 S |G| |X|.
 * yolo_v3_head_wgrad_plan (host only: the sizing call for the scratch, and the hook the tests size their cases from): cin[s] the input
 * channels of scale s.  Scale s: positions = P_s, threads_per_chunk = cin_s / channels_per_thread threads walk one chunk, chunk k holds
 * the positions [k * positions_per_chunk, min(P_s, (k + 1) * positions_per_chunk)); its slab of n_chunks * (A_s * cin_s + 8) floats lies at
 * slab_offset[s] of the scratch; the winner part runs win_workgroups[s] = A_s * ceil((5 + C) / win_tile_rows) * ceil(cin_s / win_tile_cin) workgroups.  slot
 * (int32 [batch][max_gt], reserved for max_gt = YOLO_EVAL_MAX_GT) lies at slot_offset.  Every part is 256-byte aligned.  YOLO_ERR_ARG for a
 * null pointer, a dtype that is not F16 / F32, batch < 1, a head that is not version 3 ("the head must be version 3") or otherwise
 * refused by yolo_v3_loss_rows, cin % 8 != 0, P_s above 2^30, cout_s * (cin_s + 1) beyond 31 bits. */
struct yolo_v3_wgrad_plan {
    int32_t n_scales, threads, channels_per_thread, min_chunk, win_tile_cin, win_tile_rows, reduce_tile_chunks, pad_;
    int32_t positions[YOLO_MAX_SCALES], positions_per_chunk[YOLO_MAX_SCALES], n_chunks[YOLO_MAX_SCALES], threads_per_chunk[YOLO_MAX_SCALES];
    int32_t obj_workgroups[YOLO_MAX_SCALES], win_workgroups[YOLO_MAX_SCALES];
    uint64_t slab_offset[YOLO_MAX_SCALES], slab_bytes[YOLO_MAX_SCALES];
    uint64_t slot_offset, slot_bytes, scratch_bytes;
};
int yolo_v3_head_wgrad_plan(const yolo_head_desc *head, const int32_t *cin, int batch, int x_dtype, struct yolo_v3_wgrad_plan *out);
/* The input of one head conv: a device pointer and the view's strides in elements (yolo_tensor_view with a pointer for the offset). */
struct yolo_v3_wgrad_view {
    const void *x_dev;
    int64_t image_stride;
    int32_t ld, coff;
    int32_t dtype;          /* YOLO_DTYPE_F16 | YOLO_DTYPE_F32 */
    int32_t cin;
};
/* The standalone entry.  views[n_scales] in head order; g_dev float32 [batch][R][5 + C] and assign_dev int32 [batch][R] as
 * yolo_v3_loss_grad left them; dw_dev[s] float32 [cout_s][cin_s], db_dev[s] float32 [cout_s]; scratch_dev 16-byte aligned, at least
 * yolo_v3_head_wgrad_plan's scratch_bytes.  Four kernels, enqueued on `stream` with no host synchronisation.  YOLO_ERR_ARG, with a
 * message that names the entry (and the scale), for what the plan refuses and for a null pointer, max_gt outside 1..YOLO_EVAL_MAX_GT, a
 * view whose channels do not fit ld or whose images overlap, a pointer not aligned to its element type, a scratch that is too small. */
int yolo_v3_head_wgrad(const yolo_head_desc *head, const struct yolo_v3_wgrad_view *views, int batch, const float *g_dev,
                       const int32_t *assign_dev, int max_gt, float *const *dw_dev, float *const *db_dev, void *scratch_dev,
                       size_t scratch_bytes, void *stream);

/* ---- Training the YOLOv3 head convs on a net (added within ABI 7: new exports, the yolo_head_train_v3_layout POD only) ------
 * What the entries of "Training the detection layer" are for a YOLOv2 network, for the head convs of a version 3 network (YOLOv3,
 * YOLOv3-SPP, YOLOv3-tiny): every head conv's kernel and bias receive Adam updates from the YOLOv3 loss, everything in front of them is
 * frozen and its batch norms run on their stored statistics.  The older entries keep refusing a version 3 network.  The optimiser is
 * the reference's Adam (net/v2.py:205), not Darknet's SGD with momentum.
 *
 * yolo_net_head_inputs_v3: where the input of every head conv lives in the bound workspace after a dense forward, in head order
 * (yolo_tensor_view as for yolo_net_head_input); *n receives the number of scales.  A head conv is a conv kernel of the plan that writes
 * the logits: 1 x 1, stride 1, linear, with bias and no batch norm.  The entry VERIFIES from the plan's buffer lifetimes that each input
 * is still intact behind the last kernel of the pass: no kernel behind the head conv writes its buffer, and no buffer that shares bytes
 * with it is alive later (the planner keeps the buffers of a branch tail to the end of the pass, and the last head is the last kernel).
 * YOLO_ERR_STATE with a message that names the scale when the plan reuses a head's input; the refusals of yolo_net_head_input for a net
 * that runs several stream parts ("call yolo_net_set_streams(net, 1)"), a fused-away input or cin % 8 != 0; YOLO_ERR_ARG for a net whose
 * head is not version 3 or whose head convs do not match its head.
 *
 * State (caller-owned device memory, every part 256-byte aligned): per scale the float32 master W_s [cout_s][cin_s] and b_s, their four
 * moment arrays, dW_s and db_s; one G for a full batch; the assign table, the part and image records of the v3 loss; the scratch of
 * yolo_v3_head_wgrad (slot inside it), sized for the largest split of any batch up to max_batch.  bias_src[s]: the position, in floats,
 * of conv s's bias in the Darknet stream -- its cout_s biases stand there, its cout_s * cin_s kernel values behind them -- so that a
 * caller can cut the heads out of a .weights stream and put them back.  _init (synchronous; weights loaded first) copies w_host[s]
 * [cout_s][cin_s] and b_host[s] into the masters AND, packed, into the net's device weights, and zeroes the moments; _read copies the
 * masters back (synchronous). */
typedef struct yolo_head_train_v3_layout {
    int32_t n_scales, pad_;
    int32_t cin[YOLO_MAX_SCALES], cout[YOLO_MAX_SCALES];
    uint64_t w_offset[YOLO_MAX_SCALES], b_offset[YOLO_MAX_SCALES], m_w_offset[YOLO_MAX_SCALES], v_w_offset[YOLO_MAX_SCALES];
    uint64_t m_b_offset[YOLO_MAX_SCALES], v_b_offset[YOLO_MAX_SCALES], dw_offset[YOLO_MAX_SCALES], db_offset[YOLO_MAX_SCALES];
    uint64_t bias_src[YOLO_MAX_SCALES];
    uint64_t grad_offset, assign_offset, parts_offset, images_offset, scratch_offset, scratch_bytes, total_bytes;
} yolo_head_train_v3_layout;
int yolo_net_head_inputs_v3(const yolo_net *net, yolo_tensor_view *out, int32_t *n);
int yolo_net_head_train_v3_layout(const yolo_net *net, yolo_head_train_v3_layout *out);
size_t yolo_net_head_train_v3_bytes(const yolo_net *net);
int yolo_net_head_train_v3_init(yolo_net *net, void *state_dev, size_t bytes, const float *const *w_host, const float *const *b_host);
int yolo_net_head_train_v3_read(yolo_net *net, const void *state_dev, float *const *w_host, float *const *b_host);
/* ONE enqueue with no host synchronisation for a training step on the head convs: a dense forward pass into the workspace logits, the
 * kernels of yolo_v3_loss_grad on them, yolo_v3_head_wgrad on the views of yolo_net_head_inputs_v3, and per scale the Adam update of
 * yolo_adam_step (beta1 = 0.9, beta2 = 0.999, eps = 1e-8) on the masters -- which in the same pass writes the conv's packed form into the
 * net's device weights, exactly the bytes yolo_net_load_weights would have produced from the master values (an MXFP8 plan keeps its head
 * convs fp16).  result_dev receives the yolo_loss_result of the weights BEFORE the update.  Bit-identical to yolo_net_forward[_u8] ->
 * yolo_v3_loss_grad -> yolo_v3_head_wgrad -> yolo_adam_step per scale on the same buffers.  Checks and messages as yolo_net_loss_v3 plus
 * those of yolo_net_head_inputs_v3; a null state is YOLO_ERR_ARG ("null state"). */
int yolo_net_train_head_step_v3(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream);
int yolo_net_train_head_step_v3_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev,
                                   int max_gt, double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream);

/* ---- The data gradient of the detection layer and the weight gradient of a 3 x 3 conv (added within ABI 7: new exports, the
 *      yolo_conv3x3_wgrad_plan POD only) ------
 * The two operators every backward pass behind the detection layer is built from, as standalone device ops.  The block they are written
 * for is the 3 x 3 / batch norm / leaky conv in front of the detection layer of a YOLOv2 network (net/v2.py:62):
 *       u = conv3x3_same(W3, X3);   z = s (.) u + b';   Y = leaky_0.1(z);   L = W Y + b        s[o] = gamma / sqrt(var + 1e-5)
 * with b'[o] = beta - mean * s (weights.cpp: fold_batch_norm) and G = dloss / dL from yolo_v2_loss_grad.  DELIBERATE DIFFERENCES from the
 * reference's training, beside (a) and (b) of head training above: with these operators only the block's kernel and beta and the head's
 * kernel and bias can receive gradients; gamma and the moving statistics stay frozen (the block runs on its stored statistics, (b)).
 * yolo_net_train_tail_step ("Training the tail of a YOLOv2 net" below) runs them on a net.
 *
 * Data gradient, with the activation's backward fused.  For p over the P = batch * positions_per_image positions and c < cin:
 *       D[p][c] = (S_o G[p][o] * W[o][c]) * (Y[p][c] > 0 ? 1 : slope)              o ascending from 0
 *   G   float32 [P][cout], dense.  cout is any value >= 1; the kernel pads the reduction with zeros and never reads past a row.
 *   W   float32 [cout][cin], dense: the float32 MASTER kernel of the head, NOT the fp16 packed copy the forward pass reads -- nothing
 *       is narrowed, as in yolo_conv1x1_wgrad.  cin % 8 == 0.
 *   Y   the block's stored output, a strided NHWC view as for yolo_conv1x1_wgrad (element (n, q, c) at n * image_stride + q * ld + coff +
 *       c from y_dev), fp16 or float32; the branch is decided by the STORED value: +0, -0, negatives (and NaN) take slope.  y_dev may
 *       be null: then the factor is 1 everywhere and y_dtype, ld, coff and image_stride are not looked at.
 *   Arithmetic: products and sums on the float32-input matrix cores (v_mfma_f32_32x32x2_f32: a float32 fmaf chain from +0, o ascending);
 *   the factor is ONE float32 multiply, rounded once (a multiply by 1 is exact).  D is float32, dense [P][cin]; every element is written
 *   (16-byte stores), nothing depends on what D held.  One kernel, enqueued on `stream` with no host synchronisation.
 *   YOLO_ERR_ARG for a null g / w / d, cin % 8 != 0, cout < 1, P outside 1 .. 2^30, cout * cin past 31 bits, w_dev or d_dev not 16-byte
 *   aligned, a Y view whose channels do not fit ld or whose images overlap, a y_dtype that is not F16 / F32. */
int yolo_conv1x1_dgrad(const float *g_dev, int cout, const float *w_dev, int cin, const void *y_dev, int y_dtype, int ld, int coff,
                       int64_t image_stride, int positions_per_image, int batch, float slope, float *d_dev, void *stream);

/* 3 x 3 weight gradient, stride 1, SAME zero padding.  For position p = (image n, row r, column x) of an h x w map, tap t = 3 ky + kx:
 *       R[o][t][c] = S_p D[p][o] * X3[n, r + ky - 1, x + kx - 1][c]        db[o] = S_p D[p][o]        dW3[o][t][c] = s32[o] * R[o][t][c]
 *   A tap that falls outside the image contributes nothing and is never read.  The scale is ONE float32 multiply, applied in the reduce;
 *   with a null scale_dev dW3 = R.  dbeta = db (never scaled).
 *   D    float32 [P][cout], dense, P = batch * h * w (yolo_conv1x1_dgrad's output for the block above).
 *   X3   the conv's input, a strided NHWC view as for yolo_conv1x1_wgrad with positions_per_image = h * w, fp16 or float32; cin % 8 == 0.
 *   dW3  float32 [cout][9][cin]: the K order of the packed rows.  The conversion to and from the Darknet stream's [out][in][kh][kw] is the
 *        caller's.  db float32 [cout].
 *   Arithmetic as yolo_conv1x1_wgrad: X3 widened to float32 (exact), products and sums on the float32-input matrix cores, positions
 *   ascending inside a chunk (a masked tap enters as a product with +0), chunks added in chunk order by a second kernel.  No
 *   floating-point atomics: two calls return the same bits.  Every element of dW3 and db is written by every call; nothing depends on what
 *   scratch, dW3 or db held before.  Against exact arithmetic, per element, |dW3 - exact| <= (P + 3) 2^-24 |s| S_p |D| |X3| for any split.
 * yolo_conv3x3_wgrad_plan (host only: the sizing call for the scratch, and the hook the tests size their cases from -- a changed split
 * shows there): tiles_cout x tiles_cin workgroup tiles of tile_cout couts x (9 taps x tile_cin channels) of dW3; a workgroup walks its
 * chunk tile_positions positions at a time and holds, per stage, the halo_rows = tile_positions + 2 w + 2 positions
 * [first - w - 1, first + tile_positions + w + 1) of its tile_cin channels in LDS ONCE, from which all nine taps are served.  Chunk k holds the
 * positions [k * positions_per_chunk, min(P, (k + 1) * positions_per_chunk)); scratch_bytes = n_chunks * cout * (9 cin + 1) * 4.
 * YOLO_ERR_ARG for h, w, batch < 1, w > 80 (the halo of a wider map does not fit LDS), P past 2^30, cin % 8 != 0, cout < 1,
 * cout * (9 cin + 1) past 31 bits, a dtype that is not F16 / F32. */
struct yolo_conv3x3_wgrad_plan {
    int32_t tile_cout, tile_cin, tile_positions;
    int32_t tiles_cout, tiles_cin;
    int32_t positions_per_chunk, n_chunks, halo_rows;
    uint64_t scratch_bytes;
};
int yolo_conv3x3_wgrad_plan(int h, int w, int batch, int cin, int cout, int x_dtype, struct yolo_conv3x3_wgrad_plan *out);
/* scratch_dev at least yolo_conv3x3_wgrad_plan's scratch_bytes; scale_dev float32 [cout] or null.  Two kernels, enqueued on `stream` with
 * no host synchronisation.  YOLO_ERR_ARG for what the plan refuses, a null pointer (scale_dev excepted), a pointer not aligned to its
 * element type, a view whose channels do not fit ld or whose images overlap, a scratch that is too small. */
int yolo_conv3x3_wgrad(const void *x_dev, int x_dtype, int ld, int coff, int64_t image_stride, int h, int w, int batch, int cin,
                       const float *d_dev, int cout, const float *scale_dev, float *dw_dev, float *db_dev, void *scratch_dev,
                       size_t scratch_bytes, void *stream);

/* ---- The 3 x 3 weight gradient on the fp16 matrix cores (added within ABI 7: new exports, the yolo_conv3x3_wgrad_f16_plan POD only) ------
 * yolo_conv3x3_wgrad with ONE operand narrowed, D; the arguments and their meaning are yolo_conv3x3_wgrad's: stride 1, SAME padding, a
 * strided NHWC view of X3, dW3 [cout][9][cin], db [cout], scale_dev or null; a tap outside the image contributes nothing and is never read.
 *   X3   must be YOLO_DTYPE_F16 and is used as stored (a float32 view is YOLO_ERR_ARG: that is yolo_conv3x3_wgrad's).
 *   k    the scale of the call.  m = max |D[p][o]| over the whole call; k = 0 when m is 0, Inf or NaN, else
 *        k = clamp(14 - floor(log2 m), -126, 126): the largest scaled magnitude lies in [2^14, 2^15) and cannot overflow fp16.  m is found on
 *        the device as an INTEGER maximum of the bit patterns of |D| (order-independent, no floating-point atomic; NaN patterns sort above
 *        Inf); no host synchronisation.
 *   D16  D16[p][o] = fp16_rne(D[p][o] * 2^k): one IEEE round-to-nearest-even conversion with gradual underflow of the exactly scaled value
 *        (numpy.astype(float16) of it).  Narrowed while the main kernel stages D into LDS; there is no D16 buffer.
 *   R16  R16[o][t][c] = S_p D16[p][o] * X3[p + tap t][c] on the fp16 matrix cores (v_mfma_f32_32x32x16_f16) with float32 accumulation: every
 *        fp16 x fp16 product is exact in float32, subnormal fp16 operands count; positions ascend inside a chunk, chunks are added in chunk
 *        order by the reduce kernel, no floating-point atomics.
 *   dW3  dW3 = s32[o] * (2^-k * R16): the power-of-two multiply first (exact in the normal range), then the s32 multiply, rounded once.
 *   db   db[o] = S_p D[p][o] from the UN-NARROWED float32 D (db_groups groups of db_positions positions; inside a group interleaved partial
 *        sums, positions ascending, added in a fixed order; the groups in group order): |db - exact| <= (P + 3) 2^-24 S_p |D|, as
 *        yolo_conv3x3_wgrad.
 *   Every element of dW3 and db is written by every call; nothing depends on what dW3, db or the scratch held (the call initialises the m / k
 *   record itself); two calls return the same bits.
 *   Error, per element, for any split.  With dW64 = s32[o] 2^-k S_p D16 X3 over the NARROWED operands in float64:
 *        |dW3 - dW64| <= (P + 4) 2^-24 |s32[o]| 2^-k S_p |D16| |X3|
 *   and against the un-narrowed dWexact = s32[o] S_p D X3 (float64) add the rounding of the narrowing:
 *        |dW3 - dWexact| <= (P + 4) 2^-24 |s32[o]| 2^-k S_p |D16| |X3|  +  |s32[o]| S_p (2^-11 |D| + 2^-25 2^-k) |X3|
 *   (below fp16's normal range 2^-25 2^-k is the absolute rounding of the narrowing).
 *   The mode helps every shape measured (profiles/wgrad_f16.json; README, "Training").
 * yolo_conv3x3_wgrad_f16_plan (host only): as yolo_conv3x3_wgrad_plan, with tile_positions = 64 and halo_rows = 64 + 2 w + 2 rows of 16-bit
 * elements.  scratch_bytes: the slabs, n_chunks * cout * (9 cin + 1) * 4 bytes, rounded up to 256; then, at record_offset from scratch_dev,
 * 256 bytes that start with the record -- uint32 (the bits of m) and int32 (k), written by every call; then the partial sums of db,
 * db_groups * cout * 4 bytes, rounded up to 256.  Refusals as yolo_conv3x3_wgrad_plan,
 * except that w may be up to 96: the 16-bit halo is half the size, and its rows are padded by half (64 elements in 192 bytes) for the
 * transposed LDS reads; yolo_conv3x3_wgrad keeps its 80. */
struct yolo_conv3x3_wgrad_f16_plan {
    int32_t tile_cout, tile_cin, tile_positions;
    int32_t tiles_cout, tiles_cin;
    int32_t positions_per_chunk, n_chunks, halo_rows;
    int32_t db_groups, db_positions;
    uint64_t record_offset;
    uint64_t scratch_bytes;
};
int yolo_conv3x3_wgrad_f16_plan(int h, int w, int batch, int cin, int cout, struct yolo_conv3x3_wgrad_f16_plan *out);
/* Four launches (the record's clear, the maximum and db, the products, the reduce), enqueued on `stream` with no host synchronisation.
 * YOLO_ERR_ARG as yolo_conv3x3_wgrad, and for an x_dtype that is not YOLO_DTYPE_F16. */
int yolo_conv3x3_wgrad_f16(const void *x_dev, int x_dtype, int ld, int coff, int64_t image_stride, int h, int w, int batch, int cin,
                           const float *d_dev, int cout, const float *scale_dev, float *dw_dev, float *db_dev, void *scratch_dev,
                           size_t scratch_bytes, void *stream);

/* ---- Training the tail of a YOLOv2 net: the last 3 x 3 block and the detection layer (added within ABI 7: new exports, the
 *      yolo_tail_train_layout POD only) ------
 * The tail is the 3 x 3 / stride 1 / batch norm / leaky conv whose output the detection layer reads (net/v2.py:62 in the full network, the
 * second 1024-wide conv in tiny-YOLOv2) plus the detection layer.  What is updated: the block's kernel W3 and beta, the head's kernel and
 * bias.  gamma and the moving statistics stay frozen; the block, like the backbone, runs on its stored statistics (difference (b) above).
 *
 * yolo_net_tail_inputs: where the block's input X3 and the head's input Y (the view of yolo_net_head_input) live in the bound workspace
 * after a dense forward.  Succeeds only when the last kernel is the detection layer (the checks of yolo_net_head_input) and the kernel that
 * writes its input is a 3 x 3 / stride 1 conv with batch norm and leaky ReLU that writes exactly that view; YOLO_ERR_ARG, naming what is in
 * the way, for a network that has no such block (a v3 net, a 1 x 1 or stride-2 conv, a conv with a residual, an input that no single conv
 * writes); YOLO_ERR_STATE for a plan that runs the block as an MXFP8 conv, fused it with a neighbour (pool / reorg / upsample in its
 * epilogue, a back-to-back 1 x 1, the stem), keeps its input outside the workspace or reuses that input's bytes behind it, or runs the
 * batch in several stream parts. */
int yolo_net_tail_inputs(const yolo_net *net, yolo_tensor_view *block_in, yolo_tensor_view *head_in);

/* Caller-owned device state of the tail training, every part 256-byte aligned: the head's parts as in yolo_head_train_layout; for the
 * block the float32 master W3 [cout3][9][cin3] (tap t = 3 ky + kx: the K order of the packed rows) and beta [cout3], their four moment
 * arrays, dW3 and dbeta; scale64 (float64 [cout3] = gamma / sqrt(var + 1e-5), computed ONCE on the host at init exactly as the weight
 * loader folds batch norm), scale32 (its float32 rounding: the s32 of yolo_conv3x3_wgrad) and mean; D [max_batch * h * w][cout3]; G, the
 * winner table, the per-image records; one scratch that the two weight gradients use one after the other.  cin == cout3.
 * block_src / head_src: the first float of the block (its beta) and of the head (its bias) in the Darknet stream.
 * yolo_net_tail_train_init (synchronous; weights loaded first): block_host is the block's piece of the Darknet stream -- beta, gamma,
 * moving mean, moving variance [cout3 each], then the kernel [out][in][kh][kw] --, head_w_host [cout][cin] and head_b_host [cout] the
 * head's.  Converts the kernel to [o][t][c], fills the masters, zeroes the moments and writes both layers' packed forms into the net's
 * device weights.  yolo_net_tail_train_read: synchronous copy of the master values back, the block's kernel converted to
 * [out][in][kh][kw] again. */
typedef struct yolo_tail_train_layout {
    uint64_t w_offset, b_offset, m_w_offset, v_w_offset, m_b_offset, v_b_offset, dw_offset, db_offset;
    uint64_t w3_offset, beta_offset, m_w3_offset, v_w3_offset, m_beta_offset, v_beta_offset, dw3_offset, dbeta_offset;
    uint64_t scale64_offset, scale32_offset, mean_offset;
    uint64_t d_offset, grad_offset, assign_offset, images_offset, scratch_offset, scratch_bytes, total_bytes;
    uint64_t block_src, head_src;
    int32_t cin, cout, cin3, cout3;
} yolo_tail_train_layout;
int yolo_net_tail_train_layout(const yolo_net *net, yolo_tail_train_layout *out);
size_t yolo_net_tail_train_bytes(const yolo_net *net);
int yolo_net_tail_train_init(yolo_net *net, void *state_dev, size_t bytes, const float *block_host, const float *head_w_host,
                             const float *head_b_host);
int yolo_net_tail_train_read(yolo_net *net, const void *state_dev, float *block_kernel_host, float *beta_host, float *w_host, float *b_host);
/* ONE enqueue with no host synchronisation for a step of net/yolo.py:161-173 on the tail, in this order: a dense forward pass; the kernels
 * of yolo_v2_loss_grad; the head's weight gradient (yolo_conv1x1_wgrad on Y); yolo_conv1x1_dgrad from the head's master kernel BEFORE its
 * update, with Y and slope 0.1; yolo_conv3x3_wgrad on X3 with scale32; the Adam update and re-pack of the head (as
 * yolo_net_train_head_step); the Adam update of W3 and beta, which in the same pass writes the block's packed form,
 *       pack[o][t * cin3 + c] = T((double)W3[o][t][c] * scale64[o])          b'[o] = (float)((double)beta[o] - (double)mean[o] * scale64[o])
 * (T the plan's weight type, ONE rounding from the float64 product): exactly the bytes yolo_net_load_weights produces from the stream
 * rebuilt with yolo_net_tail_train_read.  (The loader writes T((float)(product)); for T = fp16 its host compiler folds the two truncations
 * into one, so its bytes are the once-rounded ones -- rounding to float32 first differs in about one element of 30 000, which the tests
 * found; for T = float32 the two forms are the same.)  result_dev receives the yolo_loss_result of the weights BEFORE the update.  Bit-identical to the standalone
 * entries called one after the other on the same buffers (yolo_adam_step for both updates).  Checks and messages as
 * yolo_net_train_head_step plus those of yolo_net_tail_inputs. */
int yolo_net_train_tail_step(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                             void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream);
int yolo_net_train_tail_step_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream);

/* ---- The sparse data gradient of one YOLOv3 head conv (added within ABI 7: new exports, the yolo_v3_dgrad_plan POD only) ------
 * The backward pass of the head conv of scale `scale` of a version 3 head with respect to its input, times the derivative of the leaky
 * ReLU in front of it -- what yolo_conv1x1_dgrad is for the detection layer of a YOLOv2 network, from the gradient G of
 * yolo_v3_loss_grad read IN PLACE: nothing is gathered.  It is the operator a backward pass into the 3 x 3 block behind a YOLOv3 head
 * starts with (its output D is the D of yolo_conv3x3_wgrad).
 *
 * Definition.  For scale s with P_s = batch * h_s * w_s positions, position p = (image n, cell q = row * w_s + column), c < cin:
 *       D_s[p][c] = (S_o G_s[p][o] * W_s[o][c]) * (Y_s[p][c] > 0 ? 1 : slope)          o = a * (5 + C) + k
 *   G_s[p][o] is element k of row row0_s + q * A_s + a of image n of G ([B][R][5 + C], as for yolo_v3_head_wgrad), assign_dev the table of
 *   yolo_v3_loss_grad.  The sum runs over exactly those (a, k) the table does NOT declare a structural zero, by the rule of
 *   yolo_v3_head_wgrad: k == 4 for every row; every k of a row whose entry is in [0, max_gt); an entry >= max_gt counts as no winner.  A
 *   structural zero forms no product and is never read: a NaN there changes no bit of D.
 *   W   float32 [cout_s][cin], dense: the float32 MASTER kernel of the head conv, NOT the packed copy.  cin % 8 == 0.
 *   Y   the stored output of the block in front, a strided NHWC view as for yolo_conv1x1_dgrad, fp16 or float32; the STORED value
 *       decides the branch: +0, -0, negatives (and NaN) take slope.  y_dev may be null: then the factor is 1 everywhere and y_dtype, ld,
 *       coff and image_stride are not looked at.
 *   Arithmetic: ONE float32 fmaf chain per element on the vector ALU, from +0, over the remaining terms in ascending o (anchors ascend;
 *   inside a winner row k runs 0 .. 4 + C, otherwise only k == 4), then ONE float32 multiply by the factor.  D is float32, dense
 *   [P_s][cin]; every element is written by every call (16-byte stores), nothing depends on what D held.  No atomics: two calls return
 *   the same bits.  Against exact arithmetic, with T the number of terms of the position, |D - exact| <= (T + 2) 2^-24 |factor| S |G| |W|.
 *   One kernel, enqueued on `stream` with no host synchronisation.
 * Kernel shape: a thread owns channels_per_thread consecutive channels of one position; the channels are cut into tiles_cin tiles of
 *   tile_cin (the A_s objectness rows of W_s of a tile lie in lds_bytes of LDS); threads_per_position threads make a position,
 *   positions_per_round positions one round of a workgroup, which walks `rounds` rounds: the positions_per_workgroup consecutive positions
 *   from workgroup * positions_per_workgroup.  workgroups per channel tile; loops = rounds > 1.  (threads_per_position,
 *   positions_per_round and rounds are a full tile's: a last tile narrower than tile_cin takes its channels / channels_per_thread
 *   threads a position and walks the same positions in fewer rounds.)  A position with a winner row walks the
 *   5 + C rows of that anchor out of L2: with many truths per image that walk dominates.
 * yolo_v3_head_dgrad_plan (host only: the hook the tests size their cases from): YOLO_ERR_ARG for a null pointer, a head that is not
 * version 3 ("the head must be version 3") or otherwise refused by yolo_v3_loss_rows, scale outside 0 .. n_scales - 1, batch < 1,
 * cin % 8 != 0, P_s above 2^30.  yolo_v3_head_dgrad adds: a null g / assign / w / d, max_gt outside 1..YOLO_EVAL_MAX_GT, w_dev or d_dev
 * not 16-byte aligned, a Y view whose channels do not fit ld or whose images overlap, a y_dtype that is not F16 / F32.  Every message
 * names the entry. */
struct yolo_v3_dgrad_plan {
    int32_t threads, channels_per_thread, tile_cin, tiles_cin;
    int32_t threads_per_position, positions_per_round, rounds, positions_per_workgroup;
    int32_t workgroups, loops, positions, lds_bytes;
};
int yolo_v3_head_dgrad_plan(const yolo_head_desc *head, int scale, int cin, int batch, struct yolo_v3_dgrad_plan *out);
int yolo_v3_head_dgrad(const yolo_head_desc *head, int scale, const float *g_dev, const int32_t *assign_dev, int max_gt, int batch,
                       const float *w_dev, int cin, const void *y_dev, int y_dtype, int ld, int coff, int64_t image_stride, float slope,
                       float *d_dev, void *stream);

/* ---- Training the 3 x 3 blocks behind the YOLOv3 heads (added within ABI 7: new exports, the yolo_blocks_train_v3_layout POD only) ------
 * What "Training the tail of a YOLOv2 net" is for a YOLOv2 network, for every scale of a version 3 network (YOLOv3, YOLOv3-SPP,
 * YOLOv3-tiny): per scale the head conv's kernel and bias and the kernel W3 and beta of the 3 x 3 / stride 1 / batch norm / leaky conv that
 * writes the head conv's input receive Adam updates from the YOLOv3 loss.  gamma and the moving statistics stay frozen; everything in front
 * runs on its stored statistics.  yolo_net_tail_inputs keeps refusing a version 3 net.
 *
 * yolo_net_block_inputs_v3: per scale in head order, the view of the block's input X3_s and of the head conv's input Y_s in the bound
 * workspace after a dense forward; *n receives the number of scales.  Succeeds only when yolo_net_head_inputs_v3 does and, for every
 * scale, the one kernel that writes the head conv's input passes the checks of yolo_net_tail_inputs (3 x 3 / stride 1, batch norm and leaky
 * ReLU, no residual, not an MXFP8 conv, no fusion with a neighbour, writes exactly the head conv's view, its input a tensor of the
 * workspace with cin % 8 == 0 that is still intact behind the last kernel, a map at most 80 wide).  The refusal names the scale and what
 * is in the way, with the codes of yolo_net_tail_inputs.
 *
 * State (caller-owned device memory, every part 256-byte aligned): per scale the eight arrays of the head conv as in
 * yolo_head_train_v3_layout, the eight arrays of the block as in yolo_tail_train_layout (W3 [cout3][9][cin3], tap t = 3 ky + kx), scale64,
 * scale32 and mean of the block; ONE D of max_batch * max_s(h_s w_s cout3_s) floats -- the scales run one after the other on one stream --;
 * G, the assign table, the part and image records of the v3 loss; ONE scratch, the largest over the batches 1 .. max_batch of the
 * yolo_v3_head_wgrad plan and every scale's yolo_conv3x3_wgrad plan.  bias_src[s] / block_src[s]: the first float of head conv s (its bias)
 * and of block s (its beta) in the Darknet stream.
 * _init (synchronous; weights loaded first): block_host[s] is block s's piece of the Darknet stream -- beta, gamma, moving mean, moving
 * variance [cout3 each], then the kernel [out][in][kh][kw] --, w_host[s] [cout_s][cin_s] and b_host[s] the head conv's.  Fills the masters,
 * zeroes the moments and writes both convs' packed forms of every scale into the net's device weights, the heads as
 * yolo_net_head_train_v3_init, the blocks as yolo_net_tail_train_init.  _read: synchronous copy of the masters back, the blocks' kernels
 * converted to [out][in][kh][kw] again. */
typedef struct yolo_blocks_train_v3_layout {
    int32_t n_scales, pad_;
    int32_t cin[YOLO_MAX_SCALES], cout[YOLO_MAX_SCALES], cin3[YOLO_MAX_SCALES], cout3[YOLO_MAX_SCALES];
    uint64_t w_offset[YOLO_MAX_SCALES], b_offset[YOLO_MAX_SCALES], m_w_offset[YOLO_MAX_SCALES], v_w_offset[YOLO_MAX_SCALES];
    uint64_t m_b_offset[YOLO_MAX_SCALES], v_b_offset[YOLO_MAX_SCALES], dw_offset[YOLO_MAX_SCALES], db_offset[YOLO_MAX_SCALES];
    uint64_t w3_offset[YOLO_MAX_SCALES], beta_offset[YOLO_MAX_SCALES], m_w3_offset[YOLO_MAX_SCALES], v_w3_offset[YOLO_MAX_SCALES];
    uint64_t m_beta_offset[YOLO_MAX_SCALES], v_beta_offset[YOLO_MAX_SCALES], dw3_offset[YOLO_MAX_SCALES], dbeta_offset[YOLO_MAX_SCALES];
    uint64_t scale64_offset[YOLO_MAX_SCALES], scale32_offset[YOLO_MAX_SCALES], mean_offset[YOLO_MAX_SCALES];
    uint64_t bias_src[YOLO_MAX_SCALES], block_src[YOLO_MAX_SCALES];
    uint64_t d_offset, grad_offset, assign_offset, parts_offset, images_offset, scratch_offset, scratch_bytes, total_bytes;
} yolo_blocks_train_v3_layout;
int yolo_net_block_inputs_v3(const yolo_net *net, yolo_tensor_view *block_in, yolo_tensor_view *head_in, int32_t *n);
int yolo_net_blocks_train_v3_layout(const yolo_net *net, yolo_blocks_train_v3_layout *out);
size_t yolo_net_blocks_train_v3_bytes(const yolo_net *net);
int yolo_net_blocks_train_v3_init(yolo_net *net, void *state_dev, size_t bytes, const float *const *block_host, const float *const *w_host,
                                  const float *const *b_host);
int yolo_net_blocks_train_v3_read(yolo_net *net, const void *state_dev, float *const *block_kernel_host, float *const *beta_host,
                                  float *const *w_host, float *const *b_host);
/* ONE enqueue with no host synchronisation for a training step on the head convs and the blocks behind them, in this order: a dense
 * forward pass; the kernels of yolo_v3_loss_grad; yolo_v3_head_wgrad; for s ascending, yolo_v3_head_dgrad from head conv s's master kernel
 * BEFORE its update, with Y_s and slope 0.1, into D, then yolo_conv3x3_wgrad on X3_s with scale32_s; per scale the Adam update and re-pack
 * of the head conv (as yolo_net_train_head_step_v3); per scale the Adam update of W3_s and beta_s with the re-pack of the block (as
 * yolo_net_train_tail_step).  result_dev receives the yolo_loss_result of the weights BEFORE the update.  Bit-identical to the standalone
 * entries called one after the other on the same buffers.  Checks and messages as yolo_net_train_head_step_v3 plus those of
 * yolo_net_block_inputs_v3. */
int yolo_net_train_blocks_step_v3(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                  double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream);
int yolo_net_train_blocks_step_v3_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev,
                                     int max_gt, double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream);

/* ---- The fp16-operand 3 x 3 weight gradient as a mode of the tail and blocks steps (added within ABI 7: new exports only) ------
 * yolo_net_train_wgrad_f16_bytes: the largest scratch_bytes of yolo_conv3x3_wgrad_f16_plan over the net's trainable 3 x 3 blocks -- the tail
 * block of a version 2 net, every head block of a version 3 net, found with the checks of yolo_net_tail_inputs / yolo_net_block_inputs_v3 --
 * at the batches up to max_batch.  0, with yolo_last_error(), where those checks refuse, and for a plan that does not store fp16 activations.
 * yolo_net_train_set_wgrad_f16: with a buffer of at least that size, yolo_net_train_tail_step[_u8] and yolo_net_train_blocks_step_v3[_u8] run
 * yolo_conv3x3_wgrad_f16 in place of yolo_conv3x3_wgrad with extra_dev as its scratch (the buffer is the caller's and must outlive the
 * mode); everything else in the step, the state and the state layouts is unchanged, and a step is bit-identical to its parts through the
 * standalone exports with yolo_conv3x3_wgrad_f16 in that place.  extra_dev = NULL switches back: the steps are then the float32 steps, bit
 * for bit (bytes is not looked at).  YOLO_ERR_STATE for a float32 plan, saying so; YOLO_ERR_ARG for a buffer that is too small or not
 * 256-byte aligned; what the block checks refuse as they refuse it.  The mode belongs to the net and nothing but this call changes it: every
 * *_train_init*, yolo_net_load_weights, yolo_net_bind_workspace, yolo_net_set_streams and a refused yolo_net_train_set_wgrad_f16 leave it as
 * it is, the head-only steps and every call that does not train do not look at it, and a second accepted call replaces the buffer and nothing else. */
size_t yolo_net_train_wgrad_f16_bytes(const yolo_net *net);
int yolo_net_train_set_wgrad_f16(yolo_net *net, void *extra_dev, size_t bytes);

/* ---- Training augmentation on the device: flips, blur, dropout, noise, shift (added within ABI 7: new exports, one new POD) ------
 * The reference trains through an imgaug pipeline (net/base.py:15-23): Fliplr(0.5), Flipud(0.5), GaussianBlur((0, 3.0)), Dropout(0.02),
 * AdditiveGaussianNoise(scale = 0.01 * 255), AdditiveGaussianNoise(loc = 32, scale = 0.0001 * 255), Affine(translate_px x in -40 .. 40),
 * with the truth boxes carried along and remove_out_of_image().cut_out_of_image() at the end (net/base.py:100-112).  Here the same list of
 * operations in the same order, in integers, with the parameters of every image drawn on the host (net/augment.py) and one POD per image.
 * DELIBERATE DIFFERENCES from imgaug: (a) the random stream is this header's counter-based generator, not imgaug's; (b) a noise value is
 * an Irwin-Hall(4) variate -- the sum of four uniform 16-bit numbers, tails end at +-3.46 sigma -- not a true normal; (c) the blur's taps
 * are 8-bit fixed point (they add up to 256), the radius at most 9; (d) at the reference's scale the second noise step is exactly + 32;
 * (e) a truth is dropped when it lies fully outside the image (the rule below), where imgaug's remove_out_of_image has its own test.
 *
 * For an image S[h][w][3] (uint8) and its yolo_augment_image:
 *   1 flips   F[y][x] = S[flip_ud ? h-1-y : y][flip_lr ? w-1-x : x]
 *   2 blur    separable, per channel, border reflect-101 (index -k -> k, h-1+k -> h-1-k; radius < h and radius < w):
 *             Hs[y][x] = S_k taps[|k|] * F[y][x+k] (k = -radius .. radius; at most 65280, not rounded), V[y][x] = S_k taps[|k|] * Hs[y+k][x],
 *             B = (V + 32768) >> 16.  taps[0] is the centre and taps[0] + 2 * (taps[1] + .. + taps[radius]) == 256; radius == 0 is the identity.
 *             The taps are data: the library validates them and evaluates no exp.
 *   3 random  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) with the key key[0..1] and the
 *             counter (y * w + x, draw, 0, 0) gives four 32-bit words per pixel and draw.  Known answers: counter and key all zero ->
 *             6627e8d5 e169c58d bc57ac4c 9b00dbd8; all ones (0xffffffff) -> 408f276d 41c83b0e a20bc7c6 6d5451fd.
 *   4 dropout draw 0, word 0 < drop_thr: the three channels of the pixel become 0 (one decision per pixel: iaa.Dropout, per_channel = False)
 *   5 noise   step i = 0, 1 uses draw i: with h0..h3 the 16-bit halves of two words (step 0: words 1 and 2; step 1: words 0 and 1),
 *             s = h0 + h1 + h2 + h3 - 131070 and d = (s * noise_q[i] + 2^23) >> 24 (64-bit, arithmetic shift); every channel becomes
 *             clamp(v + noise_loc[i] + d, 0, 255), clamped after each step.  s has standard deviation sqrt((65536^2 - 1) / 3) = 37837.227,
 *             so noise_q = round(scale * 2^24 / 37837.227).  A step with 131070 * noise_q < 2^23 has d == 0 everywhere.
 *   6 shift   O[y][x] = T[y][x - tx] where 0 <= x - tx < w, else 0 (imgaug's cval = 0).  Steps 3-5 are indexed by the position BEFORE the shift.
 *   7 enabled == 0: O = S byte for byte; no other field of the record is looked at.
 * Field ranges (yolo_augment_check; YOLO_ERR_ARG with a message of its own each): enabled, flip_lr, flip_ud 0 | 1; radius 0 .. 9 and below
 * h and w; the taps' sum; noise_q 0 .. 16383; noise_loc -255 .. 255; |tx| <= 2^30; h, w >= 1, w % 4 == 0, h * w < 2^31. */
typedef struct yolo_augment_image {
    int32_t enabled, flip_lr, flip_ud;
    int32_t radius;
    uint16_t taps[10];
    uint32_t drop_thr;
    int32_t noise_q[2];
    int32_t noise_loc[2];
    int32_t tx;
    uint32_t key[2];
} yolo_augment_image;
/* The checks of ONE record for an h x w image (pure host function, no device). */
int yolo_augment_check(const yolo_augment_image *params, int h, int w);
/* src_dev uint8 [n][h][w][3] -> dst_dev of the same shape, image i by params_host[i] (a HOST array: the records travel in the kernel
 * arguments, images_per_launch of yolo_augment_tile per launch, larger n as consecutive launches).  A workgroup produces a rows x cols
 * tile of an output image from the tile plus a 9-pixel halo held in LDS; the source is read and the destination written, never re-read.
 * src and dst must not overlap (YOLO_ERR_ARG); every byte of dst is written by each call; a dst that is not 4-byte aligned is served by
 * byte stores.  Checks as yolo_augment_check for every record ("image i: ..." in the message).  Enqueued on `stream`. */
int yolo_augment_u8(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w, const yolo_augment_image *params_host, void *stream);
/* The truths of one image under its record (pure host function; `in` and `out` may be the same array; out holds n_in records).  Each
 * truth in order, in float64, every operation rounded on its own: x1 = x - w / 2, x2 = x + w / 2, the same for y; flip_lr maps (x1, x2)
 * to (1 - x2, 1 - x1), flip_ud the same in y; the shift adds tx / W (W = the image width w, one division) to both x corners; the truth is
 * dropped if x2 <= 0, x1 >= 1, y2 <= 0, y1 >= 1 or any of the four is NaN; otherwise each corner is clipped to [0, 1] and
 * x = float32((x1 + x2) / 2), w = float32(x2 - x1), the same for y.  class_idx and difficult are kept, the order is kept.  enabled == 0
 * copies the records untouched.  *n_out receives the number of records written. */
int yolo_augment_truths_host(const yolo_gt *in, int n_in, const yolo_augment_image *params, int h, int w, yolo_gt *out, int32_t *n_out);
/* The kernel's constants (test hook): the output tile of a workgroup and the images one launch covers.  Any pointer may be null. */
int yolo_augment_tile(int32_t *rows, int32_t *cols, int32_t *images_per_launch);

/* ---- Anchor k-means on the device (added within ABI 7: new exports, the yolo_anchor_* PODs and enums only) -------------------------
 * The reference chooses anchors with sklearn.cluster.KMeans(n_clusters, tol) over the normalised (w, h) of every annotated box and scales
 * the centres by input / stride (net/v2.py:299-323, net/base.py:49-52): k-means++ seeding, n_init = 10, max_iter = 300, Lloyd, Euclidean
 * distance, an unseeded generator.  Here the same solver as a DEFINITION that leaves no tolerance: the data are fixed-point numbers, every
 * sum is an integer, every float64 operation is rounded on its own, and the random stream is counter-based -- so the result is the same
 * bits on every call and equals a sequential NumPy restatement (tests/anchor_ref.py) for any input.  DELIBERATE DIFFERENCES from sklearn:
 * (a) the data are quantised to 40 bits; (b) seeding draws one candidate per round, not the greedy 2 + log k; (c) an empty cluster keeps
 * its centre (sklearn moves it to a far point); (d) the random stream; (e) the distance 1 - IoU is offered beside the Euclidean one
 * (YOLOv2 paper, Darknet's calc_anchors).
 *
 * Data      n boxes as float64 (w, h), normalised by their image.  A value v is valid iff it is finite, 0 < v <= 1 and
 *           q = rint(v * 2^40) >= 1 (ties to even); a box is valid iff both are.  The problem's data are v' = q * 2^-40, at most 2^-41 from
 *           v.  Invalid boxes are skipped, counted (n_bad), labelled -1 and raise YOLO_ANCHOR_BAD_BOX.  1 <= n <= 2^22, 1 <= k <= 32,
 *           1 <= n_init <= 64, 1 <= max_iter <= 10000.
 * Centres   sums of q over a cluster are exact 64-bit integers in any order; centre = float64(S q) / (float64(count) * 2^40): one
 *           conversion, one division, each correctly rounded.  A cluster without boxes keeps its centre and raises
 *           YOLO_ANCHOR_EMPTY_CLUSTER in its restart (at any centre update and at the final assignment).
 * Distance  float64, every operation rounded on its own, with (w, h) = v' of the box and (cw, ch) a centre:
 *             euclidean  d = (w - cw) * (w - cw) + (h - ch) * (h - ch)
 *             iou        i = min(w, cw) * min(h, ch), d = 1 - i / (w * h + cw * ch - i)       (the sum first, then the difference)
 *           The label is the first k with the smallest d (strict <, ascending k).  qd = floor(d * 2^40) as an unsigned 64-bit integer.
 * Iteration assign with the current centres, then new centres; iterations count from 1.  euclidean (sklearn's rule): stop after iteration
 *           t >= 2 if every label equals that of iteration t - 1; otherwise stop if S_k ((cw' - cw)^2 + (ch' - ch)^2) <= tolerate * V, the
 *           sum taken in ascending k from 0.0, one term (a * a + b * b) at a time; otherwise stop at max_iter (YOLO_ANCHOR_MAX_ITER is
 *           raised in a restart that stopped for that reason alone).  V = (var_w + var_h) / 2 with var = float64(N) / (float64(n_valid)
 *           * float64(n_valid)) * 2^-80 and N = n_valid * S(q^2) - S(q)^2, an exact integer (the prepare kernel sums hi^2, hi * lo and lo^2
 *           of q = hi * 2^20 + lo in 64-bit integers -- SPLIT accumulation -- and the host joins them in 128 bits and rounds once).
 *           iou: stop when no label changed (t >= 2), or at max_iter; tolerate is not looked at.  After the last iteration ONE more
 *           assignment against the final centres gives labels, counts, sums, the inertia S qd (an exact integer, also reported * 2^-40)
 *           and avg_iou = float64(S floor(best * 2^40)) / (float64(n_valid) * 2^40), best = the largest i / (w * h + cw * ch - i) over the
 *           centres -- reported for both distances.
 * Seeding   when init is NULL: k-means++ with one draw per round.  Philox4x32-10 (the generator of the augmentation above) with the key
 *           (seed & 0xffffffff, seed >> 32) and the counter (restart, round, 0, 0); u = word0 * 2^32 + word1.  Round j weighs every valid box
 *           with D_i = 1 (round 0) or the smallest qd to the seeds chosen so far, in the CHOSEN distance (round j >= 1); T = S D_i;
 *           t = floor(u * T / 2^64) (a 128-bit product); the pick is the first valid i whose inclusive prefix sum exceeds t, and the seed
 *           is that box's v'.  T == 0 (fewer distinct boxes than k, or no valid box) marks the restart YOLO_ANCHOR_DEGENERATE: it runs no
 *           iteration and is never best.  All integers: the picks do not depend on the order of any reduction.
 *           With init ([k][2] float64, used as given): n_init must be 1; a centre that is not finite or not in (0, 1], or n_valid == 0,
 *           marks the restart degenerate.
 * Restarts  n_init restarts run side by side; the best has the lowest integer inertia, ties to the lowest index.  Its centres are
 *           returned in ascending order of area cw * ch (float64; ties: cw, then cluster index) with counts, sums and labels renumbered to
 *           match -- the order YOLOv3's scale masks expect.  If every restart is degenerate the header says YOLO_ANCHOR_DEGENERATE,
 *           best_restart is -1, the best block is all zero and every label is -1.
 * The header's status is YOLO_ANCHOR_BAD_BOX | (all degenerate: YOLO_ANCHOR_DEGENERATE) | the best restart's own bits. */
#define YOLO_ANCHOR_MAX_K 32
#define YOLO_ANCHOR_MAX_INIT 64
#define YOLO_ANCHOR_MAX_N (1 << 22)
#define YOLO_ANCHOR_ITER_LIMIT 10000
enum yolo_anchor_distance { YOLO_ANCHOR_EUCLIDEAN = 0, YOLO_ANCHOR_IOU = 1 };
enum yolo_anchor_status { YOLO_ANCHOR_BAD_BOX = 1, YOLO_ANCHOR_EMPTY_CLUSTER = 2, YOLO_ANCHOR_DEGENERATE = 4, YOLO_ANCHOR_MAX_ITER = 8 };

typedef struct yolo_anchor_desc {
    int32_t k, n_init, max_iter;
    int32_t distance;               /* enum yolo_anchor_distance */
    double tolerate;                /* euclidean only; finite, >= 0 */
    uint64_t seed;
} yolo_anchor_desc;

/* How a call is split and where the parts of the scratch and of the result lie (every part starts at a 256-byte boundary). */
struct yolo_anchor_plan {
    int32_t chunk, n_chunks;        /* boxes per workgroup (1024), ceil(n / chunk) */
    int32_t period;                 /* iterations enqueued between two reads of the finished-restart count */
    int32_t threads;
    uint64_t prep_offset, pick_offset, state_offset, q_offset, label_offset, label_stride, sums_offset, scratch_bytes;
    uint64_t header_offset, restarts_offset, best_offset, result_bytes;
};

typedef struct yolo_anchor_header {         /* result + header_offset */
    uint32_t status;
    int32_t best_restart, n_valid, n_bad, k, n_init, distance, pad_;
} yolo_anchor_header;
typedef struct yolo_anchor_restart {        /* result + restarts_offset, [n_init] */
    int32_t n_iter;
    uint32_t status;
    uint64_t inertia_q, iou_q;              /* S qd and S floor(best IoU * 2^40) of the final assignment */
    int32_t seeds[YOLO_ANCHOR_MAX_K];       /* box index of seed j; -1: j >= k, init given, or not drawn */
} yolo_anchor_restart;
typedef struct yolo_anchor_best {           /* result + best_offset: the best restart, clusters in ascending order of area */
    double centres[YOLO_ANCHOR_MAX_K][2];   /* (w, h); entries from k on are 0 */
    int64_t counts[YOLO_ANCHOR_MAX_K];
    uint64_t sum_q[YOLO_ANCHOR_MAX_K][2];
    uint64_t inertia_q, iou_q;
    double inertia, avg_iou;                /* inertia_q * 2^-40; float64(iou_q) / (float64(n_valid) * 2^40) */
} yolo_anchor_best;

/* The plan of a call with these sizes (pure host function): the sizing call for scratch and result.  YOLO_ERR_ARG, naming the field, for
 * anything outside the ranges above, an unknown distance, or a tolerate that is negative or not finite. */
int yolo_anchor_plan(const yolo_anchor_desc *desc, int64_t n, struct yolo_anchor_plan *out);
/* wh_dev float64 [n][2]; init_dev float64 [k][2] or NULL (then seeded; with init n_init must be 1); scratch_dev / result_dev of at least the
 * plan's sizes, 256-byte aligned, the scratch overlapping nothing else; labels_dev int32 [n] or NULL.  Every byte of the result, and of
 * labels when given, is written by every successful call, and nothing the scratch, the result or labels held before is read.
 * Kernels: prepare (validate, quantise, count, variance sums) | seeding, k rounds of two launches for all restarts at once (a weight pass
 * with per-chunk integer sums; one workgroup per restart that scans them and finds the pick inside its chunk) | per iteration an
 * assignment kernel on a (chunks x restarts) grid -- centres in LDS, per-cluster (S q_w, S q_h, count) and the changed count in integer LDS
 * atomics, merged into the restart's record by 64-bit integer atomics -- and a tiny SECOND KERNEL (one workgroup per restart) for the
 * centre update and the stop decision | final assignment | finish (best restart, order by area, the result) | labels.  There are no
 * floating-point atomics, no cooperative launch and no waiting on another workgroup: a finished restart has its `done` flag set, its
 * workgroups exit at once, and extra enqueued iterations change no bit.
 * UNLIKE the step entries THIS ENTRY SYNCHRONISES WITH THE HOST on `stream`: once after the prepare kernel (the threshold is made from its
 * sums on the host) and once after every `period` (8) enqueued iterations, to read one word, the count of finished restarts; it returns
 * after a last synchronisation, with the result complete.  Every host loop is bounded by max_iter. */
int yolo_anchor_kmeans(const yolo_anchor_desc *desc, const double *wh_dev, int64_t n, const double *init_dev, void *scratch_dev,
                       size_t scratch_bytes, void *result_dev, size_t result_bytes, int32_t *labels_dev, void *stream);

/* NMS of a HOST list (x,y,w,h as double, prob float, class int; scan order = index).  Synchronous;
 * allocates its own scratch.  keep_idx receives the indices of survivors in output order.
 * x and y are rounded to float32 before the IoU arithmetic: that is the type the reference's decode gives them
 * (net/v2.py:112-113, net/v3.py:129-130 under NumPy 2) and what every golden vector holds; a caller passing
 * float64 centres that are not float32 values gets the float32-rounded result (w, h stay float64). */
int yolo_nms_host(const double *xywh, const float *prob, const int32_t *class_idx, int n, double iou_threshold,
                  int nms_mode, int32_t *keep_idx, int32_t *n_keep);

#ifdef __cplusplus
}
#endif
#endif /* YOLO_HIP_H */

// C ABI of libyolo_hip.so (declared in include/yolo_hip.h): argument and state checks, then one call into the planner (plan.cpp), the
// forward engine (forward.cpp) or a launcher.  Decode + NMS, the frame, the evaluation, the loss and the augmentation entries live here
// whole; the training entries are train_api.cpp.  No exceptions cross the boundary.
#include <cstdio>
#include <cstring>
#include <new>

#include <cmath>
#include "yolo_internal.h"

using namespace yolo;

extern "C" {

int yolo_hip_abi_version(void) { return YOLO_HIP_ABI_VERSION; }

int yolo_mx_quantize(const void *src_f16_dev, int rows, int channels, uint8_t *q_dev, uint8_t *scale_dev, void *stream) {
    if (!src_f16_dev || !q_dev || !scale_dev || rows <= 0 || channels <= 0 || channels % 32)
        return fail(YOLO_ERR_ARG, "yolo_mx_quantize: null pointer, or rows / channels not positive, or channels not a multiple of 32");
    if ((uintptr_t)src_f16_dev % 16 || (uintptr_t)q_dev % 16)
        return fail(YOLO_ERR_ARG, "yolo_mx_quantize: source and element buffers must be 16-byte aligned");
    const hipError_t e = launch_mx_quantize(src_f16_dev, rows, channels, q_dev, scale_dev, reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(YOLO_ERR_HIP, std::string("yolo_mx_quantize: ") + hipGetErrorString(e));
    return YOLO_OK;
}
int yolo_mx_quantize_host(const float *src, int rows, int channels, uint8_t *q, uint8_t *scale) {
    if (!src || !q || !scale || rows <= 0 || channels <= 0 || channels % 32)
        return fail(YOLO_ERR_ARG, "yolo_mx_quantize_host: null pointer, or rows / channels not positive, or channels not a multiple of 32");
    const size_t blocks = (size_t)rows * (size_t)(channels / 32);
    for (size_t b = 0; b < blocks; ++b) scale[b] = mx_quant_block_host(src + 32 * b, q + 32 * b);
    return YOLO_OK;
}
const char *yolo_last_error(void) { return get_error(); }

int yolo_net_create(const yolo_layer_desc *layers, int n_layers, const yolo_net_options *opt, yolo_net **out) {
    if (!layers || !opt || !out || n_layers <= 0) return fail(YOLO_ERR_ARG, "yolo_net_create: null argument");
    if (opt->dtype != YOLO_DTYPE_F16 && opt->dtype != YOLO_DTYPE_F32 && opt->dtype != YOLO_DTYPE_MXF8)
        return fail(YOLO_ERR_ARG, "yolo_net_create: bad dtype");
    if (opt->max_batch <= 0) return fail(YOLO_ERR_ARG, "yolo_net_create: max_batch must be positive");
    yolo_net *net = new (std::nothrow) yolo_net();
    if (!net) return fail(YOLO_ERR_ARG, "out of host memory");
    net->opt = *opt;
    if (opt->dtype == YOLO_DTYPE_MXF8) {      // the fp16 plan (storage, fusions, arenas, streams) with the eligible 3x3 convs on conv_mx.hip
        net->opt.dtype = YOLO_DTYPE_F16;
        net->mx = true;
    }
    if (net->opt.cand_capacity <= 0) net->opt.cand_capacity = 4096;
    if (net->opt.max_boxes <= 0) net->opt.max_boxes = 256;
    if (net->opt.cand_capacity > 65536) {
        delete net;
        return fail(YOLO_ERR_ARG, "cand_capacity above 65536 (16-bit sort indices)");
    }
    std::string err;
    int rc = YOLO_ERR_PLAN;
    try {
        rc = plan_network(net, layers, n_layers, err);
    } catch (const std::exception &e) {
        err = e.what();
    }
    if (rc != YOLO_OK) {
        delete net;
        return fail(rc, "yolo_net_create: " + err);
    }
    int n_mx = 0;
    for (Kernel &k : net->kernels) {
        k.mx = mx_eligible(net, k) ? 1 : 0;
        n_mx += k.mx;
    }
    if (net->opt.force_tile == kMxTile + 1 && (!net->mx || !n_mx)) {     // the MX kernel: only where the plan runs it
        delete net;
        return fail(YOLO_ERR_ARG, "yolo_net_create: tile 24 (the MXFP8 3x3 kernel; yolo_net_options.force_tile = 25) needs dtype MXF8 and a "
                                  "3x3 / stride-1 conv with Cin % 128 == 0 and W <= 100");
    }
    if (net->opt.force_tile > 0 && net->opt.force_tile != kMxTile + 1)        // test / tuning hook: one tile id on every conv that accepts it
        for (Kernel &k : net->kernels)
            if (conv_dispatched(k) && conv_tile_valid(net, k, net->opt.force_tile - 1)) k.tile = net->opt.force_tile - 1;
    // the split-K slab is the last region of the workspace (plan.cpp reserves nothing for it): sized from the launches that can split
    net->splitk_bytes = splitk_slab_bytes(net) * (size_t)net->arenas;
    if (net->splitk_bytes) net->tail.push_back({"split-K tickets + slabs", net->splitk_off, net->splitk_bytes, net->splitk_bytes});
    net->workspace_bytes = net->splitk_off + net->splitk_bytes;
    *out = net;
    return YOLO_OK;
}

void yolo_net_destroy(yolo_net *net) {
    if (!net) return;
    destroy_streams(net);
    delete net;
}

size_t yolo_net_weight_count(const yolo_net *net) { return net ? net->weight_count : 0; }
size_t yolo_net_weights_bytes(const yolo_net *net) { return net ? net->weights_bytes : 0; }
size_t yolo_net_workspace_bytes(const yolo_net *net) { return net ? net->workspace_bytes : 0; }
size_t yolo_net_output_count(const yolo_net *net) { return net ? net->out_count : 0; }
double yolo_net_flops_per_image(const yolo_net *net) { return net ? net->flops_per_image : 0.0; }
int yolo_net_num_kernels(const yolo_net *net) { return net ? (int)net->kernels.size() : 0; }
int yolo_net_num_streams(const yolo_net *net) { return net ? net->parts : 0; }

int yolo_net_head_desc(const yolo_net *net, yolo_head_desc *out) {
    if (!net || !out) return fail(YOLO_ERR_ARG, "yolo_net_head_desc: null argument");
    *out = net->head;
    return YOLO_OK;
}

int yolo_net_set_head(yolo_net *net, const yolo_head_desc *head) {
    if (!net || !head) return fail(YOLO_ERR_ARG, "yolo_net_set_head: null argument");
    std::string err;
    int rc = check_head(head, net->out_count, err);
    if (rc) return fail(rc, "yolo_net_set_head: " + err);
    net->head = *head;
    return YOLO_OK;
}

int yolo_net_workspace_regions(const yolo_net *net, yolo_ws_region *out, int cap) {
    if (!net) return 0;
    int n = 0;
    auto add = [&](const std::string &name, size_t off, size_t used, size_t region) {
        if (out && n < cap) {
            memset(&out[n], 0, sizeof out[n]);
            snprintf(out[n].name, sizeof out[n].name, "%s", name.c_str());
            out[n].offset = off; out[n].used_bytes = used; out[n].region_bytes = region;
        }
        ++n;
    };
    for (int a = 0; a < net->arenas; ++a)
        for (size_t b = 0; b < net->buffers.size(); ++b) {
            const Buffer &B = net->buffers[b];
            if (!B.bytes) continue;
            add("tensor " + std::to_string(b) + " arena " + std::to_string(a), (size_t)a * net->arena_bytes + B.offset, B.used, B.bytes);
        }
    for (const WsRegion &r : net->tail) add(r.name, r.offset, r.used, r.bytes);
    return n;
}

size_t yolo_net_describe(const yolo_net *net, char *buf, size_t cap) {
    if (!net) return 0;
    std::string s = describe(net);
    if (buf && cap) {
        size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size() + 1;
}

int yolo_net_load_weights(yolo_net *net, const float *host_weights, size_t n, void *dev_weights, size_t dev_bytes) {
    if (!net || !dev_weights || (!host_weights && n)) return fail(YOLO_ERR_ARG, "yolo_net_load_weights: null argument");
    if (dev_bytes < net->weights_bytes) return fail(YOLO_ERR_ARG, "yolo_net_load_weights: device buffer too small");
    if ((uintptr_t)dev_weights % 256) return fail(YOLO_ERR_ARG, "yolo_net_load_weights: device buffer must be 256-byte aligned");
    std::vector<unsigned char> blob;
    std::string err;
    int rc = pack_weights(net, host_weights, n, blob, err);
    if (rc) return fail(rc, "yolo_net_load_weights: " + err);
    HIP_TRY(hipMemcpy(dev_weights, blob.data(), blob.size(), hipMemcpyHostToDevice));
    net->dev_weights = static_cast<unsigned char *>(dev_weights);
    net->weights_loaded = true;
    return YOLO_OK;
}

int yolo_net_bind_workspace(yolo_net *net, void *ws, size_t bytes) {
    if (!net || !ws) return fail(YOLO_ERR_ARG, "yolo_net_bind_workspace: null argument");
    if (bytes < net->workspace_bytes) return fail(YOLO_ERR_ARG, "yolo_net_bind_workspace: workspace too small");
    if ((uintptr_t)ws % 256) return fail(YOLO_ERR_ARG, "yolo_net_bind_workspace: workspace must be 256-byte aligned");
    net->dev_ws = static_cast<unsigned char *>(ws);
    net->cand_clean = 0;        // (whatever the new workspace holds where the candidate counters live)
    net->dev_ws_bytes = bytes;
    return zero_pair_counters(net);
}

}  // extern "C"

// ---- the checks and launch lists that the training entries (train_api.cpp) share with the entries here: declared in yolo_internal.h
namespace yolo {

int check_head(const yolo_head_desc *h, size_t out_count, std::string &err) {
    if (h->version != 2 && h->version != 3) { err = "head version must be 2 or 3"; return YOLO_ERR_ARG; }
    if (h->n_scales < 1 || h->n_scales > YOLO_MAX_SCALES || h->n_classes < 1) { err = "bad head geometry"; return YOLO_ERR_ARG; }
    size_t rows = 0;
    for (int s = 0; s < h->n_scales; ++s) {
        if (h->n_anchors[s] < 1 || h->n_anchors[s] > YOLO_MAX_ANCHORS || h->h[s] < 1 || h->w[s] < 1) { err = "bad head scale"; return YOLO_ERR_ARG; }
        rows += (size_t)h->h[s] * h->w[s] * h->n_anchors[s];
    }
    if (out_count && rows * (5 + h->n_classes) != out_count) { err = "head geometry does not match the network output size"; return YOLO_ERR_ARG; }
    return YOLO_OK;
}

int check_ready(yolo_net *net, const void *in, int batch, const char *who) {
    if (!net || !in) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (batch <= 0 || batch > net->opt.max_batch) return fail(YOLO_ERR_ARG, std::string(who) + ": batch outside 1..max_batch");
    if (!net->weights_loaded && net->weight_count) return fail(YOLO_ERR_STATE, std::string(who) + ": weights not loaded");
    if (!net->dev_ws) return fail(YOLO_ERR_STATE, std::string(who) + ": workspace not bound");
    return YOLO_OK;
}

// every check here is made on the host, before any device call
int check_loss_args(const yolo_head_desc *head, const void *gt_dev, const void *gt_counts_dev, int max_gt, const void *images_dev,
                    const void *result_dev, const char *who) {
    if (!head || !gt_dev || !gt_counts_dev || !images_dev || !result_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (max_gt < 1 || max_gt > YOLO_EVAL_MAX_GT) return fail(YOLO_ERR_ARG, std::string(who) + ": max_gt must be 1.." + std::to_string(YOLO_EVAL_MAX_GT));
    if (head->version != 2 || head->n_scales != 1)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the head must be version 2 with one scale (the reference has a loss for YOLOv2 only)");
    std::string err;
    int rc = check_head(head, 0, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    if ((long long)head->h[0] * head->w[0] > YOLO_LOSS_MAX_CELLS)
        return fail(YOLO_ERR_ARG, std::string(who) + ": h * w must be at most " + std::to_string(YOLO_LOSS_MAX_CELLS));
    return YOLO_OK;
}

static int run_loss(const yolo_head_desc &h, const float *logits, int batch, const yolo_gt *gt, const int32_t *gt_counts, int max_gt,
                    yolo_loss_image *images, int32_t *assign, yolo_loss_result *result, hipStream_t s) {
    LossParams p;
    memset(&p, 0, sizeof p);
    p.logits = logits; p.gt = gt; p.gt_counts = gt_counts; p.max_gt = max_gt;
    p.h = h.h[0]; p.w = h.w[0]; p.na = h.n_anchors[0]; p.n_classes = h.n_classes;
    for (int a = 0; a < p.na; ++a) {
        p.aw[a] = h.anchors[0][2 * a]; p.ah[a] = h.anchors[0][2 * a + 1];
        p.awf[a] = (float)p.aw[a]; p.ahf[a] = (float)p.ah[a];
    }
    p.images = images; p.assign = assign;
    HIP_TRY(launch_loss_images(p, batch, s));
    HIP_TRY(launch_loss_finish(LossFinishParams{images, batch, 0, batch, result}, s));
    return YOLO_OK;
}

// the kernels of yolo_v2_loss_grad: the two of run_loss, then the gradient kernel on the winner table they left
int run_loss_grad(const yolo_head_desc &h, const float *logits, int batch, const yolo_gt *gt, const int32_t *gt_counts, int max_gt,
                  yolo_loss_image *images, int32_t *assign, yolo_loss_result *result, float *grad, hipStream_t s) {
    int rc = run_loss(h, logits, batch, gt, gt_counts, max_gt, images, assign, result, s);
    if (rc) return rc;
    LossGradParams p;
    memset(&p, 0, sizeof p);
    p.logits = logits; p.gt = gt; p.assign = assign; p.grad = grad; p.batch = batch; p.max_gt = max_gt;
    p.h = h.h[0]; p.w = h.w[0]; p.na = h.n_anchors[0]; p.n_classes = h.n_classes;
    for (int a = 0; a < p.na; ++a) { p.awf[a] = (float)h.anchors[0][2 * a]; p.ahf[a] = (float)h.anchors[0][2 * a + 1]; }
    HIP_TRY(launch_loss_grad(p, s));
    return YOLO_OK;
}

int run_loss3(const Loss3Geometry &geo, const float *logits, int batch, const yolo_gt *gt, const int32_t *gt_counts, int max_gt,
              double ignore_thresh, yolo_loss_image *parts, yolo_loss_image *images, int32_t *assign, yolo_loss_result *result, float *grad,
              hipStream_t s) {
    Loss3Params p;
    memset(&p, 0, sizeof p);
    p.logits = logits; p.gt = gt; p.gt_counts = gt_counts; p.batch = batch; p.max_gt = max_gt; p.ignore_thresh = ignore_thresh; p.geo = geo;
    p.parts = parts; p.images = images; p.assign = assign; p.result = result; p.grad = grad;
    HIP_TRY(launch_loss3(p, s));
    if (grad) HIP_TRY(launch_loss3_grad(p, s));
    return YOLO_OK;
}

}  // namespace yolo

namespace {

void fill_decode(const yolo_head_desc &h, DecodeParams &dp) {
    dp.version = h.version;
    dp.n_classes = h.n_classes;
    dp.n_scales = h.n_scales;
    int row0 = 0;
    for (int s = 0; s < h.n_scales; ++s) {
        dp.sc[s].row0 = row0; dp.sc[s].h = h.h[s]; dp.sc[s].w = h.w[s]; dp.sc[s].na = h.n_anchors[s];
        for (int a = 0; a < h.n_anchors[s]; ++a) { dp.sc[s].aw[a] = h.anchors[s][2 * a]; dp.sc[s].ah[a] = h.anchors[s][2 * a + 1]; }
        row0 += h.h[s] * h.w[s] * h.n_anchors[s];
    }
    dp.rows = row0;
}

int run_decode_nms(const yolo_head_desc &h, const float *logits, int batch, double thr, double iou, int mode, int cap,
                   int max_boxes, unsigned char *cand, int *cand_count, yolo_box *boxes, int32_t *counts, int32_t *status,
                   int32_t *keep_idx, hipStream_t s, unsigned char *nms_scratch = nullptr, const float *obj = nullptr, int *counters_clean = nullptr) {
    DecodeParams dp;
    memset(&dp, 0, sizeof dp);
    fill_decode(h, dp);
    dp.logits = logits;
    dp.obj = obj;
    dp.threshold = (float)thr;      // `p < threshold` compares in float32 under NumPy 2 (weak Python float)
    dp.cap = cap;
    dp.cand = cand;
    dp.cand_count = cand_count;
    dp.total_rows = (long long)batch * dp.rows;
    // counters_clean (yolo_net_detect): the counters are the net's own; the NMS kernel returns each counter it read to zero, so only the
    // first detect, one behind a failed one, and one at a LARGER batch than any before it need the memset launch (4.5 us: half a
    // percent of a batch-1 step).  *counters_clean = how many counters, from the first, are known to be zero: the memset and the NMS
    // reset cover the current call's `batch` counters only (a detect of 1 image followed by one of 32 found counters 1..31 as the
    // caller's workspace held them -- uninitialised memory for a C-ABI caller: ADVICE r4).
    const int clean_n = counters_clean ? *counters_clean : 0;
    const bool need_clear = batch > clean_n;
    if (counters_clean) *counters_clean = 0;
    HIP_TRY(launch_decode(dp, batch, s, need_clear));
    NmsParams np;
    np.cand = reinterpret_cast<const Candidate *>(cand);
    np.cand_count = cand_count;
    np.cap = cap; np.max_boxes = max_boxes; np.mode = mode;
    np.iou_threshold = iou;
    np.boxes = boxes; np.counts = counts; np.status = status; np.keep_idx = keep_idx;
    np.scratch = nms_scratch; np.scratch_stride = nms_scratch_bytes(cap);
    np.reset_count = counters_clean ? cand_count : nullptr;
    HIP_TRY(launch_nms(np, batch, s));
    if (counters_clean) *counters_clean = need_clear ? batch : clean_n;
    return YOLO_OK;
}

}  // namespace

extern "C" {

// The float32 entries and their uint8 twins (ABI 7) are one implementation each, told apart by the NetIn tag and the name in messages.
static int forward_any(yolo_net *net, const NetIn in, int batch, float *out_dev, void *stream, const char *who) {
    int rc = check_ready(net, in.ptr, batch, who);
    if (rc) return rc;
    if (!out_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null output");
    return run_forward(net, in, batch, out_dev, static_cast<hipStream_t>(stream));
}
int yolo_net_forward(yolo_net *net, const float *in_dev, int batch, float *out_dev, void *stream) {
    return forward_any(net, NetIn{in_dev, false}, batch, out_dev, stream, "yolo_net_forward");
}
int yolo_net_forward_u8(yolo_net *net, const uint8_t *in_dev, int batch, float *out_dev, void *stream) {
    return forward_any(net, NetIn{in_dev, true}, batch, out_dev, stream, "yolo_net_forward_u8");
}

static int forward_timed_any(yolo_net *net, const NetIn in_dev, int batch, float *out_dev, void *stream, float *ms_host, const char *who) {
    int rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    if (!out_dev || !ms_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null output");
    return run_forward_timed(net, in_dev, batch, out_dev, static_cast<hipStream_t>(stream), ms_host);
}
int yolo_net_forward_timed(yolo_net *net, const float *in_dev, int batch, float *out_dev, void *stream, float *ms_host) {
    return forward_timed_any(net, NetIn{in_dev, false}, batch, out_dev, stream, ms_host, "yolo_net_forward_timed");
}
int yolo_net_forward_timed_u8(yolo_net *net, const uint8_t *in_dev, int batch, float *out_dev, void *stream, float *ms_host) {
    return forward_timed_any(net, NetIn{in_dev, true}, batch, out_dev, stream, ms_host, "yolo_net_forward_timed_u8");
}

int yolo_net_kernel_info(const yolo_net *net, int kernel, yolo_kernel_info *out) {
    if (!net || !out || kernel < 0 || kernel >= (int)net->kernels.size()) return fail(YOLO_ERR_ARG, "yolo_net_kernel_info: bad argument");
    const Kernel &k = net->kernels[kernel];
    memset(out, 0, sizeof *out);
    out->kind = k.kind; out->layer = k.layer;
    if (k.kind == K_CONV) conv_kernel_info(net, kernel, out);
    else aux_kernel_info(net, kernel, out);
    return YOLO_OK;
}

static int tune_streams_any(yolo_net *net, const NetIn in_dev, int batch, void *stream, const char *who) {
    int rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    return tune_streams(net, in_dev, batch, static_cast<hipStream_t>(stream), who);
}
int yolo_net_tune_streams(yolo_net *net, const float *in_dev, int batch, void *stream) {
    return tune_streams_any(net, NetIn{in_dev, false}, batch, stream, "yolo_net_tune_streams");
}
int yolo_net_tune_streams_u8(yolo_net *net, const uint8_t *in_dev, int batch, void *stream) {
    return tune_streams_any(net, NetIn{in_dev, true}, batch, stream, "yolo_net_tune_streams_u8");
}

int yolo_net_set_streams(yolo_net *net, int parts) {
    if (!net) return fail(YOLO_ERR_ARG, "yolo_net_set_streams: null net");
    if (parts == net->parts) return YOLO_OK;
    if (!net->arena_full || parts < 1 || parts > net->arenas)
        return fail(YOLO_ERR_STATE, "yolo_net_set_streams: this net was planned for " + std::to_string(net->parts) + " part(s) only (streams given explicitly, or the rule says one)");
    net->parts = parts;
    net->parts_tuned = true;
    net->obj_valid = false;
    return YOLO_OK;
}

int yolo_net_autotune(yolo_net *net, const float *in_dev, int batch, void *stream) {
    int rc = check_ready(net, in_dev, batch, "yolo_net_autotune");
    if (rc) return rc;
    return autotune_tiles(net, NetIn{in_dev, false}, batch, static_cast<hipStream_t>(stream));
}

static int detect_any(yolo_net *net, const NetIn in_dev, int batch, double threshold, double iou_threshold, int nms_mode,
                      yolo_box *boxes_dev, int32_t *counts_dev, int32_t *status_dev, void *stream, const char *who) {
    int rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    if (!boxes_dev || !counts_dev || !status_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null output");
    std::string err;
    rc = check_head(&net->head, net->out_count, err);
    if (rc) return fail(YOLO_ERR_STATE, std::string(who) + ": head geometry not set (" + err + "); call yolo_net_set_head");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    // The logits of a detect call never leave the workspace, and the decode kernel reads the objectness of every row from the compact
    // array the head convs fill and the rest of a row only where sigmoid(objectness) reaches the threshold (p = sigmoid(obj) in v3,
    // <= sigmoid(obj) in v2): rows 0.01 below the threshold's logit are not written (conv_common.h: conv_epilogue_f32_staged).  Only
    // when EVERY head conv of this plan writes the compact array -- else the decode would look for objectness in rows never written.
    static const bool dense = getenv("YOLO_DENSE_LOGITS") != nullptr;       // A/B switch (same boxes either way)
    net->obj_min_logit = -INFINITY;
    // (thresholds within 1e-4 of 1 run dense: there the decode's float32 sigmoid saturates -- sigmoid_f32(x) rounds to 1 - 2^-23 over a range
    // of x wider than the 0.01 margin, so rows the decode accepts would lie below the cut; at 1 - 1e-4 the margin is still ten float32
    // rounding errors of p wide)
    if (!dense && threshold > 0.0 && threshold < 1.0 - 1e-4 && all_heads_write_objectness(net, in_dev, logits, batch))
        net->obj_min_logit = (float)(std::log(threshold / (1.0 - threshold)) - 0.01);
    rc = run_forward(net, in_dev, batch, logits, s);
    net->obj_min_logit = -INFINITY;
    if (rc) return rc;
    return run_decode_nms(net->head, logits, batch, threshold, iou_threshold, nms_mode, net->opt.cand_capacity,
                          net->opt.max_boxes, net->dev_ws + net->cand_off, reinterpret_cast<int *>(net->dev_ws + net->count_off),
                          boxes_dev, counts_dev, status_dev, nullptr, s, net->dev_ws + net->nms_off,
                          net->obj_valid ? reinterpret_cast<const float *>(net->dev_ws + net->obj_off) : nullptr, &net->cand_clean);
}
int yolo_net_detect(yolo_net *net, const float *in_dev, int batch, double threshold, double iou_threshold, int nms_mode,
                    yolo_box *boxes_dev, int32_t *counts_dev, int32_t *status_dev, void *stream) {
    return detect_any(net, NetIn{in_dev, false}, batch, threshold, iou_threshold, nms_mode, boxes_dev, counts_dev, status_dev, stream, "yolo_net_detect");
}
int yolo_net_detect_u8(yolo_net *net, const uint8_t *in_dev, int batch, double threshold, double iou_threshold, int nms_mode,
                       yolo_box *boxes_dev, int32_t *counts_dev, int32_t *status_dev, void *stream) {
    return detect_any(net, NetIn{in_dev, true}, batch, threshold, iou_threshold, nms_mode, boxes_dev, counts_dev, status_dev, stream, "yolo_net_detect_u8");
}

int yolo_net_read_layer(yolo_net *net, int layer, int batch, float *host_out, size_t n) {
    if (!net || !host_out) return fail(YOLO_ERR_ARG, "yolo_net_read_layer: null argument");
    if (!net->opt.keep_all) return fail(YOLO_ERR_STATE, "yolo_net_read_layer: create the net with keep_all=1");
    if (layer < 0 || layer >= (int)net->layers.size() || !net->layers[layer].materialised)
        return fail(YOLO_ERR_ARG, "yolo_net_read_layer: layer has no materialised tensor (fused away or out of range)");
    const View &v = net->layers[layer].view;
    if (v.buf < 0) return fail(YOLO_ERR_ARG, "yolo_net_read_layer: layer lives in a caller-owned tensor");
    const size_t need = (size_t)batch * v.H * v.W * v.C;
    if (n < need || batch > net->opt.max_batch) return fail(YOLO_ERR_ARG, "yolo_net_read_layer: host buffer too small");
    HIP_TRY(hipDeviceSynchronize());
    const Buffer &b = net->buffers[v.buf];
    const int es = v.f32 ? 4 : net->esize;
    std::vector<unsigned char> tmp((size_t)batch * v.img_stride * es);
    HIP_TRY(hipMemcpy(tmp.data(), net->dev_ws + b.offset, tmp.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < batch; ++i)
        for (long long px = 0; px < (long long)v.H * v.W; ++px)
            for (int c = 0; c < v.C; ++c) {
                const size_t e = (size_t)i * v.img_stride + (size_t)px * v.ld + v.coff + c;
                float f;
                if (es == 4) f = reinterpret_cast<const float *>(tmp.data())[e];
                else f = (float)reinterpret_cast<const _Float16 *>(tmp.data())[e];
                host_out[((size_t)i * v.H * v.W + px) * v.C + c] = f;
            }
    return YOLO_OK;
}

// scratch of the standalone decode + NMS: candidates at 0 | counters | NMS slabs
struct DecodeScratch {
    size_t counters, slabs, total;
    DecodeScratch(int batch, int cap) {
        counters = align256(sizeof(Candidate) * (size_t)cap * batch);
        slabs = counters + align256(sizeof(int) * (size_t)batch * kCandCountStride);
        total = slabs + nms_scratch_bytes(cap) * (size_t)batch;
    }
};

size_t yolo_decode_scratch_bytes(const yolo_head_desc *head, int batch, int cand_capacity) {
    (void)head;
    if (batch <= 0) return 0;
    return DecodeScratch(batch, cand_capacity <= 0 ? 4096 : cand_capacity).total;
}

int yolo_decode_nms(const yolo_head_desc *head, const float *logits_dev, int batch, double threshold, double iou_threshold,
                    int nms_mode, int cand_capacity, int max_boxes, void *scratch_dev, size_t scratch_bytes, yolo_box *boxes_dev,
                    int32_t *counts_dev, int32_t *status_dev, void *stream) {
    if (!head || !logits_dev || !scratch_dev || !boxes_dev || !counts_dev || !status_dev || batch <= 0)
        return fail(YOLO_ERR_ARG, "yolo_decode_nms: null argument");
    if (cand_capacity <= 0) cand_capacity = 4096;
    if (max_boxes <= 0) max_boxes = 256;
    std::string err;
    int rc = check_head(head, 0, err);
    if (rc) return fail(rc, "yolo_decode_nms: " + err);
    if (cand_capacity > 65536) return fail(YOLO_ERR_ARG, "yolo_decode_nms: cand_capacity above 65536");
    const DecodeScratch L(batch, cand_capacity);
    if (scratch_bytes < L.total) return fail(YOLO_ERR_ARG, "yolo_decode_nms: scratch too small");
    unsigned char *base = static_cast<unsigned char *>(scratch_dev);
    return run_decode_nms(*head, logits_dev, batch, threshold, iou_threshold, nms_mode, cand_capacity, max_boxes, base,
                          reinterpret_cast<int *>(base + L.counters), boxes_dev, counts_dev, status_dev, nullptr,
                          static_cast<hipStream_t>(stream), base + L.slabs);
}

static int resize_any(const uint8_t *src_dev, int src_h, int src_w, int src_row_bytes, void *dst_dev, bool dst_u8, int dst_h, int dst_w,
                      int swap_rb, void *stream, const char *who) {
    if (!src_dev || !dst_dev || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0 || src_row_bytes < 3 * src_w)
        return fail(YOLO_ERR_ARG, std::string(who) + ": bad argument");
    ResizeParams p;
    p.src = src_dev; p.dst = dst_dev;
    p.src_h = src_h; p.src_w = src_w; p.src_row_bytes = src_row_bytes; p.dst_h = dst_h; p.dst_w = dst_w; p.swap_rb = swap_rb ? 1 : 0;
    HIP_TRY(launch_resize(p, static_cast<hipStream_t>(stream), dst_u8));
    return YOLO_OK;
}
int yolo_preprocess_resize(const uint8_t *src_dev, int src_h, int src_w, int src_row_bytes, float *dst_dev, int dst_h, int dst_w,
                           int swap_rb, void *stream) {
    return resize_any(src_dev, src_h, src_w, src_row_bytes, dst_dev, false, dst_h, dst_w, swap_rb, stream, "yolo_preprocess_resize");
}
int yolo_preprocess_resize_u8(const uint8_t *src_dev, int src_h, int src_w, int src_row_bytes, uint8_t *dst_dev, int dst_h, int dst_w,
                              int swap_rb, void *stream) {
    return resize_any(src_dev, src_h, src_w, src_row_bytes, dst_dev, true, dst_h, dst_w, swap_rb, stream, "yolo_preprocess_resize_u8");
}

// ---- frames of any size (yolo_hip.h: added within ABI 7) -------------------------------------------------------------------------
static bool frame_geometry(int src_h, int src_w, int dst_h, int dst_w, int mode, int &new_h, int &new_w, int &off_y, int &off_x) {
    if (src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || (mode != YOLO_RESIZE_STRETCH && mode != YOLO_RESIZE_LETTERBOX)) return false;
    new_h = dst_h; new_w = dst_w;
    if (mode == YOLO_RESIZE_LETTERBOX) {
        if ((long long)dst_w * src_h < (long long)dst_h * src_w) {      // the width binds (Darknet: net_w / w < net_h / h, cross-multiplied)
            const long long v = (long long)src_h * dst_w / src_w;
            new_h = v < 1 ? 1 : (int)v;
        } else {
            const long long v = (long long)src_w * dst_h / src_h;
            new_w = v < 1 ? 1 : (int)v;
        }
    }
    off_y = (dst_h - new_h) / 2;
    off_x = (dst_w - new_w) / 2;
    return true;
}

int yolo_letterbox_geometry(int src_h, int src_w, int dst_h, int dst_w, int mode, int32_t *new_h, int32_t *new_w, int32_t *off_y, int32_t *off_x) {
    if (!new_h || !new_w || !off_y || !off_x) return fail(YOLO_ERR_ARG, "yolo_letterbox_geometry: null argument");
    if (mode != YOLO_RESIZE_STRETCH && mode != YOLO_RESIZE_LETTERBOX) return fail(YOLO_ERR_ARG, "yolo_letterbox_geometry: mode must be YOLO_RESIZE_STRETCH or YOLO_RESIZE_LETTERBOX");
    int nh, nw, oy, ox;
    if (!frame_geometry(src_h, src_w, dst_h, dst_w, mode, nh, nw, oy, ox)) return fail(YOLO_ERR_ARG, "yolo_letterbox_geometry: sizes must be at least 1");
    *new_h = nh; *new_w = nw; *off_y = oy; *off_x = ox;
    return YOLO_OK;
}

// the checks every frame entry makes of its descriptors and mode
static int check_frames(const yolo_frame *frames, int n, int mode, bool need_pixels, const char *who) {
    if (!frames) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (n < 1) return fail(YOLO_ERR_ARG, std::string(who) + ": frame count must be at least 1");
    if (mode != YOLO_RESIZE_STRETCH && mode != YOLO_RESIZE_LETTERBOX) return fail(YOLO_ERR_ARG, std::string(who) + ": mode must be YOLO_RESIZE_STRETCH or YOLO_RESIZE_LETTERBOX");
    for (int i = 0; i < n; ++i) {
        const yolo_frame &f = frames[i];
        if (f.h < 1 || f.w < 1) return fail(YOLO_ERR_ARG, std::string(who) + ": frame " + std::to_string(i) + " has h or w below 1");
        if (need_pixels && !f.pixels_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": frame " + std::to_string(i) + " has no pixels");
        if (need_pixels && (long long)f.row_bytes < 3LL * f.w) return fail(YOLO_ERR_ARG, std::string(who) + ": frame " + std::to_string(i) + " has row_bytes below 3 * w");
    }
    return YOLO_OK;
}

static int frames_any(const yolo_frame *frames, int n, int mode, void *dst_dev, bool dst_u8, int dst_h, int dst_w, void *stream, const char *who) {
    int rc = check_frames(frames, n, mode, true, who);
    if (rc) return rc;
    if (!dst_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (dst_h < 1 || dst_w < 1) return fail(YOLO_ERR_ARG, std::string(who) + ": dst_h and dst_w must be at least 1");
    if (dst_w % 4) return fail(YOLO_ERR_ARG, std::string(who) + ": dst_w must be a multiple of 4");
    const size_t esize = dst_u8 ? 1 : 4;
    const size_t img_bytes = (size_t)dst_h * dst_w * 3 * esize;
    FramesParams p;
    p.dst_h = dst_h; p.dst_w = dst_w;
    p.wide = (uintptr_t)dst_dev % (dst_u8 ? 4 : 16) == 0;
    for (int i0 = 0; i0 < n; i0 += kFramesPerLaunch) {
        const int m = n - i0 < kFramesPerLaunch ? n - i0 : kFramesPerLaunch;
        for (int i = 0; i < m; ++i) {
            const yolo_frame &f = frames[i0 + i];
            FrameGeom &g = p.f[i];
            g.src = f.pixels_dev; g.src_h = f.h; g.src_w = f.w; g.src_row_bytes = f.row_bytes; g.swap_rb = f.swap_rb ? 1 : 0;
            frame_geometry(f.h, f.w, dst_h, dst_w, mode, g.new_h, g.new_w, g.off_y, g.off_x);
        }
        for (int i = m; i < kFramesPerLaunch; ++i) p.f[i] = FrameGeom{nullptr, 1, 1, 3, 0, 1, 1, 0, 0};
        p.dst = static_cast<unsigned char *>(dst_dev) + (size_t)i0 * img_bytes;     // (a multiple of 12 / 48 bytes per image: alignment stays)
        HIP_TRY(launch_frames_resize(p, m, static_cast<hipStream_t>(stream), dst_u8));
    }
    return YOLO_OK;
}
int yolo_preprocess_frames_u8(const yolo_frame *frames_host, int n, int mode, uint8_t *dst_dev, int dst_h, int dst_w, void *stream) {
    return frames_any(frames_host, n, mode, dst_dev, true, dst_h, dst_w, stream, "yolo_preprocess_frames_u8");
}
int yolo_preprocess_frames(const yolo_frame *frames_host, int n, int mode, float *dst_dev, int dst_h, int dst_w, void *stream) {
    return frames_any(frames_host, n, mode, dst_dev, false, dst_h, dst_w, stream, "yolo_preprocess_frames");
}

static int boxes_to_frames_any(yolo_box *boxes_dev, const int32_t *counts_dev, int batch, int max_boxes, const yolo_frame *frames, int mode,
                               int net_h, int net_w, void *stream, const char *who) {
    int rc = check_frames(frames, batch, mode, false, who);
    if (rc) return rc;
    if (!boxes_dev || !counts_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (max_boxes < 1 || net_h < 1 || net_w < 1) return fail(YOLO_ERR_ARG, std::string(who) + ": max_boxes, net_h and net_w must be at least 1");
    if (mode == YOLO_RESIZE_STRETCH) return YOLO_OK;        // new = net, offsets 0: x * W / W is x -- nothing to launch
    RemapParams p;
    p.max_boxes = max_boxes; p.net_h = net_h; p.net_w = net_w;
    for (int i0 = 0; i0 < batch; i0 += kFramesPerLaunch) {
        const int m = batch - i0 < kFramesPerLaunch ? batch - i0 : kFramesPerLaunch;
        for (int i = 0; i < kFramesPerLaunch; ++i) {
            BoxGeom &g = p.g[i];
            g = BoxGeom{1, 1, 0, 0};
            if (i < m) frame_geometry(frames[i0 + i].h, frames[i0 + i].w, net_h, net_w, mode, g.new_h, g.new_w, g.off_y, g.off_x);
        }
        p.boxes = boxes_dev + (size_t)i0 * max_boxes;
        p.counts = counts_dev + i0;
        HIP_TRY(launch_boxes_to_frames(p, m, static_cast<hipStream_t>(stream)));
    }
    return YOLO_OK;
}
int yolo_boxes_to_frames(yolo_box *boxes_dev, const int32_t *counts_dev, int batch, int max_boxes, const yolo_frame *frames_host, int mode,
                         int net_h, int net_w, void *stream) {
    return boxes_to_frames_any(boxes_dev, counts_dev, batch, max_boxes, frames_host, mode, net_h, net_w, stream, "yolo_boxes_to_frames");
}

int yolo_net_detect_frames_u8(yolo_net *net, const yolo_frame *frames_host, int batch, int mode, uint8_t *batch_dev, double threshold,
                              double iou_threshold, int nms_mode, yolo_box *boxes_dev, int32_t *counts_dev, int32_t *status_dev, void *stream) {
    const char *who = "yolo_net_detect_frames_u8";
    if (!frames_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    int rc = check_ready(net, batch_dev, batch, who);
    if (rc) return rc;
    if (!boxes_dev || !counts_dev || !status_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null output");
    const LayerInfo &in = net->layers[0];
    if (in.C != 3) return fail(YOLO_ERR_ARG, std::string(who) + ": the network input must have 3 channels");
    rc = frames_any(frames_host, batch, mode, batch_dev, true, in.H, in.W, stream, who);
    if (rc) return rc;
    rc = detect_any(net, NetIn{batch_dev, true}, batch, threshold, iou_threshold, nms_mode, boxes_dev, counts_dev, status_dev, stream, who);
    if (rc) return rc;
    return boxes_to_frames_any(boxes_dev, counts_dev, batch, net->opt.max_boxes, frames_host, mode, in.H, in.W, stream, who);
}

// ---- evaluation (yolo_hip.h: added within ABI 7; kernels in eval.hip) --------------------------------------------------------------
// every check here is made on the host, before any device call
static int check_eval_desc(const yolo_eval_desc *d, const char *who) {
    if (!d) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (d->n_classes < 1 || d->n_classes > YOLO_EVAL_MAX_CLASSES)
        return fail(YOLO_ERR_ARG, std::string(who) + ": n_classes must be 1.." + std::to_string(YOLO_EVAL_MAX_CLASSES));
    if (d->det_capacity < 1 || d->det_capacity > YOLO_EVAL_MAX_DET_CAPACITY)
        return fail(YOLO_ERR_ARG, std::string(who) + ": det_capacity must be 1.." + std::to_string(YOLO_EVAL_MAX_DET_CAPACITY));
    if (d->max_gt < 1 || d->max_gt > YOLO_EVAL_MAX_GT)
        return fail(YOLO_ERR_ARG, std::string(who) + ": max_gt must be 1.." + std::to_string(YOLO_EVAL_MAX_GT));
    if (!(d->match_iou >= 0. && d->match_iou <= 1.)) return fail(YOLO_ERR_ARG, std::string(who) + ": match_iou must be in [0, 1]");
    return YOLO_OK;
}

size_t yolo_eval_state_bytes(const yolo_eval_desc *desc) {
    if (check_eval_desc(desc, "yolo_eval_state_bytes")) return 0;
    return eval_layout(desc->n_classes, desc->det_capacity).total;
}

size_t yolo_eval_result_bytes(const yolo_eval_desc *desc) {
    if (check_eval_desc(desc, "yolo_eval_result_bytes")) return 0;
    return sizeof(yolo_eval_result) + sizeof(yolo_eval_class) * (size_t)desc->n_classes;
}

int yolo_eval_state_layout(const yolo_eval_desc *desc, yolo_eval_layout *out) {
    int rc = check_eval_desc(desc, "yolo_eval_state_layout");
    if (rc) return rc;
    if (!out) return fail(YOLO_ERR_ARG, "yolo_eval_state_layout: null argument");
    const EvalLayout L = eval_layout(desc->n_classes, desc->det_capacity);
    out->status_offset = L.header + offsetof(EvalHeader, status);
    out->n_gt_offset = L.n_gt; out->records_offset = L.records; out->sorted_offset = L.sorted;
    out->ctp_offset = L.ctp; out->cfp_offset = L.cfp; out->total_bytes = L.total;
    return YOLO_OK;
}

int yolo_eval_reset(const yolo_eval_desc *desc, void *state_dev, size_t state_bytes, void *stream) {
    int rc = check_eval_desc(desc, "yolo_eval_reset");
    if (rc) return rc;
    if (!state_dev) return fail(YOLO_ERR_ARG, "yolo_eval_reset: null argument");
    const EvalLayout L = eval_layout(desc->n_classes, desc->det_capacity);
    if (state_bytes < L.total) return fail(YOLO_ERR_ARG, "yolo_eval_reset: state too small (yolo_eval_state_bytes)");
    HIP_TRY(hipMemsetAsync(state_dev, 0, L.records, static_cast<hipStream_t>(stream)));      // header + n_gt: the records behind are unread until written
    return YOLO_OK;
}

int yolo_eval_add(const yolo_eval_desc *desc, void *state_dev, const yolo_box *boxes_dev, const int32_t *counts_dev, int batch, int max_boxes,
                  const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int64_t image_base, void *stream) {
    int rc = check_eval_desc(desc, "yolo_eval_add");
    if (rc) return rc;
    if (!state_dev || !boxes_dev || !counts_dev || !gt_dev || !gt_counts_dev) return fail(YOLO_ERR_ARG, "yolo_eval_add: null argument");
    if (batch < 1 || max_boxes < 1) return fail(YOLO_ERR_ARG, "yolo_eval_add: batch and max_boxes must be at least 1");
    if (image_base < 0) return fail(YOLO_ERR_ARG, "yolo_eval_add: image_base must not be negative");
    if (image_base > (int64_t)1 << 32 || (unsigned long long)(image_base + batch) * (unsigned long long)max_boxes > (1ull << 32))
        return fail(YOLO_ERR_ARG, "yolo_eval_add: (image_base + batch) * max_boxes does not fit 32 bits (seq)");
    const EvalLayout L = eval_layout(desc->n_classes, desc->det_capacity);
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    EvalMatchParams p;
    p.boxes = boxes_dev; p.counts = counts_dev; p.gt = gt_dev; p.gt_counts = gt_counts_dev;
    p.max_boxes = max_boxes; p.max_gt = desc->max_gt; p.n_classes = desc->n_classes; p.det_capacity = desc->det_capacity;
    p.match_iou = desc->match_iou;
    p.seq_base = (unsigned)((unsigned long long)image_base * (unsigned long long)max_boxes);
    p.hdr = reinterpret_cast<EvalHeader *>(st + L.header);
    p.n_gt = reinterpret_cast<int *>(st + L.n_gt);
    p.records = reinterpret_cast<yolo_eval_record *>(st + L.records);
    HIP_TRY(launch_eval_match(p, batch, static_cast<hipStream_t>(stream)));
    return YOLO_OK;
}

int yolo_eval_finish(const yolo_eval_desc *desc, void *state_dev, void *result_dev, void *stream) {
    int rc = check_eval_desc(desc, "yolo_eval_finish");
    if (rc) return rc;
    if (!state_dev || !result_dev) return fail(YOLO_ERR_ARG, "yolo_eval_finish: null argument");
    const EvalLayout L = eval_layout(desc->n_classes, desc->det_capacity);
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    EvalFinishParams p;
    p.hdr = reinterpret_cast<EvalHeader *>(st + L.header);
    p.n_gt = reinterpret_cast<const int *>(st + L.n_gt);
    p.records = reinterpret_cast<const yolo_eval_record *>(st + L.records);
    p.sorted = reinterpret_cast<yolo_eval_record *>(st + L.sorted);
    p.ctp = reinterpret_cast<unsigned *>(st + L.ctp);
    p.cfp = reinterpret_cast<unsigned *>(st + L.cfp);
    p.entries = reinterpret_cast<EvalEntry *>(st + L.entries);
    p.n2 = L.n2; p.n_classes = desc->n_classes; p.det_capacity = desc->det_capacity;
    p.result = static_cast<yolo_eval_result *>(result_dev);
    HIP_TRY(launch_eval_finish(p, static_cast<hipStream_t>(stream)));
    return YOLO_OK;
}

// ---- YOLOv2 loss (yolo_hip.h: added within ABI 7; kernels in loss.hip) -----------------------------------------------------------------
int yolo_v2_loss(const yolo_head_desc *head, const float *logits_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev,
                 int max_gt, yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, void *stream) {
    if (!logits_dev) return fail(YOLO_ERR_ARG, "yolo_v2_loss: null argument");
    int rc = check_loss_args(head, gt_dev, gt_counts_dev, max_gt, images_dev, result_dev, "yolo_v2_loss");
    if (rc) return rc;
    if (batch < 1) return fail(YOLO_ERR_ARG, "yolo_v2_loss: batch must be at least 1");
    return run_loss(*head, logits_dev, batch, gt_dev, gt_counts_dev, max_gt, images_dev, assign_dev, result_dev, static_cast<hipStream_t>(stream));
}

int yolo_v2_loss_grad(const yolo_head_desc *head, const float *logits_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev,
                      int max_gt, yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, float *grad_dev, void *stream) {
    if (!logits_dev || !assign_dev || !grad_dev) return fail(YOLO_ERR_ARG, "yolo_v2_loss_grad: null argument");
    int rc = check_loss_args(head, gt_dev, gt_counts_dev, max_gt, images_dev, result_dev, "yolo_v2_loss_grad");
    if (rc) return rc;
    if (batch < 1) return fail(YOLO_ERR_ARG, "yolo_v2_loss_grad: batch must be at least 1");
    if (grad_dev == logits_dev) return fail(YOLO_ERR_ARG, "yolo_v2_loss_grad: grad_dev must not be logits_dev (the gradient is not computed in place)");
    return run_loss_grad(*head, logits_dev, batch, gt_dev, gt_counts_dev, max_gt, images_dev, assign_dev, result_dev, grad_dev,
                         static_cast<hipStream_t>(stream));
}

static int net_loss_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                        yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, void *stream, const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    std::string err;        // whether a head was set at all comes before what kind of head it is
    int rc = check_head(&net->head, net->out_count, err);
    if (rc) return fail(YOLO_ERR_STATE, std::string(who) + ": head geometry not set (" + err + "); call yolo_net_set_head");
    rc = check_loss_args(&net->head, gt_dev, gt_counts_dev, max_gt, images_dev, result_dev, who);
    if (rc) return rc;
    if (batch < 1) return fail(YOLO_ERR_ARG, std::string(who) + ": batch must be at least 1");
    rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // a DENSE pass into the workspace logits (obj_min_logit is -inf outside detect_any: every row is written)
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    rc = run_forward(net, in_dev, batch, logits, s);
    if (rc) return rc;
    return run_loss(net->head, logits, batch, gt_dev, gt_counts_dev, max_gt, images_dev, assign_dev, result_dev, s);
}
int yolo_net_loss(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                  yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, void *stream) {
    return net_loss_any(net, NetIn{in_dev, false}, batch, gt_dev, gt_counts_dev, max_gt, images_dev, assign_dev, result_dev, stream, "yolo_net_loss");
}
int yolo_net_loss_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                     yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev, void *stream) {
    return net_loss_any(net, NetIn{in_dev, true}, batch, gt_dev, gt_counts_dev, max_gt, images_dev, assign_dev, result_dev, stream, "yolo_net_loss_u8");
}

int yolo_loss_reduce(const yolo_loss_image *images_dev, int n_images, int n_repeat, int batch_size, yolo_loss_result *result_dev, void *stream) {
    if (!images_dev || !result_dev) return fail(YOLO_ERR_ARG, "yolo_loss_reduce: null argument");
    if (n_images < 1 || batch_size < 1) return fail(YOLO_ERR_ARG, "yolo_loss_reduce: n_images and batch_size must be at least 1");
    if (n_repeat < 0 || n_repeat > n_images) return fail(YOLO_ERR_ARG, "yolo_loss_reduce: n_repeat must be 0..n_images");
    HIP_TRY(launch_loss_finish(LossFinishParams{images_dev, n_images, n_repeat, batch_size, result_dev}, static_cast<hipStream_t>(stream)));
    return YOLO_OK;
}

// ---- YOLOv3 loss (yolo_hip.h: added within ABI 7; kernels in loss3.hip, geometry and checks in loss3_host.cpp) -----------------------------
int yolo_v3_loss_rows(const yolo_head_desc *head, int64_t *rows_per_image, int32_t *parts_per_image) {
    if (!head || !rows_per_image || !parts_per_image) return fail(YOLO_ERR_ARG, "yolo_v3_loss_rows: null argument");
    Loss3Geometry geo;
    std::string err;
    const int rc = loss3_geometry(head, &geo, err);
    if (rc) return fail(rc, "yolo_v3_loss_rows: " + err);
    *rows_per_image = geo.rows;
    *parts_per_image = geo.parts;
    return YOLO_OK;
}

int yolo_v3_loss(const yolo_head_desc *head, const float *logits_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                 double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev, yolo_loss_result *result_dev,
                 void *stream) {
    Loss3Geometry geo;
    std::string err;
    const int rc = loss3_check(head, logits_dev, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts_dev, images_dev, assign_dev, result_dev,
                               false, nullptr, &geo, err);
    if (rc) return fail(rc, "yolo_v3_loss: " + err);
    return run_loss3(geo, logits_dev, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts_dev, images_dev, assign_dev, result_dev, nullptr,
                     static_cast<hipStream_t>(stream));
}

int yolo_v3_loss_grad(const yolo_head_desc *head, const float *logits_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                      double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev,
                      yolo_loss_result *result_dev, float *grad_dev, void *stream) {
    Loss3Geometry geo;
    std::string err;
    const int rc = loss3_check(head, logits_dev, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts_dev, images_dev, assign_dev, result_dev,
                               true, grad_dev, &geo, err);
    if (rc) return fail(rc, "yolo_v3_loss_grad: " + err);
    return run_loss3(geo, logits_dev, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts_dev, images_dev, assign_dev, result_dev, grad_dev,
                     static_cast<hipStream_t>(stream));
}

static int net_loss_v3_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                           double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev,
                           yolo_loss_result *result_dev, void *stream, const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    std::string err;        // whether a head was set at all comes before what kind of head it is
    int rc = check_head(&net->head, net->out_count, err);
    if (rc) return fail(YOLO_ERR_STATE, std::string(who) + ": head geometry not set (" + err + "); call yolo_net_set_head");
    Loss3Geometry geo;
    // (the logits pointer is the workspace's: any non-null value stands in for it until check_ready has seen the net)
    rc = loss3_check(&net->head, net, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts_dev, images_dev, assign_dev, result_dev, false,
                     nullptr, &geo, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // a DENSE pass into the workspace logits (obj_min_logit is -inf outside detect_any: every row is written)
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    rc = run_forward(net, in_dev, batch, logits, s);
    if (rc) return rc;
    return run_loss3(geo, logits, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts_dev, images_dev, assign_dev, result_dev, nullptr, s);
}
int yolo_net_loss_v3(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                     double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev,
                     yolo_loss_result *result_dev, void *stream) {
    return net_loss_v3_any(net, NetIn{in_dev, false}, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts_dev, images_dev, assign_dev,
                           result_dev, stream, "yolo_net_loss_v3");
}
int yolo_net_loss_v3_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                        double ignore_thresh, yolo_loss_image *parts_dev, yolo_loss_image *images_dev, int32_t *assign_dev,
                        yolo_loss_result *result_dev, void *stream) {
    return net_loss_v3_any(net, NetIn{in_dev, true}, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts_dev, images_dev, assign_dev,
                           result_dev, stream, "yolo_net_loss_v3_u8");
}

// ---- training augmentation (augment_host.cpp: checks, records, truths; augment.hip: the kernel)
int yolo_augment_check(const yolo_augment_image *params, int h, int w) {
    std::string err;
    const int rc = augment_check(params, h, w, err);
    if (rc) return fail(rc, "yolo_augment_check: " + err);
    return YOLO_OK;
}

int yolo_augment_u8(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w, const yolo_augment_image *params_host, void *stream) {
    std::string err;
    const int rc = augment_call_check(src_dev, dst_dev, n, h, w, params_host, err);
    if (rc) return fail(rc, "yolo_augment_u8: " + err);
    const size_t img_bytes = (size_t)h * w * 3;
    AugmentParams p;
    memset(&p, 0, sizeof p);
    p.h = h; p.w = w;
    p.wide = (uintptr_t)dst_dev % 4 == 0;       // (an image is a multiple of 12 bytes: the alignment holds for every image)
    for (int i0 = 0; i0 < n; i0 += kAugPerLaunch) {
        const int m = n - i0 < kAugPerLaunch ? n - i0 : kAugPerLaunch;
        for (int i = 0; i < m; ++i) p.g[i] = augment_geom(params_host[i0 + i]);
        p.src = src_dev + (size_t)i0 * img_bytes;
        p.dst = dst_dev + (size_t)i0 * img_bytes;
        HIP_TRY(launch_augment(p, m, static_cast<hipStream_t>(stream)));
    }
    return YOLO_OK;
}

int yolo_augment_truths_host(const yolo_gt *in, int n_in, const yolo_augment_image *params, int h, int w, yolo_gt *out, int32_t *n_out) {
    std::string err;
    const int rc = augment_truths(in, n_in, params, h, w, out, n_out, err);
    if (rc) return fail(rc, "yolo_augment_truths_host: " + err);
    return YOLO_OK;
}

int yolo_augment_tile(int32_t *rows, int32_t *cols, int32_t *images_per_launch) {
    if (rows) *rows = kAugTileRows;
    if (cols) *cols = kAugTileCols;
    if (images_per_launch) *images_per_launch = kAugPerLaunch;
    return YOLO_OK;
}

// ---- anchor k-means (anchor_host.cpp: plan, checks, threshold; anchor.hip: the kernels)
int yolo_anchor_plan(const yolo_anchor_desc *desc, int64_t n, struct yolo_anchor_plan *out) {
    std::string err;
    const int rc = anchor_plan(desc, n, out, err);
    if (rc) return fail(rc, "yolo_anchor_plan: " + err);
    return YOLO_OK;
}

int yolo_anchor_kmeans(const yolo_anchor_desc *desc, const double *wh_dev, int64_t n, const double *init_dev, void *scratch_dev,
                       size_t scratch_bytes, void *result_dev, size_t result_bytes, int32_t *labels_dev, void *stream) {
    std::string err;
    const int rc = anchor_call_check(desc, wh_dev, n, init_dev, scratch_dev, scratch_bytes, result_dev, result_bytes, labels_dev, err);
    if (rc) return fail(rc, "yolo_anchor_kmeans: " + err);
    struct yolo_anchor_plan pl;
    anchor_plan(desc, n, &pl, err);
    hipStream_t s = static_cast<hipStream_t>(stream);
    AnchorParams p = anchor_params(*desc, pl, wh_dev, (int)n, init_dev, scratch_dev, result_dev, labels_dev);
    // nothing the scratch or the result held is read: the counts start at 0, every label of the iteration before at "none"
    HIP_TRY(hipMemsetAsync(p.prep, 0, sizeof(AnchorPrep), s));
    HIP_TRY(hipMemsetAsync(p.label8, 0xff, (size_t)pl.label_stride * (size_t)desc->n_init, s));
    HIP_TRY(hipMemsetAsync(result_dev, 0, (size_t)pl.result_bytes, s));
    HIP_TRY(launch_anchor(ANCHOR_PREPARE, p, s));
    AnchorPrep prep;
    HIP_TRY(hipMemcpyAsync(&prep, p.prep, sizeof prep, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    p.threshold = anchor_threshold(prep, desc->tolerate);
    HIP_TRY(launch_anchor(ANCHOR_INIT, p, s));
    if (!init_dev) {
        for (int round = 0; round < desc->k; ++round) {
            p.round = round;
            HIP_TRY(launch_anchor(ANCHOR_SEED_SUM, p, s));
            HIP_TRY(launch_anchor(ANCHOR_SEED_PICK, p, s));
        }
        p.round = 0;
    }
    // iterations in batches of `period`; between batches one word comes back: how many restarts have stopped.  At most max_iter
    // iterations are ever enqueued, after which the update kernel has stopped every restart.
    for (int issued = 0;;) {
        unsigned long long n_done = 0;
        HIP_TRY(hipMemcpyAsync(&n_done, &p.prep->n_done, sizeof n_done, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n_done >= (unsigned long long)desc->n_init || issued >= desc->max_iter) break;
        const int m = desc->max_iter - issued < pl.period ? desc->max_iter - issued : pl.period;
        for (int i = 0; i < m; ++i) {
            HIP_TRY(launch_anchor(ANCHOR_ASSIGN, p, s));
            HIP_TRY(launch_anchor(ANCHOR_UPDATE, p, s));
        }
        issued += m;
    }
    HIP_TRY(launch_anchor(ANCHOR_FINAL, p, s));
    HIP_TRY(launch_anchor(ANCHOR_FINISH, p, s));
    if (labels_dev) HIP_TRY(launch_anchor(ANCHOR_LABELS, p, s));
    HIP_TRY(hipStreamSynchronize(s));
    return YOLO_OK;
}

int yolo_u8_unit_table(float *out256) {
    if (!out256) return fail(YOLO_ERR_ARG, "yolo_u8_unit_table: null argument");
    for (unsigned u = 0; u < 256; ++u) out256[u] = u8_unit(u);     // the function the input kernels run on every byte
    return YOLO_OK;
}

int yolo_launch_caps(struct yolo_launch_caps *out) {
    if (!out) return fail(YOLO_ERR_ARG, "yolo_launch_caps: null argument");
    out->tap_stream_workgroups = kTapStreamGrid;
    out->stem_workgroups = kStemGrid;
    out->first_mfma_workgroups = kFirstMfmaGrid;
    out->aux_work_items = kAuxGrid * kAuxBlock;
    out->decode_rows = kDecodeGrid * kDecodeBlock;
    return YOLO_OK;
}

int yolo_nms_host(const double *xywh, const float *prob, const int32_t *class_idx, int n, double iou_threshold, int nms_mode,
                  int32_t *keep_idx, int32_t *n_keep) {
    if (n < 0 || !n_keep || (n && (!xywh || !prob || !class_idx || !keep_idx))) return fail(YOLO_ERR_ARG, "yolo_nms_host: null argument");
    *n_keep = 0;
    if (n == 0) return YOLO_OK;                      // base.py:196-197
    if (n > 65536) return fail(YOLO_ERR_OVERFLOW, "yolo_nms_host: more than 65536 boxes");
    std::vector<Candidate> c(n);
    for (int i = 0; i < n; ++i) {
        c[i].x = (float)xywh[4 * i]; c[i].y = (float)xywh[4 * i + 1]; c[i].w = xywh[4 * i + 2]; c[i].h = xywh[4 * i + 3];
        c[i].prob = prob[i]; c[i].cls = class_idx[i]; c[i].scan = (unsigned)i; c[i].pad_ = 0;
    }
    unsigned char *dev = nullptr;
    const size_t cb = sizeof(Candidate) * (size_t)n;
    struct { size_t boxes, idx, cnt, scratch; } L;      // candidates at 0 | boxes | kept indices | [count, kept, status] 256 B apart | NMS slab (only used above 4096 boxes)
    L.boxes = align256(cb); L.idx = L.boxes + align256(sizeof(yolo_box) * (size_t)n); L.cnt = L.idx + align256(sizeof(int) * (size_t)n); L.scratch = L.cnt + 768;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dev), L.scratch + nms_scratch_bytes(n)));
    unsigned char *d_c = dev, *d_b = dev + L.boxes, *d_i = dev + L.idx;
    int *d_cnt = reinterpret_cast<int *>(dev + L.cnt);
    int rc = YOLO_OK;
    do {
        if (hipMemcpy(d_c, c.data(), cb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_cnt, &n, sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { rc = fail(YOLO_ERR_HIP, "yolo_nms_host: H2D copy failed"); break; }
        NmsParams np;
        np.cand = reinterpret_cast<const Candidate *>(d_c);
        np.cand_count = d_cnt;
        np.reset_count = nullptr;
        np.cap = n; np.max_boxes = n; np.mode = nms_mode; np.iou_threshold = iou_threshold;
        np.boxes = reinterpret_cast<yolo_box *>(d_b);
        np.counts = d_cnt + 64; np.status = d_cnt + 128;
        np.keep_idx = reinterpret_cast<int *>(d_i);
        np.scratch = dev + L.scratch;
        np.scratch_stride = nms_scratch_bytes(n);
        hipError_t e = launch_nms(np, 1, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) { rc = fail(YOLO_ERR_HIP, std::string("yolo_nms_host: ") + hipGetErrorString(e)); break; }
        int kept = 0;
        if (hipMemcpy(&kept, d_cnt + 64, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(keep_idx, d_i, sizeof(int) * (size_t)kept, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(YOLO_ERR_HIP, "yolo_nms_host: D2H copy failed"); break; }
        *n_keep = kept;
    } while (0);
    (void)hipFree(dev);
    return rc;
}

}  // extern "C"

// C ABI of libyolo_hip.so (declared in include/yolo_hip.h): argument and state checks, then one call into the planner (plan.cpp), the
// forward engine (forward.cpp) or a launcher.  Decode + NMS, the frame, the evaluation, the loss, the head-training and the augmentation entries live here whole.  No exceptions cross the boundary.
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

static int check_head(const yolo_head_desc *h, size_t out_count, std::string &err) {
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

namespace {

int check_ready(yolo_net *net, const void *in, int batch, const char *who) {
    if (!net || !in) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (batch <= 0 || batch > net->opt.max_batch) return fail(YOLO_ERR_ARG, std::string(who) + ": batch outside 1..max_batch");
    if (!net->weights_loaded && net->weight_count) return fail(YOLO_ERR_STATE, std::string(who) + ": weights not loaded");
    if (!net->dev_ws) return fail(YOLO_ERR_STATE, std::string(who) + ": workspace not bound");
    return YOLO_OK;
}

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

static size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
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
// every check here is made on the host, before any device call
static int check_loss_args(const yolo_head_desc *head, const void *gt_dev, const void *gt_counts_dev, int max_gt, const void *images_dev,
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
static int run_loss_grad(const yolo_head_desc &h, const float *logits, int batch, const yolo_gt *gt, const int32_t *gt_counts, int max_gt,
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

static int run_loss3(const Loss3Geometry &geo, const float *logits, int batch, const yolo_gt *gt, const int32_t *gt_counts, int max_gt,
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

// ---- training the detection layer (yolo_hip.h: added within ABI 7; kernels in train.hip, split and checks in train_host.cpp) ---------------
int yolo_wgrad_plan(int64_t P, int cin, int cout, int x_dtype, struct yolo_wgrad_plan *out) {
    std::string err;
    const int rc = wgrad_plan(P, cin, cout, x_dtype, out, err);
    return rc ? fail(rc, "yolo_wgrad_plan: " + err) : YOLO_OK;
}

static int run_wgrad(const void *x, int x_dtype, int ld, int coff, long long image_stride, int ppi, int batch, int cin, const float *g, int cout,
                     float *dw, float *db, void *scratch, const struct yolo_wgrad_plan &pl, hipStream_t s) {
    WgradParams p;
    memset(&p, 0, sizeof p);
    p.x = x; p.g = g; p.slab = static_cast<float *>(scratch); p.dw = dw; p.db = db;
    p.P = ppi * batch; p.cin = cin; p.cout = cout; p.ld = ld; p.coff = coff; p.ppi = ppi; p.img_stride = image_stride;
    p.ppc = pl.positions_per_chunk; p.n_chunks = pl.n_chunks; p.tiles_cout = pl.tiles_cout; p.tiles_cin = pl.tiles_cin;
    p.slab_stride = cout * (cin + 1);
    HIP_TRY(launch_head_wgrad(p, x_dtype, s));
    return YOLO_OK;
}

int yolo_conv1x1_wgrad(const void *x_dev, int x_dtype, int ld, int coff, int64_t image_stride, int positions_per_image, int batch, int cin,
                       const float *g_dev, int cout, float *dw_dev, float *db_dev, void *scratch_dev, size_t scratch_bytes, void *stream) {
    std::string err;
    struct yolo_wgrad_plan pl;
    const int rc = wgrad_check(x_dev, x_dtype, ld, coff, image_stride, positions_per_image, batch, cin, g_dev, cout, dw_dev, db_dev, scratch_dev,
                               scratch_bytes, &pl, err);
    if (rc) return fail(rc, "yolo_conv1x1_wgrad: " + err);
    return run_wgrad(x_dev, x_dtype, ld, coff, image_stride, positions_per_image, batch, cin, g_dev, cout, dw_dev, db_dev, scratch_dev, pl,
                     static_cast<hipStream_t>(stream));
}

int yolo_adam_step(float *w, float *b, float *m_w, float *v_w, float *m_b, float *v_b, const float *dw, const float *db, int64_t n_w,
                   int64_t n_b, float lr_t, float beta1, float beta2, float eps, void *stream) {
    std::string err;
    const int rc = adam_check(w, b, m_w, v_w, m_b, v_b, dw, db, n_w, n_b, lr_t, beta1, beta2, eps, err);
    if (rc) return fail(rc, "yolo_adam_step: " + err);
    AdamParams p;
    memset(&p, 0, sizeof p);
    p.w = w; p.b = b; p.m_w = m_w; p.v_w = v_w; p.m_b = m_b; p.v_b = v_b; p.dw = dw; p.db = db; p.n_w = n_w; p.n_b = n_b;
    p.lr_t = lr_t; p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
    HIP_TRY(launch_adam_step(p, static_cast<hipStream_t>(stream)));
    return YOLO_OK;
}

// ---- the data gradient of the detection layer and the 3 x 3 weight gradient (yolo_hip.h: added within ABI 7; kernels in train_tail.hip, split
//      and checks in train_tail_host.cpp)
static int run_dgrad(const float *g, int cout, const float *w, int cin, const void *y, int y_dtype, int ld, int coff, long long image_stride, int ppi,
                     int batch, float slope, float *d, long long tiles, hipStream_t s) {
    DgradParams p;
    memset(&p, 0, sizeof p);
    p.g = g; p.w = w; p.y = y; p.d = d;
    p.P = ppi * batch; p.cin = cin; p.cout = cout; p.ppi = ppi;
    if (y) { p.ld = ld; p.coff = coff; p.img_stride = image_stride; }
    p.tiles_cin = (cin + kDgradTileCin - 1) / kDgradTileCin;
    p.slope = slope;
    HIP_TRY(launch_conv1x1_dgrad(p, y_dtype, tiles, s));
    return YOLO_OK;
}

int yolo_conv1x1_dgrad(const float *g_dev, int cout, const float *w_dev, int cin, const void *y_dev, int y_dtype, int ld, int coff,
                       int64_t image_stride, int positions_per_image, int batch, float slope, float *d_dev, void *stream) {
    std::string err;
    long long tiles = 0;
    const int rc = dgrad_check(g_dev, cout, w_dev, cin, y_dev, y_dtype, ld, coff, image_stride, positions_per_image, batch, slope, d_dev, &tiles, err);
    if (rc) return fail(rc, "yolo_conv1x1_dgrad: " + err);
    return run_dgrad(g_dev, cout, w_dev, cin, y_dev, y_dtype, ld, coff, image_stride, positions_per_image, batch, slope, d_dev, tiles,
                     static_cast<hipStream_t>(stream));
}

int yolo_conv3x3_wgrad_plan(int h, int w, int batch, int cin, int cout, int x_dtype, struct yolo_conv3x3_wgrad_plan *out) {
    std::string err;
    const int rc = wgrad3x3_plan(h, w, batch, cin, cout, x_dtype, out, err);
    return rc ? fail(rc, "yolo_conv3x3_wgrad_plan: " + err) : YOLO_OK;
}

static int run_wgrad3x3(const void *x, int x_dtype, int ld, int coff, long long image_stride, int h, int w, int batch, int cin, const float *d, int cout,
                        const float *scale, float *dw, float *db, void *scratch, const struct yolo_conv3x3_wgrad_plan &pl, hipStream_t s) {
    Wgrad3x3Params p;
    memset(&p, 0, sizeof p);
    p.x = x; p.d = d; p.scale = scale; p.slab = static_cast<float *>(scratch); p.dw = dw; p.db = db;
    p.P = h * w * batch; p.cin = cin; p.cout = cout; p.ld = ld; p.coff = coff; p.h = h; p.w = w; p.ppi = h * w; p.img_stride = image_stride;
    p.ppc = pl.positions_per_chunk; p.n_chunks = pl.n_chunks; p.tiles_cout = pl.tiles_cout; p.tiles_cin = pl.tiles_cin; p.halo_rows = pl.halo_rows;
    p.slab_stride = cout * (9 * cin + 1);
    HIP_TRY(launch_conv3x3_wgrad(p, x_dtype, s));
    return YOLO_OK;
}

int yolo_conv3x3_wgrad(const void *x_dev, int x_dtype, int ld, int coff, int64_t image_stride, int h, int w, int batch, int cin,
                       const float *d_dev, int cout, const float *scale_dev, float *dw_dev, float *db_dev, void *scratch_dev,
                       size_t scratch_bytes, void *stream) {
    std::string err;
    struct yolo_conv3x3_wgrad_plan pl;
    const int rc = wgrad3x3_check(x_dev, x_dtype, ld, coff, image_stride, h, w, batch, cin, d_dev, cout, scale_dev, dw_dev, db_dev, scratch_dev,
                                  scratch_bytes, &pl, err);
    if (rc) return fail(rc, "yolo_conv3x3_wgrad: " + err);
    return run_wgrad3x3(x_dev, x_dtype, ld, coff, image_stride, h, w, batch, cin, d_dev, cout, scale_dev, dw_dev, db_dev, scratch_dev, pl,
                        static_cast<hipStream_t>(stream));
}

// ---- the weight gradient of the YOLOv3 head convs (yolo_hip.h: added within ABI 7; kernels in train3.hip, split and checks in train3_host.cpp)
int yolo_v3_head_wgrad_plan(const yolo_head_desc *head, const int32_t *cin, int batch, int x_dtype, struct yolo_v3_wgrad_plan *out) {
    std::string err;
    Wgrad3Geometry geo;
    const int rc = wgrad3_plan(head, cin, batch, x_dtype, out, &geo, err);
    return rc ? fail(rc, "yolo_v3_head_wgrad_plan: " + err) : YOLO_OK;
}

static int run_wgrad3(const Wgrad3Geometry &geo, const struct yolo_v3_wgrad_plan &pl, int batch, const float *g, const int32_t *assign, int max_gt,
                      void *scratch, hipStream_t s) {
    Wgrad3Params p;
    memset(&p, 0, sizeof p);
    static_cast<Wgrad3Geometry &>(p) = geo;
    p.g = g; p.assign = assign; p.batch = batch; p.max_gt = max_gt;
    p.slot = reinterpret_cast<int *>(static_cast<unsigned char *>(scratch) + pl.slot_offset);
    HIP_TRY(launch_head3_wgrad(p, s));
    return YOLO_OK;
}

int yolo_v3_head_wgrad(const yolo_head_desc *head, const struct yolo_v3_wgrad_view *views, int batch, const float *g_dev,
                       const int32_t *assign_dev, int max_gt, float *const *dw_dev, float *const *db_dev, void *scratch_dev,
                       size_t scratch_bytes, void *stream) {
    std::string err;
    struct yolo_v3_wgrad_plan pl;
    Wgrad3Geometry geo;
    const int rc = wgrad3_check(head, views, batch, g_dev, assign_dev, max_gt, dw_dev, db_dev, scratch_dev, scratch_bytes, &pl, &geo, err);
    if (rc) return fail(rc, "yolo_v3_head_wgrad: " + err);
    return run_wgrad3(geo, pl, batch, g_dev, assign_dev, max_gt, scratch_dev, static_cast<hipStream_t>(stream));
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

// The detection layer of a net: the last kernel of the plan, if it is the 1 x 1 / stride 1 linear conv with bias that writes the logits
// from a tensor of the workspace (plan.cpp; net/v2.py:52-56).  The message says what is in the way.
static int head_conv(const yolo_net *net, const Kernel **out, const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (net->kernels.empty()) return fail(YOLO_ERR_ARG, std::string(who) + ": the plan has no kernels");
    const Kernel &k = net->kernels.back();
    if (k.kind != K_CONV || k.ksize != 1 || k.stride != 1 || k.leaky || k.batch_norm || k.out.buf != BUF_USER_OUT || !k.out.f32 || k.has_res || k.outmode != OUT_NORMAL)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the last kernel of the plan must be the detection layer, a 1 x 1 / stride 1 linear conv with "
                                                     "bias and no batch norm that writes the logits (the YOLOv2 networks; v3 heads are not trained)");
    if (k.stem || k.fuse2_prev || k.mx || k.in.buf < 0 || k.in.f32 || k.in.base)
        return fail(YOLO_ERR_STATE, std::string(who) + ": the plan has fused the detection layer's input away");
    if (k.cin % 8 || k.cin_s != k.cin) return fail(YOLO_ERR_ARG, std::string(who) + ": the detection layer's input channels must be a multiple of 8");
    if (net->parts != 1)
        return fail(YOLO_ERR_STATE, std::string(who) + ": this net runs a batch as " + std::to_string(net->parts) +
                                        " stream parts, each in its own arena; call yolo_net_set_streams(net, 1)");
    *out = &k;
    return YOLO_OK;
}

int yolo_net_head_input(const yolo_net *net, yolo_tensor_view *out) {
    const Kernel *k = nullptr;
    int rc = head_conv(net, &k, "yolo_net_head_input");
    if (rc) return rc;
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_head_input: null argument");
    memset(out, 0, sizeof *out);
    out->offset = net->buffers[k->in.buf].offset;
    out->image_stride = k->in.img_stride;
    out->ld = k->in.ld; out->coff = k->in.coff;
    out->dtype = net->opt.dtype == YOLO_DTYPE_F16 ? YOLO_DTYPE_F16 : YOLO_DTYPE_F32;
    out->cin = k->cin; out->h = k->in.H; out->w = k->in.W;
    return YOLO_OK;
}

static int head_train_layout(const yolo_net *net, const Kernel **kout, yolo_head_train_layout *L, struct yolo_wgrad_plan *pl, const char *who) {
    const Kernel *k = nullptr;
    int rc = head_conv(net, &k, who);
    if (rc) return rc;
    std::string err;
    rc = check_head(&net->head, net->out_count, err);
    if (rc) return fail(YOLO_ERR_STATE, std::string(who) + ": head geometry not set (" + err + "); call yolo_net_set_head");
    if (net->head.version != 2 || net->head.n_scales != 1)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the head must be version 2 with one scale (the reference has a loss for YOLOv2 only)");
    const size_t mb = (size_t)net->opt.max_batch, hw = (size_t)k->in.H * k->in.W;
    rc = wgrad_plan((long long)(mb * hw), k->cin, k->cout, net->opt.dtype == YOLO_DTYPE_F16 ? YOLO_DTYPE_F16 : YOLO_DTYPE_F32, pl, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    const size_t nw = (size_t)k->cout * k->cin * 4, nb = (size_t)k->cout * 4;
    size_t off = 0;
    auto part = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return (uint64_t)at; };
    memset(L, 0, sizeof *L);
    L->w_offset = part(nw); L->b_offset = part(nb);
    L->m_w_offset = part(nw); L->v_w_offset = part(nw); L->m_b_offset = part(nb); L->v_b_offset = part(nb);
    L->dw_offset = part(nw); L->db_offset = part(nb);
    L->grad_offset = part(mb * net->out_count * 4);
    L->assign_offset = part(mb * hw * 4);
    L->images_offset = part(mb * sizeof(yolo_loss_image));
    // a smaller batch never needs more chunks than the full one at the same tile counts, but its chunks may be laid out otherwise:
    // the scratch is sized for the largest split of any batch up to max_batch
    uint64_t need = pl->scratch_bytes;
    for (size_t b = 1; b < mb; ++b) {
        struct yolo_wgrad_plan q;
        if (wgrad_plan((long long)(b * hw), k->cin, k->cout, YOLO_DTYPE_F32, &q, err) == YOLO_OK && q.scratch_bytes > need) need = q.scratch_bytes;
    }
    L->scratch_bytes = need;
    L->scratch_offset = part((size_t)need);
    L->total_bytes = off;
    L->cin = k->cin; L->cout = k->cout;
    if (kout) *kout = k;
    return YOLO_OK;
}

int yolo_net_head_train_layout(const yolo_net *net, yolo_head_train_layout *out) {
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_head_train_layout: null argument");
    struct yolo_wgrad_plan pl;
    return head_train_layout(net, nullptr, out, &pl, "yolo_net_head_train_layout");
}

size_t yolo_net_head_train_bytes(const yolo_net *net) {
    yolo_head_train_layout L;
    struct yolo_wgrad_plan pl;
    if (head_train_layout(net, nullptr, &L, &pl, "yolo_net_head_train_bytes")) return 0;
    return (size_t)L.total_bytes;
}

int yolo_net_head_train_init(yolo_net *net, void *state_dev, size_t bytes, const float *head_w_host, const float *head_b_host) {
    const char *who = "yolo_net_head_train_init";
    if (!net || !state_dev || !head_w_host || !head_b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_head_train_layout L;
    struct yolo_wgrad_plan pl;
    const Kernel *k = nullptr;
    int rc = head_train_layout(net, &k, &L, &pl, who);
    if (rc) return rc;
    if (bytes < L.total_bytes) return fail(YOLO_ERR_ARG, std::string(who) + ": state too small (yolo_net_head_train_bytes)");
    if ((uintptr_t)state_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the state must be 256-byte aligned");
    if (!net->weights_loaded || !net->dev_weights) return fail(YOLO_ERR_STATE, std::string(who) + ": weights not loaded");
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    const size_t nw = (size_t)k->cout * k->cin * 4, nb = (size_t)k->cout * 4;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(st + L.w_offset, head_w_host, nw, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + L.b_offset, head_b_host, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(st + L.m_w_offset, 0, (size_t)(L.dw_offset - L.m_w_offset)));       // the four moment arrays lie one behind the other
    // the layer's packed form, as pack_weights (weights.cpp) writes a 1 x 1 conv without batch norm: row o at o * wrow bytes, bias as it is
    const size_t wrow = (size_t)k->ktiles * 128;
    const bool f16 = net->opt.dtype == YOLO_DTYPE_F16;
    std::vector<unsigned char> rows((size_t)k->cout * wrow, 0);
    for (int o = 0; o < k->cout; ++o)
        for (int c = 0; c < k->cin; ++c) {
            const float v = head_w_host[(size_t)o * k->cin + c];
            if (f16) reinterpret_cast<_Float16 *>(rows.data() + (size_t)o * wrow)[c] = (_Float16)v;
            else reinterpret_cast<float *>(rows.data() + (size_t)o * wrow)[c] = v;
        }
    HIP_TRY(hipMemcpy(net->dev_weights + k->w_off, rows.data(), rows.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(net->dev_weights + k->b_off, head_b_host, nb, hipMemcpyHostToDevice));
    return YOLO_OK;
}

int yolo_net_head_train_read(yolo_net *net, const void *state_dev, float *w_host, float *b_host) {
    const char *who = "yolo_net_head_train_read";
    if (!net || !state_dev || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_head_train_layout L;
    struct yolo_wgrad_plan pl;
    const Kernel *k = nullptr;
    int rc = head_train_layout(net, &k, &L, &pl, who);
    if (rc) return rc;
    const unsigned char *st = static_cast<const unsigned char *>(state_dev);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(w_host, st + L.w_offset, (size_t)k->cout * k->cin * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b_host, st + L.b_offset, (size_t)k->cout * 4, hipMemcpyDeviceToHost));
    return YOLO_OK;
}

static int train_head_step_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                               void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream, const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_head_train_layout L;
    struct yolo_wgrad_plan pl;
    const Kernel *k = nullptr;
    int rc = head_train_layout(net, &k, &L, &pl, who);
    if (rc) return rc;
    if (!state_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null state (yolo_net_head_train_init)");
    if ((uintptr_t)state_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the state must be 256-byte aligned");
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    yolo_loss_image *images = reinterpret_cast<yolo_loss_image *>(st + L.images_offset);
    rc = check_loss_args(&net->head, gt_dev, gt_counts_dev, max_gt, images, result_dev, who);
    if (rc) return rc;
    if (batch < 1) return fail(YOLO_ERR_ARG, std::string(who) + ": batch must be at least 1");
    rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    if (!(lr_t == lr_t)) return fail(YOLO_ERR_ARG, std::string(who) + ": lr_t is NaN");
    const int ppi = k->in.H * k->in.W;
    const int x_dtype = net->opt.dtype == YOLO_DTYPE_F16 ? YOLO_DTYPE_F16 : YOLO_DTYPE_F32;
    std::string err;
    rc = wgrad_plan((long long)ppi * batch, k->cin, k->cout, x_dtype, &pl, err);
    if (rc || pl.scratch_bytes > L.scratch_bytes) return fail(YOLO_ERR_ARG, std::string(who) + ": " + (rc ? err : std::string("weight-gradient scratch too small")));
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    float *grad = reinterpret_cast<float *>(st + L.grad_offset);
    float *dw = reinterpret_cast<float *>(st + L.dw_offset), *db = reinterpret_cast<float *>(st + L.db_offset);
    rc = run_forward(net, in_dev, batch, logits, s);        // dense: obj_min_logit is -inf outside detect_any
    if (rc) return rc;
    rc = run_loss_grad(net->head, logits, batch, gt_dev, gt_counts_dev, max_gt, images, reinterpret_cast<int32_t *>(st + L.assign_offset), result_dev, grad, s);
    if (rc) return rc;
    rc = run_wgrad(net->dev_ws + net->buffers[k->in.buf].offset, x_dtype, k->in.ld, k->in.coff, k->in.img_stride, ppi, batch, k->cin, grad, k->cout,
                   dw, db, st + L.scratch_offset, pl, s);
    if (rc) return rc;
    AdamParams p;
    memset(&p, 0, sizeof p);
    p.w = reinterpret_cast<float *>(st + L.w_offset); p.b = reinterpret_cast<float *>(st + L.b_offset);
    p.m_w = reinterpret_cast<float *>(st + L.m_w_offset); p.v_w = reinterpret_cast<float *>(st + L.v_w_offset);
    p.m_b = reinterpret_cast<float *>(st + L.m_b_offset); p.v_b = reinterpret_cast<float *>(st + L.v_b_offset);
    p.dw = dw; p.db = db; p.n_w = (long long)k->cout * k->cin; p.n_b = k->cout;
    p.lr_t = lr_t; p.beta1 = 0.9f; p.beta2 = 0.999f; p.eps = 1e-8f;        // tf.train.AdamOptimizer's defaults (net/v2.py:205)
    p.pack_w = net->dev_weights + k->w_off; p.pack_b = reinterpret_cast<float *>(net->dev_weights + k->b_off);
    p.pack_cin = k->cin; p.pack_f16 = x_dtype == YOLO_DTYPE_F16;
    p.pack_row = (int)((size_t)k->ktiles * 128 / (p.pack_f16 ? 2 : 4));
    HIP_TRY(launch_adam_step(p, s));
    return YOLO_OK;
}
int yolo_net_train_head_step(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                             void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_head_step_any(net, NetIn{in_dev, false}, batch, gt_dev, gt_counts_dev, max_gt, state_dev, lr_t, result_dev, stream, "yolo_net_train_head_step");
}
int yolo_net_train_head_step_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_head_step_any(net, NetIn{in_dev, true}, batch, gt_dev, gt_counts_dev, max_gt, state_dev, lr_t, result_dev, stream, "yolo_net_train_head_step_u8");
}

// ---- training the tail of a YOLOv2 net (yolo_hip.h: added within ABI 7; kernels in train.hip and train_tail.hip) ---------------------------
// The block behind the detection layer: the one kernel that writes the detection layer's input, if it is a 3 x 3 / stride 1 conv with batch
// norm and leaky ReLU that the plan runs on its own, from a tensor of the workspace that is still intact behind the last kernel of the
// pass.  The message says what is in the way.
static int tail_convs(const yolo_net *net, const Kernel **block, const Kernel **head, const char *who) {
    const Kernel *k = nullptr;
    int rc = head_conv(net, &k, who);
    if (rc) return rc;
    const std::vector<Kernel> &K = net->kernels;
    const int last = (int)K.size() - 1;
    if (k->out.base || (size_t)k->cout * k->in.H * k->in.W != net->out_count)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the last kernel writes one scale of several: a v3 network has no tail of this kind (its detection convs are "
                                                     "trained with yolo_net_train_head_step_v3, train_layers = heads)");
    int bi = -1, writers = 0;
    for (int j = 0; j < last; ++j)
        for (const View *v : {&K[j].out, &K[j].out2, &K[j].out3})
            if (v->buf == k->in.buf) { bi = j; ++writers; }
    const std::string at = std::string(who) + ": ";
    if (writers != 1)
        return fail(YOLO_ERR_ARG, at + "the detection layer's input is written by " + std::to_string(writers) + " kernels (a concatenation or the network input): "
                                       "there is no single 3 x 3 block behind the detection layer");
    const Kernel &b = K[bi];
    if (b.kind != K_CONV || b.out.buf != k->in.buf)
        return fail(YOLO_ERR_ARG, at + "the detection layer's input is not written by a conv (kernel " + std::to_string(bi) + ")");
    if (b.ksize != 3 || b.stride != 1) return fail(YOLO_ERR_ARG, at + "the conv behind the detection layer must be 3 x 3 / stride 1 (1 x 1 and stride-2 blocks are not trained)");
    if (!b.batch_norm || !b.leaky) return fail(YOLO_ERR_ARG, at + "the conv behind the detection layer must have batch norm and a leaky ReLU");
    if (b.has_res) return fail(YOLO_ERR_ARG, at + "the conv behind the detection layer carries a residual (a shortcut is fused into it): its output is not the block's alone");
    if (b.mx) return fail(YOLO_ERR_STATE, at + "the plan runs the conv behind the detection layer as an MXFP8 conv: its packed weights are block-scaled fp8 (use an fp16 or fp32 plan)");
    if (b.outmode != OUT_NORMAL) return fail(YOLO_ERR_STATE, at + "the plan has fused a pool, reorg or upsample into the conv behind the detection layer");
    if (b.stem != STEM_NONE || b.fuse2_next || b.fuse2_prev) return fail(YOLO_ERR_STATE, at + "the plan has fused the conv behind the detection layer with a neighbour");
    if (b.out.coff != k->in.coff || b.out.ld != k->in.ld || b.out.img_stride != k->in.img_stride || b.out.base != k->in.base || b.cout != k->cin ||
        b.out.H != k->in.H || b.out.W != k->in.W || b.out.f32)
        return fail(YOLO_ERR_ARG, at + "the conv behind the detection layer does not write exactly the detection layer's input");
    if (b.in.buf < 0 || b.in.f32 || b.in.base) return fail(YOLO_ERR_STATE, at + "the input of the conv behind the detection layer is not a tensor of the workspace");
    if (b.cin % 8 || b.cin_s != b.cin) return fail(YOLO_ERR_ARG, at + "the input channels of the conv behind the detection layer must be a multiple of 8");
    if (b.in.W > kTailMaxW) return fail(YOLO_ERR_ARG, at + "the feature map of the conv behind the detection layer is wider than " + std::to_string(kTailMaxW));
    // intact behind the last kernel: nothing behind the block writes its input's buffer, and no buffer alive later shares its bytes
    const Buffer &bb = net->buffers[b.in.buf];
    for (int j = bi; j <= last; ++j)
        for (const View *v : {&K[j].out, &K[j].out2, &K[j].out3})
            if (v->buf == b.in.buf)
                return fail(YOLO_ERR_STATE, at + "the plan reuses the block's input: kernel " + std::to_string(j) + " writes its buffer");
    for (size_t q = 0; q < net->buffers.size(); ++q) {
        const Buffer &o = net->buffers[q];
        if ((int)q == b.in.buf || o.last < 0 || !o.bytes || !bb.bytes) continue;
        const bool shares = o.offset < bb.offset + bb.bytes && bb.offset < o.offset + o.bytes;
        if (shares && o.last >= bb.first)
            return fail(YOLO_ERR_STATE, at + "the plan reuses the block's input: buffer " + std::to_string(q) + " shares its bytes and is alive behind it");
    }
    *block = &b;
    *head = k;
    return YOLO_OK;
}

static void fill_view(const yolo_net *net, const Kernel *k, yolo_tensor_view *out) {
    memset(out, 0, sizeof *out);
    out->offset = net->buffers[k->in.buf].offset;
    out->image_stride = k->in.img_stride;
    out->ld = k->in.ld; out->coff = k->in.coff;
    out->dtype = net->opt.dtype == YOLO_DTYPE_F16 ? YOLO_DTYPE_F16 : YOLO_DTYPE_F32;
    out->cin = k->cin; out->h = k->in.H; out->w = k->in.W;
}

int yolo_net_tail_inputs(const yolo_net *net, yolo_tensor_view *block_in, yolo_tensor_view *head_in) {
    const Kernel *b = nullptr, *k = nullptr;
    int rc = tail_convs(net, &b, &k, "yolo_net_tail_inputs");
    if (rc) return rc;
    if (!block_in || !head_in) return fail(YOLO_ERR_ARG, "yolo_net_tail_inputs: null argument");
    fill_view(net, b, block_in);
    fill_view(net, k, head_in);
    return YOLO_OK;
}

static int tail_train_layout(const yolo_net *net, const Kernel **bout, const Kernel **kout, yolo_tail_train_layout *L, const char *who) {
    const Kernel *b = nullptr, *k = nullptr;
    int rc = tail_convs(net, &b, &k, who);
    if (rc) return rc;
    std::string err;
    rc = check_head(&net->head, net->out_count, err);
    if (rc) return fail(YOLO_ERR_STATE, std::string(who) + ": head geometry not set (" + err + "); call yolo_net_set_head");
    if (net->head.version != 2 || net->head.n_scales != 1)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the head must be version 2 with one scale (the reference has a loss for YOLOv2 only)");
    const size_t mb = (size_t)net->opt.max_batch, hw = (size_t)k->in.H * k->in.W;
    const size_t nw = (size_t)k->cout * k->cin * 4, nb = (size_t)k->cout * 4;
    const size_t nw3 = (size_t)b->cout * 9 * b->cin * 4, nb3 = (size_t)b->cout * 4;
    size_t off = 0;
    auto part = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return (uint64_t)at; };
    memset(L, 0, sizeof *L);
    L->w_offset = part(nw); L->b_offset = part(nb);
    L->m_w_offset = part(nw); L->v_w_offset = part(nw); L->m_b_offset = part(nb); L->v_b_offset = part(nb);
    L->dw_offset = part(nw); L->db_offset = part(nb);
    L->w3_offset = part(nw3); L->beta_offset = part(nb3);
    L->m_w3_offset = part(nw3); L->v_w3_offset = part(nw3); L->m_beta_offset = part(nb3); L->v_beta_offset = part(nb3);
    L->dw3_offset = part(nw3); L->dbeta_offset = part(nb3);
    L->scale64_offset = part((size_t)b->cout * 8); L->scale32_offset = part(nb3); L->mean_offset = part(nb3);
    L->d_offset = part(mb * hw * (size_t)b->cout * 4);
    L->grad_offset = part(mb * net->out_count * 4);
    L->assign_offset = part(mb * hw * 4);
    L->images_offset = part(mb * sizeof(yolo_loss_image));
    // one scratch for both weight gradients, which run one after the other: the largest split of either, of any batch up to max_batch
    uint64_t need = 0;
    for (size_t n = 1; n <= mb; ++n) {
        struct yolo_wgrad_plan q;
        struct yolo_conv3x3_wgrad_plan q3;
        rc = wgrad_plan((long long)(n * hw), k->cin, k->cout, YOLO_DTYPE_F32, &q, err);
        if (!rc) rc = wgrad3x3_plan(b->in.H, b->in.W, (int)n, b->cin, b->cout, YOLO_DTYPE_F32, &q3, err);
        if (rc) return fail(rc, std::string(who) + ": " + err);
        if (q.scratch_bytes > need) need = q.scratch_bytes;
        if (q3.scratch_bytes > need) need = q3.scratch_bytes;
    }
    L->scratch_bytes = need;
    L->scratch_offset = part((size_t)need);
    L->total_bytes = off;
    L->block_src = b->w_src; L->head_src = k->w_src;
    L->cin = k->cin; L->cout = k->cout; L->cin3 = b->cin; L->cout3 = b->cout;
    if (bout) *bout = b;
    if (kout) *kout = k;
    return YOLO_OK;
}

int yolo_net_tail_train_layout(const yolo_net *net, yolo_tail_train_layout *out) {
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_tail_train_layout: null argument");
    return tail_train_layout(net, nullptr, nullptr, out, "yolo_net_tail_train_layout");
}

size_t yolo_net_tail_train_bytes(const yolo_net *net) {
    yolo_tail_train_layout L;
    if (tail_train_layout(net, nullptr, nullptr, &L, "yolo_net_tail_train_bytes")) return 0;
    return (size_t)L.total_bytes;
}

int yolo_net_tail_train_init(yolo_net *net, void *state_dev, size_t bytes, const float *block_host, const float *head_w_host,
                             const float *head_b_host) {
    const char *who = "yolo_net_tail_train_init";
    if (!net || !state_dev || !block_host || !head_w_host || !head_b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_tail_train_layout L;
    const Kernel *b = nullptr, *k = nullptr;
    int rc = tail_train_layout(net, &b, &k, &L, who);
    if (rc) return rc;
    if (bytes < L.total_bytes) return fail(YOLO_ERR_ARG, std::string(who) + ": state too small (yolo_net_tail_train_bytes)");
    if ((uintptr_t)state_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the state must be 256-byte aligned");
    if (!net->weights_loaded || !net->dev_weights) return fail(YOLO_ERR_STATE, std::string(who) + ": weights not loaded");
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    const bool f16 = net->opt.dtype == YOLO_DTYPE_F16;
    const int c3 = b->cout, ci3 = b->cin;
    const size_t nw = (size_t)k->cout * k->cin * 4, nb = (size_t)k->cout * 4, nb3 = (size_t)c3 * 4;
    // the block: beta, gamma, mean, var, kernel[out][in][kh][kw] (net/layers.py:53-63); the fold as weights.cpp: fold_batch_norm
    const float *beta = block_host, *gamma = block_host + c3, *mean = block_host + 2 * (size_t)c3, *var = block_host + 3 * (size_t)c3;
    const float *kern = block_host + 4 * (size_t)c3;
    std::vector<double> scale64((size_t)c3);
    std::vector<float> scale32((size_t)c3), bfold((size_t)c3), w3((size_t)c3 * 9 * ci3);
    for (int o = 0; o < c3; ++o) {
        scale64[o] = (double)gamma[o] / std::sqrt((double)var[o] + 1e-5);
        scale32[o] = (float)scale64[o];
        bfold[o] = (float)((double)beta[o] - (double)mean[o] * scale64[o]);
    }
    const size_t wrow3 = (size_t)b->ktiles * 128;
    std::vector<unsigned char> rows3((size_t)c3 * wrow3, 0);
    for (int o = 0; o < c3; ++o)
        for (int t = 0; t < 9; ++t)
            for (int c = 0; c < ci3; ++c) {
                const float w = kern[((size_t)o * ci3 + c) * 9 + t];
                w3[((size_t)o * 9 + t) * ci3 + c] = w;
                // (fp16: one rounding from the float64 product, which is what pack_weights' (_Float16)(float) compiles to on the host)
                const double v = (double)w * scale64[o];
                const size_t e = (size_t)t * b->cin_s + c;
                if (f16) reinterpret_cast<_Float16 *>(rows3.data() + (size_t)o * wrow3)[e] = (_Float16)v;
                else reinterpret_cast<float *>(rows3.data() + (size_t)o * wrow3)[e] = (float)v;
            }
    if (rows3.size() > b->w_bytes) return fail(YOLO_ERR_PLAN, std::string(who) + ": the block's packed rows do not fit its weight region");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(st + L.w_offset, head_w_host, nw, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + L.b_offset, head_b_host, nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(st + L.m_w_offset, 0, (size_t)(L.dw_offset - L.m_w_offset)));       // the four moment arrays lie one behind the other
    HIP_TRY(hipMemcpy(st + L.w3_offset, w3.data(), w3.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + L.beta_offset, beta, nb3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(st + L.m_w3_offset, 0, (size_t)(L.dw3_offset - L.m_w3_offset)));
    HIP_TRY(hipMemcpy(st + L.scale64_offset, scale64.data(), (size_t)c3 * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + L.scale32_offset, scale32.data(), nb3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + L.mean_offset, mean, nb3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(net->dev_weights + b->w_off, rows3.data(), rows3.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(net->dev_weights + b->b_off, bfold.data(), nb3, hipMemcpyHostToDevice));
    // the head's packed form, as yolo_net_head_train_init writes it
    const size_t wrow = (size_t)k->ktiles * 128;
    std::vector<unsigned char> rows((size_t)k->cout * wrow, 0);
    for (int o = 0; o < k->cout; ++o)
        for (int c = 0; c < k->cin; ++c) {
            const float v = head_w_host[(size_t)o * k->cin + c];
            if (f16) reinterpret_cast<_Float16 *>(rows.data() + (size_t)o * wrow)[c] = (_Float16)v;
            else reinterpret_cast<float *>(rows.data() + (size_t)o * wrow)[c] = v;
        }
    HIP_TRY(hipMemcpy(net->dev_weights + k->w_off, rows.data(), rows.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(net->dev_weights + k->b_off, head_b_host, nb, hipMemcpyHostToDevice));
    return YOLO_OK;
}

int yolo_net_tail_train_read(yolo_net *net, const void *state_dev, float *block_kernel_host, float *beta_host, float *w_host, float *b_host) {
    const char *who = "yolo_net_tail_train_read";
    if (!net || !state_dev || !block_kernel_host || !beta_host || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_tail_train_layout L;
    const Kernel *b = nullptr, *k = nullptr;
    int rc = tail_train_layout(net, &b, &k, &L, who);
    if (rc) return rc;
    const unsigned char *st = static_cast<const unsigned char *>(state_dev);
    std::vector<float> w3((size_t)b->cout * 9 * b->cin);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(w3.data(), st + L.w3_offset, w3.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(beta_host, st + L.beta_offset, (size_t)b->cout * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(w_host, st + L.w_offset, (size_t)k->cout * k->cin * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b_host, st + L.b_offset, (size_t)k->cout * 4, hipMemcpyDeviceToHost));
    for (int o = 0; o < b->cout; ++o)
        for (int t = 0; t < 9; ++t)
            for (int c = 0; c < b->cin; ++c) block_kernel_host[((size_t)o * b->cin + c) * 9 + t] = w3[((size_t)o * 9 + t) * b->cin + c];
    return YOLO_OK;
}

static int train_tail_step_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                               void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream, const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_tail_train_layout L;
    const Kernel *b = nullptr, *k = nullptr;
    int rc = tail_train_layout(net, &b, &k, &L, who);
    if (rc) return rc;
    if (!state_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null state (yolo_net_tail_train_init)");
    if ((uintptr_t)state_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the state must be 256-byte aligned");
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    yolo_loss_image *images = reinterpret_cast<yolo_loss_image *>(st + L.images_offset);
    rc = check_loss_args(&net->head, gt_dev, gt_counts_dev, max_gt, images, result_dev, who);
    if (rc) return rc;
    if (batch < 1) return fail(YOLO_ERR_ARG, std::string(who) + ": batch must be at least 1");
    rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    if (!(lr_t == lr_t)) return fail(YOLO_ERR_ARG, std::string(who) + ": lr_t is NaN");
    const int ppi = k->in.H * k->in.W;
    const int x_dtype = net->opt.dtype == YOLO_DTYPE_F16 ? YOLO_DTYPE_F16 : YOLO_DTYPE_F32;
    auto f32 = [&](uint64_t o) { return reinterpret_cast<float *>(st + o); };
    float *grad = f32(L.grad_offset), *d = f32(L.d_offset);
    const void *y = net->dev_ws + net->buffers[k->in.buf].offset, *x3 = net->dev_ws + net->buffers[b->in.buf].offset;
    std::string err;
    struct yolo_wgrad_plan pl;
    struct yolo_conv3x3_wgrad_plan pl3;
    long long tiles = 0;
    rc = wgrad_check(y, x_dtype, k->in.ld, k->in.coff, k->in.img_stride, ppi, batch, k->cin, grad, k->cout, f32(L.dw_offset), f32(L.db_offset),
                     st + L.scratch_offset, (size_t)L.scratch_bytes, &pl, err);
    if (!rc) rc = dgrad_check(grad, k->cout, f32(L.w_offset), k->cin, y, x_dtype, k->in.ld, k->in.coff, k->in.img_stride, ppi, batch, 0.1f, d, &tiles, err);
    if (!rc) rc = wgrad3x3_check(x3, x_dtype, b->in.ld, b->in.coff, b->in.img_stride, b->in.H, b->in.W, batch, b->cin, d, b->cout, f32(L.scale32_offset),
                                 f32(L.dw3_offset), f32(L.dbeta_offset), st + L.scratch_offset, (size_t)L.scratch_bytes, &pl3, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    rc = run_forward(net, in_dev, batch, logits, s);        // dense: obj_min_logit is -inf outside detect_any
    if (rc) return rc;
    rc = run_loss_grad(net->head, logits, batch, gt_dev, gt_counts_dev, max_gt, images, reinterpret_cast<int32_t *>(st + L.assign_offset), result_dev, grad, s);
    if (rc) return rc;
    rc = run_wgrad(y, x_dtype, k->in.ld, k->in.coff, k->in.img_stride, ppi, batch, k->cin, grad, k->cout, f32(L.dw_offset), f32(L.db_offset),
                   st + L.scratch_offset, pl, s);
    if (rc) return rc;
    // the data gradient from the head's master kernel BEFORE its update, through the leaky ReLU's derivative at the stored Y
    rc = run_dgrad(grad, k->cout, f32(L.w_offset), k->cin, y, x_dtype, k->in.ld, k->in.coff, k->in.img_stride, ppi, batch, 0.1f, d, tiles, s);
    if (rc) return rc;
    rc = run_wgrad3x3(x3, x_dtype, b->in.ld, b->in.coff, b->in.img_stride, b->in.H, b->in.W, batch, b->cin, d, b->cout, f32(L.scale32_offset),
                      f32(L.dw3_offset), f32(L.dbeta_offset), st + L.scratch_offset, pl3, s);
    if (rc) return rc;
    AdamParams p;
    memset(&p, 0, sizeof p);
    p.w = f32(L.w_offset); p.b = f32(L.b_offset); p.m_w = f32(L.m_w_offset); p.v_w = f32(L.v_w_offset); p.m_b = f32(L.m_b_offset); p.v_b = f32(L.v_b_offset);
    p.dw = f32(L.dw_offset); p.db = f32(L.db_offset); p.n_w = (long long)k->cout * k->cin; p.n_b = k->cout;
    p.lr_t = lr_t; p.beta1 = 0.9f; p.beta2 = 0.999f; p.eps = 1e-8f;        // tf.train.AdamOptimizer's defaults (net/v2.py:205)
    p.pack_w = net->dev_weights + k->w_off; p.pack_b = reinterpret_cast<float *>(net->dev_weights + k->b_off);
    p.pack_cin = k->cin; p.pack_f16 = x_dtype == YOLO_DTYPE_F16;
    p.pack_row = (int)((size_t)k->ktiles * 128 / (p.pack_f16 ? 2 : 4));
    HIP_TRY(launch_adam_step(p, s));
    TailAdamParams q;
    memset(&q, 0, sizeof q);
    q.a = p;
    q.a.w = f32(L.w3_offset); q.a.b = f32(L.beta_offset); q.a.m_w = f32(L.m_w3_offset); q.a.v_w = f32(L.v_w3_offset);
    q.a.m_b = f32(L.m_beta_offset); q.a.v_b = f32(L.v_beta_offset); q.a.dw = f32(L.dw3_offset); q.a.db = f32(L.dbeta_offset);
    q.a.n_w = (long long)b->cout * 9 * b->cin; q.a.n_b = b->cout;
    q.a.pack_w = net->dev_weights + b->w_off; q.a.pack_b = reinterpret_cast<float *>(net->dev_weights + b->b_off);
    q.a.pack_cin = 9 * b->cin;                              // (cin_s == cin: element t * cin + c of a master row is element t * cin_s + c of the packed row)
    q.a.pack_row = (int)((size_t)b->ktiles * 128 / (p.pack_f16 ? 2 : 4));
    q.scale64 = reinterpret_cast<const double *>(st + L.scale64_offset); q.mean = f32(L.mean_offset);
    HIP_TRY(launch_tail_adam(q, s));
    return YOLO_OK;
}
int yolo_net_train_tail_step(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                             void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_tail_step_any(net, NetIn{in_dev, false}, batch, gt_dev, gt_counts_dev, max_gt, state_dev, lr_t, result_dev, stream, "yolo_net_train_tail_step");
}
int yolo_net_train_tail_step_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_tail_step_any(net, NetIn{in_dev, true}, batch, gt_dev, gt_counts_dev, max_gt, state_dev, lr_t, result_dev, stream, "yolo_net_train_tail_step_u8");
}

// ---- training the YOLOv3 head convs on a net (yolo_hip.h: added within ABI 7) -------------------------------------------------------------
// The head convs of a version 3 net in head order, each the 1 x 1 / stride 1 linear conv with bias that writes its scale of the logits from
// a tensor of the workspace that is still intact behind the last kernel of the pass.  The message says what is in the way.
static int head_convs_v3(const yolo_net *net, const Kernel *out[YOLO_MAX_SCALES], const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    std::string err;
    int rc = check_head(&net->head, net->out_count, err);
    if (rc) return fail(YOLO_ERR_STATE, std::string(who) + ": head geometry not set (" + err + "); call yolo_net_set_head");
    if (net->head.version != 3)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the head must be version 3 (yolo_net_train_head_step trains the detection layer of a YOLOv2 network)");
    const std::vector<Kernel> &K = net->kernels;
    std::vector<int> heads;
    for (int i = 0; i < (int)K.size(); ++i)
        if (K[i].kind == K_CONV && K[i].head) heads.push_back(i);
    std::sort(heads.begin(), heads.end(), [&](int a, int b) { return K[a].out.base < K[b].out.base; });       // head order = the order of the rows
    if ((int)heads.size() != net->head.n_scales)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the plan has " + std::to_string(heads.size()) + " head convs for " + std::to_string(net->head.n_scales) + " scales");
    const int width = 5 + net->head.n_classes;
    for (int s = 0; s < net->head.n_scales; ++s) {
        const int ki = heads[s];
        const Kernel &k = K[ki];
        const std::string at = std::string(who) + ": scale " + std::to_string(s) + ": ";
        if (k.ksize != 1 || k.stride != 1 || k.leaky || k.batch_norm || k.out.buf != BUF_USER_OUT || !k.out.f32 || k.has_res || k.outmode != OUT_NORMAL ||
            k.cout != net->head.n_anchors[s] * width || k.in.H != net->head.h[s] || k.in.W != net->head.w[s])
            return fail(YOLO_ERR_ARG, at + "the head conv must be a 1 x 1 / stride 1 linear conv with bias and no batch norm that writes this scale of the logits");
        if (k.stem || k.fuse2_prev || k.mx || k.in.buf < 0 || k.in.f32 || k.in.base)
            return fail(YOLO_ERR_STATE, at + "the plan has fused the head conv's input away");
        if (k.cin % 8 || k.cin_s != k.cin) return fail(YOLO_ERR_ARG, at + "the head conv's input channels must be a multiple of 8");
        // intact behind the last kernel: nothing behind the head conv writes its input's buffer, and no buffer alive later shares its bytes
        const Buffer &b = net->buffers[k.in.buf];
        for (int j = ki + 1; j < (int)K.size(); ++j)
            for (const View *v : {&K[j].out, &K[j].out2, &K[j].out3})
                if (v->buf == k.in.buf)
                    return fail(YOLO_ERR_STATE, at + "the plan reuses the head conv's input: kernel " + std::to_string(j) + " writes its buffer behind the head conv");
        for (size_t q = 0; q < net->buffers.size(); ++q) {
            const Buffer &o = net->buffers[q];
            if ((int)q == k.in.buf || o.last < 0 || !o.bytes || !b.bytes) continue;
            const bool shares = o.offset < b.offset + b.bytes && b.offset < o.offset + o.bytes;
            if (shares && o.last >= b.first)
                return fail(YOLO_ERR_STATE, at + "the plan reuses the head conv's input: buffer " + std::to_string(q) + " shares its bytes and is alive behind it");
        }
        out[s] = &k;
    }
    if (net->parts != 1)
        return fail(YOLO_ERR_STATE, std::string(who) + ": this net runs a batch as " + std::to_string(net->parts) +
                                        " stream parts, each in its own arena; call yolo_net_set_streams(net, 1)");
    return YOLO_OK;
}

static int net_x_dtype(const yolo_net *net) { return net->opt.dtype == YOLO_DTYPE_F16 ? YOLO_DTYPE_F16 : YOLO_DTYPE_F32; }

int yolo_net_head_inputs_v3(const yolo_net *net, yolo_tensor_view *out, int32_t *n) {
    const Kernel *ks[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    int rc = head_convs_v3(net, ks, "yolo_net_head_inputs_v3");
    if (rc) return rc;
    if (!out || !n) return fail(YOLO_ERR_ARG, "yolo_net_head_inputs_v3: null argument");
    *n = net->head.n_scales;
    for (int s = 0; s < net->head.n_scales; ++s) {
        const Kernel *k = ks[s];
        memset(&out[s], 0, sizeof out[s]);
        out[s].offset = net->buffers[k->in.buf].offset;
        out[s].image_stride = k->in.img_stride;
        out[s].ld = k->in.ld; out[s].coff = k->in.coff;
        out[s].dtype = net_x_dtype(net);
        out[s].cin = k->cin; out[s].h = k->in.H; out[s].w = k->in.W;
    }
    return YOLO_OK;
}

static int head_train_v3_layout(const yolo_net *net, const Kernel *ks[YOLO_MAX_SCALES], yolo_head_train_v3_layout *L, const char *who) {
    int rc = head_convs_v3(net, ks, who);
    if (rc) return rc;
    std::string err;
    Loss3Geometry lg;
    rc = loss3_geometry(&net->head, &lg, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    const size_t mb = (size_t)net->opt.max_batch;
    size_t off = 0;
    auto part = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return (uint64_t)at; };
    memset(L, 0, sizeof *L);
    L->n_scales = net->head.n_scales;
    int32_t cin[YOLO_MAX_SCALES] = {0, 0, 0, 0};
    for (int s = 0; s < L->n_scales; ++s) {
        const Kernel *k = ks[s];
        const size_t nw = (size_t)k->cout * k->cin * 4, nb = (size_t)k->cout * 4;
        L->cin[s] = cin[s] = k->cin; L->cout[s] = k->cout;
        L->bias_src[s] = k->w_src;
        L->w_offset[s] = part(nw); L->b_offset[s] = part(nb);
        L->m_w_offset[s] = part(nw); L->v_w_offset[s] = part(nw); L->m_b_offset[s] = part(nb); L->v_b_offset[s] = part(nb);
        L->dw_offset[s] = part(nw); L->db_offset[s] = part(nb);
    }
    L->grad_offset = part(mb * net->out_count * 4);
    L->assign_offset = part(mb * (size_t)lg.rows * 4);
    L->parts_offset = part(mb * (size_t)lg.parts * sizeof(yolo_loss_image));
    L->images_offset = part(mb * sizeof(yolo_loss_image));
    // the slabs of a smaller batch may be laid out otherwise: the scratch is sized for the largest split of any batch up to max_batch
    uint64_t need = 0;
    for (size_t b = 1; b <= mb; ++b) {
        struct yolo_v3_wgrad_plan q;
        Wgrad3Geometry g;
        rc = wgrad3_plan(&net->head, cin, (int)b, YOLO_DTYPE_F32, &q, &g, err);
        if (rc) return fail(rc, std::string(who) + ": " + err);
        if (q.scratch_bytes > need) need = q.scratch_bytes;
    }
    L->scratch_bytes = need;
    L->scratch_offset = part((size_t)need);
    L->total_bytes = off;
    return YOLO_OK;
}

int yolo_net_head_train_v3_layout(const yolo_net *net, yolo_head_train_v3_layout *out) {
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_head_train_v3_layout: null argument");
    const Kernel *ks[YOLO_MAX_SCALES];
    return head_train_v3_layout(net, ks, out, "yolo_net_head_train_v3_layout");
}

size_t yolo_net_head_train_v3_bytes(const yolo_net *net) {
    yolo_head_train_v3_layout L;
    const Kernel *ks[YOLO_MAX_SCALES];
    if (head_train_v3_layout(net, ks, &L, "yolo_net_head_train_v3_bytes")) return 0;
    return (size_t)L.total_bytes;
}

int yolo_net_head_train_v3_init(yolo_net *net, void *state_dev, size_t bytes, const float *const *w_host, const float *const *b_host) {
    const char *who = "yolo_net_head_train_v3_init";
    if (!net || !state_dev || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_head_train_v3_layout L;
    const Kernel *ks[YOLO_MAX_SCALES];
    int rc = head_train_v3_layout(net, ks, &L, who);
    if (rc) return rc;
    for (int s = 0; s < L.n_scales; ++s)
        if (!w_host[s] || !b_host[s]) return fail(YOLO_ERR_ARG, std::string(who) + ": scale " + std::to_string(s) + ": null argument");
    if (bytes < L.total_bytes) return fail(YOLO_ERR_ARG, std::string(who) + ": state too small (yolo_net_head_train_v3_bytes)");
    if ((uintptr_t)state_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the state must be 256-byte aligned");
    if (!net->weights_loaded || !net->dev_weights) return fail(YOLO_ERR_STATE, std::string(who) + ": weights not loaded");
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    const bool f16 = net->opt.dtype == YOLO_DTYPE_F16;
    HIP_TRY(hipDeviceSynchronize());
    for (int s = 0; s < L.n_scales; ++s) {
        const Kernel *k = ks[s];
        const size_t nw = (size_t)k->cout * k->cin * 4, nb = (size_t)k->cout * 4;
        HIP_TRY(hipMemcpy(st + L.w_offset[s], w_host[s], nw, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(st + L.b_offset[s], b_host[s], nb, hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(st + L.m_w_offset[s], 0, nw));
        HIP_TRY(hipMemset(st + L.v_w_offset[s], 0, nw));
        HIP_TRY(hipMemset(st + L.m_b_offset[s], 0, nb));
        HIP_TRY(hipMemset(st + L.v_b_offset[s], 0, nb));
        // the conv's packed form, as pack_weights (weights.cpp) writes a 1 x 1 conv without batch norm: row o at o * wrow bytes, bias as it is
        const size_t wrow = (size_t)k->ktiles * 128;
        std::vector<unsigned char> rows((size_t)k->cout * wrow, 0);
        for (int o = 0; o < k->cout; ++o)
            for (int c = 0; c < k->cin; ++c) {
                const float v = w_host[s][(size_t)o * k->cin + c];
                if (f16) reinterpret_cast<_Float16 *>(rows.data() + (size_t)o * wrow)[c] = (_Float16)v;
                else reinterpret_cast<float *>(rows.data() + (size_t)o * wrow)[c] = v;
            }
        HIP_TRY(hipMemcpy(net->dev_weights + k->w_off, rows.data(), rows.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(net->dev_weights + k->b_off, b_host[s], nb, hipMemcpyHostToDevice));
    }
    return YOLO_OK;
}

int yolo_net_head_train_v3_read(yolo_net *net, const void *state_dev, float *const *w_host, float *const *b_host) {
    const char *who = "yolo_net_head_train_v3_read";
    if (!net || !state_dev || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_head_train_v3_layout L;
    const Kernel *ks[YOLO_MAX_SCALES];
    int rc = head_train_v3_layout(net, ks, &L, who);
    if (rc) return rc;
    for (int s = 0; s < L.n_scales; ++s)
        if (!w_host[s] || !b_host[s]) return fail(YOLO_ERR_ARG, std::string(who) + ": scale " + std::to_string(s) + ": null argument");
    const unsigned char *st = static_cast<const unsigned char *>(state_dev);
    HIP_TRY(hipDeviceSynchronize());
    for (int s = 0; s < L.n_scales; ++s) {
        HIP_TRY(hipMemcpy(w_host[s], st + L.w_offset[s], (size_t)L.cout[s] * L.cin[s] * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(b_host[s], st + L.b_offset[s], (size_t)L.cout[s] * 4, hipMemcpyDeviceToHost));
    }
    return YOLO_OK;
}

static int train_head_step_v3_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                  double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream, const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    yolo_head_train_v3_layout L;
    const Kernel *ks[YOLO_MAX_SCALES];
    int rc = head_train_v3_layout(net, ks, &L, who);
    if (rc) return rc;
    if (!state_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null state (yolo_net_head_train_v3_init)");
    if ((uintptr_t)state_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the state must be 256-byte aligned");
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    yolo_loss_image *parts = reinterpret_cast<yolo_loss_image *>(st + L.parts_offset);
    yolo_loss_image *images = reinterpret_cast<yolo_loss_image *>(st + L.images_offset);
    int32_t *assign = reinterpret_cast<int32_t *>(st + L.assign_offset);
    float *grad = reinterpret_cast<float *>(st + L.grad_offset);
    Loss3Geometry lg;
    std::string err;
    // (the logits pointer is the workspace's: any non-null value that is not the gradient stands in for it until check_ready has seen the net)
    rc = loss3_check(&net->head, net, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts, images, assign, result_dev, true, grad, &lg, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    if (!(lr_t == lr_t)) return fail(YOLO_ERR_ARG, std::string(who) + ": lr_t is NaN");
    yolo_v3_wgrad_view views[YOLO_MAX_SCALES];
    float *dw[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr}, *db[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    memset(views, 0, sizeof views);
    for (int s = 0; s < L.n_scales; ++s) {
        const Kernel *k = ks[s];
        views[s].x_dev = net->dev_ws + net->buffers[k->in.buf].offset;
        views[s].image_stride = k->in.img_stride; views[s].ld = k->in.ld; views[s].coff = k->in.coff;
        views[s].dtype = net_x_dtype(net); views[s].cin = k->cin;
        dw[s] = reinterpret_cast<float *>(st + L.dw_offset[s]); db[s] = reinterpret_cast<float *>(st + L.db_offset[s]);
    }
    struct yolo_v3_wgrad_plan pl;
    Wgrad3Geometry geo;
    rc = wgrad3_check(&net->head, views, batch, grad, assign, max_gt, dw, db, st + L.scratch_offset, (size_t)L.scratch_bytes, &pl, &geo, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    rc = run_forward(net, in_dev, batch, logits, s);        // dense: obj_min_logit is -inf outside detect_any
    if (rc) return rc;
    rc = run_loss3(lg, logits, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts, images, assign, result_dev, grad, s);
    if (rc) return rc;
    rc = run_wgrad3(geo, pl, batch, grad, assign, max_gt, st + L.scratch_offset, s);
    if (rc) return rc;
    const bool f16 = net->opt.dtype == YOLO_DTYPE_F16;
    for (int i = 0; i < L.n_scales; ++i) {
        const Kernel *k = ks[i];
        AdamParams p;
        memset(&p, 0, sizeof p);
        p.w = reinterpret_cast<float *>(st + L.w_offset[i]); p.b = reinterpret_cast<float *>(st + L.b_offset[i]);
        p.m_w = reinterpret_cast<float *>(st + L.m_w_offset[i]); p.v_w = reinterpret_cast<float *>(st + L.v_w_offset[i]);
        p.m_b = reinterpret_cast<float *>(st + L.m_b_offset[i]); p.v_b = reinterpret_cast<float *>(st + L.v_b_offset[i]);
        p.dw = dw[i]; p.db = db[i]; p.n_w = (long long)k->cout * k->cin; p.n_b = k->cout;
        p.lr_t = lr_t; p.beta1 = 0.9f; p.beta2 = 0.999f; p.eps = 1e-8f;        // tf.train.AdamOptimizer's defaults (net/v2.py:205)
        p.pack_w = net->dev_weights + k->w_off; p.pack_b = reinterpret_cast<float *>(net->dev_weights + k->b_off);
        p.pack_cin = k->cin; p.pack_f16 = f16;
        p.pack_row = (int)((size_t)k->ktiles * 128 / (f16 ? 2 : 4));
        HIP_TRY(launch_adam_step(p, s));
    }
    return YOLO_OK;
}
int yolo_net_train_head_step_v3(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_head_step_v3_any(net, NetIn{in_dev, false}, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, state_dev, lr_t, result_dev, stream,
                                  "yolo_net_train_head_step_v3");
}
int yolo_net_train_head_step_v3_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev,
                                   int max_gt, double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_head_step_v3_any(net, NetIn{in_dev, true}, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, state_dev, lr_t, result_dev, stream,
                                  "yolo_net_train_head_step_v3_u8");
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

// C ABI of libyolo_hip.so (declared in include/yolo_hip.h).  No exceptions cross the boundary.
#include <cstdio>
#include <cstring>
#include <new>

#include <cmath>
#include "conv_tiles.h"
#include "yolo_internal.h"

namespace yolo {
const char *get_error();
}
using namespace yolo;

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                      \
            return YOLO_ERR_HIP;                                                               \
        }                                                                                      \
    } while (0)

static int fail(int code, const std::string &msg) {
    set_error(msg);
    return code;
}

namespace {
// packed weights of a kernel; nullptr while no weights are bound (yolo_net_kernel_info / describe build launch parameters of a plan that
// has none yet: no offset is applied to a null pointer -- found by the sanitizer build, tests/test_sanitizer.py)
static inline const unsigned char *weights_at(const yolo_net *net, size_t off) { return net->dev_weights ? net->dev_weights + off : nullptr; }

// Ticket counters of the in-launch pair split: every launch returns them to zero, so they are cleared when the workspace is bound
// and again after any failed forward (a launch that did not run may leave the forward half-way).  The memset goes to the null
// stream, which does not order against the non-blocking streams a caller may launch on: hence the device-wide synchronise.
int zero_pair_counters(yolo_net *net) {
    if (!net->splitk_bytes || !net->dev_ws) return YOLO_OK;
    const size_t per = net->splitk_bytes / (size_t)net->arenas;
    for (int a = 0; a < net->arenas; ++a)
        HIP_TRY(hipMemset(net->dev_ws + net->splitk_off + (size_t)a * arena_slab_bytes(net), 0, per < kPairCounterBytes ? per : kPairCounterBytes));
    HIP_TRY(hipDeviceSynchronize());
    return YOLO_OK;
}
}

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
            if (k.kind == K_CONV && k.stem < 2 && conv_tile_valid(net, k, net->opt.force_tile - 1)) k.tile = net->opt.force_tile - 1;
    // the split-K slab is the last region of the workspace (plan.cpp reserves nothing for it): sized from the launches that can split
    net->splitk_bytes = splitk_slab_bytes(net) * (size_t)net->arenas;
    net->workspace_bytes = net->splitk_off + net->splitk_bytes;
    *out = net;
    return YOLO_OK;
}

void yolo_net_destroy(yolo_net *net) {
    if (!net) return;
    if (net->e_fork) (void)hipEventDestroy(net->e_fork);
    for (hipEvent_t e : net->e_join) (void)hipEventDestroy(e);
    for (hipStream_t st : net->side) (void)hipStreamDestroy(st);
    for (hipEvent_t e : net->e_bfork) (void)hipEventDestroy(e);
    for (hipEvent_t e : net->e_bjoin) (void)hipEventDestroy(e);
    for (hipStream_t st : net->branch) (void)hipStreamDestroy(st);
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
    const size_t mb = (size_t)net->opt.max_batch;
    add("head logits", net->logits_off, net->out_count * 4 * mb, net->cand_off - net->logits_off);
    add("candidates", net->cand_off, sizeof(Candidate) * (size_t)net->opt.cand_capacity * mb, net->count_off - net->cand_off);
    add("candidate counters", net->count_off, sizeof(int) * mb * kCandCountStride, net->nms_off - net->count_off);
    add("nms scratch", net->nms_off, nms_scratch_bytes(net->opt.cand_capacity) * mb, net->obj_off - net->nms_off);
    add("objectness", net->obj_off, net->obj_bytes, net->splitk_off - net->obj_off);
    if (net->splitk_bytes) add("split-K tickets + slabs", net->splitk_off, net->splitk_bytes, net->splitk_bytes);
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
    int rc = zero_pair_counters(net);
    if (rc) return rc;
    return YOLO_OK;
}

}  // extern "C"

// ---- forward ------------------------------------------------------------------------------------
namespace {

// The network input of one call: the caller's float32 tensor, or (ABI 7: the *_u8 entries) its uint8 one.  Only the five kernels that
// read the input look at the tag (K_PREP, K_FIRST, the stem); a byte u is to them float32(u / 255.) (yolo_internal.h: u8_unit).
struct NetIn {
    const void *ptr;
    bool u8;
    NetIn at(size_t elems) const { return NetIn{static_cast<const unsigned char *>(ptr) + elems * (u8 ? 1 : 4), u8}; }
};

struct Ptrs {
    yolo_net *net;
    NetIn in;                   // already advanced to image `img0` by the caller
    float *out;                 // ditto
    int img0 = 0;               // first image of this pass in the batch (two-stream halves: compact per-image arrays)
    int arena = 0;              // activation arena of this pass
    unsigned char *buf_base(int b) const {
        if (b == BUF_USER_IN) return static_cast<unsigned char *>(const_cast<void *>(in.ptr));
        if (b == BUF_USER_OUT) return reinterpret_cast<unsigned char *>(out);
        return net->dev_ws + (size_t)arena * net->arena_bytes + net->buffers[b].offset;
    }
    int esz(const View &v) const { return v.f32 ? 4 : net->esize; }
    // element pointer of channel 0 of pixel 0 of image 0 of the view
    unsigned char *view_ptr(const View &v) const { return buf_base(v.buf) + (size_t)(v.base + v.coff) * esz(v); }
};

// conv launch parameters for one planned kernel at the given batch: the shape half (conv_dispatch.cpp) + pointers, the byte-limit
// checks and the objectness block
int make_conv_params(yolo_net *net, const Kernel &k, const Ptrs &P, int batch, ConvParams &p) {
    const long long in_bytes = (long long)batch * k.in.img_stride * net->esize;
    if (in_bytes > 0x7ffffff0LL)
        return fail(YOLO_ERR_ARG, "conv input tensor exceeds 2 GiB (32-bit buffer addressing): lower the batch");
    if ((long long)batch * net->layers[k.src_layer].H * net->layers[k.src_layer].W > 0x7fffffffLL)
        return fail(YOLO_ERR_ARG, "too many output pixels for one launch");
    conv_shape_params(net, k, batch, p);
    p.in = P.buf_base(k.in.buf);
    p.in_bytes = (uint32_t)in_bytes;
    p.wgt = weights_at(net, k.w_off);
    p.bias = reinterpret_cast<const float *>(weights_at(net, k.b_off));
    p.out = P.view_ptr(k.out);
    p.vec_out = p.vec_out && ((uintptr_t)P.buf_base(k.out.buf) % 16 == 0);
    if (k.head && net->obj_bytes && net->head.n_classes > 0 && !p.vec_out && p.out_f32 && k.outmode == OUT_NORMAL && !k.has_res) {
        const int width = 5 + net->head.n_classes;
        const long long base = k.out.base + k.out.coff;
        const size_t rows = net->out_count / (size_t)width;
        if (k.out.ld % width == 0 && base % width == 0 && rows * width == net->out_count && (size_t)batch * rows * 4 <= net->obj_bytes) {
            p.obj_out = reinterpret_cast<float *>(net->dev_ws + net->obj_off) + (size_t)P.img0 * rows;
            p.obj_width = width; p.obj_rows = (int)rows; p.obj_row0 = (int)(base / width); p.obj_na = k.out.ld / width;
            p.obj_min = net->obj_min_logit;     // -inf outside yolo_net_detect: every row is written
        }
    }
    if (k.has_res) p.res = P.view_ptr(k.in2);
    return YOLO_OK;
}

// Back-to-back 1x1 (ConvLaunch.fuse2): `p`, the 3x3's launch parameters, takes the weights, bias and output view of the 1x1 `b` behind it
void attach_fuse2(const yolo_net *net, const Kernel &b, const Ptrs &P, int batch, ConvParams &p) {
    p.fuse2 = 1;
    p.w2 = weights_at(net, b.w_off);
    p.w2_bytes = (uint32_t)b.w_bytes;
    p.wrow2_bytes = (uint32_t)b.ktiles * 128;
    p.b2 = reinterpret_cast<const float *>(weights_at(net, b.b_off));
    p.out2 = P.view_ptr(b.out);
    p.out2_bytes = (uint32_t)((long long)batch * b.out.img_stride * net->esize);       // (below 2 GiB: resolve_conv)
    p.out2_ld = b.out.ld;
    p.out2_img_stride = b.out.img_stride;
    p.leaky2 = b.leaky;
}

// one conv launch as its record says (the split fields are set here, after the record was built from the whole-K parameters)
hipError_t launch_conv_any(const yolo_net *net, const Kernel &k, const ConvParams &p0, const ConvLaunch &L, hipStream_t s, int arena = 0) {
    const int tile = L.tile, ks = L.ks;
    ConvParams p = p0;
    if (ks > 1) {
        p.ksplit = ks; p.kunits = L.ku;
        p.cout_pad = (p.Cout + 127) / 128 * 128;
        unsigned char *base = net->dev_ws + net->splitk_off + (size_t)arena * arena_slab_bytes(net);
        p.part = reinterpret_cast<float *>(base + kPairCounterBytes);
        if (L.pair) {       // counters (zeroed at bind, returned to zero by every launch) in front of the partial sums
            const size_t data_bytes = arena_slab_data_bytes(net);
            p.pair = 1;
            p.pair_cnt = reinterpret_cast<int *>(base);
            p.part_bytes = (uint32_t)(data_bytes < 0x7ffffff0u ? data_bytes : 0x7ffffff0u);
        }
    }
    if (tile <= 0) p.f32_emu = conv_f32_emu_rule(net->opt.f32_products, net->opt.dtype, p, k.cfg, k.perchunk != 0, ks) ? 1 : 0;
    hipError_t e = tile > 0 ? launch_conv_dma(p, tile, s) : launch_conv(p, net->opt.dtype, k.cfg, k.perchunk != 0, s);
    if (e != hipSuccess || ks <= 1 || L.pair) return e;
    ReduceParams r;
    memset(&r, 0, sizeof r);
    r.part = p.part; r.bias = p.bias; r.res = p.has_res ? p.res : nullptr; r.out = p.out;
    r.obj_out = p.obj_out; r.obj_width = p.obj_width; r.obj_rows = p.obj_rows; r.obj_row0 = p.obj_row0; r.obj_na = p.obj_na;
    r.ksplit = ks; r.M = p.M; r.Cout = p.Cout; r.cout_pad = p.cout_pad; r.HoWo = p.HoWo; r.Wo = p.Wo;
    r.out_ld = p.out_ld; r.res_ld = p.res_ld; r.leaky = p.leaky; r.outmode = p.outmode; r.out_f32 = p.out_f32; r.f32 = p.f32;
    r.out_img_stride = p.out_img_stride; r.res_img_stride = p.res_img_stride;
    return launch_splitk_reduce(r, s);
}

// May the branch tails of this net run beside its main chain at this batch?  Yes when the plan has any and no launch of the pass splits K.
bool branch_tails_ok(yolo_net *net, int batch) {
    static const bool off = getenv("YOLO_NO_BRANCH_STREAM") != nullptr;       // A/B switch (same results either way)
    if (off || net->side_chains <= 0 || net->opt.keep_all || batch <= 0 || batch > net->opt.max_batch) return false;
    if (net->side_ok.size() != (size_t)net->opt.max_batch + 1) net->side_ok.assign((size_t)net->opt.max_batch + 1, -1);
    signed char &memo = net->side_ok[(size_t)batch];
    if (memo < 0) memo = pass_splits_k(net, batch) ? 0 : 1;
    return memo == 1;
}
int branch_streams(yolo_net *net, int arena) {
    if (net->branch.empty()) {
        const size_t n = (size_t)(net->arenas > 0 ? net->arenas : 1);
        net->branch.assign(n, nullptr);
        net->e_bjoin.assign(n, nullptr);
        net->e_bfork.assign(n * 4, nullptr);
        for (size_t i = 0; i < n; ++i)
            if (hipStreamCreateWithFlags(&net->branch[i], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&net->e_bjoin[i], hipEventDisableTiming) != hipSuccess)
                return fail(YOLO_ERR_HIP, "branch tail: stream / event creation failed");
        for (size_t i = 0; i < n * 4; ++i)
            if (hipEventCreateWithFlags(&net->e_bfork[i], hipEventDisableTiming) != hipSuccess)
                return fail(YOLO_ERR_HIP, "branch tail: event creation failed");
    }
    return (size_t)arena < net->branch.size() ? YOLO_OK : fail(YOLO_ERR_STATE, "branch tail: arena out of range");
}

int run_forward_pass(yolo_net *net, const NetIn in, int batch, float *out_dev, hipStream_t s, hipEvent_t *ev, int img0, int arena,
                     long long *obj_rows_out) {
    Ptrs P{net, in, out_dev, img0, arena};
    const int dtype = net->opt.dtype;
    const int epc = net->epc;
    long long obj_rows_written = 0;          // rows of the compact objectness array the head convs of this pass fill
    bool fused2_done = false;                // the previous conv launch has computed this 1x1 conv too (back-to-back fusion)
    // branch tails (plan.cpp: side_chains) on a second stream of this part: fork by an event behind the kernel in front of the tail,
    // one join in front of whatever follows the pass (the decode, the caller).  Not under per-kernel events, and not at a batch where
    // any launch of the pass splits K (the split-K slab and its ticket counters are one per arena)
    const bool use_branch = !ev && branch_tails_ok(net, batch);
    hipStream_t const s_main = s;
    hipStream_t s_branch = nullptr;
    int cur_tail = 0;
    if (use_branch) {
        const int rc = branch_streams(net, arena);
        if (rc) return rc;
        s_branch = net->branch[arena];
    }
    for (size_t ki = 0; ki < net->kernels.size(); ++ki) {
        const Kernel &k = net->kernels[ki];
        hipError_t e = hipSuccess;
        s = s_main;
        if (use_branch && k.side) {
            if (k.side != cur_tail) {
                hipEvent_t ef = net->e_bfork[(size_t)arena * 4 + (size_t)((k.side - 1) & 3)];
                if (hipEventRecord(ef, s_main) != hipSuccess || hipStreamWaitEvent(s_branch, ef, 0) != hipSuccess)
                    return fail(YOLO_ERR_HIP, "branch tail: fork failed");
                cur_tail = k.side;
            }
            s = s_branch;
        }
        if (ev && hipEventRecord(ev[2 * ki], s) != hipSuccess) return fail(YOLO_ERR_HIP, "hipEventRecord failed");
        switch (k.kind) {
        case K_PREP: {
            PrepParams p;
            p.in = in.ptr;
            p.out = P.view_ptr(k.out);
            p.pixels = (long long)batch * k.in.H * k.in.W;
            p.C = k.in.C;
            p.Cpad = k.out.ld;
            e = launch_prep(p, dtype, s, in.u8);
            break;
        }
        case K_CONV: {
            if (k.stem == 2) {      // the previous kernel (first layer) is folded into this launch
                const Kernel &f = net->kernels[ki - 1];
                StemParams p;
                memset(&p, 0, sizeof p);
                p.in = in.ptr;
                p.w1 = reinterpret_cast<const float *>(net->dev_weights + f.w_off);
                p.b1 = reinterpret_cast<const float *>(net->dev_weights + f.b_off);
                p.w2 = net->dev_weights + k.w_off;
                p.b2 = reinterpret_cast<const float *>(net->dev_weights + k.b_off);
                p.w2_bytes = (uint32_t)k.w_bytes;
                p.wrow2 = (uint32_t)k.ktiles * 128;
                p.out = P.view_ptr(k.out);
                p.H = f.in.H; p.W = f.in.W; p.Ho = k.out.H; p.Wo = k.out.W;
                p.out_ld = k.out.ld; p.out_img_stride = k.out.img_stride;
                p.in_img_stride = (long long)f.in.H * f.in.W * 3;
                if (ki + 1 < net->kernels.size() && net->kernels[ki + 1].stem == 3) {      // 1x1 64->32 on the same pixels
                    const Kernel &t = net->kernels[ki + 1];
                    p.w3 = net->dev_weights + t.w_off;
                    p.b3 = reinterpret_cast<const float *>(net->dev_weights + t.b_off);
                    p.out3 = P.view_ptr(t.out);
                    p.out3_ld = t.out.ld; p.out3_img_stride = t.out.img_stride;
                }
                e = launch_stem(p, batch, s, net->halves ? 512 / net->parts : 512, in.u8);
                break;
            }
            if (k.stem == 3) break;     // computed by the stem kernel
            if (k.fuse2_prev && fused2_done) { fused2_done = false; break; }       // computed by the conv in front of it
            ConvParams p;
            int rc = make_conv_params(net, k, P, batch, p);
            if (rc) return rc;
            if (k.head && p.obj_out) obj_rows_written += (long long)p.Ho * p.Wo * p.obj_na;
            if (k.mx) {
                e = launch_conv_mx(p, s);
                break;
            }
            const ConvLaunch L = resolve_conv(net, ki, p, k.tile, arena_slab_data_bytes(net));
            if (L.fuse2) attach_fuse2(net, net->kernels[ki + 1], P, batch, p);
            fused2_done = L.fuse2 != 0;
            e = launch_conv_any(net, k, p, L, s, P.arena);
            break;
        }
        case K_FIRST: {
            if (k.stem == 1) break;     // runs inside the next kernel (stem.hip)
            FirstParams p;
            p.in = in.ptr;
            p.wgt = reinterpret_cast<const float *>(net->dev_weights + k.w_off);
            p.bias = reinterpret_cast<const float *>(net->dev_weights + k.b_off);
            p.out = P.view_ptr(k.out);
            p.H = k.in.H; p.W = k.in.W; p.Cout = k.cout; p.out_ld = k.out.ld; p.leaky = k.leaky;
            p.pool = k.pool_fused;
            p.round_half = dtype == YOLO_DTYPE_F16;
            p.out_img_stride = k.out.img_stride;
            p.total = (long long)batch * k.in.H * k.in.W;
            if (k.out.ld % epc || (k.out.base + k.out.coff) % epc || k.out.img_stride % epc)
                return fail(YOLO_ERR_PLAN, "first-layer kernel needs a 16-byte aligned output view");
            e = launch_first(p, dtype, s, in.u8);
            break;
        }
        case K_POOL: {
            if (k.spp) {        // the three pools of an SPP block in one launch
                SppParams p;
                memset(&p, 0, sizeof p);
                p.in = P.view_ptr(k.in);
                p.H = k.in.H; p.W = k.in.W; p.chunks = k.in.C / 8;
                p.in_ld = k.in.ld; p.in_img_stride = k.in.img_stride;
                const View *ov[3] = {&k.out, &k.out2, &k.out3};
                for (int l = 0; l < 3; ++l) {
                    p.out[l] = P.view_ptr(*ov[l]);
                    p.out_ld[l] = ov[l]->ld; p.out_img_stride[l] = ov[l]->img_stride;
                }
                e = launch_spp(p, (k.pool_k - 1) / 2, batch, s);
                break;
            }
            PoolParams p;
            p.in = P.view_ptr(k.in);
            p.out = P.view_ptr(k.out);
            p.H = k.in.H; p.W = k.in.W; p.C = k.in.C; p.in_ld = k.in.ld;
            p.Ho = k.out.H; p.Wo = k.out.W; p.out_ld = k.out.ld; p.stride = k.pool_stride;
            p.in_img_stride = k.in.img_stride; p.out_img_stride = k.out.img_stride;
            p.total = (long long)batch * k.out.H * k.out.W;
            p.ksize = k.pool_k;
            e = k.pool_k == 2 ? launch_pool(p, dtype, s) : launch_pool_same(p, dtype, s);
            break;
        }
        case K_ELTWISE: {
            EltParams p;
            memset(&p, 0, sizeof p);
            p.a = P.view_ptr(k.in);
            p.a_f32 = k.in.f32;
            p.b = k.has_res ? P.view_ptr(k.in2) : nullptr;
            p.out = P.view_ptr(k.out);
            p.H = k.in.H; p.W = k.in.W; p.C = k.in.C;
            p.a_ld = k.in.ld; p.b_ld = k.in2.ld; p.out_ld = k.out.ld;
            p.outmode = k.outmode;
            p.out_f32 = k.out.f32 || dtype == YOLO_DTYPE_F32;
            p.a_img_stride = k.in.img_stride; p.b_img_stride = k.in2.img_stride; p.out_img_stride = k.out.img_stride;
            p.total = (long long)batch * k.in.H * k.in.W * k.in.C;
            e = launch_eltwise(p, dtype, s);
            break;
        }
        }
        if (e != hipSuccess) {
            char msg[160];
            snprintf(msg, sizeof msg, "kernel %zu (layer %d) launch failed: %s", ki, k.layer, hipGetErrorString(e));
            return fail(YOLO_ERR_HIP, msg);
        }
        if (ev && hipEventRecord(ev[2 * ki + 1], s) != hipSuccess) return fail(YOLO_ERR_HIP, "hipEventRecord failed");
    }
    if (cur_tail) {
        if (hipEventRecord(net->e_bjoin[arena], s_branch) != hipSuccess || hipStreamWaitEvent(s_main, net->e_bjoin[arena], 0) != hipSuccess)
            return fail(YOLO_ERR_HIP, "branch tail: join failed");
    }
    *obj_rows_out = obj_rows_written;
    return YOLO_OK;
}

// One forward pass; with YOLO_STREAMS=N (N = 2..4) the batch goes out as N parts on N streams (the caller's and internal
// ones, fork/join by events): images are independent, so the ragged tail + cold start of every kernel of one part overlaps
// the bulk of the other parts' kernels instead of leaving CUs idle at each of the ~73 kernel boundaries.  Every part has
// its own activation arena (plan.cpp: allocate).
// every head conv of the plan fills the compact objectness array at this batch (what run_forward_impl finds out afterwards as obj_valid)
bool all_heads_write_objectness(yolo_net *net, const NetIn in_dev, float *out_dev, int batch) {
    if (!net->obj_bytes || net->head.n_classes <= 0) return false;
    const int per = net->parts >= 2 && batch > part_batch(net) ? part_batch(net) : batch;
    Ptrs P{net, in_dev, out_dev, 0, 0};
    bool any = false;
    for (const Kernel &k : net->kernels) {
        if (k.kind != K_CONV || !k.head) continue;
        ConvParams p;
        if (make_conv_params(net, k, P, per, p) != 0 || !p.obj_out) return false;
        // (the rows reach the compact array through the staged float32 epilogue of the LDS-DMA tiles or the 4-wave kernel, or through
        // the split-K reduce kernel: all of them honour obj_out)
        any = true;
    }
    return any;
}

int run_forward_impl(yolo_net *net, const NetIn in_dev, int batch, float *out_dev, hipStream_t s, hipEvent_t *ev);
int run_forward(yolo_net *net, const NetIn in_dev, int batch, float *out_dev, hipStream_t s, hipEvent_t *ev = nullptr) {
    const int rc = run_forward_impl(net, in_dev, batch, out_dev, s, ev);
    if (rc != YOLO_OK) {        // leave the pair-split counters as every later launch expects them; keep the first error's message
        const std::string msg = get_error();
        (void)hipGetLastError();
        (void)zero_pair_counters(net);
        set_error(msg);
    }
    return rc;
}
int run_forward_impl(yolo_net *net, const NetIn in_dev, int batch, float *out_dev, hipStream_t s, hipEvent_t *ev) {
    const long long rows = net->head.n_classes > 0 ? (long long)(net->out_count / (size_t)(5 + net->head.n_classes)) : -1;
    const int parts = net->parts;
    const int per = (net->opt.max_batch + parts - 1) / parts;       // images a part holds
    if (parts >= 2 && batch > per) {
        if (ev) return fail(YOLO_ERR_STATE, "per-kernel events need the parts timed one by one (yolo_net_forward_timed)");
        if (net->side.empty()) {
            net->side.resize(parts - 1);
            net->e_join.resize(parts - 1);
            for (int i = 0; i < parts - 1; ++i)
                if (hipStreamCreateWithFlags(&net->side[i], hipStreamNonBlocking) != hipSuccess ||
                    hipEventCreateWithFlags(&net->e_join[i], hipEventDisableTiming) != hipSuccess)
                    return fail(YOLO_ERR_HIP, "multi-stream forward: stream/event creation failed");
            if (hipEventCreateWithFlags(&net->e_fork, hipEventDisableTiming) != hipSuccess)
                return fail(YOLO_ERR_HIP, "multi-stream forward: event creation failed");
        }
        const yolo_layer_desc &d0 = net->layers[0].d;
        const size_t in_img = (size_t)d0.h * d0.w * d0.c;
        net->halves = true;         // persistent kernels size their grids for a share of the chip
        HIP_TRY(hipEventRecord(net->e_fork, s));
        bool all = true;
        int used = 0;
        for (int part = 0, img0 = 0; img0 < batch; ++part, img0 += per) {
            const int nb = batch - img0 < per ? batch - img0 : per;
            hipStream_t st = part == 0 ? s : net->side[part - 1];
            if (part > 0) HIP_TRY(hipStreamWaitEvent(st, net->e_fork, 0));
            long long w = 0;
            const int rc = run_forward_pass(net, in_dev.at((size_t)img0 * in_img), nb, out_dev + (size_t)img0 * net->out_count, st, nullptr,
                                            img0, part, &w);
            if (rc) return rc;
            all = all && w == rows;
            used = part + 1;
        }
        for (int part = 1; part < used; ++part) {
            HIP_TRY(hipEventRecord(net->e_join[part - 1], net->side[part - 1]));
            HIP_TRY(hipStreamWaitEvent(s, net->e_join[part - 1], 0));
        }
        net->obj_valid = net->obj_bytes > 0 && rows > 0 && all;
        return YOLO_OK;
    }
    net->halves = false;
    long long w0 = 0;
    int rc = run_forward_pass(net, in_dev, batch, out_dev, s, ev, 0, 0, &w0);
    if (rc) return rc;
    net->obj_valid = net->obj_bytes > 0 && rows > 0 && w0 == rows;
    return YOLO_OK;
}

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
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nk = net->kernels.size();
    std::vector<hipEvent_t> ev(2 * nk, nullptr);
    for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(YOLO_ERR_HIP, "hipEventCreate failed");
    // with several arenas the parts are timed one after the other on the caller's stream (each kernel alone on the chip)
    // and their times added per kernel
    const int parts = net->parts;
    const int per = (net->opt.max_batch + parts - 1) / parts;
    const yolo_layer_desc &d0 = net->layers[0].d;
    const size_t in_img = (size_t)d0.h * d0.w * d0.c;
    for (size_t k = 0; k < nk; ++k) ms_host[k] = 0.f;
    net->halves = false;
    long long rows_written = 0;
    for (int part = 0, img0 = 0; rc == YOLO_OK && img0 < batch; ++part, img0 += per) {
        const int nb = batch - img0 < per ? batch - img0 : per;
        long long w = 0;
        rc = run_forward_pass(net, in_dev.at((size_t)img0 * in_img), nb, out_dev + (size_t)img0 * net->out_count, s, ev.data(), img0, part, &w);
        rows_written += w;
        if (rc == YOLO_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(YOLO_ERR_HIP, "hipStreamSynchronize failed");
        for (size_t k = 0; rc == YOLO_OK && k < nk; ++k) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, ev[2 * k], ev[2 * k + 1]) != hipSuccess) rc = fail(YOLO_ERR_HIP, "hipEventElapsedTime failed");
            ms_host[k] += t;
        }
    }
    net->obj_valid = false;     // (the timed pass is not followed by a decode)
    (void)rows_written;
    if (rc != YOLO_OK) { const std::string msg = get_error(); (void)hipGetLastError(); (void)zero_pair_counters(net); set_error(msg); }
    for (auto &e : ev) (void)hipEventDestroy(e);
    return rc;
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
    auto set_symbol = [&](const std::string &sym) { snprintf(out->symbol, sizeof out->symbol, "%s", sym.c_str()); };
    const char *t = net->opt.dtype == YOLO_DTYPE_F16 ? "f16" : "f32";
    auto elems = [](const View &v) { return (double)v.H * v.W * v.C; };
    auto esz = [&](const View &v) { return v.f32 ? 4.0 : (double)net->esize; };
    if (k.kind == K_CONV) {
        conv_kernel_info(net, kernel, out);
    } else if (k.kind == K_FIRST) {
        out->ksize = 3; out->stride = 1; out->cin = 3; out->cout = k.cout; out->out_h = k.out.H; out->out_w = k.out.W;
        out->flops = 2.0 * k.out.H * k.out.W * k.cout * 27;
        out->bytes = (double)k.in.H * k.in.W * 3 * 4 + elems(k.out) * esz(k.out);
        out->weight_bytes = 28.0 * k.cout * 4;
        snprintf(out->name, sizeof out->name, k.pool_fused ? "conv_first_pool<%s,%d>" : "conv_first<%s,%d>", t, k.cout);
        if (k.pool_fused) { out->out_h = k.in.H; out->out_w = k.in.W; out->flops = 2.0 * k.in.H * k.in.W * k.cout * 27; }
        set_symbol(first_symbol(net->opt.dtype, k.cout, k.pool_fused != 0));
        if (k.stem == 1) {
            out->symbol[0] = 0;          // no launch of its own: accounted for in the conv_stem kernel that follows
            out->flops = 0; out->bytes = 0; out->weight_bytes = 0;
            snprintf(out->name, sizeof out->name, "conv_first<fused into conv_stem>");
        }
    } else {
        out->out_h = k.out.H; out->out_w = k.out.W; out->cout = k.out.C; out->cin = k.in.C;
        out->bytes = elems(k.in) * (k.in.f32 ? 4.0 : net->esize) + elems(k.out) * esz(k.out) + (k.has_res ? elems(k.in2) * net->esize : 0.0);
        snprintf(out->name, sizeof out->name, "%s<%s>", k.kind == K_PREP ? "prep" : k.kind == K_POOL ? "pool" : "eltwise", t);
        const int epc = net->epc;       // pool: the 16-byte-vector instantiation runs when every stride is chunk-aligned (aux.hip)
        const bool vec = k.kind == K_POOL && k.in.C % epc == 0 && k.in.ld % epc == 0 && k.out.ld % epc == 0 && (k.in.base + k.in.coff) % epc == 0 &&
                         (k.out.base + k.out.coff) % epc == 0 && k.in.img_stride % epc == 0 && k.out.img_stride % epc == 0;
        set_symbol(aux_symbol(k.kind, net->opt.dtype, vec));
        if (k.kind == K_POOL && k.spp) {        // one read, three writes
            out->ksize = k.pool_k; out->stride = 1;
            out->bytes += elems(k.out2) * esz(k.out2) + elems(k.out3) * esz(k.out3);
            snprintf(out->name, sizeof out->name, "spp_pool<%s,%d-%d-%d>", t, k.pool_k, 2 * k.pool_k - 1, 3 * k.pool_k - 2);
            set_symbol(spp_pool_symbol((k.pool_k - 1) / 2));
        } else if (k.kind == K_POOL && k.pool_k != 2) {
            out->ksize = k.pool_k; out->stride = 1;
            snprintf(out->name, sizeof out->name, "pool_same<%s,%dx%d>", t, k.pool_k, k.pool_k);
            set_symbol(pool_same_symbol(net->opt.dtype, vec));
        }
    }
    return YOLO_OK;
}

static int tune_streams_any(yolo_net *net, const NetIn in_dev, int batch, void *stream, const char *who) {
    int rc = check_ready(net, in_dev.ptr, batch, who);
    if (rc) return rc;
    if (!net->arena_full || batch <= (net->opt.max_batch + 1) / 2) return YOLO_OK;       // nothing to choose (or not with this batch)
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail(YOLO_ERR_HIP, std::string(who) + ": hipEventCreate failed");
    }
    // interleaved: one pass, two halves, one pass, ... -- three forward passes per sample, the first round of each only warms up,
    // the best of the other four counts (boxes differ: the same build gains 3-4 % from two halves on one MI355X and loses 1-2 % on
    // another, so the rule's answer is re-measured where the net runs)
    float best[3] = {0.f, 1e30f, 1e30f};
    for (int rep = 0; rep < 5 && rc == YOLO_OK; ++rep)
        for (int parts = 1; parts <= 2 && rc == YOLO_OK; ++parts) {
            net->parts = parts;
            if (hipEventRecord(e0, s) != hipSuccess) rc = fail(YOLO_ERR_HIP, std::string(who) + ": hipEventRecord failed");
            for (int k = 0; k < 3 && rc == YOLO_OK; ++k) rc = run_forward(net, in_dev, batch, logits, s);
            if (rc == YOLO_OK && (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess))
                rc = fail(YOLO_ERR_HIP, std::string(who) + ": event failed");
            float ms = 0.f;
            if (rc == YOLO_OK && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && rep > 0 && ms < best[parts]) best[parts] = ms;
        }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    // two halves must win by 1.5 %: where they do not gain 3-4 % they are within +-1 % of one pass, which the later steady state
    // (warmer chip, decode + NMS behind the join) has been seen to turn into a loss
    net->parts = (rc == YOLO_OK && best[2] < 0.985f * best[1]) ? 2 : (rc == YOLO_OK ? 1 : net->arenas);
    net->parts_tuned = rc == YOLO_OK;
    net->obj_valid = false;
    return rc;
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
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    {   // every launch of a multi-stream net sees one part of the batch: tune for that size (arena 0)
        const int per = part_batch(net);
        if (batch > per) batch = per;
    }
    rc = run_forward(net, NetIn{in_dev, false}, batch, logits, s);      // real activations in every buffer
    if (rc) return rc;
    Ptrs P{net, NetIn{in_dev, false}, logits};
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    for (size_t ki = 0; ki < net->kernels.size(); ++ki) {
        Kernel &k = net->kernels[ki];
        if (k.kind != K_CONV || k.stem >= 2 || k.mx || !dma_eligible(net, k)) continue;      // (MX convs: one kernel, weights packed for it)
        ConvParams p;
        rc = make_conv_params(net, k, P, batch, p);
        if (rc) break;
        float best = 1e30f;
        int best_tile = -1;
        for (int tile = 0; tile < kNumTiles; ++tile) {
            if (!conv_tile_valid(net, k, tile)) continue;
            const ConvLaunch L = resolve_conv(net, ki, p, tile, arena_slab_data_bytes(net));       // (timed without the 1x1 behind it: L.fuse2 is not attached)
            float ms = 1e30f;
            bool ok = true;
            for (int rep = 0; rep < 4 && ok; ++rep) {       // first launch warms caches; keep the best of the rest
                ok = hipEventRecord(e0, s) == hipSuccess && launch_conv_any(net, k, p, L, s) == hipSuccess &&
                     hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
                float t = 0.f;
                if (ok && rep > 0 && hipEventElapsedTime(&t, e0, e1) == hipSuccess && t < ms) ms = t;
            }
            if (!ok) { rc = fail(YOLO_ERR_HIP, "yolo_net_autotune: launch failed"); break; }
            if (ms < best) { best = ms; best_tile = tile; }
        }
        if (rc) break;
        k.tile = best_tile;
        net->side_ok.clear();       // (whether a pass splits K -- branch_tails_ok -- depends on the tiles)
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
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

size_t yolo_decode_scratch_bytes(const yolo_head_desc *head, int batch, int cand_capacity) {
    (void)head;
    if (batch <= 0) return 0;
    if (cand_capacity <= 0) cand_capacity = 4096;
    return ((sizeof(Candidate) * (size_t)cand_capacity * batch + 255) & ~(size_t)255) + ((sizeof(int) * (size_t)batch * kCandCountStride + 255) & ~(size_t)255) +
           nms_scratch_bytes(cand_capacity) * (size_t)batch;
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
    if (scratch_bytes < yolo_decode_scratch_bytes(head, batch, cand_capacity)) return fail(YOLO_ERR_ARG, "yolo_decode_nms: scratch too small");
    unsigned char *cand = static_cast<unsigned char *>(scratch_dev);
    int *cnt = reinterpret_cast<int *>(cand + ((sizeof(Candidate) * (size_t)cand_capacity * batch + 255) & ~(size_t)255));
    unsigned char *slabs = reinterpret_cast<unsigned char *>(cnt) + ((sizeof(int) * (size_t)batch * kCandCountStride + 255) & ~(size_t)255);
    return run_decode_nms(*head, logits_dev, batch, threshold, iou_threshold, nms_mode, cand_capacity, max_boxes, cand, cnt,
                          boxes_dev, counts_dev, status_dev, nullptr, static_cast<hipStream_t>(stream), slabs);
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

int yolo_u8_unit_table(float *out256) {
    if (!out256) return fail(YOLO_ERR_ARG, "yolo_u8_unit_table: null argument");
    for (unsigned u = 0; u < 256; ++u) out256[u] = u8_unit(u);     // the function the input kernels run on every byte
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
    const size_t cb = sizeof(Candidate) * (size_t)n, bb = sizeof(yolo_box) * (size_t)n, ib = sizeof(int) * (size_t)n;
    const size_t total = ((cb + 255) & ~(size_t)255) + ((bb + 255) & ~(size_t)255) + ((ib + 255) & ~(size_t)255) + 768 + nms_scratch_bytes(n);
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dev), total));
    unsigned char *d_c = dev, *d_b = d_c + ((cb + 255) & ~(size_t)255), *d_i = d_b + ((bb + 255) & ~(size_t)255);
    int *d_cnt = reinterpret_cast<int *>(d_i + ((ib + 255) & ~(size_t)255));    // [count, kept, status] 256 B apart
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
        np.scratch = reinterpret_cast<unsigned char *>(d_cnt) + 768;      // only used above 4096 boxes
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

// The forward engine behind the C ABI (api.cpp checks arguments and calls in here).  For every kernel kind of a plan: the builder that
// fills its parameter block from (net, Kernel, Ptrs, batch) and, beside it, what yolo_net_kernel_info reports of it (the convs' half of
// both is conv_dispatch.cpp: conv_shape_params / resolve_conv / conv_kernel_info).  Behind them the pass over the kernel list, the
// parts of a batch with their streams, the timed pass, the stream tuner and the tile autotuner.
#include <cstdlib>
#include <cstring>

#include "conv_tiles.h"
#include "yolo_internal.h"

namespace yolo {
namespace {

// packed weights of a kernel; nullptr while no weights are bound (yolo_net_kernel_info / describe build launch parameters of a plan that
// has none yet: no offset is applied to a null pointer -- found by the sanitizer build, tests/test_sanitizer.py)
inline const unsigned char *weights_at(const yolo_net *net, size_t off) { return net->dev_weights ? net->dev_weights + off : nullptr; }
inline const float *floats_at(const yolo_net *net, size_t off) { return reinterpret_cast<const float *>(weights_at(net, off)); }

// One part of a batch: the images a forward pass runs in one activation arena (a whole batch, or its share under several streams)
struct Ptrs {
    yolo_net *net;
    NetIn in;                   // image `img0` of the caller's input
    float *out;                 // ditto, of the caller's output
    int img0 = 0;               // first image of this part in the batch (compact per-image arrays)
    int arena = 0;              // activation arena of this part = its index
    int nb = 0;                 // images
    unsigned char *buf_base(int b) const {
        if (b == BUF_USER_IN) return static_cast<unsigned char *>(const_cast<void *>(in.ptr));
        if (b == BUF_USER_OUT) return reinterpret_cast<unsigned char *>(out);
        return net->dev_ws + (size_t)arena * net->arena_bytes + net->buffers[b].offset;
    }
    // element pointer of channel 0 of pixel 0 of image 0 of the view
    unsigned char *view_ptr(const View &v) const { return buf_base(v.buf) + (size_t)(v.base + v.coff) * (v.f32 ? 4 : net->esize); }
};

// The parts a batch runs as, in order: part_batch(net) images each, the last one what is left.  At most four (plan.cpp: arenas).
struct Parts { int n = 0; Ptrs p[4]; };
Parts split_parts(yolo_net *net, const NetIn in_dev, float *out_dev, int batch) {
    const yolo_layer_desc &d0 = net->layers[0].d;
    const size_t in_img = (size_t)d0.h * d0.w * d0.c;
    const int per = part_batch(net);
    Parts P;
    for (int img0 = 0; img0 < batch && P.n < 4; img0 += per, ++P.n)
        P.p[P.n] = Ptrs{net, in_dev.at((size_t)img0 * in_img), out_dev + (size_t)img0 * net->out_count, img0, P.n, batch - img0 < per ? batch - img0 : per};
    return P;
}

// the report of a kernel that reads one view (+ a residual) and writes another: prep, pool, eltwise
void view_info(const yolo_net *net, const Kernel &k, const char *what, yolo_kernel_info *out) {
    out->out_h = k.out.H; out->out_w = k.out.W; out->cout = k.out.C; out->cin = k.in.C;
    out->bytes = view_elems(k.in) * (k.in.f32 ? 4.0 : net->esize) + view_elems(k.out) * view_esz(net, k.out) + (k.has_res ? view_elems(k.in2) * net->esize : 0.0);
    snprintf(out->name, sizeof out->name, "%s<%s>", what, dtype_tag(net));
}
// ---- K_PREP -------------------------------------------------------------------------------------
void prep_params(const Kernel &k, const Ptrs &P, PrepParams &p) {
    p.in = P.in.ptr;
    p.out = P.view_ptr(k.out);
    p.pixels = (long long)P.nb * k.in.H * k.in.W;
    p.C = k.in.C; p.Cpad = k.out.ld;
}
// ---- K_FIRST ------------------------------------------------------------------------------------
int first_params(const yolo_net *net, const Kernel &k, const Ptrs &P, FirstParams &p) {
    if (!view_chunk_aligned(k.out, net->epc)) return fail(YOLO_ERR_PLAN, "first-layer kernel needs a 16-byte aligned output view");
    p.in = P.in.ptr; p.out = P.view_ptr(k.out);
    p.wgt = floats_at(net, k.w_off); p.bias = floats_at(net, k.b_off);
    p.H = k.in.H; p.W = k.in.W; p.Cout = k.cout; p.out_ld = k.out.ld; p.leaky = k.leaky;
    p.pool = k.pool_fused;
    p.round_half = net->opt.dtype == YOLO_DTYPE_F16;
    p.out_img_stride = k.out.img_stride;
    p.total = (long long)P.nb * k.in.H * k.in.W;
    return YOLO_OK;
}
void first_info(const yolo_net *net, const Kernel &k, yolo_kernel_info *out) {
    out->ksize = 3; out->stride = 1; out->cin = 3; out->cout = k.cout; out->out_h = k.out.H; out->out_w = k.out.W;
    out->flops = 2.0 * k.out.H * k.out.W * k.cout * 27;
    out->bytes = (double)k.in.H * k.in.W * 3 * 4 + view_elems(k.out) * view_esz(net, k.out);
    out->weight_bytes = 28.0 * k.cout * 4;
    snprintf(out->name, sizeof out->name, k.pool_fused ? "conv_first_pool<%s,%d>" : "conv_first<%s,%d>", dtype_tag(net), k.cout);
    if (k.pool_fused) { out->out_h = k.in.H; out->out_w = k.in.W; out->flops = 2.0 * k.in.H * k.in.W * k.cout * 27; }
    set_symbol(out, first_symbol(net->opt.dtype, k.cout, k.pool_fused != 0));
    if (k.stem == STEM_FIRST_FOLDED) {
        out->symbol[0] = 0;          // no launch of its own: accounted for in the conv_stem kernel that follows
        out->flops = 0; out->bytes = 0; out->weight_bytes = 0;
        snprintf(out->name, sizeof out->name, "conv_first<fused into conv_stem>");
    }
}
// ---- the stem (K_CONV with stem == STEM_HOST; its report: conv_dispatch.cpp) ------------------------------
// the first-layer kernel in front of conv `ki` is folded into this launch, and the 1x1 64 -> 32 behind it where the plan says so (STEM_TAIL)
void stem_params(const yolo_net *net, size_t ki, const Ptrs &P, StemParams &p) {
    const Kernel &f = net->kernels[ki - 1], &k = net->kernels[ki];
    memset(&p, 0, sizeof p);
    p.in = P.in.ptr;
    p.w1 = floats_at(net, f.w_off); p.b1 = floats_at(net, f.b_off);
    p.w2 = weights_at(net, k.w_off); p.b2 = floats_at(net, k.b_off);
    p.w2_bytes = (uint32_t)k.w_bytes;
    p.wrow2 = (uint32_t)k.ktiles * 128;
    p.out = P.view_ptr(k.out);
    p.H = f.in.H; p.W = f.in.W; p.Ho = k.out.H; p.Wo = k.out.W;
    p.out_ld = k.out.ld; p.out_img_stride = k.out.img_stride;
    p.in_img_stride = (long long)f.in.H * f.in.W * 3;
    if (ki + 1 < net->kernels.size() && net->kernels[ki + 1].stem == STEM_TAIL) {      // 1x1 64->32 on the same pixels
        const Kernel &t = net->kernels[ki + 1];
        p.w3 = weights_at(net, t.w_off); p.b3 = floats_at(net, t.b_off);
        p.out3 = P.view_ptr(t.out);
        p.out3_ld = t.out.ld; p.out3_img_stride = t.out.img_stride;
    }
}
// ---- K_CONV -------------------------------------------------------------------------------------
// the shape half (conv_dispatch.cpp) + pointers, the byte-limit checks and the objectness block
int conv_params(yolo_net *net, const Kernel &k, const Ptrs &P, ConvParams &p) {
    const int batch = P.nb;
    const long long in_bytes = (long long)batch * k.in.img_stride * net->esize;
    if (in_bytes > 0x7ffffff0LL) return fail(YOLO_ERR_ARG, "conv input tensor exceeds 2 GiB (32-bit buffer addressing): lower the batch");
    if ((long long)batch * net->layers[k.src_layer].H * net->layers[k.src_layer].W > 0x7fffffffLL)
        return fail(YOLO_ERR_ARG, "too many output pixels for one launch");
    conv_shape_params(net, k, batch, p);
    p.in = P.buf_base(k.in.buf);
    p.in_bytes = (uint32_t)in_bytes;
    p.wgt = weights_at(net, k.w_off);
    p.bias = floats_at(net, k.b_off);
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
void attach_fuse2(const yolo_net *net, const Kernel &b, const Ptrs &P, ConvParams &p) {
    p.fuse2 = 1;
    p.w2 = weights_at(net, b.w_off);
    p.w2_bytes = (uint32_t)b.w_bytes;
    p.wrow2_bytes = (uint32_t)b.ktiles * 128;
    p.b2 = floats_at(net, b.b_off);
    p.out2 = P.view_ptr(b.out);
    p.out2_bytes = (uint32_t)((long long)P.nb * b.out.img_stride * net->esize);       // (below 2 GiB: resolve_conv)
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
    return launch_splitk_reduce(reduce_params(p), s);
}
// ---- K_POOL -------------------------------------------------------------------------------------
void pool_params(const Kernel &k, const Ptrs &P, PoolParams &p) {
    p.in = P.view_ptr(k.in);
    p.out = P.view_ptr(k.out);
    p.H = k.in.H; p.W = k.in.W; p.C = k.in.C; p.in_ld = k.in.ld;
    p.Ho = k.out.H; p.Wo = k.out.W; p.out_ld = k.out.ld; p.stride = k.pool_stride;
    p.in_img_stride = k.in.img_stride; p.out_img_stride = k.out.img_stride;
    p.total = (long long)P.nb * k.out.H * k.out.W;
    p.ksize = k.pool_k;
}
// the three pools of an SPP block in one launch
void spp_params(const Kernel &k, const Ptrs &P, SppParams &p) {
    memset(&p, 0, sizeof p);
    p.in = P.view_ptr(k.in);
    p.H = k.in.H; p.W = k.in.W; p.chunks = k.in.C / 8;
    p.in_ld = k.in.ld; p.in_img_stride = k.in.img_stride;
    const View *ov[3] = {&k.out, &k.out2, &k.out3};
    for (int l = 0; l < 3; ++l) {
        p.out[l] = P.view_ptr(*ov[l]);
        p.out_ld[l] = ov[l]->ld; p.out_img_stride[l] = ov[l]->img_stride;
    }
}
void pool_info(const yolo_net *net, const Kernel &k, yolo_kernel_info *out) {
    view_info(net, k, "pool", out);
    const char *t = dtype_tag(net);
    const int epc = net->epc;
    const bool vec = pool_vec_strides(k.in.C, k.in.ld, k.out.ld, k.in.img_stride, k.out.img_stride, epc) && (k.in.base + k.in.coff) % epc == 0 && (k.out.base + k.out.coff) % epc == 0;
    set_symbol(out, aux_symbol(K_POOL, net->opt.dtype, vec));
    if (k.spp) {        // one read, three writes
        out->ksize = k.pool_k; out->stride = 1;
        out->bytes += view_elems(k.out2) * view_esz(net, k.out2) + view_elems(k.out3) * view_esz(net, k.out3);
        snprintf(out->name, sizeof out->name, "spp_pool<%s,%d-%d-%d>", t, k.pool_k, 2 * k.pool_k - 1, 3 * k.pool_k - 2);
        set_symbol(out, spp_pool_symbol((k.pool_k - 1) / 2));
    } else if (k.pool_k != 2) {
        out->ksize = k.pool_k; out->stride = 1;
        snprintf(out->name, sizeof out->name, "pool_same<%s,%dx%d>", t, k.pool_k, k.pool_k);
        set_symbol(out, pool_same_symbol(net->opt.dtype, vec));
    }
}
// ---- K_ELTWISE ----------------------------------------------------------------------------------
void eltwise_params(const yolo_net *net, const Kernel &k, const Ptrs &P, EltParams &p) {
    memset(&p, 0, sizeof p);
    p.a = P.view_ptr(k.in);
    p.a_f32 = k.in.f32;
    p.b = k.has_res ? P.view_ptr(k.in2) : nullptr;
    p.out = P.view_ptr(k.out);
    p.H = k.in.H; p.W = k.in.W; p.C = k.in.C;
    p.a_ld = k.in.ld; p.b_ld = k.in2.ld; p.out_ld = k.out.ld;
    p.outmode = k.outmode;
    p.out_f32 = k.out.f32 || net->opt.dtype == YOLO_DTYPE_F32;
    p.a_img_stride = k.in.img_stride; p.b_img_stride = k.in2.img_stride; p.out_img_stride = k.out.img_stride;
    p.total = (long long)P.nb * k.in.H * k.in.W * k.in.C;
}
// ---- streams ------------------------------------------------------------------------------------
// `ns` non-blocking streams, `nf` + `nj` events without timing, created when the first of them is asked for
bool create_streams(std::vector<hipStream_t> &st, size_t ns, std::vector<hipEvent_t> &fork, size_t nf, std::vector<hipEvent_t> &join, size_t nj) {
    st.assign(ns, nullptr); fork.assign(nf, nullptr); join.assign(nj, nullptr);
    bool ok = true;
    for (hipStream_t &x : st) ok = ok && hipStreamCreateWithFlags(&x, hipStreamNonBlocking) == hipSuccess;
    for (std::vector<hipEvent_t> *ev : {&fork, &join})
        for (hipEvent_t &x : *ev) ok = ok && hipEventCreateWithFlags(&x, hipEventDisableTiming) == hipSuccess;
    return ok;
}
int side_streams(yolo_net *net) {
    StreamPool &sp = net->streams;
    if (sp.side.empty() && !create_streams(sp.side, (size_t)net->parts - 1, sp.fork, 1, sp.join, (size_t)net->parts - 1))
        return fail(YOLO_ERR_HIP, "multi-stream forward: stream/event creation failed");
    return YOLO_OK;
}
int branch_streams(yolo_net *net, int arena) {
    StreamPool &sp = net->streams;
    const size_t n = (size_t)(net->arenas > 0 ? net->arenas : 1);
    if (sp.branch.empty() && !create_streams(sp.branch, n, sp.bfork, 4 * n, sp.bjoin, n))
        return fail(YOLO_ERR_HIP, "branch tail: stream / event creation failed");
    return (size_t)arena < sp.branch.size() ? YOLO_OK : fail(YOLO_ERR_STATE, "branch tail: arena out of range");
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
// ---- the pass -----------------------------------------------------------------------------------
// The kernels of the plan for one part, on stream `s` (ev: an event pair around every kernel, the timed pass).  *obj_rows_out: rows of
// the compact objectness array the head convs of this pass fill.
int run_forward_pass(const Ptrs &P, hipStream_t s, hipEvent_t *ev, long long *obj_rows_out) {
    yolo_net *net = P.net;
    const int dtype = net->opt.dtype, batch = P.nb, arena = P.arena;
    const bool u8 = P.in.u8;
    long long obj_rows_written = 0;
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
        s_branch = net->streams.branch[arena];
    }
    for (size_t ki = 0; ki < net->kernels.size(); ++ki) {
        const Kernel &k = net->kernels[ki];
        hipError_t e = hipSuccess;
        s = s_main;
        if (use_branch && k.side) {
            if (k.side != cur_tail) {
                hipEvent_t ef = net->streams.bfork[(size_t)arena * 4 + (size_t)((k.side - 1) & 3)];
                if (hipEventRecord(ef, s_main) != hipSuccess || hipStreamWaitEvent(s_branch, ef, 0) != hipSuccess)
                    return fail(YOLO_ERR_HIP, "branch tail: fork failed");
                cur_tail = k.side;
            }
            s = s_branch;
        }
        if (ev && hipEventRecord(ev[2 * ki], s) != hipSuccess) return fail(YOLO_ERR_HIP, "hipEventRecord failed");
        bool no_launch = !has_own_launch(k);      // computed by the stem kernel (stem.hip)
        if (k.kind == K_CONV && k.stem == STEM_NONE && k.fuse2_prev && fused2_done) no_launch = true, fused2_done = false;       // computed by the conv in front of it
        if (no_launch) {
        } else if (k.kind == K_PREP) {
            PrepParams p;
            prep_params(k, P, p);
            e = launch_prep(p, dtype, s, u8);
        } else if (k.kind == K_FIRST) {
            FirstParams p;
            const int rc = first_params(net, k, P, p);
            if (rc) return rc;
            e = launch_first(p, dtype, s, u8);
        } else if (k.kind == K_CONV && k.stem == STEM_HOST) {
            StemParams p;
            stem_params(net, ki, P, p);
            e = launch_stem(p, batch, s, net->halves ? kStemGrid / net->parts : kStemGrid, u8);
        } else if (k.kind == K_CONV) {
            ConvParams p;
            const int rc = conv_params(net, k, P, p);
            if (rc) return rc;
            if (k.head && p.obj_out) obj_rows_written += (long long)p.Ho * p.Wo * p.obj_na;
            if (k.mx) {
                e = launch_conv_mx(p, s);
            } else {
                const ConvLaunch L = resolve_conv(net, ki, p, k.tile, arena_slab_data_bytes(net));
                if (L.fuse2) attach_fuse2(net, net->kernels[ki + 1], P, p);
                fused2_done = L.fuse2 != 0;
                e = launch_conv_any(net, k, p, L, s, arena);
            }
        } else if (k.kind == K_POOL && k.spp) {
            SppParams p;
            spp_params(k, P, p);
            e = launch_spp(p, (k.pool_k - 1) / 2, batch, s);
        } else if (k.kind == K_POOL) {
            PoolParams p;
            pool_params(k, P, p);
            e = k.pool_k == 2 ? launch_pool(p, dtype, s) : launch_pool_same(p, dtype, s);
        } else if (k.kind == K_ELTWISE) {
            EltParams p;
            eltwise_params(net, k, P, p);
            e = launch_eltwise(p, dtype, s);
        }
        if (e != hipSuccess) {
            char msg[160];
            snprintf(msg, sizeof msg, "kernel %zu (layer %d) launch failed: %s", ki, k.layer, hipGetErrorString(e));
            return fail(YOLO_ERR_HIP, msg);
        }
        if (ev && hipEventRecord(ev[2 * ki + 1], s) != hipSuccess) return fail(YOLO_ERR_HIP, "hipEventRecord failed");
    }
    if (cur_tail) {
        hipEvent_t ej = net->streams.bjoin[arena];
        if (hipEventRecord(ej, s_branch) != hipSuccess || hipStreamWaitEvent(s_main, ej, 0) != hipSuccess) return fail(YOLO_ERR_HIP, "branch tail: join failed");
    }
    *obj_rows_out = obj_rows_written;
    return YOLO_OK;
}

// One forward: the batch as its parts.  Several parts (YOLO_STREAMS=N, N = 2..4) go out on N streams, the caller's and internal ones,
// fork/join by events: images are independent, so the ragged tail + cold start of every kernel of one part overlaps the bulk of the
// other parts' kernels instead of leaving CUs idle at each of the ~73 kernel boundaries.  Every part has its own activation arena
// (plan.cpp: allocate).
int run_forward_parts(yolo_net *net, const NetIn in_dev, int batch, float *out_dev, hipStream_t s) {
    const long long rows = net->head.n_classes > 0 ? (long long)(net->out_count / (size_t)(5 + net->head.n_classes)) : -1;
    const Parts parts = split_parts(net, in_dev, out_dev, batch);
    const bool multi = parts.n > 1;
    StreamPool &sp = net->streams;
    if (multi) {
        const int rc = side_streams(net);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(sp.fork[0], s));
    }
    net->halves = multi;            // persistent kernels size their grids for a share of the chip
    bool all = true;
    for (int i = 0; i < parts.n; ++i) {
        hipStream_t st = i == 0 ? s : sp.side[i - 1];
        if (i > 0) HIP_TRY(hipStreamWaitEvent(st, sp.fork[0], 0));
        long long w = 0;
        const int rc = run_forward_pass(parts.p[i], st, nullptr, &w);
        if (rc) return rc;
        all = all && w == rows;
    }
    for (int i = 1; i < parts.n; ++i) {
        HIP_TRY(hipEventRecord(sp.join[i - 1], sp.side[i - 1]));
        HIP_TRY(hipStreamWaitEvent(s, sp.join[i - 1], 0));
    }
    net->obj_valid = net->obj_bytes > 0 && rows > 0 && all;
    return YOLO_OK;
}

// after a failed pass: leave the pair-split counters as every later launch expects them; keep the first error's message
int forward_failed(yolo_net *net, int rc) {
    const std::string msg = get_error();
    (void)hipGetLastError();
    (void)zero_pair_counters(net);
    set_error(msg);
    return rc;
}

}  // namespace

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

void destroy_streams(yolo_net *net) {
    StreamPool &sp = net->streams;
    for (std::vector<hipEvent_t> *ev : {&sp.fork, &sp.join, &sp.bfork, &sp.bjoin})
        for (hipEvent_t e : *ev) if (e) (void)hipEventDestroy(e);
    for (std::vector<hipStream_t> *st : {&sp.side, &sp.branch})
        for (hipStream_t x : *st) if (x) (void)hipStreamDestroy(x);
    sp = StreamPool();
}

void aux_kernel_info(const yolo_net *net, int kernel, yolo_kernel_info *out) {
    const Kernel &k = net->kernels[kernel];
    if (k.kind == K_FIRST) return first_info(net, k, out);
    if (k.kind == K_POOL) return pool_info(net, k, out);
    view_info(net, k, k.kind == K_PREP ? "prep" : "eltwise", out);      // prep_params / eltwise_params
    set_symbol(out, aux_symbol(k.kind, net->opt.dtype, false));
}

// (what run_forward finds out afterwards as obj_valid)
bool all_heads_write_objectness(yolo_net *net, const NetIn in_dev, float *out_dev, int batch) {
    if (!net->obj_bytes || net->head.n_classes <= 0) return false;
    const Ptrs P = split_parts(net, in_dev, out_dev, batch).p[0];
    bool any = false;
    for (const Kernel &k : net->kernels) {
        if (k.kind != K_CONV || !k.head) continue;
        ConvParams p;
        if (conv_params(net, k, P, p) != 0 || !p.obj_out) return false;
        // (the rows reach the compact array through the staged float32 epilogue of the LDS-DMA tiles or the 4-wave kernel, or through
        // the split-K reduce kernel: all of them honour obj_out)
        any = true;
    }
    return any;
}

int run_forward(yolo_net *net, const NetIn in_dev, int batch, float *out_dev, hipStream_t s) {
    const int rc = run_forward_parts(net, in_dev, batch, out_dev, s);
    return rc == YOLO_OK ? rc : forward_failed(net, rc);
}

// with several arenas the parts are timed one after the other on the caller's stream (each kernel alone on the chip) and their
// times added per kernel
int run_forward_timed(yolo_net *net, const NetIn in_dev, int batch, float *out_dev, hipStream_t s, float *ms_host) {
    const size_t nk = net->kernels.size();
    std::vector<hipEvent_t> ev(2 * nk, nullptr);
    for (auto &e : ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(YOLO_ERR_HIP, "hipEventCreate failed");
    for (size_t k = 0; k < nk; ++k) ms_host[k] = 0.f;
    net->halves = false;
    const Parts parts = split_parts(net, in_dev, out_dev, batch);
    int rc = YOLO_OK;
    for (int i = 0; rc == YOLO_OK && i < parts.n; ++i) {
        long long w = 0;
        rc = run_forward_pass(parts.p[i], s, ev.data(), &w);
        if (rc == YOLO_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(YOLO_ERR_HIP, "hipStreamSynchronize failed");
        for (size_t k = 0; rc == YOLO_OK && k < nk; ++k) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, ev[2 * k], ev[2 * k + 1]) != hipSuccess) rc = fail(YOLO_ERR_HIP, "hipEventElapsedTime failed");
            ms_host[k] += t;
        }
    }
    net->obj_valid = false;     // (the timed pass is not followed by a decode)
    if (rc != YOLO_OK) forward_failed(net, rc);
    for (auto &e : ev) (void)hipEventDestroy(e);
    return rc;
}

int tune_streams(yolo_net *net, const NetIn in_dev, int batch, hipStream_t s, const char *who) {
    if (!net->arena_full || batch <= (net->opt.max_batch + 1) / 2) return YOLO_OK;       // nothing to choose (or not with this batch)
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
    int rc = YOLO_OK;
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

int autotune_tiles(yolo_net *net, const NetIn in_dev, int batch, hipStream_t s) {
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    if (batch > part_batch(net)) batch = part_batch(net);       // every launch of a multi-stream net sees one part of the batch: tune for that size (arena 0)
    int rc = run_forward(net, in_dev, batch, logits, s);        // real activations in every buffer
    if (rc) return rc;
    const Ptrs P = split_parts(net, in_dev, logits, batch).p[0];
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    for (size_t ki = 0; ki < net->kernels.size(); ++ki) {
        Kernel &k = net->kernels[ki];
        if (!conv_dispatched(k) || k.mx || !dma_eligible(net, k)) continue;      // (MX convs: one kernel, weights packed for it)
        ConvParams p;
        rc = conv_params(net, k, P, p);
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

}  // namespace yolo

// The training half of the C ABI (declared in include/yolo_hip.h): the operators under a training step (weight gradients, data gradient,
// Adam) and the four paths that train convs of a net on the device -- the YOLOv2 detection layer (`head`), the 3 x 3 block behind it and
// the detection layer (`tail`), the YOLOv3 head convs (`heads`), those and the 3 x 3 block behind each (`head_blocks`).  Each path is
// explicit: which convs it trains (head_conv, tail_convs, head_convs_v3, block_convs_v3), its state layout, init, read, and a step that is a list of launches.  What the paths have in common is written once,
// in the anonymous namespace below: the record of one trained conv, the state arena, the packing of a 1 x 1 conv, the Adam parameter
// block, the checks of a step.  The checks and launch helpers shared with api.cpp are declared in yolo_internal.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "yolo_internal.h"

using namespace yolo;

namespace {

// ---- one launch each -----------------------------------------------------------------------------------------------------------------------
int run_wgrad(const void *x, int x_dtype, int ld, int coff, long long image_stride, int ppi, int batch, int cin, const float *g, int cout,
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

int run_dgrad(const float *g, int cout, const float *w, int cin, const void *y, int y_dtype, int ld, int coff, long long image_stride, int ppi,
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

int run_wgrad3x3(const void *x, int x_dtype, int ld, int coff, long long image_stride, int h, int w, int batch, int cin, const float *d, int cout,
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

int run_wgrad3x3_f16(const void *x, int ld, int coff, long long image_stride, int h, int w, int batch, int cin, const float *d, int cout,
                     const float *scale, float *dw, float *db, void *scratch, const struct yolo_conv3x3_wgrad_f16_plan &pl, hipStream_t s) {
    Wgrad3x3Params p;
    memset(&p, 0, sizeof p);
    p.x = x; p.d = d; p.scale = scale; p.slab = static_cast<float *>(scratch); p.dw = dw; p.db = db;
    p.P = h * w * batch; p.cin = cin; p.cout = cout; p.ld = ld; p.coff = coff; p.h = h; p.w = w; p.ppi = h * w; p.img_stride = image_stride;
    p.ppc = pl.positions_per_chunk; p.n_chunks = pl.n_chunks; p.tiles_cout = pl.tiles_cout; p.tiles_cin = pl.tiles_cin; p.halo_rows = pl.halo_rows;
    p.slab_stride = cout * (9 * cin + 1);
    HIP_TRY(launch_conv3x3_wgrad_f16(p, reinterpret_cast<unsigned int *>(static_cast<unsigned char *>(scratch) + pl.record_offset), pl.db_groups,
                                     pl.db_positions, s));
    return YOLO_OK;
}

int run_wgrad3(const Wgrad3Geometry &geo, const struct yolo_v3_wgrad_plan &pl, int batch, const float *g, const int32_t *assign, int max_gt,
               void *scratch, hipStream_t s) {
    Wgrad3Params p;
    memset(&p, 0, sizeof p);
    static_cast<Wgrad3Geometry &>(p) = geo;
    p.g = g; p.assign = assign; p.batch = batch; p.max_gt = max_gt;
    p.slot = reinterpret_cast<int *>(static_cast<unsigned char *>(scratch) + pl.slot_offset);
    HIP_TRY(launch_head3_wgrad(p, s));
    return YOLO_OK;
}

// ---- what the three paths share ------------------------------------------------------------------------------------------------------------
// the activations of a net are fp16 or float32 (an MXFP8 plan keeps fp16 storage)
int net_x_dtype(const yolo_net *net) { return net->opt.dtype == YOLO_DTYPE_F16 ? YOLO_DTYPE_F16 : YOLO_DTYPE_F32; }

// the parts of a training state lie one behind the other, each from a 256-byte boundary
struct Arena {
    size_t off = 0;
    uint64_t part(size_t bytes) { const size_t at = off; off = align256(off + bytes); return (uint64_t)at; }
};

// One conv that a step updates: its kernel of the plan and the byte offsets of its eight arrays in the state -- float32 master kernel
// [cout][row] and bias, Adam's two moments of each, the two gradients.  row: cin of a 1 x 1 conv, 9 * cin of the 3 x 3 block ([t][c]).
struct TrainedConv {
    const Kernel *k;
    size_t row, n_w, n_b;
    uint64_t w, b, m_w, v_w, m_b, v_b, dw, db;
};

// ... laid out in this order, and reported in the eight fields of a public layout struct
void place(TrainedConv &c, const Kernel *k, Arena &a, uint64_t &w, uint64_t &b, uint64_t &m_w, uint64_t &v_w, uint64_t &m_b, uint64_t &v_b, uint64_t &dw, uint64_t &db) {
    c.k = k;
    c.row = (size_t)k->ksize * k->ksize * k->cin; c.n_w = (size_t)k->cout * c.row; c.n_b = (size_t)k->cout;
    w = c.w = a.part(c.n_w * 4); b = c.b = a.part(c.n_b * 4);
    m_w = c.m_w = a.part(c.n_w * 4); v_w = c.v_w = a.part(c.n_w * 4); m_b = c.m_b = a.part(c.n_b * 4); v_b = c.v_b = a.part(c.n_b * 4);
    dw = c.dw = a.part(c.n_w * 4); db = c.db = a.part(c.n_b * 4);
}

// master values from the host, zeroed moments
int start_state(const TrainedConv &c, unsigned char *st, const float *w_host, const float *b_host) {
    HIP_TRY(hipMemcpy(st + c.w, w_host, c.n_w * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + c.b, b_host, c.n_b * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(st + c.m_w, 0, (size_t)(c.dw - c.m_w)));       // the four moment arrays lie one behind the other
    return YOLO_OK;
}

int read_state(const TrainedConv &c, const unsigned char *st, float *w_host, float *b_host) {
    HIP_TRY(hipMemcpy(w_host, st + c.w, c.n_w * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(b_host, st + c.b, c.n_b * 4, hipMemcpyDeviceToHost));
    return YOLO_OK;
}

// A 1 x 1 conv's float32 master rows into the device weights, as pack_weights (weights.cpp) writes a 1 x 1 conv without batch norm: row o
// at o * wrow bytes, fp16 (one rounding, as the loader's) or float32, bias as it is
int pack_conv1x1(const yolo_net *net, const Kernel *k, const float *w_host, const float *b_host) {
    const size_t wrow = (size_t)k->ktiles * 128;
    const bool f16 = net_x_dtype(net) == YOLO_DTYPE_F16;
    std::vector<unsigned char> rows((size_t)k->cout * wrow, 0);
    for (int o = 0; o < k->cout; ++o)
        for (int c = 0; c < k->cin; ++c) {
            const float v = w_host[(size_t)o * k->cin + c];
            if (f16) reinterpret_cast<_Float16 *>(rows.data() + (size_t)o * wrow)[c] = (_Float16)v;
            else reinterpret_cast<float *>(rows.data() + (size_t)o * wrow)[c] = v;
        }
    HIP_TRY(hipMemcpy(net->dev_weights + k->w_off, rows.data(), rows.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(net->dev_weights + k->b_off, b_host, (size_t)k->cout * 4, hipMemcpyHostToDevice));
    return YOLO_OK;
}

// The Adam update of one trained conv with the re-pack of its row into the device weights (train.hip: adam_step_kernel).  A master row
// of the block is a packed row's first 9 * cin elements too (cin_s == cin: element t * cin + c of one is element t * cin_s + c of the other).
AdamParams adam_params(const yolo_net *net, const TrainedConv &c, unsigned char *st, float lr_t) {
    auto f32 = [&](uint64_t o) { return reinterpret_cast<float *>(st + o); };
    AdamParams p;
    memset(&p, 0, sizeof p);
    p.w = f32(c.w); p.b = f32(c.b); p.m_w = f32(c.m_w); p.v_w = f32(c.v_w); p.m_b = f32(c.m_b); p.v_b = f32(c.v_b);
    p.dw = f32(c.dw); p.db = f32(c.db); p.n_w = (long long)c.n_w; p.n_b = (long long)c.n_b;
    p.lr_t = lr_t; p.beta1 = 0.9f; p.beta2 = 0.999f; p.eps = 1e-8f;        // tf.train.AdamOptimizer's defaults (net/v2.py:205)
    p.pack_w = net->dev_weights + c.k->w_off; p.pack_b = reinterpret_cast<float *>(net->dev_weights + c.k->b_off);
    p.pack_cin = (int)c.row; p.pack_f16 = net_x_dtype(net) == YOLO_DTYPE_F16;
    p.pack_row = (int)((size_t)c.k->ktiles * 128 / (p.pack_f16 ? 2 : 4));
    return p;
}

// where a kernel's input lives in the workspace after a dense forward
yolo_tensor_view view_of(const yolo_net *net, const Kernel *k) {
    yolo_tensor_view v;
    memset(&v, 0, sizeof v);
    v.offset = net->buffers[k->in.buf].offset; v.image_stride = k->in.img_stride; v.ld = k->in.ld; v.coff = k->in.coff;
    v.dtype = net_x_dtype(net); v.cin = k->cin; v.h = k->in.H; v.w = k->in.W;
    return v;
}

// The last part of every state: scratch for the largest split of any batch 1 .. max_batch -- a smaller batch never needs more chunks than
// the full one at the same tile counts, but its chunks may be laid out otherwise.  plan_bytes(n, &bytes, err) asks the split of batch n.
// (The plans are asked at YOLO_DTYPE_F32 whatever the net stores: scratch_bytes of wgrad_plan, wgrad3x3_plan and wgrad3_plan does not depend on x_dtype.)
template <class Layout, class F>
int place_scratch(const yolo_net *net, Layout *L, Arena &a, const char *who, F plan_bytes) {
    std::string err;
    uint64_t need = 0;
    for (int n = 1; n <= net->opt.max_batch; ++n) {
        uint64_t bytes = 0;
        const int rc = plan_bytes(n, &bytes, err);
        if (rc) return fail(rc, std::string(who) + ": " + err);
        if (bytes > need) need = bytes;
    }
    L->scratch_bytes = need;
    L->scratch_offset = a.part((size_t)need);
    L->total_bytes = a.off;
    return YOLO_OK;
}

int head_set(const yolo_net *net, const char *who) {
    std::string err;
    if (!check_head(&net->head, net->out_count, err)) return YOLO_OK;
    return fail(YOLO_ERR_STATE, std::string(who) + ": head geometry not set (" + err + "); call yolo_net_set_head");
}

int head_set_v2(const yolo_net *net, const char *who) {
    const int rc = head_set(net, who);
    if (rc) return rc;
    if (net->head.version != 2 || net->head.n_scales != 1)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the head must be version 2 with one scale (the reference has a loss for YOLOv2 only)");
    return YOLO_OK;
}

// the trained tensors live in the one arena of a single pass
int one_part(const yolo_net *net, const char *who) {
    if (net->parts != 1)
        return fail(YOLO_ERR_STATE, std::string(who) + ": this net runs a batch as " + std::to_string(net->parts) +
                                        " stream parts, each in its own arena; call yolo_net_set_streams(net, 1)");
    return YOLO_OK;
}

// Is k a detection conv -- 1 x 1 / stride 1, linear, bias and no batch norm, writing logits (`fits`: whatever else the caller asks of its
// shape) -- whose input the plan left alone as a tensor of the workspace?  `at` opens the message, `shape` is the refusal of another kind
// of kernel, `noun` is what the other two messages call it.
int detection_conv(const Kernel &k, bool fits, const std::string &at, const char *shape, const char *noun) {
    if (k.kind != K_CONV || k.ksize != 1 || k.stride != 1 || k.leaky || k.batch_norm || k.out.buf != BUF_USER_OUT || !k.out.f32 || k.has_res ||
        k.outmode != OUT_NORMAL || !fits)
        return fail(YOLO_ERR_ARG, at + shape);
    if (k.stem || k.fuse2_prev || k.mx || k.in.buf < 0 || k.in.f32 || k.in.base)
        return fail(YOLO_ERR_STATE, at + "the plan has fused the " + noun + "'s input away");
    if (k.cin % 8 || k.cin_s != k.cin) return fail(YOLO_ERR_ARG, at + "the " + noun + "'s input channels must be a multiple of 8");
    return YOLO_OK;
}

// Is buffer `buf` still intact behind the last kernel of a pass?  No kernel from `from` on writes it, and no buffer alive later shares
// its bytes.  `at` opens the message up to what is reused ("...: the plan reuses the block's input: "), `behind` closes the first one.
int input_intact(const yolo_net *net, int from, int buf, const std::string &at, const char *behind) {
    const std::vector<Kernel> &K = net->kernels;
    const Buffer &b = net->buffers[buf];
    for (int j = from; j < (int)K.size(); ++j)
        for (const View *v : {&K[j].out, &K[j].out2, &K[j].out3})
            if (v->buf == buf) return fail(YOLO_ERR_STATE, at + "kernel " + std::to_string(j) + " writes its buffer" + behind);
    for (size_t q = 0; q < net->buffers.size(); ++q) {
        const Buffer &o = net->buffers[q];
        if ((int)q == buf || o.last < 0 || !o.bytes || !b.bytes) continue;
        const bool shares = o.offset < b.offset + b.bytes && b.offset < o.offset + o.bytes;
        if (shares && o.last >= b.first) return fail(YOLO_ERR_STATE, at + "buffer " + std::to_string(q) + " shares its bytes and is alive behind it");
    }
    return YOLO_OK;
}

// The checks of a *_train_init behind its layout.
int init_checks(const yolo_net *net, const void *state_dev, size_t bytes, uint64_t total, const char *bytes_entry, const char *who) {
    if (bytes < total) return fail(YOLO_ERR_ARG, std::string(who) + ": state too small (" + bytes_entry + ")");
    if ((uintptr_t)state_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the state must be 256-byte aligned");
    if (!net->weights_loaded || !net->dev_weights) return fail(YOLO_ERR_STATE, std::string(who) + ": weights not loaded");
    return YOLO_OK;
}

// The checks of a step behind its layout, in the order every step makes them: the state, the loss arguments (loss_check: the path's own,
// the batch among them), the net, the step size.
template <class F>
int step_checks(yolo_net *net, const void *in, int batch, const void *state_dev, float lr_t, const char *init_entry, const char *who, F loss_check) {
    if (!state_dev) return fail(YOLO_ERR_ARG, std::string(who) + ": null state (" + init_entry + ")");
    if ((uintptr_t)state_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the state must be 256-byte aligned");
    int rc = loss_check();
    if (!rc) rc = check_ready(net, in, batch, who);
    if (rc) return rc;
    if (!(lr_t == lr_t)) return fail(YOLO_ERR_ARG, std::string(who) + ": lr_t is NaN");
    return YOLO_OK;
}

// ... and the loss_check of the two YOLOv2 paths
int loss_check_v2(const yolo_net *net, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt, const void *images,
                  const yolo_loss_result *result_dev, const char *who) {
    const int rc = check_loss_args(&net->head, gt_dev, gt_counts_dev, max_gt, images, result_dev, who);
    if (rc) return rc;
    return batch < 1 ? fail(YOLO_ERR_ARG, std::string(who) + ": batch must be at least 1") : YOLO_OK;
}

// ---- which convs a path trains -------------------------------------------------------------------------------------------------------------
// The detection layer of a net: the last kernel of the plan, if it is the 1 x 1 / stride 1 linear conv with bias that writes the logits
// from a tensor of the workspace (plan.cpp; net/v2.py:52-56).  The message says what is in the way.
int head_conv(const yolo_net *net, const Kernel **out, const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (net->kernels.empty()) return fail(YOLO_ERR_ARG, std::string(who) + ": the plan has no kernels");
    const Kernel &k = net->kernels.back();
    int rc = detection_conv(k, true, std::string(who) + ": ",
                            "the last kernel of the plan must be the detection layer, a 1 x 1 / stride 1 linear conv with "
                            "bias and no batch norm that writes the logits (the YOLOv2 networks; v3 heads are not trained)",
                            "detection layer");
    if (!rc) rc = one_part(net, who);
    if (rc) return rc;
    *out = &k;
    return YOLO_OK;
}

// The block behind a detection conv k (`noun`: "the detection layer", "the head conv"): the one kernel that writes k's input, if it is a
// 3 x 3 / stride 1 conv with batch norm and leaky ReLU that the plan runs on its own, from a tensor of the workspace that is still intact
// behind the last kernel of the pass.  `at` opens the message, which says what is in the way.  Shared by the YOLOv2 tail and the blocks
// behind the YOLOv3 heads.
int block_behind(const yolo_net *net, const Kernel *k, const std::string &at, const std::string &noun, const Kernel **block) {
    const std::vector<Kernel> &K = net->kernels;
    const int ki = (int)(k - K.data());
    int bi = -1, writers = 0;
    for (int j = 0; j < ki; ++j)
        for (const View *v : {&K[j].out, &K[j].out2, &K[j].out3})
            if (v->buf == k->in.buf) { bi = j; ++writers; }
    const std::string conv = "the conv behind " + noun;
    if (writers != 1)
        return fail(YOLO_ERR_ARG, at + noun + "'s input is written by " + std::to_string(writers) + " kernels (a concatenation or the network input): "
                                       "there is no single 3 x 3 block behind " + noun);
    const Kernel &b = K[bi];
    if (b.kind != K_CONV || b.out.buf != k->in.buf)
        return fail(YOLO_ERR_ARG, at + noun + "'s input is not written by a conv (kernel " + std::to_string(bi) + ")");
    if (b.ksize != 3 || b.stride != 1) return fail(YOLO_ERR_ARG, at + conv + " must be 3 x 3 / stride 1 (1 x 1 and stride-2 blocks are not trained)");
    if (!b.batch_norm || !b.leaky) return fail(YOLO_ERR_ARG, at + conv + " must have batch norm and a leaky ReLU");
    if (b.has_res) return fail(YOLO_ERR_ARG, at + conv + " carries a residual (a shortcut is fused into it): its output is not the block's alone");
    if (b.mx) return fail(YOLO_ERR_STATE, at + "the plan runs " + conv + " as an MXFP8 conv: its packed weights are block-scaled fp8 (use an fp16 or fp32 plan)");
    if (b.outmode != OUT_NORMAL) return fail(YOLO_ERR_STATE, at + "the plan has fused a pool, reorg or upsample into " + conv);
    if (b.stem != STEM_NONE || b.fuse2_next || b.fuse2_prev) return fail(YOLO_ERR_STATE, at + "the plan has fused " + conv + " with a neighbour");
    if (b.out.coff != k->in.coff || b.out.ld != k->in.ld || b.out.img_stride != k->in.img_stride || b.out.base != k->in.base || b.cout != k->cin ||
        b.out.H != k->in.H || b.out.W != k->in.W || b.out.f32)
        return fail(YOLO_ERR_ARG, at + conv + " does not write exactly " + noun + "'s input");
    if (b.in.buf < 0 || b.in.f32 || b.in.base) return fail(YOLO_ERR_STATE, at + "the input of " + conv + " is not a tensor of the workspace");
    if (b.cin % 8 || b.cin_s != b.cin) return fail(YOLO_ERR_ARG, at + "the input channels of " + conv + " must be a multiple of 8");
    if (b.in.W > kTailMaxW) return fail(YOLO_ERR_ARG, at + "the feature map of " + conv + " is wider than " + std::to_string(kTailMaxW));
    const int rc = input_intact(net, bi, b.in.buf, at + "the plan reuses the block's input: ", "");
    if (rc) return rc;
    *block = &b;
    return YOLO_OK;
}

// The tail of a YOLOv2 net: the detection layer and the block behind it.
int tail_convs(const yolo_net *net, const Kernel **block, const Kernel **head, const char *who) {
    const Kernel *k = nullptr;
    int rc = head_conv(net, &k, who);
    if (rc) return rc;
    if (k->out.base || (size_t)k->cout * k->in.H * k->in.W != net->out_count)
        return fail(YOLO_ERR_ARG, std::string(who) + ": the last kernel writes one scale of several: a v3 network has no tail of this kind (its detection convs are "
                                                     "trained with yolo_net_train_head_step_v3, train_layers = heads)");
    rc = block_behind(net, k, std::string(who) + ": ", "the detection layer", block);
    if (rc) return rc;
    *head = k;
    return YOLO_OK;
}

// The head convs of a version 3 net in head order, each the 1 x 1 / stride 1 linear conv with bias that writes its scale of the logits from
// a tensor of the workspace that is still intact behind the last kernel of the pass.  The message says what is in the way.
int head_convs_v3(const yolo_net *net, const Kernel *out[YOLO_MAX_SCALES], const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    int rc = head_set(net, who);
    if (rc) return rc;
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
        const Kernel &k = K[heads[s]];
        const std::string at = std::string(who) + ": scale " + std::to_string(s) + ": ";
        rc = detection_conv(k, k.cout == net->head.n_anchors[s] * width && k.in.H == net->head.h[s] && k.in.W == net->head.w[s], at,
                            "the head conv must be a 1 x 1 / stride 1 linear conv with bias and no batch norm that writes this scale of the logits", "head conv");
        if (!rc) rc = input_intact(net, heads[s] + 1, k.in.buf, at + "the plan reuses the head conv's input: ", " behind the head conv");
        if (rc) return rc;
        out[s] = &k;
    }
    return one_part(net, who);
}

// The head convs of a version 3 net and, per scale, the block behind each (block_behind's checks).
int block_convs_v3(const yolo_net *net, const Kernel *blocks[YOLO_MAX_SCALES], const Kernel *heads[YOLO_MAX_SCALES], const char *who) {
    int rc = head_convs_v3(net, heads, who);
    for (int s = 0; !rc && s < net->head.n_scales; ++s)
        rc = block_behind(net, heads[s], std::string(who) + ": scale " + std::to_string(s) + ": ", "the head conv", &blocks[s]);
    return rc;
}

// ---- the state of each path: the trained convs first, then what a step keeps between its launches, the scratch last ------------------------
struct HeadTrain { TrainedConv head; yolo_head_train_layout L; };
struct TailTrain { TrainedConv head, block; yolo_tail_train_layout L; };
struct HeadsTrain { TrainedConv sc[YOLO_MAX_SCALES]; yolo_head_train_v3_layout L; };
struct BlocksTrain { TrainedConv head[YOLO_MAX_SCALES], block[YOLO_MAX_SCALES]; yolo_blocks_train_v3_layout L; };

int head_train_layout(const yolo_net *net, HeadTrain *t, const char *who) {
    const Kernel *k = nullptr;
    int rc = head_conv(net, &k, who);
    if (!rc) rc = head_set_v2(net, who);
    if (rc) return rc;
    const size_t mb = (size_t)net->opt.max_batch, hw = (size_t)k->in.H * k->in.W;
    yolo_head_train_layout *L = &t->L;
    Arena a;
    memset(L, 0, sizeof *L);
    place(t->head, k, a, L->w_offset, L->b_offset, L->m_w_offset, L->v_w_offset, L->m_b_offset, L->v_b_offset, L->dw_offset, L->db_offset);
    L->grad_offset = a.part(mb * net->out_count * 4);
    L->assign_offset = a.part(mb * hw * 4);
    L->images_offset = a.part(mb * sizeof(yolo_loss_image));
    L->cin = k->cin; L->cout = k->cout;
    return place_scratch(net, L, a, who, [&](int n, uint64_t *bytes, std::string &err) {
        struct yolo_wgrad_plan q = {};
        const int r = wgrad_plan((long long)n * (long long)hw, k->cin, k->cout, YOLO_DTYPE_F32, &q, err);
        *bytes = q.scratch_bytes;
        return r;
    });
}

int tail_train_layout(const yolo_net *net, TailTrain *t, const char *who) {
    const Kernel *b = nullptr, *k = nullptr;
    int rc = tail_convs(net, &b, &k, who);
    if (!rc) rc = head_set_v2(net, who);
    if (rc) return rc;
    const size_t mb = (size_t)net->opt.max_batch, hw = (size_t)k->in.H * k->in.W, nb3 = (size_t)b->cout * 4;
    yolo_tail_train_layout *L = &t->L;
    Arena a;
    memset(L, 0, sizeof *L);
    place(t->head, k, a, L->w_offset, L->b_offset, L->m_w_offset, L->v_w_offset, L->m_b_offset, L->v_b_offset, L->dw_offset, L->db_offset);
    place(t->block, b, a, L->w3_offset, L->beta_offset, L->m_w3_offset, L->v_w3_offset, L->m_beta_offset, L->v_beta_offset, L->dw3_offset, L->dbeta_offset);
    L->scale64_offset = a.part((size_t)b->cout * 8); L->scale32_offset = a.part(nb3); L->mean_offset = a.part(nb3);
    L->d_offset = a.part(mb * hw * (size_t)b->cout * 4);
    L->grad_offset = a.part(mb * net->out_count * 4);
    L->assign_offset = a.part(mb * hw * 4);
    L->images_offset = a.part(mb * sizeof(yolo_loss_image));
    L->block_src = b->w_src; L->head_src = k->w_src;
    L->cin = k->cin; L->cout = k->cout; L->cin3 = b->cin; L->cout3 = b->cout;
    // one scratch for both weight gradients, which run one after the other
    return place_scratch(net, L, a, who, [&](int n, uint64_t *bytes, std::string &err) {
        struct yolo_wgrad_plan q = {};
        struct yolo_conv3x3_wgrad_plan q3 = {};
        int r = wgrad_plan((long long)n * (long long)hw, k->cin, k->cout, YOLO_DTYPE_F32, &q, err);
        if (!r) r = wgrad3x3_plan(b->in.H, b->in.W, n, b->cin, b->cout, YOLO_DTYPE_F32, &q3, err);
        *bytes = std::max(q.scratch_bytes, q3.scratch_bytes);
        return r;
    });
}

int head_train_v3_layout(const yolo_net *net, HeadsTrain *t, const char *who) {
    const Kernel *ks[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    int rc = head_convs_v3(net, ks, who);
    if (rc) return rc;
    std::string err;
    Loss3Geometry lg;
    rc = loss3_geometry(&net->head, &lg, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    const size_t mb = (size_t)net->opt.max_batch;
    yolo_head_train_v3_layout *L = &t->L;
    Arena a;
    memset(L, 0, sizeof *L);
    L->n_scales = net->head.n_scales;
    for (int s = 0; s < L->n_scales; ++s) {
        L->cin[s] = ks[s]->cin; L->cout[s] = ks[s]->cout;
        L->bias_src[s] = ks[s]->w_src;
        place(t->sc[s], ks[s], a, L->w_offset[s], L->b_offset[s], L->m_w_offset[s], L->v_w_offset[s], L->m_b_offset[s], L->v_b_offset[s], L->dw_offset[s], L->db_offset[s]);
    }
    L->grad_offset = a.part(mb * net->out_count * 4);
    L->assign_offset = a.part(mb * (size_t)lg.rows * 4);
    L->parts_offset = a.part(mb * (size_t)lg.parts * sizeof(yolo_loss_image));
    L->images_offset = a.part(mb * sizeof(yolo_loss_image));
    return place_scratch(net, L, a, who, [&](int n, uint64_t *bytes, std::string &e) {
        struct yolo_v3_wgrad_plan q = {};
        Wgrad3Geometry g;
        const int r = wgrad3_plan(&net->head, L->cin, n, YOLO_DTYPE_F32, &q, &g, e);
        *bytes = q.scratch_bytes;
        return r;
    });
}

int blocks_train_v3_layout(const yolo_net *net, BlocksTrain *t, const char *who) {
    const Kernel *bs[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr}, *ks[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    int rc = block_convs_v3(net, bs, ks, who);
    if (rc) return rc;
    std::string err;
    Loss3Geometry lg;
    rc = loss3_geometry(&net->head, &lg, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    const size_t mb = (size_t)net->opt.max_batch;
    yolo_blocks_train_v3_layout *L = &t->L;
    Arena a;
    memset(L, 0, sizeof *L);
    L->n_scales = net->head.n_scales;
    size_t d_floats = 0;
    for (int s = 0; s < L->n_scales; ++s) {
        const Kernel *k = ks[s], *b = bs[s];
        L->cin[s] = k->cin; L->cout[s] = k->cout; L->cin3[s] = b->cin; L->cout3[s] = b->cout;
        L->bias_src[s] = k->w_src; L->block_src[s] = b->w_src;
        place(t->head[s], k, a, L->w_offset[s], L->b_offset[s], L->m_w_offset[s], L->v_w_offset[s], L->m_b_offset[s], L->v_b_offset[s], L->dw_offset[s], L->db_offset[s]);
        place(t->block[s], b, a, L->w3_offset[s], L->beta_offset[s], L->m_w3_offset[s], L->v_w3_offset[s], L->m_beta_offset[s], L->v_beta_offset[s],
              L->dw3_offset[s], L->dbeta_offset[s]);
        L->scale64_offset[s] = a.part((size_t)b->cout * 8); L->scale32_offset[s] = a.part((size_t)b->cout * 4); L->mean_offset[s] = a.part((size_t)b->cout * 4);
        d_floats = std::max(d_floats, (size_t)k->in.H * k->in.W * (size_t)b->cout);
    }
    L->d_offset = a.part(mb * d_floats * 4);        // one D: the scales run one after the other on one stream
    L->grad_offset = a.part(mb * net->out_count * 4);
    L->assign_offset = a.part(mb * (size_t)lg.rows * 4);
    L->parts_offset = a.part(mb * (size_t)lg.parts * sizeof(yolo_loss_image));
    L->images_offset = a.part(mb * sizeof(yolo_loss_image));
    // one scratch for the heads' weight gradient and every block's, which run one after the other
    return place_scratch(net, L, a, who, [&](int n, uint64_t *bytes, std::string &e) {
        struct yolo_v3_wgrad_plan q = {};
        Wgrad3Geometry g;
        int r = wgrad3_plan(&net->head, L->cin, n, YOLO_DTYPE_F32, &q, &g, e);
        *bytes = q.scratch_bytes;
        for (int s = 0; !r && s < L->n_scales; ++s) {
            struct yolo_conv3x3_wgrad_plan q3 = {};
            r = wgrad3x3_plan(bs[s]->in.H, bs[s]->in.W, n, bs[s]->cin, bs[s]->cout, YOLO_DTYPE_F32, &q3, e);
            *bytes = std::max(*bytes, q3.scratch_bytes);
        }
        return r;
    });
}

// The scratch yolo_conv3x3_wgrad_f16 needs on this net: the largest over its trainable 3 x 3 blocks -- the tail block of a version 2 net,
// every head block of a version 3 net -- and, as place_scratch, over the batches 1 .. max_batch.
int wgrad_f16_need(const yolo_net *net, uint64_t *need, const char *who) {
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    const Kernel *bs[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr}, *ks[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    int n_blocks = 1, rc;
    std::string unset;
    if (!check_head(&net->head, net->out_count, unset) && net->head.version == 3) {
        rc = block_convs_v3(net, bs, ks, who);
        n_blocks = net->head.n_scales;
    } else {
        rc = tail_convs(net, &bs[0], &ks[0], who);
    }
    if (rc) return rc;
    if (net_x_dtype(net) != YOLO_DTYPE_F16)
        return fail(YOLO_ERR_STATE, std::string(who) + ": a float32 plan stores float32 activations: yolo_conv3x3_wgrad_f16 reads X3 as stored fp16 (use an fp16 plan)");
    std::string err;
    *need = 0;
    for (int s = 0; s < n_blocks; ++s)
        for (int n = 1; n <= net->opt.max_batch; ++n) {
            struct yolo_conv3x3_wgrad_f16_plan q = {};
            rc = wgrad3x3_f16_plan(bs[s]->in.H, bs[s]->in.W, n, bs[s]->cin, bs[s]->cout, &q, err);
            if (rc) return fail(rc, std::string(who) + ": " + err);
            *need = std::max(*need, q.scratch_bytes);
        }
    return YOLO_OK;
}

// ---- a 3 x 3 block's piece of the Darknet stream into a state and the device weights, and back ------------------------------------------------
// Do a block's packed rows fit its weight region?  Asked for every block of an init BEFORE its first copy: a refused init changes nothing.
int block_rows_fit(const Kernel *b, const std::string &who) {
    if ((size_t)b->cout * ((size_t)b->ktiles * 128) > b->w_bytes) return fail(YOLO_ERR_PLAN, who + ": the block's packed rows do not fit its weight region");
    return YOLO_OK;
}

// block_host: beta, gamma, mean, var [cout3 each], then the kernel [out][in][kh][kw] (net/layers.py:53-63).  The fold as weights.cpp:
// fold_batch_norm; masters, zeroed moments, scale64 / scale32 / mean into the state, the packed rows and the folded bias into the net.
int init_block(const yolo_net *net, const TrainedConv &blk, unsigned char *st, const float *block_host, uint64_t scale64_off, uint64_t scale32_off,
               uint64_t mean_off, const std::string &who) {
    const Kernel *b = blk.k;
    const bool f16 = net_x_dtype(net) == YOLO_DTYPE_F16;
    const int c3 = b->cout, ci3 = b->cin;
    const size_t nb3 = (size_t)c3 * 4;
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
        for (int tap = 0; tap < 9; ++tap)
            for (int c = 0; c < ci3; ++c) {
                const float w = kern[((size_t)o * ci3 + c) * 9 + tap];
                w3[((size_t)o * 9 + tap) * ci3 + c] = w;
                // (fp16: one rounding from the float64 product, which is what pack_weights' (_Float16)(float) compiles to on the host)
                const double v = (double)w * scale64[o];
                const size_t e = (size_t)tap * b->cin_s + c;
                if (f16) reinterpret_cast<_Float16 *>(rows3.data() + (size_t)o * wrow3)[e] = (_Float16)v;
                else reinterpret_cast<float *>(rows3.data() + (size_t)o * wrow3)[e] = (float)v;
            }
    const int rc = start_state(blk, st, w3.data(), beta);       // (the caller has asked block_rows_fit)
    if (rc) return rc;
    HIP_TRY(hipMemcpy(st + scale64_off, scale64.data(), (size_t)c3 * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + scale32_off, scale32.data(), nb3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st + mean_off, mean, nb3, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(net->dev_weights + b->w_off, rows3.data(), rows3.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(net->dev_weights + b->b_off, bfold.data(), nb3, hipMemcpyHostToDevice));
    return YOLO_OK;
}

// the block's masters back, the kernel converted to [out][in][kh][kw]
int read_block(const TrainedConv &blk, const unsigned char *st, float *block_kernel_host, float *beta_host) {
    const Kernel *b = blk.k;
    std::vector<float> w3(blk.n_w);
    const int rc = read_state(blk, st, w3.data(), beta_host);
    if (rc) return rc;
    for (int o = 0; o < b->cout; ++o)
        for (int tap = 0; tap < 9; ++tap)
            for (int c = 0; c < b->cin; ++c) block_kernel_host[((size_t)o * b->cin + c) * 9 + tap] = w3[((size_t)o * 9 + tap) * b->cin + c];
    return YOLO_OK;
}

// ---- the weight gradient of a trained 3 x 3 block inside a step ---------------------------------------------------------------------------
// yolo_conv3x3_wgrad on the state's scratch, or, after yolo_net_train_set_wgrad_f16, yolo_conv3x3_wgrad_f16 on the net's extra buffer: the
// same arguments, the same outputs, checked in front of the step's first launch and run in its place.
struct BlockWgrad {
    bool f16;
    struct yolo_conv3x3_wgrad_plan pl;
    struct yolo_conv3x3_wgrad_f16_plan pl16;
};

int block_wgrad_check(const yolo_net *net, const yolo_tensor_view &xv, int batch, const Kernel *b, const float *d, const float *scale, float *dw,
                      float *db, void *scratch, size_t scratch_bytes, BlockWgrad *g, std::string &err) {
    const void *x = net->dev_ws + xv.offset;
    g->f16 = net->wgrad_f16_dev != nullptr;
    if (g->f16)
        return wgrad3x3_f16_check(x, xv.dtype, xv.ld, xv.coff, xv.image_stride, xv.h, xv.w, batch, b->cin, d, b->cout, scale, dw, db, net->wgrad_f16_dev,
                                  net->wgrad_f16_bytes, &g->pl16, err);
    return wgrad3x3_check(x, xv.dtype, xv.ld, xv.coff, xv.image_stride, xv.h, xv.w, batch, b->cin, d, b->cout, scale, dw, db, scratch, scratch_bytes,
                          &g->pl, err);
}

int block_wgrad_run(const yolo_net *net, const yolo_tensor_view &xv, int batch, const Kernel *b, const float *d, const float *scale, float *dw,
                    float *db, void *scratch, const BlockWgrad &g, hipStream_t s) {
    const void *x = net->dev_ws + xv.offset;
    if (g.f16)
        return run_wgrad3x3_f16(x, xv.ld, xv.coff, xv.image_stride, xv.h, xv.w, batch, b->cin, d, b->cout, scale, dw, db, net->wgrad_f16_dev, g.pl16, s);
    return run_wgrad3x3(x, xv.dtype, xv.ld, xv.coff, xv.image_stride, xv.h, xv.w, batch, b->cin, d, b->cout, scale, dw, db, scratch, g.pl, s);
}

// ---- the steps: checks, then a list of launches on one stream ------------------------------------------------------------------------------
int train_head_step_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                        void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream, const char *who) {
    HeadTrain t;
    int rc = head_train_layout(net, &t, who);
    if (rc) return rc;
    const yolo_head_train_layout &L = t.L;
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    rc = step_checks(net, in_dev.ptr, batch, state_dev, lr_t, "yolo_net_head_train_init", who,
                     [&] { return loss_check_v2(net, batch, gt_dev, gt_counts_dev, max_gt, st + L.images_offset, result_dev, who); });
    if (rc) return rc;
    yolo_loss_image *images = reinterpret_cast<yolo_loss_image *>(st + L.images_offset);
    const Kernel *k = t.head.k;
    const yolo_tensor_view y = view_of(net, k);
    const int ppi = y.h * y.w;
    std::string err;
    struct yolo_wgrad_plan pl;
    rc = wgrad_plan((long long)ppi * batch, k->cin, k->cout, y.dtype, &pl, err);
    if (rc || pl.scratch_bytes > L.scratch_bytes) return fail(YOLO_ERR_ARG, std::string(who) + ": " + (rc ? err : std::string("weight-gradient scratch too small")));
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    float *grad = reinterpret_cast<float *>(st + L.grad_offset);
    rc = run_forward(net, in_dev, batch, logits, s);        // dense: obj_min_logit is -inf outside detect_any
    if (rc) return rc;
    rc = run_loss_grad(net->head, logits, batch, gt_dev, gt_counts_dev, max_gt, images, reinterpret_cast<int32_t *>(st + L.assign_offset), result_dev, grad, s);
    if (rc) return rc;
    rc = run_wgrad(net->dev_ws + y.offset, y.dtype, y.ld, y.coff, y.image_stride, ppi, batch, k->cin, grad, k->cout,
                   reinterpret_cast<float *>(st + L.dw_offset), reinterpret_cast<float *>(st + L.db_offset), st + L.scratch_offset, pl, s);
    if (rc) return rc;
    HIP_TRY(launch_adam_step(adam_params(net, t.head, st, lr_t), s));
    return YOLO_OK;
}

int train_tail_step_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                        void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream, const char *who) {
    TailTrain t;
    int rc = tail_train_layout(net, &t, who);
    if (rc) return rc;
    const yolo_tail_train_layout &L = t.L;
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    rc = step_checks(net, in_dev.ptr, batch, state_dev, lr_t, "yolo_net_tail_train_init", who,
                     [&] { return loss_check_v2(net, batch, gt_dev, gt_counts_dev, max_gt, st + L.images_offset, result_dev, who); });
    if (rc) return rc;
    yolo_loss_image *images = reinterpret_cast<yolo_loss_image *>(st + L.images_offset);
    const Kernel *k = t.head.k, *b = t.block.k;
    const yolo_tensor_view yv = view_of(net, k), xv = view_of(net, b);
    const int ppi = yv.h * yv.w;
    auto f32 = [&](uint64_t o) { return reinterpret_cast<float *>(st + o); };
    float *grad = f32(L.grad_offset), *d = f32(L.d_offset);
    const void *y = net->dev_ws + yv.offset;
    std::string err;
    struct yolo_wgrad_plan pl;
    BlockWgrad g3;
    long long tiles = 0;
    rc = wgrad_check(y, yv.dtype, yv.ld, yv.coff, yv.image_stride, ppi, batch, k->cin, grad, k->cout, f32(L.dw_offset), f32(L.db_offset),
                     st + L.scratch_offset, (size_t)L.scratch_bytes, &pl, err);
    if (!rc) rc = dgrad_check(grad, k->cout, f32(L.w_offset), k->cin, y, yv.dtype, yv.ld, yv.coff, yv.image_stride, ppi, batch, 0.1f, d, &tiles, err);
    if (!rc) rc = block_wgrad_check(net, xv, batch, b, d, f32(L.scale32_offset), f32(L.dw3_offset), f32(L.dbeta_offset), st + L.scratch_offset,
                                    (size_t)L.scratch_bytes, &g3, err);
    if (rc) return fail(rc, std::string(who) + ": " + err);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    rc = run_forward(net, in_dev, batch, logits, s);        // dense: obj_min_logit is -inf outside detect_any
    if (rc) return rc;
    rc = run_loss_grad(net->head, logits, batch, gt_dev, gt_counts_dev, max_gt, images, reinterpret_cast<int32_t *>(st + L.assign_offset), result_dev, grad, s);
    if (rc) return rc;
    rc = run_wgrad(y, yv.dtype, yv.ld, yv.coff, yv.image_stride, ppi, batch, k->cin, grad, k->cout, f32(L.dw_offset), f32(L.db_offset),
                   st + L.scratch_offset, pl, s);
    if (rc) return rc;
    // the data gradient from the head's master kernel BEFORE its update, through the leaky ReLU's derivative at the stored Y
    rc = run_dgrad(grad, k->cout, f32(L.w_offset), k->cin, y, yv.dtype, yv.ld, yv.coff, yv.image_stride, ppi, batch, 0.1f, d, tiles, s);
    if (rc) return rc;
    rc = block_wgrad_run(net, xv, batch, b, d, f32(L.scale32_offset), f32(L.dw3_offset), f32(L.dbeta_offset), st + L.scratch_offset, g3, s);
    if (rc) return rc;
    HIP_TRY(launch_adam_step(adam_params(net, t.head, st, lr_t), s));
    const TailAdamParams q = {adam_params(net, t.block, st, lr_t), reinterpret_cast<const double *>(st + L.scale64_offset), f32(L.mean_offset)};
    HIP_TRY(launch_tail_adam(q, s));
    return YOLO_OK;
}

int train_head_step_v3_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                           double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream, const char *who) {
    HeadsTrain t;
    int rc = head_train_v3_layout(net, &t, who);
    if (rc) return rc;
    const yolo_head_train_v3_layout &L = t.L;
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    Loss3Geometry lg;
    std::string err;
    rc = step_checks(net, in_dev.ptr, batch, state_dev, lr_t, "yolo_net_head_train_v3_init", who, [&] {
        // (the logits pointer is the workspace's: any non-null value that is not the gradient stands in for it until check_ready has seen the net)
        const int r = loss3_check(&net->head, net, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, st + L.parts_offset, st + L.images_offset,
                                  st + L.assign_offset, result_dev, true, st + L.grad_offset, &lg, err);
        return r ? fail(r, std::string(who) + ": " + err) : YOLO_OK;
    });
    if (rc) return rc;
    yolo_loss_image *parts = reinterpret_cast<yolo_loss_image *>(st + L.parts_offset);
    yolo_loss_image *images = reinterpret_cast<yolo_loss_image *>(st + L.images_offset);
    int32_t *assign = reinterpret_cast<int32_t *>(st + L.assign_offset);
    float *grad = reinterpret_cast<float *>(st + L.grad_offset);
    yolo_v3_wgrad_view views[YOLO_MAX_SCALES];
    float *dw[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr}, *db[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    memset(views, 0, sizeof views);
    for (int i = 0; i < L.n_scales; ++i) {
        const yolo_tensor_view v = view_of(net, t.sc[i].k);
        views[i].x_dev = net->dev_ws + v.offset; views[i].image_stride = v.image_stride; views[i].ld = v.ld; views[i].coff = v.coff;
        views[i].dtype = v.dtype; views[i].cin = v.cin;
        dw[i] = reinterpret_cast<float *>(st + t.sc[i].dw); db[i] = reinterpret_cast<float *>(st + t.sc[i].db);
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
    for (int i = 0; i < L.n_scales; ++i) HIP_TRY(launch_adam_step(adam_params(net, t.sc[i], st, lr_t), s));
    return YOLO_OK;
}

int train_blocks_step_v3_any(yolo_net *net, const NetIn in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                             double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream, const char *who) {
    BlocksTrain t;
    int rc = blocks_train_v3_layout(net, &t, who);
    if (rc) return rc;
    const yolo_blocks_train_v3_layout &L = t.L;
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    Loss3Geometry lg;
    std::string err;
    rc = step_checks(net, in_dev.ptr, batch, state_dev, lr_t, "yolo_net_blocks_train_v3_init", who, [&] {
        // (the logits pointer is the workspace's: any non-null value that is not the gradient stands in for it until check_ready has seen the net)
        const int r = loss3_check(&net->head, net, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, st + L.parts_offset, st + L.images_offset,
                                  st + L.assign_offset, result_dev, true, st + L.grad_offset, &lg, err);
        return r ? fail(r, std::string(who) + ": " + err) : YOLO_OK;
    });
    if (rc) return rc;
    auto f32 = [&](uint64_t o) { return reinterpret_cast<float *>(st + o); };
    yolo_loss_image *parts = reinterpret_cast<yolo_loss_image *>(st + L.parts_offset);
    yolo_loss_image *images = reinterpret_cast<yolo_loss_image *>(st + L.images_offset);
    int32_t *assign = reinterpret_cast<int32_t *>(st + L.assign_offset);
    float *grad = f32(L.grad_offset), *d = f32(L.d_offset);
    yolo_v3_wgrad_view views[YOLO_MAX_SCALES];
    yolo_tensor_view xv[YOLO_MAX_SCALES];
    float *dw[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr}, *db[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    memset(views, 0, sizeof views);
    for (int i = 0; i < L.n_scales; ++i) {
        const yolo_tensor_view v = view_of(net, t.head[i].k);
        xv[i] = view_of(net, t.block[i].k);
        views[i].x_dev = net->dev_ws + v.offset; views[i].image_stride = v.image_stride; views[i].ld = v.ld; views[i].coff = v.coff;
        views[i].dtype = v.dtype; views[i].cin = v.cin;
        dw[i] = f32(t.head[i].dw); db[i] = f32(t.head[i].db);
    }
    struct yolo_v3_wgrad_plan pl;
    Wgrad3Geometry geo;
    struct yolo_v3_dgrad_plan dpl;
    Dgrad3Params dp[YOLO_MAX_SCALES];
    BlockWgrad g3[YOLO_MAX_SCALES];
    rc = wgrad3_check(&net->head, views, batch, grad, assign, max_gt, dw, db, st + L.scratch_offset, (size_t)L.scratch_bytes, &pl, &geo, err);
    for (int i = 0; !rc && i < L.n_scales; ++i) {
        const Kernel *b = t.block[i].k;
        rc = dgrad3_check(&net->head, i, grad, assign, max_gt, batch, f32(t.head[i].w), views[i].cin, views[i].x_dev, views[i].dtype, views[i].ld,
                          views[i].coff, views[i].image_stride, 0.1f, d, &dpl, &dp[i], err);
        if (!rc) rc = block_wgrad_check(net, xv[i], batch, b, d, f32(L.scale32_offset[i]), f32(t.block[i].dw), f32(t.block[i].db), st + L.scratch_offset,
                                        (size_t)L.scratch_bytes, &g3[i], err);
        if (rc) err = "scale " + std::to_string(i) + ": " + err;
    }
    if (rc) return fail(rc, std::string(who) + ": " + err);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *logits = reinterpret_cast<float *>(net->dev_ws + net->logits_off);
    rc = run_forward(net, in_dev, batch, logits, s);        // dense: obj_min_logit is -inf outside detect_any
    if (rc) return rc;
    rc = run_loss3(lg, logits, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, parts, images, assign, result_dev, grad, s);
    if (rc) return rc;
    rc = run_wgrad3(geo, pl, batch, grad, assign, max_gt, st + L.scratch_offset, s);
    if (rc) return rc;
    for (int i = 0; i < L.n_scales; ++i) {
        // the data gradient from the head conv's master kernel BEFORE its update, through the leaky ReLU's derivative at the stored Y_s
        const Kernel *b = t.block[i].k;
        HIP_TRY(launch_head3_dgrad(dp[i], s));
        rc = block_wgrad_run(net, xv[i], batch, b, d, f32(L.scale32_offset[i]), f32(t.block[i].dw), f32(t.block[i].db), st + L.scratch_offset, g3[i], s);
        if (rc) return rc;
    }
    for (int i = 0; i < L.n_scales; ++i) HIP_TRY(launch_adam_step(adam_params(net, t.head[i], st, lr_t), s));
    for (int i = 0; i < L.n_scales; ++i) {
        const TailAdamParams q = {adam_params(net, t.block[i], st, lr_t), reinterpret_cast<const double *>(st + L.scale64_offset[i]), f32(L.mean_offset[i])};
        HIP_TRY(launch_tail_adam(q, s));
    }
    return YOLO_OK;
}

}  // namespace

extern "C" {

// ---- the operators (yolo_hip.h: added within ABI 7; kernels in train.hip, train_tail.hip, train3.hip; splits and checks in *_host.cpp) -----
int yolo_wgrad_plan(int64_t P, int cin, int cout, int x_dtype, struct yolo_wgrad_plan *out) {
    std::string err;
    const int rc = wgrad_plan(P, cin, cout, x_dtype, out, err);
    return rc ? fail(rc, "yolo_wgrad_plan: " + err) : YOLO_OK;
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
    AdamParams p;       // the caller's arrays and constants, nothing to re-pack
    memset(&p, 0, sizeof p);
    p.w = w; p.b = b; p.m_w = m_w; p.v_w = v_w; p.m_b = m_b; p.v_b = v_b; p.dw = dw; p.db = db; p.n_w = n_w; p.n_b = n_b;
    p.lr_t = lr_t; p.beta1 = beta1; p.beta2 = beta2; p.eps = eps;
    HIP_TRY(launch_adam_step(p, static_cast<hipStream_t>(stream)));
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

int yolo_conv3x3_wgrad_f16_plan(int h, int w, int batch, int cin, int cout, struct yolo_conv3x3_wgrad_f16_plan *out) {
    std::string err;
    const int rc = wgrad3x3_f16_plan(h, w, batch, cin, cout, out, err);
    return rc ? fail(rc, "yolo_conv3x3_wgrad_f16_plan: " + err) : YOLO_OK;
}

int yolo_conv3x3_wgrad_f16(const void *x_dev, int x_dtype, int ld, int coff, int64_t image_stride, int h, int w, int batch, int cin,
                           const float *d_dev, int cout, const float *scale_dev, float *dw_dev, float *db_dev, void *scratch_dev,
                           size_t scratch_bytes, void *stream) {
    std::string err;
    struct yolo_conv3x3_wgrad_f16_plan pl;
    const int rc = wgrad3x3_f16_check(x_dev, x_dtype, ld, coff, image_stride, h, w, batch, cin, d_dev, cout, scale_dev, dw_dev, db_dev, scratch_dev,
                                      scratch_bytes, &pl, err);
    if (rc) return fail(rc, "yolo_conv3x3_wgrad_f16: " + err);
    return run_wgrad3x3_f16(x_dev, ld, coff, image_stride, h, w, batch, cin, d_dev, cout, scale_dev, dw_dev, db_dev, scratch_dev, pl,
                            static_cast<hipStream_t>(stream));
}

int yolo_v3_head_wgrad_plan(const yolo_head_desc *head, const int32_t *cin, int batch, int x_dtype, struct yolo_v3_wgrad_plan *out) {
    std::string err;
    Wgrad3Geometry geo;
    const int rc = wgrad3_plan(head, cin, batch, x_dtype, out, &geo, err);
    return rc ? fail(rc, "yolo_v3_head_wgrad_plan: " + err) : YOLO_OK;
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

int yolo_v3_head_dgrad_plan(const yolo_head_desc *head, int scale, int cin, int batch, struct yolo_v3_dgrad_plan *out) {
    std::string err;
    const int rc = dgrad3_plan(head, scale, cin, batch, out, nullptr, err);
    return rc ? fail(rc, "yolo_v3_head_dgrad_plan: " + err) : YOLO_OK;
}

int yolo_v3_head_dgrad(const yolo_head_desc *head, int scale, const float *g_dev, const int32_t *assign_dev, int max_gt, int batch,
                       const float *w_dev, int cin, const void *y_dev, int y_dtype, int ld, int coff, int64_t image_stride, float slope,
                       float *d_dev, void *stream) {
    std::string err;
    struct yolo_v3_dgrad_plan pl;
    Dgrad3Params p;
    const int rc = dgrad3_check(head, scale, g_dev, assign_dev, max_gt, batch, w_dev, cin, y_dev, y_dtype, ld, coff, image_stride, slope, d_dev,
                                &pl, &p, err);
    if (rc) return fail(rc, "yolo_v3_head_dgrad: " + err);
    HIP_TRY(launch_head3_dgrad(p, static_cast<hipStream_t>(stream)));
    return YOLO_OK;
}

// ---- training the detection layer of a YOLOv2 net (yolo_hip.h: added within ABI 7) ---------------------------------------------------------
int yolo_net_head_input(const yolo_net *net, yolo_tensor_view *out) {
    const Kernel *k = nullptr;
    int rc = head_conv(net, &k, "yolo_net_head_input");
    if (rc) return rc;
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_head_input: null argument");
    *out = view_of(net, k);
    return YOLO_OK;
}

int yolo_net_head_train_layout(const yolo_net *net, yolo_head_train_layout *out) {
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_head_train_layout: null argument");
    HeadTrain t;
    const int rc = head_train_layout(net, &t, "yolo_net_head_train_layout");
    if (!rc) *out = t.L;
    return rc;
}

size_t yolo_net_head_train_bytes(const yolo_net *net) {
    HeadTrain t;
    return head_train_layout(net, &t, "yolo_net_head_train_bytes") ? 0 : (size_t)t.L.total_bytes;
}

int yolo_net_head_train_init(yolo_net *net, void *state_dev, size_t bytes, const float *head_w_host, const float *head_b_host) {
    const char *who = "yolo_net_head_train_init";
    if (!net || !state_dev || !head_w_host || !head_b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    HeadTrain t;
    int rc = head_train_layout(net, &t, who);
    if (!rc) rc = init_checks(net, state_dev, bytes, t.L.total_bytes, "yolo_net_head_train_bytes", who);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    rc = start_state(t.head, static_cast<unsigned char *>(state_dev), head_w_host, head_b_host);
    if (!rc) rc = pack_conv1x1(net, t.head.k, head_w_host, head_b_host);
    return rc;
}

int yolo_net_head_train_read(yolo_net *net, const void *state_dev, float *w_host, float *b_host) {
    const char *who = "yolo_net_head_train_read";
    if (!net || !state_dev || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    HeadTrain t;
    const int rc = head_train_layout(net, &t, who);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return read_state(t.head, static_cast<const unsigned char *>(state_dev), w_host, b_host);
}

int yolo_net_train_head_step(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                             void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_head_step_any(net, NetIn{in_dev, false}, batch, gt_dev, gt_counts_dev, max_gt, state_dev, lr_t, result_dev, stream, "yolo_net_train_head_step");
}
int yolo_net_train_head_step_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_head_step_any(net, NetIn{in_dev, true}, batch, gt_dev, gt_counts_dev, max_gt, state_dev, lr_t, result_dev, stream, "yolo_net_train_head_step_u8");
}

// ---- training the tail of a YOLOv2 net (yolo_hip.h: added within ABI 7) --------------------------------------------------------------------
int yolo_net_tail_inputs(const yolo_net *net, yolo_tensor_view *block_in, yolo_tensor_view *head_in) {
    const Kernel *b = nullptr, *k = nullptr;
    int rc = tail_convs(net, &b, &k, "yolo_net_tail_inputs");
    if (rc) return rc;
    if (!block_in || !head_in) return fail(YOLO_ERR_ARG, "yolo_net_tail_inputs: null argument");
    *block_in = view_of(net, b);
    *head_in = view_of(net, k);
    return YOLO_OK;
}

int yolo_net_tail_train_layout(const yolo_net *net, yolo_tail_train_layout *out) {
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_tail_train_layout: null argument");
    TailTrain t;
    const int rc = tail_train_layout(net, &t, "yolo_net_tail_train_layout");
    if (!rc) *out = t.L;
    return rc;
}

size_t yolo_net_tail_train_bytes(const yolo_net *net) {
    TailTrain t;
    return tail_train_layout(net, &t, "yolo_net_tail_train_bytes") ? 0 : (size_t)t.L.total_bytes;
}

int yolo_net_tail_train_init(yolo_net *net, void *state_dev, size_t bytes, const float *block_host, const float *head_w_host,
                             const float *head_b_host) {
    const char *who = "yolo_net_tail_train_init";
    if (!net || !state_dev || !block_host || !head_w_host || !head_b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    TailTrain t;
    int rc = tail_train_layout(net, &t, who);
    if (!rc) rc = init_checks(net, state_dev, bytes, t.L.total_bytes, "yolo_net_tail_train_bytes", who);
    if (!rc) rc = block_rows_fit(t.block.k, who);
    if (rc) return rc;
    const yolo_tail_train_layout &L = t.L;
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    HIP_TRY(hipDeviceSynchronize());
    rc = start_state(t.head, st, head_w_host, head_b_host);
    if (!rc) rc = init_block(net, t.block, st, block_host, L.scale64_offset, L.scale32_offset, L.mean_offset, who);
    if (rc) return rc;
    return pack_conv1x1(net, t.head.k, head_w_host, head_b_host);
}

int yolo_net_tail_train_read(yolo_net *net, const void *state_dev, float *block_kernel_host, float *beta_host, float *w_host, float *b_host) {
    const char *who = "yolo_net_tail_train_read";
    if (!net || !state_dev || !block_kernel_host || !beta_host || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    TailTrain t;
    int rc = tail_train_layout(net, &t, who);
    if (rc) return rc;
    const unsigned char *st = static_cast<const unsigned char *>(state_dev);
    HIP_TRY(hipDeviceSynchronize());
    rc = read_block(t.block, st, block_kernel_host, beta_host);
    if (!rc) rc = read_state(t.head, st, w_host, b_host);
    return rc;
}

int yolo_net_train_tail_step(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                             void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_tail_step_any(net, NetIn{in_dev, false}, batch, gt_dev, gt_counts_dev, max_gt, state_dev, lr_t, result_dev, stream, "yolo_net_train_tail_step");
}
int yolo_net_train_tail_step_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_tail_step_any(net, NetIn{in_dev, true}, batch, gt_dev, gt_counts_dev, max_gt, state_dev, lr_t, result_dev, stream, "yolo_net_train_tail_step_u8");
}

// ---- training the YOLOv3 head convs on a net (yolo_hip.h: added within ABI 7) --------------------------------------------------------------
int yolo_net_head_inputs_v3(const yolo_net *net, yolo_tensor_view *out, int32_t *n) {
    const Kernel *ks[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    int rc = head_convs_v3(net, ks, "yolo_net_head_inputs_v3");
    if (rc) return rc;
    if (!out || !n) return fail(YOLO_ERR_ARG, "yolo_net_head_inputs_v3: null argument");
    *n = net->head.n_scales;
    for (int s = 0; s < net->head.n_scales; ++s) out[s] = view_of(net, ks[s]);
    return YOLO_OK;
}

int yolo_net_head_train_v3_layout(const yolo_net *net, yolo_head_train_v3_layout *out) {
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_head_train_v3_layout: null argument");
    HeadsTrain t;
    const int rc = head_train_v3_layout(net, &t, "yolo_net_head_train_v3_layout");
    if (!rc) *out = t.L;
    return rc;
}

size_t yolo_net_head_train_v3_bytes(const yolo_net *net) {
    HeadsTrain t;
    return head_train_v3_layout(net, &t, "yolo_net_head_train_v3_bytes") ? 0 : (size_t)t.L.total_bytes;
}

int yolo_net_head_train_v3_init(yolo_net *net, void *state_dev, size_t bytes, const float *const *w_host, const float *const *b_host) {
    const char *who = "yolo_net_head_train_v3_init";
    if (!net || !state_dev || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    HeadsTrain t;
    int rc = head_train_v3_layout(net, &t, who);
    if (rc) return rc;
    for (int s = 0; s < t.L.n_scales; ++s)
        if (!w_host[s] || !b_host[s]) return fail(YOLO_ERR_ARG, std::string(who) + ": scale " + std::to_string(s) + ": null argument");
    rc = init_checks(net, state_dev, bytes, t.L.total_bytes, "yolo_net_head_train_v3_bytes", who);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    for (int s = 0; s < t.L.n_scales && !rc; ++s) {
        rc = start_state(t.sc[s], static_cast<unsigned char *>(state_dev), w_host[s], b_host[s]);
        if (!rc) rc = pack_conv1x1(net, t.sc[s].k, w_host[s], b_host[s]);
    }
    return rc;
}

int yolo_net_head_train_v3_read(yolo_net *net, const void *state_dev, float *const *w_host, float *const *b_host) {
    const char *who = "yolo_net_head_train_v3_read";
    if (!net || !state_dev || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    HeadsTrain t;
    int rc = head_train_v3_layout(net, &t, who);
    if (rc) return rc;
    for (int s = 0; s < t.L.n_scales; ++s)
        if (!w_host[s] || !b_host[s]) return fail(YOLO_ERR_ARG, std::string(who) + ": scale " + std::to_string(s) + ": null argument");
    HIP_TRY(hipDeviceSynchronize());
    for (int s = 0; s < t.L.n_scales && !rc; ++s) rc = read_state(t.sc[s], static_cast<const unsigned char *>(state_dev), w_host[s], b_host[s]);
    return rc;
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

// ---- training the 3 x 3 blocks behind the YOLOv3 heads (yolo_hip.h: added within ABI 7) ------------------------------------------------------
int yolo_net_block_inputs_v3(const yolo_net *net, yolo_tensor_view *block_in, yolo_tensor_view *head_in, int32_t *n) {
    const Kernel *bs[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr}, *ks[YOLO_MAX_SCALES] = {nullptr, nullptr, nullptr, nullptr};
    int rc = block_convs_v3(net, bs, ks, "yolo_net_block_inputs_v3");
    if (rc) return rc;
    if (!block_in || !head_in || !n) return fail(YOLO_ERR_ARG, "yolo_net_block_inputs_v3: null argument");
    *n = net->head.n_scales;
    for (int s = 0; s < net->head.n_scales; ++s) {
        block_in[s] = view_of(net, bs[s]);
        head_in[s] = view_of(net, ks[s]);
    }
    return YOLO_OK;
}

int yolo_net_blocks_train_v3_layout(const yolo_net *net, yolo_blocks_train_v3_layout *out) {
    if (!out) return fail(YOLO_ERR_ARG, "yolo_net_blocks_train_v3_layout: null argument");
    BlocksTrain t;
    const int rc = blocks_train_v3_layout(net, &t, "yolo_net_blocks_train_v3_layout");
    if (!rc) *out = t.L;
    return rc;
}

size_t yolo_net_blocks_train_v3_bytes(const yolo_net *net) {
    BlocksTrain t;
    return blocks_train_v3_layout(net, &t, "yolo_net_blocks_train_v3_bytes") ? 0 : (size_t)t.L.total_bytes;
}

int yolo_net_blocks_train_v3_init(yolo_net *net, void *state_dev, size_t bytes, const float *const *block_host, const float *const *w_host,
                                  const float *const *b_host) {
    const char *who = "yolo_net_blocks_train_v3_init";
    if (!net || !state_dev || !block_host || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    BlocksTrain t;
    int rc = blocks_train_v3_layout(net, &t, who);
    if (rc) return rc;
    const yolo_blocks_train_v3_layout &L = t.L;
    for (int s = 0; s < L.n_scales; ++s)
        if (!block_host[s] || !w_host[s] || !b_host[s]) return fail(YOLO_ERR_ARG, std::string(who) + ": scale " + std::to_string(s) + ": null argument");
    rc = init_checks(net, state_dev, bytes, L.total_bytes, "yolo_net_blocks_train_v3_bytes", who);
    for (int s = 0; s < L.n_scales && !rc; ++s) rc = block_rows_fit(t.block[s].k, who);
    if (rc) return rc;
    unsigned char *st = static_cast<unsigned char *>(state_dev);
    HIP_TRY(hipDeviceSynchronize());
    for (int s = 0; s < L.n_scales && !rc; ++s) {
        rc = start_state(t.head[s], st, w_host[s], b_host[s]);
        if (!rc) rc = pack_conv1x1(net, t.head[s].k, w_host[s], b_host[s]);
        if (!rc) rc = init_block(net, t.block[s], st, block_host[s], L.scale64_offset[s], L.scale32_offset[s], L.mean_offset[s], who);
    }
    return rc;
}

int yolo_net_blocks_train_v3_read(yolo_net *net, const void *state_dev, float *const *block_kernel_host, float *const *beta_host,
                                  float *const *w_host, float *const *b_host) {
    const char *who = "yolo_net_blocks_train_v3_read";
    if (!net || !state_dev || !block_kernel_host || !beta_host || !w_host || !b_host) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    BlocksTrain t;
    int rc = blocks_train_v3_layout(net, &t, who);
    if (rc) return rc;
    for (int s = 0; s < t.L.n_scales; ++s)
        if (!block_kernel_host[s] || !beta_host[s] || !w_host[s] || !b_host[s])
            return fail(YOLO_ERR_ARG, std::string(who) + ": scale " + std::to_string(s) + ": null argument");
    const unsigned char *st = static_cast<const unsigned char *>(state_dev);
    HIP_TRY(hipDeviceSynchronize());
    for (int s = 0; s < t.L.n_scales && !rc; ++s) {
        rc = read_block(t.block[s], st, block_kernel_host[s], beta_host[s]);
        if (!rc) rc = read_state(t.head[s], st, w_host[s], b_host[s]);
    }
    return rc;
}

int yolo_net_train_blocks_step_v3(yolo_net *net, const float *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev, int max_gt,
                                  double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_blocks_step_v3_any(net, NetIn{in_dev, false}, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, state_dev, lr_t, result_dev, stream,
                                    "yolo_net_train_blocks_step_v3");
}
int yolo_net_train_blocks_step_v3_u8(yolo_net *net, const uint8_t *in_dev, int batch, const yolo_gt *gt_dev, const int32_t *gt_counts_dev,
                                     int max_gt, double ignore_thresh, void *state_dev, float lr_t, yolo_loss_result *result_dev, void *stream) {
    return train_blocks_step_v3_any(net, NetIn{in_dev, true}, batch, gt_dev, gt_counts_dev, max_gt, ignore_thresh, state_dev, lr_t, result_dev, stream,
                                    "yolo_net_train_blocks_step_v3_u8");
}

// ---- the fp16-operand weight gradient as a mode of the tail and blocks steps (yolo_hip.h: added within ABI 7) --------------------------------
size_t yolo_net_train_wgrad_f16_bytes(const yolo_net *net) {
    uint64_t need = 0;
    return wgrad_f16_need(net, &need, "yolo_net_train_wgrad_f16_bytes") ? 0 : (size_t)need;
}

int yolo_net_train_set_wgrad_f16(yolo_net *net, void *extra_dev, size_t bytes) {
    const char *who = "yolo_net_train_set_wgrad_f16";
    if (!net) return fail(YOLO_ERR_ARG, std::string(who) + ": null argument");
    if (!extra_dev) {       // back to the float32 steps
        net->wgrad_f16_dev = nullptr;
        net->wgrad_f16_bytes = 0;
        return YOLO_OK;
    }
    uint64_t need = 0;
    const int rc = wgrad_f16_need(net, &need, who);
    if (rc) return rc;
    if (bytes < need) return fail(YOLO_ERR_ARG, std::string(who) + ": buffer too small (yolo_net_train_wgrad_f16_bytes)");
    if ((uintptr_t)extra_dev % 256) return fail(YOLO_ERR_ARG, std::string(who) + ": the buffer must be 256-byte aligned");
    net->wgrad_f16_dev = static_cast<unsigned char *>(extra_dev);
    net->wgrad_f16_bytes = bytes;
    return YOLO_OK;
}

}  // extern "C"

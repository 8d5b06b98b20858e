// Internal interfaces of libyolo_hip.so (not part of the C ABI; see include/yolo_hip.h).
//
// Data layout in HBM (DESIGN.md "Layout"):
//   activations  NHWC, element type T (fp16 or fp32), addressed as strided views
//                (pixel stride `ld`, first channel `coff`, image stride) so that
//                route/concat, upsample and reorg never copy: producers write slices.
//   weights      [Cout_pad][K] with K = (kh, kw, cin) in 16-byte chunks, BN folded,
//                rows zero-padded to a multiple of 128, K zero-padded to 8 chunks.
//   head logits  float32 in the reference's layout (net/v2.py:52-59, net/layers.py:119-133).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include <string>
#include <vector>

#include "yolo_hip.h"
#include "train_host.h"
#include "train3_host.h"
#include "train_tail_host.h"
#include "train3_tail_host.h"
#include "augment_host.h"
#include "anchor_host.h"
#include "loss3_host.h"

namespace yolo {

enum OutMode { OUT_NORMAL = 0, OUT_UP2 = 1, OUT_REORG2 = 2, OUT_POOL2 = 3 };   // OUT_POOL2: the 2x2/2 max-pool behind the conv is taken in its epilogue (2-D tap tiles)
enum BufId { BUF_NONE = -1, BUF_USER_OUT = -2, BUF_USER_IN = -3 };
enum ConvCfg { CFG_N128 = 0, CFG_N64 = 1, CFG_N32 = 2 };   // cout-tile width of the block
enum KernelKind { K_PREP = 0, K_CONV = 1, K_POOL = 2, K_ELTWISE = 3, K_FIRST = 4 };

// A strided NHWC view inside a planned buffer.
struct View {
    int buf = BUF_NONE;
    int H = 0, W = 0, C = 0;
    int ld = 0;                 // elements between consecutive pixels
    int coff = 0;               // first channel inside the pixel
    long long img_stride = 0;   // elements between consecutive images
    long long base = 0;         // extra element offset (head scale offset inside the output)
    bool f32 = false;           // float32 elements whatever the net dtype (head logits)
};
// every stride of the view, and its first element, is a multiple of `epc` elements (epc = elements per 16-byte chunk: 16-byte accesses
// are possible in a buffer that is itself aligned).  What else a caller asks of the view -- C % epc, !f32 -- stands at the call.
inline bool view_chunk_aligned(const View &v, int epc) { return v.ld % epc == 0 && (v.base + v.coff) % epc == 0 && v.img_stride % epc == 0; }

struct Buffer {
    long long elems_per_image = 0;  // elements per image
    int esize = 2;
    int first = 1 << 30, last = -1; // kernel indices of first write / last access
    size_t offset = 0;              // bytes inside the workspace
    size_t bytes = 0;               // for max_batch
    size_t used = 0;                // payload bytes of the region (the rest is alignment slack + yolo_net_options.guard_bytes)
    bool is_concat = false;
};

// ---- device-side parameter blocks -----------------------------------------------------
// Division by a launch-time constant without the ~40-instruction software divide (Granlund-Montgomery,
// exact for every 32-bit unsigned n): q = (t + ((n - t) >> sh1)) >> sh2 with t = mulhi(mul, n).
struct FastDiv {
    uint32_t mul, sh1, sh2, d;
};
inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f{1, 0, 0, d ? d : 1};
    uint32_t l = 0;
    while ((1ull << l) < f.d) ++l;
    f.mul = (uint32_t)((((1ull << l) - f.d) << 32) / f.d + 1);
    f.sh1 = l < 1 ? l : 1;
    f.sh2 = l > 0 ? l - 1 : 0;
    return f;
}
__host__ __device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv &f) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = __umulhi(f.mul, n);
#else
    const uint32_t t = (uint32_t)(((unsigned long long)f.mul * n) >> 32);
#endif
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

// leaky ReLU 0.1 (net/layers.py:6,50-51: tf.nn.leaky_relu = max(alpha x, x)) as TWO instructions: fmaxf() on an MFMA result
// makes hipcc put a canonicalising `v_max x, x` in front of the real one (three instructions per value).  Used where the kernel is VALU-bound (stem.hip:
// -5 %); the conv epilogues keep fmaxf(), whose instructions the compiler schedules freely (the opaque asm cost them +1 %,
// the staged float32 head epilogue +19 %: profiles/r03_ablation.md).  Same value for every non-NaN input.
__host__ __device__ __forceinline__ float leaky01(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r;
    const float y = 0.1f * x;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(y), "v"(x));
    return r;
#else
    return x > 0.1f * x ? x : 0.1f * x;
#endif
}

// uint8 network input (yolo_net_forward_u8 and friends): a pixel byte u enters the first conv as float32(u / 255.), the value the
// float32 entry points are handed (net/base.py:153 divides in float64, the placeholder casts to float32: net/layers.py:108).  That is
// the correctly rounded IEEE float32 quotient u / 255 -- NOT u * float32(1 / 255), which differs for 126 of the 256 bytes.  Computed
// as a quotient estimate plus one correction on its exact remainder: r = u - 255 q is exact in an FMA (q is within one ulp), and
// q + r / 255 rounds to the quotient (checked against float64 division for all 256 bytes: tests/test_u8_cpu.py, through
// yolo_u8_unit_table).  Three dependent VALU instructions, no division sequence, nothing a fast-math flag can rewrite.
__host__ __device__ __forceinline__ float u8_unit(unsigned u) {
#pragma clang fp contract(off)
    const float a = (float)u;
    const float rcp = 0x1.010102p-8f;       // float32(1 / 255.)
    const float q = a * rcp;
    return __builtin_fmaf(__builtin_fmaf(-255.f, q, a), rcp, q);
}

// The per-image candidate counters of the decode live one per 128-byte line: with the 32 counters of a batch in ONE line every
// candidate's atomicAdd of the whole batch went through one L2 channel (YOLOv3-608 b32: 2 900 atomics, decode_kernel 31 us, 5 us with
// no candidate at all).
constexpr int kCandCountStride = 32;

// Launch caps: the kernels below loop over more work than their grid holds (persistent workgroups walk tiles blockIdx, blockIdx + grid, ...;
// grid-stride loops).  Past these counts a workgroup gets a second tile / a thread a second item -- the hand-over code of those kernels
// runs only then, so the tests size their cases from these numbers (yolo_launch_caps; tests/test_rounds_cpu.py).
constexpr int kTapStreamCUs = 256, kTapStreamPerCu = 2;        // conv3x3_tap_stream_kernel: ConvTile.per_cu() resident workgroups on each CU
constexpr int kTapStreamGrid = kTapStreamCUs * kTapStreamPerCu;
constexpr int kStemGrid = 512;                                 // stem_v3_kernel: two workgroups per CU; split over the parts of a batch on streams
constexpr int kFirstMfmaGrid = 1024;                           // first_pool_mfma*_kernel: four workgroups per CU
constexpr int kAuxBlock = 256, kAuxGrid = 256 * 16;            // aux.hip grid_for: 16 blocks per CU, grid-stride the rest
constexpr int kDecodeBlock = 256, kDecodeGrid = 256 * 8;       // decode_kernel: one row per thread and round

struct ConvParams {
    const void *in;            // base of the input BUFFER (view offsets are folded into byte offsets)
    const void *wgt;
    const float *bias;
    const void *res;           // residual tensor base (element pointer incl. coff) or null
    void *out;                 // output base pointer incl. view base / coff
    uint32_t in_bytes, wgt_bytes;
    uint32_t out_bytes, res_bytes;     // extent of the output / residual tensors from `out` / `res` (0: beyond 2 GiB -> no buffer addressing)
    int H, W, in_ld, in_coff;
    long long in_img_stride;
    int Ho, Wo, HoWo, M;
    int Cout, out_ld;
    long long out_img_stride;
    int res_ld;
    long long res_img_stride;
    int ksize, stride, pad, taps;
    int ktiles, tiles_per_tap, cpt_shift;
    int cin_chunks;            // 16-byte chunks per tap (storage channels / EPC)
    uint32_t wrow_bytes;
    int leaky, has_res, outmode, out_f32, vec_out, vec_res;
    int f32;                   // elements of input / weights / residual are float32 (else fp16)
    int n_tiles_n, n_blocks;
    // split-K (small feature maps at small batch: a handful of tiles, each with a K of thousands): blockIdx.y = split s runs
    // K units [s * kunits, (s + 1) * kunits) (conv_tap.hip: channel slices; conv.hip: K tiles) and stores its raw float32
    // accumulators to part[s][pixel][cout_pad]; splitk_reduce_kernel (aux.hip) sums them and runs the fused epilogue
    int ksplit, kunits, cout_pad;
    float *part;
    // split-K IN the launch (conv_tap.hip, 128 x 128 tile, ksplit == 2): both halves of a tile write their accumulators to
    // part[tile][half] (write-through), take a ticket from pair_cnt[tile], and the second arriver adds the other half and runs
    // the fused epilogue -- no reduce launch.  For launches of 129-256 tiles (13 x 13 / 19 x 19 maps at batch 8-32).
    int pair;
    int *pair_cnt;
    uint32_t part_bytes;
    int stream;                // conv_tap.hip: run the persistent (stream) form where it applies
    int fast_epi;              // conv_common.h: conv_epilogue_fast applies (set by the launchers: conv_fast_epilogue_ok)
    // back-to-back 1x1 (conv_common.h: conv_epilogue_fused_1x1): the 1x1 conv behind this one, computed by the same workgroups
    int fuse2;                 // 1: w2 .. are set and the launch runs the fused instantiation
    const void *w2;            // packed weights of the 1x1 ([128 rows][wrow2_bytes], natural filter order), 64 filters x 128 channels
    const float *b2;           // its folded bias
    void *out2;                // its output view (fp16, 16-byte aligned strides)
    uint32_t w2_bytes, wrow2_bytes, out2_bytes;
    int out2_ld, leaky2;
    long long out2_img_stride;
    int dbg;                   // experiment flags (YOLO_CONV_DBG): 1 skip steady-state DMA, 2 skip MFMA phase
    int f32_emu;               // conv.hip, float32 nets: this launch multiplies as nine bf16 products (conv_f32_emu_rule)
    int qW, qHW, Mq;           // conv_tap.hip: padded-linear pixel grid, row stride W+1, image stride (H+1)(W+1), total
    int q_stride;              // conv_tap.hip MODE 1: first position of tile m = m * q_stride (positions per tile; qHW for the image-aligned tile)
    int t2_shift;              // conv_tap.hip MODE 2: log2 of the positions per 2-D tile (8: 16 x 16, 7: 8 x 16)
    float *obj_out;            // head convs (staged float32 epilogue): compact objectness logits [B][obj_rows] or null
    int obj_width, obj_rows, obj_row0, obj_na;     // 5 + classes; rows per image; first row of this scale; anchors per cell
    float obj_min;             // head convs inside yolo_net_detect: rows whose objectness logit is below this are not written (conv_common.h); -inf: all rows
    unsigned long long *trace; // conv_tap.hip: per-block phase timestamps (YOLO_CONV_TRACE experiment) or null
    FastDiv dHoWo, dWo, dqHW, dqW, dtiles_n, dtpt;   // set by the launchers (conv_set_divisors); dtpt: K stages per tap
};
// fp16 output through the normal index map, 16-byte aligned views below 2 GiB, whole 16-cout groups, no split-K: the lean epilogue
inline bool conv_fast_epilogue_ok(const ConvParams &p) {
    return !p.f32 && !p.out_f32 && p.outmode == OUT_NORMAL && p.vec_out && p.out_bytes && p.Cout % 16 == 0 && p.ksplit <= 1 &&
           (!p.has_res || (p.vec_res && p.res_bytes));
}
inline void conv_set_divisors(ConvParams &p, int stages_per_tap) {
    p.dtpt = make_fastdiv((uint32_t)(stages_per_tap > 0 ? stages_per_tap : 1));
    p.dHoWo = make_fastdiv((uint32_t)p.HoWo);
    p.dWo = make_fastdiv((uint32_t)p.Wo);
    p.dqHW = make_fastdiv((uint32_t)(p.qHW > 0 ? p.qHW : 1));
    p.dqW = make_fastdiv((uint32_t)(p.qW > 0 ? p.qW : 1));
    p.dtiles_n = make_fastdiv((uint32_t)(p.n_tiles_n > 0 ? p.n_tiles_n : 1));
}

struct PrepParams {            // float32 (or uint8: launch_prep's in_u8, prep_u8_kernel) NHWC [B,H,W,C] -> T NHWC [B,H,W,Cpad], zero fill
    const void *in;
    void *out;
    long long pixels;
    int C, Cpad;
};

struct FirstParams {           // first layer: 3x3/1 conv on the float32 NHWC3 input, Cout 16|32
    const void *in;            // [B,H,W,3] float32 (the caller's tensor), or uint8 for the *_u8_kernel twins (launch_first: in_u8)
    const float *wgt;          // [27][Cout] float32, BN folded (rounded through fp16 for fp16 nets)
    const float *bias;         // [Cout]
    void *out;                 // T NHWC view
    int H, W, Cout, out_ld, leaky, round_half;
    long long out_img_stride;
    long long total;           // B*H*W output pixels (< 2^31)
    FastDiv dW, dH, dHW;       // set by launch_first
    int pool;                  // 1: the 2x2/2 max-pool behind the conv is fused; `out` is the POOLED tensor [B,H/2,W/2,Cout]
    int xblocks;               // pool: 128-wide x blocks per row (set by launch_first); MFMA form: tiles per tile row
    FastDiv dXB, dHp;
    int tiles_y, n_tiles;      // MFMA form (first_pool_mfma_kernel): 8 x 16 pooled-output tiles per image column / in all
};

struct StemParams {            // stem.hip: fused conv 3x3/1 3->32 + conv 3x3/2 32->64 (both BN + leaky), fp16 nets
    const void *in;            // [B,H,W,3] float32 (the caller's tensor), or uint8 for stem_v3_u8_kernel (launch_stem: in_u8)
    const float *w1;           // first layer [27][32] float32 (K_FIRST packing)
    const float *b1;           // [32]
    const void *w2;            // second layer, K_CONV packing: [Cout_pad][wrow2 bytes] fp16, K = (kh, kw, 32 cin)
    const float *b2;           // [Cout_pad]
    void *out;                 // fp16 NHWC view [B,H/2,W/2,64]
    const void *w3;            // optional third layer (1x1 64->32, BN + leaky) on the same pixels: [Cout_pad][128 B] fp16, or null
    const float *b3;
    void *out3;                // fp16 NHWC view [B,H/2,W/2,32]
    int out3_ld;
    long long out3_img_stride;
    uint32_t w2_bytes, wrow2;
    int H, W, Ho, Wo, out_ld;
    long long in_img_stride, out_img_stride;     // in ELEMENTS of the input type (floats, or bytes for a uint8 input)
    int tiles_x, tiles_y, n_tiles;   // set by launch_stem
    FastDiv dtx, dty;
};

struct ResizeParams {          // uint8 HWC3 image -> float32 [dst_h][dst_w][3] in [0,1] (aux.hip: resize_u8_kernel), or the 8-bit value itself
    const unsigned char *src;
    void *dst;                 // float32, or uint8 for resize_u8_to_u8_kernel (launch_resize: dst_u8)
    int src_h, src_w, src_row_bytes, dst_h, dst_w, swap_rb;
};

// aux.hip: frames_resize_kernel -- up to kFramesPerLaunch frames of any size into one dense batch tensor, one launch.  The descriptors
// travel by value in the kernel argument (64 x 40 bytes: no device table, no copy); workgroups of grid row y read entry y through scalar loads.
constexpr int kFramesPerLaunch = 64;
struct FrameGeom {             // one frame and where it lands in the network input (yolo_letterbox_geometry)
    const unsigned char *src;
    int src_h, src_w, src_row_bytes, swap_rb;
    int new_h, new_w, off_y, off_x;
};
struct FramesParams {
    FrameGeom f[kFramesPerLaunch];
    void *dst;                 // image 0 of this launch: uint8 or float32 [n][dst_h][dst_w][3]
    int dst_h, dst_w;          // dst_w % 4 == 0
    int wide;                  // dst is aligned for the wide stores (4 bytes for uint8, 16 for float32); else element stores
};
struct BoxGeom { int new_h, new_w, off_y, off_x; };
struct RemapParams {           // aux.hip: boxes_to_frames_kernel -- box records from network to frame coordinates, in place
    BoxGeom g[kFramesPerLaunch];
    yolo_box *boxes;           // image 0 of this launch
    const int *counts;
    int max_boxes, net_h, net_w;
};

struct PoolParams {            // net/layers.py:70-81
    const void *in;
    void *out;
    int H, W, C, in_ld, Ho, Wo, out_ld, stride;
    long long in_img_stride, out_img_stride;
    long long total;           // B*Ho*Wo*(C/EPC) work items
    int ksize = 2;             // pool_same_kernel: odd window size (stride 1, SAME); pool_kernel is the 2x2 window whatever this says
};
// pool_kernel / pool_same_kernel: the strides allow the 16-byte-vector instantiation.  The launchers (aux.hip) add the alignment of their
// two pointers; the report (forward.cpp: pool_info) that of the views' first elements, which is the same thing in a planned buffer.
inline bool pool_vec_strides(int C, int in_ld, int out_ld, long long in_img_stride, long long out_img_stride, int epc) {
    return C % epc == 0 && in_ld % epc == 0 && out_ld % epc == 0 && in_img_stride % epc == 0 && out_img_stride % epc == 0;
}

struct SppParams {             // aux.hip: spp_pool_kernel -- the three stride-1 SAME pools of an SPP block (windows 2r+1, 4r+1, 6r+1) of one fp16 tensor
    const void *in;            // element pointers incl. view base / coff; every stride a multiple of the 16-byte chunk
    void *out[3];              // smallest window first
    int H, W, chunks;          // chunks = C / 8
    int in_ld, out_ld[3];
    long long in_img_stride, out_img_stride[3];
    int slab, slab_shift;      // 16-byte channel chunks a workgroup owns (power of two) and its log2 (set by launch_spp)
    int slabs;                 // workgroups per image
    FastDiv dW;
};

struct EltParams {             // generic fallback: out[map(p)] = a[p] (+ b[p]); scalar, any view
    const void *a;
    const void *b;
    void *out;
    int H, W, C, a_ld, b_ld, out_ld, outmode, out_f32, a_f32;
    long long a_img_stride, b_img_stride, out_img_stride;
    long long total;           // B*H*W*C
};

struct ReduceParams {          // aux.hip: splitk_reduce_kernel -- sum of the K splits + the conv epilogue (conv_common.h semantics)
    const float *part;         // [ksplit][M][cout_pad]
    const float *bias;
    const void *res;           // residual (element pointer incl. coff) or null
    void *out;
    float *obj_out;            // head convs: compact objectness logits (see ConvParams)
    int obj_width, obj_rows, obj_row0, obj_na;
    int ksplit, M, Cout, cout_pad, HoWo, Wo;
    int out_ld, res_ld, leaky, outmode, out_f32, f32;
    long long out_img_stride, res_img_stride;
};

struct DecodeScale {
    int row0, h, w, na;
    double aw[YOLO_MAX_ANCHORS], ah[YOLO_MAX_ANCHORS];
};

struct DecodeParams {
    const float *logits;       // [B, rows, 5+C]
    const float *obj;          // optional compact copy of logits[..., 4] ([B, rows]): one coalesced read per row
    int version, n_classes, rows, n_scales;
    DecodeScale sc[YOLO_MAX_SCALES];
    float threshold;
    int cap;
    void *cand;                // Candidate[B][cap]
    int *cand_count;           // [B] counters, kCandCountStride ints apart (a 128-byte line each)
    long long total_rows;      // B*rows
};

struct Candidate {             // 40 bytes
    float x, y;
    double w, h;               // the reference computes w,h in float64 (anchors are np.float64)
    float prob;
    int cls;
    unsigned scan;             // scan index (cy, cw, anchor) across scales: stable-sort tie break
    int pad_;
};

struct NmsParams {
    const Candidate *cand;
    const int *cand_count;
    int *reset_count;          // non-null: the kernel returns cand_count[b] to zero once it has read it (the next decode needs no memset launch)
    int cap, max_boxes, mode;
    double iou_threshold;
    yolo_box *boxes;
    int *counts;
    int *status;
    int *keep_idx;             // optional [B][max_boxes]: candidate index of each survivor
    unsigned char *scratch;    // cap > 4096: [B][scratch_stride] bytes of global working storage (nms_scratch_bytes)
    size_t scratch_stride;
};

// ---- evaluation (eval.hip): the caller-owned state of the yolo_eval_* entries ------------------------------------------------
// [ EvalHeader | n_gt int32[n_classes] | records[cap] (arrival order) | sorted[cap] | ctp u32[cap] | cfp u32[cap] | sort entries[n2] ],
// every part 256-byte aligned; n2 = the power of two >= max(cap, kEvalSortTile) the bitonic network runs on.
struct EvalHeader {            // 256 bytes
    unsigned long long cursor; // records appended so far (may pass the capacity: then YOLO_EVAL_OVERFLOW is set and nothing was written there)
    unsigned status;           // enum yolo_eval_status bits
    unsigned pad_[61];
};
struct EvalEntry {             // sort item: (hi, lo, idx) ascending = class ascending, prob descending, seq ascending
    unsigned long long lo;     // ~orderable(prob) << 32 | seq
    unsigned hi;               // class; 0xffffffff = padding behind the records
    unsigned idx;              // arrival position of the record
};
constexpr int kEvalSortTile = 2048;     // entries one workgroup sorts in LDS (32 KiB)
struct EvalLayout {
    size_t header, n_gt, records, sorted, ctp, cfp, entries, total;
    int n2;
};
EvalLayout eval_layout(int n_classes, int det_capacity);
struct EvalMatchParams {
    const yolo_box *boxes;     // [batch][max_boxes]
    const int *counts;
    const yolo_gt *gt;         // [batch][max_gt]
    const int *gt_counts;
    int max_boxes, max_gt, n_classes, det_capacity;
    double match_iou;
    unsigned seq_base;         // image_base * max_boxes
    EvalHeader *hdr;
    int *n_gt;
    yolo_eval_record *records;
};
struct EvalFinishParams {
    EvalHeader *hdr;
    const int *n_gt;
    const yolo_eval_record *records;
    yolo_eval_record *sorted;
    unsigned *ctp, *cfp;
    EvalEntry *entries;
    int n2, n_classes, det_capacity;
    yolo_eval_result *result;  // header, then yolo_eval_class[n_classes]
};
hipError_t launch_eval_match(const EvalMatchParams &p, int batch, hipStream_t s);
hipError_t launch_eval_finish(const EvalFinishParams &p, hipStream_t s);

// ---- YOLOv2 loss (loss.hip) ---------------------------------------------------------------------------------------------------
struct LossParams {
    const float *logits;       // [B][h][w][A][5 + C]
    const yolo_gt *gt;         // [B][max_gt]
    const int *gt_counts;
    int max_gt, h, w, na, n_classes;
    double aw[YOLO_MAX_ANCHORS], ah[YOLO_MAX_ANCHORS];     // grid units, float64: the assignment (net/v2.py:270-272)
    float awf[YOLO_MAX_ANCHORS], ahf[YOLO_MAX_ANCHORS];    // ... rounded to float32: the terms (net/v2.py:136,140)
    yolo_loss_image *images;   // [B]
    int *assign;               // [B][h][w] or null
};
struct LossFinishParams {
    const yolo_loss_image *images;
    int n, n_repeat, batch_size;
    yolo_loss_result *result;
};
struct LossGradParams {
    const float *logits;       // [B][h][w][A][5 + C]
    const yolo_gt *gt;         // [B][max_gt]
    const int *assign;         // [B][h][w]: truth * 8 + anchor | -1, as loss_image_kernel wrote it
    float *grad;               // [B][h][w][A][5 + C], every element written
    int batch, max_gt, h, w, na, n_classes;
    float awf[YOLO_MAX_ANCHORS], ahf[YOLO_MAX_ANCHORS];
};
hipError_t launch_loss_images(const LossParams &p, int batch, hipStream_t s);
hipError_t launch_loss_finish(const LossFinishParams &p, hipStream_t s);
hipError_t launch_loss_grad(const LossGradParams &p, hipStream_t s);

// ---- YOLOv3 loss (loss3.hip; the geometry and the argument checks: loss3_host.h) ------------------------------------------------------
struct Loss3Params {
    const float *logits;       // [B][R][5 + C]
    const yolo_gt *gt;         // [B][max_gt]
    const int *gt_counts;
    int batch, max_gt;
    double ignore_thresh;
    Loss3Geometry geo;
    yolo_loss_image *parts;    // [B][geo.parts]
    yolo_loss_image *images;   // [B]
    int *assign;               // [B][R]: truth index | -1 none | -2 ignored
    yolo_loss_result *result;
    float *grad;               // [B][R][5 + C], every element written (loss3_grad_kernel only)
};
hipError_t launch_loss3(const Loss3Params &p, hipStream_t s);          // assign, terms, finish
hipError_t launch_loss3_grad(const Loss3Params &p, hipStream_t s);     // the gradient kernel alone, on the table launch_loss3 left

// ---- training the detection layer (train.hip; the launch split and the argument checks: train_host.h) ---------------------------
constexpr int kWgradThreads = 256;
struct WgradParams {
    const void *x;             // element 0 of the view's buffer: fp16 or float32 (launch_head_wgrad: x_dtype)
    const float *g;            // [P][cout]
    float *slab;               // [n_chunks][cout * cin + cout]
    float *dw, *db;            // [cout][cin], [cout]
    int P, cin, cout, ld, coff, ppi;       // ppi: positions per image
    long long img_stride;
    int ppc, n_chunks, tiles_cout, tiles_cin;      // yolo_wgrad_plan
    int slab_stride;           // cout * (cin + 1)
};
struct AdamParams {
    float *w, *b, *m_w, *v_w, *m_b, *v_b;
    const float *dw, *db;
    long long n_w, n_b;
    float lr_t, beta1, beta2, eps;
    void *pack_w;              // the conv's packed weights (row o at o * pack_row elements) or null
    float *pack_b;             // its float32 bias or null
    int pack_cin, pack_row, pack_f16;
};
hipError_t launch_head_wgrad(const WgradParams &p, int x_dtype, hipStream_t s);     // both kernels
hipError_t launch_adam_step(const AdamParams &p, hipStream_t s);

// ---- the weight gradient of the YOLOv3 head convs (train3.hip; the split and the argument checks: train3_host.h) -------------------------
struct Wgrad3Params : Wgrad3Geometry {
    const float *g;            // [B][R][5 + C]
    const int *assign;         // [B][R]: truth index | -1 none | -2 ignored (yolo_v3_loss_grad)
    int *slot;                 // [B][max_gt]: the row a truth owns or -1; written by head3_slot_kernel
    int batch, max_gt;
};
hipError_t launch_head3_wgrad(const Wgrad3Params &p, hipStream_t s);   // all four kernels

// ---- the data gradient of the detection layer and the 3 x 3 weight gradient (train_tail.hip; the split and the checks: train_tail_host.h) ----
struct DgradParams {
    const float *g;            // [P][cout]
    const float *w;            // [cout][cin], the float32 master kernel
    const void *y;             // element 0 of the view's buffer (fp16 or float32) or null: no activation factor
    float *d;                  // [P][cin]
    int P, cin, cout, ld, coff, ppi;
    long long img_stride;
    int tiles_cin;
    float slope;
};
struct Wgrad3x3Params {
    const void *x;             // element 0 of the view's buffer: fp16 or float32
    const float *d;            // [P][cout]
    const float *scale;        // [cout] or null
    float *slab;               // [n_chunks][cout * 9 * cin + cout]
    float *dw, *db;            // [cout][9][cin], [cout]
    int P, cin, cout, ld, coff, h, w, ppi;
    long long img_stride;
    int ppc, n_chunks, tiles_cout, tiles_cin, halo_rows;       // yolo_conv3x3_wgrad_plan
    int slab_stride;           // cout * (9 * cin + 1)
};
struct TailAdamParams {
    AdamParams a;              // w = W3 [cout3][9 * cin3], b = beta; pack_cin = 9 * cin3; pack_w, pack_b, pack_row as for the head
    const double *scale64;     // [cout3]: the batch-norm fold's scale
    const float *mean;         // [cout3]
};
hipError_t launch_tail_adam(const TailAdamParams &p, hipStream_t s);
hipError_t launch_conv1x1_dgrad(const DgradParams &p, int y_dtype, long long tiles, hipStream_t s);
hipError_t launch_conv3x3_wgrad(const Wgrad3x3Params &p, int x_dtype, hipStream_t s);      // both kernels
// train_tail_f16.hip: the same launch on the fp16 matrix cores (x is fp16); record: the m / k record behind the slabs (yolo_conv3x3_wgrad_f16_plan)
// db_groups groups of db_positions positions: the partial sums of db, behind the record
hipError_t launch_conv3x3_wgrad_f16(const Wgrad3x3Params &p, unsigned int *record, int db_groups, int db_positions, hipStream_t s);    // the clear and all three kernels

// ---- the sparse data gradient of a YOLOv3 head conv (train3_tail.hip; the split, the record and the checks: train3_tail_host.h) ---------------
hipError_t launch_head3_dgrad(const Dgrad3Params &p, hipStream_t s);

// ---- launchers (kernels.hip / detect.hip) ------------------------------------------------
hipError_t launch_conv(const ConvParams &p, int dtype, int cfg, bool perchunk, hipStream_t s);
// conv_dma.hip: 8-wave LDS-DMA kernel for the heavy fp16 layers; conv_tap.hip: 3x3 with tap reuse.  What a tile id is: conv_tiles.h.
// choose_dma_cfg returns 0 when the 4-wave kernel of conv.hip should run, else the tile id for launch_conv_dma.
struct ConvTile;
int choose_dma_cfg(int M, int cout, int cin_chunks, int taps, int has_res, bool v1_ok, int stride, int W, bool tap_only = false);   // -1: no DMA tile and no 4-wave kernel fits
bool dma_cfg_valid(int cfg, int cout, int cin_chunks, bool v1_ok, int ksize, int stride, int W);
hipError_t launch_conv_dma(const ConvParams &p, int cfg, hipStream_t s);           // any tile id > 0: sets up the grid, then launch_conv_tap for a tap tile
hipError_t launch_conv_tap(const ConvParams &p, int tile, hipStream_t s);
bool conv_tap_fits(const ConvTile &t, int W);
// the kernel that runs THIS launch (p.ksplit, p.pair, p.fuse2 as launched), named as rocprofv3's kernel trace prints it (yolo_kernel_info.symbol)
std::string conv_tile_symbol(int tile, ConvParams p);
std::string conv_tap_symbol(const ConvTile &t, const ConvParams &p);
// conv_mx.hip (MXFP8 plans): 3x3 / stride 1, Cin % 128 == 0, W <= kMxMaxW (the 128-channel patch of a 256-position tile in LDS, twice)
constexpr int kMxMaxW = 100;
constexpr int kMxTile = 24;           // its yolo_net_options.force_tile id (force_tile = 25)
bool conv_mx_fits(int W);
const char *conv_mx_symbol(bool fast);
hipError_t launch_conv_mx(const ConvParams &p, hipStream_t s);
hipError_t launch_mx_quantize(const void *src, int rows, int channels, unsigned char *q, unsigned char *sc, hipStream_t s);
// host copy of the device quantizer (mx_quant_block): one block of 32 float values -> e4m3fn bytes, returns the E8M0 byte
unsigned char mx_quant_block_host(const float *v, unsigned char *q);
std::string conv_symbol(int dtype, int cfg, bool perchunk, bool f32_emu = false);
// float32 nets: does this launch of the 4-wave kernel run its products as nine bf16 products (yolo_net_options.f32_products)?
bool conv_f32_emu_rule(int f32_products, int dtype, const ConvParams &p, int cfg, bool perchunk, int ksplit);
std::string first_symbol(int dtype, int cout, bool pool);
std::string aux_symbol(int kind, int dtype, bool vec);
std::string pool_same_symbol(int dtype, bool vec);
std::string spp_pool_symbol(int rad);
__attribute__((visibility("hidden"))) ReduceParams reduce_params(const ConvParams &p);           // the second pass of the split-K launch `p` (p.ksplit, p.part as launched)
hipError_t launch_splitk_reduce(const ReduceParams &p, hipStream_t s);
// in_u8 / dst_u8: the kernel's uint8 twin runs -- `in` (`dst`) holds bytes, dense, any alignment (the parameter blocks are the same)
hipError_t launch_prep(const PrepParams &p, int dtype, hipStream_t s, bool in_u8 = false);
hipError_t launch_resize(const ResizeParams &p, hipStream_t s, bool dst_u8 = false);
hipError_t launch_frames_resize(const FramesParams &p, int n, hipStream_t s, bool dst_u8);     // n <= kFramesPerLaunch frames
hipError_t launch_boxes_to_frames(const RemapParams &p, int n, hipStream_t s);                 // n <= kFramesPerLaunch images
hipError_t launch_augment(const AugmentParams &p, int n, hipStream_t s);                      // augment.hip: n <= kAugPerLaunch images
// anchor.hip: one kernel of the anchor k-means (ANCHOR_SEED_SUM / _PICK: p.round is the seeding round)
enum AnchorStage { ANCHOR_PREPARE, ANCHOR_INIT, ANCHOR_SEED_SUM, ANCHOR_SEED_PICK, ANCHOR_ASSIGN, ANCHOR_UPDATE, ANCHOR_FINAL, ANCHOR_FINISH, ANCHOR_LABELS };
hipError_t launch_anchor(int stage, const AnchorParams &p, hipStream_t s);
hipError_t launch_first(const FirstParams &p, int dtype, hipStream_t s, bool in_u8 = false);
hipError_t launch_stem(const StemParams &p, int batch, hipStream_t s, int max_grid = kStemGrid, bool in_u8 = false);     // stem.hip
hipError_t launch_pool(const PoolParams &p, int dtype, hipStream_t s);
hipError_t launch_pool_same(const PoolParams &p, int dtype, hipStream_t s);     // stride 1, SAME, odd window PoolParams.ksize
constexpr int kSppMaxSide = 32;         // spp_pool_kernel: the H x W plane of a chunk lives in LDS twice (2 x 16 KiB at 32 x 32)
hipError_t launch_spp(const SppParams &p, int rad, int batch, hipStream_t s);   // p.H, p.W <= kSppMaxSide; windows 2 rad + 1, 4 rad + 1, 6 rad + 1 (rad 1 | 2)
int spp_slab(int H, int W, int chunks, int batch);                              // chunks per workgroup launch_spp picks
hipError_t launch_eltwise(const EltParams &p, int dtype, hipStream_t s);
hipError_t launch_decode(const DecodeParams &p, int batch, hipStream_t s, bool zero_counts = true);
hipError_t launch_nms(const NmsParams &p, int batch, hipStream_t s);
size_t nms_lds_bytes(int cap);
size_t nms_scratch_bytes(int cap);

// ---- plan -----------------------------------------------------------------------------------
enum StemRole {
    STEM_NONE = 0,
    STEM_FIRST_FOLDED = 1,     // K_FIRST: the first-layer kernel is fused away into the next conv (no launch)
    STEM_HOST = 2,             // K_CONV: this 3x3/2 conv runs as stem.hip, together with the first layer in front of it
    STEM_TAIL = 3,             // K_CONV: this 1x1 conv is computed by the stem kernel in front of it (no launch)
};
struct Kernel {
    int kind = 0;
    int layer = -1;            // reference layer index this kernel materialises
    int src_layer = -1;        // conv: the conv layer whose weights it uses
    View in, in2, out;
    // conv
    int ksize = 0, stride = 0, cout = 0, cin = 0, cin_s = 0, leaky = 0, outmode = 0, has_res = 0;
    int cfg = 0, perchunk = 0, cpt = 0, ktiles = 0;
    int tile = -1;             // conv_dma tile id chosen by yolo_net_autotune (-1: heuristic)
    int head = 0;              // conv writes float32 head logits into the reference-layout output
    int pool_fused = 0;        // K_FIRST: the max-pool layer behind it is taken in the same kernel
    StemRole stem = STEM_NONE; // this kernel's part in the Darknet-53 stem launch (stem.hip), if any
    int fuse2_next = 0;        // the NEXT kernel is a 1x1 128 -> 64 conv on this conv's output that the fused instantiation of this launch
                               // can compute (conv_common.h: conv_epilogue_fused_1x1); whether it does is decided per launch (conv_dispatch.cpp: resolve_conv)
    int fuse2_prev = 0;        // ... and the mark on that 1x1: skipped when the conv in front of it has computed it
    int mx = 0;                // MXFP8 plans: this conv runs conv3x3_mx_kernel (conv_mx.hip) on block-scaled e4m3 operands
    int side = 0;              // > 0: member of branch tail `side` (plan.cpp: side_chains): a run of kernels ending in a head conv whose
                               // results nothing else reads -- may run on a second stream beside the kernels that follow it in the list
    size_t w_off = 0, b_off = 0, w_bytes = 0;   // inside the device weight blob
    size_t w_src = 0;                           // first float of this conv in the Darknet stream
    int batch_norm = 0;
    // pool
    int pool_stride = 0;
    int pool_k = 2;            // window: 2 = pool_kernel; odd 3..13 (stride 1, SAME) = pool_same_kernel, or with `spp` the smallest window of the block
    int spp = 0;               // 1: spp_pool_kernel -- this launch also writes the two wider pools of the SPP block into out2 / out3
    int spp_layer[2] = {-1, -1};   // ... which materialise these layers
    View out2, out3;
    std::string note;
};
// this conv goes through the conv dispatch (conv_dispatch.cpp: resolve_conv) -- the stem's launch and the 1x1 it computes do not
inline bool conv_dispatched(const Kernel &k) { return k.kind == K_CONV && k.stem != STEM_HOST && k.stem != STEM_TAIL; }
// this kernel has a launch of its own -- the two the stem kernel computes beside its 3x3/2 conv have none
inline bool has_own_launch(const Kernel &k) { return !(k.kind == K_FIRST && k.stem == STEM_FIRST_FOLDED) && !(k.kind == K_CONV && k.stem == STEM_TAIL); }
// counts as a conv launch for the stream rule (plan.cpp: allocate)
inline bool counts_as_conv_launch(const Kernel &k) { return k.kind == K_CONV && k.stem != STEM_TAIL; }

struct LayerInfo {
    yolo_layer_desc d;
    int H = 0, W = 0, C = 0;
    std::vector<int> consumers;
    int fused_into = -1;       // conv kernel (layer idx) that produces this layer's tensor
    View view;                 // where the layer's output lives (after alias resolution)
    bool materialised = false;
};

// One region of the workspace behind the activation arenas (yolo_net_workspace_regions reports them as laid out)
struct __attribute__((visibility("hidden"))) WsRegion {
    const char *name;
    size_t offset, used, bytes;
};

// The streams and events a net creates at first use (forward.cpp: side_streams, branch_streams; destroy_streams at yolo_net_destroy).
struct __attribute__((visibility("hidden"))) StreamPool {
    std::vector<hipStream_t> side;         // multi-stream forward (YOLO_STREAMS=N): parts 1.. run here, part 0 on the caller's stream
    std::vector<hipEvent_t> fork, join;    // ... one fork event, one join event per side stream
    std::vector<hipStream_t> branch;       // one stream per arena for the branch tails (Kernel.side)
    std::vector<hipEvent_t> bfork, bjoin;  // ... with four fork events and one join event per arena
};

}  // namespace yolo

struct yolo_net {
    yolo_net_options opt;          // (an MXFP8 plan keeps dtype = YOLO_DTYPE_F16 here: fp16 storage and kernels, `mx` set)
    bool mx = false;               // created as YOLO_DTYPE_MXF8: the eligible 3x3 convs run conv_mx.hip (Kernel.mx)
    std::vector<yolo::LayerInfo> layers;
    std::vector<yolo::Kernel> kernels;
    std::vector<yolo::Buffer> buffers;
    yolo_head_desc head;
    size_t weight_count = 0;       // floats in the Darknet stream
    size_t weights_bytes = 0;
    size_t act_bytes = 0;          // activation part of the workspace
    size_t logits_off = 0, cand_off = 0, count_off = 0, nms_off = 0;   // nms_off: global NMS slabs (cand_capacity > 4096)
    size_t splitk_off = 0, splitk_bytes = 0;   // float32 partial-sum slabs of the split-K convs (small feature maps at small batch)
    std::vector<yolo::WsRegion> tail;      // the regions from logits_off on, in offset order: plan_network lays them out, yolo_net_create appends the split-K one
    size_t obj_off = 0, obj_bytes = 0;     // compact objectness logits [max_batch][rows] written by the head convs for the decode
    bool obj_valid = false;                // ... and whether the last forward filled all of it
    int cand_clean = 0;                    // how many candidate counters, from the first, are known to be zero (the last detect's NMS returned them): no memset launch in front of a decode of at most that batch
    int side_chains = 0;                   // number of branch tails (Kernel.side ids 1..side_chains)
    std::vector<signed char> side_ok;      // per batch: may the branch tails run beside the main chain (-1 unknown; no split-K launch in the pass)
    float obj_min_logit = -__builtin_inff();      // inside yolo_net_detect: objectness logit below which a row can never be a candidate (ConvParams.obj_min)
    yolo::StreamPool streams;
    int arenas = 1;                        // activation arenas (2: one per half batch)
    // streams = 0 picked two parts by rule: every arena is then planned for the FULL batch, so that the same net can also run one pass
    // on one stream, and `parts` (1 or 2) says what a forward does -- the rule's answer until yolo_net_tune_streams has timed both
    // on this device (two halves gain 3-4 % on some MI355X and lose 1-2 % on others: profiles/r04_ablation.md section 7)
    bool arena_full = false;
    int parts = 1;                         // parts a full batch currently runs as (== arenas unless arena_full)
    bool parts_tuned = false;
    size_t arena_bytes = 0;
    bool halves = false;                   // the current forward runs as two concurrent half-batch passes
    size_t workspace_bytes = 0;
    size_t out_count = 0;          // floats per image of the head output
    double flops_per_image = 0;
    int esize = 2, epc = 8;
    // bound device memory
    unsigned char *dev_weights = nullptr;
    unsigned char *dev_ws = nullptr;
    size_t dev_ws_bytes = 0;
    bool weights_loaded = false;
    // yolo_net_train_set_wgrad_f16: the caller's scratch of yolo_conv3x3_wgrad_f16, which the tail and blocks steps then run in place of
    // yolo_conv3x3_wgrad; null: the float32 steps
    unsigned char *wgrad_f16_dev = nullptr;
    size_t wgrad_f16_bytes = 0;
};

namespace yolo {
int plan_network(yolo_net *net, const yolo_layer_desc *layers, int n, std::string &err);
bool mx_eligible(const yolo_net *net, const Kernel &k);
int pack_weights(const yolo_net *net, const float *host, size_t n, std::vector<unsigned char> &blob, std::string &err);
std::string describe(const yolo_net *net);
void set_error(const std::string &s);
const char *get_error();
inline int fail(int code, const std::string &msg) {
    set_error(msg);
    return code;
}
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            yolo::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                \
            return YOLO_ERR_HIP;                                                               \
        }                                                                                      \
    } while (0)

// ---- conv dispatch (conv_dispatch.cpp) ------------------------------------------------------
// images one part of a full batch holds (what every launch of a forward pass sees at most)
inline int part_batch(const yolo_net *net) { return (net->opt.max_batch + net->parts - 1) / net->parts; }
// An arena's share of the split-K region: [ticket counters of the in-launch splits, kPairCounterBytes | float32 partial sums]
// (conv_tap.hip: one ticket per tile, a 128-byte line each, 512 tiles).  Concurrent parts (streams) must not share a slab.
constexpr size_t kPairCounterBytes = 65536;
constexpr size_t kSplitkSlabMax = (size_t)64 << 20;     // partial sums per arena, at most
inline size_t arena_slab_bytes(const yolo_net *net) { return net->splitk_bytes / (size_t)net->arenas / 256 * 256; }
inline size_t arena_slab_data_bytes(const yolo_net *net) {
    const size_t slab = arena_slab_bytes(net);
    return slab > kPairCounterBytes ? slab - kPairCounterBytes : 0;
}
// What one conv launch runs: the tile (conv_tiles.h: 0 = the 4-wave kernel of conv.hip with the planner's cfg), the K
// split (ks = 1: whole K; else ks splits of ku units), whether the splits meet inside the launch (pair), whether the launch also
// computes the 1x1 conv behind it (fuse2), and the bytes of partial sums it writes (0 if none).
struct ConvLaunch {
    int tile, ks, ku, pair, fuse2;
    size_t slab_need;
};
void conv_shape_params(const yolo_net *net, const Kernel &k, int batch, ConvParams &p);
ConvLaunch resolve_conv(const yolo_net *net, size_t ki, const ConvParams &p, int tile_req, size_t slab_bytes);
bool dma_eligible(const yolo_net *net, const Kernel &k);
bool conv_tile_valid(const yolo_net *net, const Kernel &k, int tile);
size_t splitk_slab_bytes(const yolo_net *net);          // per arena, tickets included
bool pass_splits_k(const yolo_net *net, int batch);     // any conv launch of a forward pass at this batch splits K
void conv_kernel_info(const yolo_net *net, int kernel, yolo_kernel_info *out);
// what the yolo_kernel_info reports (conv_kernel_info, aux_kernel_info) are written with
inline double view_elems(const View &v) { return (double)v.H * v.W * v.C; }
inline double view_esz(const yolo_net *net, const View &v) { return v.f32 ? 4.0 : (double)net->esize; }
inline const char *dtype_tag(const yolo_net *net) { return net->opt.dtype == YOLO_DTYPE_F16 ? "f16" : "f32"; }
inline void set_symbol(yolo_kernel_info *out, const std::string &sym) { snprintf(out->symbol, sizeof out->symbol, "%s", sym.c_str()); }

// ---- forward engine (forward.cpp) -----------------------------------------------------------
// The network input of one call: the caller's float32 tensor, or (ABI 7: the *_u8 entries) its uint8 one.  Only the five kernels that
// read the input look at the tag (K_PREP, K_FIRST, the stem); a byte u is to them float32(u / 255.) (u8_unit).
struct NetIn {
    const void *ptr;
    bool u8;
    NetIn at(size_t elems) const { return NetIn{static_cast<const unsigned char *>(ptr) + elems * (u8 ? 1 : 4), u8}; }
};
// Every entry below expects a checked call (check_ready) and leaves its message in set_error.  (Hidden: what moved out of
// api.cpp's anonymous namespace adds nothing to the symbols the library exports.)
#pragma GCC visibility push(hidden)
int run_forward(yolo_net *net, NetIn in_dev, int batch, float *out_dev, hipStream_t s);
int run_forward_timed(yolo_net *net, NetIn in_dev, int batch, float *out_dev, hipStream_t s, float *ms_host);   // ms_host[kernel]
int tune_streams(yolo_net *net, NetIn in_dev, int batch, hipStream_t s, const char *who);
int autotune_tiles(yolo_net *net, NetIn in_dev, int batch, hipStream_t s);
bool all_heads_write_objectness(yolo_net *net, NetIn in_dev, float *out_dev, int batch);   // every head conv fills the compact objectness array at this batch
int zero_pair_counters(yolo_net *net);
void destroy_streams(yolo_net *net);
void aux_kernel_info(const yolo_net *net, int kernel, yolo_kernel_info *out);              // yolo_net_kernel_info of every kind but K_CONV

// ---- shared with the training entries (api.cpp defines them, train_api.cpp calls them too) -------------------------------------
int check_head(const yolo_head_desc *h, size_t out_count, std::string &err);               // a set head, matching out_count floats per image if that is not 0
int check_ready(yolo_net *net, const void *in, int batch, const char *who);                // batch, weights, workspace
int check_loss_args(const yolo_head_desc *head, const void *gt_dev, const void *gt_counts_dev, int max_gt, const void *images_dev,
                    const void *result_dev, const char *who);                              // the arguments of a YOLOv2 loss call
int run_loss_grad(const yolo_head_desc &h, const float *logits, int batch, const yolo_gt *gt, const int32_t *gt_counts, int max_gt,
                  yolo_loss_image *images, int32_t *assign, yolo_loss_result *result, float *grad, hipStream_t s);
int run_loss3(const Loss3Geometry &geo, const float *logits, int batch, const yolo_gt *gt, const int32_t *gt_counts, int max_gt,
              double ignore_thresh, yolo_loss_image *parts, yolo_loss_image *images, int32_t *assign, yolo_loss_result *result, float *grad,
              hipStream_t s);                                                               // grad null: the loss alone
#pragma GCC visibility pop
// every part of a scratch or state arena starts at a 256-byte boundary
inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
}  // namespace yolo

// YOLOv2 loss on the device (include/yolo_hip.h: yolo_v2_loss, yolo_net_loss*, yolo_loss_reduce, yolo_v2_loss_grad; the definitions are
// there).
//
// loss_image_kernel   replaces net/v2.py:242-295 _make_ground_truths and the per-image part of net/v2.py:123-198 create_loss_fn: one
//                     workgroup per image assigns the truths to (cell, anchor) slots in LDS and sums the image's terms in float64.
// loss_finish_kernel  the reduce_sum / batch_size of net/v2.py:181-188 over the per-image records, in image order.
// loss_grad_kernel    replaces tf.gradients of net/v2.py:188 with respect to net[-1].out (what AdamOptimizer.minimize, net/v2.py:205, takes):
//                     d loss / d logits from the winner table of loss_image_kernel, a wave per grid cell.
// Compiled with default NaN handling, like detect.hip and eval.hip.
#include <hip/hip_runtime.h>

#include "yolo_internal.h"
#include "head_math.h"       // sigmoid_f32 (the decode's), eval_iou (the evaluation's)

namespace yolo {

constexpr int kLossThreads = 256;
constexpr int kLossWaves = kLossThreads / 64;
constexpr int kGradRowRegs = 16;        // elements of a row a lane of loss_grad_kernel keeps in registers

// tf.maximum / tf.minimum as NumPy's: a NaN operand is the result
__device__ __forceinline__ float np_maxf(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float np_minf(float a, float b) { return (a <= b || a != a) ? a : b; }

// net/v2.py:157-173 in float32, every operation rounded on its own; no floor on the union
__device__ __forceinline__ float loss_iou_f32(float gx, float gy, float gw, float gh, float px, float py, float pw, float ph) {
#pragma clang fp contract(off)
    const float gx1 = gx - gw / 2.f, gy1 = gy - gh / 2.f, gx2 = gx + gw / 2.f, gy2 = gy + gh / 2.f;
    const float px1 = px - pw / 2.f, py1 = py - ph / 2.f, px2 = px + pw / 2.f, py2 = py + ph / 2.f;
    const float iw = np_maxf(np_minf(px2, gx2) - np_maxf(px1, gx1), 0.f);
    const float ih = np_maxf(np_minf(py2, gy2) - np_maxf(py1, gy1), 0.f);
    const float inter = iw * ih;
    const float uni = pw * ph + gw * gh - inter;
    return inter / uni;
}

// the three terms of a winner slot (net/v2.py:181-183 without the weights), float32, every operation rounded on its own
__device__ __forceinline__ void loss_winner_terms(const float *t, float c, float r, float aw, float ah, float gx, float gy, float gw, float gh,
                                                  float po, float &xy, float &wh, float &obj) {
#pragma clang fp contract(off)
    const float px = sigmoid_f32(t[0]) + c, py = sigmoid_f32(t[1]) + r;
    const float pw = expf(t[2]) * aw, ph = expf(t[3]) * ah;
    const float dx = gx - px, dy = gy - py;
    xy = dx * dx + dy * dy;
    const float sw = sqrtf(gw) - sqrtf(pw), sh = sqrtf(gh) - sqrtf(ph);
    wh = sw * sw + sh * sh;
    const float d = loss_iou_f32(gx, gy, gw, gh, px, py, pw, ph) - po;
    obj = d * d;
}

// One workgroup per image.
//   phase 1a  a thread per truth: checks, cell, and the truth's own best anchor -- the first anchor that reaches the truth's largest IoU
//             (the IoU does not depend on the cell), into LDS
//   phase 1b  a thread per cell: scans the truths in list order for the first one of this cell that reaches the cell's largest IoU;
//             with 1a that is the first (truth, anchor) pair in the reference's scan order.  Winner table in LDS: truth * 8 + anchor | -1
//   phase 2   a thread per (cell, anchor) slot: objectness of every slot, the box terms of a winner slot
//   phase 3   a wave per cross-entropy row of the cells with a winner (all A slots), lanes striding over the classes
//   sums      float64, fixed order: thread (slots ascending) -> lane tree -> waves in index order
__global__ void __launch_bounds__(kLossThreads) loss_image_kernel(const LossParams p) {
    __shared__ double t_iou[YOLO_EVAL_MAX_GT];
    __shared__ int t_cell[YOLO_EVAL_MAX_GT];           // -1: skipped
    __shared__ int t_anchor[YOLO_EVAL_MAX_GT];
    __shared__ int s_win[YOLO_LOSS_MAX_CELLS];
    __shared__ double ws[kLossWaves][5];
    __shared__ int ws_n[kLossWaves];
    __shared__ int s_status, s_truths;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = p.h * p.w, width = 5 + p.n_classes;
    if (tid == 0) { s_status = 0; s_truths = 0; }
    __syncthreads();
    int flags = 0;
    int ng = p.gt_counts[b];
    if (ng < 0 || ng > p.max_gt) { flags |= YOLO_LOSS_BAD_COUNT; ng = ng < 0 ? 0 : p.max_gt; }
    const yolo_gt *gt = p.gt + (size_t)b * p.max_gt;
    const double half_w = (double)p.w / 2., half_h = (double)p.h / 2.;     // v2.py:269
    // ---- phase 1a
    for (int g = tid; g < ng; g += kLossThreads) {
        const yolo_gt t = gt[g];
        const double bx = (double)t.x * (double)p.w, by = (double)t.y * (double)p.h;       // v2.py:252-255
        const double bw = (double)t.w * (double)p.w, bh = (double)t.h * (double)p.h;
        const double cxf = floor(bx), cyf = floor(by);
        int bad = 0;
        if (!(cxf >= 0. && cxf < (double)p.w && cyf >= 0. && cyf < (double)p.h)) bad |= YOLO_LOSS_OUT_OF_GRID;     // (a NaN centre too)
        if (!(t.w >= 0.f) || !(t.h >= 0.f)) bad |= YOLO_LOSS_BAD_BOX;
        if (t.class_idx < 0 || t.class_idx >= p.n_classes) bad |= YOLO_LOSS_BAD_CLASS;
        double best = -1.;
        int ba = 0;
        if (!bad) {
            for (int a = 0; a < p.na; ++a) {
                const double iou = eval_iou(half_w, half_h, bw, bh, half_w, half_h, p.aw[a], p.ah[a]);
                if (best < iou) { best = iou; ba = a; }         // v2.py:273: strict, a NaN never wins
            }
            atomicAdd(&s_truths, 1);
        }
        flags |= bad;
        t_cell[g] = bad ? -1 : (int)cyf * p.w + (int)cxf;
        t_iou[g] = best;
        t_anchor[g] = ba;
    }
    if (flags) atomicOr(&s_status, flags);
    __syncthreads();
    // ---- phase 1b
    for (int cell = tid; cell < hw; cell += kLossThreads) {
        double best = -1.;
        int win = -1;
        for (int g = 0; g < ng; ++g)
            if (t_cell[g] == cell && best < t_iou[g]) { best = t_iou[g]; win = g * 8 + t_anchor[g]; }
        s_win[cell] = win;
        if (p.assign) p.assign[(size_t)b * hw + cell] = win;
    }
    __syncthreads();
    // ---- phase 2
    const int nslots = hw * p.na;
    const float *logits = p.logits + (size_t)b * nslots * width;
    double acc_xy = 0., acc_wh = 0., acc_obj = 0., acc_noobj = 0.;
    int n_assigned = 0;
    for (int s = tid; s < nslots; s += kLossThreads) {
        const int cell = s / p.na, a = s - cell * p.na;
        const int win = s_win[cell];
        const float *t = logits + (size_t)s * width;
        const float po = sigmoid_f32(t[4]);
        if (win >= 0 && (win & 7) == a) {
            const yolo_gt g = gt[win >> 3];
            const float gx = (float)((double)g.x * (double)p.w), gy = (float)((double)g.y * (double)p.h);   // the float32 placeholder, v2.py:145
            const float gw = (float)((double)g.w * (double)p.w), gh = (float)((double)g.h * (double)p.h);
            const int r = cell / p.w, c = cell - r * p.w;
            float xy, wh, obj;
            loss_winner_terms(t, (float)c, (float)r, p.awf[a], p.ahf[a], gx, gy, gw, gh, po, xy, wh, obj);
            acc_xy += (double)xy; acc_wh += (double)wh; acc_obj += (double)obj;
            ++n_assigned;
        } else {
            acc_noobj += (double)(po * po);
        }
    }
    // ---- phase 3: the wave takes 64 cells at a time, and of those the ones with a winner in index order (wave-uniform control flow)
    double acc_cls = 0.;            // (the same value on every lane)
    for (int base = wave * 64; base < hw; base += 64 * kLossWaves) {
        const int mine = base + lane < hw ? s_win[base + lane] : -1;
        unsigned long long todo = __ballot(mine >= 0);
        while (todo) {
            const int l = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int win = __shfl(mine, l);
            const int cls = gt[win >> 3].class_idx;             // (in [0, C): the truth was checked in phase 1a)
            for (int a = 0; a < p.na; ++a) {
                const float *tc = logits + ((size_t)(base + l) * p.na + a) * width + 5;
                const int label = a == (win & 7) ? cls : 0;     // v2.py:155: argmax of an all-zero one-hot is 0
                float mx = -__builtin_inff();
                for (int k = lane; k < p.n_classes; k += 64) mx = np_maxf(mx, tc[k]);
                for (int off = 32; off > 0; off >>= 1) mx = np_maxf(mx, __shfl_xor(mx, off));
                float sum = 0.f;
                for (int k = lane; k < p.n_classes; k += 64) sum += expf(tc[k] - mx);
                for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);    // (a + b == b + a: every lane ends with the same bits)
                const float ce = logf(sum) - (tc[label] - mx);
                acc_cls += (double)ce;
            }
        }
    }
    // ---- sums
    for (int d = 32; d > 0; d >>= 1) {
        acc_xy += __shfl_down(acc_xy, d); acc_wh += __shfl_down(acc_wh, d);
        acc_obj += __shfl_down(acc_obj, d); acc_noobj += __shfl_down(acc_noobj, d);
        n_assigned += __shfl_down(n_assigned, d);
    }
    if (lane == 0) {
        ws[wave][0] = acc_xy; ws[wave][1] = acc_wh; ws[wave][2] = acc_obj; ws[wave][3] = acc_noobj; ws[wave][4] = acc_cls;
        ws_n[wave] = n_assigned;
    }
    __syncthreads();
    if (tid == 0) {
        yolo_loss_image out;
        double s[5] = {0., 0., 0., 0., 0.};
        int n = 0;
        for (int w = 0; w < kLossWaves; ++w) {
            for (int k = 0; k < 5; ++k) s[k] += ws[w][k];
            n += ws_n[w];
        }
        out.xy = s[0]; out.wh = s[1]; out.obj = s[2]; out.noobj = s[3]; out.cls = s[4];
        out.n_assigned = n; out.n_truths = s_truths; out.status = s_status; out.pad_ = 0;
        p.images[b] = out;
    }
}

// One workgroup: the records come into LDS 256 at a time (parallel loads), one thread adds them in image order.
__global__ void __launch_bounds__(kLossThreads) loss_finish_kernel(const LossFinishParams p) {
    __shared__ yolo_loss_image rec[kLossThreads];
    const int tid = threadIdx.x;
    double s[5] = {0., 0., 0., 0., 0.};
    int n_assigned = 0, n_truths = 0, status = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int n = pass ? p.n_repeat : p.n;          // net/v2.py:215-217: the first n_repeat records once more
        for (int base = 0; base < n; base += kLossThreads) {
            __syncthreads();
            if (base + tid < n) rec[tid] = p.images[base + tid];
            __syncthreads();
            if (tid == 0) {
                const int m = n - base < kLossThreads ? n - base : kLossThreads;
                for (int i = 0; i < m; ++i) {
                    s[0] += rec[i].xy; s[1] += rec[i].wh; s[2] += rec[i].obj; s[3] += rec[i].noobj; s[4] += rec[i].cls;
                    n_assigned += rec[i].n_assigned; n_truths += rec[i].n_truths; status |= rec[i].status;
                }
            }
        }
    }
    if (tid == 0) {
        const double B = (double)p.batch_size;
        yolo_loss_result r;
        r.loss_xy = s[0] / B;                           // v2.py:181-185
        r.loss_wh = s[1] / B;
        r.loss_obj = 5. * s[2] / B;
        r.loss_noobj = s[3] / B;
        r.loss_class = s[4];
        r.loss = r.loss_xy + r.loss_wh + r.loss_obj + r.loss_noobj + r.loss_class;      // v2.py:188
        r.n_assigned = n_assigned; r.n_truths = n_truths; r.status = status; r.pad_ = 0;
        *p.result = r;
    }
}

// The five box elements of a winner slot (yolo_hip.h: the gradient, "winner slot"), float32, every operation rounded on its own and in
// the order tests/loss_grad_ref.py writes them, so that a non-finite element appears where the float32 restatement has one.  The
// brackets are TensorFlow's tie rules: maximum(x, y) passes to x on x >= y, minimum(x, y) on x <= y, maximum(rw, 0) on rw >= 0.
__device__ __forceinline__ void loss_grad_winner(const float *t, float c, float r, float aw, float ah, float gx, float gy, float gw, float gh,
                                                 float po, float lam, float lam_obj, float out[5]) {
#pragma clang fp contract(off)
    const float sx = sigmoid_f32(t[0]), sy = sigmoid_f32(t[1]);
    const float px = sx + c, py = sy + r;
    const float pw = expf(t[2]) * aw, ph = expf(t[3]) * ah;
    const float gx1 = gx - gw / 2.f, gy1 = gy - gh / 2.f, gx2 = gx + gw / 2.f, gy2 = gy + gh / 2.f;
    const float px1 = px - pw / 2.f, py1 = py - ph / 2.f, px2 = px + pw / 2.f, py2 = py + ph / 2.f;
    const float rw = np_minf(px2, gx2) - np_maxf(px1, gx1), rh = np_minf(py2, gy2) - np_maxf(py1, gy1);
    const float iw = np_maxf(rw, 0.f), ih = np_maxf(rh, 0.f);
    const float inter = iw * ih;
    const float uni = pw * ph + gw * gh - inter;
    const float iou = inter / uni;
    const float hi_x = px2 <= gx2 ? 1.f : 0.f, lo_x = px1 >= gx1 ? 1.f : 0.f, hi_y = py2 <= gy2 ? 1.f : 0.f, lo_y = py1 >= gy1 ? 1.f : 0.f;
    const float on_w = rw >= 0.f ? 1.f : 0.f, on_h = rh >= 0.f ? 1.f : 0.f;
    const float diw_dpx = on_w * (hi_x - lo_x), diw_dpw = on_w * (hi_x + lo_x) / 2.f;
    const float dih_dpy = on_h * (hi_y - lo_y), dih_dph = on_h * (hi_y + lo_y) / 2.f;
    const float both = uni + inter, uni2 = uni * uni;
    const float di_dpx = ih * diw_dpx * both / uni2, di_dpy = iw * dih_dpy * both / uni2;
    const float di_dpw = (ih * diw_dpw * both - inter * ph) / uni2, di_dph = (iw * dih_dph * both - inter * pw) / uni2;
    const float k = lam_obj * (2.f * (iou - po));
    const float dl_dpx = lam * (2.f * (px - gx)) + k * di_dpx, dl_dpy = lam * (2.f * (py - gy)) + k * di_dpy;
    const float rpw = sqrtf(pw), rph = sqrtf(ph);
    const float dl_dpw = lam * ((rpw - sqrtf(gw)) / rpw) + k * di_dpw, dl_dph = lam * ((rph - sqrtf(gh)) / rph) + k * di_dph;
    out[0] = dl_dpx * (sx * (1.f - sx));
    out[1] = dl_dpy * (sy * (1.f - sy));
    out[2] = dl_dpw * pw;
    out[3] = dl_dph * ph;
    out[4] = -k * (po * (1.f - po));
}

// Grid (chunks of kLossWaves cells) x (image): the winner table makes every slot independent, so a wave takes a cell -- A * (5 + C)
// contiguous floats -- and works on its A rows AT THE SAME TIME: the 64 lanes are split into groups of L = 64 / (A rounded up to a power
// of two) lanes, group a owns row a (A = 5: eight lanes a row, three groups idle).  Rows one after the other would be A dependent chains of
// load -> max -> load -> sum -> load -> store, each link a memory round trip; side by side they are one chain.  Inside a group the lanes
// stride along the row (loads and stores of L consecutive floats), the row's max and sum are xor reductions over the group's L lanes,
// and the five box elements are computed by every lane of the group (the same addresses: one broadcast) and stored by its lanes 0..4
// (L >= 8 > 5).  A lane keeps its up to kGradRowRegs elements of the row in registers (C <= 16 L - 5: 123 classes at five to eight anchors),
// so the row is read once; a longer row takes three passes over memory.  Every element of every row is written, zeros included.  No LDS,
// no atomics.
__global__ void __launch_bounds__(kLossThreads) loss_grad_kernel(const LossGradParams p) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hw = p.h * p.w, width = 5 + p.n_classes;
    const int cell = blockIdx.x * kLossWaves + wave;
    if (cell >= hw) return;                                         // (wave-uniform; nothing below synchronises the workgroup)
    const int L = p.na > 4 ? 8 : p.na > 2 ? 16 : p.na > 1 ? 32 : 64;
    const int a = lane / L, sub = lane - a * L;
    const int end = a < p.na ? width : 0;                          // (an idle group walks no element; it still takes part in the shuffles)
    const float aw = p.awf[a & (YOLO_MAX_ANCHORS - 1)], ah = p.ahf[a & (YOLO_MAX_ANCHORS - 1)];
    const float lam = 1.f / (float)p.batch, lam_obj = 5.f / (float)p.batch;
    const int r = cell / p.w, c = cell - r * p.w;
    for (int b = blockIdx.y; b < p.batch; b += gridDim.y) {
        int win = p.assign[(size_t)b * hw + cell];
        if (win >= 0 && ((win >> 3) >= p.max_gt || (win & 7) >= p.na)) win = -1;      // (never in a table loss_image_kernel wrote)
        const size_t row = (((size_t)b * hw + cell) * p.na + (a < p.na ? a : 0)) * width;
        const float *__restrict__ t = p.logits + row;
        float *__restrict__ out = p.grad + row;
        float box[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        int label = 0;                                              // v2.py:155: argmax of an all-zero one-hot is 0
        if (end) {
            const float po = sigmoid_f32(t[4]);
            if (win >= 0 && (win & 7) == a) {
                const yolo_gt g = p.gt[(size_t)b * p.max_gt + (win >> 3)];
                const float gx = (float)((double)g.x * (double)p.w), gy = (float)((double)g.y * (double)p.h);
                const float gw = (float)((double)g.w * (double)p.w), gh = (float)((double)g.h * (double)p.h);
                loss_grad_winner(t, (float)c, (float)r, aw, ah, gx, gy, gw, gh, po, lam, lam_obj, box);
                label = g.class_idx;
            } else {
                box[4] = (lam * 2.f * po) * (po * (1.f - po));
            }
        }
        if (win < 0) {                                              // (wave-uniform) no class row in a cell without a winner
            for (int j = sub; j < end; j += L) out[j] = j < 5 ? (j == 4 ? box[4] : 0.f) : 0.f;
            continue;
        }
        if (sub < 5 && end) out[sub] = sub == 0 ? box[0] : sub == 1 ? box[1] : sub == 2 ? box[2] : sub == 3 ? box[3] : box[4];
        float mx = -__builtin_inff(), sum = 0.f;
        if (width <= kGradRowRegs * L) {
            // the row in registers: ONE trip to memory, every load in flight at once; exp(t - m) is computed once and kept
            float v[kGradRowRegs];
#pragma unroll
            for (int i = 0; i < kGradRowRegs; ++i) {
                const int j = sub + i * L;
                v[i] = (j >= 5 && j < end) ? t[j] : -__builtin_inff();
            }
#pragma unroll
            for (int i = 0; i < kGradRowRegs; ++i)
                if (sub + i * L >= 5 && sub + i * L < end) mx = np_maxf(mx, v[i]);
            for (int off = L >> 1; off > 0; off >>= 1) mx = np_maxf(mx, __shfl_xor(mx, off));
#pragma unroll
            for (int i = 0; i < kGradRowRegs; ++i)
                if (sub + i * L >= 5 && sub + i * L < end) { v[i] = expf(v[i] - mx); sum += v[i]; }
            for (int off = L >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);   // (a + b == b + a: every lane of the group ends with the same bits)
#pragma unroll
            for (int i = 0; i < kGradRowRegs; ++i) {
                const int j = sub + i * L;
                if (j >= 5 && j < end) out[j] = j - 5 == label ? v[i] / sum - 1.f : v[i] / sum;
            }
        } else {
            // a row longer than the registers hold (C > 16 L - 5): three passes over memory, the later ones served by the caches
            for (int j = 5 + sub; j < end; j += L) mx = np_maxf(mx, t[j]);
            for (int off = L >> 1; off > 0; off >>= 1) mx = np_maxf(mx, __shfl_xor(mx, off));
            for (int j = 5 + sub; j < end; j += L) sum += expf(t[j] - mx);
            for (int off = L >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
            for (int j = 5 + sub; j < end; j += L) {
                const float e = expf(t[j] - mx);
                out[j] = j - 5 == label ? e / sum - 1.f : e / sum;
            }
        }
    }
}

hipError_t launch_loss_images(const LossParams &p, int batch, hipStream_t s) {
    hipLaunchKernelGGL(loss_image_kernel, dim3((unsigned)batch), dim3(kLossThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_loss_finish(const LossFinishParams &p, hipStream_t s) {
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kLossThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_loss_grad(const LossGradParams &p, hipStream_t s) {
    const int chunks = (p.h * p.w + kLossWaves - 1) / kLossWaves;
    hipLaunchKernelGGL(loss_grad_kernel, dim3((unsigned)chunks, (unsigned)(p.batch < 65535 ? p.batch : 65535)), dim3(kLossThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace yolo

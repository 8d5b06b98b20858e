// YOLOv3 loss on the device: the loss of Darknet's [yolo] layer and its gradient with respect to the logits (include/yolo_hip.h:
// yolo_v3_loss, yolo_v3_loss_grad, yolo_net_loss_v3*; the definition is there).  The reference binds no loss to YoloV3 (net/yolo.py:208-211):
// nothing of it is replaced here.
//
// loss3_assign_kernel  one workgroup per image: truth checks, the best anchor over all scales and the slot of every truth; the image's part
//                      of the table is filled with -1, then the winners are written with an integer atomicMax of the truth index (the
//                      LAST truth of a slot owns it: exact, no order dependence).
// loss3_terms_kernel   grid (parts x images): the image's truths in LDS, a lane per row -- the ignore test against every truth (broadcast
//                      LDS reads), the noobj or the winner's box terms, -2 into the table; the class rows of the winner rows by the whole
//                      wave.  One yolo_loss_image record per part.
// loss3_finish_kernel  parts -> images in part order, images -> result in image order.
// loss3_grad_kernel    a streaming kernel over the gradient tensor, four consecutive elements and one 16-byte store per lane: reads the
//                      table entry of every row, t4 of a plain row, and the element's own logit on a winner row.
// Compiled with default NaN handling, like loss.hip.
#include <hip/hip_runtime.h>

#include "yolo_internal.h"
#include "head_math.h"       // sigmoid_f32, decode_v3_f32, eval_iou

namespace yolo {

constexpr int kL3Threads = 256;
constexpr int kL3Waves = kL3Threads / 64;
constexpr int kL3RowsPerThread = kLoss3RowsPerPart / kL3Threads;
constexpr int kL3FinishThreads = 1024;
constexpr int kL3GradPerThread = 4;         // quads of elements a lane of loss3_grad_kernel writes, a workgroup's pass apart
static_assert(kLoss3RowsPerPart % kL3Threads == 0, "a part is a whole number of passes of the workgroup");

// 0 for a truth that takes part, else its yolo_loss_status bits (the same function for the assignment and for the ignore test)
__device__ __forceinline__ int loss3_truth_flags(const yolo_gt &t, int n_classes) {
    int bad = 0;
    if (!(t.x >= 0.f && t.x < 1.f && t.y >= 0.f && t.y < 1.f)) bad |= YOLO_LOSS_OUT_OF_GRID;      // floor(x * w_s) outside [0, w_s) at every scale; a NaN too
    if (!(t.w > 0.f) || !(t.h > 0.f)) bad |= YOLO_LOSS_BAD_BOX;                                   // the log of the size is taken
    if (t.class_idx < 0 || t.class_idx >= n_classes) bad |= YOLO_LOSS_BAD_CLASS;
    return bad;
}

// row of an image -> scale, cell row, cell column, anchor.  Constant indices into the kernel argument only (selects, no private copy).
struct L3Slot {
    int s, r, c, a, h, w;
};
__device__ __forceinline__ L3Slot loss3_locate(const Loss3Geometry &g, int row) {
    int s = 0, row0 = 0, h = g.sc[0].h, w = g.sc[0].w, na = g.sc[0].na;
#pragma unroll
    for (int k = 1; k < YOLO_MAX_SCALES; ++k)
        if (k < g.n_scales && row >= g.sc[k].row0) { s = k; row0 = g.sc[k].row0; h = g.sc[k].h; w = g.sc[k].w; na = g.sc[k].na; }
    const int rr = row - row0, cell = rr / na;
    L3Slot o;
    o.s = s; o.a = rr - cell * na; o.r = cell / w; o.c = cell - o.r * w; o.h = h; o.w = w;
    return o;
}
__device__ __forceinline__ void loss3_anchor(const Loss3Geometry &g, int s, int a, double &aw, double &ah) {
    aw = g.sc[0].aw[0]; ah = g.sc[0].ah[0];
#pragma unroll
    for (int k = 0; k < YOLO_MAX_SCALES; ++k)
#pragma unroll
        for (int j = 0; j < YOLO_MAX_ANCHORS; ++j)
            if (k == s && j == a) { aw = g.sc[k].aw[j]; ah = g.sc[k].ah[j]; }
}

// the targets of a winner row: float64, rounded once to float32
struct L3Target {
    float tx, ty, tw, th, m;
};
__device__ __forceinline__ L3Target loss3_target(const yolo_gt &t, const L3Slot &sl, double aw, double ah) {
#pragma clang fp contract(off)
    const double x = (double)t.x, y = (double)t.y, w = (double)t.w, h = (double)t.h;
    L3Target o;
    o.tx = (float)(x * (double)sl.w - (double)sl.c);
    o.ty = (float)(y * (double)sl.h - (double)sl.r);
    o.tw = (float)log(w * (double)sl.w / aw);
    o.th = (float)log(h * (double)sl.h / ah);
    o.m = (float)(2. - w * h);
    return o;
}

// expf and log1pf CORRECTLY rounded: computed in float64 and rounded once, so that a term does not depend on which float32 library
// evaluates it (two libraries' expf differ by an ulp now and then, and m * (sp(t0) - tx * t0 ...) amplifies that)
__device__ __forceinline__ float loss3_expf(float x) { return (float)exp((double)x); }
// softplus, float32, every operation rounded on its own
__device__ __forceinline__ float loss3_sp(float t) {
#pragma clang fp contract(off)
    const float e = loss3_expf(-fabsf(t));
    const float l = (float)log1p((double)e);
    return fmaxf(t, 0.f) + l;
}
// the sigmoid of the gradient, 1 / (1 + expf(-t)) with that expf
__device__ __forceinline__ float loss3_sigmoid(float t) {
#pragma clang fp contract(off)
    return 1.f / (1.f + loss3_expf(-t));
}

// ---- assignment ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kL3Threads) loss3_assign_kernel(const Loss3Params p) {
    __shared__ int s_status, s_truths;
    __shared__ double s_aw[YOLO_MAX_SCALES][YOLO_MAX_ANCHORS], s_ah[YOLO_MAX_SCALES][YOLO_MAX_ANCHORS];
    __shared__ int s_row0[YOLO_MAX_SCALES], s_h[YOLO_MAX_SCALES], s_w[YOLO_MAX_SCALES], s_na[YOLO_MAX_SCALES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int R = p.geo.rows;
    int *table = p.assign + (size_t)b * (size_t)R;
    if (tid == 0) { s_status = 0; s_truths = 0; }
#pragma unroll
    for (int s = 0; s < YOLO_MAX_SCALES; ++s) {         // the geometry into LDS with constant indices, so that a truth's loop can index it
        if (tid == 64 + s) { s_row0[s] = p.geo.sc[s].row0; s_h[s] = p.geo.sc[s].h; s_w[s] = p.geo.sc[s].w; s_na[s] = p.geo.sc[s].na; }
#pragma unroll
        for (int a = 0; a < YOLO_MAX_ANCHORS; ++a)
            if (tid == s * YOLO_MAX_ANCHORS + a) { s_aw[s][a] = p.geo.sc[s].aw[a]; s_ah[s][a] = p.geo.sc[s].ah[a]; }
    }
    for (int r = tid; r < R; r += kL3Threads) table[r] = -1;
    __syncthreads();            // (orders the fill in front of the atomics of this workgroup, the only one that touches this image)
    int flags = 0;
    int ng = p.gt_counts[b];
    if (ng < 0 || ng > p.max_gt) { flags |= YOLO_LOSS_BAD_COUNT; ng = ng < 0 ? 0 : p.max_gt; }
    const yolo_gt *gt = p.gt + (size_t)b * (size_t)p.max_gt;
    for (int g = tid; g < ng; g += kL3Threads) {
        const yolo_gt t = gt[g];
        const int bad = loss3_truth_flags(t, p.geo.n_classes);
        flags |= bad;
        if (bad) continue;
        double best = -1.;
        int bs = 0, ba = 0;
        for (int s = 0; s < p.geo.n_scales; ++s) {
            const double bw = (double)t.w * (double)s_w[s], bh = (double)t.h * (double)s_h[s];
            for (int a = 0; a < s_na[s]; ++a) {
                const double iou = eval_iou(0., 0., bw, bh, 0., 0., s_aw[s][a], s_ah[s][a]);
                if (best < iou) { best = iou; bs = s; ba = a; }         // strict: the first anchor to reach the largest value; a NaN never wins
            }
        }
        const int row0 = s_row0[bs], h = s_h[bs], w = s_w[bs], na = s_na[bs];
        int cx = (int)floor((double)t.x * (double)w), cy = (int)floor((double)t.y * (double)h);
        cx = cx < 0 ? 0 : cx > w - 1 ? w - 1 : cx;                      // (already inside: x in [0, 1) and the product is exact)
        cy = cy < 0 ? 0 : cy > h - 1 ? h - 1 : cy;
        atomicMax(&table[row0 + (cy * w + cx) * na + ba], g);           // the LAST truth in list order owns the slot
        atomicAdd(&s_truths, 1);
    }
    if (flags) atomicOr(&s_status, flags);
    __syncthreads();
    if (tid == 0) {             // the rest of the record: loss3_finish_kernel
        p.images[b].n_truths = s_truths;
        p.images[b].status = s_status;
    }
}

// ---- terms --------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kL3Threads) loss3_terms_kernel(const Loss3Params p) {
    __shared__ float4 s_gt[YOLO_EVAL_MAX_GT];               // (x, y, w, h); w < 0: a skipped truth
    __shared__ float s_awf[YOLO_MAX_SCALES][YOLO_MAX_ANCHORS], s_ahf[YOLO_MAX_SCALES][YOLO_MAX_ANCHORS];
    __shared__ double ws[kL3Waves][5];
    __shared__ int ws_n[kL3Waves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = p.geo.rows, C = p.geo.n_classes, width = 5 + C, part = blockIdx.x;
#pragma unroll
    for (int s = 0; s < YOLO_MAX_SCALES; ++s)
#pragma unroll
        for (int a = 0; a < YOLO_MAX_ANCHORS; ++a)
            if (tid == s * YOLO_MAX_ANCHORS + a) { s_awf[s][a] = p.geo.sc[s].awf[a]; s_ahf[s][a] = p.geo.sc[s].ahf[a]; }
    for (int b = blockIdx.y; b < p.batch; b += gridDim.y) {
        __syncthreads();        // the previous image's reads of s_gt and ws are done
        int ng = p.gt_counts[b];
        ng = ng < 0 ? 0 : ng > p.max_gt ? p.max_gt : ng;
        const yolo_gt *gt = p.gt + (size_t)b * (size_t)p.max_gt;
        for (int g = tid; g < ng; g += kL3Threads) {
            const yolo_gt t = gt[g];
            s_gt[g] = make_float4(t.x, t.y, loss3_truth_flags(t, C) ? -1.f : t.w, t.h);
        }
        __syncthreads();
        const float *logits = p.logits + (size_t)b * (size_t)R * (size_t)width;
        int *table = p.assign + (size_t)b * (size_t)R;
        double acc_xy = 0., acc_wh = 0., acc_obj = 0., acc_noobj = 0., acc_cls = 0.;
        int n_assigned = 0;
        for (int i = 0; i < kL3RowsPerThread; ++i) {
            const int r = part * kLoss3RowsPerPart + i * kL3Threads + tid;
            const bool live = r < R;
            int entry = -1, cls = 0;
            if (live) {
                const float *t = logits + (size_t)r * (size_t)width;
                entry = table[r];
                if (entry >= ng) entry = -1;                            // (never in a table loss3_assign_kernel wrote)
                const float t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4];
                const L3Slot sl = loss3_locate(p.geo, r);
                if (entry >= 0) {
#pragma clang fp contract(off)
                    const yolo_gt g = gt[entry];
                    double aw, ah;
                    loss3_anchor(p.geo, sl.s, sl.a, aw, ah);
                    const L3Target tg = loss3_target(g, sl, aw, ah);
                    const float xy = tg.m * (loss3_sp(t0) - tg.tx * t0 + loss3_sp(t1) - tg.ty * t1);
                    const float dw = t2 - tg.tw, dh = t3 - tg.th;
                    const float wh = tg.m * 0.5f * (dw * dw + dh * dh);
                    const float obj = loss3_sp(t4) - t4;
                    acc_xy += (double)xy; acc_wh += (double)wh; acc_obj += (double)obj;
                    cls = g.class_idx;
                    ++n_assigned;
                } else {
                    float bx, by, bw, bh;
                    decode_v3_f32(t0, t1, t2, t3, (float)sl.c, (float)sl.r, (float)sl.w, (float)sl.h, s_awf[sl.s][sl.a], s_ahf[sl.s][sl.a], bx, by, bw,
                                  bh);
                    const double dx = (double)bx, dy = (double)by, dw = (double)bw, dh = (double)bh;
                    double best = -1.;
                    for (int g = 0; g < ng; ++g) {
                        const float4 q = s_gt[g];                       // (the same address on every lane: a broadcast)
                        if (q.z < 0.f) continue;
                        const double iou = eval_iou(dx, dy, dw, dh, (double)q.x, (double)q.y, (double)q.z, (double)q.w);
                        if (iou > best) best = iou;                     // (a NaN compares false)
                    }
                    if (best > p.ignore_thresh) table[r] = -2;          // strict; no term at all
                    else acc_noobj += (double)loss3_sp(t4);
                }
            }
            // the class rows of this pass's winner rows, by the whole wave (wave-uniform control flow)
            unsigned long long todo = __ballot(live && entry >= 0);
            while (todo) {
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int rr = __shfl(r, l), label = __shfl(cls, l);
                const float *tc = logits + (size_t)rr * (size_t)width + 5;
                double part_sum = 0.;
                for (int k = lane; k < C; k += 64) {
#pragma clang fp contract(off)
                    const float v = tc[k];
                    const float sp = loss3_sp(v);
                    part_sum += (double)(k == label ? sp - v : sp);
                }
                for (int off = 32; off > 0; off >>= 1) part_sum += __shfl_xor(part_sum, off);      // (a + b == b + a: the same bits on every lane)
                acc_cls += part_sum;
            }
        }
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
            for (int w = 0; w < kL3Waves; ++w) {
                for (int k = 0; k < 5; ++k) s[k] += ws[w][k];
                n += ws_n[w];
            }
            out.xy = s[0]; out.wh = s[1]; out.obj = s[2]; out.noobj = s[3]; out.cls = s[4];
            out.n_assigned = n; out.n_truths = 0; out.status = 0; out.pad_ = 0;
            p.parts[(size_t)b * (size_t)p.geo.parts + (size_t)part] = out;
        }
    }
}

// ---- finish -------------------------------------------------------------------------------------------------------------------------------
// One workgroup.  Phase 1: a wave per image -- its lanes load the image's part records 64 at a time, every lane adds them in part order
// (shuffles), lane 0 completes the record loss3_assign_kernel began (n_truths, status).  Phase 2: as loss_finish_kernel, the records come
// into LDS 256 at a time and one thread adds them in image order.
__global__ void __launch_bounds__(kL3FinishThreads) loss3_finish_kernel(const Loss3Params p) {
    __shared__ yolo_loss_image rec[kL3Threads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = p.geo.parts;
    for (int b = wave; b < p.batch; b += kL3FinishThreads / 64) {
        const yolo_loss_image *parts = p.parts + (size_t)b * (size_t)P;
        double s[5] = {0., 0., 0., 0., 0.};
        int n = 0;
        for (int base = 0; base < P; base += 64) {
            double v[5] = {0., 0., 0., 0., 0.};
            int vn = 0;
            if (base + lane < P) {
                const yolo_loss_image q = parts[base + lane];
                v[0] = q.xy; v[1] = q.wh; v[2] = q.obj; v[3] = q.noobj; v[4] = q.cls; vn = q.n_assigned;
            }
            const int m = P - base < 64 ? P - base : 64;
            for (int q = 0; q < m; ++q) {
#pragma unroll
                for (int k = 0; k < 5; ++k) s[k] += __shfl(v[k], q);
                n += __shfl(vn, q);
            }
        }
        if (lane == 0) {
            yolo_loss_image out;
            out.xy = s[0]; out.wh = s[1]; out.obj = s[2]; out.noobj = s[3]; out.cls = s[4];
            out.n_assigned = n; out.n_truths = p.images[b].n_truths; out.status = p.images[b].status; out.pad_ = 0;
            p.images[b] = out;
        }
    }
    __threadfence_block();
    double s[5] = {0., 0., 0., 0., 0.};
    int n_assigned = 0, n_truths = 0, status = 0;
    for (int base = 0; base < p.batch; base += kL3Threads) {
        __syncthreads();
        if (tid < kL3Threads && base + tid < p.batch) rec[tid] = p.images[base + tid];
        __syncthreads();
        if (tid == 0) {
            const int m = p.batch - base < kL3Threads ? p.batch - base : kL3Threads;
            for (int i = 0; i < m; ++i) {
                s[0] += rec[i].xy; s[1] += rec[i].wh; s[2] += rec[i].obj; s[3] += rec[i].noobj; s[4] += rec[i].cls;
                n_assigned += rec[i].n_assigned; n_truths += rec[i].n_truths; status |= rec[i].status;
            }
        }
    }
    if (tid == 0) {
        const double B = (double)p.batch;
        yolo_loss_result r;
        r.loss_xy = s[0] / B; r.loss_wh = s[1] / B; r.loss_obj = s[2] / B; r.loss_noobj = s[3] / B; r.loss_class = s[4] / B;
        r.loss = r.loss_xy + r.loss_wh + r.loss_obj + r.loss_noobj + r.loss_class;
        r.n_assigned = n_assigned; r.n_truths = n_truths; r.status = status; r.pad_ = 0;
        *p.result = r;
    }
}

// ---- gradient -----------------------------------------------------------------------------------------------------------------------------
// One element of G: the table entry of its row says everything.  -2 -> +0; -1 -> sigmoid(t4) / B at element 4 and +0 elsewhere; a truth
// index -> the element's own logit and, for the four box elements, the truth's targets.
__device__ __forceinline__ float loss3_grad_element(const Loss3Params &p, int entry, size_t grow, int j, size_t flat, float Bf) {
#pragma clang fp contract(off)
    if (entry < 0) return (entry == -1 && j == 4) ? loss3_sigmoid(p.logits[flat]) / Bf : 0.f;
    const float t = p.logits[flat];
    const size_t b = grow / (size_t)p.geo.rows;
    const yolo_gt g = p.gt[b * (size_t)p.max_gt + (size_t)entry];
    if (j == 4) return (loss3_sigmoid(t) - 1.f) / Bf;
    if (j > 4) return (loss3_sigmoid(t) - (j - 5 == g.class_idx ? 1.f : 0.f)) / Bf;
    const L3Slot sl = loss3_locate(p.geo, (int)(grow - b * (size_t)p.geo.rows));
    double aw, ah;
    loss3_anchor(p.geo, sl.s, sl.a, aw, ah);
    const L3Target tg = loss3_target(g, sl, aw, ah);
    const float d = j == 0 ? loss3_sigmoid(t) - tg.tx : j == 1 ? loss3_sigmoid(t) - tg.ty : j == 2 ? t - tg.tw : t - tg.th;
    return tg.m * d / Bf;
}

// A streaming kernel over G as ONE flat array of B * R * (5 + C) floats: a lane owns four consecutive elements and writes them with one
// 16-byte store (VEC: grad_dev is 16-byte aligned; otherwise four 4-byte stores), consecutive lanes consecutive quads, so a wave's store is
// 1 KiB contiguous.  One 64-bit division per lane finds its first row; after that rows and elements advance by carries.  The table entry
// is read once per row a quad touches.  Zeros are written, never skipped.  No LDS, no atomics.
template <bool VEC>
__global__ void __launch_bounds__(kL3Threads) loss3_grad_kernel(const Loss3Params p) {
    const int width = 5 + p.geo.n_classes;
    const size_t total = (size_t)p.batch * (size_t)p.geo.rows * (size_t)width;
    const float Bf = (float)p.batch;
    constexpr int kStep = kL3Threads * 4;                               // elements one pass of the workgroup covers
    size_t flat = (size_t)blockIdx.x * (size_t)(kStep * kL3GradPerThread) + (size_t)threadIdx.x * 4;
    if (flat >= total) return;
    size_t grow = flat / (size_t)width;                                 // row over all images: the table's index
    int j = (int)(flat - grow * (size_t)width);
    const int step_rows = kStep / width, step_j = kStep - step_rows * width;
#pragma unroll
    for (int k = 0; k < kL3GradPerThread; ++k) {
        if (flat >= total) break;
        int entry = p.assign[grow];
        if (entry >= p.max_gt) entry = -1;                              // (never in a table loss3_assign_kernel wrote)
        float v[4];
        size_t r = grow;
        int jj = j;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (flat + q < total) v[q] = loss3_grad_element(p, entry, r, jj, flat + q, Bf);
            else v[q] = 0.f;
            if (++jj == width) {                                        // the next element opens a row
                jj = 0;
                ++r;
                if (q < 3 && flat + q + 1 < total) {
                    entry = p.assign[r];
                    if (entry >= p.max_gt) entry = -1;
                }
            }
        }
        if (VEC && flat + 4 <= total) {
            *reinterpret_cast<float4 *>(p.grad + flat) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (flat + q < total) p.grad[flat + q] = v[q];
        }
        flat += kStep;
        grow += step_rows;
        j += step_j;
        if (j >= width) { j -= width; ++grow; }
    }
}

hipError_t launch_loss3(const Loss3Params &p, hipStream_t s) {
    const unsigned by = (unsigned)(p.batch < 65535 ? p.batch : 65535);
    hipLaunchKernelGGL(loss3_assign_kernel, dim3((unsigned)p.batch), dim3(kL3Threads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(loss3_terms_kernel, dim3((unsigned)p.geo.parts, by), dim3(kL3Threads), 0, s, p);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(loss3_finish_kernel, dim3(1), dim3(kL3FinishThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_loss3_grad(const Loss3Params &p, hipStream_t s) {
    const size_t per = (size_t)kL3Threads * 4 * kL3GradPerThread;
    const size_t total = (size_t)p.batch * (size_t)p.geo.rows * (size_t)(5 + p.geo.n_classes);
    const size_t blocks = (total + per - 1) / per;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(p.grad) % 16 == 0) hipLaunchKernelGGL(loss3_grad_kernel<true>, dim3((unsigned)blocks), dim3(kL3Threads), 0, s, p);
    else hipLaunchKernelGGL(loss3_grad_kernel<false>, dim3((unsigned)blocks), dim3(kL3Threads), 0, s, p);
    return hipGetLastError();
}

}  // namespace yolo

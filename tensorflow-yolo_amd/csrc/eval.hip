// VOC-style evaluation on the device (include/yolo_hip.h: yolo_eval_*): matching of a step's detections against its truths
// (eval_match_kernel, the per-step hot path) and, once per dataset, sort + TP/FP scans + average precision (launch_eval_finish).
// Compiled with default NaN handling, like detect.hip: the IoU follows NumPy on NaN and infinity.
#include <hip/hip_runtime.h>

#include "yolo_internal.h"
#include "head_math.h"       // np_max, np_min, eval_iou

namespace yolo {

EvalLayout eval_layout(int n_classes, int det_capacity) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    EvalLayout L;
    int n2 = kEvalSortTile;
    while (n2 < det_capacity) n2 <<= 1;
    L.n2 = n2;
    const size_t cap = (size_t)det_capacity;
    L.header = 0;
    L.n_gt = up(sizeof(EvalHeader));
    L.records = L.n_gt + up(sizeof(int) * (size_t)n_classes);
    L.sorted = L.records + up(sizeof(yolo_eval_record) * cap);
    L.ctp = L.sorted + up(sizeof(yolo_eval_record) * cap);
    L.cfp = L.ctp + up(sizeof(unsigned) * cap);
    L.entries = L.cfp + up(sizeof(unsigned) * cap);
    L.total = L.entries + up(sizeof(EvalEntry) * (size_t)n2);
    return L;
}

__device__ __forceinline__ unsigned eval_orderable(float f) {   // monotone float -> uint (detect.hip: orderable)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup per image.  The truths live in LDS; the list is walked in chunks of 256 ranks, in rank order:
//   phase 1  a thread per detection scans the truths of its class for (best_iou, best_gt)
//   phase 2  atomicMin of the claiming rank into the truth's LDS word (non-difficult truths only), barrier, verdict: TP for the
//            lowest rank.  Later chunks hold higher ranks only, so a claim settled in one chunk is never undone by the next.
//   phase 3  the records go to the state behind ONE cursor bump per wave; the non-difficult truths are counted into n_gt[class].
constexpr int kEvalThreads = 256;
__global__ void __launch_bounds__(kEvalThreads) eval_match_kernel(const EvalMatchParams p) {
    __shared__ float gx[YOLO_EVAL_MAX_GT], gy[YOLO_EVAL_MAX_GT], gw[YOLO_EVAL_MAX_GT], gh[YOLO_EVAL_MAX_GT];
    __shared__ int gcls[YOLO_EVAL_MAX_GT];
    __shared__ unsigned char gdiff[YOLO_EVAL_MAX_GT];
    __shared__ unsigned claim[YOLO_EVAL_MAX_GT];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    unsigned flags = 0;
    int ng = p.gt_counts[b];
    if (ng < 0 || ng > p.max_gt) { flags |= YOLO_EVAL_BAD_COUNT; ng = ng < 0 ? 0 : p.max_gt; }
    int n = p.counts[b];
    if (n < 0 || n > p.max_boxes) { flags |= YOLO_EVAL_BAD_COUNT; n = n < 0 ? 0 : p.max_boxes; }
    const yolo_gt *gt = p.gt + (size_t)b * p.max_gt;
    for (int g = tid; g < ng; g += kEvalThreads) {
        const yolo_gt t = gt[g];
        int c = t.class_idx;
        if (c < 0 || c >= p.n_classes) { flags |= YOLO_EVAL_BAD_CLASS; c = -1; }       // never equals a detection's class
        else if (!t.difficult) atomicAdd(&p.n_gt[c], 1);
        gx[g] = t.x; gy[g] = t.y; gw[g] = t.w; gh[g] = t.h;
        gcls[g] = c;
        gdiff[g] = t.difficult ? 1 : 0;
        claim[g] = 0xffffffffu;
    }
    __syncthreads();
    const yolo_box *boxes = p.boxes + (size_t)b * p.max_boxes;
    const unsigned seq0 = p.seq_base + (unsigned)b * (unsigned)p.max_boxes;
    for (int r0 = 0; r0 < n; r0 += kEvalThreads) {          // (block-uniform: every thread meets the barrier)
        const int r = r0 + tid;
        bool valid = r < n;
        yolo_box d = {0.f, 0.f, 0.f, 0.f, 0.f, -1};
        if (valid) {
            d = boxes[r];
            if (r > 0 && boxes[r - 1].prob < d.prob) flags |= YOLO_EVAL_UNSORTED;
            if (d.class_idx < 0 || d.class_idx >= p.n_classes) { flags |= YOLO_EVAL_BAD_CLASS; valid = false; }
        }
        double best = -1.;
        int bg = -1;
        if (valid) {
            const double x1 = d.x, y1 = d.y, w1 = d.w, h1 = d.h;
            for (int g = 0; g < ng; ++g) {
                if (gcls[g] != d.class_idx) continue;
                const double iou = eval_iou(x1, y1, w1, h1, (double)gx[g], (double)gy[g], (double)gw[g], (double)gh[g]);
                if (iou > best) { best = iou; bg = g; }     // strict: the lowest index keeps a tie, a NaN never wins
            }
        }
        const bool claims = bg >= 0 && best > p.match_iou;  // strict, as VOCdevkit and Darknet (NMS suppresses at >=)
        if (claims && !gdiff[bg]) atomicMin(&claim[bg], (unsigned)r);
        __syncthreads();
        int verdict = YOLO_EVAL_FP;
        if (claims) verdict = gdiff[bg] ? YOLO_EVAL_IGNORED : (claim[bg] == (unsigned)r ? YOLO_EVAL_TP : YOLO_EVAL_FP);
        if (bg < 0) best = 0.;
        // wave-aggregated append: arrival order is free, seq orders the records later
        const unsigned long long mask = __ballot(valid);
        if (mask) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(&p.hdr->cursor, (unsigned long long)__popcll(mask));
            base = __shfl(base, 0);
            if (valid) {
                const unsigned long long pos = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
                if (pos < (unsigned long long)p.det_capacity) {
                    yolo_eval_record rec;
                    rec.best_iou = best; rec.prob = d.prob; rec.class_idx = d.class_idx; rec.seq = seq0 + (unsigned)r;
                    rec.verdict = verdict; rec.best_gt = bg; rec.pad_ = 0;
                    p.records[pos] = rec;
                } else {
                    flags |= YOLO_EVAL_OVERFLOW;            // nothing is written behind the capacity
                }
            }
        }
    }
    if (flags) atomicOr(&p.hdr->status, flags);
}

hipError_t launch_eval_match(const EvalMatchParams &p, int batch, hipStream_t s) {
    hipLaunchKernelGGL(eval_match_kernel, dim3(batch), dim3(kEvalThreads), 0, s, p);
    return hipGetLastError();
}

// ---- finish: sort ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool entry_less(const EvalEntry &a, const EvalEntry &b) {
    if (a.hi != b.hi) return a.hi < b.hi;
    if (a.lo != b.lo) return a.lo < b.lo;
    return a.idx < b.idx;
}

__device__ __forceinline__ int eval_count(const EvalHeader *hdr, int cap) {
    const unsigned long long c = hdr->cursor;
    return c > (unsigned long long)cap ? cap : (int)c;
}

__global__ void __launch_bounds__(256) eval_keys_kernel(const EvalFinishParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n2) return;
    const int n = eval_count(p.hdr, p.det_capacity);
    EvalEntry e{~0ull, 0xffffffffu, 0xffffffffu};
    if (i < n) {
        const yolo_eval_record r = p.records[i];
        e.lo = ((unsigned long long)(~eval_orderable(r.prob)) << 32) | r.seq;
        e.hi = (unsigned)r.class_idx;
        e.idx = (unsigned)i;
    }
    p.entries[i] = e;
}

// Bitonic network on n2 entries (a power of two >= kEvalSortTile).  All steps with a partner distance below kEvalSortTile run in LDS,
// one tile per workgroup: FULL = every stage k <= kEvalSortTile from scratch; else the tail (j = kEvalSortTile / 2 .. 1) of stage k.
template <bool FULL>
__global__ void __launch_bounds__(kEvalSortTile / 2) eval_sort_tile_kernel(EvalEntry *entries, int k_stage) {
    __shared__ EvalEntry e[kEvalSortTile];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kEvalSortTile;
    e[t] = entries[base + t];
    e[t + kEvalSortTile / 2] = entries[base + t + kEvalSortTile / 2];
    __syncthreads();
    for (int k = FULL ? 2 : k_stage; k <= (FULL ? kEvalSortTile : k_stage); k <<= 1) {
        for (int j = (FULL ? k : kEvalSortTile) >> 1; j > 0; j >>= 1) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
            const int l = i | j;
            const bool asc = ((base + (size_t)i) & (size_t)k) == 0;
            const EvalEntry a = e[i], c = e[l];
            if (asc ? entry_less(c, a) : entry_less(a, c)) { e[i] = c; e[l] = a; }
            __syncthreads();
        }
    }
    entries[base + t] = e[t];
    entries[base + t + kEvalSortTile / 2] = e[t + kEvalSortTile / 2];
}

__global__ void __launch_bounds__(256) eval_sort_step_kernel(EvalEntry *entries, int n2, int k, int j) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n2 / 2) return;
    const size_t i = ((t & ~((size_t)j - 1)) << 1) | (t & ((size_t)j - 1));
    const size_t l = i | (size_t)j;
    const bool asc = (i & (size_t)k) == 0;
    const EvalEntry a = entries[i], c = entries[l];
    if (asc ? entry_less(c, a) : entry_less(a, c)) { entries[i] = c; entries[l] = a; }
}

__global__ void __launch_bounds__(256) eval_gather_kernel(const EvalFinishParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = eval_count(p.hdr, p.det_capacity);
    if (i >= n) return;
    p.sorted[i] = p.records[p.entries[i].idx];      // (idx < n: the padding entries sort behind every record)
}

// ---- finish: per-class scans and AP ----------------------------------------------------------------------------------------------
constexpr int kEvalClassThreads = 1024;
constexpr int kEvalClassWaves = kEvalClassThreads / 64;

// inclusive scans over the workgroup in thread order; `total` is the workgroup's sum / maximum.  ws: kEvalClassWaves words of LDS.
__device__ __forceinline__ unsigned long long block_scan_add(unsigned long long v, unsigned long long *ws, unsigned long long &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    if (lane == 63) ws[wave] = v;
    __syncthreads();
    unsigned long long off = 0, sum = 0;
    for (int w = 0; w < kEvalClassWaves; ++w) {
        const unsigned long long x = ws[w];
        if (w < wave) off += x;
        sum += x;
    }
    __syncthreads();
    total = sum;
    return v + off;
}
__device__ __forceinline__ double block_scan_max(double v, double *ws, double &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d);
        if (lane >= d) v = o > v ? o : v;
    }
    if (lane == 63) ws[wave] = v;
    __syncthreads();
    double off = 0., mx = 0.;                       // (precisions are >= 0)
    for (int w = 0; w < kEvalClassWaves; ++w) {
        const double x = ws[w];
        if (w < wave) off = x > off ? x : off;
        mx = x > mx ? x : mx;
    }
    __syncthreads();
    total = mx;
    return off > v ? off : v;
}

__device__ __forceinline__ int entries_lower_bound(const EvalEntry *e, int n, unsigned cls) {   // first position with hi >= cls
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid].hi < cls) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per class: its segment of the sorted records -> ctp / cfp (forward, exact integers), then backwards the monotone
// precision envelope, the voc12 sum over the TPs and the eleven voc07 points.
__global__ void __launch_bounds__(kEvalClassThreads) eval_class_kernel(const EvalFinishParams p) {
    __shared__ unsigned long long ws_u[kEvalClassWaves];
    __shared__ double ws_d[kEvalClassWaves];
    __shared__ double p07[11];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int n = eval_count(p.hdr, p.det_capacity);
    const int start = entries_lower_bound(p.entries, n, (unsigned)c);
    const int end = entries_lower_bound(p.entries, n, (unsigned)c + 1u);
    const int ngt = p.n_gt[c];
    if (tid < 11) p07[tid] = 0.;
    // forward: tp in the high word, fp in the low word of one 64-bit scan
    unsigned long long carry = 0;
    for (int k0 = start; k0 < end; k0 += kEvalClassThreads) {
        const int k = k0 + tid;
        unsigned long long v = 0;
        if (k < end) {
            const int verdict = p.sorted[k].verdict;
            v = verdict == YOLO_EVAL_TP ? (1ull << 32) : verdict == YOLO_EVAL_FP ? 1ull : 0ull;
        }
        unsigned long long total;
        const unsigned long long s = block_scan_add(v, ws_u, total) + carry;
        if (k < end) { p.ctp[k] = (unsigned)(s >> 32); p.cfp[k] = (unsigned)s; }
        carry += total;
    }
    const int tp = (int)(carry >> 32), fp = (int)(unsigned)carry;
    __syncthreads();            // ctp / cfp of the segment are visible to the whole workgroup; p07 is cleared
    double acc = 0.;
    if (ngt > 0) {
        const double dn = (double)ngt;
        double env_carry = 0.;
        for (int k1 = end; k1 > start; k1 -= kEvalClassThreads) {       // thread t takes record k1 - 1 - t: a prefix scan from the end
            const int k = k1 - 1 - tid;
            const bool in = k >= start;
            double prec = 0.;
            unsigned t_k = 0;
            int verdict = YOLO_EVAL_IGNORED;
            if (in) {
                t_k = p.ctp[k];
                const double den = (double)(t_k + p.cfp[k]);
                prec = (double)t_k / (den > 0x1p-52 ? den : 0x1p-52);    // VOCdevkit: np.maximum(tp + fp, np.finfo(np.float64).eps)
                verdict = p.sorted[k].verdict;
            }
            double total;
            double env = block_scan_max(prec, ws_d, total);
            env = env_carry > env ? env_carry : env;
            env_carry = total > env_carry ? total : env_carry;
            if (in && (verdict == YOLO_EVAL_TP || k == start)) {
                if (verdict == YOLO_EVAL_TP) acc += env / dn;
                const double rec = (double)t_k / dn;
                const double rec_prev = verdict == YOLO_EVAL_TP ? (double)(t_k - 1) / dn : rec;
                for (int i = 0; i < 11; ++i) {
                    const double thr = (double)i / 10.0;
                    if (rec >= thr && (k == start || rec_prev < thr)) p07[i] = env;     // the first record with recall >= thr: one writer
                }
            }
        }
    }
    // voc12: sum of the per-thread partial sums in a fixed order
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d);
    __syncthreads();
    if ((tid & 63) == 0) ws_d[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        yolo_eval_class out;
        double ap12 = 0., ap07 = 0.;
        for (int w = 0; w < kEvalClassWaves; ++w) ap12 += ws_d[w];
        for (int i = 0; i < 11; ++i) ap07 = ap07 + p07[i] / 11.;
        if (ngt <= 0) ap12 = ap07 = __builtin_nan("");
        out.ap_voc12 = ap12; out.ap_voc07 = ap07;
        out.n_gt = ngt; out.n_det = end - start; out.tp = tp; out.fp = fp; out.ignored = end - start - tp - fp; out.pad_ = 0;
        reinterpret_cast<yolo_eval_class *>(p.result + 1)[c] = out;
    }
}

// One thread sums the classes in index order: the order is then fixed, and the cost is one dependent load + add per class -- some
// 10 us at 80 classes, under a millisecond at YOLO_EVAL_MAX_CLASSES, once per dataset behind a sort that takes longer.
__global__ void eval_map_kernel(const EvalFinishParams p) {
    if (threadIdx.x || blockIdx.x) return;
    const yolo_eval_class *cls = reinterpret_cast<const yolo_eval_class *>(p.result + 1);
    double s12 = 0., s07 = 0.;
    int m = 0;
    for (int c = 0; c < p.n_classes; ++c)
        if (cls[c].n_gt > 0) { s12 += cls[c].ap_voc12; s07 += cls[c].ap_voc07; ++m; }
    yolo_eval_result r;
    r.map_voc12 = m ? s12 / (double)m : __builtin_nan("");
    r.map_voc07 = m ? s07 / (double)m : __builtin_nan("");
    r.n_records = eval_count(p.hdr, p.det_capacity);
    r.status = (int)p.hdr->status;
    r.n_classes = p.n_classes; r.pad_ = 0;
    *p.result = r;
}

// The record count lives on the device (the cursor) and nothing here waits for it: the grids are sized by the capacity, and with 0
// records the kernels still run -- the keys are all padding, gather returns at once, each class finds an empty segment.
hipError_t launch_eval_finish(const EvalFinishParams &p, hipStream_t s) {
    const int n2 = p.n2;
    hipLaunchKernelGGL(eval_keys_kernel, dim3((n2 + 255) / 256), dim3(256), 0, s, p);
    hipLaunchKernelGGL(eval_sort_tile_kernel<true>, dim3(n2 / kEvalSortTile), dim3(kEvalSortTile / 2), 0, s, p.entries, 0);
    for (int k = 2 * kEvalSortTile; k <= n2; k <<= 1) {
        for (int j = k >> 1; j >= kEvalSortTile; j >>= 1)
            hipLaunchKernelGGL(eval_sort_step_kernel, dim3((n2 / 2 + 255) / 256), dim3(256), 0, s, p.entries, n2, k, j);
        hipLaunchKernelGGL(eval_sort_tile_kernel<false>, dim3(n2 / kEvalSortTile), dim3(kEvalSortTile / 2), 0, s, p.entries, k);
    }
    hipLaunchKernelGGL(eval_gather_kernel, dim3((p.det_capacity + 255) / 256), dim3(256), 0, s, p);
    hipLaunchKernelGGL(eval_class_kernel, dim3(p.n_classes), dim3(kEvalClassThreads), 0, s, p);
    hipLaunchKernelGGL(eval_map_kernel, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace yolo

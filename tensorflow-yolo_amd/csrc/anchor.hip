// Anchor k-means (include/yolo_hip.h "Anchor k-means on the device"): a small iterative solver in integers and float64.
//
//   prepare   one workgroup per chunk of kAnchorChunk boxes: validate, quantise to q = rint(v * 2^40), write (q_w, q_h) or (0, 0), and add the
//             counts and the split sums of the variance (AnchorPrep) -- LDS integer atomics, then one 64-bit global atomic per word
//   init      one workgroup per restart: clears the restart's record; with given centres copies and checks them
//   seed_sum  grid (chunks x restarts), round j: D_i of every box of the chunk against the j seeds so far (held in LDS) and the chunk's sum
//   seed_pick one workgroup per restart: sums and scans the chunk sums, draws t, finds the chunk, recomputes its D_i, finds the box
//   assign    grid (chunks x restarts): the k centres in LDS, every lane takes kAnchorChunk / kAnchorBlock boxes, the per-cluster
//             (S q_w, S q_h, count) and the changed count go into LDS by integer atomics and from there into the restart's record by 64-bit
//             global atomics (integer sums: no order can change them).  A restart whose done flag is set leaves at once.
//   update    the tiny second kernel of an iteration, one workgroup per restart, one thread: new centres, the shift, the stop decision
//   final     assign once more against the final centres: labels, counts, sums, S qd, S floor(best IoU * 2^40)
//   finish    best restart, the order by area, every field of the result
//   labels    the caller's int32 labels, renumbered
// No floating-point atomics, no waiting on another workgroup.  Every index is below n or below the part's size by construction: a thread's
// box index is checked against n, a cluster index against k <= 32, a chunk index against n_chunks.
#include "yolo_internal.h"
#include "philox.h"

namespace yolo {

namespace {

constexpr int CH = kAnchorChunk, BL = kAnchorBlock, PER = CH / BL, MAXK = YOLO_ANCHOR_MAX_K;
static_assert(CH % BL == 0 && BL == 256, "whole boxes per thread; the scans below walk 256 partial sums");
typedef unsigned long long u64;

__device__ __forceinline__ u64 quantise(double v) {
    if (!(v > 0.0) || !(v <= 1.0)) return 0ull;         // NaN, infinities, zero, negative, above 1
    return (u64)rint(v * 0x1p40);                       // exact product, ties to even; 0 below 2^-41
}

__device__ __forceinline__ double unit(u64 q) { return (double)q * 0x1p-40; }      // exact: q <= 2^40

// i / (w * h + cw * ch - i), every operation rounded on its own; at most 1 (see DESIGN.md "Anchor k-means")
__device__ __forceinline__ double anchor_iou(double w, double h, double cw, double ch) {
#pragma clang fp contract(off)
    const double i = (w < cw ? w : cw) * (h < ch ? h : ch);
    const double a = w * h, b = cw * ch;
    const double s = a + b;
    return i / (s - i);
}

__device__ __forceinline__ double anchor_dist(int distance, double w, double h, double cw, double ch) {
#pragma clang fp contract(off)
    if (distance == YOLO_ANCHOR_IOU) return 1.0 - anchor_iou(w, h, cw, ch);
    const double dw = w - cw, dh = h - ch;
    const double a = dw * dw, b = dh * dh;
    return a + b;
}

__device__ __forceinline__ u64 fixed40(double d) { return (u64)(d * 0x1p40); }       // d >= 0: truncation is the floor

// the weight of a valid box in seeding round `round` against the seeds in c[0 .. round)
__device__ __forceinline__ u64 seed_weight(int distance, int round, const double (*c)[2], u64 qw, u64 qh) {
    if (round == 0) return 1ull;
    const double w = unit(qw), h = unit(qh);
    u64 best = ~0ull;
    for (int j = 0; j < round; ++j) {
        const u64 d = fixed40(anchor_dist(distance, w, h, c[j][0], c[j][1]));
        best = d < best ? d : best;
    }
    return best;
}

__device__ __forceinline__ void mark_done(const AnchorParams &p, AnchorRestart &st, unsigned bits) {
    st.status |= bits;
    st.done = 1;
    atomicAdd(&p.prep->n_done, 1ull);
}

}  // namespace

__global__ void __launch_bounds__(256) anchor_prepare_kernel(const AnchorParams p) {
    __shared__ u64 s[10];
    const int tid = threadIdx.x;
    if (tid < 10) s[tid] = 0ull;
    __syncthreads();
    u64 v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < PER; ++j) {
        const long long i = (long long)blockIdx.x * CH + j * BL + tid;
        if (i >= p.n) break;
        u64 q[2] = {quantise(p.wh[2 * i]), quantise(p.wh[2 * i + 1])};
        if (!q[0] || !q[1]) {
            q[0] = q[1] = 0ull;
            v[1] += 1ull;
        } else {
            v[0] += 1ull;
            for (int c = 0; c < 2; ++c) {
                const u64 hi = q[c] >> 20, lo = q[c] & 0xfffffull;
                v[2 + c] += q[c]; v[4 + c] += hi * hi; v[6 + c] += hi * lo; v[8 + c] += lo * lo;
            }
        }
        p.q[2 * i] = q[0];
        p.q[2 * i + 1] = q[1];
    }
    for (int m = 0; m < 10; ++m)
        if (v[m]) atomicAdd(&s[m], v[m]);
    __syncthreads();
    if (tid < 10 && s[tid]) atomicAdd(reinterpret_cast<u64 *>(p.prep) + tid, s[tid]);      // AnchorPrep's first ten words, in this order
}

__global__ void __launch_bounds__(64) anchor_init_kernel(const AnchorParams p) {
    AnchorRestart &st = p.state[blockIdx.x];
    u64 *words = reinterpret_cast<u64 *>(&st);
    for (int i = threadIdx.x; i < (int)(sizeof(AnchorRestart) / 8); i += 64) words[i] = 0ull;
    __syncthreads();
    if (threadIdx.x < MAXK) st.seed[threadIdx.x] = -1;
    __syncthreads();
    if (threadIdx.x != 0) return;
    bool bad = p.prep->n_valid == 0ull && p.init != nullptr;      // (seeded: round 0 finds T == 0)
    if (p.init) {
        for (int c = 0; c < p.k; ++c)
            for (int a = 0; a < 2; ++a) {
                const double v = p.init[2 * c + a];
                if (!(v > 0.0) || !(v <= 1.0)) bad = true;
                st.centre[c][a] = v;
            }
    }
    if (bad) mark_done(p, st, YOLO_ANCHOR_DEGENERATE);
}

__global__ void __launch_bounds__(256) anchor_seed_sum_kernel(const AnchorParams p) {
    __shared__ double s_c[MAXK][2];
    __shared__ u64 s_sum;
    const AnchorRestart &st = p.state[blockIdx.y];
    if (st.done) return;
    const int tid = threadIdx.x, round = p.round;
    if (tid < 2 * round) s_c[tid >> 1][tid & 1] = st.centre[tid >> 1][tid & 1];
    if (tid == 0) s_sum = 0ull;
    __syncthreads();
    u64 mine = 0ull;
    for (int j = 0; j < PER; ++j) {
        const long long i = (long long)blockIdx.x * CH + j * BL + tid;
        if (i >= p.n) break;
        const u64 qw = p.q[2 * i], qh = p.q[2 * i + 1];
        if (qw) mine += seed_weight(p.distance, round, s_c, qw, qh);
    }
    if (mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (tid == 0) p.chunk_sum[(size_t)blockIdx.y * p.n_chunks + blockIdx.x] = s_sum;
}

__global__ void __launch_bounds__(256) anchor_seed_pick_kernel(const AnchorParams p) {
    __shared__ double s_c[MAXK][2];
    __shared__ u64 s_part[BL];
    __shared__ u64 s_t, s_base;
    __shared__ int s_chunk, s_thread;
    AnchorRestart &st = p.state[blockIdx.x];
    if (st.done) return;
    const int tid = threadIdx.x, round = p.round;
    if (tid < 2 * round) s_c[tid >> 1][tid & 1] = st.centre[tid >> 1][tid & 1];
    const u64 *sums = p.chunk_sum + (size_t)blockIdx.x * p.n_chunks;
    const int per = (p.n_chunks + BL - 1) / BL;                    // chunks per thread, consecutive
    const int c0 = tid * per, c1 = c0 + per < p.n_chunks ? c0 + per : p.n_chunks;
    u64 mine = 0ull;
    for (int c = c0; c < c1; ++c) mine += sums[c];
    s_part[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        u64 total = 0ull;
        for (int t = 0; t < BL; ++t) total += s_part[t];
        s_chunk = -1;
        if (total) {
            unsigned o[4];
            philox4x32_10(blockIdx.x, (unsigned)round, (unsigned)p.seed, (unsigned)(p.seed >> 32), o);
            const u64 u = ((u64)o[0] << 32) | (u64)o[1];
            const u64 t = __umul64hi(u, total);                    // floor(u * T / 2^64) < T
            u64 before = 0ull;
            int owner = 0;
            while (owner < BL - 1 && before + s_part[owner] <= t) before += s_part[owner++];
            const int e = (owner + 1) * per < p.n_chunks ? (owner + 1) * per : p.n_chunks;
            int c = owner * per;
            while (c < e - 1 && before + sums[c] <= t) before += sums[c++];
            if (c < p.n_chunks) { s_chunk = c; s_base = before; s_t = t; }
        }
    }
    __syncthreads();
    const int chunk = s_chunk;
    if (chunk < 0) {                                               // T == 0: fewer distinct boxes than k, or no valid box
        if (tid == 0) mark_done(p, st, YOLO_ANCHOR_DEGENERATE);
        return;
    }
    // the chunk again, PER consecutive boxes per thread so that the prefix runs in index order
    u64 d[PER];
    mine = 0ull;
    for (int j = 0; j < PER; ++j) {
        const long long i = (long long)chunk * CH + tid * PER + j;
        d[j] = 0ull;
        if (i < p.n) {
            const u64 qw = p.q[2 * i], qh = p.q[2 * i + 1];
            if (qw) d[j] = seed_weight(p.distance, round, s_c, qw, qh);
        }
        mine += d[j];
    }
    s_part[tid] = mine;                                            // (thread 0 read the chunk partials in front of the barrier above)
    __syncthreads();
    if (tid == 0) {
        u64 before = s_base;
        int owner = 0;
        while (owner < BL - 1 && before + s_part[owner] <= s_t) before += s_part[owner++];
        s_base = before;
        s_thread = owner;
    }
    __syncthreads();
    if (tid != s_thread) return;
    u64 before = s_base;
    int j = 0;
    while (j < PER - 1 && before + d[j] <= s_t) before += d[j++];
    const long long i = (long long)chunk * CH + tid * PER + j;
    if (i >= p.n || !d[j] || before + d[j] <= s_t) {               // cannot happen while both passes compute the same weights
        mark_done(p, st, YOLO_ANCHOR_DEGENERATE);
        return;
    }
    st.seed[round] = (int32_t)i;
    st.centre[round][0] = unit(p.q[2 * i]);
    st.centre[round][1] = unit(p.q[2 * i + 1]);
}

template <bool FINAL>
__global__ void __launch_bounds__(256) anchor_assign_kernel(const AnchorParams p) {
    __shared__ double s_c[MAXK][2];
    __shared__ u64 s_acc[MAXK][3];
    __shared__ u64 s_misc[2];               // iterations: [0] changed; final: [0] S qd, [1] S floor(best IoU * 2^40)
    AnchorRestart &st = p.state[blockIdx.y];
    if (FINAL ? (st.status & YOLO_ANCHOR_DEGENERATE) != 0u : st.done != 0) return;
    const int tid = threadIdx.x, k = p.k;
    if (tid < 2 * k) s_c[tid >> 1][tid & 1] = st.centre[tid >> 1][tid & 1];
    if (tid < 3 * k) s_acc[tid / 3][tid % 3] = 0ull;
    if (tid < 2) s_misc[tid] = 0ull;
    __syncthreads();
    unsigned char *lab = p.label8 + (size_t)blockIdx.y * p.label_stride;
    u64 m0 = 0ull, m1 = 0ull;
    for (int j = 0; j < PER; ++j) {
        const long long i = (long long)blockIdx.x * CH + j * BL + tid;
        if (i >= p.n) break;
        const u64 qw = p.q[2 * i], qh = p.q[2 * i + 1];
        if (!qw) continue;
        const double w = unit(qw), h = unit(qh);
        double best = anchor_dist(p.distance, w, h, s_c[0][0], s_c[0][1]);
        int label = 0;
        for (int c = 1; c < k; ++c) {
            const double d = anchor_dist(p.distance, w, h, s_c[c][0], s_c[c][1]);
            if (d < best) { best = d; label = c; }
        }
        atomicAdd(&s_acc[label][0], qw);
        atomicAdd(&s_acc[label][1], qh);
        atomicAdd(&s_acc[label][2], 1ull);
        if (FINAL) {
            double iou = anchor_iou(w, h, s_c[0][0], s_c[0][1]);
            for (int c = 1; c < k; ++c) {
                const double v = anchor_iou(w, h, s_c[c][0], s_c[c][1]);
                iou = v > iou ? v : iou;
            }
            m0 += fixed40(best);
            m1 += fixed40(iou);
            lab[i] = (unsigned char)label;
        } else if (lab[i] != (unsigned char)label) {
            lab[i] = (unsigned char)label;
            m0 += 1ull;
        }
    }
    if (m0) atomicAdd(&s_misc[0], m0);
    if (m1) atomicAdd(&s_misc[1], m1);
    __syncthreads();
    if (tid < 3 * k) {
        const u64 v = s_acc[tid / 3][tid % 3];
        if (v) atomicAdd(FINAL ? &st.fin[tid / 3][tid % 3] : &st.acc[tid / 3][tid % 3], v);
    } else if (tid >= 128 && tid < 130) {
        const u64 v = s_misc[tid - 128];
        if (v) atomicAdd(FINAL ? (tid == 128 ? &st.inertia_q : &st.iou_q) : &st.changed, v);      // (iterations: s_misc[1] stays 0)
    }
}

__global__ void __launch_bounds__(64) anchor_update_kernel(const AnchorParams p) {
#pragma clang fp contract(off)
    AnchorRestart &st = p.state[blockIdx.x];
    if (st.done || threadIdx.x != 0) return;
    double shift = 0.0;
    bool empty = false;
    for (int c = 0; c < p.k; ++c) {
        const u64 cnt = st.acc[c][2];
        if (cnt) {
            const double den = (double)cnt * 0x1p40;
            const double nw = (double)st.acc[c][0] / den, nh = (double)st.acc[c][1] / den;
            const double dw = nw - st.centre[c][0], dh = nh - st.centre[c][1];
            const double a = dw * dw, b = dh * dh;
            shift = shift + (a + b);
            st.centre[c][0] = nw;
            st.centre[c][1] = nh;
        } else {
            empty = true;
        }
        st.acc[c][0] = st.acc[c][1] = st.acc[c][2] = 0ull;
    }
    const u64 changed = st.changed;
    st.changed = 0ull;
    const int t = ++st.n_iter;
    if (empty) st.status |= YOLO_ANCHOR_EMPTY_CLUSTER;
    if (t >= 2 && changed == 0ull) mark_done(p, st, 0u);
    else if (p.distance == YOLO_ANCHOR_EUCLIDEAN && shift <= p.threshold) mark_done(p, st, 0u);
    else if (t >= p.max_iter) mark_done(p, st, YOLO_ANCHOR_MAX_ITER);
}

__global__ void __launch_bounds__(64) anchor_finish_kernel(const AnchorParams p) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, k = p.k;
    yolo_anchor_restart *table = reinterpret_cast<yolo_anchor_restart *>(p.result + p.restarts_offset);
    if (tid < p.n_init) {
        AnchorRestart &st = p.state[tid];
        unsigned status = st.status;
        if (!(status & YOLO_ANCHOR_DEGENERATE))
            for (int c = 0; c < k; ++c)
                if (!st.fin[c][2]) status |= YOLO_ANCHOR_EMPTY_CLUSTER;
        st.status = status;
        yolo_anchor_restart &r = table[tid];
        r.n_iter = st.n_iter;
        r.status = status;
        r.inertia_q = st.inertia_q;
        r.iou_q = st.iou_q;
        for (int j = 0; j < MAXK; ++j) r.seeds[j] = st.seed[j];
    }
    __syncthreads();
    if (tid != 0) return;
    int best = -1;
    for (int r = 0; r < p.n_init; ++r) {
        const AnchorRestart &st = p.state[r];
        if (st.status & YOLO_ANCHOR_DEGENERATE) continue;
        if (best < 0 || st.inertia_q < p.state[best].inertia_q) best = r;
    }
    const u64 n_valid = p.prep->n_valid, n_bad = p.prep->n_bad;
    yolo_anchor_header &hdr = *reinterpret_cast<yolo_anchor_header *>(p.result + p.header_offset);
    yolo_anchor_best &out = *reinterpret_cast<yolo_anchor_best *>(p.result + p.best_offset);
    hdr.status = (n_bad ? YOLO_ANCHOR_BAD_BOX : 0u) | (best < 0 ? YOLO_ANCHOR_DEGENERATE : p.state[best].status);
    hdr.best_restart = best;
    hdr.n_valid = (int32_t)n_valid;
    hdr.n_bad = (int32_t)n_bad;
    hdr.k = k; hdr.n_init = p.n_init; hdr.distance = p.distance; hdr.pad_ = 0;
    p.pick->best = best;
    for (int c = 0; c < MAXK; ++c) p.pick->rank[c] = -1;
    if (best < 0) return;                   // (the best block stays zero: the entry cleared the result)
    const AnchorRestart &st = p.state[best];
    int order[MAXK];
    double area[MAXK];
    for (int c = 0; c < k; ++c) {           // insertion sort: ascending area, then cw, then cluster index
        const double a = st.centre[c][0] * st.centre[c][1];
        int at = c;
        while (at > 0) {
            const int o = order[at - 1];
            const bool before = a < area[o] || (a == area[o] && st.centre[c][0] < st.centre[o][0]);
            if (!before) break;
            order[at] = o;
            --at;
        }
        order[at] = c;
        area[c] = a;
    }
    for (int j = 0; j < k; ++j) {
        const int c = order[j];
        p.pick->rank[c] = j;
        out.centres[j][0] = st.centre[c][0];
        out.centres[j][1] = st.centre[c][1];
        out.counts[j] = (int64_t)st.fin[c][2];
        out.sum_q[j][0] = st.fin[c][0];
        out.sum_q[j][1] = st.fin[c][1];
    }
    out.inertia_q = st.inertia_q;
    out.iou_q = st.iou_q;
    out.inertia = (double)st.inertia_q * 0x1p-40;
    out.avg_iou = (double)st.iou_q / ((double)n_valid * 0x1p40);
}

__global__ void __launch_bounds__(256) anchor_labels_kernel(const AnchorParams p) {
    const int best = p.pick->best;
    const unsigned char *lab = p.label8 + (size_t)(best < 0 ? 0 : best) * p.label_stride;
    for (int j = 0; j < PER; ++j) {
        const long long i = (long long)blockIdx.x * CH + j * BL + threadIdx.x;
        if (i >= p.n) break;
        int v = -1;
        if (best >= 0 && p.q[2 * i]) {
            const unsigned c = lab[i];
            if (c < (unsigned)p.k) v = p.pick->rank[c];
        }
        p.labels[i] = v;
    }
}

hipError_t launch_anchor(int stage, const AnchorParams &p, hipStream_t s) {
    if (p.n < 1 || p.n > YOLO_ANCHOR_MAX_N || p.k < 1 || p.k > MAXK || p.n_init < 1 || p.n_init > YOLO_ANCHOR_MAX_INIT ||
        p.n_chunks != (p.n + CH - 1) / CH || p.round < 0 || p.round >= MAXK)
        return hipErrorInvalidValue;
    const dim3 chunks((unsigned)p.n_chunks), both((unsigned)p.n_chunks, (unsigned)p.n_init), restarts((unsigned)p.n_init);
    switch (stage) {
    case ANCHOR_PREPARE: hipLaunchKernelGGL(anchor_prepare_kernel, chunks, dim3(256), 0, s, p); break;
    case ANCHOR_INIT: hipLaunchKernelGGL(anchor_init_kernel, restarts, dim3(64), 0, s, p); break;
    case ANCHOR_SEED_SUM: hipLaunchKernelGGL(anchor_seed_sum_kernel, both, dim3(256), 0, s, p); break;
    case ANCHOR_SEED_PICK: hipLaunchKernelGGL(anchor_seed_pick_kernel, restarts, dim3(256), 0, s, p); break;
    case ANCHOR_ASSIGN: hipLaunchKernelGGL(anchor_assign_kernel<false>, both, dim3(256), 0, s, p); break;
    case ANCHOR_UPDATE: hipLaunchKernelGGL(anchor_update_kernel, restarts, dim3(64), 0, s, p); break;
    case ANCHOR_FINAL: hipLaunchKernelGGL(anchor_assign_kernel<true>, both, dim3(256), 0, s, p); break;
    case ANCHOR_FINISH: hipLaunchKernelGGL(anchor_finish_kernel, dim3(1), dim3(64), 0, s, p); break;
    case ANCHOR_LABELS:
        if (!p.labels) return hipErrorInvalidValue;
        hipLaunchKernelGGL(anchor_labels_kernel, chunks, dim3(256), 0, s, p);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace yolo

// The weight gradient of the YOLOv3 head convs on the device (include/yolo_hip.h: yolo_v3_head_wgrad; the definition is there).
//
// The gradient G of the v3 loss is sparse by construction: a row that is no winner holds at most its objectness element, a winner row
// (one per truth at most) is full.  So dW_s = G_s^T X_s falls into two parts that share nothing:
// head3_obj_kernel     the rows o = a * (5 + C) + 4 of every dW_s and those elements of db_s: one pass over X_s and column 4 of G, float32
//                      FMAs in registers, one chunk of positions per group of cin / 8 threads, into a float32 slab.  All scales in one launch.
// head3_reduce_kernel  adds the slabs in chunk order into those rows, tiles of slabs staged through LDS.
// head3_slot_kernel    slot[n][j] = the row truth j of image n owns in the assign table, or -1.
// head3_win_kernel     every other row: the rank-1 terms of the winner rows, images ascending, then truths ascending.
// Elements of G the assign table declares a structural zero are never read.  Compiled with default NaN handling, like train.hip.
#include <hip/hip_runtime.h>

#include "wgrad_load.h"
#include "yolo_internal.h"

namespace yolo {

static_assert(kWgrad3Lane == 8, "wgrad_load8 loads eight channels");
static_assert(kWgrad3Threads % 64 == 0 && kWgrad3Threads % kWgrad3RedElems == 0 && kWgrad3RedChunks % (kWgrad3Threads / kWgrad3RedElems) == 0 &&
              kWgrad3WinTile == kWgrad3Threads && kWgrad3WinRows <= kWgrad3Threads && kWgrad3WinRows % 4 == 0, "the thread maps of the reduce and winner kernels");
static_assert(YOLO_EVAL_MAX_GT <= 1024, "head3_slot_kernel keeps an image's slots in LDS");

// the scale a workgroup of one of the three launches belongs to: blk0 is the scale's first workgroup in that launch
template <int Wgrad3Scale::*BLK0>
__device__ __forceinline__ int wgrad3_scale(const Wgrad3Params &p) {
    int s = 0;
#pragma unroll
    for (int i = 1; i < YOLO_MAX_SCALES; ++i)
        if (i < p.n_scales && (int)blockIdx.x >= p.sc[i].*BLK0) s = i;
    return s;
}

// Thread t of a scale (its workgroups counted from the scale's first) belongs to chunk t / tpc and owns the channels
// 8 (t % tpc) .. + 8 of it: it walks the positions [chunk * ppc, min(P, (chunk + 1) * ppc)) in ascending order, loads its eight channels of
// X (one 16-byte load where the view allows) and the na objectness elements of the position's rows (4-byte loads: a row of 5 + C floats
// is not 16-byte periodic), and keeps na x 8 float32 sums.  The thread of channel 0 also adds the objectness elements themselves (db).
// Every element of the chunk's slab is written.  The loop is free of branches on the view's type, so that the loads of several
// positions are in flight together: the anchor count and the load form are template parameters.
template <int NA, typename T, bool WIDE>
__device__ __forceinline__ void head3_obj_chunk(const Wgrad3Params &p, const Wgrad3Scale &sc, int chunk, int c) {
    constexpr int na = NA;
    const int stride = p.stride;
    const int p_begin = chunk * sc.ppc;
    const int p_end = sc.P - p_begin < sc.ppc ? sc.P : p_begin + sc.ppc;
    float acc[NA][8], dbs[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        dbs[a] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[a][j] = 0.f;
    }
    const T *x = static_cast<const T *>(sc.x) + sc.coff + c;
    int n = p_begin / sc.ppi, q = p_begin - n * sc.ppi;
#pragma unroll 4
    for (int pp = p_begin; pp < p_end; ++pp) {
        float v[8];
        wgrad_load8<T, WIDE>(x + (long long)n * sc.img_stride + (long long)q * sc.ld, v);
        const float *g4 = p.g + ((size_t)n * p.rows + sc.row0 + (size_t)q * na) * stride + 4;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const float g = g4[(size_t)a * stride];
            dbs[a] += g;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[a][j] += g * v[j];
        }
        const bool wrap = ++q == sc.ppi;
        q = wrap ? 0 : q;
        n += wrap;
    }
    float *slab = sc.slab + (size_t)chunk * ((size_t)na * sc.cin + 8);      // (a multiple of 8 floats; the scratch is 16-byte aligned)
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        float4 *dst = reinterpret_cast<float4 *>(slab + (size_t)a * sc.cin + c);
        dst[0] = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
        dst[1] = make_float4(acc[a][4], acc[a][5], acc[a][6], acc[a][7]);
        if (c == 0) slab[(size_t)na * sc.cin + a] = dbs[a];
    }
}

template <int NA>
__device__ __forceinline__ void head3_obj_view(const Wgrad3Params &p, const Wgrad3Scale &sc, int chunk, int c) {
    if (sc.f16) {
        if (sc.wide) head3_obj_chunk<NA, _Float16, true>(p, sc, chunk, c);
        else head3_obj_chunk<NA, _Float16, false>(p, sc, chunk, c);
    } else {
        if (sc.wide) head3_obj_chunk<NA, float, true>(p, sc, chunk, c);
        else head3_obj_chunk<NA, float, false>(p, sc, chunk, c);
    }
}

__global__ void __launch_bounds__(kWgrad3Threads) head3_obj_kernel(const Wgrad3Params p) {
    const Wgrad3Scale &sc = p.sc[wgrad3_scale<&Wgrad3Scale::obj_blk0>(p)];
    const int t = ((int)blockIdx.x - sc.obj_blk0) * kWgrad3Threads + (int)threadIdx.x;
    const int chunk = t / sc.tpc, c = (t - chunk * sc.tpc) * kWgrad3Lane;
    if (chunk >= sc.n_chunks) return;
    static_assert(YOLO_MAX_ANCHORS == 8, "one case per anchor count");
    switch (sc.na) {
        case 1: head3_obj_view<1>(p, sc, chunk, c); break;
        case 2: head3_obj_view<2>(p, sc, chunk, c); break;
        case 3: head3_obj_view<3>(p, sc, chunk, c); break;
        case 4: head3_obj_view<4>(p, sc, chunk, c); break;
        case 5: head3_obj_view<5>(p, sc, chunk, c); break;
        case 6: head3_obj_view<6>(p, sc, chunk, c); break;
        case 7: head3_obj_view<7>(p, sc, chunk, c); break;
        default: head3_obj_view<8>(p, sc, chunk, c); break;
    }
}

// Element e < na * cin of a scale is dW[a * (5 + C) + 4][c] with a = e / cin, the na behind them db[a * (5 + C) + 4]: the slabs' elements
// e added in chunk order.  A workgroup owns kWgrad3RedElems consecutive elements and walks the chunks kWgrad3RedChunks at a time: all
// threads load the tile [chunks][elements] (element = tid % 32: 128 contiguous bytes per chunk), one stage ahead, into LDS; the first
// 32 threads then add their element's column in chunk order.  Nothing is read from dW or db.
__global__ void __launch_bounds__(kWgrad3Threads) head3_reduce_kernel(const Wgrad3Params p) {
    __shared__ float tile[kWgrad3RedChunks][kWgrad3RedElems];
    constexpr int kRows = kWgrad3Threads / kWgrad3RedElems, kPer = kWgrad3RedChunks / kRows;       // 8 chunk rows a pass, 32 passes a thread
    const Wgrad3Scale &sc = p.sc[wgrad3_scale<&Wgrad3Scale::red_blk0>(p)];
    const int tid = threadIdx.x, col = tid % kWgrad3RedElems, row = tid / kWgrad3RedElems;
    const int n_dw = sc.na * sc.cin, n_all = n_dw + sc.na;
    const int e = ((int)blockIdx.x - sc.red_blk0) * kWgrad3RedElems + col;
    const size_t cs = (size_t)n_dw + 8;
    const float *src = sc.slab + (e < n_all ? e : n_all - 1);      // (clamped: every load below is in bounds and unconditional)
    float regs[kPer];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int k = k0 + row + kRows * i;
            regs[i] = src[(size_t)(k < sc.n_chunks ? k : sc.n_chunks - 1) * cs];
        }
    };
    float s = 0.f;
    load(0);
    for (int k0 = 0; k0 < sc.n_chunks; k0 += kWgrad3RedChunks) {
        __syncthreads();        // the sums of the stage before are done with the tile
#pragma unroll
        for (int i = 0; i < kPer; ++i) tile[row + kRows * i][col] = regs[i];
        __syncthreads();
        if (k0 + kWgrad3RedChunks < sc.n_chunks) load(k0 + kWgrad3RedChunks);
        if (tid < kWgrad3RedElems) {
            const int n = sc.n_chunks - k0 < kWgrad3RedChunks ? sc.n_chunks - k0 : kWgrad3RedChunks;
            int k = 0;
            if (k0 == 0) { s = tile[0][col]; k = 1; }       // (the first slab starts the sum: no 0 + x in front of it)
            for (; k + 16 <= n; k += 16) {                  // sixteen LDS reads in flight, added in chunk order
                float v[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = tile[k + i][col];
#pragma unroll
                for (int i = 0; i < 16; ++i) s += v[i];
            }
            for (; k < n; ++k) s += tile[k][col];
        }
    }
    if (tid >= kWgrad3RedElems || e >= n_all) return;
    if (e < n_dw) {
        const int a = e / sc.cin;
        sc.dw[((size_t)a * p.stride + 4) * sc.cin + (e - a * sc.cin)] = s;
    } else {
        sc.db[(size_t)(e - n_dw) * p.stride + 4] = s;
    }
}

// One workgroup per image: the image's slots start at -1 in LDS, every row whose table entry names a truth below max_gt puts itself
// there (a truth owns at most one row, so no two rows meet), and the slots go out.  Every element of slot[n][0 .. max_gt) is written.
__global__ void __launch_bounds__(kWgrad3SlotThreads) head3_slot_kernel(const Wgrad3Params p) {
    __shared__ int slots[YOLO_EVAL_MAX_GT];
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < p.max_gt; j += kWgrad3SlotThreads) slots[j] = -1;
    __syncthreads();
    const int *assign = p.assign + (size_t)n * p.rows;
    for (int r = tid; r < p.rows; r += kWgrad3SlotThreads) {
        const int j = assign[r];
        if (j >= 0 && j < p.max_gt) slots[j] = r;
    }
    __syncthreads();
    for (int j = tid; j < p.max_gt; j += kWgrad3SlotThreads) p.slot[(size_t)n * p.max_gt + j] = slots[j];
}

// A workgroup owns, for one anchor of one scale, kWgrad3WinRows consecutive elements k of the row (5 + C) and kWgrad3WinTile channels: the
// rows o = a * (5 + C) + k of dW, a thread one channel of all of them.  It walks the slots, images ascending and truths ascending,
// kWgrad3Threads at a time: every thread looks at one slot; the winner rows of this scale and anchor are compacted in slot order
// into LDS (wave ballots, a prefix over the waves) together with their elements k of G; then every thread adds
// G[row][k] * X[position][c] for the listed rows in order.  k == 4 belongs to the objectness part: nothing is written for it.  A row
// without a winner is written +0.  The workgroups of the first channel tile add db[o] alike, one thread per k.
__global__ void __launch_bounds__(kWgrad3Threads) head3_win_kernel(const Wgrad3Params p) {
    __shared__ int list_n[kWgrad3Threads], list_q[kWgrad3Threads], wave_count[kWgrad3Threads / 64];      // (image, cell) of the listed rows
    __shared__ __attribute__((aligned(16))) float gs[kWgrad3Threads][kWgrad3WinRows];
    const Wgrad3Scale &sc = p.sc[wgrad3_scale<&Wgrad3Scale::win_blk0>(p)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lb = (int)blockIdx.x - sc.win_blk0;
    const int tile = lb % sc.win_tiles; lb /= sc.win_tiles;
    const int ktile = lb % sc.win_ktiles, a = lb / sc.win_ktiles;
    const int k0 = ktile * kWgrad3WinRows;
    const int c = tile * kWgrad3WinTile + tid;
    const bool on = c < sc.cin;
    const int scale_rows = sc.ppi * sc.na;
    const long long n_slots = (long long)p.batch * p.max_gt;
    float acc[kWgrad3WinRows];
#pragma unroll
    for (int i = 0; i < kWgrad3WinRows; ++i) acc[i] = 0.f;
    float dbs = 0.f;
    for (long long base = 0; base < n_slots; base += kWgrad3Threads) {
        const long long i = base + tid;
        int n = 0, r = -1;
        if (i < n_slots) {
            n = (int)(i / p.max_gt);
            r = p.slot[i] - sc.row0;        // no row: -1 - row0 < 0
        }
        const int q = r / sc.na;
        const bool hit = r >= 0 && r < scale_rows && r - q * sc.na == a;
        const unsigned long long votes = __ballot(hit);
        __syncthreads();        // the products of the stage before are done with the lists
        if (lane == 0) wave_count[wave] = __popcll(votes);
        __syncthreads();
        int at = __popcll(votes & ((1ull << lane) - 1)), count = 0;
#pragma unroll
        for (int w = 0; w < kWgrad3Threads / 64; ++w) {
            if (w < wave) at += wave_count[w];
            count += wave_count[w];
        }
        if (hit) { list_n[at] = n; list_q[at] = q; }
        __syncthreads();
        if (count == 0) continue;       // (the same in every thread)
        // G of the listed rows into LDS, eight loads of a thread in flight (clamped: in bounds and unconditional; a thread owns one k)
        const int gk = tid % kWgrad3WinRows, k = k0 + gk, kc = k < p.stride ? k : p.stride - 1;
        const bool k_on = k < p.stride && k != 4;
        constexpr int kJ = kWgrad3Threads / kWgrad3WinRows;        // listed rows a pass of the workgroup covers
        for (int j0 = tid / kWgrad3WinRows; j0 < count; j0 += 8 * kJ) {
            float gv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int j = j0 + i * kJ < count ? j0 + i * kJ : count - 1;
                gv[i] = p.g[((size_t)list_n[j] * p.rows + sc.row0 + (size_t)list_q[j] * sc.na + a) * p.stride + kc];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (j0 + i * kJ < count) gs[j0 + i * kJ][gk] = k_on ? gv[i] : 0.f;
        }
        auto load_x = [&](int j0, float (&xv)[16]) {      // the X of sixteen listed rows in flight
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = j0 + i < count ? j0 + i : count - 1;
                const long long xat = (long long)list_n[j] * sc.img_stride + (long long)list_q[j] * sc.ld + sc.coff + (on ? c : 0);
                xv[i] = sc.f16 ? (float)static_cast<const _Float16 *>(sc.x)[xat] : static_cast<const float *>(sc.x)[xat];
            }
        };
        float xv[16];
        load_x(0, xv);          // (on their way while the G tile settles)
        __syncthreads();
        if (on) {
            for (int j0 = 0; j0 < count; j0 += 16) {        // added in list order
                if (j0) load_x(j0, xv);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (j0 + i < count) {
#pragma unroll
                        for (int kk = 0; kk < kWgrad3WinRows; kk += 4) {
                            const float4 g = *reinterpret_cast<const float4 *>(&gs[j0 + i][kk]);
                            acc[kk] += g.x * xv[i]; acc[kk + 1] += g.y * xv[i]; acc[kk + 2] += g.z * xv[i]; acc[kk + 3] += g.w * xv[i];
                        }
                    }
                }
            }
        }
        if (tile == 0 && tid < kWgrad3WinRows)
            for (int j = 0; j < count; ++j) dbs += gs[j][tid];
    }
#pragma unroll
    for (int kk = 0; kk < kWgrad3WinRows; ++kk) {
        const int k = k0 + kk;
        if (on && k < p.stride && k != 4) sc.dw[((size_t)a * p.stride + k) * sc.cin + c] = acc[kk];
    }
    if (tile == 0 && tid < kWgrad3WinRows && k0 + tid < p.stride && k0 + tid != 4) sc.db[(size_t)a * p.stride + k0 + tid] = dbs;
}

hipError_t launch_head3_wgrad(const Wgrad3Params &p, hipStream_t s) {
    hipLaunchKernelGGL(head3_obj_kernel, dim3((unsigned)p.obj_blocks), dim3(kWgrad3Threads), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head3_reduce_kernel, dim3((unsigned)p.red_blocks), dim3(kWgrad3Threads), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(head3_slot_kernel, dim3((unsigned)p.batch), dim3(kWgrad3SlotThreads), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(head3_win_kernel, dim3((unsigned)p.win_blocks), dim3(kWgrad3Threads), 0, s, p);
    return hipGetLastError();
}

}  // namespace yolo

// yolo_conv3x3_wgrad_f16 (include/yolo_hip.h; the definition is there): the 3 x 3 weight gradient with D narrowed to fp16 by one
// power-of-two scale per call, on the fp16 matrix cores.
//
// conv3x3_wgrad_f16_max_kernel     m = max |D| as an integer maximum of bit patterns into the record, and per group of positions the partial
//                                  sums of db[o] = S_p D[p][o] from the float32 D, behind the record.
// conv3x3_wgrad_f16_kernel         R16[o][t][c] = S_p fp16(D[p][o] 2^k) X3[p + tap t][c], one chunk of positions per workgroup, into a float32
//                                  slab; k from the record.
// conv3x3_wgrad_f16_reduce_kernel  adds the slabs in chunk order into dW3 (times 2^-k, then times the fold's scale) and the partial sums in group
//                                  order into db; writes k into the record.
// Compiled with default NaN and denormal handling, like train_tail.hip: subnormal fp16 operands count, a float32 subnormal of D scales exactly.
#include <hip/hip_runtime.h>

#include "train_tail_host.h"
#include "wgrad_load.h"
#include "yolo_internal.h"

namespace yolo {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int kF16Threads = 256;
constexpr int kF16Row = kTailF16RowBytes, kF16Pos = kTailF16TilePos, kF16Pairs = kTailF16TilePos / 2;
static_assert(kTailTileCout == 64 && kTailTileCin == 64 && kF16Pos == 64 && kF16Row == 192, "the loaders and wave maps of conv3x3_wgrad_f16_kernel are written for these");

// k of the header from the bits of m (the sign is clear): 0 for m = 0, Inf and NaN, else clamp(14 - floor(log2 m), -126, 126)
__device__ __forceinline__ int wgrad_f16_k(unsigned int m) {
    if (m == 0u || m >= 0x7f800000u) return 0;
    const int e = (int)(m >> 23);
    const int fl = e ? e - 127 : (31 - __clz((int)m)) - 149;       // a subnormal m: its leading bit
    const int k = 14 - fl;
    return k < -126 ? -126 : k > 126 ? 126 : k;
}
// 2^k, k in [-126, 126]: a normal float32
__device__ __forceinline__ float wgrad_f16_pow2(int k) { return __uint_as_float((unsigned int)(k + 127) << 23); }

// Grid (tiles_cout, db_groups), 256 threads.  A workgroup owns 64 couts and the positions [group * dbp, min(P, (group + 1) * dbp)); a thread
// owns V consecutive couts (V = 4: 16-byte loads, when rows of D allow them) and walks the positions begin + g, begin + g + RG, ... of its
// row group g of RG = 4 V: the maximum of the bit patterns of |D| (an integer maximum: any order gives the same bits) and the sums,
// positions ascending; the RG sums of a column are added in row-group order into partial[group][o].  The record was cleared by the launch
// in front.
template <int V>
__global__ void __launch_bounds__(kF16Threads) conv3x3_wgrad_f16_max_kernel(const float *d, int P, int cout, int dbp, float *partial, unsigned int *record) {
    constexpr int kPerRow = kTailTileCout / V, kGroups = kF16Threads / kPerRow;
    __shared__ float part[kGroups][kTailTileCout];
    __shared__ unsigned int mx_s;
    const int tid = threadIdx.x, c = (tid % kPerRow) * V, g = tid / kPerRow;
    const int o = blockIdx.x * kTailTileCout + c;
    const int p_begin = blockIdx.y * dbp;
    const int p_end = P - p_begin < dbp ? P : p_begin + dbp;
    if (tid == 0) mx_s = 0u;
    float s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 0.f;
    unsigned int mx = 0u;
    if (o < cout) {         // (V = 4: cout % 4 == 0, so all four couts or none)
#pragma unroll 4
        for (int pp = p_begin + g; pp < p_end; pp += kGroups) {
            float v[V];
            if constexpr (V == 4) {
                const float4 a = *reinterpret_cast<const float4 *>(d + (size_t)pp * cout + o);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
            } else {
                v[0] = d[(size_t)pp * cout + o];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const unsigned int b = __float_as_uint(v[j]) & 0x7fffffffu;
                s[j] += v[j];
                mx = b > mx ? b : mx;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) part[g][c + j] = s[j];
    __syncthreads();
    if (mx) atomicMax(&mx_s, mx);
    __syncthreads();
    if (tid < kTailTileCout && blockIdx.x * kTailTileCout + tid < cout) {
        float t = part[0][tid];
#pragma unroll
        for (int r = 1; r < kGroups; ++r) t += part[r][tid];
        partial[(size_t)blockIdx.y * cout + blockIdx.x * kTailTileCout + tid] = t;
    }
    if (tid == 0 && mx_s) atomicMax(record, mx_s);
}

// eight consecutive channels of one position as stored; WIDE: the address is 16-byte aligned
template <bool WIDE>
__device__ __forceinline__ f16x8 wgrad_f16_load8(const _Float16 *src) {
    if constexpr (WIDE) {
        return *reinterpret_cast<const f16x8 *>(src);
    } else {
        f16x8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = src[j];
        return h;
    }
}

// The global loads of one 64-position stage into registers, and the 9-bit tap masks of its positions into Ms.  D: position pk + drow, 16
// couts from dseg; X: halo rows xrow + 32 j, 8 channels from xcol.  What lies outside is zeros, never read.
template <bool WIDE, int PASSES>
__device__ __forceinline__ void wgrad_f16_fetch(const Wgrad3x3Params &p, int pk, int p_end, int tid, int o0, const _Float16 *xbase, bool x_on, bool d_wide,
                                                float (&dv)[16], f16x8 (&xr)[PASSES], unsigned int *Ms) {
    const int drow = tid >> 2, dseg = (tid & 3) * 16, xrow = tid >> 3, w = p.w;
    const int pp = pk + drow;
#pragma unroll
    for (int j = 0; j < 16; ++j) dv[j] = 0.f;
    if (pp < p_end) {
        const float *src = p.d + (size_t)pp * p.cout + o0 + dseg;
        if (d_wide) {
#pragma unroll
            for (int j = 0; j < 16; j += 4)
                if (o0 + dseg + j < p.cout) {
                    const float4 a = *reinterpret_cast<const float4 *>(src + j);
                    dv[j] = a.x; dv[j + 1] = a.y; dv[j + 2] = a.z; dv[j + 3] = a.w;
                }
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (o0 + dseg + j < p.cout) dv[j] = src[j];
        }
    }
#pragma unroll
    for (int j = 0; j < PASSES; ++j) {
        const int i = xrow + j * (kF16Threads / 8), q = pk - w - 1 + i;
#pragma unroll
        for (int e = 0; e < 8; ++e) xr[j][e] = (_Float16)0.f;
        if (i < p.halo_rows && x_on && q >= 0 && q < p.P) {
            const int n = q / p.ppi, qq = q - n * p.ppi;
            xr[j] = wgrad_f16_load8<WIDE>(xbase + (long long)n * p.img_stride + (long long)qq * p.ld);
        }
    }
    if (tid < kF16Pos) {
        const int pm = pk + tid;
        unsigned int m = 0u;
        if (pm < p_end) {
            const int n = pm / p.ppi, q = pm - n * p.ppi, r = q / w, x = q - r * w;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int rr = r + t / 3 - 1, xx = x + t % 3 - 1;
                if (rr >= 0 && rr < p.h && xx >= 0 && xx < w) m |= 1u << t;
            }
        }
        Ms[tid] = m;
    }
}

// Grid (tiles_cout * tiles_cin, n_chunks), 256 threads, (halo_rows + 64) * 192 + 9 * 32 * 4 + 64 * 4 bytes of dynamic LDS (all of the kernel's
// LDS: the base stays 16-byte aligned).  A workgroup owns 64 couts x (9 taps x 64 channels) of dW3 and the positions [chunk * ppc, min(P,
// (chunk + 1) * ppc)), 64 at a time, as conv3x3_wgrad_kernel does:
//   load     D[64 positions][64 couts] (16 floats a thread), scaled by 2^k (exact) and narrowed to fp16, round to nearest even; the HALO of
//            X3, the halo_rows = 64 + 2 w + 2 positions [pk - w - 1, pk + 64 + w + 1) of the tile's 64 channels as stored (8 channels a
//            thread, PASSES >= halo_rows / 32 rows a thread); and per tap and PAIR of positions a word whose halves are 0xffff where the tap
//            of that position lies inside its image (and the position inside the chunk), else 0.  Positions outside [0, P), couts behind
//            cout, channels behind cin and rows of D behind the chunk are zeros, never read.  The loads of stage s + 1 are issued into
//            registers in front of the MFMAs of stage s and written to LDS behind them
//   LDS      [position][cout] and [halo position][channel], 16-bit, rows of 192 bytes (128 used): a tap is a row offset, and
//            ds_read_b64_tr_b16 delivers a lane's 8 consecutive positions of one column.  Lane 4 q + j of a 16-lane group addresses row q,
//            columns 4 j .. 4 j + 3 of the group's 4 x 16 block and receives column (lane & 15), rows 0 .. 3.  A 32-lane half reads two
//            blocks of the same four rows, 32 bytes apart: with rows 48 words apart the eight 8-word pieces cover the 64 banks once
//   MFMA     v_mfma_f32_32x32x16_f16: lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k][column l & 31], j = 0 .. 7.  Wave (wm, wn) of
//            2 x 2 computes 32 couts x 32 channels x 9 taps in nine accumulators: one A operand (D16) and nine B operands (rows
//            k + w + 1 + (ky - 1) w + (kx - 1) of the halo, ANDed with the tap's mask words: a halo row of the neighbouring row or image
//            never enters a sum) per 16 positions
// Every lane runs every transposed read (no divergence around them: the instruction needs all lanes).  The sums go to
// slab[chunk][cout][9][cin]; every element of it is written (the cout floats behind it, the db part of the float32 kernel's slab, stay unused).
template <bool WIDE, int PASSES>
__global__ void __launch_bounds__(kF16Threads) conv3x3_wgrad_f16_kernel(const Wgrad3x3Params p, const unsigned int *record) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *Xs = smem;                                               // [halo_rows][192 bytes]
    unsigned char *Ds = smem + (size_t)p.halo_rows * kF16Row;               // [64][192 bytes]
    unsigned int *Mk = reinterpret_cast<unsigned int *>(Ds + kF16Pos * kF16Row);        // [9][32]
    unsigned int *Ms = Mk + 9 * kF16Pairs;                                  // [64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tn = blockIdx.x % p.tiles_cin, tm = blockIdx.x / p.tiles_cin, chunk = blockIdx.y;
    const int o0 = tm * kTailTileCout, c0 = tn * kTailTileCin;
    const int p_begin = chunk * p.ppc;
    const int p_end = p.P - p_begin < p.ppc ? p.P : p_begin + p.ppc;
    const float f = wgrad_f16_pow2(wgrad_f16_k(record[0]));
    const int drow = tid >> 2, dseg = (tid & 3) * 16;       // D: one position, 16 couts
    const int xrow = tid >> 3, xcol = (tid & 7) * 8;        // X: rows xrow, xrow + 32, ..., 8 channels
    const bool x_on = c0 + xcol < p.cin;                    // (cin % 8 == 0: all 8 channels or none)
    const bool d_wide = (uintptr_t)p.d % 16 == 0 && p.cout % 4 == 0;       // then four couts from a multiple of 4 are all inside a row or none
    const _Float16 *xbase = static_cast<const _Float16 *>(p.x) + p.coff + c0 + xcol;
    const int wm = wave >> 1, wn = wave & 1, w = p.w;
    const int grp = lane >> 4, lh = grp >> 1, blk = grp & 1, lq = (lane & 15) >> 2, lj = lane & 3;
    const int a_off = (8 * lh + lq) * kF16Row + (wm * 32 + 16 * blk + 4 * lj) * 2;
    const int b_off = (8 * lh + lq + w + 1) * kF16Row + (wn * 32 + 16 * blk + 4 * lj) * 2;     // the centre tap's rows
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float dv[16];
    f16x8 xr[PASSES];
    wgrad_f16_fetch<WIDE, PASSES>(p, p_begin, p_end, tid, o0, xbase, x_on, d_wide, dv, xr, Ms);
    for (int pk = p_begin; pk < p_end; pk += kF16Pos) {
        __syncthreads();        // the products of the stage before are done with the tiles; Ms of this stage is written
        {
            f16x8 lo, hi;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                lo[j] = (_Float16)(dv[j] * f);
                hi[j] = (_Float16)(dv[j + 8] * f);
            }
            *reinterpret_cast<f16x8 *>(Ds + drow * kF16Row + dseg * 2) = lo;
            *reinterpret_cast<f16x8 *>(Ds + drow * kF16Row + dseg * 2 + 16) = hi;
        }
#pragma unroll
        for (int j = 0; j < PASSES; ++j) {
            const int i = xrow + j * (kF16Threads / 8);
            if (i < p.halo_rows) *reinterpret_cast<f16x8 *>(Xs + i * kF16Row + xcol * 2) = xr[j];
        }
        for (int e = tid; e < 9 * kF16Pairs; e += kF16Threads) {
            const int t = e / kF16Pairs, pr = e - t * kF16Pairs;
            Mk[e] = ((Ms[2 * pr] >> t) & 1u ? 0xffffu : 0u) | ((Ms[2 * pr + 1] >> t) & 1u ? 0xffff0000u : 0u);
        }
        __syncthreads();
        if (pk + kF16Pos < p_end) wgrad_f16_fetch<WIDE, PASSES>(p, pk + kF16Pos, p_end, tid, o0, xbase, x_on, d_wide, dv, xr, Ms);      // in flight under the MFMAs
#pragma unroll 1
        for (int kk = 0; kk < kF16Pos; kk += 16) {
            const unsigned char *ap = Ds + a_off + kk * kF16Row;
            const u32x2 a_lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)ap));
            const u32x2 a_hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(ap + 4 * kF16Row)));
            const u32x4 a32 = {a_lo[0], a_lo[1], a_hi[0], a_hi[1]};
            const f16x8 a = __builtin_bit_cast(f16x8, a32);
            const unsigned char *xc = Xs + b_off + kk * kF16Row;
            const unsigned int *mk = Mk + (kk + 8 * lh) / 2;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const unsigned char *bp = xc + ((t / 3 - 1) * w + (t % 3 - 1)) * kF16Row;      // rows k .. k + 2 w + 2: inside the halo
                const u32x2 b_lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)bp));
                const u32x2 b_hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(bp + 4 * kF16Row)));
                const u32x4 m = *reinterpret_cast<const u32x4 *>(mk + t * kF16Pairs);
                const u32x4 b32 = {b_lo[0] & m[0], b_lo[1] & m[1], b_hi[0] & m[2], b_hi[1] & m[3]};
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(f16x8, b32), acc[t], 0, 0, 0);
            }
        }
    }
    // C / D of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *slab = p.slab + (size_t)chunk * p.slab_stride;
    const int li = lane & 31, lk = lane >> 5;
    const int c = c0 + wn * 32 + li;
    const size_t orow = (size_t)9 * p.cin;
    if (c < p.cin) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (o < p.cout) slab[(size_t)o * orow + (size_t)t * p.cin + c] = acc[t][r];
            }
    }
}

// dW3[e] = scale[o] * (2^-k * (the slabs' elements e added in chunk order)), db[o] = the partial sums added in group order: every element of
// both is written, nothing is read from them.  k goes into the record's second word.
__global__ void __launch_bounds__(kAuxBlock) conv3x3_wgrad_f16_reduce_kernel(const float *slab, const float *scale, unsigned int *record, int n_chunks,
                                                                             int row, int n_dw, int n_all, const float *partial, int db_groups,
                                                                             float *dw, float *db) {
    const int k = wgrad_f16_k(record[0]);
    const float f = wgrad_f16_pow2(-k);
    if (blockIdx.x == 0 && threadIdx.x == 0) record[1] = (unsigned int)k;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_all; e += (long long)gridDim.x * blockDim.x) {
        if (e < n_dw) {
            float s = slab[e];
            for (int j = 1; j < n_chunks; ++j) s += slab[(size_t)j * n_all + e];
            const float r = f * s;
            dw[e] = scale ? scale[e / row] * r : r;
        } else {
            const int o = (int)(e - n_dw), cout = n_all - n_dw;
            float s = partial[o];
            for (int j = 1; j < db_groups; ++j) s += partial[(size_t)j * cout + o];
            db[o] = s;
        }
    }
}

template <int PASSES>
static void launch_wgrad_f16_main(bool wide, dim3 grid, size_t lds, hipStream_t s, const Wgrad3x3Params &p, const unsigned int *record) {
    if (wide) hipLaunchKernelGGL((conv3x3_wgrad_f16_kernel<true, PASSES>), grid, dim3(kF16Threads), lds, s, p, record);
    else hipLaunchKernelGGL((conv3x3_wgrad_f16_kernel<false, PASSES>), grid, dim3(kF16Threads), lds, s, p, record);
}

hipError_t launch_conv3x3_wgrad_f16(const Wgrad3x3Params &p, unsigned int *record, int db_groups, int db_positions, hipStream_t s) {
    hipError_t e = hipMemsetAsync(record, 0, 8, s);
    if (e != hipSuccess) return e;
    float *partial = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(record) + kTailF16RecordBytes);
    const dim3 mgrid((unsigned)p.tiles_cout, (unsigned)db_groups);
    if ((uintptr_t)p.d % 16 == 0 && p.cout % 4 == 0)
        hipLaunchKernelGGL((conv3x3_wgrad_f16_max_kernel<4>), mgrid, dim3(kF16Threads), 0, s, p.d, p.P, p.cout, db_positions, partial, record);
    else
        hipLaunchKernelGGL((conv3x3_wgrad_f16_max_kernel<1>), mgrid, dim3(kF16Threads), 0, s, p.d, p.P, p.cout, db_positions, partial, record);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)(p.tiles_cout * p.tiles_cin), (unsigned)p.n_chunks);
    const size_t lds = (size_t)(p.halo_rows + kF16Pos) * kF16Row + (size_t)9 * kF16Pairs * 4 + (size_t)kF16Pos * 4;
    const bool wide = (uintptr_t)p.x % 16 == 0 && p.ld % 8 == 0 && p.coff % 8 == 0 && p.img_stride % 8 == 0;
    const int passes = (p.halo_rows + kF16Threads / 8 - 1) / (kF16Threads / 8);        // 32 halo rows a pass: 3 (w = 1) .. 9 (w = 96)
    if (passes <= 4) launch_wgrad_f16_main<4>(wide, grid, lds, s, p, record);
    else if (passes <= 6) launch_wgrad_f16_main<6>(wide, grid, lds, s, p, record);
    else launch_wgrad_f16_main<9>(wide, grid, lds, s, p, record);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int row = 9 * p.cin, n_dw = p.cout * row, n_all = n_dw + p.cout;
    int blocks = (n_all + kAuxBlock - 1) / kAuxBlock;
    if (blocks > kAuxGrid) blocks = kAuxGrid;
    hipLaunchKernelGGL(conv3x3_wgrad_f16_reduce_kernel, dim3(blocks), dim3(kAuxBlock), 0, s, p.slab, p.scale, record, p.n_chunks, row, n_dw, n_all, partial,
                       db_groups, p.dw, p.db);
    return hipGetLastError();
}

}  // namespace yolo

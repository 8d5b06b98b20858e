// The two operators a backward pass behind the detection layer is built from (include/yolo_hip.h: yolo_conv1x1_dgrad, yolo_conv3x3_wgrad; the
// definitions are there).
//
// conv1x1_dgrad_kernel         the backward pass of the last conv (1 x 1, stride 1, linear: net/v2.py:52-56) with respect to its input, times
//                              the derivative of the leaky ReLU in front of it: D[p][c] = (S_o G[p][o] W[o][c]) * (Y[p][c] > 0 ? 1 : slope).
// conv3x3_wgrad_kernel         the backward pass of a 3 x 3 / stride 1 / SAME conv with respect to its kernel and bias:
//                              R[o][t][c] = S_p D[p][o] X3[p + tap t][c], db[o] = S_p D[p][o], one chunk of positions per workgroup, into a
//                              float32 slab.
// conv3x3_wgrad_reduce_kernel  adds the slabs in chunk order into dW3 (times the fold's scale) and db.
// tail_adam_kernel             adam_step_kernel's update for a conv with batch norm (yolo_net_train_tail_step): the float32 master kernel
//                              and beta, and in the same pass the conv's packed form with the batch norm folded as the weight loader does.
// Compiled with default NaN handling, like train.hip.
#include <hip/hip_runtime.h>

#include "train_tail_host.h"
#include "wgrad_load.h"
#include "yolo_internal.h"

namespace yolo {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int kTailThreads = 256;
static_assert(kDgradTileCin == 128 && kDgradTilePos == 64 && kDgradTileK == 16, "the loader and wave maps of conv1x1_dgrad_kernel are written for these");
static_assert(kTailTileCout == 64 && kTailTileCin == 64 && kTailTilePos == 32, "the loader and wave maps of conv3x3_wgrad_kernel are written for these");

// four consecutive channels of one position of Y; WIDE: the address is aligned to the four elements
template <typename T, bool WIDE>
__device__ __forceinline__ void dgrad_load4(const T *src, float (&v)[4]) {
    if constexpr (!WIDE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)src[j];
    } else if constexpr (sizeof(T) == 2) {
        const f16x4 h = *reinterpret_cast<const f16x4 *>(src);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)h[j];
    } else {
        const float4 a = *reinterpret_cast<const float4 *>(src);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    }
}

// Grid (tiles_pos * tiles_cin), 256 threads.  A workgroup owns 128 channels x 64 positions of D and walks cout 16 at a time:
//   load     W[16 couts][128 channels] (8 channels a thread, 16-byte loads) and G[64 positions][16 couts] (4 couts a thread); rows behind
//            cout, channels behind cin and positions behind P are zeros, never read: the reduction is padded, whatever cout is
//   LDS      W as it lies in memory, [cout][channel], and G transposed, [cout][position]: the reduction index is the slow one of both (see
//            train.hip on v_mfma_f32_32x32x2_f32: a half wave reads 32 consecutive floats of one row)
//   MFMA     A = W^T (rows = channels), B = G^T (columns = positions): wave (wm, wn) of 2 x 2 computes 64 channels x 32 positions in two
//            accumulators; float32 products, float32 sums, o ascending.  A lane then holds, per group of four registers, four CONSECUTIVE
//            channels of one position: the epilogue multiplies by the slope factor and stores 16 bytes
template <typename T, bool HAS_Y, bool WIDE>
__global__ void __launch_bounds__(kTailThreads) conv1x1_dgrad_kernel(const DgradParams p) {
    __shared__ __attribute__((aligned(16))) float Ws[kDgradTileK][kDgradTileCin];
    __shared__ float Gs[kDgradTileK][kDgradTilePos + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tn = blockIdx.x % p.tiles_cin, tp = blockIdx.x / p.tiles_cin;
    const int c0 = tn * kDgradTileCin, p0 = tp * kDgradTilePos;
    const int wrow = tid >> 4, wcol = (tid & 15) * 8;       // W: one row, 8 channels
    const int gpos = tid >> 2, gk = (tid & 3) * 4;          // G: one position, 4 couts
    const bool w_on = c0 + wcol < p.cin, g_on = p0 + gpos < p.P;        // (cin % 8 == 0: all 8 channels or none)
    const float *wbase = p.w + c0 + wcol;
    const float *gbase = p.g + (size_t)(p0 + gpos) * p.cout;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lk = lane >> 5;
    f32x16 acc0 = {0}, acc1 = {0};
    for (int k0 = 0; k0 < p.cout; k0 += kDgradTileK) {
        __syncthreads();        // the products of the stage before are done with the tiles
        float wreg[8];
        if (w_on && k0 + wrow < p.cout) {
            wgrad_load8<float, true>(wbase + (size_t)(k0 + wrow) * p.cin, wreg);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) wreg[j] = 0.f;
        }
        *reinterpret_cast<float4 *>(&Ws[wrow][wcol]) = make_float4(wreg[0], wreg[1], wreg[2], wreg[3]);
        *reinterpret_cast<float4 *>(&Ws[wrow][wcol + 4]) = make_float4(wreg[4], wreg[5], wreg[6], wreg[7]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = k0 + gk + j;
            Gs[gk + j][gpos] = (g_on && o < p.cout) ? gbase[o] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kDgradTileK; kk += 2) {
            const float b = Gs[kk + lk][wn * 32 + li];
            const float a0 = Ws[kk + lk][wm * 64 + li], a1 = Ws[kk + lk][wm * 64 + 32 + li];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
        }
    }
    // C / D of the 32 x 32 forms: column = lane & 31 (position), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (channel)
    const int pp = p0 + wn * 32 + li;
    if (pp >= p.P) return;
    const T *yrow = nullptr;
    if constexpr (HAS_Y) {
        const int n = pp / p.ppi, q = pp - n * p.ppi;
        yrow = static_cast<const T *>(p.y) + p.coff + (long long)n * p.img_stride + (long long)q * p.ld;
    }
    float *drow = p.d + (size_t)pp * p.cin;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + wm * 64 + half * 32 + 8 * g + 4 * lk;
            if (c >= p.cin) continue;       // (cin % 8 == 0 and c % 4 == 0: all four channels or none)
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = half ? acc1[4 * g + j] : acc0[4 * g + j];
            if constexpr (HAS_Y) {
                float yv[4];
                dgrad_load4<T, WIDE>(yrow + c, yv);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = v[j] * (yv[j] > 0.f ? 1.f : p.slope);
            }
            *reinterpret_cast<float4 *>(drow + c) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

hipError_t launch_conv1x1_dgrad(const DgradParams &p, int y_dtype, long long tiles, hipStream_t s) {
    const dim3 grid((unsigned)tiles), block(kTailThreads);
    if (!p.y) {
        hipLaunchKernelGGL((conv1x1_dgrad_kernel<float, false, false>), grid, block, 0, s, p);
    } else {
        const int esz = y_dtype == YOLO_DTYPE_F16 ? 2 : 4;
        const bool wide = (uintptr_t)p.y % (4 * esz) == 0 && p.ld % 4 == 0 && p.coff % 4 == 0 && p.img_stride % 4 == 0;
        if (y_dtype == YOLO_DTYPE_F16) {
            if (wide) hipLaunchKernelGGL((conv1x1_dgrad_kernel<_Float16, true, true>), grid, block, 0, s, p);
            else hipLaunchKernelGGL((conv1x1_dgrad_kernel<_Float16, true, false>), grid, block, 0, s, p);
        } else {
            if (wide) hipLaunchKernelGGL((conv1x1_dgrad_kernel<float, true, true>), grid, block, 0, s, p);
            else hipLaunchKernelGGL((conv1x1_dgrad_kernel<float, true, false>), grid, block, 0, s, p);
        }
    }
    return hipGetLastError();
}

// Grid (tiles_cout * tiles_cin, n_chunks), 256 threads, halo_rows * 64 floats of dynamic LDS.  A workgroup owns 64 couts x (9 taps x 64
// channels) of dW3 and the positions [chunk * ppc, min(P, (chunk + 1) * ppc)), 32 at a time.  Positions are the flat index
// (n * h + r) * w + x, so tap (ky, kx) of position p is position p + (ky - 1) w + (kx - 1) WHEN it lies inside the image:
//   load     D[32 positions][64 couts] (8 floats a thread); the HALO of X3, the halo_rows = 32 + 2 w + 2 positions
//            [pk - w - 1, pk + 32 + w + 1) of the tile's 64 channels (8 channels a thread): each element comes into LDS once per stage
//            and serves all nine taps; and per position a 9-bit mask of the taps that lie inside its image.  Positions outside [0, P),
//            couts behind cout, channels behind cin and rows of D behind the chunk are zeros, never read
//   LDS      [position][cout], [halo position][channel]: the reduction index is the slow one of both (train.hip)
//   MFMA     wave (wm, wn) of 2 x 2 computes 32 couts x 32 channels x 9 taps in nine accumulators: one A operand (D) and nine B
//            operands (row k + w + 1 + (ky - 1) w + (kx - 1) of the halo, or +0 where the mask says the tap is outside the image: a halo
//            row of the neighbouring row or image never enters a sum) per step; float32 products, float32 sums, positions ascending
//   db       in the workgroups of the first cin tile, thread t < 64 adds column t of the D tile, positions in ascending order
// The sums go to slab[chunk][cout][9][cin] and slab[chunk][cout * 9 * cin + cout]; every element of a chunk's slab is written.
template <typename T, bool WIDE>
__global__ void __launch_bounds__(kTailThreads) conv3x3_wgrad_kernel(const Wgrad3x3Params p) {
    extern __shared__ __attribute__((aligned(16))) float Xs[];      // [halo_rows][kTailTileCin]
    __shared__ float Ds[kTailTilePos][kTailTileCout];
    __shared__ int Ms[kTailTilePos];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tn = blockIdx.x % p.tiles_cin, tm = blockIdx.x / p.tiles_cin, chunk = blockIdx.y;
    const int o0 = tm * kTailTileCout, c0 = tn * kTailTileCin;
    const int p_begin = chunk * p.ppc;
    const int p_end = p.P - p_begin < p.ppc ? p.P : p_begin + p.ppc;
    const int dcol = tid & 63, drow = tid >> 6;             // D: rows drow, drow + 4, ..., drow + 28
    const int xrow = tid >> 3, xcol = (tid & 7) * 8;        // X: rows xrow, xrow + 32, ..., 8 channels
    const bool d_on = o0 + dcol < p.cout, x_on = c0 + xcol < p.cin;     // (cin % 8 == 0: all 8 channels or none)
    const T *xbase = static_cast<const T *>(p.x) + p.coff + c0 + xcol;
    const float *dbase = p.d + o0 + dcol;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lk = lane >> 5;
    const int w = p.w;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float dbsum = 0.f;
    const bool db_on = tn == 0 && tid < kTailTileCout;
    for (int pk = p_begin; pk < p_end; pk += kTailTilePos) {
        __syncthreads();        // the products of the stage before are done with the tiles
#pragma unroll
        for (int i = 0; i < kTailTilePos / 4; ++i) {
            const int pp = pk + drow + 4 * i;
            Ds[drow + 4 * i][dcol] = (d_on && pp < p_end) ? dbase[(size_t)pp * p.cout] : 0.f;
        }
        for (int i = xrow; i < p.halo_rows; i += kTailThreads / 8) {
            const int q = pk - w - 1 + i;
            float xreg[8];
            if (x_on && q >= 0 && q < p.P) {
                const int n = q / p.ppi, qq = q - n * p.ppi;
                wgrad_load8<T, WIDE>(xbase + (long long)n * p.img_stride + (long long)qq * p.ld, xreg);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) xreg[j] = 0.f;
            }
            *reinterpret_cast<float4 *>(&Xs[i * kTailTileCin + xcol]) = make_float4(xreg[0], xreg[1], xreg[2], xreg[3]);
            *reinterpret_cast<float4 *>(&Xs[i * kTailTileCin + xcol + 4]) = make_float4(xreg[4], xreg[5], xreg[6], xreg[7]);
        }
        if (tid < kTailTilePos) {
            const int pp = pk + tid;
            int m = 0;
            if (pp < p_end) {
                const int n = pp / p.ppi, q = pp - n * p.ppi, r = q / w, x = q - r * w;
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int rr = r + t / 3 - 1, xx = x + t % 3 - 1;
                    if (rr >= 0 && rr < p.h && xx >= 0 && xx < w) m |= 1 << t;
                }
            }
            Ms[tid] = m;
        }
        __syncthreads();
        if (db_on) {
#pragma unroll
            for (int k = 0; k < kTailTilePos; ++k) dbsum += Ds[k][tid];
        }
#pragma unroll 4
        for (int kk = 0; kk < kTailTilePos; kk += 2) {
            const int k = kk + lk;
            const float a = Ds[k][wm * 32 + li];
            const int m = Ms[k];
            const float *xc = Xs + (k + w + 1) * kTailTileCin + wn * 32 + li;       // the centre tap's row
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float xv = xc[((t / 3 - 1) * w + (t % 3 - 1)) * kTailTileCin];     // rows k .. k + 2 w + 2: inside the halo
                const float b = (m >> t) & 1 ? xv : 0.f;
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
            }
        }
    }
    // C / D of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *slab = p.slab + (size_t)chunk * p.slab_stride;
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
    if (db_on && o0 + tid < p.cout) slab[(size_t)p.cout * orow + o0 + tid] = dbsum;
}

// dW3[e] = scale[o] * (the slabs' elements e added in chunk order), db likewise without the scale: every element of both is written,
// nothing is read from them
__global__ void __launch_bounds__(kAuxBlock) conv3x3_wgrad_reduce_kernel(const float *slab, const float *scale, int n_chunks, int row, int n_dw,
                                                                         int n_all, float *dw, float *db) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_all; e += (long long)gridDim.x * blockDim.x) {
        float s = slab[e];
        for (int k = 1; k < n_chunks; ++k) s += slab[(size_t)k * n_all + e];
        if (e < n_dw) dw[e] = scale ? scale[e / row] * s : s;
        else db[e - n_dw] = s;
    }
}

// adam_step_kernel (train.hip) for the block: the same update of W3 [cout3][9 * cin3] and beta, every operation float32 and rounded on
// its own, and in the same pass the block's packed form with the batch norm folded as the weight loader folds it (weights.cpp:
// fold_batch_norm, pack_weights), in float64 and rounded once to the plan's weight type:
//   pack[o][e] = T((double)w * scale64[o])        b'[o] = (float)((double)beta - (double)mean[o] * scale64[o])
__global__ void __launch_bounds__(kAuxBlock) tail_adam_kernel(const TailAdamParams q) {
#pragma clang fp contract(off)
    const AdamParams &p = q.a;
    const float om1 = 1.f - p.beta1, om2 = 1.f - p.beta2;
    const long long n = p.n_w + p.n_b;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const bool bias = i >= p.n_w;
        const long long j = bias ? i - p.n_w : i;
        float *w = bias ? p.b : p.w, *m = bias ? p.m_b : p.m_w, *v = bias ? p.v_b : p.v_w;
        const float g = (bias ? p.db : p.dw)[j];
        const float mm = p.beta1 * m[j] + om1 * g;
        const float vv = p.beta2 * v[j] + om2 * (g * g);
        const float wv = w[j] - (p.lr_t * mm) / (sqrtf(vv) + p.eps);
        m[j] = mm;
        v[j] = vv;
        w[j] = wv;
        if (bias) {
            const double prod = (double)q.mean[j] * q.scale64[j];
            p.pack_b[j] = (float)((double)wv - prod);
        } else {
            const long long o = j / p.pack_cin, e = o * p.pack_row + (j - o * p.pack_cin);
            // (fp16: ONE rounding, from the float64 product -- the bytes of the weight loader, whose two truncations the host compiler
            // folds into one; rounding to float32 first differs in about one element of 30 000)
            const double f = (double)wv * q.scale64[o];
            if (p.pack_f16) static_cast<_Float16 *>(p.pack_w)[e] = (_Float16)f;
            else static_cast<float *>(p.pack_w)[e] = (float)f;
        }
    }
}

hipError_t launch_tail_adam(const TailAdamParams &p, hipStream_t s) {
    long long blocks = (p.a.n_w + p.a.n_b + kAuxBlock - 1) / kAuxBlock;
    if (blocks > kAuxGrid) blocks = kAuxGrid;
    hipLaunchKernelGGL(tail_adam_kernel, dim3((unsigned)blocks), dim3(kAuxBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_conv3x3_wgrad(const Wgrad3x3Params &p, int x_dtype, hipStream_t s) {
    const dim3 grid((unsigned)(p.tiles_cout * p.tiles_cin), (unsigned)p.n_chunks);
    const size_t lds = (size_t)p.halo_rows * kTailTileCin * sizeof(float);
    const int esz = x_dtype == YOLO_DTYPE_F16 ? 2 : 4, epc = 16 / esz;
    const bool wide = (uintptr_t)p.x % 16 == 0 && p.ld % epc == 0 && p.coff % epc == 0 && p.img_stride % epc == 0;
    if (x_dtype == YOLO_DTYPE_F16) {
        if (wide) hipLaunchKernelGGL((conv3x3_wgrad_kernel<_Float16, true>), grid, dim3(kTailThreads), lds, s, p);
        else hipLaunchKernelGGL((conv3x3_wgrad_kernel<_Float16, false>), grid, dim3(kTailThreads), lds, s, p);
    } else {
        if (wide) hipLaunchKernelGGL((conv3x3_wgrad_kernel<float, true>), grid, dim3(kTailThreads), lds, s, p);
        else hipLaunchKernelGGL((conv3x3_wgrad_kernel<float, false>), grid, dim3(kTailThreads), lds, s, p);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int row = 9 * p.cin, n_dw = p.cout * row, n_all = n_dw + p.cout;
    int blocks = (n_all + kAuxBlock - 1) / kAuxBlock;
    if (blocks > kAuxGrid) blocks = kAuxGrid;
    hipLaunchKernelGGL(conv3x3_wgrad_reduce_kernel, dim3(blocks), dim3(kAuxBlock), 0, s, p.slab, p.scale, p.n_chunks, row, n_dw, n_all, p.dw, p.db);
    return hipGetLastError();
}

}  // namespace yolo

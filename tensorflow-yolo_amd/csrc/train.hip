// Training the detection layer on the device (include/yolo_hip.h: yolo_conv1x1_wgrad, yolo_adam_step, yolo_net_train_head_step; the
// definitions are there).
//
// head_wgrad_kernel    the backward pass of the last conv (1 x 1, stride 1, linear, with bias: net/v2.py:52-56) with respect to its kernel and
//                      bias, what AdamOptimizer.minimize (net/v2.py:205) asks tf.gradients for: dW[o][c] = S_p G[p][o] X[p][c],
//                      db[o] = S_p G[p][o], one chunk of positions per workgroup, into a float32 slab.
// head_wgrad_reduce_kernel   adds the slabs in chunk order into dW and db.
// adam_step_kernel     tf.train.AdamOptimizer's update (net/v2.py:205) of the float32 master weights, and in the same pass the layer's
//                      packed form for the next forward.
// Compiled with default NaN handling, like loss.hip.
#include <hip/hip_runtime.h>

#include "wgrad_load.h"
#include "yolo_internal.h"

namespace yolo {

typedef float f32x16 __attribute__((ext_vector_type(16)));

static_assert(kWgradThreads == 256 && kWgradTileCout == 64 && kWgradTileCin == 128 && kWgradTilePos == 16, "the loader and wave maps below are written for these");

// Grid (tiles_cout * tiles_cin, n_chunks), 256 threads.  A workgroup owns a 64 (cout) x 128 (cin) tile of dW and the positions
// [chunk * ppc, min(P, (chunk + 1) * ppc)), 16 at a time:
//   load     G[16 positions][64 couts] (4 floats a thread, a row of 64 couts per wave) and X[16 positions][128 channels] (8 channels a
//            thread) from global memory into registers, one stage ahead of the products; rows behind the chunk and columns behind
//            cout / cin are zeros, never read
//   LDS      both tiles as they lie in memory, [position][cout] and [position][channel], float32: the reduction index is the slow one
//            of both, which is what the float32 MFMA wants -- lane l of v_mfma_f32_32x32x2_f32 holds A[l & 31][k = l >> 5] and
//            B[k = l >> 5][l & 31], so a wave reads 32 consecutive floats of row k and 32 of row k + 1: ds_read_b32 serves each half
//            wave from 32 different banks
//   MFMA     wave (wm, wn) of 2 x 2 computes 32 couts x 64 channels in two accumulators; float32 products, float32 sums, positions in
//            ascending order
//   db       in the workgroups of the first cin tile, thread t < 64 adds column t of the G tile, positions in ascending order
// The sums go to slab[chunk][cout][cin] and slab[chunk][cout * cin + cout]; every element of a chunk's slab is written.
template <typename T, bool WIDE>
__global__ void __launch_bounds__(kWgradThreads) head_wgrad_kernel(const WgradParams p) {
    __shared__ __attribute__((aligned(16))) float Gs[kWgradTilePos][kWgradTileCout];
    __shared__ __attribute__((aligned(16))) float Xs[kWgradTilePos][kWgradTileCin];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tn = blockIdx.x % p.tiles_cin, tm = blockIdx.x / p.tiles_cin, chunk = blockIdx.y;
    const int o0 = tm * kWgradTileCout, c0 = tn * kWgradTileCin;
    const int p_begin = chunk * p.ppc;
    const int p_end = p.P - p_begin < p.ppc ? p.P : p_begin + p.ppc;
    const int gcol = tid & 63, grow = tid >> 6;             // G: rows grow, grow + 4, grow + 8, grow + 12
    const int xrow = tid >> 4, xcol = (tid & 15) * 8;       // X: one row, 8 channels
    const bool g_on = o0 + gcol < p.cout, x_on = c0 + xcol < p.cin;     // (cin % 8 == 0: all 8 channels or none)
    const T *xbase = static_cast<const T *>(p.x) + p.coff + c0 + xcol;
    const float *gbase = p.g + o0 + gcol;
    float greg[4], xreg[8];
    auto load = [&](int pk) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pp = pk + grow + 4 * i;
            greg[i] = (g_on && pp < p_end) ? gbase[(size_t)pp * p.cout] : 0.f;
        }
        const int pp = pk + xrow;
        if (x_on && pp < p_end) {
            const int n = pp / p.ppi, q = pp - n * p.ppi;
            wgrad_load8<T, WIDE>(xbase + (long long)n * p.img_stride + (long long)q * p.ld, xreg);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) xreg[j] = 0.f;
        }
    };
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lk = lane >> 5;
    f32x16 acc0 = {0}, acc1 = {0};
    float dbsum = 0.f;
    const bool db_on = tn == 0 && tid < kWgradTileCout;
    load(p_begin);
    for (int pk = p_begin; pk < p_end; pk += kWgradTilePos) {
        __syncthreads();        // the products of the stage before are done with the tiles
#pragma unroll
        for (int i = 0; i < 4; ++i) Gs[grow + 4 * i][gcol] = greg[i];
        *reinterpret_cast<float4 *>(&Xs[xrow][xcol]) = make_float4(xreg[0], xreg[1], xreg[2], xreg[3]);
        *reinterpret_cast<float4 *>(&Xs[xrow][xcol + 4]) = make_float4(xreg[4], xreg[5], xreg[6], xreg[7]);
        __syncthreads();
        if (pk + kWgradTilePos < p_end) load(pk + kWgradTilePos);
        if (db_on) {
#pragma unroll
            for (int k = 0; k < kWgradTilePos; ++k) dbsum += Gs[k][tid];
        }
#pragma unroll
        for (int kk = 0; kk < kWgradTilePos; kk += 2) {
            const float a = Gs[kk + lk][wm * 32 + li];
            const float b0 = Xs[kk + lk][wn * 64 + li], b1 = Xs[kk + lk][wn * 64 + 32 + li];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
        }
    }
    // C / D of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    float *slab = p.slab + (size_t)chunk * p.slab_stride;
    const int c = c0 + wn * 64 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = o0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (o < p.cout) {
            if (c < p.cin) slab[(size_t)o * p.cin + c] = acc0[r];
            if (c + 32 < p.cin) slab[(size_t)o * p.cin + c + 32] = acc1[r];
        }
    }
    if (db_on && o0 + tid < p.cout) slab[(size_t)p.cout * p.cin + o0 + tid] = dbsum;
}

// dW[e] and db[e] = the slabs' elements e added in chunk order: every element of both is written, nothing is read from them
__global__ void __launch_bounds__(kAuxBlock) head_wgrad_reduce_kernel(const float *slab, int n_chunks, int n_dw, int n_all, float *dw, float *db) {
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n_all; e += gridDim.x * blockDim.x) {
        float s = slab[e];
        for (int k = 1; k < n_chunks; ++k) s += slab[(size_t)k * n_all + e];
        if (e < n_dw) dw[e] = s;
        else db[e - n_dw] = s;
    }
}

hipError_t launch_head_wgrad(const WgradParams &p, int x_dtype, hipStream_t s) {
    const dim3 grid((unsigned)(p.tiles_cout * p.tiles_cin), (unsigned)p.n_chunks);
    const int esz = x_dtype == YOLO_DTYPE_F16 ? 2 : 4, epc = 16 / esz;
    const bool wide = (uintptr_t)p.x % 16 == 0 && p.ld % epc == 0 && p.coff % epc == 0 && p.img_stride % epc == 0;
    if (x_dtype == YOLO_DTYPE_F16) {
        if (wide) hipLaunchKernelGGL((head_wgrad_kernel<_Float16, true>), grid, dim3(kWgradThreads), 0, s, p);
        else hipLaunchKernelGGL((head_wgrad_kernel<_Float16, false>), grid, dim3(kWgradThreads), 0, s, p);
    } else {
        if (wide) hipLaunchKernelGGL((head_wgrad_kernel<float, true>), grid, dim3(kWgradThreads), 0, s, p);
        else hipLaunchKernelGGL((head_wgrad_kernel<float, false>), grid, dim3(kWgradThreads), 0, s, p);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int n_dw = p.cout * p.cin, n_all = n_dw + p.cout;
    int blocks = (n_all + kAuxBlock - 1) / kAuxBlock;
    if (blocks > kAuxGrid) blocks = kAuxGrid;
    hipLaunchKernelGGL(head_wgrad_reduce_kernel, dim3(blocks), dim3(kAuxBlock), 0, s, p.slab, p.n_chunks, n_dw, n_all, p.dw, p.db);
    return hipGetLastError();
}

// One thread per element, the weights first and the bias behind them.  Every operation is float32 and rounded on its own:
//   m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + (1 - beta2) * (g * g);  w = w - (lr_t * m) / (sqrt(v) + eps)
// with IEEE division and square root (hipcc's default for HIP).  pack_w / pack_b, if not null, receive the element in the layout the conv
// kernels read: row o of the 1 x 1 conv at o * pack_row elements, the plan's weight type (weights.cpp: pack_weights), float32 bias.
__global__ void __launch_bounds__(kAuxBlock) adam_step_kernel(const AdamParams p) {
#pragma clang fp contract(off)
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
            if (p.pack_b) p.pack_b[j] = wv;
        } else if (p.pack_w) {
            const long long o = j / p.pack_cin, e = o * p.pack_row + (j - o * p.pack_cin);
            if (p.pack_f16) static_cast<_Float16 *>(p.pack_w)[e] = (_Float16)wv;
            else static_cast<float *>(p.pack_w)[e] = wv;
        }
    }
}

hipError_t launch_adam_step(const AdamParams &p, hipStream_t s) {
    long long blocks = (p.n_w + p.n_b + kAuxBlock - 1) / kAuxBlock;
    if (blocks > kAuxGrid) blocks = kAuxGrid;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(kAuxBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace yolo

// The sparse data gradient of one YOLOv3 head conv on the device (include/yolo_hip.h: yolo_v3_head_dgrad; the definition is there).
//
// The gradient G of the v3 loss is sparse by construction: a row that is no winner holds at most its objectness element, a winner row
// (one per truth at most) is full.  So D_s = G_s W_s is, for all but a handful of positions, A products per element with the A objectness
// rows of W_s -- a streaming kernel: Y read once, D written once, one line of G per row.
// head3_dgrad_kernel   a thread owns eight consecutive channels of one position; the objectness rows of W of the workgroup's channel tile
//                      lie in LDS; a position with a winner row walks the 5 + C rows of that anchor out of L2.  One float32 fmaf chain per
//                      element, o ascending, then one multiply by the slope factor of the stored Y.
// Elements of G the assign table declares a structural zero are never read.  Compiled with default NaN handling, like train3.hip.
#include <hip/hip_runtime.h>

#include "train3_tail_host.h"
#include "wgrad_load.h"
#include "yolo_internal.h"

namespace yolo {

static_assert(kDgrad3Lane == 8, "wgrad_load8 loads eight channels; D goes out as two 16-byte stores");
static_assert(kDgrad3Threads % 64 == 0 && kDgrad3TileCin % kDgrad3Lane == 0 && kDgrad3TileCin / kDgrad3Lane <= kDgrad3Threads,
              "a position of a channel tile fits one workgroup");
static_assert(YOLO_MAX_ANCHORS == 8, "the anchors of a position are unrolled");

// Grid (tiles_cin * groups), 256 threads, na * tile_cin floats of dynamic LDS.  Workgroup b serves channel tile b % tiles_cin and the
// positions [g * ppw, min(P, (g + 1) * ppw)), g = b / tiles_cin, ppr at a time: thread t owns position t / tpp of the round and the
// channels c0 + 8 (t % tpp) .. + 8 (tpp = the tile's channels / 8, ppr = 256 / tpp).  The branch on a winner row is decided per position
// and anchor: the same in all lanes that share the position.  The sums are explicit fmaf calls: nothing for the compiler to contract or to split.
template <typename T, bool HAS_Y, bool WIDE>
__global__ void __launch_bounds__(kDgrad3Threads) head3_dgrad_kernel(const Dgrad3Params p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float wobj[];       // [na][tile_cin]: row a * (5 + C) + 4 of W, the tile's channels
    const int tid = threadIdx.x;
    const int tile = (int)blockIdx.x % p.tiles_cin, group = (int)blockIdx.x / p.tiles_cin;
    const int c0 = tile * p.tile_cin;
    const int width = p.cin - c0 < p.tile_cin ? p.cin - c0 : p.tile_cin;       // channels of this tile: a multiple of 8
    for (int i = tid * 4; i < p.na * width; i += kDgrad3Threads * 4) {
        const int a = i / width, cc = i - a * width;                            // (width % 4 == 0: the four floats lie in one row)
        *reinterpret_cast<float4 *>(&wobj[a * p.tile_cin + cc]) =
            *reinterpret_cast<const float4 *>(p.w + ((size_t)a * p.stride + 4) * p.cin + c0 + cc);
    }
    __syncthreads();
    // (a last tile narrower than tile_cin takes fewer threads a position and more positions a round: p.tpp and p.ppr are a full tile's)
    const int tpp = width / kDgrad3Lane, ppr = kDgrad3Threads / tpp;
    const int slot = tid / tpp, cl = (tid - slot * tpp) * kDgrad3Lane;
    if (slot >= ppr || cl >= width) return;         // (no barrier below)
    const int c = c0 + cl;
    const int p_begin = group * p.ppw;
    const int p_end = p.P - p_begin < p.ppw ? p.P : p_begin + p.ppw;
    for (int pp = p_begin + slot; pp < p_end; pp += ppr) {
        const int n = pp / p.ppi, q = pp - n * p.ppi;
        const size_t row = (size_t)n * p.rows + p.row0 + (size_t)q * p.na;      // the position's first row of G and of the table
        float yv[8];
        if constexpr (HAS_Y)
            wgrad_load8<T, WIDE>(static_cast<const T *>(p.y) + (long long)n * p.img_stride + (long long)q * p.ld + p.coff + c, yv);
        int entry[YOLO_MAX_ANCHORS];
        float g4[YOLO_MAX_ANCHORS];
#pragma unroll
        for (int a = 0; a < YOLO_MAX_ANCHORS; ++a) {        // (clamped: in bounds and unconditional, all in flight together)
            const int ac = a < p.na ? a : p.na - 1;
            entry[a] = p.assign[row + ac];
            g4[a] = p.g[(row + ac) * p.stride + 4];
        }
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
        for (int a = 0; a < YOLO_MAX_ANCHORS; ++a) {
            if (a >= p.na) break;
            if (entry[a] >= 0 && entry[a] < p.max_gt) {     // a winner row: every element of it, k ascending (k == 4 among them)
                const float *grow = p.g + (row + a) * p.stride;
                const float *wrow = p.w + (size_t)a * p.stride * p.cin + c;
#pragma unroll 4
                for (int k = 0; k < p.stride; ++k) {
                    const float g = grow[k];
                    float wv[8];
                    wgrad_load8<float, true>(wrow + (size_t)k * p.cin, wv);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(g, wv[j], acc[j]);
                }
            } else {
                const float4 w0 = *reinterpret_cast<const float4 *>(&wobj[a * p.tile_cin + cl]);
                const float4 w1 = *reinterpret_cast<const float4 *>(&wobj[a * p.tile_cin + cl + 4]);
                const float g = g4[a];
                acc[0] = __builtin_fmaf(g, w0.x, acc[0]); acc[1] = __builtin_fmaf(g, w0.y, acc[1]);
                acc[2] = __builtin_fmaf(g, w0.z, acc[2]); acc[3] = __builtin_fmaf(g, w0.w, acc[3]);
                acc[4] = __builtin_fmaf(g, w1.x, acc[4]); acc[5] = __builtin_fmaf(g, w1.y, acc[5]);
                acc[6] = __builtin_fmaf(g, w1.z, acc[6]); acc[7] = __builtin_fmaf(g, w1.w, acc[7]);
            }
        }
        if constexpr (HAS_Y) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = acc[j] * (yv[j] > 0.f ? 1.f : p.slope);
        }
        float4 *dst = reinterpret_cast<float4 *>(p.d + (size_t)pp * p.cin + c);
        dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
}

hipError_t launch_head3_dgrad(const Dgrad3Params &p, hipStream_t s) {
    const dim3 grid((unsigned)((long long)p.tiles_cin * p.groups)), block(kDgrad3Threads);
    const size_t lds = (size_t)p.na * p.tile_cin * sizeof(float);
    if (!p.y) {
        hipLaunchKernelGGL((head3_dgrad_kernel<float, false, false>), grid, block, lds, s, p);
    } else if (p.f16) {
        if (p.wide) hipLaunchKernelGGL((head3_dgrad_kernel<_Float16, true, true>), grid, block, lds, s, p);
        else hipLaunchKernelGGL((head3_dgrad_kernel<_Float16, true, false>), grid, block, lds, s, p);
    } else {
        if (p.wide) hipLaunchKernelGGL((head3_dgrad_kernel<float, true, true>), grid, block, lds, s, p);
        else hipLaunchKernelGGL((head3_dgrad_kernel<float, true, false>), grid, block, lds, s, p);
    }
    return hipGetLastError();
}

}  // namespace yolo

// Training augmentation of a uint8 batch (include/yolo_hip.h "Training augmentation on the device"): flips, a separable blur with
// fixed-point taps, per-pixel dropout and noise from Philox4x32-10, a horizontal shift -- one kernel, one launch for up to kAugPerLaunch
// images, the records by value in the kernel argument (AugmentParams, read with scalar loads: the index is the workgroup's).
//
// A workgroup of 256 threads produces a kAugTileRows x kAugTileCols tile of one OUTPUT image.  Output column x shows column u = x - tx of
// the image before the shift, so everything in front of the shift is computed in u:
//   load    rows y0 - R .. y0 + 32 + R, columns u0 - R .. u0 + 64 + R of the flipped image F (R = the image's radius, not the maximum:
//           an image without blur loads no halo) into LDS as bytes, the border reflected (101) and then clamped -- a clamped index is only
//           ever read on behalf of an output the shift or the image's edge discards.  Thread t owns byte column t of the LDS row (at most
//           246 of them), works out its source column once and walks the rows: every row is one coalesced read of the source.
//   pass 1  Hs = S_k taps[|k|] * F[y][u + k] for the 32 + 2 R rows and 64 columns, unrounded, into a 16-bit LDS plane (at most 65280)
//   pass 2  a thread owns runs of 4 pixels of a row: 12 channel values whose column of Hs it reads as three 8-byte LDS loads per row
//           (a run is 24 bytes, the lanes of a half-wave stand 6 banks apart: no two of their 64-bit reads meet on a bank), adds the rows
//           k and -k before the multiply, rounds, then dropout / noise per pixel and three dword stores.
// The source is read through the tile loads only and the destination is only written.  Per pixel at most two Philox calls (one at the
// reference's parameters, where the second noise step has d == 0): ~60 integer multiplies, nothing beside the LDS traffic of the blur.
#include "yolo_internal.h"
#include "philox.h"

namespace yolo {

namespace {

constexpr int TR = kAugTileRows, TC = kAugTileCols, RMAX = kAugMaxRadius;
constexpr int SRC_ROWS = TR + 2 * RMAX, SRC_COLS = TC + 2 * RMAX;
constexpr int SRC_PITCH = (SRC_COLS * 3 + 7) / 8 * 8;      // bytes of an LDS row of F
constexpr int HS_PITCH = TC * 3;                           // 16-bit values of an LDS row of Hs: 384 bytes, a run starts 8-byte aligned
static_assert(SRC_COLS * 3 <= 256, "one thread per byte column of the tile load");
static_assert(TR * (TC / 4) % 256 == 0 && TC % 4 == 0, "whole runs per thread");

// the noise of one step from two words: d = (s * q + 2^23) >> 24, s the sum of the four 16-bit halves less 131070
__device__ __forceinline__ int noise_delta(unsigned a, unsigned b, int q) {
    const int s = (int)((a & 0xffffu) + (a >> 16) + (b & 0xffffu) + (b >> 16)) - 131070;
    return (int)(((long long)s * q + (1LL << 23)) >> 24);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// index i of a line of n under the reflect-101 border, then clamped (see the head of this file)
__device__ __forceinline__ int reflect101(long long i, int n) {
    if (i < 0) i = -i;
    else if (i >= n) i = 2LL * (n - 1) - i;
    return (int)(i < 0 ? 0 : (i >= n ? n - 1 : i));
}

}  // namespace

__global__ void __launch_bounds__(256) augment_kernel(const AugmentParams p) {
    __shared__ unsigned char s_src[SRC_ROWS * SRC_PITCH];
    __shared__ __attribute__((aligned(8))) unsigned short s_hs[SRC_ROWS * HS_PITCH];
    const AugGeom &g = p.g[blockIdx.z];
    const int tid = threadIdx.x;
    const int h = p.h, w = p.w;
    const int y0 = blockIdx.y * TR, x0 = blockIdx.x * TC;
    const int R = g.radius, flags = g.flags;
    const int rows = TR + 2 * R, row_bytes = (TC + 2 * R) * 3;
    const size_t img = (size_t)blockIdx.z * (size_t)h * (size_t)w * 3u;
    const unsigned char *src = p.src + img;
    int t[RMAX + 1];
#pragma unroll
    for (int k = 0; k <= RMAX; ++k) t[k] = g.taps[k];

    // ---- load: byte column tid of every row
    if (tid < row_bytes) {
        const int c = tid / 3, ch = tid - 3 * c;
        int sx = reflect101((long long)x0 - g.tx - R + c, w);
        if (flags & AUG_FLIP_LR) sx = w - 1 - sx;
        const unsigned char *col = src + (size_t)sx * 3u + ch;
#pragma unroll 4
        for (int r = 0; r < rows; ++r) {
            int sy = reflect101((long long)y0 - R + r, h);
            if (flags & AUG_FLIP_UD) sy = h - 1 - sy;
            s_src[r * SRC_PITCH + tid] = col[(size_t)sy * (size_t)w * 3u];
        }
    }
    __syncthreads();

    // ---- pass 1: Hs[r][j] for the byte columns j of the tile itself (LDS byte column j + 3 R is its centre)
    for (int e = tid; e < rows * HS_PITCH; e += 256) {
        const int r = e / HS_PITCH, j = e - r * HS_PITCH;
        const unsigned char *c = s_src + r * SRC_PITCH + j + 3 * R;
        int acc = t[0] * c[0];
#pragma unroll
        for (int k = 1; k <= RMAX; ++k)
            if (k <= R) acc += t[k] * ((int)c[3 * k] + (int)c[-3 * k]);
        s_hs[e] = (unsigned short)acc;
    }
    __syncthreads();

    // ---- pass 2 and the per-pixel steps: runs of 4 pixels
    unsigned char *dst = p.dst + img;
#pragma unroll
    for (int i = 0; i < TR * (TC / 4) / 256; ++i) {
        const int q = tid + 256 * i;
        const int ry = q / (TC / 4), rx = (q - ry * (TC / 4)) * 4;
        const int y = y0 + ry, x = x0 + rx;
        if (y >= h || x >= w) continue;         // (w % 4 == 0: a run is inside the row or outside it)
        int acc[12];
        {
            const unsigned short *c = s_hs + (ry + R) * HS_PITCH + rx * 3;
            unsigned long long a[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) a[m] = reinterpret_cast<const unsigned long long *>(c)[m];
#pragma unroll
            for (int m = 0; m < 12; ++m) acc[m] = t[0] * (int)((a[m >> 2] >> (16 * (m & 3))) & 0xffffu);
#pragma unroll
            for (int k = 1; k <= RMAX; ++k) {
                if (k <= R) {
                    unsigned long long lo[3], hi[3];
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        lo[m] = reinterpret_cast<const unsigned long long *>(c - k * HS_PITCH)[m];
                        hi[m] = reinterpret_cast<const unsigned long long *>(c + k * HS_PITCH)[m];
                    }
#pragma unroll
                    for (int m = 0; m < 12; ++m)
                        acc[m] += t[k] * (int)(((lo[m >> 2] >> (16 * (m & 3))) & 0xffffu) + ((hi[m >> 2] >> (16 * (m & 3))) & 0xffffu));
                }
            }
        }
        unsigned v[12];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const long long u = (long long)x + px - g.tx;
            if (u < 0 || u >= w) {
                v[3 * px] = v[3 * px + 1] = v[3 * px + 2] = 0u;
                continue;
            }
            int b[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) b[ch] = (acc[3 * px + ch] + 32768) >> 16;
            const unsigned pos = (unsigned)y * (unsigned)w + (unsigned)u;
            int d = 0;
            if (flags & AUG_DRAW0) {
                unsigned o[4];
                philox4x32_10(pos, 0u, g.key0, g.key1, o);
                if (o[0] < g.drop_thr) b[0] = b[1] = b[2] = 0;
                d = noise_delta(o[1], o[2], g.q0);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) b[ch] = clamp255(b[ch] + g.loc0 + d);
            d = 0;
            if (flags & AUG_DRAW1) {
                unsigned o[4];
                philox4x32_10(pos, 1u, g.key0, g.key1, o);
                d = noise_delta(o[0], o[1], g.q1);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v[3 * px + ch] = (unsigned)clamp255(b[ch] + g.loc1 + d);
        }
        unsigned char *o = dst + ((size_t)y * (size_t)w + (size_t)x) * 3u;
        if (p.wide) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                reinterpret_cast<unsigned *>(o)[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = (unsigned char)v[k];
        }
    }
}

hipError_t launch_augment(const AugmentParams &p, int n, hipStream_t s) {
    if (n < 1 || n > kAugPerLaunch || p.h < 1 || p.w < 4 || (p.w & 3) || (long long)p.h * p.w > 0x7fffffffLL) return hipErrorInvalidValue;
    const long long gx = ((long long)p.w + TC - 1) / TC, gy = ((long long)p.h + TR - 1) / TR;
    if (gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)n), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace yolo

// Bandwidth kernels around the conv stack: input cast/pad, image resize (per image, and a batch of frames of any size in one launch) with the
// map of box records back to frame coordinates, max-pool (2x2, general stride-1 SAME, fused SPP block), and the generic strided
// element-wise fallback (standalone shortcut / upsample / reorg / concat-copy / f32 convert) the
// planner uses when a fusion into a conv epilogue is not possible.
#include "yolo_internal.h"
#include <cstring>
#include <type_traits>

namespace yolo {

typedef unsigned int uint4v __attribute__((ext_vector_type(4)));

// feed point of the graph (net/layers.py:106-109): float32 NHWC -> T NHWC with the channel count
// padded to one 16-byte chunk (zeros), so the first conv can run the chunked implicit GEMM.
// U8: the caller's tensor is uint8 (yolo_net_forward_u8), a byte u is float32(u / 255.) (u8_unit) where the float32 kernel has the float.
template <bool F32, bool U8>
__device__ __forceinline__ void prep_body(const PrepParams &p) {
    typedef typename std::conditional<F32, float, _Float16>::type T;
    typedef typename std::conditional<U8, unsigned char, float>::type TIn;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long px = (long long)blockIdx.x * blockDim.x + threadIdx.x; px < p.pixels; px += stride) {
        const TIn *src = reinterpret_cast<const TIn *>(p.in) + px * p.C;
        T *dst = reinterpret_cast<T *>(p.out) + px * p.Cpad;
        for (int c0 = 0; c0 < p.Cpad; c0 += 16 / (int)sizeof(T)) {
            T t[16 / sizeof(T)];
#pragma unroll
            for (int e = 0; e < 16 / (int)sizeof(T); ++e) {
                if constexpr (U8) t[e] = (c0 + e < p.C) ? (T)u8_unit(src[c0 + e]) : (T)0.f;
                else t[e] = (c0 + e < p.C) ? (T)src[c0 + e] : (T)0.f;
            }
            uint4v u;
            __builtin_memcpy(&u, t, 16);
            *reinterpret_cast<uint4v *>(dst + c0) = u;
        }
    }
}

template <bool F32>
__global__ void __launch_bounds__(256) prep_kernel(const PrepParams p) { prep_body<F32, false>(p); }
template <bool F32>
__global__ void __launch_bounds__(256) prep_u8_kernel(const PrepParams p) { prep_body<F32, true>(p); }

// net/layers.py:70-81.  stride 2: zero pad (0 before, 1 after) then 2x2 VALID -- the pad row/col is
// only read for odd H/W and then takes part in the max as 0.  stride 1: TF SAME, window clipped.
template <bool F32, bool VEC>
__global__ void __launch_bounds__(256) pool_kernel(const PoolParams p) {
    typedef typename std::conditional<F32, float, _Float16>::type T;
    constexpr int EPC = 16 / (int)sizeof(T);
    constexpr int STEP = VEC ? EPC : 1;
    const int cchunks = (p.C + STEP - 1) / STEP;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < p.total; w += stride) {
        const int cc = (int)(w % cchunks);
        long long t = w / cchunks;
        const int ox = (int)(t % p.Wo); t /= p.Wo;
        const int oy = (int)(t % p.Ho);
        const long long n = t / p.Ho;
        const int iy = oy * p.stride, ix = ox * p.stride;
        float best[STEP];
#pragma unroll
        for (int e = 0; e < STEP; ++e) best[e] = -INFINITY;
        const T *base = reinterpret_cast<const T *>(p.in) + n * p.in_img_stride + cc * STEP;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = iy + dy, x = ix + dx;
                if (y < p.H && x < p.W) {
                    const T *q = base + ((long long)y * p.W + x) * p.in_ld;
                    if (VEC) {
                        const uint4v u = *reinterpret_cast<const uint4v *>(q);
                        T tv[EPC];
                        __builtin_memcpy(tv, &u, 16);
#pragma unroll
                        for (int e = 0; e < STEP; ++e) best[e] = fmaxf(best[e], (float)tv[e]);
                    } else {
                        best[0] = fmaxf(best[0], (float)q[0]);
                    }
                } else if (p.stride == 2) {     // explicit zero padding takes part (layers.py:72-73)
#pragma unroll
                    for (int e = 0; e < STEP; ++e) best[e] = fmaxf(best[e], 0.f);
                }
            }
        T *o = reinterpret_cast<T *>(p.out) + n * p.out_img_stride + ((long long)oy * p.Wo + ox) * p.out_ld + cc * STEP;
        if (VEC) {
            T tv[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) tv[e] = (T)best[e];
            uint4v u;
            __builtin_memcpy(&u, tv, 16);
            *reinterpret_cast<uint4v *>(o) = u;
        } else {
            o[0] = (T)best[0];
        }
    }
}

// net/layers.py:70-81 at stride 1 with an ODD window (tf.layers.max_pooling2d, padding="SAME"): the window [i - r, i + r], r = (k - 1) / 2,
// clipped to the map -- padding never takes part, an all-negative map stays negative.  The plain form: one thread per (pixel, 16-byte
// channel chunk), k x k loads each; any view, scalar when a stride is not chunk-aligned.  The SPP block of YOLOv3-SPP runs spp_pool_kernel
// below where it applies and three launches of this one where it does not (float32 nets, maps above 32 x 32, unaligned views).
template <bool F32, bool VEC>
__global__ void __launch_bounds__(256) pool_same_kernel(const PoolParams p) {
    typedef typename std::conditional<F32, float, _Float16>::type T;
    constexpr int EPC = 16 / (int)sizeof(T);
    constexpr int STEP = VEC ? EPC : 1;
    const int cchunks = (p.C + STEP - 1) / STEP;
    const int r = p.ksize >> 1;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < p.total; w += stride) {
        const int cc = (int)(w % cchunks);
        long long t = w / cchunks;
        const int ox = (int)(t % p.W); t /= p.W;
        const int oy = (int)(t % p.H);
        const long long n = t / p.H;
        const int y0 = oy - r < 0 ? 0 : oy - r, y1 = oy + r > p.H - 1 ? p.H - 1 : oy + r;
        const int x0 = ox - r < 0 ? 0 : ox - r, x1 = ox + r > p.W - 1 ? p.W - 1 : ox + r;
        float best[STEP];
#pragma unroll
        for (int e = 0; e < STEP; ++e) best[e] = -INFINITY;
        const T *base = reinterpret_cast<const T *>(p.in) + n * p.in_img_stride + cc * STEP;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const T *q = base + ((long long)y * p.W + x) * p.in_ld;
                if (VEC) {
                    const uint4v u = *reinterpret_cast<const uint4v *>(q);
                    T tv[EPC];
                    __builtin_memcpy(tv, &u, 16);
#pragma unroll
                    for (int e = 0; e < STEP; ++e) best[e] = fmaxf(best[e], (float)tv[e]);
                } else {
                    best[0] = fmaxf(best[0], (float)q[0]);
                }
            }
        T *o = reinterpret_cast<T *>(p.out) + n * p.out_img_stride + ((long long)oy * p.W + ox) * p.out_ld + cc * STEP;
        if (VEC) {
            T tv[EPC];
#pragma unroll
            for (int e = 0; e < EPC; ++e) tv[e] = (T)best[e];
            uint4v u;
            __builtin_memcpy(&u, tv, 16);
            *reinterpret_cast<uint4v *>(o) = u;
        } else {
            o[0] = (T)best[0];
        }
    }
}

// max of eight fp16 values at a time: four packed instructions (max never rounds: the result is bit-exact whatever the order)
__device__ __forceinline__ uint4v pk_max8(const uint4v a, const uint4v b) {
    uint4v r;
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_pk_max_f16 %0, %1, %2" : "=v"(r.x) : "v"(a.x), "v"(b.x));
    asm("v_pk_max_f16 %0, %1, %2" : "=v"(r.y) : "v"(a.y), "v"(b.y));
    asm("v_pk_max_f16 %0, %1, %2" : "=v"(r.z) : "v"(a.z), "v"(b.z));
    asm("v_pk_max_f16 %0, %1, %2" : "=v"(r.w) : "v"(a.w), "v"(b.w));
#else
    r = a; (void)b;
#endif
    return r;
}

// The SPP block of YOLOv3-SPP (Darknet yolov3-spp.cfg: max-pools 5, 9 and 13 at stride 1 of one 512-channel tensor x, concatenated with x)
// as ONE launch: x is read once, the three pooled tensors are written once -- 4 tensor passes over HBM where three pool launches make 6.
//   * a workgroup owns one image x `slab` 16-byte channel chunks and keeps the H x W plane of each in LDS, twice (A, B): item i = pixel *
//     slab + chunk, 16 bytes each, consecutive lanes on consecutive 16-byte words in every pass (ds_read_b128 / ds_write_b128 without
//     bank conflicts: a shifted window is the same contiguous run of words);
//   * pools are separable (a row pass A -> B, a column pass B -> A) and they cascade: with windows clipped to the map and no padding
//     value, pool(4r+1) = pool(2r+1) o pool(2r+1) and pool(6r+1) = pool(2r+1) o pool(4r+1) exactly, because max is associative and idempotent
//     (the clipped window of a clipped window is the clipped wider window) -- so each level is 2 x (2r+1) LDS reads per item, 12r + 6 in all
//     against (6r+1)^2 + ... loads of the plain form;
//   * every level's column pass also stores the level's tensor: 16-byte stores into its own view (ld / coff / image stride: a channel
//     slice of the concat buffer or a tensor of its own).  Lanes whose chunk lies beyond C (last slab) load and store nothing.
// LDS: 2 x H W slab x 16 bytes <= 64 KiB (launch_spp picks slab); maps up to kSppMaxSide square.
template <int RAD>
__global__ void __launch_bounds__(256) spp_pool_kernel(const SppParams p) {
    extern __shared__ uint4v spp_lds[];
    const int n = blockIdx.y;
    const int sh = p.slab_shift;
    const int chunk0 = (int)blockIdx.x << sh;
    const int items = (p.H * p.W) << sh;
    const int row = p.W << sh;              // items per map row
    uint4v *A = spp_lds, *B = spp_lds + items;
    const _Float16 *in = reinterpret_cast<const _Float16 *>(p.in) + (long long)n * p.in_img_stride + chunk0 * 8;
    for (int i = threadIdx.x; i < items; i += 256) {
        const int s = i & (p.slab - 1), px = i >> sh;
        if (chunk0 + s < p.chunks) A[i] = *reinterpret_cast<const uint4v *>(in + (long long)px * p.in_ld + s * 8);
    }
    __syncthreads();
#pragma unroll
    for (int lvl = 0; lvl < 3; ++lvl) {
        for (int i = threadIdx.x; i < items; i += 256) {        // row pass
            const int px = i >> sh;
            const int x = px - (int)fdiv((uint32_t)px, p.dW) * p.W;
            uint4v v = A[i];
#pragma unroll
            for (int d = 1; d <= RAD; ++d) {
                if (x - d >= 0) v = pk_max8(v, A[i - (d << sh)]);
                if (x + d < p.W) v = pk_max8(v, A[i + (d << sh)]);
            }
            B[i] = v;
        }
        __syncthreads();
        _Float16 *out = reinterpret_cast<_Float16 *>(p.out[lvl]) + (long long)n * p.out_img_stride[lvl] + chunk0 * 8;
        const int out_ld = p.out_ld[lvl];
        for (int i = threadIdx.x; i < items; i += 256) {        // column pass + the level's tensor
            const int s = i & (p.slab - 1), px = i >> sh;
            const int y = (int)fdiv((uint32_t)px, p.dW);
            uint4v v = B[i];
#pragma unroll
            for (int d = 1; d <= RAD; ++d) {
                if (y - d >= 0) v = pk_max8(v, B[i - d * row]);
                if (y + d < p.H) v = pk_max8(v, B[i + d * row]);
            }
            if (lvl < 2) A[i] = v;
            if (chunk0 + s < p.chunks) *reinterpret_cast<uint4v *>(out + (long long)px * out_ld + s * 8) = v;
        }
        if (lvl < 2) __syncthreads();
    }
}

// Generic fallback, one element per thread: out[map(n,y,x)][c] = a[n,y,x,c] (+ b[n,y,x,c]).
// map: identity, nearest upsample x2 (layers.py:112-116) or block-major reorg x2 (layers.py:90-97).
template <bool F32>
__global__ void __launch_bounds__(256) eltwise_kernel(const EltParams p) {
    typedef typename std::conditional<F32, float, _Float16>::type T;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < p.total; w += stride) {
        const int c = (int)(w % p.C);
        long long t = w / p.C;
        const int x = (int)(t % p.W); t /= p.W;
        const int y = (int)(t % p.H);
        const long long n = t / p.H;
        const long long pa = n * p.a_img_stride + ((long long)y * p.W + x) * p.a_ld + c;
        float v = p.a_f32 ? reinterpret_cast<const float *>(p.a)[pa] : (float)reinterpret_cast<const T *>(p.a)[pa];
        if (p.b) {
            const float r = (float)reinterpret_cast<const T *>(p.b)[n * p.b_img_stride + ((long long)y * p.W + x) * p.b_ld + c];
            // the reference adds two tensors of type T: round the sum once in T
            v = v + r;
        }
        long long off[4];
        int npos = 1;
        if (p.outmode == OUT_NORMAL) {
            off[0] = n * p.out_img_stride + ((long long)y * p.W + x) * p.out_ld + c;
        } else if (p.outmode == OUT_UP2) {
            const long long W2 = 2LL * p.W;
            const long long b0 = n * p.out_img_stride + ((2LL * y) * W2 + 2LL * x) * p.out_ld + c;
            off[0] = b0; off[1] = b0 + p.out_ld; off[2] = b0 + W2 * p.out_ld; off[3] = b0 + (W2 + 1) * p.out_ld;
            npos = 4;
        } else {
            const int W2 = p.W >> 1;
            off[0] = n * p.out_img_stride + ((long long)(y >> 1) * W2 + (x >> 1)) * p.out_ld + ((y & 1) * 2 + (x & 1)) * p.C + c;
        }
        for (int q = 0; q < npos; ++q) {
            if (p.out_f32) reinterpret_cast<float *>(p.out)[off[q]] = v;
            else reinterpret_cast<T *>(p.out)[off[q]] = (T)v;
        }
    }
}

static inline unsigned grid_for(long long work) {
    long long g = (work + kAuxBlock - 1) / kAuxBlock;
    if (g > kAuxGrid) g = kAuxGrid;     // 16 blocks per CU, grid-stride the rest
    if (g < 1) g = 1;
    return (unsigned)g;
}

// Image preprocessing of the TEST loop (reference net/base.py:115-155: cv2.resize INTER_LINEAR stretch, BGR->RGB, / 255.):
// one thread per destination pixel.  8-bit INTER_LINEAR as OpenCV defines it (imgproc/resize.cpp): half-pixel centres,
// weights rounded to 11-bit fixed point, horizontal pass in int32, vertical pass
// ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2; then float32(v / 255.) (division in float64 like NumPy).
// (resize_coeff_at: the same with the caller's scale = (double)src / (double)dst -- frames_resize_kernel divides once for its four pixels)
__device__ __forceinline__ void resize_coeff_at(int d, int src, double scale, int &s0, int &s1, int &w0, int &w1) {
#pragma clang fp contract(off)
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    w0 = __float2int_rn((1.f - f) * 2048.f);        // cvRound: round half to even
    w1 = __float2int_rn(f * 2048.f);
    s0 = s;
    s1 = s + 1 < src ? s + 1 : src - 1;
}
__device__ __forceinline__ void resize_coeff(int d, int src, int dst, int &s0, int &s1, int &w0, int &w1) {
    resize_coeff_at(d, src, (double)src / (double)dst, s0, s1, w0, w1);
}

// OUT_U8: the 8-bit value itself goes to a uint8 destination (yolo_preprocess_resize_u8: the batch tensor of yolo_net_detect_u8)
template <bool OUT_U8>
__device__ __forceinline__ void resize_u8_body(const ResizeParams &p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)p.dst_h * p.dst_w) return;
    const int dy = (int)(i / p.dst_w), dx = (int)(i - (long long)dy * p.dst_w);
    int x0, x1, a0, a1, y0, y1, b0, b1;
    resize_coeff(dx, p.src_w, p.dst_w, x0, x1, a0, a1);
    resize_coeff(dy, p.src_h, p.dst_h, y0, y1, b0, b1);
    const unsigned char *r0 = p.src + (long long)y0 * p.src_row_bytes, *r1 = p.src + (long long)y1 * p.src_row_bytes;
    const bool same = p.src_h == p.dst_h && p.src_w == p.dst_w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int cs = p.swap_rb ? 2 - c : c;
        int v;
        if (same) {
            v = r0[x0 * 3 + cs];
        } else {
            const int h0 = (int)r0[x0 * 3 + cs] * a0 + (int)r0[x1 * 3 + cs] * a1;
            const int h1 = (int)r1[x0 * 3 + cs] * a0 + (int)r1[x1 * 3 + cs] * a1;
            v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
        if constexpr (OUT_U8) reinterpret_cast<unsigned char *>(p.dst)[i * 3 + c] = (unsigned char)v;
        else reinterpret_cast<float *>(p.dst)[i * 3 + c] = (float)((double)v / 255.);
    }
}
__global__ void __launch_bounds__(256) resize_u8_kernel(const ResizeParams p) { resize_u8_body<false>(p); }
__global__ void __launch_bounds__(256) resize_u8_to_u8_kernel(const ResizeParams p) { resize_u8_body<true>(p); }

hipError_t launch_resize(const ResizeParams &p, hipStream_t s, bool dst_u8) {
    const long long n = (long long)p.dst_h * p.dst_w;
    if (n <= 0 || p.src_h <= 0 || p.src_w <= 0 || (n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    if (dst_u8) hipLaunchKernelGGL(resize_u8_to_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

// The resize of a whole batch in one launch (yolo_preprocess_frames[_u8]): grid row y is frame y of the launch, whatever its size, pitch
// and alignment (FramesParams.f[y], read with scalar loads: the index is the workgroup's).  A thread produces a run of 4 consecutive
// destination pixels of one row -- 12 bytes, three dword stores, or 48 bytes of float32, three dwordx4 stores -- where resize_u8_kernel
// stores single bytes; dst_w % 4 == 0 keeps every run inside its row and aligned.  Inside the frame's new_h x new_w region at
// (off_y, off_x) a pixel is resize_u8_kernel's for the frame resized to (new_h, new_w): the same resize_coeff, the same integer passes
// (the row coefficients once per thread, the double division of the column scale once for the four pixels).  Outside it (letterbox) the
// byte 128, written without a read.  Stretch is new = dst, offsets 0.
template <bool OUT_U8>
__global__ void __launch_bounds__(256) frames_resize_kernel(const FramesParams p) {
    const int runs_per_row = p.dst_w >> 2;
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= (long long)p.dst_h * runs_per_row) return;
    const FrameGeom &g = p.f[blockIdx.y];
    const int dy = (int)(r / runs_per_row), dx0 = (int)(r - (long long)dy * runs_per_row) * 4;
    const int iy = dy - g.off_y;
    const bool row_in = iy >= 0 && iy < g.new_h;
    const bool same = g.src_h == g.new_h && g.src_w == g.new_w;
    int y0 = 0, y1 = 0, b0 = 0, b1 = 0;
    if (row_in) resize_coeff(iy, g.src_h, g.new_h, y0, y1, b0, b1);
    const unsigned char *r0 = g.src + (long long)y0 * g.src_row_bytes, *r1 = g.src + (long long)y1 * g.src_row_bytes;
    const double scale_x = (double)g.src_w / (double)g.new_w;
    unsigned v[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ix = dx0 + q - g.off_x;
        if (row_in && ix >= 0 && ix < g.new_w) {
            int x0, x1, a0, a1;
            resize_coeff_at(ix, g.src_w, scale_x, x0, x1, a0, a1);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int cs = g.swap_rb ? 2 - c : c;
                int t;
                if (same) {
                    t = r0[x0 * 3 + cs];
                } else {
                    const int h0 = (int)r0[x0 * 3 + cs] * a0 + (int)r0[x1 * 3 + cs] * a1;
                    const int h1 = (int)r1[x0 * 3 + cs] * a0 + (int)r1[x1 * 3 + cs] * a1;
                    t = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
                    t = t < 0 ? 0 : (t > 255 ? 255 : t);
                }
                v[q * 3 + c] = (unsigned)t;
            }
        } else {
            v[q * 3] = v[q * 3 + 1] = v[q * 3 + 2] = 128u;
        }
    }
    // element offset of the run: image blockIdx.y, row dy, pixel dx0
    const long long e = (((long long)blockIdx.y * p.dst_h + dy) * p.dst_w + dx0) * 3;
    if constexpr (OUT_U8) {
        unsigned char *o = reinterpret_cast<unsigned char *>(p.dst) + e;
        if (p.wide) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                reinterpret_cast<unsigned *>(o)[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = (unsigned char)v[k];
        }
    } else {
        typedef float float4v __attribute__((ext_vector_type(4)));
        float *o = reinterpret_cast<float *>(p.dst) + e;
        if (p.wide) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float4v f;
                f.x = u8_unit(v[4 * k]); f.y = u8_unit(v[4 * k + 1]); f.z = u8_unit(v[4 * k + 2]); f.w = u8_unit(v[4 * k + 3]);
                reinterpret_cast<float4v *>(o)[k] = f;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = u8_unit(v[k]);
        }
    }
}

hipError_t launch_frames_resize(const FramesParams &p, int n, hipStream_t s, bool dst_u8) {
    const long long runs = (long long)p.dst_h * (p.dst_w >> 2);
    if (n < 1 || n > kFramesPerLaunch || p.dst_h < 1 || p.dst_w < 4 || (p.dst_w & 3) || (runs + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 g((unsigned)((runs + 255) / 256), (unsigned)n), b(256);
    if (dst_u8) hipLaunchKernelGGL(frames_resize_kernel<true>, g, b, 0, s, p);
    else hipLaunchKernelGGL(frames_resize_kernel<false>, g, b, 0, s, p);
    return hipGetLastError();
}

// Box records of a detect call on a letterboxed batch, from network-input to frame coordinates, in place (yolo_boxes_to_frames): one
// workgroup per image, a thread per valid record.  float64 with one rounding to float32 each -- x * W is exact in float64 (24 + 12 bits),
// so contracting it into an FMA could not change a bit; it is switched off all the same.  One IEEE division, one narrowing: this file is
// compiled without fast-math, NumPy's float64 gives the same bits.  prob and class_idx are not touched, records behind the count neither.
__global__ void __launch_bounds__(256) boxes_to_frames_kernel(const RemapParams p) {
#pragma clang fp contract(off)
    const int img = blockIdx.x;
    const BoxGeom &g = p.g[img];
    int n = p.counts[img];
    n = n < 0 ? 0 : (n > p.max_boxes ? p.max_boxes : n);
    yolo_box *b = p.boxes + (long long)img * p.max_boxes;
    for (int k = threadIdx.x; k < n; k += 256) {
        const double x = b[k].x, y = b[k].y, w = b[k].w, h = b[k].h;
        b[k].x = (float)((x * (double)p.net_w - (double)g.off_x) / (double)g.new_w);
        b[k].y = (float)((y * (double)p.net_h - (double)g.off_y) / (double)g.new_h);
        b[k].w = (float)(w * (double)p.net_w / (double)g.new_w);
        b[k].h = (float)(h * (double)p.net_h / (double)g.new_h);
    }
}

hipError_t launch_boxes_to_frames(const RemapParams &p, int n, hipStream_t s) {
    if (n < 1 || n > kFramesPerLaunch || p.max_boxes < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(boxes_to_frames_kernel, dim3((unsigned)n), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_prep(const PrepParams &p, int dtype, hipStream_t s, bool in_u8) {
    if (in_u8) {
        if (dtype == YOLO_DTYPE_F16) hipLaunchKernelGGL(prep_u8_kernel<false>, dim3(grid_for(p.pixels)), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(prep_u8_kernel<true>, dim3(grid_for(p.pixels)), dim3(256), 0, s, p);
    } else if (dtype == YOLO_DTYPE_F16) hipLaunchKernelGGL(prep_kernel<false>, dim3(grid_for(p.pixels)), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(prep_kernel<true>, dim3(grid_for(p.pixels)), dim3(256), 0, s, p);
    return hipGetLastError();
}

// pool_kernel and pool_same_kernel: one host side.  kern[float32][vec]; the 16-byte-vector instantiation runs when the strides allow it
// (pool_vec_strides: what yolo_net_kernel_info reports from) and both pointers are aligned; p.total arrives as B*Ho*Wo pixels and
// leaves as work items.
typedef void (*PoolKernel)(const PoolParams);
static hipError_t launch_pool_with(PoolKernel const (&kern)[2][2], const PoolParams &p0, int dtype, hipStream_t s) {
    PoolParams p = p0;
    const int epc = dtype == YOLO_DTYPE_F16 ? 8 : 4;
    const bool vec = pool_vec_strides(p.C, p.in_ld, p.out_ld, p.in_img_stride, p.out_img_stride, epc) &&
                     ((uintptr_t)p.in % 16 == 0) && ((uintptr_t)p.out % 16 == 0);
    p.total *= vec ? p.C / epc : p.C;
    hipLaunchKernelGGL(kern[dtype != YOLO_DTYPE_F16][vec], dim3(grid_for(p.total)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_pool(const PoolParams &p, int dtype, hipStream_t s) {
    static const PoolKernel kern[2][2] = {{pool_kernel<false, false>, pool_kernel<false, true>}, {pool_kernel<true, false>, pool_kernel<true, true>}};
    return launch_pool_with(kern, p, dtype, s);
}

hipError_t launch_pool_same(const PoolParams &p, int dtype, hipStream_t s) {
    static const PoolKernel kern[2][2] = {{pool_same_kernel<false, false>, pool_same_kernel<false, true>},
                                          {pool_same_kernel<true, false>, pool_same_kernel<true, true>}};
    if (p.ksize < 3 || p.ksize > 13 || !(p.ksize & 1) || p.Ho != p.H || p.Wo != p.W) return hipErrorInvalidValue;
    return launch_pool_with(kern, p, dtype, s);
}

// 16-byte channel chunks per workgroup of spp_pool_kernel: as many as two copies of their planes fit 64 KiB of LDS, up to 8 (a 128-byte
// line per pixel), fewer while the launch would leave most CUs without a workgroup
int spp_slab(int H, int W, int chunks, int batch) {
    int slab = 8;
    while (slab > 1 && (long long)H * W * slab * 32 > 65536) slab >>= 1;
    while (slab > 1 && slab / 2 >= chunks) slab >>= 1;
    while (slab > 1 && (long long)batch * ((chunks + slab - 1) / slab) < 256) slab >>= 1;
    return slab;
}

hipError_t launch_spp(const SppParams &p0, int rad, int batch, hipStream_t s) {
    SppParams p = p0;
    if (p.H < 1 || p.W < 1 || p.H > kSppMaxSide || p.W > kSppMaxSide || p.chunks < 1 || batch < 1 || batch > 65535 || (rad != 1 && rad != 2))
        return hipErrorInvalidValue;
    if (p.in_ld % 8 || p.in_img_stride % 8 || (uintptr_t)p.in % 16) return hipErrorInvalidValue;
    for (int l = 0; l < 3; ++l)
        if (!p.out[l] || p.out_ld[l] % 8 || p.out_img_stride[l] % 8 || (uintptr_t)p.out[l] % 16) return hipErrorInvalidValue;
    p.slab = spp_slab(p.H, p.W, p.chunks, batch);
    p.slab_shift = p.slab == 8 ? 3 : p.slab == 4 ? 2 : p.slab == 2 ? 1 : 0;
    p.slabs = (p.chunks + p.slab - 1) / p.slab;
    p.dW = make_fastdiv((uint32_t)p.W);
    const size_t lds = (size_t)p.H * p.W * p.slab * 32;
    if (lds > 65536) return hipErrorInvalidValue;
    const dim3 g((unsigned)p.slabs, (unsigned)batch), b(256);
    if (rad == 1) hipLaunchKernelGGL(spp_pool_kernel<1>, g, b, lds, s, p);
    else hipLaunchKernelGGL(spp_pool_kernel<2>, g, b, lds, s, p);
    return hipGetLastError();
}

hipError_t launch_eltwise(const EltParams &p, int dtype, hipStream_t s) {
    const dim3 g(grid_for(p.total)), b(256);
    if (dtype == YOLO_DTYPE_F16) hipLaunchKernelGGL(eltwise_kernel<false>, g, b, 0, s, p);
    else hipLaunchKernelGGL(eltwise_kernel<true>, g, b, 0, s, p);
    return hipGetLastError();
}

// Split-K second pass: out = epilogue(sum over the K splits of the raw float32 accumulators), with the epilogue semantics of
// conv_common.h: + folded-BN bias -> leaky 0.1 -> + residual (no activation after the add) -> output index map (identity /
// nearest-upsample x2 / block-major reorg) -> T or float32; head convs also fill the compact objectness array.  One thread per
// (pixel, 4 couts); the slabs are a few MB and L2-resident.
template <bool F32>
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const ReduceParams p) {
    typedef typename std::conditional<F32, float, _Float16>::type T;
    typedef float float4v __attribute__((ext_vector_type(4)));
    const int groups = p.cout_pad >> 2;
    const long long total = (long long)p.M * groups;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
        const int m = (int)(idx / groups);
        const int c = (int)(idx - (long long)m * groups) * 4;
        if (c >= p.Cout) continue;
        const float *src = p.part + (size_t)m * p.cout_pad + c;
        float4v a = *reinterpret_cast<const float4v *>(src);
        for (int s = 1; s < p.ksplit; ++s) a += *reinterpret_cast<const float4v *>(src + (size_t)s * p.M * p.cout_pad);
        const int n = m / p.HoWo, rem = m - n * p.HoWo;
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        float v[4] = {a.x, a.y, a.z, a.w};
        const int nv = p.Cout - c < 4 ? p.Cout - c : 4;
        for (int i = 0; i < nv; ++i) {
            const float x = v[i] + p.bias[c + i];
            v[i] = p.leaky ? fmaxf(0.1f * x, x) : x;
        }
        if (p.res) {
            const T *rp = reinterpret_cast<const T *>(p.res) + (long long)n * p.res_img_stride + (long long)rem * p.res_ld + c;
            for (int i = 0; i < nv; ++i) v[i] += (float)rp[i];
        }
        long long off[4];
        int npos = 1;
        if (p.outmode == OUT_NORMAL) {
            off[0] = (long long)n * p.out_img_stride + (long long)rem * p.out_ld + c;
        } else if (p.outmode == OUT_UP2) {
            const long long W2 = 2LL * p.Wo;
            const long long base = (long long)n * p.out_img_stride + ((2LL * oy) * W2 + 2LL * ox) * p.out_ld + c;
            off[0] = base; off[1] = base + p.out_ld; off[2] = base + W2 * p.out_ld; off[3] = base + (W2 + 1) * p.out_ld;
            npos = 4;
        } else {
            const int W2 = p.Wo >> 1;
            off[0] = (long long)n * p.out_img_stride + ((long long)(oy >> 1) * W2 + (ox >> 1)) * p.out_ld + ((oy & 1) * 2 + (ox & 1)) * p.Cout + c;
        }
        for (int q = 0; q < npos; ++q) {
            if (p.out_f32) {
                float *op = reinterpret_cast<float *>(p.out) + off[q];
                for (int i = 0; i < nv; ++i) op[i] = v[i];
            } else {
                T *op = reinterpret_cast<T *>(p.out) + off[q];
                for (int i = 0; i < nv; ++i) op[i] = (T)v[i];
            }
        }
        if (p.obj_out) {
            for (int i = 0; i < nv; ++i) {
                const int a_ = (c + i) / p.obj_width;
                if (c + i - a_ * p.obj_width == 4) p.obj_out[n * p.obj_rows + p.obj_row0 + rem * p.obj_na + a_] = v[i];
            }
        }
    }
}

// the reduce pass of a conv launched with p.ksplit > 1 into p.part: the epilogue fields of its parameters
ReduceParams reduce_params(const ConvParams &p) {
    ReduceParams r;
    memset(&r, 0, sizeof r);
    r.part = p.part; r.bias = p.bias; r.res = p.has_res ? p.res : nullptr; r.out = p.out;
    r.obj_out = p.obj_out; r.obj_width = p.obj_width; r.obj_rows = p.obj_rows; r.obj_row0 = p.obj_row0; r.obj_na = p.obj_na;
    r.ksplit = p.ksplit; r.M = p.M; r.Cout = p.Cout; r.cout_pad = p.cout_pad; r.HoWo = p.HoWo; r.Wo = p.Wo;
    r.out_ld = p.out_ld; r.res_ld = p.res_ld; r.leaky = p.leaky; r.outmode = p.outmode; r.out_f32 = p.out_f32; r.f32 = p.f32;
    r.out_img_stride = p.out_img_stride; r.res_img_stride = p.res_img_stride;
    return r;
}

hipError_t launch_splitk_reduce(const ReduceParams &p, hipStream_t s) {
    if (p.ksplit < 2 || !p.part || (p.cout_pad & 3) || p.M <= 0) return hipErrorInvalidValue;
    const dim3 g(grid_for((long long)p.M * (p.cout_pad >> 2))), b(256);
    if (p.f32) hipLaunchKernelGGL(splitk_reduce_kernel<true>, g, b, 0, s, p);
    else hipLaunchKernelGGL(splitk_reduce_kernel<false>, g, b, 0, s, p);
    return hipGetLastError();
}

// the names rocprofv3's kernel trace prints (yolo_kernel_info.symbol)
std::string aux_symbol(int kind, int dtype, bool vec) {
    const char *f = dtype == YOLO_DTYPE_F16 ? "false" : "true";
    if (kind == K_PREP) return std::string("void yolo::prep_kernel<") + f + ">(yolo::PrepParams)";
    if (kind == K_POOL) return std::string("void yolo::pool_kernel<") + f + ", " + (vec ? "true" : "false") + ">(yolo::PoolParams)";
    return std::string("void yolo::eltwise_kernel<") + f + ">(yolo::EltParams)";
}
std::string pool_same_symbol(int dtype, bool vec) {
    return std::string("void yolo::pool_same_kernel<") + (dtype == YOLO_DTYPE_F16 ? "false" : "true") + ", " + (vec ? "true" : "false") + ">(yolo::PoolParams)";
}
std::string spp_pool_symbol(int rad) { return "void yolo::spp_pool_kernel<" + std::to_string(rad) + ">(yolo::SppParams)"; }

}  // namespace yolo

// 3x3 / stride-1 implicit-GEMM conv on the block-scaled fp8 matrix cores (MXFP8 plans, yolo_net_options.dtype = YOLO_DTYPE_MXF8).
//
// Operands follow OCP MX v1.0 with e4m3fn elements and one E8M0 scale per 32 input channels:
//   scale exponent e = floor(log2 amax) - 8 (8 = emax of e4m3), elements e4m3fn(v * 2^-e) rounded to nearest even and clamped to
//   +-448 before the conversion; amax = 0 gives the smallest scale (byte 0) and zero elements.
// Weights are quantized once on the host (weights.cpp: pack_weights, mx_pack); activations stay fp16 in HBM and are quantized here,
// one block per (pixel, 32 channels), by the same device function yolo_mx_quantize runs.
//
// Tiling: a workgroup owns 128 couts x 256 positions of the padded-linear grid of conv_tap.hip (one shared pad column after every
// image row, one pad row after every image: tap (kh, kw) of position q is q + (kh-1)(W+1) + (kw-1)).  For each 128-channel slice the
// 256 + 2(W+1) + 2 patch positions around the tile are read ONCE (fp16), quantized and written to LDS (128 bytes + 4 scale bytes per
// position); all nine taps read their B operand from it at a row shift.  The next slice's patch is quantized into the second LDS
// buffer a third at a time between the kernel rows of the current one; one barrier per slice.
// 8 waves = 4 (couts) x 2 (positions); a wave owns 32 couts x 128 positions = 2 x 8 tiles of v_mfma_scale_f32_16x16x128_f8f6f4.
// Fragment b of a wave holds positions m_wave + 8 fr + b (fr = lane & 15), so the three taps of a kernel row read ten position
// fragments instead of 24.  Weights come straight from global memory (L2) into registers, pre-arranged by the packer as one
// 2 KiB fragment per (32 couts, tap, slice, cout tile) plus 64 scale bytes, requested for the next kernel row before the current one ends.
//
// Lane map of v_mfma_scale_f32_16x16x128_f8f6f4 (measured on the MI355X with random e4m3 data and per-lane scales): lane l holds row
// (A) / column (B) l & 15; its bytes 0-15 are k = 16 g .. 16 g + 15 and bytes 16-31 are k = 64 + 16 g .., g = l >> 4; the scale of
// K block b (k = 32 b .. 32 b + 31) is the scale operand of lane group b.  With 32-channel block b = K block b, lane group g therefore
// reads the 16-byte chunks g and g + 4 of a 128-channel row (halves of blocks g >> 1 and 2 + (g >> 1)) and passes the scale of block g.
#include "conv_common.h"

namespace yolo {

namespace {

typedef int int8v __attribute__((ext_vector_type(8)));
typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));

constexpr int kMxNB = 256;                 // positions per workgroup
constexpr int kMxRowBytes = 128;           // one 128-channel slice of a position, e4m3
constexpr int kMxPatchRows = kMxNB + 2 * (kMxMaxW + 1) + 2;
constexpr int kMxBufBytes = kMxPatchRows * kMxRowBytes + 4 * kMxPatchRows;     // elements + scale bytes [4 blocks][rows]

// 16-byte chunk c of patch row r sits at chunk c ^ ((r ^ (r >> 3)) & 6): the 16 lanes of a fragment read rows 8 apart
__device__ __forceinline__ int mx_swz(int r) { return (r ^ (r >> 3)) & 6; }

}  // namespace

// One MX block: 32 fp16 values (four 16-byte chunks) -> 32 e4m3fn bytes + the E8M0 scale byte.
__device__ __forceinline__ uint32_t mx_quant_block(const uint4v (&v)[4], uint4v (&q)[2]) {
    ushort2v m = {0, 0};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const ushort2v h = __builtin_bit_cast(ushort2v, v[c][e] & 0x7fff7fffu);      // |x| as bits: ordered like the values
            m = __builtin_elementwise_max(m, h);
        }
    const unsigned short mb = m[0] > m[1] ? m[0] : m[1];
    const float amax = (float)__builtin_bit_cast(_Float16, mb);
    int eb = 0;                            // biased E8M0 exponent; 0 (2^-127) for an all-zero block
    float mul = 1.0f;
    if (mb != 0) {
        eb = (int)((__builtin_bit_cast(uint32_t, amax) >> 23) & 0xff) - 127 - 8 + 127;      // floor(log2 amax) - 8, biased
        eb = eb < 1 ? 1 : eb > 254 ? 254 : eb;
        mul = __builtin_bit_cast(float, (uint32_t)(254 - eb) << 23);                        // 2^-e
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            float f[4];
#pragma unroll
            for (int hw = 0; hw < 2; ++hw) {
                const uint32_t u = v[c][2 * w + hw];
                f[2 * hw] = fminf(fmaxf((float)__builtin_bit_cast(_Float16, (unsigned short)(u & 0xffff)) * mul, -448.0f), 448.0f);
                f[2 * hw + 1] = fminf(fmaxf((float)__builtin_bit_cast(_Float16, (unsigned short)(u >> 16)) * mul, -448.0f), 448.0f);
            }
            int r = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);      // bytes 0, 1
            r = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], r, true);          // bytes 2, 3
            q[c >> 1][(c & 1) * 2 + w] = (uint32_t)r;
        }
    return (uint32_t)eb;
}

namespace {

__global__ void __launch_bounds__(256) mx_quantize_kernel(const _Float16 *src, int rows, int blocks_per_row, unsigned char *q, unsigned char *sc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)rows * blocks_per_row) return;
    const uint4v *s = reinterpret_cast<const uint4v *>(src + i * 32);
    uint4v v[4] = {s[0], s[1], s[2], s[3]}, o[2];
    sc[i] = (unsigned char)mx_quant_block(v, o);
    uint4v *d = reinterpret_cast<uint4v *>(q + i * 32);
    d[0] = o[0];
    d[1] = o[1];
}

// fp16 patch item (position p of the patch, 32-channel block g of slice s): load
__device__ __forceinline__ void mx_item_load(const ConvParams &p, int qs, int np, int s, int item, uint4v (&v)[4]) {
    const int r = item >> 2, g = item & 3;
    const int q = qs + r;
    bool ok = item < 4 * np && q >= 0 && q < p.Mq;
    int n = 0, y = 0, x = 0;
    if (ok) {
        n = (int)fdiv((uint32_t)q, p.dqHW);
        const int rr = q - n * p.qHW;
        y = (int)fdiv((uint32_t)rr, p.dqW);
        x = rr - y * p.qW;
        ok = y < p.H && x < p.W;
    }
    if (ok) {
        const uint4v *src = reinterpret_cast<const uint4v *>(reinterpret_cast<const _Float16 *>(p.in) + (long long)n * p.in_img_stride +
                                                               (long long)(y * p.W + x) * p.in_ld + p.in_coff + s * 128 + g * 32);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = src[c];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = uint4v{0, 0, 0, 0};
    }
}

// ... quantize and store into the patch buffer
__device__ __forceinline__ void mx_item_store(unsigned char *buf, int np, int item, const uint4v (&v)[4]) {
    if (item >= 4 * np) return;
    const int r = item >> 2, g = item & 3;
    uint4v o[2];
    const uint32_t sc = mx_quant_block(v, o);
    unsigned char *row = buf + r * kMxRowBytes;
    const int sw = mx_swz(r);
    *reinterpret_cast<uint4v *>(row + ((2 * g) ^ sw) * 16) = o[0];
    *reinterpret_cast<uint4v *>(row + ((2 * g + 1) ^ sw) * 16) = o[1];
    buf[kMxPatchRows * kMxRowBytes + g * kMxPatchRows + r] = (unsigned char)sc;
}

}  // namespace

template <bool FAST>
__global__ void __launch_bounds__(512, 1) conv3x3_mx_kernel(const ConvParams p) {
    constexpr int TM = 2, TP = 8;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kMxBufBytes];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 3, wn = wave >> 2;
    const int fr = lane & 15, g = lane >> 4;
    const int bid = blockIdx.x;
    const int tile_m = (int)fdiv((uint32_t)bid, p.dtiles_n);
    const int tile_c = bid - tile_m * p.n_tiles_n;
    const int q0 = tile_m * kMxNB;
    const int qs = q0 - p.qW - 1;                  // patch row 0 = position q0 - (W+1) - 1
    const int np = kMxNB + 2 * p.qW + 2;
    const int S = p.kunits;                        // 128-channel slices
    const int G = tile_c * 4 + wm;                 // 32-cout group of this wave
    const int cbase = G * 32 + g * 8;              // a lane's 8 contiguous couts (conv_epilogue's contract with TM = 2)
    const int m_wave = wn * 128;

    float4v acc[TM][TP];
    conv_init_acc_bias<TM, TP>(p, acc, cbase);

    // weights: fragment (G, tap, s, a) = 64 lanes x 32 bytes at ((((G * 9 + tap) * S + s) * 2 + a) * 64 + lane) * 32; scales one byte per lane
    const unsigned char *wq = reinterpret_cast<const unsigned char *>(p.wgt);
    const unsigned char *ws = wq + (size_t)p.cout_pad * 9 * (size_t)S * 128;
    auto load_tap = [&](int s, int kh, int kw, int8v (&A)[TM], int (&sA)[TM]) {
#pragma unroll
        for (int a = 0; a < TM; ++a) {
            const size_t f = (((size_t)G * 9 + kh * 3 + kw) * S + s) * 2 + a;
            A[a] = *reinterpret_cast<const int8v *>(wq + (f * 64 + lane) * 32);
            sA[a] = ws[f * 64 + lane];
        }
    };

    // prologue: slice 0 into buffer 0
    for (int item = tid; item < 4 * np; item += 512) {
        uint4v v[4];
        mx_item_load(p, qs, np, 0, item, v);
        mx_item_store(smem, np, item, v);
    }
    int8v A[3][TM];
    int sA[3][TM];
    for (int kw = 0; kw < 3; ++kw) load_tap(0, 0, kw, A[kw], sA[kw]);
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const unsigned char *buf = smem + (s & 1) * kMxBufBytes;
        unsigned char *nbuf = smem + ((s + 1) & 1) * kMxBufBytes;
        const bool more = s + 1 < S;
#pragma unroll 1
        for (int kh = 0; kh < 3; ++kh) {
            // a third of the next slice's patch in flight during this row; the next row's weights are requested early: tap 0 into A[0] as
            // soon as this row's last fragment that uses it is issued (f = TP - 1), taps 1 and 2 behind the patch store (registers)
            const int ns = kh < 2 ? s : s + 1, nkh = kh < 2 ? kh + 1 : 0;
            uint4v pv[4];
            if (more) mx_item_load(p, qs, np, s + 1, tid + 512 * kh, pv);
#pragma unroll
            for (int f = 0; f < TP + 2; ++f) {
                if (f == (TP + 2) / 2 && more) {       // half-way: the first item in, the second in flight
                    mx_item_store(nbuf, np, tid + 512 * kh, pv);
                    mx_item_load(p, qs, np, s + 1, tid + 512 * (kh + 3), pv);
                }
                const int r = m_wave + 8 * fr + f + kh * p.qW;
                const int sw = mx_swz(r);
                const unsigned char *row = buf + r * kMxRowBytes;
                const uint4v lo = *reinterpret_cast<const uint4v *>(row + (g ^ sw) * 16);           // (see the lane map above)
                const uint4v hi = *reinterpret_cast<const uint4v *>(row + ((g + 4) ^ sw) * 16);
                const int8v B = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                const int sB = buf[kMxPatchRows * kMxRowBytes + g * kMxPatchRows + r];
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int b = f - kw;
                    if (b < 0 || b >= TP) continue;
#pragma unroll
                    for (int a = 0; a < TM; ++a)
                        acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A[kw][a], B, acc[a][b], 0, 0, 0, sA[kw][a], 0, sB);
                }
                if (f == TP - 1 && ns < S) load_tap(ns, nkh, 0, A[0], sA[0]);
            }
            if (more) mx_item_store(nbuf, np, tid + 512 * (kh + 3), pv);
            if (ns < S) {
                load_tap(ns, nkh, 1, A[1], sA[1]);
                load_tap(ns, nkh, 2, A[2], sA[2]);
            }
        }
        __syncthreads();
    }
    if constexpr (FAST) conv_epilogue_fast<TM, TP, 1, true>(p, acc, cbase, q0 + m_wave, fr);
    else conv_epilogue<_Float16, TM, TP, 1, true, true>(p, acc, cbase, q0 + m_wave, fr);
}

bool conv_mx_fits(int W) { return W >= 1 && W <= kMxMaxW; }

const char *conv_mx_symbol(bool fast) {
    return fast ? "void yolo::conv3x3_mx_kernel<true>(yolo::ConvParams)" : "void yolo::conv3x3_mx_kernel<false>(yolo::ConvParams)";
}

// p: the launch parameters of make_conv_params (fp16 views); p.wgt = the MX weight image of mx_pack (weights.cpp)
hipError_t launch_conv_mx(const ConvParams &p0, hipStream_t s) {
    ConvParams p = p0;
    if (p.ksize != 3 || p.stride != 1 || p.f32 || p.H != p.Ho || p.W != p.Wo || !conv_mx_fits(p.W) || p.HoWo <= 0 || (p.cin_chunks * 8) % 128)
        return hipErrorInvalidValue;
    p.kunits = p.cin_chunks * 8 / 128;
    p.cout_pad = (p.Cout + 127) / 128 * 128;
    p.n_tiles_n = p.cout_pad / 128;
    p.qW = p.W + 1;
    p.qHW = (p.H + 1) * (p.W + 1);
    const long long mq = (long long)(p.M / p.HoWo) * p.qHW;
    const long long blocks = (mq + kMxNB - 1) / kMxNB * p.n_tiles_n;
    if (mq <= 0 || mq > 0x7fffffffLL || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    p.Mq = (int)mq;
    p.n_blocks = (int)blocks;
    p.ksplit = 1;
    conv_set_divisors(p, 1);
    p.fast_epi = conv_fast_epilogue_ok(p) ? 1 : 0;
    if (p.fast_epi) hipLaunchKernelGGL((conv3x3_mx_kernel<true>), dim3((unsigned)blocks), dim3(512), 0, s, p);
    else hipLaunchKernelGGL((conv3x3_mx_kernel<false>), dim3((unsigned)blocks), dim3(512), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_mx_quantize(const void *src, int rows, int channels, unsigned char *q, unsigned char *sc, hipStream_t s) {
    if (!src || !q || !sc || rows <= 0 || channels <= 0 || channels % 32) return hipErrorInvalidValue;
    const long long n = (long long)rows * (channels / 32);
    if (n > 0x7fffffffLL / 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mx_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const _Float16 *>(src), rows,
                       channels / 32, q, sc);
    return hipGetLastError();
}

}  // namespace yolo

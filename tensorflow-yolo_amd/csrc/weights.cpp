// Weight packing: the Darknet float stream -> the device blob the plan laid out (plan.cpp: Planner::weight_region), BatchNorm folded.
#include <cmath>
#include <cstring>

#include "yolo_internal.h"

namespace yolo {

// float -> e4m3fn, round to nearest even; |x| <= 448 (the caller clamps)
static unsigned char e4m3_rne(double x) {
    const unsigned char sign = std::signbit(x) ? 0x80 : 0;
    const double a = std::fabs(x);
    if (a < 0.015625) return sign | (unsigned char)std::nearbyint(a * 512.0);      // subnormal m * 2^-9 (m = 8: the smallest normal)
    int E;
    const double fr = std::frexp(a, &E);        // a = fr 2^E, fr in [0.5, 1)
    int e = E - 1, mant = (int)std::nearbyint((2.0 * fr - 1.0) * 8.0);
    if (mant == 8) { ++e; mant = 0; }
    return sign | (unsigned char)((e + 7) << 3) | (unsigned char)mant;
}

// the host twin of conv_mx.hip's mx_quant_block (OCP MX: e = floor(log2 amax) - 8, clamped to E8M0; elements RNE, saturated)
unsigned char mx_quant_block_host(const float *v, unsigned char *q) {
    float amax = 0.0f;
    for (int i = 0; i < 32; ++i) amax = std::fmax(amax, std::fabs(v[i]));
    if (amax == 0.0f) {
        for (int i = 0; i < 32; ++i) q[i] = 0;
        return 0;
    }
    int E;
    (void)std::frexp(amax, &E);
    int eb = (E - 1) - 8 + 127;
    eb = eb < 0 ? 0 : eb > 254 ? 254 : eb;
    const double mul = std::ldexp(1.0, 127 - eb);
    for (int i = 0; i < 32; ++i) {
        double x = (double)v[i] * mul;
        x = x > 448.0 ? 448.0 : x < -448.0 ? -448.0 : x;
        q[i] = e4m3_rne(x);
    }
    return (unsigned char)eb;
}

// conv_mx.hip weight image of one conv: for cout group G (32 couts), tap t, 128-channel slice s, cout tile a (0, 1) and lane l, the 32
// e4m3 values of the MFMA A operand at ((((G * 9 + t) * S + s) * 2 + a) * 64 + l) * 32 -- row R = l & 15 = cout 32 G + 8 (R >> 2) +
// 4 a + (R & 3); lane group g = l >> 4 holds channels 16 g .. 16 g + 15 and 64 + 16 g .. of the slice (conv_mx.hip: lane map) --, and
// the scale byte of 32-channel block g of that row at the same fragment index behind all elements
static void mx_pack(const Kernel &k, const float *kern, const std::vector<double> &scale, unsigned char *dst) {
    const int S = k.cin / 128, cout_pad = (k.cout + 127) / 128 * 128;
    unsigned char *sdst = dst + (size_t)cout_pad * 9 * k.cin;
    float v[32];
    unsigned char q[4][32], sc[4];
    for (int G = 0; G < cout_pad / 32; ++G)
        for (int t = 0; t < 9; ++t)
            for (int s = 0; s < S; ++s)
                for (int a = 0; a < 2; ++a)
                    for (int R = 0; R < 16; ++R) {
                        const int o = 32 * G + 8 * (R >> 2) + 4 * a + (R & 3);
                        for (int b = 0; b < 4; ++b) {
                            for (int j = 0; j < 32; ++j)
                                v[j] = o < k.cout ? (float)((double)kern[((size_t)o * k.cin + s * 128 + 32 * b + j) * 9 + t] * scale[o]) : 0.0f;
                            sc[b] = mx_quant_block_host(v, q[b]);
                        }
                        for (int g = 0; g < 4; ++g) {
                            const size_t f = ((((size_t)G * 9 + t) * S + s) * 2 + a) * 64 + 16 * g + R;
                            memcpy(dst + f * 32, q[g >> 1] + 16 * (g & 1), 16);
                            memcpy(dst + f * 32 + 16, q[2 + (g >> 1)] + 16 * (g & 1), 16);
                            sdst[f] = sc[g];
                        }
                    }
}

constexpr double kBnEps = 1e-5;        // net/layers.py:5

// One conv's head of the Darknet stream (net/layers.py:53-63; net/base.py:26-46) -- BN: beta, gamma, moving_mean, moving_variance;
// else bias -- folded: w' = w * gamma/sqrt(var+eps), b' = beta - mean*gamma/sqrt(var+eps),
// computed in float64 and rounded once.  Writes the float32 bias, yields the float64 scale per cout (1 without BN) and returns the
// kernel[out][in][kh][kw] that follows.
static const float *fold_batch_norm(const Kernel &k, const float *p, std::vector<double> &scale, float *bdst) {
    scale.assign((size_t)k.cout, 1.0);
    if (!k.batch_norm) {
        for (int o = 0; o < k.cout; ++o) bdst[o] = p[o];
        return p + k.cout;
    }
    const float *beta = p, *gamma = p + k.cout, *mean = p + 2 * k.cout, *var = p + 3 * k.cout;
    for (int o = 0; o < k.cout; ++o) {
        scale[o] = (double)gamma[o] / std::sqrt((double)var[o] + kBnEps);
        bdst[o] = (float)((double)beta[o] - (double)mean[o] * scale[o]);
    }
    return p + 4 * (size_t)k.cout;
}

// Darknet stream -> device layout: per conv the folded bias, then one of three weight layouts.
int pack_weights(const yolo_net *net, const float *host, size_t n, std::vector<unsigned char> &blob, std::string &err) {
    if (n != net->weight_count) {
        err = "weight stream holds " + std::to_string(n) + " values, the layer list needs " + std::to_string(net->weight_count);
        return YOLO_ERR_WEIGHTS;
    }
    blob.assign(net->weights_bytes, 0);
    const bool f16 = net->opt.dtype == YOLO_DTYPE_F16;
    std::vector<double> scale;
    for (const Kernel &k : net->kernels) {
        if (k.kind != K_FIRST && k.kind != K_CONV) continue;
        const float *kern = fold_batch_norm(k, host + k.w_src, scale, reinterpret_cast<float *>(blob.data() + k.b_off));
        if (k.kind == K_FIRST) {        // [27 = (kh,kw,cin)][cout] float32 (first.hip)
            float *wdst = reinterpret_cast<float *>(blob.data() + k.w_off);
            for (int o = 0; o < k.cout; ++o)
                for (int t = 0; t < 9; ++t)
                    for (int ci = 0; ci < 3; ++ci) {
                        float v = (float)((double)kern[((size_t)o * 3 + ci) * 9 + t] * scale[o]);
                        if (f16) v = (float)(_Float16)v;        // same operand rounding as the MFMA path
                        wdst[(t * 3 + ci) * k.cout + o] = v;
                    }
        } else if (k.mx) {              // weights folded in float64, rounded to float32, quantized to MXFP8 once
            if ((size_t)(k.cout + 127) / 128 * 128 * 9 * k.cin * 33 / 32 > k.w_bytes) {
                err = "MX weight image does not fit the conv's weight region";
                return YOLO_ERR_PLAN;
            }
            mx_pack(k, kern, scale, blob.data() + k.w_off);
        } else {                        // [cout_pad][K] rows, K = (kh,kw) major, cin minor; chunk = e / epc
            const int taps = k.ksize * k.ksize;
            const size_t wrow = (size_t)k.ktiles * 128;
            for (int o = 0; o < k.cout; ++o) {
                unsigned char *row = blob.data() + k.w_off + (size_t)o * wrow;
                for (int t = 0; t < taps; ++t)
                    for (int ci = 0; ci < k.cin; ++ci) {
                        const float v = (float)((double)kern[((size_t)o * k.cin + ci) * taps + t] * scale[o]);
                        const size_t e = (size_t)t * k.cin_s + ci;
                        if (f16) reinterpret_cast<_Float16 *>(row)[e] = (_Float16)v;
                        else reinterpret_cast<float *>(row)[e] = v;
                    }
            }
        }
    }
    return YOLO_OK;
}

}  // namespace yolo

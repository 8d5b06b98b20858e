// Device arithmetic that more than one translation unit runs on the head's values: the decode's sigmoid (detect.hip, loss.hip) and the
// float64 IoU of net/base.py:180-192 (eval.hip: matching; loss.hip: truth-to-anchor assignment).  One definition each, so that two
// kernels that are documented to compute "the same" value run the same instructions.
#pragma once
#include <hip/hip_runtime.h>

namespace yolo {

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.f / (1.f + expf(-x)); }   // base.py:171-172

// np.maximum / np.minimum: a NaN operand is the result (fmax / fmin would drop it)
__device__ __forceinline__ double np_max(double a, double b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ double np_min(double a, double b) { return (a <= b || a != a) ? a : b; }

// net/base.py:180-192 with float64 operands, every operation rounded on its own as NumPy rounds it.  w1 * h1 and w2 * h2 are exact
// (float32-valued factors), but iw and ih are float64 differences and iw * ih is rounded in general: an FMA that took the unrounded
// product into the union would change its low bits (boxes at a frame edge, centre << extent).  So no contraction in this function.
__device__ __forceinline__ double eval_iou(double x1, double y1, double w1, double h1, double x2, double y2, double w2, double h2) {
#pragma clang fp contract(off)
    const double ax1 = x1 - w1 / 2., ay1 = y1 - h1 / 2., ax2 = x1 + w1 / 2., ay2 = y1 + h1 / 2.;      // base.py:267-272
    const double bx1 = x2 - w2 / 2., by1 = y2 - h2 / 2., bx2 = x2 + w2 / 2., by2 = y2 + h2 / 2.;
    const double iw = np_max(np_min(ax2, bx2) - np_max(ax1, bx1), 0.);
    const double ih = np_max(np_min(ay2, by2) - np_max(ay1, by1), 0.);
    const double inter = iw * ih;
    const double uni = np_max(w1 * h1 + w2 * h2 - inter, 1e-8);                                       // base.py:190
    return inter / uni;
}

// The version 3 decode of one row in float32, every operation rounded on its own (yolo_hip.h: the ignore test of the YOLOv3 loss).  Centre as
// decode_kernel computes it (v3.py:129); the size in float32 with the anchor rounded to float32 -- decode_kernel keeps the size in float64
// (its anchors are np.float64), so it does not share this function: the detect tests pin its bits.
__device__ __forceinline__ void decode_v3_f32(float t0, float t1, float t2, float t3, float c, float r, float ws, float hs, float awf, float ahf,
                                              float &bx, float &by, float &bw, float &bh) {
#pragma clang fp contract(off)
    bx = (sigmoid_f32(t0) + c) / ws;
    by = (sigmoid_f32(t1) + r) / hs;
    bw = expf(t2) * awf / ws;
    bh = expf(t3) * ahf / hs;
}

}  // namespace yolo

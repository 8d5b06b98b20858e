// The loaders of the weight-gradient kernels (train.hip, train3.hip): eight consecutive channels of one position of X.
#pragma once
#include <hip/hip_runtime.h>

namespace yolo {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// eight consecutive channels of one position, widened to float32 (exact); WIDE: the address is 16-byte aligned
template <typename T, bool WIDE>
__device__ __forceinline__ void wgrad_load8(const T *src, float (&v)[8]);
template <>
__device__ __forceinline__ void wgrad_load8<_Float16, true>(const _Float16 *src, float (&v)[8]) {
    const f16x8 h = *reinterpret_cast<const f16x8 *>(src);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
}
template <>
__device__ __forceinline__ void wgrad_load8<float, true>(const float *src, float (&v)[8]) {
    const float4 a = reinterpret_cast<const float4 *>(src)[0], b = reinterpret_cast<const float4 *>(src)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <>
__device__ __forceinline__ void wgrad_load8<_Float16, false>(const _Float16 *src, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)src[j];
}
template <>
__device__ __forceinline__ void wgrad_load8<float, false>(const float *src, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[j];
}

}  // namespace yolo

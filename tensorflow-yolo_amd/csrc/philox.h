// Philox4x32-10, the library's counter-based generator (include/yolo_hip.h: the augmentation's draws per pixel, the anchor seeding's draw
// per restart and round): counter (c0, c1, 0, 0), key (k0, k1), four 32-bit words out.
#pragma once
#include <hip/hip_runtime.h>

namespace yolo {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned k0, unsigned k1, unsigned (&o)[4]) {
    unsigned c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

}  // namespace yolo

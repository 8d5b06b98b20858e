// How does v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, E8M0 block scales) round INSIDE one instruction and from one instruction to the next?
// One wave, one accumulator chain per test: the host writes chains of operand sets (128 e4m3 bytes of A and of B in k order, four scale bytes
// each, a float32 start value), every row / column of the 16 x 16 tile gets the same operands, and the accumulator is read back after every
// step.  tools/probes/mx_sum_probe.py writes the vectors and compares the answers with candidate restatements on the host.
//   make -C tools/probes mx_sum_probe && tools/probes/mx_sum_probe vectors.bin answers.bin
// vectors.bin: int32 chains, int32 steps; A u8 [chains][steps][128]; B likewise; SA u8 [chains][steps][4]; SB likewise; C0 f32 [chains]
// answers.bin: f32 [chains][steps]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)
typedef int int8v __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

// lane l holds row (A) / column (B) l & 15; its bytes 0-15 are k = 16 g .. 16 g + 15, bytes 16-31 are k = 64 + 16 g .., g = l >> 4; the scale of
// K block b (k = 32 b .. 32 b + 31) is the scale operand of lane group b (conv_mx.hip)
__global__ void __launch_bounds__(64) chain_kernel(const unsigned char *A, const unsigned char *B, const unsigned char *SA, const unsigned char *SB,
                                                   const float *C0, float *out, int chains, int steps) {
    const int g = threadIdx.x >> 4;
    for (int c = 0; c < chains; ++c) {
        float4v acc = {C0[c], C0[c], C0[c], C0[c]};
        for (int s = 0; s < steps; ++s) {
            const size_t o = (size_t)c * steps + s;
            int8v a, b;
            int w[8];
            memcpy(w, A + o * 128 + 16 * g, 16);
            memcpy(w + 4, A + o * 128 + 64 + 16 * g, 16);
            a = int8v{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
            memcpy(w, B + o * 128 + 16 * g, 16);
            memcpy(w + 4, B + o * 128 + 64 + 16 * g, 16);
            b = int8v{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
            acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, 0, (int)SA[o * 4 + g], 0, (int)SB[o * 4 + g]);
            if (threadIdx.x == 0) out[o] = acc[0];
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 3) { printf("usage: %s vectors.bin answers.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
    int hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] < 1 || hdr[1] < 1 || (long long)hdr[0] * hdr[1] > (1 << 22)) { printf("bad header\n"); return 2; }
    const size_t n = (size_t)hdr[0] * hdr[1];
    std::vector<unsigned char> hA(n * 128), hB(n * 128), hSA(n * 4), hSB(n * 4);
    std::vector<float> hC(hdr[0]), hOut(n);
    if (fread(hA.data(), 1, hA.size(), f) != hA.size() || fread(hB.data(), 1, hB.size(), f) != hB.size() || fread(hSA.data(), 1, hSA.size(), f) != hSA.size() ||
        fread(hSB.data(), 1, hSB.size(), f) != hSB.size() || fread(hC.data(), 4, hC.size(), f) != hC.size()) { printf("short file\n"); return 2; }
    fclose(f);
    unsigned char *dA, *dB, *dSA, *dSB;
    float *dC, *dOut;
    CHECK(hipMalloc(&dA, hA.size())); CHECK(hipMalloc(&dB, hB.size())); CHECK(hipMalloc(&dSA, hSA.size())); CHECK(hipMalloc(&dSB, hSB.size()));
    CHECK(hipMalloc(&dC, hC.size() * 4)); CHECK(hipMalloc(&dOut, n * 4));
    CHECK(hipMemcpy(dA, hA.data(), hA.size(), hipMemcpyHostToDevice)); CHECK(hipMemcpy(dB, hB.data(), hB.size(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dSA, hSA.data(), hSA.size(), hipMemcpyHostToDevice)); CHECK(hipMemcpy(dSB, hSB.data(), hSB.size(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dC, hC.data(), hC.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(64), 0, 0, dA, dB, dSA, dSB, dC, dOut, hdr[0], hdr[1]);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(hOut.data(), dOut, n * 4, hipMemcpyDeviceToHost));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(hOut.data(), 4, n, f) != n) { printf("cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    printf("%d chains of %d steps -> %s\n", hdr[0], hdr[1], argv[2]);
    return 0;
}

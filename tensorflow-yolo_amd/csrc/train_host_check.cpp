// A program of its own for the host side of the head-training entries (train_host.cpp): walks yolo_wgrad_plan over a grid of sizes and the
// argument checks over good and bad calls, and verifies what the header promises.  `make san-train` builds it with AddressSanitizer +
// UndefinedBehaviorSanitizer and runs it on the CPU; no device, no HIP.  Exit status 0 and "train_host_check OK" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "train_host.h"

using namespace yolo;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
        }                                                                  \
    } while (0)

int main() {
    std::string err;
    struct yolo_wgrad_plan pl;
    long long plans = 0;
    const int couts[] = {1, 6, 30, 64, 65, 125, 130, 425, 4096};
    const int cins[] = {8, 40, 128, 136, 1024, 4096};
    const long long Ps[] = {1, 15, 16, 17, 31, 32, 33, 69, 507, 2704, 10816, 1LL << 20, (1LL << 30) - 1, 1LL << 30};
    for (int cout : couts)
        for (int cin : cins)
            for (long long P : Ps)
                for (int dt : {YOLO_DTYPE_F32, YOLO_DTYPE_F16}) {
                    const int rc = wgrad_plan(P, cin, cout, dt, &pl, err);
                    EXPECT(rc == YOLO_OK);
                    if (rc) continue;
                    ++plans;
                    EXPECT(pl.tile_cout == kWgradTileCout && pl.tile_cin == kWgradTileCin && pl.tile_positions == kWgradTilePos);
                    EXPECT((long long)pl.tiles_cout * pl.tile_cout >= cout && (long long)(pl.tiles_cout - 1) * pl.tile_cout < cout);
                    EXPECT((long long)pl.tiles_cin * pl.tile_cin >= cin && (long long)(pl.tiles_cin - 1) * pl.tile_cin < cin);
                    EXPECT(pl.positions_per_chunk >= kWgradMinChunk && pl.positions_per_chunk % pl.tile_positions == 0);
                    // the chunks cover [0, P) once: the last one is not empty and ends at or behind P
                    EXPECT(pl.n_chunks >= 1 && (long long)pl.n_chunks * pl.positions_per_chunk >= P);
                    EXPECT((long long)(pl.n_chunks - 1) * pl.positions_per_chunk < P);
                    EXPECT((long long)pl.n_chunks <= 65535);        // a grid's y extent
                    EXPECT(pl.scratch_bytes == (uint64_t)pl.n_chunks * (uint64_t)cout * (uint64_t)(cin + 1) * 4u);
                }
    EXPECT(wgrad_plan(0, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_plan((1LL << 30) + 1, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_plan(16, 12, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG && err.find("multiple of 8") != std::string::npos);
    EXPECT(wgrad_plan(16, 0, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_plan(16, 8, 0, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_plan(16, 8, 1, YOLO_DTYPE_MXF8, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_plan(16, 8, 1, YOLO_DTYPE_F32, nullptr, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_plan(16, 1 << 20, 1 << 20, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);

    // the checks in front of a launch never touch what the pointers point at: host memory stands in for device memory
    std::vector<float> buf(64);
    void *q = buf.data();
    EXPECT(wgrad_plan(169 * 3, 40, 30, YOLO_DTYPE_F16, &pl, err) == YOLO_OK);
    const size_t need = (size_t)pl.scratch_bytes;
    struct yolo_wgrad_plan got;
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, 169 * 48 + 16, 169, 3, 40, q, 30, q, q, q, need, &got, err) == YOLO_OK && got.n_chunks == pl.n_chunks);
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, 169 * 48 + 16, 169, 3, 40, q, 30, q, q, q, need - 1, &got, err) == YOLO_ERR_ARG &&
           err.find("scratch too small") != std::string::npos);
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, 169 * 48 + 16, 169, 3, 36, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);      // cin % 8
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 40, 8, 169 * 48, 169, 3, 40, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);           // coff + cin > ld
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, -8, 169 * 48, 169, 3, 40, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, 168 * 48, 169, 3, 40, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);           // images overlap
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, 168 * 48 + 48, 169, 3, 40, q, 30, q, q, q, need, &got, err) == YOLO_OK);           // the last position may be short
    EXPECT(wgrad_check(nullptr, YOLO_DTYPE_F16, 48, 8, 169 * 48, 169, 3, 40, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, 169 * 48, 169, 3, 40, q, 30, q, q, nullptr, need, &got, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, 169 * 48, 0, 3, 40, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, 169 * 48, 169, 0, 40, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);
    EXPECT(wgrad_check(q, YOLO_DTYPE_F16, 48, 8, (long long)1 << 40, 1 << 20, 1 << 12, 40, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);   // P past 2^30
    EXPECT(wgrad_check((char *)q + 1, YOLO_DTYPE_F16, 48, 8, 169 * 48, 169, 3, 40, q, 30, q, q, q, need, &got, err) == YOLO_ERR_ARG);

    EXPECT(adam_check(q, q, q, q, q, q, q, q, 30 * 1024 + 3, 30, 1e-3f, 0.9f, 0.999f, 1e-8f, err) == YOLO_OK);
    EXPECT(adam_check(q, nullptr, q, q, nullptr, nullptr, q, nullptr, 1, 0, 1e-3f, 0.9f, 0.999f, 1e-8f, err) == YOLO_OK);
    EXPECT(adam_check(q, nullptr, q, q, q, q, q, q, 1, 1, 1e-3f, 0.9f, 0.999f, 1e-8f, err) == YOLO_ERR_ARG);
    EXPECT(adam_check(nullptr, q, q, q, q, q, q, q, 1, 1, 1e-3f, 0.9f, 0.999f, 1e-8f, err) == YOLO_ERR_ARG);
    EXPECT(adam_check(q, q, q, q, q, q, q, q, 0, 1, 1e-3f, 0.9f, 0.999f, 1e-8f, err) == YOLO_ERR_ARG);
    EXPECT(adam_check(q, q, q, q, q, q, q, q, 1, -1, 1e-3f, 0.9f, 0.999f, 1e-8f, err) == YOLO_ERR_ARG);
    EXPECT(adam_check(q, q, q, q, q, q, q, q, 1, 1, 1e-3f, 1.0f, 0.999f, 1e-8f, err) == YOLO_ERR_ARG);
    EXPECT(adam_check(q, q, q, q, q, q, q, q, 1, 1, 1e-3f, 0.9f, -0.1f, 1e-8f, err) == YOLO_ERR_ARG);
    EXPECT(adam_check(q, q, q, q, q, q, q, q, 1, 1, 1e-3f, 0.9f, 0.999f, -1e-8f, err) == YOLO_ERR_ARG);
    EXPECT(adam_check(q, q, q, q, q, q, q, q, 1, 1, std::strtof("nan", nullptr), 0.9f, 0.999f, 1e-8f, err) == YOLO_ERR_ARG);

    if (failures) {
        std::fprintf(stderr, "train_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("train_host_check OK (%lld plans)\n", plans);
    return 0;
}

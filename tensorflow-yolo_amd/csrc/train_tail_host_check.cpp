// A program of its own for the host side of the data gradient and the 3 x 3 weight gradient (train_tail_host.cpp): walks
// yolo_conv3x3_wgrad_plan and yolo_conv3x3_wgrad_f16_plan over a grid of sizes and the argument checks of the entries over good and bad calls, and verifies what the header
// promises.  `make san-tail` builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it on the CPU; no device, no HIP.  Exit
// status 0 and "train_tail_host_check OK" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "train_tail_host.h"

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
    struct yolo_conv3x3_wgrad_plan pl;
    long long plans = 0;
    const int couts[] = {1, 30, 64, 65, 136, 1024, 4096};
    const int cins[] = {8, 40, 64, 72, 136, 1024, 1280};
    const int hws[][2] = {{1, 1}, {1, 5}, {5, 1}, {3, 3}, {5, 7}, {13, 13}, {19, 19}, {3, 80}, {1 << 16, 13}};
    const int batches[] = {1, 2, 3, 16, 64};
    for (int cout : couts)
        for (int cin : cins)
            for (auto &hw : hws)
                for (int batch : batches)
                    for (int dt : {YOLO_DTYPE_F32, YOLO_DTYPE_F16}) {
                        const long long P = (long long)hw[0] * hw[1] * batch;
                        const int rc = wgrad3x3_plan(hw[0], hw[1], batch, cin, cout, dt, &pl, err);
                        EXPECT(rc == YOLO_OK);
                        if (rc) continue;
                        ++plans;
                        EXPECT(pl.tile_cout == kTailTileCout && pl.tile_cin == kTailTileCin && pl.tile_positions == kTailTilePos);
                        EXPECT((long long)pl.tiles_cout * pl.tile_cout >= cout && (long long)(pl.tiles_cout - 1) * pl.tile_cout < cout);
                        EXPECT((long long)pl.tiles_cin * pl.tile_cin >= cin && (long long)(pl.tiles_cin - 1) * pl.tile_cin < cin);
                        EXPECT(pl.positions_per_chunk >= kTailMinChunk && pl.positions_per_chunk % pl.tile_positions == 0);
                        // the chunks cover [0, P) once: the last one is not empty and ends at or behind P
                        EXPECT(pl.n_chunks >= 1 && (long long)pl.n_chunks * pl.positions_per_chunk >= P);
                        EXPECT((long long)(pl.n_chunks - 1) * pl.positions_per_chunk < P);
                        EXPECT((long long)pl.n_chunks <= 65535);        // a grid's y extent
                        EXPECT(pl.halo_rows == pl.tile_positions + 2 * hw[1] + 2);
                        // the halo of the tile's channels and the D tile and the masks fit the 64 KiB of LDS a workgroup may ask for
                        EXPECT((long long)pl.halo_rows * pl.tile_cin * 4 + (long long)pl.tile_positions * pl.tile_cout * 4 + pl.tile_positions * 4 <= 65536);
                        EXPECT(pl.scratch_bytes == (uint64_t)pl.n_chunks * (uint64_t)cout * (uint64_t)(9 * cin + 1) * 4u);
                    }
    EXPECT(wgrad3x3_plan(0, 8, 1, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_plan(8, 0, 1, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_plan(8, 8, 0, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_plan(8, kTailMaxW, 1, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_OK);
    EXPECT(wgrad3x3_plan(8, kTailMaxW + 1, 1, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG && err.find("LDS") != std::string::npos);
    EXPECT(wgrad3x3_plan(1 << 24, 64, 1, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_OK);       // 2^30 positions
    EXPECT(wgrad3x3_plan(1 << 24, 64, 2, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG && err.find("2^30") != std::string::npos);
    EXPECT(wgrad3x3_plan(0x7fffffff, 80, 0x7fffffff, 8, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);      // no overflow on the way
    EXPECT(wgrad3x3_plan(13, 13, 2, 12, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG && err.find("multiple of 8") != std::string::npos);
    EXPECT(wgrad3x3_plan(13, 13, 2, 0, 1, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_plan(13, 13, 2, 8, 0, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_plan(13, 13, 2, 8, 1, YOLO_DTYPE_MXF8, &pl, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_plan(13, 13, 2, 8, 1, YOLO_DTYPE_F32, nullptr, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_plan(13, 13, 2, 1 << 16, 1 << 16, YOLO_DTYPE_F32, &pl, err) == YOLO_ERR_ARG && err.find("31 bits") != std::string::npos);

    // the checks in front of a launch never touch what the pointers point at: host memory stands in for device memory
    std::vector<float> buf(64);
    void *q = buf.data();
    EXPECT(wgrad3x3_plan(13, 13, 3, 40, 30, YOLO_DTYPE_F16, &pl, err) == YOLO_OK);
    const size_t need = (size_t)pl.scratch_bytes;
    struct yolo_conv3x3_wgrad_plan got;
    auto call = [&](const void *x, int ld, int coff, long long is, int h, int w, int batch, int cin, const void *d, const void *sc, const void *dw,
                    const void *db, const void *s, size_t bytes) {
        return wgrad3x3_check(x, YOLO_DTYPE_F16, ld, coff, is, h, w, batch, cin, d, 30, sc, dw, db, s, bytes, &got, err);
    };
    EXPECT(call(q, 48, 8, 169 * 48 + 16, 13, 13, 3, 40, q, q, q, q, q, need) == YOLO_OK && got.n_chunks == pl.n_chunks);
    EXPECT(call(q, 48, 8, 169 * 48 + 16, 13, 13, 3, 40, q, nullptr, q, q, q, need) == YOLO_OK);       // the scale may be null
    EXPECT(call(q, 48, 8, 169 * 48 + 16, 13, 13, 3, 40, q, q, q, q, q, need - 1) == YOLO_ERR_ARG && err.find("scratch too small") != std::string::npos);
    EXPECT(call(q, 48, 8, 169 * 48 + 16, 13, 13, 3, 36, q, q, q, q, q, need) == YOLO_ERR_ARG);        // cin % 8
    EXPECT(call(q, 40, 8, 169 * 48, 13, 13, 3, 40, q, q, q, q, q, need) == YOLO_ERR_ARG);             // coff + cin > ld
    EXPECT(call(q, 48, -8, 169 * 48, 13, 13, 3, 40, q, q, q, q, q, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, 168 * 48, 13, 13, 3, 40, q, q, q, q, q, need) == YOLO_ERR_ARG);             // images overlap
    EXPECT(call(q, 48, 8, 168 * 48 + 48, 13, 13, 3, 40, q, q, q, q, q, need) == YOLO_OK);             // the last position may be short
    EXPECT(call(nullptr, 48, 8, 169 * 48, 13, 13, 3, 40, q, q, q, q, q, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, 169 * 48, 13, 13, 3, 40, nullptr, q, q, q, q, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, 169 * 48, 13, 13, 3, 40, q, q, nullptr, q, q, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, 169 * 48, 13, 13, 3, 40, q, q, q, nullptr, q, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, 169 * 48, 13, 13, 3, 40, q, q, q, q, nullptr, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, 169 * 48, 0, 13, 3, 40, q, q, q, q, q, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, 169 * 48, 13, 13, 0, 40, q, q, q, q, q, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, (long long)1 << 40, 1 << 20, 64, 1 << 12, 40, q, q, q, q, q, need) == YOLO_ERR_ARG);      // P past 2^30
    EXPECT(call((char *)q + 1, 48, 8, 169 * 48, 13, 13, 3, 40, q, q, q, q, q, need) == YOLO_ERR_ARG);
    EXPECT(call(q, 48, 8, 169 * 48, 13, 13, 3, 40, q, (char *)q + 2, q, q, q, need) == YOLO_ERR_ARG);

    // ---- yolo_conv3x3_wgrad_f16_plan and the checks of yolo_conv3x3_wgrad_f16 ----
    struct yolo_conv3x3_wgrad_f16_plan p16;
    const int hws16[][2] = {{1, 1}, {1, 5}, {5, 1}, {13, 13}, {19, 19}, {3, 80}, {1, kTailF16MaxW}, {1 << 16, 13}};
    for (int cout : couts)
        for (int cin : cins)
            for (auto &hw : hws16)
                for (int batch : batches) {
                    const long long P = (long long)hw[0] * hw[1] * batch;
                    const int rc = wgrad3x3_f16_plan(hw[0], hw[1], batch, cin, cout, &p16, err);
                    EXPECT(rc == YOLO_OK);
                    if (rc) continue;
                    ++plans;
                    EXPECT(p16.tile_cout == kTailTileCout && p16.tile_cin == kTailTileCin && p16.tile_positions == kTailF16TilePos);
                    EXPECT((long long)p16.tiles_cout * p16.tile_cout >= cout && (long long)(p16.tiles_cout - 1) * p16.tile_cout < cout);
                    EXPECT((long long)p16.tiles_cin * p16.tile_cin >= cin && (long long)(p16.tiles_cin - 1) * p16.tile_cin < cin);
                    EXPECT(p16.positions_per_chunk >= kTailF16MinChunk && p16.positions_per_chunk % p16.tile_positions == 0);
                    EXPECT(p16.n_chunks >= 1 && (long long)p16.n_chunks * p16.positions_per_chunk >= P);
                    EXPECT((long long)(p16.n_chunks - 1) * p16.positions_per_chunk < P && (long long)p16.n_chunks <= 65535);
                    EXPECT(p16.halo_rows == p16.tile_positions + 2 * hw[1] + 2);
                    // the 16-bit images, the pair masks and the position masks fit the 64 KiB of LDS a workgroup may ask for
                    EXPECT((long long)(p16.halo_rows + p16.tile_positions) * kTailF16RowBytes + 9 * (p16.tile_positions / 2) * 4 + p16.tile_positions * 4 <= 65536);
                    EXPECT(p16.db_groups >= 1 && p16.db_groups <= kTailF16DbGroups && p16.db_positions % 16 == 0);
                    EXPECT((long long)p16.db_groups * p16.db_positions >= P && (long long)(p16.db_groups - 1) * p16.db_positions < P);
                    const uint64_t slabs = (uint64_t)p16.n_chunks * (uint64_t)cout * (uint64_t)(9 * cin + 1) * 4u;
                    EXPECT(p16.record_offset % 256 == 0 && p16.record_offset >= slabs && p16.record_offset < slabs + 256);
                    EXPECT(p16.scratch_bytes >= p16.record_offset + kTailF16RecordBytes + (uint64_t)p16.db_groups * (uint64_t)cout * 4u);
                }
    EXPECT(wgrad3x3_f16_plan(8, kTailF16MaxW + 1, 1, 8, 1, &p16, err) == YOLO_ERR_ARG && err.find("LDS") != std::string::npos);
    EXPECT(wgrad3x3_f16_plan(1 << 24, 64, 1, 8, 1, &p16, err) == YOLO_OK);
    EXPECT(wgrad3x3_f16_plan(1 << 24, 64, 2, 8, 1, &p16, err) == YOLO_ERR_ARG && err.find("2^30") != std::string::npos);
    EXPECT(wgrad3x3_f16_plan(0x7fffffff, 96, 0x7fffffff, 8, 1, &p16, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_f16_plan(13, 13, 2, 12, 1, &p16, err) == YOLO_ERR_ARG && err.find("multiple of 8") != std::string::npos);
    EXPECT(wgrad3x3_f16_plan(13, 13, 2, 8, 0, &p16, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_f16_plan(0, 13, 2, 8, 1, &p16, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_f16_plan(13, 13, 2, 8, 1, nullptr, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3x3_f16_plan(13, 13, 2, 1 << 16, 1 << 16, &p16, err) == YOLO_ERR_ARG && err.find("31 bits") != std::string::npos);
    EXPECT(wgrad3x3_f16_plan(13, 13, 3, 40, 30, &p16, err) == YOLO_OK);
    const size_t need16 = (size_t)p16.scratch_bytes;
    struct yolo_conv3x3_wgrad_f16_plan got16;
    auto call16 = [&](const void *x, int dt, int ld, int coff, long long is, int cin, const void *d, const void *sc, const void *dw, const void *db,
                      const void *s, size_t bytes) {
        return wgrad3x3_f16_check(x, dt, ld, coff, is, 13, 13, 3, cin, d, 30, sc, dw, db, s, bytes, &got16, err);
    };
    EXPECT(call16(q, YOLO_DTYPE_F16, 48, 8, 169 * 48 + 16, 40, q, q, q, q, q, need16) == YOLO_OK && got16.n_chunks == p16.n_chunks);
    EXPECT(call16(q, YOLO_DTYPE_F16, 48, 8, 169 * 48 + 16, 40, q, nullptr, q, q, q, need16) == YOLO_OK);
    EXPECT(call16(q, YOLO_DTYPE_F32, 48, 8, 169 * 48 + 16, 40, q, q, q, q, q, need16) == YOLO_ERR_ARG && err.find("yolo_conv3x3_wgrad's") != std::string::npos);
    EXPECT(call16(q, YOLO_DTYPE_MXF8, 48, 8, 169 * 48 + 16, 40, q, q, q, q, q, need16) == YOLO_ERR_ARG);
    EXPECT(call16(q, YOLO_DTYPE_F16, 48, 8, 169 * 48 + 16, 40, q, q, q, q, q, need16 - 1) == YOLO_ERR_ARG && err.find("scratch too small") != std::string::npos);
    EXPECT(call16(q, YOLO_DTYPE_F16, 48, 8, 169 * 48 + 16, 36, q, q, q, q, q, need16) == YOLO_ERR_ARG);
    EXPECT(call16(q, YOLO_DTYPE_F16, 40, 8, 169 * 48, 40, q, q, q, q, q, need16) == YOLO_ERR_ARG);
    EXPECT(call16(q, YOLO_DTYPE_F16, 48, 8, 168 * 48, 40, q, q, q, q, q, need16) == YOLO_ERR_ARG);
    EXPECT(call16(nullptr, YOLO_DTYPE_F16, 48, 8, 169 * 48, 40, q, q, q, q, q, need16) == YOLO_ERR_ARG);
    EXPECT(call16(q, YOLO_DTYPE_F16, 48, 8, 169 * 48, 40, q, q, q, q, nullptr, need16) == YOLO_ERR_ARG);
    EXPECT(call16((char *)q + 1, YOLO_DTYPE_F16, 48, 8, 169 * 48, 40, q, q, q, q, q, need16) == YOLO_ERR_ARG);
    EXPECT(call16(q, YOLO_DTYPE_F16, 48, 8, 169 * 48, 40, q, q, q, q, (char *)q + 2, need16) == YOLO_ERR_ARG);

    long long tiles = 0;
    auto dcall =[&](const void *g, int cout, const void *w, int cin, const void *y, int dt, int ld, int coff, long long is, int ppi, int batch,
                     const void *d) { return dgrad_check(g, cout, w, cin, y, dt, ld, coff, is, ppi, batch, 0.1f, d, &tiles, err); };
    alignas(16) static float abuf[64];
    void *a = abuf;
    EXPECT(dcall(q, 425, a, 1024, q, YOLO_DTYPE_F16, 1024, 0, 169 * 1024, 169, 2, a) == YOLO_OK && tiles == 6 * 8);
    EXPECT(dcall(q, 1, a, 8, nullptr, 77, -1, -1, -1, 1, 1, a) == YOLO_OK && tiles == 1);        // Y null: its description is not looked at
    EXPECT(dcall(q, 30, a, 40, q, YOLO_DTYPE_F32, 48, 8, 17 * 48, 17, 1, a) == YOLO_OK && tiles == 1);
    EXPECT(dcall(nullptr, 30, a, 40, nullptr, 0, 0, 0, 0, 17, 1, a) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 30, nullptr, 40, nullptr, 0, 0, 0, 0, 17, 1, a) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 30, a, 40, nullptr, 0, 0, 0, 0, 17, 1, nullptr) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 0, a, 40, nullptr, 0, 0, 0, 0, 17, 1, a) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 30, a, 36, nullptr, 0, 0, 0, 0, 17, 1, a) == YOLO_ERR_ARG && err.find("multiple of 8") != std::string::npos);
    EXPECT(dcall(q, 30, a, 40, nullptr, 0, 0, 0, 0, 0, 1, a) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 30, a, 40, nullptr, 0, 0, 0, 0, 17, 0, a) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 30, a, 40, nullptr, 0, 0, 0, 0, 1 << 20, 1 << 11, a) == YOLO_ERR_ARG && err.find("2^30") != std::string::npos);
    EXPECT(dcall(q, 1 << 16, a, 1 << 16, nullptr, 0, 0, 0, 0, 17, 1, a) == YOLO_ERR_ARG && err.find("31 bits") != std::string::npos);
    EXPECT(dcall(q, 30, (char *)a + 4, 40, nullptr, 0, 0, 0, 0, 17, 1, a) == YOLO_ERR_ARG && err.find("16-byte") != std::string::npos);
    EXPECT(dcall(q, 30, a, 40, nullptr, 0, 0, 0, 0, 17, 1, (char *)a + 8) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 30, a, 40, q, YOLO_DTYPE_MXF8, 48, 8, 17 * 48, 17, 1, a) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 30, a, 40, q, YOLO_DTYPE_F16, 40, 8, 17 * 48, 17, 1, a) == YOLO_ERR_ARG);           // coff + cin > ld
    EXPECT(dcall(q, 30, a, 40, q, YOLO_DTYPE_F16, 48, 8, 16 * 48, 17, 2, a) == YOLO_ERR_ARG);           // images overlap
    EXPECT(dcall(q, 30, a, 40, (char *)q + 1, YOLO_DTYPE_F16, 48, 8, 17 * 48, 17, 1, a) == YOLO_ERR_ARG);
    EXPECT(dcall(q, 8, a, 1 << 27, nullptr, 0, 0, 0, 0, 1 << 20, 1 << 10, a) == YOLO_ERR_ARG && err.find("one launch") != std::string::npos);

    if (failures) {
        std::fprintf(stderr, "train_tail_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("train_tail_host_check OK (%lld plans)\n", plans);
    return 0;
}

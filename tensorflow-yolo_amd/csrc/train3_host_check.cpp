// A program of its own for the host side of the YOLOv3 head weight gradient (train3_host.cpp): walks yolo_v3_head_wgrad_plan over a grid of
// heads, channel counts and batches and the argument checks over good and bad calls, and verifies what the header promises.
// `make san-train3` builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it on the CPU; no device, no HIP.  Exit status 0
// and "train3_host_check OK" when everything holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "train3_host.h"

using namespace yolo;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
        }                                                                  \
    } while (0)

static yolo_head_desc make_head(int n_scales, const int *h, const int *w, int na, int n_classes) {
    yolo_head_desc hd;
    std::memset(&hd, 0, sizeof hd);
    hd.version = 3; hd.n_classes = n_classes; hd.n_scales = n_scales;
    for (int s = 0; s < n_scales && s < YOLO_MAX_SCALES; ++s) {
        hd.h[s] = h[s]; hd.w[s] = w[s]; hd.n_anchors[s] = na;
        for (int a = 0; a < na && a < YOLO_MAX_ANCHORS; ++a) { hd.anchors[s][2 * a] = 1.5 + a + s; hd.anchors[s][2 * a + 1] = 2.25 + a; }
    }
    return hd;
}

int main() {
    std::string err;
    struct yolo_v3_wgrad_plan pl;
    Wgrad3Geometry geo;
    long long plans = 0;
    const int sizes[] = {1, 2, 13, 19};
    const int cins[] = {8, 40, 136, 256, 1024, 2048};
    for (int n_scales = 1; n_scales <= YOLO_MAX_SCALES; ++n_scales)
        for (int base : sizes)
            for (int na : {1, 3, YOLO_MAX_ANCHORS})
                for (int C : {1, 80})
                    for (int c0 = 0; c0 < 6; ++c0)
                        for (int batch : {1, 2, 31, 32, 64, 1000}) {
                            int h[YOLO_MAX_SCALES], w[YOLO_MAX_SCALES];
                            int32_t cin[YOLO_MAX_SCALES];
                            for (int s = 0; s < YOLO_MAX_SCALES; ++s) { h[s] = base << s; w[s] = (base << s) + s; cin[s] = cins[(c0 + 5 * s) % 6]; }
                            const yolo_head_desc hd = make_head(n_scales, h, w, na, C);
                            EXPECT(wgrad3_plan(&hd, cin, batch, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_OK);
                            ++plans;
                            EXPECT(pl.n_scales == n_scales && pl.threads == kWgrad3Threads && pl.channels_per_thread == kWgrad3Lane && pl.reduce_tile_chunks == kWgrad3RedChunks);
                            uint64_t end = 0;
                            long long ob = 0, wb = 0, row0 = 0;
                            for (int s = 0; s < n_scales; ++s) {
                                const long long P = (long long)h[s] * w[s] * batch, ppc = pl.positions_per_chunk[s], n = pl.n_chunks[s];
                                EXPECT(pl.positions[s] == P && ppc >= kWgrad3MinChunk && n >= 1);
                                EXPECT(n * ppc >= P && (n - 1) * ppc < P);                  // the chunks cover [0, P) once, the last one not empty
                                EXPECT(pl.threads_per_chunk[s] * kWgrad3Lane == cin[s]);
                                EXPECT((long long)pl.obj_workgroups[s] * kWgrad3Threads >= n * pl.threads_per_chunk[s]);
                                EXPECT((long long)(pl.obj_workgroups[s] - 1) * kWgrad3Threads < n * pl.threads_per_chunk[s]);
                                EXPECT(pl.win_workgroups[s] == na * ((5 + C + kWgrad3WinRows - 1) / kWgrad3WinRows) * ((cin[s] + kWgrad3WinTile - 1) / kWgrad3WinTile));
                                EXPECT(pl.slab_offset[s] % 256 == 0 && pl.slab_offset[s] >= end);
                                EXPECT(pl.slab_bytes[s] == (uint64_t)n * (uint64_t)(na * cin[s] + 8) * 4u);
                                end = pl.slab_offset[s] + pl.slab_bytes[s];
                                const Wgrad3Scale &sc = geo.sc[s];
                                EXPECT(sc.obj_blk0 == ob && sc.win_blk0 == wb && sc.row0 == row0 && sc.P == P && sc.ppi == h[s] * w[s]);
                                EXPECT(sc.ppc == ppc && sc.n_chunks == n && sc.na == na && sc.cin == cin[s]);
                                ob += pl.obj_workgroups[s]; wb += pl.win_workgroups[s]; row0 += (long long)h[s] * w[s] * na;
                            }
                            EXPECT(geo.obj_blocks == ob && geo.win_blocks == wb && geo.rows == row0 && geo.stride == 5 + C);
                            EXPECT(pl.slot_offset % 256 == 0 && pl.slot_offset >= end && pl.slot_bytes == (uint64_t)batch * YOLO_EVAL_MAX_GT * 4u);
                            EXPECT(pl.scratch_bytes % 256 == 0 && pl.scratch_bytes >= pl.slot_offset + pl.slot_bytes);
                        }
    const int g3[] = {19, 38, 76};
    const int32_t c3[] = {1024, 512, 256, 0};
    yolo_head_desc hd = make_head(3, g3, g3, 3, 80);
    EXPECT(wgrad3_plan(&hd, c3, 32, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_OK && pl.positions[2] == 32 * 76 * 76);
    // refusals of the plan
    yolo_head_desc bad = hd;
    bad.version = 2;
    EXPECT(wgrad3_plan(&bad, c3, 2, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_ERR_ARG && err == "the head must be version 3");
    EXPECT(wgrad3_plan(nullptr, c3, 2, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_ERR_ARG && err == "null argument");
    EXPECT(wgrad3_plan(&hd, nullptr, 2, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3_plan(&hd, c3, 2, YOLO_DTYPE_F16, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(wgrad3_plan(&hd, c3, 2, YOLO_DTYPE_MXF8, &pl, &geo, err) == YOLO_ERR_ARG && err.find("x_dtype") != std::string::npos);
    EXPECT(wgrad3_plan(&hd, c3, 0, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_ERR_ARG && err.find("batch") != std::string::npos);
    const int32_t c12[] = {1024, 12, 256, 0}, c0[] = {1024, 512, 0, 0};
    EXPECT(wgrad3_plan(&hd, c12, 2, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_ERR_ARG && err == "scale 1: cin must be a positive multiple of 8");
    EXPECT(wgrad3_plan(&hd, c0, 2, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_ERR_ARG && err.find("scale 2") == 0);
    EXPECT(wgrad3_plan(&hd, c3, 1 << 20, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_ERR_ARG && err.find("2^30") != std::string::npos);
    const int32_t huge[] = {1024, 512, 0x7ffffff8, 0};
    EXPECT(wgrad3_plan(&hd, huge, 2, YOLO_DTYPE_F16, &pl, &geo, err) == YOLO_ERR_ARG && err.find("31 bits") != std::string::npos);

    // the checks in front of a launch never touch what the pointers point at: host memory stands in for device memory
    alignas(256) static float buf[64];
    void *q = buf;
    float *dw[YOLO_MAX_SCALES] = {buf, buf, buf, nullptr}, *db[YOLO_MAX_SCALES] = {buf, buf, buf, nullptr};
    yolo_v3_wgrad_view v[YOLO_MAX_SCALES];
    std::memset(v, 0, sizeof v);
    for (int s = 0; s < 3; ++s) {
        v[s].x_dev = q; v[s].cin = c3[s]; v[s].ld = c3[s]; v[s].coff = 0; v[s].image_stride = (int64_t)g3[s] * g3[s] * c3[s]; v[s].dtype = YOLO_DTYPE_F16;
    }
    const size_t big = (size_t)1 << 40;
    auto call = [&](const yolo_head_desc *h_, const yolo_v3_wgrad_view *v_, int batch, const void *g_, const void *t_, int max_gt, float *const *dw_,
                    float *const *db_, void *s_, size_t bytes) { return wgrad3_check(h_, v_, batch, g_, t_, max_gt, dw_, db_, s_, bytes, &pl, &geo, err); };
    EXPECT(call(&hd, v, 2, q, q, 8, dw, db, q, big) == YOLO_OK && geo.sc[0].wide == 1 && geo.sc[1].f16 == 1 && geo.sc[2].x == q);
    EXPECT(geo.sc[1].slab == reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(q) + pl.slab_offset[1]));
    EXPECT(call(&hd, v, 2, q, q, YOLO_EVAL_MAX_GT, dw, db, q, pl.scratch_bytes) == YOLO_OK);
    EXPECT(call(&hd, v, 2, q, q, 8, dw, db, q, pl.scratch_bytes - 1) == YOLO_ERR_ARG && err.find("scratch too small") == 0);
    EXPECT(call(nullptr, v, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err == "null argument");
    EXPECT(call(&hd, nullptr, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG);
    EXPECT(call(&hd, v, 2, nullptr, q, 8, dw, db, q, big) == YOLO_ERR_ARG);
    EXPECT(call(&hd, v, 2, q, nullptr, 8, dw, db, q, big) == YOLO_ERR_ARG);
    EXPECT(call(&hd, v, 2, q, q, 8, nullptr, db, q, big) == YOLO_ERR_ARG);
    EXPECT(call(&hd, v, 2, q, q, 8, dw, nullptr, q, big) == YOLO_ERR_ARG);
    EXPECT(call(&hd, v, 2, q, q, 8, dw, db, nullptr, big) == YOLO_ERR_ARG);
    EXPECT(call(&hd, v, 0, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err.find("batch") != std::string::npos);
    EXPECT(call(&hd, v, 2, q, q, 0, dw, db, q, big) == YOLO_ERR_ARG && err.find("max_gt") != std::string::npos);
    EXPECT(call(&hd, v, 2, q, q, YOLO_EVAL_MAX_GT + 1, dw, db, q, big) == YOLO_ERR_ARG);
    EXPECT(call(&bad, v, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err == "the head must be version 3");
    EXPECT(call(&hd, v, 2, q, q, 8, dw, db, reinterpret_cast<unsigned char *>(q) + 4, big) == YOLO_ERR_ARG && err.find("16-byte") != std::string::npos);
    EXPECT(call(&hd, v, 2, reinterpret_cast<unsigned char *>(q) + 2, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err.find("aligned") != std::string::npos);
    {
        float *dw2[YOLO_MAX_SCALES] = {buf, nullptr, buf, nullptr};
        EXPECT(call(&hd, v, 2, q, q, 8, dw2, db, q, big) == YOLO_ERR_ARG && err == "scale 1: null argument");
    }
    yolo_v3_wgrad_view w[YOLO_MAX_SCALES];
    auto reset = [&]() { std::memcpy(w, v, sizeof v); };
    reset(); w[2].x_dev = nullptr;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err == "scale 2: null argument");
    reset(); w[0].dtype = YOLO_DTYPE_MXF8;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err.find("scale 0: dtype") == 0);
    reset(); w[1].cin = 508;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err.find("multiple of 8") != std::string::npos);
    reset(); w[1].ld = 504;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err.find("scale 1: the channels") == 0);
    reset(); w[1].coff = 8;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG);
    reset(); w[1].coff = -8;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG);
    reset(); w[2].image_stride -= 1;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err.find("scale 2: image_stride") == 0);
    reset(); w[0].x_dev = reinterpret_cast<unsigned char *>(q) + 1;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_ERR_ARG && err.find("aligned") != std::string::npos);
    // a view no 16-byte load fits takes the element loads; float32 views likewise
    reset(); w[0].x_dev = reinterpret_cast<unsigned char *>(q) + 2; w[1].ld = 517; w[1].coff = 3; w[1].image_stride = 38 * 38 * 517 + 7; w[2].dtype = YOLO_DTYPE_F32;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_OK && geo.sc[0].wide == 0 && geo.sc[1].wide == 0 && geo.sc[2].wide == 1 && geo.sc[2].f16 == 0);
    reset(); w[2].dtype = YOLO_DTYPE_F32; w[2].ld = 258; w[2].image_stride = 76 * 76 * 258;
    EXPECT(call(&hd, w, 2, q, q, 8, dw, db, q, big) == YOLO_OK && geo.sc[2].wide == 0);

    if (failures) {
        std::fprintf(stderr, "train3_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("train3_host_check OK (%lld plans)\n", plans);
    return 0;
}

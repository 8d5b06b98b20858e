// A program of its own for the host side of the sparse data gradient of a YOLOv3 head conv (train3_tail_host.cpp): walks
// yolo_v3_head_dgrad_plan over a grid of heads, scales, channel counts and batches and the argument checks over good and bad calls, and
// verifies what the header promises.  `make san-blocks` builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it on the CPU;
// no device, no HIP.  Exit status 0 and "train3_tail_host_check OK" when everything holds.
#include <cstdio>
#include <cstring>

#include "train3_tail_host.h"

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
    struct yolo_v3_dgrad_plan pl;
    Dgrad3Params p;
    long long plans = 0;
    const int sizes[] = {1, 2, 13, 19};
    const int cins[] = {8, 40, 136, 256, 1024, 1032, 2048, 4104};
    for (int n_scales = 1; n_scales <= YOLO_MAX_SCALES; ++n_scales)
        for (int base : sizes)
            for (int na : {1, 3, YOLO_MAX_ANCHORS})
                for (int C : {1, 80})
                    for (int cin : cins)
                        for (int batch : {1, 2, 31, 32, 64, 1000}) {
                            int h[YOLO_MAX_SCALES], w[YOLO_MAX_SCALES];
                            for (int s = 0; s < YOLO_MAX_SCALES; ++s) { h[s] = base << s; w[s] = (base << s) + s; }
                            const yolo_head_desc hd = make_head(n_scales, h, w, na, C);
                            long long row0 = 0;
                            for (int s = 0; s < n_scales; ++s) {
                                EXPECT(dgrad3_plan(&hd, s, cin, batch, &pl, &p, err) == YOLO_OK);
                                ++plans;
                                const long long P = (long long)h[s] * w[s] * batch;
                                EXPECT(pl.threads == kDgrad3Threads && pl.channels_per_thread == kDgrad3Lane && pl.positions == P);
                                EXPECT(pl.tile_cin == (cin < kDgrad3TileCin ? cin : kDgrad3TileCin) && pl.tile_cin % kDgrad3Lane == 0);
                                EXPECT((long long)pl.tiles_cin * pl.tile_cin >= cin && (long long)(pl.tiles_cin - 1) * pl.tile_cin < cin);
                                EXPECT(pl.threads_per_position * kDgrad3Lane == pl.tile_cin);
                                EXPECT(pl.positions_per_round >= 1 && pl.positions_per_round * pl.threads_per_position <= kDgrad3Threads);
                                EXPECT((pl.positions_per_round + 1) * pl.threads_per_position > kDgrad3Threads);
                                EXPECT(pl.rounds >= 1 && pl.positions_per_workgroup == pl.rounds * pl.positions_per_round && pl.loops == (pl.rounds > 1));
                                // the workgroups cover [0, P) once, the last one not empty, and stay at the target
                                EXPECT((long long)pl.workgroups * pl.positions_per_workgroup >= P && (long long)(pl.workgroups - 1) * pl.positions_per_workgroup < P);
                                EXPECT(pl.workgroups <= kDgrad3TargetGroups);
                                EXPECT(pl.lds_bytes == na * pl.tile_cin * 4 && pl.lds_bytes <= 64 * 1024);
                                EXPECT(p.cin == cin && p.na == na && p.stride == 5 + C && p.row0 == row0 && p.ppi == h[s] * w[s] && p.P == P);
                                EXPECT(p.tile_cin == pl.tile_cin && p.tiles_cin == pl.tiles_cin && p.tpp == pl.threads_per_position && p.ppr == pl.positions_per_round);
                                EXPECT(p.ppw == pl.positions_per_workgroup && p.groups == pl.workgroups && p.y == nullptr && p.d == nullptr);
                                row0 += (long long)h[s] * w[s] * na;
                            }
                            EXPECT(p.rows == row0);
                        }
    const int g3[] = {19, 38, 76};
    yolo_head_desc hd = make_head(3, g3, g3, 3, 80);
    EXPECT(dgrad3_plan(&hd, 2, 256, 32, &pl, &p, err) == YOLO_OK && pl.positions == 32 * 76 * 76 && pl.loops == 1 && pl.lds_bytes == 3 * 256 * 4);
    EXPECT(dgrad3_plan(&hd, 0, 1024, 32, &pl, nullptr, err) == YOLO_OK && pl.lds_bytes == 12 * 1024);
    // refusals of the plan
    yolo_head_desc bad = hd;
    bad.version = 2;
    EXPECT(dgrad3_plan(&bad, 0, 256, 2, &pl, &p, err) == YOLO_ERR_ARG && err == "the head must be version 3");
    EXPECT(dgrad3_plan(nullptr, 0, 256, 2, &pl, &p, err) == YOLO_ERR_ARG && err == "null argument");
    EXPECT(dgrad3_plan(&hd, 0, 256, 2, nullptr, &p, err) == YOLO_ERR_ARG);
    EXPECT(dgrad3_plan(&hd, -1, 256, 2, &pl, &p, err) == YOLO_ERR_ARG && err == "scale must be 0..2");
    EXPECT(dgrad3_plan(&hd, 3, 256, 2, &pl, &p, err) == YOLO_ERR_ARG && err.find("scale") == 0);
    EXPECT(dgrad3_plan(&hd, 0, 256, 0, &pl, &p, err) == YOLO_ERR_ARG && err.find("batch") != std::string::npos);
    EXPECT(dgrad3_plan(&hd, 0, 12, 2, &pl, &p, err) == YOLO_ERR_ARG && err == "cin must be a positive multiple of 8");
    EXPECT(dgrad3_plan(&hd, 0, 0, 2, &pl, &p, err) == YOLO_ERR_ARG);
    EXPECT(dgrad3_plan(&hd, 2, 256, 1 << 20, &pl, &p, err) == YOLO_ERR_ARG && err.find("2^30") != std::string::npos);

    // the checks in front of a launch never touch what the pointers point at: host memory stands in for device memory
    alignas(256) static float buf[64];
    void *q = buf;
    unsigned char *qb = reinterpret_cast<unsigned char *>(q);
    const long long is1 = 38 * 38 * 512;
    auto call = [&](const yolo_head_desc *h_, int s_, const void *g_, const void *t_, int max_gt, int batch, const void *w_, int cin, const void *y_,
                    int dt, int ld, int coff, long long istride, void *d_) {
        return dgrad3_check(h_, s_, g_, t_, max_gt, batch, w_, cin, y_, dt, ld, coff, istride, 0.1f, d_, &pl, &p, err);
    };
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_OK && p.wide == 1 && p.f16 == 1 && p.y == q && p.d == buf);
    EXPECT(p.row0 == 19 * 19 * 3 && p.max_gt == 8 && p.slope == 0.1f && p.ld == 512 && p.img_stride == is1);
    EXPECT(call(&hd, 1, q, q, YOLO_EVAL_MAX_GT, 2, q, 512, nullptr, 77, -1, -1, -1, q) == YOLO_OK && p.y == nullptr && p.wide == 0);    // a null Y: its view is not looked at
    EXPECT(call(nullptr, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err == "null argument");
    EXPECT(call(&hd, 1, nullptr, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG);
    EXPECT(call(&hd, 1, q, nullptr, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG);
    EXPECT(call(&hd, 1, q, q, 8, 2, nullptr, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, nullptr) == YOLO_ERR_ARG);
    EXPECT(call(&bad, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err == "the head must be version 3");
    EXPECT(call(&hd, 3, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err.find("scale") == 0);
    EXPECT(call(&hd, 1, q, q, 0, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err.find("max_gt") == 0);
    EXPECT(call(&hd, 1, q, q, YOLO_EVAL_MAX_GT + 1, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG);
    EXPECT(call(&hd, 1, q, q, 8, 0, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err.find("batch") != std::string::npos);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 508, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err.find("multiple of 8") != std::string::npos);
    EXPECT(call(&hd, 1, qb + 2, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err.find("aligned") != std::string::npos);
    EXPECT(call(&hd, 1, q, qb + 2, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG);
    EXPECT(call(&hd, 1, q, q, 8, 2, qb + 8, 512, q, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err.find("16-byte") != std::string::npos);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1, qb + 4) == YOLO_ERR_ARG && err.find("16-byte") != std::string::npos);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_MXF8, 512, 0, is1, q) == YOLO_ERR_ARG && err.find("dtype") != std::string::npos);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 504, 0, is1, q) == YOLO_ERR_ARG && err.find("the channels") == 0);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 8, is1, q) == YOLO_ERR_ARG);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, -8, is1, q) == YOLO_ERR_ARG);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 512, 0, is1 - 1, q) == YOLO_ERR_ARG && err.find("image_stride") == 0);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, qb + 1, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_ERR_ARG && err.find("aligned") != std::string::npos);
    // a view no 16-byte load fits takes the element loads; float32 views likewise
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, qb + 2, YOLO_DTYPE_F16, 512, 0, is1, q) == YOLO_OK && p.wide == 0);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F16, 517, 3, 38 * 38 * 517 + 7, q) == YOLO_OK && p.wide == 0);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F32, 516, 4, 38 * 38 * 516, q) == YOLO_OK && p.wide == 1 && p.f16 == 0);
    EXPECT(call(&hd, 1, q, q, 8, 2, q, 512, q, YOLO_DTYPE_F32, 514, 0, 38 * 38 * 514, q) == YOLO_OK && p.wide == 0);

    if (failures) {
        std::fprintf(stderr, "train3_tail_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("train3_tail_host_check OK (%lld plans)\n", plans);
    return 0;
}

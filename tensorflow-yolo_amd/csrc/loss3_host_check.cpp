// A program of its own for the host side of the YOLOv3 loss entries (loss3_host.cpp): walks the geometry over a grid of heads and the
// argument checks over good and bad calls, and verifies what the header promises.  `make san-loss3` builds it with AddressSanitizer +
// UndefinedBehaviorSanitizer and runs it on the CPU; no device, no HIP.  Exit status 0 and "loss3_host_check OK" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "loss3_host.h"

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
    Loss3Geometry geo;
    long long heads = 0;
    const int sizes[] = {1, 2, 3, 13, 19, 26, 38, 52, 76, 100};
    for (int n_scales = 1; n_scales <= YOLO_MAX_SCALES; ++n_scales)
        for (int base : sizes)
            for (int na : {1, 3, YOLO_MAX_ANCHORS})
                for (int C : {1, 20, 80, 1000}) {
                    int h[YOLO_MAX_SCALES], w[YOLO_MAX_SCALES];
                    for (int s = 0; s < YOLO_MAX_SCALES; ++s) { h[s] = base << s; w[s] = (base << s) + s; }
                    const yolo_head_desc hd = make_head(n_scales, h, w, na, C);
                    long long want = 0;
                    for (int s = 0; s < n_scales; ++s) want += (long long)h[s] * w[s] * na;
                    const bool fits = want * (5LL + C) <= 0x7fffffffLL;
                    const int rc = loss3_geometry(&hd, &geo, err);
                    EXPECT(rc == (fits ? YOLO_OK : YOLO_ERR_ARG));
                    if (rc) continue;
                    ++heads;
                    long long rows = 0;
                    for (int s = 0; s < n_scales; ++s) {
                        EXPECT(geo.sc[s].row0 == rows && geo.sc[s].h == h[s] && geo.sc[s].w == w[s] && geo.sc[s].na == na);
                        EXPECT(geo.sc[s].aw[na - 1] == hd.anchors[s][2 * (na - 1)] && geo.sc[s].ahf[0] == (float)hd.anchors[s][1]);
                        rows += (long long)h[s] * w[s] * na;
                    }
                    EXPECT(geo.rows == rows && geo.n_scales == n_scales && geo.n_classes == C);
                    // the parts cover [0, R) once: the last one is not empty and ends at or behind R
                    EXPECT(geo.parts >= 1 && (long long)geo.parts * kLoss3RowsPerPart >= rows && (long long)(geo.parts - 1) * kLoss3RowsPerPart < rows);
                }
    {   // YOLOv3-608: 19^2 / 38^2 / 76^2, three anchors
        const int h[] = {19, 38, 76};
        const yolo_head_desc hd = make_head(3, h, h, 3, 80);
        EXPECT(loss3_geometry(&hd, &geo, err) == YOLO_OK && geo.rows == 22743 && geo.parts == 23);
    }
    const int one[] = {4, 8, 16, 32};
    yolo_head_desc hd = make_head(3, one, one, 3, 20);
    yolo_head_desc bad = hd;
    bad.version = 2;
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG && err.find("the head must be version 3") != std::string::npos);
    bad = hd; bad.n_scales = 0;
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG);
    bad = hd; bad.n_scales = YOLO_MAX_SCALES + 1;
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG);
    bad = hd; bad.n_classes = 0;
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG);
    bad = hd; bad.h[1] = 0;
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG && err.find("scale 1") != std::string::npos);
    bad = hd; bad.w[2] = -3;
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG && err.find("scale 2") != std::string::npos);
    bad = hd; bad.n_anchors[0] = 0;
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG && err.find("scale 0") != std::string::npos);
    bad = hd; bad.n_anchors[0] = YOLO_MAX_ANCHORS + 1;
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG);
    bad = hd; bad.h[0] = bad.w[0] = 1 << 15; bad.n_classes = 80;       // 2^30 cells x 3 anchors x 85 floats: past 31 bits
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG && err.find("31 bits") != std::string::npos);
    bad = hd; bad.h[0] = bad.w[0] = std::numeric_limits<int32_t>::max();
    EXPECT(loss3_geometry(&bad, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_geometry(nullptr, &geo, err) == YOLO_ERR_ARG && loss3_geometry(&hd, nullptr, err) == YOLO_ERR_ARG);

    // the checks in front of a launch never touch what the pointers point at: host memory stands in for device memory
    std::vector<float> buf(64), other(64);
    void *q = buf.data(), *g = other.data();
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_OK && geo.rows == (16 + 64 + 256) * 3);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.7, q, q, q, q, true, g, &geo, err) == YOLO_OK);
    EXPECT(loss3_check(&hd, q, 2, q, q, YOLO_EVAL_MAX_GT, 1.0, q, q, q, q, true, g, &geo, err) == YOLO_OK);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.7, q, q, q, q, true, q, &geo, err) == YOLO_ERR_ARG && err.find("grad_dev must not be logits_dev") != std::string::npos);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.7, q, q, q, q, true, nullptr, &geo, err) == YOLO_ERR_ARG && err == "null argument");
    EXPECT(loss3_check(nullptr, q, 2, q, q, 8, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, nullptr, 2, q, q, 8, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, nullptr, q, 8, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, q, nullptr, 8, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.7, nullptr, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.7, q, nullptr, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.7, q, q, nullptr, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.7, q, q, q, nullptr, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 0, q, q, 8, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG && err.find("batch") != std::string::npos);
    EXPECT(loss3_check(&hd, q, 2, q, q, 0, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG && err.find("max_gt") != std::string::npos);
    EXPECT(loss3_check(&hd, q, 2, q, q, YOLO_EVAL_MAX_GT + 1, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 0.0, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG && err.find("ignore_thresh") != std::string::npos);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, 1.0000001, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, -0.5, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    EXPECT(loss3_check(&hd, q, 2, q, q, 8, std::strtod("nan", nullptr), q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG);
    bad = hd; bad.version = 2;
    EXPECT(loss3_check(&bad, q, 2, q, q, 8, 0.7, q, q, q, q, false, nullptr, &geo, err) == YOLO_ERR_ARG && err == "the head must be version 3");

    if (failures) {
        std::fprintf(stderr, "loss3_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("loss3_host_check OK (%lld heads)\n", heads);
    return 0;
}

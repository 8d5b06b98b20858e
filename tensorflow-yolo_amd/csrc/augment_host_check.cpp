// A program of its own for the host side of the augmentation entries (augment_host.cpp): walks the record checks over good and bad
// records, the kernel's record over what it folds, and the truths over boxes inside, across and outside every edge, and verifies what the
// header promises.  `make san-augment` builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it on the CPU; no device,
// no HIP.  Exit status 0 and "augment_host_check OK" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "augment_host.h"

using namespace yolo;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
        }                                                                  \
    } while (0)

static yolo_augment_image good() {
    yolo_augment_image p = {};
    p.enabled = 1; p.flip_lr = 1; p.flip_ud = 0; p.radius = 2;
    p.taps[0] = 100; p.taps[1] = 60; p.taps[2] = 18;
    p.drop_thr = 85899346u; p.noise_q[0] = 1131; p.noise_q[1] = 11; p.noise_loc[0] = 0; p.noise_loc[1] = 32; p.tx = -40;
    p.key[0] = 1u; p.key[1] = 0xffffffffu;
    return p;
}

static bool has(const std::string &s, const char *word) { return s.find(word) != std::string::npos; }

int main() {
    std::string err;
    yolo_augment_image p = good();
    EXPECT(augment_check(&p, 32, 32, err) == YOLO_OK);
    EXPECT(augment_check(nullptr, 32, 32, err) == YOLO_ERR_ARG && has(err, "null"));
    EXPECT(augment_check(&p, 0, 32, err) == YOLO_ERR_ARG && has(err, "at least 1"));
    EXPECT(augment_check(&p, 32, 30, err) == YOLO_ERR_ARG && has(err, "multiple of 4"));
    EXPECT(augment_check(&p, 1 << 16, 1 << 16, err) == YOLO_ERR_ARG && has(err, "31 bits"));
    EXPECT(augment_check(&p, 2, 4, err) == YOLO_ERR_ARG && has(err, "below h and w"));
    EXPECT(augment_check(&p, 3, 4, err) == YOLO_OK);
    struct { int yolo_augment_image::*field; int value; const char *word; } bad[] = {
        {&yolo_augment_image::enabled, 2, "enabled"}, {&yolo_augment_image::flip_lr, -1, "flip_lr"}, {&yolo_augment_image::flip_ud, 2, "flip_ud"},
        {&yolo_augment_image::radius, 10, "radius"}, {&yolo_augment_image::radius, -1, "radius"}, {&yolo_augment_image::radius, 1, "taps"},
        {&yolo_augment_image::tx, std::numeric_limits<int>::min(), "tx"}, {&yolo_augment_image::tx, (1 << 30) + 1, "tx"}};
    for (const auto &b : bad) {
        p = good();
        p.*(b.field) = b.value;
        EXPECT(augment_check(&p, 32, 32, err) == YOLO_ERR_ARG && has(err, b.word));
    }
    for (int i = 0; i < 2; ++i) {
        p = good(); p.noise_q[i] = 16384;
        EXPECT(augment_check(&p, 32, 32, err) == YOLO_ERR_ARG && has(err, "noise_q"));
        p = good(); p.noise_q[i] = -1;
        EXPECT(augment_check(&p, 32, 32, err) == YOLO_ERR_ARG && has(err, "noise_q"));
        p = good(); p.noise_q[i] = 16383; p.noise_loc[i] = 255;
        EXPECT(augment_check(&p, 32, 32, err) == YOLO_OK);
        p = good(); p.noise_loc[i] = 256;
        EXPECT(augment_check(&p, 32, 32, err) == YOLO_ERR_ARG && has(err, "noise_loc"));
        p = good(); p.noise_loc[i] = -256;
        EXPECT(augment_check(&p, 32, 32, err) == YOLO_ERR_ARG && has(err, "noise_loc"));
    }
    p = good(); p.taps[0] = 65535; p.taps[1] = 65535; p.taps[2] = 65535;      // (the sum is taken in 64 bits)
    EXPECT(augment_check(&p, 32, 32, err) == YOLO_ERR_ARG && has(err, "taps"));
    p = good(); p.enabled = 0; p.radius = 77; p.flip_lr = 9;                    // a record that is not enabled is not looked at further
    EXPECT(augment_check(&p, 32, 32, err) == YOLO_OK);

    // the kernel's record
    AugGeom g = augment_geom(p);
    EXPECT(g.radius == 0 && g.flags == 0 && g.taps[0] == 256 && g.taps[1] == 0 && g.tx == 0 && g.drop_thr == 0 && g.loc0 == 0 && g.loc1 == 0);
    p = good();
    g = augment_geom(p);
    EXPECT(g.radius == 2 && g.taps[0] == 100 && g.taps[2] == 18 && g.taps[3] == 0 && g.tx == -40 && g.key1 == 0xffffffffu && g.loc1 == 32);
    EXPECT(g.flags == (AUG_FLIP_LR | AUG_DRAW0));                               // 131070 * 11 < 2^23: no generator call for step 1
    p.noise_q[1] = 65; p.noise_q[0] = 0; p.drop_thr = 0; p.flip_lr = 0; p.flip_ud = 1;
    EXPECT(augment_geom(p).flags == (AUG_FLIP_UD | AUG_DRAW1));                 // 131070 * 65 >= 2^23 > 131070 * 64
    p.noise_q[1] = 64;
    EXPECT(augment_geom(p).flags == AUG_FLIP_UD);
    p.drop_thr = 1;
    EXPECT(augment_geom(p).flags == (AUG_FLIP_UD | AUG_DRAW0));

    // the checks of a call never touch what the pointers point at: host memory stands in for device memory
    std::vector<unsigned char> buf(2 * 3 * 8 * 8 * 3);
    std::vector<yolo_augment_image> recs(3, good());
    for (auto &r : recs) r.radius = 0, r.taps[0] = 256;
    unsigned char *a = buf.data(), *b = buf.data() + 3 * 8 * 8 * 3;
    EXPECT(augment_call_check(a, b, 3, 8, 8, recs.data(), err) == YOLO_OK);
    EXPECT(augment_call_check(a, b - 1, 3, 8, 8, recs.data(), err) == YOLO_ERR_ARG && has(err, "overlap"));
    EXPECT(augment_call_check(b, a, 3, 8, 8, recs.data(), err) == YOLO_OK);
    EXPECT(augment_call_check(a, a, 3, 8, 8, recs.data(), err) == YOLO_ERR_ARG && has(err, "overlap"));
    EXPECT(augment_call_check(nullptr, b, 3, 8, 8, recs.data(), err) == YOLO_ERR_ARG && has(err, "null"));
    EXPECT(augment_call_check(a, b, 0, 8, 8, recs.data(), err) == YOLO_ERR_ARG);
    recs[2].radius = 11;
    EXPECT(augment_call_check(a, b, 3, 8, 8, recs.data(), err) == YOLO_ERR_ARG && has(err, "image 2: radius"));

    // truths: a 100-wide image, shift +25 px
    p = good(); p.flip_lr = 0; p.tx = 25;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<yolo_gt> in = {{0.5f, 0.5f, 0.2f, 0.2f, 3, 0},       // inside: moves by 0.25
                               {0.8f, 0.5f, 0.2f, 0.4f, 1, 1},       // across the right edge after the shift: cut
                               {0.9f, 0.5f, 0.1f, 0.1f, 2, 0},       // fully out: dropped
                               {0.5f, nan, 0.1f, 0.1f, 2, 0},        // NaN: dropped
                               {0.5f, 1.5f, 0.1f, 0.2f, 2, 0},       // below the image: dropped
                               {0.1f, 0.0f, 0.2f, 0.5f, 7, 0}};      // across the top edge: cut
    std::vector<yolo_gt> out(in.size());
    int32_t n_out = -1;
    EXPECT(augment_truths(in.data(), (int)in.size(), &p, 40, 100, out.data(), &n_out, err) == YOLO_OK && n_out == 3);
    EXPECT(out[0].class_idx == 3 && out[0].x == (float)((((double)0.5f - (double)0.2f / 2) + 0.25 + (((double)0.5f + (double)0.2f / 2) + 0.25)) / 2));
    EXPECT(out[1].class_idx == 1 && out[1].difficult == 1 && out[1].x + out[1].w / 2 <= 1.0f + 1e-6f && out[1].w < 0.2f);
    EXPECT(out[2].class_idx == 7 && out[2].y == 0.125f && out[2].h == 0.25f);
    for (int i = 0; i < n_out; ++i)
        EXPECT(out[i].x - out[i].w / 2 >= -1e-6f && out[i].x + out[i].w / 2 <= 1 + 1e-6f && out[i].y - out[i].h / 2 >= -1e-6f && out[i].y + out[i].h / 2 <= 1 + 1e-6f);
    // both flips of a box, in place; twice gives the box back up to the roundings
    p = good(); p.flip_lr = 1; p.flip_ud = 1; p.tx = 0;
    std::vector<yolo_gt> one = {{0.25f, 0.75f, 0.25f, 0.25f, 0, 0}};
    EXPECT(augment_truths(one.data(), 1, &p, 40, 100, one.data(), &n_out, err) == YOLO_OK && n_out == 1 && one[0].x == 0.75f && one[0].y == 0.25f);
    // not enabled: a copy, NaN and all; no truths; many truths
    p.enabled = 0;
    EXPECT(augment_truths(in.data(), (int)in.size(), &p, 40, 100, out.data(), &n_out, err) == YOLO_OK && n_out == (int)in.size() && out[3].y != out[3].y);
    p = good();
    EXPECT(augment_truths(nullptr, 0, &p, 40, 100, nullptr, &n_out, err) == YOLO_OK && n_out == 0);
    EXPECT(augment_truths(nullptr, 1, &p, 40, 100, out.data(), &n_out, err) == YOLO_ERR_ARG);
    EXPECT(augment_truths(in.data(), -1, &p, 40, 100, out.data(), &n_out, err) == YOLO_ERR_ARG);
    EXPECT(augment_truths(in.data(), 1, &p, 40, 100, out.data(), nullptr, err) == YOLO_ERR_ARG);
    std::vector<yolo_gt> many(1024), many_out(1024);
    for (int i = 0; i < 1024; ++i) many[i] = yolo_gt{(float)i / 1024.f, 0.5f, 0.05f, 0.1f, i, 0};
    EXPECT(augment_truths(many.data(), 1024, &p, 40, 100, many_out.data(), &n_out, err) == YOLO_OK && n_out > 0 && n_out <= 1024);
    for (int i = 1; i < n_out; ++i) EXPECT(many_out[i].class_idx > many_out[i - 1].class_idx);      // the order is kept

    if (failures) {
        std::fprintf(stderr, "augment_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("augment_host_check OK\n");
    return 0;
}

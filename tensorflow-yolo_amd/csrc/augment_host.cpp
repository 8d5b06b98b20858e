// Host side of the augmentation entries: the argument checks, the kernel's record and the truths (augment_host.h).  Plain C++.
#include "augment_host.h"

namespace yolo {

int augment_check(const yolo_augment_image *p, int h, int w, std::string &err) {
    if (!p) { err = "null argument"; return YOLO_ERR_ARG; }
    if (h < 1 || w < 1) { err = "h and w must be at least 1"; return YOLO_ERR_ARG; }
    if (w % 4) { err = "w must be a multiple of 4"; return YOLO_ERR_ARG; }
    if ((long long)h * w > 0x7fffffffLL) { err = "h * w must fit 31 bits"; return YOLO_ERR_ARG; }
    if (p->enabled != 0 && p->enabled != 1) { err = "enabled must be 0 or 1"; return YOLO_ERR_ARG; }
    if (!p->enabled) return YOLO_OK;
    if (p->flip_lr != 0 && p->flip_lr != 1) { err = "flip_lr must be 0 or 1"; return YOLO_ERR_ARG; }
    if (p->flip_ud != 0 && p->flip_ud != 1) { err = "flip_ud must be 0 or 1"; return YOLO_ERR_ARG; }
    if (p->radius < 0 || p->radius > kAugMaxRadius) { err = "radius must be 0 .. 9"; return YOLO_ERR_ARG; }
    if (p->radius >= h || p->radius >= w) { err = "radius must be below h and w (the border is reflected once)"; return YOLO_ERR_ARG; }
    long long sum = p->taps[0];
    for (int k = 1; k <= p->radius; ++k) sum += 2LL * p->taps[k];
    if (sum != 256) { err = "taps[0] + 2 * (taps[1] + .. + taps[radius]) must be 256, got " + std::to_string(sum); return YOLO_ERR_ARG; }
    for (int i = 0; i < 2; ++i) {
        if (p->noise_q[i] < 0 || p->noise_q[i] > 16383) { err = "noise_q must be 0 .. 16383"; return YOLO_ERR_ARG; }
        if (p->noise_loc[i] < -255 || p->noise_loc[i] > 255) { err = "noise_loc must be -255 .. 255"; return YOLO_ERR_ARG; }
    }
    if (p->tx < -(1 << 30) || p->tx > (1 << 30)) { err = "tx must be -2^30 .. 2^30"; return YOLO_ERR_ARG; }
    return YOLO_OK;
}

int augment_call_check(const void *src, const void *dst, int n, int h, int w, const yolo_augment_image *params, std::string &err) {
    if (!src || !dst || !params) { err = "null argument"; return YOLO_ERR_ARG; }
    if (n < 1) { err = "the image count must be at least 1"; return YOLO_ERR_ARG; }
    for (int i = 0; i < n; ++i) {
        const int rc = augment_check(params + i, h, w, err);
        if (rc) { err = "image " + std::to_string(i) + ": " + err; return rc; }
    }
    const uint64_t bytes = (uint64_t)n * (uint64_t)h * (uint64_t)w * 3u;
    const uint64_t a = (uint64_t)(uintptr_t)src, b = (uint64_t)(uintptr_t)dst;
    if (a < b + bytes && b < a + bytes) { err = "src and dst must not overlap"; return YOLO_ERR_ARG; }
    return YOLO_OK;
}

AugGeom augment_geom(const yolo_augment_image &p) {
    AugGeom g = {};
    g.taps[0] = 256;
    if (!p.enabled) return g;
    g.drop_thr = p.drop_thr; g.key0 = p.key[0]; g.key1 = p.key[1];
    g.q0 = p.noise_q[0]; g.q1 = p.noise_q[1]; g.loc0 = p.noise_loc[0]; g.loc1 = p.noise_loc[1]; g.tx = p.tx;
    for (int k = 0; k <= p.radius; ++k) g.taps[k] = p.taps[k];
    g.radius = (uint8_t)p.radius;
    // |s| <= 131070: below this product the rounded shift of step 5 gives 0 for every s
    const bool d0 = 131070LL * p.noise_q[0] >= (1LL << 23), d1 = 131070LL * p.noise_q[1] >= (1LL << 23);
    g.flags = (uint8_t)((p.flip_lr ? AUG_FLIP_LR : 0) | (p.flip_ud ? AUG_FLIP_UD : 0) | ((p.drop_thr || d0) ? AUG_DRAW0 : 0) | (d1 ? AUG_DRAW1 : 0));
    return g;
}

// float64, every operation rounded on its own (no contraction: a fused 1 - x2 or x1 + tx / W would round differently from NumPy)
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
int augment_truths(const yolo_gt *in, int n_in, const yolo_augment_image *p, int h, int w, yolo_gt *out, int32_t *n_out, std::string &err) {
    if (!p || !n_out || (n_in > 0 && (!in || !out))) { err = "null argument"; return YOLO_ERR_ARG; }
    if (n_in < 0) { err = "n_in must not be negative"; return YOLO_ERR_ARG; }
    const int rc = augment_check(p, h, w, err);
    if (rc) return rc;
    if (!p->enabled) {
        for (int i = 0; i < n_in; ++i) out[i] = in[i];
        *n_out = n_in;
        return YOLO_OK;
    }
    const double shift = (double)p->tx / (double)w;
    int n = 0;
    for (int i = 0; i < n_in; ++i) {
        const yolo_gt t = in[i];
        double x1 = (double)t.x - (double)t.w / 2.0, x2 = (double)t.x + (double)t.w / 2.0;
        double y1 = (double)t.y - (double)t.h / 2.0, y2 = (double)t.y + (double)t.h / 2.0;
        if (p->flip_lr) { const double a = 1.0 - x2, b = 1.0 - x1; x1 = a; x2 = b; }
        if (p->flip_ud) { const double a = 1.0 - y2, b = 1.0 - y1; y1 = a; y2 = b; }
        x1 = x1 + shift;
        x2 = x2 + shift;
        if (x1 != x1 || x2 != x2 || y1 != y1 || y2 != y2) continue;
        if (x2 <= 0.0 || x1 >= 1.0 || y2 <= 0.0 || y1 >= 1.0) continue;
        x1 = x1 < 0.0 ? 0.0 : (x1 > 1.0 ? 1.0 : x1); x2 = x2 < 0.0 ? 0.0 : (x2 > 1.0 ? 1.0 : x2);
        y1 = y1 < 0.0 ? 0.0 : (y1 > 1.0 ? 1.0 : y1); y2 = y2 < 0.0 ? 0.0 : (y2 > 1.0 ? 1.0 : y2);
        yolo_gt o = t;
        o.x = (float)((x1 + x2) / 2.0); o.w = (float)(x2 - x1);
        o.y = (float)((y1 + y2) / 2.0); o.h = (float)(y2 - y1);
        out[n++] = o;
    }
    *n_out = n;
    return YOLO_OK;
}

}  // namespace yolo

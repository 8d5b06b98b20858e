// Host side of the anchor k-means entries: the plan, the argument checks, the kernel argument and the stop rule's threshold
// (anchor_host.h).  Plain C++.
#include "anchor_host.h"

#include <cstring>

namespace yolo {

namespace {
inline unsigned long long up256(unsigned long long b) { return (b + 255ull) & ~255ull; }
}  // namespace

int anchor_desc_check(const yolo_anchor_desc *d, long long n, std::string &err) {
    if (!d) { err = "null argument"; return YOLO_ERR_ARG; }
    if (n < 1 || n > YOLO_ANCHOR_MAX_N) { err = "n must be 1 .. 2^22, got " + std::to_string(n); return YOLO_ERR_ARG; }
    if (d->k < 1 || d->k > YOLO_ANCHOR_MAX_K) { err = "k must be 1 .. 32, got " + std::to_string(d->k); return YOLO_ERR_ARG; }
    if (d->n_init < 1 || d->n_init > YOLO_ANCHOR_MAX_INIT) { err = "n_init must be 1 .. 64, got " + std::to_string(d->n_init); return YOLO_ERR_ARG; }
    if (d->max_iter < 1 || d->max_iter > YOLO_ANCHOR_ITER_LIMIT) { err = "max_iter must be 1 .. 10000, got " + std::to_string(d->max_iter); return YOLO_ERR_ARG; }
    if (d->distance != YOLO_ANCHOR_EUCLIDEAN && d->distance != YOLO_ANCHOR_IOU) {
        err = "distance must be YOLO_ANCHOR_EUCLIDEAN or YOLO_ANCHOR_IOU, got " + std::to_string(d->distance);
        return YOLO_ERR_ARG;
    }
    if (!(d->tolerate >= 0.0) || d->tolerate > 1.7976931348623157e308) { err = "tolerate must be finite and not negative"; return YOLO_ERR_ARG; }
    return YOLO_OK;
}

int anchor_plan(const yolo_anchor_desc *d, long long n, struct yolo_anchor_plan *out, std::string &err) {
    if (!out) { err = "null argument"; return YOLO_ERR_ARG; }
    const int rc = anchor_desc_check(d, n, err);
    if (rc) return rc;
    struct yolo_anchor_plan pl;
    memset(&pl, 0, sizeof pl);
    pl.chunk = kAnchorChunk;
    pl.n_chunks = (int32_t)((n + kAnchorChunk - 1) / kAnchorChunk);
    pl.period = kAnchorPeriod;
    pl.threads = kAnchorBlock;
    const unsigned long long un = (unsigned long long)n, ri = (unsigned long long)d->n_init;
    unsigned long long o = 0;
    pl.prep_offset = o; o += sizeof(AnchorPrep);
    pl.pick_offset = o; o += sizeof(AnchorPick);
    pl.state_offset = o; o += up256(ri * sizeof(AnchorRestart));
    pl.q_offset = o; o += up256(un * 16ull);
    pl.label_stride = up256(un);
    pl.label_offset = o; o += ri * pl.label_stride;
    pl.sums_offset = o; o += up256(ri * (unsigned long long)pl.n_chunks * 8ull);
    pl.scratch_bytes = o;
    o = 0;
    pl.header_offset = o; o += up256(sizeof(yolo_anchor_header));
    pl.restarts_offset = o; o += up256(ri * sizeof(yolo_anchor_restart));
    pl.best_offset = o; o += up256(sizeof(yolo_anchor_best));
    pl.result_bytes = o;
    *out = pl;
    return YOLO_OK;
}

int anchor_call_check(const yolo_anchor_desc *d, const void *wh, long long n, const void *init, const void *scratch, size_t scratch_bytes,
                      const void *result, size_t result_bytes, const void *labels, std::string &err) {
    struct yolo_anchor_plan pl;
    const int rc = anchor_plan(d, n, &pl, err);
    if (rc) return rc;
    if (!wh || !scratch || !result) { err = "null argument"; return YOLO_ERR_ARG; }
    if (init && d->n_init != 1) { err = "n_init must be 1 when init is given, got " + std::to_string(d->n_init); return YOLO_ERR_ARG; }
    if ((uintptr_t)wh % 8 || (init && (uintptr_t)init % 8)) { err = "wh and init must be 8-byte aligned"; return YOLO_ERR_ARG; }
    if ((uintptr_t)scratch % 256 || (uintptr_t)result % 256) { err = "scratch and result must be 256-byte aligned"; return YOLO_ERR_ARG; }
    if (labels && (uintptr_t)labels % 4) { err = "labels must be 4-byte aligned"; return YOLO_ERR_ARG; }
    if (scratch_bytes < pl.scratch_bytes) {
        err = "scratch of " + std::to_string(scratch_bytes) + " bytes, the plan needs " + std::to_string(pl.scratch_bytes);
        return YOLO_ERR_ARG;
    }
    if (result_bytes < pl.result_bytes) {
        err = "result of " + std::to_string(result_bytes) + " bytes, the plan needs " + std::to_string(pl.result_bytes);
        return YOLO_ERR_ARG;
    }
    const unsigned long long s0 = (unsigned long long)(uintptr_t)scratch, s1 = s0 + pl.scratch_bytes;
    struct { const void *p; unsigned long long bytes; const char *name; } others[] = {
        {wh, (unsigned long long)n * 16ull, "wh"}, {init, (unsigned long long)d->k * 16ull, "init"},
        {result, pl.result_bytes, "result"}, {labels, (unsigned long long)n * 4ull, "labels"}};
    for (const auto &o : others) {
        if (!o.p) continue;
        const unsigned long long a = (unsigned long long)(uintptr_t)o.p;
        if (a < s1 && s0 < a + o.bytes) { err = std::string(o.name) + " must not overlap the scratch"; return YOLO_ERR_ARG; }
    }
    return YOLO_OK;
}

AnchorParams anchor_params(const yolo_anchor_desc &d, const struct yolo_anchor_plan &pl, const void *wh, int n, const void *init, void *scratch,
                           void *result, void *labels) {
    AnchorParams p;
    memset(&p, 0, sizeof p);
    unsigned char *s = static_cast<unsigned char *>(scratch);
    p.wh = static_cast<const double *>(wh);
    p.init = static_cast<const double *>(init);
    p.q = reinterpret_cast<unsigned long long *>(s + pl.q_offset);
    p.prep = reinterpret_cast<AnchorPrep *>(s + pl.prep_offset);
    p.state = reinterpret_cast<AnchorRestart *>(s + pl.state_offset);
    p.pick = reinterpret_cast<AnchorPick *>(s + pl.pick_offset);
    p.label8 = s + pl.label_offset;
    p.chunk_sum = reinterpret_cast<unsigned long long *>(s + pl.sums_offset);
    p.result = static_cast<unsigned char *>(result);
    p.labels = static_cast<int32_t *>(labels);
    p.label_stride = pl.label_stride;
    p.header_offset = pl.header_offset; p.restarts_offset = pl.restarts_offset; p.best_offset = pl.best_offset;
    p.seed = d.seed;
    p.n = n; p.k = d.k; p.n_init = d.n_init; p.max_iter = d.max_iter; p.distance = d.distance; p.n_chunks = pl.n_chunks;
    return p;
}

double anchor_u128_to_double(unsigned __int128 v) {
    const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
    if (!hi) return (double)lo;                         // one correctly rounded conversion
    int lz = 0;
    while (!((hi << lz) >> 63)) ++lz;
    // the top 64 bits with everything below them folded into the last one (a sticky bit: 64 bits are more than 53 + 2, so rounding
    // them rounds the whole number the same way)
    const int shift = 64 - lz;                          // 1 .. 64 bits are dropped
    unsigned long long top = (unsigned long long)(v >> shift);
    const unsigned __int128 dropped = v - ((unsigned __int128)top << shift);
    if (dropped) top |= 1ull;
    double r = (double)top;
    for (int i = 0; i < shift; ++i) r *= 2.0;           // exact
    return r;
}

// float64, every operation rounded on its own
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
double anchor_threshold(const AnchorPrep &p, double tolerate) {
    if (!p.n_valid) return 0.0;
    double var[2];
    for (int c = 0; c < 2; ++c) {
        const unsigned __int128 sq = ((unsigned __int128)p.hh[c] << 40) + ((unsigned __int128)p.hl[c] << 21) + (unsigned __int128)p.ll[c];
        const unsigned __int128 N = (unsigned __int128)p.n_valid * sq - (unsigned __int128)p.sum[c] * (unsigned __int128)p.sum[c];
        const double nn = (double)p.n_valid * (double)p.n_valid;
        var[c] = anchor_u128_to_double(N) / nn * 0x1p-80;
    }
    return tolerate * ((var[0] + var[1]) / 2.0);
}

}  // namespace yolo

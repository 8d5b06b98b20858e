// A program of its own for the host side of the anchor k-means entries (anchor_host.cpp): walks the plan over the sizes at its edges, every
// refusal over its message, the kernel argument over the layout, and the threshold over sums whose 128-bit join is known, and verifies what
// the header promises.  `make san-anchor` builds it with AddressSanitizer + UndefinedBehaviorSanitizer and runs it on the CPU; no device,
// no HIP.  Exit status 0 and "anchor_host_check OK" when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "anchor_host.h"

using namespace yolo;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
        }                                                                  \
    } while (0)

static yolo_anchor_desc good() {
    yolo_anchor_desc d = {};
    d.k = 5; d.n_init = 10; d.max_iter = 300; d.distance = YOLO_ANCHOR_EUCLIDEAN; d.tolerate = 0.005; d.seed = 0;
    return d;
}

static bool has(const std::string &s, const char *word) { return s.find(word) != std::string::npos; }

int main() {
    std::string err;
    yolo_anchor_desc d = good();
    struct yolo_anchor_plan pl;

    // the plan at the edges of n
    for (long long n : {1LL, 2LL, 1023LL, 1024LL, 1025LL, 2051LL, (long long)YOLO_ANCHOR_MAX_N}) {
        EXPECT(anchor_plan(&d, n, &pl, err) == YOLO_OK);
        EXPECT(pl.chunk == 1024 && pl.threads == 256 && pl.period == 8 && pl.n_chunks == (n + 1023) / 1024);
        const uint64_t parts[] = {pl.prep_offset, pl.pick_offset, pl.state_offset, pl.q_offset, pl.label_offset, pl.sums_offset, pl.scratch_bytes};
        for (size_t i = 0; i < sizeof parts / sizeof parts[0]; ++i) {
            EXPECT(parts[i] % 256 == 0);
            if (i) EXPECT(parts[i] > parts[i - 1]);
        }
        EXPECT(pl.pick_offset - pl.prep_offset >= sizeof(AnchorPrep) && pl.state_offset - pl.pick_offset >= sizeof(AnchorPick));
        EXPECT(pl.q_offset - pl.state_offset >= 10 * sizeof(AnchorRestart) && pl.label_offset - pl.q_offset >= (uint64_t)n * 16);
        EXPECT(pl.label_stride % 256 == 0 && pl.label_stride >= (uint64_t)n && pl.sums_offset - pl.label_offset == 10 * pl.label_stride);
        EXPECT(pl.scratch_bytes - pl.sums_offset >= 10ull * pl.n_chunks * 8);
        EXPECT(pl.header_offset == 0 && pl.restarts_offset == 256 && pl.best_offset == 256 + 1536 && pl.result_bytes == pl.best_offset + 1536);
    }
    static_assert(sizeof(yolo_anchor_header) == 32 && sizeof(yolo_anchor_restart) == 152 && sizeof(yolo_anchor_best) == 1312, "the result's records");
    d.n_init = 64; d.k = 32;
    EXPECT(anchor_plan(&d, YOLO_ANCHOR_MAX_N, &pl, err) == YOLO_OK && pl.scratch_bytes < (1ull << 29));

    // every refusal of the sizes
    struct { int32_t yolo_anchor_desc::*field; int value; const char *word; } bad[] = {
        {&yolo_anchor_desc::k, 0, "k must be"}, {&yolo_anchor_desc::k, 33, "k must be"}, {&yolo_anchor_desc::n_init, 0, "n_init must be"},
        {&yolo_anchor_desc::n_init, 65, "n_init must be"}, {&yolo_anchor_desc::max_iter, 0, "max_iter must be"},
        {&yolo_anchor_desc::max_iter, 10001, "max_iter must be"}, {&yolo_anchor_desc::distance, 2, "distance must be"},
        {&yolo_anchor_desc::distance, -1, "distance must be"}};
    for (const auto &b : bad) {
        d = good();
        d.*(b.field) = b.value;
        EXPECT(anchor_plan(&d, 100, &pl, err) == YOLO_ERR_ARG && has(err, b.word));
    }
    d = good();
    EXPECT(anchor_plan(&d, 0, &pl, err) == YOLO_ERR_ARG && has(err, "n must be"));
    EXPECT(anchor_plan(&d, (long long)YOLO_ANCHOR_MAX_N + 1, &pl, err) == YOLO_ERR_ARG && has(err, "n must be"));
    EXPECT(anchor_plan(&d, -5, &pl, err) == YOLO_ERR_ARG && has(err, "n must be"));
    EXPECT(anchor_plan(nullptr, 5, &pl, err) == YOLO_ERR_ARG && has(err, "null"));
    EXPECT(anchor_plan(&d, 5, nullptr, err) == YOLO_ERR_ARG && has(err, "null"));
    for (double t : {-1.0, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
        d = good(); d.tolerate = t;
        EXPECT(anchor_plan(&d, 5, &pl, err) == YOLO_ERR_ARG && has(err, "tolerate"));
    }
    d = good(); d.tolerate = 0.0;
    EXPECT(anchor_plan(&d, 5, &pl, err) == YOLO_OK);

    // the checks of a call never touch what the pointers point at: host memory stands in for device memory
    d = good();
    const long long n = 1500;
    EXPECT(anchor_plan(&d, n, &pl, err) == YOLO_OK);
    std::vector<unsigned char> arena(pl.scratch_bytes + pl.result_bytes + n * 16 + n * 4 + 5 * 16 + 1024);
    unsigned char *base = arena.data() + (256 - (uintptr_t)arena.data() % 256) % 256;
    unsigned char *scratch = base, *result = scratch + pl.scratch_bytes, *wh = result + pl.result_bytes, *labels = wh + n * 16, *init = labels + n * 4;
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_OK);
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes, result, pl.result_bytes, nullptr, err) == YOLO_OK);
    EXPECT(anchor_call_check(&d, nullptr, n, nullptr, scratch, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "null"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, nullptr, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "null"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes, nullptr, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "null"));
    EXPECT(anchor_call_check(&d, wh, n, init, scratch, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "n_init must be 1 when init"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes - 1, result, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "scratch of"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes, result, pl.result_bytes - 1, labels, err) == YOLO_ERR_ARG && has(err, "result of"));
    EXPECT(anchor_call_check(&d, wh + 4, n, nullptr, scratch, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "8-byte"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch + 128, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "256-byte"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes, result + 8, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "256-byte"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes, result, pl.result_bytes, labels + 2, err) == YOLO_ERR_ARG && has(err, "4-byte"));
    EXPECT(anchor_call_check(&d, scratch + 512, n, nullptr, scratch, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "wh must not overlap"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes, scratch + 256, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "result must not overlap"));
    EXPECT(anchor_call_check(&d, wh, n, nullptr, scratch, pl.scratch_bytes, result, pl.result_bytes, scratch + pl.scratch_bytes - 4, err) == YOLO_ERR_ARG && has(err, "labels must not overlap"));
    d.n_init = 1;
    EXPECT(anchor_plan(&d, n, &pl, err) == YOLO_OK);
    EXPECT(anchor_call_check(&d, wh, n, init, scratch, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_OK);
    EXPECT(anchor_call_check(&d, wh, n, scratch + 256, scratch, pl.scratch_bytes, result, pl.result_bytes, labels, err) == YOLO_ERR_ARG && has(err, "init must not overlap"));

    // the kernel argument: every part inside the scratch, in the plan's places
    d = good();
    EXPECT(anchor_plan(&d, n, &pl, err) == YOLO_OK);
    const AnchorParams p = anchor_params(d, pl, wh, (int)n, nullptr, scratch, result, labels);
    EXPECT((unsigned char *)p.prep == scratch + pl.prep_offset && (unsigned char *)p.pick == scratch + pl.pick_offset);
    EXPECT((unsigned char *)p.state == scratch + pl.state_offset && (unsigned char *)p.q == scratch + pl.q_offset);
    EXPECT(p.label8 == scratch + pl.label_offset && (unsigned char *)p.chunk_sum == scratch + pl.sums_offset && p.label_stride == pl.label_stride);
    EXPECT((unsigned char *)(p.chunk_sum + (size_t)d.n_init * pl.n_chunks) <= scratch + pl.scratch_bytes);
    EXPECT(p.n == n && p.k == 5 && p.n_init == 10 && p.max_iter == 300 && p.n_chunks == 2 && p.round == 0 && p.threshold == 0.0 && p.init == nullptr);

    // 128 bits to float64: exact below 2^53, ties to even above, a sticky bit far below the tie
    EXPECT(anchor_u128_to_double(0) == 0.0 && anchor_u128_to_double(12345) == 12345.0);
    const unsigned __int128 one = 1;
    EXPECT(anchor_u128_to_double(one << 100) == std::ldexp(1.0, 100));
    EXPECT(anchor_u128_to_double((one << 100) + (one << 47)) == std::ldexp(1.0, 100));                           // a tie: to even (down)
    EXPECT(anchor_u128_to_double((one << 100) + (one << 47) + 1) == std::ldexp(1.0, 100) + std::ldexp(1.0, 48));  // just above the tie
    EXPECT(anchor_u128_to_double((one << 100) + (one << 48) + (one << 47)) == std::ldexp(1.0, 100) + std::ldexp(1.0, 49));   // a tie: to even (up)
    EXPECT(anchor_u128_to_double(~(unsigned __int128)0) == std::ldexp(1.0, 128));
    EXPECT(anchor_u128_to_double((one << 64) + 1) == std::ldexp(1.0, 64));
    EXPECT(anchor_u128_to_double(((unsigned __int128)0xffffffffffffffffull << 1) + 1) == std::ldexp(1.0, 65));

    // the threshold: two boxes (1/4, 1/2) and (3/4, 1/2) -> var_w = 1/16, var_h = 0, mean 1/32
    AnchorPrep prep = {};
    const unsigned long long q[2][2] = {{1ull << 38, 1ull << 39}, {3ull << 38, 1ull << 39}};
    prep.n_valid = 2;
    for (const auto &b : q)
        for (int c = 0; c < 2; ++c) {
            const unsigned long long hi = b[c] >> 20, lo = b[c] & 0xfffff;
            prep.sum[c] += b[c]; prep.hh[c] += hi * hi; prep.hl[c] += hi * lo; prep.ll[c] += lo * lo;
        }
    EXPECT(anchor_threshold(prep, 1.0) == 1.0 / 32.0 && anchor_threshold(prep, 0.005) == 0.005 * (1.0 / 32.0) && anchor_threshold(prep, 0.0) == 0.0);
    prep.n_valid = 0;
    EXPECT(anchor_threshold(prep, 1.0) == 0.0);
    // the largest sums there can be: 2^22 boxes of q = 2^40 (variance 0) -- nothing overflows 128 bits
    AnchorPrep big = {};
    big.n_valid = 1ull << 22;
    for (int c = 0; c < 2; ++c) { big.sum[c] = 1ull << 62; big.hh[c] = 1ull << 62; }
    EXPECT(anchor_threshold(big, 1.0) == 0.0);

    if (failures) {
        std::fprintf(stderr, "anchor_host_check: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("anchor_host_check OK\n");
    return 0;
}

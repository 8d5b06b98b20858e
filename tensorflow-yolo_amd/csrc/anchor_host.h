// Host side of the anchor k-means entries (include/yolo_hip.h "Anchor k-means on the device": yolo_anchor_plan, yolo_anchor_kmeans): the plan
// (chunk size, chunk count, period, the layout of the scratch and of the result, every part 256-byte aligned), every argument check in
// front of a launch, the stop rule's threshold from the exact sums of the prepare kernel, and the records the kernels share.  No HIP here:
// anchor_host.cpp compiles as plain C++, so that anchor_host_check.cpp (a program with its own main) runs it under AddressSanitizer +
// UndefinedBehaviorSanitizer on a CPU (`make san-anchor`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "yolo_hip.h"

namespace yolo {

// anchor.hip: a workgroup of kAnchorBlock threads takes one chunk of kAnchorChunk boxes of one restart (kAnchorChunk / kAnchorBlock boxes
// per thread); the host reads the count of finished restarts in front of every batch of kAnchorPeriod enqueued iterations
constexpr int kAnchorChunk = 1024, kAnchorBlock = 256, kAnchorPeriod = 8;

// What the prepare kernel leaves (scratch, prep_offset): the counts and the exact sums the variance is made of.  A quantised value is
// q = hi * 2^20 + lo (hi <= 2^20, lo < 2^20), so q^2 = hi^2 * 2^40 + hi * lo * 2^21 + lo^2 and each of the three sums over at most 2^22
// boxes stays below 2^63: SPLIT accumulation in 64-bit integer atomics, put together in 128 bits on the host (anchor_threshold).
struct AnchorPrep {
    unsigned long long n_valid, n_bad;
    unsigned long long sum[2];          // sum of q: [0] widths, [1] heights
    unsigned long long hh[2], hl[2], ll[2];
    unsigned long long n_done;          // restarts that have stopped: the one word the host reads between batches of iterations
    unsigned long long pad_[21];
};
static_assert(sizeof(AnchorPrep) == 256, "AnchorPrep is one 256-byte part");

// One restart's record (scratch, state_offset + restart * sizeof): written by the init / seeding kernels, then by the update kernel of every
// iteration (one thread), summed into by the iteration kernel's integer atomics.
struct AnchorRestart {
    double centre[YOLO_ANCHOR_MAX_K][2];                // the current centres (w, h)
    unsigned long long acc[YOLO_ANCHOR_MAX_K][3];       // this iteration: sum of q_w, sum of q_h, count; zeroed by the update kernel
    unsigned long long fin[YOLO_ANCHOR_MAX_K][3];       // the final assignment: the same three
    unsigned long long changed;                         // boxes whose label differs from the iteration before
    unsigned long long inertia_q, iou_q;                // the final assignment: sum of floor(d * 2^40), sum of floor(best IoU * 2^40)
    int32_t seed[YOLO_ANCHOR_MAX_K];                    // box index of seed j; -1: not drawn
    int32_t n_iter, done;
    uint32_t status;
    int32_t pad_;
};
static_assert(sizeof(AnchorRestart) % 8 == 0, "AnchorRestart holds 64-bit words");

// What the finish kernel leaves for the label kernel (scratch, pick_offset: a part of its own)
struct AnchorPick {
    int32_t best;                                       // -1: every restart degenerate
    int32_t rank[YOLO_ANCHOR_MAX_K];                    // cluster index of the best restart -> its place in the order by area
    int32_t pad_[31];
};
static_assert(sizeof(AnchorPick) == 256, "AnchorPick is one 256-byte part");

// The kernel argument of every anchor kernel
struct AnchorParams {
    const double *wh;                   // [n][2] float64, the caller's
    const double *init;                 // [k][2] or null
    unsigned long long *q;              // [n][2]: q_w, q_h; 0, 0 = invalid
    AnchorPrep *prep;
    AnchorRestart *state;               // [n_init]
    AnchorPick *pick;
    unsigned char *label8;              // [n_init][label_stride]: the label of the iteration before; 0xff = none yet
    unsigned long long *chunk_sum;      // [n_init][n_chunks]: seeding
    unsigned char *result;              // the caller's result block
    int32_t *labels;                    // the caller's, or null
    unsigned long long label_stride;
    unsigned long long header_offset, restarts_offset, best_offset;
    unsigned long long seed;
    double threshold;                   // tolerate * mean(var): euclidean only
    int n, k, n_init, max_iter, distance, n_chunks, round, pad_;
};

// 0 or YOLO_ERR_ARG with the message in err (the caller puts the entry's name in front)
int anchor_desc_check(const yolo_anchor_desc *d, long long n, std::string &err);
int anchor_plan(const yolo_anchor_desc *d, long long n, struct yolo_anchor_plan *out, std::string &err);
int anchor_call_check(const yolo_anchor_desc *d, const void *wh, long long n, const void *init, const void *scratch, size_t scratch_bytes,
                      const void *result, size_t result_bytes, const void *labels, std::string &err);
// the kernel argument of a checked call (threshold 0, round 0: the caller sets them)
AnchorParams anchor_params(const yolo_anchor_desc &d, const struct yolo_anchor_plan &pl, const void *wh, int n, const void *init, void *scratch,
                           void *result, void *labels);
// float64 of a 128-bit unsigned integer, rounded to nearest, ties to even (one rounding)
double anchor_u128_to_double(unsigned __int128 v);
// tolerate * mean over the two columns of the population variance of the quantised data: per column N = n * S(q^2) - S(q)^2, an exact
// 128-bit integer, var = float64(N) / (float64(n) * float64(n)) * 2^-80; the mean is (var_w + var_h) / 2; n_valid == 0 gives 0
double anchor_threshold(const AnchorPrep &p, double tolerate);

}  // namespace yolo

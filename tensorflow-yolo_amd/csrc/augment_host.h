// Host side of the augmentation entries (include/yolo_hip.h: yolo_augment_check, yolo_augment_u8, yolo_augment_truths_host,
// yolo_augment_tile): every argument check in front of a launch, the record the kernel reads, and the truths.  No HIP here:
// augment_host.cpp compiles as plain C++, so that augment_host_check.cpp (a program with its own main) runs it under AddressSanitizer +
// UndefinedBehaviorSanitizer on a CPU (`make san-augment`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "yolo_hip.h"

namespace yolo {

// augment_kernel (augment.hip): a workgroup of 256 threads produces kAugTileRows x kAugTileCols pixels of one output image from that
// tile plus a halo of kAugMaxRadius pixels on every side
constexpr int kAugTileRows = 32, kAugTileCols = 64, kAugMaxRadius = 9;
constexpr int kAugPerLaunch = 64;           // records in one launch's kernel argument (64 x 56 bytes + 32: below the 4 KB limit)

// What the kernel reads for one image: the public record with its flags folded into bits.  An image that is not enabled travels as the
// identity (no flip, radius 0, taps[0] = 256, nothing random, no shift): the same code path copies it byte for byte.
enum { AUG_FLIP_LR = 1, AUG_FLIP_UD = 2, AUG_DRAW0 = 4, AUG_DRAW1 = 8 };
struct AugGeom {
    uint32_t drop_thr, key0, key1;
    int32_t q0, q1, loc0, loc1, tx;
    uint16_t taps[10];
    uint8_t radius, flags;      // AUG_DRAW0 / AUG_DRAW1: the generator runs for draw 0 / 1 (a dropout threshold above 0, a noise step whose d can differ from 0)
    uint16_t pad_;
};
static_assert(sizeof(AugGeom) == 56, "AugGeom is 56 bytes: 64 of them fit a kernel argument");
struct AugmentParams {          // the kernel argument of one launch: grid z = image of the launch
    AugGeom g[kAugPerLaunch];
    const unsigned char *src;   // image 0 of this launch, uint8 [n][h][w][3]
    unsigned char *dst;
    int h, w;                   // w % 4 == 0
    int wide;                   // dst is 4-byte aligned: dword stores; else byte stores
    int pad_;
};
static_assert(sizeof(AugmentParams) <= 4096, "a kernel argument holds at most 4 KB");

// 0 or YOLO_ERR_ARG with the message in err
int augment_check(const yolo_augment_image *p, int h, int w, std::string &err);
// the checks of a whole call (every record too: "image i: ...")
int augment_call_check(const void *src, const void *dst, int n, int h, int w, const yolo_augment_image *params, std::string &err);
AugGeom augment_geom(const yolo_augment_image &p);
int augment_truths(const yolo_gt *in, int n_in, const yolo_augment_image *p, int h, int w, yolo_gt *out, int32_t *n_out, std::string &err);

}  // namespace yolo

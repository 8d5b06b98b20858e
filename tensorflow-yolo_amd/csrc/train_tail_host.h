// Host side of the data gradient of the detection layer and of the 3 x 3 weight gradient (include/yolo_hip.h: yolo_conv1x1_dgrad,
// yolo_conv3x3_wgrad_plan, yolo_conv3x3_wgrad, yolo_conv3x3_wgrad_f16_plan, yolo_conv3x3_wgrad_f16): how a 3 x 3 weight-gradient launch is split, its scratch layout and every argument check
// in front of a launch.  No HIP here: train_tail_host.cpp compiles as plain C++, so that train_tail_host_check.cpp (a program with its
// own main) runs it under AddressSanitizer + UndefinedBehaviorSanitizer on a CPU (`make san-tail`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "yolo_hip.h"

namespace yolo {

// conv3x3_wgrad_kernel (train_tail.hip): a workgroup owns kTailTileCout couts x (9 taps x kTailTileCin channels) of dW3 and walks its
// chunk of positions kTailTilePos at a time, with the kTailTilePos + 2 w + 2 halo positions of its channels in LDS
constexpr int kTailTileCout = 64, kTailTileCin = 64, kTailTilePos = 32;
constexpr int kTailTargetGrid = 512;        // workgroups a launch aims at: two per CU
constexpr int kTailMinChunk = 32;           // positions a chunk holds at least
constexpr int kTailMaxW = 80;               // (kTailTilePos + 2 w + 2) rows of kTailTileCin floats + the D tile stay inside 64 KiB of LDS
// conv1x1_dgrad_kernel: a workgroup owns kDgradTileCin channels x kDgradTilePos positions of D and walks cout kDgradTileK at a time
constexpr int kDgradTileCin = 128, kDgradTilePos = 64, kDgradTileK = 16;

// conv3x3_wgrad_f16_kernel (train_tail_f16.hip): the same ownership on the fp16 matrix cores.  A workgroup walks its chunk kTailF16TilePos
// positions at a time; its LDS images are 16-bit, [position][channel] with rows of kTailF16RowBytes bytes (64 elements and 64 bytes of
// padding: the transposed reads of a 32-lane half then touch every bank once)
constexpr int kTailF16TilePos = 64;
constexpr int kTailF16RowBytes = 192;
constexpr int kTailF16MinChunk = 64;        // positions a chunk holds at least
// (kTailF16TilePos + 2 w + 2) halo rows + the D16 tile + the tap masks (9 x kTailF16TilePos / 2 words + kTailF16TilePos words) stay inside 64 KiB of LDS
constexpr int kTailF16MaxW = 96;
constexpr int kTailF16RecordBytes = 256;    // the m / k record behind the slabs: uint32 bits of m, int32 k
constexpr int kTailF16DbGroups = 64;        // groups of positions whose sums of D are added in group order into db, at most

// 0 or a YOLO_ERR_* code with the message in err
int wgrad3x3_f16_plan(int h, int w, int batch, int cin, int cout, struct yolo_conv3x3_wgrad_f16_plan *out, std::string &err);
// every check of yolo_conv3x3_wgrad_f16 that needs no device; the pointers are never followed.  Fills plan.
int wgrad3x3_f16_check(const void *x_dev, int x_dtype, int ld, int coff, long long image_stride, int h, int w, int batch, int cin,
                       const void *d_dev, int cout, const void *scale_dev, const void *dw_dev, const void *db_dev, const void *scratch_dev,
                       size_t scratch_bytes, struct yolo_conv3x3_wgrad_f16_plan *plan, std::string &err);
int wgrad3x3_plan(int h, int w, int batch, int cin, int cout, int x_dtype, struct yolo_conv3x3_wgrad_plan *out, std::string &err);
// every check of yolo_conv3x3_wgrad that needs no device; the pointers are never followed.  Fills plan.
int wgrad3x3_check(const void *x_dev, int x_dtype, int ld, int coff, long long image_stride, int h, int w, int batch, int cin,
                   const void *d_dev, int cout, const void *scale_dev, const void *dw_dev, const void *db_dev, const void *scratch_dev,
                   size_t scratch_bytes, struct yolo_conv3x3_wgrad_plan *plan, std::string &err);
// the checks of a strided NHWC view that yolo_conv1x1_wgrad makes (shared with train3_tail_host.cpp)
int view_check(const void *dev, int dtype, int ld, int coff, long long image_stride, long long positions_per_image, int cin, std::string &err);
// every check of yolo_conv1x1_dgrad that needs no device; *tiles = the workgroups of the launch
int dgrad_check(const void *g_dev, int cout, const void *w_dev, int cin, const void *y_dev, int y_dtype, int ld, int coff,
                long long image_stride, int positions_per_image, int batch, float slope, const void *d_dev, long long *tiles, std::string &err);

}  // namespace yolo

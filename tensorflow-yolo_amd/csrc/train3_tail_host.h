// Host side of the sparse data gradient of one YOLOv3 head conv (include/yolo_hip.h: yolo_v3_head_dgrad_plan, yolo_v3_head_dgrad): how a
// launch is split over workgroups, the record the kernel reads, and every argument check in front of a launch.  No HIP here:
// train3_tail_host.cpp compiles as plain C++, so that train3_tail_host_check.cpp (a program with its own main) runs it under
// AddressSanitizer + UndefinedBehaviorSanitizer on a CPU (`make san-blocks`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "loss3_host.h"
#include "yolo_hip.h"

namespace yolo {

// head3_dgrad_kernel (train3_tail.hip): a thread owns kDgrad3Lane consecutive channels of one position; the channels are cut into tiles of
// at most kDgrad3TileCin, of which a workgroup serves one; threads_per_position threads make a position, kDgrad3Threads /
// threads_per_position positions a round; a workgroup walks `rounds` rounds of consecutive positions
constexpr int kDgrad3Threads = 256, kDgrad3Lane = 8;
constexpr int kDgrad3TileCin = 1024;                // the objectness rows of a tile lie in LDS: A * 4 KiB at most
constexpr int kDgrad3TargetGroups = 2048;           // workgroups a channel tile aims at: eight per CU

// one launch, as the kernel reads it
struct Dgrad3Params {
    const float *g;             // [B][R][5 + C]
    const int *assign;          // [B][R]: truth index | -1 none | -2 ignored (yolo_v3_loss_grad)
    const float *w;             // [cout][cin], the float32 master kernel
    const void *y;              // element 0 of the view's buffer (fp16 or float32) or null: no activation factor
    float *d;                   // [P][cin]
    long long img_stride;
    int ld, coff, f16, wide;    // the view of Y; wide: every group of kDgrad3Lane channels is 16-byte aligned
    int cin, na, stride, rows, row0, ppi, P, max_gt;    // stride = 5 + C floats per row, rows = R per image, row0 = the scale's first row
    int tile_cin, tiles_cin, tpp, ppr, ppw, groups;     // channels of a tile, tiles, threads per position, positions per round and per
                                                        // workgroup, workgroups per tile
    float slope;
};

// 0 or a YOLO_ERR_* code with the message in err (without the entry's name: the caller puts it in front).  p may be null.
int dgrad3_plan(const yolo_head_desc *head, int scale, int cin, int batch, struct yolo_v3_dgrad_plan *out, Dgrad3Params *p, std::string &err);
// every check of yolo_v3_head_dgrad that needs no device; the pointers are never followed.  Fills plan and p, pointers included.
int dgrad3_check(const yolo_head_desc *head, int scale, const void *g_dev, const void *assign_dev, int max_gt, int batch, const void *w_dev,
                 int cin, const void *y_dev, int y_dtype, int ld, int coff, long long image_stride, float slope, void *d_dev,
                 struct yolo_v3_dgrad_plan *plan, Dgrad3Params *p, std::string &err);

}  // namespace yolo

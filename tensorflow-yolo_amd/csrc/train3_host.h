// Host side of the YOLOv3 head weight gradient (include/yolo_hip.h: yolo_v3_head_wgrad_plan, yolo_v3_head_wgrad): how the objectness part
// and the winner part of a call are split over workgroups, where their scratch lies, and every argument check in front of a launch.  No
// HIP here: train3_host.cpp compiles as plain C++, so that train3_host_check.cpp (a program with its own main) runs it under
// AddressSanitizer + UndefinedBehaviorSanitizer on a CPU (`make san-train3`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "loss3_host.h"
#include "yolo_hip.h"

namespace yolo {

// head3_obj_kernel (train3.hip): a thread owns kWgrad3Lane consecutive channels of one chunk of positions; cin / kWgrad3Lane threads make
// a chunk, chunks are laid one behind the other over workgroups of kWgrad3Threads
constexpr int kWgrad3Threads = 256, kWgrad3Lane = 8;
constexpr int kWgrad3SlotThreads = 1024;                        // head3_slot_kernel: one workgroup per image
constexpr int kWgrad3TargetThreads = 512 * kWgrad3Threads;      // threads the objectness part of ONE scale aims at: two workgroups per CU
constexpr int kWgrad3MinChunk = 64;                             // positions a chunk holds at least
// head3_reduce_kernel: a workgroup owns kWgrad3RedElems elements of the slabs and stages kWgrad3RedChunks chunks of them at a time
constexpr int kWgrad3RedElems = 32, kWgrad3RedChunks = 256;
// head3_win_kernel: a workgroup owns kWgrad3WinTile channels of kWgrad3WinRows rows of dW (consecutive elements k of one anchor)
constexpr int kWgrad3WinTile = 256, kWgrad3WinRows = 32;

// one scale of a call, as the kernels read it (the pointers are filled in by the caller of wgrad3_check)
struct Wgrad3Scale {
    const void *x;              // element 0 of the view's buffer
    float *slab;                // [n_chunks][na * cin + 8]: chunk k's sums of dW's objectness rows, then of db's
    float *dw, *db;             // [cout][cin], [cout]
    long long img_stride;
    int ld, coff, cin, f16, wide;
    int ppi, P, na, row0;       // positions per image (h * w) and of the batch, anchors, first row of the scale inside an image
    int ppc, n_chunks, tpc;     // positions per chunk, chunks, threads per chunk (cin / kWgrad3Lane)
    int obj_blk0, red_blk0, win_blk0;   // first workgroup of the scale in each of the three launches
    int win_tiles, win_ktiles;  // winner part: channel tiles, and tiles of kWgrad3WinRows elements of a row (5 + C), per anchor
};
struct Wgrad3Geometry {
    int n_scales, stride, rows; // stride = 5 + C floats per row, rows = R per image
    int obj_blocks, red_blocks, win_blocks;
    Wgrad3Scale sc[YOLO_MAX_SCALES];
};

// 0 or a YOLO_ERR_* code with the message in err (without the entry's name: the caller puts it in front)
int wgrad3_plan(const yolo_head_desc *head, const int32_t *cin, int batch, int x_dtype, struct yolo_v3_wgrad_plan *out, Wgrad3Geometry *geo,
                std::string &err);
// every check of yolo_v3_head_wgrad that needs no device; the pointers are never followed.  Fills plan and geo, pointers included.
int wgrad3_check(const yolo_head_desc *head, const struct yolo_v3_wgrad_view *views, int batch, const void *g_dev, const void *assign_dev,
                 int max_gt, float *const *dw_dev, float *const *db_dev, void *scratch_dev, size_t scratch_bytes,
                 struct yolo_v3_wgrad_plan *plan, Wgrad3Geometry *geo, std::string &err);

}  // namespace yolo

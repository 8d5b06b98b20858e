// Host side of the head-training entries (include/yolo_hip.h: yolo_wgrad_plan, yolo_conv1x1_wgrad, yolo_adam_step): how a weight-gradient
// launch is split and every argument check in front of a launch.  No HIP here: train_host.cpp compiles as plain C++, so that
// train_host_check.cpp (a program with its own main) runs it under AddressSanitizer + UndefinedBehaviorSanitizer on a CPU (`make san-train`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "yolo_hip.h"

namespace yolo {

// head_wgrad_kernel (train.hip): a workgroup owns kWgradTileCout x kWgradTileCin elements of dW and walks its chunk of positions
// kWgradTilePos at a time
constexpr int kWgradTileCout = 64, kWgradTileCin = 128, kWgradTilePos = 16;
constexpr int kWgradTargetGrid = 512;       // workgroups a launch aims at: two per CU
constexpr int kWgradMinChunk = 32;          // positions a chunk holds at least

// 0 or a YOLO_ERR_* code with the message in err
int wgrad_plan(long long P, int cin, int cout, int x_dtype, struct yolo_wgrad_plan *out, std::string &err);
int wgrad_check(const void *x_dev, int x_dtype, int ld, int coff, long long image_stride, int positions_per_image, int batch, int cin,
                const void *g_dev, int cout, const void *dw_dev, const void *db_dev, const void *scratch_dev, size_t scratch_bytes,
                struct yolo_wgrad_plan *plan, std::string &err);
int adam_check(const void *w, const void *b, const void *m_w, const void *v_w, const void *m_b, const void *v_b, const void *dw, const void *db,
               long long n_w, long long n_b, float lr_t, float beta1, float beta2, float eps, std::string &err);

}  // namespace yolo

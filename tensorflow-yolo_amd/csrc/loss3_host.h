// Host side of the YOLOv3 loss entries (include/yolo_hip.h: yolo_v3_loss_rows, yolo_v3_loss, yolo_v3_loss_grad, yolo_net_loss_v3*): the row
// offsets of the scales, the number of partial records an image is summed through, and every argument check in front of a launch.  No
// HIP here: loss3_host.cpp compiles as plain C++, so that loss3_host_check.cpp (a program with its own main) runs it under
// AddressSanitizer + UndefinedBehaviorSanitizer on a CPU (`make san-loss3`).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "yolo_hip.h"

namespace yolo {

// rows of an image one workgroup of loss3_terms_kernel sums into one yolo_loss_image record.  Part of the DEFINITION of the sums (it fixes
// their order), so a constant: never a function of the device
constexpr int kLoss3RowsPerPart = 1024;

struct Loss3Scale {
    int row0, h, w, na;                                     // first row of the scale inside an image
    double aw[YOLO_MAX_ANCHORS], ah[YOLO_MAX_ANCHORS];      // grid units, float64: the assignment
    float awf[YOLO_MAX_ANCHORS], ahf[YOLO_MAX_ANCHORS];     // ... rounded to float32: the decode of the ignore test
};
struct Loss3Geometry {
    int n_scales, n_classes, rows, parts;                   // rows = R; parts = ceil(R / kLoss3RowsPerPart)
    Loss3Scale sc[YOLO_MAX_SCALES];
};

// 0 or a YOLO_ERR_* code with the message in err (without the entry's name: the caller puts it in front)
int loss3_geometry(const yolo_head_desc *head, Loss3Geometry *out, std::string &err);
// every check of yolo_v3_loss (grad_required = false) / yolo_v3_loss_grad (true) that needs no device; the pointers are never followed
int loss3_check(const yolo_head_desc *head, const void *logits_dev, int batch, const void *gt_dev, const void *gt_counts_dev, int max_gt,
                double ignore_thresh, const void *parts_dev, const void *images_dev, const void *assign_dev, const void *result_dev,
                bool grad_required, const void *grad_dev, Loss3Geometry *geo, std::string &err);

}  // namespace yolo

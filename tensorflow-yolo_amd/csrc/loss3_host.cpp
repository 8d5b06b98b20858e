// Host side of the YOLOv3 loss entries: see loss3_host.h.  Plain C++, no HIP.
#include "loss3_host.h"

namespace yolo {

int loss3_geometry(const yolo_head_desc *head, Loss3Geometry *out, std::string &err) {
    if (!head || !out) { err = "null argument"; return YOLO_ERR_ARG; }
    if (head->version != 3) { err = "the head must be version 3"; return YOLO_ERR_ARG; }
    if (head->n_scales < 1 || head->n_scales > YOLO_MAX_SCALES) { err = "n_scales must be 1.." + std::to_string(YOLO_MAX_SCALES); return YOLO_ERR_ARG; }
    if (head->n_classes < 1) { err = "n_classes must be at least 1"; return YOLO_ERR_ARG; }
    Loss3Geometry g = Loss3Geometry();
    g.n_scales = head->n_scales;
    g.n_classes = head->n_classes;
    long long rows = 0;
    for (int s = 0; s < head->n_scales; ++s) {
        const int h = head->h[s], w = head->w[s], na = head->n_anchors[s];
        if (h < 1 || w < 1 || na < 1 || na > YOLO_MAX_ANCHORS) {
            err = "scale " + std::to_string(s) + ": h, w and n_anchors must be at least 1 (n_anchors at most " + std::to_string(YOLO_MAX_ANCHORS) + ")";
            return YOLO_ERR_ARG;
        }
        Loss3Scale &sc = g.sc[s];
        sc.row0 = (int)rows; sc.h = h; sc.w = w; sc.na = na;
        for (int a = 0; a < na; ++a) {
            sc.aw[a] = head->anchors[s][2 * a]; sc.ah[a] = head->anchors[s][2 * a + 1];
            sc.awf[a] = (float)sc.aw[a]; sc.ahf[a] = (float)sc.ah[a];
        }
        // the kernels index the rows and the elements of ONE image with 32 bits (images and everything across them: size_t)
        const long long cells = (long long)h * w;           // (below 2^62)
        if (cells <= 0x7fffffffLL) rows += cells * na;      // (below 2^34 + 2^31)
        if (cells > 0x7fffffffLL || rows * (5LL + head->n_classes) > 0x7fffffffLL) { err = "rows * (5 + n_classes) of one image must fit 31 bits"; return YOLO_ERR_ARG; }
    }
    g.rows = (int)rows;
    g.parts = (int)((rows + kLoss3RowsPerPart - 1) / kLoss3RowsPerPart);
    *out = g;
    return YOLO_OK;
}

int loss3_check(const yolo_head_desc *head, const void *logits_dev, int batch, const void *gt_dev, const void *gt_counts_dev, int max_gt,
                double ignore_thresh, const void *parts_dev, const void *images_dev, const void *assign_dev, const void *result_dev,
                bool grad_required, const void *grad_dev, Loss3Geometry *geo, std::string &err) {
    if (!head || !logits_dev || !gt_dev || !gt_counts_dev || !parts_dev || !images_dev || !assign_dev || !result_dev || !geo ||
        (grad_required && !grad_dev)) {
        err = "null argument";
        return YOLO_ERR_ARG;
    }
    if (batch < 1) { err = "batch must be at least 1"; return YOLO_ERR_ARG; }
    if (max_gt < 1 || max_gt > YOLO_EVAL_MAX_GT) { err = "max_gt must be 1.." + std::to_string(YOLO_EVAL_MAX_GT); return YOLO_ERR_ARG; }
    if (!(ignore_thresh > 0. && ignore_thresh <= 1.)) { err = "ignore_thresh must be in (0, 1]"; return YOLO_ERR_ARG; }      // (a NaN too)
    const int rc = loss3_geometry(head, geo, err);
    if (rc) return rc;
    if (grad_required && grad_dev == logits_dev) { err = "grad_dev must not be logits_dev (the gradient is not computed in place)"; return YOLO_ERR_ARG; }
    return YOLO_OK;
}

}  // namespace yolo

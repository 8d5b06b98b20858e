// Host side of the sparse data gradient of one YOLOv3 head conv: see train3_tail_host.h.  Plain C++, no HIP.
#include "train3_tail_host.h"

#include "train_tail_host.h"

namespace yolo {

int dgrad3_plan(const yolo_head_desc *head, int scale, int cin, int batch, struct yolo_v3_dgrad_plan *out, Dgrad3Params *p, std::string &err) {
    if (!head || !out) { err = "null argument"; return YOLO_ERR_ARG; }
    Loss3Geometry lg;
    const int rc = loss3_geometry(head, &lg, err);      // version 3, the scales' sizes, 31-bit rows of an image
    if (rc) return rc;
    if (scale < 0 || scale >= lg.n_scales) { err = "scale must be 0.." + std::to_string(lg.n_scales - 1); return YOLO_ERR_ARG; }
    if (batch < 1) { err = "batch must be at least 1"; return YOLO_ERR_ARG; }
    if (cin < 8 || cin % 8) { err = "cin must be a positive multiple of 8"; return YOLO_ERR_ARG; }
    const Loss3Scale &ls = lg.sc[scale];
    // (2^30: a position index, and a workgroup's share rounded up, stay inside 31 bits in the kernel)
    const long long ppi = (long long)ls.h * ls.w, P = ppi * batch;
    if (P > (1LL << 30)) { err = "the number of positions must be 1 .. 2^30"; return YOLO_ERR_ARG; }
    *out = yolo_v3_dgrad_plan();
    out->threads = kDgrad3Threads;
    out->channels_per_thread = kDgrad3Lane;
    out->tile_cin = cin < kDgrad3TileCin ? cin : kDgrad3TileCin;
    out->tiles_cin = (cin + kDgrad3TileCin - 1) / kDgrad3TileCin;
    out->threads_per_position = out->tile_cin / kDgrad3Lane;
    out->positions_per_round = kDgrad3Threads / out->threads_per_position;
    const long long all_rounds = (P + out->positions_per_round - 1) / out->positions_per_round;
    const long long rounds = (all_rounds + kDgrad3TargetGroups - 1) / kDgrad3TargetGroups;      // rounds that keep the grid at its target
    const long long groups = (all_rounds + rounds - 1) / rounds;
    if (groups * out->tiles_cin > 0x7fffffffLL) { err = "too many workgroups"; return YOLO_ERR_ARG; }
    out->rounds = (int32_t)rounds;
    out->positions_per_workgroup = (int32_t)(rounds * out->positions_per_round);
    out->workgroups = (int32_t)groups;
    out->loops = rounds > 1;
    out->positions = (int32_t)P;
    out->lds_bytes = ls.na * out->tile_cin * 4;
    if (p) {
        *p = Dgrad3Params();
        p->cin = cin; p->na = ls.na; p->stride = 5 + lg.n_classes; p->rows = lg.rows; p->row0 = ls.row0; p->ppi = (int)ppi; p->P = (int)P;
        p->tile_cin = out->tile_cin; p->tiles_cin = out->tiles_cin; p->tpp = out->threads_per_position; p->ppr = out->positions_per_round;
        p->ppw = out->positions_per_workgroup; p->groups = out->workgroups;
    }
    return YOLO_OK;
}

int dgrad3_check(const yolo_head_desc *head, int scale, const void *g_dev, const void *assign_dev, int max_gt, int batch, const void *w_dev,
                 int cin, const void *y_dev, int y_dtype, int ld, int coff, long long image_stride, float slope, void *d_dev,
                 struct yolo_v3_dgrad_plan *plan, Dgrad3Params *p, std::string &err) {
    if (!head || !g_dev || !assign_dev || !w_dev || !d_dev || !plan || !p) { err = "null argument"; return YOLO_ERR_ARG; }
    if (head->version != 3) { err = "the head must be version 3"; return YOLO_ERR_ARG; }
    if (max_gt < 1 || max_gt > YOLO_EVAL_MAX_GT) { err = "max_gt must be 1.." + std::to_string(YOLO_EVAL_MAX_GT); return YOLO_ERR_ARG; }
    int rc = dgrad3_plan(head, scale, cin, batch, plan, p, err);
    if (rc) return rc;
    if ((uintptr_t)g_dev % 4 || (uintptr_t)assign_dev % 4) { err = "a pointer is not aligned to its element type"; return YOLO_ERR_ARG; }
    if ((uintptr_t)w_dev % 16 || (uintptr_t)d_dev % 16) { err = "w_dev and d_dev must be 16-byte aligned"; return YOLO_ERR_ARG; }
    if (y_dev) {
        rc = view_check(y_dev, y_dtype, ld, coff, image_stride, p->ppi, cin, err);
        if (rc) return rc;
        const int epc = y_dtype == YOLO_DTYPE_F16 ? 8 : 4;      // elements of a 16-byte chunk
        p->y = y_dev; p->ld = ld; p->coff = coff; p->img_stride = image_stride; p->f16 = y_dtype == YOLO_DTYPE_F16;
        p->wide = (uintptr_t)y_dev % 16 == 0 && ld % epc == 0 && coff % epc == 0 && image_stride % epc == 0;
    }
    p->g = static_cast<const float *>(g_dev); p->assign = static_cast<const int *>(assign_dev); p->w = static_cast<const float *>(w_dev);
    p->d = static_cast<float *>(d_dev);
    p->max_gt = max_gt;
    p->slope = slope;       // any value, NaN included, is a factor like another
    return YOLO_OK;
}

}  // namespace yolo

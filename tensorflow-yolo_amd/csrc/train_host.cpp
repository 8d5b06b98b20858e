// Host side of the head-training entries: the split of a weight-gradient launch and the argument checks (train_host.h).  Plain C++.
#include "train_host.h"

namespace yolo {

int wgrad_plan(long long P, int cin, int cout, int x_dtype, struct yolo_wgrad_plan *out, std::string &err) {
    if (!out) { err = "null argument"; return YOLO_ERR_ARG; }
    if (x_dtype != YOLO_DTYPE_F16 && x_dtype != YOLO_DTYPE_F32) { err = "x_dtype must be YOLO_DTYPE_F16 or YOLO_DTYPE_F32"; return YOLO_ERR_ARG; }
    // (2^30: a chunk rounded up to whole stages, and a position index one stage past the end, stay inside 31 bits in the kernel)
    if (P < 1 || P > (1LL << 30)) { err = "the number of positions must be 1 .. 2^30"; return YOLO_ERR_ARG; }
    if (cin < 8 || cin % 8) { err = "cin must be a positive multiple of 8"; return YOLO_ERR_ARG; }
    if (cout < 1) { err = "cout must be at least 1"; return YOLO_ERR_ARG; }
    if ((long long)cout * ((long long)cin + 1) > 0x7fffffffLL) { err = "cout * (cin + 1) must fit 31 bits"; return YOLO_ERR_ARG; }
    out->tile_cout = kWgradTileCout;
    out->tile_cin = kWgradTileCin;
    out->tile_positions = kWgradTilePos;
    out->tiles_cout = (cout + kWgradTileCout - 1) / kWgradTileCout;
    out->tiles_cin = (cin + kWgradTileCin - 1) / kWgradTileCin;
    const long long tiles = (long long)out->tiles_cout * out->tiles_cin;
    const long long want = tiles >= kWgradTargetGrid ? 1 : (kWgradTargetGrid + tiles - 1) / tiles;     // chunks that fill the grid
    long long ppc = (P + want - 1) / want;
    ppc = (ppc + kWgradTilePos - 1) / kWgradTilePos * kWgradTilePos;
    if (ppc < kWgradMinChunk) ppc = kWgradMinChunk;
    out->positions_per_chunk = (int32_t)ppc;
    out->n_chunks = (int32_t)((P + ppc - 1) / ppc);
    out->pad_ = 0;
    out->scratch_bytes = (uint64_t)out->n_chunks * (uint64_t)cout * (uint64_t)(cin + 1) * 4u;
    return YOLO_OK;
}

int wgrad_check(const void *x_dev, int x_dtype, int ld, int coff, long long image_stride, int positions_per_image, int batch, int cin,
                const void *g_dev, int cout, const void *dw_dev, const void *db_dev, const void *scratch_dev, size_t scratch_bytes,
                struct yolo_wgrad_plan *plan, std::string &err) {
    if (!x_dev || !g_dev || !dw_dev || !db_dev || !scratch_dev || !plan) { err = "null argument"; return YOLO_ERR_ARG; }
    if (positions_per_image < 1 || batch < 1) { err = "positions_per_image and batch must be at least 1"; return YOLO_ERR_ARG; }
    const int rc = wgrad_plan((long long)positions_per_image * batch, cin, cout, x_dtype, plan, err);
    if (rc) return rc;
    if (coff < 0 || ld < 1 || (long long)coff + cin > ld) { err = "the channels coff .. coff + cin must lie inside the pixel stride ld"; return YOLO_ERR_ARG; }
    if (image_stride < (long long)(positions_per_image - 1) * ld + coff + cin) { err = "image_stride is smaller than one image of the view"; return YOLO_ERR_ARG; }
    if ((uintptr_t)x_dev % (x_dtype == YOLO_DTYPE_F16 ? 2 : 4) || (uintptr_t)g_dev % 4 || (uintptr_t)dw_dev % 4 || (uintptr_t)db_dev % 4 || (uintptr_t)scratch_dev % 4) {
        err = "a pointer is not aligned to its element type";
        return YOLO_ERR_ARG;
    }
    if (scratch_bytes < plan->scratch_bytes) {
        err = "scratch too small: " + std::to_string(scratch_bytes) + " bytes, yolo_wgrad_plan asks for " + std::to_string(plan->scratch_bytes);
        return YOLO_ERR_ARG;
    }
    return YOLO_OK;
}

int adam_check(const void *w, const void *b, const void *m_w, const void *v_w, const void *m_b, const void *v_b, const void *dw, const void *db,
               long long n_w, long long n_b, float lr_t, float beta1, float beta2, float eps, std::string &err) {
    if (n_w < 1 || n_b < 0 || n_w > 0x7fffffffLL || n_b > 0x7fffffffLL) { err = "n_w must be 1 .. 2^31 - 1 and n_b 0 .. 2^31 - 1"; return YOLO_ERR_ARG; }
    if (!w || !m_w || !v_w || !dw || (n_b && (!b || !m_b || !v_b || !db))) { err = "null argument"; return YOLO_ERR_ARG; }
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) { err = "beta1 and beta2 must be in [0, 1)"; return YOLO_ERR_ARG; }
    if (!(eps >= 0.f) || lr_t != lr_t) { err = "eps must not be negative and lr_t not NaN"; return YOLO_ERR_ARG; }
    return YOLO_OK;
}

}  // namespace yolo

// Host side of yolo_conv1x1_dgrad, yolo_conv3x3_wgrad and yolo_conv3x3_wgrad_f16: the split of a 3 x 3 weight-gradient launch, its scratch
// layout and the argument checks (train_tail_host.h).  Plain C++.
#include "train_tail_host.h"

namespace yolo {

int wgrad3x3_plan(int h, int w, int batch, int cin, int cout, int x_dtype, struct yolo_conv3x3_wgrad_plan *out, std::string &err) {
    if (!out) { err = "null argument"; return YOLO_ERR_ARG; }
    if (x_dtype != YOLO_DTYPE_F16 && x_dtype != YOLO_DTYPE_F32) { err = "x_dtype must be YOLO_DTYPE_F16 or YOLO_DTYPE_F32"; return YOLO_ERR_ARG; }
    if (h < 1 || w < 1 || batch < 1) { err = "h, w and batch must be at least 1"; return YOLO_ERR_ARG; }
    if (w > kTailMaxW) { err = "w must be at most " + std::to_string(kTailMaxW) + ": the halo of a wider map does not fit LDS"; return YOLO_ERR_ARG; }
    // (2^30: a chunk rounded up to whole stages, and a position index one stage and one halo past the end, stay inside 31 bits in the kernel)
    const long long hw = (long long)h * w, P = hw > (1LL << 30) ? hw : hw * batch;      // (w <= 80: neither product overflows)
    if (P > (1LL << 30)) { err = "the number of positions must be 1 .. 2^30"; return YOLO_ERR_ARG; }
    if (cin < 8 || cin % 8) { err = "cin must be a positive multiple of 8"; return YOLO_ERR_ARG; }
    if (cout < 1) { err = "cout must be at least 1"; return YOLO_ERR_ARG; }
    if ((long long)cout * (9LL * cin + 1) > 0x7fffffffLL) { err = "cout * (9 cin + 1) must fit 31 bits"; return YOLO_ERR_ARG; }
    out->tile_cout = kTailTileCout;
    out->tile_cin = kTailTileCin;
    out->tile_positions = kTailTilePos;
    out->tiles_cout = (cout + kTailTileCout - 1) / kTailTileCout;
    out->tiles_cin = (cin + kTailTileCin - 1) / kTailTileCin;
    const long long tiles = (long long)out->tiles_cout * out->tiles_cin;
    const long long want = tiles >= kTailTargetGrid ? 1 : (kTailTargetGrid + tiles - 1) / tiles;       // chunks that fill the grid
    long long ppc = (P + want - 1) / want;
    ppc = (ppc + kTailTilePos - 1) / kTailTilePos * kTailTilePos;
    if (ppc < kTailMinChunk) ppc = kTailMinChunk;
    out->positions_per_chunk = (int32_t)ppc;
    out->n_chunks = (int32_t)((P + ppc - 1) / ppc);
    out->halo_rows = kTailTilePos + 2 * w + 2;
    out->scratch_bytes = (uint64_t)out->n_chunks * (uint64_t)cout * (uint64_t)(9 * (long long)cin + 1) * 4u;
    return YOLO_OK;
}

// the checks of a strided NHWC view that yolo_conv1x1_wgrad makes
int view_check(const void *dev, int dtype, int ld, int coff, long long image_stride, long long positions_per_image, int cin, std::string &err) {
    if (dtype != YOLO_DTYPE_F16 && dtype != YOLO_DTYPE_F32) { err = "the view's dtype must be YOLO_DTYPE_F16 or YOLO_DTYPE_F32"; return YOLO_ERR_ARG; }
    if (coff < 0 || ld < 1 || (long long)coff + cin > ld) { err = "the channels coff .. coff + cin must lie inside the pixel stride ld"; return YOLO_ERR_ARG; }
    if (image_stride < (positions_per_image - 1) * ld + coff + cin) { err = "image_stride is smaller than one image of the view"; return YOLO_ERR_ARG; }
    if ((uintptr_t)dev % (dtype == YOLO_DTYPE_F16 ? 2 : 4)) { err = "a pointer is not aligned to its element type"; return YOLO_ERR_ARG; }
    return YOLO_OK;
}

int wgrad3x3_check(const void *x_dev, int x_dtype, int ld, int coff, long long image_stride, int h, int w, int batch, int cin,
                   const void *d_dev, int cout, const void *scale_dev, const void *dw_dev, const void *db_dev, const void *scratch_dev,
                   size_t scratch_bytes, struct yolo_conv3x3_wgrad_plan *plan, std::string &err) {
    if (!x_dev || !d_dev || !dw_dev || !db_dev || !scratch_dev || !plan) { err = "null argument"; return YOLO_ERR_ARG; }
    int rc = wgrad3x3_plan(h, w, batch, cin, cout, x_dtype, plan, err);
    if (rc) return rc;
    rc = view_check(x_dev, x_dtype, ld, coff, image_stride, (long long)h * w, cin, err);
    if (rc) return rc;
    if ((uintptr_t)d_dev % 4 || (uintptr_t)scale_dev % 4 || (uintptr_t)dw_dev % 4 || (uintptr_t)db_dev % 4 || (uintptr_t)scratch_dev % 4) {
        err = "a pointer is not aligned to its element type";
        return YOLO_ERR_ARG;
    }
    if (scratch_bytes < plan->scratch_bytes) {
        err = "scratch too small: " + std::to_string(scratch_bytes) + " bytes, yolo_conv3x3_wgrad_plan asks for " + std::to_string(plan->scratch_bytes);
        return YOLO_ERR_ARG;
    }
    return YOLO_OK;
}

// The split of wgrad3x3_plan with the fp16 kernel's stage, and behind the slabs the m / k record the call initialises itself and the partial
// sums of db.  D is narrowed while the main kernel stages it into LDS: there is no D16 buffer.
int wgrad3x3_f16_plan(int h, int w, int batch, int cin, int cout, struct yolo_conv3x3_wgrad_f16_plan *out, std::string &err) {
    if (!out) { err = "null argument"; return YOLO_ERR_ARG; }
    if (h < 1 || w < 1 || batch < 1) { err = "h, w and batch must be at least 1"; return YOLO_ERR_ARG; }
    if (w > kTailF16MaxW) { err = "w must be at most " + std::to_string(kTailF16MaxW) + ": the halo of a wider map does not fit LDS"; return YOLO_ERR_ARG; }
    // (2^30: a chunk rounded up to whole stages, and a position index one stage and one halo past the end, stay inside 31 bits in the kernel)
    const long long hw = (long long)h * w, P = hw > (1LL << 30) ? hw : hw * batch;      // (w <= 96: neither product overflows)
    if (P > (1LL << 30)) { err = "the number of positions must be 1 .. 2^30"; return YOLO_ERR_ARG; }
    if (cin < 8 || cin % 8) { err = "cin must be a positive multiple of 8"; return YOLO_ERR_ARG; }
    if (cout < 1) { err = "cout must be at least 1"; return YOLO_ERR_ARG; }
    if ((long long)cout * (9LL * cin + 1) > 0x7fffffffLL) { err = "cout * (9 cin + 1) must fit 31 bits"; return YOLO_ERR_ARG; }
    out->tile_cout = kTailTileCout;
    out->tile_cin = kTailTileCin;
    out->tile_positions = kTailF16TilePos;
    out->tiles_cout = (cout + kTailTileCout - 1) / kTailTileCout;
    out->tiles_cin = (cin + kTailTileCin - 1) / kTailTileCin;
    const long long tiles = (long long)out->tiles_cout * out->tiles_cin;
    const long long want = tiles >= kTailTargetGrid ? 1 : (kTailTargetGrid + tiles - 1) / tiles;       // chunks that fill the grid
    long long ppc = (P + want - 1) / want;
    ppc = (ppc + kTailF16TilePos - 1) / kTailF16TilePos * kTailF16TilePos;
    if (ppc < kTailF16MinChunk) ppc = kTailF16MinChunk;
    out->positions_per_chunk = (int32_t)ppc;
    out->n_chunks = (int32_t)((P + ppc - 1) / ppc);
    out->halo_rows = kTailF16TilePos + 2 * w + 2;
    const uint64_t slabs = (uint64_t)out->n_chunks * (uint64_t)cout * (uint64_t)(9 * (long long)cin + 1) * 4u;
    out->record_offset = (slabs + 255u) / 256u * 256u;
    // db: up to kTailF16DbGroups groups of positions, each a multiple of the 16 row groups of the kernel that adds them
    long long dbp = (P + kTailF16DbGroups - 1) / kTailF16DbGroups;
    dbp = (dbp + 15) / 16 * 16;
    out->db_positions = (int32_t)dbp;
    out->db_groups = (int32_t)((P + dbp - 1) / dbp);
    const uint64_t partials = ((uint64_t)out->db_groups * (uint64_t)cout * 4u + 255u) / 256u * 256u;
    out->scratch_bytes = out->record_offset + (uint64_t)kTailF16RecordBytes + partials;
    return YOLO_OK;
}

int wgrad3x3_f16_check(const void *x_dev, int x_dtype, int ld, int coff, long long image_stride, int h, int w, int batch, int cin,
                       const void *d_dev, int cout, const void *scale_dev, const void *dw_dev, const void *db_dev, const void *scratch_dev,
                       size_t scratch_bytes, struct yolo_conv3x3_wgrad_f16_plan *plan, std::string &err) {
    if (!x_dev || !d_dev || !dw_dev || !db_dev || !scratch_dev || !plan) { err = "null argument"; return YOLO_ERR_ARG; }
    if (x_dtype != YOLO_DTYPE_F16) { err = "X3 must be YOLO_DTYPE_F16: a float32 view is yolo_conv3x3_wgrad's"; return YOLO_ERR_ARG; }
    int rc = wgrad3x3_f16_plan(h, w, batch, cin, cout, plan, err);
    if (rc) return rc;
    rc = view_check(x_dev, x_dtype, ld, coff, image_stride, (long long)h * w, cin, err);
    if (rc) return rc;
    if ((uintptr_t)d_dev % 4 || (uintptr_t)scale_dev % 4 || (uintptr_t)dw_dev % 4 || (uintptr_t)db_dev % 4 || (uintptr_t)scratch_dev % 4) {
        err = "a pointer is not aligned to its element type";
        return YOLO_ERR_ARG;
    }
    if (scratch_bytes < plan->scratch_bytes) {
        err = "scratch too small: " + std::to_string(scratch_bytes) + " bytes, yolo_conv3x3_wgrad_f16_plan asks for " + std::to_string(plan->scratch_bytes);
        return YOLO_ERR_ARG;
    }
    return YOLO_OK;
}

int dgrad_check(const void *g_dev, int cout, const void *w_dev, int cin, const void *y_dev, int y_dtype, int ld, int coff,
                long long image_stride, int positions_per_image, int batch, float slope, const void *d_dev, long long *tiles, std::string &err) {
    (void)slope;        // any value, NaN included, is a factor like another
    if (!g_dev || !w_dev || !d_dev || !tiles) { err = "null argument"; return YOLO_ERR_ARG; }
    if (positions_per_image < 1 || batch < 1) { err = "positions_per_image and batch must be at least 1"; return YOLO_ERR_ARG; }
    const long long P = (long long)positions_per_image * batch;
    if (P > (1LL << 30)) { err = "the number of positions must be 1 .. 2^30"; return YOLO_ERR_ARG; }
    if (cin < 8 || cin % 8) { err = "cin must be a positive multiple of 8"; return YOLO_ERR_ARG; }
    if (cout < 1) { err = "cout must be at least 1"; return YOLO_ERR_ARG; }
    if ((long long)cout * cin > 0x7fffffffLL) { err = "cout * cin must fit 31 bits"; return YOLO_ERR_ARG; }
    if ((uintptr_t)g_dev % 4) { err = "a pointer is not aligned to its element type"; return YOLO_ERR_ARG; }
    if ((uintptr_t)w_dev % 16 || (uintptr_t)d_dev % 16) { err = "w_dev and d_dev must be 16-byte aligned"; return YOLO_ERR_ARG; }
    if (y_dev) {
        const int rc = view_check(y_dev, y_dtype, ld, coff, image_stride, positions_per_image, cin, err);
        if (rc) return rc;
    }
    const long long t = ((P + kDgradTilePos - 1) / kDgradTilePos) * ((cin + kDgradTileCin - 1) / kDgradTileCin);
    if (t > 0x7fffffffLL) { err = "positions * cin is too large for one launch"; return YOLO_ERR_ARG; }
    *tiles = t;
    return YOLO_OK;
}

}  // namespace yolo

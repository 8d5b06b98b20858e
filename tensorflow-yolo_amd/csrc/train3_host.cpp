// Host side of the YOLOv3 head weight gradient: see train3_host.h.  Plain C++, no HIP.
#include "train3_host.h"

namespace yolo {

static uint64_t up256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }

int wgrad3_plan(const yolo_head_desc *head, const int32_t *cin, int batch, int x_dtype, struct yolo_v3_wgrad_plan *out, Wgrad3Geometry *geo,
                std::string &err) {
    if (!head || !cin || !out || !geo) { err = "null argument"; return YOLO_ERR_ARG; }
    if (x_dtype != YOLO_DTYPE_F16 && x_dtype != YOLO_DTYPE_F32) { err = "x_dtype must be YOLO_DTYPE_F16 or YOLO_DTYPE_F32"; return YOLO_ERR_ARG; }
    if (batch < 1) { err = "batch must be at least 1"; return YOLO_ERR_ARG; }
    Loss3Geometry lg;
    const int rc = loss3_geometry(head, &lg, err);      // version 3, the scales' sizes, 31-bit rows of an image
    if (rc) return rc;
    *out = yolo_v3_wgrad_plan();
    *geo = Wgrad3Geometry();
    geo->n_scales = out->n_scales = lg.n_scales;
    geo->stride = 5 + lg.n_classes;
    geo->rows = lg.rows;
    out->threads = kWgrad3Threads;
    out->channels_per_thread = kWgrad3Lane;
    out->min_chunk = kWgrad3MinChunk;
    out->win_tile_cin = kWgrad3WinTile;
    out->win_tile_rows = kWgrad3WinRows;
    out->reduce_tile_chunks = kWgrad3RedChunks;
    uint64_t off = 0;
    long long obj_blocks = 0, red_blocks = 0, win_blocks = 0;
    for (int s = 0; s < lg.n_scales; ++s) {
        const std::string at = "scale " + std::to_string(s) + ": ";
        const int c = cin[s], na = lg.sc[s].na;
        if (c < 8 || c % 8) { err = at + "cin must be a positive multiple of 8"; return YOLO_ERR_ARG; }
        const long long cout = (long long)na * geo->stride, ppi = (long long)lg.sc[s].h * lg.sc[s].w, P = ppi * batch;
        // (2^30: a position index, and a chunk rounded up, stay inside 31 bits in the kernels)
        if (P > (1LL << 30)) { err = at + "the number of positions must be 1 .. 2^30"; return YOLO_ERR_ARG; }
        if (cout * ((long long)c + 1) > 0x7fffffffLL) { err = at + "cout * (cin + 1) must fit 31 bits"; return YOLO_ERR_ARG; }
        Wgrad3Scale &sc = geo->sc[s];
        sc.cin = c; sc.na = na; sc.row0 = lg.sc[s].row0; sc.ppi = (int)ppi; sc.P = (int)P;
        sc.tpc = c / kWgrad3Lane;
        long long want = kWgrad3TargetThreads / sc.tpc;                 // chunks that fill the grid
        if (want < 1) want = 1;
        long long ppc = (P + want - 1) / want;
        if (ppc < kWgrad3MinChunk) ppc = kWgrad3MinChunk;
        sc.ppc = (int)ppc;
        sc.n_chunks = (int)((P + ppc - 1) / ppc);
        sc.win_tiles = (c + kWgrad3WinTile - 1) / kWgrad3WinTile;
        sc.win_ktiles = (geo->stride + kWgrad3WinRows - 1) / kWgrad3WinRows;
        const long long ob = ((long long)sc.n_chunks * sc.tpc + kWgrad3Threads - 1) / kWgrad3Threads;
        const long long rb = ((long long)na * (c + 1) + kWgrad3RedElems - 1) / kWgrad3RedElems;
        const long long wb = (long long)na * sc.win_ktiles * sc.win_tiles;
        sc.obj_blk0 = (int)obj_blocks; sc.red_blk0 = (int)red_blocks; sc.win_blk0 = (int)win_blocks;
        obj_blocks += ob; red_blocks += rb; win_blocks += wb;
        if (obj_blocks > 0x7fffffffLL || win_blocks > 0x7fffffffLL) { err = at + "too many workgroups"; return YOLO_ERR_ARG; }
        out->positions[s] = (int32_t)P;
        out->positions_per_chunk[s] = sc.ppc;
        out->n_chunks[s] = sc.n_chunks;
        out->threads_per_chunk[s] = sc.tpc;
        out->obj_workgroups[s] = (int32_t)ob;
        out->win_workgroups[s] = (int32_t)wb;
        out->slab_offset[s] = off;
        out->slab_bytes[s] = (uint64_t)sc.n_chunks * (uint64_t)((long long)na * c + 8) * 4u;
        off = up256(off + out->slab_bytes[s]);
    }
    geo->obj_blocks = (int)obj_blocks; geo->red_blocks = (int)red_blocks; geo->win_blocks = (int)win_blocks;
    out->slot_offset = off;
    out->slot_bytes = (uint64_t)batch * YOLO_EVAL_MAX_GT * 4u;          // slot[batch][max_gt] for the largest max_gt
    out->scratch_bytes = up256(off + out->slot_bytes);
    return YOLO_OK;
}

int wgrad3_check(const yolo_head_desc *head, const struct yolo_v3_wgrad_view *views, int batch, const void *g_dev, const void *assign_dev,
                 int max_gt, float *const *dw_dev, float *const *db_dev, void *scratch_dev, size_t scratch_bytes,
                 struct yolo_v3_wgrad_plan *plan, Wgrad3Geometry *geo, std::string &err) {
    if (!head || !views || !g_dev || !assign_dev || !dw_dev || !db_dev || !scratch_dev || !plan || !geo) { err = "null argument"; return YOLO_ERR_ARG; }
    if (head->version != 3) { err = "the head must be version 3"; return YOLO_ERR_ARG; }
    if (head->n_scales < 1 || head->n_scales > YOLO_MAX_SCALES) { err = "n_scales must be 1.." + std::to_string(YOLO_MAX_SCALES); return YOLO_ERR_ARG; }
    if (max_gt < 1 || max_gt > YOLO_EVAL_MAX_GT) { err = "max_gt must be 1.." + std::to_string(YOLO_EVAL_MAX_GT); return YOLO_ERR_ARG; }
    int32_t cin[YOLO_MAX_SCALES] = {0, 0, 0, 0};
    for (int s = 0; s < head->n_scales; ++s) {
        const std::string at = "scale " + std::to_string(s) + ": ";
        if (!views[s].x_dev || !dw_dev[s] || !db_dev[s]) { err = at + "null argument"; return YOLO_ERR_ARG; }
        if (views[s].dtype != YOLO_DTYPE_F16 && views[s].dtype != YOLO_DTYPE_F32) { err = at + "dtype must be YOLO_DTYPE_F16 or YOLO_DTYPE_F32"; return YOLO_ERR_ARG; }
        cin[s] = views[s].cin;
    }
    const int rc = wgrad3_plan(head, cin, batch, YOLO_DTYPE_F32, plan, geo, err);
    if (rc) return rc;
    for (int s = 0; s < geo->n_scales; ++s) {
        const std::string at = "scale " + std::to_string(s) + ": ";
        const yolo_v3_wgrad_view &v = views[s];
        Wgrad3Scale &sc = geo->sc[s];
        if (v.coff < 0 || v.ld < 1 || (long long)v.coff + v.cin > v.ld) { err = at + "the channels coff .. coff + cin must lie inside the pixel stride ld"; return YOLO_ERR_ARG; }
        if (v.image_stride < (long long)(sc.ppi - 1) * v.ld + v.coff + v.cin) { err = at + "image_stride is smaller than one image of the view"; return YOLO_ERR_ARG; }
        const int f16 = v.dtype == YOLO_DTYPE_F16, esz = f16 ? 2 : 4, epc = 16 / esz;
        if ((uintptr_t)v.x_dev % esz || (uintptr_t)dw_dev[s] % 4 || (uintptr_t)db_dev[s] % 4) { err = at + "a pointer is not aligned to its element type"; return YOLO_ERR_ARG; }
        sc.x = v.x_dev; sc.ld = v.ld; sc.coff = v.coff; sc.img_stride = v.image_stride; sc.f16 = f16;
        sc.wide = (uintptr_t)v.x_dev % 16 == 0 && v.ld % epc == 0 && v.coff % epc == 0 && v.image_stride % epc == 0;
        sc.dw = dw_dev[s]; sc.db = db_dev[s];
        sc.slab = reinterpret_cast<float *>(static_cast<unsigned char *>(scratch_dev) + plan->slab_offset[s]);
    }
    if ((uintptr_t)g_dev % 4 || (uintptr_t)assign_dev % 4) { err = "a pointer is not aligned to its element type"; return YOLO_ERR_ARG; }
    if ((uintptr_t)scratch_dev % 16) { err = "scratch_dev must be 16-byte aligned"; return YOLO_ERR_ARG; }
    if (scratch_bytes < plan->scratch_bytes) {
        err = "scratch too small: " + std::to_string(scratch_bytes) + " bytes, yolo_v3_head_wgrad_plan asks for " + std::to_string(plan->scratch_bytes);
        return YOLO_ERR_ARG;
    }
    return YOLO_OK;
}

}  // namespace yolo

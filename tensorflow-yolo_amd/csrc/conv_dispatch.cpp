// What one (non-stem) conv launch runs, decided once: resolve_conv builds the ConvLaunch record that the forward pass launches from,
// the workspace sizing takes its partial-sum slab from, branch_tails_ok scans and yolo_net_kernel_info formats -- so what is
// reported and reserved is what runs.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "conv_tiles.h"
#include "yolo_internal.h"

namespace yolo {

// 16-byte epilogue accesses are possible when every stride of the view is chunk-aligned (planned buffers start 4096-byte aligned
// inside a 256-byte aligned workspace; a caller-owned tensor is checked at launch)
static void conv_vec_flags(const yolo_net *net, const Kernel &k, bool out_f32, int &vec_out, int &vec_res) {
    const int epc = net->epc;
    const int ch = k.cfg == CFG_N32 ? 8 : 16;
    const int oepc = out_f32 ? 4 : epc;
    vec_out = (k.cout % ch == 0) && view_chunk_aligned(k.out, oepc);
    vec_res = k.has_res && (k.cout % ch == 0) && view_chunk_aligned(k.in2, epc);       // (a residual has no base: plan.cpp refuses float32 head views)
}

// Every field of a conv's launch parameters that needs no device pointer, for one planned kernel at the given batch: all that
// resolve_conv and the symbol functions read.  forward.cpp's conv_params adds the pointers, the 2 GiB checks and the objectness block.
void conv_shape_params(const yolo_net *net, const Kernel &k, int batch, ConvParams &p) {
    memset(&p, 0, sizeof p);
    const yolo_layer_desc &d = net->layers[k.src_layer].d;
    p.H = k.in.H; p.W = k.in.W; p.in_ld = k.in.ld; p.in_coff = k.in.coff; p.in_img_stride = k.in.img_stride;
    p.Ho = net->layers[k.src_layer].H; p.Wo = net->layers[k.src_layer].W; p.HoWo = p.Ho * p.Wo;
    p.M = (int)((long long)batch * p.HoWo);
    p.Cout = k.cout;
    p.out_ld = k.out.ld;
    p.out_img_stride = k.out.img_stride;
    p.f32 = net->opt.dtype == YOLO_DTYPE_F32;
    p.out_f32 = k.out.f32 || p.f32;
    {   // extents for buffer-addressed epilogues (conv_tap.hip stream kernel): 0 when a tensor is not below 2 GiB
        const long long ob = (long long)batch * k.out.img_stride * (p.out_f32 ? 4 : net->esize);
        p.out_bytes = ob > 0 && ob <= 0x7ffffff0LL ? (uint32_t)ob : 0u;
    }
    p.wgt_bytes = (uint32_t)k.w_bytes;
    p.ksize = d.ksize; p.stride = d.stride; p.pad = (d.ksize - 1) / 2; p.taps = d.ksize * d.ksize;
    p.ktiles = k.ktiles;
    p.tiles_per_tap = k.perchunk ? 1 : k.cpt / 8;
    p.cin_chunks = k.cpt;
    p.cpt_shift = k.cpt == 1 ? 0 : k.cpt == 2 ? 1 : 2;
    p.wrow_bytes = (uint32_t)k.ktiles * 128;
    p.leaky = k.leaky; p.outmode = k.outmode; p.has_res = k.has_res;
    conv_vec_flags(net, k, p.out_f32 != 0, p.vec_out, p.vec_res);
    if (k.has_res) {
        p.res_ld = k.in2.ld;
        p.res_img_stride = k.in2.img_stride;
        const long long rb = (long long)batch * k.in2.img_stride * net->esize;
        p.res_bytes = rb > 0 && rb <= 0x7ffffff0LL ? (uint32_t)rb : 0u;
    }
}

// the LDS-DMA kernels take fp16 convs whose Cin is a multiple of 4 chunks (32 channels)
// float32 nets: only the tap-reuse kernel (3x3/1) has a float32 instantiation besides the 4-wave kernel
bool dma_eligible(const yolo_net *net, const Kernel &k) {
    if (k.cpt % 4) return false;
    return net->opt.dtype == YOLO_DTYPE_F16 || (k.ksize == 3 && k.stride == 1);
}
// tile 0 = the 4-wave kernel of conv.hip with the planner's cfg (always available)
bool conv_tile_valid(const yolo_net *net, const Kernel &k, int tile) {
    if (tile < 0 || tile >= kNumTiles) return false;
    const ConvTile &t = conv_tile(tile);
    if (k.outmode == OUT_POOL2 && !t.has(CAP_POOL)) return false;      // the fused max-pool lives in the 16 x 16 2-D tap tiles
    if (tile == TILE_4WAVE) return true;
    if (net->opt.dtype == YOLO_DTYPE_F32 && !t.f32_ok()) return false;
    if (t.image_aligned() && k.in.H != k.in.W) return false;     // the image-aligned tap tiles: square maps (the rules price tiles by W alone)
    if (t.stride2() && ((k.in.H & 1) || net->opt.dtype != YOLO_DTYPE_F16)) return false;      // stride 2 over parity planes: even maps, fp16
    return dma_eligible(net, k) && dma_cfg_valid(tile, k.cout, k.cpt, true, k.ksize, k.stride, k.in.W);
}

namespace {

// Tile geometry.  Workgroups a stride-1 tap tile of the padded-linear grid launches (p.HoWo > 0; the tiles that split K are such): position
// tiles -- image-aligned: a tile per image -- times cout tiles.
long long tap_blocks(const ConvParams &p, int tile) {
    const ConvTile &t = conv_tile(tile);
    const long long images = p.M / p.HoWo, mq = images * (p.H + 1) * (p.W + 1);         // mq: padded-linear positions
    return (t.image_aligned() ? images : (mq + t.nb() - 1) / t.nb()) * ((p.Cout + t.na() - 1) / t.na());
}
// Partial sums of a launch whose splits meet inside it (conv_tap.hip): every split of every tile owns a float32 slab of the whole tile
size_t pair_slab_bytes(int tile, long long tiles, int ks) { return (size_t)tiles * (size_t)ks * 128 * (size_t)conv_tile(tile).nb() * 4; }
// ... and of one whose splits meet in splitk_reduce_kernel: part[ks][M][cout_pad]
size_t reduce_slab_bytes(const ConvParams &p, long long ks) { return (size_t)ks * (size_t)p.M * (size_t)((p.Cout + 127) / 128 * 128) * 4; }

// Split-K decision for one conv launch (0 = the 4-wave kernel with the planner's cfg, else a tap-reuse tile): when the launch
// would leave most of the chip idle (<= 128 workgroups) and K is long, the K range is cut into `ks` splits of `ku` units
// (conv_tap.hip: channel slices, conv.hip: K tiles) so that ~384 workgroups exist; their float32 partial sums meet in
// splitk_reduce_kernel.  Returns 1 when the launch stays whole.
int choose_ksplit(const Kernel &k, const ConvParams &p, int tile, size_t slab_bytes, int &ku) {
    ku = 0;
    if (!slab_bytes || p.M <= 0) return 1;
    long long blocks;
    int units, min_units;
    if (tile == TILE_4WAVE) {
        const int na = k.cfg == CFG_N128 ? 128 : k.cfg == CFG_N64 ? 64 : 32, nb = k.cfg == CFG_N128 ? 128 : 256;
        blocks = ((long long)p.M + nb - 1) / nb * ((p.Cout + na - 1) / na);
        units = p.ktiles;
        min_units = 2;                  // >= 64 (float32) / 128 (fp16) k per split: these launches are latency-bound, not MFMA-bound
    } else if (conv_tile(tile).has(CAP_SPLITK)) {
        blocks = tap_blocks(p, tile);
        units = p.cin_chunks >> 2;
        min_units = 2;                  // >= 288 (float32) / 576 (fp16) k per split
    } else {
        return 1;
    }
    if (blocks > 128 || units < 2 * min_units) return 1;
    // workgroups = blocks x ks: 512 (two per CU) when K is long enough for that many splits, else 256, else whatever K allows --
    // a count between the two leaves some CUs with two workgroups and the rest with one, and the pairs set the time
    const long long kmax = units / min_units < 32 ? units / min_units : 32;
    long long ks = 512 / blocks;
    if (ks > kmax) ks = 256 / blocks;
    if (ks > kmax) ks = kmax;
    // the partial sums are written and read back once: worth it while that traffic stays in the order of the weight stream the
    // launch reads anyway (measured: YOLOv2 13x13 at batch 1, 22 MB of partials beside 38 MB of weights, 553 -> 70 us; YOLOv3 19x19
    // at batch 8, 47 MB beside 9 MB, slower than unsplit); a few MB are always fine (L2-resident, ~2 us)
    const size_t wbytes = (size_t)p.Cout * (size_t)p.taps * (size_t)p.cin_chunks * 16;
    // (1x1 layers: up to 24 MB -- tiny-YOLOv2's head 1024 -> 125 at 13x13, batch 64, is 85 workgroups walking K = 1024 alone: 85 us whole,
    // 53 us as four splits with 22 MB of partial sums)
    // 3x3: 8 MB; 16 MB where a split still walks a long K loop -- float32 (MFMA 16x slower: YOLOv2-416 b1 104 x 104 64 -> 128 43 -> 33 us,
    // 52 x 52 and 26 x 26 layers 40 -> 33 us, step 0.815 -> 0.757 ms) or >= 8 channel slices (YOLOv3-608 b1 38 x 38: 2 -> 4 splits, 19.6 -> 18 us);
    // a short-K fp16 layer loses with it (76 x 76 128 -> 256 at batch 1: 15.7 -> 18.8 us)
    const size_t small_cap = (size_t)(p.taps == 1 ? 24 : (p.f32 || units >= 8) ? 16 : 8) << 20;
    while (ks >= 2 && (reduce_slab_bytes(p, ks) > slab_bytes || reduce_slab_bytes(p, ks) > (2 * wbytes > small_cap ? 2 * wbytes : small_cap))) --ks;
    if (ks < 2) return 1;
    ku = (int)((units + ks - 1) / ks);
    return (units + ku - 1) / ku;       // every split owns at least one unit
}

}  // namespace

// The record of one launch of conv `ki` with the shape parameters `p` (conv_shape_params, ksplit not yet set: the lean epilogue
// the back-to-back fusion needs is judged for the whole-K launch).  tile_req < 0: the rules of choose_dma_cfg; >= 0: an autotuned or
// forced tile, or an autotune candidate, which runs as named.  slab_bytes: partial-sum bytes the launch may use -- the arena's real
// data bytes when launching or reporting, kSplitkSlabMax when the slab is being sized.
ConvLaunch resolve_conv(const yolo_net *net, size_t ki, const ConvParams &p, int tile_req, size_t slab_bytes) {
    const Kernel &k = net->kernels[ki];
    int tile = tile_req;
    if (!dma_eligible(net, k) || (tile > 0 && !conv_tile_valid(net, k, tile))) tile = 0;
    else if (tile < 0) {
        tile = choose_dma_cfg(p.M, k.cout, k.cpt, p.taps, k.has_res, true, k.stride, k.in.W, net->opt.dtype == YOLO_DTYPE_F32);
        auto or_else = [&](int a, int b) { return conv_tile_valid(net, k, a) ? a : b; };
        if (tile == TILE_TAPIMG_128x384 && !conv_tile_valid(net, k, tile)) tile = or_else(TILE_TAP_256x224, TILE_TAP_128x256);
        if (tile == TILE_TAPIMG_128x192 && !conv_tile_valid(net, k, tile)) tile = or_else(TILE_TAP_128x192, TILE_TAP_128x256);
        if ((tile == TILE_TAPS2_128x256 || tile == TILE_TAPS2IMG_128x384) && !conv_tile_valid(net, k, tile)) tile = or_else(TILE_TAPS2_128x256, or_else(TILE_DMA_256x128_K32, TILE_4WAVE));
        if (tile == TILE_TAPS2_128x256_WIDE && !conv_tile_valid(net, k, tile)) tile = or_else(TILE_DMA_128x256_K32, TILE_4WAVE);
    }
    ConvLaunch r{tile, 1, 0, 0, 0, 0};
    const bool tap_by_rule = conv_tile(tile).is_tap() && tile_req <= 0;     // (an explicitly requested tile -- force_tile, an autotune candidate -- runs as requested: the hook must time and test the tile it names)
    const int units = p.cin_chunks >> 2;        // channel slices
    // K in two halves inside ONE launch (conv_tap.hip): two co-resident half-K workgroups per tile, the second arriver sums -- no reduce
    // kernel, two slabs per tile.  For a long K on a tap tile by rule; `lo`..`hi` tiles of tile `t`.
    static const bool no_pair = getenv("YOLO_NO_PAIR_SPLIT") != nullptr;       // A/B switch (read once; results unchanged up to summation order)
    const bool pair_ok = tap_by_rule && !no_pair && units >= 8 && p.HoWo > 0;
    auto pair_on = [&](int t, long long lo, long long hi) {
        if (!pair_ok || !conv_tile_valid(net, k, t)) return false;
        const long long tiles = tap_blocks(p, t);
        if (tiles < lo || tiles > hi || pair_slab_bytes(t, tiles, 2) > slab_bytes) return false;
        r.tile = t; r.ks = 2; r.ku = (units + 1) / 2; r.pair = 1;
        return true;
    };
    // The WIDE tiles first (fp16): 64-128 tiles of the image-aligned 128 x 192 or of the 128 x 256 -- half the weight bytes per flop of
    // the 128 x 128 tile, whose K loop is bound per CU by the LDS-DMA path (8 KiB of weights per tap for 1 MFLOP: two half-K workgroups
    // on a CU were measured no faster than one whole-K one).  Such a launch is not split any other way.
    // (those instantiations are built for ONE workgroup per CU -- they need 180 registers --, so at most 128 tiles = 256 half-K workgroups:
    // 26 x 26 at batch 16 = 184 tiles ran 48 us as 368 halves against 33 us whole)
    // (12 x 12 / 13 x 13 maps: one image per 192-position tile -- 5 % padding where 256-position tiles of the padded-linear grid
    // compute 23 %, and 16 images x 8 cout tiles x 2 halves are exactly 256 workgroups: YOLOv2-416 b16 13 x 13 layers -25 %)
    const bool wide_pair = !p.f32 && (pair_on(TILE_TAPIMG_128x192, 64, 128) || pair_on(TILE_TAP_128x256, 64, 128));
    if (!wide_pair) {
        r.ks = choose_ksplit(k, p, tile, slab_bytes, r.ku);
        // a 3x3/1 layer small enough for split-K runs it on the 128 x 128 tap tile (the one with the split-K instantiation), whatever
        // tile the cost model would pick for the whole-K launch
        if (r.ks <= 1 && tap_by_rule && tile != TILE_TAP_128x128 && conv_tile_valid(net, k, TILE_TAP_128x128)) {
            int ku11 = 0;
            const int ks11 = choose_ksplit(k, p, TILE_TAP_128x128, slab_bytes, ku11);
            if (ks11 > 1) { r.tile = TILE_TAP_128x128; r.ks = ks11; r.ku = ku11; }
        }
        // still whole: 129-256 tiles of 128 x 128 (13 x 13 / 19 x 19 maps at batch 8-32, any dtype) -- every workgroup would run ALONE on
        // its CU at 0.6 of the rate a pair reaches (block trace, profiles/r03_ablation.md)
        if (r.ks <= 1) pair_on(TILE_TAP_128x128, 129, 256);
        // Split-K on the 128 x 128 tap tile (small maps at batch 1-4: a handful of tiles, K in up to 32 splits): the splits meet INSIDE the
        // launch -- ticket per tile, the last arriver sums every split's slab in split order and runs the fused epilogue (conv_tap.hip) --
        // instead of in a splitk_reduce_kernel launch of its own (YOLOv3-608 at batch 1: 20 of 95 launches).
        // (up to eight splits: ONE workgroup reads them all -- 38 x 38 at batch 1, 2 splits: 23 -> 20 us; 19 x 19, 8 splits: 25.5 -> 24; beyond
        // that the reduce launch, which spreads the sum over the chip, wins: 13 x 13 float32 with 16 / 32 splits 38 -> 40.5 / 61 -> 67 us)
        static const bool no_inl = getenv("YOLO_NO_INLAUNCH_SPLITK") != nullptr;      // A/B switch (same results up to the fp32 summation order of the splits)
        if (r.ks > 1 && r.ks <= 8 && !r.pair && r.tile == TILE_TAP_128x128 && !no_inl) {
            const long long tiles = tap_blocks(p, r.tile);
            if (tiles * 128 <= (long long)kPairCounterBytes && pair_slab_bytes(r.tile, tiles, r.ks) <= slab_bytes) r.pair = 1;
        }
    }
    if (r.pair) r.slab_need = pair_slab_bytes(r.tile, tap_blocks(p, r.tile), r.ks);
    else if (r.ks > 1) r.slab_need = reduce_slab_bytes(p, r.ks);
    // Back-to-back 1x1: does this launch also compute the 1x1 conv `ki + 1` (plan.cpp marked the pair)?  Yes when the tile holds all 128
    // couts of 256 positions per workgroup and has the fused instantiation (CAP_FUSE2) -- the 2-D 128 x 256 tap tile with a residual, the
    // 128 x 256 K32 LDS-DMA tile or the wide stride-2 tap tile, both without --, whole K, lean epilogue.
    const ConvTile &rt = conv_tile(r.tile);
    if (k.fuse2_next && ki + 1 < net->kernels.size() && net->kernels[ki + 1].fuse2_prev && rt.has(CAP_FUSE2) &&
        r.ks <= 1 && conv_fast_epilogue_ok(p) && rt.has(CAP_FUSE2_RES) == (p.has_res != 0) && p.HoWo > 0) {
        const long long ob = (long long)(p.M / p.HoWo) * net->kernels[ki + 1].out.img_stride * net->esize;       // the 1x1's output: buffer-addressed
        r.fuse2 = ob > 0 && ob <= 0x7ffffff0LL;
    }
    return r;
}

// float32 partial-sum slab one arena needs for ANY batch up to its share of max_batch (a net built for batch 32 also runs
// the short last batch of a TEST directory, where the small maps do split): 0 when no launch ever splits
// (an MXFP8 conv counts as the fp16 launch it replaces)
size_t splitk_slab_bytes(const yolo_net *net) {
    const int per = net->arena_full ? net->opt.max_batch : (net->opt.max_batch + net->arenas - 1) / net->arenas;
    size_t need = 0;
    for (size_t ki = 0; ki < net->kernels.size(); ++ki) {
        const Kernel &k = net->kernels[ki];
        if (!conv_dispatched(k)) continue;
        for (int b = 1; b <= per; ++b) {
            ConvParams p;
            conv_shape_params(net, k, b, p);
            const size_t bytes = resolve_conv(net, ki, p, k.tile, kSplitkSlabMax).slab_need;
            if (bytes > need) need = bytes;
        }
    }
    // layout of an arena's slab: [ticket counters of the in-launch pair split, kPairCounterBytes | partial sums]: the counters must
    // never be written by anything but the pair kernels (they rely on finding them at zero)
    return need ? kPairCounterBytes + (need + 4095) / 4096 * 4096 : 0;
}

bool pass_splits_k(const yolo_net *net, int batch) {
    for (size_t ki = 0; ki < net->kernels.size(); ++ki) {
        const Kernel &k = net->kernels[ki];
        if (!conv_dispatched(k)) continue;
        ConvParams p;
        conv_shape_params(net, k, batch, p);
        if (resolve_conv(net, ki, p, k.tile, arena_slab_data_bytes(net)).ks > 1) return true;
    }
    return false;
}

// yolo_net_kernel_info of a conv kernel (out: zeroed, kind and layer set): its work, and the kernel that runs at max_batch (bench.py runs at
// max_batch) -- the record the launch path builds, formatted
void conv_kernel_info(const yolo_net *net, int kernel, yolo_kernel_info *out) {
    const Kernel &k = net->kernels[kernel];
    const char *t = dtype_tag(net);
    const LayerInfo &li = net->layers[k.src_layer];
    out->variant = k.cfg + 4 * k.perchunk;
    out->ksize = k.ksize; out->stride = k.stride; out->cin = k.cin; out->cout = k.cout; out->out_h = li.H; out->out_w = li.W;
    out->flops = 2.0 * li.H * li.W * k.cout * k.ksize * k.ksize * k.cin;
    out->bytes = (double)k.in.H * k.in.W * k.cin * net->esize + view_elems(k.out) * view_esz(net, k.out) + (k.has_res ? view_elems(k.in2) * net->esize : 0.0);
    out->weight_bytes = (double)k.cout * k.ksize * k.ksize * k.cin * net->esize + 4.0 * k.cout;
    if (k.stem == STEM_TAIL) {          // no launch of its own
        out->flops = 0; out->bytes = 0; out->weight_bytes = 0;
        snprintf(out->name, sizeof out->name, "conv_igemm<fused into conv_stem>");
        return;
    }
    if (k.stem == STEM_HOST) {
        const Kernel &f = net->kernels[kernel - 1];
        out->flops += 2.0 * f.out.H * f.out.W * f.cout * 27;
        out->bytes = (double)f.in.H * f.in.W * 3 * 4 + view_elems(k.out) * view_esz(net, k.out);
        out->weight_bytes += 28.0 * f.cout * 4;
        snprintf(out->name, sizeof out->name, "conv_stem<f16,3-32-64>");
        set_symbol(out, "yolo::stem_v3_kernel(yolo::StemParams)");
        if (kernel + 1 < (int)net->kernels.size() && net->kernels[kernel + 1].stem == STEM_TAIL) {
            const Kernel &t3 = net->kernels[kernel + 1];
            out->flops += 2.0 * li.H * li.W * t3.cout * t3.cin;
            out->bytes += view_elems(t3.out) * view_esz(net, t3.out);
            out->weight_bytes += (double)t3.cout * t3.cin * net->esize + 4.0 * t3.cout;
            snprintf(out->name, sizeof out->name, "conv_stem<f16,3-32-64-32>");
        }
        return;
    }
    if (k.mx) {         // e4m3 weights + one scale byte per 32 of them; fp16 activations in and out
        ConvParams mp;
        conv_shape_params(net, k, part_batch(net), mp);
        out->variant = 8 + kMxTile;
        out->weight_bytes = (double)k.cout * k.ksize * k.ksize * k.cin * (1.0 + 1.0 / 32) + 4.0 * k.cout;
        snprintf(out->name, sizeof out->name, "conv_mx<mxf8,128x256>");
        set_symbol(out, conv_mx_symbol(conv_fast_epilogue_ok(mp)));
        return;
    }
    ConvParams sp;
    const int per_arena = part_batch(net);
    if (k.fuse2_prev && kernel > 0) {       // computed by the conv in front of it at this batch?
        conv_shape_params(net, net->kernels[kernel - 1], per_arena, sp);
        if (resolve_conv(net, (size_t)kernel - 1, sp, net->kernels[kernel - 1].tile, arena_slab_data_bytes(net)).fuse2) {
            out->flops = 0; out->bytes = 0; out->weight_bytes = 0;
            snprintf(out->name, sizeof out->name, "conv_igemm<fused into the conv in front>");
            return;
        }
    }
    conv_shape_params(net, k, per_arena, sp);
    const ConvLaunch pk = resolve_conv(net, (size_t)kernel, sp, k.tile, arena_slab_data_bytes(net));
    const bool fused2 = pk.fuse2 != 0;
    if (fused2) {       // this launch also computes the 1x1 behind it: its work and its output belong here
        const Kernel &b2 = net->kernels[kernel + 1];
        out->flops += 2.0 * li.H * li.W * b2.cout * b2.cin;
        out->bytes += view_elems(b2.out) * view_esz(net, b2.out);
        out->weight_bytes += (double)b2.cout * b2.cin * net->esize + 4.0 * b2.cout;
    }
    const int tile = pk.tile;
    if (tile > 0) {
        out->variant = 8 + tile;
        snprintf(out->name, sizeof out->name, "conv_igemm_dma<%s,%s>", t, conv_tile(tile).name);
        sp.ksplit = pk.ks; sp.pair = pk.pair; sp.fuse2 = pk.fuse2;       // as launched
        set_symbol(out, conv_tile_symbol(tile, sp));
    } else {
        const bool emu = conv_f32_emu_rule(net->opt.f32_products, net->opt.dtype, sp, k.cfg, k.perchunk != 0, pk.ks);
        set_symbol(out, conv_symbol(net->opt.dtype, k.cfg, k.perchunk != 0, emu));
        if (emu) snprintf(out->name, sizeof out->name, "conv_igemm_emu<f32 as 9 x bf16,N128>");
        else snprintf(out->name, sizeof out->name, "conv_igemm<%s,N%d,%s>", t, k.cfg == CFG_N128 ? 128 : k.cfg == CFG_N64 ? 64 : 32,
                      k.perchunk ? "perchunk" : "uniform");
    }
    const double part_bytes = (double)pk.ks * (double)li.H * li.W * ((k.cout + 127) / 128 * 128) * 4.0;
    std::string tags;
    if (k.outmode == OUT_POOL2) tags += "+pool";
    if (fused2) tags += "+1x1";
    if (pk.pair) {              // K in two halves (or pk.ks splits) inside the launch
        tags += pk.ks == 2 ? "+pairK" : "+splitK" + std::to_string(pk.ks) + ",1launch";
        out->bytes += part_bytes;
    } else if (pk.ks > 1) {     // two launches: K splits into the float32 slab, then splitk_reduce_kernel (sum + fused epilogue)
        tags += "+splitK" + std::to_string(pk.ks);
        out->bytes += 2.0 * part_bytes;     // partial sums written + read once
    }
    const size_t n = strlen(out->name);
    snprintf(out->name + n, sizeof out->name - n, "%s", tags.c_str());
}

}  // namespace yolo

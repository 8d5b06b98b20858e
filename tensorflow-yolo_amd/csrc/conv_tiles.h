// What a conv tile id IS: one row of kTiles per id.  The ids are public (yolo_net_options.force_tile, yolo_kernel_info.variant =
// 8 + tile, bench.py --force-tile, every file under profiles/), so a row never moves.
// A row holds the template arguments of the tile's kernel -- the launchers instantiate from the row, the symbol functions format the same
// numbers, the geometry (couts x positions per workgroup, workgroups per CU) is computed from them --, what the tile can do (caps) and its
// constants in the cost model (choose_dma_cfg).  A PROPERTY ("is image-aligned") is read from the row; only a measured RULE ("152 x 152
// 64 -> 128 runs on the 2-D 128 x 256 tile") names a TileId.
// Adding tile 24: a row here and its TileId; an arm in the family's *_form / launch_*_tile pair if it brings a form no tile has yet; a rule
// or cost constants in choose_dma_cfg if anything should pick it.
#pragma once

namespace yolo {

enum TileId {
    TILE_4WAVE = 0,     // conv.hip, with the planner's cfg
    TILE_DMA_256x256_K64 = 1, TILE_DMA_256x128_K64 = 2, TILE_DMA_128x256_K64 = 3, TILE_DMA_256x256_K32 = 4, TILE_DMA_256x128_K32 = 5,
    TILE_DMA_128x256_K32 = 6, TILE_DMA_64x512 = 7,
    TILE_TAP_128x256 = 8, TILE_TAP_256x256 = 9, TILE_TAP_128x192 = 10, TILE_TAP_128x128 = 11, TILE_TAP2D_128x256 = 12, TILE_TAP2D_64x256 = 13,
    TILE_DMA_128x128_X3 = 14,
    TILE_TAP_256x224 = 15, TILE_TAP2D_128x128_X3 = 16, TILE_TAP2D_32x256 = 17, TILE_TAPIMG_128x384 = 18,
    TILE_DMA_128x192_S4 = 19,
    TILE_TAPS2_128x256 = 20, TILE_TAPS2IMG_128x384 = 21, TILE_TAPIMG_128x192 = 22, TILE_TAPS2_128x256_WIDE = 23,
    kNumTiles = 24
};

enum TileFamily { FAM_4WAVE, FAM_DMA, FAM_TAP };      // conv.hip conv_igemm_kernel | conv_dma.hip conv_igemm_dma_kernel | conv_tap.hip conv3x3_tap_kernel
enum TileCaps : unsigned {
    CAP_F32 = 1,        // has float32 instantiations (tap tiles with TP <= 2: room for the second-level accumulator)
    CAP_SPLITK = 2,     // takes ConvParams.ksplit with a reduce launch behind it (the in-launch pair: ConvTile.split_occ)
    CAP_POOL = 4,       // the 2x2/2 max-pool behind the conv in its epilogue (MODE 3 of the 16 x 16 2-D tiles)
    CAP_FUSE2 = 8,      // hosts the back-to-back 1x1: all 128 couts of 256 positions in one workgroup, no residual ...
    CAP_FUSE2_RES = 16, // ... or (with CAP_FUSE2) only WITH a residual: the residual block's 3x3
    CAP_STREAM = 32,    // has the persistent form (conv3x3_tap_stream_kernel)
    CAP_RULE_ONLY = 64, // never a candidate of the cost model: chosen by a rule of choose_dma_cfg / the planner, or by name
    CAP_NO_LEAN = 128,  // generic epilogue even where the lean one applies, unless it hosts the 1x1 (lean only): the lean two-per-CU stride-2 build spills 13 registers
    CAP_IMAGE = 256     // image-aligned: a tile = one whole image of the padded-linear grid (tile stride (H+1)(W+1)), the pad row behind an image is never computed
};

// Cost model of choose_dma_cfg: us per 64-deep K tile when more workgroups than slots share the CUs / when 257-512 of a two-per-CU
// tile do / when a workgroup has its CU alone; fixed us per round.  All zero: chosen by rule.
struct TileCost { float a_shared, a_mid, a_alone, f; };
struct ConvTile {
    int id;
    TileFamily family;
    const char *name;           // part of yolo_kernel_info.name
    // template arguments of the kernel: WM x WN waves of TM x TP 16 x 16 fragments; S = LDS ring depth (LDS-DMA); PRG = 16-position row
    // groups of the input patch in LDS (tap); BKC = 16-byte K chunks per stage: Cin must be a multiple; OCC = waves per SIMD the
    // register budget allows; MODE (tap) = the position grid: 1 padded-linear (one shared pad column per row, one pad row per image), 2 2-D
    // (NB / 16 x 16 pixels), 4 stride 2 (padded-linear grid of the OUTPUT map over the input's four parity planes); the other kernels: NB consecutive pixels
    int wm, wn, tm, tp, s, prg, bkc, occ, mode;
    unsigned caps;
    int split_occ;              // tap: OCC of the SPLITK instantiation the in-launch pair split runs (0: none).  The wide tiles' are built
                                // for one workgroup per CU: <= 512 half-K workgroups on 256 CUs, and they need 180 registers
    TileCost cost;

    constexpr int na() const { return wm * tm * 16; }           // couts per workgroup
    constexpr int nb() const { return wn * tp * 16; }           // positions per workgroup
    constexpr int per_cu() const { return occ / 2; }            // resident workgroups per CU
    constexpr bool has(unsigned cap) const { return (caps & cap) != 0; }
    constexpr bool is_tap() const { return family == FAM_TAP; }
    constexpr bool f32_ok() const { return has(CAP_F32); }
    constexpr bool stride2() const { return mode == 4; }
    constexpr bool is2d() const { return mode == 2; }
    constexpr bool image_aligned() const { return has(CAP_IMAGE); }
};

constexpr ConvTile dma_tile(int id, const char *name, int wm, int wn, int tm, int tp, int s, int bkc, int occ, unsigned caps, TileCost cost) {
    return {id, FAM_DMA, name, wm, wn, tm, tp, s, 0, bkc, occ, 0, caps, 0, cost};
}
constexpr ConvTile tap_tile(int id, const char *name, int wm, int wn, int tm, int tp, int prg, int occ, int mode, unsigned caps, int split_occ, TileCost cost) {
    return {id, FAM_TAP, name, wm, wn, tm, tp, 0, prg, 4, occ, mode, caps, split_occ, cost};
}
constexpr TileCost kByRule = {0.0f, 0.0f, 0.0f, 0.0f};
constexpr ConvTile kTiles[kNumTiles] = {
    // the CFG_N128 form of the 4-wave register-staged kernel: 2 x 2 waves, two workgroups per CU
    {TILE_4WAVE, FAM_4WAVE, "", 2, 2, 4, 4, 0, 0, 8, 4, 0, 0, 0, {1.14f, 1.14f, 0.82f, 9.0f}},
    //       id                     name                  WM WN TM TP  S BKC OCC
    dma_tile(TILE_DMA_256x256_K64, "256x256,K64,S2",       2, 4, 8, 4, 2, 8, 2, 0, {1.45f, 1.45f, 1.45f, 20.0f}),
    dma_tile(TILE_DMA_256x128_K64, "256x128,K64,S3",       4, 2, 4, 4, 3, 8, 2, 0, {0.82f, 0.82f, 0.82f, 12.0f}),
    dma_tile(TILE_DMA_128x256_K64, "128x256,K64,S3",       2, 4, 4, 4, 3, 8, 2, 0, {0.82f, 0.82f, 0.82f, 12.0f}),
    dma_tile(TILE_DMA_256x256_K32, "256x256,K32,S4",       2, 4, 8, 4, 4, 4, 2, 0, {1.47f, 1.47f, 1.47f, 20.0f}),      // 96 KiB in flight instead of 64
    dma_tile(TILE_DMA_256x128_K32, "256x128,K32,S3,x2",    4, 2, 4, 4, 3, 4, 4, 0, {1.75f, 1.75f, 1.30f, 8.0f}),       // 72 KiB LDS, <= 128 VGPRs: two workgroups per CU
    dma_tile(TILE_DMA_128x256_K32, "128x256,K32,S3,x2",    2, 4, 4, 4, 3, 4, 4, CAP_FUSE2, {1.75f, 1.75f, 1.30f, 8.0f}),
    dma_tile(TILE_DMA_64x512, "64x512,K32,S2,x2",          1, 8, 4, 4, 2, 4, 4, CAP_RULE_ONLY, kByRule),               // narrow early layers (Cout <= 64), bandwidth-bound
    // conv_tap.hip, 3x3 only: the input patch is loaded once for the nine taps (the cost constants are fitted on the sweep of
    // tools/gpu_tile_sweep.sh: v3-608-b32, v3-416-b32, v2-416-b16, within ~8 %)
    //       id                 name                   WM WN TM TP PRG OCC MODE                            split_occ
    tap_tile(TILE_TAP_128x256, "128x256,tap9,x2",       2, 4, 4, 4, 26, 4, 1, 0, 2, {1.20f, 1.45f, 0.76f, 7.9f}),
    tap_tile(TILE_TAP_256x256, "256x256,tap9",          2, 4, 8, 4, 26, 2, 1, 0, 0, {1.20f, 1.20f, 1.20f, 20.0f}),
    tap_tile(TILE_TAP_128x192, "128x192,tap9,x2",       2, 4, 4, 3, 26, 4, 1, 0, 0, {0.94f, 1.32f, 0.68f, 8.5f}),      // smaller position tiles fill the 512 workgroup slots better on small maps
    tap_tile(TILE_TAP_128x128, "128x128,tap9,x2",       2, 4, 4, 2, 28, 4, 1, CAP_F32 | CAP_SPLITK, 4, {0.76f, 0.90f, 0.63f, 6.9f}),
    // 2-D 16 x 16 tiles for maps wider than 78 (152x152 64->128: 175 us, 76x76: 117, 38x38: 138)
    tap_tile(TILE_TAP2D_128x256, "128x256,tap9,2d,x2",  2, 4, 4, 4, 27, 4, 2, CAP_POOL | CAP_FUSE2 | CAP_FUSE2_RES, 0, {0.90f, 1.10f, 0.60f, 17.0f}),
    tap_tile(TILE_TAP2D_64x256, "64x256,tap9,2d,x2",    1, 8, 4, 2, 27, 4, 2, CAP_F32 | CAP_POOL | CAP_STREAM | CAP_RULE_ONLY, 0, {1.00f, 1.00f, 0.60f, 5.8f}),    // ... and Cout <= 64
    // 48 KiB LDS, <= 80 VGPRs: three workgroups per CU; 1x1 layers only (short K, memory / latency bound)
    dma_tile(TILE_DMA_128x128_X3, "128x128,K32,S3,x3",     2, 4, 4, 2, 3, 4, 6, 0, {1.10f, 1.50f, 0.70f, 8.0f}),
    // 19 x 19 at batch 32 = 12 800 padded positions -> 232 tiles on 256 CUs (256-position tiles: 200 or 400 workgroups on 256 / 512 slots); 7/8 of the 256x256 tile's loop
    tap_tile(TILE_TAP_256x224, "256x224,tap9",          4, 2, 4, 7, 17, 2, 1, 0, 0, {1.05f, 1.05f, 1.05f, 18.0f}),
    // 8 x 16 2-D tile, THREE per CU (48 KiB LDS, <= 80 VGPRs): wide maps with a short K, setup + epilogue as long as the K loop (152 x 152 64 -> 128: profiles/r03_ablation.md)
    tap_tile(TILE_TAP2D_128x128_X3, "128x128,tap9,2d,x3", 2, 4, 4, 2, 12, 6, 2, CAP_RULE_ONLY, 0, kByRule),
    // tiny-YOLOv2 16 -> 32 at 208 x 208 (float32 MFMA is 1/16 of fp16's: the 64-cout tile's idle half would double an MFMA-bound launch)
    tap_tile(TILE_TAP2D_32x256, "32x256,tap9,2d,x2",    1, 8, 2, 2, 27, 4, 2, CAP_F32 | CAP_POOL | CAP_RULE_ONLY, 0, kByRule),
    // one whole image with H (W+1) <= 384 per tile (19 x 19: 380; 6 % padding instead of 10.8 %); at batch 32 32 x 8 = 256 tiles: every CU busy, 6/7 of the 256 x 224 tile's loop
    tap_tile(TILE_TAPIMG_128x384, "128x384,tap9,img",   2, 4, 4, 6, 27, 2, 1, CAP_IMAGE, 0, {0.90f, 0.90f, 0.90f, 18.0f}),
    // the whole LDS as a four-stage ring (120 KiB in flight), for one-round 1x1 layers on small maps
    dma_tile(TILE_DMA_128x192_S4, "128x192,K64,S4",        2, 4, 4, 3, 4, 8, 2, 0, {0.60f, 0.60f, 0.60f, 12.0f}),
    // 3x3 / stride 2 with tap reuse over the input's parity planes: fp16 only (costs as tiles 8 and 18)
    tap_tile(TILE_TAPS2_128x256, "128x256,tap9,s2,x2",  2, 4, 4, 4, 21, 4, 4, CAP_NO_LEAN, 0, {1.20f, 1.45f, 0.76f, 7.9f}),
    tap_tile(TILE_TAPS2IMG_128x384, "128x384,tap9,s2,img", 2, 4, 4, 6, 26, 2, 4, CAP_IMAGE, 0, {0.90f, 0.90f, 0.90f, 18.0f}),
    // one 12 x 12 or 13 x 13 image per tile (YOLOv2-416 / YOLOv3-416 tails: 182 of 192 positions real, 256-position padded-linear tiles compute 23 % padding);
    // with the in-launch pair split 16 images x 8 cout tiles x 2 K halves = 256 workgroups (costs as tile 10)
    tap_tile(TILE_TAPIMG_128x192, "128x192,tap9,img,x2", 2, 4, 4, 3, 14, 4, 1, CAP_IMAGE, 2, {0.94f, 1.32f, 0.68f, 8.5f}),
    // tile 20 with a patch of 26 row groups (output maps up to 158 wide): the stride-2 conv into the 152 x 152 stage; hosts the back-to-back 1x1
    tap_tile(TILE_TAPS2_128x256_WIDE, "128x256,tap9,s2,wide,x2", 2, 4, 4, 4, 26, 4, 4, CAP_FUSE2 | CAP_NO_LEAN | CAP_RULE_ONLY, 0, kByRule),
};
constexpr bool tiles_in_id_order(int i = 0) { return i == kNumTiles || (kTiles[i].id == i && tiles_in_id_order(i + 1)); }
static_assert(tiles_in_id_order(), "kTiles[id].id == id");
inline const ConvTile &conv_tile(int id) { return kTiles[id]; }        // 0 <= id < kNumTiles

// The instantiation one launch runs, chosen from (row, ConvParams as launched) by dma_form / tap_form: the launchers launch it, the symbol functions name it
enum ConvForm {
    FORM_INVALID = 0,   // the tile has no instantiation for this launch
    FORM_GENERIC,       // any output map / view (tap tiles: fp16 or float32 by ConvParams.f32, like the split-K and pool forms)
    FORM_LEAN,          // conv_common.h: conv_epilogue_fast
    FORM_HEAD_F32,      // LDS-DMA: the head convs' float32 rows through LDS slabs
    FORM_SPLITK,        // tap: K split over blockIdx.y -- reduce launch or in-launch pair
    FORM_POOL,          // tap: the fused 2x2/2 max-pool
    FORM_FUSED,         // + the 1x1 conv behind it
    FORM_STREAM         // tap: the persistent kernel
};

}  // namespace yolo

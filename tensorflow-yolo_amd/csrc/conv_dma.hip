// Second-generation implicit-GEMM conv for the heavy fp16 layers: same GEMM view and epilogue as
// conv.hip, but
//   * 8 waves (512 threads), one workgroup per CU, block tiles 256x256 / 256x128 / 128x256
//     (couts x pixels) -> fewer L2->LDS bytes per FLOP than the 128x128 tile;
//   * operands go global -> LDS directly with `buffer_load_dwordx4 ... lds` (LDS-DMA): no staging
//     VGPRs and no ds_write pass (ds_write_b128 tops out at ~79 B/clk/CU and was the bottleneck of
//     the register-staged kernel).  One wave instruction fills 1 KiB of LDS rows (lane-linear), the
//     XOR swizzle is applied to the per-lane SOURCE chunk, zero padding / M tail come from the
//     buffer range check (verified on gfx950: out-of-range lanes write zeros to LDS);
//   * an S-stage LDS ring with counted `s_waitcnt vmcnt(N)` and raw `s_barrier`, so the DMA of the
//     next tile(s) stays in flight across the barrier while the MFMAs of the current tile run.
//     PMC showed the loop is bound by DMA round-trip latency (~5k cycles under load): throughput =
//     bytes in flight / latency, so the K depth of a stage (BKC chunks: 64 or 32 halfs) and S are
//     chosen to keep as much of the 160 KiB LDS in flight as possible (256x256: 4 stages of K=32).
// Per K tile: wait(tile kt landed) -> barrier -> issue DMA of tile kt+S-1 into the stage read at
// kt-1 -> ds_read fragments + MFMAs of tile kt.
#include "conv_common.h"
#include "conv_tiles.h"
#include <cstdio>
#include <utility>
#include <vector>

namespace yolo {

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

typedef __attribute__((address_space(3))) void lds_void;

// One LDS-DMA wave instruction: every lane fetches 16 bytes at byte offset `voff` of the buffer and
// the wave's 1 KiB lands lane-linearly at `lds_dst` (wave-uniform).  The builtin only exists in the
// device pass (its instantiation inside a kernel template fails in the host pass).
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned char *lds_dst, uint32_t voff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void *)lds_dst, 16, voff, 0, 0, 0);
#else
    (void)rsrc; (void)lds_dst; (void)voff;
#endif
}

// LDS image: rows of BKC 16-byte chunks (128 B or 64 B), logical chunk c of row r stored at physical
// chunk c ^ swz(r).  Chosen so that the ds_read_b128 fragment reads (16 rows x one chunk per 16-lane
// group, hardware lane groups {0-3,12-15,20-27} ...) hit 16 distinct 16-byte slots of the 256-byte
// bank window:   BKC = 8: swz = (r >> 1) & 7;   BKC = 4: swz = {0,2,3,1}[(r >> 2) & 3].
template <int BKC>
__device__ __forceinline__ int lds_swz(int r) {
    if (BKC == 8) return (r >> 1) & 7;
    return (0x78 >> (2 * ((r >> 2) & 3))) & 3;
}

// WM x WN = 8 waves; a wave owns TM*16 couts x TP*16 pixels; S = LDS ring depth; BKC = K chunks per stage;
// OCC = waves per SIMD the register budget must allow (2: one workgroup per CU, 4: two per CU, so that
// one workgroup's epilogue -- ~190 MB of residual reads + output writes per 76x76 layer -- overlaps the
// other's MFMA loop; with one lock-stepped workgroup per CU that traffic was 44 % of the layer time).
// FUSE2: the 1x1 conv behind this one computed by the same workgroups (conv_common.h: conv_epilogue_fused_1x1); the 128 x 256 K32
// tile only (all 128 couts of 256 pixels in one workgroup).
// EPI: which epilogue this instantiation carries -- 0 the generic one (any output map / view), 1 the lean one of conv_common.h
// (conv_epilogue_fast: plain fp16 output maps), 2 the head convs' float32 rows through LDS slabs (conv_epilogue_f32_staged).
// Instantiations of their own, like in conv_tap.hip: with the three behind run-time branches in one kernel seven of the ten tiles
// spilled 12-176 registers (the staged epilogue's row flags alone cost the generic path its last registers).
template <int WM, int WN, int TM, int TP, int S, int BKC, int OCC, bool FUSE2 = false, int EPI = 0>
__global__ void __launch_bounds__(512, OCC) conv_igemm_dma_kernel(const ConvParams p) {
    typedef _Float16 T;
    static_assert(WM * WN == 8, "eight waves per workgroup");
    static_assert(S >= 2 && S <= 4, "ring depth 2..4");
    static_assert(BKC == 8 || BKC == 4, "stage depth 64 or 32 halfs");
    constexpr int ROWB = BKC * 16;          // bytes per LDS row
    constexpr int RPI = 1024 / ROWB;        // rows one DMA wave-instruction fills (8 or 16)
    constexpr int NA = WM * TM * 16;        // couts per block
    constexpr int NB = WN * TP * 16;        // pixels per block
    constexpr int JA_TOT = NA / RPI;        // weight DMA wave-instructions per stage, dealt round-robin to the waves
    constexpr int JA = (JA_TOT + 7) / 8;    // per wave (waves >= JA_TOT carry none when the weight tile is small)
    constexpr int JB = NB / (8 * RPI);      // pixel DMA wave-instructions per wave per stage
    constexpr bool A_ALL = JA_TOT % 8 == 0; // every wave issues the same number of weight instructions
    constexpr int NL = JA + JB;             // DMA instructions per stage of a wave that carries weights
    constexpr int KS = BKC / 4;             // 32-deep MFMA k-steps per stage
    constexpr int CH = 4 * TM;
    constexpr int TILE_BYTES = (NA + NB) * ROWB;
    static_assert(JB >= 1 && (A_ALL || JA_TOT < 8), "unsupported tile for the DMA mapping");
    constexpr int LDS_BYTES = FUSE2 && kFuse2LdsBytes > S * TILE_BYTES ? kFuse2LdsBytes : S * TILE_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];

    const int tid = threadIdx.x;
#ifdef YOLO_EXPERIMENT      // block trace (tools/trace_blocks.py); not in the product build
    const unsigned long long t_start = p.trace ? wall_clock64() : 0ull;
    const unsigned long long c_start = p.trace ? (unsigned long long)clock64() : 0ull;
    unsigned long long t_first = 0ull;
#endif
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const bool has_a = A_ALL || wave < JA_TOT;     // wave-uniform

    const int bid = xcd_remap(blockIdx.x, p.n_blocks);
    const int mt = (int)fdiv((uint32_t)bid, p.dtiles_n);
    const int nt = bid - mt * p.n_tiles_n;
    const int n0 = nt * NA;
    const int m0 = mt * NB;

    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.in), 0, p.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.wgt), 0, p.wgt_bytes, 0x00020000);

    // ---- DMA geometry ---------------------------------------------------------------------------
    // wave instruction j of wave w fills row group g = 8 j + w (RPI rows = 1 KiB, lane-linear):
    // lane -> row RPI g + lane / BKC, PHYSICAL chunk lane % BKC, which must hold LOGICAL chunk
    // phys ^ swz(row).  swz(row) only depends on (w & 1, lane) [BKC 8] or lane [BKC 4]: same for all j.
    const int lrow = lane / BKC;
    const uint32_t csw = (uint32_t)(((lane % BKC) ^ lds_swz<BKC>(RPI * (wave & 1) + lrow)) << 4);

    uint32_t a_off[JA];
#pragma unroll
    for (int j = 0; j < JA; ++j) {
        const int r = (j * 8 + wave) * RPI + lrow;              // LDS row of the weight tile
        const int ws = r / (TM * 16), R = r % (TM * 16);
        const int tm = R >> 4, g4 = (R >> 2) & 3, jj = R & 3;
        const int ch = ws * (TM * 16) + g4 * CH + 4 * tm + jj;  // the cout that LDS row holds
        a_off[j] = (uint32_t)(n0 + ch) * p.wrow_bytes + csw;
    }
    uint32_t b_base[JB], b_mask[JB];
#pragma unroll
    for (int j = 0; j < JB; ++j) {
        const int m = m0 + (j * 8 + wave) * RPI + lrow;
        const bool ok = m < p.M;
        const int mm = ok ? m : 0;
        const int n = (int)fdiv((uint32_t)mm, p.dHoWo);
        const int rem = mm - n * p.HoWo;
        const int oy = (int)fdiv((uint32_t)rem, p.dWo);
        const int ox = rem - oy * p.Wo;
        const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
        const long long e = (long long)n * p.in_img_stride + ((long long)iy0 * p.W + ix0) * p.in_ld + p.in_coff;
        b_base[j] = (uint32_t)(e * 2) + csw;
        uint32_t mask = 0;
        if (ok) {
            for (int t = 0; t < p.taps; ++t) {
                const int kh = p.ksize == 3 ? (t * 11) >> 5 : 0, kw = t - kh * p.ksize;    // ksize is 1 or 3
                if ((unsigned)(iy0 + kh) < (unsigned)p.H && (unsigned)(ix0 + kw) < (unsigned)p.W) mask |= 1u << t;
            }
        }
        b_mask[j] = mask;
    }

    const int tpt = p.cin_chunks / BKC;     // stages per tap (Cin is a multiple of BKC chunks)
    auto issue_tile = [&](int kt, int stage) {
        unsigned char *base = smem + stage * TILE_BYTES + wave * 1024;
        const uint32_t ka = (uint32_t)kt * ROWB;
        if (has_a) {
#pragma unroll
            for (int j = 0; j < JA; ++j)
                dma16(rs_w, base + j * 8192, a_off[j] + ka);
        }
        const int tap = (int)fdiv((uint32_t)kt, p.dtpt);
        const uint32_t koff = (uint32_t)(kt - tap * tpt) * ROWB;
        const int kh = p.ksize == 3 ? (tap * 11) >> 5 : 0;
        const int kw = tap - kh * p.ksize;
        const uint32_t toff = (uint32_t)((kh * p.W + kw) * p.in_ld * 2) + koff;
#pragma unroll
        for (int j = 0; j < JB; ++j) {
            const bool ok = (b_mask[j] >> tap) & 1u;
            dma16(rs_in, base + NA * ROWB + j * 8192, ok ? b_base[j] + toff : YOLO_INVALID_OFF);
        }
    };

    const int fr = lane & 15, fq = lane >> 4;
    float4v acc[TM][TP];
    conv_init_acc_bias<TM, TP>(p, acc, n0 + wm * (TM * 16) + fq * CH);     // the accumulators start from the bias (conv_common.h)
    const int fswz = lds_swz<BKC>(fr);      // fragment rows are 16-aligned + fr
    auto compute = [&](int stage) {
        const unsigned char *A = smem + stage * TILE_BYTES + (wm * TM * 16 + fr) * ROWB;
        const unsigned char *B = smem + stage * TILE_BYTES + NA * ROWB + (wn * TP * 16 + fr) * ROWB;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int so = (((ks * 4 + fq) ^ fswz) & (BKC - 1)) << 4;
            uint4v fa[TM], fb[TP];
#pragma unroll
            for (int a = 0; a < TM; ++a) fa[a] = *reinterpret_cast<const uint4v *>(A + a * 16 * ROWB + so);
#pragma unroll
            for (int b = 0; b < TP; ++b) fb[b] = *reinterpret_cast<const uint4v *>(B + b * 16 * ROWB + so);
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TP; ++b) acc[a][b] = mma_chunk<T>(fa[a], fb[b], acc[a][b]);
        }
    };

    // ---- main loop: S-stage ring, counted vmcnt, raw barrier ------------------------------------
    const int KT = p.taps * tpt;
#ifdef YOLO_EXPERIMENT
    const unsigned long long t_setup = p.trace ? wall_clock64() : 0ull;
#endif
#pragma unroll
    for (int s = 0; s < S - 1; ++s)
        if (s < KT) issue_tile(s, s);
    int stage = 0;                  // stage holding tile kt
    int fill = S - 1;               // stage that tile kt+S-1 goes to (== the stage read at kt-1)
    for (int kt = 0; kt < KT; ++kt) {
        // tiles issued after tile kt that may stay in flight: min(S-2, KT-1-kt)
        const int after = KT - 1 - kt;
        if (has_a) {
            if (S >= 4 && after >= 2) wait_vmcnt<2 * NL>();
            else if (S >= 3 && after >= 1) wait_vmcnt<NL>();
            else wait_vmcnt<0>();
        } else {
            if (S >= 4 && after >= 2) wait_vmcnt<2 * JB>();
            else if (S >= 3 && after >= 1) wait_vmcnt<JB>();
            else wait_vmcnt<0>();
        }
        __builtin_amdgcn_sched_barrier(0);  // no ds_read / MFMA of the previous tile moves below the barrier (see conv_tap.hip)
        __builtin_amdgcn_s_barrier();       // tile kt visible to every wave; stage `fill` no longer read
#ifdef YOLO_EXPERIMENT      // ablation flags (tools/ablate.py: results intentionally wrong); not in the product build
        if (p.trace && kt == 0) t_first = wall_clock64();
        if (kt + S - 1 < KT && !(p.dbg & 1)) issue_tile(kt + S - 1, fill);
        if (!(p.dbg & 2)) compute(stage);
#else
        if (kt + S - 1 < KT) issue_tile(kt + S - 1, fill);
        compute(stage);
#endif
        stage = stage + 1 == S ? 0 : stage + 1;
        fill = fill + 1 == S ? 0 : fill + 1;
    }

#ifdef YOLO_EXPERIMENT
    if (p.dbg & 4) return;             // experiment: no epilogue
    const unsigned long long t_loop = p.trace ? wall_clock64() : 0ull;
#endif
    if constexpr (FUSE2) {
        static_assert(!FUSE2 || (WM == 2 && WN == 4 && TM == 4 && TP == 4 && 2 * LDS_BYTES <= 163840), "back-to-back 1x1: 128 x 256 tile, two per CU");
        conv_epilogue_fused_1x1<0, false>(p, acc, m0, wm, wn, wave, lane, smem);      // (the stride-2 conv into a stage: no residual)
    } else
    if constexpr (EPI == 2) {      // head conv: coalesced float32 rows via LDS
        static_assert(8 * 16 * kStagePitch(TM) * 4 + NB * kStageFlagAnchors * 4 <= S * TILE_BYTES, "staging slabs + row flags must fit in the ring");
        __syncthreads();            // every wave is done reading the ring
        conv_epilogue_f32_staged<TM, TP, 0, true, NB>(p, acc, n0 + wm * (TM * 16), m0 + wn * (TP * 16), lane,
                                         reinterpret_cast<float *>(smem) + wave * 16 * kStagePitch(TM),
                                         reinterpret_cast<float *>(smem) + 8 * 16 * kStagePitch(TM), wn * (TP * 16));
    } else if constexpr (EPI == 1) {    // (plain fp16 output map, aligned views below 2 GiB)
        conv_epilogue_fast<TM, TP, 0>(p, acc, n0 + wm * (TM * 16) + fq * CH, m0 + wn * (TP * 16), fr);
    } else {
        conv_epilogue<T, TM, TP, 0, true>(p, acc, n0 + wm * (TM * 16) + fq * CH, m0 + wn * (TP * 16), fr);
    }
#ifdef YOLO_EXPERIMENT
    if (p.trace && tid == 0) {          // YOLO_CONV_TRACE: phase timestamps (100 MHz) + placement of wave 0 of every block
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned long long *r = p.trace + (size_t)blockIdx.x * 8;
        r[0] = t_start; r[1] = t_setup; r[2] = t_loop; r[3] = wall_clock64();
        r[4] = __builtin_amdgcn_s_getreg(0xF804);      // HW_ID
        r[5] = __builtin_amdgcn_s_getreg(0xF814);      // XCC_ID
        r[6] = t_first;                                // first K tile landed (prologue DMA latency)
        r[7] = (unsigned long long)clock64() - c_start;
    }
#endif
}

// Pick the block tile that minimises rounds x tile time on 256 CUs (tail quantisation matters:
// e.g. 38x38x512 at batch 32 is 362 tiles of 256x256 = 2 rounds at 71 % but 722 of 256x128 = 3 at 94 %).
bool dma_cfg_valid(int cfg, int cout, int cin_chunks, bool v1_ok, int ksize, int stride, int W) {
    if (cfg < 0 || cfg >= kNumTiles) return false;
    const ConvTile &k = conv_tile(cfg);
    if (k.family == FAM_4WAVE) return v1_ok;
    if (cin_chunks % k.bkc) return false;
    if (k.is_tap() && (ksize != 3 || stride != (k.stride2() ? 2 : 1) || !conv_tap_fits(k, W))) return false;
    if (k.na() == 32) return cout <= 32 && cout > 16;
    if (k.na() == 64) return cout <= 64 && (!k.is_tap() || cout > 32);
    return k.na() <= (cout + 127) / 128 * 128 && cout > 64;
}

// Default tile per layer: a cost model calibrated on MI355X (profiles/r01_ablation.md).  A launch runs
// ceil(workgroups / resident slots) rounds; a round costs `a` microseconds per 64-deep K tile (MFMA +
// DMA of the tile) plus a fixed `f` (setup, prologue DMA latency, epilogue traffic; ~30 % less without a
// residual to read).  The constants reproduce the measured layer times of YOLOv3-608/416 and YOLOv2-416
// within ~10 %, e.g. 13x13x512->1024 at batch 16: 124 us predicted on 256x256 (123 measured, 44
// workgroups on 256 CUs) vs 71 us on 256x128,K64 (75 measured).  yolo_net_autotune replaces the model by
// on-device timing when asked.
// Two-per-CU tiles have three regimes: more workgroups than the 512 slots (back-filled rounds, `a_shared`), between
// 257 and 512 (one round, most CUs shared and in lockstep: `a_mid`), at most 256 (a workgroup has its CU alone): ConvTile.cost.
int choose_dma_cfg(int M, int cout, int cin_chunks, int taps, int has_res, bool v1_ok, int stride, int W, bool tap_only) {
    const int ksize = taps == 9 ? 3 : 1;
    auto valid = [&](int c) { return dma_cfg_valid(c, cout, cin_chunks, v1_ok, ksize, stride, W); };
#ifdef YOLO_EXPERIMENT      // tools/gpu_tile_sweep.sh: force one tile id on every layer that accepts it
    const char *force = getenv("YOLO_CONV_TILE");
    if (force && *force && valid(atoi(force)) && (!tap_only || conv_tile(atoi(force)).family != FAM_DMA))
        return atoi(force);
#endif
    const int fallback = v1_ok ? TILE_4WAVE : -1;
    if (cout <= 32 && M >= 8192 && valid(TILE_TAP2D_32x256)) return TILE_TAP2D_32x256;     // (tiny-YOLOv2 16 -> 32 at 208 x 208)
    if (cout <= 64) {   // narrow, bandwidth-bound layers: 3x3/1 with tap reuse (304x304 32->64: 239 us vs 273 on the 64x512 tile)
        if (M >= 8192 && valid(TILE_TAP2D_64x256)) return TILE_TAP2D_64x256;
        return !tap_only && valid(TILE_DMA_64x512) && M >= 8192 ? TILE_DMA_64x512 : fallback;
    }
    // wide maps with a short K (152x152 64 -> 128 at batch 32, round 3, after the bias moved into the accumulators and the 2-D
    // tile lost its 36 spilled registers: 155 us on the 128 x 256 2-D tap tile, 161 on the 128 x 128 2-D tile at three
    // workgroups per CU, 175 on the padded-linear 128 x 128 tile, 181 on the per-tap LDS-DMA tile the model picks)
    if (!tap_only && taps == 9 && stride == 1 && W > 110 && cout <= 128 && cin_chunks <= 8 && M >= 262144 && valid(TILE_TAP2D_128x256))
        return TILE_TAP2D_128x256;
    // ... and at a quarter of that batch the 8 x 16 tile at three workgroups per CU (152x152 64->128 at batch 8: 40 us vs 47.5 on
    // the per-tap LDS-DMA tile the model picks; at batch 32 it is the slower of the two 2-D tiles, 161 vs 155)
    if (!tap_only && taps == 9 && stride == 1 && W > 110 && cout <= 128 && cin_chunks <= 8 && M >= 65536 && M < 262144 && valid(TILE_TAP2D_128x128_X3))
        return TILE_TAP2D_128x128_X3;
    // float32, MFMA-bound (fp32 matrix peak is 1/16 of fp16's): long K on a 13x13 map over more than one round of workgroups.  There
    // the padded-linear grid's (14/13)^2 = 16 % of computed-and-dropped positions are the whole difference: tiny-YOLOv2 b64
    // 1024->1024 2.09 ms on the tap tile (97 TFLOP/s) vs 1.81 ms on the 4-wave kernel (113 TFLOP/s = 72 % of the fp32 MFMA peak),
    // 512->1024 1.06 vs 0.91 ms; 256->512 (one round, K 2304) and every 26x26 / 52x52 layer stay faster on the tap tile.
    if (tap_only && v1_ok && taps == 9 && stride == 1 && W <= 14 && taps * cin_chunks * 4 >= 4608 &&
        ((long long)M * (W + 1) * (W + 1) / ((long long)W * W) + 127) / 128 * ((cout + 127) / 128) > 512)
        return TILE_4WAVE;
    // (tile 23, the parity-plane tap tile with the back-to-back 1x1 for the stride-2 conv 64 -> 128 into a wide stage, is NOT chosen by
    // rule: at 304 -> 152, batch 32, it measures 211 us against 208 for LDS-DMA tile 6 with the same fusion -- two channel slices are
    // too short a K loop for tap reuse to matter, the launch is the 660 MB it moves)
    const double k64 = taps * cin_chunks / 8.0;         // 64-deep K tiles
    int best = fallback;
    double best_t = 1e300;
    for (int c = 0; c < kNumTiles; ++c) {
        const ConvTile &k = conv_tile(c);
        // float32 nets: only conv_tap.hip has a float32 instantiation, and it beats the 4-wave kernel by ~10 % on every 3x3/1
        // layer measured (tiny-YOLOv2 b64: 1024->1024 at 13x13 2.26 -> 2.06 ms), so the 4-wave kernel is only the fallback
        if (tap_only && !k.f32_ok()) continue;
        if (c == TILE_TAP2D_128x256 && W <= 110) continue;      // the padded-linear tiles fit and measured faster (104x104: 70 vs 84 us)
        // the three-per-CU tile: 1x1 layers; measured 10-20 % slower than the larger tiles on every 3x3 layer that fills the chip, but
        // the best tile for a stride-2 layer of 129-256 workgroups (19x19 512->1024 at batch 8: 57 us vs 72 on the 4-wave kernel)
        // (with <= 128 workgroups the 4-wave kernel's split-K wins: 25 vs 49 us at batch 1)
        const long long wg128 = (long long)((M + 127) / 128) * ((cout + 127) / 128);
        if (c == TILE_DMA_128x128_X3 && taps != 1 && !(stride == 2 && wg128 > 128 && wg128 <= 256)) continue;
        if (c == TILE_DMA_128x192_S4 && taps != 1) continue;     // (measured on 1x1 layers only)
        if (k.has(CAP_RULE_ONLY) || !valid(c)) continue;
        const int na = k.na(), nb = k.nb();
        // tap-reuse tiles walk the padded position grid: (H+1)(W+1) positions per image (square maps assumed here)
        long long Meff = M;
        const int Wq = k.stride2() ? W / 2 : W;      // width of the map the tap tiles walk
        if (k.stride2()) {
            if (cin_chunks <= 8) continue;      // (Cin <= 64, two slices: the LDS-DMA tile that also computes the 1x1 behind it is the better launch)
            Meff = (long long)M * (Wq + 1) * (Wq + 1) / ((long long)Wq * Wq);
        } else if (k.is_tap()) {
            if (k.is2d()) { const long long th = nb / 16, tx = (W + 15) / 16, ty = (W + th - 1) / th; Meff = (long long)M * tx * ty * nb / ((long long)W * W); }
            else Meff = (long long)M * (W + 1) * (W + 1) / ((long long)W * W);
        }
        long long blocks = (Meff + nb - 1) / nb * ((cout + na - 1) / na);
        if (k.image_aligned()) blocks = (long long)(M / (Wq * Wq)) * ((cout + na - 1) / na);    // a tile per image
        // (a stride-2 launch of a handful of tiles belongs to the 4-wave kernel, which splits K: 38 -> 19 at batch 1 25 us there, 58 us here)
        if (k.stride2() && blocks <= 128) continue;
        const long long slots = 256LL * k.per_cu();     // resident workgroups on the chip
        // one workgroup per CU: whole rounds; two per CU: the dispatcher back-fills, the tail costs ~half a round
        double rounds, a;
        if (k.per_cu() == 1) {
            rounds = (double)((blocks + slots - 1) / slots);
            a = k.cost.a_shared;
        } else if (blocks > slots) {
            rounds = (double)blocks / slots + 0.5;
            a = k.cost.a_shared;
        } else {
            rounds = 1.0;
            a = blocks <= 256 ? k.cost.a_alone : k.cost.a_mid;
        }
        const double t = rounds * (k64 * a + k.cost.f * (has_res ? 1.0 : 0.7));
        if (t < best_t) { best_t = t; best = c; }
    }
    return best;
}

// Which instantiation of conv_igemm_dma_kernel a launch runs (see its EPI): launch_dma_tile launches it, conv_tile_symbol names it
static ConvForm dma_form(const ConvTile &t, const ConvParams &p) {
    if (t.family != FAM_DMA) return FORM_INVALID;
    if (p.fuse2) return t.has(CAP_FUSE2) && conv_fast_epilogue_ok(p) ? FORM_FUSED : FORM_INVALID;
    if (p.out_f32 && !p.vec_out && p.outmode == OUT_NORMAL && !p.has_res) return FORM_HEAD_F32;
    static const bool no_fast_epi = getenv("YOLO_NO_FAST_EPI") != nullptr;        // A/B switch, read once (same results either way)
    return !no_fast_epi && conv_fast_epilogue_ok(p) ? FORM_LEAN : FORM_GENERIC;
}
static constexpr int dma_epi(ConvForm f) { return f == FORM_HEAD_F32 ? 2 : f == FORM_LEAN ? 1 : 0; }       // the template argument EPI of a form

template <int ID, ConvForm F>
static hipError_t launch_dma_inst(const ConvParams &p, hipStream_t s) {
    constexpr ConvTile t = kTiles[ID];
    hipLaunchKernelGGL((conv_igemm_dma_kernel<t.wm, t.wn, t.tm, t.tp, t.s, t.bkc, t.occ, F == FORM_FUSED, dma_epi(F)>), dim3((unsigned)p.n_blocks), dim3(512), 0, s, p);
    return hipGetLastError();
}
template <int ID>
static hipError_t launch_dma_tile_id(ConvForm f, const ConvParams &p, hipStream_t s) {
    constexpr ConvTile t = kTiles[ID];
    if constexpr (t.family == FAM_DMA) {
        switch (f) {
        case FORM_GENERIC: return launch_dma_inst<ID, FORM_GENERIC>(p, s);
        case FORM_LEAN: return launch_dma_inst<ID, FORM_LEAN>(p, s);
        case FORM_HEAD_F32: return launch_dma_inst<ID, FORM_HEAD_F32>(p, s);
        case FORM_FUSED: if constexpr (t.has(CAP_FUSE2)) return launch_dma_inst<ID, FORM_FUSED>(p, s); break;
        default: break;
        }
    }
    return hipErrorInvalidValue;
}
template <int... ID>
static hipError_t launch_dma_by_id(int id, ConvForm f, const ConvParams &p, hipStream_t s, std::integer_sequence<int, ID...>) {
    hipError_t e = hipErrorInvalidValue;
    (void)((id == ID && ((e = launch_dma_tile_id<ID>(f, p, s)), true)) || ...);
    return e;
}

static hipError_t launch_dma_tile(const ConvParams &p, int cfg, hipStream_t s) {
    const ConvForm f = dma_form(conv_tile(cfg), p);
    // back-to-back 1x1: the 128 x 256 K32 tile
    if (f == FORM_FUSED && (p.has_res || p.n_tiles_n != 1 || p.Cout != 128 || !p.w2 || !p.b2 || !p.out2 || !p.out2_bytes)) return hipErrorInvalidValue;
    return launch_dma_by_id(cfg, f, p, s, std::make_integer_sequence<int, kNumTiles>());
}

static int tap_stream_wanted() {      // ConvParams.stream of a tap launch: the persistent form where it exists and applies (conv_tap.hip: tap_stream_ok)
#ifdef YOLO_EXPERIMENT
    if (getenv("YOLO_NO_TAP_STREAM")) return 0;
#endif
    return 1;
}

#ifdef YOLO_EXPERIMENT
// experiment: YOLO_CONV_TRACE=<file> appends, for every LDS-DMA / tap-reuse launch, a header {blocks, M, Cout, cin_chunks, H, W, cfg,
// ksize * 10 + stride} and 8 uint64 per block (see the kernels); synchronous, for tools/trace_blocks.py only
static hipError_t launch_traced(ConvParams p, int cfg, hipStream_t s) {
    const char *tf = getenv("YOLO_CONV_TRACE");
    unsigned long long *dev = nullptr;
    const size_t bytes = (size_t)p.n_blocks * 64;
    if (hipMalloc((void **)&dev, bytes) != hipSuccess) return hipErrorOutOfMemory;
    (void)hipMemset(dev, 0, bytes);
    p.trace = dev;
    hipError_t e = conv_tile(cfg).is_tap() ? launch_conv_tap(p, cfg, s) : launch_dma_tile(p, cfg, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    std::vector<unsigned long long> host((size_t)p.n_blocks * 8);
    if (e == hipSuccess) e = hipMemcpy(host.data(), dev, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    if (e == hipSuccess) {
        if (FILE *fp = fopen(tf, "ab")) {
            const unsigned long long hdr[8] = {(unsigned long long)p.n_blocks, (unsigned long long)p.M, (unsigned long long)p.Cout,
                                               (unsigned long long)p.cin_chunks, (unsigned long long)p.H, (unsigned long long)p.W,
                                               (unsigned long long)cfg, (unsigned long long)(p.ksize * 10 + p.stride)};
            fwrite(hdr, 8, 8, fp);
            fwrite(host.data(), 8, host.size(), fp);
            fclose(fp);
        }
    }
    return e;
}
#endif

hipError_t launch_conv_dma(const ConvParams &p0, int cfg, hipStream_t s) {
    if (cfg <= 0 || cfg >= kNumTiles) return hipErrorInvalidValue;
    ConvParams p = p0;
    const ConvTile &k = conv_tile(cfg);
    const int na = k.na(), nb = k.nb();
#ifdef YOLO_EXPERIMENT
    { const char *d = getenv("YOLO_CONV_DBG"); p.dbg = d ? atoi(d) : 0; }
#endif
    p.n_tiles_n = (p.Cout + na - 1) / na;
    const long long blocks = ((long long)p.M + nb - 1) / nb * p.n_tiles_n;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    p.n_blocks = (int)blocks;
    conv_set_divisors(p, p.cin_chunks / k.bkc);
    if (k.is_tap()) {          // padded-linear position grid: one shared pad column per row, one pad row per image
        long long mq;
        if (k.is2d()) {     // TH x 16 tiles (TH = positions per block / 16): qW = tiles per tile row, qHW = tiles per image
            const int th = nb / 16;
            p.t2_shift = th == 16 ? 8 : 7;
            if (th != 16 && th != 8) return hipErrorInvalidValue;
            p.qW = (p.W + 15) / 16;
            p.qHW = p.qW * ((p.H + th - 1) / th);
            mq = (long long)(p.M / p.HoWo) * p.qHW * nb;
        } else {
            p.qW = p.Wo + 1;          // (stride 1: Ho = H, Wo = W; the stride-2 tiles walk the OUTPUT map)
            p.qHW = (p.Ho + 1) * (p.Wo + 1);
            mq = (long long)(p.M / p.HoWo) * p.qHW;
        }
        const bool img = k.image_aligned();
        p.q_stride = img ? p.qHW : nb;
        const long long qblocks = img ? (long long)(p.M / p.HoWo) * p.n_tiles_n : (mq + nb - 1) / nb * p.n_tiles_n;
        if (qblocks <= 0 || qblocks > 0x7fffffffLL) return hipErrorInvalidValue;
        p.Mq = (int)mq;
        p.n_blocks = (int)qblocks;
        conv_set_divisors(p, p.cin_chunks / k.bkc);
#ifdef YOLO_EXPERIMENT
        if (getenv("YOLO_CONV_TRACE")) return launch_traced(p, cfg, s);
#endif
        p.stream = tap_stream_wanted();
        return launch_conv_tap(p, cfg, s);
    }
#ifdef YOLO_EXPERIMENT
    if (getenv("YOLO_CONV_TRACE")) return launch_traced(p, cfg, s);
#endif
    return launch_dma_tile(p, cfg, s);
}

// the name rocprofv3's kernel trace prints for the kernel that runs THIS launch of a tile (yolo_kernel_info.symbol: joins bench.py's
// roofline to profiles/*.csv); p as launched: ksplit, pair, fuse2 set
std::string conv_tile_symbol(int cfg, ConvParams p) {
    const ConvTile &t = conv_tile(cfg);
    if (t.is_tap()) {
        p.stream = tap_stream_wanted();
        return conv_tap_symbol(t, p);
    }
    const ConvForm f = dma_form(t, p);
    if (f == FORM_INVALID) return "";
    char b[160];
    snprintf(b, sizeof b, "void yolo::conv_igemm_dma_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %d>(yolo::ConvParams)", t.wm, t.wn, t.tm, t.tp, t.s, t.bkc, t.occ,
             f == FORM_FUSED ? "true" : "false", dma_epi(f));
    return b;
}

}  // namespace yolo

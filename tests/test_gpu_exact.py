"""GPU: every conv kernel bit for bit on integer data (tests/exact_ref.py).

Inputs, folded kernels and biases are small integers, so every product and every partial sum -- in ANY order -- is exact in the fp32
accumulator: the output no longer depends on tile, K order, split-K, pair-K, stream count or fusion, and must EQUAL the plain integer
reference, the single fp16 rounding of the store included (odd integers in (2048, 4096) are exact fp16 ties).  Every comparison is
np.array_equal; exact_ref.check_preconditions is asserted for a case before anything touches the GPU (and for the whole table, without
a GPU, by test_exact_cpu.py).  Each case also asserts that the kernel meant is the one that ran, and prints the kernel names, the
count of fp16 ties and of values on leaky's negative branch (both counted on the reference).

Which kernel is meant: every single-conv probe names its conv kernel in full (tile, split-K form and split count: ",1launch" = the
ticketed split inside the launch, "+splitK<n>" alone = splitk_reduce_kernel, "+pairK" = the in-launch pair), per variant, in
tests/golden/exact_kernels.json -- the plan of the case as recorded from yolo_net_kernel_info (`python tests/test_gpu_exact.py` rewrites it
after a deliberate change of the tile rules; planning needs no GPU).  A forced tile that is valid for a layer must run it; where the
recorded plan shows the forced tile is NOT valid for a shape the case is left out (the default kernel of that shape runs in the
"-tdef" cases), except ONE case per tile and dtype, kept to show the fall-back: it asserts that the default runs and still requires equality.

CASES is the table; it is built without a GPU so that test_exact_cpu.py can loop over it.
"""
import functools
import json
import os
import zlib

import numpy as np
import pytest

from helpers import GOLDEN, new_graph, run_hip, to_oracle
import exact_ref as X
from tensorflow_yolo_amd.net import layers as PL

pytestmark = pytest.mark.gpu

# conv_dma.hip kCfgs: tile id -> what yolo_kernel_info.name says when that tile runs (0 = the 4-wave kernel of conv.hip)
TILE_NAME = {0: "conv_igemm<", 1: ",256x256,K64,S2>", 2: ",256x128,K64,S3>", 3: ",128x256,K64,S3>", 4: ",256x256,K32,S4>", 5: ",256x128,K32,S3,x2>",
             6: ",128x256,K32,S3,x2>", 7: ",64x512,K32,S2,x2>", 8: ",128x256,tap9,x2>", 9: ",256x256,tap9>", 10: ",128x192,tap9,x2>", 11: ",128x128,tap9,x2>",
             12: ",128x256,tap9,2d,x2>", 13: ",64x256,tap9,2d,x2>", 14: ",128x128,K32,S3,x3>", 15: ",256x224,tap9>", 16: ",128x128,tap9,2d,x3>",
             17: ",32x256,tap9,2d,x2>", 18: ",128x384,tap9,img>", 19: ",128x192,K64,S4>", 20: ",128x256,tap9,s2,x2>", 21: ",128x384,tap9,s2,img>",
             22: ",128x192,tap9,img,x2>", 23: ",128x256,tap9,s2,wide,x2>"}
F32_TILES = (0, 11, 13, 17)           # the tiles with a float32 instantiation


# ---- graphs -------------------------------------------------------------------------------------------------------------------
def _conv(g, src, f, k, s=1, bn=True, act="leaky"):
    g.append(PL.conv2d_bn_act(src.out, f, k, s, use_batch_normalization=bn, activation_fn=act))


def g_probe(H, W, cin, cout, k, s, bn, act, variant):
    """ONE conv on the graph input: "f32" = read as the final float32 output; "pool" = read as an fp16 store through a trailing stride-1
    max-pool; "res" = the same with the graph input as fused residual (Cin = Cout, stride 1); "pool2" = 2x2/2 pool behind it;
    "res_last" = the fused residual as the graph's LAST layer (written as float32, unrounded: DESIGN.md section 4)"""
    g = new_graph(H, W, cout if variant in ("res", "res_last") else cin)
    _conv(g, g[-1], cout, k, s, bn, act)
    if variant in ("res", "res_last"):
        g.append(PL.shortcut(g[-1].out, g[0].out))
    if variant in ("pool", "res"):
        g.append(PL.max_pool2d(g[-1].out, 2, stride=1))
    if variant == "pool2":
        g.append(PL.max_pool2d(g[-1].out, 2, stride=2))
        g.append(PL.max_pool2d(g[-1].out, 2, stride=1))
    return g


def g_mx(H, W, cin, cout, residual, concat, linear):
    g = new_graph(H, W, cin)
    _conv(g, g[-1], cout, 3, 1, not linear, None if linear else "leaky")
    if residual:
        g.append(PL.shortcut(g[-1].out, g[0].out))
    if concat:
        _conv(g, g[0], 128, 1)
        g.append(PL.route([g[1].out, g[-1].out]))
    g.append(PL.max_pool2d(g[-1].out, 2, stride=1))
    return g


def g_stem(H, W, third):
    g = new_graph(H, W, 3)
    _conv(g, g[-1], 32, 3)
    _conv(g, g[-1], 64, 3, 2)
    if third == 32:         # Darknet-53: 1x1 64 -> 32, 3x3 32 -> 64, shortcut
        _conv(g, g[-1], 32, 1)
        _conv(g, g[-1], 64, 3)
        g.append(PL.shortcut(g[-1].out, g[-3].out))
    else:
        _conv(g, g[-1], 64, 1)
    g.append(PL.max_pool2d(g[-1].out, 2, stride=1))
    return g


def g_first_pool(H, W, cout, tail):
    g = new_graph(H, W, 3)
    _conv(g, g[-1], cout, 3)
    g.append(PL.max_pool2d(g[-1].out, 2, stride=2))
    _conv(g, g[-1], tail, 3)
    g.append(PL.max_pool2d(g[-1].out, 2, stride=1))
    return g


def g_pool2d(H, W, cin, couts):
    """conv 3x3 + 2x2/2 pool pairs (the pool is fused into the 2-D tap tile), then a 1x1"""
    g = new_graph(H, W, cin)
    for c in couts:
        _conv(g, g[-1], c, 3)
        g.append(PL.max_pool2d(g[-1].out, 2, stride=2))
    _conv(g, g[-1], 32, 1)
    return g


def g_fuse2(case):
    if case.startswith("stride2"):
        g = new_graph(44, 58, 64)
        _conv(g, g[-1], 128, 3, 2)
        _conv(g, g[-1], 64, 1)
        _conv(g, g[-1], 128, 3)
        g.append(PL.shortcut(g[-1].out, g[1].out))
    else:
        g = new_graph(37, 50, 32)
        _conv(g, g[-1], 128, 3)
        _conv(g, g[-1], 64, 1)
        _conv(g, g[-1], 128, 3)
        g.append(PL.shortcut(g[-1].out, g[1].out))
        _conv(g, g[-1], 64, 1)
        _conv(g, g[-1], 128, 3)
        g.append(PL.shortcut(g[-1].out, g[4].out))
    g.append(PL.max_pool2d(g[-1].out, 2, stride=1))         # read the last shortcut as an fp16 store (the "shortcut-last" cases read it as the output)
    return g


def g_upsample():
    g = new_graph(8, 8, 64)
    _conv(g, g[-1], 64, 3)
    _conv(g, g[-1], 128, 3, 2)
    _conv(g, g[-1], 64, 1)
    g.append(PL.upsample(g[-1].out, 2))
    g.append(PL.route([g[-1].out, g[1].out]))
    _conv(g, g[-1], 32, 1)
    return g


def g_reorg():
    g = new_graph(8, 8, 64)
    _conv(g, g[-1], 64, 3)
    g.append(PL.max_pool2d(g[-1].out, 2, 2))
    _conv(g, g[-1], 128, 3)
    g.append(PL.route([g[1].out]))
    _conv(g, g[-1], 16, 1)
    g.append(PL.reorg(g[-1].out, 2))
    g.append(PL.route([g[-1].out, g[3].out]))
    _conv(g, g[-1], 64, 3)
    return g


def g_fallback(H=8, W=8, cin=16):
    g = new_graph(H, W, cin)
    _conv(g, g[-1], 32, 3)
    g.append(PL.max_pool2d(g[-1].out, 2, 1))
    g.append(PL.shortcut(g[1].out, g[2].out))
    g.append(PL.max_pool2d(g[-1].out, 2, 2))
    g.append(PL.upsample(g[-1].out, 2))
    g.append(PL.reorg(g[3].out, 2))
    g.append(PL.route([g[4].out, g[6].out]))
    g.append(PL.route([g[7].out, g[4].out]))
    _conv(g, g[-1], 32, 1)
    g.append(PL.route([g[5].out, g[3].out]))
    return g


def g_maxpool_odd():
    g = new_graph(7, 9, 3)
    _conv(g, g[-1], 32, 3)
    g.append(PL.max_pool2d(g[-1].out, 2, 2))
    g.append(PL.max_pool2d(g[-1].out, 2, 1))
    g.append(PL.max_pool2d(g[-1].out, 2, 2))
    return g


def g_residual_blocks():
    g = new_graph(16, 16, 3)
    _conv(g, g[-1], 32, 3)
    _conv(g, g[-1], 64, 3, 2)
    for _ in range(2):
        _conv(g, g[-1], 32, 1)
        _conv(g, g[-1], 64, 3)
        g.append(PL.shortcut(g[-1].out, g[-3].out))
    _conv(g, g[-1], 18, 1, 1, False, "linear")
    return g


GRAPHS = {f.__name__: f for f in (g_probe, g_mx, g_stem, g_first_pool, g_pool2d, g_fuse2, g_upsample, g_reorg, g_fallback, g_maxpool_odd,
                                  g_residual_blocks)}


# ---- the case table -----------------------------------------------------------------------------------------------------------
CASES = []


def case(id, graph, B, dtype, tile=None, kw=None, expect=(), absent=(), ties=False, neg=True, keep_all=False, repeat=False, data=None,
         variants=None):
    """graph: (builder name, args); for g_probe the last argument is filled from `variants`, which one test runs in turn.
    expect / absent: substrings of the kernel names + symbols + plan description that must / must not appear.
    ties / neg: the reference must show fp16 ties in front of a rounding / values on leaky's negative branch (in some variant)."""
    CASES.append(dict(id=id, graph=graph, B=B, dtype=dtype, tile=tile, kw=kw or {}, expect=tuple(expect), absent=tuple(absent), ties=ties,
                      neg=neg, keep_all=keep_all, repeat=repeat, data=data or {}, variants=variants or (None,)))


def probe_cases(fam, name, shape, k, s, dtype, tile=None, bn=True, act="leaky", **kw):
    B, H, W, cin, cout = shape
    variants = ["f32", "pool"] + (["res"] if s == 1 else [])
    case("%s-%s-%s-t%s" % (fam, name, dtype, "def" if tile is None else tile), ("g_probe", (H, W, cin, cout, k, s, bn, act)), B, dtype, tile=tile,
         ties=dtype == "fp16", neg=act == "leaky", variants=tuple(variants), **kw)


def _shape_name(sh):
    return "x".join(str(v) for v in sh)


TAP_SHAPES = [(2, 19, 19, 512, 256), (2, 20, 21, 128, 256), (5, 13, 13, 128, 256), (3, 38, 38, 64, 128), (1, 76, 76, 128, 256), (2, 7, 78, 32, 128),
              (2, 5, 110, 64, 128), (1, 9, 152, 64, 128), (2, 33, 100, 32, 64), (1, 48, 304, 32, 64), (2, 21, 70, 32, 32)]
for _sh in TAP_SHAPES:
    for _t in (8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 22):
        probe_cases("tap", _shape_name(_sh), _sh, 3, 1, "fp16", _t)
        if _t in F32_TILES:
            probe_cases("tap", _shape_name(_sh), _sh, 3, 1, "fp32", _t)

S2_SHAPES = [(3, 38, 38, 256, 512), (2, 76, 76, 128, 256), (1, 152, 152, 128, 256), (2, 22, 150, 64, 128), (5, 12, 20, 32, 128), (2, 36, 36, 192, 384),
             (1, 34, 34, 128, 320)]
for _sh in S2_SHAPES:
    for _t in (20, 21, 23):
        probe_cases("s2", _shape_name(_sh), _sh, 3, 2, "fp16", _t)

CONV_CASES = {     # test_gpu_ops.CONV_CASES: name: (B, H, W, Cin, Cout, k, s, bn, act)
    "first_3to32": (2, 17, 19, 3, 32, 3, 1, True, "leaky"),
    "first_3to16_tiny": (2, 16, 16, 3, 16, 3, 1, True, "leaky"),
    "c16to32": (2, 12, 12, 16, 32, 3, 1, True, "leaky"),
    "c32to64_s2_odd": (2, 15, 13, 32, 64, 3, 2, True, "leaky"),
    "c32to64_s1": (1, 20, 20, 32, 64, 3, 1, True, "leaky"),
    "c64to128": (2, 9, 11, 64, 128, 3, 1, True, "leaky"),
    "c128to64_1x1": (2, 9, 11, 128, 64, 1, 1, True, "leaky"),
    "c64to32_1x1": (2, 10, 10, 64, 32, 1, 1, True, "leaky"),
    "c128to256_s2": (2, 10, 10, 128, 256, 3, 2, True, "leaky"),
    "c256to512_linear_bias": (1, 7, 7, 256, 512, 3, 1, False, "linear"),
    "c768_1x1": (1, 6, 6, 768, 256, 1, 1, True, "leaky"),
    "c384_1x1": (1, 6, 6, 384, 128, 1, 1, True, "leaky"),
    "m_tail_3069": (3, 33, 31, 64, 64, 3, 1, True, "leaky"),
    "k_long_1280": (1, 13, 13, 1280, 256, 3, 1, True, "leaky"),
}
for _n, (_B, _H, _W, _ci, _co, _k, _s, _bn, _act) in sorted(CONV_CASES.items()):
    _first = _ci == 3
    for _dt in ("fp16", "fp32"):
        if _first:      # first.hip takes the 3-channel conv that is not the graph's float32 output
            case("conv-%s-%s" % (_n, _dt), ("g_probe", (_H, _W, _ci, _co, _k, _s, _bn, _act)), _B, _dt, expect=("conv_first<",), ties=_dt == "fp16", variants=("pool",))
        else:
            probe_cases("conv", _n, (_B, _H, _W, _ci, _co), _k, _s, _dt, None, bn=_bn, act=_act)
    if not _first:
        for _t in (0, 1, 2, 3, 4, 5, 6, 7, 14, 19):
            probe_cases("dma", _n, (_B, _H, _W, _ci, _co), _k, _s, "fp16", _t, bn=_bn, act=_act)
        probe_cases("dma", _n, (_B, _H, _W, _ci, _co), _k, _s, "fp32", 0, bn=_bn, act=_act)


def _random_rule_shapes(dtype):
    """the ten seeded first-conv shapes of test_gpu_ops.test_random_layer_shapes_through_the_default_rules (same draws)"""
    rng = np.random.RandomState(1234 if dtype == "fp16" else 4321)
    widths = [13, 14, 19, 26, 38, 52, 76, 96, 104, 112, 152]
    chans = [32, 64, 128, 256] if dtype == "fp16" else [16, 32, 64, 128]
    out = []
    for _ in range(10):
        W = int(widths[rng.randint(len(widths))])
        H = int(rng.randint(6, 20)) if W > 60 else W
        B = int(rng.randint(1, 7))
        cin = int(chans[rng.randint(len(chans))])
        c1 = int(chans[rng.randint(len(chans))])
        if H % 2 == 0 and W % 2 == 0:
            rng.randint(2)
        out.append((B, H, W, cin, c1))
    return out


for _dt in ("fp16", "fp32"):
    for _i, _sh in enumerate(_random_rule_shapes(_dt)):
        probe_cases("rules", "%d-%s" % (_i, _shape_name(_sh)), _sh, 3, 1, _dt, None, expect=("conv_igemm",))

# in-launch pair split-K (the four shapes of test_in_launch_pair_split_k): the pair kernel must be what runs, three launches the same bits
for _dt, _sh in [("fp16", (24, 13, 13, 256, 512)), ("fp16", (20, 19, 19, 512, 256)), ("fp32", (24, 13, 13, 128, 512)), ("fp32", (24, 19, 19, 128, 256))]:
    case("pairk-%s-%s" % (_shape_name(_sh), _dt), ("g_probe", _sh[1:] + (3, 1, True, "leaky")), _sh[0], _dt, expect=("+pairK",), ties=_dt == "fp16",
         repeat=True, variants=("pool", "res"))

# split K on small maps at batch 1-2: the ticketed multi-split inside the launch (",1launch") and splitk_reduce_kernel ("+splitK<n>" alone); which
# form a variant runs is part of its recorded kernel name (variants the plan does not split are left out: select_cases)
SPLITK = [("13-64to512", (13, 13, 64, 512, 3, 1)), ("13-512to1024", (13, 13, 512, 1024, 3, 1)), ("13-1024to512-1x1", (13, 13, 1024, 512, 1, 1)),
          ("13-1024to320-s2", (13, 13, 1024, 320, 3, 2)), ("7x9-256to1024", (7, 9, 256, 1024, 3, 1)), ("7x9-1024to255-1x1", (7, 9, 1024, 255, 1, 1))]
for _n, (_H, _W, _ci, _co, _k, _s) in SPLITK:
    for _dt in ("fp16", "fp32"):
        for _B in (1, 2):
            case("splitk-%s-b%d-%s" % (_n, _B, _dt), ("g_probe", (_H, _W, _ci, _co, _k, _s, True, "leaky")), _B, _dt, ties=_dt == "fp16", repeat=True,
                 variants=("f32", "pool") + (("res",) if _s == 1 else ()))

# float32 products as nine bf16 products: integers up to 256 are ONE bf16 term, so the emulation is exact too
for _mode, _exp, _abs in [(0, ("conv_igemm_emu",), ()), (1, (), ("conv_igemm_emu",)), (2, ("conv_igemm_emu",), ())]:
    case("emu-13-512to1024-mode%d" % _mode, ("g_probe", (13, 13, 512, 1024, 3, 1, True, "leaky")), 26, "fp32", tile=0, kw={"f32_products": _mode}, expect=_exp,
         absent=_abs, variants=("pool", "res"))
    if _mode:       # K = 2304: below the library's rule, the emulation runs only where mode 2 asks for it
        case("emu-13-256to1024-mode%d" % _mode, ("g_probe", (13, 13, 256, 1024, 3, 1, True, "leaky")), 26, "fp32", tile=0, kw={"f32_products": _mode},
             expect=_exp, absent=_abs, variants=("pool",))

# the MX kernel: |x|, |w| <= 14 are exact in e4m3fn at every block scale
MX_DATA = {"xmax": X.MX_MAX, "wmax": X.MX_MAX}
for _ci, _co, _H, _W, _B in [(128, 256, 17, 23, 2), (256, 128, 9, 11, 3), (512, 256, 13, 13, 1), (1024, 192, 7, 5, 2), (128, 128, 76, 76, 1), (256, 128, 3, 100, 2),
                             (128, 128, 5, 100, 4)]:
    case("mx-%dto%d-%dx%d-b%d" % (_ci, _co, _H, _W, _B), ("g_mx", (_H, _W, _ci, _co, False, False, False)), _B, "mxfp8", expect=("conv_mx",), ties=True, data=MX_DATA)
for _n in ("residual", "concat", "linear", "forced"):
    case("mx-epilogue-%s" % _n, ("g_mx", (19, 21, 256, 256, _n == "residual", _n == "concat", _n == "linear")), 2, "mxfp8", tile=24 if _n == "forced" else None,
         expect=("conv_mx",), ties=True, neg=_n != "linear", data=MX_DATA)

# input layers: first.hip (MFMA and VALU variants, with and without the fused pool) and stem.hip -- chains: hidden layers non-negative
for _sh in [(3, 40, 56), (2, 64, 64), (1, 18, 34), (2, 21, 30)]:
    _even = _sh[1] % 2 == 0 and _sh[2] % 2 == 0
    case("stem-3-32-64-32-%s" % _shape_name(_sh), ("g_stem", (_sh[1], _sh[2], 32)), _sh[0], "fp16", expect=("conv_stem<f16,3-32-64-32>",) if _even else (),
         absent=() if _even else ("conv_stem",), ties=True)
    case("stem-3-32-64-%s" % _shape_name(_sh), ("g_stem", (_sh[1], _sh[2], 64)), _sh[0], "fp16", expect=("conv_stem<f16,3-32-64>",) if _even else (),
         absent=("3-32-64-32",) if _even else ("conv_stem",), ties=True)
    case("stem-fp32-%s" % _shape_name(_sh), ("g_stem", (_sh[1], _sh[2], 32)), _sh[0], "fp32", absent=("conv_stem",))
for _hw in [(20, 44), (32, 64), (6, 130)]:
    for _co in (32, 16):
        case("firstpool-%dx%d-%d-fp16" % (_hw + (_co,)), ("g_first_pool", _hw + (_co, 64)), 3, "fp16", ties=True,
             expect=("conv_first_pool", "yolo::first_pool_mfma_kernel(" if _co == 32 else "conv_first_kernel<false, 16, true>"))
        case("firstpool-%dx%d-%d-fp32" % (_hw + (_co,)), ("g_first_pool", _hw + (_co, 64)), 3, "fp32",
             expect=("conv_first_pool", "first_pool_mfma_f32_kernel<%d>(" % (_co // 16)))
for (_B, _H, _W), _co in [((2, 32, 40), 32), ((1, 18, 300), 16), ((3, 6, 130), 32), ((2, 9, 20), 16)]:
    for _dt in ("fp16", "fp32"):
        _even = _H % 2 == 0 and _W % 2 == 0
        case("firstpool128-%s-%d-%s" % (_shape_name((_B, _H, _W)), _co, _dt), ("g_first_pool", (_H, _W, _co, 32)), _B, _dt, ties=_dt == "fp16",
             expect=("conv_first_pool",) if _even else ("conv_first<",), absent=() if _even else ("conv_first_pool",))
# ... and the first layer + pool with SIGNED kernels, read through the pool alone (rounding and the negative branch inside the pooled epilogue)
for _co in (32, 16):
    for _dt in ("fp16", "fp32"):
        case("firstpool-signed-%d-%s" % (_co, _dt), ("g_probe", (20, 44, 3, _co, 3, 1, True, "leaky")), 3, _dt, expect=("conv_first_pool",), ties=_dt == "fp16",
             variants=("pool2",))

# fused epilogues
for _dt in ("fp16", "fp32"):
    case("pool2d-64-128-%s" % _dt, ("g_pool2d", (12, 200, 32, (64, 128))), 3, _dt, expect=("+pool",))
    case("pool2d-32-%s" % _dt, ("g_pool2d", (26, 104, 16 if _dt == "fp32" else 32, (32,))), 4, _dt, expect=("32x256,tap9,2d,x2>+pool",))
    # the pooled conv itself with signed kernels
    for _co, _ci in ((64, 32), (32, 32 if _dt == "fp16" else 16)) + (((128, 32),) if _dt == "fp16" else ()):
        case("pool2d-signed-%d-%s" % (_co, _dt), ("g_probe", (12, 200, _ci, _co, 3, 1, True, "leaky")), 3, _dt, expect=("+pool",), ties=_dt == "fp16", variants=("pool2",))
for _n, _t, _sym in [("residual_block_3x3", 12, "conv3x3_tap_kernel<false, 2, 4, 4, 4, 27, 4, 2, false, true, true>"),
                     ("stride2_into_stage", 6, "conv_igemm_dma_kernel<2, 4, 4, 4, 3, 4, 4, true, 0>"),
                     ("stride2_into_stage_tap", 23, "conv3x3_tap_kernel<false, 2, 4, 4, 4, 26, 4, 4, false, true, true>")]:
    case("fuse2-%s" % _n, ("g_fuse2", (_n,)), 3, "fp16", tile=_t, expect=("+1x1", "fused into the conv in front", _sym), ties=True)
for _dt in ("fp16", "fp32"):
    case("upsample-concat-%s" % _dt, ("g_upsample", ()), 2, _dt, expect=("fused: upsample x2", "concat slice"))
    case("reorg-concat-%s" % _dt, ("g_reorg", ()), 2, _dt, expect=("fused: reorg x2",))
    for _n, (_B, _H, _W, _ci, _co) in sorted({"head255": (2, 5, 5, 256, 255), "head425": (2, 13, 13, 1024, 425), "head125": (1, 13, 13, 1024, 125),
                                              "head18_tower": (1, 13, 13, 1024, 18), "head_vec_256": (2, 6, 6, 128, 256)}.items()):
        case("%s-%s" % (_n, _dt), ("g_probe", (_H, _W, _ci, _co, 1, 1, False, "linear")), _B, _dt, neg=False, variants=("f32",))
    if _dt == "fp16":       # YOLOv3's 255-channel heads on the one-round 1x1 tile: the float32 scalar-store epilogue of conv_dma.hip
        for _sh in ((2, 5, 5, 256, 255), (1, 38, 38, 512, 255)):
            case("head255-%s-t19" % _shape_name(_sh), ("g_probe", _sh[1:] + (1, 1, False, "linear")), _sh[0], "fp16", tile=19, neg=False, variants=("f32",),
                 expect=(TILE_NAME[19], "conv_igemm_dma_kernel<2, 4, 4, 3, 4, 8, 2, false, 2>"))
    # data movement alone: every layer of the unfused plan read back
    case("fallback-kernels-%s" % _dt, ("g_fallback", ()), 2, _dt, keep_all=True, expect=("eltwise<", "pool<"))
    case("maxpool-odd-%s" % _dt, ("g_maxpool_odd", ()), 3, _dt, keep_all=True, expect=("pool<",), ties=_dt == "fp16")
    # run structure: parts of a batch on two / three streams, and a forward after autotune -- no summation-order noise left to excuse a difference
    for _st in (2, 3):
        case("streams%d-%s" % (_st, _dt), ("g_residual_blocks", ()), 5, _dt, kw={"streams": _st, "max_batch": 6}, neg=False, repeat=True)
    case("autotune-%s" % _dt, ("g_residual_blocks", ()), 4, _dt, kw={"autotune": True}, neg=False, repeat=True)

# the one deviation from forward_ref.forward(storage="fp16"): a fused residual that is the graph's LAST layer goes to the caller's float32 tensor
# unrounded (on integer data still exact); the reference of this variant leaves that one rounding out
for _sh in ((2, 19, 19, 128, 128), (1, 38, 38, 256, 256)):
    case("shortcut-last-%s" % _shape_name(_sh), ("g_probe", _sh[1:] + (3, 1, True, "leaky")), _sh[0], "fp16", expect=("fused: +shortcut",), variants=("res_last",))

# ---- past the first round --------------------------------------------------------------------------------------------------------
# The persistent kernels (conv3x3_tap_stream_kernel, stem_v3_kernel, first_pool_mfma*_kernel) launch at most a fixed number of workgroups,
# each of which walks tiles blockIdx, blockIdx + grid, ...; the grid-stride kernels of aux.hip launch at most a fixed number of threads.
# What happens between two tiles of one workgroup (the next tile's patch and weights requested under the current tile's last slice, the
# epilogue's stores between the DMAs of the counted waits, the accumulators restarted from the bias copy in LDS, the register prefetch one
# tile ahead, tile i + 1 overwriting the patches of tile i) runs only past those caps: the cases below are the smallest shapes that get
# there.  ROUNDS says, per case, which cap of yolo_launch_caps it is about, how its work is counted from the shape and what it claims
# ("control": exactly one round; "one-more": cap + 1, ONE workgroup gets a second tile; "three": at least three rounds; "two": more than
# one round); tests/test_rounds_cpu.py holds every claim against the library's own caps, so a changed cap turns them red instead of
# quietly turning these into one-round tests.  The default tile rules apply (no forced tile).
TAP_STREAM_SYM = "conv3x3_tap_stream_kernel<1, 8, 4, 2, 27, 4, 2>"
ROUNDS = {}       # case id -> dict(cap, tile=(rows, columns of OUTPUT positions per tile) | None, work, claim, parts)


def _cdiv(a, b):
    return -(-a // b)


def rounds_case(id, cap, work, claim, tile=None, parts=1, **kw):
    ROUNDS[id] = dict(cap=cap, tile=tile, work=int(work), claim=claim, parts=parts)
    case(id, **kw)


# the stream tap kernel, fp16: tiles of 16 x 16 positions.  "pool" reads the fp16 store through a stride-1 pool ("res": + the fused residual,
# where Cin = Cout); the float32 output is not a stream launch (tap_stream_ok).  The pool behind the 1089-tile case is pool_kernel<false, true>
# on 2.2 M items as well: aux.hip's grid-stride loop in its third round (no case of its own).
for (_B, _H, _W, _ci, _co), _bn, _claim in [
        ((2, 256, 256, 32, 64), True, "control"),      # 512 tiles: exactly the grid, nobody gets a second tile
        ((3, 304, 144, 32, 64), True, "one-more"),     # 513: one workgroup gets a second tile
        ((9, 176, 176, 32, 64), True, "three"),        # 1089: three rounds, the last of 65; one slice per tile: consecutive tiles alternate patch buffers
        ((3, 200, 210, 64, 64), True, "two"),          # 546 (= 2 mod 8: xcd_remap on a count that is no multiple of 8), two slices per tile, partial tiles both ways
        ((3, 200, 210, 128, 48), True, "two"),         # four slices, Cout 48: lanes beyond Cout, bias from LDS
        ((3, 200, 210, 192, 64), True, "two"),         # six slices
        ((4, 192, 200, 32, 64), False, "two")]:        # 624, no BN, linear, bias: the other epilogue arm
    rounds_case("rounds-tap-%s%s" % (_shape_name((_B, _H, _W, _ci, _co)), "" if _bn else "-linear"), "tap_stream_workgroups",
                _B * _cdiv(_H, 16) * _cdiv(_W, 16), _claim, tile=(16, 16),
                graph=("g_probe", (_H, _W, _ci, _co, 3, 1, _bn, "leaky" if _bn else "linear")), B=_B, dtype="fp16", expect=(TAP_STREAM_SYM,), ties=True, neg=_bn,
                variants=("pool",) + (("res",) if _ci == _co else ()))

# the stem, both forms: tiles of 8 x 16 outputs (16 x 32 input pixels).  The 3x3 32 -> 64 conv + shortcut behind the Darknet-53 form is a
# stream-kernel launch at these sizes as well.
for (_B, _H, _W), _claim in [((2, 256, 512), "control"), ((3, 144, 608), "one-more"), ((6, 224, 416), "three"), ((5, 180, 300), "two")]:
    for _third in (32, 64):
        rounds_case("rounds-stem-3-32-64%s-%s" % ("-32" if _third == 32 else "", _shape_name((_B, _H, _W))), "stem_workgroups",
                    _B * _cdiv(_H, 16) * _cdiv(_W, 32), _claim, tile=(8, 16), graph=("g_stem", (_H, _W, _third)), B=_B, dtype="fp16", ties=True,
                    expect=("conv_stem<f16,3-32-64-32>", "yolo::stem_v3_kernel(", TAP_STREAM_SYM) if _third == 32 else ("conv_stem<f16,3-32-64>", "yolo::stem_v3_kernel("),
                    absent=() if _third == 32 else ("3-32-64-32",))
# ... and as two parts on two streams: 546 tiles each on a grid of 256 (the cap is divided by the parts)
rounds_case("rounds-stem-3-32-64-32-6x224x416-streams2", "stem_workgroups", 3 * _cdiv(224, 16) * _cdiv(416, 32), "three", tile=(8, 16), parts=2,
            graph=("g_stem", (224, 416, 32)), B=6, dtype="fp16", ties=True, kw={"streams": 2, "max_batch": 6}, repeat=True,
            expect=("conv_stem<f16,3-32-64-32>", "yolo::stem_v3_kernel("))

# first layer + pool on the matrix cores: tiles of 8 x 16 POOLED outputs (16 x 32 input pixels)
for (_B, _H, _W), _claim in [((4, 256, 512), "control"), ((5, 80, 1312), "one-more"), ((10, 240, 464), "three"), ((5, 244, 470), "two")]:
    for _dt, _co, _sym in [("fp16", 32, "yolo::first_pool_mfma_kernel("), ("fp32", 32, "first_pool_mfma_f32_kernel<2>("), ("fp32", 16, "first_pool_mfma_f32_kernel<1>(")]:
        rounds_case("rounds-firstpool-%s-%d-%s" % (_shape_name((_B, _H, _W)), _co, _dt), "first_mfma_workgroups", _B * _cdiv(_H, 16) * _cdiv(_W, 32), _claim,
                    tile=(8, 16), graph=("g_first_pool", (_H, _W, _co, 32)), B=_B, dtype=_dt, ties=_dt == "fp16", expect=("conv_first_pool", _sym))

# the grid-stride kernels of aux.hip past 1 048 576 work items, every layer read back.  eltwise_kernel counts elements of its input: the
# standalone add, the reorg and the concat copies (4.5 M), the upsample of the pooled map (1 115 136: the count the case is sized by).
# pool_kernel counts 16-byte vectors where the strides allow them: the 2/1 pool is 1 115 136 items in float32 and 557 568 in fp16, the 2/2
# pool a quarter of that -- fp16 pools get past the cap behind the 1089-tile stream case above.  prep_kernel counts pixels: 1 076 480
# (8 input channels: not a first-layer kernel) in front of a 1x1 conv.  (Every rounds case ends in an eltwise copy to the float32 output
# that is past the cap as well.)
for _dt in ("fp16", "fp32"):
    rounds_case("rounds-fallback-kernels-2x264x264x16-%s" % _dt, "aux_work_items", 2 * 132 * 132 * 32, "two", graph=("g_fallback", (264, 264, 16)), B=2, dtype=_dt,
                keep_all=True, expect=("eltwise<", "pool<"))
    rounds_case("rounds-prep-5x464x464x8-%s" % _dt, "aux_work_items", 5 * 464 * 464, "two", graph=("g_probe", (464, 464, 8, 16, 1, 1, True, "leaky")), B=5, dtype=_dt,
                keep_all=True, expect=("prep<",), ties=_dt == "fp16", variants=("pool",))

RAW_CASES = CASES
KERNELS_JSON = os.path.join(GOLDEN, "exact_kernels.json")


FORCED_FAMILIES = ("tap", "s2", "dma", "head255")      # the cases that are about a forced tile id


def is_forced(c):
    return c["id"].split("-")[0] in FORCED_FAMILIES and c["tile"] in TILE_NAME


def _is_split(name):
    return "splitK" in name or "+pairK" in name


def select_cases(raw, golden):
    """Attach the recorded conv kernel name of every single-conv probe variant (c["kernel"]) and leave out what the recorded plan shows as a
    repeat: forced-tile variants whose tile is not valid for the shape (one fall-back case per tile and dtype stays, c["fallback"]) and
    split-K variants the plan does not split.  golden = None (no record yet / being rewritten): everything stays, nothing is named."""
    out, fallbacks = [], set()
    for c in raw:
        c = dict(c, kernel=None, fallback=False)
        if golden is not None and c["graph"][0] == "g_probe":
            names = golden[c["id"]]
            c["kernel"] = names
            if is_forced(c):
                runs = tuple(v for v in c["variants"] if TILE_NAME[c["tile"]] in names[v])
                if not runs:
                    if (c["tile"], c["dtype"]) in fallbacks:
                        continue
                    fallbacks.add((c["tile"], c["dtype"]))
                    c["fallback"] = True
                    runs = c["variants"][-1:]
                c["variants"] = runs
            if c["id"].startswith("splitk-"):
                c["variants"] = tuple(v for v in c["variants"] if _is_split(names[v]))
                if not c["variants"]:
                    continue
            c["ties"] = c["ties"] and any(v != "f32" for v in c["variants"])        # (the float32 output is not rounded)
        out.append(c)
    return out


def _load_golden():
    if not os.path.exists(KERNELS_JSON):
        return None
    with open(KERNELS_JSON) as f:
        return json.load(f)


CASES = select_cases(RAW_CASES, None if __name__ == "__main__" else _load_golden())      # (the record is being rewritten: new cases are not in it yet)
IDS = [c["id"] for c in CASES]
assert len(set(IDS)) == len(IDS)


def plan_of(c, variant):
    """the plan of a case variant (no GPU needed) -> (Plan, kernel names, names + symbols + description as one text)"""
    import ctypes as C
    from tensorflow_yolo_amd import _hip
    from tensorflow_yolo_amd.net import engine
    kw = dict(c["kw"])
    kw.pop("autotune", None)
    p = engine.Plan(build_graph(c, variant), dtype=c["dtype"], max_batch=kw.pop("max_batch", c["B"]), keep_all=c["keep_all"], force_tile=c["tile"], **kw)
    return (p,) + kernel_text(p, [_info(p, k, C, _hip) for k in range(p.num_kernels)])


def _info(p, k, C, _hip):
    ki = _hip.KernelInfo()
    _hip.check(p.lib.yolo_net_kernel_info(p.handle, k, C.byref(ki)), "yolo_net_kernel_info")
    return ki


def kernel_text(p, infos):
    names = [ki.name.decode() for ki in infos]
    return names, " ".join(names) + " " + " ".join(ki.symbol.decode() for ki in infos) + " " + p.describe()


def check_kernels(c, variant, p, names, text):
    """the kernel meant is the one that runs (the same assertions on the CPU plan and on the engine that ran)"""
    for s in c["expect"]:
        assert s in text, (c["id"], variant, s, names)
    for s in c["absent"]:
        assert s not in text, (c["id"], variant, s, names)
    note = ""
    if c["kernel"] is not None:
        convs = [n for n in names if n.startswith("conv")]
        assert convs == [c["kernel"][variant]], (c["id"], variant, convs, c["kernel"][variant])
        if is_forced(c):
            runs = TILE_NAME[c["tile"]] in convs[0]
            assert runs != c["fallback"], (c["id"], variant, convs)
            note = " [forced tile %d runs]" % c["tile"] if runs else " [tile %d is not valid for this layer: the default runs]" % c["tile"]
    if "streams" in c["kw"]:
        assert p.num_streams == c["kw"]["streams"], (c["id"], p.num_streams)
    return note


# ---- reference side (no GPU) --------------------------------------------------------------------------------------------------
def build_graph(c, variant):
    name, args = c["graph"]
    return GRAPHS[name](*(args + ((variant,) if name == "g_probe" else ())))


@functools.lru_cache(maxsize=24)
def _reference(graph, variant, B, storage, data, keep_all):
    """(L, case data, reference output, kept layers, preconditions report): depends on the graph and the data only, never on tile or plan"""
    c = {"graph": graph}
    g = build_graph(c, variant)
    L = to_oracle(g)
    seed = zlib.crc32(repr((graph, variant, B)).encode()) % (1 << 31)
    d = X.make_case(L, B, seed=seed, **dict(data))
    rep = X.check_preconditions(L, d, storage, keep=set(range(len(L))) if keep_all else set(), last_shortcut_f32=variant == "res_last")
    return L, d, rep.pop("out"), rep.pop("kept"), rep


def reference(c, variant):
    return _reference(c["graph"], variant, c["B"], c["dtype"], tuple(sorted(c["data"].items())), c["keep_all"])


def case_report(c):
    """preconditions of every variant of a case; the ties / negative-branch requirement is met by at least one variant"""
    reps = [reference(c, v)[4] for v in c["variants"]]
    ties, neg = sum(r["ties"] for r in reps), sum(r["neg"] for r in reps)
    assert ties > 0 or not c["ties"], "%s: no fp16 tie in front of a rounding" % c["id"]
    assert neg > 0 or not c["neg"], "%s: nothing on leaky's negative branch" % c["id"]
    return ties, neg


# ---- device side --------------------------------------------------------------------------------------------------------------
def _launch_position(cap, g, n_tiles):
    """conv3x3_tap_stream_kernel walks launch positions it = blockIdx, blockIdx + grid, ... and computes tile xcd_remap(it, n_tiles)
    (conv_common.h: the positions of one XCD, it % 8, take consecutive tiles): the position whose tile is g"""
    if cap != "tap_stream_workgroups":
        return g
    q, r = n_tiles >> 3, n_tiles & 7
    start = lambda x: x * (q + 1) if x < r else r * (q + 1) + (x - r) * q
    x = max(v for v in range(8) if start(v) <= g)
    return (g - start(x)) * 8 + x


def where_in_rounds(rounds, idx, shape, batch):
    """What whoever reads a failure of a rounds case needs first: the tile (image, tile row, tile column) of the element at idx = (n, y, x, c)
    of a tensor of `shape`, and whether the workgroup that computed it was past its first tile -- its launch position at or above the cap (a
    cap divided by the parts of the batch on streams; tiles counted per part).  A tensor that is not on the kernel's output grid, and the
    grid-stride kernels: the linear element index against the cap."""
    from tensorflow_yolo_amd import _hip
    cap = _hip.launch_caps()[rounds["cap"]] // rounds["parts"]
    n, y, x = (int(v) for v in idx[:3])
    if rounds["tile"] is None:
        lin = int(np.ravel_multi_index(tuple(int(v) for v in idx), shape))
        return "element %d of %d: %s the cap of %d work items (%s)" % (lin, int(np.prod(shape)), "AT OR ABOVE" if lin >= cap else "below", cap, rounds["cap"])
    th, tw = rounds["tile"]
    tiles_y, tiles_x = _cdiv(shape[1], th), _cdiv(shape[2], tw)
    per_part = _cdiv(batch, rounds["parts"])
    images = min(per_part, batch - n // per_part * per_part)           # images of the part image n is in
    g = ((n % per_part) * tiles_y + y // th) * tiles_x + x // tw
    pos = _launch_position(rounds["cap"], g, images * tiles_y * tiles_x)
    return "tile (image %d, tile row %d, tile column %d) = tile %d, launch position %d of its part: %s the cap of %d workgroups (%s): the %s tile of its workgroup" % (
        n, y // th, x // tw, g, pos, "AT OR ABOVE" if pos >= cap else "below", cap, rounds["cap"], "%d." % (pos // cap + 1))


def assert_equal(got, want, what, rounds=None, batch=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    rows = ["  (n, y, x, c) = %s: got %r want %r" % (tuple(int(v) for v in i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:12]]
    if rounds is not None:
        rows.insert(0, "  first difference in " + where_in_rounds(rounds, bad[0], got.shape, batch or got.shape[0]))
    raise AssertionError("%s: %d of %d elements differ\n%s" % (what, len(bad), got.size, "\n".join(rows)))


@pytest.mark.parametrize("cid", IDS)
def test_exact(cid):
    c = CASES[IDS.index(cid)]
    ties, neg = case_report(c)                      # reference and data only: before anything touches the GPU
    for variant in c["variants"]:
        L, d, want, kept, rep = reference(c, variant)
        g = build_graph(c, variant)
        kw = dict(c["kw"])
        tune = kw.pop("autotune", False)
        got, eng = run_hip(g, d["stream"], d["x"], c["dtype"], keep_all=c["keep_all"], force_tile=c["tile"], **kw)
        names, text = kernel_text(eng, eng.kernel_infos())
        note = check_kernels(c, variant, eng, names, text)
        print("%s/%s: kernels %s%s; reference: %d fp16 ties, %d on leaky's negative branch, max conv(|x|,|w|)+|b| %g"
              % (cid, variant, names, note, rep["ties"], rep["neg"], rep["bound"]))
        if variant == "res_last":       # the case is about values an fp16 store would have changed
            assert np.any(want != X.round_f16(want)), "nothing in the reference that an fp16 rounding would change"
        what = "%s/%s %s" % (cid, variant, names)
        rounds = ROUNDS.get(cid)                    # (a rounds case: a failure names the tile and which round of its workgroup it was)
        assert_equal(got, want, what, rounds)
        if c["keep_all"]:
            for i in range(1, len(L) - 1):          # (the last layer lives in the caller's tensor: it is `got`)
                assert_equal(eng.read_layer(i, c["B"]), kept[i], what + " layer %d" % i, rounds and dict(rounds, tile=None))
        if tune:
            eng.autotune(d["x"])
            assert_equal(eng.forward(d["x"]).cpu().numpy(), want, what + " after autotune")
        if c["repeat"]:
            for r in range(2):
                assert_equal(eng.forward(d["x"]).cpu().numpy(), want, what + " launch %d" % (r + 2), rounds)
            if c["B"] > 1:          # a smaller batch than max_batch: the same bits per image
                assert_equal(eng.forward(d["x"][:c["B"] - 1]).cpu().numpy(), want[:c["B"] - 1], what + " at batch %d" % (c["B"] - 1), rounds, c["B"] - 1)


if __name__ == "__main__":      # rewrite the recorded plans of the single-conv probes (no GPU needed)
    CASES = select_cases(RAW_CASES, None)
    rec = {}
    for c in CASES:
        if c["graph"][0] == "g_probe":
            rec[c["id"]] = {}
            for v in c["variants"]:
                convs = [n for n in plan_of(c, v)[1] if n.startswith("conv")]
                assert len(convs) == 1, (c["id"], v, convs)
                rec[c["id"]][v] = convs[0]
    with open(KERNELS_JSON, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d probes recorded in %s" % (len(rec), KERNELS_JSON))

"""The cases of tests/test_gpu_large.py (every forward kernel on tensors at and past the 2 GiB line), as a table that needs no GPU:
tests/test_large_cpu.py plans every row with engine.Plan, derives the batch sizes from the plan alone and holds the kernels a row is in
the table for against the plan's own text, so a changed constant or rule fails there instead of quietly turning the GPU cases into
ordinary ones.

What the library decides by SIZE (conv_dispatch.cpp: conv_shape_params, resolve_conv; forward.cpp: conv_params): a conv whose input
buffer has more than LIMIT = 0x7ffffff0 bytes is refused; an output or residual above LIMIT sets out_bytes / res_bytes to 0, which
turns the lean, buffer-addressed epilogue off (the generic one is addressed through long long) and drops the back-to-back 1x1.

Sizing.  A tensor of S bytes per image (image stride x element size; the WHOLE concat buffer where the view is a slice; 4 bytes per
element for a float32 output) is at the limit at B_last = LIMIT // S images and past it at B_first = B_last + 1.  A row names the
tensor it is about by the planned kernel that writes it ("about": the layer; "what": in | out | res | out2 | final) and states S from
the shape; test_large_cpu.py reads the same S from the plan.  Maps are 252 x 266 (67 032 pixels = 261.8 tiles of 256: ragged in M; 15.75 x
16.6 tiles of 16 x 16; S never a power of two), 86 x 98 for the MX kernel (maps up to 100 wide) and 30 x 26 for the SPP kernel (maps up to
32 x 32).  Image n of a batch is distinct image n mod D, D = 3: 2^31 and 2^32 are no multiples of 3, so an offset truncated by either
cannot land on an image of equal content (S is no power of two either).

Sides of a row: "last" (B_last), "first" (B_first), "refuse" (B_first of a conv INPUT: the call must fail), "past4g" (the first batch
whose tensor exceeds 2^32 bytes), "parts2" (B_first of a conv input on two streams: each part holds half).
"""
import numpy as np

import exact_ref as X
import spp_ref
from helpers import new_graph, to_oracle
from tensorflow_yolo_amd.net import layers as PL

LIMIT = 0x7ffffff0
D = 3                                   # distinct images
H, W = 252, 266
PX = H * W
MXH, MXW = 86, 98
CAP_BYTES = 16 << 30                    # no test may hold more device memory than this
COMPARE_BYTES = 3 << 28                 # what the chunked comparison holds at its peak beside the tensors (helpers.large_difference)


def _conv(g, src, f, k, s=1, bn=True, act="leaky"):
    g.append(PL.conv2d_bn_act(src.out, f, k, s, use_batch_normalization=bn, activation_fn=act))


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------
def g_conv(h, w, cin, cout, k, s, tail, bn=True, act="leaky"):
    """ONE conv on the graph input.  tail "f32": the conv is the last layer (float32, the caller's tensor); "pool2": a 2x2/2 max-pool
    behind it, so that the conv stores fp16 into the workspace (read there through a view) and the float32 tail stays small"""
    g = new_graph(h, w, cin)
    _conv(g, g[0], cout, k, s, bn, act)
    if tail == "pool2":
        g.append(PL.max_pool2d(g[-1].out, 2, stride=2))
    return g


def g_res_slice(h, w):
    """a 3x3 conv 32 -> 32 with a fused residual that is a 32-channel SLICE of a 128-channel concat buffer: the residual's extent counts the
    whole buffer, so res_bytes is 0 at a batch where the conv's own input and output are a quarter of the limit"""
    g = new_graph(h, w, 32)
    _conv(g, g[0], 32, 1)                                   # 1: the residual, channels 0..31 of the concat
    _conv(g, g[0], 96, 1)                                   # 2: channels 32..127
    g.append(PL.route([g[1].out, g[2].out]))                # 3
    _conv(g, g[0], 32, 3)                                   # 4
    g.append(PL.shortcut(g[4].out, g[1].out))               # 5: fused into conv 4
    g.append(PL.max_pool2d(g[5].out, 2, stride=2))          # 6
    g.append(PL.max_pool2d(g[3].out, 2, stride=2))          # 7
    g.append(PL.route([g[6].out, g[7].out]))                # 8
    return g


def g_up(h, w):
    """a 1x1 conv whose epilogue writes the nearest-upsample x2 map into a slice of a 128-channel concat buffer"""
    g = new_graph(h, w, 32)
    g.append(PL.max_pool2d(g[0].out, 2, stride=2))          # 1: h/2 x w/2
    _conv(g, g[1], 64, 1)                                   # 2
    g.append(PL.upsample(g[2].out, 2))                      # 3: fused into conv 2
    _conv(g, g[0], 64, 1)                                   # 4
    g.append(PL.route([g[3].out, g[4].out]))                # 5: 128 channels at h x w
    g.append(PL.max_pool2d(g[5].out, 2, stride=2))          # 6
    return g


def g_reorg(h, w):
    """a 1x1 conv whose epilogue writes the block-major reorg x2 map into a slice of a 160-channel concat buffer"""
    g = new_graph(h, w, 32)
    _conv(g, g[0], 32, 1)                                   # 1
    g.append(PL.reorg(g[1].out, 2))                         # 2: h/2 x w/2 x 128, fused into conv 1
    g.append(PL.max_pool2d(g[0].out, 2, stride=2))          # 3
    _conv(g, g[3], 32, 1)                                   # 4
    g.append(PL.route([g[2].out, g[4].out]))                # 5: 160 channels
    g.append(PL.max_pool2d(g[5].out, 2, stride=2))          # 6
    return g


def g_pooled(h, w, cin, cout):
    """conv 3x3 + 2x2/2 max-pool (fused into the 2-D tap tile's epilogue by the production plan), a second pool as the small tail"""
    g = new_graph(h, w, cin)
    _conv(g, g[0], cout, 3)
    g.append(PL.max_pool2d(g[1].out, 2, stride=2))
    g.append(PL.max_pool2d(g[2].out, 2, stride=2))
    return g


def g_fuse2(h, w):
    """the stride-2 conv into a stage with the next block's 1x1 128 -> 64 behind it (back-to-back fusion), the 1x1's output being a slice of a
    256-channel concat buffer: its extent is four times its payload and twice the 3x3's"""
    g = new_graph(h, w, 32)
    _conv(g, g[0], 128, 3, 2)                               # 1: h/2 x w/2 x 128
    _conv(g, g[1], 64, 1)                                   # 2
    g.append(PL.max_pool2d(g[0].out, 2, stride=2))          # 3
    _conv(g, g[3], 192, 1)                                  # 4
    g.append(PL.route([g[2].out, g[4].out]))                # 5: 256 channels
    g.append(PL.max_pool2d(g[5].out, 2, stride=2))          # 6
    g.append(PL.max_pool2d(g[1].out, 2, stride=2))          # 7
    g.append(PL.route([g[6].out, g[7].out]))                # 8
    return g


def g_move(h, w, c, op):
    """ONE data-movement kernel of the unfused plan on the graph input (prep_kernel in front), a 2x2/2 pool as the small tail:
    "add" = a 2x2/1 pool and the standalone add of it to the input; "up" / "reorg" = the standalone upsample / reorg copy; "pool2" = the 2x2/2 pool"""
    g = new_graph(h, w, c)
    if op == "add":
        g.append(PL.max_pool2d(g[0].out, 2, 1))
        g.append(PL.shortcut(g[0].out, g[1].out))
    elif op == "up":
        g.append(PL.upsample(g[0].out, 2))
    elif op == "reorg":
        g.append(PL.reorg(g[0].out, 2))
    else:
        assert op == "pool2"
    g.append(PL.max_pool2d(g[-1].out, 2, 2))
    return g


def g_pool_same(h, w, c, k):
    """an odd stride-1 SAME pool of the graph input, a 2x2/2 pool as tail"""
    g = new_graph(h, w, c)
    g.append(PL.max_pool2d(g[0].out, k, 1))
    g.append(PL.max_pool2d(g[1].out, 2, 2))
    return g


def g_spp(h, w, c):
    """the SPP block (pools 5, 9, 13 of one tensor, concatenated with it) on the graph input"""
    g = new_graph(h, w, c)
    for k in (5, 9, 13):
        g.append(PL.max_pool2d(g[0].out, k, 1))
    g.append(PL.route([g[3].out, g[2].out, g[1].out, g[0].out]))
    g.append(PL.max_pool2d(g[4].out, 2, 2))
    return g


def g_first(h, w, cout, pooled):
    """the 3-channel first conv; pooled: with the 2x2/2 pool the production plan fuses into it"""
    g = new_graph(h, w, 3)
    _conv(g, g[0], cout, 3)
    g.append(PL.max_pool2d(g[1].out, 2, 2))
    if pooled:
        g.append(PL.max_pool2d(g[2].out, 2, 2))
    return g


def g_stem(h, w):
    """Darknet-53's first block: 3 -> 32, 32 -> 64 / 2, 1x1 64 -> 32 (the stem kernel with its out3 store), 3x3 32 -> 64 + shortcut"""
    g = new_graph(h, w, 3)
    _conv(g, g[0], 32, 3)
    _conv(g, g[1], 64, 3, 2)
    _conv(g, g[2], 32, 1)
    _conv(g, g[3], 64, 3)
    g.append(PL.shortcut(g[4].out, g[2].out))
    g.append(PL.max_pool2d(g[5].out, 2, 2))
    return g


GRAPHS = {f.__name__: f for f in (g_conv, g_res_slice, g_up, g_reorg, g_pooled, g_fuse2, g_move, g_pool_same, g_spp, g_first, g_stem)}

# ---- the table ------------------------------------------------------------------------------------------------------------------------
CASES = []


def case(id, graph, dtype, about, what, S, sides, kernel, tile=None, kw=None, keep_all=True, read=(), data=None, u8=False, expect=(), part=0):
    """about: the layer whose planned kernel the row is about; what: which of its tensors sets S -- "in" (its input buffer), "out", "res", "out2"
    (the back-to-back 1x1's output), "final" (the caller's float32 tensor), "user_in" (the caller's input tensor).
    kernel: {side: substring of that kernel's name + symbol}; expect: substrings of the whole plan text at every side.
    read: layers compared through a view of the workspace (the final output always is); (layer, "in", consumer): the whole concat buffer of
    a route, as the kernel of layer `consumer` reads it.  part: which list of the issue the row answers."""
    CASES.append(dict(id=id, graph=graph, dtype=dtype, about=about, what=what, S=int(S), sides=tuple(sides), kernel=kernel, tile=tile, kw=kw or {},
                      keep_all=keep_all, read=tuple(read), data=data or {}, u8=u8, expect=tuple(expect), part=part))


def batch_of(c, side):
    b_last = LIMIT // c["S"]
    if side == "last":
        return b_last
    if side in ("first", "refuse", "parts2"):
        return b_last + 1
    if side == "past4g":
        return (1 << 32) // c["S"] + 1
    raise ValueError(side)


F16_IN = PX * 32 * 2                    # a 32-channel fp16 map of 252 x 266: 4 290 048 bytes
# 1. conv inputs in the last bytes below the limit (and 2., 7.: the refusal at B_first, and the same batch as two parts) ------------------
IGEMM = "conv_igemm_kernel<false, 1, 4, 2, 4, true>"
for _n, _k, _s in (("3x3", 3, 1), ("3x3s2", 3, 2), ("1x1", 1, 1)):
    case("in-4wave-%s" % _n, ("g_conv", (H, W, 32, 32, _k, _s, "pool2")), "fp16", 1, "in", F16_IN,
         ("last", "refuse", "parts2") if _n == "3x3" else ("last",), {"last": IGEMM}, tile=0, read=(1,), part=1)
case("in-dma-64x512", ("g_conv", (H, W, 32, 32, 1, 1, "pool2")), "fp16", 1, "in", F16_IN, ("last",), {"last": "conv_igemm_dma_kernel<1, 8, 4, 4, 2, 4, 4, false, 1>"},
     tile=7, read=(1,), part=1)
case("in-tap-stream", ("g_conv", (H, W, 64, 64, 3, 1, "pool2")), "fp16", 1, "in", PX * 64 * 2, ("last",), {"last": "conv3x3_tap_stream_kernel<1, 8, 4, 2, 27, 4, 2>"},
     read=(1,), part=1)
case("in-tap2d-32x256", ("g_conv", (H, W, 32, 32, 3, 1, "pool2")), "fp16", 1, "in", F16_IN, ("last",),
     {"last": "conv3x3_tap_kernel<false, 1, 8, 2, 2, 27, 4, 2, false, true, false>"}, tile=17, read=(1,), part=1)
case("in-taps2-wide", ("g_conv", (H, W, 32, 128, 3, 2, "pool2")), "fp16", 1, "in", F16_IN, ("last",), {"last": "128x256,tap9,s2,wide,x2>"}, tile=23, read=(1,), part=1)
MX_DATA = {"xmax": X.MX_MAX, "wmax": X.MX_MAX}
case("in-mx", ("g_conv", (MXH, MXW, 128, 32, 3, 1, "pool2")), "mxfp8", 1, "in", MXH * MXW * 128 * 2, ("last",), {"last": "conv3x3_mx_kernel<true>"},
     read=(1,), data=MX_DATA, part=1)
case("in-f32-4wave", ("g_conv", (H, W, 32, 32, 3, 1, "pool2")), "fp32", 1, "in", PX * 32 * 4, ("last", "refuse"), {"last": "conv_igemm_kernel<true, 1, 4, 2, 4, false>"},
     tile=0, read=(1,), part=1)
case("in-f32-tap2d-32x256", ("g_conv", (H, W, 32, 32, 3, 1, "pool2")), "fp32", 1, "in", PX * 32 * 4, ("last",),
     {"last": "conv3x3_tap_kernel<true, 1, 8, 2, 2, 27, 4, 2, false, false, false>"}, tile=17, read=(1,), part=1)
# the second 4-wave kernel of conv.hip (float32 products as nine bf16 products) takes 128 couts: at stride 2 its output is as large as its input
case("in-f32-emu", ("g_conv", (H, W, 32, 128, 3, 2, "pool2")), "fp32", 1, "in", PX * 32 * 4, ("last",), {"last": "conv_igemm_emu_kernel<2, 4, 4, 2>"},
     tile=0, kw={"f32_products": 2}, read=(1,), data={"xmax": 8, "wmax": 8}, part=1)

# 3. outputs across the limit while the input stays below it (and 4.: past 2^32 bytes) -----------------------------------------------------
OUT128 = PX * 128 * 2                   # 17 160 192 bytes: B_last = 125
case("out-dma-1x1", ("g_conv", (H, W, 32, 128, 1, 1, "pool2")), "fp16", 1, "out", OUT128, ("last", "first", "past4g"),
     {"last": "conv_igemm_dma_kernel<2, 4, 4, 4, 3, 4, 4, false, 1>", "first": "conv_igemm_dma_kernel<2, 4, 4, 4, 3, 4, 4, false, 0>",
      "past4g": "conv_igemm_dma_kernel<2, 4, 4, 4, 3, 4, 4, false, 0>"}, read=(1,), part=3)
case("out-tap2d-128x256", ("g_conv", (H, W, 32, 128, 3, 1, "pool2")), "fp16", 1, "out", OUT128, ("last", "first"),
     {"last": "conv3x3_tap_kernel<false, 2, 4, 4, 4, 27, 4, 2, false, true, false>", "first": "conv3x3_tap_kernel<false, 2, 4, 4, 4, 27, 4, 2, false, false, false>"},
     read=(1,), part=3)
case("out-mx", ("g_conv", (MXH, MXW, 128, 256, 3, 1, "pool2")), "mxfp8", 1, "out", MXH * MXW * 256 * 2, ("last", "first"),
     {"last": "conv3x3_mx_kernel<true>", "first": "conv3x3_mx_kernel<false>"}, read=(1,), data=MX_DATA, part=3)
# res_bytes = 0 IS reachable with the input below the limit: the residual is a 32-channel slice of a 128-channel concat buffer
case("res-slice", ("g_res_slice", (H, W)), "fp16", 5, "res", OUT128, ("last", "first"),
     {"last": "conv3x3_tap_kernel<false, 1, 8, 2, 2, 27, 4, 2, false, true, false>", "first": "conv3x3_tap_kernel<false, 1, 8, 2, 2, 27, 4, 2, false, false, false>"},
     read=(1, 2, 5), expect=("fused: +shortcut", "concat slice"), part=3)
case("out-upsample", ("g_up", (H, W)), "fp16", 3, "out", OUT128, ("last", "first"), {"last": "conv_igemm", "first": "conv_igemm"}, read=(3, 4),
     expect=("fused: upsample x2", "concat slice"), part=3)
case("out-reorg", ("g_reorg", (H, W)), "fp16", 2, "out", (PX // 4) * 160 * 2, ("last", "first"), {"last": "conv_igemm", "first": "conv_igemm"}, read=(2, 4),
     expect=("fused: reorg x2",), part=3)
case("out-pooled", ("g_pooled", (H, W, 32, 256)), "fp16", 2, "out", (PX // 4) * 256 * 2, ("last", "first"), {"last": "+pool", "first": "+pool"}, keep_all=False,
     read=(2,), part=3)
case("out-f32-last", ("g_conv", (H, W, 32, 64, 1, 1, "f32")), "fp16", 1, "final", PX * 64 * 4, ("last", "first", "past4g"),
     {"last": "conv_igemm", "first": "conv_igemm", "past4g": "conv_igemm"}, part=3)

# 5. the back-to-back 1x1: its output extent can pass the limit while the 3x3 in front keeps its lean epilogue (a slice of a wider concat buffer)
case("fuse2-slice", ("g_fuse2", (H, W)), "fp16", 1, "out2", (PX // 4) * 256 * 2, ("last", "first"),
     {"last": "+1x1", "first": "conv3x3_tap_kernel<false, 2, 4, 4, 4, 26, 4, 4, false, false, false>"}, tile=23, keep_all=False, read=(1, (5, "in", 6)), part=5)

# 6. the other forward kernels ------------------------------------------------------------------------------------------------------------------
case("prep-f32", ("g_pool_same", (H, W, 32, 3)), "fp16", 0, "user_in", PX * 32 * 4, ("past4g",), {"past4g": "prep_kernel<false>"}, read=(0, 1),
     expect=("pool_same_kernel<false, true>",), part=6)
case("prep-u8", ("g_pool_same", (H, W, 32, 3)), "fp16", 0, "out", F16_IN, ("first",), {"first": "prep_kernel<false>"}, read=(0, 1), u8=True, part=6)
case("move-add-vec", ("g_move", (H, W, 32, "add")), "fp16", 2, "out", F16_IN, ("first",), {"first": "eltwise_kernel<false>"}, read=(0, 1, 2),
     expect=("pool_kernel<false, true>",), part=6)
case("move-add-scalar", ("g_move", (H, W, 10, "add")), "fp32", 2, "out", PX * 10 * 4, ("first",), {"first": "eltwise_kernel<true>"}, read=(0, 1, 2),
     expect=("pool_kernel<true, false>",), part=6)
case("move-up", ("g_move", (H, W, 16, "up")), "fp16", 1, "out", 4 * PX * 16 * 2, ("first",), {"first": "eltwise_kernel<false>"}, read=(1,), part=6)
case("move-reorg", ("g_move", (H, W, 32, "reorg")), "fp16", 1, "out", F16_IN, ("first",), {"first": "eltwise_kernel<false>"}, read=(1,), part=6)
case("move-pool2", ("g_move", (H, W, 32, "pool2")), "fp16", 1, "in", F16_IN, ("first",), {"first": "pool_kernel<false, true>"}, read=(0, 1), part=6)
case("pool-same-scalar", ("g_pool_same", (H, W, 12, 5)), "fp16", 1, "out", PX * 12 * 2, ("first",), {"first": "pool_same_kernel<false, false>"}, read=(1,), part=6)
case("spp", ("g_spp", (30, 26, 64)), "fp16", 1, "out", 30 * 26 * 256 * 2, ("first",), {"first": "spp_pool_kernel<2>"}, keep_all=False, read=((4, "in", 5),), part=6)
case("first", ("g_first", (H, W, 32, False)), "fp16", 1, "out", PX * 32 * 2, ("first",), {"first": "conv_first_kernel<false, 32, false>"}, read=(1,), part=6)
case("first-pool-mfma", ("g_first", (H, W, 32, True)), "fp16", 2, "out", (PX // 4) * 32 * 2, ("first",), {"first": "yolo::first_pool_mfma_kernel("}, keep_all=False,
     read=(2,), part=6)
case("first-pool-mfma-f32", ("g_first", (H, W, 32, True)), "fp32", 2, "out", (PX // 4) * 32 * 4, ("first",), {"first": "first_pool_mfma_f32_kernel<2>("},
     keep_all=False, read=(2,), part=6)
case("stem-out3", ("g_stem", (H, W)), "fp16", 2, "out", (PX // 4) * 64 * 2, ("first",), {"first": "yolo::stem_v3_kernel("}, keep_all=False,
     read=(2,), expect=("conv_stem<f16,3-32-64-32>", "fused: +shortcut"), part=6)

IDS = ["%s-%s" % (c["id"], s) for c in CASES for s in c["sides"]]
assert len(set(IDS)) == len(IDS)


def find(cid_side):
    for c in CASES:
        for s in c["sides"]:
            if "%s-%s" % (c["id"], s) == cid_side:
                return c, s
    raise KeyError(cid_side)


def build_graph(c):
    name, args = c["graph"]
    return GRAPHS[name](*args)


def engine_kw(c, side):
    """the options of the engine / plan of a row at one side"""
    kw = dict(c["kw"])
    keep_all = c["keep_all"]
    if side == "parts2":                # (two arenas need the production plan: keep_all plans one)
        kw["streams"], keep_all = 2, False
    else:
        kw.setdefault("streams", 1)
    return dict(dtype=c["dtype"], max_batch=batch_of(c, side), keep_all=keep_all, force_tile=c["tile"], **kw)


# ---- reference side (no GPU) ----------------------------------------------------------------------------------------------------------
def _has_conv(L):
    return any(op[0] == "conv" for op in L)


def moves_reference(L, x, dtype, keep):
    """the conv-less graphs: max-pools (2x2 as exact_ref, odd windows at stride 1 as spp_ref's clipped-window loop), route, reorg, upsample and
    the float32 add with its one rounding; the graph input rounded to the storage type"""
    q16 = dtype != "fp32"
    outs = []
    for op in L:
        k = op[0]
        if k == "input":
            y = X.round_f16(x) if q16 else x
        elif k == "maxpool":
            y = spp_ref.maxpool_naive(outs[op[1]], op[2]) if op[3] == 1 and op[2] % 2 else X.maxpool(outs[op[1]], op[2], op[3])
        elif k == "route":
            y = np.concatenate([outs[j] for j in op[1]], axis=3)
        elif k == "reorg":
            y = X.reorg(outs[op[1]], op[2])
        elif k == "upsample":
            y = X.upsample(outs[op[1]], op[2])
        elif k == "shortcut":
            y = outs[op[1]] + outs[op[2]]
            y = X.round_f16(y) if q16 else y
        else:
            raise ValueError(k)
        outs.append(np.ascontiguousarray(y, np.float32))
    return outs[-1], {i: outs[i] for i in keep}


_REF = {}


def reference(c):
    """(stream of weights, D distinct inputs, expected final output [D, ...], {layer: expected}, report) of a row: computed once, shared by its
    sides, read-only.  A uint8 row: the bytes themselves are the input; the library's float of a byte u is float32(u / 255.)."""
    if c["id"] in _REF:
        return _REF[c["id"]]
    g = build_graph(c)
    L = to_oracle(g)
    keep = {r if isinstance(r, int) else r[0] for r in c["read"]}
    if _has_conv(L):
        assert not c["u8"]
        d = X.make_case(L, D, seed=len(c["id"]) * 7919 + sum(map(ord, c["id"])), **c["data"])
        rep = X.check_preconditions(L, d, c["dtype"], keep=keep)
        out, kept, stream, x = rep.pop("out"), rep.pop("kept"), d["stream"], d["x"]
    else:
        rng = np.random.RandomState(sum(map(ord, c["id"])))
        shape = (D,) + tuple(g[0].out.hwc)
        if c["u8"]:
            x = rng.randint(0, 256, shape).astype(np.uint8)
            xf = (x.astype(np.float64) / 255.).astype(np.float32)
        else:
            x = rng.randint(-2048, 2049, shape).astype(np.float32)         # exact in fp16; sums of two stay below 65504
            xf = x
        out, kept = moves_reference(L, xf, c["dtype"], keep)
        stream, rep = np.zeros(0, np.float32), {"ties": 0, "neg": 0, "bound": 0.0}
    assert all(not np.array_equal(x[a], x[b]) for a in range(D) for b in range(a)), "the D images are not distinct"
    assert all(not np.array_equal(out[a], out[b]) for a in range(D) for b in range(a)), "the D expected outputs are not distinct"
    for a in (x, out) + tuple(kept.values()):
        a.setflags(write=False)
    _REF[c["id"]] = (stream, x, out, kept, rep)
    return _REF[c["id"]]

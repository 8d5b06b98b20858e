"""CPU: the conv dispatch decisions of whole plans, pinned against a record (tests/golden/dispatch_plans.json).

What a conv launch runs -- tile, K split, in-launch pair, back-to-back 1x1 fusion, kernel symbol -- and what the plan reserves for its
partial sums is decided on the host (csrc/conv_dispatch.cpp) and reported by yolo_net_kernel_info / yolo_net_workspace_regions without
a GPU.  For every plan of PLANS the record holds, per kernel, name, variant, symbol and the exact reprs of flops / bytes /
weight_bytes; the workspace size; offset, used and region bytes of the "split-K tickets + slabs" region; and the stream count.  The
comparison is exact equality.  test_grid_reaches_every_arm asserts that the recorded names cover every arm of the decision,
test_every_instantiation_is_reachable_and_every_report_is_real that the recorded symbols and the library's conv kernels are the same set
(up to a listed remainder).  The plans of FORCED are recorded once per tile id: what a tile id accepts, what a forced tile falls back
to and the symbol of every form it runs.

The record is a statement about behaviour, not about this code: a refactor of the dispatch must leave it untouched.
`python tests/test_dispatch_cpu.py` rewrites it after a DELIBERATE change of the rules (with YOLO_HIP_LIB pointing at another build of
the library, from that build).  Distinct names, symbols, kernel lines and kernel lists are stored once and referred to by index.
"""
import ctypes as C
import json
import os
import re

import numpy as np

from helpers import GOLDEN, new_graph
import spp_ref
from oracle import cases
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine, layers as PL, v2, v3

PLANS_JSON = os.path.join(GOLDEN, "dispatch_plans.json")
NAMES80 = ["c%d" % i for i in range(80)]
SPLITK_REGION = "split-K tickets + slabs"


def _coco_v3(make, size):
    return make(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(size, size, 3))


NETS = {
    "v3-608": lambda: _coco_v3(v3.create_network, 608),
    "v3-416": lambda: _coco_v3(v3.create_network, 416),
    "v3spp-416": lambda: _coco_v3(v3.create_spp_network, 416),
    "v3tiny-416": lambda: v3.create_tiny_network(np.reshape(spp_ref.TINY_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(416, 416, 3)),
    "v2-416": lambda: v2.create_full_network(np.reshape(cases.COCO_V2_ANCHORS, [-1, 2]), NAMES80, False),
    "tinyv2voc-416": lambda: v2.create_tiny_network(np.reshape(cases.VOC_TINY_ANCHORS, [-1, 2]), NAMES80[:20], False),
}
# the op-level graph of tests/test_gpu_ops.py::test_in_launch_pair_split_k: (dtype, (B, H, W, cin, cout))
PAIR_GRAPHS = [("fp16", (24, 13, 13, 256, 512)), ("fp16", (20, 19, 19, 512, 256)), ("fp32", (24, 13, 13, 128, 512)), ("fp32", (24, 19, 19, 128, 256))]


# (net, dtype, batch) of the plans that are recorded once per forced tile id
FORCED = [("v3-608", "fp16", 8), ("v3-608", "fp16", 32), ("v3-416", "fp16", 32), ("v2-416", "fp16", 16), ("v2-416", "fp32", 1), ("v2-416", "fp32", 16),
          ("tinyv2voc-416", "fp32", 64)]


def _pair_graph(shape):
    _, H, W, cin, cout = shape
    g = new_graph(H, W, cin)
    g.append(PL.conv2d_bn_act(g[-1].out, cout, 3, 1))
    g.append(PL.conv2d_bn_act(g[-1].out, cout, 3, 1))
    g.append(PL.shortcut(g[-1].out, g[1].out))
    return g


def _plans():
    """[(key, net name or graph shape, Plan keyword arguments)]"""
    out = []
    for net in NETS:
        for dtype in ("fp16", "fp32", "mxfp8"):
            for b in (1, 2, 4, 8, 16, 32) + ((64,) if "v2" in net else ()):
                out.append(("%s/%s/b%d" % (net, dtype, b), net, dict(dtype=dtype, max_batch=b)))
    for b in (32, 16):
        for s in (1, 2):
            out.append(("v3-608/fp16/b%d/streams%d" % (b, s), "v3-608", dict(dtype="fp16", max_batch=b, streams=s)))
    out.append(("v3-608/fp16/b2/keep_all", "v3-608", dict(dtype="fp16", max_batch=2, keep_all=True)))
    for net, dtype, b in FORCED:
        for tile in range(24):      # every tile id (0: the 4-wave kernel): validity, the fall-backs of a forced tile, the symbol of every form
            out.append(("%s/%s/b%d/tile%d" % (net, dtype, b, tile), net, dict(dtype=dtype, max_batch=b, force_tile=tile)))
    # (the MXFP8 kernel by name: yolo_net_options.force_tile = 25, which engine.Plan spells force_tile=24)
    out.append(("v3-608/mxfp8/b8/tile24", "v3-608", dict(dtype="mxfp8", max_batch=8, force_tile=24)))
    for f in (1, 2):
        out.append(("v2-416/fp32/b1/f32_products%d" % f, "v2-416", dict(dtype="fp32", max_batch=1, f32_products=f)))
    for dtype, shape in PAIR_GRAPHS:
        out.append(("pair-graph/%s/%s" % (dtype, "x".join(map(str, shape))), shape, dict(dtype=dtype, max_batch=shape[0])))
    return out


PLANS = _plans()


def record_plan(net, kw):
    p = engine.Plan(net, **kw)
    kernels = []
    for k in range(p.num_kernels):
        ki = _hip.KernelInfo()
        _hip.check(p.lib.yolo_net_kernel_info(p.handle, k, C.byref(ki)), "yolo_net_kernel_info")
        kernels.append((ki.name.decode(), int(ki.variant), ki.symbol.decode(), repr(float(ki.flops)), repr(float(ki.bytes)), repr(float(ki.weight_bytes))))
    splitk = [list(r[1:]) for r in p.workspace_regions() if r[0] == SPLITK_REGION]
    assert len(splitk) <= 1
    rec = dict(kernels=kernels, workspace_bytes=int(p.workspace_bytes), splitk=splitk[0] if splitk else None, num_streams=int(p.num_streams))
    p.close()
    return rec


def record_all():
    nets = {}
    out = {}
    for key, net, kw in PLANS:
        if isinstance(net, str):
            if net not in nets:
                nets[net] = NETS[net]()
            out[key] = record_plan(nets[net], kw)
        else:
            out[key] = record_plan(_pair_graph(net), kw)
    return out


def pack(plans):
    """Distinct names, symbols, kernel lines and kernel lists once; a list holds the indices of its kernel lines."""
    names, symbols, lines, lists = {}, {}, {}, {}

    def idx(table, v):
        return table.setdefault(v, len(table))

    packed = {}
    for key, rec in plans.items():
        ks = tuple(idx(lines, (idx(names, n), var, idx(symbols, sym), fl, by, wb)) for n, var, sym, fl, by, wb in rec["kernels"])
        packed[key] = dict(rec, kernels=idx(lists, ks))
    return dict(names=list(names), symbols=list(symbols), lines=[list(l) for l in lines], lists=[list(l) for l in lists], plans=packed)


def unpack(g):
    plans = {}
    for key, rec in g["plans"].items():
        ks = []
        for i in g["lists"][rec["kernels"]]:
            n, var, sym, fl, by, wb = g["lines"][i]
            ks.append((g["names"][n], var, g["symbols"][sym], fl, by, wb))
        plans[key] = dict(rec, kernels=ks)
    return plans


_got = []


def got_plans():
    if not _got:
        _got.append(record_all())
    return _got[0]


def test_dispatch_matches_the_record():
    with open(PLANS_JSON) as f:
        want = unpack(json.load(f))
    got = got_plans()
    assert sorted(got) == sorted(want), "the grid and the record list different plans: rewrite the record only after a deliberate change"
    bad = []
    for key in sorted(got):
        g, w = got[key], want[key]
        diff = []
        for field in ("workspace_bytes", "splitk", "num_streams"):
            if g[field] != w[field]:
                diff.append("  %s: %r, recorded %r" % (field, g[field], w[field]))
        if len(g["kernels"]) != len(w["kernels"]):
            diff.append("  %d kernels, recorded %d" % (len(g["kernels"]), len(w["kernels"])))
        for i, (a, b) in enumerate(zip(g["kernels"], w["kernels"])):
            if tuple(a) != tuple(b):
                diff.append("  kernel %d: %r\n  recorded  %r" % (i, tuple(a), tuple(b)))
        if diff:
            bad.append(key)
            print("plan %s differs from the record:\n%s" % (key, "\n".join(diff)))
    assert not bad, "%d plan(s) differ from the record (lines above): %s" % (len(bad), ", ".join(bad))


def test_grid_reaches_every_arm():
    """Every arm of the per-launch decision occurs in at least one recorded name."""
    names = {k[0] for rec in got_plans().values() for k in rec["kernels"]}
    arms = {
        "pair on the image-aligned 128x192 tile": lambda n: ",128x192,tap9,img,x2>" in n and "+pairK" in n,
        "pair on the 128x256 tile": lambda n: ",128x256,tap9,x2>" in n and "+pairK" in n,
        "pair on the 128x128 tile": lambda n: ",128x128,tap9,x2>" in n and "+pairK" in n,
        "split-K inside the launch": lambda n: re.search(r"\+splitK\d+,1launch$", n),
        "split-K with a reduce launch, more than 8 splits": lambda n: (lambda m: m and int(m.group(1)) > 8)(re.search(r"\+splitK(\d+)$", n)),
        "back-to-back 1x1": lambda n: "+1x1" in n,
        "1x1 computed by the conv in front": lambda n: "fused into the conv in front" in n,
        "fused max-pool": lambda n: "+pool" in n,
        "float32 as nine bf16 products": lambda n: n.startswith("conv_igemm_emu"),
        "MXFP8 kernel": lambda n: n.startswith("conv_mx"),
        "4-wave kernel with split-K": lambda n: n.startswith("conv_igemm<") and "+splitK" in n,
    }
    missing = [what for what, hit in arms.items() if not any(hit(n) for n in names)]
    assert not missing, missing


CONV_KERNEL = re.compile(r"void yolo::(?:conv3x3_tap_kernel|conv3x3_tap_stream_kernel|conv_igemm_dma_kernel)<[^>]*>\(yolo::ConvParams\)")
_G = "generic-epilogue fp16 form: every pinned fp16 launch of this tile has the plain, aligned output map the lean form takes"
_F = "float32 form of a tile without float32 support (built with every tile, refused by the launcher)"
# instantiations in the library that no recorded plan runs, with the reason (from the record itself: a new or a lost instantiation shows up here)
UNREACHED = {
    "conv3x3_tap_kernel<false, 2, 4, 4, 4, 26, 4, 1, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 2, 4, 8, 4, 26, 2, 1, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 2, 4, 4, 3, 26, 4, 1, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 2, 4, 4, 2, 28, 4, 1, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 2, 4, 4, 4, 27, 4, 2, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 4, 2, 4, 7, 17, 2, 1, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 2, 4, 4, 2, 12, 6, 2, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 2, 4, 4, 6, 27, 2, 1, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 2, 4, 4, 6, 26, 2, 4, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 2, 4, 4, 3, 14, 4, 1, false, false, false>": _G,
    "conv3x3_tap_kernel<false, 1, 8, 4, 2, 27, 4, 2, false, false, false>": "fp16 64-cout 2-D tile, generic: the pinned launches take its persistent form",
    "conv3x3_tap_kernel<false, 1, 8, 4, 2, 27, 4, 2, false, true, false>": "fp16 64-cout 2-D tile, lean: the pinned launches take its persistent form",
    "conv3x3_tap_kernel<false, 1, 8, 2, 2, 27, 4, 2, false, false, false>": "fp16 form of the 32-cout tile: no pinned fp16 net has a 3x3 conv of 17-32 filters on 32+ channels",
    "conv3x3_tap_kernel<false, 1, 8, 2, 2, 27, 4, 2, false, true, false>": "fp16 form of the 32-cout tile (lean)",
    "conv3x3_tap_kernel<false, 1, 8, 2, 2, 27, 4, 3, false, false, false>": "fp16 form of the 32-cout tile (fused pool)",
    "conv3x3_tap_kernel<true, 1, 8, 2, 2, 27, 4, 2, false, false, false>": "float32 32-cout tile without the pool: its one pinned layer (tiny-YOLOv2 16 -> 32) runs the fused-pool form",
    "conv3x3_tap_kernel<false, 2, 4, 4, 4, 21, 4, 4, false, true, false>": "lean form of the two-per-CU stride-2 tile: spills, the launcher runs the generic one",
    "conv3x3_tap_kernel<false, 2, 4, 4, 4, 26, 4, 4, false, true, false>": "lean form of the wide stride-2 tile without the 1x1: the launcher runs the generic one",
    "conv3x3_tap_kernel<true, 2, 4, 4, 4, 26, 4, 1, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 8, 4, 26, 2, 1, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 4, 3, 26, 4, 1, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 4, 4, 27, 4, 2, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 4, 2, 4, 7, 17, 2, 1, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 4, 2, 12, 6, 2, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 4, 6, 27, 2, 1, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 4, 4, 21, 4, 4, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 4, 6, 26, 2, 4, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 4, 3, 14, 4, 1, false, false, false>": _F,
    "conv3x3_tap_kernel<true, 2, 4, 4, 4, 26, 4, 4, false, false, false>": _F,
    "conv_igemm_dma_kernel<1, 8, 4, 4, 2, 4, 4, false, 2>": "float32 head rows on the 64 x 512 tile: no head conv has 64 filters or fewer",
}


def test_every_instantiation_is_reachable_and_every_report_is_real():
    """The conv kernels the library exports (nm -DC) against the symbols of the recorded plans: a reported symbol is a kernel that
    exists, and every kernel that exists runs in some recorded plan or is listed in UNREACHED with its reason."""
    import subprocess
    nm = subprocess.run(["nm", "-DC", _hip.LIB_PATH], check=True, capture_output=True, text=True).stdout
    built = {m.group(0) for line in nm.splitlines() if "__device_stub__" not in line for m in [CONV_KERNEL.search(line)] if m}
    assert len(built) > 50, "no conv kernels found in nm -DC of %s" % _hip.LIB_PATH
    with open(PLANS_JSON) as f:
        recorded = {s for s in json.load(f)["symbols"] if CONV_KERNEL.fullmatch(s)}
    assert recorded <= {k[2] for rec in got_plans().values() for k in rec["kernels"]}
    assert not recorded - built, "reported, but not in the library: %s" % sorted(recorded - built)
    listed = {"void yolo::%s(yolo::ConvParams)" % k for k in UNREACHED}
    assert built - recorded == listed, ("in the library, in no recorded plan and not listed: %s; listed but recorded or not built: %s"
                                        % (sorted(built - recorded - listed), sorted(listed - (built - recorded))))


if __name__ == "__main__":      # rewrite the record (no GPU needed)
    rec = pack(record_all())
    assert unpack(rec) == {k: dict(v, kernels=[tuple(x) for x in v["kernels"]]) for k, v in record_all().items()}
    with open(PLANS_JSON, "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d plans, %d distinct kernel lines recorded in %s (%d bytes) from %s"
          % (len(rec["plans"]), len(rec["lines"]), PLANS_JSON, os.path.getsize(PLANS_JSON), _hip.LIB_PATH))

"""CPU: the cases of tests/large_cases.py are at and past the 2 GiB line -- by the library's own numbers.

The GPU cases of test_gpu_large.py are sized from ONE constant, 0x7ffffff0 bytes: conv_params (forward.cpp) refuses a conv whose input buffer
is larger; conv_shape_params (conv_dispatch.cpp) sets out_bytes / res_bytes to 0 for a larger output / residual, which turns the lean
epilogue off (conv_fast_epilogue_ok, tap_lean, the form choice of conv_dma.hip, launch_conv_mx); resolve_conv drops the back-to-back 1x1 for
a larger output of the 1x1.  Here, without a GPU and for every row: S (bytes per image of the tensor the row is about) is read from the
plan and must be what the table states from the shape; B_last = floor(0x7ffffff0 / S) and B_first = B_last + 1 follow; the plan at B_last
names the lean / fused kernel and the plan at B_first the generic / unfused one (yolo_kernel_info name and symbol, describe()).  A
change of the constant, or of a rule that reads it, fails here instead of quietly turning the GPU cases into ordinary ones
(test_rounds_cpu.py does the same for the grid caps).  Also per row: the kernel meant runs, a forced tile is valid for the shape, the
workspace views the GPU test reads exist and share bytes with nothing, and the peak device memory stays under 16 GiB.
"""
import ctypes as C

import numpy as np
import pytest

import helpers as Hp
import large_cases as LC
import test_gpu_exact as T
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine


def plan_of(c, side, batch=None):
    kw = LC.engine_kw(c, side)
    if batch is not None:
        kw["max_batch"] = batch
    p = engine.Plan(LC.build_graph(c), guard_bytes=4096, **kw)
    infos = [T._info(p, k, C, _hip) for k in range(p.num_kernels)]
    return p, infos


def tensor_bytes_per_image(c, p):
    """S of the tensor a row is about, from the plan alone"""
    ks = [k for k in Hp.plan_kernels(p) if k["layer"] == c["about"]]
    assert ks, (c["id"], p.describe())
    what = c["what"]
    if what == "in":
        return Hp.view_image_bytes(p, ks[0]["in"])
    if what == "out":
        return Hp.view_image_bytes(p, Hp.layer_view(p, c["about"]))
    if what == "res":           # the residual of the fused shortcut: the tensor of the shortcut's other source
        g = engine.number_layers(LC.build_graph(c))
        conv, other = (s.index for s in g[c["about"]].inputs)
        return Hp.view_image_bytes(p, Hp.layer_view(p, other))
    if what == "out2":          # the output of the 1x1 behind the conv
        return Hp.view_image_bytes(p, Hp.layer_view(p, c["about"] + 1))
    if what == "final":
        return p.output_count * 4
    assert what == "user_in", what
    return int(np.prod(p.input_hwc)) * 4


def peak_bytes(c, p, batch):
    """what test_gpu_large.run_case holds at its peak: workspace, weights, records, the batch, the output, D inputs / expected tensors and the
    comparison's chunks"""
    x_bytes = batch * int(np.prod(p.input_hwc)) * (1 if c["u8"] else 4)
    out_bytes = batch * p.output_count * 4
    from tensorflow_yolo_amd.net import dist as ydist
    records = ydist.record_words(p.max_batch, p.max_boxes) * 4
    small = LC.D * (int(np.prod(p.input_hwc)) * 4 + p.output_count * 4)
    return max(p.workspace_bytes, 256) + max(p.weights_bytes, 256) + records + x_bytes + out_bytes + small + LC.COMPARE_BYTES


@pytest.mark.parametrize("cid", [c["id"] for c in LC.CASES])
def test_sizes_and_kernels_on_both_sides_of_the_line(cid):
    c = [c for c in LC.CASES if c["id"] == cid][0]
    S = None
    for side in c["sides"]:
        B = LC.batch_of(c, side)
        p, infos = plan_of(c, side)
        s_plan = tensor_bytes_per_image(c, p) if side != "parts2" else S         # (two arenas: a buffer holds its part's images only)
        assert s_plan == c["S"], "%s/%s: the plan says %d bytes per image, the table %d" % (cid, side, s_plan, c["S"])
        S = s_plan
        b_last = LC.LIMIT // S
        assert b_last * S <= LC.LIMIT < (b_last + 1) * S and S & (S - 1) != 0, (cid, S)
        assert B == {"last": b_last, "first": b_last + 1, "refuse": b_last + 1, "parts2": b_last + 1, "past4g": (1 << 32) // S + 1}[side]
        if side == "past4g":
            assert B * S > 1 << 32 and (c["what"] != "out" or B * S // (4 if c["dtype"] == "fp32" else 2) > 1 << 31)
        name, sym = Hp.kernel_of_layer(infos, c["about"])
        want = c["kernel"].get(side, c["kernel"].get("last"))
        assert want in name + " " + sym, "%s/%s: layer %d runs %s [%s], not %s\n%s" % (cid, side, c["about"], name, sym, want, p.describe())
        text = T.kernel_text(p, infos)[1]
        for e in c["expect"]:
            assert e in text, (cid, side, e, p.describe())
        if c["tile"] is not None and c["tile"] > 0:          # a forced tile is valid for the shape: it is the one that runs
            assert T.TILE_NAME[c["tile"]] in name, (cid, c["tile"], name)
        assert p.num_streams == (2 if side == "parts2" else 1)
        for r in c["read"]:                                 # the views the GPU test reads
            v = Hp.layer_view(p, r) if isinstance(r, int) else [k for k in Hp.plan_kernels(p) if k["layer"] == r[2]][0]["in"]
            assert v["buf"] >= 0 and Hp.buffer_is_alone(p, v["buf"]), "%s/%s: layer %r cannot be read through a view\n%s" % (cid, side, r, p.describe())
        peak = peak_bytes(c, p, B)
        assert peak <= LC.CAP_BYTES, "%s/%s: %.2f GiB at the peak" % (cid, side, peak / 2.0 ** 30)
        print("%s/%s: S = %d, batch %d, tensor %.3f GiB, peak %.2f GiB, layer %d: %s" % (cid, side, S, B, B * S / 2.0 ** 30, peak / 2.0 ** 30, c["about"], name))
    if "last" in c["sides"] and "first" in c["sides"]:
        assert c["kernel"]["last"] != c["kernel"]["first"] or c["what"] in ("final",) or "fused: " in " ".join(c["expect"]) or "+pool" in c["kernel"]["last"], \
            "%s: a row with both sides names what differs between them" % cid


def test_the_line_is_where_the_library_draws_it():
    """one byte-exact probe of each rule: the lean epilogue, the residual, the back-to-back 1x1 and the MX kernel flip between B_last and
    B_first and nowhere near (one image fewer / more changes nothing)"""
    for cid, flips in (("out-dma-1x1", True), ("out-tap2d-128x256", True), ("out-mx", True), ("res-slice", True), ("fuse2-slice", True)):
        c = [c for c in LC.CASES if c["id"] == cid][0]
        b_last = LC.LIMIT // c["S"]
        names = {}
        for b in (b_last - 1, b_last, b_last + 1, b_last + 2):
            p, infos = plan_of(c, "last", batch=b)
            names[b] = Hp.kernel_of_layer(infos, c["about"])
        assert names[b_last - 1] == names[b_last] and names[b_last + 1] == names[b_last + 2], (cid, names)
        assert (names[b_last] != names[b_last + 1]) == flips, (cid, names)
        assert c["kernel"]["last"] in " ".join(names[b_last]) and c["kernel"]["first"] in " ".join(names[b_last + 1]), (cid, names)


def test_the_back_to_back_pair_is_one_launch_below_and_two_above():
    c = [c for c in LC.CASES if c["id"] == "fuse2-slice"][0]
    p, infos = plan_of(c, "last")
    names = [ki.name.decode() for ki in infos]
    assert "conv_igemm<fused into the conv in front>" in names and any(n.endswith("+1x1") for n in names), names
    assert sum(1 for ki in infos if ki.kind == infos[1].kind and ki.symbol) == 2, names        # the 3x3 (+ 1x1) and the 192-channel 1x1
    # the 3x3 keeps its buffer-addressed epilogue: the fused instantiation is the lean one (conv_tap.hip: tap_form)
    assert "false, true, true>" in Hp.kernel_of_layer(infos, 1)[1]
    p, infos = plan_of(c, "first")
    names = [ki.name.decode() for ki in infos]
    assert "conv_igemm<fused into the conv in front>" not in names and not any("+1x1" in n for n in names), names
    assert sum(1 for ki in infos if ki.kind == infos[1].kind and ki.symbol) == 3, names
    assert "computed by the conv in front of it" in p.describe()          # (still marked by plan.cpp: the launch decides)


def test_the_table_covers_what_the_issue_lists():
    ids = {c["id"] for c in LC.CASES}
    for must in ("in-4wave-3x3", "in-4wave-3x3s2", "in-4wave-1x1", "in-dma-64x512", "in-tap-stream", "in-tap2d-32x256", "in-taps2-wide", "in-mx",
                 "in-f32-4wave", "in-f32-tap2d-32x256", "out-dma-1x1", "out-tap2d-128x256", "out-mx", "res-slice", "out-upsample", "out-reorg",
                 "out-pooled", "out-f32-last", "fuse2-slice", "prep-f32", "prep-u8", "move-add-vec", "move-add-scalar", "move-up", "move-reorg",
                 "move-pool2", "pool-same-scalar", "spp", "first", "first-pool-mfma", "first-pool-mfma-f32", "stem-out3"):
        assert must in ids, must
    sides = [s for c in LC.CASES for s in c["sides"]]
    assert sides.count("refuse") == 2 and {c["dtype"] for c in LC.CASES if "refuse" in c["sides"]} == {"fp16", "fp32"}
    assert sides.count("parts2") == 1 and sides.count("past4g") >= 3
    assert LC.D % 2 == 1 and (1 << 31) % LC.D and (1 << 32) % LC.D


@pytest.mark.parametrize("cid", [c["id"] for c in LC.CASES if c["what"] == "in" and c["part"] == 1])
def test_input_cases_end_within_one_image_of_the_line_with_a_ragged_tail(cid):
    """part 1: the last image's offsets end within S of 2^31; the M tail and padding taps fall into the last image"""
    c = [c for c in LC.CASES if c["id"] == cid][0]
    B, S = LC.batch_of(c, "last"), c["S"]
    assert (1 << 31) - S < B * S <= LC.LIMIT
    name, args = c["graph"]
    h, w, k, s = args[0], args[1], args[4], args[5]
    ho, wo = -(-h // s), -(-w // s)
    assert (B * ho * wo) % 256 and (B * ho * wo) % 128 and ho % 16 and wo % 16, "no ragged tile at the end of M"
    assert k == 3 or "1x1" in cid or "dma" in cid


def test_the_harness_sees_one_wrong_element():
    """helpers.large_difference on the CPU (the same code the GPU test runs): a strided view with one flipped bit in the last image is
    reported as exactly that element, its offset as computed from the view's strides; an untouched tensor gives None"""
    import torch
    rng = np.random.RandomState(5)
    want = rng.randint(-2048, 2049, (LC.D, 5, 7, 12)).astype(np.float32)
    buf = torch.full((11, 5 * 7 * 16 + 24), float("nan"), dtype=torch.float16)           # 11 images, ld 16, 24 elements of slack per image
    view = buf[:, :5 * 7 * 16].view(11, 5, 7, 16)[..., 4:16]
    view.copy_(torch.from_numpy(want)[torch.arange(11) % LC.D].to(torch.float16))
    assert Hp.large_difference(view, want) is None
    view.view(torch.int16)[10, 3, 2, 7] ^= 1
    d = Hp.large_difference(view, want)
    assert d["index"] == (10, 3, 2, 7) and d["differing"] == 1 and d["want"] == float(want[10 % LC.D, 3, 2, 7]) and d["got"] != d["want"], d
    where = dict(image_bytes=(5 * 7 * 16 + 24) * 2, ld=16, coff=4, esize=2, w=7)
    off = Hp.large_offset(d["index"], where, tuple(view.shape))
    assert off == (view[10, 3, 2, 7:].data_ptr() - buf.data_ptr())
    text = Hp.large_report(d, "case/layer 1", where, tuple(view.shape), ("name", "symbol"))
    assert "(10, 3, 2, 7)" in text and "byte offset %d " % off in text and "below 2^31" in text and "name [symbol]" in text, text
    assert "AT OR PAST 2^31" in Hp.large_report(dict(d, index=(1 << 21, 0, 0, 0)), "x", where, tuple(view.shape), ("n", "s"))
    # an element nothing wrote (NaN) differs, and so does -0 from 0
    view.view(torch.int16)[10, 3, 2, 7] ^= 1
    assert Hp.large_difference(view, want) is None
    buf2 = torch.zeros(3, 2, 2, 4)
    assert Hp.large_difference(buf2, np.zeros((3, 2, 2, 4), np.float32)) is None
    buf2[2, 1, 1, 3] = -0.0
    assert Hp.large_difference(buf2, np.zeros((3, 2, 2, 4), np.float32))["index"] == (2, 1, 1, 3)
    # a dense float32 tensor: the offset is the linear index times four
    assert Hp.large_offset((2, 1, 1, 3), None, (3, 2, 2, 4)) == 47 * 4


@pytest.mark.parametrize("cid", [c["id"] for c in LC.CASES])
def test_references_hold_their_preconditions(cid):
    """exact_ref.check_preconditions for every conv row (inside large_cases.reference) and D distinct expected outputs"""
    c = [c for c in LC.CASES if c["id"] == cid][0]
    stream, x, out, kept, rep = LC.reference(c)
    assert x.shape[0] == LC.D and out.shape[0] == LC.D
    p, _ = plan_of(c, c["sides"][0], batch=LC.D)
    assert stream.size == p.weight_count and tuple(out.shape[1:]) == tuple(p.output_shape), (cid, stream.size, p.weight_count, out.shape)
    for r in c["read"]:                 # the view the GPU test reads has the shape of what it is compared with
        v = Hp.layer_view(p, r) if isinstance(r, int) else [k for k in Hp.plan_kernels(p) if k["layer"] == r[2]][0]["in"]
        want = kept[r if isinstance(r, int) else r[0]]
        assert (v["h"], v["w"], v["c"]) == tuple(want.shape[1:]), (cid, r, v, want.shape)


def test_the_largest_batch_of_yolov3_608():
    """what DESIGN.md section 2 and INTEGRATION.md state: the largest conv INPUT buffer of YOLOv3-608 per image, and the largest batch one part
    can run -- 181 in fp16 (the 304 x 304 x 64 tensor the stem writes and the stride-2 conv reads: 11 829 248 bytes), 45 in float32 (the
    608 x 608 x 32 tensor of the first conv: 47 316 992 bytes).  The stem kernel reads the caller's tensor and is not a conv_params launch."""
    import poison_cases as P
    from oracle import cases
    from tensorflow_yolo_amd import YoloV3
    net = YoloV3.create_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), P.NAMES80, False, input_shape=(608, 608, 3))
    for dtype, s_want, b_want in (("fp16", 304 * 304 * 64 * 2, 181), ("fp32", 608 * 608 * 32 * 4, 45)):
        p = engine.Plan(net, dtype=dtype, max_batch=2, streams=1)
        infos = [T._info(p, k, C, _hip) for k in range(p.num_kernels)]
        S = max(k["in"]["h"] * k["in"]["w"] * k["in"]["ld"] * Hp.view_esize(p, k["in"]) for k, ki in zip(Hp.plan_kernels(p), infos)
                if k["kind"] == "conv" and ki.symbol and b"conv_stem" not in ki.name)
        assert S == s_want and LC.LIMIT // S == b_want, (dtype, S, LC.LIMIT // S)

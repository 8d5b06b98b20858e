"""GPU: every forward kernel on tensors at and past the 2 GiB line (the table: tests/large_cases.py; its sizes and kernels are held against
the plan, without a GPU, by tests/test_large_cpu.py).

Method.  Integer-exact data (tests/exact_ref.py: make_case, forward_exact, check_preconditions asserted) for D = 3 DISTINCT images; the D
expected outputs come from the float64 integer reference on the CPU.  Image n of the batch is distinct image n mod D, gathered on the
device.  The comparison runs on the device, in chunks, over the WHOLE tensor: element (n, y, x, c) must equal expected[n mod D](y, x, c) bit
for bit (helpers.large_difference: torch.equal on integer views, no tolerance anywhere).  The final float32 output is read from the caller's
tensor; a tensor in the workspace through a typed view of the engine's workspace, placed by workspace_regions() and the plan's description.
Before the pass the whole workspace and the output tensor hold 0xFF bytes (helpers.poison_and_bind(eng, "ones")): an element nothing wrote is
NaN and fails.  Plans carry 4096 guard bytes behind every tensor; every byte no region claims must still be 0xFF after the pass.  A failed
comparison names the case and layer, the first differing element (image, y, x, channel), its byte offset inside the tensor, whether that
is at or past 2^31 and 2^32, and the kernel's name and symbol.

Device memory: one engine at a time, freed (with torch.cuda.empty_cache()) before a test returns; the peak of every test is below 16 GiB
(test_large_cpu.py computes it per case: workspace + weights + batch + output + the comparison's chunks; the largest is 13.4 GiB).
"""
import gc

import pytest

import helpers as Hp
import large_cases as LC
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine

pytestmark = pytest.mark.gpu

GUARD = 4096


def free():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def make_engine(c, side):
    """the engine of a row at one side on memory nobody zeroed: weights loaded, the whole workspace 0xFF, bound"""
    import torch
    stream = LC.reference(c)[0]
    eng = engine.HipNetwork(LC.build_graph(c), guard_bytes=GUARD, **LC.engine_kw(c, side))
    if eng.weight_count:
        eng.load_weights(stream)
    else:
        eng.weights_loaded = True
    Hp.poison_and_bind(eng, "ones")
    torch.cuda.synchronize()
    return eng


def check_kernels(c, side, eng):
    infos = eng.kernel_infos()
    name, sym = Hp.kernel_of_layer(infos, c["about"])
    want = c["kernel"].get(side, c["kernel"].get("last"))
    assert want in name + " " + sym, "%s/%s: layer %d ran %s [%s], not %s" % (c["id"], side, c["about"], name, sym, want)
    return infos


def forward(c, eng, batch):
    """one pass of `batch` images (image n = distinct image n mod D) into an output tensor full of 0xFF -> (the batch, the output)"""
    xb = Hp.large_batch(LC.reference(c)[1], batch)
    out = Hp.poisoned_out(eng, batch)
    (eng.forward_u8 if c["u8"] else eng.forward)(xb, out=out)
    eng.torch.cuda.synchronize()
    return xb, out


def compare_all(c, side, eng, out, batch, infos):
    """the caller's tensor and every workspace tensor the row reads, whole, bit for bit"""
    _, _, want, kept, _ = LC.reference(c)
    last = len(eng.layers) - 1
    what = "%s/%s (batch %d)" % (c["id"], side, batch)
    Hp.assert_large_equal(out.view((batch,) + tuple(want.shape[1:])), want, what + " final output (layer %d)" % last, None, Hp.kernel_of_layer(infos, last))
    for r in c["read"]:
        if isinstance(r, int):
            t, where = Hp.layer_tensor(eng, r, batch)
            Hp.assert_large_equal(t, kept[r], what + " layer %d" % r, where, Hp.kernel_of_layer(infos, r))
        else:                       # the whole concat buffer of route r[0], as the kernel of layer r[2] reads it
            t, where = Hp.layer_tensor(eng, r[2], batch, side="in")
            Hp.assert_large_equal(t, kept[r[0]], what + " layer %d (concat buffer)" % r[0], where, Hp.kernel_of_layer(infos, r[2]))
    assert Hp.assert_slack_intact(eng, 0xFF, what) >= GUARD, "nothing to check"


def run_case(c, side):
    batch = LC.batch_of(c, side)
    eng = make_engine(c, side)
    try:
        infos = check_kernels(c, side, eng)
        xb, out = forward(c, eng, batch)
        compare_all(c, side, eng, out, batch, infos)
    finally:
        eng.close()


RUN_IDS = ["%s-%s" % (c["id"], s) for c in LC.CASES for s in c["sides"] if s in ("last", "first", "past4g")]


@pytest.mark.parametrize("cid", RUN_IDS)
def test_large(cid):
    """One pass at a batch at, just past or far past the 2 GiB line; every tensor the row names equals the reference bit for bit.
    Peak device memory: below 13.4 GiB (per case: test_large_cpu.py prints it)."""
    c, side = LC.find(cid)
    try:
        run_case(c, side)
    finally:
        free()


@pytest.mark.parametrize("cid", ["%s-refuse" % c["id"] for c in LC.CASES if "refuse" in c["sides"]])
def test_input_past_the_line_is_refused(cid):
    """A conv input of more than 0x7ffffff0 bytes: forward fails with YOLO_ERR_ARG and the "exceeds 2 GiB" message (the Python binding raises
    it), the output tensor keeps its 0xFF fill, and the same engine then runs batch D and equals the reference bit for bit (forward_failed:
    the counters are cleared).  Peak device memory: 11.4 GiB."""
    import torch
    c, side = LC.find(cid)
    batch = LC.batch_of(c, side)
    eng = make_engine(c, side)
    try:
        infos = check_kernels(c, side, eng)
        xb = Hp.large_batch(LC.reference(c)[1], batch)
        out = Hp.poisoned_out(eng, batch)
        with pytest.raises(_hip.YoloHipError) as e:
            eng.forward(xb, out=out)
        torch.cuda.synchronize()
        assert "status 1" in str(e.value) and "conv input tensor exceeds 2 GiB" in str(e.value) and "lower the batch" in str(e.value), str(e.value)
        flat = out.view(torch.int32).view(-1)
        for a in range(0, flat.numel(), 1 << 28):
            assert torch.equal(flat[a:a + (1 << 28)], torch.full_like(flat[a:a + (1 << 28)], -1)), "the refused pass wrote into the output tensor"
        del xb, out, flat
        free()
        xb, out = forward(c, eng, LC.D)
        compare_all(c, "after the refusal", eng, out, LC.D, infos)
    finally:
        eng.close()
        free()


def test_two_parts_take_the_refused_batch():
    """The batch one pass refuses (in-4wave-3x3 at B_first = 501) on two streams: each part holds half of it in its own arena, no conv
    input reaches the line, the pass runs and equals the reference.  Peak device memory: 10.9 GiB."""
    c, side = LC.find("in-4wave-3x3-parts2")
    batch = LC.batch_of(c, side)
    eng = make_engine(c, side)
    try:
        assert eng.num_streams == 2
        infos = check_kernels(c, side, eng)
        xb, out = forward(c, eng, batch)
        _, _, want, _, _ = LC.reference(c)
        Hp.assert_large_equal(out.view((batch,) + tuple(want.shape[1:])), want, "%s (batch %d, two parts) final output" % (c["id"], batch), None,
                              Hp.kernel_of_layer(infos, len(eng.layers) - 1))
        assert Hp.assert_slack_intact(eng, 0xFF, c["id"]) >= GUARD
    finally:
        eng.close()
        free()


def test_the_comparison_reports_exactly_the_element_that_was_changed():
    """HARNESS MUTATION (nothing in the library is mutated): after a correct pass of out-dma-1x1 at 251 images (a 4.01 GiB fp16 tensor), one bit of one
    element of the conv's output is flipped on the device; the comparison must name exactly that image,
    position and byte offset -- once just behind 2^31, once in the last image behind 2^32 --, and a flip in the caller's float32 tensor likewise.  Peak device memory: 12.9 GiB."""
    import torch
    c, side = LC.find("out-dma-1x1-past4g")
    batch = LC.batch_of(c, side)
    eng = make_engine(c, side)
    try:
        infos = check_kernels(c, side, eng)
        xb, out = forward(c, eng, batch)
        compare_all(c, side, eng, out, batch, infos)
        _, _, want, kept, _ = LC.reference(c)
        t, where = Hp.layer_tensor(eng, 1, batch)
        # the first image that lies wholly behind byte 2^31, and the last image (behind 2^32)
        for n, (y, x, ch) in (((1 << 31) // where["image_bytes"] + 1, (100, 7, 5)), (batch - 1, (LC.H - 1, LC.W - 1, 127))):
            off = Hp.large_offset((n, y, x, ch), where, tuple(t.shape))
            assert off >= 1 << 31 and (n != batch - 1 or off >= 1 << 32), off
            t.view(torch.int16)[n, y, x, ch] ^= 1
            d = Hp.large_difference(t, kept[1])
            assert d is not None and d["index"] == (n, y, x, ch) and d["differing"] == 1 and d["want"] == float(kept[1][n % LC.D, y, x, ch]), d
            text = Hp.large_report(d, "mutation", where, tuple(t.shape), Hp.kernel_of_layer(infos, 1))
            assert "(%d, %d, %d, %d)" % (n, y, x, ch) in text and "byte offset %d " % off in text and "AT OR PAST 2^31" in text, text
            assert ("AT OR PAST 2^32" in text) == (off >= 1 << 32) and "conv_igemm_dma_kernel<2, 4, 4, 4, 3, 4, 4, false, 0>" in text, text
            with pytest.raises(AssertionError):
                Hp.assert_large_equal(t, kept[1], "mutation", where, Hp.kernel_of_layer(infos, 1))
            t.view(torch.int16)[n, y, x, ch] ^= 1
            assert Hp.large_difference(t, kept[1]) is None
        # the caller's float32 tensor (dense): the last element of the last image
        o = out.view((batch,) + tuple(want.shape[1:]))
        idx = (batch - 1,) + tuple(v - 1 for v in want.shape[1:])
        o.view(torch.int32)[idx] ^= 1
        d = Hp.large_difference(o, want)
        assert d is not None and d["index"] == idx and d["differing"] == 1, d
        assert "byte offset %d " % (o.numel() * 4 - 4) in Hp.large_report(d, "mutation", None, tuple(o.shape), ("n", "s"))
    finally:
        eng.close()
        free()

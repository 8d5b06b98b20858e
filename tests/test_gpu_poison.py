"""GPU: results must not depend on what the workspace held.

INTEGRATION.md tells a C-ABI caller that the workspace "need not be zeroed: the library clears what it counts on"; engine.HipNetwork
allocates torch.zeros, so every other GPU test starts from a workspace of zero bytes and, after its first pass, from stale FINITE data.
A kernel that reads bytes no earlier kernel of the pass wrote -- K padding, padded input channels, a neighbouring concat slice, positions
and images behind the batch, split-K slab columns, skipped head rows, the compact objectness array, NMS scratch, LDS planes filled from
global memory, the pad rows of the weight buffer -- is harmless there: stale operand x zero weight = 0.  Here the whole workspace is filled
first (tests/helpers.py: "ones" = every byte 0xFF, NaN in every float format and -1 as an integer; "inf" = +inf of the plan's storage
type, which wins every max and is 2.66e36 where an fp16 plan keeps float32), the weight buffer is filled with 0xFF before the weights are
loaded, the workspace is bound as the contract says, and the caller's output tensor is 0xFF as well.  One NaN anywhere breaks equality.

a. test_exact_on_a_poisoned_workspace: every case of tests/test_gpu_exact.py (the same list, graphs, data, variants, options, forced
   tiles, kernel assertions and integer reference), per variant with "ones", with "inf", and with "ones" at one image fewer than
   max_batch (the last image's slots stay poisoned beside the work).  No tolerance: test_gpu_exact.assert_equal.
b. whole plans (tests/poison_cases.py; tests/test_poison_cpu.py holds what each row is in the table for): a poisoned twin equals a
   zeroed twin bit for bit on real values -- forward, forward_u8, detect, detect_frames, loss, loss_grad.  Equality of twins measures
   nothing against the code under test; that the zeroed twin is right is the job of the other tests.

The sensitivity tests show that the poison lies under every tensor: before the pass every readable layer of a keep_all engine is all-NaN
/ all-inf, after it none holds a non-finite value.  The harness's own mutation: an output tensor left poisoned behind a one-image-smaller
batch is reported.

How to read a failure.  With keep_all the layers are compared in graph order BEFORE the output, so the message names the FIRST layer that
differs: the kernel that wrote it (yolo_net_describe, printed with the message, maps layers to kernels) is the one that read poison.  A
`rounds-*` case adds the tile (image, tile row, tile column) of the first differing element and whether its workgroup was past its first
tile (test_gpu_exact.where_in_rounds).  NaN in the output behind "ones" and a huge or infinite value behind "inf" is a read of memory
nothing wrote; NaN behind BOTH in an element whose neighbours are right is an element nothing wrote (the output tensor's own 0xFF).
A case that fails only at the smaller batch read an image behind the batch.  The fix belongs where the cause is -- an exact extent, a
masked lane, a written pad, a clear at bind -- never a torch.zeros in the caller."""
import numpy as np
import pytest

import poison_cases as P
import test_gpu_exact as E
from helpers import POISONS, forward_poisoned, poison_and_bind, poisoned_out, run_hip_poisoned
from tensorflow_yolo_amd import YoloV2Tiny, _hip
from tensorflow_yolo_amd.net import evaluate as yeval, synth, v3

pytestmark = pytest.mark.gpu


# ---- a. every exact case ------------------------------------------------------------------------------------------------------------
def check_exact(c, eng, got, want, kept, n_layers, batch, what, rounds):
    """layers in graph order first (keep_all), then the output: the first assertion that fails names the first layer that differs"""
    if c["keep_all"]:
        for i in range(1, n_layers - 1):        # (the last layer lives in the caller's tensor: it is `got`)
            E.assert_equal(eng.read_layer(i, batch), kept[i][:batch], what + " layer %d (the FIRST that differs)\n%s" % (i, eng.describe()),
                           rounds and dict(rounds, tile=None), batch)
    E.assert_equal(got, want[:batch], what, rounds, batch)


@pytest.mark.parametrize("cid", E.IDS)
def test_exact_on_a_poisoned_workspace(cid):
    c = E.CASES[E.IDS.index(cid)]
    E.case_report(c)                                # reference and data only: before anything touches the GPU
    rounds = E.ROUNDS.get(cid)
    B = c["B"]
    for variant in c["variants"]:
        L, d, want, kept, rep = E.reference(c, variant)
        g = E.build_graph(c, variant)
        kw = dict(c["kw"])
        tune = kw.pop("autotune", False)
        got, eng = run_hip_poisoned(g, d["stream"], d["x"], c["dtype"], "ones", keep_all=c["keep_all"], force_tile=c["tile"], **kw)
        names, text = E.kernel_text(eng, eng.kernel_infos())
        E.check_kernels(c, variant, eng, names, text)
        what = "%s/%s %s" % (cid, variant, names)
        check_exact(c, eng, got, want, kept, len(L), B, what + " on 0xFF", rounds)
        check_exact(c, eng, forward_poisoned(eng, d["x"], "inf"), want, kept, len(L), B, what + " on +inf", rounds)
        if B > 1:
            check_exact(c, eng, forward_poisoned(eng, d["x"][:B - 1], "ones"), want, kept, len(L), B - 1, what + " on 0xFF at batch %d" % (B - 1), rounds)
        if tune:
            eng.autotune(d["x"])
            check_exact(c, eng, forward_poisoned(eng, d["x"], "ones"), want, kept, len(L), B, what + " on 0xFF after autotune", rounds)


def readable_layers(eng, batch):
    """{layer: float32 copy} of every layer read_layer serves (a fused-away layer and one in a caller's tensor are refused)"""
    out = {}
    for i in range(len(eng.layers)):
        try:
            out[i] = eng.read_layer(i, batch)
        except _hip.YoloHipError:
            pass
    return out


def assert_poison_under_every_layer(eng, batch, poison):
    layers = readable_layers(eng, batch)
    assert layers, "no readable layer"
    for i, a in layers.items():
        ok = np.isnan(a).all() if poison == "ones" else (a == np.inf).all()
        assert ok, "layer %d does not lie on the poison %r before the pass" % (i, poison)
    return sorted(layers)


def assert_all_finite(eng, batch, out):
    assert np.isfinite(out).all(), "the output holds a non-finite value"
    for i, a in readable_layers(eng, batch).items():
        assert np.isfinite(a).all(), "layer %d holds a non-finite value after the pass" % i


KEEP_ALL_IDS = [i for i in E.IDS if E.CASES[E.IDS.index(i)]["keep_all"] and i not in E.ROUNDS]


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("cid", KEEP_ALL_IDS)
def test_sensitivity_exact_graphs(cid, poison):
    """the poison lies under every layer test_exact reads, and the pass leaves none of it"""
    c = E.CASES[E.IDS.index(cid)]
    L, d, want, kept, rep = E.reference(c, None)
    seen = []
    got, eng = run_hip_poisoned(E.build_graph(c, None), d["stream"], d["x"], c["dtype"], poison, keep_all=True,
                                before_pass=lambda e: seen.extend(assert_poison_under_every_layer(e, c["B"], poison)))
    assert set(range(1, len(L) - 1)) <= set(seen), (seen, len(L))
    assert_all_finite(eng, c["B"], got)
    print("%s %s: layers %s all poison before the pass, all finite after it" % (cid, poison, seen))


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("pid", ["v3-tiny-fp16-keep_all", "v3-tiny-fp32-keep_all"])
def test_sensitivity_whole_net(pid, poison):
    p = P.PLANS[pid]
    net = P.create_network(p["net"])
    w = P.weights_of(p["net"])
    h, wd = P.NETS[p["net"]][3]
    x = synth.synthetic_input(P.MAX_BATCH, h, wd, 3, seed=43)
    seen = []
    got, eng = run_hip_poisoned(net, w, x, p["dtype"], poison, keep_all=True, streams=1,
                                before_pass=lambda e: seen.extend(assert_poison_under_every_layer(e, P.MAX_BATCH, poison)))
    convs = [l.index for l in net if type(l).__name__ == "conv2d_bn_act" and l.batch_norm]
    # (a conv whose upsample is fused into its epilogue is stored as the upsample's layer: then that one is read)
    lost = [i for i in convs if i not in seen and not any(l.index in seen for l in net if any(s.index == i for s in l.inputs))]
    assert not lost, "a batch-normalised conv of a keep_all plan is readable neither itself nor as the layer fused behind it: %s of %s" % (lost, seen)
    assert_all_finite(eng, P.MAX_BATCH, got)
    assert np.any(got != 0)
    print("%s %s: %d of %d layers readable, all poison before the pass, all finite after it" % (pid, poison, len(seen), len(net)))


def test_harness_reports_an_image_the_pass_did_not_write():
    """the mutation of the harness itself (test side only): the output tensor of B images stays poisoned and the pass gets B - 1 images,
    so one image of the result is what the tensor held.  The comparison must say so, and must say nothing about the images written."""
    c = E.CASES[E.IDS.index("fallback-kernels-fp16")]
    L, d, want, kept, rep = E.reference(c, None)
    B = c["B"]
    assert B > 1
    got, eng = run_hip_poisoned(E.build_graph(c, None), d["stream"], d["x"], c["dtype"], "ones", keep_all=True)
    E.assert_equal(got, want, "control")
    poison_and_bind(eng, "ones")
    out = poisoned_out(eng, B)
    eng.forward(d["x"][:B - 1], out=out[:B - 1])
    got = out.cpu().numpy()
    E.assert_equal(got[:B - 1], want[:B - 1], "the images of the pass")
    assert np.isnan(got[B - 1]).all()
    with pytest.raises(AssertionError, match="%d of %d elements differ" % (want[B - 1].size, want.size)):
        E.assert_equal(got, want, "mutation")


# ---- b. whole plans: a poisoned twin equals a zeroed twin ----------------------------------------------------------------------------
def twins(pid, w, **more):
    """(zeroed, poisoned): two models of one plan and one weight stream.  The first is left as constructed (a workspace of zero bytes); the
    second has its weight buffer filled with 0xFF before the weights are loaded, and is poisoned and bound before every pass."""
    import torch
    zero = P.build_model(pid, weights=w, **more)
    pois = P.build_model(pid, **more)
    pois.net.engine._weights.fill_(0xFF)
    torch.cuda.synchronize()
    v3.attach_weights(pois.net, w)
    return zero, pois


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    a, b = got.view(np.uint8), want.view(np.uint8)
    if np.array_equal(a, b):
        return
    bad = np.argwhere(got != want) if got.dtype.kind == "f" else np.argwhere(a != b)
    first = tuple(int(v) for v in bad[0]) if len(bad) else None
    raise AssertionError("%s: the poisoned twin differs from the zeroed twin in %d of %d elements, first at %s: %r vs %r"
                         % (what, len(bad), got.size, first, got[first] if first is not None else None, want[first] if first is not None else None))


def input_of(pid, batch, seed=44):
    h, w = P.NETS[P.PLANS[pid]["net"]][3]
    return synth.synthetic_input(batch, h, w, 3, seed=seed)


@pytest.mark.parametrize("pid", sorted(P.PLANS))
def test_whole_plan_forward(pid):
    p = P.PLANS[pid]
    zero, pois = twins(pid, P.weights_of(p["net"]))
    ze, pe = zero.net.engine, pois.net.engine
    assert ze.num_streams == pe.num_streams == p["kw"]["streams"]
    x = input_of(pid, max(p["batches"]))
    for b in p["batches"]:
        want = ze.forward(x[:b]).cpu().numpy()
        assert np.isfinite(want).all() and np.any(want != 0), "the zeroed twin's output must be finite and non-zero"
        kept = readable_layers(ze, b) if p["keep_all"] else {}
        for poison in POISONS:
            got = forward_poisoned(pe, x[:b], poison)
            what = "%s batch %d on %s" % (pid, b, poison)
            for i in sorted(kept):
                same_bits(pe.read_layer(i, b), kept[i], what + " layer %d (the FIRST that differs)" % i)
            same_bits(got, want, what)


@pytest.mark.parametrize("pid", ["v2-fp16-plan", "v3-fp16-plan"])
def test_whole_plan_forward_u8(pid):
    p = P.PLANS[pid]
    zero, pois = twins(pid, P.weights_of(p["net"]))
    h, w = P.NETS[p["net"]][3]
    x8 = np.random.RandomState(45).randint(0, 256, size=(P.MAX_BATCH, h, w, 3)).astype(np.uint8)
    for b in p["batches"]:
        want = zero.net.engine.forward_u8(x8[:b]).cpu().numpy()
        assert np.isfinite(want).all() and np.any(want != 0)
        for poison in POISONS:
            same_bits(forward_poisoned(pois.net.engine, x8[:b], poison, u8=True), want, "%s forward_u8 batch %d on %s" % (pid, b, poison))


def records(result):
    """(boxes, counts, status) device views of the engine's record buffer -> host copies"""
    return tuple(t.cpu().numpy().copy() for t in result)


def same_records(got, want, what):
    """counts, status and the first `count` records of every image"""
    (gb, gc, gs), (wb, wc, ws) = got, want
    assert np.array_equal(gc, wc), (what, "counts", gc, wc)
    assert np.array_equal(gs, ws), (what, "status", gs, ws)
    for i, n in enumerate(wc):
        same_bits(gb[i, :n], wb[i, :n], "%s image %d: its %d records" % (what, i, n))
    return int(wc.sum())


def calibrated_twins(pid, factor, **more):
    """twins on weights whose objectness biases are re-centred on the test's own input, as the detect tests do (synth.calibrate_model)"""
    p = P.PLANS[pid]
    cls = P.NETS[p["net"]][0]
    x = input_of(pid, P.MAX_BATCH)
    model = P.build_model(pid, weights=P.weights_of(p["net"]), **more)
    w = synth.calibrate_model(model, x, factor * synth.HEAD_DEFAULTS[cls.version][1])
    return twins(pid, w, **more) + (x,)


@pytest.mark.parametrize("pid", ["v3-fp16-plan", "v2-fp16-plan"])
def test_whole_plan_detect(pid):
    zero, pois, x = calibrated_twins(pid, 8 if pid.startswith("v3") else 1, max_boxes=1024)
    ze, pe = zero.net.engine, pois.net.engine
    total = 0
    for thr in (0.5, 0.05):
        want = records(ze.detect(x, thr, 0.6))
        for poison in POISONS:
            poison_and_bind(pe, poison)
            total += same_records(records(pe.detect(x, thr, 0.6)), want, "%s detect(%g) on %s" % (pid, thr, poison))
    assert total > 0, "no box anywhere: the fixture detects nothing"
    # ONE poison + bind, then a batch of two and a batch of three: the third image's counter and candidate list are as the caller left them
    poison_and_bind(pe, "ones")
    for b in (2, 3):
        assert same_records(records(pe.detect(x[:b], 0.5, 0.6)), records(ze.detect(x[:b], 0.5, 0.6)), "%s detect at batch %d behind one bind" % (pid, b)) > 0


def test_whole_plan_detect_frames_letterbox():
    """the two frame sizes of tests/test_gpu_eval.py, letterboxed; the batch tensor the frames are resized into is poisoned as well (the grey
    canvas is written, not assumed)"""
    pid = "v3-tiny-fp32-plan"
    zero, pois, _ = calibrated_twins(pid, 10, max_boxes=256)
    ze, pe = zero.net.engine, pois.net.engine
    rng = np.random.default_rng(23)
    frames = [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in ((120, 90), (75, 200))]
    pe._frames_batch(len(frames))
    total = 0
    for thr in (0.5, 0.1):
        want = records(ze.detect_frames(frames, thr, 0.6, _hip.NMS_AGNOSTIC, _hip.RESIZE_LETTERBOX))
        for poison in POISONS:
            pe._frames_u8.fill_(0xFF)
            poison_and_bind(pe, poison)
            got = records(pe.detect_frames(frames, thr, 0.6, _hip.NMS_AGNOSTIC, _hip.RESIZE_LETTERBOX))
            total += same_records(got, want, "%s detect_frames(%g) on %s" % (pid, thr, poison))
    assert total > 0, "no box anywhere: the fixture detects nothing"


def test_loss_and_loss_grad():
    """tiny-YOLOv2 at 32 x 32 as tests/test_gpu_loss_grad.py builds it: every returned record and the gradient, float and uint8 batches,
    the full batch and one image"""
    import torch
    from loss_grad_cases import ANCHORS8
    hw, names, anchors = (32, 32), ["a", "b", "c"], ANCHORS8[:10]
    net = YoloV2Tiny.create_network(np.reshape(anchors, [-1, 2]), names, False, input_shape=hw + (3,))
    w = synth.darknet_stream(net, seed=31, num_classes=3, head_gain=synth.HEAD_DEFAULTS["v2-tiny"][0], obj_bias=0.0)
    models = [YoloV2Tiny(), YoloV2Tiny()]
    for m in models:
        m.build(anchors, names, hw + (3,), dtype="fp32", max_batch=2, streams=1)
    models[1].net.engine._weights.fill_(0xFF)
    torch.cuda.synchronize()
    for m in models:
        v3.attach_weights(m.net, w)
    ze, pe = models[0].net.engine, models[1].net.engine
    x8 = np.random.RandomState(32).randint(0, 256, size=(2,) + hw + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    truths = [[(0.3, 0.4, 0.2, 0.5, 1), (0.8, 0.2, 0.3, 0.3, 2)], []]

    def host(ts):       # (result: its named fields -- the record's trailing pad word is nobody's output)
        out = [t.cpu().numpy().copy() for t in ts]
        rec = out[1].view(yeval.LOSS_RESULT_DTYPE)
        out[1] = np.concatenate([rec[k].view(np.uint8) for k in rec.dtype.names if k != "pad_"])
        return out

    for x, u8 in ((xf, False), (x8, True)):
        for b in (2, 1):
            gts = yeval.pack_gts(truths[:b], 2)
            want_loss = host((ze.loss_u8 if u8 else ze.loss)(x[:b], gts, assign=True))
            want_grad = host((ze.loss_grad_u8 if u8 else ze.loss_grad)(x[:b], gts))
            assert np.isfinite(want_grad[3]).all() and np.any(want_grad[3] != 0) and int((want_grad[2] >= 0).sum()) == 1
            for poison in POISONS:
                what = "%s batch %d on %s" % ("uint8" if u8 else "float32", b, poison)
                poison_and_bind(pe, poison)
                for k, (g, wnt) in enumerate(zip(host((pe.loss_u8 if u8 else pe.loss)(x[:b], gts, assign=True)), want_loss)):
                    same_bits(g, wnt, "loss %s: %s" % (what, ("images", "result", "assign")[k]))
                poison_and_bind(pe, poison)
                for k, (g, wnt) in enumerate(zip(host((pe.loss_grad_u8 if u8 else pe.loss_grad)(x[:b], gts)), want_grad)):
                    same_bits(g, wnt, "loss_grad %s: %s" % (what, ("images", "result", "assign", "grad")[k]))

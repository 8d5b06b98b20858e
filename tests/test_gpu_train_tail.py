"""GPU: the data gradient of the detection layer and the weight gradient of a 3 x 3 conv (include/yolo_hip.h: yolo_conv1x1_dgrad,
yolo_conv3x3_wgrad), through the C ABI, against tests/tail_ref.py; the shapes come from tests/tail_cases.py, which
tests/test_train_tail_cpu.py checks against the library's plan.

Every device output lies in a buffer with a 256-byte 0xA5 guard band on both sides; outputs and scratch are pre-filled with 0x00 and with
0xFF bytes.

  dgrad exact   integer G and W (|values| <= 8, cout <= 425: every sum below 2^24): D EQUALS the float32 reference, the slope factor as one
                float32 multiply; Y dense, sliced and unaligned, fp16 and float32, with +0, -0, negatives and positives; Y null
  wgrad exact   integer D and X3 (|values| <= 8, P <= 507): dW3 and db EQUAL the integer reference; taps at row ends, at image ends (the
                images differ) and chunk boundaries in the middle of a row; scale null and powers of two
  poison        NaN in every byte of the Y / X3 buffer outside the view changes no bit
  real          |device - ref64| / ((P + 3) 2^-24 |s| S |D| |X3|) <= 1.  Measured on an MI355X: see README.md, "Training the tail".
  step          yolo_net_train_tail_step is forward -> yolo_v2_loss_grad -> yolo_conv1x1_wgrad -> yolo_conv1x1_dgrad -> yolo_conv3x3_wgrad ->
                yolo_adam_step x 2, bit for bit; its uint8 twin on a state that was all 0xFF; the re-pack: the device weight blob equals
                that of a net loaded with the stream rebuilt from the master values, byte for byte; head-only training is what it was
  it trains     20 steps on a fixed batch, beside the float64 and float32 loops of tests/tail_ref.py on the device's block input
  train mode    launcher --mode train with train_layers = tail"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import loss_grad_cases
import tail_cases as cases
import tail_ref
from loss_grad_cases import ANCHORS8
from tensorflow_yolo_amd import YoloV2, YoloV2Tiny, _hip, launcher
from tensorflow_yolo_amd.net import base, engine, evaluate as yeval, synth, train as ytrain

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 256, 0xA5
NP_DTYPES = ((np.float16, _hip.DTYPE_F16), (np.float32, _hip.DTYPE_F32))


def guarded(nbytes, fill):
    import torch
    t = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    t[GUARD:GUARD + nbytes] = fill
    return t, t.data_ptr() + GUARD


def check_guards(bufs):
    for t, _ in bufs:
        assert bool((t[:GUARD] == PATTERN).all()) and bool((t[-GUARD:] == PATTERN).all()), "a guard band was written"


def payload(buf, shape):
    return buf[0][GUARD:-GUARD].cpu().numpy().view(np.float32).reshape(shape).copy()


def lay_out(values, batch, ppi, cin, view, background):
    """values [batch * ppi, cin] inside a flat buffer of `background` values (a callable n -> array) as the view (pad, coff, gap, start) ->
    (flat buffer, ld, coff, image_stride, start)"""
    pad, coff, gap, start = view
    ld = cin + pad
    img_stride = ppi * ld + gap
    flat = np.asarray(background(start + batch * img_stride + 16), dtype=np.float64)
    idx = (np.arange(batch)[:, None, None] * img_stride + np.arange(ppi)[None, :, None] * ld + coff + np.arange(cin)[None, None, :])
    flat[start + idx.reshape(-1)] = np.asarray(values, dtype=np.float64).reshape(-1)
    return flat, ld, coff, img_stride, start


# ---- yolo_conv1x1_dgrad -------------------------------------------------------------------------------------------------------------------
def run_dgrad(G, W, y, batch, ppi, slope=0.1, fill=0x00):
    """y: None or (flat np array of the view's dtype, ld, coff, image_stride, start) -> D [P, cin]"""
    import torch
    P, cout = G.shape
    cin = W.shape[1]
    d_g, d_w = torch.from_numpy(np.ascontiguousarray(G, dtype=np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).cuda()
    out = guarded(P * cin * 4, fill)
    if y is None:
        yp, ydt, ld, coff, istride = None, 0, 0, 0, 0
    else:
        flat, ld, coff, istride, start = y
        d_y = torch.from_numpy(flat).cuda()
        yp, ydt = d_y.data_ptr() + start * d_y.element_size(), (_hip.DTYPE_F16 if flat.dtype == np.float16 else _hip.DTYPE_F32)
    _hip.check(_hip.lib().yolo_conv1x1_dgrad(d_g.data_ptr(), cout, d_w.data_ptr(), cin, yp, ydt, ld, coff, istride, ppi, batch, slope, out[1],
                                             torch.cuda.current_stream().cuda_stream), "yolo_conv1x1_dgrad")
    torch.cuda.synchronize()
    check_guards([out])
    return payload(out, (P, cin))


@pytest.mark.parametrize("cout", cases.DGRAD_COUTS)
@pytest.mark.parametrize("cin", cases.DGRAD_CINS)
def test_dgrad_equals_the_float32_reference(cin, cout):
    rng = np.random.RandomState(1000 * cout + cin)
    W = rng.randint(-8, 9, size=(cout, cin)).astype(np.float32)
    for batch, ppi in cases.DGRAD_POSITIONS:
        P = batch * ppi
        G = rng.randint(-8, 9, size=(P, cout)).astype(np.float32)
        Y = cases.y_values(rng, P * cin).reshape(P, cin)
        assert (Y > 0).any() and (Y < 0).any() or P * cin < 64
        want_plain = tail_ref.dgrad(G, W, None, mode="float32")
        want = tail_ref.dgrad(G, W, Y, mode="float32")
        assert np.abs(want_plain).max() < 2 ** 24
        for fill in (0x00, 0xFF):
            assert np.array_equal(run_dgrad(G, W, None, batch, ppi, fill=fill), want_plain), (cout, cin, P, "no Y", fill)
            for view in cases.VIEWS:
                flat, ld, coff, istride, start = lay_out(Y, batch, ppi, cin, view, lambda n: cases.y_values(rng, n))
                for np_dtype, _ in NP_DTYPES:
                    got = run_dgrad(G, W, (flat.astype(np_dtype), ld, coff, istride, start), batch, ppi, fill=fill)
                    assert got.tobytes() == want.tobytes(), (cout, cin, P, view, np_dtype.__name__, fill)


def test_dgrad_signed_zeros_take_the_slope_and_other_slopes_multiply_once():
    G, W = np.full((3, 1), 3.0, dtype=np.float32), np.full((1, 8), 7.0, dtype=np.float32)
    Y = np.array([[0.0, -0.0, -1.0, 1.0, 6e-8, -6e-8, 65504.0, -65504.0]] * 3)
    for slope in (0.1, 0.0, -0.25, 1.0):
        want = tail_ref.dgrad(G, W, Y.astype(np.float16), slope, mode="float32")
        assert want[0, 3] == 21.0 and want[0, 0] == np.float32(21.0) * np.float32(slope)
        for np_dtype, _ in NP_DTYPES:
            got = run_dgrad(G, W, (Y.astype(np_dtype).reshape(-1), 8, 0, 8, 0), 3, 1, slope=slope, fill=0xFF)
            assert got.tobytes() == tail_ref.dgrad(G, W, Y.astype(np_dtype), slope, mode="float32").tobytes(), (slope, np_dtype.__name__)


def test_dgrad_nan_outside_the_view_changes_no_bit():
    rng = np.random.RandomState(11)
    cout, cin, batch, ppi = 30, 40, 2, 37
    G, W = rng.randint(-8, 9, size=(batch * ppi, cout)).astype(np.float32), rng.randint(-8, 9, size=(cout, cin)).astype(np.float32)
    Y = cases.y_values(rng, batch * ppi * cin).reshape(-1, cin)
    want = tail_ref.dgrad(G, W, Y, mode="float32")
    for view in cases.VIEWS[1:]:
        flat, ld, coff, istride, start = lay_out(Y, batch, ppi, cin, view, lambda n: np.full(n, np.nan))
        assert np.isnan(flat).sum() == flat.size - Y.size
        for np_dtype, _ in NP_DTYPES:
            got = run_dgrad(G, W, (flat.astype(np_dtype), ld, coff, istride, start), batch, ppi, fill=0xFF)
            assert got.tobytes() == want.tobytes(), (view, np_dtype.__name__)


# ---- yolo_conv3x3_wgrad -------------------------------------------------------------------------------------------------------------------
def run_wgrad(x, h, w, batch, cin, D, scale=None, fill=0x00, calls=1):
    """x: (flat np array of the view's dtype, ld, coff, image_stride, start) -> [(dW3 [cout, 9, cin], db [cout])] of each call, the outputs
    and the scratch filled with `fill` bytes once, before the first call"""
    import torch
    flat, ld, coff, istride, start = x
    dtype = _hip.DTYPE_F16 if flat.dtype == np.float16 else _hip.DTYPE_F32
    P, cout = D.shape
    assert P == batch * h * w
    pl = _hip.conv3x3_wgrad_plan(h, w, batch, cin, cout, dtype)
    d_x = torch.from_numpy(flat).cuda()
    d_d = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32)).cuda()
    d_s = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32)).cuda()
    bufs = [guarded(cout * 9 * cin * 4, fill), guarded(cout * 4, fill), guarded(pl["scratch_bytes"], fill)]
    out = []
    for _ in range(calls):
        _hip.check(_hip.lib().yolo_conv3x3_wgrad(d_x.data_ptr() + start * d_x.element_size(), dtype, ld, coff, istride, h, w, batch, cin,
                                                 d_d.data_ptr(), cout, None if d_s is None else d_s.data_ptr(), bufs[0][1], bufs[1][1], bufs[2][1],
                                                 pl["scratch_bytes"], torch.cuda.current_stream().cuda_stream), "yolo_conv3x3_wgrad")
        torch.cuda.synchronize()
        check_guards(bufs)
        out.append((payload(bufs[0], (cout, 9, cin)), payload(bufs[1], (cout,))))
    return out


def exact_case(h, w, batch, cin, cout, seed):
    rng = np.random.RandomState(seed)
    X3 = rng.randint(-8, 9, size=(batch, h, w, cin))
    X3[X3 == 0] = 5                 # no zeros: a tap that leaks across a row end or an image end, or a dropped one, changes a sum
    D = rng.randint(-8, 9, size=(batch * h * w, cout))
    D[D == 0] = -3
    scale = np.exp2(rng.randint(-3, 4, size=cout))
    return rng, X3, D, scale


def check_exact(h, w, batch, cin, cout, seed):
    rng, X3, D, scale = exact_case(h, w, batch, cin, cout, seed)
    if batch > 1:
        assert not any(np.array_equal(X3[0], X3[n]) for n in range(1, batch))           # the images differ
    want = {None: tail_ref.wgrad3x3_exact(X3, D), "pow2": tail_ref.wgrad3x3_exact(X3, D, scale)}
    for view in cases.VIEWS:
        flat, ld, coff, istride, start = lay_out(X3.reshape(-1, cin), batch, h * w, cin, view, lambda n: rng.randint(-8, 9, size=n))
        for np_dtype, _ in NP_DTYPES:
            for key, s in ((None, None), ("pow2", scale)):
                x = (flat.astype(np_dtype), ld, coff, istride, start)
                got = run_wgrad(x, h, w, batch, cin, D, s, 0x00, calls=2) + run_wgrad(x, h, w, batch, cin, D, s, 0xFF, calls=2)
                tag = (h, w, batch, cin, cout, view, np_dtype.__name__, key)
                for dw, db in got:
                    assert np.array_equal(dw, want[key][0]), tag
                    assert np.array_equal(db, want[key][1]), tag
                assert all(dw.tobytes() == got[0][0].tobytes() and db.tobytes() == got[0][1].tobytes() for dw, db in got), tag
                if h == 1 and w == 1:       # only the centre tap exists: the other eight are +0, bit for bit
                    assert not got[0][0][:, [0, 1, 2, 3, 5, 6, 7, 8], :].view(np.uint32).any(), tag
                    assert got[0][0][:, 4, :].any()


@pytest.mark.parametrize("shape", cases.wgrad_shapes(), ids=lambda s: "x".join(str(v) for v in s))
def test_wgrad_equals_the_integer_reference(shape):
    h, w, batch, cin, cout = shape
    check_exact(h, w, batch, cin, cout, seed=hash(shape) % 2 ** 31)


def test_wgrad_equals_the_integer_reference_around_a_chunks_end():
    """one position short of a chunk, exactly one, one past it, two chunks and five positions: sized from the plan"""
    for cin, cout in ((8, 1), (136, 65)):
        plan = lambda h, w, b: _hip.conv3x3_wgrad_plan(h, w, b, cin, cout)
        for h, w, batch, chunks in cases.wgrad_plan_shapes(plan):
            assert plan(h, w, batch)["n_chunks"] == chunks
            check_exact(h, w, batch, cin, cout, seed=h * 100 + w + cin)


def test_wgrad_nan_outside_the_view_changes_no_bit():
    for h, w, batch, cin, cout in ((5, 7, 3, 40, 30), (13, 13, 2, 136, 65), (1, 1, 3, 8, 1)):
        rng, X3, D, scale = exact_case(h, w, batch, cin, cout, seed=7)
        want_w, want_b = tail_ref.wgrad3x3_exact(X3, D, scale)
        for view in cases.VIEWS[1:]:
            flat, ld, coff, istride, start = lay_out(X3.reshape(-1, cin), batch, h * w, cin, view, lambda n: np.full(n, np.nan))
            assert np.isnan(flat).sum() == flat.size - X3.size
            for np_dtype, _ in NP_DTYPES:
                (dw, db), = run_wgrad((flat.astype(np_dtype), ld, coff, istride, start), h, w, batch, cin, D, scale, 0xFF)
                assert np.array_equal(dw, want_w) and np.array_equal(db, want_b), (h, w, batch, view, np_dtype.__name__)


@pytest.mark.parametrize("shape", [(13, 13, 2, 136, 64), (3, 5, 1, 1280, 30)], ids=lambda s: "x".join(str(v) for v in s))
def test_wgrad_real_values_within_the_float32_bound(shape):
    """|device - ref64| <= (P + 3) 2^-24 |s| S_p |D| |X3| per element.  Measured on an MI355X, largest |device - ref64| / bound (printed
    below): 13 x 13 x 136 -> 64, batch 2 (11 chunks): dW3 0.0075, db 0.0040; 3 x 5, cin 1280 -> 30 (one chunk): dW3 0.3273, db 0.1450."""
    h, w, batch, cin, cout = shape
    rng = np.random.RandomState(sum(shape))
    P = batch * h * w
    X3 = rng.randn(batch, h, w, cin).astype(np.float16)
    D = (np.exp2(rng.uniform(-20, 8, size=(P, cout))) * rng.choice([-1.0, 1.0], size=(P, cout))).astype(np.float32)
    scale = (rng.uniform(0.5, 2.0, size=cout) * rng.choice([-1.0, 1.0], size=cout)).astype(np.float32)
    (dw, db), = run_wgrad((X3.reshape(-1), cin, 0, h * w * cin, 0), h, w, batch, cin, D, scale, 0xFF)
    ref_w, ref_b, bound_w, bound_b = tail_ref.wgrad3x3_ref64(X3, D, scale)
    live = bound_w > 0
    assert np.array_equal(dw[~live], np.zeros_like(dw[~live]))          # taps that never lie inside the image
    ratio_w = float(np.max(np.abs(dw.astype(np.float64) - ref_w)[live] / bound_w[live]))
    ratio_b = float(np.max(np.abs(db.astype(np.float64) - ref_b) / bound_b))
    print("conv3x3_wgrad %s (%d chunks): largest |device - ref64| / bound: dW3 %.4f db %.4f"
          % (shape, _hip.conv3x3_wgrad_plan(h, w, batch, cin, cout)["n_chunks"], ratio_w, ratio_b))
    assert ratio_w <= 1 and ratio_b <= 1


# ---- the tail of a net: the step is its parts; the next forward sees the update -----------------------------------------------------------
V2_ANCHORS = ANCHORS8[:10]
NAMES20 = ["c%d" % i for i in range(20)]
BATCH = 3
LR = 1e-4       # (the block has 10 M weights that all move by lr in Adam's first step: at 1e-3 the second step's logits overflow exp())


class SmallTail(YoloV2):
    """the small tail of tests/tail_cases.py as a model"""
    create_network = staticmethod(cases.small_tail_network)


MODELS = {"v2": YoloV2, "v2-tiny": YoloV2Tiny, "small": SmallTail}
NETS = {"v2-64": ("v2", (64, 64)), "v2-96x160": ("v2", (96, 160)), "v2-tiny-64": ("v2-tiny", (64, 64))}


@functools.lru_cache(maxsize=None)
def stream_of(version, hw, n_classes):
    net = MODELS[version].create_network(np.reshape(V2_ANCHORS, [-1, 2]), ["c%d" % i for i in range(n_classes)], False, input_shape=hw + (3,))
    w = synth.darknet_stream(net, seed=41, num_classes=n_classes, head_gain=synth.HEAD_DEFAULTS["v2-tiny" if version == "small" else version][0],
                             obj_bias=0.0)
    w.setflags(write=False)
    return w


def build(version, hw, dtype, weights, names=NAMES20, max_batch=BATCH):
    m = MODELS[version]()
    m.build(V2_ANCHORS, names, hw + (3,), dtype=dtype, max_batch=max_batch, weights=weights, streams=1)
    return m


TAIL_PARTS = ("w", "b", "m_w", "v_w", "m_b", "v_b", "dw", "db", "w3", "beta", "m_w3", "v_w3", "m_beta", "v_beta", "dw3", "dbeta")


def tail_part(eng, name, nbytes):
    o = int(getattr(eng.tail_layout, name + "_offset"))
    return eng._tail_state[o:o + nbytes]


def same_bytes(state_slice, tensor):
    import torch
    return bool(torch.equal(state_slice, tensor.reshape(-1).view(torch.uint8)))


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("name", sorted(NETS))
def test_train_tail_step_is_its_parts_and_the_next_forward_sees_it(name, dtype):
    import torch
    lib = _hip.lib()
    version, hw = NETS[name]
    A, n_classes = 5, 20
    cout = A * (5 + n_classes)
    weights = stream_of(version, hw, n_classes)
    m = build(version, hw, dtype, weights)
    eng = m.net.engine
    h, w, _ = m.net[-1].out.hwc
    P = BATCH * h * w
    _, gt, counts = loss_grad_cases.random_case((h, w, A, n_classes, BATCH), 7)
    x8 = np.random.RandomState(42).randint(0, 256, size=(BATCH,) + hw + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    cin = ytrain.head_counts(m.net)[1]
    cout3, cin3, pos, n_block = ytrain.tail_counts(m.net)
    block, w0, b0 = ytrain.split_tail(weights, m.net)
    eng.tail_train_init(block, w0, b0)
    lay = eng.tail_layout
    bview, hview = eng.tail_inputs()
    assert (bview.cin, bview.h, bview.w, hview.cin) == (cin3, h, w, cin) and cin == cout3
    st = torch.cuda.current_stream().cuda_stream
    hd = eng.head
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(BATCH, -1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
    # the composition's own state: master values and moments in plain tensors
    w3_0 = tail_ref.stream_to_otc(block[4 * cout3:], cout3, cin3)
    scale64, _ = tail_ref.fold(block[:cout3], block[cout3:2 * cout3], block[2 * cout3:3 * cout3], block[3 * cout3:4 * cout3])
    scale32 = torch.from_numpy(scale64.astype(np.float32)).cuda()
    zeros = lambda n: np.zeros(n, np.float32)
    nw, nw3 = cout * cin, cout3 * 9 * cin3
    comp = {k: torch.from_numpy(np.array(v)).cuda() for k, v in
            (("w", w0.reshape(-1)), ("b", b0), ("m_w", zeros(nw)), ("v_w", zeros(nw)), ("m_b", zeros(cout)), ("v_b", zeros(cout)),
             ("w3", w3_0.reshape(-1)), ("beta", block[:cout3]), ("m_w3", zeros(nw3)), ("v_w3", zeros(nw3)), ("m_beta", zeros(cout3)),
             ("v_beta", zeros(cout3)))}
    for k, n in (("dw", nw), ("db", cout), ("dw3", nw3), ("dbeta", cout3), ("grad", P * cout), ("d", P * cout3)):
        comp[k] = torch.empty(n, dtype=torch.float32, device="cuda")
    pl = _hip.wgrad_plan(P, cin, cout, hview.dtype)
    pl3 = _hip.conv3x3_wgrad_plan(h, w, BATCH, cin3, cout3, bview.dtype)
    images = torch.empty(BATCH * 56, dtype=torch.uint8, device="cuda")
    assign = torch.empty(P, dtype=torch.int32, device="cuda")
    result = torch.empty(64, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(max(pl["scratch_bytes"], pl3["scratch_bytes"]), dtype=torch.uint8, device="cuda")
    ws = eng._workspace.data_ptr()
    p = lambda k: comp[k].data_ptr()

    def check_parts(tag):
        for k in TAIL_PARTS:
            assert same_bytes(tail_part(eng, k, comp[k].numel() * 4), comp[k]), tag + (k,)
        assert same_bytes(tail_part(eng, "grad", P * cout * 4), comp["grad"]), tag + ("G",)
        assert same_bytes(tail_part(eng, "d", P * cout3 * 4), comp["d"]), tag + ("D",)

    results = []
    for t in (1, 2):
        lr_t = float(engine.adam_lr_t(LR, t))
        logits = eng.forward(xf)
        _hip.check(lib.yolo_v2_loss_grad(C.byref(hd), logits.data_ptr(), BATCH, d_gt.data_ptr(), d_gc.data_ptr(), gt.shape[1], images.data_ptr(),
                                         assign.data_ptr(), result.data_ptr(), p("grad"), st), "yolo_v2_loss_grad")
        _hip.check(lib.yolo_conv1x1_wgrad(ws + hview.offset, hview.dtype, hview.ld, hview.coff, hview.image_stride, h * w, BATCH, cin, p("grad"), cout,
                                          p("dw"), p("db"), scratch.data_ptr(), scratch.numel(), st), "yolo_conv1x1_wgrad")
        _hip.check(lib.yolo_conv1x1_dgrad(p("grad"), cout, p("w"), cin, ws + hview.offset, hview.dtype, hview.ld, hview.coff, hview.image_stride, h * w,
                                          BATCH, 0.1, p("d"), st), "yolo_conv1x1_dgrad")
        _hip.check(lib.yolo_conv3x3_wgrad(ws + bview.offset, bview.dtype, bview.ld, bview.coff, bview.image_stride, h, w, BATCH, cin3, p("d"), cout3,
                                          scale32.data_ptr(), p("dw3"), p("dbeta"), scratch.data_ptr(), scratch.numel(), st), "yolo_conv3x3_wgrad")
        _hip.check(lib.yolo_adam_step(p("w"), p("b"), p("m_w"), p("v_w"), p("m_b"), p("v_b"), p("dw"), p("db"), nw, cout, lr_t, 0.9, 0.999, 1e-8, st),
                   "yolo_adam_step")
        _hip.check(lib.yolo_adam_step(p("w3"), p("beta"), p("m_w3"), p("v_w3"), p("m_beta"), p("v_beta"), p("dw3"), p("dbeta"), nw3, cout3, lr_t, 0.9,
                                      0.999, 1e-8, st), "yolo_adam_step")
        want_result = result.cpu().numpy().tobytes()
        got_result = eng.train_tail_step(xf, (gt, counts), lr_t).cpu().numpy().tobytes()
        assert got_result == want_result, (name, dtype, t)
        check_parts((name, dtype, t))
        assert bool(comp["dw3"].abs().sum() > 0) and bool(comp["d"].abs().sum() > 0) and bool(torch.isfinite(comp["w3"]).all())
        results.append(got_result)
    assert results[0] != results[1] and np.isfinite(np.frombuffer(results[1], dtype=yeval.LOSS_RESULT_DTYPE)[0]["loss"])
    k3, beta2, w2, b2 = eng.tail_train_read()
    assert tail_ref.stream_to_otc(k3.reshape(-1), cout3, cin3).tobytes() == comp["w3"].cpu().numpy().tobytes() and k3.tobytes() != block[4 * cout3:].tobytes()
    assert beta2.tobytes() == comp["beta"].cpu().numpy().tobytes() and w2.tobytes() == comp["w"].cpu().numpy().tobytes()
    # the re-pack of both layers: a second net, loaded with the rebuilt stream through yolo_net_load_weights, computes the same logits
    fresh = synth.synthetic_input(BATCH, hw[0], hw[1], 3, seed=43)
    stepped = eng.forward(fresh).cpu().numpy()
    rebuilt = ytrain.replace_tail(weights, m.net, k3, beta2, w2, b2)
    changed = np.flatnonzero(rebuilt != weights)
    assert changed.min() >= pos and not ((changed >= pos + cout3) & (changed < pos + 4 * cout3)).any()       # gamma and the statistics stay
    second = build(version, hw, dtype, rebuilt).net.engine
    assert bool(torch.equal(second._weights, eng._weights)), "the re-packed device weights are not the bytes yolo_net_load_weights produces"
    assert second.forward(fresh).cpu().numpy().tobytes() == stepped.tobytes()
    assert build(version, hw, dtype, ytrain.replace_head(weights, w2, b2)).net.engine.forward(fresh).cpu().numpy().tobytes() != stepped.tobytes()
    # the uint8 twin from the same start, on a state whose every byte was 0xFF before the init: the same bits
    eng._tail_state.fill_(0xFF)
    _hip.check(lib.yolo_net_tail_train_init(eng.handle, eng._tail_state.data_ptr(), eng._tail_state.numel(), block.ctypes.data, w0.ctypes.data,
                                            b0.ctypes.data), "yolo_net_tail_train_init")
    for t in (1, 2):
        assert eng.train_tail_step_u8(x8, (gt, counts), engine.adam_lr_t(LR, t)).cpu().numpy().tobytes() == results[t - 1]
    check_parts((name, dtype, "u8 on 0xFF"))
    # head-only training on the same net, from the same start: its first step sees the same weights, so the same record, the same dW and
    # the same head -- the old path is what it was (tests/test_gpu_train.py holds it to its parts)
    v2net = build(version, hw, dtype, weights).net.engine
    v2net.head_train_init(w0, b0)
    first = v2net.train_head_step(xf, (gt, counts), engine.adam_lr_t(LR, 1)).cpu().numpy().tobytes()
    assert first == results[0]
    eng.tail_train_init(block, w0, b0)
    eng.train_tail_step(xf, (gt, counts), engine.adam_lr_t(LR, 1))
    hl = v2net.train_layout
    for k, n in (("w", nw), ("b", cout), ("dw", nw), ("db", cout), ("m_w", nw), ("v_w", nw)):
        o = int(getattr(hl, k + "_offset"))
        assert bool(torch.equal(v2net._train_state[o:o + 4 * n], tail_part(eng, k, 4 * n))), (name, dtype, "head-only", k)


# ---- it trains --------------------------------------------------------------------------------------------------------------------------
def test_twenty_steps_on_a_fixed_batch_lower_the_loss_and_track_the_yardstick():
    """The small tail (tests/tail_cases.py) at 64 x 64, fp16, batch 4, 1 class, lr 1e-4, on a fixed batch: the loss falls at every step
    (2869.5 -> 49.75) and tracks the yardstick's float64 loop (tests/tail_ref.py: tail_train_loop on the device's stored block input, with
    the fp16 rounding of the packed weights and of Y restated, since those are part of the function).

    The per-step form 4 |ref32 - ref64| + 1 float32 ulp is too tight here, as foreseen when this test was specified: the yardstick's own
    float32 loop lies anywhere between 5e-8 and 1e-4 (relative) from its float64 loop, step by step -- fp16 roundings of Y that flip, Adam's
    sign-like first steps -- and where it happens to lie close, a device that is as far off as the float32 loop usually is misses the
    bound (measured on an MI355X: 1.38 x the per-step bound at step 12, where |ref32 - ref64| / ref64 = 7.6e-8, and at most 0.52 x at the
    other 19 steps; at lr 1e-3, where the loss is not monotone, 1.70 x at step 5 and at most 0.63 x elsewhere).  Asserted instead, as
    specified for this case: the largest relative gap of the device over the 20 steps is at most 4 x the largest relative gap of the
    yardstick's float32 loop.  Measured on an MI355X: device 1.049e-4, float32 loop 1.050e-4 (both at step 4; printed with the per-step
    figures)."""
    import torch
    hw, n_classes, B, steps, lr = (64, 64), 1, 4, 20, 1e-4
    weights = stream_of("small", hw, n_classes)
    m = build("small", hw, "fp16", weights, names=["tower"], max_batch=B)
    eng = m.net.engine
    h, w, cout = m.net[-1].out.hwc
    _, gt, counts = loss_grad_cases.random_case((h, w, 5, n_classes, B), 7)
    x = synth.synthetic_input(B, hw[0], hw[1], 3, seed=44)
    cout3, cin3, pos, n_block = ytrain.tail_counts(m.net)
    block, w0, b0 = ytrain.split_tail(weights, m.net)
    eng.tail_train_init(block, w0, b0)
    eng.forward(x)
    torch.cuda.synchronize()
    bview, _ = eng.tail_inputs()
    flat = eng._workspace[bview.offset:bview.offset + 2 * B * bview.image_stride].cpu().numpy().view(np.float16)
    idx = (np.arange(B)[:, None, None] * bview.image_stride + np.arange(h * w)[None, :, None] * bview.ld + bview.coff + np.arange(cin3)[None, None, :])
    X3 = flat[idx].reshape(B, h, w, cin3)
    records = torch.empty((steps, 64), dtype=torch.uint8, device="cuda")
    for t in range(1, steps + 1):
        eng.train_tail_step(x, (gt, counts), engine.adam_lr_t(lr, t), result=records[t - 1])
    dev = np.array([float(r["loss"]) for r in records.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE).reshape(-1)])          # the one read
    blk = (block[:cout3], block[cout3:2 * cout3], block[2 * cout3:3 * cout3], block[3 * cout3:4 * cout3], tail_ref.stream_to_otc(block[4 * cout3:], cout3, cin3))
    args = (X3, blk, w0, b0, h, w, V2_ANCHORS, n_classes, gt, counts, lr, steps, np.float16)
    ref64 = np.array(tail_ref.tail_train_loop(*args, mode="float64")[0])
    ref32 = np.array(tail_ref.tail_train_loop(*args, mode="float32")[0])
    tol = 4 * np.abs(ref32 - ref64) + np.spacing(ref64.astype(np.float32)).astype(np.float64)
    gap, own = np.abs(dev - ref64) / ref64, np.abs(ref32 - ref64) / ref64
    print("device :", " ".join("%.6f" % v for v in dev))
    print("float64:", " ".join("%.6f" % v for v in ref64))
    print("float32:", " ".join("%.6f" % v for v in ref32))
    print("|device - ref64| / ref64 :", " ".join("%.2e" % v for v in gap))
    print("|ref32  - ref64| / ref64 :", " ".join("%.2e" % v for v in own))
    print("|device - ref64| / (4 |ref32 - ref64| + 1 ulp):", " ".join("%.2f" % v for v in np.abs(dev - ref64) / tol))
    print("largest relative gap: device %.3e, the yardstick's float32 loop %.3e" % (gap.max(), own.max()))
    assert np.isfinite(dev).all() and all(a > c for a, c in zip(dev, dev[1:])), dev
    assert all(a > c for a, c in zip(ref64, ref64[1:]))
    assert gap.max() <= 4 * own.max(), (gap.max(), own.max())


# ---- refusals that need a device --------------------------------------------------------------------------------------------------------
def test_step_refuses_a_missing_init_and_a_net_without_a_tail():
    import torch
    hw = (64, 64)
    eng = build("small", hw, "fp16", stream_of("small", hw, 20)).net.engine
    with pytest.raises(RuntimeError, match="follows tail_train_init"):
        eng.train_tail_step(np.zeros((1,) + hw + (3,), np.float32), [[]], 1e-3)
    mx = build("v2", hw, "mxfp8", stream_of("v2", hw, 20))
    with pytest.raises(_hip.YoloHipError, match="MXFP8 conv"):
        mx.net.engine.tail_train_init(*ytrain.split_tail(stream_of("v2", hw, 20), mx.net))


# ---- train mode -------------------------------------------------------------------------------------------------------------------------
VOC_XML = ("<annotation><filename>%s</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>"
           "<object><name>tower</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object></annotation>")


def test_launcher_mode_train_with_train_layers_tail(tmp_path, capsys):
    """two images at batch 2, two epochs, a checkpoint every step, tiny-YOLOv2 from a full weight file: the reference's lines, a first loss
    that holds the bits of train_tail_step_u8 on the same batch, and checkpoints that differ from the initial stream in the block's kernel
    and beta and the head only"""
    import random
    from PIL import Image
    rng = np.random.RandomState(53)
    hw = (96, 160)
    for d in ("train", "val", "out"):
        (tmp_path / d).mkdir()
    for d in ("train", "val"):
        for i in range(2):
            fname = "im%d.png" % i
            Image.fromarray(rng.randint(0, 256, size=(120, 200, 3)).astype(np.uint8)).save(str(tmp_path / d / fname))
            x1, y1 = int(rng.randint(0, 100)), int(rng.randint(0, 60))
            (tmp_path / d / ("im%d.xml" % i)).write_text(VOC_XML % (fname, 200, 120, x1, y1, x1 + int(rng.randint(20, 100)), y1 + int(rng.randint(20, 60))))
    full = stream_of("v2-tiny", hw, 1)
    base.write_darknet_weights(str(tmp_path / "full.weights"), full, "v2")
    (tmp_path / "cfg.ini").write_text(
        "[COMMON]\nversion = v2-tiny\ninput_h = %d\ninput_w = %d\ninput_c = 3\n"
        "[TRAIN]\ntrain_layers = tail\nseed = 3\nimage_dir = train/\nannotation_dir = train/\nval_image_dir = val/\nval_annotation_dir = val/\n"
        "batch_size = 2\nlearning_rate = 1e-3\nepochs = 2\nmax_step = -1\naugment_probability = 0.0\ncheckpoint_dir = out/\ncheckpoint_step = 1\n"
        "checkpoint_prefix = yolo\ntensorboard_log_dir = log/\npretrained_weights_path = full.weights\nanchors = %s\nclass_names = [\"tower\"]\n"
        "cpu_only = False\ndtype = fp16\n" % (hw[0], hw[1], list(V2_ANCHORS)))
    launcher.run(launcher.read_config(str(tmp_path / "cfg.ini")), "train")
    out = capsys.readouterr().out.splitlines()
    steps = [l for l in out if l.startswith("step ")]
    assert len(steps) == 2 and steps[0].startswith("step 1 (1/2): ") and steps[1].startswith("step 2 (2/2): ") and "(moving average: " in steps[1]
    assert sum(l.startswith("validation loss: ") for l in out) == 2 and out[-1] == "Done" and "Epoch (2/2) completed." in out
    assert any("tensorboard_log_dir is ignored" in l for l in out) and "Pre-trained weights loaded." in out
    # the first loss: the step entry on the same batch, from the same start
    ann, _ = yeval.parse_voc_annotations(str(tmp_path / "train"), str(tmp_path / "train"), ["tower"])
    batch, = ytrain.make_batches(ann, 2, random.Random(3))
    m = build("v2-tiny", hw, "fp16", full, names=["tower"], max_batch=2)
    eng = m.net.engine
    eng.tail_train_init(*ytrain.split_tail(full, m.net))
    x, truths = ytrain.batch_to_device(eng, batch)
    rec = eng.train_tail_step_u8(x, truths, engine.adam_lr_t(1e-3, 1)).cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]
    assert steps[0] == "step 1 (1/2): {} (moving average: {})".format(np.float32(rec["loss"]), np.float32(rec["loss"]))
    # checkpoints
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["yolo-%d.weights" % s for s in (0, 1, 2)]
    header0, body0 = base.read_darknet_weights(str(tmp_path / "out" / "yolo-0.weights"), "v2")
    assert body0.tobytes() == full.tobytes()
    cout3, cin3, pos, n_block = ytrain.tail_counts(m.net)
    inside = np.zeros(len(full), dtype=bool)
    inside[pos:pos + cout3] = True
    inside[pos + 4 * cout3:] = True
    for s in (1, 2):
        header, body = base.read_darknet_weights(str(tmp_path / "out" / ("yolo-%d.weights" % s)), "v2")
        assert header == header0 and len(body) == len(full)
        assert body[~inside].tobytes() == full[~inside].tobytes()
        assert body[pos:pos + cout3].tobytes() != full[pos:pos + cout3].tobytes()
        assert body[pos + 4 * cout3:pos + n_block].tobytes() != full[pos + 4 * cout3:pos + n_block].tobytes()
        assert body[pos + n_block:].tobytes() != full[pos + n_block:].tobytes()
    _, body1 = base.read_darknet_weights(str(tmp_path / "out" / "yolo-1.weights"), "v2")
    assert body1.tobytes() == ytrain.replace_tail(full, m.net, *eng.tail_train_read()).tobytes()

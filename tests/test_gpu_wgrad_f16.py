"""GPU: the 3 x 3 weight gradient on the fp16 matrix cores (include/yolo_hip.h: yolo_conv3x3_wgrad_f16) and its mode on a net
(yolo_net_train_set_wgrad_f16), through the C ABI, against tests/wgrad_f16_ref.py; the shapes come from its case table, which
tests/test_wgrad_f16_cpu.py checks against the library's plan.

Every device output lies in a buffer with a 256-byte 0xA5 guard band on both sides; outputs and scratch are pre-filled with 0x00 and with
0xFF bytes.

  exact         integer D and X3: dW3 and db EQUAL the integer reference; taps at row ends, at image ends and chunk boundaries in the middle
                of a row; views dense, sliced and unaligned; scale null and powers of two; a second call returns the same bits
  the scale     the same data times 2^-20 and 2^10: the reference times the same power, bit for bit; k as the yardstick's; zero D: +0, k = 0
  narrowing     a one-hot X3 shows 2^-k D16 in the centre tap: ties, the maximum, fp16 subnormals, bit-equal to the NumPy conversion
  subnormal X3  fp16 subnormal activations count: the exact sum, bit for bit
  leaks         NaN in a neighbouring image, in a neighbouring row, outside a sliced view: no bit changes
  real          the header's two bounds and db's, element by element.  Measured on an MI355X: see README.md, "Training"
  the mode      a step with set_wgrad_f16 is its parts, bit for bit; switching back gives the float32 step; the re-pack; refusals
  it trains     20 steps in the mode beside the float32 mode and the yardstick's loops
  train mode    launcher --mode train with wgrad = fp16"""
import ctypes as C

import numpy as np
import pytest

import tail_ref
import test_gpu_train_tail as TT
import wgrad_f16_ref as ref
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine

pytestmark = pytest.mark.gpu
VIEWS = TT.cases.VIEWS


def run16(x, h, w, batch, cin, D, scale=None, fill=0x00, calls=1):
    """x: (flat float16 array, ld, coff, image_stride, start) -> [(dW3 [cout, 9, cin], db [cout], bits of m, k)] of each call, the outputs
    and the scratch filled with `fill` bytes once, before the first call"""
    import torch
    flat, ld, coff, istride, start = x
    assert flat.dtype == np.float16
    P, cout = D.shape
    assert P == batch * h * w
    pl = _hip.conv3x3_wgrad_f16_plan(h, w, batch, cin, cout)
    d_x = torch.from_numpy(flat).cuda()
    d_d = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32)).cuda()
    d_s = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32)).cuda()
    bufs = [TT.guarded(cout * 9 * cin * 4, fill), TT.guarded(cout * 4, fill), TT.guarded(pl["scratch_bytes"], fill)]
    out = []
    for _ in range(calls):
        _hip.check(_hip.lib().yolo_conv3x3_wgrad_f16(d_x.data_ptr() + start * 2, _hip.DTYPE_F16, ld, coff, istride, h, w, batch, cin, d_d.data_ptr(),
                                                     cout, None if d_s is None else d_s.data_ptr(), bufs[0][1], bufs[1][1], bufs[2][1],
                                                     pl["scratch_bytes"], torch.cuda.current_stream().cuda_stream), "yolo_conv3x3_wgrad_f16")
        torch.cuda.synchronize()
        TT.check_guards(bufs)
        o = TT.GUARD + pl["record_offset"]
        rec = bufs[2][0][o:o + 8].cpu().numpy()
        out.append((TT.payload(bufs[0], (cout, 9, cin)), TT.payload(bufs[1], (cout,)), int(rec.view(np.uint32)[0]), int(rec.view(np.int32)[1])))
    return out


def dense(X3):
    b, h, w, cin = X3.shape
    return (np.ascontiguousarray(X3, dtype=np.float16).reshape(-1), cin, 0, h * w * cin, 0)


def check_exact(h, w, batch, cin, cout, seed, views=VIEWS):
    rng, X3, D, scale = TT.exact_case(h, w, batch, cin, cout, seed)
    if batch > 1:
        assert not any(np.array_equal(X3[0], X3[n]) for n in range(1, batch))           # the images differ
    want = {None: ref.wgrad3x3_f16_exact(X3, D), "pow2": ref.wgrad3x3_f16_exact(X3, D, scale)}
    for view in views:
        flat, ld, coff, istride, start = TT.lay_out(X3.reshape(-1, cin), batch, h * w, cin, view, lambda n: rng.randint(-8, 9, size=n))
        for key, s in ((None, None), ("pow2", scale)):
            x = (flat.astype(np.float16), ld, coff, istride, start)
            got = run16(x, h, w, batch, cin, D, s, 0x00, calls=2) + run16(x, h, w, batch, cin, D, s, 0xFF, calls=2)
            tag = (h, w, batch, cin, cout, view, key)
            for dw, db, bits, k in got:
                assert np.array_equal(dw, want[key][0]), tag
                assert np.array_equal(db, want[key][1]), tag
                assert bits == ref.max_bits(D) and k == ref.k_of(D), tag
            assert all(dw.tobytes() == got[0][0].tobytes() and db.tobytes() == got[0][1].tobytes() for dw, db, _, _ in got), tag
            if h == 1 and w == 1:       # only the centre tap exists: the other eight are +0, bit for bit
                assert not got[0][0][:, [0, 1, 2, 3, 5, 6, 7, 8], :].view(np.uint32).any(), tag
                assert got[0][0][:, 4, :].any()


@pytest.mark.parametrize("shape", ref.SHAPES + ref.WIDE_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_wgrad_f16_equals_the_integer_reference(shape):
    h, w, batch, cin, cout = shape
    check_exact(h, w, batch, cin, cout, seed=sum((i + 1) * v for i, v in enumerate(shape)))


def test_wgrad_f16_equals_the_integer_reference_around_a_chunks_end():
    """one position short of a chunk, exactly one, one past it, two chunks and five positions: sized from the plan"""
    for cin, cout in ((8, 1), (136, 65)):
        plan = lambda h, w, b: _hip.conv3x3_wgrad_f16_plan(h, w, b, cin, cout)
        for h, w, batch, chunks in ref.plan_shapes(plan):
            assert plan(h, w, batch)["n_chunks"] == chunks
            check_exact(h, w, batch, cin, cout, seed=h * 100 + w + cin, views=VIEWS[::2])


def test_wgrad_f16_largest_integers_that_fp16_holds():
    """|D| <= 2047 (eleven bits), |X3| <= 2048, S |D| |X3| < 2^24"""
    rng = np.random.RandomState(5)
    h, w, batch, cin, cout = 1, 5, 1, 8, 30
    X3 = rng.choice([-2048, 2048, 2047, -1025, 3, -1], size=(batch, h, w, cin))
    D = rng.choice([-2047, 2047, 1025, -3, 1], size=(batch * h * w, cout))
    want_w, want_b = ref.wgrad3x3_f16_exact(X3 // 8, D)         # (the reference asserts S |D| |X3| < 2^24: 3 positions x 2047 x 256)
    (dw, db, bits, k), = run16(dense(X3 // 8), h, w, batch, cin, D, None, 0xFF)
    assert np.array_equal(dw, want_w) and np.array_equal(db, want_b) and k == 4
    X1 = np.zeros_like(X3)
    X1[0, 0, 2, :] = 2048
    (dw, _, _, _), = run16(dense(X1), h, w, batch, cin, D, None, 0xFF)
    assert np.array_equal(dw, ref.wgrad3x3_f16_exact(X1, D)[0])


@pytest.mark.parametrize("power", [-20, 10, -100, 100])
def test_wgrad_f16_scale_follows_the_data(power):
    h, w, batch, cin, cout = 13, 13, 2, 40, 30
    rng, X3, D, scale = TT.exact_case(h, w, batch, cin, cout, seed=3)
    want_w, want_b = ref.wgrad3x3_f16_exact(X3, D, scale)
    Ds = np.ldexp(D.astype(np.float32), power)
    (dw, db, bits, k), = run16(dense(X3), h, w, batch, cin, Ds, scale, 0xFF)
    assert k == ref.k_of(Ds) == 11 - power and bits == ref.max_bits(Ds)
    assert dw.tobytes() == np.ldexp(want_w, power).astype(np.float32).tobytes()
    assert db.tobytes() == np.ldexp(want_b.astype(np.float64), power).astype(np.float32).tobytes()


def test_wgrad_f16_zero_gradient_gives_plus_zero():
    h, w, batch, cin, cout = 3, 5, 2, 40, 30
    rng, X3, D, scale = TT.exact_case(h, w, batch, cin, cout, seed=4)
    for D0 in (np.zeros_like(D, dtype=np.float32), -np.zeros_like(D, dtype=np.float32)):
        (dw, db, bits, k), = run16(dense(X3), h, w, batch, cin, D0, np.abs(scale), 0xFF)
        assert bits == 0 and k == 0 and not dw.view(np.uint32).any() and not db.view(np.uint32).any()


def test_wgrad_f16_narrowing_is_one_rounding_to_nearest_even():
    """X3 one-hot: the centre tap of dW3 at that channel is 2^-k D16[p][.]"""
    rng = np.random.RandomState(9)
    h, w, batch, cin, cout = 3, 5, 1, 8, 72
    P, p0, c0, k = h * w, 7, 5, 11
    # scaled values y = D 2^k: the maximum, ties between neighbours in the normal range and in the subnormal range, ties with zero
    y = [1.5 * 2 ** 14, 1025.5, 1026.5, 2049.0, 2051.0, -1025.5, 3 * 2.0 ** -25, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 5.5 * 2.0 ** -24, -7.5 * 2.0 ** -24,
         2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12), 2.0 ** -26, 1023.5 * 2.0 ** -24, 0.0]
    y = np.concatenate([y, np.exp2(rng.uniform(-24, 14, size=cout - len(y))) * rng.choice([-1.0, 1.0], size=cout - len(y))])
    D = np.ldexp(np.exp2(rng.uniform(-16, 13, size=(P, cout))), -k).astype(np.float32)
    D[p0] = np.ldexp(y.astype(np.float32), -k)
    assert np.array_equal(np.ldexp(D[p0].astype(np.float64), k)[:16], y[:16]) and ref.k_of(D) == k
    assert np.abs(D[p0]).max() / np.abs(D[p0][D[p0] != 0]).min() >= 2.0 ** 30
    X3 = np.zeros((batch, h, w, cin), dtype=np.float16)
    X3[0, p0 // w, p0 % w, c0] = 1.0
    (dw, db, bits, got_k), = run16(dense(X3), h, w, batch, cin, D, None, 0xFF)
    D16 = ref.narrow(D, k)
    assert got_k == k and (D16[p0] == 0).sum() >= 3 and np.isfinite(D16).all()
    assert (np.abs(D16[p0].astype(np.float64)) < 2.0 ** -14).sum() >= 8                  # fp16 subnormals among them
    want = np.ldexp(D16[p0].astype(np.float64), -k).astype(np.float32)
    assert dw[:, 4, c0].tobytes() == want.tobytes()
    others = np.ones(cin, dtype=bool)
    others[c0] = False
    assert not dw[:, 4, others].view(np.uint32).any()


def test_wgrad_f16_subnormal_activations_count():
    """X3 = small integers x 2^-24 (fp16 subnormals), D = powers of two: the exact sum"""
    rng = np.random.RandomState(10)
    h, w, batch, cin, cout = 13, 13, 2, 40, 30
    Xi = rng.randint(-8, 9, size=(batch, h, w, cin))
    X3 = np.ldexp(Xi.astype(np.float64), -24).astype(np.float16)
    assert np.array_equal(np.ldexp(X3.astype(np.float64), 24), Xi) and (np.abs(X3[X3 != 0]) < 6.1e-5).all()
    e = rng.randint(-3, 4, size=(batch * h * w, cout))
    D = (np.exp2(e) * rng.choice([-1.0, 1.0], size=e.shape)).astype(np.float32)
    (dw, db, bits, k), = run16(dense(X3), h, w, batch, cin, D, None, 0xFF)
    T = tail_ref.taps(X3.astype(np.float64))
    want = np.einsum("po,ptc->otc", D.astype(np.float64), T)
    assert k == 11 and np.abs(want).max() > 0
    assert dw.tobytes() == want.astype(np.float32).tobytes() and np.array_equal(want.astype(np.float32), want)


def test_wgrad_f16_nothing_leaks_across_images_rows_or_views():
    rng, X3, D, scale = TT.exact_case(1, 1, 3, 40, 30, seed=6)
    Xn = X3.astype(np.float16)
    Xn[1] = np.nan
    (dw, db, _, _), = run16(dense(Xn), 1, 1, 3, 40, D, scale, 0xFF)
    assert not dw[:, [0, 1, 2, 3, 5, 6, 7, 8], :].view(np.uint32).any() and np.isnan(dw[:, 4, :]).all()
    rng, X3, D, scale = TT.exact_case(5, 1, 2, 8, 30, seed=7)
    (dw, db, _, _), = run16(dense(X3), 5, 1, 2, 8, D, scale, 0xFF)
    assert not dw[:, [0, 2, 3, 5, 6, 8], :].view(np.uint32).any() and np.array_equal(dw, ref.wgrad3x3_f16_exact(X3, D, scale)[0])
    for h, w, batch, cin, cout in ((5, 7, 3, 40, 30), (13, 13, 2, 136, 65)):
        rng, X3, D, scale = TT.exact_case(h, w, batch, cin, cout, seed=7)
        want_w, want_b = ref.wgrad3x3_f16_exact(X3, D, scale)
        for view in VIEWS[1:]:
            flat, ld, coff, istride, start = TT.lay_out(X3.reshape(-1, cin), batch, h * w, cin, view, lambda n: np.full(n, np.nan))
            assert np.isnan(flat).sum() == flat.size - X3.size
            (dw, db, _, _), = run16((flat.astype(np.float16), ld, coff, istride, start), h, w, batch, cin, D, scale, 0xFF)
            assert np.array_equal(dw, want_w) and np.array_equal(db, want_b), (h, w, batch, view)


@pytest.mark.parametrize("shape", ref.REAL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_wgrad_f16_real_values_within_both_bounds(shape):
    """Per element |device - dW64| <= bound1 (the narrowed operands in float64), |device - dWexact| <= bound2 (the un-narrowed sum),
    |db - exact| <= (P + 3) 2^-24 S |D|.  The largest ratios are printed; measured on an MI355X: README.md, "Training"."""
    h, w, batch, cin, cout = shape
    rng = np.random.RandomState(sum(shape))
    P = batch * h * w
    X3 = rng.randn(batch, h, w, cin).astype(np.float16)
    D = (np.exp2(rng.uniform(-20, 8, size=(P, cout))) * rng.choice([-1.0, 1.0], size=(P, cout))).astype(np.float32)
    scale = (rng.uniform(0.5, 2.0, size=cout) * rng.choice([-1.0, 1.0], size=cout)).astype(np.float32)
    (dw, db, bits, k), = run16(dense(X3), h, w, batch, cin, D, scale, 0xFF)
    r = ref.sums64(X3, D, scale)
    assert k == r["k"]
    live = r["bound2"] > 0
    assert np.array_equal(dw[~live], np.zeros_like(dw[~live]))          # taps that never lie inside the image
    live1 = r["bound1"] > 0
    assert not np.abs(dw.astype(np.float64) - r["dW64"])[~live1].any()
    ratio1 = float(np.max(np.abs(dw.astype(np.float64) - r["dW64"])[live1] / r["bound1"][live1]))
    ratio2 = float(np.max(np.abs(dw.astype(np.float64) - r["dWexact"])[live] / r["bound2"][live]))
    ratio_b = float(np.max(np.abs(db.astype(np.float64) - r["db"]) / r["bound_db"]))
    print("conv3x3_wgrad_f16 %s (%d chunks, k = %d): largest |device - ref| / bound: narrowed sums %.4f, un-narrowed sums %.4f, db %.4f"
          % (shape, _hip.conv3x3_wgrad_f16_plan(h, w, batch, cin, cout)["n_chunks"], k, ratio1, ratio2, ratio_b))
    assert ratio1 <= 1 and ratio2 <= 1 and ratio_b <= 1


ERR_ARG, ERR_STATE = 1, 5        # enum yolo_status


def last_error():
    return _hip.lib().yolo_last_error().decode()


def test_wgrad_f16_refusals():
    import torch
    h, w, batch, cin, cout = 3, 5, 1, 8, 4
    pl = _hip.conv3x3_wgrad_f16_plan(h, w, batch, cin, cout)
    x = torch.zeros(batch * h * w * cin + 8, dtype=torch.float16, device="cuda")
    d = torch.zeros((batch * h * w, cout), dtype=torch.float32, device="cuda")
    dw, db = torch.zeros(cout * 9 * cin + 1, dtype=torch.float32, device="cuda"), torch.zeros(cout + 1, dtype=torch.float32, device="cuda")
    s = torch.zeros(pl["scratch_bytes"] + 8, dtype=torch.uint8, device="cuda")
    before = [t.clone() for t in (dw, db, s)]
    good = dict(x=x.data_ptr(), dt=_hip.DTYPE_F16, h=h, w=w, cin=cin, d=d.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr(), s=s.data_ptr(),
                bytes=pl["scratch_bytes"])

    def call(**over):
        a = dict(good, **over)
        return _hip.lib().yolo_conv3x3_wgrad_f16(a["x"], a["dt"], cin, 0, h * w * cin, a["h"], a["w"], batch, a["cin"], a["d"], cout, None, a["dw"],
                                                 a["db"], a["s"], a["bytes"], torch.cuda.current_stream().cuda_stream)

    def refused(rc, text):
        assert rc == ERR_ARG and text in last_error(), (rc, last_error())

    refused(call(dt=_hip.DTYPE_F32), "yolo_conv3x3_wgrad_f16: X3 must be YOLO_DTYPE_F16: a float32 view is yolo_conv3x3_wgrad's")
    refused(call(bytes=pl["scratch_bytes"] - 1),
            "scratch too small: %d bytes, yolo_conv3x3_wgrad_f16_plan asks for %d" % (pl["scratch_bytes"] - 1, pl["scratch_bytes"]))
    refused(call(x=good["x"] + 1), "a pointer is not aligned to its element type")
    for key in ("d", "dw", "db", "s"):
        refused(call(**{key: good[key] + 2}), "a pointer is not aligned to its element type")
    refused(call(x=None), "null argument")
    refused(call(w=ref.MAX_W + 1), "w must be at most %d: the halo of a wider map does not fit LDS" % ref.MAX_W)
    refused(call(cin=12), "cin must be a positive multiple of 8")
    refused(call(h=0), "h, w and batch must be at least 1")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (dw, db, s)))          # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize()


# ---- the mode on a net: a step is its parts, with yolo_conv3x3_wgrad_f16 in the place of yolo_conv3x3_wgrad --------------------------------
def extra_of(eng):
    return eng._wgrad_f16_buf


@pytest.mark.parametrize("name", ["v2-64", "v2-tiny-64"])
def test_tail_step_in_the_mode_is_its_parts(name):
    import torch
    lib = _hip.lib()
    version, hw = TT.NETS[name]
    BATCH, LR = TT.BATCH, TT.LR
    A, n_classes = 5, 20
    cout = A * (5 + n_classes)
    weights = TT.stream_of(version, hw, n_classes)
    net = TT.build(version, hw, "fp16", weights).net
    eng = net.engine
    h, w, _ = net[-1].out.hwc
    P = BATCH * h * w
    _, gt, counts = TT.loss_grad_cases.random_case((h, w, A, n_classes, BATCH), 7)
    x8 = np.random.RandomState(42).randint(0, 256, size=(BATCH,) + hw + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    cin = TT.ytrain.head_counts(net)[1]
    cout3, cin3, pos, n_block = TT.ytrain.tail_counts(net)
    block, w0, b0 = TT.ytrain.split_tail(weights, net)
    eng.set_wgrad_f16(True)                     # before the init ...
    eng.tail_train_init(block, w0, b0)
    before = eng.tail_train_layout()
    lay = eng.tail_layout
    assert bytes(before) == bytes(lay)          # the state layout is what it was
    bview, hview = eng.tail_inputs()
    st = torch.cuda.current_stream().cuda_stream
    hd = eng.head
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(BATCH, -1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
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
    pl16 = _hip.conv3x3_wgrad_f16_plan(h, w, BATCH, cin3, cout3)
    assert extra_of(eng).numel() == lib.yolo_net_train_wgrad_f16_bytes(eng.handle) >= pl16["scratch_bytes"]
    images = torch.empty(BATCH * 56, dtype=torch.uint8, device="cuda")
    assign = torch.empty(P, dtype=torch.int32, device="cuda")
    result = torch.empty(64, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda")
    scratch16 = torch.full((pl16["scratch_bytes"],), 0xFF, dtype=torch.uint8, device="cuda")
    ws = eng._workspace.data_ptr()
    p = lambda k: comp[k].data_ptr()

    def check_parts(tag):
        for k in TT.TAIL_PARTS:
            assert TT.same_bytes(TT.tail_part(eng, k, comp[k].numel() * 4), comp[k]), tag + (k,)
        assert TT.same_bytes(TT.tail_part(eng, "grad", P * cout * 4), comp["grad"]), tag + ("G",)
        assert TT.same_bytes(TT.tail_part(eng, "d", P * cout3 * 4), comp["d"]), tag + ("D",)

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
        _hip.check(lib.yolo_conv3x3_wgrad_f16(ws + bview.offset, bview.dtype, bview.ld, bview.coff, bview.image_stride, h, w, BATCH, cin3, p("d"), cout3,
                                              scale32.data_ptr(), p("dw3"), p("dbeta"), scratch16.data_ptr(), scratch16.numel(), st),
                   "yolo_conv3x3_wgrad_f16")
        _hip.check(lib.yolo_adam_step(p("w"), p("b"), p("m_w"), p("v_w"), p("m_b"), p("v_b"), p("dw"), p("db"), nw, cout, lr_t, 0.9, 0.999, 1e-8, st),
                   "yolo_adam_step")
        _hip.check(lib.yolo_adam_step(p("w3"), p("beta"), p("m_w3"), p("v_w3"), p("m_beta"), p("v_beta"), p("dw3"), p("dbeta"), nw3, cout3, lr_t, 0.9,
                                      0.999, 1e-8, st), "yolo_adam_step")
        want_result = result.cpu().numpy().tobytes()
        got_result = eng.train_tail_step(xf, (gt, counts), lr_t).cpu().numpy().tobytes()
        assert got_result == want_result, (name, t)
        check_parts((name, t))
        assert bool(comp["dw3"].abs().sum() > 0) and bool(torch.isfinite(comp["w3"]).all())
        results.append(got_result)
    # after two steps in the mode the re-packed weight blob is that of a fresh net loaded with the stream tail_train_read gives
    k3, beta2, w2, b2 = eng.tail_train_read()
    second = TT.build(version, hw, "fp16", TT.ytrain.replace_tail(weights, net, k3, beta2, w2, b2)).net.engine
    assert bool(torch.equal(second._weights, eng._weights))
    # the narrowing shows: a float32 twin from the same start holds another dW3 (and the same loss, G, D, dW, db, dbeta at its first step)
    twin = TT.build(version, hw, "fp16", weights).net.engine
    twin.tail_train_init(block, w0, b0)
    assert twin.train_tail_step(xf, (gt, counts), engine.adam_lr_t(LR, 1)).cpu().numpy().tobytes() == results[0]
    # the uint8 twin from the same start, on a state and an extra buffer whose every byte was 0xFF: the same bits
    eng._tail_state.fill_(0xFF)
    extra_of(eng).fill_(0xFF)
    _hip.check(lib.yolo_net_tail_train_init(eng.handle, eng._tail_state.data_ptr(), eng._tail_state.numel(), block.ctypes.data, w0.ctypes.data,
                                            b0.ctypes.data), "yolo_net_tail_train_init")
    for t in (1, 2):
        assert eng.train_tail_step_u8(x8, (gt, counts), engine.adam_lr_t(LR, t)).cpu().numpy().tobytes() == results[t - 1]
    check_parts((name, "u8 on 0xFF"))
    # set_wgrad_f16(False): a step from the same state equals, bit for bit, the step of an engine that never had the mode
    eng.set_wgrad_f16(False)
    assert extra_of(eng) is None
    twin._tail_state.copy_(eng._tail_state)
    twin._weights.copy_(eng._weights)
    lr3 = engine.adam_lr_t(LR, 3)
    assert eng.train_tail_step(xf, (gt, counts), lr3).cpu().numpy().tobytes() == twin.train_tail_step(xf, (gt, counts), lr3).cpu().numpy().tobytes()
    assert bool(torch.equal(eng._tail_state, twin._tail_state)) and bool(torch.equal(eng._weights, twin._weights))
    eng.set_wgrad_f16(True)                     # ... and after it
    twin.train_tail_step(xf, (gt, counts), lr3)
    eng.train_tail_step(xf, (gt, counts), lr3)
    o, n = int(lay.dw3_offset), nw3 * 4
    assert not bool(torch.equal(eng._tail_state[o:o + n], twin._tail_state[o:o + n]))         # the mode is on again: dW3 carries the narrowing


@pytest.mark.parametrize("model", ["v3", "v3-tiny"])
def test_blocks_step_in_the_mode_is_its_parts(model):
    import torch
    import test_gpu_train_blocks_v3 as TB
    lib = _hip.lib()
    BATCH = TB.BATCH
    hw = TB.NETS[model][2]
    weights = TB.stream_of(model)
    gt, counts = TB.yeval.pack_gts(TB.TRUTHS, 3)
    x8 = np.random.RandomState(42).randint(0, 256, size=(BATCH,) + hw + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    m = TB.build(model, "fp16", weights)
    eng = m.net.engine
    heads, blocks = TB.ytrain.head_convs_v3(m.net), TB.ytrain.block_convs_v3(m.net)
    ws0, bs0 = TB.ytrain.split_heads(weights, heads)
    blk0 = TB.ytrain.split_blocks(weights, blocks)
    eng.blocks_train_init_v3(blk0, ws0, bs0)
    eng.set_wgrad_f16(True)
    lay = eng.blocks_layout_v3
    bviews, hviews = eng.block_inputs_v3()
    ns, hd = len(heads), eng.head
    st = torch.cuda.current_stream().cuda_stream
    R, parts = engine.v3_loss_rows(hd)
    width, max_gt = 5 + hd.n_classes, gt.shape[1]
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(BATCH, -1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
    comp, scale32 = {}, []
    z = lambda n: np.zeros(n, np.float32)
    for s, ((_, cout, cin), (_, cout3, cin3)) in enumerate(zip(heads, blocks)):
        b = blk0[s]
        scale64, _ = tail_ref.fold(b[:cout3], b[cout3:2 * cout3], b[2 * cout3:3 * cout3], b[3 * cout3:4 * cout3])
        scale32.append(torch.from_numpy(scale64.astype(np.float32)).cuda())
        nw, nw3 = cout * cin, cout3 * 9 * cin3
        for k, v in (("w", ws0[s].reshape(-1)), ("b", bs0[s]), ("m_w", z(nw)), ("v_w", z(nw)), ("m_b", z(cout)), ("v_b", z(cout)), ("dw", z(nw)), ("db", z(cout)),
                     ("w3", tail_ref.stream_to_otc(b[4 * cout3:], cout3, cin3).reshape(-1)), ("beta", b[:cout3]), ("m_w3", z(nw3)), ("v_w3", z(nw3)),
                     ("m_beta", z(cout3)), ("v_beta", z(cout3)), ("dw3", z(nw3)), ("dbeta", z(cout3))):
            comp[(k, s)] = torch.from_numpy(np.array(v)).cuda()
    pl = _hip.v3_head_wgrad_plan(hd, [cin for _, _, cin in heads], BATCH, hviews[0].dtype)
    need16 = max(_hip.conv3x3_wgrad_f16_plan(hd.h[s], hd.w[s], BATCH, cin3, cout3)["scratch_bytes"] for s, (_, cout3, cin3) in enumerate(blocks))
    assert extra_of(eng).numel() == lib.yolo_net_train_wgrad_f16_bytes(eng.handle) >= need16
    d_parts = torch.empty(BATCH * parts * 56, dtype=torch.uint8, device="cuda")
    images = torch.empty(BATCH * 56, dtype=torch.uint8, device="cuda")
    assign = torch.empty(BATCH * R, dtype=torch.int32, device="cuda")
    result = torch.empty(64, dtype=torch.uint8, device="cuda")
    grad = torch.empty(BATCH * R * width, dtype=torch.float32, device="cuda")
    d = torch.empty(BATCH * max(hd.h[s] * hd.w[s] * blocks[s][1] for s in range(ns)), dtype=torch.float32, device="cuda")
    scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda")
    scratch16 = torch.full((need16,), 0xFF, dtype=torch.uint8, device="cuda")
    ws_ptr = eng._workspace.data_ptr()
    vs = (_hip.V3WgradView * _hip.MAX_SCALES)()
    for s, v in enumerate(hviews):
        vs[s].x_dev, vs[s].image_stride, vs[s].ld, vs[s].coff = ws_ptr + v.offset, v.image_stride, v.ld, v.coff
        vs[s].dtype, vs[s].cin = v.dtype, v.cin
    dws = (C.c_void_p * _hip.MAX_SCALES)(*[comp[("dw", s)].data_ptr() for s in range(ns)])
    dbs = (C.c_void_p * _hip.MAX_SCALES)(*[comp[("db", s)].data_ptr() for s in range(ns)])
    results = []
    for t in (1, 2):
        lr_t = float(engine.adam_lr_t(1e-3, t))
        logits = eng.forward(xf)
        _hip.check(lib.yolo_v3_loss_grad(C.byref(hd), logits.data_ptr(), BATCH, d_gt.data_ptr(), d_gc.data_ptr(), max_gt, 0.7, d_parts.data_ptr(),
                                         images.data_ptr(), assign.data_ptr(), result.data_ptr(), grad.data_ptr(), st), "yolo_v3_loss_grad")
        _hip.check(lib.yolo_v3_head_wgrad(C.byref(hd), vs, BATCH, grad.data_ptr(), assign.data_ptr(), max_gt, dws, dbs, scratch.data_ptr(),
                                          scratch.numel(), st), "yolo_v3_head_wgrad")
        for s, ((_, cout, cin), (_, cout3, cin3)) in enumerate(zip(heads, blocks)):
            hv, bv = hviews[s], bviews[s]
            _hip.check(lib.yolo_v3_head_dgrad(C.byref(hd), s, grad.data_ptr(), assign.data_ptr(), max_gt, BATCH, comp[("w", s)].data_ptr(), cin,
                                              ws_ptr + hv.offset, hv.dtype, hv.ld, hv.coff, hv.image_stride, 0.1, d.data_ptr(), st), "yolo_v3_head_dgrad")
            _hip.check(lib.yolo_conv3x3_wgrad_f16(ws_ptr + bv.offset, bv.dtype, bv.ld, bv.coff, bv.image_stride, bv.h, bv.w, BATCH, cin3, d.data_ptr(),
                                                  cout3, scale32[s].data_ptr(), comp[("dw3", s)].data_ptr(), comp[("dbeta", s)].data_ptr(),
                                                  scratch16.data_ptr(), scratch16.numel(), st), "yolo_conv3x3_wgrad_f16")
        for s, ((_, cout, cin), (_, cout3, cin3)) in enumerate(zip(heads, blocks)):
            _hip.check(lib.yolo_adam_step(*[comp[(k, s)].data_ptr() for k in TB.HEAD_KEYS], cout * cin, cout, lr_t, 0.9, 0.999, 1e-8, st), "yolo_adam_step")
            _hip.check(lib.yolo_adam_step(*[comp[(k, s)].data_ptr() for k in TB.BLOCK_KEYS], cout3 * 9 * cin3, cout3, lr_t, 0.9, 0.999, 1e-8, st),
                       "yolo_adam_step")
        want_result = result.cpu().numpy().tobytes()
        got_result = eng.train_blocks_step_v3(xf, (gt, counts), lr_t).cpu().numpy().tobytes()
        assert got_result == want_result, (model, t)
        got = TB.blocks_state_parts(eng, BATCH)
        assert got["grad"] == grad.cpu().numpy().tobytes(), (model, t, "G")
        assert got["d"] == d.cpu().numpy().tobytes()[:len(got["d"])], (model, t, "D")
        for k, v in comp.items():
            assert got[k] == v.cpu().numpy().tobytes(), (model, t, k)
        assert all(bool(comp[("dw3", s)].abs().sum() > 0) and bool(torch.isfinite(comp[("w3", s)]).all()) for s in range(ns))
        results.append(got_result)
    after_float = TB.blocks_state_parts(eng, BATCH)
    k3, beta2, ws2, bs2 = eng.blocks_train_read_v3()
    second = TB.build(model, "fp16", TB.ytrain.replace_head_blocks(weights, blocks, heads, k3, beta2, ws2, bs2)).net.engine
    assert bool(torch.equal(second._weights, eng._weights))
    # the uint8 twin on a 0xFF-filled state and a 0xFF-filled extra buffer
    eng._blocks_state_v3.fill_(0xFF)
    extra_of(eng).fill_(0xFF)
    TB.blocks_init_in_place(eng, blk0, ws0, bs0)
    for t in (1, 2):
        assert eng.train_blocks_step_v3_u8(x8, (gt, counts), engine.adam_lr_t(1e-3, t)).cpu().numpy().tobytes() == results[t - 1]
    assert TB.blocks_state_parts(eng, BATCH) == after_float
    # back to float32: a step from the same state is the step of an engine that never had the mode
    twin = TB.build(model, "fp16", weights).net.engine
    twin.blocks_train_init_v3(blk0, ws0, bs0)
    eng.set_wgrad_f16(False)
    twin._blocks_state_v3.copy_(eng._blocks_state_v3)
    twin._weights.copy_(eng._weights)
    lr3 = engine.adam_lr_t(1e-3, 3)
    a = eng.train_blocks_step_v3(xf, (gt, counts), lr3).cpu().numpy().tobytes()
    assert a == twin.train_blocks_step_v3(xf, (gt, counts), lr3).cpu().numpy().tobytes()
    assert bool(torch.equal(eng._blocks_state_v3, twin._blocks_state_v3)) and bool(torch.equal(eng._weights, twin._weights))


class ResidualTail(TT.YoloV2):
    """the small tail with a shortcut fused into its block: no block to train"""
    create_network = staticmethod(lambda *a, **k: TT.cases.small_tail_network(*a, residual=True, **k))


def test_set_wgrad_f16_refuses_a_float32_plan_and_a_net_without_a_block():
    hw = (64, 64)
    e32 = TT.build("small", hw, "fp32", TT.stream_of("small", hw, 20)).net.engine
    with pytest.raises(_hip.YoloHipError, match="a float32 plan stores float32 activations"):
        e32.set_wgrad_f16(True)
    e32.set_wgrad_f16(False)
    res = ResidualTail()
    res.build(TT.V2_ANCHORS, TT.NAMES20, hw + (3,), dtype="fp16", max_batch=2, streams=1)
    with pytest.raises(_hip.YoloHipError, match="residual"):
        res.net.engine.set_wgrad_f16(True)


# ---- it trains ---------------------------------------------------------------------------------------------------------------------------
def test_twenty_steps_in_the_mode_lower_the_loss_and_stay_beside_the_float32_mode():
    """The tail test's fixed batch (tests/test_gpu_train_tail.py: the small tail at 64 x 64, fp16, batch 4, one class, lr 1e-4), twenty steps
    in the mode and twenty in the float32 mode from the same start.  dist(a, b): the largest relative distance of the per-step losses.
    Asserted: the mode lowers the loss at every step, and
        dist(device fp16 mode, device float32 mode) <= 4 d_narrow + 2 dist(float32 yardstick loop, float64 yardstick loop)
    with d_narrow the distance of the float64 yardstick loops with and without the narrowing, all on the device's stored block input.
    The three distances are printed; measured on an MI355X: README.md, "Training"."""
    import torch
    hw, n_classes, B, steps, lr = (64, 64), 1, 4, 20, 1e-4
    weights = TT.stream_of("small", hw, n_classes)
    losses = {}
    for mode in ("fp16", "fp32"):
        m = TT.build("small", hw, "fp16", weights, names=["tower"], max_batch=B)
        eng = m.net.engine
        h, w, cout = m.net[-1].out.hwc
        _, gt, counts = TT.loss_grad_cases.random_case((h, w, 5, n_classes, B), 7)
        x = TT.synth.synthetic_input(B, hw[0], hw[1], 3, seed=44)
        cout3, cin3, pos, n_block = TT.ytrain.tail_counts(m.net)
        block, w0, b0 = TT.ytrain.split_tail(weights, m.net)
        eng.tail_train_init(block, w0, b0)
        eng.set_wgrad_f16(mode == "fp16")
        eng.forward(x)
        torch.cuda.synchronize()
        bview, _ = eng.tail_inputs()
        flat = eng._workspace[bview.offset:bview.offset + 2 * B * bview.image_stride].cpu().numpy().view(np.float16)
        idx = (np.arange(B)[:, None, None] * bview.image_stride + np.arange(h * w)[None, :, None] * bview.ld + bview.coff + np.arange(cin3)[None, None, :])
        X3 = flat[idx].reshape(B, h, w, cin3)
        records = torch.empty((steps, 64), dtype=torch.uint8, device="cuda")
        for t in range(1, steps + 1):
            eng.train_tail_step(x, (gt, counts), engine.adam_lr_t(lr, t), result=records[t - 1])
        losses[mode] = np.array([float(r["loss"]) for r in records.cpu().numpy().view(TT.yeval.LOSS_RESULT_DTYPE).reshape(-1)])
    blk = (block[:cout3], block[cout3:2 * cout3], block[2 * cout3:3 * cout3], block[3 * cout3:4 * cout3], tail_ref.stream_to_otc(block[4 * cout3:], cout3, cin3))
    head = (X3, blk, w0, b0, h, w, TT.V2_ANCHORS, n_classes, gt, counts)
    rate, narrowed, plain, d_narrow = ref.narrowed_loops(head + (steps, np.float16), lr)
    ref32 = tail_ref.tail_train_loop(*head, lr, steps, np.float16, mode="float32")[0]
    d_dev, d_ref = ref.dist(losses["fp16"], losses["fp32"]), ref.dist(ref32, plain)
    print("fp16 mode :", " ".join("%.6f" % v for v in losses["fp16"]))
    print("fp32 mode :", " ".join("%.6f" % v for v in losses["fp32"]))
    print("dist(device fp16 mode, device float32 mode) = %.3e; d_narrow = %.3e; dist(float32 loop, float64 loop) = %.3e; bound %.3e"
          % (d_dev, d_narrow, d_ref, 4 * d_narrow + 2 * d_ref))
    dev = losses["fp16"]
    assert rate == lr and np.isfinite(dev).all() and all(a > c for a, c in zip(dev, dev[1:])), dev
    assert d_dev <= ref.FACTOR * d_narrow + 2 * d_ref, (d_dev, d_narrow, d_ref)


# ---- train mode --------------------------------------------------------------------------------------------------------------------------
def test_launcher_mode_train_with_wgrad_fp16(tmp_path, capsys):
    """tiny-YOLOv2 with the keys of config/yolo_2_tail_train_f16.ini: the reference's lines, and a first loss with the bits of the step entry in
    the mode"""
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
            (tmp_path / d / ("im%d.xml" % i)).write_text(TT.VOC_XML % (fname, 200, 120, x1, y1, x1 + int(rng.randint(20, 100)), y1 + int(rng.randint(20, 60))))
    full = TT.stream_of("v2-tiny", hw, 1)
    TT.base.write_darknet_weights(str(tmp_path / "full.weights"), full, "v2")
    (tmp_path / "cfg.ini").write_text(
        "[COMMON]\nversion = v2-tiny\ninput_h = %d\ninput_w = %d\ninput_c = 3\n"
        "[TRAIN]\ntrain_layers = tail\nwgrad = fp16\nseed = 3\nimage_dir = train/\nannotation_dir = train/\nval_image_dir = val/\nval_annotation_dir = val/\n"
        "batch_size = 2\nlearning_rate = 1e-3\nepochs = 2\nmax_step = -1\naugment_probability = 0.0\ncheckpoint_dir = out/\ncheckpoint_step = 1\n"
        "checkpoint_prefix = yolo\ntensorboard_log_dir =\npretrained_weights_path = full.weights\nanchors = %s\nclass_names = [\"tower\"]\n"
        "cpu_only = False\ndtype = fp16\n" % (hw[0], hw[1], list(TT.V2_ANCHORS)))
    TT.launcher.run(TT.launcher.read_config(str(tmp_path / "cfg.ini")), "train")
    out = capsys.readouterr().out.splitlines()
    steps = [l for l in out if l.startswith("step ")]
    assert len(steps) == 2 and steps[0].startswith("step 1 (1/2): ") and steps[1].startswith("step 2 (2/2): ") and "(moving average: " in steps[1]
    assert sum(l.startswith("validation loss: ") for l in out) == 2 and out[-1] == "Done" and "Epoch (2/2) completed." in out
    assert "Pre-trained weights loaded." in out and "3 x 3 weight gradients on the fp16 matrix cores." in out
    ann, _ = TT.yeval.parse_voc_annotations(str(tmp_path / "train"), str(tmp_path / "train"), ["tower"])
    batch, = TT.ytrain.make_batches(ann, 2, random.Random(3))
    steps_of = {}
    for mode in (True, False):
        m = TT.build("v2-tiny", hw, "fp16", full, names=["tower"], max_batch=2)
        eng = m.net.engine
        eng.tail_train_init(*TT.ytrain.split_tail(full, m.net))
        eng.set_wgrad_f16(mode)
        x, truths = TT.ytrain.batch_to_device(eng, batch)
        rec = eng.train_tail_step_u8(x, truths, engine.adam_lr_t(1e-3, 1)).cpu().numpy().view(TT.yeval.LOSS_RESULT_DTYPE)[0]
        steps_of[mode] = "step 1 (1/2): {} (moving average: {})".format(np.float32(rec["loss"]), np.float32(rec["loss"]))
        if mode:        # the first checkpoint holds the master values of a step in the mode, and not those of a float32 step
            _, body1 = TT.base.read_darknet_weights(str(tmp_path / "out" / "yolo-1.weights"), "v2")
            in_mode = TT.ytrain.replace_tail(full, m.net, *eng.tail_train_read())
            assert body1.tobytes() == in_mode.tobytes()
        else:
            assert TT.ytrain.replace_tail(full, m.net, *eng.tail_train_read()).tobytes() != in_mode.tobytes()
    assert steps[0] == steps_of[True]
    assert sorted(TT.os.listdir(str(tmp_path / "out"))) == ["yolo-%d.weights" % s for s in (0, 1, 2)]


def test_launcher_mode_train_with_wgrad_fp16_head_blocks(tmp_path, capsys):
    """YOLOv3-tiny with the keys of config/yolo_3_head_blocks_train_f16.ini: the reference's lines, a first loss with the bits of the step entry
    in the mode, and a first checkpoint that holds the master values of a step in the mode"""
    import random
    from PIL import Image
    import test_gpu_train_blocks_v3 as TB
    rng = np.random.RandomState(52)
    hw = TB.NETS["v3-tiny"][2]
    for d in ("train", "val", "out"):
        (tmp_path / d).mkdir()
    for d in ("train", "val"):
        for i in range(2):
            name = "im%d.png" % i
            Image.fromarray(rng.randint(0, 256, size=(120, 200, 3)).astype(np.uint8)).save(str(tmp_path / d / name))
            x1, y1 = int(rng.randint(0, 100)), int(rng.randint(0, 60))
            (tmp_path / d / ("im%d.xml" % i)).write_text(TB.VOC_XML % (name, 200, 120, TB.NAMES3[i], x1, y1, x1 + int(rng.randint(20, 100)),
                                                                      y1 + int(rng.randint(20, 60))))
    full = TB.stream_of("v3-tiny")
    TB.base.write_darknet_weights(str(tmp_path / "full.weights"), full, "v3")
    (tmp_path / "cfg.ini").write_text(
        "[COMMON]\nversion = v3-tiny\ninput_h = %d\ninput_w = %d\ninput_c = 3\n"
        "[TRAIN]\ntrain_layers = head_blocks\nwgrad = fp16\nignore_thresh = 0.6\nseed = 3\nimage_dir = train/\nannotation_dir = train/\nval_image_dir = val/\n"
        "val_annotation_dir = val/\nbatch_size = 2\nlearning_rate = 1e-3\nepochs = 2\nmax_step = -1\naugment_probability = 0.0\n"
        "checkpoint_dir = out/\ncheckpoint_step = 1\ncheckpoint_prefix = yolo\ntensorboard_log_dir =\npretrained_weights_path = full.weights\n"
        "anchors = %s\nclass_names = %s\ncpu_only = False\ndtype = fp16\n" % (hw[0], hw[1], TB.TINY_ANCHORS, str(TB.NAMES3).replace("'", '"')))
    TB.launcher.run(TB.launcher.read_config(str(tmp_path / "cfg.ini")), "train")
    out = capsys.readouterr().out.splitlines()
    steps = [l for l in out if l.startswith("step ")]
    assert len(steps) == 2 and steps[0].startswith("step 1 (1/2): ") and steps[1].startswith("step 2 (2/2): ") and "(moving average: " in steps[1]
    assert sum(l.startswith("validation loss: ") for l in out) == 2 and out[-1] == "Done" and "Epoch (2/2) completed." in out
    assert "Pre-trained weights loaded." in out and "3 x 3 weight gradients on the fp16 matrix cores." in out
    ann, _ = TB.yeval.parse_voc_annotations(str(tmp_path / "train"), str(tmp_path / "train"), TB.NAMES3)
    batch, = TB.ytrain.make_batches(ann, 2, random.Random(3))
    _, body1 = TB.base.read_darknet_weights(str(tmp_path / "out" / "yolo-1.weights"), "v3")
    streams = {}
    for mode in (True, False):
        m = TB.build("v3-tiny", "fp16", full, max_batch=2)
        eng = m.net.engine
        heads, blocks = TB.ytrain.head_convs_v3(m.net), TB.ytrain.block_convs_v3(m.net)
        eng.set_wgrad_f16(mode)
        eng.blocks_train_init_v3(TB.ytrain.split_blocks(full, blocks), *TB.ytrain.split_heads(full, heads))
        x, truths = TB.ytrain.batch_to_device(eng, batch)
        rec = eng.train_blocks_step_v3_u8(x, truths, engine.adam_lr_t(1e-3, 1), 0.6).cpu().numpy().view(TB.yeval.LOSS_RESULT_DTYPE)[0]
        assert steps[0] == "step 1 (1/2): {} (moving average: {})".format(np.float32(rec["loss"]), np.float32(rec["loss"]))
        streams[mode] = TB.ytrain.replace_head_blocks(full, blocks, heads, *eng.blocks_train_read_v3()).tobytes()
    assert body1.tobytes() == streams[True] and streams[True] != streams[False]

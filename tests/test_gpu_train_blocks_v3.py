"""GPU: the sparse data gradient of one YOLOv3 head conv (include/yolo_hip.h: yolo_v3_head_dgrad), through the C ABI, against
tests/blocks_v3_ref.py, and the 3 x 3 weight gradient (yolo_conv3x3_wgrad, unchanged) on the wide maps the blocks behind the YOLOv3 heads
have; the shapes come from tests/blocks_v3_cases.py, which tests/test_train_blocks_v3_cpu.py checks against the library's plans.

Every device output lies in a buffer with a 256-byte 0xA5 guard band on both sides; outputs and scratch are pre-filled with 0x00 and with
0xFF bytes.

  dgrad exact   integer G and W (|values| <= 8, at most 3 * 85 terms: every sum below 2^24) with hand-made assign tables: D EQUALS the
                float32 reference, the slope factor as one float32 multiply; every winner pattern; Y dense, sliced and unaligned, fp16 and
                float32, with +0, -0, negatives and positives; Y null
  poison        NaN in every element of G the table declares a structural zero: the same bits
  dense route   on integers, yolo_conv1x1_dgrad on the gathered G_s (its structural zeros +0) returns the same bits
  real          |device - ref64| / ((T + 2) 2^-24 |factor| S |G| |W|) <= 1.  Measured on an MI355X: see README.md
  wide wgrad    integer D and X3 at 3 x 26, 2 x 38, 2 x 76, 2 x 80: dW3 and db EQUAL the integer reference; 2 x 81 is refused
  step          yolo_net_train_blocks_step_v3 is forward -> yolo_v3_loss_grad -> yolo_v3_head_wgrad -> per scale yolo_v3_head_dgrad and
                yolo_conv3x3_wgrad -> yolo_adam_step per conv, bit for bit; its uint8 twin on a state that was all 0xFF; the re-pack: the
                device weight blob equals that of a net loaded with the stream rebuilt from the master values, byte for byte; head-only
                training sees the same first record
  it trains     20 steps on a fixed batch lower the loss at every step, beside the float64 and float32 loops of tests/blocks_v3_ref.py on
                the device's block inputs
  call order    a step, detect, a step equals a fresh engine's two steps
  train mode    launcher --mode train with train_layers = head_blocks"""
import ctypes as C

import numpy as np
import pytest

import blocks_v3_cases as cases
import blocks_v3_ref as ref
import tail_ref
import train_v3_ref
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 256, 0xA5
NP_DTYPES = (np.float16, np.float32)


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


def head_of(grids, A, n_classes):
    return engine.head_desc_v3(grids, [[(1. + a, 2. + a) for a in range(A)] for _ in grids], n_classes)


def plan(grids, A, n_classes, scale, cin, batch):
    return _hip.head_dgrad_plan(head_of(grids, A, n_classes), scale, cin, batch)


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


class Operands(object):
    """G, the table and W of one call on the device, uploaded once"""

    def __init__(self, grids, A, n_classes, scale, G, table, W):
        import torch
        self.hd, self.scale, self.batch = head_of(grids, A, n_classes), scale, G.shape[0]
        self.P, self.cin = self.batch * grids[scale][0] * grids[scale][1], W.shape[1]
        self.g = torch.from_numpy(np.ascontiguousarray(G, dtype=np.float32)).cuda()
        self.t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda()
        self.w = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)).cuda()

    def run(self, y, max_gt=cases.MAX_GT, slope=0.1, fill=0x00, g=None):
        """y: None or (flat np array of the view's dtype, ld, coff, image_stride, start) -> D [P, cin]"""
        import torch
        out = guarded(self.P * self.cin * 4, fill)
        if y is None:
            yp, ydt, ld, coff, istride = None, 0, 0, 0, 0
        else:
            flat, ld, coff, istride, start = y
            d_y = torch.from_numpy(flat).cuda()
            yp, ydt = d_y.data_ptr() + start * d_y.element_size(), (_hip.DTYPE_F16 if flat.dtype == np.float16 else _hip.DTYPE_F32)
        _hip.check(_hip.lib().yolo_v3_head_dgrad(C.byref(self.hd), self.scale, (self.g if g is None else g).data_ptr(), self.t.data_ptr(), max_gt,
                                                 self.batch, self.w.data_ptr(), self.cin, yp, ydt, ld, coff, istride, slope, out[1],
                                                 torch.cuda.current_stream().cuda_stream), "yolo_v3_head_dgrad")
        torch.cuda.synchronize()
        check_guards([out])
        return payload(out, (self.P, self.cin))


# ---- yolo_v3_head_dgrad: exact, poison, the dense route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in cases.DGRAD_CASES] + ["cin1024-second-round"])
def test_dgrad_equals_the_float32_reference_clean_and_poisoned(name):
    import torch
    table_of_cases = cases.DGRAD_CASES + (cases.loop_case(plan),)
    _, grids, A, n_classes, scale, cin, batch = [c for c in table_of_cases if c[0] == name][0]
    R, scales = train_v3_ref.scales_of(grids, A)
    row0, h, w, _ = scales[scale]
    assert scale == 0 or row0 > 0
    ppi, P, width = h * w, batch * h * w, 5 + n_classes
    rng = np.random.RandomState(sum(map(ord, name)))
    W = rng.randint(-8, 9, size=(A * width, cin)).astype(np.float32)
    Y = cases.y_values(rng, P * cin).reshape(P, cin)
    runs = 0
    for i, pattern in enumerate(cases.PATTERNS):
        table = cases.make_table(pattern, grids, A, batch, rng, scale)
        G = cases.integer_g(table, width, rng)
        Gp = cases.integer_g(table, width, np.random.RandomState(0), poison=True)
        Gp[~np.isnan(Gp)] = G[~np.isnan(Gp)]
        assert np.isnan(Gp).any() and np.array_equal(np.isnan(Gp), ~train_v3_ref.terms(table, width, cases.MAX_GT))
        want_plain = ref.head_dgrad(G, table, W, scales[scale], cases.MAX_GT, None, mode="float32")
        want = ref.head_dgrad(G, table, W, scales[scale], cases.MAX_GT, Y, mode="float32")
        assert np.abs(want_plain).max() < 2 ** 24 and want.tobytes() == ref.head_dgrad(Gp, table, W, scales[scale], cases.MAX_GT, Y).tobytes()
        ops = Operands(grids, A, n_classes, scale, G, table, W)
        poisoned = torch.from_numpy(Gp).cuda()
        for fill in (0x00, 0xFF):
            assert np.array_equal(ops.run(None, fill=fill), want_plain), (name, pattern, "no Y", fill)
        assert ops.run(None, fill=0xFF, g=poisoned).tobytes() == want_plain.tobytes(), (name, pattern, "no Y", "poisoned")
        runs += 3
        for j, view in enumerate(cases.VIEWS):
            flat, ld, coff, istride, start = lay_out(Y, batch, ppi, cin, view, lambda n: cases.y_values(rng, n))
            for np_dtype in NP_DTYPES:
                # every pattern runs clean and poisoned; the first one on all views and types, the others on one view and type each
                if i and (j != i % len(cases.VIEWS) or np_dtype != NP_DTYPES[i % 2]):
                    continue
                y = (flat.astype(np_dtype), ld, coff, istride, start)
                tag = (name, pattern, view, np_dtype.__name__)
                for fill in (0x00, 0xFF):
                    assert ops.run(y, fill=fill).tobytes() == want.tobytes(), tag + (fill,)
                assert ops.run(y, fill=0xFF, g=poisoned).tobytes() == want.tobytes(), tag + ("poisoned",)
                runs += 3
        if pattern in ("full-image", "all-anchors"):        # the dense route on the gathered G_s returns the same bits
            Gs, _ = ref.gathered(G, table, scales[scale], cases.MAX_GT)
            dense = engine.conv1x1_dgrad(torch.from_numpy(Gs).cuda(), ops.w, torch.from_numpy(Y.astype(np.float16).reshape(batch, h, w, cin)).cuda())
            torch.cuda.synchronize()
            assert dense.cpu().numpy().tobytes() == want.tobytes(), (name, pattern, "dense route")
    print("%s: %d calls, plan %s" % (name, runs, plan(grids, A, n_classes, scale, cin, batch)))


def test_dgrad_signed_zeros_take_the_slope_and_other_slopes_multiply_once():
    grids, A, n_classes = ((1, 1), (1, 3)), 2, 1
    R, scales = train_v3_ref.scales_of(grids, A)
    table = np.full((1, R), -1, dtype=np.int32)
    table[0, scales[1][0] + 2] = 5                      # anchor 0 of the middle cell of scale 1
    G = np.full((1, R, 6), 3.0, dtype=np.float32)
    W = np.full((12, 8), 7.0, dtype=np.float32)
    Y = np.array([[0.0, -0.0, -1.0, 1.0, 6e-8, -6e-8, 65504.0, -65504.0]] * 3)
    ops = Operands(grids, A, n_classes, 1, G, table, W)
    for slope in (0.1, 0.0, -0.25, 1.0):
        want = ref.head_dgrad(G, table, W, scales[1], cases.MAX_GT, Y.astype(np.float16), slope)
        assert want[0, 3] == 42.0 and want[1, 3] == 147.0 and want[1, 0] == np.float32(147.0) * np.float32(slope)
        for np_dtype in NP_DTYPES:
            got = ops.run((Y.astype(np_dtype).reshape(-1), 8, 0, 24, 0), slope=slope, fill=0xFF)
            assert got.tobytes() == ref.head_dgrad(G, table, W, scales[1], cases.MAX_GT, Y.astype(np_dtype), slope).tobytes(), (slope, np_dtype.__name__)
    # max_gt decides what a winner is: the entry 5 names no truth under max_gt = 5
    assert np.array_equal(ops.run(None, max_gt=5), ref.head_dgrad(G, table, W, scales[1], 5))
    assert ops.run(None, max_gt=5)[1, 0] == 42.0 and ops.run(None, max_gt=6)[1, 0] == 147.0


def test_dgrad_nan_outside_the_view_changes_no_bit():
    _, grids, A, n_classes, scale, cin, batch = cases.DGRAD_CASES[4]
    R, scales = train_v3_ref.scales_of(grids, A)
    _, h, w, _ = scales[scale]
    rng = np.random.RandomState(11)
    table = cases.make_table("full-image", grids, A, batch, rng, scale)
    G = cases.integer_g(table, 5 + n_classes, rng)
    W = rng.randint(-8, 9, size=(A * (5 + n_classes), cin)).astype(np.float32)
    Y = cases.y_values(rng, batch * h * w * cin).reshape(-1, cin)
    want = ref.head_dgrad(G, table, W, scales[scale], cases.MAX_GT, Y)
    ops = Operands(grids, A, n_classes, scale, G, table, W)
    for view in cases.VIEWS[1:]:
        flat, ld, coff, istride, start = lay_out(Y, batch, h * w, cin, view, lambda n: np.full(n, np.nan))
        assert np.isnan(flat).sum() == flat.size - Y.size
        for np_dtype in NP_DTYPES:
            assert ops.run((flat.astype(np_dtype), ld, coff, istride, start), fill=0xFF).tobytes() == want.tobytes(), (view, np_dtype.__name__)


# ---- real values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.REAL_CASES, ids=lambda c: c[0])
def test_dgrad_real_values_within_the_float32_bound(case):
    """G as the loss leaves it in magnitude (|G| log-uniform over 2^-20 .. 2^8), W ~ N(0, 1 / cin), Y ~ N(0, 1) in fp16; max_gt truths per
    image.  The bound is the header's: the chain of T fmaf and the one multiply."""
    import torch
    name, grids, A, n_classes, scale, cin, batch = case
    max_gt = 8
    rng = np.random.RandomState(len(name))
    R, scales = train_v3_ref.scales_of(grids, A)
    row0, h, w, _ = scales[scale]
    width = 5 + n_classes
    table = np.where(rng.uniform(size=(batch, R)) < 0.1, -2, -1).astype(np.int32)
    for n in range(batch):
        table[n, row0 + rng.choice(h * w * A, size=max_gt, replace=False)] = rng.permutation(max_gt)
    G = (np.exp2(rng.uniform(-20, 8, size=(batch, R, width))) * rng.choice([-1.0, 1.0], size=(batch, R, width))).astype(np.float32)
    G[table == -2, 4] = 0
    G[~train_v3_ref.terms(table, width, max_gt)] = np.nan
    W = (rng.randn(A * width, cin) / np.sqrt(cin)).astype(np.float32)
    Y = rng.randn(batch, h, w, cin).astype(np.float16)
    got = engine.v3_head_dgrad(head_of(grids, A, n_classes), scale, torch.from_numpy(G).cuda(), torch.from_numpy(table).cuda(), max_gt,
                               torch.from_numpy(W).cuda(), torch.from_numpy(Y).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy().astype(np.float64)
    want, bound = ref.head_dgrad_ref64(G, table, W, scales[scale], max_gt, Y.reshape(-1, cin))
    assert np.isfinite(got).all() and ((bound > 0) | (got == 0)).all()
    ratio = float(np.max(np.abs(got - want)[bound > 0] / bound[bound > 0]))
    print("%s: max |device - ref64| / bound = %.4f over %d elements" % (name, ratio, got.size))
    assert ratio <= 1.0


# ---- yolo_conv3x3_wgrad on wide maps --------------------------------------------------------------------------------------------------------
def run_wgrad(x, h, w, batch, cin, D, fill):
    import torch
    flat, ld, coff, istride, start = x
    dtype = _hip.DTYPE_F16 if flat.dtype == np.float16 else _hip.DTYPE_F32
    cout = D.shape[1]
    pl = _hip.conv3x3_wgrad_plan(h, w, batch, cin, cout, dtype)
    d_x = torch.from_numpy(flat).cuda()
    d_d = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32)).cuda()
    bufs = [guarded(cout * 9 * cin * 4, fill), guarded(cout * 4, fill), guarded(pl["scratch_bytes"], fill)]
    _hip.check(_hip.lib().yolo_conv3x3_wgrad(d_x.data_ptr() + start * d_x.element_size(), dtype, ld, coff, istride, h, w, batch, cin,
                                             d_d.data_ptr(), cout, None, bufs[0][1], bufs[1][1], bufs[2][1], pl["scratch_bytes"],
                                             torch.cuda.current_stream().cuda_stream), "yolo_conv3x3_wgrad")
    torch.cuda.synchronize()
    check_guards(bufs)
    return payload(bufs[0], (cout, 9, cin)), payload(bufs[1], (cout,))


@pytest.mark.parametrize("shape", cases.WIDE_WGRAD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_wgrad_equals_the_integer_reference_on_wide_maps(shape):
    h, w, batch, cin, cout = shape
    rng = np.random.RandomState(sum(shape))
    X3 = rng.randint(-8, 9, size=(batch, h, w, cin))
    X3[X3 == 0] = 5                 # no zeros: a tap that leaks across a row end or an image end, or a dropped one, changes a sum
    D = rng.randint(-8, 9, size=(batch * h * w, cout))
    D[D == 0] = -3
    if batch > 1:
        assert not np.array_equal(X3[0], X3[1])
    want_w, want_b = tail_ref.wgrad3x3_exact(X3, D)
    for i, view in enumerate(cases.VIEWS):
        flat, ld, coff, istride, start = lay_out(X3.reshape(-1, cin), batch, h * w, cin, view, lambda n: rng.randint(-8, 9, size=n))
        np_dtype = NP_DTYPES[i % 2]
        for fill in (0x00, 0xFF):
            dw, db = run_wgrad((flat.astype(np_dtype), ld, coff, istride, start), h, w, batch, cin, D, fill)
            assert np.array_equal(dw, want_w) and np.array_equal(db, want_b), (shape, view, np_dtype.__name__, fill)


def test_wgrad_refuses_a_map_wider_than_80():
    import torch
    h, w, batch, cin, cout = cases.WIDE_WGRAD_REFUSED
    t = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    rc = _hip.lib().yolo_conv3x3_wgrad(t.data_ptr(), _hip.DTYPE_F32, cin, 0, h * w * cin, h, w, batch, cin, t.data_ptr(), cout, None, t.data_ptr(),
                                       t.data_ptr(), t.data_ptr(), t.numel() * 4, None)
    assert rc == 1 and "w must be at most 80" in _hip.lib().yolo_last_error().decode()


# ---- the step on a net ------------------------------------------------------------------------------------------------------------------
import functools                                                                              # noqa: E402
import os                                                                                     # noqa: E402

from tensorflow_yolo_amd import YoloV3, YoloV3Tiny, launcher                                  # noqa: E402
from tensorflow_yolo_amd.net import base, evaluate as yeval, synth, train as ytrain          # noqa: E402

NAMES3 = ["a", "b", "c"]
TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
NETS = {"v3": (YoloV3, V3_ANCHORS, (64, 64)), "v3-tiny": (YoloV3Tiny, TINY_ANCHORS, (96, 160))}
BATCH = 3
TRUTHS = [[(0.3, 0.4, 0.2, 0.5, 1), (0.8, 0.2, 0.3, 0.3, 2), (0.5, 0.5, 0.9, 0.9, 0)], [], [(0.6, 0.6, 0.1, 0.15, 0), (0.1, 0.9, 0.05, 0.08, 2)]]
HEAD_KEYS = ("w", "b", "m_w", "v_w", "m_b", "v_b", "dw", "db")
BLOCK_KEYS = ("w3", "beta", "m_w3", "v_w3", "m_beta", "v_beta", "dw3", "dbeta")


@functools.lru_cache(maxsize=None)
def stream_of(model):
    cls, anchors, hw = NETS[model]
    net = cls.create_network(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=hw + (3,))
    w = synth.darknet_stream(net, seed=41, num_classes=3)
    w.setflags(write=False)
    return w


def build(model, dtype, weights, max_batch=BATCH):
    cls, anchors, hw = NETS[model]
    m = cls()
    m.build(anchors, NAMES3, hw + (3,), dtype=dtype, max_batch=max_batch, weights=weights, streams=1)
    return m


def blocks_state_parts(eng, batch):
    """the parts of the engine's blocks-training state a step leaves behind, as bytes: per scale the eight arrays of the head conv and of
    the block; G; the D of the last scale"""
    lay = eng.blocks_layout_v3
    raw = eng._blocks_state_v3.cpu().numpy()
    out = {}
    for s in range(lay.n_scales):
        nw, nb, nw3, nb3 = lay.cout[s] * lay.cin[s] * 4, lay.cout[s] * 4, lay.cout3[s] * 9 * lay.cin3[s] * 4, lay.cout3[s] * 4
        for keys, n_w, n_b in ((HEAD_KEYS, nw, nb), (BLOCK_KEYS, nw3, nb3)):
            for k in keys:
                at = int(getattr(lay, k + "_offset")[s])
                out[(k, s)] = raw[at:at + (n_w if k.endswith(("w", "w3")) else n_b)].tobytes()
    R, _ = engine.v3_loss_rows(eng.head)
    out["grad"] = raw[int(lay.grad_offset):int(lay.grad_offset) + batch * R * (5 + eng.head.n_classes) * 4].tobytes()
    last = lay.n_scales - 1
    n_d = batch * eng.head.h[last] * eng.head.w[last] * lay.cout3[last] * 4
    out["d"] = raw[int(lay.d_offset):int(lay.d_offset) + n_d].tobytes()
    return out


def blocks_init_in_place(eng, blocks, ws, bs):
    """yolo_net_blocks_train_v3_init on the engine's existing state buffer (whatever it holds)"""
    ptrs = lambda arrs: (C.c_void_p * _hip.MAX_SCALES)(*[a.ctypes.data for a in arrs])
    _hip.check(eng.lib.yolo_net_blocks_train_v3_init(eng.handle, eng._blocks_state_v3.data_ptr(), eng._blocks_state_v3.numel(), ptrs(blocks), ptrs(ws),
                                                     ptrs(bs)), "yolo_net_blocks_train_v3_init")


@pytest.mark.parametrize("model,dtype", [("v3", "fp16"), ("v3", "fp32"), ("v3-tiny", "fp16")])
def test_train_blocks_step_v3_is_its_parts_and_the_next_forward_sees_it(model, dtype):
    import torch
    lib = _hip.lib()
    hw = NETS[model][2]
    weights = stream_of(model)
    gt, counts = yeval.pack_gts(TRUTHS, 3)
    x8 = np.random.RandomState(42).randint(0, 256, size=(BATCH,) + hw + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    m = build(model, dtype, weights)
    eng = m.net.engine
    heads, blocks = ytrain.head_convs_v3(m.net), ytrain.block_convs_v3(m.net)
    ws0, bs0 = ytrain.split_heads(weights, heads)
    blk0 = ytrain.split_blocks(weights, blocks)
    eng.blocks_train_init_v3(blk0, ws0, bs0)
    lay = eng.blocks_layout_v3
    bviews, hviews = eng.block_inputs_v3()
    ns = len(heads)
    hd = eng.head
    assert [(v.cin, v.h, v.w) for v in hviews] == [(cin, hd.h[s], hd.w[s]) for s, (_, _, cin) in enumerate(heads)]
    assert [(v.cin, v.h, v.w) for v in bviews] == [(cin3, hd.h[s], hd.w[s]) for s, (_, _, cin3) in enumerate(blocks)]
    assert [int(lay.bias_src[s]) for s in range(ns)] == [p for p, _, _ in heads] and [int(lay.block_src[s]) for s in range(ns)] == [p for p, _, _ in blocks]
    assert [(lay.cout3[s], lay.cin3[s]) for s in range(ns)] == [(c, i) for _, c, i in blocks] and [lay.cout3[s] for s in range(ns)] == [lay.cin[s] for s in range(ns)]
    st = torch.cuda.current_stream().cuda_stream
    R, parts = engine.v3_loss_rows(hd)
    width = 5 + hd.n_classes
    max_gt = gt.shape[1]
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(BATCH, -1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
    # the composition's own state: master values and moments in plain tensors
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
    pl3 = [_hip.conv3x3_wgrad_plan(hd.h[s], hd.w[s], BATCH, cin3, cout3, bviews[s].dtype) for s, (_, cout3, cin3) in enumerate(blocks)]
    need = max([pl["scratch_bytes"]] + [q["scratch_bytes"] for q in pl3])
    assert need <= lay.scratch_bytes
    d_parts = torch.empty(BATCH * parts * 56, dtype=torch.uint8, device="cuda")
    images = torch.empty(BATCH * 56, dtype=torch.uint8, device="cuda")
    assign = torch.empty(BATCH * R, dtype=torch.int32, device="cuda")
    result = torch.empty(64, dtype=torch.uint8, device="cuda")
    grad = torch.empty(BATCH * R * width, dtype=torch.float32, device="cuda")
    d = torch.empty(BATCH * max(hd.h[s] * hd.w[s] * blocks[s][1] for s in range(ns)), dtype=torch.float32, device="cuda")
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
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
            _hip.check(lib.yolo_conv3x3_wgrad(ws_ptr + bv.offset, bv.dtype, bv.ld, bv.coff, bv.image_stride, bv.h, bv.w, BATCH, cin3, d.data_ptr(), cout3,
                                              scale32[s].data_ptr(), comp[("dw3", s)].data_ptr(), comp[("dbeta", s)].data_ptr(), scratch.data_ptr(),
                                              scratch.numel(), st), "yolo_conv3x3_wgrad")
        for s, ((_, cout, cin), (_, cout3, cin3)) in enumerate(zip(heads, blocks)):
            _hip.check(lib.yolo_adam_step(*[comp[(k, s)].data_ptr() for k in HEAD_KEYS], cout * cin, cout, lr_t, 0.9, 0.999, 1e-8, st), "yolo_adam_step")
            _hip.check(lib.yolo_adam_step(*[comp[(k, s)].data_ptr() for k in BLOCK_KEYS], cout3 * 9 * cin3, cout3, lr_t, 0.9, 0.999, 1e-8, st),
                       "yolo_adam_step")
        want_result = result.cpu().numpy().tobytes()
        got_result = eng.train_blocks_step_v3(xf, (gt, counts), lr_t).cpu().numpy().tobytes()
        assert got_result == want_result, (model, dtype, t)
        got = blocks_state_parts(eng, BATCH)
        assert got["grad"] == grad.cpu().numpy().tobytes(), (model, dtype, t, "G")
        assert got["d"] == d.cpu().numpy().tobytes()[:len(got["d"])], (model, dtype, t, "D")
        for k, v in comp.items():
            assert got[k] == v.cpu().numpy().tobytes(), (model, dtype, t, k)
        assert all(bool(comp[("dw3", s)].abs().sum() > 0) and bool(torch.isfinite(comp[("w3", s)]).all()) for s in range(ns))
        results.append(got_result)
    rec = np.frombuffer(results[1], dtype=yeval.LOSS_RESULT_DTYPE)[0]
    assert results[0] != results[1] and np.isfinite(rec["loss"]) and rec["n_assigned"] == 5
    after_float = blocks_state_parts(eng, BATCH)
    k3, beta2, ws2, bs2 = eng.blocks_train_read_v3()
    for s, (_, cout3, cin3) in enumerate(blocks):
        assert tail_ref.stream_to_otc(k3[s].reshape(-1), cout3, cin3).tobytes() == after_float[("w3", s)] and beta2[s].tobytes() == after_float[("beta", s)]
        assert ws2[s].tobytes() == after_float[("w", s)] and bs2[s].tobytes() == after_float[("b", s)]
        assert k3[s].tobytes() != blk0[s][4 * cout3:].tobytes() and ws2[s].tobytes() != ws0[s].tobytes()
    # the re-pack of every conv: a second net, loaded with the rebuilt stream through yolo_net_load_weights, holds the same device weights,
    # byte for byte, and computes the same logits on a fresh input; gamma and the statistics stay
    fresh = synth.synthetic_input(BATCH, hw[0], hw[1], 3, seed=43)
    stepped = eng.forward(fresh).cpu().numpy()
    rebuilt = ytrain.replace_head_blocks(weights, blocks, heads, k3, beta2, ws2, bs2)
    inside = np.zeros(len(weights), dtype=bool)
    for pos, cout, cin in heads:
        inside[pos:pos + cout * (cin + 1)] = True
    for pos, cout3, cin3 in blocks:
        inside[pos:pos + cout3] = True
        inside[pos + 4 * cout3:pos + cout3 * (4 + 9 * cin3)] = True
    assert rebuilt[~inside].tobytes() == weights[~inside].tobytes() and (rebuilt != weights).sum() > 0.9 * inside.sum()
    second = build(model, dtype, rebuilt).net.engine
    assert bool(torch.equal(second._weights, eng._weights)), "the re-packed device weights are not the bytes yolo_net_load_weights produces"
    assert second.forward(fresh).cpu().numpy().tobytes() == stepped.tobytes()
    assert build(model, dtype, ytrain.replace_heads(weights, heads, ws2, bs2)).net.engine.forward(fresh).cpu().numpy().tobytes() != stepped.tobytes()
    # the uint8 twin from the same start, on a state whose every byte was 0xFF before the init: the same bits
    eng._blocks_state_v3.fill_(0xFF)
    blocks_init_in_place(eng, blk0, ws0, bs0)
    for t in (1, 2):
        assert eng.train_blocks_step_v3_u8(x8, (gt, counts), engine.adam_lr_t(1e-3, t)).cpu().numpy().tobytes() == results[t - 1]
    assert blocks_state_parts(eng, BATCH) == after_float
    # head-only training on the same net, from the same start: its first step sees the same weights, so the same record and the same heads
    honly = build(model, dtype, weights).net.engine
    honly.head_train_init_v3(ws0, bs0)
    assert honly.train_head_step_v3(xf, (gt, counts), engine.adam_lr_t(1e-3, 1)).cpu().numpy().tobytes() == results[0]


def test_twenty_blocks_steps_on_a_fixed_batch_lower_the_loss_and_track_the_yardstick():
    """YOLOv3 at 64 x 64, float32, batch 3, one fixed batch, at the rate at which the yardstick's float64 loop lowers the loss at every step
    (cases.TRAIN_LR: tests/test_train_blocks_v3_cpu.py asserts that on the oracle's features; here the loop runs on the device's stored
    block inputs).  The device's loss falls at every step, and at every step it lies within twice the distance of the yardstick's own
    float32 loop from the float64 loop.
    Measured on an MI355X: see README.md, "Training the 3x3 blocks behind the YOLOv3 heads"."""
    import torch
    model, steps, lr = "v3", cases.TRAIN_STEPS, cases.TRAIN_LR
    hw, B = cases.TRAIN_HW, cases.TRAIN_BATCH
    assert NETS[model][2] == hw and NETS[model][1] == cases.TRAIN_ANCHORS and NAMES3 == cases.TRAIN_NAMES
    weights = stream_of(model)
    gt, counts = yeval.pack_gts(cases.TRAIN_TRUTHS, 3)
    x = synth.synthetic_input(B, hw[0], hw[1], 3, seed=cases.TRAIN_INPUT_SEED)
    m = build(model, "fp32", weights, max_batch=B)
    eng = m.net.engine
    heads, blocks = ytrain.head_convs_v3(m.net), ytrain.block_convs_v3(m.net)
    eng.blocks_train_init_v3(ytrain.split_blocks(weights, blocks), *ytrain.split_heads(weights, heads))
    eng.forward(x)
    torch.cuda.synchronize()
    X3s = []
    for v in eng.block_inputs_v3()[0]:
        flat = eng._workspace[v.offset:v.offset + 4 * B * v.image_stride].cpu().numpy().view(np.float32)
        idx = (np.arange(B)[:, None, None] * v.image_stride + np.arange(v.h * v.w)[None, :, None] * v.ld + v.coff + np.arange(v.cin)[None, None, :])
        X3s.append(flat[idx].reshape(B, v.h, v.w, v.cin))
    records = torch.empty((steps, 64), dtype=torch.uint8, device="cuda")
    for t in range(1, steps + 1):
        eng.train_blocks_step_v3(x, (gt, counts), engine.adam_lr_t(lr, t), result=records[t - 1])
    dev = np.array([float(r["loss"]) for r in records.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE).reshape(-1)])          # the one read
    args = cases.train_loop_args(m.net, weights, X3s, eng.head)
    ref64 = np.array(ref.blocks_train_loop(*args, gt, counts, lr, steps, np.float32, mode="float64")[0])
    ref32 = np.array(ref.blocks_train_loop(*args, gt, counts, lr, steps, np.float32, mode="float32")[0])
    tol = 2 * np.abs(ref32 - ref64)
    gap, own = np.abs(dev - ref64) / ref64, np.abs(ref32 - ref64) / ref64
    print("device :", " ".join("%.6f" % v for v in dev))
    print("float64:", " ".join("%.6f" % v for v in ref64))
    print("float32:", " ".join("%.6f" % v for v in ref32))
    print("|device - ref64| / ref64 :", " ".join("%.2e" % v for v in gap))
    print("|ref32  - ref64| / ref64 :", " ".join("%.2e" % v for v in own))
    print("|device - ref64| / (2 |ref32 - ref64|):", " ".join("%.2f" % v for v in np.abs(dev - ref64) / tol))
    print("largest relative gap: device %.3e, the yardstick's float32 loop %.3e" % (gap.max(), own.max()))
    assert np.isfinite(dev).all() and all(a > c for a, c in zip(dev, dev[1:])), dev
    assert all(a > c for a, c in zip(ref64, ref64[1:]))
    assert (np.abs(dev - ref64) <= tol).all(), np.abs(dev - ref64) / tol


def test_a_blocks_step_followed_by_detect_equals_a_fresh_engine():
    """call order: step, detect, step on one engine leaves the state and returns the records of step, step on a fresh one"""
    model, dtype = "v3-tiny", "fp16"
    hw = NETS[model][2]
    weights = stream_of(model)
    gt, counts = yeval.pack_gts(TRUTHS, 3)
    x = synth.synthetic_input(BATCH, hw[0], hw[1], 3, seed=45)
    other = synth.synthetic_input(2, hw[0], hw[1], 3, seed=46)
    out = []
    for with_detect in (False, True):
        m = build(model, dtype, weights)
        eng = m.net.engine
        heads, blocks = ytrain.head_convs_v3(m.net), ytrain.block_convs_v3(m.net)
        eng.blocks_train_init_v3(ytrain.split_blocks(weights, blocks), *ytrain.split_heads(weights, heads))
        recs = [eng.train_blocks_step_v3(x, (gt, counts), engine.adam_lr_t(1e-3, 1)).cpu().numpy().tobytes()]
        if with_detect:
            eng.detect(other, 0.3, 0.5)
        recs.append(eng.train_blocks_step_v3(x, (gt, counts), engine.adam_lr_t(1e-3, 2)).cpu().numpy().tobytes())
        out.append((recs, blocks_state_parts(eng, BATCH), eng._weights.cpu().numpy().tobytes()))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][2] == out[1][2]


def test_blocks_step_refuses_a_missing_init_and_an_mxfp8_plan():
    hw = NETS["v3-tiny"][2]
    eng = build("v3-tiny", "fp16", stream_of("v3-tiny")).net.engine
    with pytest.raises(RuntimeError, match="follows blocks_train_init_v3"):
        eng.train_blocks_step_v3(np.zeros((1,) + hw + (3,), np.float32), [[]], 1e-3)
    mx = build("v3-tiny", "mxfp8", stream_of("v3-tiny"))
    heads, blocks = ytrain.head_convs_v3(mx.net), ytrain.block_convs_v3(mx.net)
    with pytest.raises(_hip.YoloHipError, match="scale 0: .*MXFP8 conv"):
        mx.net.engine.blocks_train_init_v3(ytrain.split_blocks(stream_of("v3-tiny"), blocks), *ytrain.split_heads(stream_of("v3-tiny"), heads))


# ---- train mode -------------------------------------------------------------------------------------------------------------------------
VOC_XML = ("<annotation><filename>%s</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>"
           "<object><name>%s</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object></annotation>")


def test_launcher_mode_train_with_train_layers_head_blocks(tmp_path, capsys):
    """two images at batch 2, two epochs, a checkpoint every step, YOLOv3-tiny from a full weight file: the reference's lines, a first loss
    that holds the bits of train_blocks_step_v3_u8 on the same batch, and checkpoints that differ from the initial stream in the blocks'
    kernels and betas and the head convs only"""
    import random
    from PIL import Image
    rng = np.random.RandomState(52)
    hw = NETS["v3-tiny"][2]
    for d in ("train", "val", "out"):
        (tmp_path / d).mkdir()
    for d in ("train", "val"):
        for i in range(2):
            name = "im%d.png" % i
            Image.fromarray(rng.randint(0, 256, size=(120, 200, 3)).astype(np.uint8)).save(str(tmp_path / d / name))
            x1, y1 = int(rng.randint(0, 100)), int(rng.randint(0, 60))
            (tmp_path / d / ("im%d.xml" % i)).write_text(VOC_XML % (name, 200, 120, NAMES3[i], x1, y1, x1 + int(rng.randint(20, 100)),
                                                                   y1 + int(rng.randint(20, 60))))
    full = stream_of("v3-tiny")
    base.write_darknet_weights(str(tmp_path / "full.weights"), full, "v3")
    (tmp_path / "cfg.ini").write_text(
        "[COMMON]\nversion = v3-tiny\ninput_h = %d\ninput_w = %d\ninput_c = 3\n"
        "[TRAIN]\ntrain_layers = head_blocks\nignore_thresh = 0.6\nseed = 3\nimage_dir = train/\nannotation_dir = train/\nval_image_dir = val/\n"
        "val_annotation_dir = val/\nbatch_size = 2\nlearning_rate = 1e-3\nepochs = 2\nmax_step = -1\naugment_probability = 0.0\n"
        "checkpoint_dir = out/\ncheckpoint_step = 1\ncheckpoint_prefix = yolo\ntensorboard_log_dir = log/\npretrained_weights_path = full.weights\n"
        "anchors = %s\nclass_names = %s\ncpu_only = False\ndtype = fp16\n" % (hw[0], hw[1], TINY_ANCHORS, str(NAMES3).replace("'", '"')))
    launcher.run(launcher.read_config(str(tmp_path / "cfg.ini")), "train")
    out = capsys.readouterr().out.splitlines()
    steps = [l for l in out if l.startswith("step ")]
    assert len(steps) == 2 and steps[0].startswith("step 1 (1/2): ") and steps[1].startswith("step 2 (2/2): ") and "(moving average: " in steps[1]
    assert sum(l.startswith("validation loss: ") for l in out) == 2 and out[-1] == "Done" and "Epoch (2/2) completed." in out
    assert any("tensorboard_log_dir is ignored" in l for l in out) and "Pre-trained weights loaded." in out
    # the first loss: the step entry on the same batch, from the same start
    ann, _ = yeval.parse_voc_annotations(str(tmp_path / "train"), str(tmp_path / "train"), NAMES3)
    batch, = ytrain.make_batches(ann, 2, random.Random(3))
    m = build("v3-tiny", "fp16", full, max_batch=2)
    eng = m.net.engine
    heads, blocks = ytrain.head_convs_v3(m.net), ytrain.block_convs_v3(m.net)
    eng.blocks_train_init_v3(ytrain.split_blocks(full, blocks), *ytrain.split_heads(full, heads))
    x, truths = ytrain.batch_to_device(eng, batch)
    rec = eng.train_blocks_step_v3_u8(x, truths, engine.adam_lr_t(1e-3, 1), 0.6).cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]
    assert steps[0] == "step 1 (1/2): {} (moving average: {})".format(np.float32(rec["loss"]), np.float32(rec["loss"]))
    assert rec["n_assigned"] == 2
    # checkpoints
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["yolo-%d.weights" % s for s in (0, 1, 2)]
    header0, body0 = base.read_darknet_weights(str(tmp_path / "out" / "yolo-0.weights"), "v3")
    assert body0.tobytes() == full.tobytes()
    inside = np.zeros(len(full), dtype=bool)
    for pos, cout, cin in heads:
        inside[pos:pos + cout * (cin + 1)] = True
    for pos, cout3, cin3 in blocks:
        inside[pos:pos + cout3] = True
        inside[pos + 4 * cout3:pos + cout3 * (4 + 9 * cin3)] = True
    for s in (1, 2):
        header, body = base.read_darknet_weights(str(tmp_path / "out" / ("yolo-%d.weights" % s)), "v3")
        assert header == header0 and len(body) == len(full)
        assert body[~inside].tobytes() == full[~inside].tobytes()
        for pos, cout, cin in heads:
            assert body[pos:pos + cout * (cin + 1)].tobytes() != full[pos:pos + cout * (cin + 1)].tobytes()
        for pos, cout3, cin3 in blocks:
            assert body[pos:pos + cout3].tobytes() != full[pos:pos + cout3].tobytes()
            assert body[pos + 4 * cout3:pos + cout3 * (4 + 9 * cin3)].tobytes() != full[pos + 4 * cout3:pos + cout3 * (4 + 9 * cin3)].tobytes()
    _, body1 = base.read_darknet_weights(str(tmp_path / "out" / "yolo-1.weights"), "v3")
    assert body1.tobytes() == ytrain.replace_head_blocks(full, blocks, heads, *eng.blocks_train_read_v3()).tobytes()

"""GPU: the weight gradient of the YOLOv3 head convs (include/yolo_hip.h "The weight gradient of the YOLOv3 head convs"), through the C
ABI: yolo_v3_head_wgrad against tests/train_v3_ref.py.

Every device output lies in a buffer with a 256-byte 0xA5 guard band on both sides.

  exact       integer operands (|X|, |G| <= 8, P_s < 2^18: every partial sum below 2^24) with hand-made assign tables: every dW_s and
              db_s EQUALS the integer reference, for the shapes of train_v3_ref.shape_cases (sized from yolo_v3_head_wgrad_plan), every
              winner pattern, X as fp16 and float32, dense, sliced and unaligned views; scratch (slot included), dW and db pre-filled with
              0x00 and with 0xFF bytes, two calls each: four equal results
  poison      the same with NaN in every element of G the table declares a structural zero: the same bits
  slot        the slot table the call leaves in its scratch equals the yardstick's
  real        X ~ N(0, 1) in fp16, |G| log-uniform over 2^-20 .. 2^8: |device - ref64| <= (T + 2) 2^-24 S |G| |X| per element
  old kernel  on integer operands, yolo_conv1x1_wgrad on the gathered dense G_s returns the same bits

Measured on an MI355X (printed by the tests): see README.md, "Status"."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import train_ref
import train_v3_ref as ref
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 256, 0xA5


def guarded(nbytes, fill):
    import torch
    t = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    t[GUARD:GUARD + nbytes] = fill
    return t, t.data_ptr() + GUARD


def check_guards(bufs):
    for t, _ in bufs:
        assert bool((t[:GUARD] == PATTERN).all()) and bool((t[-GUARD:] == PATTERN).all()), "a guard band was written"


def head_of(grids, A, n_classes):
    return engine.head_desc_v3(grids, [[(1. + a, 2. + a) for a in range(A)] for _ in grids], n_classes)


def plan(grids, A, n_classes, cins, batch, dtype=_hip.DTYPE_F16):
    return _hip.v3_head_wgrad_plan(head_of(grids, A, n_classes), cins, batch, dtype)


def make_views(grids, cins, batch, pad, coff, rng, real=False):
    """per scale (flat buffer float64, shift, ld, coff, image_stride, cin, operand [P_s, cin]): the whole buffer holds values, so a kernel
    that ignores the view reads other numbers.  The unaligned view (coff % 4 != 0) also starts one element into its buffer and has a gap
    of 7 elements between its images."""
    out = []
    for (h, w), cin in zip(grids, cins):
        ppi, ld = h * w, cin + pad
        shift, gap = (1, 7) if coff % 4 else (0, 0)
        img_stride = ppi * ld + gap
        n = shift + batch * img_stride + 16
        flat = rng.randn(n) if real else rng.randint(-8, 9, size=n).astype(np.float64)
        out.append((flat, shift, ld, coff, img_stride, cin))
    return out


def operands(views, grids, batch, np_dtype):
    """the [P_s, cin_s] operands the views hold once the buffers are stored as np_dtype"""
    return [train_ref.view_positions(flat.astype(np_dtype)[shift:], batch, h * w, ld, coff, img_stride, cin)
            for (flat, shift, ld, coff, img_stride, cin), (h, w) in zip(views, grids)]


def run_v3(grids, A, n_classes, batch, views, np_dtype, G, table, max_gt, fill=0x00, calls=1):
    """yolo_v3_head_wgrad into guarded buffers filled with `fill` bytes once, before the first call -> per call ([dW_s], [db_s], slot)"""
    import torch
    lib = _hip.lib()
    hd = head_of(grids, A, n_classes)
    ns, width = len(grids), 5 + n_classes
    dtype = _hip.DTYPE_F16 if np_dtype == np.float16 else _hip.DTYPE_F32
    cins = [v[5] for v in views]
    pl = plan(grids, A, n_classes, cins, batch, dtype)
    d_x = [torch.from_numpy(v[0].astype(np_dtype)).cuda() for v in views]
    d_g = torch.from_numpy(np.ascontiguousarray(G, dtype=np.float32)).cuda()
    d_t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda()
    vs = (_hip.V3WgradView * _hip.MAX_SCALES)()
    for s, (flat, shift, ld, coff, img_stride, cin) in enumerate(views):
        vs[s].x_dev, vs[s].image_stride, vs[s].ld, vs[s].coff = d_x[s].data_ptr() + shift * d_x[s].element_size(), img_stride, ld, coff
        vs[s].dtype, vs[s].cin = dtype, cin
    couts = [A * width] * ns
    bw = [guarded(couts[s] * cins[s] * 4, fill) for s in range(ns)]
    bb = [guarded(couts[s] * 4, fill) for s in range(ns)]
    scratch = guarded(pl["scratch_bytes"], fill)
    dws = (C.c_void_p * _hip.MAX_SCALES)(*[b[1] for b in bw])
    dbs = (C.c_void_p * _hip.MAX_SCALES)(*[b[1] for b in bb])
    out = []
    for _ in range(calls):
        _hip.check(lib.yolo_v3_head_wgrad(C.byref(hd), vs, batch, d_g.data_ptr(), d_t.data_ptr(), max_gt, dws, dbs, scratch[1],
                                          pl["scratch_bytes"], torch.cuda.current_stream().cuda_stream), "yolo_v3_head_wgrad")
        torch.cuda.synchronize()
        check_guards(bw + bb + [scratch])
        slot = scratch[0][GUARD + pl["slot_offset"]:GUARD + pl["slot_offset"] + batch * max_gt * 4].cpu().numpy().view(np.int32)
        out.append(([b[0][GUARD:-GUARD].cpu().numpy().view(np.float32).reshape(couts[s], cins[s]).copy() for s, b in enumerate(bw)],
                    [b[0][GUARD:-GUARD].cpu().numpy().view(np.float32).copy() for b in bb], slot.reshape(batch, max_gt).copy()))
    return out


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[0] + a[1], b[0] + b[1]))


@functools.lru_cache(maxsize=None)
def shape_cases():
    return ref.shape_cases(plan)


CASE_NAMES = ("three-scales", "two-anchors-one-class", "row-of-85", "one-scale-below-a-chunk", "one-scale-past-a-chunk",
              "one-scale-several-chunks", "one-position-short", "exactly-one-chunk", "one-position-more", "three-chunks-and-one",
              "past-a-reduce-tile")


# ---- exact, poison, slot ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_wgrad_equals_the_integer_reference_clean_and_poisoned(name):
    assert tuple(c[0] for c in shape_cases()) == CASE_NAMES
    _, grids, A, n_classes, cins, batch = [c for c in shape_cases() if c[0] == name][0]
    pl = plan(grids, A, n_classes, cins, batch)
    assert ref.expected_chunks(name, pl["positions"][0], pl["positions_per_chunk"][0], pl["reduce_tile_chunks"]), pl
    assert max(pl["positions"]) <= 2 ** 24 // 64        # |X|, |G| <= 8: no partial sum reaches 2^24
    width = 5 + n_classes
    rng = np.random.RandomState(sum(map(ord, name)))
    runs = 0
    for i, pattern in enumerate(ref.PATTERNS):
        table = ref.make_table(pattern, grids, A, batch, rng)
        G = ref.integer_g(table, width, rng)
        Gp = ref.integer_g(table, width, np.random.RandomState(0), poison=True)
        Gp[~np.isnan(Gp)] = G[~np.isnan(Gp)]
        assert np.isnan(Gp).any() and np.array_equal(np.isnan(Gp), ~ref.terms(table, width, ref.MAX_GT))
        want_slot = ref.slot_table(table, ref.MAX_GT)
        for j, (pad, coff) in enumerate(ref.VIEWS):
            views = make_views(grids, cins, batch, pad, coff, rng)
            for np_dtype in (np.float16, np.float32):
                # every pattern runs clean and poisoned; the first one on all views and types, the others on one view and type each
                if i and (j != i % len(ref.VIEWS) or np_dtype != (np.float16, np.float32)[i % 2]):
                    continue
                want = ref.wgrad_exact(operands(views, grids, batch, np_dtype), G, table, grids, A, ref.MAX_GT)
                assert max(np.abs(w).max() for w, _ in want) < 2 ** 24
                got = run_v3(grids, A, n_classes, batch, views, np_dtype, G, table, ref.MAX_GT, 0x00, calls=2)
                got += run_v3(grids, A, n_classes, batch, views, np_dtype, G, table, ref.MAX_GT, 0xFF, calls=2)
                got += run_v3(grids, A, n_classes, batch, views, np_dtype, Gp, table, ref.MAX_GT, 0xFF, calls=1)
                runs += len(got)
                tag = (name, pattern, pad, coff, np_dtype.__name__)
                for dws, dbs, slot in got:
                    assert np.array_equal(slot, want_slot), tag
                    for s, (want_w, want_b) in enumerate(want):
                        assert np.array_equal(dws[s], want_w), tag + (s, "dW")
                        assert np.array_equal(dbs[s], want_b), tag + (s, "db")
                assert all(same_bits(g, got[0]) for g in got), tag
    print("%s: %d calls, objectness chunks per scale %s" % (name, runs, pl["n_chunks"]))


def test_a_row_without_a_term_is_plus_zero():
    """no winner anywhere: every row of dW and db but the objectness rows is +0, bit for bit, out of 0xFF-filled buffers"""
    grids, A, n_classes, cins, batch = ref.GRIDS3, 3, 3, (40, 8, 136), 2
    rng = np.random.RandomState(3)
    table = ref.make_table("none", grids, A, batch, rng)
    G = ref.integer_g(table, 5 + n_classes, rng, poison=True)
    views = make_views(grids, cins, batch, 0, 0, rng)
    (dws, dbs, _), = run_v3(grids, A, n_classes, batch, views, np.float16, G, table, ref.MAX_GT, 0xFF)
    other = np.arange(A * (5 + n_classes)) % (5 + n_classes) != 4
    for dw, db in zip(dws, dbs):
        assert not dw[other].view(np.uint32).any() and not db[other].view(np.uint32).any()
        assert dw[~other].any()


# ---- real values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,grids,n_classes,cins", [("tiny", ref.GRIDS3, 3, (136, 40, 8)),
                                                       ("yolov3-608-heads", ((19, 19), (38, 38), (76, 76)), 80, (1024, 512, 256))])
def test_wgrad_real_values_within_the_float32_bound(name, grids, n_classes, cins):
    import torch
    A, batch, max_gt = 3, 2, 8
    rng = np.random.RandomState(len(name))
    R, scales = ref.scales_of(grids, A)
    table = np.where(rng.uniform(size=(batch, R)) < 0.1, -2, -1).astype(np.int32)
    for n in range(batch):
        table[n, rng.choice(R, size=max_gt, replace=False)] = rng.permutation(max_gt)
    width = 5 + n_classes
    G = (np.exp2(rng.uniform(-20, 8, size=(batch, R, width))) * rng.choice([-1.0, 1.0], size=(batch, R, width))).astype(np.float32)
    G[table == -2, 4] = 0
    G[~ref.terms(table, width, max_gt)] = 0
    hd = head_of(grids, A, n_classes)
    xs = [rng.randn(batch, h, w, cin).astype(np.float16) for (h, w), cin in zip(grids, cins)]
    dws, dbs, _ = engine.v3_head_wgrad(hd, [torch.from_numpy(x).cuda() for x in xs], torch.from_numpy(G).cuda(),
                                       torch.from_numpy(table).cuda(), max_gt)
    torch.cuda.synchronize()
    want = ref.wgrad_ref64([x.reshape(-1, x.shape[3]) for x in xs], G, table, grids, A, max_gt)
    worst_w = worst_b = 0.0
    for s, (ref_w, ref_b, bound_w, bound_b) in enumerate(want):
        dw, db = dws[s].cpu().numpy().astype(np.float64), dbs[s].cpu().numpy().astype(np.float64)
        assert ((bound_w > 0) | (dw == 0)).all() and ((bound_b > 0) | (db == 0)).all()
        rw = float(np.max(np.abs(dw - ref_w)[bound_w > 0] / bound_w[bound_w > 0]))
        rb = float(np.max(np.abs(db - ref_b)[bound_b > 0] / bound_b[bound_b > 0]))
        print("v3 wgrad %s scale %d (%d positions, cin %d): largest |device - ref64| / bound: dW %.4f db %.4f"
              % (name, s, batch * grids[s][0] * grids[s][1], cins[s], rw, rb))
        worst_w, worst_b = max(worst_w, rw), max(worst_b, rb)
    assert worst_w <= 1.0 and worst_b <= 1.0


# ---- the old kernel, repeatability ------------------------------------------------------------------------------------------------------
def test_wgrad_equals_the_dense_kernel_on_the_gathered_gradient():
    """integer operands whose structural zeros ARE zeros: yolo_conv1x1_wgrad on each gathered dense G_s returns the same bits, and a
    second call of yolo_v3_head_wgrad returns the first one's"""
    import torch
    grids, A, n_classes, cins, batch = ref.GRIDS3, 3, 80, (1024, 136, 40), 3
    rng = np.random.RandomState(11)
    table = ref.make_table("full-image", grids, A, batch, rng)
    table[0, 5], table[2, 100] = 3, 1
    width = 5 + n_classes
    G = ref.integer_g(table, width, rng)
    views = make_views(grids, cins, batch, 0, 0, rng)
    first, second = run_v3(grids, A, n_classes, batch, views, np.float16, G, table, ref.MAX_GT, 0xFF, calls=2)
    assert same_bits(first, second)
    R, scales = ref.scales_of(grids, A)
    lib = _hip.lib()
    for s, sc in enumerate(scales):
        Gs, _ = ref.scale_operands(G, ref.terms(table, width, ref.MAX_GT), sc)
        P, cout, cin = Gs.shape[0], Gs.shape[1], cins[s]
        pl = _hip.wgrad_plan(P, cin, cout, _hip.DTYPE_F16)
        d_x = torch.from_numpy(views[s][0].astype(np.float16)).cuda()
        d_g = torch.from_numpy(np.ascontiguousarray(Gs)).cuda()
        dw, db = torch.empty((cout, cin), dtype=torch.float32, device="cuda"), torch.empty(cout, dtype=torch.float32, device="cuda")
        scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda")
        _hip.check(lib.yolo_conv1x1_wgrad(d_x.data_ptr(), _hip.DTYPE_F16, cin, 0, views[s][4], P // batch, batch, cin, d_g.data_ptr(), cout,
                                          dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), pl["scratch_bytes"],
                                          torch.cuda.current_stream().cuda_stream), "yolo_conv1x1_wgrad")
        torch.cuda.synchronize()
        assert dw.cpu().numpy().tobytes() == first[0][s].tobytes() and db.cpu().numpy().tobytes() == first[1][s].tobytes(), s


# ---- the net-level step -----------------------------------------------------------------------------------------------------------------
from tensorflow_yolo_amd import YoloV2Tiny, YoloV3, YoloV3Tiny, launcher                      # noqa: E402
from tensorflow_yolo_amd.net import base, evaluate as yeval, synth, train as ytrain          # noqa: E402

NAMES3 = ["a", "b", "c"]
TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
NETS = {"v3": (YoloV3, V3_ANCHORS, (64, 64)), "v3-tiny": (YoloV3Tiny, TINY_ANCHORS, (96, 160))}
BATCH = 3
TRUTHS = [[(0.3, 0.4, 0.2, 0.5, 1), (0.8, 0.2, 0.3, 0.3, 2), (0.5, 0.5, 0.9, 0.9, 0)], [], [(0.6, 0.6, 0.1, 0.15, 0), (0.1, 0.9, 0.05, 0.08, 2)]]


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


def state_parts(eng, batch):
    """the parts of the engine's YOLOv3 training state a step leaves behind, as bytes: per scale the masters, the moments, dW and db; G"""
    lay = eng.train_layout_v3
    raw = eng._train_state_v3.cpu().numpy()
    out = {}
    for s in range(lay.n_scales):
        nw, nb = lay.cout[s] * lay.cin[s] * 4, lay.cout[s] * 4
        for k, n in (("w", nw), ("b", nb), ("m_w", nw), ("v_w", nw), ("m_b", nb), ("v_b", nb), ("dw", nw), ("db", nb)):
            at = int(getattr(lay, k + "_offset")[s])
            out[(k, s)] = raw[at:at + n].tobytes()
    R, _ = engine.v3_loss_rows(eng.head)
    out["grad"] = raw[int(lay.grad_offset):int(lay.grad_offset) + batch * R * (5 + eng.head.n_classes) * 4].tobytes()
    return out


def init_in_place(eng, ws, bs):
    """yolo_net_head_train_v3_init on the engine's existing state buffer (whatever it holds)"""
    wp = (C.c_void_p * _hip.MAX_SCALES)(*[w.ctypes.data for w in ws])
    bp = (C.c_void_p * _hip.MAX_SCALES)(*[b.ctypes.data for b in bs])
    _hip.check(eng.lib.yolo_net_head_train_v3_init(eng.handle, eng._train_state_v3.data_ptr(), eng._train_state_v3.numel(), wp, bp),
               "yolo_net_head_train_v3_init")


@pytest.mark.parametrize("model,dtype", [("v3", "fp16"), ("v3", "fp32"), ("v3-tiny", "fp16")])
def test_train_head_step_v3_is_its_parts_and_the_next_forward_sees_it(model, dtype):
    import torch
    lib = _hip.lib()
    hw = NETS[model][2]
    weights = stream_of(model)
    gt, counts = yeval.pack_gts(TRUTHS, 3)
    x8 = np.random.RandomState(42).randint(0, 256, size=(BATCH,) + hw + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    m = build(model, dtype, weights)
    eng = m.net.engine
    heads = ytrain.head_convs_v3(m.net)
    ws0, bs0 = ytrain.split_heads(weights, heads)
    eng.head_train_init_v3(ws0, bs0)
    lay = eng.train_layout_v3
    views = eng.head_inputs_v3()
    ns = len(heads)
    assert [(v.cin, v.h, v.w) for v in views] == [(cin, eng.head.h[s], eng.head.w[s]) for s, (_, _, cin) in enumerate(heads)]
    assert [int(lay.bias_src[s]) for s in range(ns)] == [pos for pos, _, _ in heads]
    st = torch.cuda.current_stream().cuda_stream
    hd = eng.head
    R, parts = engine.v3_loss_rows(hd)
    width = 5 + hd.n_classes
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(BATCH, -1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
    # the composition's own state: master values and moments in plain tensors
    comp = {}
    for s, (_, cout, cin) in enumerate(heads):
        for k, v in (("w", ws0[s].reshape(-1)), ("b", bs0[s]), ("m_w", np.zeros(cout * cin, np.float32)), ("v_w", np.zeros(cout * cin, np.float32)),
                     ("m_b", np.zeros(cout, np.float32)), ("v_b", np.zeros(cout, np.float32)), ("dw", np.zeros(cout * cin, np.float32)),
                     ("db", np.zeros(cout, np.float32))):
            comp[(k, s)] = torch.from_numpy(np.array(v)).cuda()
    pl = _hip.v3_head_wgrad_plan(hd, [cin for _, _, cin in heads], BATCH, views[0].dtype)
    assert pl["scratch_bytes"] <= lay.scratch_bytes
    d_parts = torch.empty(BATCH * parts * 56, dtype=torch.uint8, device="cuda")
    images = torch.empty(BATCH * 56, dtype=torch.uint8, device="cuda")
    assign = torch.empty(BATCH * R, dtype=torch.int32, device="cuda")
    result = torch.empty(64, dtype=torch.uint8, device="cuda")
    grad = torch.empty(BATCH * R * width, dtype=torch.float32, device="cuda")
    scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda")
    vs = (_hip.V3WgradView * _hip.MAX_SCALES)()
    for s, v in enumerate(views):
        vs[s].x_dev, vs[s].image_stride, vs[s].ld, vs[s].coff = eng._workspace.data_ptr() + v.offset, v.image_stride, v.ld, v.coff
        vs[s].dtype, vs[s].cin = v.dtype, v.cin
    dws = (C.c_void_p * _hip.MAX_SCALES)(*[comp[("dw", s)].data_ptr() for s in range(ns)])
    dbs = (C.c_void_p * _hip.MAX_SCALES)(*[comp[("db", s)].data_ptr() for s in range(ns)])
    results = []
    for t in (1, 2):
        lr_t = engine.adam_lr_t(1e-3, t)
        logits = eng.forward(xf)
        _hip.check(lib.yolo_v3_loss_grad(C.byref(hd), logits.data_ptr(), BATCH, d_gt.data_ptr(), d_gc.data_ptr(), gt.shape[1], 0.7, d_parts.data_ptr(),
                                         images.data_ptr(), assign.data_ptr(), result.data_ptr(), grad.data_ptr(), st), "yolo_v3_loss_grad")
        _hip.check(lib.yolo_v3_head_wgrad(C.byref(hd), vs, BATCH, grad.data_ptr(), assign.data_ptr(), gt.shape[1], dws, dbs, scratch.data_ptr(),
                                          scratch.numel(), st), "yolo_v3_head_wgrad")
        for s, (_, cout, cin) in enumerate(heads):
            _hip.check(lib.yolo_adam_step(*[comp[(k, s)].data_ptr() for k in ("w", "b", "m_w", "v_w", "m_b", "v_b", "dw", "db")], cout * cin, cout,
                                          float(lr_t), 0.9, 0.999, 1e-8, st), "yolo_adam_step")
        want_result = result.cpu().numpy().tobytes()
        got_result = eng.train_head_step_v3(xf, (gt, counts), lr_t).cpu().numpy().tobytes()
        assert got_result == want_result, (model, dtype, t)
        got = state_parts(eng, BATCH)
        assert got["grad"] == grad.cpu().numpy().tobytes(), (model, dtype, t, "G")
        for k, v in comp.items():
            assert got[k] == v.cpu().numpy().tobytes(), (model, dtype, t, k)
        results.append(got_result)
    rec = np.frombuffer(results[1], dtype=yeval.LOSS_RESULT_DTYPE)[0]
    assert results[0] != results[1] and np.isfinite(rec["loss"]) and rec["n_assigned"] == 5
    after_float = state_parts(eng, BATCH)
    ws2, bs2 = eng.head_train_read_v3()
    for s in range(ns):
        assert ws2[s].tobytes() == after_float[("w", s)] and bs2[s].tobytes() == after_float[("b", s)] and ws2[s].tobytes() != ws0[s].tobytes()
    # the uint8 twin from the same start, on a state that held 0xFF bytes before its init: the same bits
    eng._train_state_v3.fill_(0xFF)
    init_in_place(eng, ws0, bs0)
    for t in (1, 2):
        assert eng.train_head_step_v3_u8(x8, (gt, counts), engine.adam_lr_t(1e-3, t)).cpu().numpy().tobytes() == results[t - 1]
    assert state_parts(eng, BATCH) == after_float
    # the re-pack: a second net, loaded with the stream rebuilt from the master values, computes the same logits on a fresh input
    fresh = synth.synthetic_input(BATCH, hw[0], hw[1], 3, seed=43)
    stepped = eng.forward(fresh).cpu().numpy()
    second = build(model, dtype, ytrain.replace_heads(weights, heads, ws2, bs2))
    assert second.net.engine.forward(fresh).cpu().numpy().tobytes() == stepped.tobytes()
    assert build(model, dtype, weights).net.engine.forward(fresh).cpu().numpy().tobytes() != stepped.tobytes()


def test_twenty_steps_on_a_fixed_batch_lower_the_loss_at_every_step():
    """YOLOv3 at 64 x 64, float32, batch 3, lr 1e-3; beside it the float64 loop of tests/train_v3_ref.py on the device's features.  The
    device's loss falls at every step; the two loops are printed side by side (float32 steps and a float64 yardstick drift apart, so only
    the yardstick's endpoints are asserted)."""
    import torch
    model, steps = "v3", 20
    hw = NETS[model][2]
    weights = stream_of(model)
    gt, counts = yeval.pack_gts(TRUTHS, 3)
    x = synth.synthetic_input(BATCH, hw[0], hw[1], 3, seed=44)
    m = build(model, "fp32", weights)
    eng = m.net.engine
    heads = ytrain.head_convs_v3(m.net)
    ws0, bs0 = ytrain.split_heads(weights, heads)
    eng.head_train_init_v3(ws0, bs0)
    eng.forward(x)
    torch.cuda.synchronize()
    Xs = []
    for v in eng.head_inputs_v3():
        flat = eng._workspace[v.offset:v.offset + 4 * BATCH * v.image_stride].cpu().numpy().view(np.float32)
        Xs.append(train_ref.view_positions(flat, BATCH, v.h * v.w, v.ld, v.coff, v.image_stride, v.cin))
    records = torch.empty((steps, 64), dtype=torch.uint8, device="cuda")
    for t in range(1, steps + 1):
        eng.train_head_step_v3(x, (gt, counts), engine.adam_lr_t(1e-3, t), result=records[t - 1])
    dev = [float(r["loss"]) for r in records.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE).reshape(-1)]        # the one read
    hd = eng.head
    grids = [(hd.h[s], hd.w[s]) for s in range(hd.n_scales)]
    anchors = [[(hd.anchors[s][2 * a], hd.anchors[s][2 * a + 1]) for a in range(hd.n_anchors[s])] for s in range(hd.n_scales)]
    want, _, _ = ref.heads_train_loop64(Xs, ws0, bs0, grids, anchors, hd.n_classes, gt, counts, 1e-3, steps)
    print("device :", " ".join("%.4f" % v for v in dev))
    print("float64:", " ".join("%.4f" % v for v in want))
    print("largest |device - float64| / float64 over the %d steps: %.3e" % (steps, max(abs(a - b) / b for a, b in zip(dev, want))))
    assert np.isfinite(dev).all() and np.isfinite(want).all()
    assert all(b < a for a, b in zip(dev, dev[1:])), "the loss did not fall at every step"
    assert want[-1] < want[0]


# ---- refusals that need a device --------------------------------------------------------------------------------------------------------
def test_step_v3_refuses_a_null_state_a_missing_init_and_a_v2_head():
    import torch
    m = build("v3-tiny", "fp16", stream_of("v3-tiny"))
    eng = m.net.engine
    hw = NETS["v3-tiny"][2]
    with pytest.raises(RuntimeError, match="follows head_train_init_v3"):
        eng.train_head_step_v3(np.zeros((1,) + hw + (3,), np.float32), [[]], 1e-3)
    x = torch.zeros((1,) + hw + (3,), dtype=torch.float32, device="cuda")
    gt, counts = yeval.pack_gts([[]], 1)
    d_gt, d_gc = torch.from_numpy(gt.view(np.uint8).reshape(1, -1)).cuda(), torch.from_numpy(counts).cuda()
    res = torch.empty(64, dtype=torch.uint8, device="cuda")
    for name in ("yolo_net_train_head_step_v3", "yolo_net_train_head_step_v3_u8"):
        rc = getattr(eng.lib, name)(eng.handle, x.data_ptr(), 1, d_gt.data_ptr(), d_gc.data_ptr(), 1, 0.7, None, 1e-3, res.data_ptr(), None)
        assert rc == 1 and eng.lib.yolo_last_error().decode() == name + ": null state (yolo_net_head_train_v3_init)"
    # the old entries keep refusing this net, and the new ones refuse a YOLOv2 net
    with pytest.raises(_hip.YoloHipError, match="detection layer|version 2"):
        eng.head_train_layout()
    anchors = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071]
    m2 = YoloV2Tiny()
    net = YoloV2Tiny.create_network(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=(32, 32, 3))
    m2.build(anchors, NAMES3, (32, 32, 3), dtype="fp32", max_batch=1, weights=synth.darknet_stream(net, seed=31, num_classes=3), streams=1)
    e2 = m2.net.engine
    with pytest.raises(_hip.YoloHipError, match="the head must be version 3"):
        e2.head_inputs_v3()
    x2 = torch.zeros((1, 32, 32, 3), dtype=torch.float32, device="cuda")
    rc = e2.lib.yolo_net_train_head_step_v3(e2.handle, x2.data_ptr(), 1, d_gt.data_ptr(), d_gc.data_ptr(), 1, 0.7, res.data_ptr(), 1e-3, res.data_ptr(), None)
    assert rc == 1 and "yolo_net_train_head_step_v3: the head must be version 3" in e2.lib.yolo_last_error().decode()


# ---- train mode -------------------------------------------------------------------------------------------------------------------------
VOC_XML = ("<annotation><filename>%s</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>"
           "<object><name>%s</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object></annotation>")


def test_launcher_mode_train_with_train_layers_heads(tmp_path, capsys):
    """two images at batch 2, two epochs, a checkpoint every step, YOLOv3-tiny from a full weight file: the reference's lines, a first loss
    that is train_head_step_v3_u8 on the same batch, and checkpoints that differ from the initial stream in the head floats only"""
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
        "[TRAIN]\ntrain_layers = heads\nignore_thresh = 0.6\nseed = 3\nimage_dir = train/\nannotation_dir = train/\nval_image_dir = val/\n"
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
    heads = ytrain.head_convs_v3(m.net)
    eng.head_train_init_v3(*ytrain.split_heads(full, heads))
    x, truths = ytrain.batch_to_device(eng, batch)
    rec = eng.train_head_step_v3_u8(x, truths, engine.adam_lr_t(1e-3, 1), 0.6).cpu().numpy().view(yeval.LOSS_RESULT_DTYPE)[0]
    assert steps[0] == "step 1 (1/2): {} (moving average: {})".format(np.float32(rec["loss"]), np.float32(rec["loss"]))
    assert rec["n_assigned"] == 2
    # checkpoints
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["yolo-%d.weights" % s for s in (0, 1, 2)]
    header0, body0 = base.read_darknet_weights(str(tmp_path / "out" / "yolo-0.weights"), "v3")
    assert body0.tobytes() == full.tobytes()
    inside = np.zeros(len(full), dtype=bool)
    for pos, cout, cin in heads:
        inside[pos:pos + cout * (cin + 1)] = True
    for s in (1, 2):
        header, body = base.read_darknet_weights(str(tmp_path / "out" / ("yolo-%d.weights" % s)), "v3")
        assert header == header0 and len(body) == len(full)
        assert body[~inside].tobytes() == full[~inside].tobytes()
        for pos, cout, cin in heads:
            assert body[pos:pos + cout * (cin + 1)].tobytes() != full[pos:pos + cout * (cin + 1)].tobytes()
    ws1, bs1 = eng.head_train_read_v3()
    _, body1 = base.read_darknet_weights(str(tmp_path / "out" / "yolo-1.weights"), "v3")
    assert body1.tobytes() == ytrain.replace_heads(full, heads, ws1, bs1).tobytes()

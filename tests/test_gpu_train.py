"""GPU: training the detection layer (include/yolo_hip.h "Training the detection layer"), through the C ABI: yolo_conv1x1_wgrad,
yolo_adam_step, yolo_net_head_input, yolo_net_train_head_step[_u8], yolo_net_head_train_init / _read, against tests/train_ref.py.

Every device output of the standalone entries lies in a buffer with a 256-byte 0xA5 guard band on both sides.

  exact       integer operands (|X|, |G| <= 8, P <= 4096: every partial sum below 2^24): dW and db EQUAL the integer reference, for the
              shapes sized from yolo_wgrad_plan, X as fp16 and float32, dense and sliced views; scratch and outputs pre-filled with 0x00
              and with 0xFF bytes, two calls each: four equal results
  real        X ~ N(0, 1) in fp16, |G| log-uniform over 2^-20 .. 2^8: |device - ref64| <= (P + 2) 2^-24 S_p |G| |X| per element, the
              derived worst case of float32 products and float32 sums in any order
  adam        bit for bit against the float32 restatement over 5 consecutive steps
  step        yolo_net_train_head_step is forward -> yolo_v2_loss_grad -> yolo_conv1x1_wgrad -> yolo_adam_step, bit for bit; its uint8
              twin; the re-pack: the next forward equals that of a net loaded with the master values
  it trains   40 steps on a fixed batch, beside the float64 loop on the device's features

Measured on an MI355X (printed by the tests): see DESIGN.md section 3, "head_wgrad / adam_step"."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import loss_grad_cases as cases
import train_ref
from loss_grad_cases import ANCHORS8
from tensorflow_yolo_amd import YoloV2, YoloV2Tiny, _hip, launcher
from tensorflow_yolo_amd.net import base, engine, evaluate as yeval, synth, train as ytrain

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


def plan(P, cin, cout, dtype=_hip.DTYPE_F16):
    return _hip.wgrad_plan(P, cin, cout, dtype)


def run_wgrad(x_flat, ld, coff, img_stride, ppi, batch, cin, G, fill=0x00, calls=1):
    """yolo_conv1x1_wgrad on a view of x_flat (np.float16 | np.float32) -> [(dW [cout, cin], db [cout])] of each call, the outputs and the
    scratch filled with `fill` bytes once, before the first call"""
    import torch
    lib = _hip.lib()
    dtype = _hip.DTYPE_F16 if x_flat.dtype == np.float16 else _hip.DTYPE_F32
    P, cout = G.shape
    assert P == batch * ppi
    pl = plan(P, cin, cout, dtype)
    d_x = torch.from_numpy(np.ascontiguousarray(x_flat)).cuda()
    d_g = torch.from_numpy(np.ascontiguousarray(G, dtype=np.float32)).cuda()
    bufs = [guarded(cout * cin * 4, fill), guarded(cout * 4, fill), guarded(pl["scratch_bytes"], fill)]
    out = []
    for _ in range(calls):
        _hip.check(lib.yolo_conv1x1_wgrad(d_x.data_ptr(), dtype, ld, coff, img_stride, ppi, batch, cin, d_g.data_ptr(), cout, bufs[0][1],
                                          bufs[1][1], bufs[2][1], pl["scratch_bytes"], torch.cuda.current_stream().cuda_stream),
                   "yolo_conv1x1_wgrad")
        torch.cuda.synchronize()
        check_guards(bufs)
        out.append((bufs[0][0][GUARD:-GUARD].cpu().numpy().view(np.float32).reshape(cout, cin).copy(),
                    bufs[1][0][GUARD:-GUARD].cpu().numpy().view(np.float32).copy()))
    return out


# ---- exact ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout", train_ref.COUTS)
@pytest.mark.parametrize("cin", train_ref.CINS)
def test_wgrad_equals_the_integer_reference(cin, cout):
    rng = np.random.RandomState(1000 * cout + cin)
    for batch, ppi, gap, chunks in train_ref.wgrad_position_cases(lambda P: plan(P, cin, cout)):
        P = batch * ppi
        assert P <= 4096 and plan(P, cin, cout)["n_chunks"] == chunks
        G = rng.randint(-8, 9, size=(P, cout)).astype(np.float32)
        for pad, coff in train_ref.VIEWS:
            ld = cin + pad
            img_stride = ppi * ld + gap
            flat = rng.randint(-8, 9, size=batch * img_stride + 16)         # the whole buffer: a kernel that ignores the view reads other integers
            want_w, want_b = train_ref.wgrad_exact(train_ref.view_positions(flat, batch, ppi, ld, coff, img_stride, cin), G)
            assert np.abs(want_w).max() < 2 ** 24
            for np_dtype in (np.float16, np.float32):
                got = run_wgrad(flat.astype(np_dtype), ld, coff, img_stride, ppi, batch, cin, G, 0x00, calls=2)
                got += run_wgrad(flat.astype(np_dtype), ld, coff, img_stride, ppi, batch, cin, G, 0xFF, calls=2)
                tag = (cout, cin, batch, ppi, ld, coff, np_dtype.__name__)
                for dw, db in got:
                    assert np.array_equal(dw, want_w), tag
                    assert np.array_equal(db, want_b), tag
                assert all(dw.tobytes() == got[0][0].tobytes() and db.tobytes() == got[0][1].tobytes() for dw, db in got), tag


def test_wgrad_unaligned_view_takes_the_element_loads():
    """ld, coff and the image stride no multiples of the 16-byte chunk, and a buffer that starts 2 bytes past one: the instantiation
    without vector loads"""
    import torch
    cin, cout, batch, ppi, ld, coff = 40, 30, 2, 37, 45, 3
    img_stride = ppi * ld + 7
    rng = np.random.RandomState(5)
    G = rng.randint(-8, 9, size=(batch * ppi, cout)).astype(np.float32)
    flat = rng.randint(-8, 9, size=batch * img_stride + 16)
    want_w, want_b = train_ref.wgrad_exact(train_ref.view_positions(flat[1:], batch, ppi, ld, coff, img_stride, cin), G)
    lib = _hip.lib()
    for np_dtype, dtype in ((np.float16, _hip.DTYPE_F16), (np.float32, _hip.DTYPE_F32)):
        d_x = torch.from_numpy(flat.astype(np_dtype)).cuda()
        d_g = torch.from_numpy(G).cuda()
        pl = plan(batch * ppi, cin, cout, dtype)
        bufs = [guarded(cout * cin * 4, 0xFF), guarded(cout * 4, 0xFF), guarded(pl["scratch_bytes"], 0xFF)]
        _hip.check(lib.yolo_conv1x1_wgrad(d_x.data_ptr() + d_x.element_size(), dtype, ld, coff, img_stride, ppi, batch, cin, d_g.data_ptr(), cout,
                                          bufs[0][1], bufs[1][1], bufs[2][1], pl["scratch_bytes"], torch.cuda.current_stream().cuda_stream),
                   "yolo_conv1x1_wgrad")
        torch.cuda.synchronize()
        check_guards(bufs)
        assert np.array_equal(bufs[0][0][GUARD:-GUARD].cpu().numpy().view(np.float32).reshape(cout, cin), want_w)
        assert np.array_equal(bufs[1][0][GUARD:-GUARD].cpu().numpy().view(np.float32), want_b)


# ---- real values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,cout,cin", [(507, 30, 136), (2704, 425, 1024)])
def test_wgrad_real_values_within_the_float32_bound(P, cout, cin):
    rng = np.random.RandomState(P + cout)
    X = rng.randn(P, cin).astype(np.float16)
    G = (np.exp2(rng.uniform(-20, 8, size=(P, cout))) * rng.choice([-1.0, 1.0], size=(P, cout))).astype(np.float32)
    ppi = 169
    (dw, db), = run_wgrad(X.reshape(-1), cin, 0, ppi * cin, ppi, P // ppi, cin, G, 0xFF)
    ref_w, ref_b, bound_w, bound_b = train_ref.wgrad_ref64(X, G)
    ratio_w = float(np.max(np.abs(dw.astype(np.float64) - ref_w) / bound_w))
    ratio_b = float(np.max(np.abs(db.astype(np.float64) - ref_b) / bound_b))
    print("wgrad P %d cout %d cin %d (%d chunks): largest |device - ref64| / bound: dW %.4f db %.4f"
          % (P, cout, cin, plan(P, cin, cout)["n_chunks"], ratio_w, ratio_b))
    assert np.all(np.abs(dw.astype(np.float64) - ref_w) <= bound_w)
    assert np.all(np.abs(db.astype(np.float64) - ref_b) <= bound_b)


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_w", [1, 255, 30 * 1024 + 3])
def test_adam_step_is_the_float32_restatement_bit_for_bit(n_w):
    import torch
    lib = _hip.lib()
    n_b = min(n_w, 30)
    rng = np.random.RandomState(n_w)
    host = {"w": rng.randn(n_w), "b": rng.randn(n_b), "m_w": np.zeros(n_w), "v_w": np.zeros(n_w), "m_b": np.zeros(n_b), "v_b": np.zeros(n_b)}
    host = {k: v.astype(np.float32) for k, v in host.items()}
    dev = {k: guarded(v.nbytes, 0) for k, v in host.items()}
    for k, v in host.items():
        dev[k][0][GUARD:-GUARD] = torch.from_numpy(v.view(np.uint8)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    saw_small = False
    for t in range(1, 6):
        dw, db = rng.randn(n_w).astype(np.float32), rng.randn(n_b).astype(np.float32)
        # zeros, a gradient whose second moment has sqrt(v) < eps, and one huge value (its square overflows: v = inf, the step 0)
        if n_w == 1:
            dw[0] = np.float32((1e-12, 0.0, 1e-12, 3e30, 0.0)[t - 1])
        else:
            dw[rng.randint(0, n_w, size=max(1, n_w // 8))] = 0.0
            dw[(t + 1) % n_w] = np.float32(1e-12)
            dw[(t + 8) % n_w] = np.float32(3e30) if t != 3 else np.float32(0.0)
        db[t % n_b] = np.float32(1e-12)
        lr_t = train_ref.adam_lr_t(1e-3, t)
        d_dw, d_db = torch.from_numpy(dw).cuda(), torch.from_numpy(db).cuda()
        _hip.check(lib.yolo_adam_step(dev["w"][1], dev["b"][1], dev["m_w"][1], dev["v_w"][1], dev["m_b"][1], dev["v_b"][1], d_dw.data_ptr(),
                                      d_db.data_ptr(), n_w, n_b, float(lr_t), 0.9, 0.999, 1e-8, st), "yolo_adam_step")
        host["w"], host["m_w"], host["v_w"] = train_ref.adam_ref32(host["w"], host["m_w"], host["v_w"], dw, lr_t)
        host["b"], host["m_b"], host["v_b"] = train_ref.adam_ref32(host["b"], host["m_b"], host["v_b"], db, lr_t)
        saw_small |= bool((np.sqrt(host["v_w"][host["v_w"] > 0]) < 1e-8).any())
        torch.cuda.synchronize()
        check_guards(dev.values())
        for k in host:
            got = dev[k][0][GUARD:-GUARD].cpu().numpy().view(np.float32)
            assert got.tobytes() == host[k].tobytes(), (n_w, t, k, np.flatnonzero(got.view(np.uint32) != host[k].view(np.uint32))[:8])
    assert np.isinf(host["v_w"]).any() and saw_small and np.isfinite(host["w"]).all()           # the yardstick itself met every case


# ---- the step is its parts; the next forward sees the update ---------------------------------------------------------------------------
HW, GRID, BATCH = (96, 160), (3, 5), 3
NAMES20 = ["c%d" % i for i in range(20)]
V2_ANCHORS = ANCHORS8[:10]
MODELS = {"v2": YoloV2, "v2-tiny": YoloV2Tiny}


@functools.lru_cache(maxsize=None)
def stream_of(version, n_classes):
    net = MODELS[version].create_network(np.reshape(V2_ANCHORS, [-1, 2]), ["c%d" % i for i in range(n_classes)], False, input_shape=HW + (3,))
    w = synth.darknet_stream(net, seed=41, num_classes=n_classes, head_gain=synth.HEAD_DEFAULTS[version][0], obj_bias=0.0)
    w.setflags(write=False)
    return w


def build(version, dtype, weights, names=NAMES20, max_batch=BATCH):
    m = MODELS[version]()
    m.build(V2_ANCHORS, names, HW + (3,), dtype=dtype, max_batch=max_batch, weights=weights, streams=1)
    return m


def state_parts(eng):
    """the master values and the four moment arrays of the engine's training state, as bytes"""
    lay = eng.train_layout
    nw, nb = lay.cout * lay.cin * 4, lay.cout * 4
    raw = eng._train_state.cpu().numpy()
    return {k: raw[int(getattr(lay, k + "_offset")):int(getattr(lay, k + "_offset")) + n].tobytes()
            for k, n in (("w", nw), ("b", nb), ("m_w", nw), ("v_w", nw), ("m_b", nb), ("v_b", nb))}


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("version", ["v2", "v2-tiny"])
def test_train_head_step_is_its_parts_and_the_next_forward_sees_it(version, dtype):
    import torch
    lib = _hip.lib()
    h, w = GRID
    A, n_classes = 5, 20
    cout = A * (5 + n_classes)
    weights = stream_of(version, n_classes)
    _, gt, counts = cases.random_case((h, w, A, n_classes, BATCH), 7)
    assert counts[1] == 0                                      # one image has no truth
    x8 = np.random.RandomState(42).randint(0, 256, size=(BATCH,) + HW + (3,)).astype(np.uint8)
    xf = (x8 / 255.).astype(np.float32)
    m = build(version, dtype, weights)
    eng = m.net.engine
    cin = ytrain.head_counts(m.net)[1]
    w0, b0 = ytrain.split_head(weights, cout, cin)
    eng.head_train_init(w0, b0)
    view = eng.head_input()
    assert (view.cin, view.h, view.w) == (cin, h, w) and view.dtype == (_hip.DTYPE_F16 if dtype == "fp16" else _hip.DTYPE_F32)
    st = torch.cuda.current_stream().cuda_stream
    hd = eng.head
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(BATCH, -1)).cuda()
    d_gc = torch.from_numpy(counts).cuda()
    # the composition's own state: master values and moments in plain tensors
    comp = {k: torch.from_numpy(np.array(v)).cuda() for k, v in
            (("w", w0.reshape(-1)), ("b", b0), ("m_w", np.zeros(cout * cin, np.float32)), ("v_w", np.zeros(cout * cin, np.float32)),
             ("m_b", np.zeros(cout, np.float32)), ("v_b", np.zeros(cout, np.float32)))}
    pl = plan(BATCH * h * w, cin, cout, view.dtype)
    images = torch.empty(BATCH * 56, dtype=torch.uint8, device="cuda")
    assign = torch.empty(BATCH * h * w, dtype=torch.int32, device="cuda")
    result = torch.empty(64, dtype=torch.uint8, device="cuda")
    grad = torch.empty(BATCH * h * w * cout, dtype=torch.float32, device="cuda")
    dw = torch.empty(cout * cin, dtype=torch.float32, device="cuda")
    db = torch.empty(cout, dtype=torch.float32, device="cuda")
    scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda")
    results = []
    for t in (1, 2):
        lr_t = engine.adam_lr_t(1e-3, t)
        assert lr_t == train_ref.adam_lr_t(1e-3, t)
        logits = eng.forward(xf)
        _hip.check(lib.yolo_v2_loss_grad(C.byref(hd), logits.data_ptr(), BATCH, d_gt.data_ptr(), d_gc.data_ptr(), gt.shape[1], images.data_ptr(),
                                         assign.data_ptr(), result.data_ptr(), grad.data_ptr(), st), "yolo_v2_loss_grad")
        _hip.check(lib.yolo_conv1x1_wgrad(eng._workspace.data_ptr() + view.offset, view.dtype, view.ld, view.coff, view.image_stride, h * w, BATCH,
                                          cin, grad.data_ptr(), cout, dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), scratch.numel(), st),
                   "yolo_conv1x1_wgrad")
        _hip.check(lib.yolo_adam_step(comp["w"].data_ptr(), comp["b"].data_ptr(), comp["m_w"].data_ptr(), comp["v_w"].data_ptr(),
                                      comp["m_b"].data_ptr(), comp["v_b"].data_ptr(), dw.data_ptr(), db.data_ptr(), cout * cin, cout, float(lr_t),
                                      0.9, 0.999, 1e-8, st), "yolo_adam_step")
        want_result = result.cpu().numpy().tobytes()
        got_result = eng.train_head_step(xf, (gt, counts), lr_t).cpu().numpy().tobytes()
        assert got_result == want_result, (version, dtype, t)
        got = state_parts(eng)
        for k, v in comp.items():
            assert got[k] == v.cpu().numpy().tobytes(), (version, dtype, t, k)
        results.append(got_result)
    assert results[0] != results[1] and np.isfinite(np.frombuffer(results[1], dtype=yeval.LOSS_RESULT_DTYPE)[0]["loss"])
    after_float = state_parts(eng)
    w2, b2 = eng.head_train_read()
    assert w2.tobytes() == after_float["w"] and b2.tobytes() == after_float["b"] and w2.tobytes() != w0.tobytes()
    # the uint8 twin, from the same start: the same bits as the float32 entry fed float32(u / 255.)
    eng.head_train_init(w0, b0)
    for t in (1, 2):
        assert eng.train_head_step_u8(x8, (gt, counts), engine.adam_lr_t(1e-3, t)).cpu().numpy().tobytes() == results[t - 1]
    assert state_parts(eng) == after_float
    # the re-pack: a second net, loaded with the master values through yolo_net_load_weights, computes the same logits on a fresh input
    fresh = synth.synthetic_input(BATCH, HW[0], HW[1], 3, seed=43)
    stepped = eng.forward(fresh).cpu().numpy()
    second = build(version, dtype, ytrain.replace_head(weights, w2, b2))
    assert second.net.engine.forward(fresh).cpu().numpy().tobytes() == stepped.tobytes()
    assert build(version, dtype, weights).net.engine.forward(fresh).cpu().numpy().tobytes() != stepped.tobytes()


# ---- it trains --------------------------------------------------------------------------------------------------------------------------
def test_forty_steps_on_a_fixed_batch_lower_the_loss():
    """grid 3 x 5, batch 4, 1 class, 5 anchors, lr 1e-3; beside it the float64 loop of tests/train_ref.py on the device's features.  Only
    the ordering of the two endpoints is asserted (and that everything is finite): float32 steps and a float64 yardstick drift apart."""
    import torch
    h, w = GRID
    A, n_classes, B, steps = 5, 1, 4, 40
    cout = A * (5 + n_classes)
    weights = stream_of("v2-tiny", n_classes)
    _, gt, counts = cases.random_case((h, w, A, n_classes, B), 7)
    x = synth.synthetic_input(B, HW[0], HW[1], 3, seed=44)
    m = build("v2-tiny", "fp32", weights, names=["tower"], max_batch=B)
    eng = m.net.engine
    cin = ytrain.head_counts(m.net)[1]
    w0, b0 = ytrain.split_head(weights, cout, cin)
    eng.head_train_init(w0, b0)
    # the device's X: the view of yolo_net_head_input after a dense forward
    eng.forward(x)
    torch.cuda.synchronize()
    view = eng.head_input()
    flat = eng._workspace[view.offset:view.offset + 4 * B * view.image_stride].cpu().numpy().view(np.float32)
    X = train_ref.view_positions(flat, B, h * w, view.ld, view.coff, view.image_stride, cin)
    records = torch.empty((steps, 64), dtype=torch.uint8, device="cuda")
    for t in range(1, steps + 1):
        eng.train_head_step(x, (gt, counts), engine.adam_lr_t(1e-3, t), result=records[t - 1])
    dev = [float(r["loss"]) for r in records.cpu().numpy().view(yeval.LOSS_RESULT_DTYPE).reshape(-1)]        # the one read
    ref, _, _ = train_ref.head_train_loop64(X, w0, b0, h, w, V2_ANCHORS, n_classes, gt, counts, 1e-3, steps)
    print("device :", " ".join("%.4f" % v for v in dev))
    print("float64:", " ".join("%.4f" % v for v in ref))
    assert np.isfinite(dev).all() and np.isfinite(ref).all()
    assert dev[-1] < dev[0] and ref[-1] < ref[0]


# ---- refusals that need a device --------------------------------------------------------------------------------------------------------
def test_step_refuses_a_null_state_and_a_missing_init():
    import torch
    m = build("v2-tiny", "fp16", stream_of("v2-tiny", 20))
    eng = m.net.engine
    with pytest.raises(RuntimeError, match="follows head_train_init"):
        eng.train_head_step(np.zeros((1,) + HW + (3,), np.float32), [[]], 1e-3)
    x = torch.zeros((1,) + HW + (3,), dtype=torch.float32, device="cuda")
    gt, counts = yeval.pack_gts([[]], 1)
    d_gt, d_gc = torch.from_numpy(gt.view(np.uint8).reshape(1, -1)).cuda(), torch.from_numpy(counts).cuda()
    res = torch.empty(64, dtype=torch.uint8, device="cuda")
    rc = eng.lib.yolo_net_train_head_step(eng.handle, x.data_ptr(), 1, d_gt.data_ptr(), d_gc.data_ptr(), 1, None, 1e-3, res.data_ptr(), None)
    assert rc == 1 and b"null state" in eng.lib.yolo_last_error()


# ---- train mode -------------------------------------------------------------------------------------------------------------------------
VOC_XML = ("<annotation><filename>%s</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>"
           "<object><name>tower</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object></annotation>")


def test_launcher_mode_train(tmp_path, capsys):
    """five images at batch 2, two epochs, a checkpoint every 2 steps, from a backbone-only weight file: the reference's lines, and
    checkpoints that differ from the pretrained stream in the head's floats only"""
    from PIL import Image
    rng = np.random.RandomState(51)
    for d in ("train", "val", "out"):
        (tmp_path / d).mkdir()
    for d, n in (("train", 5), ("val", 3)):
        for i in range(n):
            name = "im%d.png" % i
            Image.fromarray(rng.randint(0, 256, size=(120, 200, 3)).astype(np.uint8)).save(str(tmp_path / d / name))
            x1, y1 = int(rng.randint(0, 100)), int(rng.randint(0, 60))
            (tmp_path / d / ("im%d.xml" % i)).write_text(VOC_XML % (name, 200, 120, x1, y1, x1 + int(rng.randint(20, 100)), y1 + int(rng.randint(20, 60))))
    anchors = V2_ANCHORS
    full = stream_of("v2-tiny", 1)
    cout, cin = 5 * 6, 1024
    backbone = full[:len(full) - cout * (cin + 1)]
    base.write_darknet_weights(str(tmp_path / "backbone.weights"), backbone, "v2")
    (tmp_path / "cfg.ini").write_text(
        "[COMMON]\nversion = v2-tiny\ninput_h = %d\ninput_w = %d\ninput_c = 3\n"
        "[TRAIN]\ntrain_layers = head\nseed = 3\nimage_dir = train/\nannotation_dir = train/\nval_image_dir = val/\nval_annotation_dir = val/\n"
        "batch_size = 2\nlearning_rate = 1e-3\nepochs = 2\nmax_step = -1\naugment_probability = 0.0\ncheckpoint_dir = out/\ncheckpoint_step = 2\n"
        "checkpoint_prefix = yolo\ntensorboard_log_dir = log/\npretrained_weights_path = backbone.weights\nanchors = %s\nclass_names = [\"tower\"]\n"
        "cpu_only = False\ndtype = fp16\n" % (HW[0], HW[1], list(anchors)))
    launcher.run(launcher.read_config(str(tmp_path / "cfg.ini")), "train")
    out = capsys.readouterr().out.splitlines()
    steps = [l for l in out if l.startswith("step ")]
    assert len(steps) == 6 and steps[0].startswith("step 1 (1/2): ") and steps[5].startswith("step 6 (2/2): ") and "(moving average: " in steps[3]
    assert sum(l.startswith("validation loss: ") for l in out) == 3 and out[-1] == "Done" and "Epoch (2/2) completed." in out
    assert any("tensorboard_log_dir is ignored" in l for l in out) and any("drawn from N(0, 0.02)" in l for l in out)
    losses = [float(l.split(": ")[1].split(" ")[0]) for l in steps]
    assert np.isfinite(losses).all()
    header0, body0 = base.read_darknet_weights(str(tmp_path / "out" / "yolo-0.weights"), "v2")
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["yolo-%d.weights" % s for s in (0, 2, 4, 6)]
    for s in (2, 4, 6):
        header, body = base.read_darknet_weights(str(tmp_path / "out" / ("yolo-%d.weights" % s)), "v2")
        assert header == header0 and len(body) == len(full)
        assert body[:len(backbone)].tobytes() == backbone.tobytes() and body[len(backbone):].tobytes() != body0[len(backbone):].tobytes()
    assert body0[:len(backbone)].tobytes() == backbone.tobytes() and not body0[len(backbone):len(backbone) + cout].any()

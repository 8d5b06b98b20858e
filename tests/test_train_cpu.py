"""CPU: the host side of the head training -- yolo_wgrad_plan pinned for the shapes the GPU tests run, the yardstick of tests/train_ref.py
against torch.optim.Adam, every refusal that needs no device, the reference's batching, checkpoints, and the sanitizer run of the host
code as a program of its own."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import train_ref
from helpers import ROOT
from tensorflow_yolo_amd import YoloV2, YoloV2Tiny, YoloV3Tiny, _hip, launcher
from tensorflow_yolo_amd.net import base, engine, train as ytrain, v2, v3

NAMES3 = ["a", "b", "c"]
V2_ANCHORS = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071]


# ---- yolo_wgrad_plan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [_hip.DTYPE_F16, _hip.DTYPE_F32])
def test_wgrad_plan_is_pinned_for_the_shapes_the_gpu_tests_run(dtype):
    for cout in train_ref.COUTS:
        for cin in train_ref.CINS:
            plan = lambda P: _hip.wgrad_plan(P, cin, cout, dtype)
            one = plan(1)
            assert (one["tile_cout"], one["tile_cin"], one["tile_positions"]) == (64, 128, 16)
            assert one["tiles_cout"] == -(-cout // 64) and one["tiles_cin"] == -(-cin // 128)
            ppc = one["positions_per_chunk"]
            seen = []
            for batch, ppi, gap, chunks in train_ref.wgrad_position_cases(plan):
                P = batch * ppi
                pl = plan(P)
                assert 1 <= P <= 4096 and pl["positions_per_chunk"] % pl["tile_positions"] == 0
                # the chunks [k * ppc, min(P, (k + 1) * ppc)) cover [0, P) once and none is empty
                assert pl["n_chunks"] == chunks == -(-P // pl["positions_per_chunk"])
                assert pl["scratch_bytes"] == pl["n_chunks"] * cout * (cin + 1) * 4
                if batch == 1:
                    assert pl["positions_per_chunk"] == ppc         # the cases around a chunk's end are sized from the same chunk
                seen.append(pl["n_chunks"])
            # one chunk three times (1 position, one short, exactly one), two, three with a ragged last, and many across image borders
            assert seen[:5] == [1, 1, 1, 2, 3] and seen[5] >= 3
            last = plan(2 * ppc + 5)
            assert 2 * ppc + 5 - 2 * last["positions_per_chunk"] == 5 and 5 % last["tile_positions"] != 0


def test_wgrad_plan_splits_the_flagship_shapes_over_the_chip():
    """COCO at batch 16 (P = 2704, 425 x 1024) and the one-class head at batch 64: enough workgroups for 256 CUs, and a scratch of tens of
    megabytes at most"""
    for P, cout in ((2704, 425), (10816, 30), (2704, 125)):
        pl = _hip.wgrad_plan(P, 1024, cout)
        grid = pl["tiles_cout"] * pl["tiles_cin"] * pl["n_chunks"]
        assert 256 <= grid <= 1024 and pl["scratch_bytes"] <= 64 << 20, (P, cout, pl)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def last_error():
    return _hip.lib().yolo_last_error().decode()


def test_wgrad_refusals():
    lib = _hip.lib()
    pl = _hip.WgradPlan()
    assert lib.yolo_wgrad_plan(64, 12, 30, _hip.DTYPE_F16, C.byref(pl)) == 1 and "multiple of 8" in last_error()
    assert lib.yolo_wgrad_plan(64, 16, 30, _hip.DTYPE_MXF8, C.byref(pl)) == 1 and "x_dtype" in last_error()
    assert lib.yolo_wgrad_plan(0, 16, 30, _hip.DTYPE_F16, C.byref(pl)) == 1
    assert lib.yolo_wgrad_plan(64, 16, 30, _hip.DTYPE_F16, None) == 1
    # the checks run before anything is launched: numbers stand in for device pointers
    need = _hip.wgrad_plan(64, 16, 30)["scratch_bytes"]
    p = 4096
    good = [p, _hip.DTYPE_F16, 16, 0, 64 * 16, 64, 1, 16, p, 30, p, p, p, need, None]
    for at, value, word in ((7, 12, "multiple of 8"), (13, need - 1, "scratch too small"), (0, None, "null"), (10, None, "null"), (12, None, "null"),
                            (2, 8, "inside the pixel stride"), (4, 63 * 16, "image_stride"), (1, _hip.DTYPE_MXF8, "x_dtype"), (6, 0, "at least 1")):
        args = list(good)
        args[at] = value
        assert lib.yolo_conv1x1_wgrad(*args) == 1 and word in last_error(), (at, last_error())
    assert lib.yolo_adam_step(None, p, p, p, p, p, p, p, 4, 4, 1e-3, 0.9, 0.999, 1e-8, None) == 1 and "null" in last_error()
    assert lib.yolo_adam_step(p, p, p, p, p, p, p, p, 0, 4, 1e-3, 0.9, 0.999, 1e-8, None) == 1
    assert lib.yolo_adam_step(p, p, p, p, p, p, p, p, 4, 4, 1e-3, 1.0, 0.999, 1e-8, None) == 1 and "beta" in last_error()


def v2_plan(streams=1, dtype="fp16", hw=(96, 160), max_batch=3):
    net = v2.create_tiny_network(np.reshape(V2_ANCHORS, [-1, 2]), NAMES3, False, input_shape=hw + (3,))
    p = engine.Plan(net, dtype=dtype, max_batch=max_batch, streams=streams)
    p.set_head(engine.head_desc_v2(hw[0] // 32, hw[1] // 32, V2_ANCHORS, len(NAMES3)))
    return p


def test_head_input_and_state_layout_of_the_v2_networks():
    for make, names in ((v2.create_full_network, ["c%d" % i for i in range(80)]), (v2.create_tiny_network, NAMES3)):
        for dtype in ("fp16", "fp32", "mxfp8"):
            net = make(np.reshape(V2_ANCHORS, [-1, 2]), names, False, input_shape=(96, 160, 3))
            p = engine.Plan(net, dtype=dtype, max_batch=3, streams=1)
            p.set_head(engine.head_desc_v2(3, 5, V2_ANCHORS, len(names)))
            view = p.head_input()           # a plain conv output in every v2 plan; an MXFP8 plan keeps its head conv fp16
            assert (view.cin, view.h, view.w) == (1024, 3, 5) and view.dtype == (_hip.DTYPE_F32 if dtype == "fp32" else _hip.DTYPE_F16)
            assert view.ld >= view.coff + view.cin and view.image_stride >= 15 * view.ld and view.offset % 256 == 0
            assert view.offset + (2 if view.dtype == _hip.DTYPE_F16 else 4) * 3 * view.image_stride <= p.workspace_bytes
            lay = p.head_train_layout()
            cout = 5 * (5 + len(names))
            assert (lay.cin, lay.cout) == (1024, cout) and lay.total_bytes == p.lib.yolo_net_head_train_bytes(p.handle)
            offs = [getattr(lay, n) for n, _ in _hip.HeadTrainLayout._fields_[:12]]
            assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and offs[0] == 0
            assert lay.b_offset >= cout * 1024 * 4 and lay.grad_offset - lay.db_offset >= cout * 4
            assert lay.assign_offset - lay.grad_offset >= 3 * 15 * cout * 4 and lay.images_offset - lay.assign_offset >= 3 * 15 * 4
            assert lay.scratch_offset - lay.images_offset >= 3 * 56
            assert lay.scratch_bytes >= max(_hip.wgrad_plan(b * 15, 1024, cout)["scratch_bytes"] for b in (1, 2, 3))
            assert lay.total_bytes >= lay.scratch_offset + lay.scratch_bytes


def test_net_refusals_without_a_device():
    lib = _hip.lib()
    # a v3 head
    anchors = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
    p3 = engine.Plan(v3.create_tiny_network(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3)), dtype="fp16", max_batch=1, streams=1)
    assert lib.yolo_net_head_train_bytes(p3.handle) == 0 and ("version 2" in last_error() or "detection layer" in last_error())
    lay = _hip.HeadTrainLayout()
    assert lib.yolo_net_head_train_layout(p3.handle, C.byref(lay)) == 1
    assert lib.yolo_net_train_head_step(p3.handle, 4096, 1, 4096, 4096, 1, 4096, 1e-3, 4096, None) == 1
    assert lib.yolo_net_head_train_init(p3.handle, 4096, 1 << 30, 4096, 4096) == 1
    # a net in two stream parts
    p2 = v2_plan(streams=2, max_batch=4)
    assert p2.num_streams == 2
    view = _hip.TensorView()
    assert lib.yolo_net_head_input(p2.handle, C.byref(view)) == 5 and "yolo_net_set_streams(net, 1)" in last_error()
    assert lib.yolo_net_head_train_bytes(p2.handle) == 0 and "yolo_net_set_streams(net, 1)" in last_error()
    assert lib.yolo_net_train_head_step(p2.handle, 4096, 1, 4096, 4096, 1, 4096, 1e-3, 4096, None) == 5
    # a null state, a null net, a head that was never set
    p1 = v2_plan()
    assert lib.yolo_net_head_train_bytes(p1.handle) > 0
    assert lib.yolo_net_train_head_step(p1.handle, 4096, 1, 4096, 4096, 1, None, 1e-3, 4096, None) == 1 and "null state" in last_error()
    assert lib.yolo_net_train_head_step_u8(p1.handle, 4096, 1, 4096, 4096, 1, None, 1e-3, 4096, None) == 1 and "null state" in last_error()
    assert lib.yolo_net_train_head_step(None, 4096, 1, 4096, 4096, 1, 4096, 1e-3, 4096, None) == 1
    assert lib.yolo_net_train_head_step(p1.handle, 4096, 1, 4096, 4096, 1, 4096 + 8, 1e-3, 4096, None) == 1 and "256-byte aligned" in last_error()
    assert lib.yolo_net_train_head_step(p1.handle, 4096, 1, 4096, 4096, 1, 4096, 1e-3, 4096, None) == 5 and "weights not loaded" in last_error()
    assert lib.yolo_net_head_train_init(p1.handle, None, 1 << 30, 4096, 4096) == 1
    assert lib.yolo_net_head_train_init(p1.handle, 4096, 16, 4096, 4096) == 1 and "state too small" in last_error()
    assert lib.yolo_net_head_train_init(p1.handle, 4096, 1 << 30, 4096, 4096) == 5 and "weights not loaded" in last_error()
    assert lib.yolo_net_head_train_read(p1.handle, None, 4096, 4096) == 1
    assert lib.yolo_net_head_input(p1.handle, None) == 1
    net = v2.create_tiny_network(np.reshape(V2_ANCHORS, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3))
    unset = engine.Plan(net, dtype="fp16", max_batch=1, streams=1)
    assert lib.yolo_net_head_train_bytes(unset.handle) == 0 and "head geometry not set" in last_error()


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def test_adam_yardstick_against_torch():
    """torch.optim.Adam in float64: w -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), which is the form of tests/train_ref.py
    (lr_t = lr sqrt(bc2) / bc1) except for where eps stands: equal with eps = 0"""
    import torch
    rng = np.random.RandomState(3)
    w0 = rng.randn(300)
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=0.0)
    w, m, v = w0.copy(), np.zeros(300), np.zeros(300)
    for t in range(1, 8):
        g = rng.randn(300) * np.exp2(rng.uniform(-10, 10, size=300))
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        lr_t = 1e-3 * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        w, m, v = train_ref.adam_ref64(w, m, v, g, lr_t, eps=0.0)
        got = p.detach().numpy()
        assert np.max(np.abs(got - w) / np.abs(w)) <= 1e-12, t
    assert np.max(np.abs(w - w0)) > 1e-3
    # the float32 restatement is the same formula: it follows the float64 one within float32 rounding
    w32, m32, v32 = train_ref.adam_ref32(w0, np.zeros(300), np.zeros(300), g, train_ref.adam_lr_t(1e-3, 1))
    w64, _, _ = train_ref.adam_ref64(w0.astype(np.float32).astype(np.float64), np.zeros(300), np.zeros(300), g.astype(np.float32).astype(np.float64),
                                     1e-3 * np.sqrt(1.0 - 0.999) / (1.0 - 0.9))
    assert np.max(np.abs(w32 - w64)) <= 4 * 2.0 ** -24 * np.max(np.abs(w64))
    assert engine.adam_lr_t(1e-3, 5) == train_ref.adam_lr_t(1e-3, 5) and engine.adam_lr_t(1e-3, 5).dtype == np.float32


def test_wgrad_yardsticks_agree():
    rng = np.random.RandomState(4)
    flat = rng.randint(-8, 9, size=3 * (13 * 48 + 24) + 16)
    X = train_ref.view_positions(flat, 3, 13, 48, 8, 13 * 48 + 24, 40)
    assert X.shape == (39, 40) and X[14, 3] == flat[1 * (13 * 48 + 24) + 1 * 48 + 8 + 3]
    G = rng.randint(-8, 9, size=(39, 6))
    dw, db = train_ref.wgrad_exact(X, G)
    assert dw[2, 5] == sum(int(G[p, 2]) * int(X[p, 5]) for p in range(39)) and db[4] == G[:, 4].sum()
    r = train_ref.wgrad_ref64(X, G)
    assert np.array_equal(r[0], dw) and np.array_equal(r[1], db) and r[2][2, 5] == 41 * 2.0 ** -24 * sum(abs(int(G[p, 2]) * int(X[p, 5])) for p in range(39))


# ---- train mode: host logic ---------------------------------------------------------------------------------------------------------------
def test_train_without_the_key_raises_todays_message():
    for model in (YoloV2(), YoloV2Tiny(), YoloV3Tiny()):
        with pytest.raises(NotImplementedError) as e:
            model.train({"batch_size": "2"})
        assert str(e.value) == "train mode is not supported by the HIP inference backend"
        for call in (lambda: model.create_loss_fn(1, None, None, None), lambda: model.make_batch(None, [], 1, None, None, 0),
                     lambda: model.create_train_optimizer(None, 1e-3)):
            with pytest.raises(NotImplementedError, match="^training is not supported by the HIP inference backend$"):
                call()


def test_train_option_and_refusals(tmp_path):
    assert ytrain.train_option({}) is False and ytrain.train_option({"train_layers": " Head "}) is True
    with pytest.raises(ValueError, match="train_layers must be head"):
        ytrain.train_option({"train_layers": "all"})
    with pytest.raises(ValueError, match="augment_probability must be 0"):
        YoloV2().train({"train_layers": "head", "augment_probability": "0.5"})
    ytrain.check_params({"augment_probability": "0.0"}, "v2-tiny")
    with pytest.raises(NotImplementedError, match="train mode is not supported by the HIP inference backend for v3-tiny networks"):
        YoloV3Tiny().train({"train_layers": "head", "augment_probability": "0"})
    # the launcher: without the key train mode ends as it did; with a bad value or augmentation it says why before anything is built
    ini = tmp_path / "cfg.ini"
    ini.write_text("[COMMON]\nversion = v2\n[TRAIN]\nbatch_size = 2\n")
    with pytest.raises(SystemExit, match="mode 'train' is not supported by the HIP inference backend"):
        launcher.run(launcher.read_config(str(ini)), "train")
    ini.write_text("[COMMON]\nversion = v2\n[TRAIN]\ntrain_layers = head\naugment_probability = 0.3\n")
    with pytest.raises(ValueError, match="augment_probability must be 0"):
        launcher.run(launcher.read_config(str(ini)), "train")
    ini.write_text("[COMMON]\nversion = v3\n[TRAIN]\ntrain_layers = head\naugment_probability = 0\n")
    with pytest.raises(NotImplementedError, match="for v3 networks"):
        launcher.run(launcher.read_config(str(ini)), "train")


def test_shipped_train_config():
    cfg = launcher.read_config(os.path.join(ROOT, "tensorflow-yolo_amd", "config", "yolo_2_head_train.ini"))
    params = dict(cfg["TRAIN"])
    params.update(cfg["COMMON"])
    assert ytrain.train_option(params) and float(params["augment_probability"]) == 0 and params["version"] == "v2"
    ytrain.check_params(params, params["version"])
    for key in ("image_dir", "annotation_dir", "val_image_dir", "val_annotation_dir", "batch_size", "learning_rate", "epochs", "max_step",
                "checkpoint_dir", "checkpoint_step", "checkpoint_prefix", "pretrained_weights_path", "anchors", "class_names", "seed"):
        assert key in params, key
    for name in ("yolo_2.ini", "yolo_3.ini", "yolov2_tiny_voc.ini"):        # the other files stay as they were: no train mode there
        assert "train_layers" not in launcher.read_config(os.path.join(ROOT, "tensorflow-yolo_amd", "config", name)).get("TRAIN", {})


def reference_batches(annotations, batch_size, seed):
    """net/v2.py:209-219 restated: shrink, pad with the first annotations, shuffle with the module's generator"""
    if len(annotations) < batch_size:
        batch_size = len(annotations)
    total_batches = int(np.ceil(len(annotations) / batch_size))
    if len(annotations) % batch_size > 0:
        annotations.extend(annotations[0:batch_size - len(annotations) % batch_size])
    random.seed(seed)
    random.shuffle(annotations)
    return [[annotations[b * batch_size + i] for i in range(batch_size)] for b in range(total_batches)]


def test_batches_are_the_references():
    for n, bs in ((7, 3), (6, 3), (2, 3), (1, 1)):
        ann = [("img%d.jpg" % i, [(0.5, 0.5, 0.1, 0.1, 0, 0)]) for i in range(n)]
        mine, theirs = list(ann), list(ann)
        got = ytrain.make_batches(mine, bs, random.Random(11))
        want = reference_batches(theirs, bs, 11)
        assert got == want and mine == theirs
    ann = [("img%d.jpg" % i, []) for i in range(7)]
    rng = random.Random(5)
    first = ytrain.make_batches(ann, 3, rng)
    assert len(first) == 3 and all(len(b) == 3 for b in first) and len(ann) == 9
    assert sorted(p for b in first for p, _ in b) == sorted(["img%d.jpg" % i for i in range(7)] + ["img0.jpg", "img1.jpg"])
    second = ytrain.make_batches(ann, 3, rng)           # the next epoch: the padded list, shuffled again
    assert len(ann) == 9 and second != first and sorted(map(str, sum(second, []))) == sorted(map(str, sum(first, [])))
    assert ytrain.make_batches([], 3, rng) == []


def test_checkpoint_roundtrip_changes_the_head_only(tmp_path):
    net = v2.create_tiny_network(np.reshape(V2_ANCHORS[:2], [-1, 2]), ["tower"], False, input_shape=(96, 160, 3))
    cout, cin, n_head, need = ytrain.head_counts(net)
    assert (cout, cin, n_head) == (6, 1024, 6 * 1025)
    rng = np.random.RandomState(8)
    body = rng.randn(need).astype(np.float32)
    w, b = ytrain.split_head(body, cout, cin)
    assert w.shape == (cout, cin) and b.tobytes() == body[need - n_head:need - n_head + cout].tobytes() and w[1, 2] == body[need - cout * cin + cin + 2]
    w2, b2 = w + np.float32(1), b - np.float32(1)
    path = ytrain.checkpoint_path(str(tmp_path / "ck"), "yolo", 20)
    assert path.endswith(os.path.join("ck", "yolo-20.weights"))
    ytrain.write_checkpoint(path, (0, 2, 0, 1234), ytrain.replace_head(body, w2, b2))
    header, back = base.read_darknet_weights(path, "v2")
    assert header == (0, 2, 0, 1234) and len(back) == need
    assert back[:need - n_head].tobytes() == body[:need - n_head].tobytes()
    wb, bb = ytrain.split_head(back, cout, cin)
    assert wb.tobytes() == w2.tobytes() and bb.tobytes() == b2.tobytes()
    ytrain.write_checkpoint(ytrain.checkpoint_path(str(tmp_path / "ck"), "yolo", 3), header, body)
    (tmp_path / "ck" / "yolo-x.weights").write_text("")
    assert ytrain.latest_checkpoint(str(tmp_path / "ck"), "yolo") == (20, path) and ytrain.latest_checkpoint(str(tmp_path / "none"), "yolo") == (-1, None)
    # a backbone-only stream gets a seeded head; anything else is refused
    full, drawn = ytrain.initial_stream(body, net, 0)
    assert not drawn and full.tobytes() == body.tobytes()
    full, drawn = ytrain.initial_stream(body[:need - n_head], net, 9)
    wd, bd = ytrain.split_head(full, cout, cin)
    assert drawn and len(full) == need and not bd.any() and 0.015 < wd.std() < 0.025 and abs(wd.mean()) < 2e-3
    assert ytrain.initial_stream(body[:need - n_head], net, 9)[0].tobytes() == full.tobytes()
    assert ytrain.initial_stream(body[:need - n_head], net, 10)[0].tobytes() != full.tobytes()
    with pytest.raises(ValueError, match="without the detection layer"):
        ytrain.initial_stream(body[:need - 1], net, 0)


# ---- host code under sanitizers -----------------------------------------------------------------------------------------------------------
def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """train_host.cpp (yolo_wgrad_plan and every argument check in front of a launch) with train_host_check.cpp, a program with its own
    main, built with -fsanitize=address,undefined and run on the CPU"""
    csrc = os.path.join(ROOT, "tensorflow-yolo_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc, "san-train", "OBJDIR=" + str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "train_host_check OK" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr

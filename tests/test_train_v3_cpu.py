"""CPU: the host side of the YOLOv3 head training -- yolo_v3_head_wgrad_plan for the shapes the GPU tests run, every refusal that needs no
device, yolo_net_head_inputs_v3 and the state layout on the three v3 networks, the `heads` train mode's host logic, the yardstick of
tests/train_v3_ref.py against itself, and the sanitizer run of the host code as a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import train_v3_ref as ref
from helpers import ROOT
from tensorflow_yolo_amd import YoloV2, YoloV3, YoloV3Tiny, _hip, launcher
from tensorflow_yolo_amd.net import engine, train as ytrain, v2, v3

NAMES3 = ["a", "b", "c"]
TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
V2_ANCHORS = [1.3221, 1.73145, 3.19275, 4.00944, 5.05587, 8.09892, 9.47112, 4.84053, 11.2364, 10.0071]
MAKERS = {"v3": (v3.create_network, V3_ANCHORS, (1024, 512, 256)), "v3-spp": (v3.create_spp_network, V3_ANCHORS, (1024, 512, 256)),
          "v3-tiny": (v3.create_tiny_network, TINY_ANCHORS, (512, 256))}


def head_of(grids, A, n_classes):
    return engine.head_desc_v3(grids, [[(1. + a, 2. + a) for a in range(A)] for _ in grids], n_classes)


def plan(grids, A, n_classes, cins, batch, dtype=_hip.DTYPE_F16):
    return _hip.v3_head_wgrad_plan(head_of(grids, A, n_classes), cins, batch, dtype)


def last_error():
    return _hip.lib().yolo_last_error().decode()


# ---- yolo_v3_head_wgrad_plan ------------------------------------------------------------------------------------------------------------
def test_plan_is_consistent_for_the_shapes_the_gpu_tests_run():
    assert C.sizeof(_hip.V3WgradPlan) == 32 + 6 * 16 + 2 * 32 + 24 and C.sizeof(_hip.V3WgradView) == 32
    names = []
    for name, grids, A, n_classes, cins, batch in ref.shape_cases(plan):
        names.append(name)
        for dtype in (_hip.DTYPE_F16, _hip.DTYPE_F32):
            pl = plan(grids, A, n_classes, cins, batch, dtype)
            assert (pl["threads"], pl["channels_per_thread"], pl["win_tile_cin"], pl["win_tile_rows"], pl["reduce_tile_chunks"]) == (256, 8, 256, 32, 256) and pl["n_scales"] == len(grids)
            end = 0
            for s, ((h, w), cin) in enumerate(zip(grids, cins)):
                P, ppc, n = pl["positions"][s], pl["positions_per_chunk"][s], pl["n_chunks"][s]
                assert P == batch * h * w <= 2 ** 24 // 64 and ppc >= pl["min_chunk"]
                assert n == -(-P // ppc)            # the chunks [k * ppc, min(P, (k + 1) * ppc)) cover [0, P) once and none is empty
                assert pl["threads_per_chunk"][s] * 8 == cin and pl["obj_workgroups"][s] == -(-n * pl["threads_per_chunk"][s] // 256)
                assert pl["win_workgroups"][s] == A * -(-(5 + n_classes) // 32) * -(-cin // 256)
                assert pl["slab_offset"][s] % 256 == 0 and pl["slab_offset"][s] >= end and pl["slab_bytes"][s] == n * (A * cin + 8) * 4
                end = pl["slab_offset"][s] + pl["slab_bytes"][s]
            assert pl["slot_offset"] % 256 == 0 and pl["slot_offset"] >= end and pl["slot_bytes"] == batch * 1024 * 4
            assert pl["scratch_bytes"] >= pl["slot_offset"] + pl["slot_bytes"]
            assert ref.expected_chunks(name, pl["positions"][0], pl["positions_per_chunk"][0], pl["reduce_tile_chunks"]), (name, pl)
    assert len(set(names)) == len(names) == 11


def test_plan_splits_the_flagship_heads_over_the_chip():
    """YOLOv3-608 at batch 16 and 32, YOLOv3-tiny-416 at batch 64: the objectness launch (all scales) has at least a workgroup for every
    second CU and the scratch stays in the tens of megabytes"""
    for grids, cins, batch in ((((19, 19), (38, 38), (76, 76)), (1024, 512, 256), 16), (((19, 19), (38, 38), (76, 76)), (1024, 512, 256), 32),
                               (((13, 13), (26, 26)), (512, 256), 64)):
        pl = plan(grids, 3, 80, cins, batch)
        assert sum(pl["obj_workgroups"]) >= 128 and pl["scratch_bytes"] <= 64 << 20, pl


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_wgrad_refusals():
    lib = _hip.lib()
    pl = _hip.V3WgradPlan()
    hd = head_of(ref.GRIDS3, 3, 3)
    cins = (C.c_int32 * 4)(1024, 136, 40, 0)
    assert lib.yolo_v3_head_wgrad_plan(C.byref(hd), cins, 2, _hip.DTYPE_F16, C.byref(pl)) == 0
    assert lib.yolo_v3_head_wgrad_plan(C.byref(hd), (C.c_int32 * 4)(1024, 12, 40, 0), 2, _hip.DTYPE_F16, C.byref(pl)) == 1
    assert last_error() == "yolo_v3_head_wgrad_plan: scale 1: cin must be a positive multiple of 8"
    assert lib.yolo_v3_head_wgrad_plan(C.byref(hd), cins, 2, _hip.DTYPE_MXF8, C.byref(pl)) == 1 and "x_dtype" in last_error()
    assert lib.yolo_v3_head_wgrad_plan(C.byref(hd), cins, 0, _hip.DTYPE_F16, C.byref(pl)) == 1 and "batch" in last_error()
    assert lib.yolo_v3_head_wgrad_plan(C.byref(hd), cins, 2, _hip.DTYPE_F16, None) == 1 and "null" in last_error()
    assert lib.yolo_v3_head_wgrad_plan(None, cins, 2, _hip.DTYPE_F16, C.byref(pl)) == 1
    v2_head = engine.head_desc_v2(3, 5, V2_ANCHORS, 3)
    assert lib.yolo_v3_head_wgrad_plan(C.byref(v2_head), cins, 2, _hip.DTYPE_F16, C.byref(pl)) == 1
    assert last_error() == "yolo_v3_head_wgrad_plan: the head must be version 3"
    # the checks run before anything is launched: numbers stand in for device pointers
    need = plan(ref.GRIDS3, 3, 3, (1024, 136, 40), 2)["scratch_bytes"]
    p = 4096

    def call(head=hd, batch=2, g=p, table=p, max_gt=8, dw=(p, p, p), db=(p, p, p), scratch=p, nbytes=need, **change):
        views = (_hip.V3WgradView * 4)()
        for s, ((h, w), cin) in enumerate(zip(ref.GRIDS3, (1024, 136, 40))):
            views[s].x_dev, views[s].image_stride, views[s].ld, views[s].coff, views[s].dtype, views[s].cin = p, h * w * cin, cin, 0, _hip.DTYPE_F16, cin
        for (s, field), value in change.get("view", {}).items():
            setattr(views[s], field, value)
        return lib.yolo_v3_head_wgrad(C.byref(head) if head is not None else None, views, batch, g, table, max_gt, (C.c_void_p * 4)(*dw),
                                      (C.c_void_p * 4)(*db), scratch, nbytes, None)

    for kw, word in (({"head": None}, "null argument"), ({"g": None}, "null argument"), ({"table": None}, "null argument"),
                     ({"scratch": None}, "null argument"), ({"dw": (p, None, p)}, "scale 1: null argument"), ({"db": (p, p, None)}, "scale 2: null argument"),
                     ({"view": {(0, "x_dev"): None}}, "scale 0: null argument"), ({"view": {(1, "dtype"): _hip.DTYPE_MXF8}}, "scale 1: dtype must be"),
                     ({"view": {(2, "cin"): 36}}, "scale 2: cin must be a positive multiple of 8"),
                     ({"view": {(1, "ld"): 128}}, "scale 1: the channels coff .. coff + cin must lie inside the pixel stride ld"),
                     ({"view": {(1, "coff"): 8}}, "inside the pixel stride"), ({"view": {(2, "image_stride"): 96 * 40 - 1}}, "scale 2: image_stride is smaller"),
                     ({"view": {(0, "x_dev"): p + 1}}, "not aligned to its element type"), ({"nbytes": need - 1}, "scratch too small"),
                     ({"scratch": p + 4}, "scratch_dev must be 16-byte aligned"), ({"batch": 0}, "batch must be at least 1"),
                     ({"max_gt": 0}, "max_gt must be 1..1024"), ({"max_gt": 1025}, "max_gt must be 1..1024"), ({"head": v2_head}, "the head must be version 3")):
        assert call(**kw) == 1 and last_error().startswith("yolo_v3_head_wgrad: ") and word in last_error(), (kw, last_error())


# ---- yolo_net_head_inputs_v3, the state -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(MAKERS))
def test_head_inputs_and_state_layout_of_the_v3_networks(model):
    make, anchors, cins = MAKERS[model]
    lib = _hip.lib()
    for dtype in ("fp16", "fp32", "mxfp8"):
        net = make(np.reshape(anchors, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3))
        p = engine.Plan(net, dtype=dtype, max_batch=3, streams=1)
        views = p.head_inputs_v3()
        grids = [(3 << s, 5 << s) for s in range(len(cins))]
        assert [(v.cin, v.h, v.w) for v in views] == [(c,) + g for c, g in zip(cins, grids)]
        esz = 4 if dtype == "fp32" else 2           # an MXFP8 plan keeps its head convs fp16
        for v, (h, w) in zip(views, grids):
            assert v.dtype == (_hip.DTYPE_F32 if dtype == "fp32" else _hip.DTYPE_F16)
            assert v.ld >= v.coff + v.cin and v.image_stride >= h * w * v.ld and v.offset % 256 == 0
            assert v.offset + esz * 3 * v.image_stride <= p.workspace_bytes
        # no two inputs share bytes
        spans = sorted((v.offset, v.offset + esz * 3 * v.image_stride) for v in views)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        lay = p.head_train_layout_v3()
        heads = ytrain.head_convs_v3(net)
        ns = len(cins)
        assert lay.n_scales == ns and list(lay.cin[:ns]) == list(cins) and list(lay.cout[:ns]) == [3 * 8] * ns
        assert [int(lay.bias_src[s]) for s in range(ns)] == [pos for pos, _, _ in heads]         # the stream positions of the Python layer list
        assert [(cout, cin) for _, cout, cin in heads] == [(24, c) for c in cins]
        offs = [int(getattr(lay, k + "_offset")[s]) for s in range(ns) for k in ("w", "b", "m_w", "v_w", "m_b", "v_b", "dw", "db")]
        offs += [int(lay.grad_offset), int(lay.assign_offset), int(lay.parts_offset), int(lay.images_offset), int(lay.scratch_offset)]
        assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and offs[0] == 0 and len(set(offs)) == len(offs)
        R, parts = engine.v3_loss_rows(p.head)
        assert lay.assign_offset - lay.grad_offset >= 3 * R * 8 * 4 and lay.parts_offset - lay.assign_offset >= 3 * R * 4
        assert lay.images_offset - lay.parts_offset >= 3 * parts * 56 and lay.scratch_offset - lay.images_offset >= 3 * 56
        # the scratch holds the largest split of any batch up to max_batch
        assert lay.scratch_bytes == max(_hip.v3_head_wgrad_plan(p.head, cins, b)["scratch_bytes"] for b in (1, 2, 3))
        assert lay.total_bytes >= lay.scratch_offset + lay.scratch_bytes and lay.total_bytes == lib.yolo_net_head_train_v3_bytes(p.handle)


def test_net_refusals_without_a_device():
    lib = _hip.lib()
    net = v3.create_network(np.reshape(V3_ANCHORS, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3))
    # two stream parts
    p2 = engine.Plan(net, dtype="fp16", max_batch=4, streams=2)
    assert p2.num_streams == 2
    views, n = (_hip.TensorView * 4)(), C.c_int32(0)
    assert lib.yolo_net_head_inputs_v3(p2.handle, views, C.byref(n)) == 5
    assert last_error().startswith("yolo_net_head_inputs_v3: this net runs a batch as 2 stream parts") and "call yolo_net_set_streams(net, 1)" in last_error()
    assert lib.yolo_net_head_train_v3_bytes(p2.handle) == 0 and "yolo_net_set_streams(net, 1)" in last_error()
    assert lib.yolo_net_train_head_step_v3(p2.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096, 1e-3, 4096, None) == 5
    # a v2 net
    pv2 = engine.Plan(v2.create_tiny_network(np.reshape(V2_ANCHORS, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3)), dtype="fp16", max_batch=1, streams=1)
    assert lib.yolo_net_head_inputs_v3(pv2.handle, views, C.byref(n)) == 5 and "head geometry not set" in last_error()
    pv2.set_head(engine.head_desc_v2(3, 5, V2_ANCHORS, 3))
    assert lib.yolo_net_head_inputs_v3(pv2.handle, views, C.byref(n)) == 1 and "yolo_net_head_inputs_v3: the head must be version 3" in last_error()
    assert lib.yolo_net_head_train_v3_bytes(pv2.handle) == 0 and "the head must be version 3" in last_error()
    # the old entries still refuse a v3 net, with the messages they had
    p1 = engine.Plan(net, dtype="fp16", max_batch=2, streams=1)
    assert lib.yolo_net_head_train_bytes(p1.handle) == 0 and "the head must be version 2 with one scale" in last_error()
    assert lib.yolo_net_train_head_step(p1.handle, 4096, 1, 4096, 4096, 1, 4096, 1e-3, 4096, None) == 1
    # nulls, a null state, alignment, call order
    assert lib.yolo_net_head_inputs_v3(None, views, C.byref(n)) == 1 and lib.yolo_net_head_inputs_v3(p1.handle, None, C.byref(n)) == 1
    assert lib.yolo_net_head_inputs_v3(p1.handle, views, None) == 1 and lib.yolo_net_head_train_v3_layout(p1.handle, None) == 1
    assert lib.yolo_net_head_inputs_v3(p1.handle, views, C.byref(n)) == 0 and n.value == 3
    for name in ("yolo_net_train_head_step_v3", "yolo_net_train_head_step_v3_u8"):
        fn = getattr(lib, name)
        assert fn(p1.handle, 4096, 1, 4096, 4096, 1, 0.7, None, 1e-3, 4096, None) == 1 and last_error() == name + ": null state (yolo_net_head_train_v3_init)"
        assert fn(None, 4096, 1, 4096, 4096, 1, 0.7, 4096, 1e-3, 4096, None) == 1
        assert fn(p1.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096 + 8, 1e-3, 4096, None) == 1 and "256-byte aligned" in last_error()
        assert fn(p1.handle, 4096, 1, 4096, 4096, 1, 0.0, 4096, 1e-3, 4096, None) == 1 and "ignore_thresh" in last_error()
        assert fn(p1.handle, 4096, 1, 4096, 4096, 0, 0.7, 4096, 1e-3, 4096, None) == 1 and "max_gt" in last_error()
        assert fn(p1.handle, 4096, 1, None, 4096, 1, 0.7, 4096, 1e-3, 4096, None) == 1 and "null argument" in last_error()
        assert fn(p1.handle, 4096, 3, 4096, 4096, 1, 0.7, 4096, 1e-3, 4096, None) == 1 and "batch outside 1..max_batch" in last_error()
        assert fn(p1.handle, 4096, 1, 4096, 4096, 1, 0.7, 4096, 1e-3, 4096, None) == 5 and "weights not loaded" in last_error()
    ptrs = (C.c_void_p * 4)(4096, 4096, 4096, 0)
    assert lib.yolo_net_head_train_v3_init(p1.handle, None, 1 << 30, ptrs, ptrs) == 1
    assert lib.yolo_net_head_train_v3_init(p1.handle, 4096, 16, ptrs, ptrs) == 1 and "state too small" in last_error()
    assert lib.yolo_net_head_train_v3_init(p1.handle, 4096, 1 << 30, (C.c_void_p * 4)(4096, 0, 4096, 0), ptrs) == 1 and "scale 1: null argument" in last_error()
    assert lib.yolo_net_head_train_v3_init(p1.handle, 4096, 1 << 30, ptrs, ptrs) == 5 and "weights not loaded" in last_error()
    assert lib.yolo_net_head_train_v3_read(p1.handle, None, ptrs, ptrs) == 1


# ---- train mode: host logic ---------------------------------------------------------------------------------------------------------------
def test_train_option_heads_and_refusals(tmp_path):
    assert ytrain.train_option({}) is False and ytrain.train_option({"train_layers": " Head "}) is True          # as it was
    assert ytrain.train_option({"train_layers": "heads"}) is True and ytrain.train_layers({"train_layers": " HEADS "}) == "heads"
    assert ytrain.train_layers({}) is None and ytrain.train_layers({"train_layers": "head"}) == "head"
    with pytest.raises(ValueError, match="^train_layers must be head "):
        ytrain.train_option({"train_layers": "all"})
    for version in ("v3", "v3-tiny", "v3-spp"):
        assert ytrain.check_params({"train_layers": "heads"}, version) == 0.0
        with pytest.raises(NotImplementedError, match="train mode is not supported by the HIP inference backend for %s networks: the reference has a "
                                                      "loss for YOLOv2 only" % version):
            ytrain.check_params({"train_layers": "head"}, version)
    for version in ("v2", "v2-tiny"):
        with pytest.raises(ValueError, match="train_layers = heads trains the detection convs of a v3 network"):
            ytrain.check_params({"train_layers": "heads"}, version)
    with pytest.raises(ValueError, match="train_layers = heads"):
        YoloV2().train({"train_layers": "heads", "augment_probability": "0"})
    with pytest.raises(ValueError, match="ignore_thresh must be in"):
        ytrain.check_params({"train_layers": "heads", "ignore_thresh": "1.5"}, "v3")
    with pytest.raises(ValueError, match="augment_probability must be 0"):
        YoloV3Tiny().train({"train_layers": "heads", "augment_probability": "0.5"})
    assert ytrain.check_params({"train_layers": "heads", "augment": "device", "augment_probability": "0.5", "ignore_thresh": "0.5"}, "v3") == 0.5
    ini = tmp_path / "cfg.ini"
    ini.write_text("[COMMON]\nversion = v2\n[TRAIN]\ntrain_layers = heads\naugment_probability = 0\n")
    with pytest.raises(ValueError, match="a v2 network takes train_layers = head"):
        launcher.run(launcher.read_config(str(ini)), "train")


def test_shipped_v3_train_config():
    cfg = launcher.read_config(os.path.join(ROOT, "tensorflow-yolo_amd", "config", "yolo_3_head_train.ini"))
    params = dict(cfg["TRAIN"])
    params.update(cfg["COMMON"])
    assert ytrain.train_layers(params) == "heads" and params["version"] == "v3" and float(params["ignore_thresh"]) == 0.7
    assert ytrain.check_params(params, params["version"]) == 0.0 and int(params["pretrained_classes"]) == 80
    for key in ("image_dir", "annotation_dir", "val_image_dir", "val_annotation_dir", "batch_size", "learning_rate", "epochs", "max_step",
                "checkpoint_dir", "checkpoint_step", "checkpoint_prefix", "pretrained_weights_path", "anchors", "class_names", "seed"):
        assert key in params, key
    assert len(params["anchors"]) == 18 and len(params["class_names"]) == 3
    assert "yolo_3_head_train.ini" in open(os.path.join(ROOT, "README.md")).read()


def test_heads_are_cut_replaced_and_seeded_at_their_stream_positions():
    make = v3.create_tiny_network
    net = make(np.reshape(TINY_ANCHORS, [-1, 2]), NAMES3, False, input_shape=(96, 160, 3))
    heads = ytrain.head_convs_v3(net)
    need = sum(l.weight_count() for l in net if hasattr(l, "weight_count"))
    assert [(cout, cin) for _, cout, cin in heads] == [(24, 512), (24, 256)] and heads[1][0] + 24 * 257 == need
    body = np.random.RandomState(8).randn(need).astype(np.float32)
    ws, bs = ytrain.split_heads(body, heads)
    for (pos, cout, cin), w, b in zip(heads, ws, bs):
        assert w.shape == (cout, cin) and b.tobytes() == body[pos:pos + cout].tobytes() and w[1, 2] == body[pos + cout + cin + 2]
    assert ytrain.replace_heads(body, heads, ws, bs).tobytes() == body.tobytes()
    ws2, bs2 = [w + np.float32(1) for w in ws], [b - np.float32(1) for b in bs]
    back = ytrain.replace_heads(body, heads, ws2, bs2)
    inside = np.zeros(need, dtype=bool)
    for pos, cout, cin in heads:
        inside[pos:pos + cout * (cin + 1)] = True
    assert back[~inside].tobytes() == body[~inside].tobytes() and (back[inside] != body[inside]).all()
    wb, bb = ytrain.split_heads(back, heads)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(wb + bb, ws2 + bs2))
    # a stream of the net's own length is used as it is
    full, drawn = ytrain.initial_stream_v3(body, net, None, 0)
    assert not drawn and full.tobytes() == body.tobytes()
    # a stream of the same network for 80 classes: everything outside the heads is kept, the heads are drawn
    net80 = make(np.reshape(TINY_ANCHORS, [-1, 2]), ["c%d" % i for i in range(80)], False, input_shape=(96, 160, 3))
    heads80 = ytrain.head_convs_v3(net80)
    need80 = sum(l.weight_count() for l in net80 if hasattr(l, "weight_count"))
    body80 = np.random.RandomState(9).randn(need80).astype(np.float32)
    inside80 = np.zeros(need80, dtype=bool)
    for pos, cout, cin in heads80:
        inside80[pos:pos + cout * (cin + 1)] = True
    full, drawn = ytrain.initial_stream_v3(body80, net, net80, 9)
    assert drawn and len(full) == need and full[~inside].tobytes() == body80[~inside80].tobytes()
    wd, bd = ytrain.split_heads(full, heads)
    assert not any(b.any() for b in bd) and all(0.015 < w.std() < 0.025 and abs(w.mean()) < 3e-3 for w in wd)
    assert ytrain.initial_stream_v3(body80, net, net80, 9)[0].tobytes() == full.tobytes()
    assert ytrain.initial_stream_v3(body80, net, net80, 10)[0].tobytes() != full.tobytes()
    with pytest.raises(ValueError, match="weight file holds %d values, the network needs %d \\(%d with pretrained_classes" % (need - 1, need, need80)):
        ytrain.initial_stream_v3(body[:need - 1], net, net80, 0)
    with pytest.raises(ValueError, match="no pretrained_classes key"):
        ytrain.initial_stream_v3(body80, net, None, 0)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def test_yardstick_modes_agree_and_the_sparse_sum_is_the_dense_one_when_the_zeros_are_zeros():
    grids, A, n_classes, cins, batch = ref.GRIDS3, 3, 3, (16, 8, 24), 3
    width = 5 + n_classes
    rng = np.random.RandomState(4)
    R, scales = ref.scales_of(grids, A)
    assert R == (6 + 24 + 96) * 3 and [s[0] for s in scales] == [0, 18, 90]
    for pattern in ref.PATTERNS:
        table = ref.make_table(pattern, grids, A, batch, rng)
        n_win = int((table >= 0).sum())
        assert n_win == {"none": 0, "one": 1, "full-image": ref.MAX_GT, "edges": 6, "two-anchors": 4}[pattern] and (table == -2).any()
        G = ref.integer_g(table, width, rng)
        Gp = ref.integer_g(table, width, np.random.RandomState(0), poison=True)
        Gp[~np.isnan(Gp)] = G[~np.isnan(Gp)]
        mask = ref.terms(table, width, ref.MAX_GT)
        assert mask.sum() == batch * R + n_win * (width - 1) and not G[~mask].any() and not G[table == -2].any()
        Xs = [rng.randint(-8, 9, size=(batch * h * w, c)) for (h, w), c in zip(grids, cins)]
        exact, exact_p = (ref.wgrad_exact(Xs, g, table, grids, A, ref.MAX_GT) for g in (G, Gp))
        f64 = ref.wgrad_ref64(Xs, Gp, table, grids, A, ref.MAX_GT)
        for s, sc in enumerate(scales):
            Gs, Ms = ref.scale_operands(G, mask, sc)
            assert np.array_equal(exact[s][0], Gs.astype(np.int64).T @ Xs[s]) and np.array_equal(exact[s][1], Gs.astype(np.int64).sum(axis=0))
            assert np.array_equal(exact[s][0], exact_p[s][0]) and np.array_equal(exact[s][1], exact_p[s][1])       # the poison is never looked at
            assert np.array_equal(f64[s][0], exact[s][0]) and np.array_equal(f64[s][1], exact[s][1])
            o = 4                                       # an objectness row: T = every position of the scale
            assert f64[s][3][o] == (Ms[:, o].sum() + 2) * 2.0 ** -24 * np.abs(Gs[:, o]).sum() and Ms[:, o].sum() == Gs.shape[0]
        slot = ref.slot_table(table, ref.MAX_GT)
        assert (slot >= 0).sum() == n_win and all(table[n, slot[n, j]] == j for n, j in zip(*np.nonzero(slot >= 0)))
    # hand-made: one winner at image 1, scale 1, cell 5, anchor 2; everything else is objectness
    table = np.full((2, R), -1, dtype=np.int32)
    row = 18 + 5 * 3 + 2
    table[1, row] = 3
    G = np.zeros((2, R, width), dtype=np.float32)
    G[..., 4] = 1
    G[1, row] = np.arange(1, width + 1)
    Xs = [np.arange(2 * h * w * 8).reshape(2 * h * w, 8) % 7 for h, w in grids]
    (dw0, db0), (dw1, db1), _ = ref.wgrad_exact(Xs, G, table, grids, A, ref.MAX_GT)
    assert not dw0[[0, 1, 2, 3, 5, 6, 7]].any() and np.array_equal(dw0[4], Xs[0].sum(axis=0)) and db0.tolist() == [0, 0, 0, 0, 12, 0, 0, 0] * 3
    x = Xs[1][24 + 5]
    assert np.array_equal(dw1[2 * width + 1], 2 * x) and np.array_equal(dw1[2 * width + 4], Xs[1].sum(axis=0) + 4 * x) and db1[2 * width + 7] == 8


def test_float64_loop_lowers_the_loss():
    import loss_v3_cases as cases
    from tensorflow_yolo_amd.net import evaluate as yeval
    grids, A, n_classes = [(2, 2), (4, 4)], 3, 2
    anchors = cases.anchors_for(grids, A)
    gt, counts = yeval.pack_gts([[(0.3, 0.4, 0.2, 0.5, 1)], [(0.6, 0.6, 0.1, 0.15, 0), (0.1, 0.9, 0.5, 0.8, 1)]], 2)
    rng = np.random.RandomState(0)
    Xs = [rng.randn(2 * h * w, 16) for h, w in grids]
    Ws, bs = [rng.randn(A * (5 + n_classes), 16) * 0.02 for _ in grids], [np.zeros(A * (5 + n_classes)) for _ in grids]
    losses, W2, b2 = ref.heads_train_loop64(Xs, Ws, bs, grids, anchors, n_classes, gt, counts, 1e-2, 5)
    assert all(b < a for a, b in zip(losses, losses[1:])) and all((w != w0).any() for w, w0 in zip(W2, Ws))
    # the first Adam step moves an element by lr |g| / (|g| + eps / sqrt(1 - beta2)): never more than lr, and lr for all but tiny gradients
    _, W1, _ = ref.heads_train_loop64(Xs, Ws, bs, grids, anchors, n_classes, gt, counts, 1e-2, 1)
    step = np.abs(W1[0] - Ws[0])
    assert (step <= 1e-2 * (1 + 1e-12)).all() and np.median(step[step > 0]) > 0.999e-2


# ---- host code under sanitizers -----------------------------------------------------------------------------------------------------------
def test_host_code_runs_clean_under_asan_and_ubsan(tmp_path):
    """train3_host.cpp (yolo_v3_head_wgrad_plan and every argument check in front of a launch) with train3_host_check.cpp, a program with
    its own main, built with -fsanitize=address,undefined and run on the CPU"""
    csrc = os.path.join(ROOT, "tensorflow-yolo_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc, "san-train3", "OBJDIR=" + str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "train3_host_check OK" in out.stdout

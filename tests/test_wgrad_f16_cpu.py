"""CPU: the host side of the 3 x 3 weight gradient on the fp16 matrix cores -- yolo_conv3x3_wgrad_f16_plan and the case table of
tests/wgrad_f16_ref.py against each other, every refusal that needs no device, the yardstick against itself, the [TRAIN] key `wgrad`,
the header's exports, and the float64 training loop with the narrowing beside the one without it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tail_cases
import tail_ref
import wgrad_f16_ref as ref
from helpers import ROOT
from tensorflow_yolo_amd import _hip, launcher
from tensorflow_yolo_amd.net import engine, synth, train as ytrain

V2_ANCHORS = [0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828]
ERR_ARG, ERR_STATE = 1, 5


def last_error():
    return _hip.lib().yolo_last_error().decode()


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def test_plan_fields_are_sane_and_monotone():
    for cout in (1, 30, 64, 65, 136, 1024):
        for cin in (8, 40, 64, 72, 136, 1280):
            last = None
            for h, w in ((1, 1), (1, 5), (5, 1), (3, 5), (13, 13), (19, 19), (5, 26), (2, 80), (1, ref.MAX_W), (76, 76)):
                for batch in (1, 2, 3, 16, 64):
                    pl, P = _hip.conv3x3_wgrad_f16_plan(h, w, batch, cin, cout), h * w * batch
                    assert (pl["tile_cout"], pl["tile_cin"], pl["tile_positions"]) == (64, 64, 64)
                    assert pl["tiles_cout"] == -(-cout // 64) and pl["tiles_cin"] == -(-cin // 64)
                    ppc, n = pl["positions_per_chunk"], pl["n_chunks"]
                    assert ppc >= 64 and ppc % 64 == 0 and n >= 1 and (n - 1) * ppc < P <= n * ppc and n <= 65535
                    assert pl["halo_rows"] == 64 + 2 * w + 2
                    # the 16-bit images (rows of 192 bytes), the pair masks and the position masks fit the 64 KiB a workgroup may ask for
                    assert (pl["halo_rows"] + 64) * 192 + 9 * 32 * 4 + 64 * 4 <= 65536
                    g, dbp = pl["db_groups"], pl["db_positions"]
                    assert 1 <= g <= 64 and dbp % 16 == 0 and (g - 1) * dbp < P <= g * dbp
                    slabs = n * cout * (9 * cin + 1) * 4
                    assert pl["record_offset"] % 256 == 0 and slabs <= pl["record_offset"] < slabs + 256
                    assert pl["scratch_bytes"] >= pl["record_offset"] + 8 + g * cout * 4 and pl["scratch_bytes"] % 256 == 0
                    # a larger batch of the same map: chunks and db groups never shrink (their counts may: the split is by the tile count);
                    # the scratch is NOT monotone in the batch, which is why yolo_net_train_wgrad_f16_bytes asks every batch up to max_batch
                    if last is not None and last[0] == (h, w):
                        assert ppc >= last[1] and dbp >= last[2]
                    last = ((h, w), ppc, dbp)


def test_plan_refusals_with_their_text():
    lib, pl = _hip.lib(), _hip.Conv3x3WgradF16Plan()
    call = lambda h, w, b, cin, cout, out=pl: lib.yolo_conv3x3_wgrad_f16_plan(h, w, b, cin, cout, C.byref(out) if out is not None else None)
    for args, text in (((0, 8, 1, 8, 1), "h, w and batch must be at least 1"), ((8, 0, 1, 8, 1), "h, w and batch must be at least 1"),
                       ((8, 8, 0, 8, 1), "h, w and batch must be at least 1"),
                       ((8, ref.MAX_W + 1, 1, 8, 1), "w must be at most %d: the halo of a wider map does not fit LDS" % ref.MAX_W),
                       ((1 << 24, 64, 2, 8, 1), "the number of positions must be 1 .. 2^30"), ((0x7fffffff, 80, 0x7fffffff, 8, 1), "2^30"),
                       ((13, 13, 2, 12, 1), "cin must be a positive multiple of 8"), ((13, 13, 2, 0, 1), "cin must be a positive multiple of 8"),
                       ((13, 13, 2, 8, 0), "cout must be at least 1"), ((13, 13, 2, 1 << 16, 1 << 16), "cout * (9 cin + 1) must fit 31 bits")):
        assert call(*args) == ERR_ARG and last_error() == "yolo_conv3x3_wgrad_f16_plan: " + text or text in last_error(), (args, last_error())
        assert last_error().startswith("yolo_conv3x3_wgrad_f16_plan: ")
    assert call(13, 13, 2, 8, 1, out=None) == ERR_ARG and "null argument" in last_error()
    assert call(8, ref.MAX_W, 1, 8, 1) == 0 and call(1 << 24, 64, 1, 8, 1) == 0
    assert ref.MAX_W >= 80


def test_gpu_cases_are_what_they_claim():
    """the GPU cases are derived from the plan here: a changed split fails on the CPU"""
    for h, w, batch, cin, cout in ref.WIDE_SHAPES:
        assert ref.boundary_inside_a_row(_hip.conv3x3_wgrad_f16_plan(h, w, batch, cin, cout), w), (h, w)
    assert {w for _, w, _, _, _ in ref.WIDE_SHAPES} == {26, 80, ref.MAX_W}
    assert {(h, w) for h, w, _, _, _ in ref.SHAPES} == {(1, 1), (1, 5), (5, 1), (3, 5), (13, 13)}
    assert {b for _, _, b, _, _ in ref.SHAPES} == {1, 2, 3}
    assert {8, 40, 136} < {c for _, _, _, c, _ in ref.SHAPES} and {1, 30, 72, 136} == {o for _, _, _, _, o in ref.SHAPES}
    counts = [h * w * b for h, w, b, _, _ in ref.SHAPES]
    assert any(P % 8 and P > 64 for P in counts) and any(P < 8 for P in counts)
    # several chunks at 13 x 13 x 136 -> 64, batch 2, one of them ending inside a row; the chunk-end shapes hold the chunk counts they name
    h, w, batch, cin, cout = ref.REAL_SHAPES[0]
    assert ref.boundary_inside_a_row(_hip.conv3x3_wgrad_f16_plan(h, w, batch, cin, cout), w)
    for cin, cout in ((8, 1), (136, 65)):
        plan = lambda h, w, b: _hip.conv3x3_wgrad_f16_plan(h, w, b, cin, cout)
        assert [plan(h, w, b)["n_chunks"] for h, w, b, _ in ref.plan_shapes(plan)] == [1, 1, 2, 3]


def test_net_mode_refusals_that_need_no_device():
    anchors = np.reshape(V2_ANCHORS, [-1, 2])
    lib = _hip.lib()
    net = tail_cases.small_tail_network(anchors, ["a", "b", "c"], False)
    p16 = engine.Plan(net, dtype="fp16", max_batch=2, streams=1)
    need = lib.yolo_net_train_wgrad_f16_bytes(p16.handle)
    cout3, cin3, _, _ = ytrain.tail_counts(net)
    assert need == max(_hip.conv3x3_wgrad_f16_plan(4, 4, b, cin3, cout3)["scratch_bytes"] for b in (1, 2)) > 0
    assert lib.yolo_net_train_set_wgrad_f16(p16.handle, 4096, need - 1) == ERR_ARG and "buffer too small (yolo_net_train_wgrad_f16_bytes)" in last_error()
    assert lib.yolo_net_train_set_wgrad_f16(p16.handle, 4096 + 128, need) == ERR_ARG and "256-byte aligned" in last_error()
    assert lib.yolo_net_train_set_wgrad_f16(p16.handle, 4096, need) == 0 and lib.yolo_net_train_set_wgrad_f16(p16.handle, None, 0) == 0
    assert lib.yolo_net_train_set_wgrad_f16(None, None, 0) == ERR_ARG
    p32 = engine.Plan(net, dtype="fp32", max_batch=2, streams=1)
    assert lib.yolo_net_train_wgrad_f16_bytes(p32.handle) == 0 and "a float32 plan stores float32 activations" in last_error()
    assert lib.yolo_net_train_set_wgrad_f16(p32.handle, 4096, 1 << 30) == ERR_STATE and last_error().startswith("yolo_net_train_set_wgrad_f16: a float32 plan")
    assert lib.yolo_net_train_set_wgrad_f16(p32.handle, None, 0) == 0            # switching back is always possible
    res = engine.Plan(tail_cases.small_tail_network(anchors, ["a", "b", "c"], False, residual=True), dtype="fp16", max_batch=2, streams=1)
    assert lib.yolo_net_train_wgrad_f16_bytes(res.handle) == 0 and "residual" in last_error()
    assert lib.yolo_net_train_set_wgrad_f16(res.handle, 4096, 1 << 30) == ERR_ARG and "residual" in last_error()


# ---- the yardstick against itself -----------------------------------------------------------------------------------------------------------
def test_k_follows_the_definition():
    f32 = lambda v: np.array([v], dtype=np.float32)
    assert ref.scale_k(0.0) == ref.scale_k(np.inf) == ref.scale_k(np.nan) == 0
    assert ref.k_of(f32(-0.0)) == ref.k_of(f32(-np.inf)) == ref.k_of(f32(np.nan)) == 0
    assert ref.k_of(np.array([1.0, np.nan, np.inf], dtype=np.float32)) == 0 and ref.max_bits(f32(np.nan)) > ref.max_bits(f32(np.inf))
    assert ref.scale_k(2.0 ** -149) == ref.scale_k(2.0 ** -127) == 126 and ref.scale_k(2.0 ** -113) == 126 and ref.scale_k(2.0 ** -112) == 126
    assert ref.scale_k(2.0 ** -111) == 125 and ref.scale_k(2.0 ** 127) == -113
    for e in (-111, -20, -1, 0, 1, 10, 100, 127):
        lo, hi = np.float32(2.0 ** e), np.float32(2.0 ** e * (2 - 2.0 ** -23))
        assert ref.scale_k(lo) == ref.scale_k(hi) == 14 - e == ref.k_of(f32(-hi))
        for m in (lo, hi):          # the largest scaled magnitude lies in [2^14, 2^15): no overflow
            assert 2.0 ** 14 <= float(m) * 2.0 ** ref.scale_k(m) < 2.0 ** 15 and np.isfinite(ref.narrow(f32(m), ref.scale_k(m))).all()


def test_narrowing_is_one_rounding_to_nearest_even():
    y = np.array([1025.5, 1026.5, 2049.0, 2051.0, 3 * 2.0 ** -25, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 5.5 * 2.0 ** -24, 1023.5 * 2.0 ** -24, 2.0 ** -26])
    want = np.array([1026.0, 1026.0, 2048.0, 2052.0, 2.0 ** -23, 0.0, 2.0 ** -24, 6 * 2.0 ** -24, 2.0 ** -14, 0.0])
    for k in (-20, 0, 11, 100):
        D = np.ldexp(y, -k).astype(np.float32)
        assert np.array_equal(np.ldexp(D.astype(np.float64), k), y)
        got = ref.narrow(D, k)
        assert got.dtype == np.float16 and np.array_equal(got.astype(np.float64), want) and np.array_equal(ref.narrow(-D, k).astype(np.float64), -want)
    assert np.isinf(ref.narrow(np.array([1e6], dtype=np.float32), 0)).all()             # (k = 0 because of an Inf or NaN elsewhere)


def test_narrowed_sums_of_integers_equal_the_integer_reference():
    rng = np.random.RandomState(2)
    B, h, w, cin, cout = 2, 3, 5, 8, 6
    X3 = rng.choice([-2048, 2048, 2047, -1025, 3, -1, 0], size=(B, h, w, cin)) // 4
    D = rng.choice([-2047, 2047, 1025, -3, 1, 0], size=(B * h * w, cout))
    scale = np.exp2(rng.randint(-3, 4, size=cout))
    want_w, want_b = ref.wgrad3x3_f16_exact(X3, D, scale)          # (asserts S |D| |X3| < 2^24)
    r = ref.sums64(X3, D.astype(np.float32), scale)
    assert r["k"] == 4 and np.array_equal(r["dW64"], want_w) and np.array_equal(r["dWexact"], want_w) and np.array_equal(r["db"], want_b)
    assert np.array_equal(np.ldexp(ref.narrow(D, 4).astype(np.float64), -4), D)
    for power in (-20, 10):
        rs = ref.sums64(X3, np.ldexp(D.astype(np.float32), power), scale)
        assert rs["k"] == 4 - power and np.array_equal(rs["dW64"], np.ldexp(want_w, power))
    # real values: the narrowed sums lie inside the second bound of the un-narrowed ones
    X, Dr = rng.randn(B, h, w, cin).astype(np.float16), rng.randn(B * h * w, cout).astype(np.float32)
    rr = ref.sums64(X, Dr, scale)
    assert np.all(np.abs(rr["dW64"] - rr["dWexact"]) <= rr["bound2"] - rr["bound1"])


# ---- the [TRAIN] key and the header ------------------------------------------------------------------------------------------------------------
def test_wgrad_key_accepted_refused_and_absent(tmp_path):
    assert ytrain.wgrad_option({}) is False and ytrain.wgrad_option({"wgrad": " FP32 "}) is False and ytrain.wgrad_option({"wgrad": "fp16"}) is True
    with pytest.raises(ValueError, match="^wgrad must be fp32 .* or fp16"):
        ytrain.wgrad_option({"wgrad": "bf16"})
    assert ytrain.check_params({"train_layers": "tail", "wgrad": "fp16", "dtype": "fp16"}, "v2") == 0.0
    assert ytrain.check_params({"train_layers": "head_blocks", "wgrad": "fp16", "dtype": "fp16"}, "v3-tiny") == 0.0
    assert ytrain.check_params({"train_layers": "tail", "wgrad": "fp32"}, "v2") == 0.0              # fp32 goes with any plan
    for layers, version in (("head", "v2"), ("heads", "v3")):
        with pytest.raises(ValueError, match="goes with train_layers = tail or head_blocks, not with train_layers = %s" % layers):
            ytrain.check_params({"train_layers": layers, "wgrad": "fp16", "dtype": "fp16"}, version)
    for params in ({"train_layers": "tail", "wgrad": "fp16"}, {"train_layers": "tail", "wgrad": "fp16", "dtype": "fp32"}):
        with pytest.raises(ValueError, match="needs dtype = fp16"):
            ytrain.check_params(params, "v2")
    ini = tmp_path / "cfg.ini"          # refused before a net is built: nothing else of the file is looked at
    ini.write_text("[COMMON]\nversion = v2\n[TRAIN]\ntrain_layers = head\nwgrad = fp16\ndtype = fp16\naugment_probability = 0\n")
    with pytest.raises(ValueError, match="no 3 x 3 block is trained"):
        launcher.run(launcher.read_config(str(ini)), "train")


@pytest.mark.parametrize("name, base, layers, version", [("yolo_2_tail_train_f16.ini", "yolo_2_tail_train.ini", "tail", "v2"),
                                                         ("yolo_3_head_blocks_train_f16.ini", "yolo_3_head_blocks_train.ini", "head_blocks", "v3")])
def test_shipped_configs_are_the_existing_ones_plus_the_key(name, base, layers, version):
    cfg_dir = os.path.join(ROOT, "tensorflow-yolo_amd", "config")
    cfg, old = launcher.read_config(os.path.join(cfg_dir, name)), launcher.read_config(os.path.join(cfg_dir, base))
    params = dict(cfg["TRAIN"])
    params.update(cfg["COMMON"])
    assert ytrain.wgrad_option(params) is True and ytrain.train_layers(params) == layers and params["version"] == version
    ytrain.check_params(params, version)
    for section in ("COMMON", "TRAIN", "TEST", "EVAL"):
        new = dict(cfg[section])
        assert new.pop("wgrad", None) == ("fp16" if section == "TRAIN" else None) and new == dict(old[section]), section
    assert ytrain.wgrad_option(dict(old["TRAIN"])) is False


def test_header_declares_what_the_library_exports():
    text = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    lib = _hip.lib()
    for name in ("yolo_conv3x3_wgrad_f16_plan", "yolo_conv3x3_wgrad_f16", "yolo_net_train_wgrad_f16_bytes", "yolo_net_train_set_wgrad_f16"):
        assert re.search(r"^(int|size_t) %s\(" % name, text, re.M), name
        assert name in _hip.SIGNATURES and getattr(lib, name) is not None
    assert "struct yolo_conv3x3_wgrad_f16_plan {" in text and "#define YOLO_HIP_ABI_VERSION 7 " in text
    assert C.sizeof(_hip.Conv3x3WgradF16Plan) == 10 * 4 + 2 * 8
    assert "(P + 4) 2^-24 |s32[o]| 2^-k S_p |D16| |X3|" in text and "2^-11 |D| + 2^-25 2^-k" in text          # both bounds stand in the header


# ---- the training loop with the narrowing --------------------------------------------------------------------------------------------------
def small_tail_setup(B=4, seed=44):
    """the net, weights and truths of the tail test's fixed batch (tests/test_gpu_train_tail.py) -> (net, weights, block, w0, b0, h, w, gt, counts)"""
    import loss_grad_cases
    anchors = np.reshape(V2_ANCHORS, [-1, 2])
    net = tail_cases.small_tail_network(anchors, ["tower"], False, input_shape=(64, 64, 3))
    weights = synth.darknet_stream(net, seed=41, num_classes=1, head_gain=synth.HEAD_DEFAULTS["v2-tiny"][0], obj_bias=0.0)
    cout3, cin3, _, _ = ytrain.tail_counts(net)
    block, w0, b0 = ytrain.split_tail(weights, net)
    h, w, _ = net[-1].out.hwc
    _, gt, counts = loss_grad_cases.random_case((h, w, 5, 1, B), 7)
    blk = (block[:cout3], block[cout3:2 * cout3], block[2 * cout3:3 * cout3], block[3 * cout3:4 * cout3], tail_ref.stream_to_otc(block[4 * cout3:], cout3, cin3))
    return net, weights, blk, w0, b0, h, w, gt, counts


def test_the_narrowed_float64_loop_descends_beside_the_plain_one():
    """Twenty steps of the float64 loop of tests/tail_ref.py with the narrowing and without it, on the net, weights and truths of the tail
    test's fixed batch; the block's input, which the device test reads from the device, is a stand-in of the same shape here (post-leaky
    normal variates in fp16).  Both lower the loss at every step at the tail test's rate, 1e-4 (narrowed_loops halves the rate until they
    do and reports it: asserted to be the first one).  d_narrow, their largest relative distance, is computed and printed, not fixed."""
    net, weights, blk, w0, b0, h, w, gt, counts = small_tail_setup()
    rng = np.random.RandomState(44)
    z = rng.randn(4, h, w, blk[4].shape[2])
    X3 = np.where(z > 0, z, 0.1 * z).astype(np.float16)
    rate, narrowed, plain, d_narrow = ref.narrowed_loops((X3, blk, w0, b0, h, w, V2_ANCHORS, 1, gt, counts, 20, np.float16), 1e-4)
    print("rate %g: d_narrow = %.3e; narrowed %.4f -> %.4f, plain %.4f -> %.4f" % (rate, d_narrow, narrowed[0], narrowed[-1], plain[0], plain[-1]))
    assert rate == 1e-4 and len(narrowed) == 20 and all(a > c for a, c in zip(narrowed, narrowed[1:])) and all(a > c for a, c in zip(plain, plain[1:]))
    assert narrowed[0] == plain[0] and 0 < d_narrow < 1         # the first loss is taken before any gradient; the narrowing then shows

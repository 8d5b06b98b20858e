"""CPU: the integer reference of the exact-arithmetic tests (tests/exact_ref.py) and the case table of test_gpu_exact.py.

- the reference EQUALS the pinned oracle (forward_ref.forward with and without fp16 storage) on integer data;
- the preconditions that make bit equality a theorem hold for EVERY case the GPU module parametrises, and the plan of every case
  names the kernel the case is about (planning needs no GPU);
- every conv tile id, and every conv / first / stem symbol of the YOLOv3-608 b32 plans, is covered by at least one case;
- three deliberate errors on the reference side (one product dropped at a border pixel, one tap of one row shifted by a column, the fp16
  rounding replaced by truncation) change the result; helpers.rel_err -- the metric of every other GPU test -- is printed beside the
  fp16 tolerance (the dropped product and the truncating store stay far below it: the gap these tests close).
"""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import test_gpu_exact as T
from helpers import rel_err, to_oracle
from oracle import cases as ocases, forward_ref as FR
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine, synth, v3


def _infos(p):
    out = []
    for k in range(p.num_kernels):
        ki = _hip.KernelInfo()
        _hip.check(p.lib.yolo_net_kernel_info(p.handle, k, C.byref(ki)), "yolo_net_kernel_info")
        out.append(ki)
    return out


ORACLE_CASES = ["conv-c64to128-fp16-tdef", "conv-c32to64_s2_odd-fp16-tdef", "conv-c256to512_linear_bias-fp16-tdef", "conv-first_3to32-fp16",
                "stem-3-32-64-32-1x18x34", "stem-3-32-64-2x21x30", "firstpool-20x44-16-fp16", "pool2d-32-fp16", "upsample-concat-fp16", "reorg-concat-fp16",
                "fallback-kernels-fp16", "maxpool-odd-fp16", "head255-fp16", "streams2-fp16", "mx-256to128-9x11-b3", "mx-epilogue-residual", "mx-epilogue-concat"]


@pytest.mark.parametrize("cid", ORACLE_CASES)
def test_reference_equals_the_oracle_on_integer_data(cid):
    """layer by layer: forward_exact(fp16) == forward_ref.forward(storage="fp16"), forward_exact(fp32) == forward_ref.forward"""
    c = T.CASES[T.IDS.index(cid)]
    for variant in c["variants"]:
        g = T.build_graph(c, variant)
        L = to_oracle(g)
        d = X.make_case(L, c["B"], seed=5, **c["data"])
        keep = set(range(len(L)))
        for dtype, storage in (("fp16", "fp16"), ("fp32", None)):
            want, wkept = FR.forward(L, d["stream"], d["x"], keep=keep, storage=storage)
            got, gkept = X.forward_exact(L, d, dtype, keep=keep)
            fused, _ = X.storage_rules(L)
            for i in sorted(keep - (fused if storage else set())):       # (the oracle keeps a fused conv unrounded: only the sum is stored)
                assert np.array_equal(gkept[i], wkept[i]), (cid, variant, dtype, i, L[i], int(np.count_nonzero(gkept[i] != wkept[i])))
            assert np.array_equal(got, want), (cid, variant, dtype)


def test_the_stream_is_what_the_engine_and_the_oracle_parse():
    g = T.g_residual_blocks()
    L = to_oracle(g)
    d = X.make_case(L, 2, seed=1)
    assert d["stream"].size == synth.darknet_stream(g, seed=0).size
    parsed = FR.parse_darknet_weights(L, d["stream"])
    for i, wd in d["weights"].items():
        for k, v in wd.items():
            assert np.array_equal(parsed[i][k], v), (i, k)
    assert engine.Plan(g, dtype="fp16", max_batch=2).weight_count == d["stream"].size


def test_the_fold_returns_every_integer():
    """gamma = 1, var = float32(1 - 1e-5): w * gamma / sqrt(var + 1e-5) in float64, rounded to float32 and to fp16, is w for |w| <= 2048"""
    w = np.arange(-2048, 2049, dtype=np.float32).reshape(-1, 1, 1, 1)
    wd = {"kernel_oihw": w, "gamma": np.ones(len(w), np.float32), "mean": np.zeros(len(w), np.float32), "var": np.full(len(w), X.BN_VAR, np.float32),
          "beta": np.zeros(len(w), np.float32)}
    f, b = X.folded(wd)
    assert not np.array_equal(f, w.astype(np.float64))            # the scale is NOT one: the rounding is what returns the integer
    assert np.array_equal(f.astype(np.float32), w) and np.array_equal(f.astype(np.float32).astype(np.float16).astype(np.float32), w) and not b.any()


def test_e4m3_holds_integers_up_to_14_at_every_block_scale():
    """a block whose largest magnitude is m (1..14) is scaled so that m lands in [256, 512) (clamped to 448): every integer up to 14 in it
    stays representable -- the torch restatement and the library's host quantizer both return the block unchanged"""
    rows = []
    for m in range(1, X.MX_MAX + 1):
        for sign in (1, -1):
            v = np.zeros(32, np.float32)
            v[:m + 1] = np.arange(m + 1) * sign
            v[m + 1:2 * m + 1] = -np.arange(1, m + 1) * sign
            rows.append(v)
    X._check_mx_identity(np.stack(rows))
    with pytest.raises(AssertionError):
        X._check_mx_identity(np.stack([np.r_[np.float32(15), np.float32(1), np.zeros(30, np.float32)]]))      # 15 x 32 = 480 > 448: saturates


@pytest.mark.parametrize("cid", T.IDS)
def test_preconditions_and_plan_of_every_gpu_case(cid):
    c = T.CASES[T.IDS.index(cid)]
    ties, neg = T.case_report(c)        # check_preconditions of every variant + the per-case ties / negative-branch requirement
    assert (ties > 0 or not c["ties"]) and (neg > 0 or not c["neg"])
    for variant in c["variants"]:
        p, names, text = T.plan_of(c, variant)
        T.check_kernels(c, variant, p, names, text)      # the same kernel assertions the GPU test makes on the engine that ran


def test_the_recorded_plans_cover_the_table():
    """every single-conv probe has its kernel recorded for every variant it runs; the split-K family holds each hand-over form, in both
    dtypes: the ticketed split inside the launch, splitk_reduce_kernel behind the tap tile and behind the 4-wave kernel, and the pair"""
    assert all(c["kernel"] is not None and set(c["variants"]) <= set(c["kernel"]) for c in T.CASES if c["graph"][0] == "g_probe")
    for dtype in ("fp16", "fp32"):
        names = [c["kernel"][v] for c in T.CASES if c["dtype"] == dtype and c["id"].split("-")[0] in ("splitk", "pairk") for v in c["variants"]]
        assert all(T._is_split(n) for n in names)
        assert any(",1launch" in n for n in names), dtype
        assert any("tap9" in n and "splitK" in n and ",1launch" not in n for n in names), dtype
        assert any(n.startswith("conv_igemm<") and "splitK" in n for n in names), dtype
        assert any("+pairK" in n for n in names), dtype
    # one fall-back case per forced tile at most, and every other forced case runs its tile
    fb = [(c["tile"], c["dtype"]) for c in T.CASES if c["fallback"]]
    assert len(fb) == len(set(fb))


def test_last_layer_shortcut_differs_from_the_oracle_by_one_rounding():
    """the reference of the "shortcut-last" cases (what the library writes: float32, unrounded) rounded to fp16 IS the oracle's value"""
    c = T.CASES[T.IDS.index("shortcut-last-2x19x19x128x128")]
    L, d, want, _, _ = T.reference(c, "res_last")
    oracle = FR.forward(L, d["stream"], d["x"], storage="fp16")
    assert np.array_equal(X.round_f16(want), oracle) and not np.array_equal(want, oracle)
    assert np.array_equal(X.forward_exact(L, d, "fp16"), oracle)


def _case_plans():
    for c in T.CASES:
        for variant in c["variants"]:
            yield c, T.plan_of(c, variant)[0]


def test_every_tile_and_every_yolov3_symbol_is_in_the_table():
    """every conv tile id 0-23 is forced AND runs in some fp16 case, the float32 tiles in some fp32 case; and every distinct conv / first /
    stem kernel symbol of the YOLOv3-608 batch-32 fp16, fp32 and mxfp8 plans runs in at least one exact case"""
    ran, syms = set(), set()
    for c, p in _case_plans():
        for ki in _infos(p):
            syms.add(ki.symbol.decode())
            if (T.is_forced(c) or c["id"].startswith("fuse2")) and T.TILE_NAME[c["tile"]] in ki.name.decode():
                ran.add((c["dtype"], c["tile"]))
    assert {t for d, t in ran if d == "fp16"} == set(range(24)), sorted(ran)
    assert {t for d, t in ran if d == "fp32"} == set(T.F32_TILES), sorted(ran)
    names = ["c%d" % i for i in range(80)]
    missing = {}
    for dtype in ("fp16", "fp32", "mxfp8"):
        net = v3.create_network(np.reshape(ocases.COCO_V3_ANCHORS, [-1, 2]), names, False, input_shape=(608, 608, 3))
        for ki in _infos(engine.Plan(net, dtype=dtype, max_batch=32)):
            s = ki.symbol.decode()
            if s and ki.name.decode().startswith("conv") and s not in syms:
                missing.setdefault(s, ki.name.decode())
    assert not missing, "YOLOv3-608 b32 kernels no exact case runs:\n" + "\n".join("%s  %s" % (n, s) for s, n in sorted(missing.items()))


# ---- mutations: what equality catches and rel_err does not ---------------------------------------------------------------------
def _mutation_case():
    """3x3 conv, 1024 input channels (K = 9216: the deepest 3x3 convs of the networks), on a 13 x 13 map, read through an fp16 store"""
    g = T.g_probe(13, 13, 1024, 64, 3, 1, True, "leaky", "pool")
    L = to_oracle(g)
    d = X.make_case(L, 1, seed=77)
    X.check_preconditions(L, d, "fp16", want_ties=True, want_neg=True)
    return L, d, X.forward_exact(L, d, "fp16", keep={1})[1][1]


FP16_TOL = 2.5e-3           # test_gpu_ops.TOL["fp16"]: what the same error is measured against today


def test_mutation_one_product_dropped_at_a_border_pixel():
    L, d, want = _mutation_case()
    w = d["weights"][1]["kernel_oihw"]
    co, (dy, dx) = 5, (1, 1)
    prod = np.abs(w[co, :, dy, dx] * d["x"][0, 0, 12, :])
    ci = int(np.argmin(np.where(prod > 0, prod, np.inf)))         # the smallest product that is not zero
    assert prod[ci] > 0
    got = X.forward_exact(L, d, "fp16", keep={1}, mutate=("drop", 1, (0, 0, 12, co), (dy, dx, ci)))[1][1]
    print("one product dropped: rel_err %.2e (tolerance %.1e), %d element(s) differ" % (rel_err(got, want), FP16_TOL, np.count_nonzero(got != want)))
    assert not np.array_equal(got, want)


def test_mutation_one_tap_shifted_by_a_column_in_one_row():
    L, d, want = _mutation_case()
    got = X.forward_exact(L, d, "fp16", keep={1}, mutate=("shift", 1, (0, 6), (0, 2)))[1][1]
    print("one tap of one row shifted: rel_err %.2e (tolerance %.1e), %d elements differ" % (rel_err(got, want), FP16_TOL, np.count_nonzero(got != want)))
    assert not np.array_equal(got, want)
    assert np.array_equal(np.delete(got, 6, axis=1), np.delete(want, 6, axis=1))          # (confined to that row)


def test_mutation_fp16_store_truncates():
    L, d, want = _mutation_case()
    got = X.forward_exact(L, d, "fp16", keep={1}, mutate=("trunc", 1))[1][1]
    print("fp16 store truncates: rel_err %.2e (tolerance %.1e), %d elements differ" % (rel_err(got, want), FP16_TOL, np.count_nonzero(got != want)))
    assert not np.array_equal(got, want)

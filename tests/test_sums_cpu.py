"""CPU: the reference, the yardstick and the case table of the real-valued sum tests (tests/sum_ref.py, test_gpu_sums.py).

- the float64 reference IS the oracle's conv on the same operands (forward_ref._conv in float64 to 1e-12 of S_e; forward_ref.forward
  returns float32, so its result is the reference rounded once);
- the interval check accepts the correctly rounded reference everywhere;
- the yardstick has teeth: on a case's own products two correct accumulation orders pass both checks, and precision faults that
  helpers.rel_err lets through at test_gpu_ops.TOL fail them;
- the preconditions, the planned kernel and the committed yardstick hold for every GPU case; every tile id and split-K form is in the table.
"""
import numpy as np
import pytest
import torch

import exact_ref as X
import sum_ref as R
import test_gpu_exact as T
import test_gpu_ops
from helpers import rel_err, to_oracle
from oracle import forward_ref as FR


def _case(cid):
    return R.CASES[R.IDS.index(cid)]


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,variant", [("tap-2x21x70x32x32-fp32-t17", "f32"), ("s2-1x34x34x128x320-fp16-t20", "f32"), ("head255-fp32", "f32"),
                                         ("dma-c768_1x1-fp16-t1", "res")])
def test_reference_equals_the_oracle(cid, variant):
    """the oracle's conv operator in float64 on the operands as stored (identity BN: gamma 1, mean 0, var + eps = 1; leaky applied here with
    the float32 slope the kernels use -- the oracle's float64 pass multiplies by the double 0.1, 1.5e-9 away) against act64, to 1e-12 of
    S_e per element; and forward_ref.forward(dtype=float64) of the whole graph, which returns float32: act64 rounded once (+ that slope)"""
    c = _case(cid)
    for ds in R.DATASETS:
        ref = R.reference(c, variant, ds)
        d = ref["data"]
        L = to_oracle(R.build_graph(c, variant))
        wd = dict(d["weights"])
        if "var" in wd:
            wd["var"] = np.full(wd["var"].shape, 1.0 - FR._BN_EPS, np.float64)
        _, src, f, k, s, bn, act = L[1]
        x = torch.from_numpy(np.array(d["x"])).permute(0, 3, 1, 2).contiguous().to(torch.float64)
        y = R.act64(FR._conv(x, wd, k, s, bn, "linear", torch.float64).permute(0, 2, 3, 1).numpy(), act == "leaky")
        if variant == "res":
            y = y + d["x"].astype(np.float64)
        assert np.all(np.abs(y - ref["act"]) <= 1e-12 * ref["S"]), (cid, ds, float(np.max(np.abs(y - ref["act"]) / ref["S"])))
        out = FR.forward(L, {1: wd}, np.array(d["x"]), dtype=torch.float64)
        want = R.pooled(variant, ref["act"])
        assert np.all(np.abs(out - want) <= 2.0 ** -24 * np.abs(want) + 2e-9 * R.pooled(variant, ref["S"])), (cid, ds)


@pytest.mark.parametrize("cid", ["tap-2x21x70x32x32-fp16-t17", "dma-c768_1x1-fp16-t1", "firstpool-signed-16-fp16", "mx-1024to192-7x5-b2", "pool2d-signed-32-fp32"])
def test_interval_accepts_the_rounded_reference(cid):
    """round_f16(act64) (fp32 plans: act64 as float32) read the way the graph reads it lies inside every interval; a store that truncates
    to fp16 does not: on more than 20 % of the elements of an fp16 plan"""
    c = _case(cid)
    for variant in c["variants"]:
        if not R.is_store(c, variant):
            continue
        for ds in R.DATASETS:
            ref = R.reference(c, variant, ds)
            a32 = ref["act"].astype(np.float32)
            good = R.pooled(variant, R._f16_round(ref["act"]) if c["dtype"] != "fp32" else a32.astype(np.float64))
            res = R.check_store(c, variant, good, ref)
            assert res["ok"], (cid, variant, ds, res)
            if c["dtype"] != "fp32":        # (mxfp8: the MX yardstick is as wide as an fp16 ulp -- a truncating store leaves it on a few elements only)
                res = R.check_store(c, variant, R.pooled(variant, X.trunc_f16(a32).astype(np.float64)), ref)
                share = 0.2 if c["dtype"] == "fp16" else 0.0
                assert not res["ok"] and res["out"] > share * ref["act"].size / (4 if variant == "pool2" else 1), (cid, variant, ds, res["out"])


# ---- the yardstick has teeth ------------------------------------------------------------------------------------------------------
TEETH_FP16 = "splitk-13-512to1024-b1-fp16"          # K = 4608, fp16 operands: products exact in float32
TEETH_FP32 = "splitk-13-512to1024-b1-fp32"          # the same shape on general float32 operands
TEETH_EMU_SHORT = "emu-13-32to512-1x1-mode2"        # K = 32
ROWS = np.arange(5, 169, 11)                        # 15 of the 169 positions, all 1024 couts: every weight scale


def _teeth(cid, ds):
    c = _case(cid)
    ref = R.reference(c, "f32", ds)
    o = R.operands(c, R.spec_of(c, "f32"), ref["data"])
    sub = dict(act=ref["act"].reshape(-1, ref["act"].shape[-1])[ROWS], S=ref["S"].reshape(-1, ref["S"].shape[-1])[ROWS], r_seq=ref["r_seq"])
    return c, o, sub


def _figures(c, o, sub, mode):
    v = R.simulate(o, mode, ROWS)
    res = R.check_f32(v, sub, R.n_ops(c, "conv_igemm_emu" if mode.startswith("emu") else ""))
    res["rel_err"] = rel_err(v, sub["act"])
    return res


@pytest.mark.parametrize("cid", [TEETH_FP16, TEETH_FP32])
@pytest.mark.parametrize("ds", R.DATASETS)
def test_yardstick_has_teeth(cid, ds):
    """on the case's own products: 32-wide blocks then a chain, and two levels every 288 k, pass both checks; 288-k partials rounded through
    fp16, truncating adds and one dropped product fail check 2 -- the first two, on the fp16 plan's operands, WHILE they pass the max-norm
    tolerance the operator tests apply to that plan (test_gpu_ops.TOL["fp16"]; they sit at 0.9e-4 ... 2.0e-4 of the maximum), which is
    the gap these tests close.  On the float32 plan's operands they are at 0.5e-4 ... 1.7e-4, on either side of its 1e-4: printed only"""
    c, o, sub = _teeth(cid, ds)
    tol = test_gpu_ops.TOL[c["dtype"]]
    for mode in ("blocks32", "two_level"):
        res = _figures(c, o, sub, mode)
        print("%s %s %-12s R %.2f x 2^-24 = %.3f x R_seq, rel_err %.2e" % (cid, ds, mode, res["R_dev"] / R.U24, res["ratio"], res["rel_err"]))
        assert res["bound_ok"] and res["yard_ok"], (mode, res)
    for mode in ("partials_f16", "trunc", "drop"):
        res = _figures(c, o, sub, mode)
        print("%s %s %-12s R %.2f x 2^-24 = %.3f x R_seq, rel_err %.2e (tolerance %.1e)" % (cid, ds, mode, res["R_dev"] / R.U24, res["ratio"], res["rel_err"], tol))
        assert not res["yard_ok"], (mode, res)
        if mode != "drop" and c["dtype"] == "fp16":
            assert res["rel_err"] <= tol, (mode, res["rel_err"], tol)


@pytest.mark.parametrize("ds", R.DATASETS)
def test_yardstick_has_teeth_for_the_emulation(ds):
    """float32 operands as three bf16 terms each (conv.hip's split), the nine partial products added to ONE float32 chain: passes both
    checks at K = 4608 and at K = 32.  Without the middle x middle term check 2 fails at K = 32, the shortest K the emulation runs at
    (8 - 11 x R_seq), WHILE it passes the max-norm tolerance.  At K = 4608 it does not fail (printed: 0.9 x R_seq signed, 1.2 x same-sign,
    the same figures as with the term): the lost term is at most 2^-18 |w x| with a random sign, and in a long sum that is less than a
    sequential float32 chain loses -- why the case table holds the emulation at K = 32 as well"""
    for cid in (TEETH_FP32, TEETH_EMU_SHORT):
        c, o, sub = _teeth(cid, ds)
        res = _figures(c, o, sub, "emu")
        print("%s %s emu          R %.2f x 2^-24 = %.3f x R_seq" % (cid, ds, res["R_dev"] / R.U24, res["ratio"]))
        assert res["bound_ok"] and res["yard_ok"], res
        res = _figures(c, o, sub, "emu_no_mid")
        print("%s %s emu_no_mid   R %.2f x 2^-24 = %.3f x R_seq, rel_err %.2e (tolerance %.1e)" % (cid, ds, res["R_dev"] / R.U24, res["ratio"], res["rel_err"],
                                                                                                    test_gpu_ops.TOL["fp32"]))
        if cid == TEETH_EMU_SHORT:
            assert not res["yard_ok"] and res["rel_err"] <= test_gpu_ops.TOL["fp32"], res


# ---- the table ----------------------------------------------------------------------------------------------------------------
SHORT_K = [c["id"] for c in R.CASES if R._macs(c) < 20e6]


@pytest.mark.parametrize("cid", SHORT_K)
def test_committed_yardstick_is_what_the_restatement_gives(cid):
    """the short cases recomputed (seed and R_seq): equality with tests/golden/sum_yardstick.json"""
    c = _case(cid)
    for variant in c["variants"]:
        for ds in R.DATASETS:
            key = R.data_key(c, variant, ds)
            assert R.yardstick()["entries"][R.entry_key(c, variant, ds)] == key
            k, e = R.compute_entry((key, cid, "res" if variant == "res" else "f32", ds))
            assert e == R.yardstick()["data"][key], (cid, variant, ds, e, R.yardstick()["data"][key])


def test_yardstick_covers_the_table():
    data, entries = R.all_entries()
    assert set(R.yardstick()["data"]) == set(data) and R.yardstick()["entries"] == entries
    assert all(e["r_seq"] >= R.R_SEQ_MIN for e in R.yardstick()["data"].values())


@pytest.mark.parametrize("cid", R.IDS)
def test_preconditions_and_plan_of_every_gpu_case(cid):
    """range, subnormal cap, yardstick floor and BN fold identity of every variant and data set; the plan runs the kernel its recorded name says"""
    c = _case(cid)
    for variant in c["variants"]:
        for ds in R.DATASETS:
            frac, top = R.preconditions(c, variant, ds)
            ref = R.reference(c, variant, ds)
            assert np.log10(ref["S"].max() / ref["S"].min()) > 4, (cid, variant, ds)        # S_e spans more than four decades inside the tensor
            if ds == "same":          # no cancellation: |sum + b| = S_e in front of leaky and the residual
                o = R.operands(c, R.spec_of(c, variant), ref["data"])
                assert np.all(o["cols"] >= 0) and np.all((o["w"] >= 0) == (np.arange(o["w"].shape[1]) % 2 == 0)[None, :] | (o["w"] == 0))
                assert np.all((o["b"] > 0) == (np.arange(o["b"].size) % 2 == 0))
        p, names, text = T.plan_of(c, None if c["graph"][0] == "g_mx" else variant)
        T.check_kernels(R.recorded(c, variant), None if c["graph"][0] == "g_mx" else variant, p, names, text)


def test_every_tile_and_every_split_form_is_in_the_table():
    names = {}
    for c in R.CASES:
        for variant in c["variants"]:
            rec = R.recorded(c, variant)["kernel"]
            name = rec[variant] if rec else " ".join(n for n in T.plan_of(c, None if c["graph"][0] == "g_mx" else variant)[1] if n.startswith("conv"))
            names.setdefault(c["dtype"], set()).add(name)
    for t, s in T.TILE_NAME.items():
        assert any(s in n for n in names["fp16"]), (t, s)
        if t in T.F32_TILES:
            assert any(s in n and "f32" in n for n in names["fp32"]), (t, s)
    every = set().union(*names.values())
    for form in (",1launch", "+splitK", "+pairK", "conv_igemm_emu", "conv_mx"):
        assert any(form in n for n in every), form
    assert any("+splitK" in n and ",1launch" not in n and "tap9" in n for n in every) and any(n.startswith("conv_igemm<") and "+splitK" in n for n in every)


@pytest.mark.parametrize("ds", R.DATASETS)
def test_back_to_back_1x1_preconditions_and_plan(ds):
    """both convs of the "+1x1" cases: range, subnormal cap, yardstick floor (the 1x1's on the host's rounding of the first conv's tensor; the
    GPU test asserts them again on the device's values), the correctly rounded values inside their intervals, a truncating store outside;
    and the fusion plans on both tiles"""
    d = R.fuse2_data(ds)
    ref2 = R.fuse2_second(d["host_x2"], d)
    for ref in (d["ref1"], ref2):
        res = R.check_plain_store(R._f16_round(ref["act"]), ref)
        assert res["ok"] and res["top"] < 65504 and res["frac"] <= R.SUBNORMAL_CAP and ref["r_seq"] >= R.R_SEQ_MIN, res
        assert np.log10(ref["S"].max() / ref["S"].min()) > 4
        assert not R.check_plain_store(X.trunc_f16(ref["act"].astype(np.float32)), ref)["ok"]
    assert d["w2"].any(axis=0).all()
    for name in R.FUSE2:
        c = T.CASES[T.IDS.index("fuse2-" + name)]
        p, names, text = T.plan_of(c, None)
        T.check_kernels(c, None, p, names, text)
        assert "+1x1" in text and c["tile"] == R.FUSE2[name]

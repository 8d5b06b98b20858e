"""GPU: real-valued sums of every conv kernel, element by element (tests/sum_ref.py; DESIGN.md section 5, "Sums of real values").

The single-conv probes of test_gpu_exact.py -- same graphs, same forced tiles, the same assertion that the kernel meant is the one that
ran -- on two seeded real-valued data sets ("signed": per-element sum|w x| spans more than four decades inside one tensor; "same": no
cancellation, so a systematic error adds up).  Every element is compared with a float64 sum over the operands as stored, in units of its
OWN S_e = sum|w x| + |b| (+ |r|):

  float32 read ("f32"):  1. |dev - act64| <= (n_ops + 4) 2^-24 S_e for every element (worst case of round-to-nearest float32 operations in
                            any order; n_ops = K, 2 K native float32, 9 K the bf16 emulation);
                         2. R_dev = max_e |dev - act64| / S_e <= 4 R_seq, R_seq the same statistic of a strictly sequential float32
                            chain on the same data (tests/golden/sum_yardstick.json);
  stored ("pool", "res", "pool2"):  the element lies in [round_f16(act64 - E_e), round_f16(act64 + E_e)], E_e = 4 R_seq S_e, both ends read
                            through the same max-pool (fp32 plans: the same interval without the rounding).

mxfp8 plans: the yardstick's step is one scaled MFMA as sum_ref.mx_dot restates it (the instruction drops low product bits).
test_back_to_back_1x1: the "+1x1" fusion, the 1x1 against a float64 sum over the device's own values of the 3x3's tensor.
Every case prints its kernel name and, per float32 read, R_dev in units of 2^-24 and R_dev / R_seq.  The margins are fixed and are
not to be raised to make a kernel pass: a kernel above them is a finding.  Preconditions (sum_ref.preconditions) are asserted for a case
before anything touches the GPU.
"""
import numpy as np
import pytest

import sum_ref as R
import test_gpu_exact as T
from helpers import layer_tensor, run_hip

pytestmark = pytest.mark.gpu


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("cid", R.IDS)
def test_sums(cid):
    c = R.CASES[R.IDS.index(cid)]
    for variant in c["variants"]:
        for ds in R.DATASETS:
            R.preconditions(c, variant, ds)             # reference and data only: before anything touches the GPU
    failures = []
    for variant in c["variants"]:
        gv = None if c["graph"][0] == "g_mx" else variant
        for ds in R.DATASETS:
            ref = R.reference(c, variant, ds)
            d = ref["data"]
            got, eng = run_hip(R.build_graph(c, variant), d["stream"], d["x"], c["dtype"], force_tile=c["tile"], **c["kw"])
            infos = eng.kernel_infos()
            names, text = T.kernel_text(eng, infos)
            T.check_kernels(R.recorded(c, variant), gv, eng, names, text)
            name, symbol = [(ki.name.decode(), ki.symbol.decode()) for ki in infos if ki.name.decode().startswith("conv")][0]
            what = "%s/%s/%s %s [%s]" % (cid, variant, ds, name, symbol)
            assert np.all(np.isfinite(got)), what
            if R.is_store(c, variant):
                res = R.check_store(c, variant, got, ref)
                print("%s: every stored element inside its interval: %s" % (what, "yes" if res["ok"] else "NO (%d outside)" % res["out"]))
                if not res["ok"]:
                    failures.append("%s: %d of %d elements outside [round(act64 - E), round(act64 + E)]; worst %s: interval [%r, %r]; its window's first "
                                    "conv element %s" % (what, res["out"], got.size, res["worst"], res["lo"], res["hi"], R.describe_worst(c, variant, ref, got, res["worst"])))
            else:
                nops = R.n_ops(c, name)
                res = R.check_f32(got, ref, nops)
                print("%s: R_dev %.3f x 2^-24, R_seq %.3f x 2^-24, R_dev / R_seq %.3f (n_ops %d)" % (what, res["R_dev"] / R.U24, ref["r_seq"] / R.U24, res["ratio"], nops))
                if not res["bound_ok"]:
                    failures.append("%s: an element is beyond (n_ops + 4) 2^-24 S_e, n_ops = %d: %s" % (what, nops, R.describe_worst(c, variant, ref, got, res["worst"])))
                if not res["yard_ok"]:
                    failures.append("%s: R_dev = %.3f x R_seq > %g x R_seq: %s" % (what, res["ratio"], R.FACTOR, R.describe_worst(c, variant, ref, got, res["worst"])))
            if c["repeat"]:         # split-K / pair-K: a second launch gives the same bytes
                again = eng.forward(d["x"]).cpu().numpy()
                if not _same_bytes(again, got):
                    failures.append("%s: the second launch differs in %d elements" % (what, int(np.count_nonzero(again != got))))
            del eng
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("ds", R.DATASETS)
@pytest.mark.parametrize("name", sorted(R.FUSE2))
def test_back_to_back_1x1(name, ds):
    """the "+1x1" fusion: the 3x3 / 2 conv's tensor as one more stored probe, and the 1x1 the same launch computes against a float64 sum
    over the DEVICE's own fp16 values of that tensor (its yardstick computed on those values: K = 128)"""
    c = T.CASES[T.IDS.index("fuse2-" + name)]
    d = R.fuse2_data(ds)
    pre = R.check_plain_store(R._f16_round(d["ref1"]["act"]), d["ref1"])               # before anything touches the GPU
    assert pre["ok"] and pre["top"] < 65504 and pre["frac"] <= R.SUBNORMAL_CAP and d["ref1"]["r_seq"] >= R.R_SEQ_MIN, pre
    got, eng = run_hip(T.build_graph(c, None), d["stream"], d["x"], "fp16", force_tile=c["tile"])
    names, text = T.kernel_text(eng, eng.kernel_infos())
    T.check_kernels(c, None, eng, names, text)
    assert "+1x1" in text and np.all(np.isfinite(got))
    t1 = layer_tensor(eng, 1, c["B"])[0].float().cpu().numpy()
    t2 = layer_tensor(eng, 2, c["B"])[0].float().cpu().numpy()
    what = "fuse2-%s/%s %s" % (name, ds, names[1])
    res1 = R.check_plain_store(t1, d["ref1"])
    ref2 = R.fuse2_second(t1.reshape(-1, t1.shape[-1]), d)
    res2 = R.check_plain_store(t2.reshape(ref2["act"].shape), ref2)
    print("%s: 3x3 inside its intervals: %s (R_seq %.2f x 2^-24); 1x1 on the device's values: %s (R_seq %.2f x 2^-24, %.2e of the outputs subnormal, largest %.0f)"
          % (what, "yes" if res1["ok"] else "NO", d["ref1"]["r_seq"] / R.U24, "yes" if res2["ok"] else "NO", ref2["r_seq"] / R.U24, res2["frac"], res2["top"]))
    assert res2["top"] < 65504 and res2["frac"] <= R.SUBNORMAL_CAP and ref2["r_seq"] >= R.R_SEQ_MIN, (what, res2)
    assert res1["ok"], "%s: the 3x3: %d elements outside their interval; worst (image, y, x, cout) = %s: dev %r, interval [%r, %r]" % (
        what, res1["out"], res1["worst"], res1["dev"], res1["lo"], res1["hi"])
    M = np.unravel_index(res2["worst"][0], t2.shape[:3])
    assert res2["ok"], "%s: the 1x1: %d elements outside their interval; worst (image, y, x, cout) = %s: dev %r, interval [%r, %r], act64 %r S_e %r" % (
        what, res2["out"], tuple(int(v) for v in M) + (res2["worst"][1],), res2["dev"], res2["lo"], res2["hi"], float(ref2["act"][res2["worst"]]),
        float(ref2["S"][res2["worst"]]))

"""No GPU: what tests/test_gpu_poison.py rests on.  The two poison patterns decode as claimed; every whole-network plan of
tests/poison_cases.py still has the features it is in the table for (a later planner change must fail here, not quietly turn the GPU
tests into tests of something else); part a covers every exact case because it is parametrised by the same list object."""
import ctypes as C

import numpy as np
import pytest

import poison_cases as P
import test_gpu_exact as E
import test_gpu_poison as G
from tensorflow_yolo_amd import _hip


# ---- the patterns (what helpers.poison_fill writes, restated with NumPy views) ----------------------------------------------------------
def test_ones_is_nan_in_every_float_format_and_minus_one_as_an_integer():
    raw = np.full(64, 0xFF, dtype=np.uint8)
    for dt in (np.float16, np.float32, np.float64):
        assert np.isnan(raw.view(dt)).all(), dt
    assert (raw.view(np.int32) == -1).all() and (raw.view(np.uint32) == 4294967295).all()
    assert (raw.view(np.int16) == -1).all() and (raw.view(np.int64) == -1).all()


def test_inf_is_plus_infinity_of_the_storage_type():
    h = np.full(32, 0x7C00, dtype=np.uint16)            # fp16 and mxfp8 plans: per 16 bits
    assert (h.view(np.float16) == np.inf).all()
    f = np.full(16, 0x7F800000, dtype=np.uint32)        # fp32 plans: per 32 bits
    assert (f.view(np.float32) == np.inf).all()
    # the fp16 form where an fp16 plan keeps float32 (head logits, objectness, split-K slabs): finite, and wrong wherever it is used
    as_f32 = h.view(np.float32)
    assert np.isfinite(as_f32).all() and np.all(as_f32 == np.float32(2.0) ** 121 * np.float32(1 + 0x7C00 / 2.0 ** 23))
    assert 2.66e36 <= float(as_f32[0]) < 2.67e36                # 2.6685e36, "2.66e36" to the digits written
    assert (h.view(np.int32) == 0x7C007C00).all()       # ... and as an integer: far above any count or capacity


def test_the_harness_writes_these_patterns():
    """helpers.poison_fill on the CPU (torch tensors of bytes, as the engine's buffers are)"""
    import torch
    from helpers import poison_fill
    t = torch.zeros(64, dtype=torch.uint8)
    poison_fill(t, "ones", False)
    assert (t.numpy() == 0xFF).all()
    poison_fill(t, "inf", False)
    assert (t.numpy().view(np.float16) == np.inf).all()
    poison_fill(t, "inf", True)
    assert (t.numpy().view(np.float32) == np.inf).all()
    with pytest.raises(ValueError):
        poison_fill(t, "zeros", False)


# ---- the table of whole plans ------------------------------------------------------------------------------------------------------------
def plan_text(pid):
    p = P.plan_only(pid)
    names, text = E.kernel_text(p, [E._info(p, k, C, _hip) for k in range(p.num_kernels)])
    return p, names, text


def test_the_table_is_what_the_issue_asks_for():
    nets = {(p["net"], p["dtype"], p["keep_all"]) for p in P.PLANS.values() if p["kw"]["streams"] == 1}
    for net in P.NETS:
        for dt in ("fp16", "fp32"):
            assert (net, dt, True) in nets and (net, dt, False) in nets, (net, dt)
    assert ("v3", "mxfp8", False) in nets and ("v3", "mxfp8", True) in nets
    assert {n: P.NETS[n][3] for n in P.NETS} == {"v2": (160, 160), "v2-tiny": (160, 160), "v3": (160, 160), "v3-spp": (96, 160), "v3-tiny": (96, 160)}
    for pid, p in P.PLANS.items():
        if p["kw"]["streams"] == 1:
            assert p["kw"]["max_batch"] == 3 and p["batches"] == (3, 2), pid
    s2 = P.PLANS["v3-fp16-plan-streams2"]
    assert s2["kw"] == {"streams": 2, "max_batch": 6} and s2["batches"] == (5,) and not s2["keep_all"]
    assert set(P.FEATURES) <= set(P.PLANS)


@pytest.mark.parametrize("pid", sorted(P.PLANS))
def test_plan_has_the_features_it_is_in_the_table_for(pid):
    p, names, text = plan_text(pid)
    assert p.num_streams == P.PLANS[pid]["kw"]["streams"], (pid, p.num_streams)
    for s in P.FEATURES.get(pid, ()):
        assert s in text, (pid, s, sorted(set(names)))
    if P.PLANS[pid]["dtype"] == "mxfp8":
        assert any(n.startswith("conv_mx") for n in names), names
    if not P.PLANS[pid]["keep_all"]:        # the production plan packs lifetimes: its workspace is smaller than keep_all's
        keep = P.plan_only(pid.replace("-plan", "-keep_all").replace("-streams2", ""))
        assert p.workspace_bytes / P.PLANS[pid]["kw"]["streams"] < keep.workspace_bytes, pid


def test_named_features():
    """the five the table must never lose, by name"""
    assert "conv_stem<" in plan_text("v3-fp16-plan")[2]                                # the stem in YOLOv3
    assert "conv_first_pool" in plan_text("v2-tiny-fp16-plan")[2]                       # the pool-fused first conv in tiny-YOLOv2
    assert "spp_pool_kernel" in plan_text("v3-spp-fp16-plan")[2]                        # the SPP kernel
    assert plan_text("v3-fp16-plan-streams2")[0].num_streams == 2                       # two parts
    assert sum(n.startswith("conv_mx") for n in plan_text("v3-mxfp8-plan")[1]) >= 1     # at least one MX conv


# ---- part a covers every exact case ------------------------------------------------------------------------------------------------------
def test_part_a_is_parametrised_by_the_exact_list_itself():
    marks = [m for m in G.test_exact_on_a_poisoned_workspace.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "cid"
    assert marks[0].args[1] is E.IDS, "a copy of the list: a case added to test_gpu_exact.py would not be run on a poisoned workspace"
    exact = [m for m in E.test_exact.pytestmark if m.name == "parametrize"]
    assert exact[0].args[1] is E.IDS and len(E.IDS) == len(E.CASES) == len(set(E.IDS))
    assert G.KEEP_ALL_IDS and {E.CASES[E.IDS.index(i)]["dtype"] for i in G.KEEP_ALL_IDS} == {"fp16", "fp32"}


def test_the_mutation_case_has_an_image_to_leave_out():
    c = E.CASES[E.IDS.index("fallback-kernels-fp16")]
    assert c["B"] > 1 and c["keep_all"]

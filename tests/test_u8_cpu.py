"""CPU: the uint8 input path (ABI 7) as far as it exists without a GPU -- the five exports and their ctypes signatures, the argument
checks of the device-free half, the byte -> float32 conversion table, the engine's input validation, and the register budget of the
uint8 kernel twins against their float32 forms."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import ROOT, new_graph
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine, layers as PL

U8_ENTRIES = {
    "yolo_net_forward_u8": "yolo_net_forward",
    "yolo_net_detect_u8": "yolo_net_detect",
    "yolo_net_forward_timed_u8": "yolo_net_forward_timed",
    "yolo_net_tune_streams_u8": "yolo_net_tune_streams",
    "yolo_preprocess_resize_u8": "yolo_preprocess_resize",
}


def test_u8_exports_and_signatures():
    """every uint8 entry is exported, declared in the header, and has the ctypes signature of its float32 twin (the input / output
    pointer is a void pointer either way)"""
    assert _hip.ABI_VERSION == 7 and _hip.lib().yolo_hip_abi_version() == 7
    raw = C.CDLL(_hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    for name, twin in U8_ENTRIES.items():
        assert hasattr(raw, name), name
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert _hip.SIGNATURES[name] == _hip.SIGNATURES[twin], name
    assert "const uint8_t *in_dev" in header and "#define YOLO_HIP_ABI_VERSION 7" in header


def test_u8_argument_errors_name_the_u8_entry():
    """the same YOLO_ERR_* as the float32 twins (tests/test_abi.py::test_argument_errors_have_messages) with the u8 entry's name in the message"""
    lib = _hip.lib()
    g = new_graph(8, 8, 3)
    g.append(PL.conv2d_bn_act(g[-1].out, 16, 3, 1))
    p = engine.Plan(g, dtype="fp16", max_batch=2)
    buf = (C.c_uint8 * 1024)()
    out = (C.c_float * 4096)()
    ms = (C.c_float * 16)()

    def msg():
        return lib.yolo_last_error().decode()

    calls = {
        "yolo_net_forward_u8": lambda inp, b: lib.yolo_net_forward_u8(p.handle, inp, b, out, None),
        "yolo_net_forward_timed_u8": lambda inp, b: lib.yolo_net_forward_timed_u8(p.handle, inp, b, out, None, ms),
        "yolo_net_tune_streams_u8": lambda inp, b: lib.yolo_net_tune_streams_u8(p.handle, inp, b, None),
        "yolo_net_detect_u8": lambda inp, b: lib.yolo_net_detect_u8(p.handle, inp, b, 0.5, 0.5, 0, out, out, out, None),
    }
    for name, call in calls.items():
        assert call(None, 1) == 1 and msg() == name + ": null argument"
        for bad in (0, 3, -1):
            assert call(buf, bad) == 1 and msg() == name + ": batch outside 1..max_batch"
        assert call(buf, 1) == 5 and msg() == name + ": weights not loaded"
    # the float32 twins answer the same, under their own names
    assert lib.yolo_net_forward(p.handle, out, 3, out, None) == 1 and msg() == "yolo_net_forward: batch outside 1..max_batch"
    assert lib.yolo_net_forward(p.handle, out, 1, out, None) == 5 and msg() == "yolo_net_forward: weights not loaded"
    # weights "loaded" is not needed by a net without weights: a graph of a pool only reaches the workspace check
    g2 = new_graph(8, 8, 16)
    g2.append(PL.max_pool2d(g2[-1].out, 2, 2))
    p2 = engine.Plan(g2, dtype="fp16", max_batch=2)
    assert p2.weight_count == 0
    assert lib.yolo_net_forward_u8(p2.handle, buf, 1, out, None) == 5 and msg() == "yolo_net_forward_u8: workspace not bound"
    assert lib.yolo_net_detect_u8(p2.handle, buf, 1, 0.5, 0.5, 0, out, out, out, None) == 5 and msg() == "yolo_net_detect_u8: workspace not bound"
    assert lib.yolo_net_forward(p2.handle, out, 1, out, None) == 5 and msg() == "yolo_net_forward: workspace not bound"
    # resize: bad arguments
    for args in ((None, 4, 4, 12, buf, 4, 4), (buf, 0, 4, 12, buf, 4, 4), (buf, 4, 4, 11, buf, 4, 4), (buf, 4, 4, 12, None, 4, 4), (buf, 4, 4, 12, buf, 4, 0)):
        assert lib.yolo_preprocess_resize_u8(*(args + (0, None))) == 1 and msg() == "yolo_preprocess_resize_u8: bad argument"
    assert lib.yolo_u8_unit_table(None) == 1


def test_conversion_table_is_numpy_float64_division():
    """a byte u enters the first conv as float32(u / 255.) with the division in float64 (net/base.py:153 + the float32 placeholder):
    the library's conversion (yolo_u8_unit_table runs the function the input kernels run) gives exactly that for all 256 bytes, which is
    the IEEE float32 quotient and NOT a reciprocal multiply; rounded to fp16 (what fp16 nets feed the matrix cores) the 256 values stay distinct."""
    table = np.zeros(256, dtype=np.float32)
    assert _hip.lib().yolo_u8_unit_table(table.ctypes.data) == 0
    u = np.arange(256)
    want = (u.astype(np.float64) / 255.).astype(np.float32)
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, u.astype(np.float32) / np.float32(255))
    assert int(np.sum(u.astype(np.float32) * (np.float32(1) / np.float32(255)) == want)) == 130       # why not a reciprocal multiply
    h = table.astype(np.float16)
    assert np.array_equal(h.view(np.uint16), want.astype(np.float16).view(np.uint16)) and len(set(h.tolist())) == 256
    assert table[0] == 0.0 and table[255] == 1.0


def test_engine_u8_input_validation():
    """HipNetwork.check_u8 (device-free: called on a Plan): dtype, rank, H / W / C and batch range"""
    g = new_graph(8, 10, 3)
    g.append(PL.conv2d_bn_act(g[-1].out, 16, 3, 1))
    p = engine.Plan(g, dtype="fp16", max_batch=2)
    check = lambda x: engine.HipNetwork.check_u8(p, x)
    assert check(np.zeros((1, 8, 10, 3), np.uint8)) == 1 and check(np.zeros((2, 8, 10, 3), np.uint8)) == 2
    import torch
    assert check(torch.zeros((2, 8, 10, 3), dtype=torch.uint8)) == 2
    for bad in (np.zeros((1, 8, 10, 3), np.float32), np.zeros((1, 8, 10, 3), np.int8), np.zeros((1, 8, 10, 3), np.int32),
                torch.zeros((1, 8, 10, 3), dtype=torch.float32), [[1, 2, 3]], None):
        with pytest.raises(ValueError, match="uint8"):
            check(bad)
    for shape in ((8, 10, 3), (1, 8, 10), (1, 10, 8, 3), (1, 8, 10, 4), (1, 8, 10, 1), (1, 1, 8, 10, 3)):
        with pytest.raises(ValueError, match="expected uint8 input"):
            check(np.zeros(shape, np.uint8))
    for b in (0, 3):
        with pytest.raises(ValueError, match="batch %d outside" % b):
            check(np.zeros((b, 8, 10, 3), np.uint8))


def _resource_rows(src, extra):
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC"] + extra + ["--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                          "--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, cwd=os.path.dirname(src)).stderr
    rows, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = t.split(": ", 1)[1]
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            rows[cur][k.strip()] = v.strip()
    names = sorted(rows)
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {d.strip(): rows[n] for n, d in zip(names, demangled)}


@pytest.mark.parametrize("src, flags, n_u8", [("stem.hip", ["-fno-honor-nans"], 1), ("first.hip", ["-fno-honor-nans"], 11), ("aux.hip", [], 2)])
def test_u8_kernels_hold_the_register_budget_of_their_float32_twins(src, flags, n_u8):
    """hipcc's resource remarks with the flags of csrc/Makefile: every uint8-input kernel has no spilled VGPR, no scratch, and at least the
    occupancy of its float32 twin IN THE SAME COMPILE (the stem: two workgroups of 8 waves per CU); the float32 kernels still exist under
    the names profiles/ and yolo_kernel_info.symbol use."""
    rows = _resource_rows(os.path.join(ROOT, "tensorflow-yolo_amd", "csrc", src), flags)
    u8 = [n for n in rows if "_u8_kernel" in n and "resize" not in n]
    assert len(u8) == n_u8, sorted(rows)
    for name in u8:
        twin = name.replace("_u8_kernel", "_kernel")
        assert twin in rows, (name, sorted(rows))
        r, t = rows[name], rows[twin]
        print(name, {k: r[k] for k in ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")}, "| twin",
              {k: t[k] for k in ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]")})
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= int(t["Occupancy [waves/SIMD]"]), (name, r, t)
        assert int(r["LDS Size [bytes/block]"]) == int(t["LDS Size [bytes/block]"]), (name, r, t)
    if src == "stem.hip":
        assert "yolo::stem_v3_kernel(yolo::StemParams)" in rows
        assert int(rows["yolo::stem_v3_u8_kernel(yolo::StemParams)"]["Occupancy [waves/SIMD]"]) >= 4
    if src == "first.hip":
        for n in ("yolo::first_pool_mfma_kernel(yolo::FirstParams)", "void yolo::first_pool_mfma_f32_kernel<1>(yolo::FirstParams)",
                  "void yolo::first_pool_mfma_f32_kernel<2>(yolo::FirstParams)", "void yolo::conv_first_kernel<false, 32, false>(yolo::FirstParams)",
                  "void yolo::conv_first_kernel<true, 16, true>(yolo::FirstParams)"):
            assert n in rows, n
    if src == "aux.hip":
        assert "void yolo::prep_kernel<true>(yolo::PrepParams)" in rows and "void yolo::prep_kernel<false>(yolo::PrepParams)" in rows
        assert "yolo::resize_u8_kernel(yolo::ResizeParams)" in rows and "yolo::resize_u8_to_u8_kernel(yolo::ResizeParams)" in rows
        r = rows["yolo::resize_u8_to_u8_kernel(yolo::ResizeParams)"]
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0

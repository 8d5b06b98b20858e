"""CPU: the MXFP8 plan (dtype="mxfp8") -- the quantizer restatement on hand-worked blocks, what the planner marks, and the
MX kernel's register allocation."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mx_ref
from helpers import ROOT, new_graph
from oracle import cases
from tensorflow_yolo_amd import _hip
from tensorflow_yolo_amd.net import engine, layers as PL, v2, v3

NAMES80 = ["c%d" % i for i in range(80)]


def _q(vals):
    v = torch.zeros(32, dtype=torch.float32)
    v[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
    q, s = mx_ref.quantize(v)
    return q.tolist(), int(s[0])


def test_quantizer_hand_worked_blocks():
    q, s = _q([])                                       # zero block: smallest scale, zero elements
    assert s == 0 and q == [0] * 32
    q, s = _q([1.0, 0.5, -2.0])                         # amax 2 = 2^1: e = 1 - 8 = -7, 2 * 2^7 = 256 = 1.0 x 2^8
    assert s == 127 - 7 and q[2] == 0x80 | (15 << 3) and q[0] == (14 << 3) and q[1] == (13 << 3)
    q, s = _q([448.0 / 256, 464.0 / 256, 1.0])          # amax 1.8125 -> e = -8: 448 exact (0x7e); 464 = (448 + 480) / 2 -> even 448
    assert s == 119 and q[0] == 0x7E and q[1] == 0x7E
    q, s = _q([1.9375, -1.99])                          # 496 and -509.4 after scaling: saturate to +-448, never NaN (0x7f)
    assert s == 119 and q[0] == 0x7E and q[1] == 0xFE
    q, s = _q([1.0, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -17])     # e = -8: subnormals m 2^-9 after scaling by 2^8
    # 2^-9 * 2^8 = 2^-1 -> normal (6 << 3); 3 * 2^-10 * 2^8 = 0.75 -> 1.5 x 2^-1 -> (6 << 3) | 4; 2^-17 * 2^8 = 2^-9: the smallest subnormal
    assert q[1] == 6 << 3 and q[2] == (6 << 3) | 4 and q[3] == 0x01
    q, s = _q([1.0, 2.0 ** -18, 3 * 2.0 ** -18])        # 2^-10 -> tie between 0 and 2^-9: even (0); 1.5 x 2^-9 -> tie -> 2 x 2^-9
    assert q[1] == 0 and q[2] == 0x02
    q, s = _q([-3.0, -0.25])                            # negatives: sign bit; amax 3 -> e = 1 - 8
    assert s == 120 and q[0] == 0x80 | (15 << 3) | 4 and q[1] == 0x80 | (12 << 3)
    # the dequantized values are what the MFMA multiplies
    d = mx_ref.dequantize(*mx_ref.quantize(torch.tensor([[-3.0, -0.25] + [0.0] * 30])))
    assert d[0, 0].item() == -3.0 and d[0, 1].item() == -0.25


def test_host_weight_quantizer_is_bit_identical_to_the_restatement():
    """yolo_mx_quantize_host: the rule yolo_net_load_weights applies to the folded float32 weights of the MX convs"""
    rng = np.random.RandomState(5)
    rows, ch = 400, 128
    v = (rng.standard_normal((rows, ch)) * np.exp2(rng.randint(-40, 20, (rows, 1)))).astype(np.float32)
    v[0, :32] = 0
    v[1, :3] = [448 / 256, 464 / 256, 1.0]                    # the 448 / 480 tie -> 448
    v[2, :2] = [1.9375, -1.99]                                # saturation
    v[3, :4] = [1.0, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -17]   # subnormal results
    v[4, :3] = [1.0, 2.0 ** -18, 3 * 2.0 ** -18]              # ties at the subnormal end
    v[5, :32] = -np.abs(v[5, :32])
    v[6, :2] = [2.0 ** -126, 1e-45]                           # float32 denormal inputs: the scale clamps at E8M0 byte 0
    v[7, :2] = [3.0e38, -1.0]
    q = np.zeros((rows, ch), np.uint8)
    s = np.zeros((rows, ch // 32), np.uint8)
    _hip.check(_hip.lib().yolo_mx_quantize_host(v.ctypes.data, rows, ch, q.ctypes.data, s.ctypes.data), "yolo_mx_quantize_host")
    wq, ws = mx_ref.quantize(torch.from_numpy(v))
    assert np.array_equal(s, ws.numpy()), np.argwhere(s != ws.numpy())[:8]
    bad = np.argwhere(q != wq.numpy())
    assert len(bad) == 0, [(tuple(i), float(v[tuple(i)]), int(q[tuple(i)]), int(wq.numpy()[tuple(i)])) for i in bad[:8]]


def _plan(kind, size, dtype, batch=32, **kw):
    if kind == "v3":
        net = v3.create_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(size, size, 3))
    elif kind == "v2":
        net = v2.create_full_network(np.reshape(cases.COCO_V2_ANCHORS, [-1, 2]), NAMES80, False, input_shape=(size, size, 3))
    else:
        net = v2.create_tiny_network(np.reshape(cases.VOC_TINY_ANCHORS, [-1, 2]), NAMES80[:20], False, input_shape=(size, size, 3))
    return engine.Plan(net, dtype=dtype, max_batch=batch, **kw)


def _infos(p):
    import ctypes as C
    out = []
    for k in range(p.num_kernels):
        ki = _hip.KernelInfo()
        _hip.check(p.lib.yolo_net_kernel_info(p.handle, k, C.byref(ki)), "yolo_net_kernel_info")
        out.append(ki)
    return out


def test_mxfp8_plan_yolov3_608():
    pm, pf = _plan("v3", 608, "mxfp8"), _plan("v3", 608, "fp16")
    assert pm.num_kernels == pf.num_kernels == 75 and pm.num_streams == pf.num_streams
    assert pm.workspace_bytes == pf.workspace_bytes and pm.weights_bytes == pf.weights_bytes
    mx = [ki for ki in _infos(pm) if ki.name.decode().startswith("conv_mx")]
    assert len(mx) == 29
    fam = sorted((ki.out_h, ki.cin, ki.ksize, ki.stride) for ki in mx)
    assert fam.count((76, 128, 3, 1)) == 11 and fam.count((38, 256, 3, 1)) == 11 and fam.count((19, 512, 3, 1)) == 7
    for ki in mx:
        assert ki.symbol.decode().startswith("void yolo::conv3x3_mx_kernel<") and ki.flops == 2.0 * ki.out_h * ki.out_w * ki.cout * 9 * ki.cin
    dm, df = pm.describe(), pf.describe()
    assert dm.startswith("yolo_hip plan: dtype=mxf8") and dm.count("[mx: ") == 29
    # the same plan otherwise: kernels, fusions, buffers, branch tails
    assert dm.replace(" [mx: e4m3 x e4m3, block-scaled]", "").replace("dtype=mxf8", "dtype=f16") == df


def test_mxfp8_plans_of_v2_and_tiny():
    assert _plan("v2", 416, "mxfp8", batch=2).num_kernels == _plan("v2", 416, "fp16", batch=2).num_kernels
    assert sum(ki.name.decode().startswith("conv_mx") for ki in _infos(_plan("v2", 416, "mxfp8", batch=2))) > 0
    _plan("tiny", 416, "mxfp8", batch=2)


def test_fp16_and_fp32_plans_have_no_mx_kernel():
    for dtype in ("fp16", "fp32"):
        p = _plan("v3", 608, dtype)
        assert not any(ki.name.decode().startswith("conv_mx") for ki in _infos(p))
        assert "[mx: " not in p.describe() and "mxf8" not in p.describe()


def test_dtype_errors_and_forced_mx_tile():
    with pytest.raises(ValueError, match="fp16, fp32 or mxfp8"):
        _plan("tiny", 416, "fp8")
    with pytest.raises(_hip.YoloHipError, match="tile 24"):
        _plan("v3", 416, "fp16", batch=2, force_tile=24)
    g = new_graph(16, 16, 64)
    g.append(PL.conv2d_bn_act(g[-1].out, 64, 3, 1))            # Cin 64: no conv the MX kernel takes
    with pytest.raises(_hip.YoloHipError, match="tile 24"):
        engine.Plan(g, dtype="mxfp8", max_batch=2, force_tile=24)
    _plan("v3", 416, "mxfp8", batch=2, force_tile=24)


def test_mx_kernel_register_allocation_is_guarded():
    """hipcc's resource remarks for conv_mx.hip: both epilogue instantiations without scratch, at the occupancy designed
    (one 8-wave workgroup per CU: two waves per SIMD)."""
    src = os.path.join(ROOT, "tensorflow-yolo_amd", "csrc", "conv_mx.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-fno-honor-nans", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
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
    mx = {n: r for n, r in rows.items() if "conv3x3_mx_kernel" in n}
    assert len(mx) == 2, sorted(rows)
    for name, r in mx.items():
        assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["Occupancy [waves/SIMD]"]) >= 2, (name, r)

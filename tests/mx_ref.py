"""Torch-CPU restatement of the MXFP8 plan's numerics (OCP MX v1.0, e4m3fn elements, block 32 along the input channels).

quantize():  e = floor(log2 amax) - 8 per block of 32 (clamped to E8M0's range; amax 0 -> scale byte 0 and zero elements),
elements e4m3fn(v * 2^-e): clamped to +-448 first (torch's cast does not saturate), then round-to-nearest-even by the cast.
forward():   oracle/forward_ref.py's fp16-storage forward in which the convs the plan marks as MX multiply MX-quantized
activations (per pixel and 32 channels) by MX-quantized folded weights (per cout, tap and 32 input channels), in float32.
"""
import ctypes as C
import contextlib

import numpy as np
import torch

from oracle import forward_ref as FR

E4M3_MAX = 448.0


def quantize(v):
    """v: float tensor [..., C], C % 32 == 0 -> (q uint8 [..., C] e4m3fn bits, scale uint8 [..., C // 32] E8M0 bytes)."""
    v = torch.as_tensor(v).to(torch.float32)
    shp = v.shape
    b = v.reshape(-1, shp[-1] // 32, 32)
    amax = b.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)                          # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    eb = torch.clamp(ex.to(torch.int32) - 1 - 8 + 127, 0, 254)
    eb = torch.where(amax == 0, torch.zeros_like(eb), eb)
    mul = torch.ldexp(torch.ones_like(amax, dtype=torch.float64), (127 - eb).to(torch.float64))
    x = torch.clamp(b.to(torch.float64) * mul.unsqueeze(-1), -E4M3_MAX, E4M3_MAX).to(torch.float32)
    q = x.to(torch.float8_e4m3fn).view(torch.uint8)
    return q.reshape(shp), eb.to(torch.uint8).reshape(shp[:-1] + (shp[-1] // 32,))


def dequantize(q, scale):
    """inverse map onto float32 values: e4m3fn(q) * 2^(scale - 127)"""
    q = torch.as_tensor(q)
    shp = q.shape
    vals = q.view(torch.float8_e4m3fn).to(torch.float64).reshape(-1, shp[-1] // 32, 32)
    s = torch.ldexp(torch.ones((), dtype=torch.float64), torch.as_tensor(scale).to(torch.float64) - 127).reshape(-1, shp[-1] // 32, 1)
    return (vals * s).to(torch.float32).reshape(shp)


def mx_round(v):
    """quantize + dequantize along the last dimension"""
    return dequantize(*quantize(v))


def mx_conv_layers(L, eng):
    """indices (into the oracle layer list L) of the convs the engine's plan runs on the MX kernel (kernel_info names
    conv_mx<...>; a conv whose residual add is fused reports the shortcut layer)"""
    from tensorflow_yolo_amd import _hip
    out = set()
    for k in range(eng.num_kernels):
        ki = _hip.KernelInfo()
        _hip.check(eng.lib.yolo_net_kernel_info(eng.handle, k, C.byref(ki)), "yolo_net_kernel_info")
        if not ki.name.decode().startswith("conv_mx"):
            continue
        i = ki.layer
        if L[i][0] == "shortcut":
            i = next(s for s in L[i][1:3] if L[s][0] == "conv" and L[s][3] == 3 and L[s][4] == 1)
        assert L[i][0] == "conv" and L[i][3] == 3 and L[i][4] == 1, (i, L[i])
        out.add(i)
    return out


def _mx_conv(x, wd, k, s, bn, act, dtype, head):
    """_conv_folded_fp16 with MX operands: x (NCHW, fp16-valued) per pixel and 32 channels, the folded float32 kernel per
    (cout, tap, 32 input channels); float32 products and sums, float32 bias, leaky"""
    assert k == 3 and s == 1
    w = torch.from_numpy(np.ascontiguousarray(wd["kernel_oihw"])).to(torch.float64)
    if bn:
        scale = torch.from_numpy(wd["gamma"]).double() / torch.sqrt(torch.from_numpy(wd["var"]).double() + FR._BN_EPS)
        bias = torch.from_numpy(wd["beta"]).double() - torch.from_numpy(wd["mean"]).double() * scale
        w = w * scale.view(-1, 1, 1, 1)
    else:
        bias = torch.from_numpy(wd["bias"]).double()
    w = w.float()
    wq = mx_round(w.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)            # blocks along cin of each (cout, kh, kw)
    xq = mx_round(x.to(torch.float32).permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xq, wq, None, stride=1, padding=1).to(dtype)
    y = y + bias.float().to(dtype).view(1, -1, 1, 1)
    if act == "leaky":
        y = torch.maximum(FR._LEAKY * y, y)
    return y


@contextlib.contextmanager
def _patched(mx_ids):
    orig = FR._conv_folded_fp16

    def conv(x, wd, *a):
        return _mx_conv(x, wd, *a) if id(wd) in mx_ids else orig(x, wd, *a)
    FR._conv_folded_fp16 = conv
    try:
        yield
    finally:
        FR._conv_folded_fp16 = orig


def forward(L, weights, x, mx_layers):
    """forward_ref.forward(..., storage="fp16") with the convs `mx_layers` (oracle indices) on MXFP8 operands"""
    wl = FR.parse_darknet_weights(L, weights) if isinstance(weights, np.ndarray) else weights
    ids = {id(wl[i]) for i in mx_layers}
    with _patched(ids):
        return FR.forward(L, wl, x, storage="fp16")

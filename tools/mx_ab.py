"""A/B of the MXFP8 plan against the fp16 plan: YOLOv3-608 b32 (bench.py's workload) in both dtypes on one GPU in one process.

    python tools/mx_ab.py [--steps 20] [--blocks 6] [--warmup 10] [--images 2]

Both plans are built from the same calibrated synthetic weights (bench.make_model).  After a warm-up of each, blocks of `steps`
steps (forward + decode + NMS, as bench.py times them) alternate between the plans; ms/step is the median over the blocks.
The same alternation times the forward alone.  forward_timed gives the per-kernel device times of each plan (an event pair around every
launch) with both plans set to one pass of the whole batch; the 3x3 / stride-1 convs with Cin % 128 == 0 are grouped by map
size (the 76^2, 38^2 and 19^2 families the MX kernel takes).  The logit error of both plans is measured against the fp32 oracle
on `--images` distinct images.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP8_DENSE_PEAK = 5.0e15      # MI355X dense fp8 (MI355X_MICROARCH.md); MXFP8 runs at this rate
FP16_DENSE_PEAK = 2.5e15


def families(eng, ms, batch):
    """(out_h) -> [kernel ms, flops of the batch, launches, any MX] over the 3x3 / stride-1 convs with Cin % 128 == 0
    (yolo_kernel_info.flops is per image)"""
    fam = {}
    for i, ki in enumerate(eng.kernel_infos()):
        if ki.kind != 1 or ki.ksize != 3 or ki.stride != 1 or ki.cin % 128 or ki.flops <= 0:
            continue
        f = fam.setdefault(int(ki.out_h), [0.0, 0.0, 0, False])
        f[0] += float(ms[i]); f[1] += ki.flops * batch; f[2] += 1
        f[3] = f[3] or ki.name.decode().startswith("conv_mx")
    return fam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=608)
    a = ap.parse_args()
    import torch
    import bench
    from helpers import to_oracle
    from oracle import forward_ref
    from tensorflow_yolo_amd import YoloV3, _hip
    from tensorflow_yolo_amd.net import dist as ydist, synth
    assert torch.cuda.is_available(), "tools/mx_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    B, size = a.batch, a.size
    m16, w, anchors, ncls = bench.make_model("v3", size, B, "fp16")
    mmx = YoloV3()
    mmx.build(anchors, ["c%d" % i for i in range(ncls)], (size, size, 3), dtype="mxfp8", max_batch=B, weights=w)
    engs = {"fp16": m16.net.engine, "mxfp8": mmx.net.engine}
    xs = [torch.from_numpy(synth.synthetic_input(B, size, size, 3, seed=s)).cuda() for s in (1, 2)]
    for e in engs.values():
        for i in range(a.warmup):
            ydist.detect_sharded(e, xs[i & 1], 0.5, 0.6)
    torch.cuda.synchronize()
    times = {k: [] for k in engs}
    for blk in range(a.blocks):
        for k in (("fp16", "mxfp8") if blk % 2 == 0 else ("mxfp8", "fp16")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                ydist.detect_sharded(engs[k], xs[i & 1], 0.5, 0.6)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    # forward alone (no decode / NMS: their cost follows the number of candidates, which the two plans' logits do not share)
    fwd = {k: [] for k in engs}
    for blk in range(a.blocks):
        for k in (("fp16", "mxfp8") if blk % 2 == 0 else ("mxfp8", "fp16")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                engs[k].forward(xs[i & 1])
            torch.cuda.synchronize()
            fwd[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    parts = {k: int(e.lib.yolo_net_num_streams(e.handle)) for k, e in engs.items()}      # what each plan's tuner chose for the steps
    fam, kern_ms = {}, {}
    for k, e in engs.items():
        _hip.check(e.lib.yolo_net_set_streams(e.handle, 1), "yolo_net_set_streams")        # per-kernel times of the same one-pass b32 launches
        ms = np.median(np.stack([e.forward_timed(xs[0]) for _ in range(5)]), axis=0)
        fam[k] = families(e, ms, B)
        kern_ms[k] = round(float(np.sum(ms)), 4)
    # logits of both plans against the fp32 oracle on distinct images
    x = synth.synthetic_input(a.images, size, size, 3, seed=77)
    t = torch.get_num_threads()
    torch.set_num_threads(min(16, t))
    try:
        ref = forward_ref.forward(to_oracle(m16.net), w, x)
    finally:
        torch.set_num_threads(t)
    err = {k: float(np.max(np.abs(e.forward(x).cpu().numpy().astype(np.float64) - ref))) for k, e in engs.items()}
    res = {"workload": "yolov3-%d b%d" % (size, B), "gpu": torch.cuda.get_device_name(0),
           "ms_per_step": {k: round(float(np.median(v)), 4) for k, v in times.items()},
           "ms_per_step_blocks": {k: [round(x_, 4) for x_ in v] for k, v in times.items()},
           "max_abs_logit_err_vs_fp32_oracle": err, "max_abs_logit_fp32_oracle": float(np.max(np.abs(ref))), "images": a.images}
    res["forward_ms"] = {k: round(float(np.median(v)), 4) for k, v in fwd.items()}
    res["stream_parts_in_steps"] = parts
    res["forward_timed_sum_ms"] = kern_ms      # one pass of the whole batch, every kernel alone on the chip
    res["speedup_step"] = round(res["ms_per_step"]["fp16"] / res["ms_per_step"]["mxfp8"], 4)
    rows = {}
    for h in sorted(fam["fp16"], reverse=True):
        f16, fmx = fam["fp16"][h], fam["mxfp8"].get(h, [0, 0, 0, False])
        rows["%dx%d" % (h, h)] = {"launches": f16[2], "mx": fmx[3], "fp16_ms": round(f16[0], 4), "mxfp8_ms": round(fmx[0], 4),
                                  "speedup": round(f16[0] / fmx[0], 3) if fmx[0] > 0 else None,
                                  "mx_tflops": round(fmx[1] / (fmx[0] * 1e-3) / 1e12, 1) if fmx[0] > 0 else None,
                                  "mx_of_fp8_peak": round(fmx[1] / (fmx[0] * 1e-3) / FP8_DENSE_PEAK, 3) if fmx[0] > 0 else None,
                                  "fp16_tflops": round(f16[1] / (f16[0] * 1e-3) / 1e12, 1) if f16[0] > 0 else None,
                                  "fp16_of_fp16_peak": round(f16[1] / (f16[0] * 1e-3) / FP16_DENSE_PEAK, 3) if f16[0] > 0 else None}
    res["conv3x3_families"] = rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()

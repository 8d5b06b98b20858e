#!/usr/bin/env python3
"""PCIe-inclusive rate of the product API: Yolo.predict() on HOST batches -- float32 / float64 NumPy arrays as the
reference's test loop holds them (net/base.py:153) -- and Yolo.predict_u8() on the same pixels as uint8, including the host cast,
the H2D copy, the records' D2H copy and the BoundingBox lists; next to the device-resident rates.  YOLOv3-608 batch 32 fp16.
All rows run INTERLEAVED in one process: `--rounds` rounds, every row once per round (5 predicts each); per row the median over
the rounds and their spread (min .. max).  `--json FILE` writes the rows."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from tensorflow_yolo_amd.net import synth

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

model, w, anchors, ncls = bench.make_model("v3", 608, 32, "fp16")
# (the float32 rows run on the SAME pixels, quantised to 8 bits and back: not bit for bit the batch of the round-3 table in docs/HISTORY.md)
u8 = np.rint(synth.synthetic_input(32, 608, 608, 3, seed=5) * 255.).astype(np.uint8)
x32 = (u8.astype(np.float64) / 255.).astype(np.float32)     # the same pixels as the float32 batch the reference feeds
x64 = x32.astype(np.float64)
rows = [("device-resident float32 (bench.py's step)", model.predict, torch.from_numpy(x32).cuda()),
        ("device-resident uint8", model.predict_u8, torch.from_numpy(u8).cuda()),
        ("host float32, pinned", model.predict, torch.from_numpy(x32).pin_memory()),
        ("host uint8, pinned", model.predict_u8, torch.from_numpy(u8).pin_memory()),
        ("host float32, pageable", model.predict, x32),
        ("host uint8, pageable", model.predict_u8, u8),
        ("host float64 (the reference's dtype)", model.predict, x64)]
for name, fn, x in rows:        # warm-up (the first full batch also tunes the streams)
    for _ in range(2):
        boxes = fn(x)
ms = {name: [] for name, _, _ in rows}
nbox = {}
for r in range(args.rounds):
    for name, fn, x in rows:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 5
        for _ in range(n):
            boxes = fn(x)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) / n * 1e3)
        nbox[name] = sum(len(b) for b in boxes)
out = []
for name, _, _ in rows:
    v = sorted(ms[name])
    med = v[len(v) // 2]
    print("%-44s %7.2f ms/batch (min %.2f .. max %.2f over %d rounds)  %8.1f images/s   (%d boxes)"
          % (name, med, v[0], v[-1], len(v), 32e3 / med, nbox[name]))
    out.append({"row": name, "ms_median": round(med, 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3), "rounds": len(v), "boxes": nbox[name]})
if args.json:
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)

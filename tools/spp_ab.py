"""A/B of the fused SPP kernel against the three pool launches it replaces, and the step times of the two nets that came with it.

    python tools/spp_ab.py [--rounds 9] [--steps 10] [--blocks 6] [--warmup 5] [--out profiles/spp_tiny.json]

One process, one GPU.  Two plans of YOLOv3-SPP-608 b32 fp16 are built from the same calibrated synthetic weights: the default one
(spp_pool_kernel: x read once, the three pooled tensors written once) and one planned under YOLO_NO_SPP_FUSE=1 (three pool_same_kernel
launches).  The legs alternate:
  * kernel time: `rounds` rounds of yolo_net_forward_timed per leg, one pass of the whole batch (an event pair around every launch); a
    round's figure is the time of the SPP kernel, or the sum of the three launches;
  * step time (forward + decode + NMS as bench.py times it): blocks of `steps` steps per leg, ms/step per block;
  * YOLOv3-tiny-416 b64 fp16 (no SPP block: one leg) is timed in blocks between them.
Every figure is reported as median and min - max over its rounds / blocks.  The condition of the fusion is evaluated here: the fused
kernel's median must not exceed the median sum of the three launches by more than those launches' own round-to-round spread (max - min).
Both legs must give bit-identical logits (max never rounds).  Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
SPP_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
NAMES = ["c%d" % i for i in range(80)]


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def make(cls, anchors, kind, size, batch, weights=None, no_fuse=False):
    from tensorflow_yolo_amd.net import synth
    m = cls()
    if no_fuse:
        os.environ["YOLO_NO_SPP_FUSE"] = "1"        # read by the planner when the net is created
    try:
        if weights is None:
            net = cls.create_network(np.reshape(anchors, [-1, 2]), NAMES, False, input_shape=(size, size, 3))
            hg, frac = synth.HEAD_DEFAULTS[kind]
            w = synth.darknet_stream(net, seed=5, num_classes=80, head_gain=hg, obj_bias=0.0)
            m.build(anchors, NAMES, (size, size, 3), dtype="fp16", max_batch=batch, weights=w)
            weights = synth.calibrate_model(m, synth.synthetic_input(min(batch, 8), size, size, 3, seed=6), frac)
        else:
            m.build(anchors, NAMES, (size, size, 3), dtype="fp16", max_batch=batch, weights=weights)
    finally:
        os.environ.pop("YOLO_NO_SPP_FUSE", None)
    return m, weights


def pool_kernels(eng):
    return [(i, ki.name.decode(), ki.symbol.decode(), float(ki.bytes)) for i, ki in enumerate(eng.kernel_infos()) if ki.kind == 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--tiny-batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spp_tiny.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import YoloV3SPP, YoloV3Tiny, _hip
    from tensorflow_yolo_amd.net import dist as ydist, synth
    assert torch.cuda.is_available(), "tools/spp_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    B, size = a.batch, a.size
    fused, w = make(YoloV3SPP, SPP_ANCHORS, "v3-spp", size, B)
    plain, _ = make(YoloV3SPP, SPP_ANCHORS, "v3-spp", size, B, weights=w, no_fuse=True)
    tiny, _ = make(YoloV3Tiny, TINY_ANCHORS, "v3-tiny", 416, a.tiny_batch)
    legs = {"fused": fused.net.engine, "three_launches": plain.net.engine}
    pk = {k: pool_kernels(e) for k, e in legs.items()}
    assert len(pk["fused"]) == 1 and pk["fused"][0][1].startswith("spp_pool"), pk["fused"]
    assert len(pk["three_launches"]) == 3 and all(n.startswith("pool_same") for _, n, _, _ in pk["three_launches"]), pk["three_launches"]
    xs = [torch.from_numpy(synth.synthetic_input(B, size, size, 3, seed=s)).cuda() for s in (1, 2)]
    xt = [torch.from_numpy(synth.synthetic_input(a.tiny_batch, 416, 416, 3, seed=s)).cuda() for s in (3, 4)]
    te = tiny.net.engine
    for e in legs.values():
        for i in range(a.warmup):
            ydist.detect_sharded(e, xs[i & 1], 0.5, 0.6)
    for i in range(a.warmup):
        ydist.detect_sharded(te, xt[i & 1], 0.5, 0.6)
    torch.cuda.synchronize()
    same = bool(np.array_equal(legs["fused"].forward(xs[0]).cpu().numpy().view(np.uint32),
                               legs["three_launches"].forward(xs[0]).cpu().numpy().view(np.uint32))) \
        if legs["fused"].num_streams == legs["three_launches"].num_streams else None

    def block(e, x):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            ydist.detect_sharded(e, x[i & 1], 0.5, 0.6)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    step = {k: [] for k in legs}
    step_tiny = []
    for blk in range(a.blocks):
        for k in (("fused", "three_launches") if blk % 2 == 0 else ("three_launches", "fused")):
            step[k].append(block(legs[k], xs))
        step_tiny.append(block(te, xt))
    parts = {k: int(e.num_streams) for k, e in legs.items()}
    # per-kernel device times: one pass of the whole batch in both legs
    for e in legs.values():
        _hip.check(e.lib.yolo_net_set_streams(e.handle, 1), "yolo_net_set_streams")
    for e in legs.values():
        e.forward_timed(xs[0])
    kern = {k: [] for k in legs}
    each = {n: [] for _, n, _, _ in pk["three_launches"]}
    fwd_sum = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (("fused", "three_launches") if r % 2 == 0 else ("three_launches", "fused")):
            ms = legs[k].forward_timed(xs[r & 1])
            kern[k].append(sum(float(ms[i]) for i, _, _, _ in pk[k]))
            fwd_sum[k].append(float(np.sum(ms)))
            if k == "three_launches":
                for i, n, _, _ in pk[k]:
                    each[n].append(float(ms[i]))
    if same is None:
        same = bool(np.array_equal(legs["fused"].forward(xs[0]).cpu().numpy().view(np.uint32),
                                   legs["three_launches"].forward(xs[0]).cpu().numpy().view(np.uint32)))
    ks = {k: stats(v) for k, v in kern.items()}
    spread = ks["three_launches"]["max"] - ks["three_launches"]["min"]
    bytes_ = {k: sum(b for _, _, _, b in pk[k]) * B for k in legs}          # yolo_kernel_info.bytes is per image
    res = {
        "gpu": torch.cuda.get_device_name(0),
        "workload": "yolov3-spp-%d b%d fp16" % (size, B),
        "spp_kernels": {k: [{"name": n, "symbol": s} for _, n, s, _ in v] for k, v in pk.items()},
        "spp_kernel_ms": ks,
        "three_launches_each_ms": {n: stats(v) for n, v in each.items()},
        "spp_bytes": bytes_,
        "spp_GBps_at_median": {k: round(bytes_[k] / (ks[k]["median"] * 1e-3) / 1e9, 1) for k in legs},
        "three_launches_spread_ms": round(spread, 4),
        "fused_no_slower_than_three_launches": bool(ks["fused"]["median"] <= ks["three_launches"]["median"] + spread),
        "fused_speedup_at_median": round(ks["three_launches"]["median"] / ks["fused"]["median"], 3),
        "forward_timed_sum_ms": {k: stats(v) for k, v in fwd_sum.items()},
        "ms_per_step": {k: stats(v) for k, v in step.items()},
        "stream_parts_in_steps": parts,
        "logits_bit_identical": same,
        "tiny": {"workload": "yolov3-tiny-416 b%d fp16" % a.tiny_batch, "ms_per_step": stats(step_tiny),
                 "images_per_s_at_median": round(a.tiny_batch / (float(np.median(step_tiny)) * 1e-3), 1),
                 "stream_parts": int(te.num_streams)},
        "images_per_s_at_median": {k: round(B / (float(np.median(v)) * 1e-3), 1) for k, v in step.items()},
        "method": {"rounds": a.rounds, "steps_per_block": a.steps, "blocks": a.blocks, "warmup_steps": a.warmup,
                   "kernel_time": "yolo_net_forward_timed (hipEvents around every launch), one pass of the batch, legs alternating",
                   "step_time": "host clock around `steps` x (forward + decode + NMS) ending in a device synchronise, legs alternating"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""What the device-side evaluation costs beside the step it follows, and the first plan-vs-plan mAPs.

    python tools/eval_ab.py [--batch 32] [--size 608] [--rounds 12] [--warmup 3] [--out profiles/eval.json]

One process, one GPU.  YOLOv3 on the bench batch (bench.make_model: synthetic calibrated weights), fp16, threshold 0.005, max_boxes 1024,
about 20 synthetic truths per image (the fp32 plan's boxes at 0.5, cut or padded with random boxes to 20).
  (a) device time (a hipEvent pair) of yolo_eval_add beside the detect step of the same round, the legs alternating; beside a HOST arm
      in the same rounds: the step's records copied D2H and matched by tests/eval_ref.py (wall clock, copy included); and
      yolo_eval_finish on 2^16 and 2^20 random records.  Medians with min - max over the rounds; no target is set.
  (b) mAP of the fp32 (sanity: 1.0), fp16 and mxfp8 plans at threshold 0.005 against the fp32 plan's boxes at 0.5 as truths.
Writes the JSON to --out and prints it as one line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def host_lists(boxes, counts):
    b, c = boxes.cpu().numpy(), counts.cpu().numpy()
    cls = b[..., 5].view(np.int32)
    return [[tuple(b[i, r, :5]) + (int(cls[i, r]),) for r in range(int(c[i]))] for i in range(len(c))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval.json"))
    a = ap.parse_args()
    import torch
    import bench
    import eval_ref
    from tensorflow_yolo_amd import YoloV3, _hip
    from tensorflow_yolo_amd.net import evaluate as yeval, synth
    assert torch.cuda.is_available(), "tools/eval_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    B, size, K = a.batch, a.size, 1024
    _, w, anchors, ncls = bench.make_model("v3", size, B, "fp16")
    names = ["c%d" % i for i in range(ncls)]
    x = torch.from_numpy(synth.synthetic_input(B, size, size, 3, seed=1)).cuda()

    def model(dtype):
        m = YoloV3()
        m.build(anchors, names, (size, size, 3), dtype=dtype, max_batch=B, weights=w, max_boxes=K, cand_capacity=65536)
        return m.net.engine

    out = {"workload": "v3-%d-b%d" % (size, B), "threshold": 0.005, "max_boxes": K}
    # ---- (b) plan-vs-plan mAP: truths = the fp32 plan's boxes at 0.5 --------------------------------------------------------------
    engines = {"fp32": model("fp32"), "fp16": model("fp16")}
    e32 = engines["fp32"]
    truths = [[d[:4] + (d[5], 0) for d in img] for img in host_lists(*e32.detect(x, 0.5, 0.6)[:2])]
    max_gt = max(32, max(len(t) for t in truths))
    plans = {}
    for dtype in ("fp32", "fp16", "mxfp8"):
        eng = engines[dtype] if dtype in engines else model(dtype)
        ev = yeval.Evaluator(ncls, det_capacity=B * K, max_gt=max_gt)
        boxes, counts, status = eng.detect(x, 0.005, 0.6)
        ev.add(boxes, counts, truths, status)
        r = ev.finish()
        plans[dtype] = {"map_voc12": r.map_voc12, "map_voc07": r.map_voc07, "n_records": r.n_records, "truths": int(r.n_gt.sum()),
                        "tp": int(r.tp.sum()), "fp": int(r.fp.sum()), "status": r.status, "images_truncated": ev.images_truncated}
    out["plan_vs_plan"] = plans
    e16 = engines["fp16"]
    del e32, engines, eng
    # ---- (a) cost of yolo_eval_add beside the detect step, fp16 ------------------------------------------------------------------
    rng = np.random.default_rng(2)
    gts = [list(t[:20]) + [(float(rng.uniform(.1, .9)), float(rng.uniform(.1, .9)), float(rng.uniform(.05, .3)), float(rng.uniform(.05, .3)),
                            int(rng.integers(0, ncls)), 0) for _ in range(max(0, 20 - len(t)))] for t in truths]
    ev = yeval.Evaluator(ncls, det_capacity=1 << 20, max_gt=max_gt)
    packed = ev.upload_gts(gts)                 # on the device once, as Yolo.evaluate does it
    t_det, t_add, t_host = [], [], []
    for rnd in range(a.warmup + a.rounds):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev.reset()
        torch.cuda.synchronize()
        e[0].record()
        boxes, counts, status = e16.detect(x, 0.005, 0.6)
        e[1].record()
        ev.add(boxes, counts, packed, status)
        e[2].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()             # the host arm of the same round: D2H of the records + the sequential NumPy evaluator
        eval_ref.evaluate(host_lists(boxes, counts), gts, ncls, max_boxes=K)
        t1 = time.perf_counter()
        if rnd >= a.warmup:
            t_det.append(e[0].elapsed_time(e[1]))
            t_add.append(e[1].elapsed_time(e[2]))
            t_host.append((t1 - t0) * 1e3)
    out["match"] = {"detect_ms": stats(t_det), "eval_add_ms": stats(t_add), "host_arm_ms": stats(t_host),
                    "records_per_step": int(counts.sum().item()), "truths_per_image": 20,
                    "add_over_detect": round(float(np.median(t_add) / np.median(t_det)), 4)}
    # ---- yolo_eval_finish at 2^16 and 2^20 records -----------------------------------------------------------------------------
    out["finish"] = {}
    for n in (1 << 16, 1 << 20):
        evn = yeval.Evaluator(ncls, det_capacity=n, max_gt=max_gt)
        fake = np.zeros((n // K, K, 6), dtype=np.float32)
        fake[..., :4] = rng.uniform(0.1, 0.9, (n // K, K, 4))
        fake[..., 4] = np.sort(rng.uniform(0, 1, (n // K, K)), axis=1)[:, ::-1]
        fake[..., 5] = rng.integers(0, ncls, (n // K, K)).astype(np.int32).view(np.float32)
        fb = torch.from_numpy(fake).cuda()
        fc = torch.full((n // K,), K, dtype=torch.int32, device="cuda")
        for lo in range(0, n // K, B):
            evn.add(fb[lo:lo + B], fc[lo:lo + B], [[] for _ in range(min(B, n // K - lo))])
        ts = []
        for rnd in range(a.warmup + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            _hip.check(evn.lib.yolo_eval_finish(C.byref(evn.desc), evn.state.data_ptr(), evn.result.data_ptr(), evn._stream()), "yolo_eval_finish")
            e1.record()
            torch.cuda.synchronize()
            if rnd >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        out["finish"][str(n)] = stats(ts)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Device time of the gradient of the YOLOv2 loss: yolo_v2_loss_grad against yolo_v2_loss on a 13 x 13 x 5 x 80 head.

    python tools/loss_grad_ab.py [--rounds 9] [--enqueues 100] [--warmup 20] [--batches 16,64] [--truths 0,8,256] [--out profiles/loss_grad.json]

One process, one GPU.  Every figure is the time between two hipEvents around `enqueues` back-to-back enqueues (no host wait in
between), divided by the enqueues; `rounds` such figures per arm, the two arms alternating round by round, reported as median and
min - max.  yolo_v2_loss_grad runs the two kernels of yolo_v2_loss and then the gradient kernel, so the difference of the medians is
what the gradient adds to a call: the gradient kernel with its launch, AND what its stores cost the loss kernels of the next call (at
batch 64 the logits no longer stay in the L2s: DESIGN.md section 10).  Batch 16 and 64, with 0, 8 and 256 truths per image (random
logits in [-6, 6], random truths; both arms write the winner table).  The gradient kernel reads only the table, never the truths of a
cell that has no winner; its own work grows with the number of cells that have one.  Bytes: one read and one write of the logits.  --batches / --truths narrow the cases (one case under `rocprofv3 --kernel-trace --stats`
gives the gradient kernel's own duration).  Writes the JSON to --out and prints it as one line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2_ANCHORS = [0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828]


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def random_truths(rng, batch, n):
    return [[(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), int(rng.randint(0, 80)), 0) for _ in range(n)]
            for _ in range(batch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--enqueues", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--truths", default="0,8,256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_grad.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import _hip
    from tensorflow_yolo_amd.net import engine, evaluate as yeval
    assert torch.cuda.is_available(), "tools/loss_grad_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    lib = _hip.lib()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(7)

    def timed_us(fn):
        """microseconds per enqueue of `enqueues` back-to-back calls of fn"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.enqueues):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.enqueues

    hd = engine.head_desc_v2(13, 13, V2_ANCHORS, 80)
    out = {}
    for batch in [int(v) for v in a.batches.split(",")]:
        logits = torch.from_numpy(rng.uniform(-6, 6, size=(batch, 13, 13, 5, 85)).astype(np.float32)).cuda()
        grad = torch.empty_like(logits)
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        result = torch.empty(64, dtype=torch.uint8, device="cuda")
        assign = torch.empty((batch, 13, 13), dtype=torch.int32, device="cuda")
        for n in [int(v) for v in a.truths.split(",")]:
            arr, counts = yeval.pack_gts(random_truths(rng, batch, n), max(n, 1))
            gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
            arms = {"loss": lambda: _hip.check(lib.yolo_v2_loss(C.byref(hd), logits.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), max(n, 1),
                                                                images.data_ptr(), assign.data_ptr(), result.data_ptr(), st), "yolo_v2_loss"),
                    "loss_grad": lambda: _hip.check(lib.yolo_v2_loss_grad(C.byref(hd), logits.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(),
                                                                          max(n, 1), images.data_ptr(), assign.data_ptr(), result.data_ptr(),
                                                                          grad.data_ptr(), st), "yolo_v2_loss_grad")}
            for fn in arms.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in arms}
            for r in range(a.rounds):
                for k in (("loss", "loss_grad") if r % 2 == 0 else ("loss_grad", "loss")):
                    t[k].append(timed_us(arms[k]))
            ss = {k: stats(v) for k, v in t.items()}
            diff = round(ss["loss_grad"]["median"] - ss["loss"]["median"], 3)
            nbytes = 2 * logits.numel() * 4
            out["b%d_truths%d" % (batch, n)] = dict(ss, grad_minus_loss_at_median=diff, loss_spread=round(ss["loss"]["max"] - ss["loss"]["min"], 3),
                                                    logits_read_plus_grad_written_bytes=nbytes,
                                                    gbytes_per_s_at_that_difference=round(nbytes / diff * 1e-3, 1) if diff > 0 else None)
    res = {"gpu": torch.cuda.get_device_name(0), "head": "13x13x5x80", "yolo_v2_loss_grad_vs_yolo_v2_loss_us": out,
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "warmup_enqueues": a.warmup,
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; arms alternating round by round"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

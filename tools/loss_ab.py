"""Device time of the YOLOv2 loss: the standalone entry on a 13 x 13 x 5 x 80 head, and the loss step against the forward pass alone.

    python tools/loss_ab.py [--rounds 9] [--enqueues 100] [--warmup 20] [--out profiles/loss.json]

One process, one GPU.  Every figure is the time between two hipEvents around `enqueues` back-to-back enqueues (no host wait in
between), divided by the enqueues; `rounds` such figures per case, reported as median and min - max.
  * yolo_v2_loss at 13 x 13 x 5 x 80, batch 16 and 64, with 0, 8 and 256 truths per image (random logits in [-6, 6], random truths);
  * YOLOv2-416 fp16 at batch 16, synthetic weights: yolo_net_loss_u8 against yolo_net_forward_u8 alone, the two legs interleaved round by
    round, 8 truths per image; the difference of the medians is what the loss adds to a step.
Writes the JSON to --out and prints it as one line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2_ANCHORS = [0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828]
NAMES = ["c%d" % i for i in range(80)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import YoloV2, _hip
    from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth
    assert torch.cuda.is_available(), "tools/loss_ab.py measures on the GPU"
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

    def upload(truths, max_gt):
        arr, counts = yeval.pack_gts(truths, max_gt)
        return torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()

    hd = engine.head_desc_v2(13, 13, V2_ANCHORS, 80)
    standalone = {}
    for batch in (16, 64):
        logits = torch.from_numpy(rng.uniform(-6, 6, size=(batch, 13, 13, 5, 85)).astype(np.float32)).cuda()
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        result = torch.empty(64, dtype=torch.uint8, device="cuda")
        for n in (0, 8, 256):
            gt, gc = upload(random_truths(rng, batch, n), max(n, 1))
            fn = lambda: _hip.check(lib.yolo_v2_loss(C.byref(hd), logits.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), max(n, 1),
                                                     images.data_ptr(), None, result.data_ptr(), st), "yolo_v2_loss")
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            standalone["b%d_truths%d" % (batch, n)] = stats([timed_us(fn) for _ in range(a.rounds)])

    batch = 16
    m = YoloV2()
    net = YoloV2.create_network(np.reshape(V2_ANCHORS, [-1, 2]), NAMES, False, input_shape=(416, 416, 3))
    w = synth.darknet_stream(net, seed=5, num_classes=80, head_gain=synth.HEAD_DEFAULTS["v2"][0], obj_bias=0.0)
    m.build(V2_ANCHORS, NAMES, (416, 416, 3), dtype="fp16", max_batch=batch, weights=w)
    eng = m.net.engine
    x = torch.from_numpy(rng.randint(0, 256, size=(batch, 416, 416, 3)).astype(np.uint8)).cuda()
    gts = upload(random_truths(rng, batch, 8), 8)
    gts = (gts[0].reshape(batch, -1), gts[1])
    out = torch.empty((batch,) + tuple(eng.output_shape), dtype=torch.float32, device="cuda")
    images = torch.empty((batch, 56), dtype=torch.uint8, device="cuda")
    legs = {"forward_u8": lambda: eng.forward_u8(x, out=out), "loss_u8": lambda: eng.loss_u8(x, gts, images=images)}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    step = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (("forward_u8", "loss_u8") if r % 2 == 0 else ("loss_u8", "forward_u8")):
            step[k].append(timed_us(legs[k]))
    ss = {k: stats(v) for k, v in step.items()}
    res = {"gpu": torch.cuda.get_device_name(0),
           "yolo_v2_loss_us": {"head": "13x13x5x80", "cases": standalone},
           "yolov2_416_fp16_b16_us": dict(ss, loss_minus_forward_at_median=round(ss["loss_u8"]["median"] - ss["forward_u8"]["median"], 3),
                                          forward_spread=round(ss["forward_u8"]["max"] - ss["forward_u8"]["min"], 3)),
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "warmup_enqueues": a.warmup,
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; legs alternating round by round"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Device time of the YOLOv3 loss entries: yolo_v3_loss and yolo_v3_loss_grad on the YOLOv3-608 head (19^2 / 38^2 / 76^2, A = 3, C = 80),
and yolo_net_loss_v3_u8 against yolo_net_forward_u8 alone.

    python tools/loss_v3_ab.py [--rounds 9] [--enqueues 100] [--warmup 20] [--batches 16,32] [--truths 0,8,64] [--nets v3-608:32,v3-tiny-416:64]
                               [--net-enqueues 10] [--out profiles/loss_v3.json]

One process, one GPU.  Every figure is the time between two hipEvents around `enqueues` back-to-back enqueues (no host wait in
between), divided by the enqueues; `rounds` such figures per arm, the two arms alternating round by round, reported as median and
min - max.  yolo_v3_loss is three kernels (assign, terms, finish); yolo_v3_loss_grad runs them and then the gradient kernel, so the
difference of the medians is what the gradient adds to a call.  Random logits in [-4, 4], random truths.

Beside each figure, the bytes the ALGORITHM must move, computed from the shapes, and those bytes over the measured HBM peak of 6.29 TB/s
(float4 copy):
    terms kernel     the 128-byte cache lines that hold t0..t4 of every row, plus one read of the table
    gradient kernel  one write of G, the cache lines that hold t4 of every row, plus one read of the table
They are floors for ONE kernel each; the figure beside the first is the time of all three kernels of yolo_v3_loss, launches included.
Writes the JSON to --out and prints it as one line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = ((19, 19), (38, 38), (76, 76))
# the anchors of yolov3.cfg in pixels of a 608 input, coarse scale first; grid units: over the stride
ANCHORS_PX = (((116, 90), (156, 198), (373, 326)), ((30, 61), (62, 45), (59, 119)), ((10, 13), (16, 30), (33, 23)))
V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
HBM_PEAK = 6.29e12
LINE = 128


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def random_truths(rng, batch, n, n_classes=80):
    return [[(rng.uniform(0.02, 0.98), rng.uniform(0.02, 0.98), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), int(rng.randint(0, n_classes)), 0)
             for _ in range(n)] for _ in range(batch)]


def lines_touched(rows, width, first, last):
    """128-byte lines that hold elements first..last of every row of a dense float32 [rows][width] tensor"""
    start = np.arange(rows, dtype=np.int64) * width * 4
    lo, hi = (start + 4 * first) // LINE, (start + 4 * last + 3) // LINE
    return int(np.unique(np.concatenate([lo, hi])).size)


def floors(batch, rows, width):
    n_rows = batch * rows
    terms = lines_touched(n_rows, width, 0, 4) * LINE + 4 * n_rows
    grad = 4 * n_rows * width + lines_touched(n_rows, width, 4, 4) * LINE + 4 * n_rows
    return {"terms_kernel_floor_bytes": terms, "terms_kernel_floor_us_at_hbm_peak": round(terms / HBM_PEAK * 1e6, 2),
            "grad_kernel_floor_bytes": grad, "grad_kernel_floor_us_at_hbm_peak": round(grad / HBM_PEAK * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--enqueues", type=int, default=100)
    ap.add_argument("--net-enqueues", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", default="16,32")
    ap.add_argument("--truths", default="0,8,64")
    ap.add_argument("--nets", default="v3-608:32,v3-tiny-416:64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_v3.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import YoloV3, YoloV3Tiny, _hip
    from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth
    assert torch.cuda.is_available(), "tools/loss_v3_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    lib = _hip.lib()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(7)

    def timed_us(fn, enqueues):
        """microseconds per enqueue of `enqueues` back-to-back calls of fn"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(enqueues):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / enqueues

    def ab(arms, enqueues, warmup):
        names = list(arms)
        for fn in arms.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in names}
        for r in range(a.rounds):
            for k in (names if r % 2 == 0 else names[::-1]):
                t[k].append(timed_us(arms[k], enqueues))
        return {k: stats(v) for k, v in t.items()}

    anchors = [[(w / (608. / g[1]), h / (608. / g[0])) for w, h in px] for g, px in zip(GRIDS, ANCHORS_PX)]
    hd = engine.head_desc_v3(GRIDS, anchors, 80)
    rows, parts = engine.v3_loss_rows(hd)
    head = {}
    for batch in [int(v) for v in a.batches.split(",") if v]:
        logits = torch.from_numpy(rng.uniform(-4, 4, size=(batch, rows, 85)).astype(np.float32)).cuda()
        grad = torch.empty_like(logits)
        scratch = torch.empty(batch * parts * 56, dtype=torch.uint8, device="cuda")
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        result = torch.empty(64, dtype=torch.uint8, device="cuda")
        assign = torch.empty((batch, rows), dtype=torch.int32, device="cuda")
        for n in [int(v) for v in a.truths.split(",")]:
            arr, counts = yeval.pack_gts(random_truths(rng, batch, n), max(n, 1))
            gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
            arms = {"loss": lambda: _hip.check(lib.yolo_v3_loss(C.byref(hd), logits.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), max(n, 1), 0.7,
                                                                scratch.data_ptr(), images.data_ptr(), assign.data_ptr(), result.data_ptr(), st),
                                               "yolo_v3_loss"),
                    "loss_grad": lambda: _hip.check(lib.yolo_v3_loss_grad(C.byref(hd), logits.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(),
                                                                          max(n, 1), 0.7, scratch.data_ptr(), images.data_ptr(), assign.data_ptr(),
                                                                          result.data_ptr(), grad.data_ptr(), st), "yolo_v3_loss_grad")}
            ss = ab(arms, a.enqueues, a.warmup)
            torch.cuda.synchronize()
            ignored = int((assign == -2).sum())
            head["b%d_truths%d" % (batch, n)] = dict(ss, grad_minus_loss_at_median=round(ss["loss_grad"]["median"] - ss["loss"]["median"], 3),
                                                     ignored_rows=ignored, **floors(batch, rows, 85))
    nets = {}
    for spec in [v for v in a.nets.split(",") if v]:
        name, batch = spec.split(":")
        batch = int(batch)
        cls, anc, size = (YoloV3Tiny, TINY_ANCHORS, 416) if name == "v3-tiny-416" else (YoloV3, V3_ANCHORS, 608)
        names = ["c%d" % i for i in range(80)]
        net = cls.create_network(np.reshape(anc, [-1, 2]), names, False, input_shape=(size, size, 3))
        m = cls()
        m.build(anc, names, (size, size, 3), dtype="fp16", max_batch=batch, weights=synth.darknet_stream(net, seed=1, num_classes=80))
        eng = m.net.engine
        x = torch.from_numpy(rng.randint(0, 256, size=(batch, size, size, 3)).astype(np.uint8)).to(eng.device)
        arr, counts = yeval.pack_gts(random_truths(rng, batch, 8), 8)
        gts = (torch.from_numpy(arr.view(np.uint8).reshape(batch, -1)).to(eng.device), torch.from_numpy(counts).to(eng.device))
        out = eng.forward_u8(x)
        arms = {"forward_u8": lambda: eng.forward_u8(x, out=out), "loss_v3_u8": lambda: eng.loss_v3_u8(x, gts)}
        ss = ab(arms, a.net_enqueues, 3)
        nets["%s_fp16_b%d" % (name, batch)] = dict(ss, loss_minus_forward_at_median=round(ss["loss_v3_u8"]["median"] - ss["forward_u8"]["median"], 3),
                                                  forward_spread=round(ss["forward_u8"]["max"] - ss["forward_u8"]["min"], 3))
        del m, eng
    res = {"gpu": torch.cuda.get_device_name(0), "head": "19x19,38x38,76x76 x3 x80 (%d rows, %d parts)" % (rows, parts),
           "yolo_v3_loss_grad_vs_yolo_v3_loss_us": head, "yolo_net_loss_v3_u8_vs_yolo_net_forward_u8_us": nets,
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "net_enqueues_per_round": a.net_enqueues, "warmup_enqueues": a.warmup,
                      "hbm_peak_bytes_per_s": HBM_PEAK,
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; arms alternating round by round"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Device time of a training step of the detection layer: yolo_net_train_head_step_u8 against yolo_net_loss_u8 on the same build, and
yolo_conv1x1_wgrad alone.

    python tools/train_ab.py [--rounds 7] [--enqueues 20] [--kernel-enqueues 100] [--warmup 5] [--batches 16,64] [--couts 30,125,425]
                             [--out profiles/train_head.json]

One process, one GPU.  Every figure is the time between two hipEvents around back-to-back enqueues (no host wait in between), divided by
the enqueues; `rounds` such figures per arm, the arms alternating round by round, reported as median and min - max.

  step    YOLOv2-416 (COCO head: 425 x 1024), fp16 plan, one stream part, synthetic weights, uint8 batches of 16 and 64 with 8 truths per
          image.  yolo_net_train_head_step_u8 runs the forward pass and the loss kernels of yolo_net_loss_u8 and then the gradient kernel,
          the two weight-gradient kernels and the Adam + re-pack kernel, so the difference of the medians is what training the layer adds
          to a validation step.
  wgrad   yolo_conv1x1_wgrad alone on a dense fp16 X [P][1024], P = batch * 169, for cout 30 / 125 / 425: both kernels.  Bytes counted:
          X and G read once, the slabs written and read once, dW and db written.

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


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def random_truths(rng, batch, n):
    return [[(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), int(rng.randint(0, 80)), 0) for _ in range(n)]
            for _ in range(batch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--enqueues", type=int, default=20)
    ap.add_argument("--kernel-enqueues", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--couts", default="30,125,425")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_head.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import YoloV2, _hip
    from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth, train as ytrain
    assert torch.cuda.is_available(), "tools/train_ab.py measures on the GPU"
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

    def interleaved(arms, enqueues):
        for fn in arms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        names = list(arms)
        t = {k: [] for k in names}
        for r in range(a.rounds):
            for k in (names if r % 2 == 0 else names[::-1]):
                t[k].append(timed_us(arms[k], enqueues))
        return {k: stats(v) for k, v in t.items()}

    batches = [int(v) for v in a.batches.split(",")]
    names = ["c%d" % i for i in range(80)]
    weights = None
    step = {}
    for batch in batches:
        m = YoloV2()
        net = YoloV2.create_network(np.reshape(V2_ANCHORS, [-1, 2]), names, False, input_shape=(416, 416, 3))
        if weights is None:
            weights = synth.darknet_stream(net, seed=1, num_classes=80, head_gain=synth.HEAD_DEFAULTS["v2"][0], obj_bias=0.0)
        m.build(V2_ANCHORS, names, (416, 416, 3), dtype="fp16", max_batch=batch, weights=weights, streams=1)
        eng = m.net.engine
        cout, cin, _, _ = ytrain.head_counts(m.net)
        eng.head_train_init(*ytrain.split_head(weights, cout, cin))
        x = torch.from_numpy(rng.randint(0, 256, size=(batch, 416, 416, 3)).astype(np.uint8)).cuda()
        arr, counts = yeval.pack_gts(random_truths(rng, batch, 8), 8)
        gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        result = torch.empty(64, dtype=torch.uint8, device="cuda")
        lr_t = float(engine.adam_lr_t(1e-4, 1000))         # (a late step: small updates, the weights stay where they are)
        arms = {"loss": lambda: _hip.check(lib.yolo_net_loss_u8(eng.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8, images.data_ptr(),
                                                                None, result.data_ptr(), st), "yolo_net_loss_u8"),
                "train_step": lambda: _hip.check(lib.yolo_net_train_head_step_u8(eng.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8,
                                                                                 eng._train_state.data_ptr(), lr_t, result.data_ptr(), st),
                                                 "yolo_net_train_head_step_u8")}
        ss = interleaved(arms, a.enqueues)
        diff = round(ss["train_step"]["median"] - ss["loss"]["median"], 3)
        pl = _hip.wgrad_plan(batch * 169, cin, cout)
        step["b%d" % batch] = dict(ss, step_minus_loss_at_median=diff, loss_spread=round(ss["loss"]["max"] - ss["loss"]["min"], 3),
                                   percent_of_the_loss_step=round(100.0 * diff / ss["loss"]["median"], 2), wgrad_chunks=pl["n_chunks"],
                                   wgrad_scratch_bytes=pl["scratch_bytes"])
        del m, eng
    wgrad = {}
    cin = 1024
    for batch in batches:
        P = batch * 169
        X = torch.from_numpy(rng.randn(P, cin).astype(np.float16)).cuda()
        for cout in [int(v) for v in a.couts.split(",")]:
            pl = _hip.wgrad_plan(P, cin, cout)
            G = torch.from_numpy(rng.randn(P, cout).astype(np.float32)).cuda()
            dw = torch.empty(cout * cin, dtype=torch.float32, device="cuda")
            db = torch.empty(cout, dtype=torch.float32, device="cuda")
            scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda")
            fn = lambda: _hip.check(lib.yolo_conv1x1_wgrad(X.data_ptr(), _hip.DTYPE_F16, cin, 0, 169 * cin, 169, batch, cin, G.data_ptr(), cout,
                                                           dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), scratch.numel(), st), "yolo_conv1x1_wgrad")
            ss = interleaved({"wgrad": fn}, a.kernel_enqueues)["wgrad"]
            operands = P * cin * 2 + P * cout * 4
            nbytes = operands + 2 * pl["scratch_bytes"] + cout * (cin + 1) * 4
            wgrad["b%d_cout%d" % (batch, cout)] = dict(ss, chunks=pl["n_chunks"], positions_per_chunk=pl["positions_per_chunk"],
                                                       workgroups=pl["tiles_cout"] * pl["tiles_cin"] * pl["n_chunks"], operand_bytes=operands,
                                                       bytes_with_slabs=nbytes, gbytes_per_s=round(nbytes / ss["median"] * 1e-3, 1),
                                                       gflop=round(2.0 * P * cout * cin * 1e-9, 3),
                                                       tflops=round(2.0 * P * cout * cin / ss["median"] * 1e-6, 2))
    res = {"gpu": torch.cuda.get_device_name(0), "network": "YOLOv2-416 fp16, COCO head 425 x 1024, 8 truths per image",
           "yolo_net_train_head_step_u8_vs_yolo_net_loss_u8_us": step, "yolo_conv1x1_wgrad_us": wgrad,
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "kernel_enqueues_per_round": a.kernel_enqueues, "warmup_enqueues": a.warmup,
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; arms alternating round by round"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

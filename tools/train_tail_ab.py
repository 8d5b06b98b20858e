"""Device time of training the tail of YOLOv2-416: yolo_conv1x1_dgrad and yolo_conv3x3_wgrad alone, and yolo_net_train_tail_step_u8 against
yolo_net_train_head_step_u8 and yolo_net_loss_u8 (whose code this change does not touch) in one interleaved run.

    python tools/train_tail_ab.py [--rounds 7] [--enqueues 10] [--kernel-enqueues 20] [--warmup 3] [--batches 16,64]
                                  [--out profiles/train_tail.json]

One process, one GPU.  Every figure is the time between two hipEvents around back-to-back enqueues (no host wait in between), divided by
the enqueues; `rounds` such figures per arm, the arms alternating round by round, reported as median and min - max.

  step    YOLOv2-416 (COCO head: 425 x 1024; block 1280 -> 1024 on 13 x 13), fp16 plan, one stream part, synthetic weights, uint8 batches
          with 8 truths per image.  Three nets of the same weights, one per arm, so that no arm's update moves another's weights.
  dgrad   yolo_conv1x1_dgrad alone: G [P][425], W [425][1024], Y fp16 dense [P][1024], P = batch * 169.
  wgrad   yolo_conv3x3_wgrad alone: X3 fp16 dense [batch][13][13][1280], D [P][1024], with the scale: both kernels.  The rate counts
          2 * P * cout * 9 * cin FLOP -- the products of taps outside the image included, which the kernel multiplies by +0 -- against the
          157.3 TFLOP/s float32 matrix peak of the MI355X.

Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2_ANCHORS = [0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828]
F32_MATRIX_PEAK_TFLOPS = 157.3


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def random_truths(rng, batch, n):
    return [[(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), int(rng.randint(0, 80)), 0) for _ in range(n)]
            for _ in range(batch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--enqueues", type=int, default=10)
    ap.add_argument("--kernel-enqueues", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_tail.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import YoloV2, _hip
    from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth, train as ytrain
    assert torch.cuda.is_available(), "tools/train_tail_ab.py measures on the GPU"
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
    net0 = YoloV2.create_network(np.reshape(V2_ANCHORS, [-1, 2]), names, False, input_shape=(416, 416, 3))
    weights = synth.darknet_stream(net0, seed=1, num_classes=80, head_gain=synth.HEAD_DEFAULTS["v2"][0], obj_bias=0.0)
    cout, cin, _, _ = ytrain.head_counts(net0)
    cout3, cin3, _, _ = ytrain.tail_counts(net0)
    step, dgrad, wgrad = {}, {}, {}
    for batch in batches:
        engs = []
        for _ in range(3):
            m = YoloV2()
            m.build(V2_ANCHORS, names, (416, 416, 3), dtype="fp16", max_batch=batch, weights=weights, streams=1)
            engs.append(m.net.engine)
        e_loss, e_head, e_tail = engs
        e_head.head_train_init(*ytrain.split_head(weights, cout, cin))
        e_tail.tail_train_init(*ytrain.split_tail(weights, net0))
        x = torch.from_numpy(rng.randint(0, 256, size=(batch, 416, 416, 3)).astype(np.uint8)).cuda()
        arr, counts = yeval.pack_gts(random_truths(rng, batch, 8), 8)
        gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        result = torch.empty(64, dtype=torch.uint8, device="cuda")
        lr_t = float(engine.adam_lr_t(1e-4, 1000))         # (a late step: small updates, the weights stay where they are)
        arms = {"loss": lambda: _hip.check(lib.yolo_net_loss_u8(e_loss.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8, images.data_ptr(),
                                                                None, result.data_ptr(), st), "yolo_net_loss_u8"),
                "head_step": lambda: _hip.check(lib.yolo_net_train_head_step_u8(e_head.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8,
                                                                                e_head._train_state.data_ptr(), lr_t, result.data_ptr(), st),
                                                "yolo_net_train_head_step_u8"),
                "tail_step": lambda: _hip.check(lib.yolo_net_train_tail_step_u8(e_tail.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8,
                                                                                e_tail._tail_state.data_ptr(), lr_t, result.data_ptr(), st),
                                                "yolo_net_train_tail_step_u8")}
        ss = interleaved(arms, a.enqueues)
        lay = e_tail.tail_layout
        step["b%d" % batch] = dict(ss, tail_minus_head_at_median=round(ss["tail_step"]["median"] - ss["head_step"]["median"], 3),
                                   tail_minus_loss_at_median=round(ss["tail_step"]["median"] - ss["loss"]["median"], 3),
                                   head_minus_loss_at_median=round(ss["head_step"]["median"] - ss["loss"]["median"], 3),
                                   loss_spread=round(ss["loss"]["max"] - ss["loss"]["min"], 3), state_bytes=int(lay.total_bytes),
                                   scratch_bytes=int(lay.scratch_bytes))
        del engs, e_loss, e_head, e_tail
        torch.cuda.empty_cache()
        # the two operators alone, at the tail's shapes
        P = batch * 169
        G = torch.from_numpy(rng.randn(P, cout).astype(np.float32)).cuda()
        W = torch.from_numpy((rng.randn(cout, cin) * 0.03).astype(np.float32)).cuda()
        Y = torch.from_numpy(rng.randn(P, cin).astype(np.float16)).cuda()
        D = torch.empty(P * cin, dtype=torch.float32, device="cuda")
        fn = lambda: _hip.check(lib.yolo_conv1x1_dgrad(G.data_ptr(), cout, W.data_ptr(), cin, Y.data_ptr(), _hip.DTYPE_F16, cin, 0, 169 * cin, 169, batch,
                                                       0.1, D.data_ptr(), st), "yolo_conv1x1_dgrad")
        ds = interleaved({"dgrad": fn}, a.kernel_enqueues)["dgrad"]
        nbytes = P * cout * 4 + cout * cin * 4 + P * cin * 2 + P * cin * 4
        dgrad["b%d" % batch] = dict(ds, gflop=round(2.0 * P * cout * cin * 1e-9, 3), tflops=round(2.0 * P * cout * cin / ds["median"] * 1e-6, 2),
                                    bytes=nbytes, gbytes_per_s=round(nbytes / ds["median"] * 1e-3, 1))
        pl = _hip.conv3x3_wgrad_plan(13, 13, batch, cin3, cout3)
        X3 = torch.from_numpy(rng.randn(P, cin3).astype(np.float16)).cuda()
        D3 = torch.from_numpy(rng.randn(P, cout3).astype(np.float32)).cuda()
        scale = torch.from_numpy(rng.uniform(0.5, 2.0, size=cout3).astype(np.float32)).cuda()
        dw = torch.empty(cout3 * 9 * cin3, dtype=torch.float32, device="cuda")
        db = torch.empty(cout3, dtype=torch.float32, device="cuda")
        scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda")
        fn = lambda: _hip.check(lib.yolo_conv3x3_wgrad(X3.data_ptr(), _hip.DTYPE_F16, cin3, 0, 169 * cin3, 13, 13, batch, cin3, D3.data_ptr(), cout3,
                                                       scale.data_ptr(), dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), scratch.numel(), st),
                                "yolo_conv3x3_wgrad")
        ws = interleaved({"wgrad": fn}, a.kernel_enqueues)["wgrad"]
        flop = 2.0 * P * cout3 * 9 * cin3
        tflops = flop / ws["median"] * 1e-6
        wgrad["b%d" % batch] = dict(ws, chunks=pl["n_chunks"], positions_per_chunk=pl["positions_per_chunk"], halo_rows=pl["halo_rows"],
                                    workgroups=pl["tiles_cout"] * pl["tiles_cin"] * pl["n_chunks"], scratch_bytes=pl["scratch_bytes"],
                                    gflop=round(flop * 1e-9, 3), tflops=round(tflops, 2),
                                    percent_of_f32_matrix_peak=round(100.0 * tflops / F32_MATRIX_PEAK_TFLOPS, 1))
        del G, W, Y, D, X3, D3, dw, db, scratch
        torch.cuda.empty_cache()
    res = {"gpu": torch.cuda.get_device_name(0),
           "network": "YOLOv2-416 fp16, COCO head 425 x 1024, block 3 x 3 1280 -> 1024 on 13 x 13, 8 truths per image",
           "steps_us": step, "yolo_conv1x1_dgrad_us": dgrad, "yolo_conv3x3_wgrad_us": wgrad,
           "f32_matrix_peak_tflops": F32_MATRIX_PEAK_TFLOPS, "head_wgrad_kernel_best_percent_of_peak": 41,
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "kernel_enqueues_per_round": a.kernel_enqueues, "warmup_enqueues": a.warmup,
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; arms alternating round by round"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

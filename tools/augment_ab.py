"""Device time of the training augmentation: yolo_augment_u8 beside yolo_preprocess_frames_u8 on the same batch, and
yolo_net_train_head_step_u8 with and without the augmentation in front.

    python tools/augment_ab.py [--rounds 7] [--enqueues 20] [--warmup 5] [--batches 16,64] [--out profiles/augment.json]

One process, one GPU.  Every figure is the time between two hipEvents around back-to-back enqueues (no host wait in between), divided by
the enqueues; `rounds` such figures per arm, all the arms of a batch size in ONE interleaved run (their order reversed every other round),
reported as median and min - max.

  augment_sigma0 / augment_sigma3   yolo_augment_u8 on a uint8 batch [B, 416, 416, 3] with the reference's parameters for every image
                  (both flips, dropout 0.02, both noise steps, tx = 17, a key per image) and no blur / the widest blur net/augment.py draws
                  (sigma = 3: radius 8).  GB/s counts the source read once and the destination written once: 2 * B * 416 * 416 * 3 bytes.
  frames          yolo_preprocess_frames_u8 of B frames of 480 x 640 into the same batch: the kernel in front of the augmentation
  train_step      yolo_net_train_head_step_u8 (YOLOv2-416, fp16 plan, COCO head, 8 truths per image) on the batch
  augment_train_step                the sigma = 3 augmentation into a second buffer and the step on that buffer, enqueued back to back

Writes the JSON to --out and prints it as one line."""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--enqueues", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import YoloV2, _hip
    from tensorflow_yolo_amd.net import augment as yaug, engine, evaluate as yeval, synth, train as ytrain
    assert torch.cuda.is_available(), "tools/augment_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    lib = _hip.lib()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(7)

    def timed_us(fn, enqueues):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(enqueues):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / enqueues

    def interleaved(arms):
        for fn in arms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        names = list(arms)
        t = {k: [] for k in names}
        for r in range(a.rounds):
            for k in (names if r % 2 == 0 else names[::-1]):
                t[k].append(timed_us(arms[k], a.enqueues))
        return {k: stats(v) for k, v in t.items()}

    names = ["c%d" % i for i in range(80)]
    weights = None
    out = {}
    for batch in [int(v) for v in a.batches.split(",")]:
        m = YoloV2()
        net = YoloV2.create_network(np.reshape(V2_ANCHORS, [-1, 2]), names, False, input_shape=(416, 416, 3))
        if weights is None:
            weights = synth.darknet_stream(net, seed=1, num_classes=80, head_gain=synth.HEAD_DEFAULTS["v2"][0], obj_bias=0.0)
        m.build(V2_ANCHORS, names, (416, 416, 3), dtype="fp16", max_batch=batch, weights=weights, streams=1)
        eng = m.net.engine
        cout, cin, _, _ = ytrain.head_counts(m.net)
        eng.head_train_init(*ytrain.split_head(weights, cout, cin))
        frames = [torch.from_numpy(rng.randint(0, 256, size=(480, 640, 3)).astype(np.uint8)).cuda() for _ in range(batch)]
        descs, keep = eng.frame_descs(frames)
        x = torch.empty((batch, 416, 416, 3), dtype=torch.uint8, device="cuda")
        xa = torch.empty_like(x)
        truths = [[(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), int(rng.randint(0, 80)), 0) for _ in range(8)]
                  for _ in range(batch)]
        arr, counts = yeval.pack_gts(truths, 8)
        gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
        result = torch.empty(64, dtype=torch.uint8, device="cuda")
        lr_t = float(engine.adam_lr_t(1e-4, 1000))         # (a late step: small updates, the weights stay where they are)
        recs = {}
        for sigma in (0.0, 3.0):
            recs[sigma] = yaug.params_array([yaug.make(flip_lr=True, flip_ud=True, sigma=sigma, drop=yaug.DROP_PROBABILITY, scales=yaug.NOISE_SCALES,
                                                       locs=yaug.NOISE_LOCS, tx=17, key=int(rng.randint(1, 1 << 62))) for _ in range(batch)])

        def frames_fn():
            _hip.check(lib.yolo_preprocess_frames_u8(descs, batch, _hip.RESIZE_STRETCH, x.data_ptr(), 416, 416, st), "yolo_preprocess_frames_u8")

        def augment_fn(sigma):
            return lambda: _hip.check(lib.yolo_augment_u8(x.data_ptr(), xa.data_ptr(), batch, 416, 416, recs[sigma], st), "yolo_augment_u8")

        def step_fn(src):
            return lambda: _hip.check(lib.yolo_net_train_head_step_u8(eng.handle, src.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8,
                                                                      eng._train_state.data_ptr(), lr_t, result.data_ptr(), st),
                                      "yolo_net_train_head_step_u8")

        aug3, step_plain, step_aug = augment_fn(3.0), step_fn(x), step_fn(xa)
        frames_fn()
        arms = {"augment_sigma0": augment_fn(0.0), "augment_sigma3": aug3, "frames": frames_fn, "train_step": step_plain,
                "augment_train_step": lambda: (aug3(), step_aug())}
        ss = interleaved(arms)
        nbytes = 2 * batch * 416 * 416 * 3
        for k in ("augment_sigma0", "augment_sigma3"):
            ss[k]["gbytes_per_s"] = round(nbytes / ss[k]["median"] * 1e-3, 1)
        ss["bytes_source_plus_destination"] = nbytes
        ss["radius_at_sigma3"] = int(recs[3.0][0].radius)
        ss["augment_sigma3_percent_of_train_step"] = round(100.0 * ss["augment_sigma3"]["median"] / ss["train_step"]["median"], 2)
        ss["augment_train_step_minus_train_step_at_median"] = round(ss["augment_train_step"]["median"] - ss["train_step"]["median"], 3)
        ss["train_step_spread"] = round(ss["train_step"]["max"] - ss["train_step"]["min"], 3)
        out["b%d" % batch] = ss
        del m, eng, keep
    res = {"gpu": torch.cuda.get_device_name(0), "shape": "uint8 [B, 416, 416, 3]; YOLOv2-416 fp16, COCO head, 8 truths per image",
           "us": out,
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "warmup_enqueues": a.warmup,
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; the arms of a batch size interleaved in one run"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Device time of the 3 x 3 weight gradient on the fp16 matrix cores: yolo_conv3x3_wgrad_f16 against yolo_conv3x3_wgrad on the same data, and
the tail step (YOLOv2-416) and the blocks step (YOLOv3-608) in both modes beside the validation step, in one interleaved run.

    python tools/wgrad_f16_ab.py [--rounds 7] [--enqueues 6] [--kernel-enqueues 10] [--warmup 3] [--out profiles/wgrad_f16.json]

One process, one GPU.  Every figure is the time between two hipEvents around back-to-back enqueues (no host wait in between), divided by
the enqueues; `rounds` such figures per arm, the arms alternating round by round, reported as median and min - max (tools/train_tail_ab.py).

  operator  X3 fp16 dense [batch][h][w][cin], D float32 [P][cout] (normal variates), with the scale: every launch of either entry.  The rate
            counts 2 * P * cout * 9 * cin FLOP -- the products of taps outside the image included -- against the fp16 matrix peak of the
            MI355X, 16 x the 157.3 TFLOP/s of the float32 matrix cores.
  steps     fp16 plans, one stream part, synthetic weights, uint8 batches with 8 truths per image; one net per arm, so that no arm's update
            moves another's weights.

Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V2_ANCHORS = [0.57273, 0.677385, 1.87446, 2.06253, 3.33843, 5.47434, 7.88282, 3.52778, 9.77052, 9.16828]
V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
F32_MATRIX_PEAK_TFLOPS = 157.3
F16_MATRIX_PEAK_TFLOPS = 16 * F32_MATRIX_PEAK_TFLOPS
# (name, map, cin, cout, batches)
SHAPES = (("v2-416 13^2", 13, 1280, 1024, (16, 64)), ("v3-608 19^2", 19, 512, 1024, (16, 32)), ("v3-608 38^2", 38, 256, 512, (16, 32)),
          ("v3-608 76^2", 76, 128, 256, (16, 32)), ("v3-tiny-416 13^2", 13, 256, 512, (64,)), ("v3-tiny-416 26^2", 26, 384, 256, (64,)))


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def random_truths(rng, batch, n):
    return [[(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), int(rng.randint(0, 80)), 0) for _ in range(n)]
            for _ in range(batch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--enqueues", type=int, default=6)
    ap.add_argument("--kernel-enqueues", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tail-batches", default="16,64")
    ap.add_argument("--blocks-batches", default="32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgrad_f16.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import YoloV2, YoloV3, _hip
    from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth, train as ytrain
    assert torch.cuda.is_available(), "tools/wgrad_f16_ab.py measures on the GPU"
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

    # ---- the operator against the float32 one, on the same data ----------------------------------------------------------------------------
    ops = {}
    for name, g, cin3, cout3, batches in SHAPES:
        for batch in batches:
            P = batch * g * g
            pl32, pl16 = _hip.conv3x3_wgrad_plan(g, g, batch, cin3, cout3), _hip.conv3x3_wgrad_f16_plan(g, g, batch, cin3, cout3)
            X3 = torch.from_numpy(rng.randn(P, cin3).astype(np.float16)).cuda()
            D3 = torch.from_numpy(rng.randn(P, cout3).astype(np.float32)).cuda()
            scale = torch.from_numpy(rng.uniform(0.5, 2.0, size=cout3).astype(np.float32)).cuda()
            dw = torch.empty(cout3 * 9 * cin3, dtype=torch.float32, device="cuda")
            db = torch.empty(cout3, dtype=torch.float32, device="cuda")
            scratch = torch.empty(max(pl32["scratch_bytes"], pl16["scratch_bytes"]), dtype=torch.uint8, device="cuda")
            args = (X3.data_ptr(), _hip.DTYPE_F16, cin3, 0, g * g * cin3, g, g, batch, cin3, D3.data_ptr(), cout3, scale.data_ptr(), dw.data_ptr(),
                    db.data_ptr(), scratch.data_ptr(), scratch.numel(), st)
            arms = {"float32": lambda: _hip.check(lib.yolo_conv3x3_wgrad(*args), "yolo_conv3x3_wgrad"),
                    "fp16": lambda: _hip.check(lib.yolo_conv3x3_wgrad_f16(*args), "yolo_conv3x3_wgrad_f16")}
            ss = interleaved(arms, a.kernel_enqueues)
            flop = 2.0 * P * cout3 * 9 * cin3
            tf16, tf32 = flop / ss["fp16"]["median"] * 1e-6, flop / ss["float32"]["median"] * 1e-6
            ops["b%d %s %d->%d" % (batch, name, cin3, cout3)] = dict(
                ss, gflop=round(flop * 1e-9, 3), fp16_tflops=round(tf16, 2), float32_tflops=round(tf32, 2),
                fp16_percent_of_f16_matrix_peak=round(100.0 * tf16 / F16_MATRIX_PEAK_TFLOPS, 2),
                float32_percent_of_f32_matrix_peak=round(100.0 * tf32 / F32_MATRIX_PEAK_TFLOPS, 1),
                float32_over_fp16=round(ss["float32"]["median"] / ss["fp16"]["median"], 2), fp16_chunks=pl16["n_chunks"],
                fp16_workgroups=pl16["tiles_cout"] * pl16["tiles_cin"] * pl16["n_chunks"], fp16_halo_rows=pl16["halo_rows"])
            del X3, D3, scale, dw, db, scratch
            torch.cuda.empty_cache()

    # ---- the tail step of YOLOv2-416 in both modes beside the validation step -----------------------------------------------------------------
    names = ["c%d" % i for i in range(80)]
    steps = {}
    result = torch.empty(64, dtype=torch.uint8, device="cuda")
    net0 = YoloV2.create_network(np.reshape(V2_ANCHORS, [-1, 2]), names, False, input_shape=(416, 416, 3))
    weights = synth.darknet_stream(net0, seed=1, num_classes=80, head_gain=synth.HEAD_DEFAULTS["v2"][0], obj_bias=0.0)
    for batch in [int(v) for v in a.tail_batches.split(",") if v]:
        engs = []
        for _ in range(3):
            m = YoloV2()
            m.build(V2_ANCHORS, names, (416, 416, 3), dtype="fp16", max_batch=batch, weights=weights, streams=1)
            engs.append(m.net.engine)
        e_loss, e32, e16 = engs
        for e in (e32, e16):
            e.tail_train_init(*ytrain.split_tail(weights, net0))
        e16.set_wgrad_f16(True)
        x = torch.from_numpy(rng.randint(0, 256, size=(batch, 416, 416, 3)).astype(np.uint8)).cuda()
        arr, counts = yeval.pack_gts(random_truths(rng, batch, 8), 8)
        gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        lr_t = float(engine.adam_lr_t(1e-4, 1000))         # (a late step: small updates, the weights stay where they are)
        tail = lambda e: (lambda: _hip.check(lib.yolo_net_train_tail_step_u8(e.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8,
                                                                             e._tail_state.data_ptr(), lr_t, result.data_ptr(), st), "yolo_net_train_tail_step_u8"))
        arms = {"loss": lambda: _hip.check(lib.yolo_net_loss_u8(e_loss.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8, images.data_ptr(),
                                                                None, result.data_ptr(), st), "yolo_net_loss_u8"),
                "tail_step_float32": tail(e32), "tail_step_fp16": tail(e16)}
        ss = interleaved(arms, a.enqueues)
        steps["v2-416 tail b%d" % batch] = dict(ss, float32_over_loss=round(ss["tail_step_float32"]["median"] / ss["loss"]["median"], 3),
                                                fp16_over_loss=round(ss["tail_step_fp16"]["median"] / ss["loss"]["median"], 3),
                                                float32_over_fp16=round(ss["tail_step_float32"]["median"] / ss["tail_step_fp16"]["median"], 3),
                                                extra_bytes=int(e16._wgrad_f16_buf.numel()))
        del engs, e_loss, e32, e16
        torch.cuda.empty_cache()

    # ---- the blocks step of YOLOv3-608 in both modes beside the validation step ----------------------------------------------------------------
    net3 = YoloV3.create_network(np.reshape(V3_ANCHORS, [-1, 2]), names, False, input_shape=(608, 608, 3))
    R, _ = engine.v3_loss_rows(engine.head_desc_v3(net3[-1].yolos))
    weights3 = synth.darknet_stream(net3, seed=1, num_classes=80)
    heads, blocks = ytrain.head_convs_v3(net3), ytrain.block_convs_v3(net3)
    for batch in [int(v) for v in a.blocks_batches.split(",") if v]:
        engs = []
        for _ in range(3):
            m = YoloV3()
            m.build(V3_ANCHORS, names, (608, 608, 3), dtype="fp16", max_batch=batch, weights=weights3, streams=1)
            engs.append(m.net.engine)
        e_loss, e32, e16 = engs
        for e in (e32, e16):
            e.blocks_train_init_v3(ytrain.split_blocks(weights3, blocks), *ytrain.split_heads(weights3, heads))
        e16.set_wgrad_f16(True)
        x = torch.from_numpy(rng.randint(0, 256, size=(batch, 608, 608, 3)).astype(np.uint8)).cuda()
        lay = e32.blocks_layout_v3
        parts = torch.empty(int(lay.images_offset - lay.parts_offset), dtype=torch.uint8, device="cuda")
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        table = torch.empty(batch * R, dtype=torch.int32, device="cuda")
        lr_t = float(engine.adam_lr_t(1e-5, 1000))
        arr, counts = yeval.pack_gts(random_truths(rng, batch, 8), 8)
        gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
        blk = lambda e: (lambda: _hip.check(lib.yolo_net_train_blocks_step_v3_u8(e.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8, 0.7,
                                                                                 e._blocks_state_v3.data_ptr(), lr_t, result.data_ptr(), st),
                                            "yolo_net_train_blocks_step_v3_u8"))
        arms = {"loss": lambda: _hip.check(lib.yolo_net_loss_v3_u8(e_loss.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), 8, 0.7, parts.data_ptr(),
                                                                   images.data_ptr(), table.data_ptr(), result.data_ptr(), st), "yolo_net_loss_v3_u8"),
                "blocks_step_float32": blk(e32), "blocks_step_fp16": blk(e16)}
        ss = interleaved(arms, a.enqueues)
        steps["v3-608 blocks b%d" % batch] = dict(ss, float32_over_loss=round(ss["blocks_step_float32"]["median"] / ss["loss"]["median"], 3),
                                                  fp16_over_loss=round(ss["blocks_step_fp16"]["median"] / ss["loss"]["median"], 3),
                                                  float32_over_fp16=round(ss["blocks_step_float32"]["median"] / ss["blocks_step_fp16"]["median"], 3),
                                                  extra_bytes=int(e16._wgrad_f16_buf.numel()))
        del engs, e_loss, e32, e16
        torch.cuda.empty_cache()

    res = {"gpu": torch.cuda.get_device_name(0), "yolo_conv3x3_wgrad_f16_vs_float32_us": ops, "steps_us": steps,
           "f16_matrix_peak_tflops": F16_MATRIX_PEAK_TFLOPS, "f32_matrix_peak_tflops": F32_MATRIX_PEAK_TFLOPS,
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "kernel_enqueues_per_round": a.kernel_enqueues, "warmup_enqueues": a.warmup,
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; arms alternating round by round"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

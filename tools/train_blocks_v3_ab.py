"""Device time of training the 3 x 3 blocks behind the YOLOv3 heads: the sparse data gradient yolo_v3_head_dgrad against the dense route on
the same data, yolo_conv3x3_wgrad at the head-block shapes, and yolo_net_train_blocks_step_v3_u8 against yolo_net_train_head_step_v3_u8 and
yolo_net_loss_v3_u8 (whose code this change does not touch) in one interleaved run.

    python tools/train_blocks_v3_ab.py [--rounds 7] [--enqueues 6] [--kernel-enqueues 20] [--warmup 3] [--batches 16,32] [--truths 0,8,64]
                                       [--out profiles/train_blocks_v3.json]

One process, one GPU.  Every figure is the time between two hipEvents around back-to-back enqueues (no host wait in between), divided by
the enqueues; `rounds` such figures per arm, the arms alternating round by round, reported as median and min - max.

  dgrad   per scale of YOLOv3-608 (COCO heads: 255 x 1024 / 512 / 256 on 19^2 / 38^2 / 76^2), fp16 Y dense, G and the assign table of
          yolo_v3_loss_grad on random logits with `truths` truths per image.  (a) sparse: yolo_v3_head_dgrad on G in place.  (b) dense: a
          gather of G_s [P_s][255] out of G (torch.index_select-free: a strided copy of the scale's rows) and yolo_conv1x1_dgrad on it;
          the gather is timed with it and alone.  The byte floor: Y_s once + D_s once + a 128-byte line per row of G + the table, at the
          project's measured 6.29 TB/s.
  wgrad   yolo_conv3x3_wgrad alone at the three YOLOv3-608 head-block shapes and the two YOLOv3-tiny-416 ones, with the scale: both
          kernels.  The rate counts 2 * P * cout * 9 * cin FLOP against the 157.3 TFLOP/s float32 matrix peak of the MI355X.
  step    YOLOv3-608, fp16 plan, one stream part, synthetic weights, uint8 batches.  Three nets of the same weights, one per arm.

Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
F32_MATRIX_PEAK_TFLOPS = 157.3
HBM_TB_PER_S = 6.29
WGRAD_SHAPES = (("v3-608 19^2", 19, 512, 1024), ("v3-608 38^2", 38, 256, 512), ("v3-608 76^2", 76, 128, 256), ("v3-tiny-416 13^2", 13, 256, 512),
                ("v3-tiny-416 26^2", 26, 384, 256))


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
    ap.add_argument("--kernel-enqueues", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="16,32")
    ap.add_argument("--truths", default="0,8,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_blocks_v3.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import YoloV3, _hip
    from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth, train as ytrain
    assert torch.cuda.is_available(), "tools/train_blocks_v3_ab.py measures on the GPU"
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
    truth_counts = [int(v) for v in a.truths.split(",")]
    names = ["c%d" % i for i in range(80)]
    net0 = YoloV3.create_network(np.reshape(V3_ANCHORS, [-1, 2]), names, False, input_shape=(608, 608, 3))
    hd = engine.head_desc_v3(net0[-1].yolos)
    R, _ = engine.v3_loss_rows(hd)
    width, cins, grids = 85, (1024, 512, 256), (19, 38, 76)
    row0 = [0, 19 * 19 * 3, (19 * 19 + 38 * 38) * 3]
    dgrad, wgrad, step = {}, {}, {}

    # ---- the data gradient, sparse against dense, per scale ---------------------------------------------------------------------------------
    for batch in batches:
        for n_truths in truth_counts:
            logits = torch.from_numpy(rng.randn(batch, R, width).astype(np.float32)).cuda()
            _, _, assign, grad, keep = engine.v3_loss_grad(hd, logits, yeval.pack_gts(random_truths(rng, batch, n_truths), max(n_truths, 1)))
            max_gt = max(n_truths, 1)
            torch.cuda.synchronize()
            winners = int(((assign >= 0) & (assign < max_gt)).sum())
            for s, (g, cin) in enumerate(zip(grids, cins)):
                P, cout = batch * g * g, 3 * width
                W = torch.from_numpy((rng.randn(cout, cin) * 0.03).astype(np.float32)).cuda()
                Y = torch.from_numpy(rng.randn(batch, g, g, cin).astype(np.float16)).cuda()
                D = torch.empty(P * cin, dtype=torch.float32, device="cuda")
                Gs = torch.empty((P, cout), dtype=torch.float32, device="cuda")
                rows = grad[:, row0[s]:row0[s] + g * g * 3]
                gather = lambda: Gs.view(batch, g * g * 3, width).copy_(rows)
                sparse = lambda: _hip.check(lib.yolo_v3_head_dgrad(hd, s, grad.data_ptr(), assign.data_ptr(), max_gt, batch, W.data_ptr(), cin, Y.data_ptr(),
                                                                   _hip.DTYPE_F16, cin, 0, g * g * cin, 0.1, D.data_ptr(), st), "yolo_v3_head_dgrad")
                dense_only = lambda: _hip.check(lib.yolo_conv1x1_dgrad(Gs.data_ptr(), cout, W.data_ptr(), cin, Y.data_ptr(), _hip.DTYPE_F16, cin, 0, g * g * cin,
                                                                       g * g, batch, 0.1, D.data_ptr(), st), "yolo_conv1x1_dgrad")

                def dense():
                    gather()
                    dense_only()
                ss = interleaved({"sparse": sparse, "dense_with_gather": dense, "gather": gather}, a.kernel_enqueues)
                floor_bytes = P * cin * 2 + P * cin * 4 + P * 3 * 128 + P * 3 * 4
                floor_us = floor_bytes / (HBM_TB_PER_S * 1e6)
                pl = _hip.head_dgrad_plan(hd, s, cin, batch)
                dgrad["b%d_t%d_s%d" % (batch, n_truths, s)] = dict(
                    ss, positions=P, cin=cin, winner_rows_all_scales=winners, floor_bytes=floor_bytes, floor_us=round(floor_us, 2),
                    sparse_over_floor=round(ss["sparse"]["median"] / floor_us, 2),
                    sparse_over_dense=round(ss["sparse"]["median"] / ss["dense_with_gather"]["median"], 3),
                    dense_gflop=round(2.0 * P * 256 * cin * 1e-9, 2), workgroups=pl["workgroups"], rounds=pl["rounds"])
                del W, Y, D, Gs
            del logits, assign, grad, keep
            torch.cuda.empty_cache()

    # ---- the 3 x 3 weight gradient at the head-block shapes --------------------------------------------------------------------------------------
    for batch in batches:
        for name, g, cin3, cout3 in WGRAD_SHAPES:
            P = batch * g * g
            pl = _hip.conv3x3_wgrad_plan(g, g, batch, cin3, cout3)
            X3 = torch.from_numpy(rng.randn(P, cin3).astype(np.float16)).cuda()
            D3 = torch.from_numpy(rng.randn(P, cout3).astype(np.float32)).cuda()
            scale = torch.from_numpy(rng.uniform(0.5, 2.0, size=cout3).astype(np.float32)).cuda()
            dw = torch.empty(cout3 * 9 * cin3, dtype=torch.float32, device="cuda")
            db = torch.empty(cout3, dtype=torch.float32, device="cuda")
            scratch = torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda")
            fn = lambda: _hip.check(lib.yolo_conv3x3_wgrad(X3.data_ptr(), _hip.DTYPE_F16, cin3, 0, g * g * cin3, g, g, batch, cin3, D3.data_ptr(), cout3,
                                                           scale.data_ptr(), dw.data_ptr(), db.data_ptr(), scratch.data_ptr(), scratch.numel(), st),
                                    "yolo_conv3x3_wgrad")
            ws = interleaved({"wgrad": fn}, max(2, a.kernel_enqueues // 2))["wgrad"]
            flop = 2.0 * P * cout3 * 9 * cin3
            tflops = flop / ws["median"] * 1e-6
            wgrad["b%d %s %d->%d" % (batch, name, cin3, cout3)] = dict(
                ws, chunks=pl["n_chunks"], positions_per_chunk=pl["positions_per_chunk"], halo_rows=pl["halo_rows"],
                workgroups=pl["tiles_cout"] * pl["tiles_cin"] * pl["n_chunks"], scratch_bytes=pl["scratch_bytes"], gflop=round(flop * 1e-9, 3),
                tflops=round(tflops, 2), percent_of_f32_matrix_peak=round(100.0 * tflops / F32_MATRIX_PEAK_TFLOPS, 1))
            del X3, D3, scale, dw, db, scratch
            torch.cuda.empty_cache()

    # ---- the steps ------------------------------------------------------------------------------------------------------------------------------
    weights = synth.darknet_stream(net0, seed=1, num_classes=80)
    heads, blocks = ytrain.head_convs_v3(net0), ytrain.block_convs_v3(net0)
    for batch in batches:
        engs = []
        for _ in range(3):
            m = YoloV3()
            m.build(V3_ANCHORS, names, (608, 608, 3), dtype="fp16", max_batch=batch, weights=weights, streams=1)
            engs.append(m.net.engine)
        e_loss, e_head, e_blocks = engs
        e_head.head_train_init_v3(*ytrain.split_heads(weights, heads))
        e_blocks.blocks_train_init_v3(ytrain.split_blocks(weights, blocks), *ytrain.split_heads(weights, heads))
        x = torch.from_numpy(rng.randint(0, 256, size=(batch, 608, 608, 3)).astype(np.uint8)).cuda()
        lay = e_blocks.blocks_layout_v3
        parts = torch.empty(int(e_head.train_layout_v3.images_offset - e_head.train_layout_v3.parts_offset), dtype=torch.uint8, device="cuda")
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        table = torch.empty(batch * R, dtype=torch.int32, device="cuda")
        result = torch.empty(64, dtype=torch.uint8, device="cuda")
        lr_t = float(engine.adam_lr_t(1e-5, 1000))         # (a late step: small updates, the weights stay where they are)
        for n_truths in truth_counts:
            max_gt = max(n_truths, 1)
            arr, counts = yeval.pack_gts(random_truths(rng, batch, n_truths), max_gt)
            gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
            arms = {"loss": lambda: _hip.check(lib.yolo_net_loss_v3_u8(e_loss.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), max_gt, 0.7,
                                                                       parts.data_ptr(), images.data_ptr(), table.data_ptr(), result.data_ptr(), st), "yolo_net_loss_v3_u8"),
                    "head_step": lambda: _hip.check(lib.yolo_net_train_head_step_v3_u8(e_head.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), max_gt,
                                                                                       0.7, e_head._train_state_v3.data_ptr(), lr_t, result.data_ptr(), st),
                                                    "yolo_net_train_head_step_v3_u8"),
                    "blocks_step": lambda: _hip.check(lib.yolo_net_train_blocks_step_v3_u8(e_blocks.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(),
                                                                                           max_gt, 0.7, e_blocks._blocks_state_v3.data_ptr(), lr_t,
                                                                                           result.data_ptr(), st), "yolo_net_train_blocks_step_v3_u8")}
            ss = interleaved(arms, a.enqueues)
            step["b%d_t%d" % (batch, n_truths)] = dict(
                ss, blocks_minus_head_at_median=round(ss["blocks_step"]["median"] - ss["head_step"]["median"], 3),
                blocks_minus_loss_at_median=round(ss["blocks_step"]["median"] - ss["loss"]["median"], 3),
                blocks_over_loss=round(ss["blocks_step"]["median"] / ss["loss"]["median"], 3),
                loss_spread=round(ss["loss"]["max"] - ss["loss"]["min"], 3), state_bytes=int(lay.total_bytes), scratch_bytes=int(lay.scratch_bytes))
        del engs, e_loss, e_head, e_blocks
        torch.cuda.empty_cache()
    res = {"gpu": torch.cuda.get_device_name(0), "network": "YOLOv3-608 fp16, COCO heads 255 x 1024 / 512 / 256, blocks 3 x 3 512 -> 1024, 256 -> 512, 128 -> 256",
           "yolo_v3_head_dgrad_vs_dense_us": dgrad, "yolo_conv3x3_wgrad_us": wgrad, "steps_us": step, "f32_matrix_peak_tflops": F32_MATRIX_PEAK_TFLOPS,
           "hbm_tb_per_s": HBM_TB_PER_S,
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "kernel_enqueues_per_round": a.kernel_enqueues, "warmup_enqueues": a.warmup,
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; arms alternating round by round"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

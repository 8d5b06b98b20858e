"""Device time of training the YOLOv3 head convs: the sparse weight gradient yolo_v3_head_wgrad against the dense route through
yolo_conv1x1_wgrad, and yolo_net_train_head_step_v3_u8 against yolo_net_loss_v3_u8 on the same build.

    python tools/train_v3_ab.py [--rounds 7] [--enqueues 20] [--kernel-enqueues 50] [--warmup 5] [--truths 0,8,64]
                                [--cases yolov3-608:16,yolov3-608:32,yolov3-tiny-416:64] [--limit 300] [--out profiles/train_head_v3.json]

The driver touches no GPU: every (case, part) is a child process of its own under `timeout`, one after the other, and the first one that
fails ends the run (what the children before it measured is still written).  A child is this file with --child.

Every figure is the time between two hipEvents around back-to-back enqueues (no host wait in between), divided by the enqueues; `rounds`
such figures per arm, the arms alternating round by round, reported as median and min - max.  fp16 plans, one stream part, synthetic
weights; G and the assign table come from yolo_v3_loss_grad on N(0, 1) logits with the given number of random truths per image.

  wgrad   (a) sparse: yolo_v3_head_wgrad on dense fp16 X_s, all scales in one call (four kernels).
          (b) dense:  one yolo_conv1x1_wgrad per scale on a dense G_s [P_s][cout_s] gathered beforehand (the gather is not timed): the route
              the older kernel would take, six kernels.
          byte floor of (a): every X_s read once plus one 128-byte line per row of G (a row is 340 bytes at C = 80: every row's element 4
              lies in a line of its own), over the 6.29 TB/s this project measured as the HBM peak.
  step    (c) yolo_net_train_head_step_v3_u8 against yolo_net_loss_v3_u8: the difference of the medians is what training the heads adds to
              a validation step (the gradient kernel, the four weight-gradient kernels, one Adam + re-pack kernel per scale).

Writes the JSON to --out and prints it as one line."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 6.29e12
V3_ANCHORS = [10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326]
TINY_ANCHORS = [10, 14, 23, 27, 37, 58, 81, 82, 135, 169, 344, 319]
NETS = {"yolov3-608": ("v3", V3_ANCHORS, 608), "yolov3-tiny-416": ("v3-tiny", TINY_ANCHORS, 416)}


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def random_truths(rng, batch, n):
    return [[(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), int(rng.randint(0, 80)), 0) for _ in range(n)]
            for _ in range(batch)]


def child(a):
    import torch
    from tensorflow_yolo_amd import YoloV3, YoloV3Tiny, _hip
    from tensorflow_yolo_amd.net import engine, evaluate as yeval, synth, train as ytrain
    assert torch.cuda.is_available(), "tools/train_v3_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    lib = _hip.lib()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(7)
    name, batch = a.case.split(":")
    batch = int(batch)
    version, anchors, size = NETS[name]
    cls = YoloV3Tiny if version == "v3-tiny" else YoloV3
    names = ["c%d" % i for i in range(80)]
    truth_counts = [int(v) for v in a.truths.split(",")]

    def timed_us(fn, enqueues):
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
        keys = list(arms)
        t = {k: [] for k in keys}
        for r in range(a.rounds):
            for k in (keys if r % 2 == 0 else keys[::-1]):
                t[k].append(timed_us(arms[k], enqueues))
        return {k: stats(v) for k, v in t.items()}

    net = cls.create_network(np.reshape(anchors, [-1, 2]), names, False, input_shape=(size, size, 3))
    heads = ytrain.head_convs_v3(net)
    out = {}
    if a.part == "wgrad":
        from tensorflow_yolo_amd.net.layers import yolo_layer
        hd = engine.head_desc_v3([l for l in net if isinstance(l, yolo_layer)])
        ns, width = hd.n_scales, 5 + hd.n_classes
        cins = [cin for _, _, cin in heads]
        rows, _ = engine.v3_loss_rows(hd)
        xs = [torch.from_numpy(rng.randn(batch, hd.h[s], hd.w[s], cins[s]).astype(np.float16)).cuda() for s in range(ns)]
        pl = _hip.v3_head_wgrad_plan(hd, cins, batch)
        x_bytes = sum(x.numel() * 2 for x in xs)
        floor = x_bytes + batch * rows * 128
        for n in truth_counts:
            logits = torch.from_numpy(rng.randn(batch, rows, width).astype(np.float32)).cuda()
            _, _, assign, grad, keep = engine.v3_loss_grad(hd, logits, yeval.pack_gts(random_truths(rng, batch, n), max(n, 1)))
            torch.cuda.synchronize()
            max_gt = max(n, 1)
            dws, dbs, scratch = engine.v3_head_wgrad(hd, xs, grad, assign, max_gt)
            sparse = lambda: engine.v3_head_wgrad(hd, xs, grad, assign, max_gt, scratch=scratch, out=(dws, dbs))
            dense_calls, row0 = [], 0
            for s in range(ns):
                ppi, cout = hd.h[s] * hd.w[s], hd.n_anchors[s] * width
                gs = grad[:, row0:row0 + ppi * hd.n_anchors[s]].reshape(batch * ppi, cout).contiguous()
                row0 += ppi * hd.n_anchors[s]
                p1 = _hip.wgrad_plan(batch * ppi, cins[s], cout)
                dw = torch.empty(cout * cins[s], dtype=torch.float32, device="cuda")
                db = torch.empty(cout, dtype=torch.float32, device="cuda")
                sc = torch.empty(p1["scratch_bytes"], dtype=torch.uint8, device="cuda")
                dense_calls.append((xs[s], cins[s], ppi, gs, cout, dw, db, sc))

            def dense():
                for x, cin, ppi, gs, cout, dw, db, sc in dense_calls:
                    _hip.check(lib.yolo_conv1x1_wgrad(x.data_ptr(), _hip.DTYPE_F16, cin, 0, ppi * cin, ppi, batch, cin, gs.data_ptr(), cout,
                                                      dw.data_ptr(), db.data_ptr(), sc.data_ptr(), sc.numel(), st), "yolo_conv1x1_wgrad")

            ss = interleaved({"sparse": sparse, "dense": dense}, a.kernel_enqueues)
            # the two routes agree where the dense one's structural zeros are zeros (they are: G comes from yolo_v3_loss_grad)
            sparse(); dense(); torch.cuda.synchronize()
            worst = max(float((dws[s].reshape(-1) - dense_calls[s][5]).abs().max()) for s in range(ns))
            winners = int((assign >= 0).sum())
            out["truths%d" % n] = dict(ss, winners=winners, ignored=int((assign == -2).sum()), largest_abs_difference_of_the_routes=worst,
                                       dense_over_sparse_at_median=round(ss["dense"]["median"] / ss["sparse"]["median"], 2),
                                       sparse_over_floor=round(ss["sparse"]["median"] / (floor / HBM_PEAK * 1e6), 2))
        out["plan"] = {k: pl[k] for k in ("positions", "positions_per_chunk", "n_chunks", "obj_workgroups", "win_workgroups", "scratch_bytes")}
        out["x_bytes"], out["floor_bytes"], out["floor_us"] = x_bytes, floor, round(floor / HBM_PEAK * 1e6, 2)
        out["dense_gflop"] = round(sum(2.0 * batch * hd.h[s] * hd.w[s] * hd.n_anchors[s] * width * cins[s] for s in range(ns)) * 1e-9, 3)
    else:
        m = cls()
        weights = synth.darknet_stream(net, seed=1, num_classes=80)
        m.build(anchors, names, (size, size, 3), dtype="fp16", max_batch=batch, weights=weights, streams=1)
        eng = m.net.engine
        eng.head_train_init_v3(*ytrain.split_heads(weights, heads))
        rows, parts = engine.v3_loss_rows(eng.head)
        x = torch.from_numpy(rng.randint(0, 256, size=(batch, size, size, 3)).astype(np.uint8)).cuda()
        images = torch.empty(batch * 56, dtype=torch.uint8, device="cuda")
        d_parts = torch.empty(batch * parts * 56, dtype=torch.uint8, device="cuda")
        assign = torch.empty(batch * rows, dtype=torch.int32, device="cuda")
        result = torch.empty(64, dtype=torch.uint8, device="cuda")
        lr_t = float(engine.adam_lr_t(1e-4, 1000))         # (a late step: small updates, the weights stay where they are)
        for n in truth_counts:
            max_gt = max(n, 1)
            arr, counts = yeval.pack_gts(random_truths(rng, batch, n), max_gt)
            gt, gc = torch.from_numpy(arr.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(counts).cuda()
            arms = {"loss": lambda: _hip.check(lib.yolo_net_loss_v3_u8(eng.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(), max_gt, 0.7,
                                                                       d_parts.data_ptr(), images.data_ptr(), assign.data_ptr(), result.data_ptr(), st),
                                               "yolo_net_loss_v3_u8"),
                    "train_step": lambda: _hip.check(lib.yolo_net_train_head_step_v3_u8(eng.handle, x.data_ptr(), batch, gt.data_ptr(), gc.data_ptr(),
                                                                                        max_gt, 0.7, eng._train_state_v3.data_ptr(), lr_t,
                                                                                        result.data_ptr(), st), "yolo_net_train_head_step_v3_u8")}
            ss = interleaved(arms, a.enqueues)
            diff = round(ss["train_step"]["median"] - ss["loss"]["median"], 3)
            out["truths%d" % n] = dict(ss, step_minus_loss_at_median=diff, loss_spread=round(ss["loss"]["max"] - ss["loss"]["min"], 3),
                                       percent_of_the_loss_step=round(100.0 * diff / ss["loss"]["median"], 2))
    out["gpu"] = torch.cuda.get_device_name(0)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--enqueues", type=int, default=20)
    ap.add_argument("--kernel-enqueues", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--truths", default="0,8,64")
    ap.add_argument("--cases", default="yolov3-608:16,yolov3-608:32,yolov3-tiny-416:64")
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_head_v3.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--case")
    ap.add_argument("--part", choices=("wgrad", "step"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"yolo_v3_head_wgrad_vs_dense_us": {}, "yolo_net_train_head_step_v3_u8_vs_yolo_net_loss_v3_u8_us": {},
           "method": {"rounds": a.rounds, "enqueues_per_round": a.enqueues, "kernel_enqueues_per_round": a.kernel_enqueues, "warmup_enqueues": a.warmup,
                      "hbm_peak_bytes_per_s": HBM_PEAK, "network": "fp16 plans, COCO heads (C = 80), synthetic weights, one stream part",
                      "time": "hipEvents around back-to-back enqueues on one stream, per enqueue; arms alternating round by round; one child "
                              "process per case and part"}}
    failed = None
    for case in a.cases.split(","):
        for part, key in (("wgrad", "yolo_v3_head_wgrad_vs_dense_us"), ("step", "yolo_net_train_head_step_v3_u8_vs_yolo_net_loss_v3_u8_us")):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", "--case", case, "--part", part,
                   "--rounds", str(a.rounds), "--enqueues", str(a.enqueues), "--kernel-enqueues", str(a.kernel_enqueues), "--warmup", str(a.warmup),
                   "--truths", a.truths]
            print("train_v3_ab: %s %s ..." % (case, part), file=sys.stderr, flush=True)
            run = subprocess.run(cmd, capture_output=True, text=True)
            lines = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
            if run.returncode != 0 or not lines:
                failed = {"case": case, "part": part, "exit_status": run.returncode, "stderr_tail": run.stderr[-2000:]}
                break
            got = json.loads(lines[-1][len("RESULT "):])
            res["gpu"] = got.pop("gpu")
            res[key][case.replace(":", "_b")] = got
        if failed:
            break
    if failed:
        res["failed"] = failed      # nothing more was started on the GPU after it
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

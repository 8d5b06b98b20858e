"""Do two builds of libyolo_hip.so compute the same bits?  For a host-side refactor: the parent commit's library against the tree's.

    python tools/lib_identity.py build_ab/lib_prev.so tensorflow-yolo_amd/libyolo_hip.so [--timeout 240] [--out bench_out/lib_identity.json]

Three fresh child processes, one at a time, each with YOLO_HIP_LIB set and under its own time limit: library A, library A again,
library B.  The run stops at the first child that does not exit 0.  A child (--child) runs the fixed list of small cases below --
synthetic weights and inputs (net/synth.py), every path of the forward engine, no timing-dependent choice: no autotune, streams given
explicitly -- and prints one SHA-256 per case over the raw bytes of the results (logits; of a detect call the boxes below each count,
the counts and the status words; the times of forward_timed are not hashed; of the three training paths the state, the device weights,
the loss records and the arrays read back: train_cases).  The parent process compares the lists:

  * A against A: a case on which a library disagrees with itself is listed and left out of the second comparison.  That list must stay
    below a tenth of the cases and hold no single-stream `forward` case -- those are deterministic by design (fixed split order, no
    float atomics);
  * A against B on the remaining cases: every hash equal, or the exit status is 1.

Prints the table, writes the JSON to --out."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spp_ref
    from oracle import cases
    from tensorflow_yolo_amd import _hip
    from tensorflow_yolo_amd.net import base, engine, synth, v2, v3
    assert torch.cuda.is_available(), "tools/lib_identity.py runs on the GPU"
    torch.cuda.set_device(0)
    names = ["c%d" % i for i in range(80)]
    out = []

    def emit(case, *arrays):
        h = hashlib.sha256()
        for a in arrays:
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            h.update(np.ascontiguousarray(a).tobytes())
        out.append((case, h.hexdigest()))

    def records(rec):
        boxes, counts, status = (t.cpu().numpy() for t in rec)
        return [boxes[i, :max(0, int(counts[i]))] for i in range(len(counts))] + [counts, status]

    def build(kind, size, dtype, batch, **kw):
        """(HipNetwork with synthetic weights, float32 input, its uint8 twin's bytes)"""
        hw = (size, size, 3)
        if kind == "v3":
            layers = v3.create_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), names, False, input_shape=hw)
        elif kind == "v3-spp":
            layers = v3.create_spp_network(np.reshape(cases.COCO_V3_ANCHORS, [-1, 2]), names, False, input_shape=hw)
        elif kind == "v3-tiny":
            layers = v3.create_tiny_network(np.reshape(spp_ref.TINY_V3_ANCHORS, [-1, 2]), names, False, input_shape=hw)
        elif kind == "v2":
            layers = v2.create_full_network(np.reshape(cases.COCO_V2_ANCHORS, [-1, 2]), names, False, input_shape=hw)
        else:
            layers = v2.create_tiny_network(np.reshape(cases.VOC_TINY_ANCHORS, [-1, 2]), names[:20], False, input_shape=hw)
        ncls = 20 if kind == "v2-tiny" else 80
        net = engine.HipNetwork(layers, dtype=dtype, max_batch=batch, **kw)
        net.load_weights(synth.darknet_stream(layers, seed=1, obj_bias=-2.0, num_classes=ncls, head_gain=synth.HEAD_DEFAULTS[kind][0]))
        if kind.startswith("v2"):
            h, w, _ = layers[-1].out.hwc
            anchors = cases.VOC_TINY_ANCHORS if kind == "v2-tiny" else cases.COCO_V2_ANCHORS
            net.set_head(engine.head_desc_v2(h, w, anchors, ncls))
        xu = np.random.RandomState(2).randint(0, 256, size=(batch,) + hw).astype(np.uint8)
        return net, (xu / 255.).astype(np.float32), xu

    def five(tag, net, x, xu):
        emit(tag + " forward", net.forward(x))
        emit(tag + " forward_u8", net.forward_u8(xu))
        emit(tag + " detect", *records(net.detect(x, 0.3, 0.5)))
        emit(tag + " detect_u8", *records(net.detect_u8(xu, 0.3, 0.5)))
        logits = torch.zeros((x.shape[0],) + tuple(net.output_shape), dtype=torch.float32, device=net.device)
        net.forward_timed(x, out=logits)
        emit(tag + " forward_timed", logits)

    for dtype in ("fp16", "fp32", "mxfp8"):
        for batch in (2, 6):
            net, x, xu = build("v3", 160, dtype, batch, streams=1)
            five("v3-160 %s b%d" % (dtype, batch), net, x, xu)
            net.close()
    for streams in (2, 3):
        net, x, xu = build("v3", 160, "fp16", 6, streams=streams)
        for b in (6, 2):        # 2: fits one arena
            emit("v3-160 fp16 max6 streams%d b%d forward" % (streams, b), net.forward(x[:b]))
            emit("v3-160 fp16 max6 streams%d b%d detect" % (streams, b), *records(net.detect(x[:b], 0.3, 0.5)))
        net.close()
    for kind, size, dtype, batch in [("v2", 160, "fp16", 3), ("v2", 160, "fp32", 3), ("v2-tiny", 416, "fp32", 2), ("v3-tiny", 160, "fp16", 2),
                                     ("v3-spp", 160, "fp16", 2)]:
        net, x, xu = build(kind, size, dtype, batch, streams=1)
        five("%s-%d %s b%d" % (kind, size, dtype, batch), net, x, xu)
        net.close()
    net, x, xu = build("v3", 160, "fp16", 2, keep_all=True)
    net.forward(x)
    torch.cuda.synchronize()
    held = {}
    for i in range(1, len(net.layers) - 1):
        try:
            held[i] = net.read_layer(i, 2)
        except _hip.YoloHipError:       # fused away: no tensor of its own
            pass
    ids = sorted(held)
    emit("v3-160 fp16 b2 keep_all read_layer x3", *[held[i] for i in (ids[0], ids[len(ids) // 2], ids[-1])])
    net.close()
    net, x, xu = build("v3", 160, "fp16", 4, streams=1)
    rng = np.random.RandomState(3)
    frames = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in ((120, 200), (333, 111), (160, 160), (481, 640))]
    for mode, resize in (("stretch", _hip.RESIZE_STRETCH), ("letterbox", _hip.RESIZE_LETTERBOX)):
        emit("v3-160 fp16 b4 detect_frames " + mode, *records(net.detect_frames(frames, 0.3, 0.5, resize=resize)))
    logits = net.forward(x)
    for cap in (4096, 16384):
        recs, status = engine.decode_nms(net.head, logits, 0.3, 0.5, cand_capacity=cap, allow_truncation=True)
        emit("decode_nms cap%d" % cap, np.array([r for img in recs for r in img], dtype=np.float64).reshape(-1, 6), [len(img) for img in recs], status)
    net.close()
    rng = np.random.RandomState(4)
    boxes = [base.BoundingBox(*rng.uniform(0.05, 0.95, 2), *rng.uniform(0.02, 0.4, 2), 0, 0, int(rng.randint(0, 5)), float(np.float32(rng.randint(1, 50) / 50.)))
             for _ in range(300)]
    for per_class in (False, True):
        kept = base.non_maximum_suppression(boxes, 0.45, per_class=per_class)
        emit("nms_host 300 boxes " + ("per class" if per_class else "agnostic"), [boxes.index(b) for b in kept])
    train_cases(emit)
    torch.cuda.synchronize()
    print("HASHES " + json.dumps(out))


def train_cases(emit):
    """The three training paths on the smallest nets the GPU training tests use (tests/test_gpu_train*.py), fp16 and fp32, max_batch 3:
    *_train_init into a zeroed state, steps at batch 3, 1 (a smaller split inside a scratch sized for 3) and 3, one uint8 step.  Hashed:
    the whole state, the device weights (the trained layers' packed rows and biases are the bytes that move), the four loss records and
    the arrays of *_train_read."""
    import ctypes as C
    import numpy as np
    import torch
    import spp_ref
    import tail_cases
    from oracle import cases
    from tensorflow_yolo_amd import YoloV2, YoloV2Tiny, YoloV3Tiny, _hip
    from tensorflow_yolo_amd.net import engine, synth, train as ytrain

    class SmallTail(YoloV2):
        create_network = staticmethod(tail_cases.small_tail_network)

    B = 3
    names20, names3 = ["c%d" % i for i in range(20)], ["a", "b", "c"]
    rng = np.random.RandomState(7)
    truths = [[(rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.02, 0.9), rng.uniform(0.02, 0.9), int(rng.randint(0, 3))) for _ in range(n)]
              for n in (5, 0, 2)]       # (classes 0..2: valid for every head here; one image without a truth)
    ptrs = lambda arrays: (C.c_void_p * _hip.MAX_SCALES)(*[a.ctypes.data for a in arrays])
    for mode, cls, anchors, names, hw, lr in (("head", YoloV2Tiny, cases.VOC_TINY_ANCHORS, names20, (96, 160), 1e-3),
                                              ("tail", SmallTail, cases.VOC_TINY_ANCHORS, names20, (64, 64), 1e-4),
                                              ("heads", YoloV3Tiny, spp_ref.TINY_V3_ANCHORS, names3, (96, 160), 1e-3)):
        layers = cls.create_network(np.reshape(anchors, [-1, 2]), names, False, input_shape=hw + (3,))
        kw = {} if mode == "heads" else dict(head_gain=synth.HEAD_DEFAULTS["v2-tiny"][0], obj_bias=0.0)
        weights = synth.darknet_stream(layers, seed=41, num_classes=len(names), **kw)
        x8 = np.random.RandomState(42).randint(0, 256, size=(B,) + hw + (3,)).astype(np.uint8)
        xf = (x8 / 255.).astype(np.float32)
        for dtype in ("fp16", "fp32"):
            m = cls()
            m.build(anchors, names, hw + (3,), dtype=dtype, max_batch=B, weights=weights, streams=1)
            eng, lib = m.net.engine, _hip.lib()
            # init twice: the engine's own call allocates the state, the second one starts it again from zeroed bytes (the parts between
            # the arrays and the scratch are otherwise whatever the allocator returned)
            if mode == "head":
                args = [np.ascontiguousarray(a, dtype=np.float32) for a in ytrain.split_head(weights, *ytrain.head_counts(m.net)[:2])]
                st = eng.head_train_init(*args)
                again = lambda: lib.yolo_net_head_train_init(eng.handle, st.data_ptr(), st.numel(), *[a.ctypes.data for a in args])
                step, step_u8, read = eng.train_head_step, eng.train_head_step_u8, eng.head_train_read
            elif mode == "tail":
                args = [np.ascontiguousarray(a, dtype=np.float32) for a in ytrain.split_tail(weights, m.net)]
                st = eng.tail_train_init(*args)
                again = lambda: lib.yolo_net_tail_train_init(eng.handle, st.data_ptr(), st.numel(), *[a.ctypes.data for a in args])
                step, step_u8, read = eng.train_tail_step, eng.train_tail_step_u8, eng.tail_train_read
            else:
                ws, bs = ytrain.split_heads(weights, ytrain.head_convs_v3(m.net))
                ws, bs = [np.ascontiguousarray(a, dtype=np.float32) for a in ws], [np.ascontiguousarray(a, dtype=np.float32) for a in bs]
                st = eng.head_train_init_v3(ws, bs)
                again = lambda: lib.yolo_net_head_train_v3_init(eng.handle, st.data_ptr(), st.numel(), ptrs(ws), ptrs(bs))
                step, step_u8, read = eng.train_head_step_v3, eng.train_head_step_v3_u8, lambda: sum(eng.head_train_read_v3(), [])
            st.zero_()
            torch.cuda.synchronize()
            _hip.check(again(), "the second init")
            records = [step(xf[:b], truths[:b], engine.adam_lr_t(lr, t + 1)).clone() for t, b in enumerate((3, 1, 3))]
            records.append(step_u8(x8, truths, engine.adam_lr_t(lr, 4)).clone())
            torch.cuda.synchronize()
            tag = "train %s %s max3" % (mode, dtype)
            emit(tag + " state after b3 b1 b3 u8-b3", st)
            emit(tag + " device weights", eng._weights)
            emit(tag + " loss records x4", *records)
            emit(tag + " read", *read())
            m.net.engine.close()


def run_child(lib, timeout):
    env = dict(os.environ, YOLO_HIP_LIB=os.path.abspath(lib))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        print("child with %s did not finish in %d s: stopping" % (lib, timeout))
        sys.exit(124)
    lines = [l for l in r.stdout.splitlines() if l.startswith("HASHES ")]
    if r.returncode != 0 or not lines:
        print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
        print("child with %s exited %d: stopping" % (lib, r.returncode))
        sys.exit(r.returncode or 1)
    return json.loads(lines[-1][len("HASHES "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "lib_identity.json"))
    a = ap.parse_args()
    if a.child:
        return child()
    if len(a.libs) != 2:
        ap.error("two library files: the reference build and the build under test")
    a1, a2, b = (run_child(lib, a.timeout) for lib in (a.libs[0], a.libs[0], a.libs[1]))
    assert [c for c, _ in a1] == [c for c, _ in a2] == [c for c, _ in b], "the children ran different case lists"
    unstable = [c for (c, h1), (_, h2) in zip(a1, a2) if h1 != h2]
    differ = [c for (c, h1), (_, h2) in zip(a1, b) if h1 != h2 and c not in unstable]
    print("%-52s %-12s %-12s %s" % ("case", "A", "B", "verdict"))
    for (c, h1), (_, h2) in zip(a1, b):
        print("%-52s %-12s %-12s %s" % (c, h1[:12], h2[:12], "A differs from itself: left out" if c in unstable else "DIFFERENT" if h1 != h2 else "same"))
    single = [c for c in unstable if c.endswith(" forward") and "streams" not in c]
    ok = not differ and 10 * len(unstable) < len(a1) and not single
    res = dict(A=a.libs[0], B=a.libs[1], cases=len(a1), same=len(a1) - len(unstable) - len(differ), different=differ, a_differs_from_itself=unstable,
               single_stream_forward_unstable=single, identical=bool(ok), hashes=dict(A=a1, A_again=a2, B=b))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases: %d same, %d different, %d left out (A differs from itself)%s -> %s"
          % (len(a1), res["same"], len(differ), len(unstable), ", a single-stream forward among them" if single else "", "IDENTICAL" if ok else "NOT IDENTICAL"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

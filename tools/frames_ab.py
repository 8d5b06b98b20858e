"""A/B of the batched resize (yolo_preprocess_frames[_u8]: one launch for a batch of frames) against the per-image launches it replaces
in the TEST loop (yolo_preprocess_resize[_u8], which stay in the library).

    python tools/frames_ab.py [--frames 32] [--src 576x768] [--size 608] [--rounds 15] [--warmup 3] [--out profiles/frames_ab.json]

One process, one GPU, no network: `frames` seeded random frames of the source size are resized to size x size.  Four comparisons --
{uint8, float32 results} x {stretch: per-image launches against the batched one; letterbox: the batched launch alone, which has no
per-image counterpart, beside stretch} -- with the legs alternating inside every round:
  * device time: a hipEvent pair around the leg's launches (all 32 per-image launches between one pair);
  * host enqueue time: the host clock around the leg's ctypes calls, device idle before and not waited for inside.
Every figure is a median with min - max over the rounds; GB/s counts the bytes algorithmically moved -- every source frame read once,
the destination written once.  The condition of the TEST-loop switch is evaluated here: for both result types the batched launch must
not be slower than the per-image launches, in device time and in host time, each beyond the per-image leg's own round-to-round spread
(max - min).  The batched stretch result must equal the per-image one bit for bit.  Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--src", default="576x768")
    ap.add_argument("--size", type=int, default=608)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_ab.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import _hip
    assert torch.cuda.is_available(), "tools/frames_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    lib = _hip.lib()
    n, size = a.frames, a.size
    sh, sw = (int(v) for v in a.src.lower().split("x"))
    rng = np.random.default_rng(1)
    src = torch.from_numpy(rng.integers(0, 256, size=(n, sh, sw, 3), dtype=np.uint8)).cuda()
    descs = (_hip.Frame * n)()
    for i in range(n):
        descs[i] = _hip.Frame(src[i].data_ptr(), sh, sw, 3 * sw, 0)
    stream = torch.cuda.current_stream().cuda_stream
    dst = {True: torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda"),
           False: torch.empty((n, size, size, 3), dtype=torch.float32, device="cuda")}
    ptrs = {u8: [dst[u8][i].data_ptr() for i in range(n)] for u8 in dst}

    def per_image(u8):
        fn = lib.yolo_preprocess_resize_u8 if u8 else lib.yolo_preprocess_resize
        for i in range(n):
            rc = fn(descs[i].pixels_dev, sh, sw, 3 * sw, ptrs[u8][i], size, size, 0, stream)
            if rc:
                _hip.check(rc, "yolo_preprocess_resize")

    def batched(u8, mode):
        fn = lib.yolo_preprocess_frames_u8 if u8 else lib.yolo_preprocess_frames
        _hip.check(fn(descs, n, mode, dst[u8].data_ptr(), size, size, stream), "yolo_preprocess_frames")

    legs = {"per_image_stretch": lambda u8: per_image(u8), "batched_stretch": lambda u8: batched(u8, _hip.RESIZE_STRETCH),
            "batched_letterbox": lambda u8: batched(u8, _hip.RESIZE_LETTERBOX)}
    same = {}
    for u8 in (True, False):
        per_image(u8)
        torch.cuda.synchronize()
        want = dst[u8].clone()
        dst[u8].zero_()
        batched(u8, _hip.RESIZE_STRETCH)
        torch.cuda.synchronize()
        same["u8" if u8 else "f32"] = bool(torch.equal(want, dst[u8]))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev = {(k, u8): [] for k in legs for u8 in (True, False)}
    hst = {(k, u8): [] for k in legs for u8 in (True, False)}
    names = list(legs)
    for r in range(-a.warmup, a.rounds):
        order = names if r % 2 == 0 else names[::-1]
        for u8 in (True, False):
            for k in order:
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                legs[k](u8)
                t1 = time.perf_counter()
                e1.record()
                e1.synchronize()
                if r >= 0:
                    dev[(k, u8)].append(e0.elapsed_time(e1))
                    hst[(k, u8)].append((t1 - t0) * 1e3)
    res = {"gpu": torch.cuda.get_device_name(0), "workload": "%d frames %dx%d -> %dx%d" % (n, sh, sw, size, size),
           "batched_stretch_bit_identical_to_per_image": same, "launches": {"per_image_stretch": n, "batched_stretch": -(-n // _hip.FRAMES_PER_LAUNCH),
                                                                            "batched_letterbox": -(-n // _hip.FRAMES_PER_LAUNCH)},
           "method": {"rounds": a.rounds, "warmup_rounds": a.warmup,
                      "device_ms": "hipEvent pair around the leg's launches (the event pair's own cost is inside), device idle before, legs alternating",
                      "host_ms": "host clock around the leg's ctypes calls only",
                      "bytes": "source frames read once + destination written once; letterbox reads the same frames"}}
    ok = True
    for u8 in (True, False):
        key = "u8" if u8 else "f32"
        moved = n * (sh * sw * 3 + size * size * 3 * (1 if u8 else 4))
        out = {"bytes_moved": moved}
        for k in legs:
            d, h = stats(dev[(k, u8)]), stats(hst[(k, u8)])
            out[k] = {"device_ms": d, "host_enqueue_ms": h, "GBps_at_median_device_ms": round(moved / (d["median"] * 1e-3) / 1e9, 1)}
        p, b = out["per_image_stretch"], out["batched_stretch"]
        spread_d = p["device_ms"]["max"] - p["device_ms"]["min"]
        spread_h = p["host_enqueue_ms"]["max"] - p["host_enqueue_ms"]["min"]
        out["per_image_spread_ms"] = {"device": round(spread_d, 4), "host": round(spread_h, 4)}
        out["batched_no_slower_device"] = bool(b["device_ms"]["median"] <= p["device_ms"]["median"] + spread_d)
        out["batched_no_slower_host"] = bool(b["host_enqueue_ms"]["median"] <= p["host_enqueue_ms"]["median"] + spread_h)
        out["speedup_at_median"] = {"device": round(p["device_ms"]["median"] / b["device_ms"]["median"], 2),
                                    "host": round(p["host_enqueue_ms"]["median"] / b["host_enqueue_ms"]["median"], 2)}
        ok = ok and out["batched_no_slower_device"] and out["batched_no_slower_host"]
        res[key] = out
    res["batched_replaces_per_image_in_the_test_loop"] = bool(ok and all(same.values()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

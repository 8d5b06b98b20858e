"""Device time of the anchor k-means: yolo_anchor_kmeans on synthetic boxes, beside the yardstick and scikit-learn on the host.

    python tools/anchor_ab.py [--rounds 5] [--warmup 1] [--host-max 100000] [--yardstick-max 10000] [--out profiles/anchors.json]

One process, one GPU.  The data are log-normal(-1.5, 0.8) sizes clipped to [0.01, 1] (default_rng(0)), n = 1e4 / 1e5 / 1e6, k = 5 / 9, both
distances, n_init = 1 / 10, tolerate 0.005, max_iter 300, seed 0.  A figure is the time between two hipEvents around ONE call (the entry
synchronises with the host between batches of iterations, so the events span its host waits too: this is what a caller sees on the stream);
`rounds` figures per case in one interleaved run -- every round walks all the cases, the order reversed every other round -- reported as
median and min - max, with the iterations of the best restart and avg_iou.
Host legs, once each (they are not the product, only the scale): the NumPy yardstick (tests/anchor_ref.py; sequential Python, up to
--yardstick-max boxes, and whether its centres equal the device's bit for bit) and, where it is importable,
sklearn.cluster.KMeans(init="k-means++", n_init=10, algorithm="lloyd", tol=0.005) -- Euclidean only -- on the data up to --host-max boxes,
with wall time, iterations and avg_iou of each.  Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    v = [float(x) for x in v]
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def avg_iou(wh, centres):
    i = np.minimum(wh[:, None, 0], centres[None, :, 0]) * np.minimum(wh[:, None, 1], centres[None, :, 1])
    u = (wh[:, 0] * wh[:, 1])[:, None] + (centres[:, 0] * centres[:, 1])[None, :] - i
    return float((i / u).max(axis=1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-max", type=int, default=100000)
    ap.add_argument("--yardstick-max", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchors.json"))
    a = ap.parse_args()
    import torch
    from tensorflow_yolo_amd import _hip
    from tensorflow_yolo_amd.net import engine
    assert torch.cuda.is_available(), "tools/anchor_ab.py measures on the GPU"
    torch.cuda.set_device(0)
    sizes, ks, distances, inits = (10000, 100000, 1000000), (5, 9), ("euclidean", "iou"), (1, 10)
    data = {n: np.clip(np.random.default_rng(0).lognormal(-1.5, 0.8, size=(n, 2)), 0.01, 1.0) for n in sizes}
    dev = {n: torch.from_numpy(data[n]).cuda() for n in sizes}
    cases = [(n, k, d, r) for n in sizes for k in ks for d in distances for r in inits]
    bufs, info, times = {}, {}, {c: [] for c in cases}

    def call(c):
        n, k, d, r = c
        if c not in bufs:
            pl = engine.anchor_plan(n, k, _hip.anchor_distance(d), n_init=r)
            bufs[c] = (torch.empty(pl["scratch_bytes"], dtype=torch.uint8, device="cuda"), torch.empty(pl["result_bytes"], dtype=torch.uint8, device="cuda"),
                       torch.empty(n, dtype=torch.int32, device="cuda"))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res, _ = engine.anchor_kmeans(dev[n], k, _hip.anchor_distance(d), n_init=r, scratch=bufs[c][0], result=bufs[c][1], labels=bufs[c][2])
        e1.record()
        e1.synchronize()
        info[c] = {"n_iter_best": res["restarts"][res["best_restart"]]["n_iter"], "n_iter_all": [row["n_iter"] for row in res["restarts"]],
                   "avg_iou": round(res["avg_iou"], 6), "status": res["status"]}
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        for c in cases:
            call(c)
    for r in range(a.rounds):
        for c in (cases if r % 2 == 0 else cases[::-1]):
            times[c].append(call(c))
    device = {"n%d_k%d_%s_init%d" % c: dict(info[c], ms=stats(times[c])) for c in cases}

    host = {}
    import anchor_ref as ref
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        KMeans = None
    for n in sizes:
        if n > a.host_max:
            continue
        for k in ks:
            if n <= a.yardstick_max:
                t0 = time.perf_counter()
                y = ref.kmeans(data[n], k, ref.EUCLIDEAN, n_init=10)
                host["yardstick_n%d_k%d_euclidean_init10" % (n, k)] = {
                    "s": round(time.perf_counter() - t0, 3), "n_iter_best": y["restarts"][y["best_restart"]]["n_iter"], "avg_iou": round(y["avg_iou"], 6),
                    "equals_device": bool(np.array_equal(y["centres"][:k], engine.anchor_kmeans(dev[n], k, n_init=10)[0]["centres"][:k]))}
            if KMeans is not None:
                t0 = time.perf_counter()
                km = KMeans(n_clusters=k, init="k-means++", n_init=10, algorithm="lloyd", tol=0.005, random_state=0).fit(data[n])
                host["sklearn_n%d_k%d_euclidean_init10" % (n, k)] = {"s": round(time.perf_counter() - t0, 3), "n_iter_best": int(km.n_iter_),
                                                                    "avg_iou": round(avg_iou(data[n], km.cluster_centers_), 6)}
    res = {"gpu": torch.cuda.get_device_name(0), "yolo_anchor_kmeans": device, "host": host,
           "method": {"rounds": a.rounds, "warmup_rounds": a.warmup, "time": "hipEvents around one call each (the call's host waits included), "
                      "all cases interleaved round by round, order reversed every other round; host legs: wall time of one run",
                      "data": "log-normal(-1.5, 0.8) clipped to [0.01, 1], default_rng(0); tolerate 0.005, max_iter 300, seed 0",
                      "sklearn": "KMeans(init='k-means++', n_init=10, algorithm='lloyd', tol=0.005, random_state=0)" if KMeans else "not importable"}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Euclidean clusters of ragged scans on the GPU (GPU box only): how long ops.scan_clusters takes next to what a user does
today — `torch.cdist(c, c) <= r` per scan on the device, the matrix copied to the host, scipy's connected components.

    python tools/bench_clusters.py [--out profiles/clusters.json] [--repeats 20] [--yardstick-repeats 3]

Shapes (S scans of n points): (64, 2048), (8, 16384), (1, 32768), seeded.  Two inputs per shape:
    uniform    clouds uniform in [0, 1]^3, the radius twice the mean nearest-neighbour distance of the set (ops.knn_points,
               k = 1): a few dozen neighbours per point, few hits per row in the sweep
    two_blobs  half of every scan around (-2, 0, 0), half around (2, 0, 0), sigma 0.1, rows interleaved, radius 1: every pair
               inside a blob is an edge — the sweep unites at every candidate, its worst case
Per shape and input, warmed up, device-event time of one call, the median and the extremes:
    scan_clusters   one launch over the whole ragged set, outputs reused, max_points = n
    cdist_scipy     per scan the boolean matrix on the device, `.cpu()`, csr_matrix, connected_components(directed=False) —
                    wall-clock time (the host does most of it), synchronised before and after
The legs alternate.  `agreement` is the share of scans whose number of components equals scipy's: cdist works through a
matrix product at these sizes and rounds differently at the radius, so it is reported, not asserted; the kernel's own check
is tests/test_clusters_gpu.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

SHAPES = ((64, 2048), (8, 16384), (1, 32768))


def event_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def cdist_scipy(clouds, radius):
    """Components per scan the way a user gets them today."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    counts = []
    for c in clouds:
        near = (torch.cdist(c, c) <= radius).cpu().numpy()
        counts.append(connected_components(csr_matrix(near), directed=False)[0])
    return counts


def inputs(S, n):
    r = np.random.RandomState(S + n)
    uniform = r.uniform(0, 1, (S, n, 3)).astype(np.float32)
    blobs = r.normal(0, 0.1, (S, n, 3))
    blobs[:, 0::2, 0] -= 2.0
    blobs[:, 1::2, 0] += 2.0
    return {"uniform": uniform, "two_blobs": blobs.astype(np.float32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clusters.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--yardstick-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clusters.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    result = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for S, n in SHAPES:
        for what, host in inputs(S, n).items():
            clouds = torch.from_numpy(host).cuda()
            points = clouds.view(-1, 3)
            offsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * n
            if what == "uniform":
                radius = 2.0 * float(ops.knn_points(points, offsets, 1)[1].sqrt().mean())
            else:
                radius = 1.0
            out = {"label": torch.empty((S * n,), dtype=torch.int32, device="cuda"),
                   "size": torch.empty((S * n,), dtype=torch.int32, device="cuda"),
                   "clusters": torch.empty((S,), dtype=torch.int32, device="cuda"),
                   "largest": torch.empty((S,), dtype=torch.int32, device="cuda")}
            kernel = lambda: ops.scan_clusters(points, offsets, radius, max_points=n, out=out)
            kernel()                                                   # warm-up: the code object, the LDS attribute
            kernel()
            _, theirs = wall_ms(lambda: cdist_scipy(clouds, radius))   # ... and the yardstick's libraries
            times = {"scan_clusters": [], "cdist_scipy": []}
            rounds = args.yardstick_repeats
            for _ in range(rounds):                                    # alternate the legs
                times["scan_clusters"] += event_ms(kernel, max(1, -(-args.repeats // rounds)))
                times["cdist_scipy"].append(wall_ms(lambda: cdist_scipy(clouds, radius))[0])
            times["scan_clusters"] = times["scan_clusters"][:max(args.repeats, rounds)]
            res = {name: summary(ms) for name, ms in times.items()}
            mine = out["clusters"].cpu().tolist()
            res["radius"] = round(radius, 6)
            res["plan"] = dict(zip(("threads", "tile", "lds_bytes"), ops.scan_clusters_plan(n)))
            res["pairs"] = S * n * (n - 1) // 2
            res["pairs_per_ns"] = round(res["pairs"] / (res["scan_clusters"]["median_ms"] * 1e6), 2)
            res["cdist_scipy_over_scan_clusters"] = round(res["cdist_scipy"]["median_ms"] / res["scan_clusters"]["median_ms"], 1)
            res["clusters_per_scan_mean"] = round(float(np.mean(mine)), 2)
            res["largest_share_mean"] = round(float(out["size"].view(S, n).max(dim=1).values.float().mean()) / n, 4)
            res["agreement_with_scipy"] = round(float(np.mean([a == b for a, b in zip(mine, theirs)])), 4)
            result["shapes"][f"S={S},n={n},{what}"] = res
            print(f"S={S},n={n},{what}", json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

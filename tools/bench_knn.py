#!/usr/bin/env python3
"""k nearest neighbours and statistical outlier removal on the GPU (GPU box only): how long ops.knn_points and
ops.scan_outliers take next to what a user does today on the same device, `torch.cdist` + `topk` per scan.

    python tools/bench_knn.py [--out profiles/knn.json] [--repeats 20] [--yardstick-repeats 5]

Shapes (S scans of n points, k): (64, 2048, 16), (8, 16384, 16), (1, 65536, 32), seeded uniform clouds in [-0.5, 0.5]^3.
Per shape, warmed up, device-event time of one call, the median and the extremes:
    knn_points     one launch over the whole ragged set, outputs reused
    scan_outliers  two launches (the neighbour sweep with the mean fused, the per-scan statistics), outputs reused
    cdist_topk     per scan `torch.cdist(c, c).topk(k + 1, largest=False)` — the k + 1 smallest, the first being the row
                   itself — in query blocks of at most 8192 rows so that the distance matrix stays below 2.2 GB; this is
                   the neighbour search alone, so it is the yardstick of knn_points and a lower bound of what an outlier
                   filter written in torch costs
The legs alternate.  `agreement` is the share of rows whose neighbour set equals the kernel's: cdist works through a
matrix product at these sizes and returns rounded distances, so it is reported, not asserted; the kernel's own check is
tests/test_knn_gpu.py.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

SHAPES = ((64, 2048, 16), (8, 16384, 16), (1, 65536, 32))
BLOCK = 8192


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


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def cdist_topk(clouds, k):
    """Per scan the k + 1 smallest cdist entries of every row, self included: index (S,n,k+1)."""
    out = []
    for c in clouds:
        parts = [torch.cdist(c[lo:lo + BLOCK], c).topk(k + 1, dim=1, largest=False).indices for lo in range(0, c.size(0), BLOCK)]
        out.append(torch.cat(parts))
    return torch.stack(out)


def agreement(index, theirs, S, n, k):
    """Share of rows whose k neighbours (as a set) are the yardstick's k + 1 smallest without the row itself."""
    mine = index.view(S, n, k).long().sort(dim=2).values
    rows = torch.arange(n, device=index.device).view(1, n, 1)
    other = theirs.masked_fill(theirs == rows, n + 1).sort(dim=2).values[:, :, :k]      # the row itself moves behind the rest
    return float((mine == other).all(dim=2).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--yardstick-repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    result = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for S, n, k in SHAPES:
        clouds = torch.from_numpy(np.random.RandomState(S + n).uniform(-0.5, 0.5, (S, n, 3)).astype(np.float32)).cuda()
        points = clouds.view(-1, 3)
        offsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * n
        lists = {"index": torch.empty((S * n, k), dtype=torch.int32, device="cuda"),
                 "dist2": torch.empty((S * n, k), dtype=torch.float32, device="cuda")}
        sor = {"keep": torch.empty((S * n,), dtype=torch.uint8, device="cuda"),
               "mean_dist": torch.empty((S * n,), dtype=torch.float32, device="cuda"),
               "kept": torch.empty((S,), dtype=torch.int32, device="cuda")}
        legs = {"knn_points": lambda: ops.knn_points(points, offsets, k, out=lists),
                "scan_outliers": lambda: ops.scan_outliers(points, offsets, k, 2.0, out=sor),
                "cdist_topk": lambda: cdist_topk(clouds, k)}
        for fn in legs.values():                                       # warm-up: code objects, library heuristics, the allocator
            fn()
            fn()
        torch.cuda.synchronize()
        same = agreement(lists["index"], cdist_topk(clouds, k), S, n, k)
        times = {name: [] for name in legs}
        rounds = args.yardstick_repeats
        for _ in range(rounds):                                        # alternate the legs
            times["knn_points"] += event_ms(legs["knn_points"], max(1, args.repeats // rounds))
            times["scan_outliers"] += event_ms(legs["scan_outliers"], max(1, args.repeats // rounds))
            times["cdist_topk"] += event_ms(legs["cdist_topk"], 1)
        res = {name: summary(ms) for name, ms in times.items()}
        res["plan"] = dict(zip(("instance_k", "threads", "tile"), ops.knn_points_plan(k)))
        res["pairs"] = S * n * n
        res["knn_pairs_per_ns"] = round(S * n * n / (res["knn_points"]["median_ms"] * 1e6), 2)
        res["cdist_topk_over_knn_points"] = round(res["cdist_topk"]["median_ms"] / res["knn_points"]["median_ms"], 2)
        res["cdist_topk_over_scan_outliers"] = round(res["cdist_topk"]["median_ms"] / res["scan_outliers"]["median_ms"], 2)
        res["agreement_with_cdist_topk"] = round(same, 6)
        res["kept_share"] = round(float(sor["kept"].sum()) / (S * n), 4)
        result["shapes"][f"S={S},n={n},k={k}"] = res
        print(f"S={S},n={n},k={k}", json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

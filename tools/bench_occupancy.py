#!/usr/bin/env python3
"""Occupancy-grid / JSD timing (GPU box only): one entropy_of_occupancy_grid call at S = 300, n = 1024, R = 28 clipped for
five point distributions (the share of points that needs the column search moves the time), the wall time of
jsd_between_point_cloud_sets on two such sets, and beside them an hp_nndistance call of all 307 200 points against the
10 144 kept centres — the fp32 brute force already in the library (it answers both directions, so twice the pairs).

    python tools/bench_occupancy.py                      device events and wall clock, then one JSON line
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_occupancy.py --trace
    python tools/bench_occupancy.py --summarize DIR      per-distribution kernel times out of that trace

--trace runs a fixed number of launches per distribution (CALLS) and nothing else, so the trace's occupancy_kernel
dispatches, in start order, fall into one group per distribution.
"""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

S, N, R = 300, 1024, 28
CALLS = 6                  # launches per distribution under --trace; the first is the warm-up
DISTRIBUTIONS = ("ball r=0.45", "ball r=0.5", "cube +-0.5", "sphere r=0.5", "cube +-0.6")


def clouds(name, seed):
    r = np.random.RandomState(seed)
    d = r.standard_normal((S, N, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    u = r.uniform(size=(S, N, 1)) ** (1.0 / 3.0)
    pts = {"ball r=0.45": d * 0.45 * u, "ball r=0.5": d * 0.5 * u, "cube +-0.5": r.uniform(-0.5, 0.5, (S, N, 3)),
           "sphere r=0.5": d * 0.5, "cube +-0.6": r.uniform(-0.6, 0.6, (S, N, 3))}[name]
    return pts.astype(np.float32)


def summarize(directory):
    f = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    occ = [us(r) for r in rows if "occupancy_kernel" in r["Kernel_Name"]]
    assert len(occ) == CALLS * len(DISTRIBUTIONS), len(occ)
    out = {}
    for i, name in enumerate(DISTRIBUTIONS):
        t = sorted(occ[i * CALLS + 1:(i + 1) * CALLS])
        out[name] = {"kernel_us_median": t[len(t) // 2], "kernel_us_min": t[0], "kernel_us_max": t[-1]}
        print(f"occupancy_kernel {name:14s}: median {t[len(t) // 2]:8.1f} us  (min {t[0]:.1f}, max {t[-1]:.1f}, {len(t)} launches)")
    nn = sorted(us(r) for r in rows if "nn_distance" in r["Kernel_Name"])
    if nn:
        out["nn_distance_kernel"] = {"kernel_us_median": nn[len(nn) // 2], "launches": len(nn)}
        print(f"nn_distance_kernel 307200 x 10144 (both directions): median {nn[len(nn) // 2]:.1f} us ({len(nn)} launches)")
    print(json.dumps(out))


def main():
    if "--summarize" in sys.argv:
        return summarize(sys.argv[sys.argv.index("--summarize") + 1])
    import torch
    from hyperpocket_amd.utils import metrics
    from hyperpocket_amd.utils.pytorch_structural_losses import StructuralLossesBackend as B
    assert torch.cuda.is_available(), "needs a GPU: a timing taken elsewhere says nothing"
    sets = {name: torch.from_numpy(clouds(name, i)).cuda() for i, name in enumerate(DISTRIBUTIONS)}
    centres = torch.from_numpy(metrics.unit_cube_grid_point_cloud(R, True)[0]).cuda()[None].contiguous()
    if "--trace" in sys.argv:
        for name in DISTRIBUTIONS:
            for _ in range(CALLS):
                metrics._occupancy_counts(sets[name], R, True)
        for _ in range(3):
            B.NNDistance(sets["sphere r=0.5"].view(1, -1, 3), centres)
        torch.cuda.synchronize()
        return
    res = {}
    for name, pts in sets.items():
        counters, _ = metrics._occupancy_counts(pts, R, True)         # warm-up; tables built and cached
        times = []
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metrics.entropy_of_occupancy_grid(pts, R, True)
            times.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"entropy_call_wall_ms_median": sorted(times)[5], "points": int(counters.sum())}
        print(f"entropy_of_occupancy_grid {name:14s}: wall {sorted(times)[5]:.3f} ms per call (median of 10, result on the host)")
    a, b = sets["sphere r=0.5"], sets["cube +-0.5"]
    times = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jsd = metrics.jsd_between_point_cloud_sets(a, b)
        times.append((time.perf_counter() - t0) * 1e3)
    res["jsd_between_point_cloud_sets"] = {"wall_ms_median": sorted(times)[5], "value": jsd}
    print(f"jsd_between_point_cloud_sets, two sets of {S} x {N}: wall {sorted(times)[5]:.3f} ms (median of 10), JSD {jsd:.6f}")
    flat = a.view(1, -1, 3)
    for _ in range(2):
        B.NNDistance(flat, centres)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(10):
        B.NNDistance(flat, centres)
    e.record()
    torch.cuda.synchronize()
    res["nndistance_307200_x_10144"] = {"event_ms": s.elapsed_time(e) / 10}
    print(f"hp_nndistance (1, {S * N}, 3) vs (1, {centres.size(1)}, 3), both directions: {s.elapsed_time(e) / 10:.3f} ms per call")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Farthest-point sampling on the GPU (GPU box only): how long one hp_farthest_points launch takes next to a plain torch
statement of the same law, and what a ScanBatcher batch costs with resample="farthest" next to resample="subset".

    python tools/bench_fps.py [--out profiles/r11_fps.json] [--repeats 20] [--loop-repeats 3]

(a) ops.farthest_points at (B, P, k) = (64, 8192, 1024), (8, 8192, 1024), (64, 2048, 1024) on seeded uniform clouds:
    device-event time of one call (one launch), warmed up, the median and the extremes of --repeats calls.  The baseline
    is the law written in torch on the device — per pick one gather of the picked rows, the squared distances, a
    `minimum` and an `argmax` over (B,P): about a dozen launches per pick where the kernel has one per call — timed the
    same way over --loop-repeats calls, the two alternated.  Both must give the same index (checked before timing).
(b) One ScanBatcher batch of 64 scans of 30000 points to 1024 rows, resample="subset" against resample="farthest"
    (pool 8192): device-event time of the whole `next()`, alternated.
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

SHAPES = ((64, 8192, 1024), (8, 8192, 1024), (64, 2048, 1024))
SCANS, SCAN_POINTS, TARGET = 64, 30000, 1024


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


def torch_loop(clouds, k):
    """The law of include/hyperpocket_hip.h in torch, start row 0, all rows valid: (index (B,k) int64, radius2 (B,k))."""
    B, P, _ = clouds.shape
    index = torch.empty((B, k), dtype=torch.int64, device=clouds.device)
    radius2 = torch.empty((B, k), dtype=torch.float32, device=clouds.device)
    pick = torch.zeros((B,), dtype=torch.int64, device=clouds.device)
    mind = torch.full((B, P), float("inf"), device=clouds.device)
    rows = torch.arange(B, device=clouds.device)
    for j in range(k):
        index[:, j] = pick
        d = clouds - clouds[rows, pick].unsqueeze(1)
        sq = d * d
        mind = torch.minimum(mind, (sq[..., 0] + sq[..., 1]) + sq[..., 2])
        radius2[:, j], pick = mind.max(dim=1)
    return index, radius2


def part_a(repeats, loop_repeats):
    from hyperpocket_amd import ops
    out = {}
    for B, P, k in SHAPES:
        clouds = torch.from_numpy(np.random.RandomState(B + P).uniform(-0.5, 0.5, (B, P, 3)).astype(np.float32)).cuda()
        bufs = ops.farthest_points_buffers(B, k, "cuda")
        failed = torch.zeros((1,), dtype=torch.int32, device="cuda")
        kernel = lambda: ops.farthest_points(clouds, k, out=bufs, failed=failed)
        loop = lambda: torch_loop(clouds, k)
        kernel()
        want_index, want_radius2 = loop()                                  # also the loop's warm-up
        torch.cuda.synchronize()
        # torch.max does not promise the first of equal values; on uniform random clouds equal distances do not occur
        same = bool(torch.equal(bufs["index"].long(), want_index)) and bool(torch.equal(bufs["radius2"], want_radius2))
        k_ms, l_ms = [], []
        for r in range(loop_repeats):                                      # alternate the two
            k_ms += event_ms(kernel, max(1, repeats // loop_repeats))
            l_ms += event_ms(loop, 1)
        res = {"kernel": summary(k_ms), "torch_loop": summary(l_ms), "same_result": same, "failed": int(failed.item()),
               "kernel_us_per_pick": round(sorted(k_ms)[len(k_ms) // 2] * 1e3 / k, 4)}
        res["loop_over_kernel"] = round(res["torch_loop"]["median_ms"] / res["kernel"]["median_ms"], 2)
        out[f"B={B},P={P},k={k}"] = res
        print(f"B={B},P={P},k={k}", json.dumps(res), flush=True)
    return out


def part_b(repeats):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    r = np.random.RandomState(5)
    # dense near the sensor, thin elsewhere: radii drawn so that the density falls with the distance
    scans = [(r.standard_normal((SCAN_POINTS, 3)) * r.uniform(0.02, 0.5, (SCAN_POINTS, 1))).astype(np.float32) for _ in range(SCANS)]
    data = DeviceScanDataset(scans, device="cuda")
    legs = {"subset": ScanBatcher(data, SCANS, target=TARGET, normalize=True, seed=1),
            "farthest": ScanBatcher(data, SCANS, target=TARGET, normalize=True, seed=1, resample="farthest", pool=8192)}
    times = {name: [] for name in legs}
    for name, batcher in legs.items():
        next(iter(batcher))
    torch.cuda.synchronize()
    for _ in range(repeats):
        for name, batcher in legs.items():
            times[name] += event_ms(lambda: next(iter(batcher)), 1)
    out = {name: summary(ms) for name, ms in times.items()}
    out["farthest"]["radius2_mean"] = float(legs["farthest"].last_radius2.mean())
    out["failures"] = {name: b.failures() for name, b in legs.items()}
    print("batch", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_fps.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--loop-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fps.py measures on the GPU: none here")
    import ctypes
    from hyperpocket_amd import ops
    plans = {}
    for _, P, _ in SHAPES:
        threads, per_lane = ctypes.c_int(0), ctypes.c_int(0)
        ops.load_library().hp_farthest_points_plan(P, ctypes.byref(threads), ctypes.byref(per_lane))
        plans[f"P={P}"] = {"threads": threads.value, "points_per_lane": per_lane.value}
    result = {"device": torch.cuda.get_device_name(0), "plans": plans,
              "farthest_points": part_a(args.repeats, args.loop_repeats),
              "scan_batch": {"scans": SCANS, "points_per_scan": SCAN_POINTS, "target": TARGET, "pool": 8192,
                             **part_b(args.repeats)}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The supporting plane of ragged scans on the GPU (GPU box only): how long ops.scan_plane and the whole
DeviceScanDataset.without_plane take next to the same consensus counted by a plain torch expression on the same device.

    python tools/bench_plane.py [--out profiles/plane.json] [--repeats 20] [--yardstick-repeats 5]

Shapes (S scans of n rows, `trials` hypotheses per scan), seeded, every scan a plane that holds 60 % of the rows (noise
+-0.004) in uniform clutter, threshold 0.01:
    scene    S = 8,   n = 200 000, trials 512 and 4096
    object   S = 256, n = 4096,    trials 512
Per shape, warmed up, the median and the extremes of:
    scan_plane      device-event time of one call (five launches), outputs and workspace reused
    without_plane   wall-clock time of the dataset method, refine=True, synchronised before and after: scan_plane, the
                    moments read back and refitted on the host, scan_plane_side, the kept rows packed
    torch_consensus device-event time of the yardstick: per scan, the kernel's own hypotheses (a, nrm, rhs — drawing them is
                    not timed) against all rows, e = P @ nrm^T - a . nrm, (e * e <= rhs).sum(0) — a matrix product, a square,
                    a compare and a sum; scans are taken one after the other and in slices of at most 2^28 (row, trial)
                    pairs, because the (n, trials) intermediate does not fit otherwise
The legs alternate.  The yardstick rounds differently from the law (P @ nrm^T - a . nrm instead of nrm . (P - a)), so its
winner's count is reported next to the kernel's (`count_ratio`), not asserted; the kernel's own check is
tests/test_plane_gpu.py.  `pairs_per_ns` is S * n * trials over the median scan_plane time.
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

SHAPES = (("scene", 8, 200_000, 512), ("scene", 8, 200_000, 4096), ("object", 256, 4096, 512))
THRESHOLD = 0.01
SLICE_PAIRS = 1 << 28


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


def inputs(S, n):
    """(S, n, 3) float32: per scan a plane through the box [-1, 1]^3 with 60 % of the rows, the rest uniform."""
    r = np.random.RandomState(S + n)
    clouds = r.uniform(-1, 1, (S, n, 3))
    m = int(0.6 * n)
    for s in range(S):
        normal = r.normal(size=3)
        normal /= np.linalg.norm(normal)
        off = r.uniform(-0.004, 0.004, m) + r.uniform(-0.3, 0.3) - clouds[s, :m] @ normal
        clouds[s, :m] += off[:, None] * normal
        clouds[s] = clouds[s, r.permutation(n)]
    return clouds.astype(np.float32)


def torch_consensus(clouds, a, nrm, rhs, counts):
    """counts (S, H) int64 of the hypotheses (a, nrm, rhs) (S, H, .) over the rows of clouds (S, n, 3)."""
    S, n, _ = clouds.shape
    H = a.size(1)
    step = max(1, SLICE_PAIRS // H)
    for s in range(S):
        offset = (a[s] * nrm[s]).sum(1)
        total = torch.zeros(H, dtype=torch.int64, device=clouds.device)
        for lo in range(0, n, step):
            e = clouds[s, lo:lo + step] @ nrm[s].t() - offset
            total += (e * e <= rhs[s]).sum(0)
        counts[s] = total
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--yardstick-repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plane.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    result = {"device": torch.cuda.get_device_name(0), "threshold": THRESHOLD, "shapes": {}}
    made = {}
    for what, S, n, trials in SHAPES:
        if (S, n) not in made:
            made = {(S, n): torch.from_numpy(inputs(S, n)).cuda()}          # one shape's rows at a time
        clouds = made[(S, n)]
        points = clouds.view(-1, 3)
        offsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * n
        out, ws = ops.scan_plane_buffers(S, S * n, trials, "cuda")
        kernel = lambda: ops.scan_plane(points, offsets, THRESHOLD, trials=trials, min_share=0.2, out=out, ws=ws)
        data = DeviceScanDataset((points, offsets))
        method = lambda: data.without_plane(THRESHOLD, trials=trials)
        kernel()                                                       # warm-up: the code objects
        kernel()
        hyp = ws.view(torch.float32)[:S * trials * 8].view(S, trials, 8).clone()     # the workspace's first part: a, nrm, rhs, valid
        a, nrm, rhs = hyp[:, :, 0:3].contiguous(), hyp[:, :, 3:6].contiguous(), hyp[:, :, 6].contiguous()
        counts = torch.zeros((S, trials), dtype=torch.int64, device="cuda")
        yardstick = lambda: torch_consensus(clouds, a, nrm, rhs, counts)
        yardstick()                                                    # ... the yardstick's libraries
        method()
        times = {"scan_plane": [], "without_plane": [], "torch_consensus": []}
        rounds = args.yardstick_repeats
        for _ in range(rounds):                                        # alternate the legs
            times["scan_plane"] += event_ms(kernel, max(1, -(-args.repeats // rounds)))
            times["torch_consensus"] += event_ms(yardstick, 1)
            times["without_plane"].append(wall_ms(method)[0])
        res = {name: summary(ms) for name, ms in times.items()}
        res["plan"] = dict(zip(("threads", "rows_per_lane", "trial_tile"), ops.scan_plane_plan(trials)))
        res["pairs"] = S * n * trials
        res["pairs_per_ns"] = round(res["pairs"] / (res["scan_plane"]["median_ms"] * 1e6), 2)
        res["torch_over_scan_plane"] = round(res["torch_consensus"]["median_ms"] / res["scan_plane"]["median_ms"], 2)
        res["inliers_share_mean"] = round(float(out["inliers"].float().mean()) / n, 4)
        res["found"] = int(out["found"].sum())
        res["count_ratio"] = round(float(counts.max(dim=1).values.float().mean() / out["inliers"].float().mean()), 5)
        result["shapes"][f"{what},S={S},n={n},trials={trials}"] = res
        print(f"{what},S={S},n={n},trials={trials}", json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Voxel-grid thinning of ragged scans on the GPU (GPU box only): how long ops.scan_voxels and DeviceScanDataset.thinned take
next to the same cells found by plain torch expressions on the same device.

    python tools/bench_voxels.py [--out profiles/voxels.json] [--repeats 20] [--yardstick-repeats 5]

Shapes (S scans of n rows), seeded:
    scene    S = 8,   n = 500 000: a floor and two walls of the box [-1, 1]^3 (noise 0.002) and ten blobs (sigma 0.05), a
             quarter of the rows each, in the sweep order of a sensor at (2, 1.5, 2): by elevation line, then by azimuth.
             voxel 0.005 (a few rows per cell)
    dense    the same rows at voxel 0.05: hundreds of rows per cell, and neighbouring rows share cells — the contention case
    object   S = 256, n = 16 384: a noisy sphere of radius 0.5, rows shuffled; voxel 0.01
Per shape, warmed up, the median and the extremes of:
    scan_voxels     device-event time of one call (three launches), outputs and workspace reused, keep="center"
    thinned_voxel   wall-clock time of DeviceScanDataset.thinned(voxel=...), synchronised before and after: scan_voxels, the
                    counts read back, the kept rows packed
    thinned_budget  wall-clock time of thinned(max_points=32768): 17 scan_voxels calls and the packing (on `object` every
                    scan is within the budget: no call, the packing alone)
    torch_unique    device-event time of the yardstick: the same cells by floor(p / voxel) packed with the scan's number into
                    one int64 (18 bits per axis — enough for these shapes, asserted), torch.unique(return_inverse=True),
                    the packed ranks (bits of d2, row) and scatter_reduce(amin), keep = the rank equals its cell's minimum
The legs alternate.  The yardstick's cells and kept rows are compared with the kernel's (`same_keep`); the kernel's own check
is tests/test_voxels_gpu.py.  `rows_per_us` is S * n over the median scan_voxels time.
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

SHAPES = (("scene", 8, 500_000, 0.005), ("dense", 8, 500_000, 0.05), ("object", 256, 16_384, 0.01))
BUDGET = 32768
AXIS_BITS = 18


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


def scene(r, n):
    """(n,3) float32: three faces of the box, ten blobs, in sweep order."""
    q = n // 4
    uv = r.uniform(-1, 1, (3, q, 2))
    noise = r.normal(0, 0.002, (3, q))
    floor = np.stack([uv[0, :, 0], -1 + noise[0], uv[0, :, 1]], axis=1)
    back = np.stack([uv[1, :, 0], uv[1, :, 1], -1 + noise[1]], axis=1)
    side = np.stack([-1 + noise[2], uv[2, :, 0], uv[2, :, 1]], axis=1)
    centre = r.uniform(-0.7, 0.7, (10, 3))
    blobs = centre[r.randint(0, 10, n - 3 * q)] + r.normal(0, 0.05, (n - 3 * q, 3))
    cloud = np.concatenate([floor, back, side, blobs])
    d = cloud - np.array([2.0, 1.5, 2.0])
    line = np.floor(np.arcsin(d[:, 1] / np.linalg.norm(d, axis=1)) * 600.0)
    return cloud[np.lexsort((np.arctan2(d[:, 0], d[:, 2]), line))].astype(np.float32)


def sphere(r, n):
    p = r.normal(size=(n, 3))
    return (0.5 * p / np.linalg.norm(p, axis=1, keepdims=True) + r.normal(0, 0.003, (n, 3))).astype(np.float32)


def inputs(what, S, n):
    r = np.random.RandomState(S + n)
    return np.stack([scene(r, n) if what != "object" else sphere(r, n) for _ in range(S)])


def torch_unique(points, scan, row, voxel):
    """(keep (T) bool, cells) of the yardstick; voxel: a 0-dim float32 device tensor."""
    half = 1 << (AXIS_BITS - 1)
    qf = torch.floor(points / voxel)
    q = qf.to(torch.int64) + half
    key = (scan << (3 * AXIS_BITS)) | (q[:, 0] << (2 * AXIS_BITS)) | (q[:, 1] << AXIS_BITS) | q[:, 2]
    d = points - (qf + 0.5) * voxel
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    rank = (d2.view(torch.int32).to(torch.int64) << 32) | row
    cells, inverse = torch.unique(key, return_inverse=True)
    best = torch.full((cells.numel(),), torch.iinfo(torch.int64).max, dtype=torch.int64, device=points.device)
    best.scatter_reduce_(0, inverse, rank, "amin")
    return best[inverse] == rank, cells.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxels.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--yardstick-repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxels.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    result = {"device": torch.cuda.get_device_name(0), "budget": BUDGET, "shapes": {}}
    made = {}
    for what, S, n, voxel in SHAPES:
        if (S, n) not in made:
            made = {(S, n): torch.from_numpy(inputs(what, S, n)).cuda()}          # one shape's rows at a time
        clouds = made[(S, n)]
        points = clouds.view(-1, 3)
        offsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * n
        edge = torch.full((S,), voxel, dtype=torch.float32, device="cuda")
        bufs = ops.scan_voxels_buffers(S, S * n, "cuda")
        kernel = lambda: ops.scan_voxels(points, offsets, edge, out=bufs, ws=bufs["ws"])
        data = DeviceScanDataset((points, offsets))
        scan, row = data._scan_of_rows(), torch.arange(S * n, device="cuda") % n
        assert float(points.abs().max()) / voxel < (1 << (AXIS_BITS - 1))         # the yardstick's packing holds
        edge0 = edge[0]                                                # a device scalar: a true division, as the kernel's
        yardstick = lambda: torch_unique(points, scan, row, edge0)
        kernel()                                                       # warm-up: the code objects
        kernel()
        keep, cells = yardstick()                                      # ... the yardstick's libraries
        data.thinned(voxel=voxel)
        data.thinned(max_points=BUDGET)
        times = {"scan_voxels": [], "thinned_voxel": [], "thinned_budget": [], "torch_unique": []}
        rounds = args.yardstick_repeats
        for _ in range(rounds):                                        # alternate the legs
            times["scan_voxels"] += event_ms(kernel, max(1, -(-args.repeats // rounds)))
            times["torch_unique"] += event_ms(yardstick, 1)
            times["thinned_voxel"].append(wall_ms(lambda: data.thinned(voxel=voxel))[0])
            times["thinned_budget"].append(wall_ms(lambda: data.thinned(max_points=BUDGET))[0])
        res = {name: summary(ms) for name, ms in times.items()}
        kernel()
        res["plan"] = dict(zip(("threads", "rows_per_lane"), ops.scan_voxels_plan()))
        res["rows"] = S * n
        res["cells"] = int(bufs["kept"].sum())
        res["rows_per_cell"] = round(res["rows"] / max(1, res["cells"]), 2)
        res["rows_per_us"] = round(res["rows"] / (res["scan_voxels"]["median_ms"] * 1e3), 1)
        res["torch_over_scan_voxels"] = round(res["torch_unique"]["median_ms"] / res["scan_voxels"]["median_ms"], 2)
        res["same_keep"] = bool(cells == res["cells"] and torch.equal(keep, bufs["keep"] != 0))
        budget = data.thinned(max_points=BUDGET)
        res["budget_rows_max"] = int(budget.lengths.max())
        res["budget_voxel_mean"] = round(float(budget.voxels.nanmean()), 6) if not bool(budget.voxels.isnan().all()) else None
        result["shapes"][f"{what},S={S},n={n},voxel={voxel}"] = res
        print(f"{what},S={S},n={n},voxel={voxel}", json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Visibility of ragged scans from their sensor positions on the GPU (GPU box only): how long ops.scan_visibility takes next to
the same law written as plain torch expressions on the same device.

    python tools/bench_visibility.py [--out profiles/visibility.json] [--repeats 20] [--yardstick-repeats 5]

Shapes (S scans of n rows), seeded:
    scene    S = 8,  n = 500 000: a floor and two walls of the box [-1, 1]^3 (noise 0.002) and ten blobs (sigma 0.05), a
             quarter of the rows each, in the sweep order of a sensor at (2, 1.5, 2) — the viewpoint: by elevation line, then by
             azimuth.  resolution 512 (a pixel of about two sample spacings), window 1
    object   S = 64, n = 2048: a noisy sphere of radius 0.5 about the origin seen from 64 positions on the sphere of radius
             2.5, rows shuffled.  resolution 32, window 1 — the defaults, the shape of DeviceScanDataset.virtual_scans
Per shape, warmed up, the median and the extremes of:
    scan_visibility   device-event time of one call (a memset and two launches), label, winner and workspace reused
    torch_scatter     device-event time of the yardstick: the projection in float64 tensor expressions, the keys packed into
                      int64, scatter_reduce(amin) into a buffer of the same layout, then (2w+1)^2 gathers and the label rules
The legs alternate.  The yardstick's labels and winners are compared with the kernel's (`same_label`, `same_winner`); the
kernel's own check is tests/test_visibility_gpu.py.  `rows_per_us` is S * n over the median scan_visibility time.  The ratio
is recorded, not judged: there is no pass or fail here.
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

SHAPES = (("scene", 8, 500_000, 512, 1), ("object", 64, 2048, 32, 1))
MARGIN, SLOPE = 0.01, 2.0
SENSOR = (2.0, 1.5, 2.0)


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


def scene(r, n):
    """(n,3) float32: three faces of the box, ten blobs, in the sweep order of the sensor."""
    q = n // 4
    uv = r.uniform(-1, 1, (3, q, 2))
    noise = r.normal(0, 0.002, (3, q))
    floor = np.stack([uv[0, :, 0], -1 + noise[0], uv[0, :, 1]], axis=1)
    back = np.stack([uv[1, :, 0], uv[1, :, 1], -1 + noise[1]], axis=1)
    side = np.stack([-1 + noise[2], uv[2, :, 0], uv[2, :, 1]], axis=1)
    centre = r.uniform(-0.7, 0.7, (10, 3))
    blobs = centre[r.randint(0, 10, n - 3 * q)] + r.normal(0, 0.05, (n - 3 * q, 3))
    cloud = np.concatenate([floor, back, side, blobs])
    d = cloud - np.array(SENSOR)
    line = np.floor(np.arcsin(d[:, 1] / np.linalg.norm(d, axis=1)) * 600.0)
    return cloud[np.lexsort((np.arctan2(d[:, 0], d[:, 2]), line))].astype(np.float32)


def sphere(r, n):
    p = r.normal(size=(n, 3))
    return (0.5 * p / np.linalg.norm(p, axis=1, keepdims=True) + r.normal(0, 0.003, (n, 3))).astype(np.float32)


def inputs(what, S, n):
    """(clouds (S,n,3), viewpoints (S,3)) float32."""
    from hyperpocket_amd.datasets.scan_dataset import viewpoints_on_sphere
    r = np.random.RandomState(S + n)
    if what == "scene":
        return np.stack([scene(r, n) for _ in range(S)]), np.tile(np.array(SENSOR, np.float32), (S, 1))
    return np.stack([sphere(r, n) for _ in range(S)]), viewpoints_on_sphere(S, 2.5, seed=S + n)


def torch_scatter(points, scan, row, views, S, R, w, margin, pitch):
    """(label (T) uint8, winner (T) bool) of the yardstick, for finite rows none of which is the viewpoint."""
    big = torch.iinfo(torch.int64).max
    d = points.double() - views.double()[scan]
    a = d.abs()
    ax, ay, az = a.unbind(1)
    m = torch.where(ax >= ay, torch.where(ax >= az, 0, 2), torch.where(ay >= az, 1, 2))
    pick = lambda k: d.gather(1, ((m + k) % 3).unsqueeze(1)).squeeze(1)
    dm, du, dt = pick(0), pick(1), pick(2)
    am = dm.abs()
    face = 2 * m + (dm < 0)
    half = 0.5 * R
    iu = torch.floor((du / am + 1.0) * half).to(torch.int64).clamp_(max=R - 1)
    it = torch.floor((dt / am + 1.0) * half).to(torch.int64).clamp_(max=R - 1)
    z = am.float()
    key = (z.view(torch.int32).to(torch.int64) << 32) | row
    plane = (scan * 6 + face) * R
    buf = torch.full((S * 6 * R * R,), big, dtype=torch.int64, device=points.device)
    buf.scatter_reduce_(0, (plane + it) * R + iu, key, "amin")
    z0 = z.double()
    slant = z0 * pitch
    seen = torch.zeros_like(row, dtype=torch.bool)
    hidden = torch.zeros_like(seen)
    behind = torch.ones_like(seen)
    for dy in range(-w, w + 1):
        for dx in range(-w, w + 1):
            y, x = it + dy, iu + dx
            inside = (y >= 0) & (y < R) & (x >= 0) & (x < R)
            k = buf[torch.where(inside, (plane + y) * R + x, 0)]
            full = inside & (k != big)
            zz = (k >> 32).to(torch.int32).view(torch.float32).double()
            tol = margin + slant * float(max(abs(dx), abs(dy)) + 1)
            seen |= full
            hidden |= full & (zz + tol < z0)
            behind &= ~full | (zz - tol > z0)
    label = torch.where(~seen, 3, torch.where(hidden, 2, torch.where(behind, 0, 1))).to(torch.uint8)
    return label, buf[(plane + it) * R + iu] == key


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--yardstick-repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visibility.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    result = {"device": torch.cuda.get_device_name(0), "margin": MARGIN, "slope": SLOPE, "shapes": {}}
    for what, S, n, R, w in SHAPES:
        clouds, views = inputs(what, S, n)
        points = torch.from_numpy(clouds).cuda().view(-1, 3)
        views = torch.from_numpy(views).cuda()
        offsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * n
        bufs = ops.scan_visibility_buffers(S, R, "cuda", Q=S * n)
        bufs["winner"] = torch.empty_like(bufs["label"])
        kernel = lambda: ops.scan_visibility(points, offsets, views, resolution=R, window=w, margin=MARGIN, slope=SLOPE, out=bufs,
                                             ws=bufs["ws"])
        row = torch.arange(S * n, device="cuda") % n
        scan = torch.arange(S * n, device="cuda") // n
        pitch = 2.0 * SLOPE / R
        yardstick = lambda: torch_scatter(points, scan, row, views, S, R, w, MARGIN, pitch)
        kernel()                                                       # warm-up: the code objects
        kernel()
        label, winner = yardstick()                                    # ... the yardstick's libraries
        yardstick()
        times = {"scan_visibility": [], "torch_scatter": []}
        rounds = args.yardstick_repeats
        for _ in range(rounds):                                        # alternate the legs
            times["scan_visibility"] += event_ms(kernel, max(1, -(-args.repeats // rounds)))
            times["torch_scatter"] += event_ms(yardstick, 1)
        res = {name: summary(ms) for name, ms in times.items()}
        kernel()
        res["plan"] = dict(zip(("threads", "rows_per_lane", "scatter_groups", "classify_groups"), ops.scan_visibility_plan(S * n)))
        res["rows"], res["resolution"], res["window"] = S * n, R, w
        res["workspace_bytes"] = bufs["ws"].nbytes
        res["visible_share"] = round(float((bufs["label"] == 1).double().mean()), 4)
        res["winners"] = int(bufs["winner"].sum())
        res["rows_per_us"] = round(res["rows"] / (res["scan_visibility"]["median_ms"] * 1e3), 1)
        res["torch_over_scan_visibility"] = round(res["torch_scatter"]["median_ms"] / res["scan_visibility"]["median_ms"], 2)
        res["same_label"] = bool(torch.equal(label, bufs["label"]))
        res["same_winner"] = bool(torch.equal(winner, bufs["winner"] != 0))
        result["shapes"][f"{what},S={S},n={n},R={R},w={w}"] = res
        print(f"{what},S={S},n={n},R={R},w={w}", json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

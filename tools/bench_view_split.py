#!/usr/bin/env python3
"""The viewpoint batch maker on the GPU (GPU box only): how long one ops.make_view_batch call takes next to one ops.make_batch
call at the same shape and next to the same law written as plain torch expressions, on the same device in the same run.

    python tools/bench_view_split.py [--out profiles/view_split.json] [--windows 30] [--calls 50] [--yardstick-calls 5]

Shapes (B items of N rows from M = B seeded clouds, uniform balls of radius 0.5 — tools/bench_batcher.py's — with the sensor at
distance 3, the image fitted to the ball):
    training   B = 64, N = 2048, target 1024, R = 32, w = 1: the defaults, the shape of a training step
    dense      B = 64, N = 8192, target 4096, R = 64, w = 1
Per shape, warmed up, over `windows` timed windows that alternate between the legs — a window is `calls` calls between two
device events, divided by `calls`, so a figure is the time of a call in a stream of calls: kernel and launch —, the median and
the extremes of:
    make_view_batch   one launch; side and occlusion not written, as DeviceViewBatcher calls it
    make_batch        the random-plane batch maker with its defaults (groups, max_candidates): a memset and two launches.  Its
                      time follows the slowest item's candidate search, so the streams change from window to window
    torch_law         the law in torch: the projection in float64 tensor expressions, scatter_reduce(amin) into a (B, R^2)
                      buffer, the windowed minimum by (2w+1)^2 gathers, a stable sort of the occlusions for the ranking and a
                      stable sort of the sides for the order-preserving compaction
The yardstick's `side` is compared with the kernel's (`same_side`); the kernel's own check is tests/test_view_split_gpu.py.
The ratios are recorded, not judged: there is no pass or fail here.
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

SHAPES = (("training", 64, 2048, 1024, 32, 1), ("dense", 64, 8192, 4096, 64, 1))
DIST, RADIUS = 3.0, 0.5


def balls(m, n, seed):
    r = np.random.RandomState(seed)
    d = r.standard_normal((m, n, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return (d * RADIUS * r.uniform(size=(m, n, 1)) ** (1.0 / 3.0)).astype(np.float32)


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(ms, calls):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 5), "min_ms": round(ms[0], 5), "max_ms": round(ms[-1], 5), "windows": len(ms),
            "calls_per_window": calls}


def torch_law(clouds, frames, target, dist, scale, R, w):
    """(existing, missing, side) of the law for finite rows in front of the sensor."""
    B, N, _ = clouds.shape
    big = torch.iinfo(torch.int64).max
    p, Q = clouds.double(), frames.double()
    c = [(Q[:, k, 0:1] * p[..., 0] + Q[:, k, 1:2] * p[..., 1]) + Q[:, k, 2:3] * p[..., 2] for k in range(3)]
    delta = dist - c[2]
    z = delta.float()
    half = 0.5 * R
    iu = torch.floor(((c[0] / delta) * scale + half).clamp(0.0, R - 1.0)).to(torch.int64)
    it = torch.floor(((c[1] / delta) * scale + half).clamp(0.0, R - 1.0)).to(torch.int64)
    zb = z.view(torch.int32).to(torch.int64)
    buf = torch.full((B, R * R), big, dtype=torch.int64, device=clouds.device)
    buf.scatter_reduce_(1, it * R + iu, zb, "amin")
    front = torch.full_like(zb, big)
    for dy in range(-w, w + 1):
        for dx in range(-w, w + 1):
            y, x = it + dy, iu + dx
            inside = (y >= 0) & (y < R) & (x >= 0) & (x < R)
            front = torch.minimum(front, torch.where(inside, buf.gather(1, torch.where(inside, y * R + x, 0)), big))
    o = z - front.to(torch.int32).view(torch.float32)
    order = torch.sort(o, dim=1, stable=True).indices
    side = torch.zeros((B, N), dtype=torch.uint8, device=clouds.device)
    side.scatter_(1, order[:, :target], 1)
    rows = torch.sort(side, dim=1, descending=True, stable=True).indices                    # existing first, each in row order
    parts = clouds.gather(1, rows.unsqueeze(-1).expand(B, N, 3))
    return parts[:, :target].contiguous(), parts[:, target:].contiguous(), side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_split.json"))
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--yardstick-calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_view_split.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    dev = "cuda"
    h = ops.view_half_extent(RADIUS, DIST)
    result = {"device": torch.cuda.get_device_name(0), "distance": DIST, "radius": RADIUS, "shapes": {}}
    for what, B, N, target, R, w in SHAPES:
        clouds = torch.from_numpy(balls(B, N, N)).to(dev)
        ids = torch.arange(B, dtype=torch.int32, device=dev)
        frames = ops.view_frames(B, N).to(dev)
        scale = (0.5 * R) / h
        view_bufs = ops.make_view_batch_buffers(B, N, target, dev, side=False, occlusion=False)
        plane_bufs, ws = ops.make_batch_buffers(B, N, target, dev), ops.make_batch_workspace(B, N, dev)
        failed = torch.zeros((1,), dtype=torch.int32, device=dev)
        streams = [torch.arange(B, dtype=torch.int64, device=dev) + 1000 * s for s in range(args.windows)]
        state = {"streams": streams[0]}
        legs = {"make_view_batch": (lambda: ops.make_view_batch(clouds, ids, frames, target, None, None, DIST, h, R, w, out=view_bufs),
                                    args.calls),
                "make_batch": (lambda: ops.make_batch(clouds, ids, state["streams"], target, out=plane_bufs, ws=ws, failed=failed),
                               args.calls),
                "torch_law": (lambda: torch_law(clouds, frames, target, DIST, scale, R, w), args.yardstick_calls)}
        for fn, _ in legs.values():                                    # warm-up: the code objects, the yardstick's libraries
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for k in range(args.windows):                                  # alternate the legs
            state["streams"] = streams[k]
            for name, (fn, calls) in legs.items():
                times[name].append(window_ms(fn, calls))
        res = {name: summary(ms, legs[name][1]) for name, ms in times.items()}
        full = ops.make_view_batch(clouds, ids, frames, target, None, None, DIST, h, R, w)
        ex, mi, side = torch_law(clouds, frames, target, DIST, scale, R, w)
        res["same_side"] = bool(torch.equal(side, full[3]))
        res["same_parts"] = bool(torch.equal(ex, full[0]) and torch.equal(mi, full[1]))
        threads, lds = ops._plan("hp_make_view_batch_plan", (N, R), 2, "plan")
        res["plan"] = {"threads": threads, "dynamic_lds_bytes": lds, "workgroups": B}
        res["make_batch_failed_items"] = int(failed.item())
        res["existing_share_on_the_sensors_half"] = round(float(
            (((clouds.double() * frames.double()[:, 2:3, :]).sum(-1) > 0) & (full[3] != 0)).double().sum() / (B * target)), 4)
        v = res["make_view_batch"]["median_ms"]
        res["make_batch_over_make_view_batch"] = round(res["make_batch"]["median_ms"] / v, 2)
        res["torch_law_over_make_view_batch"] = round(res["torch_law"]["median_ms"] / v, 2)
        key = f"{what},B={B},N={N},target={target},R={R},w={w}"
        result["shapes"][key] = res
        print(key, json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

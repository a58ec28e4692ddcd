#!/usr/bin/env python3
"""The cut by coordinate rank on the GPU (GPU box only): how long one hp_axis_split launch takes next to the torch statement
of the same law, torch.argsort(stable=True) and two gathers, on the same inputs.  A record, not a gate.

    python tools/bench_axis_split.py [--out FILE.json] [--repeats 50]

Shapes (B, n, k): (64, 2048, 1024) — a test set's worth of clouds cut in halves — and (64, 8192, 4096), the largest cloud.
Seeded uniform clouds, axis 0.  Device-event time of one call, warmed up, the two alternated; the median and the extremes of
--repeats calls each.  Both must give the same permutation and the same rows (checked before timing).
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

SHAPES = ((64, 2048, 1024), (64, 8192, 4096))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def torch_split(clouds, k, axis):
    order = torch.argsort(clouds[:, :, axis], dim=1, stable=True)
    pick = lambda rows: torch.gather(clouds, 1, rows.unsqueeze(2).expand(-1, -1, 3))
    return pick(order[:, :k]), pick(order[:, k:]), order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_axis_split.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    result = {"device": torch.cuda.get_device_name(0)}
    for B, n, k in SHAPES:
        clouds = torch.from_numpy(np.random.RandomState(B + n).uniform(-0.5, 0.5, (B, n, 3)).astype(np.float32)).cuda()
        bufs = ops.axis_split_buffers(B, n, k, "cuda")
        kernel = lambda: ops.axis_split(clouds, k, 0, out=bufs)
        plain = lambda: torch_split(clouds, k, 0)
        kernel()
        want = plain()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(g.long() if g.dtype == torch.int32 else g, w))
                   for g, w in zip((bufs["lower"], bufs["upper"], bufs["order"]), want))
        k_ms, t_ms = [], []
        for _ in range(args.repeats):
            k_ms.append(event_ms(kernel))
            t_ms.append(event_ms(plain))
        res = {"kernel": summary(k_ms), "torch_argsort_gather": summary(t_ms), "same_result": same}
        res["torch_over_kernel"] = round(res["torch_argsort_gather"]["median_ms"] / res["kernel"]["median_ms"], 2)
        result[f"B={B},n={n},k={k}"] = res
        print(f"B={B},n={n},k={k}", json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

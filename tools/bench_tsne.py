#!/usr/bin/env python3
"""Exact t-SNE on the GPU (GPU box only): how long its three stages take at the sizes of make_tsne_reduction — a category's
training set plus the test rows, n = 5 000, as decoder weights (d = 19 011) and as latents (d = 256).  A record, not a gate.

    python tools/bench_tsne.py [--out FILE.json] [--repeats 5] [--iters 1000]

Stages: hp_pairwise_sqdist, hp_tsne_affinities (perplexity 30), and hp_tsne_descend over --iters iterations with the KL of
the result (explore 250, exaggeration 12, the 'auto' learning rate), from a seeded 1e-4 normal start.  Seeded rows with a
large common part, as weight vectors of similar shapes have.  Device-event time of one call, warmed up; the median and the
extremes of --repeats calls.  The classical-scaling start (torch.linalg.eigh, plumbing) is timed once beside them.
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

SHAPES = ((5000, 19011), (5000, 256))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsne.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    from hyperpocket_amd.utils.tsne import auto_learning_rate, classical_scaling
    result = {"device": torch.cuda.get_device_name(0), "iterations": args.iters, "shapes": []}
    for n, d in SHAPES:
        g = torch.Generator().manual_seed(n + d)
        X = (3 * torch.randn(1, d, generator=g) + 0.05 * torch.randn(n, d, generator=g)).cuda()
        D = torch.empty((n, n), device="cuda")
        ws = torch.empty((n * n + n + 1,), device="cuda")
        Y0 = (1e-4 * torch.randn(n, 2, generator=g)).cuda()
        lr = auto_learning_rate(n, 12.0)
        kl = torch.zeros(3, device="cuda")
        held = {}

        def distances():
            ops.pairwise_sqdist(X, out=D)

        def affinities():
            held["P"] = ops.tsne_affinities(D, 30.0, ws=ws)

        def descent():
            Y = Y0.clone()
            update, gains, rowacc = ops.tsne_state(Y)
            ops.tsne_descend(held["P"][0], Y, update, gains, rowacc, 0, args.iters, 250, 12.0, lr, kl=kl)
            held["Y"] = Y

        row = {"n": n, "d": d}
        for name, fn in (("distances", distances), ("affinities", affinities), ("descent", descent)):
            fn()
            torch.cuda.synchronize()
            row[name] = summary([event_ms(fn) for _ in range(args.repeats)])
        row["descent"]["per_iteration_us"] = round(1000 * row["descent"]["median_ms"] / max(args.iters, 1), 3)
        row["kl"] = round(float(kl[0]), 5)
        row["search_steps_max"] = int(held["P"][2].max())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        classical_scaling(D)
        torch.cuda.synchronize()
        row["classical_scaling_start_ms_once"] = round(1000 * (time.perf_counter() - t0), 1)
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One step of rigid registration on the GPU (GPU box only): how long ops.scan_align_step and a whole ops.scan_align take
next to the same step written as a plain torch expression on the same device.

    python tools/bench_align.py [--out profiles/align.json] [--repeats 20] [--yardstick-repeats 5]

Shapes (S pairs of n source rows against m target rows, H transforms per pair), seeded: the target is uniform in [-1, 1]^3,
the source a subset of it moved by a few degrees and some noise.
    object  256 pairs of 2048 x 4096 rows, H = 1     a refinement step over a dataset of cleaned scans
    yaw     the same with H = 24                      a step of the yaw search
    scan    8 pairs of 32768 x 65536 rows, H = 1      the largest sets the kernel takes

Legs, warmed up, medians:
    scan_align_step   device-event time of one call (a memset and one launch), outputs reused
    scan_align        wall-clock time of ten steps of the driver (H = 1 shapes), synchronised before and after: per step the
                      kernel, the moments read back, the solve on the host, the transforms sent
    torch_step        device-event time of the yardstick: the rows moved by a batched matrix product, torch.cdist and
                      min(-1), the matched rows gathered and their masked sums — in fp32, not bound to the law
There is no reference implementation and no earlier timing of this operation: the ratio to torch_step is reported and
nothing is gated.  `pairs_per_ns` is S * n * m * H over the median scan_align_step time.
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

SHAPES = (("object", 256, 2048, 4096, 1), ("yaw", 256, 2048, 4096, 24), ("scan", 8, 32768, 65536, 1))
MAX_DIST = 0.1
SLICE_BYTES = 1 << 32                  # distance matrices the yardstick holds at a time


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


def inputs(S, n, m, H):
    """(sources (S,n,3), targets (S,m,3), transforms (S,H,12)) float32 on the device."""
    g = torch.Generator(device="cuda").manual_seed(S + n + m)
    targets = torch.rand((S, m, 3), generator=g, device="cuda") * 2 - 1
    picks = torch.rand((S, m), generator=g, device="cuda").argsort(1)[:, :n]
    sources = torch.gather(targets, 1, picks.unsqueeze(-1).expand(-1, -1, 3))
    sources = sources + torch.randn((S, n, 3), generator=g, device="cuda") * 0.005
    r = np.random.RandomState(H)
    out = np.zeros((S, H, 3, 4), dtype=np.float32)
    for s in range(S):
        for h in range(H):
            k = r.normal(size=3)
            k /= np.linalg.norm(k)
            a = np.radians(r.uniform(-5, 5))
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            out[s, h, :, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
            out[s, h, :, 3] = r.uniform(-0.02, 0.02, 3)
    return sources.contiguous(), targets.contiguous(), torch.from_numpy(out.reshape(S, H, 12)).cuda()


def torch_step(sources, targets, transforms, gate, sums):
    """sums (S,H,17) float32: count, sum p' (3), sum q (3), sum p' q^T (9), sum |p' - q|^2 of the gated matches."""
    S, n, _ = sources.shape
    m, H = targets.size(1), transforms.size(1)
    per = max(1, SLICE_BYTES // (n * m * 4))
    for h in range(H):
        M = transforms[:, h].view(S, 3, 4)
        for lo in range(0, S, per):
            hi = min(S, lo + per)
            moved = torch.baddbmm(M[lo:hi, :, 3].unsqueeze(1), sources[lo:hi], M[lo:hi, :, :3].transpose(1, 2))
            d, j = torch.cdist(moved, targets[lo:hi]).min(-1)
            q = torch.gather(targets[lo:hi], 1, j.unsqueeze(-1).expand(-1, -1, 3))
            w = (d <= gate).to(torch.float32).unsqueeze(-1)
            sums[lo:hi, h, 0] = w.sum((1, 2))
            sums[lo:hi, h, 1:4] = (moved * w).sum(1)
            sums[lo:hi, h, 4:7] = (q * w).sum(1)
            sums[lo:hi, h, 7:16] = torch.einsum("sna,snb->sab", moved * w, q).reshape(hi - lo, 9)
            sums[lo:hi, h, 16] = ((moved - q).square() * w).sum((1, 2))
    return sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--yardstick-repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    result = {"device": torch.cuda.get_device_name(0), "max_dist": MAX_DIST, "shapes": {}}
    for what, S, n, m, H in SHAPES:
        sources, targets, transforms = inputs(S, n, m, H)
        points, tpoints = sources.view(-1, 3), targets.view(-1, 3)
        offsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * n
        toffsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * m
        anchor, shift = ops.align_frame(tpoints, toffsets, MAX_DIST)
        out = ops.scan_align_step(points, offsets, tpoints, toffsets, transforms, MAX_DIST, anchor, shift)
        kernel = lambda: ops.scan_align_step(points, offsets, tpoints, toffsets, transforms, MAX_DIST, anchor, shift, out=out)
        driver = lambda: ops.scan_align(points, offsets, tpoints, toffsets, MAX_DIST, iters=9)     # nine steps and the final one
        sums = torch.zeros((S, H, 17), device="cuda")
        yardstick = lambda: torch_step(sources, targets, transforms, MAX_DIST, sums)
        kernel()                                                       # warm-up: the code objects
        yardstick()                                                    # ... the yardstick's libraries
        times = {"scan_align_step": [], "torch_step": [], "scan_align": []}
        if H == 1:
            driver()
        for _ in range(args.yardstick_repeats):                        # alternate the legs
            times["scan_align_step"] += event_ms(kernel, max(1, -(-args.repeats // args.yardstick_repeats)))
            times["torch_step"] += event_ms(yardstick, 1)
            if H == 1:
                times["scan_align"].append(wall_ms(driver)[0])
        res = {name: summary(ms) for name, ms in times.items() if ms}
        res["plan"] = dict(zip(("threads", "rows_per_lane", "hypothesis_group", "tile"), ops.scan_align_plan(H)))
        res["pairs"] = S * n * m * H
        res["pairs_per_ns"] = round(res["pairs"] / (res["scan_align_step"]["median_ms"] * 1e6), 2)
        res["torch_over_scan_align_step"] = round(res["torch_step"]["median_ms"] / res["scan_align_step"]["median_ms"], 2)
        used = out["moments"][:, :, 0].double()
        res["matched_share_mean"] = round(float(used.mean()) / n, 4)
        res["count_ratio"] = round(float(sums[:, :, 0].double().sum() / used.sum()), 5)      # the yardstick counts the same matches
        result["shapes"][f"{what},S={S},n={n},m={m},H={H}"] = res
        print(f"{what},S={S},n={n},m={m},H={H}", json.dumps(res), flush=True)
        del sources, targets, points, tpoints, sums
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

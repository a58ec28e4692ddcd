#!/usr/bin/env python3
"""Distance-matrix benchmark (GPU box only): pairwise_EMD_CD — one hp_cloud_pairs call and one chunked hp_emd_pairs call over all
pairs — against _pairwise_EMD_CD_(..., batch_size=64), the Python loop over expanded copies, on seeded U(-0.5, 0.5) clouds at the
generativity experiment's shape (128 x 128 clouds of 1024 points) and at 64 x 64 clouds of 2048 points.

Both paths run in this one process, alternately (old, new, old, new, ...) after a warm-up of each at every shape; a repeat is
device-synchronised wall time of one whole call.  Per shape the medians, the spread (min, max) of both and the agreement of the
two results are recorded; the results must agree at rtol 1e-5 or the tool fails.  Prints one line per shape, then one JSON line,
and writes the JSON to --out (default profiles/r11_emd_pairs.json).

    python tools/bench_emd_pairs.py [--repeats 7] [--out PATH] [--only 128x1024|64x2048] [--pair-only]

--pair-only runs pairwise_EMD_CD alone, `--repeats` times after one warm-up call, compares and writes nothing: with
--only 128x1024 the command of the kernel trace (rocprofv3 --kernel-trace --stats) that gives emd_order_kernel's share of the
pair call.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))
from hyperpocket_amd.utils.evaluation.emd_pairs import emd_pairs_chunk  # noqa: E402
from hyperpocket_amd.utils.metrics import _pairwise_EMD_CD_, pairwise_EMD_CD  # noqa: E402

SHAPES = {"128x1024": (128, 1024), "64x2048": (64, 2048)}
RTOL = 1e-5


def clouds(count, points, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(count, points, 3, generator=g) - 0.5).cuda()


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "repeats_ms": ms}


def rel(a, b):
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    return float(np.max(np.abs(a - b) / np.abs(b)))


def measure(count, points, repeats):
    sample, ref = clouds(count, points, 11), clouds(count, points, 12)
    old = lambda: _pairwise_EMD_CD_(sample, ref, 64)
    new = lambda: pairwise_EMD_CD(sample, ref)
    _, (cd_old, emd_old) = wall_ms(old)          # the warm-up of both, and the results that are compared
    _, (cd_new, emd_new) = wall_ms(new)
    t_old, t_new = [], []
    for _ in range(repeats):
        t_old.append(wall_ms(old)[0])
        t_new.append(wall_ms(new)[0])
    res = {"clouds": count, "points": points, "pairs": count * count, "emd_chunk": min(count * count, emd_pairs_chunk(points, points)),
           "loop_batch64": spread(t_old), "pair_form": spread(t_new),
           "pair_over_loop_medians": statistics.median(t_new) / statistics.median(t_old),
           "max_rel_diff_cd": rel(cd_new, cd_old), "max_rel_diff_emd": rel(emd_new, emd_old)}
    res["pair_form_slower_than_loop_spread"] = res["pair_form"]["median_ms"] > res["loop_batch64"]["max_ms"]
    print(f"{count} x {count} clouds of {points} points ({count * count} pairs): loop {res['loop_batch64']['median_ms']:.2f} ms "
          f"[{min(t_old):.2f}, {max(t_old):.2f}], pair form {res['pair_form']['median_ms']:.2f} ms [{min(t_new):.2f}, {max(t_new):.2f}], "
          f"max rel diff CD {res['max_rel_diff_cd']:.2e} EMD {res['max_rel_diff_emd']:.2e}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_emd_pairs.json"))
    ap.add_argument("--only", choices=sorted(SHAPES), default=None)
    ap.add_argument("--pair-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_emd_pairs needs a GPU: both paths run on the HIP kernels only")
    if args.pair_only:
        for name, (count, points) in SHAPES.items():
            if args.only in (None, name):
                sample, ref = clouds(count, points, 11), clouds(count, points, 12)
                ms = [wall_ms(lambda: pairwise_EMD_CD(sample, ref))[0] for _ in range(args.repeats + 1)][1:]
                print(f"{name}: pair form alone, {args.repeats} calls after one warm-up: median {statistics.median(ms):.2f} ms")
        return
    res = {"device": torch.cuda.get_device_name(0), "timing": "device-synchronised wall time per call, old and new alternating in one process",
           "rtol": RTOL}
    for name, (count, points) in SHAPES.items():
        if args.only in (None, name):
            res[name] = measure(count, points, args.repeats)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    bad = [k for k in SHAPES if k in res and max(res[k]["max_rel_diff_cd"], res[k]["max_rel_diff_emd"]) > RTOL]
    if bad:
        sys.exit(f"the two paths disagree beyond rtol {RTOL} at {bad}")


if __name__ == "__main__":
    main()

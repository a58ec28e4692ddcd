#!/usr/bin/env python3
"""Exact EMD on record (GPU box only): how far the approximate EMD is from the true one, and what the exact solver costs.

1. The gap, at n = 2048 on the synthetic families of tests/assign_law.py (uniform, clustered, near-coincident, tie-heavy grid)
   and on a completion-like pair (a clustered cloud against a jittered copy of itself); and on the trained-state `rec`
   against `gt` of tests/golden/model_trained.npz, which has 256 points per cloud and so cannot serve at 2048.  Per pair:
   the approximate EMD (emd_pairs), the exact EMD (emd_exact_pairs), their ratio, the auction rounds.
2. The solver's time: hp_assign_pairs at n = 1024 with P = 1, 256 and 4096 pairs of uniform clouds, device-synchronised wall
   time of the whole call after one warm-up, as ms per pair; and one pair at n = 2048.
3. scipy.optimize.linear_sum_assignment on the same host and the same integer costs, per pair, at n = 1024 and 2048.

Nothing is gated: the numbers are printed, one line each, then one JSON line, and written to --out.

    python tools/bench_assign.py [--repeats 3] [--out PATH] [--skip-scipy]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from assign_law import clustered_cloud, family_pair, quantised_costs  # noqa: E402
from hyperpocket_amd.utils.evaluation.emd_exact import emd_exact_pairs  # noqa: E402
from hyperpocket_amd.utils.evaluation.emd_pairs import emd_pairs  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def gap(names, A, B):
    """One line and one record per diagonal pair of the sets A, B (numpy)."""
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    pairs = [(k, k) for k in range(len(A))]
    approx = emd_pairs(dA, dB, pairs).double().cpu().numpy()
    cost, _, rounds = emd_exact_pairs(dA, dB, pairs, return_assignment=True)
    exact, rounds = cost.cpu().numpy(), rounds.cpu().numpy()
    n, out = A.shape[1], []
    for k, name in enumerate(names):
        rec = {"pair": name, "n": n, "approx_emd": approx[k] / n, "exact_emd": exact[k] / n,
               "approx_over_exact": approx[k] / exact[k] if exact[k] > 0 else None, "rounds": int(rounds[k])}
        ratio = "n/a" if rec["approx_over_exact"] is None else "%.4f" % rec["approx_over_exact"]
        print(f"n={n} {name}: approx EMD {rec['approx_emd']:.6f}  exact EMD {rec['exact_emd']:.6f}  approx/exact {ratio}  "
              f"rounds {rec['rounds']}", flush=True)
        out.append(rec)
    return out


def timing(n, P, repeats, seed=3):
    g = torch.Generator().manual_seed(seed)
    count = max(1, min(64, int(np.ceil(np.sqrt(P)))))
    A = (torch.rand(count, n, 3, generator=g) - 0.5).cuda()
    B = (torch.rand(count, n, 3, generator=g) - 0.5).cuda()
    pairs = torch.stack([torch.arange(count).repeat_interleave(count), torch.arange(count).repeat(count)], 1)[:P]
    pairs = pairs.to(torch.int32).cuda()
    run = lambda: emd_exact_pairs(A, B, pairs, return_assignment=True)
    _, (_, _, rounds) = wall_ms(run)
    ms = [wall_ms(run)[0] for _ in range(repeats)]
    rec = {"n": n, "pairs": P, "call_ms_median": statistics.median(ms), "call_ms": ms,
           "ms_per_pair": statistics.median(ms) / P, "rounds_mean": float(rounds.float().mean()), "rounds_max": int(rounds.max())}
    print(f"hp_assign_pairs n={n} P={P}: {rec['call_ms_median']:.2f} ms per call, {rec['ms_per_pair']:.4f} ms per pair "
          f"(rounds mean {rec['rounds_mean']:.0f}, max {rec['rounds_max']})", flush=True)
    return rec


def scipy_time(n, seed=3):
    from scipy.optimize import linear_sum_assignment
    a, b = family_pair("uniform", n, seed)
    q, _ = quantised_costs(a, b)
    t0 = time.perf_counter()
    linear_sum_assignment(q)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"scipy linear_sum_assignment n={n}: {ms:.1f} ms per pair on this host (cost matrix not counted)", flush=True)
    return {"n": n, "ms_per_pair": ms}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_gap.json"))
    ap.add_argument("--skip-scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_assign needs a GPU: both EMDs run on the HIP kernels only")
    res = {"device": torch.cuda.get_device_name(0), "timing": "device-synchronised wall time per call after one warm-up"}

    names = ["uniform", "clustered", "near", "grid"]
    ab = [family_pair(f, 2048, 0) for f in names]
    rng = np.random.default_rng(0)
    base = clustered_cloud(rng, 2048)
    ab.append((base, (base + rng.normal(0.0, 0.01, base.shape)).astype(np.float32)))
    res["gap_2048"] = gap(names + ["clustered vs jittered copy"], np.stack([a for a, _ in ab]), np.stack([b for _, b in ab]))
    with np.load(os.path.join(ROOT, "tests", "golden", "model_trained.npz")) as g:
        rec, gt = np.ascontiguousarray(g["rec"].transpose(0, 2, 1)), np.ascontiguousarray(g["gt"])
    res["gap_trained_256"] = gap([f"trained rec vs gt #{k}" for k in range(len(rec))], rec, gt)

    res["solver"] = [timing(1024, P, args.repeats) for P in (1, 256, 4096)] + [timing(2048, 1, args.repeats)]
    if not args.skip_scipy:
        res["scipy"] = [scipy_time(n) for n in (1024, 2048)]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Completion-metric benchmark (GPU box only): the cloud-pair kernel (hp_cloud_pairs) against NNDistance at the same
sizes, and the full-size TMD / UHD / all-pairs MMD workloads against today's expanded-copy route on the training NN
kernel and a reference-style scipy KD-tree TMD on 16 host threads.  Prints one line per measurement, then one JSON line.

    python tools/bench_completion.py [--quick]
"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))
from hyperpocket_amd.utils.evaluation import cloud_pairs as cp  # noqa: E402
from hyperpocket_amd.utils.evaluation.completeness import uhd_per_input  # noqa: E402
from hyperpocket_amd.utils.evaluation.mmd import minimum_matching_distance_all_pairs  # noqa: E402
from hyperpocket_amd.utils.evaluation.total_mutual_diff import total_mutual_difference  # noqa: E402
from hyperpocket_amd.utils.metrics import dist_chamfer  # noqa: E402
from hyperpocket_amd.utils.pytorch_structural_losses import StructuralLossesBackend as B  # noqa: E402

VALU_PEAK = 157.3e12    # fp32 vector FLOP/s of the MI355X (packed fp32 FMA), the denominator DESIGN.md uses
FLOP_PER_PAIR = 8       # 3 sub, 1 mul, 2 fma, min (counted as in tools/bench_losses.py)


def timeit(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)))


def clouds(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) - 0.5).cuda()


def rate_lines(res, sizes):
    for b, n in sizes:
        x, y = clouds(b, n, 3, seed=1), clouds(b, n, 3, seed=2)
        idx = torch.arange(b, device="cuda")
        pairs = torch.stack([idx, idx], 1).int()
        t_nn = timeit(lambda: B.NNDistance(x, y))
        t_cp = timeit(lambda: cp.cloud_pairs(cp.CHAMFER, x, y, pairs))
        pd = 2.0 * b * n * n
        for name, t in (("NNDistance", t_nn), ("cloud_pairs chamfer", t_cp)):
            share = pd * FLOP_PER_PAIR / (t * 1e-3) / VALU_PEAK
            print(f"{name:22s} b={b} n=m={n}: {t:.3f} ms  {pd / t / 1e6:.1f} Gpair/s  {100 * share:.1f} % of VALU peak")
        res[f"rate_b{b}_n{n}"] = {"nndistance_ms": t_nn, "pairs_ms": t_cp, "pairs_over_nn": t_cp / t_nn,
                                  "pairs_valu_share": pd * FLOP_PER_PAIR / (t_cp * 1e-3) / VALU_PEAK}


def tmd_today(gen):
    """today's route: per input, the k(k-1)/2 (j, l) pairs as expanded copies through dist_chamfer (the NN kernel)."""
    S, k, N, _ = gen.shape
    j, l = torch.triu_indices(k, k, 1, device=gen.device)
    out = []
    for s in range(S):
        dl, dr = dist_chamfer(gen[s, j].contiguous(), gen[s, l].contiguous())
        out.append((dl.double().mean(1) + dr.double().mean(1)).sum() * 2.0 / (k - 1))
    return torch.stack(out)


def uhd_today(existing, gen):
    """today's route: every input repeated k times (copies) through NNDistance, max of its minima per completion."""
    S, k, N, _ = gen.shape
    ex = existing.repeat_interleave(k, 0).contiguous()
    d1 = B.NNDistance(ex, gen.reshape(S * k, N, 3).contiguous())[0]
    return d1.max(1).values.sqrt().double().view(S, k).mean(1)


def mmd_today(sample, ref, batch=64):
    """today's route: _pairwise_EMD_CD_'s CD half — each sample expanded against every chunk of references."""
    rows = []
    for i in range(sample.size(0)):
        row = []
        for r in range(0, ref.size(0), batch):
            rb = ref[r:r + batch].contiguous()
            se = sample[i].view(1, -1, 3).expand(rb.size(0), -1, -1).contiguous()
            dl, dr = dist_chamfer(se, rb)
            row.append(dl.double().mean(1) + dr.double().mean(1))
        rows.append(torch.cat(row))
    cd = torch.stack(rows)             # (n_sample, n_ref)
    return cd.min(0).values


def tmd_kdtree(gen_np, threads=16):
    """reference-style CPU line: compute_trimesh_chamfer (two scipy KD-trees per pair) over every (j<l), 16 threads."""
    from scipy.spatial import cKDTree

    def one(pcs):
        k, s = len(pcs), 0.0
        trees = [cKDTree(p) for p in pcs]
        for j in range(k):
            for l in range(j + 1, k):
                a = trees[l].query(pcs[j])[0]
                b = trees[j].query(pcs[l])[0]
                s += np.mean(np.square(a)) + np.mean(np.square(b))
        return s * 2 / (k - 1)
    with ThreadPoolExecutor(threads) as ex:
        return np.array(list(ex.map(one, [g.astype(np.float64) for g in gen_np])))


def main():
    quick = "--quick" in sys.argv
    res = {}
    rate_lines(res, [(64, 2048)] if quick else [(64, 2048), (64, 8192)])
    S, k, N, NE, NREF, NSMP = (8, 10, 512, 256, 16, 80) if quick else (64, 10, 2048, 1024, 64, 640)

    gen = clouds(S, k, N, 3, seed=3)
    t_new = timeit(lambda: total_mutual_difference(gen))
    t_old = timeit(lambda: tmd_today(gen), iters=3, warm=1)
    v_new, v_old = total_mutual_difference(gen), tmd_today(gen)
    res["tmd"] = {"S": S, "k": k, "N": N, "pairs": S * k * (k - 1) // 2, "pair_kernel_ms": t_new, "expanded_nn_ms": t_old,
                  "max_rel_diff": rel(v_new.cpu(), v_old.cpu())}
    try:
        g_np = gen.cpu().numpy()
        t0 = time.perf_counter()
        v_kd = tmd_kdtree(g_np)
        res["tmd"]["kdtree_16_threads_ms"] = (time.perf_counter() - t0) * 1e3
        res["tmd"]["kdtree_max_rel_diff"] = rel(v_new.cpu(), v_kd)
    except ImportError:
        res["tmd"]["kdtree_16_threads_ms"] = "not measured (scipy missing)"
    print(f"TMD S={S} k={k} N={N}: pair kernel {t_new:.3f} ms, expanded dist_chamfer loop {t_old:.3f} ms "
          f"(max rel diff {res['tmd']['max_rel_diff']:.2e}), KD-tree x16 threads {res['tmd']['kdtree_16_threads_ms']} ms")

    existing = clouds(S, NE, 3, seed=4)
    t_new = timeit(lambda: uhd_per_input(existing, gen))
    t_old = timeit(lambda: uhd_today(existing, gen), iters=5, warm=1)
    v_new, v_old = uhd_per_input(existing, gen), uhd_today(existing, gen)
    res["uhd"] = {"S": S, "k": k, "Ne": NE, "N": N, "pair_kernel_ms": t_new, "expanded_nn_ms": t_old,
                  "max_rel_diff": rel(v_new.cpu(), v_old.cpu()), "bit_equal": bool(torch.equal(v_new, v_old))}
    print(f"UHD S={S} k={k} Ne={NE} N={N}: pair kernel {t_new:.3f} ms, expanded NNDistance {t_old:.3f} ms "
          f"(bit-equal {res['uhd']['bit_equal']})")

    ref, sample = clouds(NREF, N, 3, seed=5), clouds(NSMP, N, 3, seed=6)
    t_new = timeit(lambda: minimum_matching_distance_all_pairs(sample, ref), iters=3, warm=1)
    t_old = timeit(lambda: mmd_today(sample, ref), iters=1, warm=1)
    v_new, v_old = minimum_matching_distance_all_pairs(sample, ref)[1], mmd_today(sample, ref)
    res["mmd_all_pairs"] = {"refs": NREF, "samples": NSMP, "N": N, "pair_kernel_ms": t_new, "expanded_nn_ms": t_old,
                            "max_rel_diff": rel(v_new.cpu(), v_old.cpu())}
    print(f"all-pairs MMD {NREF} refs x {NSMP} samples N={N}: pair kernel {t_new:.3f} ms, expanded dist_chamfer loop "
          f"{t_old:.3f} ms (max rel diff {res['mmd_all_pairs']['max_rel_diff']:.2e})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

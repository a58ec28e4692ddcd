#!/usr/bin/env python3
"""Batch production on the GPU (GPU box only): how long one hp_make_batch call takes, against one hp_slice_clouds launch
on the same clouds, and what a training step costs with the DeviceBatcher feeding it.

    python tools/bench_batcher.py [--out profiles/r10_batch_maker.json] [--steps 200] [--precondition 100]

(a) 64 seeded clouds of 2048 points, target 1024, once a uniform ball of radius 0.5 and once the cube of half-width 0.5.
    Device-event time of one hp_make_batch call (memset + search + write-out) per `groups`, and of one hp_slice_clouds
    launch, each over SEEDS candidate sequences x REPEATS calls (the time of a call follows its slowest cloud, so it is
    quoted per seed and as the mean over the seeds).  The two kernels draw different sequences from the same law; both
    report the candidates their accepted planes stand for (make_batch: index + 1 per item; slice_clouds: the accepted
    plane is looked up in a restatement of its Philox sequence) and that count over the call time.
(b) B = 64 Chamfer + EMD training steps with the bench's engine settings: the same loop on one fixed pre-made batch, with
    a DeviceBatcher producing every batch (prefetch off), and with prefetch on; wall clock around --steps steps that end
    in a device synchronise, the three loops alternated twice.
"""
import argparse
import copy
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

B, N, TARGET = 64, 2048, 1024
SEEDS, REPEATS = 6, 5
GROUPS = (1, 4, 16, 32, 64)


def clouds_of(name, m, seed):
    r = np.random.RandomState(seed)
    if name == "cube":
        return r.uniform(-0.5, 0.5, (m, N, 3)).astype(np.float32)
    d = r.standard_normal((m, N, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return (d * 0.5 * r.uniform(size=(m, N, 1)) ** (1.0 / 3.0)).astype(np.float32)


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


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on int64 tensors holding 32-bit values."""
    m32 = 0xFFFFFFFF
    for _ in range(10):
        # 32x32 -> 64-bit products in two 16-bit halves of the multiplier (int64 would overflow)
        def mul(a, x):
            lo, hi = x * (a & 0xFFFF), x * (a >> 16)
            full_lo = (lo + ((hi & 0xFFFF) << 16))
            return ((hi >> 16) + (full_lo >> 32)) & m32, full_lo & m32
        h0, l0 = mul(0xD2511F53, c0)
        h1, l1 = mul(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return c0, c1, c2, c3


def slice_clouds_candidates(planes, seed, max_rounds=30000, block=2000):
    """Candidate number + 1 of the plane hp_slice_clouds accepted, per cloud: its candidate (cloud, round, wave) is
    Philox(counter (cloud, round, wave, k), key seed) (csrc/aux_kernels.hip); the accepted plane is found by value."""
    dev = planes.device
    nb = planes.size(0)
    found = torch.zeros((nb,), dtype=torch.int64, device=dev)
    cloud = torch.arange(nb, device=dev).view(nb, 1, 1)
    wave = torch.arange(4, device=dev).view(1, 1, 4)
    for r0 in range(0, max_rounds, block):
        rnd = torch.arange(r0, r0 + block, device=dev).view(1, block, 1)
        shape = (nb, block, 4)
        p = []
        for k in range(3):
            x = philox(cloud.expand(shape), rnd.expand(shape), wave.expand(shape), torch.full(shape, k, device=dev), seed & 0xFFFFFFFF,
                       seed >> 32)
            p.append(torch.stack([(v >> 8).double() * 2.0 ** -24 for v in x[:3]], -1))
        normal = torch.linalg.cross(p[1] - p[0], p[2] - p[0])
        cand = torch.cat([normal, (normal * p[0]).sum(-1, keepdim=True)], -1)                       # (nb, block, 4, 4)
        hit = ((cand - planes.double().view(nb, 1, 1, 4)).abs().amax(-1) <= 2e-6).view(nb, block * 4)
        first = torch.where(hit.any(1), hit.int().argmax(1) + r0 * 4 + 1, torch.zeros_like(found))
        found = torch.where(found == 0, first, found)
        if bool((found > 0).all()):
            break
    return found


def part_a():
    from hyperpocket_amd import ops
    from hyperpocket_amd._lib import call, current_stream
    dev = "cuda"
    out = {}
    for name in ("ball", "cube"):
        C = torch.from_numpy(clouds_of(name, B, 1)).to(dev)
        ids = torch.arange(B, dtype=torch.int32, device=dev)
        bufs, ws = ops.make_batch_buffers(B, N, TARGET, dev), ops.make_batch_workspace(B, N, dev)
        failed = torch.zeros((1,), dtype=torch.int32, device=dev)
        res = {"make_batch": {}, "slice_clouds": {}}
        for g in GROUPS:
            per_seed = []
            for s in range(SEEDS):
                streams = torch.arange(B, dtype=torch.int64, device=dev) + 1000 * s
                fn = lambda: ops.make_batch(C, ids, streams, TARGET, seed=s, groups=g, out=bufs, ws=ws, failed=failed)
                fn()
                torch.cuda.synchronize()
                ms = sorted(event_ms(fn, REPEATS))[REPEATS // 2]
                cands = int((bufs["index"].long() + 1).sum())
                per_seed.append({"ms": ms, "candidates": cands, "worst_item": int(bufs["index"].max()) + 1})
            mean_ms = float(np.mean([p["ms"] for p in per_seed]))
            res["make_batch"][f"groups={g}"] = {
                "call_ms_mean": mean_ms, "call_ms_per_seed": [round(p["ms"], 4) for p in per_seed],
                "candidates_per_call_mean": float(np.mean([p["candidates"] for p in per_seed])),
                "worst_item_candidates_per_seed": [p["worst_item"] for p in per_seed],
                "accepted_sequence_candidates_per_s": float(sum(p["candidates"] for p in per_seed) / sum(p["ms"] for p in per_seed) * 1e3)}
        assert int(failed.item()) == 0
        a, b_ = torch.empty((B, TARGET, 3), device=dev), torch.empty((B, N - TARGET, 3), device=dev)
        plane, status = torch.empty((B, 4), device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
        per_seed = []
        for s in range(SEEDS):
            import ctypes
            fn = lambda: call("hp_slice_clouds", B, N, TARGET, C, ctypes.c_ulonglong(s), 100000, a, b_, plane, status, current_stream(dev))
            fn()
            torch.cuda.synchronize()
            ms = sorted(event_ms(fn, REPEATS))[REPEATS // 2]
            assert int(status.max()) == 0
            found = slice_clouds_candidates(plane, s)
            assert bool((found > 0).all()), "an accepted plane was not found in the restated sequence"
            # the kernel tests four candidates per round: whole rounds are its unit of work
            per_seed.append({"ms": ms, "candidates": int((((found + 3) // 4) * 4).sum()), "worst_item": int(found.max())})
        res["slice_clouds"] = {
            "call_ms_mean": float(np.mean([p["ms"] for p in per_seed])), "call_ms_per_seed": [round(p["ms"], 4) for p in per_seed],
            "candidates_per_call_mean": float(np.mean([p["candidates"] for p in per_seed])),
            "worst_item_candidates_per_seed": [p["worst_item"] for p in per_seed],
            "tested_candidates_per_s": float(sum(p["candidates"] for p in per_seed) / sum(p["ms"] for p in per_seed) * 1e3)}
        out[name] = res
        print(name, json.dumps(res), flush=True)
    return out


def part_b(steps, warmup, precondition):
    import bench
    from hyperpocket_amd import ops
    from hyperpocket_amd.core.engine import TrainEngine
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.datasets.device_dataset import DeviceBatcher, DeviceDataset
    from hyperpocket_amd.model.full_model import FullModel
    dev = torch.device("cuda", 0)
    torch.manual_seed(2020)
    model = FullModel(copy.deepcopy(bench.MODEL_CFG))
    model.apply(weights_init)
    model = model.to(dev)
    with torch.no_grad():
        for head in model.hyper_network.output:
            head.weight.mul_(2.0 ** -6)
    engine = TrainEngine(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, loss_coef=0.05, emd_coef=0.05)
    data = DeviceDataset(clouds_of("cube", 1024, 2))
    fixed = [t.clone() for t in next(iter(DeviceBatcher(data, B, target=TARGET, seed=9)))[:3]]
    for _ in range(precondition):
        engine.step(*fixed, epoch=1)

    def fixed_loop(n):
        for _ in range(n):
            engine.step(*fixed, epoch=1)

    def batcher_loop(batcher):
        def loop(n):
            done = 0
            while done < n:
                for ex, mi, gt, _ in batcher:
                    engine.step(ex, mi, gt, epoch=1)
                    done += 1
                    if done == n:
                        break
        return loop

    plain = DeviceBatcher(data, B, target=TARGET, rotate=True, seed=9)
    ahead = DeviceBatcher(data, B, target=TARGET, rotate=True, seed=9, prefetch=True)
    legs = {"fixed_batch": fixed_loop, "batcher": batcher_loop(plain), "batcher_prefetch": batcher_loop(ahead)}
    times = {k: [] for k in legs}
    gc.collect()
    gc.disable()
    try:
        for _ in range(2):
            for name, loop in legs.items():
                loop(warmup)
                engine.finish_pending()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop(steps)
                engine.finish_pending()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / steps * 1e3)
    finally:
        gc.enable()
        ops.clear_grad_views()
    assert plain.failures() == 0 and ahead.failures() == 0
    out = {"steps": steps, "warmup": warmup, "precondition": precondition,
           "step_ms": {k: {"runs": [round(x, 4) for x in v], "best": round(min(v), 4)} for k, v in times.items()}}
    print("step", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_batch_maker.json"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precondition", type=int, default=100)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batcher.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    result = {"shape": {"B": B, "N": N, "target": TARGET, "seeds": SEEDS, "repeats": REPEATS},
              "default_groups": ops.make_batch_default_groups(B), "production": part_a()}
    if not args.skip_steps:
        result["training_step"] = part_b(args.steps, args.warmup, args.precondition)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

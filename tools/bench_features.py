#!/usr/bin/env python3
"""Global registration on the GPU (GPU box only): how long the kernels of csrc/features.hip and csrc/pose_trials.hip take next
to the same quantities from plain torch expressions on the same device.

    python tools/bench_features.py [--out profiles/features.json] [--repeats 10] [--yardstick-repeats 3]

Shapes (S sets of n source rows against m target rows), seeded: two independent samplings of a bumpy sheet per set, noise
0.002, the source turned 140 degrees about (1, 2, 3) and shifted; lists over k = 32 and normals facing each side's sensor.
    objects  S = 256, n = 2 048,  m = 4 096
    scenes   S = 8,   n = 32 768, m = 65 536 (the cap)
Per shape, warmed up, the median and the extremes of the device-event time of:
    scan_features       the source side's descriptors from given lists and normals (two launches), outputs reused
    scan_feature_match  the nearest target descriptor of every source row
    scan_pose_trials    32 768 trials, keep 1 024, inlier distance 0.05
    scan_align_global   the whole chain (both sides' lists, normals and descriptors, the match, the trials, its host read)
    torch_cdist_argmin  the yardstick of the match: torch.cdist over float descriptors and argmin, set by set, 8 192 source rows
                        at a time
    torch_inlier_count  the yardstick of the score: the kept transforms of the same call applied to the matched rows by one
                        einsum per 128 transforms, the squared distances to their targets gated and summed, argmax
The legs alternate.  `match_agree` is the share of rows on which the yardstick's argmin is the kernel's match (cdist is not
exact; the kernel's own check is tests/test_features_gpu.py), `winner_inliers` the two winners' counts.  Every shape runs in a
process of its own under a time limit, and the first that fails ends the run.  No ratio is required and nothing is gated on
these figures; no reference implementation and no earlier timing of these stages exist.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

SHAPES = (("objects", 256, 2_048, 4_096), ("scenes", 8, 32_768, 65_536))
K, TRIALS, KEEP, DIST = 32, 32_768, 1_024, 0.05
STEP_SECONDS = 420


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def child(what, S, n, m, repeats, rounds):
    import numpy as np
    import torch
    from hyperpocket_amd import ops

    def event_ms(fn, count):
        out = []
        for _ in range(count):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    r = np.random.RandomState(S + n)
    ph = r.uniform(0, 6, (S, 1))                                    # a surface of its own for every set

    def sheet(rows):
        x, y = r.uniform(-1, 1, (2, S, rows))
        z = 0.25 * np.sin(2.1 * x + ph) * np.cos(1.7 * y) + 0.15 * np.sin(3.3 * x * y + ph) + 0.2 * x * x - 0.1 * y
        return (np.stack([x, y, z], axis=2) + 0.002 * r.normal(size=(S, rows, 3))).reshape(-1, 3)

    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    a = np.radians(140.0)
    R, t = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx), np.array([0.3, -0.2, 0.5])
    up = np.array([0.0, 0.0, 5.0])
    tpoints = torch.from_numpy(sheet(m).astype(np.float32)).cuda()
    points = torch.from_numpy(((sheet(n) - t) @ R).astype(np.float32)).cuda()
    offsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * n
    toffsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * m
    views = torch.tensor((up - t) @ R, dtype=torch.float32, device="cuda")
    tviews = torch.tensor(up, dtype=torch.float32, device="cuda")

    def describe(p, o, v):
        index, _ = ops.knn_points(p, o, K)
        return index, ops.scan_normals(p, o, K, viewpoints=v, index=index)[0]

    index, normals = describe(points, offsets, views)
    tindex, tnormals = describe(tpoints, toffsets, tviews)
    fout = {"features": torch.empty((S * n, 36), dtype=torch.uint8, device="cuda"),
            "count": torch.empty((S * n,), dtype=torch.int32, device="cuda"), "ws": torch.empty((S * n * 36,), dtype=torch.uint8, device="cuda")}
    feat, cnt = ops.scan_features(points, offsets, normals, index, out=fout)
    tfeat, tcnt = ops.scan_features(tpoints, toffsets, tnormals, tindex)
    mout = {"match": torch.empty((S * n,), dtype=torch.int32, device="cuda"), "dist": torch.empty((S * n,), dtype=torch.int32, device="cuda")}
    match, _ = ops.scan_feature_match(feat, offsets, tfeat, toffsets, cnt, tcnt, out=mout)
    ws = torch.empty((S * KEEP * 14,), dtype=torch.int32, device="cuda")
    pout = ops.scan_pose_trials(points, offsets, tpoints, toffsets, match, DIST, trials=TRIALS, keep=KEEP, ws=ws)
    ff, tff = feat.float().view(S, n, 36), tfeat.float().view(S, m, 36)
    absent = (tcnt.view(S, m) <= 0)

    def cdist_argmin():
        out = torch.empty((S, n), dtype=torch.int64, device="cuda")
        for s in range(S):
            for i0 in range(0, n, 8192):
                d = torch.cdist(ff[s, i0:i0 + 8192], tff[s])
                d[:, absent[s]] = float("inf")
                out[s, i0:i0 + 8192] = d.argmin(dim=1)
        return out

    hyp = ws[:S * KEEP * 12].view(torch.float32).view(S, KEEP, 3, 4)
    P = points.view(S, n, 3)
    Q = tpoints.view(S, m, 3).gather(1, match.view(S, n, 1).clamp(min=0).long().expand(S, n, 3))
    matched = match.view(S, n) >= 0

    def inlier_count():
        counts = torch.empty((S, KEEP), dtype=torch.int64, device="cuda")
        for h0 in range(0, KEEP, 128):
            M = hyp[:, h0:h0 + 128]
            moved = torch.einsum("shab,snb->shna", M[..., :3], P) + M[..., 3].unsqueeze(2)
            d2 = (moved - Q.unsqueeze(1)).square().sum(dim=3)
            counts[:, h0:h0 + 128] = ((d2 <= DIST * DIST) & matched.unsqueeze(1)).sum(dim=2)
        live = torch.arange(KEEP, device="cuda").unsqueeze(0) < pout["kept"].unsqueeze(1)
        return torch.where(live, counts, torch.full_like(counts, -1)).max(dim=1)

    legs = {"scan_features": lambda: ops.scan_features(points, offsets, normals, index, out=fout),
            "scan_feature_match": lambda: ops.scan_feature_match(feat, offsets, tfeat, toffsets, cnt, tcnt, out=mout),
            "scan_pose_trials": lambda: ops.scan_pose_trials(points, offsets, tpoints, toffsets, match, DIST, trials=TRIALS, keep=KEEP,
                                                             out=pout, ws=ws),
            "scan_align_global": lambda: ops.scan_align_global(points, offsets, tpoints, toffsets, DIST, k=K, trials=TRIALS, keep=KEEP,
                                                               viewpoints=views, tviewpoints=tviews),
            "torch_cdist_argmin": cdist_argmin, "torch_inlier_count": inlier_count}
    slow = ("torch_cdist_argmin", "torch_inlier_count")
    for fn in legs.values():                                        # warm-up: code objects and libraries
        fn()
    times = {name: [] for name in legs}
    for _ in range(rounds):                                         # alternate the legs
        for name, fn in legs.items():
            times[name] += event_ms(fn, 1 if name in slow else max(1, -(-repeats // rounds)))
    res = {"sets": S, "source_rows": n, "target_rows": m, "k": K, "trials": TRIALS, "keep": KEEP,
           "plan": {"features": ops.scan_features_plan(K), "match": ops.scan_feature_match_plan(),
                    "pose_trials": ops.scan_pose_trials_plan(TRIALS, KEEP)}}
    res.update({name: summary(ms) for name, ms in times.items()})
    have = cnt.view(S, n) > 0
    res["match_agree"] = float((cdist_argmin()[have] == match.view(S, n)[have]).float().mean())
    best = inlier_count()
    res["winner_inliers"] = {"kernel": pout["inliers"].tolist()[:8], "torch": best.values.tolist()[:8]}
    res["found"] = int(pout["found"].sum())
    res["valid_median"], res["kept_median"] = int(pout["valid"].median()), int(pout["kept"].median())
    res["descriptors"] = int(have.sum())
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--yardstick-repeats", type=int, default=3)
    ap.add_argument("--child", nargs=4, metavar=("SHAPE", "S", "N", "M"))
    args = ap.parse_args()
    if args.child:
        what, S, n, m = args.child
        return child(what, int(S), int(n), int(m), args.repeats, args.yardstick_repeats)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_features.py measures on the GPU: none here")
    result = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for what, S, n, m in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what, str(S), str(n), str(m), "--repeats", str(args.repeats),
               "--yardstick-repeats", str(args.yardstick_repeats)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=STEP_SECONDS, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{what}: no result within {STEP_SECONDS} s; stopping")
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            raise SystemExit(f"{what}: exit {done.returncode}; stopping\n{done.stdout[-2000:]}")
        res = json.loads(lines[-1][len("RESULT "):])
        result["shapes"][f"{what},S={S},n={n},m={m}"] = res
        print(f"{what},S={S},n={n},m={m}", json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

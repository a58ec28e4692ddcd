#!/usr/bin/env python3
"""Surface normals of ragged scans on the GPU (GPU box only): how long the kernel of csrc/normals.hip and ops.scan_normals
take next to the same quantities from plain torch expressions on the same device.

    python tools/bench_normals.py [--out profiles/normals.json] [--repeats 20] [--yardstick-repeats 5]

Shapes (S scans of n rows), seeded: a noisy sphere of radius 0.5 (sigma 0.003), rows shuffled.
    scene    S = 8,   n = 65 536 (the neighbour search's cap)
    objects  S = 256, n = 2 048
each at k = 8, 16 and 32 — the three instances.  Per shape and k, warmed up, the median and the extremes of:
    kernel        device-event time of hp_scan_normals alone: ops.scan_normals with the lists given, outputs reused
    scan_normals  device-event time of ops.scan_normals whole: knn_points, then the kernel
    knn_points    device-event time of the search alone, for the difference
    torch_eigh    device-event time of the yardstick on the same lists: the neighbours gathered, (T,k+1,3) differences, the
                  batched scatter by one einsum, torch.linalg.eigh in fp32, the first eigenvector and l0 / trace
The legs alternate.  The yardstick's normals are compared with the kernel's where the spectrum has a gap (`angle_max`, the
line angle in radians over rows with (l1 - l0) / l2 > 0.05); the kernel's own check is tests/test_normals_gpu.py.
`rows_per_us` is S * n over the median kernel time.  Every (shape, k) runs in a process of its own under a time limit, and
the first that fails ends the run.  Nothing is gated on these figures.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

SHAPES = (("scene", 8, 65_536), ("objects", 256, 2_048))
KS = (8, 16, 32)
STEP_SECONDS = 240


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def child(what, S, n, k, repeats, rounds):
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
    p = r.normal(size=(S * n, 3))
    cloud = (0.5 * p / np.linalg.norm(p, axis=1, keepdims=True) + r.normal(0, 0.003, (S * n, 3))).astype(np.float32)
    points = torch.from_numpy(cloud).cuda()
    offsets = torch.arange(S + 1, dtype=torch.int64, device="cuda") * n
    lists = {"index": torch.empty((S * n, k), dtype=torch.int32, device="cuda"),
             "dist2": torch.empty((S * n, k), dtype=torch.float32, device="cuda")}
    index, _ = ops.knn_points(points, offsets, k, out=lists)
    out = {"normal": torch.empty((S * n, 3), device="cuda"), "curvature": torch.empty((S * n,), device="cuda"),
           "count": torch.empty((S * n,), dtype=torch.int32, device="cuda")}
    base = torch.repeat_interleave(offsets[:-1], n).unsqueeze(1)

    def yardstick():
        rows = torch.cat([torch.arange(S * n, device="cuda").unsqueeze(1), base + index], dim=1)     # every slot is valid here
        d = points[rows] - points.unsqueeze(1)
        d = d - d.mean(dim=1, keepdim=True)
        lam, vec = torch.linalg.eigh(torch.einsum("nka,nkb->nab", d, d))
        return vec[:, :, 0], lam[:, 0].clamp(min=0) / lam.sum(dim=1), lam

    legs = {"kernel": lambda: ops.scan_normals(points, offsets, k, index=index, out=out),
            "scan_normals": lambda: ops.scan_normals(points, offsets, k, out=out),
            "knn_points": lambda: ops.knn_points(points, offsets, k, out=lists)}
    res = {"rows": S * n, "k": k, "plan": dict(zip(("instance_k", "threads", "sweeps"), ops.scan_normals_plan(k)))}
    try:
        vec, _, lam = yardstick()
        legs["torch_eigh"] = yardstick
    except Exception as e:                                          # a torch build without the batched solver: said, not hidden
        res["torch_eigh"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    for fn in legs.values():                                        # warm-up: code objects and libraries
        fn()
        fn()
    times = {name: [] for name in legs}
    for _ in range(rounds):                                         # alternate the legs
        for name, fn in legs.items():
            times[name] += event_ms(fn, 1 if name == "torch_eigh" else max(1, -(-repeats // rounds)))
    res.update({name: summary(ms) for name, ms in times.items()})
    res["rows_per_us"] = round(S * n / (res["kernel"]["median_ms"] * 1e3), 1)
    if "torch_eigh" in legs:
        res["torch_over_kernel"] = round(res["torch_eigh"]["median_ms"] / res["kernel"]["median_ms"], 2)
        res["torch_over_scan_normals"] = round(res["torch_eigh"]["median_ms"] / res["scan_normals"]["median_ms"], 2)
        normal = ops.scan_normals(points, offsets, k, index=index)[0].double()
        gap = ((lam[:, 1] - lam[:, 0]) / lam[:, 2]) > 0.05
        v = vec.double()
        ang = torch.atan2(torch.linalg.cross(normal, v).norm(dim=1), (normal * v).sum(dim=1).abs())
        res["angle_max"] = float(ang[gap].max())
        res["rows_compared"] = int(gap.sum())
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--yardstick-repeats", type=int, default=5)
    ap.add_argument("--child", nargs=4, metavar=("SHAPE", "S", "N", "K"))
    args = ap.parse_args()
    if args.child:
        what, S, n, k = args.child
        return child(what, int(S), int(n), int(k), args.repeats, args.yardstick_repeats)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals.py measures on the GPU: none here")
    result = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for what, S, n in SHAPES:
        for k in KS:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", what, str(S), str(n), str(k), "--repeats", str(args.repeats),
                   "--yardstick-repeats", str(args.yardstick_repeats)]
            try:
                done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=STEP_SECONDS, text=True)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{what}, k = {k}: no result within {STEP_SECONDS} s; stopping")
            lines = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
            if done.returncode != 0 or not lines:
                raise SystemExit(f"{what}, k = {k}: exit {done.returncode}; stopping\n{done.stdout[-2000:]}")
            res = json.loads(lines[-1][len("RESULT "):])
            result["shapes"][f"{what},S={S},n={n},k={k}"] = res
            print(f"{what},S={S},n={n},k={k}", json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One step of point-to-plane registration on the GPU (GPU box only): how long ops.scan_align_plane_step takes next to
ops.scan_align_step at the same shape — the baseline the new epilogue is paid against — and next to the composition the fused
kernel replaces.

    python tools/bench_align_plane.py [--out profiles/align_plane.json] [--repeats 20] [--rounds 5] [--no-trace]

Shapes (S pairs of n source rows against m target rows, H = 1), seeded: both sides are independent samplings of the sheet
z = 0.15 sin(3x) cos(2y) + 0.1 x^2 over [-1, 1]^2 with noise 0.002, the source turned by a few degrees; the targets' normals
are the sheet's own.
    object  256 pairs of 2048 x 4096 rows     a refinement step over a dataset of cleaned scans
    scan    1 pair of 65536 x 65536 rows      the largest set the kernel takes: 128 workgroups, half the device

Legs, every one warmed up, the legs alternating within a round, medians over the rounds:
    plane_step    device-event time of one ops.scan_align_plane_step (a memset and one launch), outputs reused
    point_step    the same of ops.scan_align_step
    composition   device-event time of ops.scan_align_step(want_index=True) (a memset, a fill, the sweep) followed by the 28
                  sums as a torch expression in int64 over the matched rows (gathers, the quantisation, the (hi, lo) split and
                  the column sums): what a caller without the fused kernel would run.  Its moved rows come from a batched
                  matrix product and are not bound to the law's rounding — under the identity, the transform timed here,
                  they are exact, and `composition_equals_fused_bits` says whether all 60 numbers of every job agree.
    kernels       the sweep kernels alone, from a `rocprofv3 --kernel-trace` run of a child process that does nothing but these
                  launches (device events see the memset too); skipped with --no-trace
Nothing is gated.  The file also records what the CPU suites assert (tests/test_align_plane_law_host.py) and the two
degeneracy ratios, measured here with tests/align_plane_law.py.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

SHAPES = (("object", 256, 2048, 4096), ("scan", 1, 65536, 65536))
MAX_DIST = 0.1
WARMUP = 3
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)] + [(i, 6) for i in range(6)] + [(6, 6)]      # the 28 sums, a_6 = b


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


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def sheet(S, rows, g, device):
    """(points (S,rows,3), unit normals (S,rows,3)) float32: a noisy sampling of the sheet and the sheet's normals there."""
    xy = torch.rand((S, rows, 2), generator=g, device=device) * 2 - 1
    x, y = xy[..., 0], xy[..., 1]
    z = 0.15 * torch.sin(3 * x) * torch.cos(2 * y) + 0.1 * x * x
    n = torch.stack([-(0.45 * torch.cos(3 * x) * torch.cos(2 * y) + 0.2 * x), 0.3 * torch.sin(3 * x) * torch.sin(2 * y), torch.ones_like(x)], -1)
    points = torch.stack([x, y, z], -1) + 0.002 * torch.randn((S, rows, 3), generator=g, device=device)
    return points.contiguous(), (n / n.norm(dim=-1, keepdim=True)).contiguous()


def inputs(S, n, m, device="cuda"):
    """(sources (S,n,3), targets (S,m,3), tnormals (S,m,3), transforms (S,1,12)) float32; the identity as the transform, the
    sources turned by up to 5 degrees and shifted by up to 0.02."""
    g = torch.Generator(device=device).manual_seed(S + n + m)
    targets, tnormals = sheet(S, m, g, device)
    sources, _ = sheet(S, n, g, device)
    r = np.random.RandomState(1)
    turn = np.zeros((S, 3, 4), dtype=np.float32)
    for s in range(S):
        k = r.normal(size=3)
        k /= np.linalg.norm(k)
        a = np.radians(r.uniform(-5, 5))
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        turn[s, :, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
        turn[s, :, 3] = r.uniform(-0.02, 0.02, 3)
    turn = torch.from_numpy(turn).to(device)
    sources = torch.baddbmm(turn[:, :, 3].unsqueeze(1), sources, turn[:, :, :3].transpose(1, 2)).contiguous()
    eye = torch.eye(3, 4, device=device).reshape(1, 1, 12).repeat(S, 1, 1).contiguous()
    return sources, targets, tnormals, eye


def torch_sums(sources, targets, tnormals, transforms, index, dist2, max_dist, anchor, scale, out):
    """The epilogue of the fused kernel as a torch expression: out (S,60) int64 from scan_align_step's index and dist2 (1,T);
    scale (S,1,1) float32 = 2^(19 - shift), made on the host: torch.ldexp on the device is a pow and is not exact."""
    S, n, _ = sources.shape
    M = transforms[:, 0].view(S, 3, 4)
    moved = torch.baddbmm(M[:, :, 3].unsqueeze(1), sources, M[:, :, :3].transpose(1, 2))
    index, dist2 = index.view(S, n), dist2.view(S, n)
    j = index.clamp(min=0).long().unsqueeze(-1).expand(-1, -1, 3)
    q, nrm = torch.gather(targets, 1, j), torch.gather(tnormals, 1, j)
    su, sv = (moved - anchor.unsqueeze(1)) * scale, (q - anchor.unsqueeze(1)) * scale
    sn = nrm * 512.0
    corr = (index >= 0) & (dist2 <= max_dist * max_dist)
    inside = ((su.abs() < 1048576.0) & (sv.abs() < 1048576.0)).all(-1)
    small = (sn.abs() < 1024.0).all(-1)
    zero = torch.zeros((), device=su.device)
    u = torch.where(inside.unsqueeze(-1), su, zero).trunc().long()
    v = torch.where(inside.unsqueeze(-1), sv, zero).trunc().long()
    w = torch.where(small.unsqueeze(-1), sn, zero).trunc().long()
    ww = (w * w).sum(-1)
    has = small & (ww != 0) & (ww <= (1 << 18) + (1 << 11))
    use = corr & inside & has
    c = torch.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)
    b = -((u - v) * w).sum(-1, keepdim=True)
    a = torch.cat([c, w, b], -1) * use.unsqueeze(-1)
    left, right = (torch.tensor([p[k] for p in PAIRS], device=a.device) for k in (0, 1))
    terms = a[..., left] * a[..., right]
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = use.sum(1), (corr & ~inside).sum(1), (corr & inside & ~has).sum(1), 0
    out[:, 4::2] = (terms >> 31).sum(1)
    out[:, 5::2] = (terms & 0x7FFFFFFF).sum(1)
    return out


class Shape:
    def __init__(self, S, n, m):
        from hyperpocket_amd import ops
        self.ops, self.S, self.n = ops, S, n
        self.sources, self.targets, self.tnormals, self.transforms = inputs(S, n, m)
        self.sets = (self.sources.view(-1, 3), torch.arange(S + 1, dtype=torch.int64, device="cuda") * n,
                     self.targets.view(-1, 3), torch.arange(S + 1, dtype=torch.int64, device="cuda") * m)
        self.frame = ops.align_frame(self.sets[2], self.sets[3], MAX_DIST)
        self.scale = torch.from_numpy(np.ldexp(np.float32(1), 19 - self.frame[1].cpu().numpy())).cuda().view(S, 1, 1)
        self.plane_out = self.point_out = self.index_out = None
        self.sums = torch.zeros((S, 60), dtype=torch.int64, device="cuda")

    def plane(self):
        self.plane_out = self.ops.scan_align_plane_step(*self.sets, self.tnormals.view(-1, 3), self.transforms, MAX_DIST, *self.frame,
                                                        out=self.plane_out)

    def point(self):
        self.point_out = self.ops.scan_align_step(*self.sets, self.transforms, MAX_DIST, *self.frame, out=self.point_out)

    def composition(self):
        self.index_out = self.ops.scan_align_step(*self.sets, self.transforms, MAX_DIST, *self.frame, out=self.index_out, want_index=True)
        torch_sums(self.sources, self.targets, self.tnormals, self.transforms, self.index_out["index"], self.index_out["dist2"],
                   MAX_DIST, self.frame[0], self.scale, self.sums)


def trace_child(repeats):
    for _, S, n, m in SHAPES:
        shape = Shape(S, n, m)
        for leg in (shape.plane, shape.point):
            for _ in range(WARMUP + repeats):
                leg()
        torch.cuda.synchronize()


def kernel_trace(repeats):
    """Median microseconds of the two sweep kernels per shape from a rocprofv3 run of the child, or {"error": ...}."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="align_plane_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", "--repeats", str(repeats)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if done.returncode != 0 or not files:
            return {"error": f"rocprofv3 exit {done.returncode}, {len(files)} trace files", "tail": done.stdout.decode(errors="replace")[-400:]}
        rows = [r for f in files for r in csv.DictReader(open(f)) if "align_plane_sweep_kernel" in r["Kernel_Name"]
                or "align_sweep_kernel" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        per = WARMUP + repeats
        if len(rows) != 2 * per * len(SHAPES):
            return {"error": f"{len(rows)} dispatches traced, {2 * per * len(SHAPES)} expected"}
        res = {}
        for c, (what, _, _, _) in enumerate(SHAPES):
            for k, leg in enumerate(("plane_sweep_kernel", "point_sweep_kernel")):
                mine = rows[(2 * c + k) * per + WARMUP:(2 * c + k + 1) * per]
                if not all(("align_plane" in r["Kernel_Name"]) == (k == 0) for r in mine):
                    return {"error": "the dispatches are not in the order of the legs"}
                us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine)
                res.setdefault(what, {})[leg] = {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2),
                                                 "max_us": round(us[-1], 2), "dispatches": len(us)}
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def law_figures():
    """What the CPU suites assert, and the two degeneracy ratios measured here with the law."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import align_law
    import align_plane_law as law
    import test_align_plane_law_host as suite
    ratios = {}
    for name, (source, target, normals) in {"slab_pair": law.slab_pair(), "wavy_pair": law.wavy_pair()[:2] + (law.normals_of(),),
                                            "normals_law.slab (noise 0.02, not used)": law.slab_pair(noise=0.02)}.items():
        toffsets = np.array([0, len(target)])
        anchor, shift = align_law.frame(target, toffsets, suite.GATE)
        mom = law.step(source, [0, len(source)], target, toffsets, normals, np.eye(3, 4, dtype=np.float32).reshape(1, 1, 12), suite.GATE,
                       anchor, shift)["moments"][0, 0]
        ratios[name] = float(law.solve_plane(mom)[2])
    return {"degeneracy": {"scaling": "one scale per block: sqrt(mean diagonal) of the rotation and of the translation block",
                           "lambda_min_over_lambda_max": ratios, "DEGENERATE_PLANE": law.DEGENERATE_PLANE,
                           "jacobi_scaling_measured_and_not_used": {"normals_law.slab": 0.656, "slab_pair": 0.611, "wavy_pair": 0.0988}},
            "asserted": {"factor": 4,
                         "step_vs_fp64_first_step": {"omega_rad": suite.STEP_FIRST[0], "t": suite.STEP_FIRST[1]},
                         "step_vs_fp64_later_steps": {"omega_rad": suite.STEP_LATER[0], "t": suite.STEP_LATER[1]},
                         "pose_after_3_steps": {"rotation_rad": suite.POSE_ROT / 4, "translation": suite.POSE_MOVE / 4},
                         "point_to_point_after_30_steps_above": {"rotation_rad": 10 * suite.POSE_ROT, "translation": 10 * suite.POSE_MOVE}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_plane.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child run")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align_plane.py measures on the GPU: none here")
    if args.trace_child:
        return trace_child(args.repeats)
    from hyperpocket_amd import ops
    result = {"device": torch.cuda.get_device_name(0), "max_dist": MAX_DIST, "shapes": {},
              "plan": dict(zip(("threads", "rows_per_lane", "hypothesis_group", "tile"), ops.scan_align_plane_plan(1)))}
    for what, S, n, m in SHAPES:
        shape = Shape(S, n, m)
        legs = {"plane_step": shape.plane, "point_step": shape.point, "composition": shape.composition}
        for leg in legs.values():
            for _ in range(WARMUP):
                leg()
        torch.cuda.synchronize()
        times = {name: [] for name in legs}
        for _ in range(args.rounds):                                    # alternate the legs
            for name, leg in legs.items():
                times[name] += event_ms(leg, max(1, -(-args.repeats // args.rounds)))
        res = {name: summary(ms) for name, ms in times.items()}
        res["pairs"] = S * n * m
        res["pairs_per_ns"] = round(res["pairs"] / (res["plane_step"]["median_ms"] * 1e6), 2)
        res["plane_over_point_step"] = round(res["plane_step"]["median_ms"] / res["point_step"]["median_ms"], 3)
        res["composition_over_plane_step"] = round(res["composition"]["median_ms"] / res["plane_step"]["median_ms"], 3)
        mom = shape.plane_out["moments"][:, 0]
        res["used_share_mean"] = round(float(mom[:, 0].double().mean()) / n, 4)
        res["same_matches_as_point_step"] = bool((mom[:, 0] + mom[:, 2] == shape.point_out["moments"][:, 0, 0]).all())
        res["composition_used_ratio"] = round(float(shape.sums[:, 0].double().sum() / mom[:, 0].double().sum()), 6)
        res["composition_equals_fused_bits"] = bool(torch.equal(shape.sums, mom))
        result["shapes"][f"{what},S={S},n={n},m={m},H=1"] = res
        print(f"{what},S={S},n={n},m={m},H=1", json.dumps(res), flush=True)
        del shape
        torch.cuda.empty_cache()
    if not args.no_trace:
        result["kernels"] = kernel_trace(args.repeats)
        print("kernels", json.dumps(result["kernels"]), flush=True)
    result["law"] = law_figures()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

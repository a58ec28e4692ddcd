#!/usr/bin/env python3
"""Posed depth images fused into a surface on the GPU (GPU box only): how long ops.fuse_volume and ops.fuse_surface take next to
the same law written as float64 torch expressions on the same device.

    python tools/bench_fuse.py [--out profiles/fuse.json] [--repeats 10] [--yardstick-repeats 3]

Input, seeded: B = 8 images of 480 x 640 uint16 millimetres — the synthetic scene of tests/depth_law.py (a floor, a box and a
sphere seen from 1.2 m above the floor, 35 degrees down) from its eight poses, about a tenth of the pixels holes, the mask that
drops the lowest eighth of every image, window 1, the default jump (0, 0.05) —, one group of all eight, fused into 256^3 voxels of
5 mm about the two objects, truncation 4 voxels, min_weight 1.
Before anything is timed, every output of the two legs — tsdf, weight, points, normals, cell, offsets — is compared bit for bit,
and the tool stops with an error when one differs: the legs then do not do the same work.
Warmed up, the legs alternating in one process, the median and the extremes of device-event times of:
    fuse           one ops.fuse_volume and one ops.fuse_surface (five launches), outputs and workspaces reused, intrinsics and
                   poses prepared once on the device, the row capacity fixed beforehand so that nothing synchronises; the
                   interval still holds the wrappers' host checks, two small uploads (the group tables) and the ctypes calls.
                   fuse_volume and fuse_surface are also timed on their own
    torch_law      the yardstick: the keep test by shifted comparisons, the voxel loop as broadcast float64 expressions image by
                   image, the crossings by shifted volumes, nonzero, and a sort of the cells into the law's order
What bounds the call, from the shapes: `bytes` is what the law must move — 8 per voxel written (tsdf and weight), the depth and
mask bytes read, 32 per row written (point, normal, cell), the offsets; `fp64_ops` is the rounded operations of the voxel loop,
30 per voxel and image that runs the whole chain (3 of them divisions), an upper count: a voxel behind a camera or outside an
image stops early.  `hbm_bound_ms` = bytes over the achievable HBM rate of 6.3e12 bytes/s, `fp64_bound_ms` = fp64_ops over 39.3e12
operations/s (the data sheet's 78.6 TFLOPS of the fp64 vector pipe count a fused multiply-add as two; the law has none);
`bound` names the larger and `share_of_bound` is that time over the median.  Kernel times, the division's real cost and the
cache behaviour of the gather are not measured.  The ratio of the legs is recorded; the one condition is that it exceeds 1.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))                       # depth_law: the scene

B, H, W, WINDOW, JUMP = 8, 480, 640, 1, (0.0, 0.05)
DIMS, VOXEL = (256, 256, 256), 0.005
TRUNCATION = 4 * VOXEL
ORIGIN = (-0.70, -0.24, 0.90)                                          # the box and the sphere stand on y = 0 between z = 1.3 and 1.7
HBM_BYTES_PER_S = 6.3e12                                               # achievable, not the 8e12 of the data sheet
FP64_OPS_PER_S = 39.3e12                                               # 78.6e12 FLOPS with a fused multiply-add counted twice
OPS_PER_VOXEL_IMAGE = 30                                               # 4 sub, 12 mul, 11 add, 3 div: the whole chain


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


def _shift(a, dv, du, fill):
    """out[b, v, u] = a[b, v + dv, u + du], `fill` outside the image."""
    out = torch.full_like(a, fill)
    Hh, Ww = a.shape[1:]
    v0, v1, u0, u1 = max(0, -dv), min(Hh, Hh - dv), max(0, -du), min(Ww, Ww - du)
    out[:, v0:v1, u0:u1] = a[:, v0 + dv:v1 + dv, u0 + du:u1 + du]
    return out


def _shift3(a, axis, step, fill):
    """out[c] = a[c + step along axis] of a (nz, ny, nx) volume, `fill` outside; axis 0, 1, 2 = x, y, z."""
    out = torch.full_like(a, fill)
    ax = 2 - axis
    n = a.size(ax)
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    src[ax], dst[ax] = (slice(1, n), slice(0, n - 1)) if step > 0 else (slice(0, n - 1), slice(1, n))
    out[tuple(dst)] = a[tuple(src)]
    return out


def torch_volume(depth, K, poses, masks, scale, w, jump, origin, dims, voxel, truncation):
    """(tsdf, weight) of one group of all images by the law's expressions in torch."""
    jump_abs, jump_rel = jump
    z = depth.double() * scale
    meas = torch.isfinite(z) & (z > 0)
    zz = torch.where(meas, z, 1.0)
    jumps = lambda a, b: (a - b).abs() > jump_abs + jump_rel * torch.minimum(a, b)
    keep = meas & (masks != 0)
    for dv in range(-w, w + 1):
        for du in range(-w, w + 1):
            if dv or du:
                keep &= ~(_shift(meas, dv, du, False) & jumps(zz, _shift(zz, dv, du, 1.0)))
    nx, ny, nz = dims
    dev = depth.device
    c = [origin[a] + (torch.arange(n, device=dev, dtype=torch.float64) + 0.5) * voxel for a, n in enumerate(dims)]
    c = [c[0].view(1, 1, nx), c[1].view(1, ny, 1), c[2].view(nz, 1, 1)]
    F = torch.zeros((nz, ny, nx), device=dev, dtype=torch.float64)
    n = torch.zeros((nz, ny, nx), device=dev, dtype=torch.int32)
    Hh, Ww = depth.shape[1:]
    for b in range(depth.size(0)):
        fx, fy, cx, cy = K[b].tolist()
        M = poses[b].double().tolist()
        d = [c[a] - M[a][3] for a in range(3)]
        q = [(M[0][a] * d[0] + M[1][a] * d[1]) + M[2][a] * d[2] for a in range(3)]
        uf = torch.floor((((q[0] * fx) / q[2]) + cx) + 0.5)
        vf = torch.floor((((q[1] * fy) / q[2]) + cy) + 0.5)
        ok = (q[2] > 0) & (uf >= 0) & (uf <= Ww - 1) & (vf >= 0) & (vf <= Hh - 1)
        u, v = torch.where(ok, uf, 0.0).long(), torch.where(ok, vf, 0.0).long()
        ok &= keep[b][v, u]
        s = torch.where(ok, z[b][v, u], 0.0) - q[2]
        ok &= ~(s < -truncation)
        f = s / truncation
        F = torch.where(ok, F + torch.where(f > 1, 1.0, f), F)
        n = n + ok
    tsdf = torch.where(n > 0, F / n.clamp(min=1).double(), 1.0).float()
    return tsdf.unsqueeze(0), n.unsqueeze(0)


def torch_surface(tsdf, weight, origin, voxel, min_weight):
    """(points, normals, cell, offsets) of one volume by the law's expressions in torch."""
    f, use = tsdf[0].double(), weight[0] >= min_weight
    nz, ny, nx = f.shape
    dev = f.device
    grad = [torch.where(_shift3(use, d, 1, False), _shift3(f, d, 1, 0.0), f) - torch.where(_shift3(use, d, -1, False), _shift3(f, d, -1, 0.0), f)
            for d in range(3)]
    idx = [torch.arange(n, device=dev, dtype=torch.float64) for n in (nx, ny, nz)]
    centre = [(origin[0] + (idx[0] + 0.5) * voxel).view(1, 1, nx), (origin[1] + (idx[1] + 0.5) * voxel).view(1, ny, 1),
              (origin[2] + (idx[2] + 0.5) * voxel).view(nz, 1, 1)]
    P, N, C = [], [], []
    for e in range(3):
        fb = _shift3(f, e, 1, 0.0)
        row = use & _shift3(use, e, 1, False) & ((f < 0) != (fb < 0))
        at = torch.nonzero(row.view(-1)).view(-1)
        pick = lambda x: x.expand(nz, ny, nx).reshape(-1)[at]
        fa, fbr = pick(f), pick(fb)
        t = fa / (fa - fbr)
        p = [pick(centre[d]) + t * voxel if d == e else pick(centre[d]) for d in range(3)]
        m = [pick(grad[d]) + t * (pick(_shift3(grad[d], e, 1, 0.0)) - pick(grad[d])) for d in range(3)]
        l = torch.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        unit = torch.isfinite(l) & (l != 0)
        P.append(torch.stack(p, 1))
        N.append(torch.stack([torch.where(unit, x / l, 0.0) for x in m], 1))
        C.append(at * 3 + e)
    P, N, C = torch.cat(P), torch.cat(N), torch.cat(C)
    C, order = torch.sort(C)
    offsets = torch.tensor([0, C.numel()], device=dev, dtype=torch.int64)
    return P[order].float(), N[order].float(), C, offsets


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) if a.dtype == torch.float32 else bool(torch.equal(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--yardstick-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse.py measures on the GPU: none here")
    import depth_law
    from hyperpocket_amd import ops
    s = depth_law.scene(0, B, H, W)
    depth, masks = torch.from_numpy(s["depth"]).cuda(), torch.from_numpy(s["masks"]).cuda()
    K = torch.from_numpy(np.tile(s["K"], (B, 1))).cuda()
    poses = torch.from_numpy(s["poses"]).cuda()
    Kd, Md = ops.depth_points_tables(B, s["K"], s["poses"], "cuda")     # prepared once: a timed call uploads the group tables only
    origin = torch.tensor([ORIGIN], dtype=torch.float64).cuda()
    vbufs = ops.fuse_volume_buffers(B, H, W, 1, DIMS, "cuda")
    volume = lambda: ops.fuse_volume(depth, Kd, Md, None, origin, DIMS, VOXEL, TRUNCATION, masks=masks, window=WINDOW, jump=JUMP, out=vbufs,
                                     ws=vbufs["ws"])
    vol = volume()
    exact = ops.fuse_surface(vol)                                      # counts, reads the total, emits: the rows to compare
    T = int(exact["offsets"][-1])
    sbufs = ops.fuse_surface_buffers(1, DIMS, T, "cuda")
    surface = lambda: ops.fuse_surface(vol, capacity=T, out=sbufs, ws=sbufs["ws"])
    fuse = lambda: (volume(), surface())
    yard_volume = lambda: torch_volume(depth, K, poses, masks, 0.001, WINDOW, JUMP, ORIGIN, DIMS, VOXEL, TRUNCATION)
    yardstick = lambda: torch_surface(*yard_volume(), ORIGIN, VOXEL, 1)
    fuse()                                                             # warm-up: the code objects
    tsdf, weight = yard_volume()                                       # ... and the yardstick's libraries
    points, normals, cell, offsets = torch_surface(tsdf, weight, ORIGIN, VOXEL, 1)
    res = {"device": torch.cuda.get_device_name(0), "images": B, "height": H, "width": W, "window": WINDOW, "jump": list(JUMP),
           "dims": list(DIMS), "voxel": VOXEL, "truncation": TRUNCATION, "origin": list(ORIGIN), "rows": T,
           "observed_share": round(float((vol["weight"] > 0).double().mean()), 4),
           "mean_weight_observed": round(float(vol["weight"].double().sum() / (vol["weight"] > 0).sum().clamp(min=1)), 3)}
    got = {"tsdf": vol["tsdf"], "weight": vol["weight"], "points": sbufs["points"], "normals": sbufs["normals"], "cell": sbufs["cell"],
           "offsets": sbufs["offsets"]}
    want = {"tsdf": tsdf, "weight": weight, "points": points, "normals": normals, "cell": cell, "offsets": offsets}
    res["same_bits"] = {name: same_bits(got[name], want[name]) for name in got}
    if not all(res["same_bits"].values()):                             # the legs do not do the same work: nothing to compare
        raise SystemExit(f"bench_fuse.py: the torch form and the kernels differ: {res['same_bits']}; nothing was timed")
    del tsdf, weight, points, normals, cell, offsets, want
    times = {"fuse": [], "fuse_volume": [], "fuse_surface": [], "torch_law": []}
    rounds = args.yardstick_repeats
    per = max(1, -(-args.repeats // rounds))
    for _ in range(rounds):                                            # alternate the legs
        times["fuse"] += event_ms(fuse, per)
        times["torch_law"] += event_ms(yardstick, 1)
        times["fuse_volume"] += event_ms(volume, per)
        times["fuse_surface"] += event_ms(surface, per)
    res.update({name: summary(ms) for name, ms in times.items()})
    res["volume_plan"] = dict(zip(("threads", "words", "blocks_per_group", "blocks"), ops.fuse_volume_plan(B, H, W, 1, DIMS)))
    res["surface_plan"] = dict(zip(("threads", "voxels_per_lane", "chunks", "scan_threads", "scan_rounds"), ops.fuse_surface_plan(1, DIMS)))
    res["workspace_bytes"] = {"volume": vbufs["ws"].nbytes, "surface": sbufs["ws"].nbytes}
    voxels = DIMS[0] * DIMS[1] * DIMS[2]
    res["bytes"] = voxels * 8 + B * H * W * (depth.element_size() + masks.element_size()) + T * 32 + 2 * 8
    res["fp64_ops"] = voxels * B * OPS_PER_VOXEL_IMAGE
    res["fp64_ops_per_voxel_image"] = OPS_PER_VOXEL_IMAGE
    res["hbm_bytes_per_s"], res["fp64_ops_per_s"] = HBM_BYTES_PER_S, FP64_OPS_PER_S
    res["hbm_bound_ms"] = round(res["bytes"] / HBM_BYTES_PER_S * 1e3, 4)
    res["fp64_bound_ms"] = round(res["fp64_ops"] / FP64_OPS_PER_S * 1e3, 4)
    res["bound"] = "fp64" if res["fp64_bound_ms"] >= res["hbm_bound_ms"] else "hbm"
    res["share_of_bound"] = round(max(res["fp64_bound_ms"], res["hbm_bound_ms"]) / res["fuse"]["median_ms"], 4)
    res["torch_over_fuse"] = round(res["torch_law"]["median_ms"] / res["fuse"]["median_ms"], 2)
    res["not_measured"] = ["kernel times (no profiler run)", "the cost of an fp64 division in vector instructions",
                           "cache hit rates of the depth gather"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["torch_over_fuse"] > 1.0:
        raise SystemExit("bench_fuse.py: the HIP path is not faster than the torch form at this size")


if __name__ == "__main__":
    main()

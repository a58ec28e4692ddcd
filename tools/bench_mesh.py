#!/usr/bin/env python3
"""Surface sampling of decoded meshes on the GPU (GPU box only): how long one hp_mesh_sample launch takes next to the torch
composition a user would otherwise write on the device — cross, cumsum, searchsorted and gathers in fp64 — on the same
meshes.  A record, not a gate.

    python tools/bench_mesh.py [--out FILE.json] [--repeats 30]

Shapes (K, sphere, n): (640, edge depth 5: F = 8192, 2048) — fixed()'s operating point, 64 items x 10 noises — and
(8, edge depth 6: F = 32768, 2048), few large meshes whose tables live in the workspace.  Vertices: the sphere's, each pushed
out by a smooth seeded bump so that areas differ.  Device-event time of one call, warmed up, the two alternated; the median
and the extremes of --repeats calls each.  The two draw from different generators, so they are not compared point by point:
the kernel's area is checked against half the composition's summed cross-product lengths (1e-9 relative) and the number of
distinct faces each of them hits is reported, before timing.  The same call is also timed under forced slice counts, which is how
the launcher's choice was looked at; hp_mesh_normals is timed alone.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

SHAPES = ((640, 5, 2048, (1, 2, 4, 8)), (8, 6, 2048, (1, 8, 32, 128)))


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


def torch_sample(verts, faces, n, generator):
    """The same distribution from torch operators, fp64: (points (K,n,3) float32, face (K,n), area (K))."""
    x = verts.double()
    f = faces.long()
    a = x[:, f[:, 0]]
    e1, e2 = x[:, f[:, 1]] - a, x[:, f[:, 2]] - a
    d = torch.linalg.cross(e1, e2, dim=2).norm(dim=2)                      # (K,F)
    cdf = torch.cumsum(d, 1)
    K = verts.size(0)
    rnd = torch.rand((3, K, n), dtype=torch.float64, device=verts.device, generator=generator)
    face = torch.searchsorted(cdf, rnd[0] * cdf[:, -1:], right=True).clamp_(max=f.size(0) - 1)
    u, v = rnd[1], rnd[2]
    fold = u + v > 1
    u, v = torch.where(fold, 1 - u, u).unsqueeze(2), torch.where(fold, 1 - v, v).unsqueeze(2)
    idx = face.unsqueeze(2).expand(-1, -1, 3)
    p = torch.gather(a, 1, idx) + u * torch.gather(e1, 1, idx) + v * torch.gather(e2, 1, idx)
    return p.float(), face, 0.5 * cdf[:, -1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py measures on the GPU: none here")
    from hyperpocket_amd import ops
    from hyperpocket_amd.utils.sphere_mesh import sphere_mesh
    lib = ops.load_library()
    result = {"device": torch.cuda.get_device_name(0)}
    for K, depth, n, forced in SHAPES:
        mesh = sphere_mesh("edge", depth)
        F, V = mesh.faces.shape[0], mesh.vertices.shape[0]
        r = np.random.RandomState(K + depth)
        direction = r.standard_normal((K, 1, 3))
        direction /= np.linalg.norm(direction, axis=2, keepdims=True)
        bump = 1.0 + 0.5 * (mesh.vertices[None].astype(np.float64) * direction).sum(2, keepdims=True) ** 2
        verts = torch.from_numpy((mesh.vertices[None] * bump * 0.3).astype(np.float32)).cuda()
        faces = torch.from_numpy(mesh.faces).cuda()
        vf = tuple(torch.from_numpy(a).cuda() for a in mesh.vertex_faces)
        gen = torch.Generator(device="cuda").manual_seed(1)
        bufs = ops.mesh_sample_buffers(K, F, n, "cuda")
        kernel = lambda: ops.mesh_sample(verts, faces, n, 1, out=bufs)
        plain = lambda: torch_sample(verts, faces, n, gen)
        points, face, area, failed = kernel()
        t_points, t_face, t_area = plain()
        torch.cuda.synchronize()
        area_ok = bool(((area - t_area).abs() <= 1e-9 * t_area).all()) and not bool(failed.any())
        hist = lambda fc: torch.zeros(K, F, device="cuda").scatter_add_(1, fc.long(), torch.ones(K, n, device="cuda"))
        threads, slices, in_lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        lib.hp_mesh_sample_plan(K, F, n, ctypes.byref(threads), ctypes.byref(slices), ctypes.byref(in_lds))
        k_ms, t_ms = [], []
        for _ in range(args.repeats):
            k_ms.append(event_ms(kernel))
            t_ms.append(event_ms(plain))
        res = {"F": F, "V": V, "plan": {"threads": threads.value, "slices": slices.value, "in_lds": in_lds.value},
               "kernel": summary(k_ms), "torch_fp64_composition": summary(t_ms), "area_agrees": area_ok,
               "faces_hit": [int((hist(face) > 0).sum()), int((hist(t_face) > 0).sum())]}
        res["torch_over_kernel"] = round(res["torch_fp64_composition"]["median_ms"] / res["kernel"]["median_ms"], 2)
        res["forced_slices"] = {}
        for s in forced:
            prev = lib.hp_mesh_sample_set_slices(s)
            try:
                fb = ops.mesh_sample_buffers(K, F, n, "cuda")
                call = lambda: ops.mesh_sample(verts, faces, n, 1, out=fb)
                call()
                same = bool(torch.equal(fb["points"], bufs["points"]) and torch.equal(fb["face"], bufs["face"]))
                res["forced_slices"][str(s)] = dict(summary([event_ms(call) for _ in range(args.repeats)]), same_bits=same)
            finally:
                lib.hp_mesh_sample_set_slices(prev)
        normals = lambda: ops.mesh_normals(verts, faces, vf)
        normals()
        res["normals"] = summary([event_ms(normals) for _ in range(args.repeats)])
        result[f"K={K},F={F},n={n}"] = res
        print(f"K={K},F={F},n={n}", json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

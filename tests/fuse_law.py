"""The law of ops.fuse_volume and ops.fuse_surface (csrc/fuse.hip, include/hyperpocket_hip.h) in numpy: posed depth images in,
a truncated signed distance volume per group of images and the ragged set of its zero crossings out.  Every floating operation
is one IEEE fp64 rounding in the association written, no library function but sqrt and floor, one cast to fp32 at the end.
Stated twice: fuse_volume_law and fuse_surface_law, vectorised, what the GPU tests call, and the *_loop forms, a per-voxel loop
in Python floats that the host tests hold the first against.  The keep test of a pixel is depth_law's, taken from there.

    voxel    (i, j, k) of group g: c = (ox + (double(i) + 0.5) * voxel, oy + (double(j) + 0.5) * voxel, oz + (double(k) + 0.5) * voxel)
    image    b of the group, in list order: d = c - t; q_a = (R_0a d0 + R_1a d1) + R_2a d2; skipped unless q2 > 0;
             x = ((q0 fx) / q2) + cx, y = ((q1 fy) / q2) + cy; u = floor(x + 0.5), v = floor(y + 0.5); skipped unless
             0 <= u <= W - 1 and 0 <= v <= H - 1 (in fp64: a NaN is outside) and pixel (v, u) is kept; s = z(v, u) - q2; skipped
             when s < -truncation; f = s / truncation, 1 when f > 1; F = F + f, n = n + 1
    volume   weight = n (int32), tsdf = float(F / double(n)), 1.0f when n = 0; layout (G, nz, ny, nx)
    usable   inside the grid and weight >= min_weight
    row      voxel a, axis e in (x, y, z), b = a + e inside the grid, both usable, (fa < 0) != (fb < 0), fa and fb the fp32 values
             widened; t = fa / (fa - fb); the point is a's centre with t * voxel added to component e
    normal   g_d(c) = (usable(c + d) ? f(c + d) : f(c)) - (usable(c - d) ? f(c - d) : f(c)); m_d = g_d(a) + t * (g_d(b) - g_d(a));
             l = sqrt((m0^2 + m1^2) + m2^2); m / l, or zero when l is 0 or not finite: it points into free space
    order    group, k, j, i, then axis; cell = (((g * nz + k) * ny + j) * nx + i) * 3 + e (int64); offsets (G+1) int64
    grid     fuse_grid(lo, hi, voxel, truncation): origin = lo - truncation, n_d = max(1, ceil(((hi_d - lo_d) + 2 * truncation) /
             voxel)), the shared dims the maximum over the groups
"""
import math

import numpy as np

import depth_law

f32, f64 = np.float32, np.float64


def fuse_grid(lo, hi, voxel, truncation):
    """(origin (G,3) float64, (nx, ny, nz)) of the default grid around the boxes lo, hi (G,3)."""
    lo, hi = np.asarray(lo, f64).reshape(-1, 3), np.asarray(hi, f64).reshape(-1, 3)
    voxel, truncation = float(voxel), float(truncation)
    n = np.maximum(1, np.ceil(((hi - lo) + 2 * truncation) / voxel)).max(0)
    return lo - truncation, tuple(int(x) for x in n)


def _arguments(depth, K, poses, groups, origin, masks, scale, truncation, voxel):
    depth, K, poses, masks, scale = depth_law._arguments(depth, K, poses, masks, scale)
    groups = [list(range(depth.shape[0]))] if groups is None else [[int(b) for b in g] for g in groups]
    origin = np.broadcast_to(np.asarray(origin, f64).reshape(-1, 3), (len(groups), 3))
    return depth, K, poses, groups, origin, masks, scale, float(4 * voxel if truncation is None else truncation)


def _kept(law, depth, K, masks, scale, near, far, jump, w):
    """(B,H,W) bool: the kept pixels, by the depth law's own pixel numbers."""
    keep = np.zeros(depth.size, bool)
    keep[law(depth, K, None, masks, scale, near, far, jump, w)["pixel"]] = True
    return keep.reshape(depth.shape)


def fuse_volume_law(depth, K, poses, groups, origin, dims, voxel, truncation=None, masks=None, scale=None, near=0.0, far=np.inf,
                    jump=(0.0, 0.05), w=1):
    """dict(tsdf (G,nz,ny,nx) f32, weight (G,nz,ny,nx) i32), vectorised over a volume."""
    depth, K, poses, groups, origin, masks, scale, trunc = _arguments(depth, K, poses, groups, origin, masks, scale, truncation, voxel)
    voxel = float(voxel)
    nx, ny, nz = dims
    B, H, W = depth.shape
    keep = _kept(depth_law.depth_law, depth, K, masks, scale, near, far, jump, w)
    tsdf, weight = np.empty((len(groups), nz, ny, nx), f32), np.empty((len(groups), nz, ny, nx), np.int32)
    with np.errstate(all="ignore"):
        for g, images in enumerate(groups):
            c = [origin[g, a] + (np.arange(n, dtype=f64) + 0.5) * voxel for a, n in enumerate((nx, ny, nz))]
            c = [c[0][None, None, :], c[1][None, :, None], c[2][:, None, None]]
            F, n = np.zeros((nz, ny, nx), f64), np.zeros((nz, ny, nx), np.int32)
            for b in images:
                fx, fy, cx, cy = K[b]
                R, t = poses[b, :, :3], poses[b, :, 3]
                d = [c[a] - t[a] for a in range(3)]
                q = [(R[0, a] * d[0] + R[1, a] * d[1]) + R[2, a] * d[2] for a in range(3)]
                ok = q[2] > 0
                uf = np.floor((((q[0] * fx) / q[2]) + cx) + 0.5)
                vf = np.floor((((q[1] * fy) / q[2]) + cy) + 0.5)
                ok = ok & (uf >= 0) & (uf <= W - 1) & (vf >= 0) & (vf <= H - 1)
                u, v = np.where(ok, uf, 0).astype(np.int64), np.where(ok, vf, 0).astype(np.int64)
                ok &= keep[b][v, u]
                s = np.where(ok, depth[b][v, u].astype(f64) * scale, 0.0) - q[2]
                ok &= ~(s < -trunc)
                f = s / trunc
                F = np.where(ok, F + np.where(f > 1, 1.0, f), F)
                n = n + ok
            weight[g] = n
            tsdf[g] = np.where(n > 0, F / np.maximum(n, 1).astype(f64), 1.0).astype(f32)
    return {"tsdf": tsdf, "weight": weight}


def fuse_volume_law_loop(depth, K, poses, groups, origin, dims, voxel, truncation=None, masks=None, scale=None, near=0.0, far=np.inf,
                         jump=(0.0, 0.05), w=1):
    """The same law voxel by voxel in Python floats."""
    depth, K, poses, groups, origin, masks, scale, trunc = _arguments(depth, K, poses, groups, origin, masks, scale, truncation, voxel)
    voxel = float(voxel)
    nx, ny, nz = dims
    B, H, W = depth.shape
    keep = _kept(depth_law.depth_law_loop, depth, K, masks, scale, near, far, jump, w)
    tsdf, weight = np.empty((len(groups), nz, ny, nx), f32), np.empty((len(groups), nz, ny, nx), np.int32)
    for g, images in enumerate(groups):
        o = [float(x) for x in origin[g]]
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    c = (o[0] + (float(i) + 0.5) * voxel, o[1] + (float(j) + 0.5) * voxel, o[2] + (float(k) + 0.5) * voxel)
                    F, n = 0.0, 0
                    for b in images:
                        fx, fy, cx, cy = (float(x) for x in K[b])
                        M = [[float(x) for x in row] for row in poses[b]]
                        d = [c[a] - M[a][3] for a in range(3)]
                        q = [(M[0][a] * d[0] + M[1][a] * d[1]) + M[2][a] * d[2] for a in range(3)]
                        if not q[2] > 0:
                            continue
                        x, y = (((q[0] * fx) / q[2]) + cx) + 0.5, (((q[1] * fy) / q[2]) + cy) + 0.5
                        if not (math.isfinite(x) and math.isfinite(y)):
                            continue
                        uf, vf = float(math.floor(x)), float(math.floor(y))
                        if not (0 <= uf <= W - 1 and 0 <= vf <= H - 1) or not keep[b, int(vf), int(uf)]:
                            continue
                        s = float(depth[b, int(vf), int(uf)]) * scale - q[2]
                        if s < -trunc:
                            continue
                        f = s / trunc
                        F, n = F + (1.0 if f > 1 else f), n + 1
                    weight[g, k, j, i] = n
                    tsdf[g, k, j, i] = f32(F / float(n)) if n > 0 else f32(1.0)
    return {"tsdf": tsdf, "weight": weight}


def _surface_result(points, normals, cell, counts):
    cat = lambda parts, shape, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(shape, dtype)
    return {"points": cat(points, (0, 3), f32), "normals": cat(normals, (0, 3), f32), "cell": cat(cell, (0,), np.int64),
            "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)}


def _shift3(a, axis, step, fill):
    """out[c] = a[c + step along axis], `fill` where that lies outside the grid; axis 0, 1, 2 = x, y, z of a (nz, ny, nx) array."""
    out = np.full_like(a, fill)
    ax = 2 - axis
    n = a.shape[ax]
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    src[ax], dst[ax] = (slice(1, n), slice(0, n - 1)) if step > 0 else (slice(0, n - 1), slice(1, n))
    out[tuple(dst)] = a[tuple(src)]
    return out


def fuse_surface_law(tsdf, weight, origin, voxel, min_weight=1):
    """dict(points (T,3) f32, normals (T,3) f32, cell (T) i64, offsets (G+1) i64), vectorised over a volume."""
    tsdf, weight = np.asarray(tsdf, f32), np.asarray(weight, np.int32)
    G, nz, ny, nx = tsdf.shape
    origin, voxel = np.broadcast_to(np.asarray(origin, f64).reshape(-1, 3), (G, 3)), float(voxel)
    points, normals, cell, counts = [], [], [], []
    with np.errstate(all="ignore"):
        for g in range(G):
            f, use = tsdf[g].astype(f64), weight[g] >= min_weight
            grad = [np.where(_shift3(use, d, 1, False), _shift3(f, d, 1, 0.0), f) - np.where(_shift3(use, d, -1, False), _shift3(f, d, -1, 0.0), f)
                    for d in range(3)]
            kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
            centre = [origin[g, 0] + (ii.astype(f64) + 0.5) * voxel, origin[g, 1] + (jj.astype(f64) + 0.5) * voxel,
                      origin[g, 2] + (kk.astype(f64) + 0.5) * voxel]
            P, N, C = [], [], []
            for e in range(3):
                fb = _shift3(f, e, 1, 0.0)
                row = use & _shift3(use, e, 1, False) & ((f < 0) != (fb < 0))
                t = f / (f - fb)
                p = [centre[d] + t * voxel if d == e else centre[d] for d in range(3)]
                m = [grad[d] + t * (_shift3(grad[d], e, 1, 0.0) - grad[d]) for d in range(3)]
                l = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                unit = np.isfinite(l) & (l != 0)
                P.append(np.stack([x[row] for x in p], 1))
                N.append(np.stack([np.where(unit, x / l, 0.0)[row] for x in m], 1))
                C.append(((((g * nz + kk) * ny + jj) * nx + ii).astype(np.int64) * 3 + e)[row])
            P, N, C = np.concatenate(P), np.concatenate(N), np.concatenate(C)
            order = np.argsort(C, kind="stable")
            points.append(P[order]), normals.append(N[order]), cell.append(C[order]), counts.append(len(C))
    return _surface_result(points, normals, cell, counts)


def fuse_surface_law_loop(tsdf, weight, origin, voxel, min_weight=1):
    """The same law voxel by voxel in Python floats."""
    tsdf, weight = np.asarray(tsdf, f32), np.asarray(weight, np.int32)
    G, nz, ny, nx = tsdf.shape
    origin, voxel = np.broadcast_to(np.asarray(origin, f64).reshape(-1, 3), (G, 3)), float(voxel)
    points, normals, cell, counts = [], [], [], []
    for g in range(G):
        usable = lambda c: 0 <= c[0] < nx and 0 <= c[1] < ny and 0 <= c[2] < nz and weight[g, c[2], c[1], c[0]] >= min_weight
        value = lambda c: float(tsdf[g, c[2], c[1], c[0]])
        step = lambda c, d, by: tuple(c[a] + by * (a == d) for a in range(3))

        def slope(c, d):
            hi, lo = step(c, d, 1), step(c, d, -1)
            return (value(hi) if usable(hi) else value(c)) - (value(lo) if usable(lo) else value(c))

        rows = 0
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    a = (i, j, k)
                    for e in range(3):
                        b = step(a, e, 1)
                        if not (usable(a) and usable(b)) or (value(a) < 0) == (value(b) < 0):
                            continue
                        fa, fb = value(a), value(b)
                        t = fa / (fa - fb)
                        p = [float(origin[g, d]) + (float(a[d]) + 0.5) * voxel for d in range(3)]
                        p[e] = p[e] + t * voxel
                        m = [slope(a, d) + t * (slope(b, d) - slope(a, d)) for d in range(3)]
                        l = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                        m = [x / l for x in m] if math.isfinite(l) and l != 0 else [0.0, 0.0, 0.0]
                        points.append(np.asarray([p], f64)), normals.append(np.asarray([m], f64))
                        cell.append([(((g * nz + k) * ny + j) * nx + i) * 3 + e])
                        rows += 1
        counts.append(rows)
    return _surface_result(points, normals, cell, counts)


# ---- what the tests and the benchmark share: rendered views ----------------------------------------------------------------
def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """(3,4) float32 camera-to-world [R | t] of a camera at `eye` looking at `target`: columns x right, y down, z forward."""
    eye, target = np.asarray(eye, f64), np.asarray(target, f64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, f64))                     # right-handed with y down: x = z x up
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), eye[:, None]], 1).astype(f32)


def render(pose, K, H, W, planes=(), spheres=()):
    """(H,W) float64 z-depth along the optical axis (0 where nothing is hit) of planes (normal n, offset: n . p = offset) and
    spheres (centre, radius) seen through the fp32 pose as the kernels widen it."""
    M = np.asarray(pose, f32).astype(f64)
    R, eye = M[:, :3], M[:, 3]
    fx, fy, cx, cy = (float(x) for x in K)
    rays = np.stack(np.broadcast_arrays((np.arange(W)[None, :] - cx) / fx, (np.arange(H)[:, None] - cy) / fy, 1.0), -1) @ R.T
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for n, offset in planes:
            hit = (offset - np.dot(n, eye)) / (rays @ np.asarray(n, f64))
            best = np.where(hit > 0, np.minimum(best, hit), best)
        for centre, radius in spheres:
            oc = eye - np.asarray(centre, f64)
            bb, cc, aa = (rays * oc).sum(-1), oc @ oc - radius * radius, (rays * rays).sum(-1)
            disc = bb * bb - aa * cc
            hit = (-bb - np.sqrt(np.maximum(disc, 0))) / aa
            best = np.where((disc > 0) & (hit > 0), np.minimum(best, hit), best)
    return np.where(np.isfinite(best), best, 0.0)

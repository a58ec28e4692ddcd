"""The law of ops.depth_points (csrc/depth.hip, include/hyperpocket_hip.h) in numpy: depth images in, the kept pixels'
world points, sensor-facing normals and pixel numbers out.  Every floating operation is one IEEE fp64 rounding in the
association written, no library function but sqrt, one cast to fp32 at the end.  Stated twice: depth_law, vectorised, what
the GPU tests call, and depth_law_loop, a per-pixel loop in Python floats that the host tests hold the first against.

    z        = double(d) * scale; measured: z finite and > 0
    jump     (a, b) = |a - b| > jump_abs + jump_rel * min(a, b)
    edge     w > 0, measured, and some measured pixel within |dv|, |du| <= w inside the image jumps against it
    kept     measured, near <= z <= far, mask != 0 where given, not an edge
    q        = (((u - cx) * z) / fx, ((v - cy) * z) / fy, z)
    normal   a = (right usable ? q_right : q) - (left usable ? q_left : q), b likewise down - up, usable: inside, measured,
             no jump against the centre; n = a x b; n = -n when (nx qx + ny qy) + nz qz > 0; l = sqrt((nx^2 + ny^2) + nz^2);
             n / l, or (0, 0, 0) when l is 0 or not finite
    world    p_k = ((R_k0 qx + R_k1 qy) + R_k2 qz) + t_k; the normal likewise without t
    order    image, row, column; pixel = (b * H + v) * W + u
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(f32)


def default_scale(depth):
    return 0.001 if np.asarray(depth).dtype == np.uint16 else 1.0


def _arguments(depth, K, poses, masks, scale):
    depth = np.asarray(depth)
    assert depth.ndim == 3 and depth.dtype in (np.uint16, np.float32), (depth.shape, depth.dtype)
    B = depth.shape[0]
    K = np.broadcast_to(np.asarray(K, f64).reshape(-1, 4), (B, 4))
    poses = IDENTITY if poses is None else np.asarray(poses, f32)
    poses = np.broadcast_to(poses.reshape(-1, 3, 4), (B, 3, 4)).astype(f64)
    if masks is not None:
        masks = np.asarray(masks)
        assert masks.shape == depth.shape and masks.dtype == np.uint8
    return depth, K, poses, masks, float(default_scale(depth) if scale is None else scale)


def _result(points, normals, pixel, counts):
    cat = lambda parts, shape, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(shape, dtype)
    return {"points": cat(points, (0, 3), f32), "normals": cat(normals, (0, 3), f32), "pixel": cat(pixel, (0,), np.int64),
            "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)}


def _shift(a, dv, du, fill):
    """out[v, u] = a[v + dv, u + du], `fill` where that lies outside the image."""
    H, W = a.shape
    out = np.full_like(a, fill)
    v0, v1, u0, u1 = max(0, -dv), min(H, H - dv), max(0, -du), min(W, W - du)
    if v0 < v1 and u0 < u1:
        out[v0:v1, u0:u1] = a[v0 + dv:v1 + dv, u0 + du:u1 + du]
    return out


def _jump(a, b, jump_abs, jump_rel):
    return np.abs(a - b) > jump_abs + jump_rel * np.minimum(a, b)


def depth_law(depth, K, poses=None, masks=None, scale=None, near=0.0, far=np.inf, jump=(0.0, 0.05), w=1):
    """dict(points (T,3) f32, normals (T,3) f32, pixel (T) i64, offsets (B+1) i64), vectorised over an image."""
    depth, K, poses, masks, scale = _arguments(depth, K, poses, masks, scale)
    jump_abs, jump_rel = float(jump[0]), float(jump[1])
    B, H, W = depth.shape
    points, normals, pixel, counts = [], [], [], []
    with np.errstate(all="ignore"):
        for b in range(B):
            fx, fy, cx, cy = K[b]
            z = depth[b].astype(f64) * scale
            meas = np.isfinite(z) & (z > 0)
            z = np.where(meas, z, 1.0)                             # a hole's value is never used: keep NaNs out of the way
            keep = meas & (z >= near) & (z <= far)
            if masks is not None:
                keep &= masks[b] != 0
            for dv in range(-w, w + 1):
                for du in range(-w, w + 1):
                    if dv or du:
                        keep &= ~(_shift(meas, dv, du, False) & _jump(z, _shift(z, dv, du, 1.0), jump_abs, jump_rel))
            vv, uu = np.nonzero(keep)                              # row-major: row, then column
            counts.append(len(vv))
            q = np.stack([((np.arange(W, dtype=f64)[None, :] - cx) * z) / fx, ((np.arange(H, dtype=f64)[:, None] - cy) * z) / fy, z])

            def side(dv, du):
                usable = _shift(meas, dv, du, False) & ~_jump(z, _shift(z, dv, du, 1.0), jump_abs, jump_rel)
                qn = np.stack([_shift(q[c], dv, du, 0.0) for c in range(3)])
                return np.where(usable[vv, uu], qn[:, vv, uu], q[:, vv, uu])

            qk = q[:, vv, uu]
            a = side(0, 1) - side(0, -1)
            c = side(1, 0) - side(-1, 0)
            n = np.stack([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]])
            n = np.where((n[0] * qk[0] + n[1] * qk[1]) + n[2] * qk[2] > 0, -n, n)
            l = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            n = np.where(np.isfinite(l) & (l != 0), n / l, 0.0)
            R, t = poses[b, :, :3], poses[b, :, 3]
            rot = lambda x: np.stack([(R[k, 0] * x[0] + R[k, 1] * x[1]) + R[k, 2] * x[2] for k in range(3)], 1)
            points.append(rot(qk) + t[None, :])
            normals.append(rot(n))
            pixel.append((b * H + vv.astype(np.int64)) * W + uu)
    return _result(points, normals, pixel, counts)


def depth_law_loop(depth, K, poses=None, masks=None, scale=None, near=0.0, far=np.inf, jump=(0.0, 0.05), w=1):
    """The same law pixel by pixel in Python floats (IEEE doubles: +, -, *, / and math.sqrt each round once)."""
    depth, K, poses, masks, scale = _arguments(depth, K, poses, masks, scale)
    jump_abs, jump_rel = float(jump[0]), float(jump[1])
    near, far = float(near), float(far)
    B, H, W = depth.shape
    points, normals, pixel, counts = [], [], [], []
    measured = lambda z: math.isfinite(z) and z > 0.0
    jumps = lambda a, b: abs(a - b) > jump_abs + jump_rel * min(a, b)
    for b in range(B):
        fx, fy, cx, cy = (float(x) for x in K[b])
        R = [[float(x) for x in row] for row in poses[b]]
        z = [[float(d) * scale for d in row] for row in depth[b]]
        camera = lambda v, u: (((float(u) - cx) * z[v][u]) / fx, ((float(v) - cy) * z[v][u]) / fy, z[v][u])
        rows = 0
        for v in range(H):
            for u in range(W):
                z0 = z[v][u]
                if not (measured(z0) and near <= z0 <= far) or (masks is not None and masks[b, v, u] == 0):
                    continue
                if any(measured(z[y][x]) and jumps(z0, z[y][x]) for y in range(max(0, v - w), min(H, v + w + 1))
                       for x in range(max(0, u - w), min(W, u + w + 1)) if (y, x) != (v, u)):
                    continue
                q = camera(v, u)

                def side(y, x):
                    return camera(y, x) if 0 <= y < H and 0 <= x < W and measured(z[y][x]) and not jumps(z0, z[y][x]) else q

                right, left, down, up = side(v, u + 1), side(v, u - 1), side(v + 1, u), side(v - 1, u)
                a = [right[c] - left[c] for c in range(3)]
                d = [down[c] - up[c] for c in range(3)]
                n = [a[1] * d[2] - a[2] * d[1], a[2] * d[0] - a[0] * d[2], a[0] * d[1] - a[1] * d[0]]
                if (n[0] * q[0] + n[1] * q[1]) + n[2] * q[2] > 0:
                    n = [-x for x in n]
                l = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                n = [x / l for x in n] if math.isfinite(l) and l != 0 else [0.0, 0.0, 0.0]
                points.append([[(R[k][0] * q[0] + R[k][1] * q[1]) + R[k][2] * q[2] + R[k][3] for k in range(3)]])
                normals.append([[(R[k][0] * n[0] + R[k][1] * n[1]) + R[k][2] * n[2] for k in range(3)]])
                pixel.append([(b * H + v) * W + u])
                rows += 1
        counts.append(rows)
    as64 = lambda parts: [np.asarray(p, f64) for p in parts]
    return _result(as64(points), as64(normals), pixel, counts)


# ---- what the tests and the benchmark share: seeded images -----------------------------------------------------------------
def lattice_images(seed, B, H, W, dtype, holes=0.15):
    """B images whose depths lie on a 1/64 lattice (in metres) between 1 and 2: a staircase that rises by one step — a tie of
    the jump test at jump_abs = 1/64 — every 16 pixels along u + 2 v, so that pixels within a window of 4 differ by a step at
    most; three blocks an image that stand 8 steps off it, and a share of holes.  uint16 images hold z * 64 and want
    scale = 1/64; float32 images hold z itself and every kind of hole."""
    r = np.random.RandomState(seed)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    steps = np.stack([(u + 2 * v + r.randint(0, 16)) // 16 % 40 + r.randint(0, 8) for _ in range(B)])
    for b in range(B):
        for _ in range(3):
            v0, u0 = r.randint(0, H), r.randint(0, W)
            steps[b, v0:v0 + 1 + H // 4, u0:u0 + 1 + W // 4] += 8
    hole = r.rand(B, H, W) < holes
    if dtype == np.uint16:
        return np.where(hole, 0, 64 + steps).astype(np.uint16)
    kinds = np.array([0.0, -1.0, np.nan, np.inf, -np.inf], f32)
    return np.where(hole, kinds[r.randint(0, 5, (B, H, W))], (1.0 + steps / 64.0).astype(f32)).astype(f32)


def scene(seed, B, H, W, holes=0.1):
    """The synthetic scene of the benchmark and the dataset tests: a sensor 1.2 m above a floor, looking 35 degrees down at a box
    and a sphere that stand on it.  -> dict(depth (B,H,W) uint16 in millimetres with a share of holes, K (4,), poses (B,3,4)
    float32 camera-to-world — image b stands 0.01 * b further to the right —, masks (B,H,W) uint8: 0 on the image's lowest
    eighth).  World frame: y up, the floor at y = 0."""
    r = np.random.RandomState(seed)
    f = 0.9 * W
    K = np.array([f, f, (W - 1) / 2.0, (H - 1) / 2.0])
    t = math.radians(35.0)
    R = np.array([[1, 0, 0], [0, -math.cos(t), -math.sin(t)], [0, -math.sin(t), math.cos(t)]])     # columns: x right, y down, z forward
    rays = np.stack(np.broadcast_arrays((np.arange(W)[None, :] - K[2]) / f, (np.arange(H)[:, None] - K[3]) / f, 1.0), -1) @ R.T
    depth, poses = np.zeros((B, H, W), np.uint16), np.zeros((B, 3, 4), f32)
    for b in range(B):
        eye = np.array([0.01 * b, 1.2, 0.0])
        best = np.where(rays[..., 1] < 0, -eye[1] / np.minimum(rays[..., 1], -1e-9), np.inf)      # the floor y = 0
        lo, hi = np.array([-0.45, 0.0, 1.3]), np.array([-0.15, 0.3, 1.6])                         # the box
        with np.errstate(all="ignore"):
            t0, t1 = (lo - eye) / rays, (hi - eye) / rays
        enter, leave = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
        best = np.where((enter < leave) & (enter > 0), np.minimum(best, enter), best)
        centre, radius = np.array([0.3, 0.2, 1.5]), 0.2                                           # the sphere
        oc = eye - centre
        bb, cc, aa = (rays * oc).sum(-1), oc @ oc - radius * radius, (rays * rays).sum(-1)
        disc = bb * bb - aa * cc
        hit = (-bb - np.sqrt(np.maximum(disc, 0))) / aa
        best = np.where((disc > 0) & (hit > 0), np.minimum(best, hit), best)
        mm = np.where(np.isfinite(best), np.rint(best * 1000.0), 0)                               # z along the optical axis: rays have z' = 1
        depth[b] = np.where((mm < 65535) & (r.rand(H, W) >= holes), mm, 0).astype(np.uint16)
        poses[b] = np.concatenate([R, eye[:, None]], 1).astype(f32)
    masks = np.ones((B, H, W), np.uint8)
    masks[:, H - H // 8:, :] = 0
    return {"depth": depth, "K": K, "poses": poses, "masks": masks}

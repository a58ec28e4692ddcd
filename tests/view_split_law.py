"""The viewpoint batch maker's law in numpy (include/hyperpocket_hip.h, hp_make_view_batch) — written from the text, not from
the kernel.  numpy's float64 and float32 element operations are single IEEE roundings, which is what the law asks for.

    project    p = double(row); c_k = (Q[k,0] p_x + Q[k,1] p_y) + Q[k,2] p_z; delta = dist - c_2; z = float32(delta).
               absent: a non-finite coordinate, not (delta > 0), z not finite.
               u = c_0 / delta; fu = (u * scale) + 0.5 R; iu = int(floor(min(max(fu, 0), R - 1))); `it` from c_1; pixel = it R + iu.
    buffer     R^2 uint32, all ones when empty, else the smallest bits(z) of the pixel's rows.
    occlusion  front = the smallest word within w pixels, inside the image; o = z - float32(front) in float32; +inf when absent.
    split      the `target` rows lowest in (o, row) are existing, the rest missing, both in row order.
"""
import numpy as np

EMPTY = np.uint32(0xFFFFFFFF)


def scale_of(resolution, half_extent):
    """(0.5 R) / h, once, in fp64."""
    return (0.5 * float(resolution)) / float(half_extent)


def _clamp_pixel(f, R):
    lo = np.where(f > 0.0, f, 0.0)                                  # a NaN goes to 0
    return np.floor(np.where(lo < R - 1.0, lo, R - 1.0)).astype(np.int64)


def project(cloud, frame, dist, scale, R):
    """-> (present (N) bool, pixel (N) int64 — -1 where absent —, z (N) float32 — undefined where absent)."""
    cloud = np.asarray(cloud, np.float32)
    Q = np.asarray(frame, np.float32).astype(np.float64).reshape(3, 3)
    p = cloud.astype(np.float64)
    with np.errstate(all="ignore"):
        c = [(Q[k, 0] * p[:, 0] + Q[k, 1] * p[:, 1]) + Q[k, 2] * p[:, 2] for k in range(3)]
        delta = np.float64(dist) - c[2]
        z = delta.astype(np.float32)
        present = np.isfinite(cloud).all(1) & (delta > 0.0) & np.isfinite(z)
        safe = np.where(present, delta, 1.0)
        half = 0.5 * float(R)
        fu = (c[0] / safe) * np.float64(scale) + half
        ft = (c[1] / safe) * np.float64(scale) + half
    iu, it = _clamp_pixel(fu, R), _clamp_pixel(ft, R)
    return present, np.where(present, it * R + iu, -1), z


def depth_buffer(present, pixel, z, R):
    buf = np.full(R * R, EMPTY, np.uint32)
    np.minimum.at(buf, pixel[present], z[present].view(np.uint32))
    return buf


def occlusion_of(present, pixel, z, buf, R, w):
    """o (N) float32: z - float32(the nearest depth within w pixels of the row's own), +inf for an absent row."""
    pad = np.full((R + 2 * w, R + 2 * w), EMPTY, np.uint32)
    pad[w:w + R, w:w + R] = buf.reshape(R, R)
    front = np.full((R, R), EMPTY, np.uint32)
    for dy in range(2 * w + 1):
        for dx in range(2 * w + 1):
            front = np.minimum(front, pad[dy:dy + R, dx:dx + R])
    o = np.full(present.shape, np.inf, np.float32)
    f = front.reshape(-1)[pixel[present]]
    assert (f != EMPTY).all()                                       # a row's own pixel is never empty
    with np.errstate(all="ignore"):
        o[present] = z[present] - f.view(np.float32)                # float32 - float32: one rounding
    return o


def view_split(cloud, frame, dist, scale, R, w, target):
    """The law for one item: a dict of side (N) uint8, occlusion (N) float32, existing, missing and gt (unrotated), and the
    intermediates present, pixel, buffer."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    N = cloud.shape[0]
    assert 2 <= N <= 8192 and 4 <= R <= 128 and 0 <= w <= 4 and 0 < target < N and dist > 0 and scale > 0
    present, pixel, z = project(cloud, frame, dist, scale, R)
    buf = depth_buffer(present, pixel, z, R)
    o = occlusion_of(present, pixel, z, buf, R, w)
    order = np.argsort(o, kind="stable")                            # float32 `<`, equal values in row order, +inf last
    side = np.zeros(N, np.uint8)
    side[order[:target]] = 1
    return {"side": side, "occlusion": o, "existing": cloud[side == 1], "missing": cloud[side == 0], "gt": cloud,
            "present": present, "pixel": pixel, "buffer": buf}


def view_split_naive(cloud, frame, dist, scale, R, w, target):
    """The same law row by row in Python scalars — slow, for small clouds: a second statement to hold view_split against."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    Q = np.asarray(frame, np.float32).reshape(3, 3)
    N = cloud.shape[0]
    buf = [0xFFFFFFFF] * (R * R)
    rows = []
    for i in range(N):
        x, y, zc = (np.float64(v) for v in cloud[i])
        rows.append(None)
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(zc)):
            continue
        with np.errstate(all="ignore"):
            c = [(np.float64(Q[k, 0]) * x + np.float64(Q[k, 1]) * y) + np.float64(Q[k, 2]) * zc for k in range(3)]
            delta = np.float64(dist) - c[2]
            z = np.float32(delta)
            if not (delta > 0.0) or not np.isfinite(z):
                continue
            ij = []
            for k in (0, 1):
                f = (c[k] / delta) * np.float64(scale) + np.float64(0.5 * R)
                f = f if f > 0.0 else np.float64(0.0)
                f = f if f < R - 1.0 else np.float64(R - 1.0)
                ij.append(int(np.floor(f)))
        iu, it = ij
        bits = int(np.float32(z).view(np.uint32))
        buf[it * R + iu] = min(buf[it * R + iu], bits)
        rows[i] = (it, iu, z)
    o = np.full(N, np.inf, np.float32)
    for i, r in enumerate(rows):
        if r is None:
            continue
        it, iu, z = r
        front = min(buf[y * R + x] for y in range(max(0, it - w), min(R, it + w + 1))
                    for x in range(max(0, iu - w), min(R, iu + w + 1)))
        o[i] = z - np.uint32(front).view(np.float32)
    rank = sorted(range(N), key=lambda i: (float(o[i]), i))
    side = np.zeros(N, np.uint8)
    side[rank[:target]] = 1
    return {"side": side, "occlusion": o, "buffer": np.array(buf, np.uint32)}


# ---- the fixtures of the law's facts.  Both facts are about holes in the near side, so they are facts about a sample: of the
# random shells of seeds 0..5 the least share over the 8 frames is 0.949-0.986 (seed 1: 0.986), and of the plates of seeds
# 0..11 five have a hole of 3 x 3 pixels at (2048, 64, 1) through which 3-4 rows of the back plate show, and four a pixel
# without a front row at (128, 8, 0); seeds 5 and 6 have neither.  The seeds below are such samples; the lattice shell is even
# by construction.
def sphere_shell(n, radius=0.5, seed=1):
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True) * radius).astype(np.float32)


def lattice_shell(n, radius=0.5):
    """The Fibonacci lattice on the sphere: an even shell without a seed."""
    i = np.arange(n) + 0.5
    z, phi = 1.0 - 2.0 * i / n, i * (np.pi * (3.0 - 5.0 ** 0.5))
    s = np.sqrt(1.0 - z * z)
    return (np.stack([s * np.cos(phi), s * np.sin(phi), z], 1) * radius).astype(np.float32)


def two_plates(n, seed=5):
    """Two parallel square plates at z = +-0.2, rows alternating between them (even rows in front, z = +0.2), x and y uniform in
    +-0.4."""
    r = np.random.default_rng(seed)
    c = np.empty((n, 3), np.float32)
    c[:, :2] = r.uniform(-0.4, 0.4, (n, 2)).astype(np.float32)
    c[:, 2] = np.where(np.arange(n) % 2 == 0, 0.2, -0.2).astype(np.float32)
    return c

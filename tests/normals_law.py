"""The surface-normal law in numpy — the checker of csrc/normals.hip, written from the law itself.

Everything is per scan (rows offsets[s] .. offsets[s+1] of points (T,3) float32, n_s of them) and per row i, given a neighbour
list index (T,k) int32 of rows within the scan — knn_law's output format, taken as given.

    absent     a row with a non-finite coordinate (as in knn_law).
    neighbourhood  row i itself, plus every slot t of its list with 0 <= index[i,t] < n_s whose row is present.  Any other
               slot is empty: -1, and garbage too.  Duplicates and a slot equal to i count as listed.
               count = the size of the neighbourhood; 0 for an absent row i.
    dq         = p_j - p_i per component, one float32 rounding; row i contributes (0, 0, 0).
    frame      M = the largest |dq_c| over the neighbourhood; e = M's biased exponent field - 127;
               q_c = trunc(ldexp(dq_c, 19 - e)): exact, |q_c| < 2**20 (plane_law's frame).
    scatter    m = count;  S_a = sum q_a, S_ab = sum q_a q_b, exact integers;  C_ab = m S_ab - S_a S_b, exact in int64.
               With m <= 33: m S_ab <= 33 * 32 * (2**20 - 1)**2 < 2**50.05 and |S_a S_b| <= (32 * (2**20 - 1))**2 < 2**50, so
               |C_ab| < 2**51.1, and the trace, a sum of three 0 <= C_aa <= m S_aa, < 2**51.7: all below 2**53, so the
               conversion to float64 is exact.
    undefined  count < 3, M == 0, M not finite, or trace == 0: the normal is three quiet NaNs (0x7FC00000) and so is the curvature.
    eigen      cyclic Jacobi on A = float64(C), V = I: SWEEPS sweeps, no convergence exit, the pairs (p, q) in the order
               (0,1), (0,2), (1,2), r the third index.  A rotation is skipped only where a_pq == 0 exactly.  Otherwise
                   theta = (a_qq - a_pp) / (2 * a_pq);   t = sgn(theta) / (|theta| + sqrt(theta * theta + 1)), sgn(0) = +1;
                   c = 1 / sqrt(t * t + 1);   s = t * c;   h = t * a_pq;
                   a_pp = a_pp - h;   a_qq = a_qq + h;   a_pq = 0;
                   (a_rp, a_rq) = (c * a_rp - s * a_rq,  s * a_rp + c * a_rq);
                   (v_kp, v_kq) = (c * v_kp - s * v_kq,  s * v_kp + c * v_kq)   for k = 0, 1, 2,
               every + - * / sqrt one float64 rounding in the association written (2 * a_pq is exact); a pair's new values
               are computed from its old ones.  An overflowed theta * theta gives t = 0: a value.
    normal     the column of V of the smallest diagonal entry of A after the sweeps (ties to the lower index), divided by its
               length sqrt((x*x + y*y) + z*z) in float64.  Sign: the component of largest magnitude (ties to the lower axis)
               is made positive.  Then, with a viewpoint v_s: w = float64(v_s) - float64(p_i), dot = (nx*wx + ny*wy) + nz*wz;
               the normal is negated iff dot < 0 (a NaN dot never flips).  Rounded to float32.
    curvature  the surface variation max(lambda_min, 0) / trace in float64, lambda_min that smallest diagonal entry and trace
               the exact integer trace of C (not the rotated one), rounded to float32.  0: flat.  1/3: isotropic.
"""
import functools

import numpy as np

import knn_law

f32, f64 = np.float32, np.float64
SWEEPS = 6
MAX_K = 32
QNAN = np.uint32(0x7FC00000).view(f32)
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))                   # (p, q, r)
BOUND = 1 << 53


def scatter(q, cnt):
    """C (.., 3, 3) int64 from the neighbours' q (.., k, 3) int64 (row i's zeros left out, empty slots zeros) and m = cnt (..)
    int64: exact, with the bound of the law asserted in Python integers."""
    k = q.shape[-2]
    assert k <= MAX_K and int(np.abs(q).max(initial=0)) < (1 << 20) and int(cnt.max(initial=0)) <= k + 1
    S1 = q.sum(axis=-2)
    S2 = np.einsum("...ka,...kb->...ab", q, q)
    big = (k + 1) * k * ((1 << 20) - 1) ** 2 + (k * ((1 << 20) - 1)) ** 2       # Python integers: the worst |C_ab|
    assert big < BOUND and 3 * (k + 1) * k * ((1 << 20) - 1) ** 2 < BOUND
    C = cnt[..., None, None] * S2 - S1[..., :, None] * S1[..., None, :]
    assert int(np.abs(C).max(initial=0)) < BOUND
    return C


def rotate(a, v, p, q, r):
    """One Jacobi rotation of the pair (p, q) over arrays: a[(i, j)] float64 (n) for i <= j, v[k][j] float64 (n); in place."""
    key = lambda i, j: (min(i, j), max(i, j))
    apq = a[key(p, q)]
    on = apq != 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = np.where(on, apq, f64(1))
        theta = (a[(q, q)] - a[(p, p)]) / (f64(2) * d)
        t = np.where(theta >= 0, f64(1), f64(-1)) / (np.abs(theta) + np.sqrt(theta * theta + f64(1)))
        c = f64(1) / np.sqrt(t * t + f64(1))
        s = t * c
        h = t * d
        new = {(p, p): a[(p, p)] - h, (q, q): a[(q, q)] + h, key(p, q): np.zeros_like(apq),
               key(r, p): c * a[key(r, p)] - s * a[key(r, q)], key(r, q): s * a[key(r, p)] + c * a[key(r, q)]}
        for name, val in new.items():
            a[name] = np.where(on, val, a[name])
        for k in range(3):
            vp, vq = v[k][p], v[k][q]
            v[k][p], v[k][q] = np.where(on, c * vp - s * vq, vp), np.where(on, s * vp + c * vq, vq)


def jacobi(C, sweeps=SWEEPS):
    """(lam (n,3) float64 — the diagonal after the sweeps, V (n,3,3) float64 with V[:, k, j] = v_kj) of C (n,3,3) int64."""
    C = np.asarray(C)
    a = {(i, j): C[:, i, j].astype(f64) for i in range(3) for j in range(i, 3)}
    v = [[np.full(len(C), f64(i == j)) for j in range(3)] for i in range(3)]
    for _ in range(sweeps):
        for p, q, r in PAIRS:
            rotate(a, v, p, q, r)
    lam = np.stack([a[(0, 0)], a[(1, 1)], a[(2, 2)]], axis=1)
    return lam, np.stack([np.stack(row, axis=1) for row in v], axis=1)


def neighbourhood(cloud, index):
    """(dq (n,k,3) float32 with zeros in the empty slots, count (n) int32) of one scan."""
    n = len(cloud)
    present = np.isfinite(cloud).all(axis=1)
    inr = (index >= 0) & (index < n)
    safe = np.where(inr, index, 0)
    valid = inr & present[safe] & present[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        dq = cloud[safe] - cloud[:, None, :]
    assert dq.dtype == f32
    dq[~valid] = 0
    count = np.where(present, 1 + valid.sum(axis=1), 0).astype(np.int32)
    return dq, count


def normals_scan(cloud, index, viewpoint=None, sweeps=SWEEPS):
    """One scan -> (normal (n,3) float32, curvature (n) float32, count (n) int32)."""
    cloud = np.ascontiguousarray(np.asarray(cloud, dtype=f32)).reshape(-1, 3)
    index = np.asarray(index, dtype=np.int32).reshape(len(cloud), -1)
    n, k = index.shape
    assert 2 <= k <= MAX_K
    normal = np.full((n, 3), QNAN, dtype=f32)
    curvature = np.full(n, QNAN, dtype=f32)
    dq, count = neighbourhood(cloud, index)
    M = np.abs(dq).reshape(n, -1).max(axis=1) if n else np.zeros(0, f32)
    ok = (count >= 3) & (M != 0) & np.isfinite(M)
    rows = np.flatnonzero(ok)
    if len(rows) == 0:
        return normal, curvature, count
    e = ((M[rows].view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int64) - 127
    scaled = np.ldexp(dq[rows], (19 - e)[:, None, None].astype(np.int32))
    assert scaled.dtype == f32
    q = np.trunc(scaled).astype(np.int64)
    C = scatter(q, count[rows].astype(np.int64))
    trace = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]
    assert int(trace.max()) < BOUND and int(C[:, [0, 1, 2], [0, 1, 2]].min()) >= 0
    live = trace != 0
    rows, C, trace = rows[live], C[live], trace[live]
    lam, V = jacobi(C, sweeps)
    col = np.argmin(lam, axis=1)                                # the first of equals: the lower index
    lmin = lam[np.arange(len(rows)), col]
    x, y, z = (V[np.arange(len(rows)), c, col] for c in range(3))
    length = np.sqrt((x * x + y * y) + z * z)
    nrm = np.stack([x / length, y / length, z / length], axis=1)
    lead = np.argmax(np.abs(nrm), axis=1)                       # the first of equals: the lower axis
    nrm = np.where((nrm[np.arange(len(rows)), lead] < 0)[:, None], -nrm, nrm)
    if viewpoint is not None:
        w = np.asarray(viewpoint, dtype=f32).astype(f64)[None, :] - cloud[rows].astype(f64)
        with np.errstate(invalid="ignore", over="ignore"):
            dot = (nrm[:, 0] * w[:, 0] + nrm[:, 1] * w[:, 1]) + nrm[:, 2] * w[:, 2]
        nrm = np.where((dot < 0)[:, None], -nrm, nrm)
    normal[rows] = nrm.astype(f32)
    curvature[rows] = (np.maximum(lmin, f64(0)) / trace.astype(f64)).astype(f32)
    return normal, curvature, count


def normals_law(points, offsets, index, viewpoints=None, sweeps=SWEEPS):
    """(normal (T,3) float32, curvature (T) float32, count (T) int32) over a ragged set; viewpoints (S,3) float32 or None."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    index = np.asarray(index, dtype=np.int32).reshape(len(points), -1)
    normal = np.empty((len(points), 3), dtype=f32)
    curvature = np.empty(len(points), dtype=f32)
    count = np.empty(len(points), dtype=np.int32)
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        view = None if viewpoints is None else np.asarray(viewpoints, dtype=f32).reshape(-1, 3)[s]
        normal[lo:hi], curvature[lo:hi], count[lo:hi] = normals_scan(points[lo:hi], index[lo:hi], view, sweeps)
    return normal, curvature, count


def reference_fp64(cloud, index):
    """What the law approximates, per row with count >= 3: numpy.linalg.eigh of the unquantised float64 scatter of the
    neighbourhood.  Returns (normal (n,3), curvature (n), gap (n) = (l1 - l0) / l2, ok (n))."""
    cloud = np.asarray(cloud, dtype=f32)
    dq, count = neighbourhood(cloud, np.asarray(index, dtype=np.int32))
    d = dq.astype(f64)
    m = count.astype(f64)[:, None, None]
    S1 = d.sum(axis=1)
    C = m * np.einsum("nka,nkb->nab", d, d) - S1[:, :, None] * S1[:, None, :]
    ok = count >= 3
    C[~ok] = np.eye(3)
    lam, vec = np.linalg.eigh(C)
    return vec[:, :, 0], np.maximum(lam[:, 0], 0) / lam.sum(axis=1), (lam[:, 1] - lam[:, 0]) / lam[:, 2], ok


def reference_law(points, offsets, index):
    """reference_fp64 over a ragged set."""
    parts = [reference_fp64(points[lo:hi], index[lo:hi]) for lo, hi in zip(offsets[:-1], offsets[1:])]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def angle(a, b):
    """The angle between the lines of a and b (n,3), float64, in radians."""
    a, b = np.asarray(a, dtype=f64), np.asarray(b, dtype=f64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(axis=1)))


# ---- fixtures of the suites, not of the law -------------------------------------------------------------------------------


def _lists(cloud, k):
    return knn_law.knn_scan(cloud, k)[0]


@functools.lru_cache(maxsize=None)
def shell(n=1024, k=16, seed=0):
    """(cloud, index): n points on the sphere of radius 0.5."""
    r = np.random.RandomState(seed)
    p = r.normal(size=(n, 3))
    cloud = (0.5 * p / np.linalg.norm(p, axis=1, keepdims=True)).astype(f32)
    out = cloud, _lists(cloud, k)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def slab(n=1024, k=16, seed=1):
    """(cloud, index): x, z uniform in [-1, 1], y = 0.02 N(0, 1)."""
    r = np.random.RandomState(seed)
    cloud = np.stack([r.uniform(-1, 1, n), 0.02 * r.normal(size=n), r.uniform(-1, 1, n)], axis=1).astype(f32)
    out = cloud, _lists(cloud, k)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mix(n=1024, k=16, seed=2):
    """(points, offsets, index): a ragged set of four scans (100, 37, 500 and n - 637 rows) cut from a shuffle of three kinds of
    rows, a third each: uniform in a box, flat (a tilted plane with little noise) and nearly collinear."""
    r = np.random.RandomState(seed)
    a = r.uniform(-1, 1, (n // 3, 3))
    u, v = r.uniform(-1, 1, (2, n // 3))
    b = np.stack([u + 3, v, 0.3 * u - 0.2 * v + 1e-3 * r.normal(size=n // 3)], axis=1)
    t = r.uniform(-1, 1, n - 2 * (n // 3))
    c = np.stack([t - 3, 2 * t, -t], axis=1) + 1e-3 * r.normal(size=(len(t), 3))
    cloud = np.concatenate([a, b, c])[r.permutation(n)].astype(f32)
    offsets = np.array([0, 100, 137, 637, n], dtype=np.int64)
    out = cloud, offsets, knn_law.knn_law(cloud, offsets, k)[0]
    for a in out:
        a.setflags(write=False)
    return out


def hand_index(lengths, k, seed=3):
    """A hand-made list for scans of the given lengths: random rows of the scan with -1, out-of-range values on both sides,
    duplicates and the row itself mixed in.  (sum(lengths), k) int32."""
    r = np.random.RandomState(seed)
    out = []
    for n in lengths:
        idx = r.randint(0, n, (n, k)).astype(np.int64)
        kind = r.randint(0, 8, (n, k))
        idx = np.where(kind == 0, -1, idx)
        idx = np.where(kind == 1, n + r.randint(0, 5, (n, k)), idx)
        idx = np.where(kind == 2, r.choice([-2, -(1 << 31), (1 << 31) - 1, 1 << 20], (n, k)), idx)
        idx = np.where(kind == 3, np.arange(n)[:, None], idx)                    # the row itself
        idx[:, 1] = np.where(kind[:, 1] == 4, idx[:, 0], idx[:, 1])              # a duplicate
        out.append(idx)
    return np.concatenate(out).astype(np.int32)


def edge_fixture(side=24, gap=0.15):
    """Two parallel square grids of side x side rows (y = 0 and y = gap = 3.6 spacings of 1/side: for k = 8 a row's neighbours
    lie within 1.42 spacings, a corner row's within 2.83, so a plane never sees the other) and one row of mixed pixels between them — the
    rows a depth sensor invents at a depth edge: `side` rows along x half a spacing off a grid line in z, at heights
    scattered over the middle 40 % of the gap, so their neighbourhoods reach both planes.  Returns (cloud float32,
    planted (n) bool, interior (n) bool — the planes' rows more than 3 spacings in z from the planted row: exactly flat)."""
    g = (np.arange(side) + 0.5) / side
    x, z = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    low = np.stack([x, np.zeros_like(x), z], axis=1)
    high = np.stack([x, np.full_like(x, gap), z], axis=1)
    z0 = side // 2 / side                                       # between two grid lines
    ys = gap * (0.3 + 0.4 * ((np.arange(side) * 7) % 11) / 10.0)
    veil = np.stack([g, ys, np.full(side, z0)], axis=1)
    cloud = np.concatenate([low, high, veil]).astype(f32)
    planted = np.arange(len(cloud)) >= 2 * side * side
    interior = ~planted & (np.abs(cloud[:, 2] - z0) > 3.0 / side)
    return cloud, planted, interior

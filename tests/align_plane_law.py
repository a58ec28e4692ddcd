"""The point-to-plane registration law in numpy — the checker of csrc/align_plane.hip, written from the law itself.

The sets, the jobs, the transform, absence, the match, the gate, the frame and `quantise` are align_law's, taken as they are:
index and dist2 are align_law.step's bit for bit.  What differs is what a correspondence contributes.

    normals    tnormals (U,3) float32, aligned with tpoints.  A correspondence matched to row j uses n = tnormals[j];
               w = trunc(ldexp(n, 9)) per component.  It is *without normal* when a component of n is not finite, when
               w.w == 0 or when w.w > 2**18 + 2**11 (not a unit vector; a component with |ldexp(n, 9)| >= 2**10 alone exceeds
               that and is never converted): counted in [2], in no sum.  scan_normals' NaN rows are without normal.
    order      of a gated correspondence: clipped (align_law's rule, counted in [1]) first, then without normal.
    terms      u, v as in align_law (magnitude < 2**20), d = u - v, c = u x w, a = (c, w) (6), b = -d.w.
               |u|_2 < sqrt(3) 2**20, |d|_2 < sqrt(3) 2**21, |w|_2 <= sqrt(2**18 + 2**11) < 1.004 * 2**9, so by Cauchy-Schwarz
               |c|_2 < 1.74 * 2**29 < 2**30 and |b| < 1.74 * 2**30 < 2**31: every product a_i a_j, a_i b, b b is below 2**62 in
               magnitude.  Asserted here in Python integers.
    sums       28 exact integers: the 21 a_i a_j (i <= j, row-major), the 6 a_i b, then b b.  A sum over 2**16 rows can reach
               2**78, so each is carried as a pair: per row lo = term & (2**31 - 1), hi = term >> 31 (arithmetic), each summed
               on its own — both stay below 2**48 in magnitude — and the host rebuilds hi * 2**31 + lo as a Python integer.
    moments    (S,H,60) int64: [0] used, [1] clipped, [2] without normal, [3] 0, [4 + 2i] and [5 + 2i] the hi and lo of sum i.
               Sets that align_law treats as empty give zeros.

    solve      rigid_from_plane_moments: A (6x6) = sum a a^T and g = sum a b from the exact integers, converted to float64;
               A x = g with x = (omega, t') solved in the scaling D^-1 A D^-1, D = (r, r, r, m, m, m) with r = sqrt(trace of
               the rotation block / 3) and m = sqrt(trace of the translation block / 3): the two blocks have different
               units, and one scale per block removes the units without touching the anisotropy within a block (see
               DEGENERATE_PLANE for why not sqrt(diag A)).  R = the exact rotation by |omega| about omega (the identity at
               0), t = ldexp(t', shift - 19), delta = [R | anchor - R anchor + t]: the turn is about the anchor.
               rms = ldexp(sqrt(sum b b / used), shift - 28), the rms point-to-plane distance.
               used < 6, a zero on the diagonal, or lambda_min <= DEGENERATE_PLANE * lambda_max of the scaled matrix
               (numpy.linalg.eigh): the identity, ok False.
    chain      align_plane: align_law.align's loop without the yaw branch.
"""
import functools

import numpy as np

import align_law
import normals_law

f32 = np.float32
MOMENTS = 60
SUMS = 28
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]          # the 21 entries of A, row-major over i <= j
NORMAL_BITS = 9
NORMAL_MAX = 2 ** 18 + 2 ** 11                                   # w.w of a unit normal is at most 2**18; above this: not one
MASK31 = (1 << 31) - 1
# lambda_min / lambda_max of the block-scaled 6x6 system at or below which sliding counts as unconstrained.  Measured with this
# law at the first step from the identity (test_align_plane_law_host.py asserts the figures):
#     slab_pair()  (one plane, noise 0.002, turned 2 degrees)    3.75e-5    refused
#     wavy_pair()  (noise 0.002, turned 8 degrees)               7.38e-3    accepted
# a factor 197 apart; the geometric mean is 5.3e-4 and the nearest power of two 2**-11 = 4.9e-4.
# Two things were measured and not used.  (1) normals_law.slab(), noise 0.02 over neighbourhoods of radius ~0.14: 5.5e-3, as
# constrained as the wavy sheet itself — its normals tilt by some 15 degrees, and those tilts do hold the slide; it is no
# fixture of a degenerate system, so the refused fixture is the same slab at the sheet's noise.  (2) The scaling by sqrt(diag A)
# (Jacobi's): it gives 0.66 for normals_law.slab(), 0.61 for slab_pair() and 0.10 for wavy_pair() — the plane *above* the
# sheet.  On a noisy plane the columns c_y, w_x, w_z hold nothing but the normals' noise; dividing each by its own length makes
# them unit columns that correlate with nothing, and the scaled matrix is well conditioned at every noise level until the
# normals round to one integer vector and the diagonal holds an exact zero (slab noise <= 1e-4).  It cannot see a slide.
DEGENERATE_PLANE = 2.0 ** -11


def normal_ints(normals):
    """(w (n,3) int64, has (n) bool) of normals (n,3) float32: the 10-bit integers and which rows have a usable normal."""
    normals = np.asarray(normals, dtype=f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        scaled = np.ldexp(normals, NORMAL_BITS)
        small = (np.abs(scaled) < f32(2 ** 10)).all(axis=1)      # false for a NaN and an infinity
    assert scaled.dtype == f32
    w = np.trunc(np.where(small[:, None], scaled, f32(0))).astype(np.int64)
    ww = (w * w).sum(axis=1)
    return w, small & (ww != 0) & (ww <= NORMAL_MAX)


def terms_of(u, v, w):
    """(n,28) int64: the terms of the used correspondences u, v, w (n,3) int64, with the law's bounds asserted."""
    d = u - v
    c = np.cross(u, w)
    b = -(d * w).sum(axis=1)
    if len(u):
        assert int(np.abs(u).max()) < 2 ** 20 and int(np.abs(v).max()) < 2 ** 20
        assert max(sum(int(x) ** 2 for x in row) for row in c) < 2 ** 60        # |c|_2 < 2**30, in Python integers
        assert max(abs(int(x)) for x in b) < 2 ** 31
    a = np.concatenate([c, w], axis=1)
    out = np.empty((len(u), SUMS), dtype=np.int64)
    for k, (i, j) in enumerate(PAIRS):
        out[:, k] = a[:, i] * a[:, j]
    out[:, 21:27] = a * b[:, None]
    out[:, 27] = b * b
    if len(u):
        assert max(abs(int(x)) for x in np.abs(out).max(axis=0)) < 2 ** 62
    return out


def used_rows(moved, target, normals, index, dist2, g2, anchor, shift):
    """(u, v, w (n,3) int64 of the used correspondences, rows (n) their source rows, clipped, without) of one job."""
    with np.errstate(all="ignore"):
        corr = (index >= 0) & (dist2 <= g2)
    rows = np.flatnonzero(corr)
    u, iu = align_law.quantise(moved[rows], anchor, shift)
    v, iv = align_law.quantise(target[index[rows]], anchor, shift)
    inside = iu & iv
    w, has = normal_ints(normals[index[rows]])
    use = inside & has
    return u[use], v[use], w[use], rows[use], int((~inside).sum()), int((inside & ~has).sum())


def moments_of(moved, target, normals, index, dist2, g2, anchor, shift):
    """(60) int64 of one job."""
    out = np.zeros(MOMENTS, dtype=np.int64)
    u, v, w, _, clipped, without = used_rows(moved, target, normals, index, dist2, g2, anchor, shift)
    out[0], out[1], out[2] = len(u), clipped, without
    t = terms_of(u, v, w)
    out[4::2] = (t >> 31).sum(axis=0)
    out[5::2] = (t & MASK31).sum(axis=0)
    assert max(abs(int(x)) for x in out) < 2 ** 48
    return out


def sums_of(moments60):
    """The 28 sums of one job as Python integers."""
    m = [int(x) for x in moments60]
    return [m[4 + 2 * i] * (1 << 31) + m[5 + 2 * i] for i in range(SUMS)]


def step(points, offsets, tpoints, toffsets, tnormals, transforms, max_dist, anchor, shift, match=None):
    """One point-to-plane step of every job -> dict(moments (S,H,60) int64, index (H,T) int32, dist2 (H,T) float32).
    match: as in align_law.step."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    tpoints = np.ascontiguousarray(np.asarray(tpoints, dtype=f32)).reshape(-1, 3)
    tnormals = np.ascontiguousarray(np.asarray(tnormals, dtype=f32)).reshape(-1, 3)
    assert len(tnormals) == len(tpoints)
    offsets, toffsets = np.asarray(offsets, dtype=np.int64), np.asarray(toffsets, dtype=np.int64)
    S = len(offsets) - 1
    transforms = np.asarray(transforms, dtype=f32).reshape(S, -1, 12)
    H, T = transforms.shape[1], len(points)
    assert len(toffsets) == S + 1 and 1 <= H <= align_law.MAX_HYPOTHESES
    md = f32(max_dist)
    assert md >= 0
    with np.errstate(over="ignore"):
        g2 = f32(md * md)
    anchor, shift = np.asarray(anchor, dtype=f32).reshape(S, 3), np.asarray(shift).reshape(S)
    out = {"moments": np.zeros((S, H, MOMENTS), dtype=np.int64), "index": np.full((H, T), -1, dtype=np.int32),
           "dist2": np.full((H, T), np.inf, dtype=f32)}
    for s in range(S):
        if not (align_law.valid_set(offsets, s, T) and align_law.valid_set(toffsets, s, len(tpoints))):
            continue
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        tlo, thi = int(toffsets[s]), int(toffsets[s + 1])
        cloud, target, normals = points[lo:hi], tpoints[tlo:thi], tnormals[tlo:thi]
        for h in range(H):
            moved, present = align_law.transform_rows(cloud, transforms[s, h])
            if match is not None:
                index, dist2 = match["index"][h, lo:hi], match["dist2"][h, lo:hi]
            elif present.any():
                index, dist2 = align_law.match_rows(moved, present, target)
            else:
                continue
            out["index"][h, lo:hi], out["dist2"][h, lo:hi] = index, dist2
            out["moments"][s, h] = moments_of(moved, target, normals, index, dist2, g2, anchor[s], shift[s])
    return out


def system_of(moments60):
    """(A (6,6) float64, g (6) float64, bb) of one job: the exact integers, converted once."""
    sums = sums_of(moments60)
    A = [[0] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(PAIRS):
        A[i][j] = A[j][i] = sums[k]
    return np.array(A, dtype=object).astype(np.float64), np.array(sums[21:27], dtype=object).astype(np.float64), sums[27]


def solve_plane(moments60):
    """(x (6) float64 = (omega, t' in units of the frame), ok, ratio = lambda_min / lambda_max of the scaled system, NaN
    where it was not reached) of one job."""
    x, ratio = np.zeros(6, dtype=np.float64), np.nan
    if int(moments60[0]) < 6:
        return x, False, ratio
    A, g, _ = system_of(moments60)
    diag = np.diagonal(A)
    if not (diag > 0).all():
        return x, False, ratio
    r, m = np.sqrt((diag[0] + diag[1] + diag[2]) / 3.0), np.sqrt((diag[3] + diag[4] + diag[5]) / 3.0)
    D = np.array([r, r, r, m, m, m])
    scaled = A / D[:, None] / D[None, :]
    values = np.linalg.eigh(scaled)[0]
    ratio = float(values[0] / values[5])
    if not values[0] > DEGENERATE_PLANE * values[5]:
        return x, False, ratio
    return np.linalg.solve(scaled, g / D) / D, True, ratio


def rigid_from_plane_moments(moments, shift, anchor):
    """(delta (...,3,4) float64, ok (...) bool, rms (...) float64) of moments (...,60) with the sets on the first axis; shift
    (S), anchor (S,3).  delta is the Gauss-Newton step of the point-to-plane error, with the exact rotation of its twist."""
    moments = np.asarray(moments)
    lead = moments.shape[:-1]
    S = lead[0]
    mom = moments.reshape(S, -1, MOMENTS)
    shift, anchor = np.asarray(shift).reshape(S), np.asarray(anchor, dtype=np.float64).reshape(S, 3)
    J = mom.shape[1]
    delta = np.zeros((S, J, 3, 4), dtype=np.float64)
    delta[:, :, :, :3] = np.eye(3)
    ok, rms = np.zeros((S, J), dtype=bool), np.full((S, J), np.inf, dtype=np.float64)
    for s in range(S):
        back = int(shift[s]) - 19
        for j in range(J):
            used = int(mom[s, j, 0])
            if used > 0:
                rms[s, j] = np.ldexp(np.sqrt(sums_of(mom[s, j])[27] / used), back - NORMAL_BITS)
            x, ok[s, j], _ = solve_plane(mom[s, j])
            if not ok[s, j]:
                continue
            angle = float(np.linalg.norm(x[:3]))
            R = align_law.rotation(x[:3], angle) if angle != 0 else np.eye(3)
            delta[s, j, :, :3], delta[s, j, :, 3] = R, anchor[s] - R @ anchor[s] + np.ldexp(x[3:], back)
    return delta.reshape(lead + (3, 4)), ok.reshape(lead), rms.reshape(lead)


def align_plane(points, offsets, tpoints, toffsets, tnormals, max_dist, iters=10, tol=0.0, init=None, step_fn=step):
    """The point-to-plane chain -> (transforms (S,3,4) float64, ok (S) bool, rms (S) float64, matched (S) int64): T in
    float64, step at float32(T), T <- delta o T where ok; `iters` steps, fewer once every set's delta is within tol of the
    identity (as align_law.align); one more step measures ok, rms and matched at the transforms returned."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    tpoints = np.ascontiguousarray(np.asarray(tpoints, dtype=f32)).reshape(-1, 3)
    offsets, toffsets = np.asarray(offsets, dtype=np.int64), np.asarray(toffsets, dtype=np.int64)
    S = len(offsets) - 1
    anchor, shift = align_law.frame(tpoints, toffsets, max_dist)
    run = lambda T: step_fn(points, offsets, tpoints, toffsets, tnormals, T.astype(f32).reshape(S, -1, 12), max_dist, anchor,
                            shift)["moments"]
    if init is None:
        T = np.zeros((S, 3, 4), dtype=np.float64)
        T[:, :, :3] = np.eye(3)
    else:
        T = np.array(init, dtype=np.float64).reshape(S, 3, 4)
    for _ in range(iters):
        delta, ok, _ = rigid_from_plane_moments(run(T[:, None]), shift, anchor)
        still = False
        for s in range(S):
            if ok[s, 0]:
                T[s] = align_law.compose(delta[s, 0], T[s])
                angle, move = align_law.motion(delta[s, 0])
                still = still or not (angle <= tol and np.ldexp(move, -int(shift[s])) <= tol)
        if tol > 0 and not still:
            break
    mom = run(T[:, None])
    _, ok, rms = rigid_from_plane_moments(mom, shift, anchor)
    return T, ok[:, 0], rms[:, 0], mom[:, 0, 0].astype(np.int64)


def reference_fp64_step(points, tpoints, tnormals, transform, max_dist, anchor, shift):
    """What one step approximates, for one set: the unquantised Gauss-Newton step in float64 on the correspondences and the
    normals the law uses.  Returns x (6) = (omega, t in the units of the points), the turn about `anchor`."""
    points, tpoints = np.asarray(points, dtype=f32).reshape(-1, 3), np.asarray(tpoints, dtype=f32).reshape(-1, 3)
    tnormals = np.asarray(tnormals, dtype=f32).reshape(-1, 3)
    moved, present = align_law.transform_rows(points, np.asarray(transform, dtype=f32).reshape(12))
    index, dist2 = align_law.match_rows(moved, present, tpoints)
    md = f32(max_dist)
    with np.errstate(over="ignore"):
        g2 = f32(md * md)
    _, _, _, rows, _, _ = used_rows(moved, tpoints, tnormals, index, dist2, g2, anchor, shift)
    p = moved[rows].astype(np.float64) - np.asarray(anchor, dtype=np.float64)
    q = tpoints[index[rows]].astype(np.float64) - np.asarray(anchor, dtype=np.float64)
    n = tnormals[index[rows]].astype(np.float64)
    a = np.concatenate([np.cross(p, n), n], axis=1)
    b = -((p - q) * n).sum(axis=1)
    return np.linalg.solve(a.T @ a, a.T @ b)


def pose_error(T, R, t):
    """(rotation error in radians, translation error) of a (3,4) pose against the planted (R, t)."""
    return align_law.motion(np.concatenate([T[:, :3] @ R.T, (T[:, 3] - t)[:, None]], axis=1))


# ---- fixtures of the suites, not of the law -------------------------------------------------------------------------------


def _wavy(x, y):
    return 0.15 * np.sin(3 * x) * np.cos(2 * y) + 0.1 * x * x


@functools.lru_cache(maxsize=None)
def wavy_pair(seed=0, n=1500, noise=0.002, degrees=8.0):
    """(source (n,3) float32, target (n,3) float32, R, t): two independent samplings of the sheet z = 0.15 sin(3x) cos(2y) +
    0.1 x^2, the target over [-1,1]^2 and the source over x > -0.6, each with `noise` N(0,1) on every coordinate; the source is
    moved by the inverse of (R, t), a turn of `degrees` about (0.3, 0.2, 0.9) and a shift: (R, t) takes it back onto the sheet."""
    r = np.random.RandomState(seed)
    x, y = r.uniform(-1, 1, (2, n))
    target = np.stack([x, y, _wavy(x, y)], axis=1) + noise * r.normal(size=(n, 3))
    r2 = np.random.RandomState(seed + 1)
    x = r2.uniform(-0.6, 1, n)
    y = r2.uniform(-1, 1, n)
    src = np.stack([x, y, _wavy(x, y)], axis=1) + noise * r2.normal(size=(n, 3))
    t = np.array([0.05, -0.03, 0.02])
    R = align_law.rotation((0.3, 0.2, 0.9), np.radians(degrees))
    out = ((src - t) @ R).astype(f32), target.astype(f32), R, t
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def normals_of(seed=0, n=1500, noise=0.002, k=16):
    """The normals (n,3) float32 of wavy_pair's target by the normals law over k neighbours."""
    target = wavy_pair(seed, n, noise)[1]
    out = normals_law.normals_scan(target, normals_law._lists(target, k))[0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def slab_pair(noise=0.002, degrees=2.0, n=1024, k=16, seed=1):
    """(source, target, normals): normals_law.slab() with y = noise N(0, 1) — at the default, wavy_pair's noise — and itself
    turned by `degrees` about (0.3, 0.2, 0.9): one noisy plane, on which sliding is unconstrained."""
    r = np.random.RandomState(seed)
    target = np.stack([r.uniform(-1, 1, n), noise * r.normal(size=n), r.uniform(-1, 1, n)], axis=1).astype(f32)
    normals = normals_law.normals_scan(target, normals_law._lists(target, k))[0]
    source = (target.astype(np.float64) @ align_law.rotation((0.3, 0.2, 0.9), np.radians(degrees))).astype(f32)
    out = source, target, normals
    for a in out:
        a.setflags(write=False)
    return out

"""The rigid-registration law in numpy — the checker of csrc/align.hip, written from the law itself.

Two ragged sets over the same S sets: the sources, rows offsets[s] .. offsets[s+1] of points (T,3) float32, and the targets,
rows toffsets[s] .. toffsets[s+1] of tpoints (U,3) float32.  Rows of other sets never take part.  A job is (set s, hypothesis
h < H) with the transform transforms[s, h] (12) float32, row-major [R | t].  Every float operation below is one float32
rounding, in the association written.

    transform  p' = (((r00*x + r01*y) + r02*z) + tx, likewise y', z').  A source row whose coordinates or p' are not all
               finite is absent for this job: index -1, dist2 +inf, no correspondence.
    match      candidates are the rows j of target set s with finite coordinates; d = q - p',
               d2 = ((dx*dx + dy*dy) + dz*dz) (knn_law's formula); a NaN d2 counts as +inf; best = the smallest d2, ties to
               the lower j; with no candidate below +inf: index -1, dist2 +inf.
    gate       g2 = max_dist*max_dist (+inf allowed); the row is a correspondence iff index >= 0 and d2 <= g2 (inclusive).
    quantise   u = trunc(ldexp(p' - anchor_s, 19 - shift_s)), v = trunc(ldexp(q - anchor_s, 19 - shift_s)) per component:
               one rounding in the subtraction, an exact scaling, truncation towards zero.  The correspondence is clipped if
               any of the six scaled components is non-finite or has magnitude >= 2**20: counted in [1], in no sum.
    moments    (S,H,18) int64, exact: [0] correspondences used, [1] clipped, [2:5] sum u, [5:8] sum v, [8:17] sum u_a*v_b
               row-major, [17] sum |u - v|^2.  At most 2**16 rows of magnitude < 2**20: every sum stays below 2**60.
    index, dist2  (H,T) int32 / float32: the best candidate (row within the target set) of every source row.
    A set that is empty on either side, beyond MAX_POINTS on either side, or whose offsets are not 0 <= lo <= hi <= T (U) gets
    the empty result: moments 0, index -1, dist2 +inf.

    frame      anchor_s = the target box centre (scan_law.boxes_fp32), 0 where it is not finite.  With
               half = float64(scale_s) * 0.45 (half the longest side) and x = half + min(float64(float32(max_dist)), half):
               shift_s = the smallest integer e with x < 2**e, clamped to [-100, 128]; 0 when x is NaN.  A component is
               clipped at 2**(shift + 1), twice that bound: no target row is ever clipped, and no gated correspondence while
               max_dist <= 3 * half.

    solve      rigid_from_moments: Horn's closed form on the exact integers, numpy float64, numpy.linalg.eigh.
    chain      align: T in float64, step at float32(T), T <- delta o T where ok.
"""
import numpy as np

import scan_law

MAX_POINTS = 65536
MAX_HYPOTHESES = 64
SHIFT_MIN, SHIFT_MAX = -100, 128
DEGENERATE = 2.0 ** -40        # the two largest eigenvalues count as equal within this share of the largest magnitude
f32 = np.float32


def frame(tpoints, toffsets, max_dist):
    """(anchor (S,3) float32, shift (S) int32) of the target sets."""
    tpoints = np.asarray(tpoints, dtype=f32).reshape(-1, 3)
    toffsets = np.asarray(toffsets, dtype=np.int64)
    S = len(toffsets) - 1
    anchor, shift = np.zeros((S, 3), dtype=f32), np.zeros(S, dtype=np.int32)
    md = float(f32(max_dist))
    for s in range(S):
        cloud = tpoints[int(toffsets[s]):int(toffsets[s + 1])]
        if len(cloud) == 0:
            continue
        with np.errstate(all="ignore"):
            center, scale = scan_law.boxes_fp32(cloud)
        anchor[s], shift[s] = frame_of_box(center, scale, md)
    return anchor, shift


def frame_of_box(center, scale, max_dist):
    """(anchor (3) float32, shift) from one box (center (3) float32, scale float32) — the rule of the docstring."""
    center = np.asarray(center, dtype=f32)
    anchor = np.where(np.isfinite(center), center, f32(0)).astype(f32)
    half = float(scale) * 0.45
    x = half + min(float(max_dist), half)
    if np.isnan(x):
        return anchor, 0
    if x == np.inf:
        return anchor, SHIFT_MAX
    if x <= 0:
        return anchor, SHIFT_MIN
    _, e = np.frexp(x)                                             # x = m * 2**e with 0.5 <= m < 1: 2**(e-1) <= x < 2**e
    return anchor, int(min(max(int(e), SHIFT_MIN), SHIFT_MAX))


def transform_rows(cloud, t12):
    """p' (n,3) float32 of the rows under one transform (12) float32; absent rows (input or result not finite) are NaN."""
    t = np.asarray(t12, dtype=f32).reshape(3, 4)
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    with np.errstate(all="ignore"):
        out = np.stack([((t[a, 0] * x + t[a, 1] * y) + t[a, 2] * z) + t[a, 3] for a in range(3)], axis=1)
    assert out.dtype == f32
    present = np.isfinite(cloud).all(axis=1) & np.isfinite(out).all(axis=1)
    out[~present] = np.nan
    return out, present


def match_rows(moved, present, target, block=32):
    """(index (n) int32, dist2 (n) float32): the best candidate of every moved row among the finite rows of target."""
    n, m = len(moved), len(target)
    index, dist2 = np.full(n, -1, dtype=np.int32), np.full(n, np.inf, dtype=f32)
    cand = np.isfinite(target).all(axis=1)
    if m == 0:
        return index, dist2
    tx, ty, tz = (np.ascontiguousarray(target[:, a]) for a in range(3))
    with np.errstate(all="ignore"):
        for i0 in range(0, n, block):
            dx, dy, dz = (t[None, :] - moved[i0:i0 + block, a, None] for a, t in enumerate((tx, ty, tz)))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == f32
            d2[:, ~cand] = np.inf
            d2[np.isnan(d2)] = np.inf
            j = np.argmin(d2, axis=1)                              # the first of equals: the lower row
            best = d2[np.arange(len(j)), j]
            hit = (best < np.inf) & present[i0:i0 + block]
            index[i0:i0 + block] = np.where(hit, j, -1)
            dist2[i0:i0 + block] = np.where(hit, best, f32(np.inf))
    return index, dist2


def quantise(rows, anchor, shift):
    """(q (n,3) int64, inside (n) bool) of rows (n,3) float32 in the frame (anchor (3) float32, shift)."""
    with np.errstate(all="ignore"):
        scaled = np.ldexp(rows - np.asarray(anchor, dtype=f32), 19 - int(shift))
    assert scaled.dtype == f32
    inside = (np.isfinite(scaled) & (np.abs(scaled) < f32(2 ** 20))).all(axis=1)
    q = np.trunc(np.where(inside[:, None], scaled, f32(0))).astype(np.int64)
    return q, inside


def moments_of(moved, target, index, dist2, g2, anchor, shift):
    """(18) int64 of one job."""
    out = np.zeros(18, dtype=np.int64)
    with np.errstate(all="ignore"):
        corr = (index >= 0) & (dist2 <= g2)
    if not corr.any():
        return out
    u, iu = quantise(moved[corr], anchor, shift)
    v, iv = quantise(target[index[corr]], anchor, shift)
    use = iu & iv
    u, v = u[use], v[use]
    out[0], out[1] = int(use.sum()), int((~use).sum())
    out[2:5], out[5:8] = u.sum(axis=0), v.sum(axis=0)
    out[8:17] = (u[:, :, None] * v[:, None, :]).sum(axis=0).reshape(9)
    out[17] = int(((u - v) ** 2).sum())
    assert max(abs(int(x)) for x in out) < 2 ** 62
    return out


def valid_set(offsets, s, rows):
    lo, hi = int(offsets[s]), int(offsets[s + 1])
    return 0 <= lo < hi <= rows and hi - lo <= MAX_POINTS


def step(points, offsets, tpoints, toffsets, transforms, max_dist, anchor, shift, match=None):
    """One ICP step of every job -> dict(moments (S,H,18) int64, index (H,T) int32, dist2 (H,T) float32).
    match: the result of an earlier call with the same sets and transforms — the matches do not depend on the gate or the
    frame, so a suite that varies those takes index and dist2 from it and only the moments are made anew."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    tpoints = np.ascontiguousarray(np.asarray(tpoints, dtype=f32)).reshape(-1, 3)
    offsets, toffsets = np.asarray(offsets, dtype=np.int64), np.asarray(toffsets, dtype=np.int64)
    S = len(offsets) - 1
    transforms = np.asarray(transforms, dtype=f32).reshape(S, -1, 12)
    H, T = transforms.shape[1], len(points)
    assert len(toffsets) == S + 1 and 1 <= H <= MAX_HYPOTHESES
    md = f32(max_dist)
    assert md >= 0
    with np.errstate(over="ignore"):
        g2 = f32(md * md)
    anchor, shift = np.asarray(anchor, dtype=f32).reshape(S, 3), np.asarray(shift).reshape(S)
    out = {"moments": np.zeros((S, H, 18), dtype=np.int64), "index": np.full((H, T), -1, dtype=np.int32),
           "dist2": np.full((H, T), np.inf, dtype=f32)}
    for s in range(S):
        if not (valid_set(offsets, s, T) and valid_set(toffsets, s, len(tpoints))):
            continue
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        cloud, target = points[lo:hi], tpoints[int(toffsets[s]):int(toffsets[s + 1])]
        for h in range(H):
            moved, present = transform_rows(cloud, transforms[s, h])
            if match is not None:
                index, dist2 = match["index"][h, lo:hi], match["dist2"][h, lo:hi]
            elif present.any():
                index, dist2 = match_rows(moved, present, target)
            else:
                continue
            out["index"][h, lo:hi], out["dist2"][h, lo:hi] = index, dist2
            out["moments"][s, h] = moments_of(moved, target, index, dist2, g2, anchor[s], shift[s])
    return out


def rigid_from_moments(moments, shift, anchor):
    """(delta (...,3,4) float64, ok (...) bool, rms (...) float64) of moments (...,18) with the sets on the first axis; shift
    (S), anchor (S,3).  delta takes the used source rows onto their targets in the least-squares sense: Horn's closed form.
    cnt < 3, or the two largest eigenvalues equal (within DEGENERATE of the largest magnitude): identity, ok False."""
    moments = np.asarray(moments)
    lead = moments.shape[:-1]
    S = lead[0]
    mom = moments.reshape(S, -1, 18)
    shift, anchor = np.asarray(shift).reshape(S), np.asarray(anchor, dtype=np.float64).reshape(S, 3)
    J = mom.shape[1]
    delta = np.zeros((S, J, 3, 4), dtype=np.float64)
    delta[:, :, :, :3] = np.eye(3)
    ok, rms = np.zeros((S, J), dtype=bool), np.full((S, J), np.inf, dtype=np.float64)
    for s in range(S):
        back = int(shift[s]) - 19
        for j in range(J):
            m = [int(x) for x in mom[s, j]]
            cnt = m[0]
            if cnt > 0:
                rms[s, j] = np.ldexp(np.sqrt(m[17] / cnt), back)
            if cnt < 3:
                continue
            c = [[cnt * m[8 + 3 * a + b] - m[2 + a] * m[5 + b] for b in range(3)] for a in range(3)]    # exact, up to 2**72
            N = np.array([[c[0][0] + c[1][1] + c[2][2], c[1][2] - c[2][1], c[2][0] - c[0][2], c[0][1] - c[1][0]],
                          [c[1][2] - c[2][1], c[0][0] - c[1][1] - c[2][2], c[0][1] + c[1][0], c[2][0] + c[0][2]],
                          [c[2][0] - c[0][2], c[0][1] + c[1][0], c[1][1] - c[0][0] - c[2][2], c[1][2] + c[2][1]],
                          [c[0][1] - c[1][0], c[2][0] + c[0][2], c[1][2] + c[2][1], c[2][2] - c[0][0] - c[1][1]]],
                         dtype=object).astype(np.float64)
            values, vectors = np.linalg.eigh(N)
            if not values[3] - values[2] > DEGENERATE * max(abs(values[0]), abs(values[3])):
                continue
            w, x, y, z = vectors[:, 3] / np.linalg.norm(vectors[:, 3])
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
            cu = anchor[s] + np.ldexp(np.array(m[2:5], dtype=np.float64) / cnt, back)
            cv = anchor[s] + np.ldexp(np.array(m[5:8], dtype=np.float64) / cnt, back)
            delta[s, j, :, :3], delta[s, j, :, 3] = R, cv - R @ cu
            ok[s, j] = True
    return delta.reshape(lead + (3, 4)), ok.reshape(lead), rms.reshape(lead)


def compose(delta, T):
    """delta o T of (3,4) float64 transforms."""
    out = np.empty((3, 4), dtype=np.float64)
    out[:, :3] = delta[:, :3] @ T[:, :3]
    out[:, 3] = delta[:, :3] @ T[:, 3] + delta[:, 3]
    return out


def motion(delta):
    """(rotation angle in radians, length of the translation) of a (3,4) transform."""
    R = delta[:, :3]
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(axis) / 2, (np.trace(R) - 1) / 2)), float(np.linalg.norm(delta[:, 3]))


def rotation(axis, angle):
    """(3,3) float64: the rotation by `angle` radians about `axis` (Rodrigues)."""
    k = np.asarray(axis, dtype=np.float64).reshape(3)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def yaw_transforms(H, axis, src_center, dst_center):
    """(..., H, 3, 4) float64: the rotation by 2 pi h / H about `axis` that takes src_center (..., 3) to dst_center."""
    src, dst = np.asarray(src_center, dtype=np.float64), np.asarray(dst_center, dtype=np.float64)
    out = np.empty(src.shape[:-1] + (H, 3, 4), dtype=np.float64)
    for h in range(H):
        R = rotation(axis, 2.0 * np.pi * h / H)
        out[..., h, :, :3] = R
        out[..., h, :, 3] = dst - src @ R.T
    return out


def align(points, offsets, tpoints, toffsets, max_dist, iters=30, tol=0.0, init=None, yaw=0, axis=(0, 1, 0), coarse_iters=3,
          step_fn=step):
    """The ICP chain -> (transforms (S,3,4) float64, ok (S) bool, rms (S) float64, matched (S) int64, hypothesis (S) int64).
    yaw = H > 0: H starts turned about `axis` through the box centres run coarse_iters steps together, one more step scores
    them (more correspondences, then the lower [17], then the lower h) and the best of each set is refined.  The refinement
    runs `iters` steps, fewer once every set's delta is within tol of the identity (angle in radians, translation over
    2**shift; tol = 0 never stops); one more step measures ok, rms and matched at the transforms returned."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    tpoints = np.ascontiguousarray(np.asarray(tpoints, dtype=f32)).reshape(-1, 3)
    offsets, toffsets = np.asarray(offsets, dtype=np.int64), np.asarray(toffsets, dtype=np.int64)
    S = len(offsets) - 1
    anchor, shift = frame(tpoints, toffsets, max_dist)
    run = lambda T: step_fn(points, offsets, tpoints, toffsets, T.astype(f32).reshape(S, -1, 12), max_dist, anchor, shift)["moments"]
    hypothesis = np.full(S, -1, dtype=np.int64)
    if yaw:
        assert init is None and 1 <= yaw <= MAX_HYPOTHESES
        centres = np.zeros((2, S, 3), dtype=np.float64)
        for k, (p, o) in enumerate(((points, offsets), (tpoints, toffsets))):
            for s in range(S):
                cloud = p[int(o[s]):int(o[s + 1])]
                if len(cloud):
                    with np.errstate(all="ignore"):
                        centres[k, s] = np.nan_to_num(scan_law.boxes_fp32(cloud)[0], nan=0.0, posinf=0.0, neginf=0.0)
        TH = yaw_transforms(yaw, axis, centres[0], centres[1])
        for _ in range(coarse_iters):
            delta, ok, _ = rigid_from_moments(run(TH), shift, anchor)
            for s in range(S):
                for h in range(yaw):
                    if ok[s, h]:
                        TH[s, h] = compose(delta[s, h], TH[s, h])
        mom = run(TH)
        T = np.empty((S, 3, 4), dtype=np.float64)
        for s in range(S):
            hypothesis[s] = min(range(yaw), key=lambda h: (-int(mom[s, h, 0]), int(mom[s, h, 17]), h))
            T[s] = TH[s, hypothesis[s]]
    elif init is None:
        T = np.zeros((S, 3, 4), dtype=np.float64)
        T[:, :, :3] = np.eye(3)
    else:
        T = np.array(init, dtype=np.float64).reshape(S, 3, 4)
    for _ in range(iters):
        delta, ok, _ = rigid_from_moments(run(T[:, None]), shift, anchor)
        still = False
        for s in range(S):
            if ok[s, 0]:
                T[s] = compose(delta[s, 0], T[s])
                angle, move = motion(delta[s, 0])
                still = still or not (angle <= tol and np.ldexp(move, -int(shift[s])) <= tol)
        if tol > 0 and not still:
            break
    mom = run(T[:, None])
    _, ok, rms = rigid_from_moments(mom, shift, anchor)
    return T, ok[:, 0], rms[:, 0], mom[:, 0, 0].astype(np.int64), hypothesis


def planted_pair(seed, n_target=600, n_source=400, degrees=20.0, shift=0.1):
    """A fixture of the suites, not of the law: (source (n_source,3) float32, target (n_target,3) float32, R (3,3), t (3),
    rows): the target is uniform in [-1, 1]^3, the source a subset `rows` of it moved by the inverse of (R, t) in float64 —
    so (R, t), a turn of `degrees` about a skew axis and a translation of length `shift`, takes the source onto the target."""
    r = np.random.RandomState(seed)
    target = r.uniform(-1, 1, (n_target, 3)).astype(f32)
    rows = np.sort(r.permutation(n_target)[:n_source])
    R = rotation((0.3, 0.9, -0.4), np.radians(degrees))
    t = np.array([0.6, -0.2, 0.77])
    t = t / np.linalg.norm(t) * shift
    source = ((target[rows].astype(np.float64) - t) @ R).astype(f32)          # R^T (q - t), row-wise
    return source, target, R, t, rows


def l_block(seed=0, n=1500):
    """A fixture of the suites: (source, target (n,3) float32, R, t).  The target is an L-shaped block — a bar along x from
    -0.25 to 1 with an arm up in z over x in [0.6, 1] —, the source its part with x > 0 moved so that (R, t), a turn of 137
    degrees about y and a shift, takes it back.  At seed 0 ICP from the identity ends 130 degrees from (R, t) and a yaw
    search over 24 starts lands on it (measured with this law: 3.5e-8 rad, 4.1e-8 in t)."""
    r = np.random.RandomState(seed)
    bar = int(n * 0.7)
    target = np.concatenate([r.uniform([-0.25, -0.25, -0.2], [1, 0.25, 0.2], (bar, 3)),
                             r.uniform([0.6, -0.25, 0.2], [1, 0.25, 0.9], (n - bar, 3))])[r.permutation(n)].astype(f32)
    R, t = rotation((0, 1, 0), np.radians(137.0)), np.array([0.15, 0.05, -0.1])
    source = ((target[target[:, 0] > 0].astype(np.float64) - t) @ R).astype(f32)
    return source, target, R, t


def two_views(seed=2, n=2000, cut=0.2):
    """A fixture of the suites: (object (n,3) float32, view 0, view 1, R, t).  The object fills a block of 0.7 x 0.6 x 0.4 with
    a second block on top of its x > 0 half; view 0 is its part with x < cut, view 1 the part with x > -cut turned 25 degrees
    about y and shifted: (R, t) takes view 1 back onto the object."""
    r = np.random.RandomState(seed)
    low = int(n * 0.7)
    obj = np.concatenate([r.uniform([-0.35, -0.3, -0.2], [0.35, 0.3, 0.2], (low, 3)),
                          r.uniform([0.0, -0.1, 0.2], [0.35, 0.3, 0.7], (n - low, 3))])[r.permutation(n)].astype(f32)
    R, t = rotation((0, 1, 0), np.radians(25.0)), np.array([0.05, 0.02, -0.04])
    view1 = ((obj[obj[:, 0] > -cut].astype(np.float64) - t) @ R).astype(f32)
    return obj, obj[obj[:, 0] < cut], view1, R, t

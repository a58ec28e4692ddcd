"""The pose-consensus law in numpy — the checker of csrc/pose_trials.hip, written from the law itself.

Two ragged sets over the same S sets, as align_law: sources points (T,3) float32 / offsets, targets tpoints (U,3) float32 /
toffsets, and match (T) int32 — for every source row a target row within its set, or -1 (feature_law.match_law's output).
Per set s with n source rows and m target rows:

    matched    a source row with 0 <= match < m whose coordinates and whose target row's coordinates are finite.
    draws      Philox4x32-10 as scan_law: key = seed, counter (stream_lo, stream_hi, q, TAG), TAG = 5; trial h < trials samples
               the source rows r_k = (word[3h+k] * n) >> 32, k = 0, 1, 2.  a, b, c are those rows, a', b', c' their targets.
    valid      a trial is valid iff: the three rows are matched; they differ; their three target rows differ; every side agrees in
               length — with l2 = ((dx*dx + dy*dy) + dz*dz) of the float32 difference, one float32 rounding per operation, for
               the sides (a,b), (a,c), (b,c): both l2 finite, ls2 >= rho2 * lt2 and lt2 >= rho2 * ls2, rho2 = float32(edge_ratio^2)
               rounded once on the host —; both triangles have a frame; the 12 float32 of the transform are finite.
    frame      of (a, b, c) in float64, one rounding per operation, dot(a, b) = (a0*b0 + a1*b1) + a2*b2, cross as feature_law:
               u = b - a, v = c - a;  l1 = sqrt(dot(u, u)), needs l1 > 0;  e1 = u / l1;  x = cross(e1, v);
               needs dot(x, x) > 2**-24 * dot(v, v) (the angle at a above 2**-12: not collinear);  e3 = x / sqrt(dot(x, x));
               e2 = cross(e3, e1);  centre = ((a + b) + c) / 3.
    fit        R_ij = (e1t_i * e1s_j + e2t_i * e2s_j) + e3t_i * e3s_j;  t_i = ct_i - ((R_i0 * cs_0 + R_i1 * cs_1) + R_i2 * cs_2);
               the transform is [R | t] row-major rounded to float32 — a start, not a least-squares fit.
    kept       the first `keep` valid trials in ascending h.  valid = the number of valid trials, kept = min(valid, keep).
    score      of a kept trial: the matched rows with d2 <= g2 and d2 finite, where p' is align_law's float32 transform of the
               row, d = q - p' with q its target row and d2 = ((dx*dx + dy*dy) + dz*dz) in float32; g2 = float32(inlier_dist)^2
               in float32, +inf allowed.
    winner     the kept trial with the most inliers, ties to the lower h: trial = its h, inliers, transform (12) float32;
               found = inliers >= min_inliers.  Without a kept trial: trial -1, inliers 0, found 0, the transform 12 quiet NaNs.
    A set that is empty on either side, beyond MAX_POINTS on either side, or whose offsets are not 0 <= lo < hi <= rows gets
    that empty result, with valid = kept = 0.
"""
import numpy as np

import scan_law
from feature_law import cross, dot

TAG = 5
MAX_TRIALS = 65536
MAX_KEEP = 4096
MAX_POINTS = 65536
COLLINEAR = 2.0 ** -24
f32, f64 = np.float32, np.float64
QNAN = np.uint32(0x7FC00000).view(f32)


def sample_rows(seed, stream, trials, n):
    """(trials, 3) int64: the sample rows of every trial of an n-row set."""
    w = scan_law.words(seed, stream, TAG, 3 * trials)
    return ((w * np.uint64(n)) >> scan_law.S32).astype(np.int64).reshape(trials, 3)


def len2(a, b):
    d = b - a
    assert d.dtype == f32
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def edges_agree(src, dst, rho2):
    """(h) bool of triangles src, dst (h,3,3) float32."""
    rho2 = f32(rho2)
    ok = np.ones(len(src), dtype=bool)
    with np.errstate(all="ignore"):
        for i, j in ((0, 1), (0, 2), (1, 2)):
            ls, lt = len2(src[:, i], src[:, j]), len2(dst[:, i], dst[:, j])
            ok &= np.isfinite(ls) & np.isfinite(lt) & (ls >= rho2 * lt) & (lt >= rho2 * ls)
    return ok


def frames(tri):
    """(ok (h), E (h,3,3) with E[:, k] = e_(k+1), centre (h,3)) of triangles (h,3,3), float64."""
    a, b, c = (tri[:, k].astype(f64) for k in range(3))
    with np.errstate(all="ignore"):
        u, v = b - a, c - a
        l1 = np.sqrt(dot(u, u))
        ok = l1 > 0
        e1 = u / np.where(ok, l1, f64(1))[:, None]
        x = cross(e1, v)
        xx = dot(x, x)
        ok = ok & (xx > f64(COLLINEAR) * dot(v, v))
        e3 = x / np.sqrt(np.where(ok, xx, f64(1)))[:, None]
        e2 = cross(e3, e1)
        centre = ((a + b) + c) / f64(3)
    return ok, np.stack([e1, e2, e3], axis=1), centre


def fit(src, dst):
    """(ok (h), transforms (h,12) float32) of triangle pairs (h,3,3) float32: the triad fit."""
    oks, Es, cs = frames(src)
    okt, Et, ct = frames(dst)
    out = np.zeros((len(src), 3, 4), dtype=f64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                out[:, i, j] = (Et[:, 0, i] * Es[:, 0, j] + Et[:, 1, i] * Es[:, 1, j]) + Et[:, 2, i] * Es[:, 2, j]
            out[:, i, 3] = ct[:, i] - ((out[:, i, 0] * cs[:, 0] + out[:, i, 1] * cs[:, 1]) + out[:, i, 2] * cs[:, 2])
        t32 = out.reshape(-1, 12).astype(f32)
    return oks & okt & np.isfinite(t32).all(axis=1), t32


def score(cloud, target, matched, t12, g2):
    """The inliers of one transform (12) float32 over the matched rows: cloud, target (n,3) float32 row for row."""
    t = np.asarray(t12, dtype=f32).reshape(3, 4)
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    with np.errstate(all="ignore"):
        moved = np.stack([((t[a, 0] * x + t[a, 1] * y) + t[a, 2] * z) + t[a, 3] for a in range(3)], axis=1)
        d2 = len2(moved, target)
        return int((matched & np.isfinite(d2) & (d2 <= g2)).sum())


def valid_set(offsets, s, rows):
    lo, hi = int(offsets[s]), int(offsets[s + 1])
    return 0 <= lo < hi <= rows and hi - lo <= MAX_POINTS


def pose_trials_law(points, offsets, tpoints, toffsets, match, inlier_dist, trials=32768, keep=1024, seed=0, streams=None,
                    edge_ratio=0.9, min_inliers=6):
    """dict(trial, inliers, found, valid, kept (S) int32, transform (S,12) float32)."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    tpoints = np.ascontiguousarray(np.asarray(tpoints, dtype=f32)).reshape(-1, 3)
    offsets, toffsets = np.asarray(offsets, dtype=np.int64), np.asarray(toffsets, dtype=np.int64)
    match = np.asarray(match, dtype=np.int32)
    S = len(offsets) - 1
    assert 1 <= trials <= MAX_TRIALS and 1 <= keep <= MAX_KEEP and len(match) == len(points)
    with np.errstate(over="ignore"):
        g2 = f32(inlier_dist) * f32(inlier_dist)
    rho2 = f32(float(edge_ratio) * float(edge_ratio))
    out = {k: np.zeros(S, dtype=np.int32) for k in ("trial", "inliers", "found", "valid", "kept")}
    out["trial"][:] = -1
    out["transform"] = np.full((S, 12), QNAN, dtype=f32)
    for s in range(S):
        if not (valid_set(offsets, s, len(points)) and valid_set(toffsets, s, len(tpoints))):
            continue
        cloud, tcloud = points[int(offsets[s]):int(offsets[s + 1])], tpoints[int(toffsets[s]):int(toffsets[s + 1])]
        mt = match[int(offsets[s]):int(offsets[s + 1])]
        n, m = len(cloud), len(tcloud)
        inr = (mt >= 0) & (mt < m)
        safe = np.where(inr, mt, 0)
        target = tcloud[safe]
        matched = inr & np.isfinite(cloud).all(axis=1) & np.isfinite(target).all(axis=1)
        rows = sample_rows(seed, s if streams is None else int(streams[s]), trials, n)
        ok = matched[rows].all(axis=1)
        ok &= (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2])
        tr = safe[rows]
        ok &= (tr[:, 0] != tr[:, 1]) & (tr[:, 0] != tr[:, 2]) & (tr[:, 1] != tr[:, 2])
        src = np.where(ok[:, None, None], cloud[rows], f32(0))
        dst = np.where(ok[:, None, None], target[rows], f32(0))
        ok &= edges_agree(src, dst, rho2)
        fit_ok, t12 = fit(src, dst)
        ok &= fit_ok
        hs = np.flatnonzero(ok)
        out["valid"][s], out["kept"][s] = len(hs), min(len(hs), keep)
        best = -1
        for h in hs[:keep]:
            c = score(cloud, target, matched, t12[h], g2)
            if c > best:
                best, out["trial"][s], out["transform"][s] = c, h, t12[h]
        if best >= 0:
            out["inliers"][s], out["found"][s] = best, int(best >= min_inliers)
    return out


def pose_error(T, R, t):
    """(rotation error in degrees, translation error) of a (3,4) or (12) transform against the planted (R, t)."""
    T = np.asarray(T, dtype=f64).reshape(3, 4)
    D = T[:, :3] @ np.asarray(R, dtype=f64).T
    axis = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.degrees(np.arctan2(np.linalg.norm(axis) / 2, (np.trace(D) - 1) / 2))), float(np.linalg.norm(T[:, 3] - t))


def global_start_law(points, offsets, tpoints, toffsets, max_dist, k=32, trials=32768, keep=1024, seed=0, streams=None,
                     edge_ratio=0.9, inlier_dist=None, min_inliers=6, viewpoints=None, tviewpoints=None):
    """The chain of ops.scan_align_global with the laws: lists (knn_law), normals facing the viewpoints (normals_law),
    descriptors and matches (feature_law), then pose_trials_law.  Returns its dict, with match (T) added."""
    import feature_law
    import knn_law
    import normals_law

    def describe(p, o, v):
        p, o = np.asarray(p, dtype=f32).reshape(-1, 3), np.asarray(o, dtype=np.int64)
        index = knn_law.knn_law(p, o, k)[0]
        views = None if v is None else np.broadcast_to(np.asarray(v, dtype=f32), (len(o) - 1, 3))
        normals = normals_law.normals_law(p, o, index, views)[0]
        return feature_law.feature_law(p, o, normals, index)[:2]

    feat, cnt = describe(points, offsets, viewpoints)
    tfeat, tcnt = describe(tpoints, toffsets, tviewpoints)
    match = feature_law.match_law(feat, offsets, tfeat, toffsets, cnt, tcnt)[0]
    out = pose_trials_law(points, offsets, tpoints, toffsets, match, max_dist if inlier_dist is None else inlier_dist, trials=trials,
                          keep=keep, seed=seed, streams=streams, edge_ratio=edge_ratio, min_inliers=min_inliers)
    out["match"] = match
    return out


def refine_law(points, offsets, tpoints, toffsets, start, max_dist, iters=10, k=32, coarse=5):
    """DeviceScanDataset.aligned_globally's refinement with the laws: `coarse` point-to-point steps from `start` (S,3,4), then
    `iters` point-to-plane steps on the targets' normals over k neighbours; a stage that is refused keeps the one before."""
    import align_law
    import align_plane_law
    import knn_law
    import normals_law
    start = np.asarray(start, dtype=f64)
    poses, ok, _, _, _ = align_law.align(points, offsets, tpoints, toffsets, max_dist, iters=coarse, init=start)
    poses[~ok] = start[~ok]
    tpoints, toffsets = np.asarray(tpoints, dtype=f32).reshape(-1, 3), np.asarray(toffsets, dtype=np.int64)
    tnormals = normals_law.normals_law(tpoints, toffsets, knn_law.knn_law(tpoints, toffsets, k)[0])[0]
    fine, fine_ok, _, _ = align_plane_law.align_plane(points, offsets, tpoints, toffsets, tnormals, max_dist, iters=iters, init=poses)
    poses[fine_ok] = fine[fine_ok]
    return poses

"""The supporting-plane law in numpy — the checker of csrc/plane.hip, written from the law itself.

Everything is per scan (rows offsets[s] .. offsets[s+1] of points (T,3) float32); rows of other scans never take part.
Every float operation below is one float32 rounding, in the association written.

    absent     a row with a non-finite coordinate (as in knn_law); never an inlier.
    draws      Philox4x32-10 as in scan_law: key = seed, counter (stream_lo, stream_hi, q, TAG), TAG = 4; word i is lane
               i & 3 of block i >> 2.  Trial h samples rows r_k = (word[3h+k] * n) >> 32, k = 0, 1, 2.
    trial h    a, b, c = rows r_0, r_1, r_2;  u = b - a, v = c - a;
               nrm = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x);  len2 = ((nx*nx + ny*ny) + nz*nz);
               t2 = threshold*threshold;  rhs = t2*len2;  valid iff n >= 3, len2 finite and > 0, rhs finite.
    inlier     row p of trial h iff e*e <= rhs with e = ((nx*(p.x-a.x) + ny*(p.y-a.y)) + nz*(p.z-a.z)): inclusive; a NaN or an
               overflowed e*e is never <= rhs.
    winner     the valid trial with the most inliers, ties to the lower h; trial = -1 when no trial is valid.
               found = count >= min_inliers and float64(count) >= float64(float32(min_share)) * float64(n).
    outputs    inliers = the winner's count (0);  sample = its rows (-1, -1, -1);  sample_plane = (nx, ny, nz,
               -((nx*a.x + ny*a.y) + nz*a.z)), not normalised (four quiet NaNs);  inlier = its mask (zeros).
    moments    of the winner's inliers: dq = p - a; M = the largest |dq_c|; e = M's biased exponent field - 127 (= floor(log2 M)
               for a normal M); q_c = trunc(ldexp(dq_c, 19 - e)), exact, |q_c| < 2**20;
               moments = [cnt, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz] over the q's as int64, cnt the winner's count; shift = e.
               M == 0 (every inlier sits on row a): shift = 0 and the nine sums are 0.  trial = -1: ten zeros, shift 0.
    A scan longer than MAX_POINTS, or shorter than 3 rows, gets the empty result (trial -1).

    side       against a given plane (nx, ny, nz, d): dist = ((nx*p.x + ny*p.y) + nz*p.z) + d, the quiet NaN for an absent row
               (and for any NaN); keep = present and not |dist| <= threshold; kept = the scan's count.
"""
import numpy as np

import scan_law

TAG = 4
MAX_POINTS = 1 << 22
MAX_TRIALS = 4096
f32 = np.float32


def t2_of(threshold):
    t = f32(threshold)
    with np.errstate(over="ignore"):
        t2 = f32(t * t)
    assert t >= 0 and np.isfinite(t2), threshold
    return t2


def sample_rows(seed, stream, trials, n):
    """(trials, 3) int64: the sample rows of every trial of an n-row scan."""
    w = scan_law.words(seed, stream, TAG, 3 * trials)
    return ((w * np.uint64(n)) >> scan_law.S32).astype(np.int64).reshape(trials, 3)


def hypotheses(cloud, rows, t2):
    """a (H,3), nrm (H,3), rhs (H), valid (H) of the trials with sample rows `rows` (H,3)."""
    with np.errstate(all="ignore"):
        a, b, c = (cloud[rows[:, k]] for k in range(3))
        u, v = b - a, c - a
        nrm = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1],
                        u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                        u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        len2 = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        rhs = t2 * len2
    assert nrm.dtype == f32 and len2.dtype == f32 and rhs.dtype == f32
    return a, nrm, rhs, np.isfinite(len2) & (len2 > 0) & np.isfinite(rhs)


def inlier_mask(cloud, a, nrm, rhs):
    """(n) bool: the inliers of one trial."""
    with np.errstate(all="ignore"):
        dq = cloud - a
        e = (nrm[0] * dq[:, 0] + nrm[1] * dq[:, 1]) + nrm[2] * dq[:, 2]
        e2 = e * e
    assert e2.dtype == f32
    return np.isfinite(cloud).all(axis=1) & (e2 <= rhs)              # a NaN compares false


def moments_of(cloud, mask, a):
    """(moments (10) int64, shift) of the rows `mask` about the row a."""
    out = np.zeros(10, dtype=np.int64)
    out[0] = int(mask.sum())
    dq = cloud[mask] - a
    assert dq.dtype == f32
    M = f32(np.abs(dq).max()) if len(dq) else f32(0)
    if M == 0:
        return out, 0
    e = int((M.view(np.uint32) >> np.uint32(23)) & np.uint32(0xFF)) - 127
    scaled = np.ldexp(dq, 19 - e)
    assert scaled.dtype == f32
    q = np.trunc(scaled).astype(np.int64)
    assert np.abs(q).max() < 2 ** 20
    out[1:4] = q.sum(axis=0)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    out[4:] = [int((q[:, i] * q[:, j]).sum()) for i, j in pairs]
    return out, e


def plane_scan(cloud, seed, stream, trials, threshold, min_inliers=3, min_share=0.0, block=64):
    """One scan -> dict(trial, inliers, found, sample (3), sample_plane (4) float32, inlier (n) uint8, moments (10) int64,
    shift, counts (H) int64, valid (H))."""
    cloud = np.ascontiguousarray(np.asarray(cloud, dtype=f32)).reshape(-1, 3)
    n, t2 = len(cloud), t2_of(threshold)
    assert 1 <= trials <= MAX_TRIALS and min_inliers >= 3 and 0 <= min_share <= 1
    res = {"trial": -1, "inliers": 0, "found": 0, "sample": np.full(3, -1, dtype=np.int32),
           "sample_plane": np.full(4, np.nan, dtype=f32), "inlier": np.zeros(n, dtype=np.uint8),
           "moments": np.zeros(10, dtype=np.int64), "shift": 0,
           "counts": np.zeros(trials, dtype=np.int64), "valid": np.zeros(trials, dtype=bool)}
    if n < 3 or n > MAX_POINTS:
        return res
    rows = sample_rows(seed, stream, trials, n)
    a, nrm, rhs, valid = hypotheses(cloud, rows, t2)
    present = np.isfinite(cloud).all(axis=1)
    counts = np.zeros(trials, dtype=np.int64)
    with np.errstate(all="ignore"):
        for h0 in range(0, trials, block):                           # (block, n) at a time
            A, N, R = a[h0:h0 + block], nrm[h0:h0 + block], rhs[h0:h0 + block]
            dq = cloud[None, :, :] - A[:, None, :]
            e = (N[:, None, 0] * dq[:, :, 0] + N[:, None, 1] * dq[:, :, 1]) + N[:, None, 2] * dq[:, :, 2]
            e2 = e * e
            assert e2.dtype == f32
            counts[h0:h0 + block] = ((e2 <= R[:, None]) & present[None, :]).sum(axis=1)
    counts[~valid] = 0
    res["counts"], res["valid"] = counts, valid
    if not valid.any():
        return res
    h = int(np.argmax(np.where(valid, counts, -1)))                  # argmax: the first of equals, the lower trial
    mask = inlier_mask(cloud, a[h], nrm[h], rhs[h])
    assert int(mask.sum()) == counts[h]
    with np.errstate(all="ignore"):
        d = -((nrm[h, 0] * a[h, 0] + nrm[h, 1] * a[h, 1]) + nrm[h, 2] * a[h, 2])
    share = np.float64(f32(min_share)) * np.float64(n)
    res.update(trial=h, inliers=int(counts[h]), sample=rows[h].astype(np.int32),
               found=int(counts[h] >= min_inliers and np.float64(counts[h]) >= share),
               sample_plane=np.array([nrm[h, 0], nrm[h, 1], nrm[h, 2], d], dtype=f32), inlier=mask.astype(np.uint8))
    res["moments"], res["shift"] = moments_of(cloud, mask, a[h])
    return res


def plane_law(points, offsets, threshold, trials=512, seed=0, streams=None, min_inliers=3, min_share=0.0):
    """The ragged set -> dict of arrays: trial, inliers, found (S) int32, sample (S,3) int32, sample_plane (S,4) float32,
    inlier (T) uint8, moments (S,10) int64, shift (S) int32."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    S = len(offsets) - 1
    streams = np.arange(S) if streams is None else np.asarray(streams)
    out = {"trial": np.zeros(S, np.int32), "inliers": np.zeros(S, np.int32), "found": np.zeros(S, np.int32),
           "sample": np.zeros((S, 3), np.int32), "sample_plane": np.zeros((S, 4), f32),
           "inlier": np.zeros(len(points), np.uint8), "moments": np.zeros((S, 10), np.int64), "shift": np.zeros(S, np.int32)}
    for s in range(S):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        r = plane_scan(points[lo:hi], seed, int(streams[s]), trials, threshold, min_inliers, min_share)
        for name in out:
            if name == "inlier":
                out[name][lo:hi] = r[name]
            else:
                out[name][s] = r[name]
    return out


def planted_scan(r, n, share=0.6, band=0.004, normal=(0.3, 0.9, -0.2), d=-0.1):
    """A fixture of the suites, not of the law: (cloud (n,3) float32, planted (n) bool, unit normal, d).  round(share * n) rows
    lie within +-band of the plane normal . p + d = 0 across the box [-1, 1]^3, the rest is uniform in the box; shuffled."""
    normal = np.asarray(normal, dtype=np.float64)
    normal = normal / np.linalg.norm(normal)
    m = int(round(share * n))
    p = r.uniform(-1, 1, (m, 3))
    p += ((r.uniform(-band, band, m) - d) - p @ normal)[:, None] * normal[None, :]
    cloud = np.concatenate([p, r.uniform(-1, 1, (n - m, 3))])
    planted = np.arange(n) < m
    order = r.permutation(n)
    return cloud[order].astype(f32), planted[order], normal, d


def side_law(points, offsets, planes, threshold):
    """(dist (T) float32, keep (T) uint8, kept (S) int32) against the planes (S,4) float32."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    planes = np.asarray(planes, dtype=f32).reshape(-1, 4)
    t2_of(threshold)
    S = len(offsets) - 1
    pl = planes[np.repeat(np.arange(S), np.diff(offsets))]
    with np.errstate(all="ignore"):
        d = ((pl[:, 0] * points[:, 0] + pl[:, 1] * points[:, 1]) + pl[:, 2] * points[:, 2]) + pl[:, 3]
        assert d.dtype == f32
        present = np.isfinite(points).all(axis=1)
        d = np.where(present & ~np.isnan(d), d, f32(np.nan)).astype(f32)
        keep = present & ~(np.abs(d) <= f32(threshold))
    kept = np.array([int(keep[int(offsets[s]):int(offsets[s + 1])].sum()) for s in range(S)], dtype=np.int32)
    return d, keep.astype(np.uint8), kept

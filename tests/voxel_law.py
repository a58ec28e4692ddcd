"""The voxel-grid law in numpy — the checker of csrc/voxels.hip, written from the law itself.

Everything is per scan (rows offsets[s] .. offsets[s+1] of points (T,3) float32); rows of other scans never take part.
Every float operation below is one float32 rounding, in the association written; numpy's float32 division is the correctly
rounded one.

    voxel      the scan's cell edge, float32.  Not finite or not > 0: the empty result.
    origin     None: u = p, no operation.  Otherwise u = p - origin, one subtraction per axis.
    absent     a row with a non-finite coordinate (as in knn_law).
    cell       q_c = floor(u_c / voxel); inside iff -2**20 <= q_c < 2**20 on all three axes (a NaN or infinite quotient is
               not inside); a present row that is not inside is beyond the grid and takes no part.
               key = ((qx + 2**20) << 42) | ((qy + 2**20) << 21) | (qz + 2**20).
    centre     m_c = (float32(q_c) + 0.5) * voxel: the convert and the add are exact, the product is rounded once.
    d2         ((dx*dx + dy*dy) + dz*dz) with d = u - m; +inf is a legal value.
    rank       keep "center": (the uint32 bits of d2, the row), ascending;  keep "first": the row.
    label      the smallest row among the inside rows of the row's cell; -1 for absent and beyond rows.
    size       the inside rows of that cell; 0 for absent and beyond rows.
    keep       1 iff the row is inside and has the smallest rank of its cell.
    kept       the rows kept = the occupied cells.    beyond = the present rows outside the grid.
    A scan that is empty, longer than MAX_POINTS or has a bad voxel: every label -1, size 0, keep 0, kept 0, beyond 0.

    thin_to    the bisection of DeviceScanDataset.thinned(max_points=m): hi = the scan's box scale (max side / 0.9 on float32
               as datasets/real_data.py:26-33; 1 where it is 0), lo = 0; 16 rounds of mid = (lo + hi) * 0.5 in float32,
               accepted (hi = mid) iff kept(mid) <= m and beyond(mid) == 0, else lo = mid; the edge used is hi.
"""
import numpy as np

GRID_HALF = 1 << 20
MAX_POINTS = 1 << 22
ROUNDS = 16
f32 = np.float32
KEEPS = ("center", "first")


def _empty(n):
    return {"label": np.full(n, -1, np.int32), "size": np.zeros(n, np.int32), "keep": np.zeros(n, np.uint8), "kept": 0, "beyond": 0}


def cells(cloud, voxel, origin=None):
    """(present (n) bool, inside (n) bool, q (n,3) int64 — 0 where not inside —, u (n,3) float32) of one scan."""
    voxel = f32(voxel)
    present = np.isfinite(cloud).all(axis=1)
    with np.errstate(all="ignore"):
        u = cloud if origin is None else cloud - np.asarray(origin, dtype=f32).reshape(1, 3)
        qf = np.floor(u / voxel)
    assert u.dtype == f32 and qf.dtype == f32
    inside = present & ((qf >= -GRID_HALF) & (qf < GRID_HALF)).all(axis=1)        # a NaN compares false
    q = np.where(inside[:, None], qf, 0).astype(np.int64)
    return present, inside, q, u


def voxel_scan(cloud, voxel, origin=None, keep="center"):
    """One scan -> dict(label (n) int32, size (n) int32, keep (n) uint8, kept, beyond)."""
    assert keep in KEEPS
    cloud = np.ascontiguousarray(np.asarray(cloud, dtype=f32)).reshape(-1, 3)
    n, voxel = len(cloud), f32(voxel)
    res = _empty(n)
    if n == 0 or n > MAX_POINTS or not np.isfinite(voxel) or not voxel > 0:
        return res
    present, inside, q, u = cells(cloud, voxel, origin)
    res["beyond"] = int((present & ~inside).sum())
    rows = np.flatnonzero(inside)
    if len(rows) == 0:
        return res
    q, u = q[rows], u[rows]
    key = ((q[:, 0] + GRID_HALF) << 42) | ((q[:, 1] + GRID_HALF) << 21) | (q[:, 2] + GRID_HALF)
    if keep == "center":
        with np.errstate(all="ignore"):
            m = (q.astype(f32) + f32(0.5)) * voxel
            d = u - m
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert m.dtype == f32 and d2.dtype == f32
        rank = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    else:
        rank = rows.astype(np.uint64)
    order = np.lexsort((rows, key))                                  # by cell, then by row
    skey = key[order]
    start = np.flatnonzero(np.concatenate([[True], skey[1:] != skey[:-1]]))
    count = np.diff(np.concatenate([start, [len(rows)]]))
    cell = np.repeat(np.arange(len(start)), count)                   # the cell of every sorted row
    res["label"][rows[order]] = rows[order][start][cell]
    res["size"][rows[order]] = count[cell]
    best = np.minimum.reduceat(rank[order], start)
    res["keep"][rows[order]] = rank[order] == best[cell]
    res["kept"] = len(start)
    assert int(res["keep"].sum()) == len(start)
    return res


def voxel_law(points, offsets, voxel, origin=None, keep="center"):
    """The ragged set -> dict of arrays: label, size (T) int32, keep (T) uint8, kept, beyond (S) int32.  voxel: one edge or
    (S); origin: None or (S,3)."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    S = len(offsets) - 1
    voxel = np.broadcast_to(np.asarray(voxel, dtype=f32), (S,))
    origin = None if origin is None else np.asarray(origin, dtype=f32).reshape(S, 3)
    out = {"label": np.zeros(len(points), np.int32), "size": np.zeros(len(points), np.int32),
           "keep": np.zeros(len(points), np.uint8), "kept": np.zeros(S, np.int32), "beyond": np.zeros(S, np.int32)}
    for s in range(S):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        r = voxel_scan(points[lo:hi], voxel[s], None if origin is None else origin[s], keep)
        for name in ("label", "size", "keep"):
            out[name][lo:hi] = r[name]
        out["kept"][s], out["beyond"][s] = r["kept"], r["beyond"]
    return out


BOUNDARY_VOXEL = 0.25


def boundary_rows():
    """A fixture of the suites, not of the law: (cloud (16,3) float32, want) at voxel 0.25 and no origin, want = the expected
    label, size, keep under "center", keep under "first", kept and beyond, all worked out by hand:
      rows 0-1    (0,0,0) and (-0.0,0,0): exact multiples, -0.0 / 0.25 = -0.0 and floor(-0.0) is cell 0; equal d2, row 0 wins
      rows 2-3    (-1e-30,0,0) and (-0.25,0,0): both in cell -1 (floor of -4e-30, and of exactly -1); dx = +0.125 (the 1e-30 is
                  rounded away) and -0.125: equal d2, row 2 wins
      row 4       (0.25,0.5,0.75): cell (1,2,3), alone
      rows 5-6    1.125 -+ 0.0625 on x about the centre 1.125 of cell 4: a mirrored pair, equal d2, the lower row wins
      rows 7-8    exact duplicates: the lower row wins
      row 9       x = 2^20 * 0.25: q = 2^20, beyond      row 10   x = -2^20 * 0.25: q = -2^20, inside and alone
      rows 11-12  NaN, +inf: absent                      row 13   x = 1e9: beyond
      rows 14-15  (2.01,)*3 and (2.12,)*3 in cell 8 (centre 2.125): "center" keeps row 15, "first" row 14"""
    big = float(GRID_HALF) * BOUNDARY_VOXEL
    cloud = np.array([[0, 0, 0], [-0.0, 0, 0], [-1e-30, 0, 0], [-0.25, 0, 0], [0.25, 0.5, 0.75], [1.0625, 1.125, 1.125],
                      [1.1875, 1.125, 1.125], [3.3, 3.3, 3.3], [3.3, 3.3, 3.3], [big, 0, 0], [-big, 0, 0], [np.nan, 0, 0],
                      [0.1, np.inf, 0], [1e9, 0, 0], [2.01, 2.01, 2.01], [2.12, 2.12, 2.12]], dtype=f32)
    want = {"label": np.array([0, 0, 2, 2, 4, 5, 5, 7, 7, -1, 10, -1, -1, -1, 14, 14], np.int32),
            "size": np.array([2, 2, 2, 2, 1, 2, 2, 2, 2, 0, 1, 0, 0, 0, 2, 2], np.int32),
            "center": np.array([1, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1], np.uint8),
            "first": np.array([1, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0], np.uint8), "kept": 7, "beyond": 2}
    return cloud, want


def box(cloud):
    """(center (3), scale) of a scan as datasets/real_data.py:26-33 on float32."""
    cloud = np.asarray(cloud, dtype=f32).reshape(-1, 3)
    mx, mn = cloud.max(axis=0), cloud.min(axis=0)
    center = (mx + mn) / f32(2)
    scale = (mx - mn).max() / f32(0.9)
    assert center.dtype == f32 and scale.dtype == f32
    return center, scale


def thin_to(cloud, max_points, origin=None, keep="center"):
    """(edge float32, the voxel_scan result at it) of the bisection; a scan of at most max_points rows is not thinned by the
    dataset and has no edge — that case is the caller's."""
    assert max_points >= 8
    cloud = np.ascontiguousarray(np.asarray(cloud, dtype=f32)).reshape(-1, 3)
    scale = box(cloud)[1]
    hi, lo = (f32(1) if scale == 0 else scale), f32(0)
    for _ in range(ROUNDS):
        mid = f32(f32(lo + hi) * f32(0.5))
        r = voxel_scan(cloud, mid, origin, keep)
        if r["kept"] <= max_points and r["beyond"] == 0:
            hi = mid
        else:
            lo = mid
    return hi, voxel_scan(cloud, hi, origin, keep)

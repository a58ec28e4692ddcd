"""The Euclidean-cluster law in numpy — the checker of csrc/clusters.hip, written from the law itself.

Everything is per scan (rows offsets[s] .. offsets[s+1] of points (T,3) float32); rows of other scans never take part.

    absent     a row with a non-finite coordinate (as in knn_law).
    d2(i, j)   knn_law.d2_block's formula: ((dx*dx + dy*dy) + dz*dz), one float32 rounding per operation; symmetric bit for
               bit, a NaN counts as +inf.
    r2         = float32(radius) * float32(radius), one float32 rounding; 0 <= radius and r2 finite are required.
    edge       {i, j} iff i != j, both rows present and d2(i, j) <= r2: inclusive (exact duplicates join at radius 0), and an
               overflowed +inf distance never joins.
    label[i]   the smallest row index within the scan of the connected component of i; -1 for an absent row.
    size[i]    the number of rows of that component; 0 for an absent row.
    clusters[s] the number of components;  largest[s] the label of the component with the most rows, equal sizes to the
               smaller label; -1 when no row is present.
    A scan longer than max_points gets the empty result: labels -1, sizes 0, clusters 0, largest -1.
The result is a function of the input alone.
"""
import numpy as np

from knn_law import d2_block

MAX_POINTS = 32768


def r2_of(radius):
    r = np.float32(radius)
    with np.errstate(over="ignore"):
        r2 = np.float32(r * r)
    assert r >= 0 and np.isfinite(r2), radius
    return r2


def cluster_scan(cloud, radius, block=1024):
    """(label (n) int32, size (n) int32, clusters, largest) of one scan."""
    cloud = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32)).reshape(-1, 3)
    n, r2 = len(cloud), r2_of(radius)
    label = np.full(n, -1, dtype=np.int32)
    size = np.zeros(n, dtype=np.int32)
    rows = np.flatnonzero(np.isfinite(cloud).all(axis=1))
    if len(rows) == 0:
        return label, size, 0, -1
    pts = cloud[rows]
    m = len(rows)
    comp = np.arange(m, dtype=np.int32)                         # the smallest member seen so far, by min-label propagation
    # +inf (an overflow, or a NaN) is never <= a finite r2; the diagonal (d2 = 0) only offers a row its own label
    near = [d2_block(pts[lo:lo + block], pts) <= r2 for lo in range(0, m, block)]
    while True:                                                 # every round: a row takes the smallest label among its neighbours',
        best = np.concatenate([np.where(blk, comp[None, :], np.int32(m)).min(axis=1) for blk in near])
        best = np.minimum(best, comp)                           # then jumps to its label's label; ends when nothing moves
        best = best[best]
        if np.array_equal(best, comp):
            break
        comp = best
    label[rows] = rows[comp]
    counts = np.bincount(comp, minlength=m)
    size[rows] = counts[comp]
    roots = np.flatnonzero(counts)
    top = roots[np.argmax(counts[roots])]                       # argmax: the first of equals, the smaller label
    return label, size, len(roots), int(rows[top])


def cluster_law(points, offsets, radius, max_points=MAX_POINTS):
    """(label (T) int32, size (T) int32, clusters (S) int32, largest (S) int32) over a ragged set."""
    points = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    assert 1 <= max_points <= MAX_POINTS
    S = len(offsets) - 1
    label = np.full(len(points), -1, dtype=np.int32)
    size = np.zeros(len(points), dtype=np.int32)
    clusters = np.zeros(S, dtype=np.int32)
    largest = np.full(S, -1, dtype=np.int32)
    r2_of(radius)
    for s in range(S):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        if hi - lo > max_points:
            continue
        label[lo:hi], size[lo:hi], clusters[s], largest[s] = cluster_scan(points[lo:hi], radius)
    return label, size, clusters, largest

"""CPU suite for tests/knn_law.py, the numpy checker of csrc/knn.hip: the neighbour law against an independent float64 brute
force where both are exact, and the outlier law on the recipe it was written for and at its edges."""
import numpy as np

import knn_law


def _brute_f64(cloud, k):
    """Independent statement: float64 distances, a stable argsort per row, self skipped."""
    c = cloud.astype(np.float64)
    n = len(c)
    index = np.full((n, k), -1, dtype=np.int64)
    dist2 = np.full((n, k), np.inf)
    for i in range(n):
        d = ((c - c[i]) ** 2).sum(axis=1)
        order = [j for j in np.argsort(d, kind="stable") if j != i][:k]
        index[i, :len(order)] = order
        dist2[i, :len(order)] = d[order]
    return index, dist2


def test_neighbours_equal_a_float64_brute_force_on_integer_lattices():
    r = np.random.RandomState(3)
    lengths = [1, 2, 5, 40, 300]                                # 300 points out of 17^3 = 4913 sites: many equal distances
    clouds = [r.randint(-8, 9, (n, 3)).astype(np.float32) for n in lengths]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    for k in (1, 7, 32):
        index, dist2 = knn_law.knn_law(np.concatenate(clouds), offsets, k)
        for s, cloud in enumerate(clouds):
            want_index, want_dist2 = _brute_f64(cloud, k)       # d2 <= 3 * 16^2: exact in both precisions
            got = slice(offsets[s], offsets[s + 1])
            assert np.array_equal(index[got], want_index), (k, s)
            assert np.array_equal(dist2[got].astype(np.float64), want_dist2), (k, s)
    full = knn_law.knn_law(np.concatenate(clouds), offsets, 32)
    part = knn_law.knn_law(np.concatenate(clouds), offsets, 9)
    assert np.array_equal(full[0][:, :9], part[0]) and np.array_equal(full[1][:, :9], part[1])     # a smaller k is a prefix


def test_absent_rows_cross_queries_and_overflow():
    cloud = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [3, 0, 0], [0, np.inf, 0], [1e30, 0, 0]], dtype=np.float32)
    index, dist2 = knn_law.knn_law(cloud, [0, 6], 4)
    assert index[2].tolist() == [-1] * 4 and index[4].tolist() == [-1] * 4 and np.isinf(dist2[[2, 4]]).all()
    assert index[0].tolist() == [1, 3, 5, -1] and dist2[0].tolist() == [1.0, 9.0, np.inf, np.inf]   # an overflow is a value
    assert index[5].tolist() == [0, 1, 3, -1] and np.isinf(dist2[5]).all()                           # ... ordered by row
    queries = np.array([[1, 0, 0], [np.nan, 1, 1], [2, 0, 0]], dtype=np.float32)
    index, dist2 = knn_law.knn_law(cloud, [0, 6], 2, queries, [0, 3])
    assert index.tolist() == [[1, 0], [-1, -1], [1, 3]] and dist2[0].tolist() == [0.0, 1.0] and dist2[2].tolist() == [1.0, 1.0]
    index, _ = knn_law.knn_law(cloud, [0, 6], 2, queries, [0, 3], exclude_self=True)
    assert index[0].tolist() == [1, 3] and index[2].tolist() == [1, 3]       # query 0 skips row 0; row 2 is absent anyway


def test_outlier_law_on_the_shell_with_strays():
    points, shell = knn_law.shell_with_strays(1024, seed=0)
    assert len(points) == 1030
    keep, mean, kept = knn_law.outliers_law(points, [0, len(points)], k=16, ratio=2.0)
    assert kept.tolist() == [1024] and keep.sum() == 1024
    assert np.array_equal(np.flatnonzero(keep), shell)          # every shell point stays, the strays and the NaN row go
    gone = np.setdiff1d(np.arange(len(points)), shell)
    assert np.isinf(mean[gone]).sum() == 1 and (mean[gone][np.isfinite(mean[gone])] > 1.0).all()
    finite = points[np.isfinite(points).all(axis=1)]
    side = lambda p: float((p.max(axis=0) - p.min(axis=0)).max())
    assert side(finite) == 9.0 and side(points[keep]) == 1.0    # the box the strays set, and the object's


def test_identical_points_are_all_kept():
    points = np.full((50, 3), 0.25, dtype=np.float32)
    keep, mean, kept = knn_law.outliers_law(points, [0, 50], k=16, ratio=0.0)
    assert keep.all() and kept.tolist() == [50] and (mean == 0).all()


def test_scans_of_one_and_two_points():
    points = np.array([[1, 2, 3], [0, 0, 0], [0, 3, 4]], dtype=np.float32)
    index, dist2 = knn_law.knn_law(points, [0, 1, 3], 2)
    assert index.tolist() == [[-1, -1], [1, -1], [0, -1]] and dist2[1:, 0].tolist() == [25.0, 25.0]
    keep, mean, kept = knn_law.outliers_law(points, [0, 1, 3], k=2, ratio=1.0)
    assert keep.tolist() == [False, True, True] and kept.tolist() == [0, 2]      # a lone point has no neighbour: absent
    assert np.isinf(mean[0]) and mean[1:].tolist() == [5.0, 5.0]


def test_threshold_cuts_between_equal_and_larger_means():
    """ratio = 0 keeps exactly the rows with q_i <= mu: on a line of unit steps with one gap the two rows at the gap go."""
    x = np.array([0, 1, 2, 3, 4, 5, 6, 16], dtype=np.float32)
    points = np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)
    keep, mean, kept = knn_law.outliers_law(points, [0, 8], k=1, ratio=0.0)
    assert mean.tolist() == [1.0] * 7 + [10.0] and keep.tolist() == [True] * 7 + [False] and kept.tolist() == [7]

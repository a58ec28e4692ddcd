"""CPU suite for tests/cluster_law.py, the checker of csrc/clusters.hip: against scipy's connected components of a graph built
by a float64 brute force, on integer lattices scaled by powers of two — there fp32 and fp64 distances are both exact, so the
two must agree on every label, size, count and `largest`."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import cluster_law


def _scipy(cloud, radius):
    """The law's four results of one scan from scipy: the graph in float64, components relabelled by smallest member."""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 3)
    n = len(cloud)
    label, size = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    rows = np.flatnonzero(np.isfinite(cloud).all(axis=1))
    if len(rows) == 0:
        return label, size, 0, -1
    p = cloud[rows].astype(np.float64)
    with np.errstate(over="ignore"):
        d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        d2[d2 > np.finfo(np.float32).max] = np.inf              # what overflows in fp32 joins nothing
    adj = d2 <= np.float64(cluster_law.r2_of(radius))          # the threshold is the law's: the fp32 product
    np.fill_diagonal(adj, False)
    count, comp = connected_components(csr_matrix(adj), directed=False)
    first = np.full(count, len(rows), dtype=np.int64)
    np.minimum.at(first, comp, np.arange(len(rows)))            # the smallest member of every component
    label[rows] = rows[first[comp]]
    sizes = np.bincount(comp, minlength=count)
    size[rows] = sizes[comp]
    order = np.lexsort((rows[first], -sizes))                   # most rows first, then the smaller label
    return label, size, count, int(rows[first[order[0]]])


def _agree(cloud, radius):
    got = cluster_law.cluster_scan(cloud, radius)
    want = _scipy(cloud, radius)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:], (got, want)
    return got


def _chain(n, step):
    c = np.zeros((n, 3), dtype=np.float32)
    c[:, 1] = np.arange(n, dtype=np.float32) * np.float32(step)
    return c


@pytest.mark.parametrize("step", [1.0, 0.125, 2.0 ** -10, 64.0])
def test_chain_at_the_radius_and_one_ulp_below(step):
    chain = _chain(97, step)
    label, size, clusters, largest = _agree(chain, step)        # inclusive: one component
    assert (label == 0).all() and (size == 97).all() and (clusters, largest) == (1, 0)
    below = np.nextafter(np.float32(step), np.float32(0))
    label, size, clusters, largest = _agree(chain, below)
    assert np.array_equal(label, np.arange(97)) and (size == 1).all() and (clusters, largest) == (97, 0)
    r = np.random.RandomState(3)
    for perm in (np.arange(97)[::-1], r.permutation(97)):      # the answer follows the numbering, not the geometry
        label, size, clusters, largest = _agree(chain[perm], step)
        assert (label == 0).all() and clusters == 1


def test_two_interleaved_lattices():
    g = np.arange(5, dtype=np.float32)
    a = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * np.float32(0.25)
    b = a + np.float32(64.0)
    both = np.empty((250, 3), dtype=np.float32)
    both[0::2], both[1::2] = a, b
    label, size, clusters, largest = _agree(both, 0.25)
    assert np.array_equal(label, np.arange(250) % 2) and (size == 125).all() and (clusters, largest) == (2, 0)
    _agree(both, 0.125)                                         # all singletons
    _agree(both, 0.375)                                         # the diagonals (0.3535..) join too: the same two
    label, _, clusters, _ = _agree(both, 128.0)                 # far enough to reach across
    assert clusters == 1 and (label == 0).all()


def test_duplicates_join_at_radius_zero():
    r = np.random.RandomState(1)
    base = r.randint(-8, 8, (12, 3)).astype(np.float32) * np.float32(0.5)
    base = np.unique(base, axis=0)
    cloud = base[r.randint(0, len(base), 80)]
    label, size, clusters, _ = _agree(cloud, 0.0)
    assert clusters == len(np.unique(cloud, axis=0))
    for i in range(80):
        same = np.flatnonzero((cloud == cloud[i]).all(axis=1))
        assert label[i] == same[0] and size[i] == len(same)


def test_non_finite_rows_are_absent():
    cloud = _chain(40, 1.0)
    cloud[3, 0] = np.nan
    cloud[10, 2] = np.inf
    cloud[11, 1] = -np.inf
    cloud[39] = np.nan
    label, size, clusters, largest = _agree(cloud, 1.0)
    assert (label[[3, 10, 11, 39]] == -1).all() and (size[[3, 10, 11, 39]] == 0).all()
    assert label[:3].tolist() == [0, 0, 0] and label[4:10].tolist() == [4] * 6 and label[12:39].tolist() == [12] * 27
    assert (clusters, largest) == (3, 12)
    gone = np.full((6, 3), np.nan, dtype=np.float32)
    assert _agree(gone, 1.0)[2:] == (0, -1)


def test_overflowing_distances_never_join():
    cloud = np.zeros((8, 3), dtype=np.float32)
    cloud[0::2, 0] = 1e30                                       # d2 between the two groups is +inf in fp32
    cloud[:, 1] = np.repeat(np.arange(4), 2)
    label, size, clusters, _ = _agree(cloud, 1.0)
    assert label.tolist() == [0, 1] * 4 and (size == 4).all() and clusters == 2
    label, _, clusters, _ = _agree(cloud, 1.5e19)               # r2 = 2.25e38 is finite, +inf is still beyond it
    assert clusters == 2
    with pytest.raises(AssertionError):
        cluster_law.r2_of(2e19)                                 # r2 overflows: refused
    with pytest.raises(AssertionError):
        cluster_law.r2_of(-1.0)
    with pytest.raises(AssertionError):
        cluster_law.r2_of(float("nan"))


def test_empty_and_single_row_scans_and_the_ragged_form():
    points = np.concatenate([_chain(5, 1.0), _chain(1, 1.0), _chain(7, 2.0)])
    offsets = [0, 5, 5, 6, 13]                                  # a chain, an empty scan, one row, a chain too sparse to join
    label, size, clusters, largest = cluster_law.cluster_law(points, offsets, 1.0)
    assert label.tolist() == [0] * 5 + [0] + list(range(7)) and size.tolist() == [5] * 5 + [1] + [1] * 7
    assert clusters.tolist() == [1, 0, 1, 7] and largest.tolist() == [0, -1, 0, 0]
    assert all(a.dtype == np.int32 for a in (label, size, clusters, largest))
    _agree(points[5:6], 1.0)
    _agree(points[:0], 1.0)
    # rows of other scans never take part: the same rows as one scan join across the old boundary
    assert cluster_law.cluster_law(points[:6], [0, 6], 1.0)[2].tolist() == [1]
    # a scan beyond max_points gets the empty result, the others are as without it
    label, size, clusters, largest = cluster_law.cluster_law(points, offsets, 1.0, max_points=5)
    assert label.tolist() == [0] * 5 + [0] + [-1] * 7 and size.tolist() == [5] * 5 + [1] + [0] * 7
    assert clusters.tolist() == [1, 0, 1, 0] and largest.tolist() == [0, -1, 0, -1]


def test_tied_sizes_go_to_the_smaller_label():
    cloud = np.zeros((9, 3), dtype=np.float32)
    cloud[:, 0] = [64, 0, 64, 0, 64, 0, 32, 32, 96]             # rows 0,2,4 / 1,3,5 / 6,7 / 8
    label, size, clusters, largest = _agree(cloud, 0.0)
    assert label.tolist() == [0, 1, 0, 1, 0, 1, 6, 6, 8] and size.tolist() == [3, 3, 3, 3, 3, 3, 2, 2, 1]
    assert (clusters, largest) == (4, 0)
    label, _, _, largest = _agree(cloud[::-1], 0.0)             # rows 8,6,4 <- 64 ... now 0 is the single, 1,2 the pair
    assert largest == 3 and label.tolist() == [0, 1, 1, 3, 4, 3, 4, 3, 4]


def test_random_lattice_clouds():
    r = np.random.RandomState(7)
    for n, scale, radius in ((300, 0.25, 0.5), (700, 2.0 ** -6, 2.0 ** -5), (1500, 1.0, 2.0), (1500, 1.0, 1.0)):
        cloud = r.randint(-12, 12, (n, 3)).astype(np.float32) * np.float32(scale)
        cloud[r.randint(0, n, 5)] = np.nan
        _agree(cloud, radius)

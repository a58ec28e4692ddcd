"""GPU suite for the nearest-neighbour kernel (csrc/knn.hip): index and dist2 bit for bit against tests/knn_law.py — every
instance and every boundary of k over a ragged set whose scan boundaries fall inside waves, chunks and tiles; isolation of
the scans; ties; absent rows and overflowed distances; scans shorter than k; cross-set queries; the cap; reuse and streams."""
import numpy as np
import pytest
import torch

import knn_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
KS = (1, 7, 8, 9, 16, 17, 32)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(CUDA) if dtype is None else torch.as_tensor(np.array(a), dtype=dtype, device=CUDA)


def _run(points, offsets, k, queries=None, query_offsets=None, **kw):
    from hyperpocket_amd import ops
    q = (None, None) if queries is None else (_dev(np.asarray(queries, np.float32)), _dev(query_offsets, torch.int64))
    index, dist2 = ops.knn_points(_dev(np.asarray(points, np.float32)), _dev(offsets, torch.int64), k, *q, **kw)
    return index.cpu().numpy(), dist2.cpu().numpy()


def _same(got, want, what):
    (gi, gd), (wi, wd) = got, want
    assert gi.shape == wi.shape and gd.shape == wd.shape and gi.dtype == np.int32 and gd.dtype == np.float32, what
    wrong = np.flatnonzero((gi != wi).any(axis=1))
    assert len(wrong) == 0, (what, "index", len(wrong), int(wrong[0]), gi[wrong[0]].tolist(), wi[wrong[0]].tolist())
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, "dist2")


def _check(points, offsets, k, queries=None, query_offsets=None, what=None, **kw):
    got = _run(points, offsets, k, queries, query_offsets, **kw)
    _same(got, knn_law.knn_law(points, offsets, k, queries, query_offsets, **kw), what)
    return got


def _tile():
    from hyperpocket_amd import ops
    plans = {k: ops.knn_points_plan(k) for k in range(1, 33)}
    assert {p[0] for p in plans.values()} == {8, 16, 32} and {plans[k][0] for k in KS} == {8, 16, 32}
    assert len({p[1:] for p in plans.values()}) == 1
    return plans[1][2]


@pytest.mark.parametrize("k", KS)
def test_sizes_and_instances(k):
    tile = _tile()
    points, offsets, lengths, lists = knn_law.ragged_mix(tile)
    assert {1, 2, 8, 9, 16, 17, 32, 33, 63, 64, 65, 255, 256, 257, 1000, tile - 1, tile, tile + 1, 4097} <= set(lengths)
    _same(_run(points, offsets, k), (lists[0][:, :k], lists[1][:, :k]), k)


def test_scans_are_isolated():
    r = np.random.RandomState(5)
    both = r.uniform(-1, 1, (600, 3)).astype(np.float32)
    a, b = both[0::2], both[1::2]                                  # two scans whose points interleave in space
    points, offsets = np.concatenate([a, b]), [0, 300, 600]
    index, dist2 = _check(points, offsets, 8, what="interleaved")
    alone = _run(a, [0, 300], 8), _run(b, [0, 300], 8)             # each scan alone gives the same rows
    _same((index[:300], dist2[:300]), alone[0], "scan 0 alone")
    _same((index[300:], dist2[300:]), alone[1], "scan 1 alone")
    assert index.min() >= 0 and index.max() < 300


def test_ties_go_to_the_lower_row():
    same = np.full((300, 3), 0.375, dtype=np.float32)
    index, dist2 = _check(same, [0, 300], 32, what="identical")
    assert (dist2 == 0).all()
    assert index[0].tolist() == list(range(1, 33)) and index[40].tolist() == list(range(32)) and index[7].tolist() == \
        [0, 1, 2, 3, 4, 5, 6] + list(range(8, 33))
    g = np.arange(7, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    for k in (7, 16, 32):
        _check(lattice, [0, 343], k, what=("lattice", k))
    _check(np.concatenate([lattice[::-1], same, lattice]), [0, 343, 643, 986], 17, what="lattice, identical, lattice")


def test_non_finite_rows_are_absent_and_overflow_is_a_value():
    r = np.random.RandomState(9)
    cloud = r.uniform(-1, 1, (700, 3)).astype(np.float32)
    bad = r.permutation(700)[:60]
    cloud[bad[:20], r.randint(0, 3, 20)] = np.nan
    cloud[bad[20:40], r.randint(0, 3, 20)] = np.inf
    cloud[bad[40:], r.randint(0, 3, 20)] = -np.inf
    index, dist2 = _check(cloud, [0, 700], 16, what="non-finite")
    assert (index[bad] == -1).all() and np.isinf(dist2[bad]).all()             # absent queries: the empty result
    assert not np.isin(index, bad).any()                                        # ... and nobody's neighbour
    huge = np.zeros((40, 3), dtype=np.float32)
    huge[::2, 0] = 1e30
    huge[1::4, 1] = -1e30
    huge[5] = (3e38, 3e38, 3e38)
    index, dist2 = _check(huge, [0, 40], 32, what="huge")
    assert (dist2[0, :19] == 0).all() and np.isinf(dist2[0, 19:]).all()        # +inf distances are candidates, in row order
    assert index[0, 19:].tolist() == list(range(1, 27, 2))
    everything_absent = np.full((70, 3), np.nan, dtype=np.float32)
    index, dist2 = _check(np.concatenate([everything_absent, cloud[:5]]), [0, 70, 75], 8, what="a scan of NaN")
    assert (index[:70] == -1).all()


def test_scans_shorter_than_k():
    r = np.random.RandomState(2)
    lengths = [1, 3, 8, 9, 1, 31, 32, 33, 2]
    points = r.uniform(-1, 1, (sum(lengths), 3)).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    for k in (8, 9, 32):
        index, dist2 = _check(points, offsets, k, what=("short", k))
        for s, n in enumerate(lengths):
            rows = slice(offsets[s], offsets[s + 1])
            assert (index[rows, min(n - 1, k):] == -1).all() and np.isinf(dist2[rows, min(n - 1, k):]).all()
            assert (index[rows, :min(n - 1, k)] >= 0).all()


def test_cross_set_queries():
    r = np.random.RandomState(4)
    lengths, asks = [300, 1, 70, 1100, 5], [17, 260, 0, 300, 64]    # a scan without queries, queries of a one-point scan
    points = r.uniform(-1, 1, (sum(lengths), 3)).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    queries = r.uniform(-1, 1, (sum(asks), 3)).astype(np.float32)
    qo = np.concatenate([[0], np.cumsum(asks)])
    queries[0:10] = points[5:15]                                     # queries that coincide with candidates
    queries[qo[3]:qo[3] + 50] = points[offsets[3] + 100:offsets[3] + 150]
    queries[3] = np.nan
    for k in (1, 9, 32):
        index, dist2 = _check(points, offsets, k, queries, qo, what=("cross", k))
        assert index[:3, 0].tolist() == [5, 6, 7] and (dist2[:3, 0] == 0).all() and index[3, 0] == -1
    _check(points, offsets, 8, queries, qo, exclude_self=True, what="cross, own row number skipped")


def test_the_cap():
    from hyperpocket_amd import HipExtensionError, ops
    n, k = ops.KNN_MAX_POINTS, 32
    assert n == 65536
    points = np.zeros((n, 3), dtype=np.float32)
    points[:, 0] = np.arange(n)
    index, dist2 = _run(points, [0, n], k)
    steps = np.array([s * t for t in range(1, k + 1) for s in (-1, 1)])         # i-1, i+1, i-2, i+2, ..: the lower row first
    cand = np.arange(n)[:, None] + steps[None, :]
    valid = (cand >= 0) & (cand < n)
    first = np.argsort(~valid, axis=1, kind="stable")[:, :k]                     # the first k that exist, order kept
    want = np.take_along_axis(cand, first, axis=1)
    assert np.take_along_axis(valid, first, axis=1).all()
    assert np.array_equal(index, want.astype(np.int32))
    assert np.array_equal(dist2, ((want - np.arange(n)[:, None]) ** 2).astype(np.float32))
    with pytest.raises(HipExtensionError):
        ops.knn_points(torch.zeros((n + 1, 3), device=CUDA), torch.tensor([0, n + 1], device=CUDA), k)
    with pytest.raises(HipExtensionError):
        ops.scan_outliers(torch.zeros((n + 1, 3), device=CUDA), torch.tensor([0, n + 1], device=CUDA))
    # a scan beyond the cap next to a short one is seen on the device only: its queries get the empty result
    two = torch.zeros((n + 11, 3), device=CUDA)
    two[:, 1] = torch.arange(n + 11, device=CUDA)
    index, dist2 = ops.knn_points(two, torch.tensor([0, n + 1, n + 11], device=CUDA), 4)
    assert bool((index[:n + 1] == -1).all()) and bool(torch.isinf(dist2[:n + 1]).all())
    assert index[n + 1].tolist() == [1, 2, 3, 4] and dist2[n + 1].tolist() == [1.0, 4.0, 9.0, 16.0]


def test_reuse_and_streams():
    from hyperpocket_amd import ops
    tile = _tile()
    points, offsets, _, lists = knn_law.ragged_mix(tile)
    p, o, k = _dev(points), _dev(offsets), 9
    want = lists[0][:, :k], lists[1][:, :k]
    out = {"index": torch.full((len(points), k), 123456, dtype=torch.int32, device=CUDA),
           "dist2": torch.full((len(points), k), float("nan"), device=CUDA)}
    index, dist2 = ops.knn_points(p, o, k, out=out)
    assert index.data_ptr() == out["index"].data_ptr() and dist2.data_ptr() == out["dist2"].data_ptr()
    _same((index.cpu().numpy(), dist2.cpu().numpy()), want, "poisoned out")
    ops.knn_points(p, o, k, out=out)
    _same((index.cpu().numpy(), dist2.cpu().numpy()), want, "second call")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        index2, dist22 = ops.knn_points(p, o, k)
    side.synchronize()
    _same((index2.cpu().numpy(), dist22.cpu().numpy()), want, "another stream")

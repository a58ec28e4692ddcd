"""GPU suite for the grid-backed nearest-neighbour search (csrc/knn_grid.hip): index and dist2 bit for bit against
tests/knn_law.py and against ops.knn_points — every instance and boundary of k over the ragged mix at several cell edges (the
grid output proves which cases ran on many cells), ties and rows on cell edges, absent rows and overflowed extents, scans
shorter than k, isolation, cross-set queries inside and outside the box, the lifted cap, reuse and streams."""
import numpy as np
import pytest
import torch

import knn_grid_law
import knn_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
KS = (1, 7, 8, 9, 16, 17, 32)
CELLS = (None, 2.0 ** -5, 0.25, 4.0)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(CUDA) if dtype is None else torch.as_tensor(np.array(a), dtype=dtype, device=CUDA)


def _run(points, offsets, k, queries=None, query_offsets=None, **kw):
    from hyperpocket_amd import ops
    q = (None, None) if queries is None else (_dev(np.asarray(queries, np.float32)), _dev(query_offsets, torch.int64))
    index, dist2 = ops.knn_points_grid(_dev(np.asarray(points, np.float32)), _dev(offsets, torch.int64), k, *q, **kw)
    return index.cpu().numpy(), dist2.cpu().numpy()


def _same(got, want, what):
    (gi, gd), (wi, wd) = got, want
    assert gi.shape == wi.shape and gd.shape == wd.shape and gi.dtype == np.int32 and gd.dtype == np.float32, what
    wrong = np.flatnonzero((gi != wi).any(axis=1))
    assert len(wrong) == 0, (what, "index", len(wrong), int(wrong[0]), gi[wrong[0]].tolist(), wi[wrong[0]].tolist())
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, "dist2")


def _check(points, offsets, k, queries=None, query_offsets=None, what=None, cells=(None,), **kw):
    want = knn_law.knn_law(points, offsets, k, queries, query_offsets, **kw)
    for cell in cells:
        got = _run(points, offsets, k, queries, query_offsets, cell=cell, **kw)
        _same(got, want, (what, cell))
    return got


def _mix():
    from hyperpocket_amd import ops
    plans = {k: ops.knn_grid_plan(k) for k in range(1, 33)}
    assert {p[0] for p in plans.values()} == {8, 16, 32} and {plans[k][0] for k in KS} == {8, 16, 32}
    assert len({p[1:] for p in plans.values()}) == 1
    return knn_law.ragged_mix(plans[1][2])


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("k", KS)
def test_sizes_instances_and_cell_edges(k, cell):
    from hyperpocket_amd import ops
    points, offsets, lengths, lists = _mix()
    S = len(lengths)
    out = {"index": torch.empty((len(points), k), dtype=torch.int32, device=CUDA),
           "dist2": torch.empty((len(points), k), dtype=torch.float32, device=CUDA),
           "grid": torch.full((S, 4), -1.0, device=CUDA)}
    index, dist2 = ops.knn_points_grid(_dev(points), _dev(offsets), k, cell=cell, out=out)
    _same((index.cpu().numpy(), dist2.cpu().numpy()), (lists[0][:, :k], lists[1][:, :k]), (k, cell))
    grid = out["grid"].cpu().numpy()
    G = grid[:, 1:]
    assert (grid[:, 0] > 0).all() and (G >= 1).all() and (G <= 1024).all() and (G == np.floor(G)).all()
    assert (G.prod(axis=1) <= 2 * np.array(lengths) + 64).all()                 # the budget that sizes the workspace
    if cell == 2.0 ** -5:                                                        # not a one-cell grid in disguise
        assert (G[np.array(lengths) >= 256] >= 8).all() and (np.array(lengths) >= 256).sum() >= 4
    if cell == 4.0:
        assert (G == 1).all() and (grid[:, 0] == 4.0).all()
    if cell == 0.25:
        assert (grid[np.array(lengths) >= 256, 0] == 0.25).all()                 # a request within the caps is taken as it is


def test_agreement_with_brute_force():
    from hyperpocket_amd import ops
    points, offsets, _, _ = _mix()
    p, o = _dev(points), _dev(offsets)
    for k in (7, 16, 32):
        a, b = ops.knn_points(p, o, k), ops.knn_points_grid(p, o, k)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), k


def _lattice(n=7, step=1.0):
    g = np.arange(n, dtype=np.float32) * np.float32(step)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_ties_and_rows_on_cell_edges():
    same = np.full((300, 3), 0.375, dtype=np.float32)
    index, dist2 = _check(same, [0, 300], 32, what="identical", cells=(None, 0.125))
    assert (dist2 == 0).all()
    assert index[0].tolist() == list(range(1, 33)) and index[40].tolist() == list(range(32))
    lattice = _lattice()                                                          # lo on a lattice point, spacing == h
    for k in (7, 16, 32):
        _check(lattice, [0, 343], k, what=("lattice", k), cells=(1.0, 0.5, None))
    _check(np.concatenate([lattice[::-1], same, lattice]), [0, 343, 643, 986], 17, what="lattice, identical, lattice", cells=(1.0,))
    r = np.random.RandomState(3)
    far = (1e6 + r.randint(0, 64, (700, 3)) * 0.0625).astype(np.float32)          # the fp32 ulp at 10^6 is 0.0625
    _check(far, [0, 700], 16, what="offset 1e6", cells=(0.25, 0.01, None))


def test_non_finite_rows_and_overflowed_extents():
    r = np.random.RandomState(9)
    cloud = r.uniform(-1, 1, (700, 3)).astype(np.float32)
    bad = r.permutation(700)[:60]
    cloud[bad[:20], r.randint(0, 3, 20)] = np.nan
    cloud[bad[20:40], r.randint(0, 3, 20)] = np.inf
    cloud[bad[40:], r.randint(0, 3, 20)] = -np.inf
    index, dist2 = _check(cloud, [0, 700], 16, what="non-finite", cells=(None, 0.2))
    assert (index[bad] == -1).all() and np.isinf(dist2[bad]).all()
    assert not np.isin(index, bad).any()
    huge = r.uniform(-1, 1, (500, 3)).astype(np.float32)
    huge[:6, 0] = (3e38, -3e38, 3e38, -3e38, 3e38, -3e38)                        # the x extent overflows: one cell along x
    from hyperpocket_amd import ops
    out = {"index": torch.empty((500, 32), dtype=torch.int32, device=CUDA), "dist2": torch.empty((500, 32), device=CUDA),
           "grid": torch.zeros((1, 4), device=CUDA)}
    got = ops.knn_points_grid(_dev(huge), _dev([0, 500], torch.int64), 32, cell=0.25, out=out)
    _same((got[0].cpu().numpy(), got[1].cpu().numpy()), knn_law.knn_law(huge, [0, 500], 32), "huge")
    g = out["grid"].cpu().numpy()[0]
    assert g[1] == 1 and g[2] >= 4 and g[3] >= 4
    everything_absent = np.full((70, 3), np.nan, dtype=np.float32)
    index, _ = _check(np.concatenate([everything_absent, cloud[:5]]), [0, 70, 75], 8, what="a scan of NaN")
    assert (index[:70] == -1).all()


def test_scans_shorter_than_k():
    r = np.random.RandomState(2)
    lengths = [1, 3, 8, 9, 1, 31, 32, 33, 2]
    points = r.uniform(-1, 1, (sum(lengths), 3)).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    for k in (8, 9, 32):
        index, dist2 = _check(points, offsets, k, what=("short", k), cells=(None, 0.3))
        for s, n in enumerate(lengths):
            rows = slice(offsets[s], offsets[s + 1])
            assert (index[rows, min(n - 1, k):] == -1).all() and np.isinf(dist2[rows, min(n - 1, k):]).all()
            assert (index[rows, :min(n - 1, k)] >= 0).all()


def test_scans_are_isolated():
    r = np.random.RandomState(5)
    both = r.uniform(-1, 1, (600, 3)).astype(np.float32)
    a, b = both[0::2], both[1::2]                                  # two scans whose points interleave in space
    points, offsets = np.concatenate([a, b]), [0, 300, 600]
    index, dist2 = _check(points, offsets, 8, what="interleaved", cells=(0.2,))
    alone = _run(a, [0, 300], 8, cell=0.2), _run(b, [0, 300], 8, cell=0.2)
    _same((index[:300], dist2[:300]), alone[0], "scan 0 alone")
    _same((index[300:], dist2[300:]), alone[1], "scan 1 alone")
    assert index.min() >= 0 and index.max() < 300


def test_cross_set_queries():
    from hyperpocket_amd import HipExtensionError, ops
    r = np.random.RandomState(4)
    lengths, asks = [300, 1, 70, 1100, 5], [17, 260, 0, 300, 64]    # a scan without queries, queries of a one-point scan
    points = r.uniform(-1, 1, (sum(lengths), 3)).astype(np.float32)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    queries = r.uniform(-1, 1, (sum(asks), 3)).astype(np.float32)
    qo = np.concatenate([[0], np.cumsum(asks)])
    queries[0:10] = points[5:15]                                     # queries that coincide with candidates
    queries[qo[3]:qo[3] + 50] = points[offsets[3] + 100:offsets[3] + 150]
    queries[qo[3] + 50:qo[3] + 120] += r.choice([-50.0, 50.0, 0.0], (70, 3)).astype(np.float32)   # far outside the box
    queries[qo[3] + 120] = (3e38, -3e38, 0)
    queries[3] = np.nan
    for k in (1, 9, 32):
        index, dist2 = _check(points, offsets, k, queries, qo, what=("cross", k), cells=(None, 0.15))
        assert index[:3, 0].tolist() == [5, 6, 7] and (dist2[:3, 0] == 0).all() and index[3, 0] == -1
    _check(points, offsets, 8, queries, qo, exclude_self=True, what="cross, own row number skipped", cells=(0.15,))
    _check(points, offsets, 8, queries, qo, exclude_self=False, what="cross, nothing skipped", cells=(0.15,))
    p, o = _dev(points), _dev(offsets)
    with pytest.raises(HipExtensionError):
        ops.knn_points_grid(p, o, 4, exclude_self=False)
    with pytest.raises(HipExtensionError):
        ops.knn_points_grid(p, o, 4, p, o, exclude_self=False)


def test_the_lifted_cap_on_a_line():
    n, k = 65537, 32
    points = np.zeros((n, 3), dtype=np.float32)
    points[:, 0] = np.arange(n)
    index, dist2 = _run(points, [0, n], k)
    steps = np.array([s * t for t in range(1, k + 1) for s in (-1, 1)])         # i-1, i+1, i-2, i+2, ..: the lower row first
    cand = np.arange(n)[:, None] + steps[None, :]
    valid = (cand >= 0) & (cand < n)
    first = np.argsort(~valid, axis=1, kind="stable")[:, :k]
    want = np.take_along_axis(cand, first, axis=1)
    assert np.take_along_axis(valid, first, axis=1).all()
    assert np.array_equal(index, want.astype(np.int32))
    assert np.array_equal(dist2, ((want - np.arange(n)[:, None]) ** 2).astype(np.float32))


def jittered_lattice(n=41, seed=21):
    """n^3 rows of a unit lattice, each moved by up to 0.2 per axis, shuffled: 68 921 rows for n = 41."""
    r = np.random.RandomState(seed)
    cloud = (_lattice(n) + r.uniform(-0.2, 0.2, (n ** 3, 3))).astype(np.float32)
    return cloud[r.permutation(len(cloud))]


def test_the_lifted_cap_on_a_jittered_lattice():
    from hyperpocket_amd import ops
    cloud = jittered_lattice()
    n, k = len(cloud), 32
    assert n == 68921 and n > ops.KNN_MAX_POINTS
    out = {"index": torch.empty((n, k), dtype=torch.int32, device=CUDA), "dist2": torch.empty((n, k), device=CUDA),
           "grid": torch.zeros((1, 4), device=CUDA)}
    index, dist2 = ops.knn_points_grid(_dev(cloud), _dev([0, n], torch.int64), k, out=out)
    rows = np.random.RandomState(1).permutation(n)[:512]
    _same((index[rows].cpu().numpy(), dist2[rows].cpu().numpy()), knn_grid_law.knn_rows(cloud, k, rows), "68921 rows")
    assert (out["grid"].cpu().numpy()[0, 1:] >= 8).all()
    assert bool((index >= 0).all()) and bool((index < n).all())


def test_a_scan_beyond_the_cap_is_a_value():
    from hyperpocket_amd import ops
    n = ops.KNN_GRID_MAX_POINTS + 1
    assert n == (1 << 22) + 1
    pts = torch.zeros((5 + n + 6, 3), device=CUDA)
    pts[:5, 1] = torch.arange(5, device=CUDA)
    pts[5 + n:, 2] = torch.arange(6, device=CUDA)
    offsets = torch.tensor([0, 5, 5 + n, 5 + n + 6], device=CUDA)
    index, dist2 = ops.knn_points_grid(pts, offsets, 1)
    assert bool((index[5:5 + n] == -1).all()) and bool(torch.isinf(dist2[5:5 + n]).all())
    assert index[:5, 0].tolist() == [1, 0, 1, 2, 3] and index[5 + n:, 0].tolist() == [1, 0, 1, 2, 3, 4]
    assert bool((dist2[:5] == 1).all()) and bool((dist2[5 + n:] == 1).all())


def test_reuse_and_streams():
    from hyperpocket_amd import HipExtensionError, ops
    points, offsets, lengths, lists = _mix()
    p, o, k = _dev(points), _dev(offsets), 9
    want = lists[0][:, :k], lists[1][:, :k]
    ws = ops.knn_grid_buffers(len(lengths), len(points), CUDA)
    ws.fill_(-1)                                                   # a workspace with anything in it
    out = {"index": torch.full((len(points), k), 123456, dtype=torch.int32, device=CUDA),
           "dist2": torch.full((len(points), k), float("nan"), device=CUDA)}
    index, dist2 = ops.knn_points_grid(p, o, k, out=out, ws=ws)
    assert index.data_ptr() == out["index"].data_ptr() and dist2.data_ptr() == out["dist2"].data_ptr()
    _same((index.cpu().numpy(), dist2.cpu().numpy()), want, "poisoned out and ws")
    ops.knn_points_grid(p, o, k, out=out, ws=ws)
    _same((index.cpu().numpy(), dist2.cpu().numpy()), want, "second call")
    with pytest.raises(HipExtensionError):                         # a workspace that is too small is refused on the host
        ops.knn_points_grid(p, o, k, ws=ws[:8])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        index2, dist22 = ops.knn_points_grid(p, o, k, cell=0.1)
    side.synchronize()
    _same((index2.cpu().numpy(), dist22.cpu().numpy()), want, "another stream")

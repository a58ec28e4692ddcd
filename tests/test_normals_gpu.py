"""GPU suite for the normal-estimation kernel (csrc/normals.hip): normal, curvature and count bit for bit against
tests/normals_law.py — every instance and the k in between over a ragged set whose scan boundaries fall inside waves and
chunks, with and without viewpoints; hand-made lists with empty, out-of-range, duplicate and self slots; absent rows and
overflowed differences; isolation of the scans; both ways of reading the lists; a scan beyond the neighbour search's cap;
reuse and streams."""
import functools

import numpy as np
import pytest
import torch

import knn_law
import normals_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
KS = (2, 8, 9, 16, 17, 32)


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(CUDA) if dtype is None else torch.as_tensor(np.array(a), dtype=dtype, device=CUDA)


def _run(points, offsets, k, index=None, viewpoints=None, **kw):
    from hyperpocket_amd import ops
    index = None if index is None else _dev(np.asarray(index, np.int32))
    viewpoints = None if viewpoints is None else _dev(np.asarray(viewpoints, np.float32))
    out = ops.scan_normals(_dev(np.asarray(points, np.float32)), _dev(offsets, torch.int64), k, viewpoints=viewpoints,
                           index=index, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want, what):
    (gn, gc, gm), (wn, wc, wm) = got, want
    assert gn.shape == wn.shape and gc.shape == wc.shape and gm.shape == wm.shape, what
    assert gn.dtype == np.float32 and gc.dtype == np.float32 and gm.dtype == np.int32, what
    wrong = np.flatnonzero(gm != wm)
    assert len(wrong) == 0, (what, "count", len(wrong), int(wrong[0]), int(gm[wrong[0]]), int(wm[wrong[0]]))
    wrong = np.flatnonzero((gn.view(np.uint32) != wn.view(np.uint32)).any(axis=1))     # integer views: NaN payloads count
    assert len(wrong) == 0, (what, "normal", len(wrong), int(wrong[0]), gn[wrong[0]].tolist(), wn[wrong[0]].tolist())
    wrong = np.flatnonzero(gc.view(np.uint32) != wc.view(np.uint32))
    assert len(wrong) == 0, (what, "curvature", len(wrong), int(wrong[0]), float(gc[wrong[0]]), float(wc[wrong[0]]))


def _mix():
    from hyperpocket_amd import ops
    return knn_law.ragged_mix(ops.knn_points_plan(1)[2])


@functools.lru_cache(maxsize=None)
def _viewpoints(S):
    v = np.random.RandomState(21).uniform(-2, 2, (S, 3)).astype(np.float32)
    v[::3] *= 0.1                                                   # some inside their scan: normals turn both ways
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _want(k, views):
    points, offsets, _, lists = _mix()
    return law.normals_law(points, offsets, lists[0][:, :k], _viewpoints(len(offsets) - 1) if views else None)


@pytest.mark.parametrize("views", [False, True])
@pytest.mark.parametrize("k", KS)
def test_sizes_and_instances(k, views):
    from hyperpocket_amd import ops
    assert {ops.scan_normals_plan(k)[0] for k in KS} == {8, 16, 32}
    points, offsets, lengths, lists = _mix()
    assert {1, 2, 8, 9, 16, 17, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4097} <= set(lengths)
    want = _want(k, views)
    v = _viewpoints(len(offsets) - 1) if views else None
    _same(_run(points, offsets, k, viewpoints=v), want, (k, views, "index=None"))      # through knn_points
    if k in (9, 16):
        _same(_run(points, offsets, k, index=lists[0][:, :k], viewpoints=v), want, (k, views, "given lists"))
    live = ~np.isnan(want[1])
    assert live.sum() > 9000 and (want[2][live] == np.minimum(np.repeat(lengths, lengths)[live], k + 1)).all()
    if views:                                                       # the viewpoint turned some normals and not others
        turned = (want[0][live] != _want(k, False)[0][live]).any(axis=1)
        assert 0 < turned.sum() < live.sum()


def test_one_viewpoint_serves_all_scans():
    points, offsets, _, lists = _mix()
    S, k = len(offsets) - 1, 8
    one = np.array([0.3, -2.0, 0.1], np.float32)
    want = law.normals_law(points, offsets, lists[0][:, :k], np.tile(one, (S, 1)))
    _same(_run(points, offsets, k, index=lists[0][:, :k], viewpoints=one), want, "(3,)")
    _same(_run(points, offsets, k, index=lists[0][:, :k], viewpoints=np.tile(one, (S, 1))), want, "(S,3)")


@pytest.mark.parametrize("k", [5, 12, 16, 32])
def test_hand_made_lists(k):
    """-1, out-of-range values on both sides, duplicates and the row itself; absent rows as neighbours and as row i."""
    lengths = [1, 2, 3, 40, 257, 1000, 7]
    r = np.random.RandomState(k)
    points = r.uniform(-1, 1, (sum(lengths), 3)).astype(np.float32)
    bad = r.permutation(len(points))[:90]
    points[bad[:30], r.randint(0, 3, 30)] = np.nan
    points[bad[30:60], r.randint(0, 3, 30)] = np.inf
    points[bad[60:], r.randint(0, 3, 30)] = -np.inf
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    index = law.hand_index(lengths, k, seed=k)
    assert (index == -1).any() and (index < -1).any() and (index > 1000).any()
    want = law.normals_law(points, offsets, index)
    _same(_run(points, offsets, k, index=index), want, ("hand-made", k))
    assert (want[2][bad] == 0).all() and np.isnan(want[0][bad]).all()
    assert (want[2] <= k + 1).all() and (want[2][offsets[4]:] < k + 1).any() and len(np.unique(want[2])) > 3


def test_lists_read_both_ways_agree():
    """Lists whose rows do not start on 16 bytes are read with scalar loads: the same bits."""
    from hyperpocket_amd import ops
    points, offsets, _, lists = _mix()
    k = 16
    p, o = _dev(points), _dev(offsets)
    flat = torch.full((len(points) * k + 1,), -1, dtype=torch.int32, device=CUDA)
    shifted = flat[1:].view(len(points), k)
    shifted.copy_(_dev(lists[0][:, :k]))
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    got = tuple(t.cpu().numpy() for t in ops.scan_normals(p, o, k, index=shifted))
    _same(got, _want(k, False), "unaligned lists")


def test_non_finite_rows_are_absent_and_overflow_is_undefined():
    r = np.random.RandomState(9)
    cloud = r.uniform(-1, 1, (700, 3)).astype(np.float32)
    bad = r.permutation(700)[:60]
    cloud[bad[:20], r.randint(0, 3, 20)] = np.nan
    cloud[bad[20:40], r.randint(0, 3, 20)] = np.inf
    cloud[bad[40:], r.randint(0, 3, 20)] = -np.inf
    huge = np.zeros((12, 3), dtype=np.float32)                      # shorter than k: every other row is a neighbour
    huge[::2, 0] = 3e38
    huge[1::2, 0] = -3e38
    huge[:, 1] = np.arange(12)
    same = np.full((20, 3), 0.375, dtype=np.float32)
    tiny = (r.uniform(-1, 1, (50, 3)) * 1e-42).astype(np.float32)   # subnormal differences: the frame's lowest exponent
    points = np.concatenate([cloud, huge, same, tiny, cloud[:2]])
    offsets = [0, 700, 712, 732, 782, 784]
    k = 16
    index = knn_law.knn_law(points, offsets, k)[0]
    want = law.normals_law(points, offsets, index)
    _same(_run(points, offsets, k), want, "non-finite")
    normal, curvature, count = want
    assert (count[bad] == 0).all() and np.isnan(normal[bad]).all()
    assert (count[700:712] == 12).all() and np.isnan(curvature[700:712]).all()          # every row has a neighbour 6e38 away
    assert (count[712:732] == 17).all() and np.isnan(curvature[712:732]).all()          # M == 0
    assert np.isfinite(normal[732:782]).all() and (count[782:] == 2).all() and np.isnan(normal[782:]).all()


def test_scans_are_isolated():
    """Two scans with identical contents at different offsets give identical results."""
    r = np.random.RandomState(5)
    a = r.uniform(-1, 1, (300, 3)).astype(np.float32)
    b = r.uniform(-1, 1, (77, 3)).astype(np.float32)
    points, offsets = np.concatenate([a, b, a]), [0, 300, 377, 677]
    views = np.array([[0, 0, 3], [1, 1, 1], [0, 0, 3]], np.float32)
    index = knn_law.knn_law(points, offsets, 9)[0]
    got = _run(points, offsets, 9, viewpoints=views)
    _same(got, law.normals_law(points, offsets, index, views), "three scans")
    _same(tuple(g[:300] for g in got), tuple(g[377:] for g in got), "the same scan twice")
    _same(tuple(g[:300] for g in got), _run(a, [0, 300], 9, viewpoints=views[:1]), "the scan alone")


def test_a_scan_beyond_the_cap_is_undefined_and_its_neighbours_untouched():
    from hyperpocket_amd import ops
    n = ops.KNN_MAX_POINTS + 1
    r = np.random.RandomState(3)
    before, after = r.uniform(-1, 1, (100, 3)).astype(np.float32), r.uniform(-1, 1, (33, 3)).astype(np.float32)
    big = np.zeros((n, 3), dtype=np.float32)
    big[:, 0] = np.arange(n)
    points, offsets = np.concatenate([before, big, after]), [0, 100, 100 + n, 133 + n]
    normal, curvature, count = _run(points, offsets, 8)
    assert (count[100:100 + n] == 1).all()
    assert (normal[100:100 + n].view(np.uint32) == 0x7FC00000).all() and (curvature[100:100 + n].view(np.uint32) == 0x7FC00000).all()
    for rows, cloud in ((slice(0, 100), before), (slice(100 + n, 133 + n), after)):
        want = law.normals_scan(cloud, knn_law.knn_scan(cloud, 8)[0])
        _same((normal[rows], curvature[rows], count[rows]), want, "a neighbour of the long scan")
    # with lists of its own the long scan is served: the cap is the neighbour search's
    index = np.full((len(points), 8), -1, dtype=np.int32)
    index[100:100 + n, 0] = np.maximum(np.arange(n) - 1, 1)
    index[100:100 + n, 1] = np.minimum(np.arange(n) + 1, n - 2)
    index[100:100 + n, 2] = (np.arange(n) * 7919) % n
    big[:, 1] = (np.arange(n) % 5) * 0.25
    points = np.concatenate([before, big, after])
    got = _run(points, offsets, 8, index=index)
    _same(got, law.normals_law(points, offsets, index), "own lists, a long scan")
    assert (got[2][100:100 + n] == 4).all() and np.isfinite(got[1][100:100 + n]).sum() > n - 10


def test_reuse_and_streams():
    from hyperpocket_amd import HipExtensionError, ops
    points, offsets, _, lists = _mix()
    p, o, k = _dev(points), _dev(offsets), 9
    want = _want(k, False)
    out = {"normal": torch.full((len(points), 3), 7.0, device=CUDA), "curvature": torch.full((len(points),), 7.0, device=CUDA),
           "count": torch.full((len(points),), 123456, dtype=torch.int32, device=CUDA)}
    res = ops.scan_normals(p, o, k, out=out)
    assert all(r.data_ptr() == out[name].data_ptr() for r, name in zip(res, ("normal", "curvature", "count")))
    _same(tuple(t.cpu().numpy() for t in res), want, "poisoned out")
    ops.scan_normals(p, o, k, out=out)
    _same(tuple(t.cpu().numpy() for t in res), want, "second call")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res2 = ops.scan_normals(p, o, k)
    side.synchronize()
    _same(tuple(t.cpu().numpy() for t in res2), want, "another stream")
    with pytest.raises(HipExtensionError):
        ops.scan_normals(p, o, k, out={**out, "count": out["count"][:-1]})
    with pytest.raises(HipExtensionError):                         # the lists' width is k
        ops.scan_normals(p, o, k, index=_dev(lists[0][:, :8]))
    with pytest.raises(HipExtensionError):
        ops.scan_normals(p, o, k, viewpoints=torch.zeros((2, 3), device=CUDA))
    empty = ops.scan_normals(torch.zeros((0, 3), device=CUDA), torch.zeros(2, dtype=torch.int64, device=CUDA), k)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0,), (0,)]

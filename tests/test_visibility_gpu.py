"""GPU suite for the visibility kernels (csrc/visibility.hip): label, winner and the whole workspace of ops.scan_visibility bit
for bit against tests/visibility_law.py — a sweep of resolutions and windows over scans of 0 to 1000 rows with viewpoints
outside, inside and on a coordinate plane of the data; ties and edges of the projection; ragged queries; a scan that crosses
workgroups and crowds its pixels; the largest face; repeatability and independence of the rows' order."""
import functools

import numpy as np
import pytest
import torch

import visibility_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32 = np.float32


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=CUDA)


def _run(points, offsets, views, R, w, margin=0.01, slope=2.0, queries=None, query_offsets=None):
    """ops.scan_visibility on fresh buffers -> numpy dict(label, winner?, buffer (S,6,R,R) uint64)."""
    from hyperpocket_amd import ops
    S = len(offsets) - 1
    p = _dev(np.asarray(points, f32).reshape(-1, 3))
    kw = {}
    if queries is not None:
        kw = dict(queries=_dev(np.asarray(queries, f32).reshape(-1, 3)), query_offsets=_dev(query_offsets, torch.int64))
    bufs = ops.scan_visibility_buffers(S, R, CUDA)
    res = ops.scan_visibility(p, _dev(offsets, torch.int64), _dev(np.asarray(views, f32)), resolution=R, window=w, margin=margin,
                              slope=slope, ws=bufs["ws"], **kw)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert bufs["ws"].numel() == S * 6 * R * R
    got["buffer"] = bufs["ws"].cpu().numpy().view(np.uint64).reshape(S, 6, R, R)
    return got


def _same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in want:
        g, w = got[name], np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        wrong = np.argwhere(g != w)
        assert len(wrong) == 0, (what, name, len(wrong), wrong[0].tolist(), g[tuple(wrong[0])], w[tuple(wrong[0])])


def _check(points, offsets, views, R, w, what=None, **kw):
    got = _run(points, offsets, views, R, w, **kw)
    _same(got, law.visibility_law(points, offsets, views, R, w, kw.get("margin", 0.01), kw.get("slope", 2.0), kw.get("queries"),
                                  kw.get("query_offsets")), what)
    return got


# ---- the sweep: S = 4 scans of 0, 1, 65 and 1000 rows in the box [0.25, 0.75]^3, coordinates on a 1/64 lattice so that rows
# ---- share pixels, depths and coordinate planes with a viewpoint on the lattice
LENGTHS = (0, 1, 65, 1000)
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)])
VIEWS = {"outside": [[2, 1.5, 3], [-1, 0.5, 0.5], [0.5, -2, 0.25], [3, 3, 3]],
         "inside": [[0.5, 0.5, 0.5]] * 4,
         "on a coordinate plane of the data": [[0.5, 2, 0.5], [2, 0.5, 0.5], [0.25, 0.25, 2], [0.75, 0.5, -1]]}


@functools.lru_cache(maxsize=None)
def _lattice():
    r = np.random.RandomState(7)
    return (r.randint(16, 49, (sum(LENGTHS), 3)) / 64.0).astype(f32)


@pytest.mark.parametrize("where", sorted(VIEWS))
@pytest.mark.parametrize("R", [4, 8, 33])
def test_parameter_sweep(R, where):
    for w in (0, 1, 2, 4):
        got = _check(_lattice(), OFFSETS, VIEWS[where], R, w, what=(R, w, where), margin=1 / 64, slope=1.0)
        assert set(np.unique(got["label"]).tolist()) <= {1, 2}
    if where == "inside":
        used = {f for f in range(6) if (got["buffer"][3, f] != law.EMPTY).any()}
        assert used == set(range(6))


def test_ties_and_edges():
    view = np.array([0.5, 0.25, -1.0], f32)
    cloud = np.array([[0.5, 0.25, -1.0],                                   # at the viewpoint
                      [np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 0, np.nan],    # absent
                      [1.5, 1.25, 0.0], [-0.5, -0.75, -2.0], [1.5, -0.75, 0.0],    # |dx| = |dy| = |dz|: the x axis, u, t = +-1 clamp
                      [1.5, 0.25, -1.0], [1.5, 0.25, -1.0], [1.5, 0.25, -1.0],     # duplicates: the lowest row wins
                      [0.5, 1.25, 0.0], [0.5, -0.75, 0.0], [1.5, 0.25, 0.0], [-0.5, 0.25, 0.0], [1.5, 1.25, -1.0],   # two equal
                      [0.5, 0.25, -1.0 + 2.0 ** -23], [0.5, 0.25 - 2.0 ** -25, -1.0],          # one ulp from the viewpoint
                      [2.5, 0.25, -1.0], [0.5, 0.25, 7.0]], f32)
    got = _check(cloud, [0, len(cloud)], [view], 8, 1, what="ties", margin=0.0, slope=0.0)
    assert got["label"][:4].tolist() == [1, 4, 4, 4] and got["winner"][:4].tolist() == [0, 0, 0, 0]
    assert got["winner"][7:10].tolist() == [1, 0, 0]
    for R, w in ((4, 0), (33, 4), (1024, 2)):
        _check(cloud, [0, len(cloud)], [view], R, w, what=("ties", R, w))
    # depths below the smallest normal fp32: the conversion rounds, it does not flush
    tiny = np.array([[1e-40, 0, 0], [2e-40, 1e-41, 0], [1e-45, 0, 0], [0, -1e-45, 0], [3e-39, 3e-39, 1e-39]], f32)
    got = _check(tiny, [0, len(tiny)], [[0, 0, 0]], 8, 1, what="denormal depths", margin=0.0, slope=0.0)
    assert (got["buffer"] != law.EMPTY).sum() >= 3 and (got["buffer"][got["buffer"] != law.EMPTY] >> np.uint64(32)).min() == 1
    # a non-finite viewpoint: the whole scan is absent, its neighbour is not
    both = np.concatenate([cloud, cloud])
    got = _check(both, [0, len(cloud), 2 * len(cloud)], [[np.nan, 0, 0], view], 8, 1, what="nan view")
    assert (got["label"][:len(cloud)] == 4).all() and (got["buffer"][0] == law.EMPTY).all()


def test_overflowing_depths_stay_ordered():
    cloud = np.array([[3e38, 0, 0], [3e38, 1e37, 0], [0, 0, 0], [3e38, 3.2e38, 0], [3e38, 3.2e38, 0], [-3e38, 3e38, 0]], f32)
    for slope in (0.0, 2.0):
        got = _check(cloud, [0, len(cloud)], [[-3e38, 0, 0]], 4, 0, what="overflow", margin=0.0, slope=slope)
    assert (got["buffer"] >> np.uint64(32) == 0x7F800000).sum() == 1       # +inf is a depth like any other


def test_queries():
    r = np.random.RandomState(11)
    points = r.uniform(-1, 1, (700, 3)).astype(f32)
    offsets = [0, 300, 300, 700]                                           # the scan in the middle has no rows
    views = np.array([[3, 0, 0], [0, 0, 0], [0.1, 0.2, -0.3]], f32)
    queries = r.uniform(-1.5, 1.5, (450, 3)).astype(f32)
    qoffsets = [0, 200, 250, 250]                                          # the last scan has no queries
    queries[10] = views[0]                                                 # a query at the viewpoint
    queries[20, 1] = np.nan
    queries[210] = [np.inf, 0, 0]
    queries = queries[:250]
    seen = set()
    for R, w in ((8, 1), (16, 0), (33, 4)):
        got = _check(points, offsets, views, R, w, what=("queries", R, w), queries=queries, query_offsets=qoffsets, margin=0.05)
        seen |= set(got["label"][:200].tolist())
    assert got["label"][10] == 1 and got["label"][20] == 4 and got["label"][210] == 4
    finite = np.isfinite(queries[200:250]).all(1)
    assert (got["label"][200:250][finite] == 3).all() and (got["buffer"][1] == law.EMPTY).all()
    assert "winner" not in got and seen == {0, 1, 2, 3, 4}
    # scans without any row: the kernel still answers the queries
    got = _check(np.zeros((0, 3), f32), [0, 0, 0, 0], views, 8, 1, what="no rows", queries=queries, query_offsets=qoffsets)
    assert sorted(set(got["label"].tolist())) == [1, 3, 4] and (got["label"] == 1).sum() == 1      # the query at the viewpoint


def test_launch_geometry():
    """One scan of 2^16 + 1 rows at R = 8: its rows cross wave and workgroup boundaries, and thousands contend for a pixel."""
    from hyperpocket_amd import ops
    n = (1 << 16) + 1
    threads, rows_per_lane, scatter, classify = ops.scan_visibility_plan(n)
    assert scatter > 1 and classify > 1 and scatter == -(-n // (threads * rows_per_lane))
    cloud = (np.random.RandomState(3).randint(-32, 33, (n, 3)) / 32.0).astype(f32)       # 65^3 lattice: equal depths abound
    got = _check(cloud, [0, n], [[0.25, 0.125, 2.5]], 8, 1, what="2^16 + 1 rows")
    crowd = np.bincount(law.project(cloud, [0.25, 0.125, 2.5], 8)[1], minlength=6 * 64)
    assert crowd.max() > 2000 and int(got["winner"].sum()) == int((got["buffer"] != law.EMPTY).sum())


def test_largest_face():
    cloud = np.random.RandomState(5).uniform(-1, 1, (1000, 3)).astype(f32)
    got = _check(cloud, [0, 1000], [[0.0, 0.0, 0.0]], 1024, 1, what="R = 1024")
    assert got["buffer"].nbytes == 6 * 1024 * 1024 * 8 and (got["buffer"] != law.EMPTY).sum() == got["winner"].sum()


def test_repeatability_and_row_order():
    r = np.random.RandomState(13)
    lengths = [500, 1, 1500]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    points = (r.randint(-40, 41, (2001, 3)) / 40.0).astype(f32)
    views = np.array([[2, 1, 0.5], [0, 0, 0], [0.0125, 0.0125, 0.0125]], f32)
    a = _run(points, offsets, views, 16, 2)
    b = _run(points, offsets, views, 16, 2)
    _same(a, b, "two runs")
    _same(a, law.visibility_law(points, offsets, views, 16, 2), "the law")
    flipped = np.concatenate([points[offsets[s]:offsets[s + 1]][::-1] for s in range(3)])
    back = np.concatenate([np.arange(offsets[s], offsets[s + 1])[::-1] for s in range(3)])
    c = _run(flipped, offsets, views, 16, 2)
    assert (c["buffer"] >> np.uint64(32) == a["buffer"] >> np.uint64(32)).all()           # the same depth in every pixel
    assert (c["label"][back] == a["label"]).all()
    assert c["winner"].sum() == a["winner"].sum()


def test_buffers_are_reused_and_the_rest_of_a_larger_workspace_is_left_alone():
    from hyperpocket_amd import ops
    cloud = _dev(law.shell(300))
    offsets = _dev([0, 100, 300], torch.int64)
    ws = torch.full((2 * 6 * 8 * 8 + 5,), 77, dtype=torch.int64, device=CUDA)
    out = {"label": torch.full((300,), 9, dtype=torch.uint8, device=CUDA)}
    res = ops.scan_visibility(cloud, offsets, (3.0, 0.0, 0.0), resolution=8, out=out, ws=ws)
    assert res is out and "winner" not in res and (ws[-5:] == 77).all()
    want = law.visibility_law(law.shell(300), [0, 100, 300], (3.0, 0.0, 0.0), 8)
    assert (res["label"].cpu().numpy() == want["label"]).all()
    assert (ws[:-5].cpu().numpy().view(np.uint64).reshape(2, 6, 8, 8) == want["buffer"]).all()

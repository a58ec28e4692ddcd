"""GPU suite for the voxel kernels (csrc/voxels.hip): every output of ops.scan_voxels bit for bit against tests/voxel_law.py — a
ragged mix whose scan lengths sit on the wave and workgroup-chunk edges at three voxels, both keep modes and every table
size (one slot per row with every row alone fills the table); many rows per cell; the boundary rows; origins; isolation of
the scans; the order of the rows; reuse of the buffers and streams; more rows than one sweep of the grid covers."""
import functools

import numpy as np
import pytest
import torch

import voxel_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
NAMES = ("label", "size", "keep", "kept", "beyond")
f32 = np.float32


def _dev(points, offsets):
    p = torch.from_numpy(np.array(points, dtype=f32).reshape(-1, 3)).to(CUDA)
    return p, torch.as_tensor(np.array(offsets), dtype=torch.int64, device=CUDA)


def _tensor(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(CUDA)


def _run(points, offsets, voxel, origin=None, **kw):
    from hyperpocket_amd import ops
    p, o = _dev(points, offsets)
    voxel = voxel if isinstance(voxel, float) else _tensor(voxel)
    return {k: v.cpu().numpy() for k, v in ops.scan_voxels(p, o, voxel, origin=_tensor(origin), **kw).items()}


def _same(got, want, what):
    assert set(got) == set(NAMES), what
    for name in NAMES:
        g, w = got[name], np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        wrong = np.argwhere(g != w)
        assert len(wrong) == 0, (what, name, len(wrong), wrong[0].tolist(), g[tuple(wrong[0])], w[tuple(wrong[0])])


def _check(points, offsets, voxel, origin=None, keep="center", what=None, **kw):
    got = _run(points, offsets, voxel, origin, keep=keep, **kw)
    _same(got, voxel_law.voxel_law(points, offsets, voxel, origin, keep), what)
    return got


def _chunk():
    from hyperpocket_amd import ops
    threads, rows = ops.scan_voxels_plan()
    return threads * rows


@functools.lru_cache(maxsize=None)
def _mix(chunk):
    """Scans of 0 .. 4097 rows on the wave and chunk edges (chunk = threads * rows_per_lane, the rows of a workgroup), in
    mixed order: each a union of 1-5 Gaussian blobs (sigma 0.05, centres in [-1, 1]^3) plus uniform strays in
    [-1.5, 1.5]^3.  Read-only."""
    lengths = sorted({0, 1, 2, 63, 64, 65, 255, 256, 257, 4097, chunk - 1, chunk, chunk + 1, 2 * chunk})
    r = np.random.RandomState(41)
    lengths = [lengths[i] for i in r.permutation(len(lengths))]
    clouds = []
    for n in lengths:
        blobs = r.randint(1, 6)
        centre = r.uniform(-1, 1, (blobs, 3))
        c = centre[r.randint(0, blobs, n)] + r.normal(0, 0.05, (n, 3))
        stray = r.rand(n) < 0.05
        c[stray] = r.uniform(-1.5, 1.5, (int(stray.sum()), 3))
        clouds.append(c.astype(f32))
    points = np.concatenate(clouds)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    points.setflags(write=False)
    offsets.setflags(write=False)
    return points, offsets, tuple(lengths)


@functools.lru_cache(maxsize=None)
def _mix_law(chunk, voxel, keep):
    points, offsets, _ = _mix(chunk)
    return voxel_law.voxel_law(points, offsets, voxel, None, keep)


MIX_VOXELS = (1e-5, 0.05, 8.0)         # every row alone / a few rows per cell / one cell per octant


def test_the_mix_walks_the_edges():
    chunk = _chunk()
    _, _, lengths = _mix(chunk)
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257, 4097, chunk - 1, chunk, chunk + 1, 2 * chunk} == set(lengths)
    assert lengths != tuple(sorted(lengths))


@pytest.mark.parametrize("slots_per_row", [1, 2, 4])
@pytest.mark.parametrize("keep", voxel_law.KEEPS)
@pytest.mark.parametrize("voxel", MIX_VOXELS)
def test_ragged_mix(voxel, keep, slots_per_row):
    chunk = _chunk()
    points, offsets, lengths = _mix(chunk)
    want = _mix_law(chunk, voxel, keep)
    _same(_run(points, offsets, voxel, keep=keep, slots_per_row=slots_per_row), want, (voxel, keep, slots_per_row))
    n = np.array(lengths)
    assert not want["beyond"].any()
    if voxel == MIX_VOXELS[0]:                                      # with one slot per row the table is full: every probe path
        assert np.array_equal(want["kept"], n) and want["keep"].all()
    if voxel == MIX_VOXELS[1]:
        big = n > 64
        assert ((want["kept"] > 8) & (want["kept"] < n))[big].all()
    if voxel == MIX_VOXELS[2]:
        assert (want["kept"][n > 0] >= 1).all() and (want["kept"] <= 8).all()


@pytest.mark.parametrize("keep", voxel_law.KEEPS)
def test_many_rows_per_cell(keep):
    """Contention on one slot: a scan in one cell, a scan whose neighbouring rows never share a cell (row i in cell i mod 7),
    a scan sorted by cell."""
    r = np.random.RandomState(8)
    one = r.uniform(0.1, 0.9, (4097, 3)).astype(f32)
    seven = r.uniform(0.05, 0.95, (4096, 3))
    seven[:, 0] += np.arange(4096) % 7
    seven = seven.astype(f32)
    sweep = r.uniform(-2, 2, (3000, 3)).astype(f32)
    _, inside, q, _ = voxel_law.cells(sweep, 1.0)
    assert inside.all()
    sweep = sweep[np.lexsort((q[:, 2], q[:, 1], q[:, 0]))]
    points = np.concatenate([one, seven, sweep])
    offsets = [0, 4097, 4097 + 4096, len(points)]
    for spr in (1, 4):
        got = _check(points, offsets, 1.0, keep=keep, slots_per_row=spr, what=(keep, spr))
    assert got["kept"].tolist()[:2] == [1, 7] and got["size"][0] == 4097 and got["kept"][2] <= 64
    assert set(got["size"][4097:4097 + 4096].tolist()) == {585, 586}


def test_boundary_rows_on_the_device():
    cloud, hand = voxel_law.boundary_rows()
    for keep in voxel_law.KEEPS:
        got = _check(cloud, [0, len(cloud)], voxel_law.BOUNDARY_VOXEL, keep=keep, what=keep)
        _same(got, {"label": hand["label"], "size": hand["size"], "keep": hand[keep], "kept": np.array([hand["kept"]], np.int32),
                    "beyond": np.array([hand["beyond"]], np.int32)}, ("by hand", keep))


def test_bad_voxels_per_scan_give_the_empty_result():
    cloud, hand = voxel_law.boundary_rows()
    n = len(cloud)
    points = np.concatenate([cloud] * 5)
    offsets = np.arange(6) * n
    voxel = np.array([voxel_law.BOUNDARY_VOXEL, np.nan, 0.0, -1.0, np.inf], dtype=f32)
    got = _check(points, offsets, voxel, what="bad voxels")
    assert got["kept"].tolist() == [hand["kept"], 0, 0, 0, 0] and got["beyond"].tolist() == [hand["beyond"], 0, 0, 0, 0]
    assert (got["label"][n:] == -1).all() and not got["size"][n:].any() and not got["keep"][n:].any()


def test_origin_moves_the_grid():
    r = np.random.RandomState(12)
    cloud = r.uniform(-0.5, 0.5, (3000, 3)).astype(f32)
    shift = np.array([[0.0, 0.0, 0.0], [0.013, -0.27, 3.1], [1e6, 1e6, 1e6]], dtype=f32)
    points = np.concatenate([cloud + s for s in shift]).astype(f32)
    offsets = np.arange(4) * len(cloud)
    for keep in voxel_law.KEEPS:
        anchored = _check(points, offsets, 0.01, origin=shift, keep=keep, what=("origin", keep))
        free = _check(points, offsets, 0.01, keep=keep, what=("no origin", keep))
        # an origin of zeros is a subtraction that changes nothing
        _same(_run(points, offsets, 0.01, origin=np.zeros((3, 3), f32), keep=keep), free, ("zero origin", keep))
    assert not anchored["beyond"].any() and (anchored["kept"] > 0).all()
    # a scan at +1e6 with extent 1 and voxel 0.01: every row is beyond the grid without an origin, none with its centre
    assert free["beyond"].tolist() == [0, 0, len(cloud)] and free["kept"][2] == 0


def test_scans_do_not_meet():
    r = np.random.RandomState(13)
    cloud = r.normal(0, 0.2, (1500, 3)).astype(f32)
    others = [r.normal(0, 0.2, (n, 3)).astype(f32) for n in (700, 1, 2000)]
    points = np.concatenate([cloud, others[0], others[1], cloud, others[2]])
    offsets = np.cumsum([0, 1500, 700, 1, 1500, 2000])
    alone = voxel_law.voxel_scan(cloud, 0.03)
    for spr in (1, 2):
        got = _check(points, offsets, 0.03, slots_per_row=spr, what=("isolation", spr))
        for s in (0, 3):
            lo, hi = offsets[s], offsets[s + 1]
            for name in ("label", "size", "keep"):
                assert np.array_equal(got[name][lo:hi], alone[name]), (s, name)
            assert got["kept"][s] == alone["kept"]


def test_the_kept_points_do_not_depend_on_the_order_of_the_rows():
    r = np.random.RandomState(14)
    cloud = r.uniform(-1, 1, (5000, 3)).astype(f32)                # continuous draws: no two rows of a cell at one distance
    perm = r.permutation(len(cloud))
    a = _check(cloud, [0, len(cloud)], 0.1, what="order")
    b = _check(cloud[perm], [0, len(cloud)], 0.1, what="permuted")
    rows = lambda c, res: sorted(map(bytes, c[res["keep"].astype(bool)]))
    assert a["kept"] == b["kept"] and rows(cloud, a) == rows(cloud[perm], b)


def test_buffers_and_streams_are_reusable():
    from hyperpocket_amd import ops
    r = np.random.RandomState(15)
    offsets = [0, 1000, 1000, 3500]
    first = r.normal(0, 0.3, (3500, 3)).astype(f32)
    second = r.uniform(-1, 1, (3500, 3)).astype(f32)
    second[5] = np.nan
    bufs = ops.scan_voxels_buffers(3, 3500, CUDA, slots_per_row=1)
    for stream in (None, torch.cuda.Stream()):
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            for cloud, voxel in ((first, 0.02), (second, 0.3), (first, 0.02)):
                p, o = _dev(cloud, offsets)
                res = ops.scan_voxels(p, o, voxel, slots_per_row=1, out=bufs, ws=bufs["ws"])
                assert all(res[name] is bufs[name] for name in NAMES)
                got = {name: res[name].cpu().numpy() for name in NAMES}
                _same(got, voxel_law.voxel_law(cloud, offsets, voxel), (voxel, stream is None))
    p, o = _dev(first, offsets)
    again = [{k: v.cpu().numpy() for k, v in ops.scan_voxels(p, o, 0.02).items()} for _ in range(2)]
    _same(again[0], again[1], "repeat")


def test_more_rows_than_one_sweep_of_the_grid():
    """Every workgroup strides to a second chunk: a scan longer than 2048 chunks, and a short scan behind it."""
    r = np.random.RandomState(16)
    n = 2048 * _chunk() + 1500
    assert n <= voxel_law.MAX_POINTS
    points = np.concatenate([r.normal(0, 0.4, (n, 3)), r.uniform(-1, 1, (300, 3))]).astype(f32)
    got = _check(points, [0, n, n + 300], 0.02, slots_per_row=1, what="long")
    assert 1000 < got["kept"][0] < n

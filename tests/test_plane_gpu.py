"""GPU suite for the plane kernels (csrc/plane.hip): every output of ops.scan_plane bit for bit against tests/plane_law.py — a
ragged mix whose scan lengths sit on the wave, workgroup-chunk and tile edges, at trial counts on the edges of the LDS tile
and three thresholds; the trial cap; isolation of the scans and their streams; absent rows, overflow and underflow;
min_inliers / min_share; reuse, streams and the length cap; ops.scan_plane_side against numpy."""
import functools

import numpy as np
import pytest
import torch

import plane_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
NAMES = ("trial", "inliers", "found", "sample", "sample_plane", "inlier", "moments", "shift")
f32 = np.float32


def _dev(points, offsets):
    p = torch.from_numpy(np.array(points, dtype=f32).reshape(-1, 3)).to(CUDA)
    return p, torch.as_tensor(np.array(offsets), dtype=torch.int64, device=CUDA)


def _run(points, offsets, threshold, streams=None, **kw):
    from hyperpocket_amd import ops
    p, o = _dev(points, offsets)
    if streams is not None:
        streams = torch.as_tensor(np.asarray(streams), dtype=torch.int64, device=CUDA)
    return {k: v.cpu().numpy() for k, v in ops.scan_plane(p, o, threshold, streams=streams, **kw).items()}


def _bits(a):
    return a.view(np.uint32) if a.dtype == f32 else a


def _same(got, want, what):
    assert set(got) == set(NAMES), what
    for name in NAMES:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        wrong = np.argwhere(_bits(g) != _bits(w))
        assert len(wrong) == 0, (what, name, len(wrong), wrong[0].tolist(), g[tuple(wrong[0])], w[tuple(wrong[0])])


def _check(points, offsets, threshold, what=None, **kw):
    got = _run(points, offsets, threshold, **kw)
    _same(got, plane_law.plane_law(points, offsets, threshold, **kw), what)
    return got


def _geometry():
    from hyperpocket_amd import ops
    threads, rows, tile = ops.scan_plane_plan()
    assert (threads, rows, tile) == ops.scan_plane_plan(1) == ops.scan_plane_plan(ops.PLANE_MAX_TRIALS)
    return threads, rows, tile


@functools.lru_cache(maxsize=None)
def _mix(chunk):
    """Scans of 0 .. 4097 rows on the wave and chunk edges (chunk = threads * rows_per_lane, the rows of a workgroup), in
    mixed order: each a planted plane (60 % of the rows within 0.004 of it) plus uniform clutter.  Read-only."""
    lengths = sorted({0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 4097})
    r = np.random.RandomState(31)
    lengths = [lengths[i] for i in r.permutation(len(lengths))]
    clouds, planted = zip(*[plane_law.planted_scan(r, n, normal=r.normal(size=3), d=r.uniform(-0.3, 0.3))[:2] for n in lengths])
    points, planted = np.concatenate(clouds), np.concatenate(planted)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    for a in (points, offsets, planted):
        a.setflags(write=False)
    return points, offsets, tuple(lengths), planted


@functools.lru_cache(maxsize=None)
def _mix_law(chunk, trials, threshold):
    points, offsets, _, _ = _mix(chunk)
    return plane_law.plane_law(points, offsets, threshold, trials=trials, seed=7)


MIX_THRESHOLDS = (0.0, 0.01, 10.0)     # exact hits only / the planted band / everything
TILE = 256                             # hypotheses per LDS tile: test_the_mix_walks_the_edges holds it against the plan
MIX_TRIALS = sorted({1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 512})


def test_the_mix_walks_the_edges():
    threads, rows, tile = _geometry()
    chunk = threads * rows
    _, _, lengths, _ = _mix(chunk)
    assert {0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 4097} == set(lengths)
    assert lengths != tuple(sorted(lengths)) and tile == TILE


@pytest.mark.parametrize("threshold", MIX_THRESHOLDS)
@pytest.mark.parametrize("trials", MIX_TRIALS)
def test_ragged_mix(trials, threshold):
    threads, rows, _ = _geometry()
    chunk = threads * rows
    points, offsets, lengths, planted = _mix(chunk)
    want = _mix_law(chunk, trials, threshold)
    _same(_run(points, offsets, threshold, trials=trials, seed=7), want, (trials, threshold))
    n = np.array(lengths)
    has = want["trial"] >= 0
    assert not has[n < 3].any()
    if trials == 512:                                               # the range the thresholds are meant to span
        assert has[n >= 3].all()
        if threshold == MIX_THRESHOLDS[0]:                          # the three sample rows or fewer
            assert ((want["inliers"] >= 1) & (want["inliers"] <= 3))[has].all()
        if threshold == MIX_THRESHOLDS[1]:                          # the planted rows, little else
            for s in np.flatnonzero(n >= 255):
                lo, hi = offsets[s], offsets[s + 1]
                mask = want["inlier"][lo:hi].astype(bool)
                assert (mask & planted[lo:hi]).sum() >= 0.9 * planted[lo:hi].sum() and mask.sum() <= 0.7 * n[s], (s, n[s])
        if threshold == MIX_THRESHOLDS[2]:                          # every present row
            assert np.array_equal(want["inliers"][has], n[has])


def test_the_trial_cap():
    from hyperpocket_amd import ops
    assert ops.PLANE_MAX_TRIALS == 4096 == plane_law.MAX_TRIALS
    r = np.random.RandomState(2)
    cloud = plane_law.planted_scan(r, 300)[0]
    got = _check(cloud, [0, 300], 0.01, what="4096 trials", trials=4096, seed=3)
    assert got["found"][0] == 1 and got["inliers"][0] >= 180
    _check(np.concatenate([cloud, cloud[:100]]), [0, 300, 400], 0.01, what="4096 trials, two scans", trials=4096, seed=3)


def test_scans_are_isolated_and_streams_decide():
    r = np.random.RandomState(5)
    cloud = plane_law.planted_scan(r, 700)[0]
    other = plane_law.planted_scan(r, 333, normal=(1, 0, 0.2))[0]
    points, offsets = np.concatenate([cloud, cloud]), [0, 700, 1400]       # identical coordinates, stored side by side
    got = _check(points, offsets, 0.01, what="twins", trials=64, seed=11)
    assert got["trial"][0] != got["trial"][1] and (got["sample"][0] != got["sample"][1]).any()     # stream = the scan's number
    same = _check(points, offsets, 0.01, what="twins, one stream", trials=64, seed=11, streams=[5, 5])
    for name in NAMES:
        a, b = (same[name][:700], same[name][700:]) if name == "inlier" else (same[name][0], same[name][1])
        assert np.array_equal(_bits(a), _bits(b)), name
    # a scan's result depends on its rows and its stream, not on its neighbours or its place
    scans, streams = [cloud, other, cloud[:0], cloud[:100]], [3, 1 << 40, 9, -2]
    first = _check(np.concatenate(scans), np.cumsum([0] + [len(c) for c in scans]), 0.01, what="order", trials=64, seed=11,
                   streams=streams)
    order = [3, 1, 0, 2]
    again = _check(np.concatenate([scans[i] for i in order]), np.cumsum([0] + [len(scans[i]) for i in order]), 0.01,
                   what="permuted", trials=64, seed=11, streams=[streams[i] for i in order])
    lo = np.cumsum([0] + [len(c) for c in scans])
    lo2 = np.cumsum([0] + [len(scans[i]) for i in order])
    for place, i in enumerate(order):
        for name in NAMES:
            if name == "inlier":
                a, b = first[name][lo[i]:lo[i + 1]], again[name][lo2[place]:lo2[place + 1]]
            else:
                a, b = first[name][i], again[name][place]
            assert np.array_equal(_bits(a), _bits(b)), (name, i)
    alone = _run(other, [0, 333], 0.01, trials=64, seed=11, streams=[1 << 40])
    assert alone["trial"][0] == first["trial"][1] and np.array_equal(alone["moments"][0], first["moments"][1])


def test_absent_rows_overflow_and_underflow():
    r = np.random.RandomState(9)
    cloud = plane_law.planted_scan(r, 1500)[0]
    bad = r.permutation(1500)[:240]
    cloud[bad[:80], r.randint(0, 3, 80)] = np.nan
    cloud[bad[80:160], r.randint(0, 3, 80)] = np.inf
    cloud[bad[160:], r.randint(0, 3, 80)] = -np.inf
    got = _check(cloud, [0, 1500], 0.01, what="non-finite rows", trials=128, seed=1)
    assert got["trial"][0] >= 0 and not got["inlier"][bad].any() and got["inliers"][0] > 400
    rows = plane_law.sample_rows(1, 0, 128, 1500)
    assert np.isin(rows, bad).any(axis=1).sum() >= 20               # absent rows were drawn as samples: those trials are invalid
    sick = cloud.copy()
    sick[np.unique(plane_law.sample_rows(1, 0, 4, 1500))] = np.nan  # every sample row of the only trials is absent
    got = _check(sick, [0, 1500], 0.01, what="absent samples", trials=4, seed=1)
    assert got["trial"][0] == -1 and not got["inlier"].any()
    huge = (plane_law.planted_scan(r, 600)[0] * f32(1e19)).astype(f32)      # nrm ~ 1e38 and beyond: len2 and e*e overflow
    _check(huge, [0, 600], 1e17, what="huge", trials=64)
    part = huge.copy()
    part[::2] = plane_law.planted_scan(r, 300)[0]                   # half of the rows near the origin: some trials stay finite
    got = _check(part, [0, 600], 0.01, what="huge and small", trials=256)
    assert got["trial"][0] >= 0
    tiny = (plane_law.planted_scan(r, 600)[0].astype(np.float64) * 2.0 ** -60).astype(f32)
    got = _check(np.concatenate([tiny, cloud[:50]]), [0, 600, 650], 0.01, what="tiny", trials=64)
    assert got["trial"][0] == -1 and not got["inlier"][:600].any() and got["trial"][1] >= 0       # len2 underflows to 0
    nothing = np.full((70, 3), np.nan, dtype=f32)
    got = _check(np.concatenate([nothing, cloud[:5]]), [0, 70, 75], 0.5, what="a scan of NaN", trials=32)
    assert got["trial"][0] == -1 and np.isnan(got["sample_plane"][0]).all()


def test_min_inliers_and_min_share():
    r = np.random.RandomState(4)
    cloud = plane_law.planted_scan(r, 512)[0]                       # 512 rows: count / 512 is an fp32 number, the test at equality
    count = int(plane_law.plane_scan(cloud, 0, 0, 128, 0.01)["inliers"])
    assert 290 <= count <= 360
    for kw, found in ((dict(min_inliers=count), 1), (dict(min_inliers=count + 1), 0),
                      (dict(min_share=count / 512), 1), (dict(min_share=(count + 0.5) / 512), 0),
                      (dict(min_share=(count - 0.5) / 512), 1), (dict(min_share=1.0), 0), (dict(min_share=0.0), 1),
                      (dict(min_inliers=count, min_share=(count + 0.5) / 512), 0)):
        got = _check(cloud, [0, 512], 0.01, what=kw, trials=128, **kw)
        assert got["found"].tolist() == [found] and got["inliers"].tolist() == [count], kw


def test_reuse_streams_and_the_length_cap():
    from hyperpocket_amd import HipExtensionError, ops
    threads, rows, tile = _geometry()
    points, offsets, _, _ = _mix(threads * rows)
    p, o = _dev(points, offsets)
    T, S = len(points), len(offsets) - 1
    out, ws = ops.scan_plane_buffers(S, T, 512, CUDA)
    for t in out.values():
        t.fill_(99)
    ws.fill_(-1)
    cpu = lambda d: {k: v.cpu().numpy() for k, v in d.items()}
    got = ops.scan_plane(p, o, MIX_THRESHOLDS[2], trials=512, seed=7, out=out, ws=ws)      # everything first ...
    assert all(got[name].data_ptr() == out[name].data_ptr() for name in NAMES)
    _same(cpu(got), _mix_law(threads * rows, 512, MIX_THRESHOLDS[2]), "poisoned out and ws")
    got = ops.scan_plane(p, o, MIX_THRESHOLDS[1], trials=512, seed=7, out=out, ws=ws)      # ... then the band: nothing is left over
    _same(cpu(got), _mix_law(threads * rows, 512, MIX_THRESHOLDS[1]), "second call, another threshold")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.scan_plane(p, o, MIX_THRESHOLDS[1], trials=512, seed=7)
    side.synchronize()
    _same(cpu(other), _mix_law(threads * rows, 512, MIX_THRESHOLDS[1]), "another stream")
    empty = ops.scan_plane(torch.zeros((0, 3), device=CUDA), torch.zeros(3, dtype=torch.int64, device=CUDA), 0.01, trials=8)
    _same(cpu(empty), plane_law.plane_law(np.zeros((0, 3)), [0, 0, 0], 0.01, trials=8), "T == 0")
    # the cap: known on the host when the rows cannot fit S scans, otherwise a value on the device
    cap = ops.SCAN_MAX_POINTS
    assert cap == plane_law.MAX_POINTS
    with pytest.raises(HipExtensionError, match="at most"):
        ops.scan_plane(torch.empty((cap + 1, 3), device=CUDA), torch.tensor([0, cap + 1], device=CUDA), 0.01, trials=8)
    long = torch.zeros((cap + 1 + 300, 3), device=CUDA)
    tail = plane_law.planted_scan(np.random.RandomState(1), 300)[0]
    long[cap + 1:] = torch.from_numpy(tail).to(CUDA)
    got = cpu(ops.scan_plane(long, torch.tensor([0, cap + 1, cap + 301], device=CUDA), 0.01, trials=8))
    want = plane_law.plane_scan(tail, 0, 1, 8, 0.01)
    assert got["trial"].tolist() == [-1, want["trial"]] and got["inliers"].tolist() == [0, want["inliers"]]
    assert not got["inlier"][:cap + 1].any() and np.array_equal(got["inlier"][cap + 1:], want["inlier"])
    assert np.array_equal(got["moments"][1], want["moments"]) and not got["moments"][0].any()


def test_scan_plane_side():
    from hyperpocket_amd import ops
    threads, rows, _ = _geometry()
    points, offsets, lengths, _ = _mix(threads * rows)
    points = points.copy()
    points[::37, 1] = np.nan
    points[5::91, 2] = np.inf
    p, o = _dev(points, offsets)
    S = len(lengths)
    res = ops.scan_plane(p, o, 0.01, trials=128, seed=7)
    anchor = p[(o[:-1] + res["sample"][:, 0].clamp(min=0)).clamp(max=len(points) - 1)]
    refit = ops.plane_from_moments(res["moments"], res["shift"], res["sample_plane"], anchor).astype(f32)
    assert np.isnan(refit[np.array(lengths) < 3]).all() and np.isfinite(refit[np.array(lengths) >= 255]).all()
    r = np.random.RandomState(3)
    arbitrary = r.normal(size=(S, 4)).astype(f32)
    arbitrary[2] = (0, 0, 0, 0)
    arbitrary[3] = (1e30, 1e30, 1e30, 0)
    out = None
    for what, planes, threshold in (("refit", refit, 0.01), ("arbitrary", arbitrary, 0.25), ("arbitrary, 0", arbitrary, 0.0)):
        want = plane_law.side_law(points, offsets, planes, threshold)
        got = ops.scan_plane_side(p, o, torch.from_numpy(planes).to(CUDA), threshold, out=out)
        out = dict(zip(("dist", "keep", "kept"), got))              # the next round reuses the buffers
        for name, g, w in zip(("dist", "keep", "kept"), got, want):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
            wrong = np.flatnonzero(_bits(g) != _bits(w))
            assert len(wrong) == 0, (what, name, len(wrong), int(wrong[0]), g[wrong[0]], w[wrong[0]])
    big = np.array(lengths) >= 255
    dist, keep, kept = plane_law.side_law(points, offsets, refit, 0.01)
    assert (kept[big] < 0.5 * np.array(lengths)[big]).all() and (kept[big] > 0).all()       # the refit drops the planted rows

"""GPU suite for csrc/pose_trials.hip: every output bit for bit against tests/pose_trials_law.py — trial counts about the draw's
round of 256 and at the cap, keep below, at and above the number of valid trials, sets with under three matches, with all
matches on one target row, collinear sets, empty and absent rows, edge_ratio 0 and 1, gates 0 and +inf, given streams, reuse,
and two runs giving the same bits."""
import functools

import numpy as np
import pytest
import torch

import align_law
import pose_trials_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32 = np.float32
NAMES = ("trial", "inliers", "found", "valid", "kept", "transform")


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(CUDA) if dtype is None else torch.as_tensor(np.array(a), dtype=dtype, device=CUDA)


@functools.lru_cache(maxsize=None)
def _sets():
    """(points, offsets, tpoints, toffsets, match): eight sets.
    0 a planted motion, 300 rows, 60 % true matches, the rest anywhere   1 two matches only   2 every match on target row 4
    3 rows on one line   4 1100 rows (beyond a chunk of 1024), a planted motion on a grid, an exact shift: equal sides
    5 no source rows   6 no target rows   7 40 rows, true matches, some rows and targets absent, matches out of range."""
    r = np.random.RandomState(17)
    R, t = align_law.rotation((1, 2, 3), np.radians(140.0)), np.array([0.3, -0.2, 0.5])
    src, dst, mat = [], [], []

    def planted(n, m, share):
        target = r.uniform(-1, 1, (m, 3)).astype(f32)
        rows = r.randint(0, m, n)
        source = ((target[rows].astype(np.float64) - t) @ R + 0.001 * r.normal(size=(n, 3))).astype(f32)
        return source, target, np.where(r.uniform(size=n) < share, rows, r.randint(0, m, n)).astype(np.int32)

    s, d, m = planted(300, 400, 0.6)
    src.append(s), dst.append(d), mat.append(m)
    s, d, m = planted(50, 60, 1.0)
    m[2:] = -1
    src.append(s), dst.append(d), mat.append(m)
    s, d, m = planted(50, 60, 1.0)
    src.append(s), dst.append(d), mat.append(np.full(50, 4, dtype=np.int32))
    line = np.outer(np.arange(64), [0.01, 0.02, -0.005]).astype(f32)
    src.append(line), dst.append(line.copy()), mat.append(np.arange(64, dtype=np.int32))
    grid = (r.randint(-1024, 1024, (1100, 3)) / 1024.0).astype(f32)
    m = np.arange(1100, dtype=np.int32)
    m[::3] = r.randint(0, 1100, len(m[::3]))
    src.append(grid), dst.append(grid + f32(2)), mat.append(m)
    src.append(np.zeros((0, 3), f32)), dst.append(d[:5]), mat.append(np.zeros(0, np.int32))
    src.append(s[:7]), dst.append(np.zeros((0, 3), f32)), mat.append(np.zeros(7, np.int32))
    s, d, m = planted(40, 40, 1.0)
    s[3], d[int(m[8]), 1] = np.nan, np.inf
    m[10], m[11], m[12] = 40, -5, 2 ** 31 - 1
    src.append(s), dst.append(d), mat.append(m)
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    out = np.concatenate(src), off(src), np.concatenate(dst), off(dst), np.concatenate(mat)
    for a in out:
        a.setflags(write=False)
    return out


def _run(sets, inlier_dist, out=None, ws=None, **kw):
    from hyperpocket_amd import ops
    points, offsets, tpoints, toffsets, match = sets
    if "streams" in kw and kw["streams"] is not None:
        kw["streams"] = _dev(np.asarray(kw["streams"], dtype=np.int64))
    res = ops.scan_pose_trials(_dev(points), _dev(offsets, torch.int64), _dev(tpoints), _dev(toffsets, torch.int64), _dev(match),
                               inlier_dist, out=out, ws=ws, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(got, want, what):
    for name in NAMES:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.dtype, w.dtype)
        if name == "transform":
            g, w = g.view(np.uint32), w.view(np.uint32)                # integer views: NaN payloads count
        assert np.array_equal(g, w), (what, name, g.tolist(), w.tolist())


@pytest.mark.parametrize("trials", [1, 255, 256, 257, 65536])
def test_trial_counts(trials):
    sets = _sets()
    kw = dict(trials=trials, keep=1024, seed=9, edge_ratio=0.9, min_inliers=6)
    want = law.pose_trials_law(*sets, 0.05, **kw)
    _same(_run(sets, 0.05, **kw), want, trials)
    if trials == 65536:                                                # the fixture holds what the suite is about
        assert want["found"].tolist() == [1, 0, 0, 0, 1, 0, 0, 1] and want["valid"][[1, 2, 3, 5, 6]].tolist() == [0] * 5
        assert want["valid"][0] > want["kept"][0] == 1024 and want["inliers"][0] > 100
        R, t = align_law.rotation((1, 2, 3), np.radians(140.0)), np.array([0.3, -0.2, 0.5])
        assert law.pose_error(want["transform"][0], R, t)[0] < 3.0
        assert np.isnan(want["transform"][[1, 2, 3, 5, 6]]).all()


def test_keep_below_at_and_above_the_valid_trials():
    sets = _sets()
    base = law.pose_trials_law(*sets, 0.05, trials=257, keep=4096, seed=2)
    V = int(base["valid"][0])
    assert 3 <= V < 257
    for keep in (1, V - 1, V, V + 1, 4096):
        want = law.pose_trials_law(*sets, 0.05, trials=257, keep=keep, seed=2)
        assert want["kept"][0] == min(V, keep) and want["valid"][0] == V
        _same(_run(sets, 0.05, trials=257, keep=keep, seed=2), want, keep)


@pytest.mark.parametrize("edge_ratio", [0.0, 1.0])
def test_edge_ratio_at_its_ends(edge_ratio):
    sets = _sets()
    want = law.pose_trials_law(*sets, 0.05, trials=2048, keep=512, seed=4, edge_ratio=edge_ratio)
    if edge_ratio == 1.0:                                              # only the exact shift has equal sides
        assert want["valid"][4] > 0 and want["valid"][0] == 0 and want["found"][4] == 1
    else:                                                              # every non-degenerate matched triple passes
        assert want["valid"][0] > 1000 and want["valid"][3] == 0
    _same(_run(sets, 0.05, trials=2048, keep=512, seed=4, edge_ratio=edge_ratio), want, edge_ratio)


@pytest.mark.parametrize("gate", [0.0, float("inf")])
def test_gates_zero_and_infinite(gate):
    sets = _sets()
    want = law.pose_trials_law(*sets, gate, trials=1024, keep=256, seed=6, min_inliers=0)
    if gate:
        points, offsets, tpoints, toffsets, match = sets                # every matched row: not the absent ones or those out of range
        mt, rows, tgt = match[int(offsets[7]):], points[int(offsets[7]):], tpoints[int(toffsets[7]):]
        inr = (mt >= 0) & (mt < 40)
        matched = inr & np.isfinite(rows).all(axis=1) & np.isfinite(tgt[np.where(inr, mt, 0)]).all(axis=1)
        assert want["inliers"][7] == matched.sum() == 34 and want["inliers"][4] == 1100
    _same(_run(sets, gate, trials=1024, keep=256, seed=6, min_inliers=0), want, gate)


def test_streams_reuse_and_two_runs():
    from hyperpocket_amd import ops
    sets = _sets()
    S = len(sets[1]) - 1
    streams = np.arange(S, dtype=np.int64)[::-1] * (2 ** 33 + 7) + 3
    kw = dict(trials=1000, keep=100, seed=2 ** 40 + 5)
    want = law.pose_trials_law(*sets, 0.05, streams=streams, **kw)
    plain = law.pose_trials_law(*sets, 0.05, **kw)
    assert want["trial"][0] != plain["trial"][0]
    _same(_run(sets, 0.05, streams=streams, **kw), want, "streams")
    out = {name: torch.full((S,) + tail, 77, dtype=dtype, device=CUDA) for name, dtype, tail in ops._POSE_OUT}
    ws = torch.full((S * 100 * 14 + 8,), -1, dtype=torch.int32, device=CUDA)
    first = _run(sets, 0.05, out=out, ws=ws, **kw)
    _same(first, plain, "poisoned out and ws")
    _same(_run(sets, 0.05, out=out, ws=ws, **kw), first, "a second run into the same buffers")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _run(sets, 0.05, **kw)
    _same(got, plain, "side stream")

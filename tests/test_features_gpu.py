"""GPU suite for csrc/features.hip: features, count, match and dist bit for bit against tests/feature_law.py — every list length
and instance over a ragged set whose boundaries fall inside waves and chunks, both ways of reading the lists, lists with empty,
out-of-range, duplicate and self slots, duplicated points, stacked points (d along the normal), absent rows and unusable
normals, sets without a descriptor, equal descriptors (the tie rule), every target length about the LDS tile, garbage offsets, a
set beyond the cap, reuse and streams."""
import functools

import numpy as np
import pytest
import torch

import feature_law as law
import knn_law
import normals_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
KS = (1, 4, 7, 8, 16, 31, 32)
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 513)
f32 = np.float32


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(CUDA) if dtype is None else torch.as_tensor(np.array(a), dtype=dtype, device=CUDA)


@functools.lru_cache(maxsize=None)
def _scans():
    """(points, offsets, normals, lists (T,32), hand (T,32)): nine scans of a bumpy sheet with their normals, then spoiled."""
    r = np.random.RandomState(11)
    clouds, normals, lists, hand = [], [], [], []
    for s, n in enumerate(LENGTHS):
        x, y = r.uniform(-1, 1, (2, n))
        cloud = np.stack([x, y, 0.3 * np.sin(2 * x + s) * np.cos(1.5 * y) + 0.003 * r.normal(size=n)], axis=1).astype(f32)
        if n == 64:                                                # a flat patch with a second storey right above it: d along the normal
            g = (np.arange(32) % 8) / 8.0, (np.arange(32) // 8) / 8.0
            cloud = np.concatenate([np.stack([g[0], g[1], np.zeros(32)], axis=1), np.stack([g[0], g[1], np.full(32, 0.05)], axis=1)]).astype(f32)
        if n >= 63:
            cloud[5], cloud[9] = cloud[4], cloud[4]                # duplicated points: d = 0
        index = knn_law.knn_scan(cloud, 32)[0] if n else np.zeros((0, 32), np.int32)
        nrm = normals_law.normals_scan(cloud, index[:, :16], f32([0, 0, 5]))[0] if n else np.zeros((0, 3), f32)
        if n == 64:
            nrm[:] = (0, 0, 1)
        if n >= 63:
            cloud[11, 0], cloud[12, 2], cloud[13, 1] = np.nan, np.inf, -np.inf
            nrm[20], nrm[21, 1], nrm[22, 0], nrm[23] = 0, np.nan, np.inf, (0, -0.0, 0)
            cloud[30] = 3e38
            cloud[31] = -3e38                                      # an overflowed difference
        clouds.append(cloud)
        normals.append(nrm)
        lists.append(index)
        if n:
            hand.append(normals_law.hand_index([n], 32, seed=3 + s))
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    out = np.concatenate(clouds), offsets, np.concatenate(normals), np.concatenate(lists), np.concatenate(hand)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _index(k):
    _, _, _, lists, hand = _scans()
    pick = np.random.RandomState(100 + k).randint(0, 4, (len(lists), k)) == 0
    return np.where(pick, hand[:, :k], lists[:, :k]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _want(k):
    points, offsets, normals, _, _ = _scans()
    return law.feature_law(points, offsets, normals, _index(k))


def _run(points, offsets, normals, index, **kw):
    from hyperpocket_amd import ops
    out = ops.scan_features(_dev(points), _dev(offsets, torch.int64), _dev(normals), _dev(index), **kw)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("features", "count")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        wrong = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert len(wrong) == 0, (what, name, len(wrong), int(wrong[0]), g[wrong[0]].tolist(), w[wrong[0]].tolist())


@pytest.mark.parametrize("k", KS)
def test_every_list_length_and_instance(k):
    from hyperpocket_amd import ops
    assert {ops.scan_features_plan(k)[0] for k in KS} == {8, 16, 32}
    points, offsets, normals, _, _ = _scans()
    want = _want(k)
    _same(_run(points, offsets, normals, _index(k)), want[:2], k)
    if k == 32:                                                    # the fixture holds what the suite is about
        count = want[1]
        assert (count > 0).sum() > 1000 and (count == 0).sum() > 20 and count.max() == 32
        assert not want[0][count == 0].any() and (want[0][count > 0][:, :33].reshape(-1, 3, 11).sum(axis=2) > 240).all()
        flat = slice(int(offsets[3]), int(offsets[4]))
        assert (count[flat] > 0).sum() > 40 and count[flat].max() < 32       # the storey above is listed and skipped


def test_both_ways_of_reading_the_lists():
    points, offsets, normals, _, _ = _scans()
    T = len(points)
    for k in (8, 16):
        base = torch.full((T * k + 1,), -1, dtype=torch.int32, device=CUDA)
        off = base[1:].view(T, k)                                  # 4 bytes off a 16-byte boundary: the scalar loads
        off.copy_(_dev(_index(k)))
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        from hyperpocket_amd import ops
        got = ops.scan_features(_dev(points), _dev(offsets, torch.int64), _dev(normals), off)
        _same(tuple(t.cpu().numpy() for t in got), _want(k)[:2], ("unaligned", k))


def test_out_is_reused_whole_and_streams_agree():
    from hyperpocket_amd import ops
    points, offsets, normals, _, _ = _scans()
    T = len(points)
    out = {"features": torch.full((T, 36), 0xAB, dtype=torch.uint8, device=CUDA),
           "count": torch.full((T,), -7, dtype=torch.int32, device=CUDA), "ws": torch.full((T * 36,), 0xCD, dtype=torch.uint8, device=CUDA)}
    args = _dev(points), _dev(offsets, torch.int64), _dev(normals)
    for k in (32, 7):                                              # the second call finds the first one's records in ws
        got = ops.scan_features(*args, _dev(_index(k)), out=out)
        assert got[0].data_ptr() == out["features"].data_ptr()
        _same(tuple(t.cpu().numpy() for t in got), _want(k)[:2], ("reuse", k))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.scan_features(*args, _dev(_index(16)))
    side.synchronize()
    _same(tuple(t.cpu().numpy() for t in got), _want(16)[:2], "side stream")


def test_rows_of_no_scan_have_no_descriptor():
    points, offsets, normals, _, _ = _scans()
    lo, hi = int(offsets[6]), int(offsets[8])                      # offsets that start late and end early
    sub = np.array([lo, int(offsets[7]), hi], dtype=np.int64)
    index = _index(16)
    got = _run(points, sub, normals, index)
    want = law.feature_law(points, sub, normals, index)
    _same(got, want[:2], "partial offsets")
    assert not got[1][:lo].any() and not got[1][hi:].any() and got[1][lo:hi].any()


@functools.lru_cache(maxsize=None)
def _descriptors():
    from hyperpocket_amd import ops
    tile = ops.scan_feature_match_plan()[2]
    tl = (1, 0, tile - 1, tile, tile + 1, 2 * tile + 1, 1, tile, 300)
    r = np.random.RandomState(5)

    def make(lengths):
        T = sum(lengths)
        feat = r.randint(0, 256, (T, 36)).astype(np.uint8)
        feat[:, 33:] = 0
        feat[r.randint(0, 3, T) == 0, :] //= 16                    # near descriptors: many close distances
        counts = np.where(r.randint(0, 6, T) == 0, 0, r.randint(1, 33, T)).astype(np.int32)
        return feat, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), counts

    feat, off, cnt = make(LENGTHS)
    tfeat, toff, tcnt = make(tl)
    for s in (3, 5, 8):                                            # equal descriptors in a target set: ties to the lower row
        lo, hi = int(toff[s]), int(toff[s + 1])
        tfeat[lo + 7:hi:5] = tfeat[lo + 2]
        tfeat[hi - 1] = tfeat[lo]
    feat[int(off[5]) + 3] = tfeat[int(toff[5]) + 2]                # an exact hit among equals
    cnt[int(off[5]) + 3] = tcnt[int(toff[5]) + 2] = 5
    feat[int(off[6]), :33], tfeat[int(toff[6])], cnt[int(off[6])], tcnt[int(toff[6])] = 255, 0, 1, 1      # the largest distance there is
    cnt[int(off[4]):int(off[5])] = 0                               # a source set without a descriptor
    tcnt[int(toff[7]):int(toff[8])] = 0                            # a target set without one
    return feat, off, cnt, tfeat, toff, tcnt, tl


def _match(feat, off, cnt, tfeat, toff, tcnt, **kw):
    from hyperpocket_amd import ops
    out = ops.scan_feature_match(_dev(feat), _dev(off, torch.int64), _dev(tfeat), _dev(toff, torch.int64), _dev(cnt), _dev(tcnt), **kw)
    return tuple(t.cpu().numpy() for t in out)


def _same_match(got, want, what):
    for g, w, name in zip(got, want, ("match", "dist")):
        assert g.shape == w.shape and g.dtype == np.int32 == w.dtype, (what, name)
        wrong = np.flatnonzero(g != w)
        assert len(wrong) == 0, (what, name, len(wrong), int(wrong[0]), int(g[wrong[0]]), int(w[wrong[0]]))


def test_match_every_length_about_the_tile():
    feat, off, cnt, tfeat, toff, tcnt, tl = _descriptors()
    want = law.match_law(feat, off, tfeat, toff, cnt, tcnt)
    _same_match(_match(feat, off, cnt, tfeat, toff, tcnt), want, "mix")
    match, dist = want
    assert (match >= 0).sum() > 800 and dist.max() == 33 * 255 * 255 and (dist[match >= 0] >= 0).all()
    assert (match[int(off[4]):int(off[5])] == -1).all() and (match[int(off[7]):int(off[8])] == -1).all()
    assert match[int(off[5]) + 3] == 2 and dist[int(off[5]) + 3] == 0          # rows 7, 12, .. of the set hold the same bytes
    # the real thing: a scan's own descriptors against another k's
    points, offsets, _, _, _ = _scans()
    a, b = law.feature_law(*_scans()[:3], _index(32))[:2], law.feature_law(*_scans()[:3], _index(16))[:2]
    _same_match(_match(a[0], offsets, a[1], b[0], offsets, b[1]), law.match_law(a[0], offsets, b[0], offsets, a[1], b[1]), "fpfh")


def test_match_out_is_reused_whole_and_streams_agree():
    feat, off, cnt, tfeat, toff, tcnt, _ = _descriptors()
    want = law.match_law(feat, off, tfeat, toff, cnt, tcnt)
    out = {"match": torch.full((len(feat),), 12345, dtype=torch.int32, device=CUDA),
           "dist": torch.full((len(feat),), -99, dtype=torch.int32, device=CUDA)}
    _same_match(_match(feat, off, cnt, tfeat, toff, tcnt, out=out), want, "poisoned out")
    _same_match(_match(feat, off, cnt, tfeat, toff, tcnt, out=out), want, "reused out")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _match(feat, off, cnt, tfeat, toff, tcnt)
    _same_match(got, want, "side stream")


def test_match_takes_garbage_offsets_and_a_set_beyond_the_cap_as_values():
    feat, off, cnt, tfeat, toff, tcnt, _ = _descriptors()
    bad = toff.copy()
    bad[-1] += 5                                                   # the last target set reaches beyond its tensor
    bad[3] = bad[2] - 1                                            # and one runs backwards
    _same_match(_match(feat, off, cnt, tfeat, bad, tcnt), law.match_law(feat, off, tfeat, bad, cnt, tcnt), "garbage offsets")
    n = law.MAX_POINTS + 1                                         # one row beyond the cap on the target side, then on the source side
    big = np.zeros((n, 36), dtype=np.uint8)
    big[:, 0] = np.arange(n) % 251
    ones = np.ones(n, dtype=np.int32)
    sets = np.array([0, 40, 80], dtype=np.int64), np.array([0, n, n + 40], dtype=np.int64)
    small, tall = np.concatenate([big[:40], big[100:140]]), np.concatenate([big, big[60:100]])
    want = law.match_law(small, sets[0], tall, sets[1], ones[:80], np.ones(n + 40, dtype=np.int32))
    assert (want[0][:40] == -1).all() and (want[0][40:] >= 0).all()
    _same_match(_match(small, sets[0], ones[:80], tall, sets[1], np.ones(n + 40, dtype=np.int32)), want, "target beyond the cap")
    want = law.match_law(tall, sets[1], small, sets[0], np.ones(n + 40, dtype=np.int32), ones[:80])
    assert (want[0][:n] == -1).all() and (want[0][n:] >= 0).all()
    _same_match(_match(tall, sets[1], np.ones(n + 40, dtype=np.int32), small, sets[0], ones[:80]), want, "source beyond the cap")

"""GPU suite for the registration kernel (csrc/align.hip): every output of ops.scan_align_step bit for bit against
tests/align_law.py — a ragged mix in which every source length on the wave and chunk edges meets every target length on the
LDS-tile edges, at hypothesis counts on the edges of the hypothesis group and three gates; ties, absent rows and overflow; the
edges of the integer frame; isolation of the sets; buffers, streams and the cap — and the chain on top of it: ops.scan_align
against align_law.align bit for bit, recovery of a planted motion, and the yaw search."""
import functools

import numpy as np
import pytest
import torch

import align_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32 = np.float32
INF = float("inf")
# |rigid_from_moments - fp64 Kabsch| on the planted fixture at seed 0, measured on the CPU (test_align_law_host.py asserts 4 x)
ROT_TOL, MOVE_TOL = 4 * 4.27e-7, 4 * 2.79e-7


def _t(a, dtype):
    return torch.as_tensor(np.array(a), dtype=dtype).to(CUDA)              # a copy: the fixtures are read-only


def _sets(points, offsets, tpoints, toffsets):
    return (_t(np.asarray(points, dtype=f32).reshape(-1, 3), torch.float32), _t(offsets, torch.int64),
            _t(np.asarray(tpoints, dtype=f32).reshape(-1, 3), torch.float32), _t(toffsets, torch.int64))


def _run(points, offsets, tpoints, toffsets, transforms, max_dist, anchor, shift, want_index=True, out=None):
    from hyperpocket_amd import ops
    S = len(offsets) - 1
    res = ops.scan_align_step(*_sets(points, offsets, tpoints, toffsets), _t(np.asarray(transforms, dtype=f32).reshape(S, -1, 12),
                              torch.float32), max_dist, _t(anchor, torch.float32), _t(shift, torch.int32), out=out,
                              want_index=want_index)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _bits(a):
    return a.view(np.uint32) if a.dtype == f32 else a


def _same(got, want, what, names=("moments", "index", "dist2")):
    assert set(got) == set(names), what
    for name in names:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        wrong = np.argwhere(_bits(g) != _bits(w))
        assert len(wrong) == 0, (what, name, len(wrong), wrong[0].tolist(), g[tuple(wrong[0])], w[tuple(wrong[0])])


def _check(points, offsets, tpoints, toffsets, transforms, max_dist, anchor=None, shift=None, what=None):
    if anchor is None:
        anchor, shift = align_law.frame(tpoints, toffsets, max_dist)
    want = align_law.step(points, offsets, tpoints, toffsets, transforms, max_dist, anchor, shift)
    _same(_run(points, offsets, tpoints, toffsets, transforms, max_dist, anchor, shift), want, what)
    return want


def _identity(S, H=1):
    return np.tile(np.eye(3, 4, dtype=f32).reshape(12), (S, H, 1))


def _motion(degrees, axis, t):
    return np.concatenate([align_law.rotation(axis, np.radians(degrees)), np.reshape(t, (3, 1))], axis=1).astype(f32).reshape(12)


def _geometry(H):
    from hyperpocket_amd import ops
    return ops.scan_align_plan(H)


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _mix(chunk, tile):
    """Every source length meets every target length, in mixed order; uniform rows in [-1, 1]^3.  Read-only."""
    src = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1]
    dst = [0, 1, tile - 1, tile, tile + 1, 2 * tile + 1]
    r = np.random.RandomState(17)
    pairs = [(n, m) for n in src for m in dst]
    pairs = [pairs[i] for i in r.permutation(len(pairs))]
    n, m = [p[0] for p in pairs], [p[1] for p in pairs]
    points, tpoints = r.uniform(-1, 1, (sum(n), 3)).astype(f32), r.uniform(-1, 1, (sum(m), 3)).astype(f32)
    for a in (points, tpoints):
        a.setflags(write=False)
    return points, _offsets(n), tpoints, _offsets(m), tuple(pairs)


@functools.lru_cache(maxsize=None)
def _mix_transforms(S, H):
    """Per job one of: the identity, a general motion (its own per job), a transform holding a NaN."""
    r = np.random.RandomState(5)
    out = _identity(S, H)
    for s in range(S):
        for h in range(H):
            kind = (s + h) % 3
            if kind == 1:
                out[s, h] = _motion(r.uniform(-180, 180), r.normal(size=3), r.uniform(-0.3, 0.3, 3))
            elif kind == 2:
                out[s, h, r.randint(12)] = np.nan
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _mix_match(chunk, tile, H):
    points, offsets, tpoints, toffsets, _ = _mix(chunk, tile)
    S = len(offsets) - 1
    anchor, shift = align_law.frame(tpoints, toffsets, INF)
    return align_law.step(points, offsets, tpoints, toffsets, _mix_transforms(S, H), INF, anchor, shift)


MIX_GATES = (0.0, 0.15, INF)           # exact hits only / a part of the rows / every matched row
GROUP = 4                              # hypotheses a lane serves when H > 1: test_the_mix_walks_the_edges holds it against the plan


def test_the_mix_walks_the_edges():
    from hyperpocket_amd import ops
    threads, rows, group, tile = _geometry(2)
    assert _geometry(ops.ALIGN_MAX_HYPOTHESES) == (threads, rows, group, tile) and _geometry(1)[::2] == (threads, 1)
    assert group == GROUP and ops.ALIGN_MAX_POINTS == align_law.MAX_POINTS and ops.ALIGN_MAX_HYPOTHESES == align_law.MAX_HYPOTHESES
    for H in (1, 2):                                                # the two instances have chunks of their own
        threads, rows, _, tile = _geometry(H)
        chunk = threads * rows
        pairs = _mix(chunk, tile)[4]
        assert {n for n, _ in pairs} == {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1}
        assert {m for _, m in pairs} == {0, 1, tile - 1, tile, tile + 1, 2 * tile + 1}
        assert len(set(pairs)) == 13 * 6 and list(pairs) != sorted(pairs)


@pytest.mark.parametrize("H", [1, 2, GROUP + 1, 64])
def test_ragged_mix(H):
    threads, rows, _, tile = _geometry(H)
    points, offsets, tpoints, toffsets, pairs = _mix(threads * rows, tile)
    S = len(pairs)
    transforms = _mix_transforms(S, H)
    match = _mix_match(threads * rows, tile, H)
    for gate in MIX_GATES:
        anchor, shift = align_law.frame(tpoints, toffsets, gate)
        want = align_law.step(points, offsets, tpoints, toffsets, transforms, gate, anchor, shift, match=match)
        _same(_run(points, offsets, tpoints, toffsets, transforms, gate, anchor, shift), want, (H, gate))
        used = want["moments"][:, :, 0]
        full = np.array([n if m else 0 for n, m in pairs])
        if gate == INF:                                             # every row of a job whose transform is finite
            finite = np.isfinite(transforms).all(axis=2)
            assert np.array_equal(used + want["moments"][:, :, 1], np.where(finite, full[:, None], 0))
            wide = np.array([m > 1 for _, m in pairs])              # a single target row has a box of no extent: all is clipped
            assert not want["moments"][wide, :, 1].any() and want["moments"][~wide, :, 1].any()
        elif gate == 0.0:
            assert not used.any()
        else:
            assert 0 < used.sum() < np.where(np.isfinite(transforms).all(axis=2), full[:, None], 0).sum()


def test_the_frame_of_the_mix():
    from hyperpocket_amd import ops
    threads, rows, _, tile = _geometry(1)
    _, _, tpoints, toffsets, _ = _mix(threads * rows, tile)
    for gate in MIX_GATES + (1e-3, 7.0):
        anchor, shift = ops.align_frame(_t(tpoints, torch.float32), _t(toffsets, torch.int64), gate)
        want = align_law.frame(tpoints, toffsets, gate)
        assert np.array_equal(anchor.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), gate
        assert np.array_equal(shift.cpu().numpy(), want[1]) and shift.dtype == torch.int32, gate


def test_ties_go_to_the_lower_row():
    r = np.random.RandomState(3)
    base = r.uniform(-1, 1, (300, 3)).astype(f32)
    target = np.concatenate([base, base[::-1], base[:50]])          # every row two or three times
    want = _check(base, [0, 300], target, [0, len(target)], _identity(1), INF, what="duplicates")
    assert np.array_equal(want["index"][0], np.minimum(np.arange(300), 599 - np.arange(300)))
    assert not want["dist2"].any() and want["moments"][0, 0, 17] == 0 and want["moments"][0, 0, 0] == 300
    _check(base, [0, 300], target, [0, len(target)], _identity(1), 0.0, what="duplicates at gate 0")
    lattice = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    _check(lattice + f32(0.5), [0, 512], lattice, [0, 512], _identity(1), INF, what="a cell centre has eight nearest rows")


def test_absent_rows_and_overflow():
    r = np.random.RandomState(4)
    src, dst = r.uniform(-1, 1, (400, 3)).astype(f32), r.uniform(-1, 1, (700, 3)).astype(f32)
    for a, rows in ((src, r.permutation(400)[:60]), (dst, r.permutation(700)[:90])):
        a[rows, r.randint(0, 3, len(rows))] = r.choice([np.nan, np.inf, -np.inf], len(rows))
    anchor, shift = np.zeros((1, 3), f32), np.array([1], np.int32)
    transforms = np.stack([_identity(1)[0, 0], _motion(40, (1, 2, 3), (0.1, 0.2, -0.1))])[None]
    want = _check(src, [0, 400], dst, [0, 700], transforms, INF, anchor, shift, "absent rows")
    absent = ~np.isfinite(src).all(axis=1)
    assert (want["index"][:, absent] == -1).all() and np.isinf(want["dist2"][:, absent]).all()
    assert np.isfinite(dst[want["index"][:, ~absent]]).all() and (want["moments"][0, :, 0] == (~absent).sum()).all()
    allnan = np.full((5, 3), np.nan, f32)
    _check(src, [0, 400], allnan, [0, 5], transforms, INF, anchor, shift, "no candidate at all")
    big = src.copy()
    big[::2] = np.where(big[::2] < 0, f32(-2e19), f32(2e19))         # coordinates of 10^19: d2 overflows to +inf, no match
    want = _check(big, [0, 400], dst, [0, 700], transforms[:, :1], INF, anchor, shift, "overflow")
    assert (want["index"][0, 0::2] == -1).all()
    far = dst.copy()
    far[np.isfinite(far).all(axis=1)] *= f32(4e19)
    _check(src, [0, 400], far, [0, 700], transforms, INF, anchor, shift, "overflowing targets")
    moved = np.tile(_motion(10, (0, 0, 1), (3e38, 0, 0)), (1, 1, 1))    # p' overflows for x > 0
    _check(src * f32(4), [0, 400], dst, [0, 700], moved, INF, anchor, shift, "an overflowing transform")


def test_frame_edges():
    r = np.random.RandomState(6)
    dst = r.uniform(-1, 1, (500, 3)).astype(f32)
    src = r.uniform(-1, 1, (300, 3)).astype(f32)
    src[:40] += f32(9)                                              # far outside the targets' box
    anchor, shift = align_law.frame(dst, [0, 500], 0.0)             # gate 0: the tightest frame, clipping at 2^(shift + 1)
    assert shift[0] == 0
    want = _check(src, [0, 300], dst, [0, 500], _identity(1), INF, anchor, shift, "rows outside the frame")
    assert want["moments"][0, 0, 1] == 40 and want["moments"][0, 0, 0] == 260
    inside = align_law.step(src[40:], [0, 260], dst, [0, 500], _identity(1), INF, anchor, shift)
    assert np.array_equal(inside["moments"][0, 0, 2:], want["moments"][0, 0, 2:])     # counted, and in no sum
    edge = np.array([[2, 0, 0], [np.nextafter(f32(2), f32(0)), 0, 0], [-2, 0, 0]], f32)   # exactly at the bound, and just inside
    _check(edge, [0, 3], edge, [0, 3], _identity(1), INF, np.zeros((1, 3), f32), np.array([0], np.int32), "the bound itself")
    tiny = f32(2.0 ** -60)
    want = _check(src * tiny, [0, 300], dst * tiny, [0, 500], _identity(1), INF, what="scaled by 2^-60")
    assert align_law.frame(dst * tiny, [0, 500], INF)[1][0] == align_law.frame(dst, [0, 500], INF)[1][0] - 60
    assert want["moments"][0, 0, 0] == 260 and want["moments"][0, 0, 1] == 40     # the frame follows the scale
    for s in (-100, 128, 140, -140):                                # the frame's own range, and shifts beyond it
        _check(src, [0, 300], dst, [0, 500], _identity(1), INF, np.zeros((1, 3), f32), np.array([s], np.int32), ("shift", s))
    _check(src, [0, 300], dst, [0, 500], _identity(1), INF, np.full((1, 3), np.nan, f32), np.array([1], np.int32), "a NaN anchor")


def test_sets_are_isolated():
    r = np.random.RandomState(8)
    n, m = [130, 70, 130, 513, 1], [300, 20, 300, 90, 600]
    clouds = [r.uniform(-1, 1, (k, 3)).astype(f32) for k in n]
    targets = [r.uniform(-1, 1, (k, 3)).astype(f32) for k in m]
    clouds[2], targets[2] = clouds[0], targets[0]                   # twins
    transforms = np.stack([np.stack([_motion(r.uniform(-30, 30), r.normal(size=3), r.uniform(-0.1, 0.1, 3)) for _ in range(3)])
                           for _ in n])
    transforms[2] = transforms[0]
    pack = lambda order: (np.concatenate([clouds[i] for i in order]), _offsets([n[i] for i in order]),
                          np.concatenate([targets[i] for i in order]), _offsets([m[i] for i in order]), transforms[list(order)])
    base = _check(*pack(range(5)), 0.3, what="in order")
    assert np.array_equal(base["moments"][0], base["moments"][2]) and base["moments"][0, :, 0].all()
    assert np.array_equal(base["index"][:, :130], base["index"][:, 200:330])
    order = [3, 0, 4, 2, 1]
    moved = _check(*pack(order), 0.3, what="permuted")
    assert np.array_equal(moved["moments"], base["moments"][order])
    starts, at = _offsets(n), 0
    for i in order:
        assert np.array_equal(moved["index"][:, at:at + n[i]], base["index"][:, starts[i]:starts[i] + n[i]])
        at += n[i]


def test_buffers_streams_and_the_cap():
    from hyperpocket_amd import ops
    r = np.random.RandomState(9)
    src, dst = r.uniform(-1, 1, (700, 3)).astype(f32), r.uniform(-1, 1, (900, 3)).astype(f32)
    offsets, toffsets = [0, 300, 700], [0, 500, 900]
    transforms = np.stack([np.stack([_motion(5 * h + s, (1, 1, 0), (0.01 * h, 0, 0)) for h in range(6)]) for s in range(2)])
    anchor, shift = align_law.frame(dst, toffsets, 0.2)
    want = align_law.step(src, offsets, dst, toffsets, transforms, 0.2, anchor, shift)
    dev = _sets(src, offsets, dst, toffsets) + (_t(transforms, torch.float32),)
    frame = (_t(anchor, torch.float32), _t(shift, torch.int32))
    out = {"moments": torch.full((2, 6, 18), -7, dtype=torch.int64, device=CUDA),
           "index": torch.full((6, 700), -7, dtype=torch.int32, device=CUDA),
           "dist2": torch.full((6, 700), float("nan"), device=CUDA)}
    res = ops.scan_align_step(*dev, 0.2, *frame, out=out, want_index=True)
    assert res["moments"] is out["moments"] and res["index"] is out["index"]
    _same({k: v.cpu().numpy() for k, v in res.items()}, want, "poisoned buffers")
    res = ops.scan_align_step(*dev, 0.2, *frame, out=out, want_index=True)      # ... and again over its own results
    _same({k: v.cpu().numpy() for k, v in res.items()}, want, "reused buffers")
    bare = ops.scan_align_step(*dev, 0.2, *frame)
    assert set(bare) == {"moments"} and np.array_equal(bare["moments"].cpu().numpy(), want["moments"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.scan_align_step(*dev, 0.2, *frame, want_index=True)
    side.synchronize()
    _same({k: v.cpu().numpy() for k, v in other.items()}, want, "a second stream")
    # a set one row beyond the cap, on either side, and offsets that reach beyond the rows: the empty result, the others whole
    cap = ops.ALIGN_MAX_POINTS
    long = r.uniform(-1, 1, (cap + 1, 3)).astype(f32)
    for what, (p, o, q, to) in {"a long source": (np.concatenate([src[:300], long]), [0, 300, cap + 301], dst, toffsets),
                                "a long target": (src, offsets, np.concatenate([dst[:500], long]), [0, 500, cap + 501])}.items():
        a, s = align_law.frame(dst[:500], [0, 500], 0.2)
        a, s = np.concatenate([a, a]), np.concatenate([s, s])
        got = _run(p, o, q, to, transforms[:, :2], 0.2, a, s)
        assert not got["moments"][1].any() and (got["index"][:, 300:] == -1).all() and np.isinf(got["dist2"][:, 300:]).all(), what
        assert np.array_equal(got["moments"][0], want["moments"][0, :2]) and np.array_equal(got["index"][:, :300], want["index"][:2, :300])
    wild = _run(src, [0, 300, 701], dst, [0, 500, 900], transforms, 0.2, anchor, shift)
    assert not wild["moments"][1].any() and np.array_equal(wild["moments"][0], want["moments"][0])
    wild = _run(src, offsets, dst, [0, 500, 901], transforms, 0.2, anchor, shift)
    assert not wild["moments"][1].any() and (wild["index"][:, 300:] == -1).all()


@functools.lru_cache(maxsize=None)
def _chain_fixture():
    r = np.random.RandomState(12)
    clouds, targets = [], []
    for s, (n, m) in enumerate(((300, 600), (280, 610), (310, 590))):
        target = r.uniform(-1, 1, (m, 3)).astype(f32)
        R, t = align_law.rotation(r.normal(size=3), np.radians(8.0 + 4 * s)), r.uniform(-0.05, 0.05, 3)
        clouds.append(((target[r.permutation(m)[:n]].astype(np.float64) + r.normal(0, 0.004, (n, 3)) - t) @ R).astype(f32))
        targets.append(target)
    return (np.concatenate(clouds), _offsets([len(c) for c in clouds]), np.concatenate(targets), _offsets([len(c) for c in targets]))


def test_the_chain_equals_the_law():
    from hyperpocket_amd import ops
    sets = _chain_fixture()
    for kw in (dict(iters=10), dict(iters=10, tol=1e-4), dict(iters=4, yaw=5, coarse_iters=2)):
        want = align_law.align(*sets, 0.25, **kw)
        got = ops.scan_align(*_sets(*sets), 0.25, **kw)
        for g, w, name in zip(got, want, ("transforms", "ok", "rms", "matched", "hypothesis")):
            assert g.dtype == w.dtype and g.shape == w.shape, (kw, name)
            assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w), \
                (kw, name, g, w)
        assert want[1].all() and (want[3] > 200).all()
    init = np.tile(np.eye(3, 4), (3, 1, 1))
    init[:, :, 3] = 0.01
    want, got = align_law.align(*sets, 0.25, iters=3, init=init), ops.scan_align(*_sets(*sets), 0.25, iters=3, init=init)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3])


def _error(T, R, t):
    rel = np.concatenate([T[:, :3] @ R.T, np.zeros((3, 1))], axis=1)
    return align_law.motion(rel)[0], float(np.linalg.norm(T[:, 3] - t))


def test_recovery_of_a_planted_motion():
    from hyperpocket_amd import ops
    source, target, R, t, _ = align_law.planted_pair(0)
    T, ok, rms, matched, hypothesis = ops.scan_align(*_sets(source, [0, 400], target, [0, 600]), INF)
    angle, move = _error(T[0], R, t)
    print(f"recovery: rotation error {angle:.3e} rad, translation error {move:.3e}, rms {rms[0]:.3e}")
    assert ok[0] and matched[0] == 400 and hypothesis[0] == -1
    assert angle <= ROT_TOL and move <= MOVE_TOL, (angle, move)


def test_yaw_search():
    """align_law.l_block at seed 0: measured with the law on the CPU, ICP from the identity ends 130 degrees from the planted
    motion and the search over 24 starts lands 3.0e-8 rad and 4.1e-8 from it."""
    from hyperpocket_amd import ops
    source, target, R, t = align_law.l_block(0)
    sets = (source, [0, len(source)], target, [0, len(target)])
    plain = ops.scan_align(*_sets(*sets), INF)
    angle, move = _error(plain[0][0], R, t)
    print(f"from the identity: {np.degrees(angle):.2f} degrees, {move:.3f}")
    assert angle > np.radians(30) and plain[4][0] == -1
    T, ok, rms, matched, hypothesis = ops.scan_align(*_sets(*sets), INF, yaw=24)
    want = align_law.align(*sets, INF, yaw=24)
    angle, move = _error(T[0], R, t)
    print(f"yaw = 24: hypothesis {hypothesis[0]}, rotation error {angle:.3e} rad, translation error {move:.3e}")
    assert ok[0] and hypothesis[0] == want[4][0] and np.array_equal(T, want[0])
    assert angle <= ROT_TOL and move <= MOVE_TOL, (angle, move)

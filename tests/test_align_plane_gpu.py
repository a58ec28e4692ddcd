"""GPU suite for the point-to-plane registration kernel (csrc/align_plane.hip): every output of ops.scan_align_plane_step bit
for bit against tests/align_plane_law.py — a ragged mix in which every source length on the wave and chunk edges meets every
target length on the LDS-tile edges, with normals of every kind, at the hypothesis counts and three gates; sums whose (hi, lo)
pairs leave 32 bits; ties and the frame's edge; isolation of the sets; buffers, streams and reproducibility — and the chain on
top of it: ops.scan_align_plane against align_plane_law.align_plane bit for bit, and recovery of the planted motion."""
import functools

import numpy as np
import pytest
import torch

import align_law
import align_plane_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32 = np.float32
INF = float("inf")
# the pose error of three steps on wavy_pair, measured with the law on the CPU (test_align_plane_law_host.py asserts 4 x)
POSE_ROT, POSE_MOVE = 4 * 1.27e-3, 4 * 3.73e-4
NAMES = ("moments", "index", "dist2")


def _t(a, dtype):
    return torch.as_tensor(np.array(a), dtype=dtype).to(CUDA)              # a copy: the fixtures are read-only


def _sets(points, offsets, tpoints, toffsets):
    return (_t(np.asarray(points, dtype=f32).reshape(-1, 3), torch.float32), _t(offsets, torch.int64),
            _t(np.asarray(tpoints, dtype=f32).reshape(-1, 3), torch.float32), _t(toffsets, torch.int64))


def _run(points, offsets, tpoints, toffsets, tnormals, transforms, max_dist, anchor, shift, want_index=True, out=None):
    from hyperpocket_amd import ops
    S = len(offsets) - 1
    res = ops.scan_align_plane_step(*_sets(points, offsets, tpoints, toffsets), _t(np.asarray(tnormals, dtype=f32), torch.float32),
                                    _t(np.asarray(transforms, dtype=f32).reshape(S, -1, 12), torch.float32), max_dist,
                                    _t(anchor, torch.float32), _t(shift, torch.int32), out=out, want_index=want_index)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _bits(a):
    return a.view(np.uint32) if a.dtype == f32 else a


def _same(got, want, what, names=NAMES):
    assert set(got) == set(names), what
    for name in names:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        wrong = np.argwhere(_bits(g) != _bits(w))
        assert len(wrong) == 0, (what, name, len(wrong), wrong[0].tolist(), g[tuple(wrong[0])], w[tuple(wrong[0])])


def _check(points, offsets, tpoints, toffsets, tnormals, transforms, max_dist, anchor=None, shift=None, what=None):
    if anchor is None:
        anchor, shift = align_law.frame(tpoints, toffsets, max_dist)
    want = law.step(points, offsets, tpoints, toffsets, tnormals, transforms, max_dist, anchor, shift)
    _same(_run(points, offsets, tpoints, toffsets, tnormals, transforms, max_dist, anchor, shift), want, what)
    return want


def _identity(S, H=1):
    return np.tile(np.eye(3, 4, dtype=f32).reshape(12), (S, H, 1))


def _motion(degrees, axis, t):
    return np.concatenate([align_law.rotation(axis, np.radians(degrees)), np.reshape(t, (3, 1))], axis=1).astype(f32).reshape(12)


def _geometry(H=1):
    from hyperpocket_amd import ops
    return ops.scan_align_plane_plan(H)


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _unit(r, n):
    v = r.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _normals_of_every_kind(r, n):
    """Unit rows, and an eighth each of: NaN rows, zero rows, a row of length 1.5, axis-aligned rows (w has two zeros)."""
    out = _unit(r, n)
    kind = r.randint(0, 8, n)
    out[kind == 0] = np.nan
    out[kind == 1] = 0
    out[kind == 2] *= f32(1.5)
    axes = np.eye(3, dtype=f32)[r.randint(0, 3, n)] * r.choice([-1, 1], n).astype(f32)[:, None]
    out[kind == 3] = axes[kind == 3]
    return out


@functools.lru_cache(maxsize=None)
def _mix(chunk, tile):
    """Every source length meets every target length, in mixed order; uniform rows in [-1, 1]^3.  Read-only."""
    src = [0, 1, 63, 64, 65, 257, chunk - 1, chunk, chunk + 1]
    dst = [0, 1, tile - 1, tile, tile + 1, 2 * tile + 1]
    r = np.random.RandomState(17)
    pairs = [(n, m) for n in src for m in dst]
    pairs = [pairs[i] for i in r.permutation(len(pairs))]
    n, m = [p[0] for p in pairs], [p[1] for p in pairs]
    points, tpoints = r.uniform(-1, 1, (sum(n), 3)).astype(f32), r.uniform(-1, 1, (sum(m), 3)).astype(f32)
    tnormals = _normals_of_every_kind(r, sum(m))
    for a in (points, tpoints, tnormals):
        a.setflags(write=False)
    return points, _offsets(n), tpoints, _offsets(m), tnormals, tuple(pairs)


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


MIX_GATES = (0.0, 0.25, INF)           # exact hits only / a part of the rows / every matched row


def test_the_mix_walks_the_edges():
    from hyperpocket_amd import ops
    threads, rows, group, tile = _geometry(1)
    assert _geometry(2) == _geometry(ops.ALIGN_MAX_HYPOTHESES) == (threads, rows, group, tile) and group == 1
    chunk = threads * rows
    pairs = _mix(chunk, tile)[5]
    assert {n for n, _ in pairs} == {0, 1, 63, 64, 65, 257, chunk - 1, chunk, chunk + 1}
    assert {m for _, m in pairs} == {0, 1, tile - 1, tile, tile + 1, 2 * tile + 1}
    assert len(set(pairs)) == 9 * 6 and list(pairs) != sorted(pairs)
    has = law.normal_ints(_mix(chunk, tile)[4])[1]
    assert 0.4 < has.mean() < 0.8                                   # NaN, zero and long rows are without normal; the rest is used


@pytest.mark.parametrize("H", [1, 2])                               # {1, 2, group, group + 1} with the plan's group of 1
def test_ragged_mix(H):
    threads, rows, group, tile = _geometry(H)
    assert group == 1
    points, offsets, tpoints, toffsets, tnormals, pairs = _mix(threads * rows, tile)
    S = len(pairs)
    transforms = _mix_transforms(S, H)
    match = None
    for gate in MIX_GATES[::-1]:
        anchor, shift = align_law.frame(tpoints, toffsets, gate)
        want = law.step(points, offsets, tpoints, toffsets, tnormals, transforms, gate, anchor, shift, match=match)
        match = want                                                # the matches do not depend on the gate or the frame
        _same(_run(points, offsets, tpoints, toffsets, tnormals, transforms, gate, anchor, shift), want, (H, gate))
        counts = want["moments"][:, :, :3]
        full = np.array([n if m else 0 for n, m in pairs])
        finite = np.isfinite(transforms).all(axis=2)
        assert not want["moments"][:, :, 3].any()
        if gate == INF:                                             # every row of a job whose transform is finite is accounted for
            assert np.array_equal(counts.sum(axis=2), np.where(finite, full[:, None], 0))
            assert counts[:, :, 0].any() and counts[:, :, 1].any() and counts[:, :, 2].any()
        elif gate == 0.0:
            assert not counts.any()
        else:
            assert 0 < counts[:, :, 0].sum() < np.where(finite, full[:, None], 0).sum() and counts[:, :, 2].any()


@pytest.mark.parametrize("gate", [INF, 0.25])
@pytest.mark.parametrize("H", [1, 2])                               # at 2 the point step sweeps a partial group of 4, this one groups of 1
def test_the_match_is_the_point_steps(H, gate):
    """index and dist2 are ops.scan_align_step's bit for bit: both steps are one sweep (csrc/hp_align.h)."""
    from hyperpocket_amd import ops
    threads, rows, _, tile = _geometry(H)
    points, offsets, tpoints, toffsets, tnormals, pairs = _mix(threads * rows, tile)
    S = len(pairs)
    anchor, shift = align_law.frame(tpoints, toffsets, gate)
    sets = _sets(points, offsets, tpoints, toffsets)
    frame = _t(_mix_transforms(S, H).reshape(S, H, 12), torch.float32), gate, _t(anchor, torch.float32), _t(shift, torch.int32)
    plane = ops.scan_align_plane_step(*sets, _t(tnormals, torch.float32), *frame, want_index=True)
    point = ops.scan_align_step(*sets, *frame, want_index=True)
    got, want = ({k: res[k].cpu().numpy() for k in NAMES[1:]} for res in (plane, point))
    _same(got, want, (H, gate), NAMES[1:])
    assert (want["index"] >= 0).any() and (want["index"] < 0).any()    # matched rows, and absent ones


def test_sums_beyond_32_bits():
    """One job, two chunks, every row matched across a large residual: the lo sums pass 2^31 and hi sums are negative."""
    threads, rows, _, tile = _geometry(1)
    n = 2 * threads * rows
    r = np.random.RandomState(21)
    source = (r.uniform(-1, 1, (n, 3)) + [0.9, -0.7, 0.8]).astype(f32)
    target = r.uniform(-1, 1, (3 * tile + 5, 3)).astype(f32)
    want = _check(source, [0, n], target, [0, len(target)], _unit(r, len(target)), _identity(1), INF, what="a large residual")
    mom = want["moments"][0, 0]
    assert mom[:4].tolist() == [n, 0, 0, 0]
    assert (mom[5::2] > 2 ** 31).any() and (mom[4::2] < 0).any() and np.abs(mom[4::2]).max() > 2 ** 31
    assert max(abs(s) for s in law.sums_of(mom)) > 2 ** 62
    # and the smallest: one used row, so every sum is one term
    one = _check(source[:1], [0, 1], target, [0, len(target)], _unit(r, len(target)), _identity(1), INF, what="one row")
    assert one["moments"][0, 0, 0] == 1


def test_ties_and_the_frames_edge():
    r = np.random.RandomState(3)
    base = r.uniform(-1, 1, (300, 3)).astype(f32)
    target = np.concatenate([base, base[::-1], base[:50]])          # every row two or three times, each copy with its own normal
    normals = _unit(r, len(target))
    want = _check(base, [0, 300], target, [0, len(target)], normals, _identity(1), INF, what="duplicates")
    assert np.array_equal(want["index"][0], np.minimum(np.arange(300), 599 - np.arange(300)))
    assert want["moments"][0, 0, 0] == 300 and not want["moments"][0, 0, 46:].any()      # b == 0: the a_i b and b b sums vanish
    assert want["moments"][0, 0, 4:46].any()
    lattice = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)
    _check(lattice + f32(0.5), [0, 512], lattice, [0, 512], _unit(r, 512), _identity(1), INF, what="a cell centre has eight nearest rows")
    # the frame's edge: rows far outside the targets' box are clipped whatever their normal says, and enter no sum
    dst, src = r.uniform(-1, 1, (500, 3)).astype(f32), r.uniform(-1, 1, (300, 3)).astype(f32)
    src[:40] += f32(9)
    dnormals = _normals_of_every_kind(r, 500)
    anchor, shift = align_law.frame(dst, [0, 500], 0.0)             # gate 0: the tightest frame, clipping at 2^(shift + 1)
    want = _check(src, [0, 300], dst, [0, 500], dnormals, _identity(1), INF, anchor, shift, "rows outside the frame")
    assert want["moments"][0, 0, 1] == 40 and want["moments"][0, 0, 0] + want["moments"][0, 0, 2] == 260
    inside = law.step(src[40:], [0, 260], dst, [0, 500], dnormals, _identity(1), INF, anchor, shift)
    assert np.array_equal(inside["moments"][0, 0, 2:], want["moments"][0, 0, 2:])
    edge = np.array([[2, 0, 0], [np.nextafter(f32(2), f32(0)), 0, 0], [-2, 0, 0]], f32)   # exactly at the bound, and just inside
    _check(edge, [0, 3], edge, [0, 3], np.eye(3, dtype=f32), _identity(1), INF, np.zeros((1, 3), f32), np.array([0], np.int32),
           "the bound itself")
    for s in (-100, 128, 140, -140):                                # the frame's own range, and shifts beyond it
        _check(src, [0, 300], dst, [0, 500], dnormals, _identity(1), INF, np.zeros((1, 3), f32), np.array([s], np.int32), ("shift", s))
    # absent rows on both sides and a job with a NaN transform
    src[50:90, 1] = np.nan
    dst[::7, 2] = np.inf
    T = np.stack([_identity(1)[0, 0], _motion(40, (1, 2, 3), (0.1, 0.2, -0.1)), np.full(12, np.nan, f32)])[None]
    want = _check(src, [0, 300], dst, [0, 500], dnormals, T, 0.5, what="absent rows")
    assert not want["moments"][0, 2].any() and (want["index"][:, 50:90] == -1).all()


def test_sets_are_isolated():
    r = np.random.RandomState(8)
    n, m = [130, 70, 513], [300, 20, 90]
    clouds = [r.uniform(-1, 1, (k, 3)).astype(f32) for k in n]
    targets = [r.uniform(-1, 1, (k, 3)).astype(f32) for k in m]
    normals = [_normals_of_every_kind(r, k) for k in m]
    transforms = np.stack([np.stack([_motion(r.uniform(-30, 30), r.normal(size=3), r.uniform(-0.1, 0.1, 3)) for _ in range(2)])
                           for _ in n])
    pack = lambda c, t, w: (np.concatenate(c), _offsets(n), np.concatenate(t), _offsets(m), np.concatenate(w), transforms)
    anchor, shift = align_law.frame(np.concatenate(targets), _offsets(m), 0.3)
    base = _check(*pack(clouds, targets, normals), 0.3, anchor, shift, what="clean neighbours")
    assert base["moments"][:, :, 0].all()
    # the middle set between poisoned neighbours: their rows and their normals are NaN and huge values
    poison = lambda a: np.where(r.randint(0, 2, a.shape).astype(bool), f32(np.nan), f32(3e38)).astype(f32)
    bad = _check(*pack([poison(clouds[0]), clouds[1], poison(clouds[2])], [poison(targets[0]), targets[1], poison(targets[2])],
                       [poison(normals[0]), normals[1], poison(normals[2])]), 0.3, anchor, shift, what="poisoned neighbours")
    assert np.array_equal(bad["moments"][1], base["moments"][1]) and not bad["moments"][0].any() and not bad["moments"][2].any()
    assert np.array_equal(bad["index"][:, 130:200], base["index"][:, 130:200])
    # poisoned normals alone: the neighbours match as before and count every gated row as without normal
    odd = _check(*pack(clouds, targets, [poison(normals[0]), normals[1], poison(normals[2])]), 0.3, anchor, shift, what="poisoned normals")
    assert np.array_equal(odd["moments"][1], base["moments"][1]) and np.array_equal(odd["index"], base["index"])
    assert not odd["moments"][0, :, 0].any() and np.array_equal(odd["moments"][0, :, 2], base["moments"][0, :, 0] + base["moments"][0, :, 2])


def test_buffers_streams_and_reproducibility():
    from hyperpocket_amd import ops
    r = np.random.RandomState(9)
    src, dst = r.uniform(-1, 1, (700, 3)).astype(f32), r.uniform(-1, 1, (900, 3)).astype(f32)
    nrm = _normals_of_every_kind(r, 900)
    offsets, toffsets = [0, 300, 700], [0, 500, 900]
    transforms = np.stack([np.stack([_motion(5 * h + s, (1, 1, 0), (0.01 * h, 0, 0)) for h in range(3)]) for s in range(2)])
    anchor, shift = align_law.frame(dst, toffsets, 0.2)
    want = law.step(src, offsets, dst, toffsets, nrm, transforms, 0.2, anchor, shift)
    dev = _sets(src, offsets, dst, toffsets) + (_t(nrm, torch.float32), _t(transforms, torch.float32))
    frame = (_t(anchor, torch.float32), _t(shift, torch.int32))
    out = {"moments": torch.full((2, 3, 60), -7, dtype=torch.int64, device=CUDA),
           "index": torch.full((3, 700), -7, dtype=torch.int32, device=CUDA),
           "dist2": torch.full((3, 700), float("nan"), device=CUDA)}
    res = ops.scan_align_plane_step(*dev, 0.2, *frame, out=out, want_index=True)
    assert res["moments"] is out["moments"] and res["index"] is out["index"]
    first = {k: v.cpu().numpy() for k, v in res.items()}
    _same(first, want, "poisoned buffers")
    res = ops.scan_align_plane_step(*dev, 0.2, *frame, out=out, want_index=True)      # ... and again over its own results
    _same({k: v.cpu().numpy() for k, v in res.items()}, first, "reused buffers: two runs, the same bits")
    bare = ops.scan_align_plane_step(*dev, 0.2, *frame)
    assert set(bare) == {"moments"} and np.array_equal(bare["moments"].cpu().numpy(), want["moments"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.scan_align_plane_step(*dev, 0.2, *frame, want_index=True)
    side.synchronize()
    _same({k: v.cpu().numpy() for k, v in other.items()}, want, "a second stream")
    # offsets that reach beyond the rows: the empty result, the other set whole
    wild = _run(src, [0, 300, 701], dst, toffsets, nrm, transforms, 0.2, anchor, shift)
    assert not wild["moments"][1].any() and np.array_equal(wild["moments"][0], want["moments"][0])
    wild = _run(src, offsets, dst, [0, 500, 901], nrm, transforms, 0.2, anchor, shift)
    assert not wild["moments"][1].any() and (wild["index"][:, 300:] == -1).all()


def test_the_chain_equals_the_law_and_recovers_the_motion():
    from hyperpocket_amd import ops
    pairs = [law.wavy_pair(seed=0), law.wavy_pair(seed=1, degrees=15.0)]
    points, tpoints = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    tnormals = np.concatenate([law.normals_of(seed=0), law.normals_of(seed=1)])
    sets = (points, _offsets([1500, 1500]), tpoints, _offsets([1500, 1500]))
    same = lambda g, w: np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w)
    for kw in (dict(iters=3), dict(iters=6, tol=2e-3)):
        want = law.align_plane(*sets, tnormals, 0.3, **kw)
        got = ops.scan_align_plane(*_sets(*sets), 0.3, tnormals=_t(tnormals, torch.float32), **kw)
        for g, w, name in zip(got, want, ("transforms", "ok", "rms", "matched")):
            assert g.dtype == w.dtype and g.shape == w.shape and same(g, w), (kw, name, g, w)
        assert want[1].all() and (want[3] > 1400).all()
    for s, (_, _, R, t) in enumerate(pairs):
        angle, move = law.pose_error(got[0][s], R, t)
        print(f"pair {s}: rotation error {angle:.3e} rad, translation error {move:.3e}, rms {got[2][s]:.3e}")
        assert angle <= POSE_ROT and move <= POSE_MOVE, (s, angle, move)
    init = np.tile(np.eye(3, 4), (2, 1, 1))
    init[:, :, 3] = 0.01
    want = law.align_plane(*sets, tnormals, 0.3, iters=2, init=init)
    got = ops.scan_align_plane(*_sets(*sets), 0.3, iters=2, init=init, tnormals=_t(tnormals, torch.float32))
    assert same(got[0], want[0]) and np.array_equal(got[3], want[3])
    # the normals of the device (ops.scan_normals equals normals_law bit for bit) give the same chain
    own = ops.scan_align_plane(*_sets(*sets), 0.3, iters=2, init=init, k=16)
    assert same(own[0], want[0]) and same(own[2], want[2])

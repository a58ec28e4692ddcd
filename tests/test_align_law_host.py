"""CPU suite for the registration law itself (tests/align_law.py, no library and no GPU): the match against a float64
brute-force nearest neighbour, ties, the empty results, the frame's rule, the closed-form solve against the fp64 Kabsch / SVD
fit, its degenerate cases, the yaw starts, and the two fixtures the GPU suite relies on."""
import numpy as np
import pytest

import align_law

f32 = np.float32
INF = float("inf")
# measured here at seed 0: |rigid_from_moments - Kabsch| = 4.27e-7 rad and 2.79e-7 in t (the frame's quantum is 2^-17 = 7.6e-6)
SEED0_ROT, SEED0_MOVE = 4.27e-7, 2.79e-7


def _identity(S=1, H=1):
    return np.tile(np.eye(3, 4, dtype=f32).reshape(12), (S, H, 1))


def test_match_equals_a_float64_brute_force_on_separated_inputs():
    r = np.random.RandomState(0)
    grid = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3) / 4.0 - 1.0
    target = (grid[r.permutation(len(grid))] + r.uniform(-0.02, 0.02, grid.shape)).astype(f32)     # rows at least 0.21 apart
    picks = r.permutation(len(target))[:300]
    source = (target[picks] + r.uniform(-0.05, 0.05, (300, 3))).astype(f32)                        # 0.087 at most from its own
    res = align_law.step(source, [0, 300], target, [0, len(target)], _identity(), INF, *align_law.frame(target, [0, len(target)], INF))
    d = np.linalg.norm(source.astype(np.float64)[:, None] - target.astype(np.float64)[None], axis=2)
    assert np.array_equal(res["index"][0], d.argmin(axis=1)) and np.array_equal(res["index"][0], picks)
    assert np.allclose(res["dist2"][0], d.min(axis=1) ** 2, rtol=1e-5, atol=0)
    assert res["moments"][0, 0, 0] == 300 and res["moments"][0, 0, 1] == 0


def test_ties_go_to_the_lower_row_and_absent_rows_match_nothing():
    target = np.array([[1, 0, 0], [-1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], f32)
    source = np.array([[0, 0, 0], [0.9, 0, 0], [np.nan, 1, 1], [-3, 0, 0]], f32)
    res = align_law.step(source, [0, 4], target, [0, 5], _identity(), INF, np.zeros((1, 3), f32), [2])
    assert res["index"][0].tolist() == [0, 0, -1, 1] and np.isinf(res["dist2"][0, 2]) and res["dist2"][0, 0] == 1
    gated = align_law.step(source, [0, 4], target, [0, 5], _identity(), 1.0, np.zeros((1, 3), f32), [2])
    assert gated["moments"][0, 0, 0] == 2 and np.array_equal(gated["index"], res["index"])        # d2 = 1 <= 1: inclusive
    none = align_law.step(source, [0, 4], target[3:], [0, 2], _identity(), INF, np.zeros((1, 3), f32), [2])
    assert (none["index"] == -1).all() and not none["moments"].any()


def test_empty_results_are_values():
    r = np.random.RandomState(1)
    src, dst = r.uniform(-1, 1, (10, 3)).astype(f32), r.uniform(-1, 1, (12, 3)).astype(f32)
    frame = (np.zeros((2, 3), f32), [1, 1])
    for offsets, toffsets in (([0, 0, 10], [0, 6, 12]), ([0, 5, 10], [0, 0, 12]), ([0, 5, 11], [0, 6, 12]), ([0, 5, 10], [0, 6, 13])):
        res = align_law.step(src, offsets, dst, toffsets, _identity(2), INF, *frame)
        empty = 0 if 0 in (offsets[1], toffsets[1]) else 1
        assert not res["moments"][empty].any() and res["moments"][1 - empty, 0, 0] > 0
    assert align_law.valid_set([0, align_law.MAX_POINTS], 0, 1 << 20) and not align_law.valid_set([0, align_law.MAX_POINTS + 1], 0, 1 << 20)


def test_the_frame_never_clips_a_target_row():
    r = np.random.RandomState(2)
    for k in range(200):
        n = int(r.choice([1, 2, 5, 100]))
        cloud = (r.normal(size=(n, 3)) * 10.0 ** r.uniform(-12, 12) + r.normal(size=3) * 10.0 ** r.uniform(-12, 12)).astype(f32)
        gate = float(r.choice([0.0, 10.0 ** r.uniform(-12, 12), INF]))
        anchor, shift = align_law.frame(cloud, [0, n], gate)
        assert align_law.SHIFT_MIN <= shift[0] <= align_law.SHIFT_MAX
        _, inside = align_law.quantise(cloud, anchor[0], shift[0])
        assert inside.all(), (k, n, gate, shift)
        half = float(np.ptp(cloud.astype(np.float64), axis=0).max()) / 2
        if half > 0 and shift[0] > align_law.SHIFT_MIN:                    # the smallest e: one less would not hold the sum
            x = float(align_law.scan_law.boxes_fp32(cloud)[1]) * 0.45
            assert 2.0 ** (int(shift[0]) - 1) <= x + min(float(f32(gate)), x) < 2.0 ** int(shift[0])
        near = (cloud + f32(min(gate, half) * 0.57)).astype(f32)          # within the gate of a target row, per component
        assert align_law.quantise(near, anchor[0], shift[0])[1].all()
    assert align_law.frame(np.zeros((0, 3), f32), [0, 0], 1.0)[1][0] == 0


def _kabsch(p, q):
    cp, cq = p.mean(axis=0), q.mean(axis=0)
    U, _, Vt = np.linalg.svd((p - cp).T @ (q - cq))
    R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    return R, cq - R @ cp


def _planted(seed):
    """600 rows in [-1, 1]^3 and their images under a turn of 20 degrees about a skew axis and a translation of 0.1, with
    noise of 0.01 so that the fit is not the planted motion itself."""
    r = np.random.RandomState(seed)
    p = r.uniform(-1, 1, (600, 3)).astype(f32)
    R = align_law.rotation((0.3, 0.9, -0.4), np.radians(20.0))
    t = np.array([0.6, -0.2, 0.77])
    q = (p.astype(np.float64) @ R.T + t / np.linalg.norm(t) * 0.1 + r.normal(0, 0.01, (600, 3))).astype(f32)
    return p, q


def _solve_error(seed):
    p, q = _planted(seed)
    anchor, shift = align_law.frame(q, [0, 600], INF)
    m = align_law.moments_of(p, q, np.arange(600, dtype=np.int32), np.zeros(600, f32), f32(INF), anchor[0], shift[0])
    assert m[0] == 600 and m[1] == 0
    delta, ok, rms = align_law.rigid_from_moments(m[None], shift, anchor)
    assert ok[0] and 0.2 < rms[0] < 0.4                             # the rms before the motion: the rows are 20 degrees apart
    R, t = _kabsch(p.astype(np.float64), q.astype(np.float64))
    rel = np.concatenate([delta[0, :, :3] @ R.T, np.zeros((3, 1))], axis=1)
    assert abs(np.linalg.det(delta[0, :, :3]) - 1) < 1e-12 and np.allclose(delta[0, :, :3] @ delta[0, :, :3].T, np.eye(3), atol=1e-12)
    return align_law.motion(rel)[0], float(np.linalg.norm(delta[0, :, 3] - t))


def test_the_solve_equals_kabsch_on_the_unquantised_rows():
    """Measured: seed 0 gives 4.26e-7 rad and 2.79e-7; seeds 0-6 stay below 8.4e-7 rad and 6.0e-7.  The bound is 4 x the
    seed-0 figure, the margin test_plane_law_host.py uses for the same 20-bit quantisation."""
    errors = [_solve_error(seed) for seed in range(7)]
    print("solve vs Kabsch (rad, t):", ["%.3e %.3e" % e for e in errors])
    assert errors[0][0] <= SEED0_ROT and errors[0][1] <= SEED0_MOVE, errors[0]       # the figure itself, as recorded
    for angle, move in errors:
        assert angle <= 4 * SEED0_ROT and move <= 4 * SEED0_MOVE, errors


def test_too_few_or_collinear_rows_give_the_identity():
    anchor, shift = np.zeros((1, 3), f32), np.array([1], np.int32)
    line = (np.arange(-25, 25)[:, None] / 32.0 * np.array([[0.5, 0.25, -0.75]])).astype(f32)     # dyadic: exact in the frame
    cases = {"two rows": (line[:2], line[:2] + f32(0.125)), "a line": (line, (line * f32(0.5) + f32(0.25)).astype(f32)),
             "one point": (np.zeros((5, 3), f32), np.ones((5, 3), f32))}
    for what, (p, q) in cases.items():
        m = align_law.moments_of(p, q, np.arange(len(p), dtype=np.int32), np.zeros(len(p), f32), f32(INF), anchor[0], shift[0])
        assert m[0] == len(p)
        delta, ok, rms = align_law.rigid_from_moments(m[None], shift, anchor)
        assert not ok[0] and np.array_equal(delta[0], np.eye(3, 4)) and np.isfinite(rms[0]), what
    delta, ok, rms = align_law.rigid_from_moments(np.zeros((1, 4, 18), np.int64), shift, anchor)
    assert delta.shape == (1, 4, 3, 4) and not ok.any() and np.isinf(rms).all()
    # three rows in general position are enough
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    m = align_law.moments_of(p, p[:, [1, 2, 0]], np.arange(3, dtype=np.int32), np.zeros(3, f32), f32(INF), anchor[0], shift[0])
    delta, ok, _ = align_law.rigid_from_moments(m[None], shift, anchor)
    assert ok[0] and np.allclose(delta[0, :, :3] @ p.T, p[:, [1, 2, 0]].T, atol=1e-9)


def test_yaw_starts_are_rotations_that_map_centre_to_centre():
    src, dst = np.array([[0.3, -1.0, 2.0], [5.0, 5.0, 5.0]]), np.array([[-0.2, 0.4, 0.1], [0.0, 0.0, 0.0]])
    for axis in ((0, 1, 0), (1, 2, -0.5)):
        T = align_law.yaw_transforms(24, axis, src, dst)
        assert T.shape == (2, 24, 3, 4)
        k = np.asarray(axis, float) / np.linalg.norm(axis)
        for s in range(2):
            for h in range(24):
                R = T[s, h, :, :3]
                assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) < 1e-14
                assert np.allclose(R @ k, k, atol=1e-14) and np.allclose(R @ src[s] + T[s, h, :, 3], dst[s], atol=1e-14)
                assert abs(align_law.motion(T[s, h])[0] - min(h, 24 - h) * np.pi / 12) < 1e-12
        assert np.array_equal(T[0, 0, :, :3], np.eye(3))
    assert align_law.yaw_transforms(3, (0, 0, 1), src[0], dst[0]).shape == (3, 3, 4)


def _error(T, R, t):
    return align_law.motion(np.concatenate([T[:, :3] @ R.T, np.zeros((3, 1))], axis=1))[0], float(np.linalg.norm(T[:, 3] - t))


def test_the_chain_recovers_a_planted_motion():
    source, target, R, t, rows = align_law.planted_pair(0)
    T, ok, rms, matched, hypothesis = align_law.align(source, [0, 400], target, [0, 600], INF)
    angle, move = _error(T[0], R, t)
    print(f"recovery: {angle:.3e} rad, {move:.3e}")                 # measured: 6.3e-8 rad, 6.4e-8
    assert ok[0] and matched[0] == 400 and hypothesis[0] == -1 and angle <= 4 * SEED0_ROT and move <= 4 * SEED0_MOVE
    early = align_law.align(source, [0, 400], target, [0, 600], INF, iters=30, tol=1e-9)
    assert np.allclose(early[0], T, atol=1e-6)


def test_the_yaw_fixture_needs_the_search():
    """align_law.l_block at seed 0, measured: from the identity ICP ends 130.5 degrees from the planted motion; yaw = 24 lands
    3.0e-8 rad and 4.1e-8 from it (hypothesis 7)."""
    source, target, R, t = align_law.l_block(0)
    sets = (source, [0, len(source)], target, [0, len(target)])
    plain = _error(align_law.align(*sets, INF)[0][0], R, t)
    T, ok, rms, matched, hypothesis = align_law.align(*sets, INF, yaw=24)
    angle, move = _error(T[0], R, t)
    print(f"identity: {np.degrees(plain[0]):.1f} degrees; yaw 24: {angle:.3e} rad, {move:.3e}, hypothesis {hypothesis[0]}")
    assert plain[0] > np.radians(30) and ok[0] and angle <= 4 * SEED0_ROT and move <= 4 * SEED0_MOVE

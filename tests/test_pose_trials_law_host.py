"""CPU suite for tests/pose_trials_law.py, the law csrc/pose_trials.hip is checked against: the triad fit of a congruent
triangle returns the planted motion, the edge test at rho exactly, the validity rules one by one, the kept list and the winner."""
import numpy as np

import align_law
import pose_trials_law as law

f32, f64 = np.float32, np.float64


def _planted(seed=0, n=40, degrees=140.0):
    """(source, target, R, t): target = R source + t exactly enough for the gates below; match is the identity."""
    r = np.random.RandomState(seed)
    target = r.uniform(-1, 1, (n, 3)).astype(f32)
    R, t = align_law.rotation((1, 2, 3), np.radians(degrees)), np.array([0.3, -0.2, 0.5])
    source = ((target.astype(f64) - t) @ R).astype(f32)
    return source, target, R, t


def test_the_triad_fit_of_a_congruent_triangle_returns_the_planted_motion():
    source, target, R, t = _planted()
    tri = np.array([[0, 1, 2], [5, 9, 30], [39, 3, 17]])
    ok, T = law.fit(source[tri], target[tri])
    assert ok.all()
    for k in range(len(tri)):
        angle, move = law.pose_error(T[k], R, t)
        assert angle < 1e-3 and move < 1e-5, (angle, move)             # fp32 corners: a few 1e-7 over sides of order 1
    # the fit maps the source's corners' centroid onto the target's, and is a rotation
    M = T[0].astype(f64).reshape(3, 4)
    assert np.allclose(M[:, :3] @ M[:, :3].T, np.eye(3), atol=1e-6) and np.linalg.det(M[:, :3]) > 0.999
    assert np.allclose(M[:, :3] @ source[tri[0]].astype(f64).mean(0) + M[:, 3], target[tri[0]].astype(f64).mean(0), atol=1e-6)


def test_a_hand_worked_frame():
    tri = np.array([[[0, 0, 0], [2, 0, 0], [0, 3, 0]]], dtype=f32)
    ok, E, centre = law.frames(tri)
    assert ok[0] and np.array_equal(E[0], np.eye(3)) and np.array_equal(centre[0], np.array([2, 3, 0]) / f64(3))
    ok, T = law.fit(tri, tri + f32(1))
    assert ok[0] and np.allclose(T[0].reshape(3, 4), np.concatenate([np.eye(3), np.ones((3, 1))], axis=1), atol=1e-7)


def test_collinear_and_coincident_corners_have_no_frame():
    line = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2]]], dtype=f32)
    same = np.array([[[1, 2, 3], [1, 2, 3], [0, 0, 1]]], dtype=f32)
    sliver = np.array([[[0, 0, 0], [1, 0, 0], [1, 1e-4, 0]]], dtype=f32)       # an angle of 1e-4 < 2**-12
    wide = np.array([[[0, 0, 0], [1, 0, 0], [1, 1e-3, 0]]], dtype=f32)
    assert not law.frames(line)[0][0] and not law.frames(same)[0][0] and not law.frames(sliver)[0][0] and law.frames(wide)[0][0]


def test_the_edge_test_at_rho_exactly():
    # the source's sides are exactly 0.5 of the target's: ls2 = lt2 / 4, all powers of two, so rho2 * lt2 is exact
    dst = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]], dtype=f32)
    src = dst * f32(0.5)
    assert law.edges_agree(src, dst, f32(0.25))[0]                             # ls2 >= rho2 * lt2 holds with equality: inclusive
    assert law.edges_agree(dst, src, f32(0.25))[0]                             # and the other way round
    assert not law.edges_agree(src, dst, np.nextafter(f32(0.25), f32(1)))[0]
    assert law.edges_agree(src, src, f32(1))[0] and not law.edges_agree(src, dst, f32(1))[0]
    assert law.edges_agree(src, dst, f32(0))[0]                                # rho = 0: every finite side passes
    far = dst * f32(1e30)                                                      # an overflowed squared length is refused
    assert not law.edges_agree(far, far, f32(0))[0]


def test_validity_rules_and_the_winner():
    source, target, R, t = _planted(seed=1, n=30)
    off = np.array([0, 30])
    match = np.arange(30, dtype=np.int32)
    out = law.pose_trials_law(source, off, target, off, match, 1e-4, trials=256, keep=64, seed=3)
    rows = law.sample_rows(3, 0, 256, 30)
    distinct = (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2])
    assert out["valid"][0] == distinct.sum() and out["kept"][0] == 64          # a planted set: every distinct triple is valid
    assert out["trial"][0] == np.flatnonzero(distinct)[0]                      # all score 30: ties to the lower h
    assert out["inliers"][0] == 30 and out["found"][0] == 1
    assert law.pose_error(out["transform"][0], R, t)[0] < 1e-2
    # a wrong match breaks the triples that use it and is no inlier of the others
    wrong = match.copy()
    wrong[7] = 8
    out2 = law.pose_trials_law(source, off, target, off, wrong, 1e-4, trials=256, keep=4096, seed=3)
    uses7 = (rows == 7).any(axis=1)
    assert (distinct & ~uses7).sum() <= out2["valid"][0] < distinct.sum() and out2["inliers"][0] == 29
    # under three matches, all matches on one target row, no rows: no valid trial
    few = np.full(30, -1, dtype=np.int32)
    few[:2] = [0, 1]
    for m in (few, np.zeros(30, dtype=np.int32), np.full(30, 31, dtype=np.int32)):
        none = law.pose_trials_law(source, off, target, off, m, 1.0, trials=64)
        assert none["valid"][0] == 0 and none["trial"][0] == -1 and none["found"][0] == 0 and np.isnan(none["transform"]).all()
    # keep below the number of valid trials: the first ones in ascending h
    low = law.pose_trials_law(source, off, target, off, match, 1e-4, trials=256, keep=1, seed=3)
    assert low["kept"][0] == 1 and low["valid"][0] == out["valid"][0] and low["trial"][0] == out["trial"][0]
    # streams name the draw, not the set's number
    by_stream = law.pose_trials_law(source, off, target, off, match, 1e-4, trials=256, keep=64, seed=3, streams=[5])
    assert by_stream["trial"][0] == np.flatnonzero((lambda r: (r[:, 0] != r[:, 1]) & (r[:, 0] != r[:, 2]) & (r[:, 1] != r[:, 2]))(
        law.sample_rows(3, 5, 256, 30)))[0]


def test_gates_zero_and_infinite():
    source, target, R, t = _planted(seed=2, n=20)
    off = np.array([0, 20])
    match = np.arange(20, dtype=np.int32)
    zero = law.pose_trials_law(source, off, target, off, match, 0.0, trials=64)
    every = law.pose_trials_law(source, off, target, off, match, np.inf, trials=64)
    assert zero["trial"][0] >= 0 and 0 <= zero["inliers"][0] < 20 and every["inliers"][0] == 20
    src = source.copy()
    src[3] = np.nan                                                            # an absent row is nobody's inlier, whatever the gate
    assert law.pose_trials_law(src, off, target, off, match, np.inf, trials=64)["inliers"][0] == 19

"""CPU suite for the point-to-plane law itself (tests/align_plane_law.py, the checker of csrc/align_plane.hip): its integer
bounds, the (hi, lo) pairs against Python integers, the match against align_law's, the quantised step against the float64
Gauss-Newton step, convergence against point-to-point ICP, and what is refused.

Measured with the law (every test prints its figures before it asserts; the asserted bounds are 4 x these, the project's convention):
    the quantised step against reference_fp64_step on wavy_pair(noise=0.002), six iterations from the identity:
        first step (an 8 degree residual)    |d omega| 6.72e-4 rad    |d t| 1.68e-4
        steps 2 to 6                         |d omega| 2.22e-5 rad    |d t| 1.32e-5
      both sides linearise and use the same rows: the difference is the 9-bit normals acting on the residual.
    pose error after 3 steps of align_plane on wavy_pair, seeds 0 to 2 at 8 and at 15 degrees, the largest:
        rotation 1.27e-3 rad, translation 3.73e-4 — the noise floor of 1500 rows at noise 0.002.
    pose error after 30 steps of align_law.align (point-to-point) at seed 0:
        8 degrees 7.37e-2 rad / 3.28e-2, 15 degrees 1.30e-1 rad / 5.48e-2.
    lambda_min / lambda_max of the block-scaled system, first step: slab_pair() 3.75e-5, wavy_pair() 7.38e-3."""
import numpy as np
import pytest

import align_law
import align_plane_law as law
import normals_law

f32 = np.float32
INF = float("inf")
GATE = 0.3
STEP_FIRST = (6.72e-4, 1.68e-4)
STEP_LATER = (2.22e-5, 1.32e-5)
POSE_ROT, POSE_MOVE = 4 * 1.27e-3, 4 * 3.73e-4
RATIO_SLAB, RATIO_WAVY = 3.75e-5, 7.38e-3


def _one(source, target):
    return source, np.array([0, len(source)]), target, np.array([0, len(target)])


def _identity():
    return np.eye(3, 4, dtype=f32).reshape(1, 1, 12)


def _first_step(source, target, normals, gate=GATE):
    sets = _one(source, target)
    anchor, shift = align_law.frame(target, sets[3], gate)
    return law.step(*sets, normals, _identity(), gate, anchor, shift), anchor, shift


def test_the_integer_bounds_hold():
    source, target, _, _ = law.wavy_pair()
    out, _, _ = _first_step(source, target, law.normals_of())       # the law asserts its bounds as it goes
    assert out["moments"][0, 0, 0] == 1500 and not out["moments"][0, 0, 1:4].any()
    # the adversarial set: targets on the corners of [-1, 1]^3, sources just inside the frame's corners (it clips at 8 = 2^(shift + 1)),
    # no gate, normals along the diagonals — u at its largest magnitude, d across the frame, w with three equal components
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=f32)
    edge = np.nextafter(f32(8), f32(0))
    far = np.concatenate([corners * edge, -corners * edge, corners * edge * np.array([1, -1, 1], f32)])
    normals = (corners.astype(np.float64) * [1, -1, 1] / np.sqrt(3.0)).astype(f32)       # another diagonal than the row's own
    anchor, shift = align_law.frame(corners, [0, 8], INF)
    assert shift[0] == 2 and not anchor.any()
    out = law.step(far, [0, 24], corners, [0, 8], normals, _identity(), INF, anchor, shift)
    assert out["moments"][0, 0, :4].tolist() == [24, 0, 0, 0]
    moved, present = align_law.transform_rows(far, _identity().reshape(12))
    u, v, w, _, _, _ = law.used_rows(moved, corners, normals, out["index"][0], out["dist2"][0], f32(INF), anchor[0], shift[0])
    c, b = np.cross(u, w), -((u - v) * w).sum(axis=1)
    print(f"adversarial: |u| up to {np.abs(u).max()} (2^20 = {2 ** 20}), |c|_2 up to 2^{np.log2(np.sqrt((c.astype(float) ** 2).sum(1)).max()):.2f},"
          f" |b| up to 2^{np.log2(np.abs(b).max()):.2f}, largest |term| 2^{np.log2(float(np.abs(law.terms_of(u, v, w)).max())):.2f}")
    assert np.abs(u).max() == 2 ** 20 - 1 and (w * w).sum(axis=1).max() <= law.NORMAL_MAX
    assert np.abs(law.terms_of(u, v, w)).max() > 2 ** 55                # far beyond what one 64-bit sum of 2^16 rows could take


def test_the_pairs_rebuild_the_exact_sums():
    source, target, _, _ = law.wavy_pair(degrees=15.0)
    out, anchor, shift = _first_step(source, target, law.normals_of())
    moved, _ = align_law.transform_rows(source, _identity().reshape(12))
    u, v, w, _, clipped, without = law.used_rows(moved, target, law.normals_of(), out["index"][0], out["dist2"][0], f32(GATE * GATE),
                                                 anchor[0], shift[0])
    sums = [0] * 28
    for ui, vi, wi in zip(u.tolist(), v.tolist(), w.tolist()):      # Python integers throughout
        c = [ui[1] * wi[2] - ui[2] * wi[1], ui[2] * wi[0] - ui[0] * wi[2], ui[0] * wi[1] - ui[1] * wi[0]]
        a = c + wi
        b = -sum((ui[k] - vi[k]) * wi[k] for k in range(3))
        terms = [a[i] * a[j] for i in range(6) for j in range(i, 6)] + [x * b for x in a] + [b * b]
        sums = [s + t for s, t in zip(sums, terms)]
    mom = out["moments"][0, 0]
    assert mom[:4].tolist() == [len(u), clipped, without, 0] and len(u) > 1000
    assert law.sums_of(mom) == sums
    assert (mom[5::2] >= 0).all() and (mom[4::2] < 0).any() and max(abs(s) for s in sums) > 2 ** 62
    A, g, bb = law.system_of(mom)
    assert np.array_equal(A, A.T) and bb == sums[27] and A[0, 0] == float(sums[0]) and A[5, 5] == float(sums[20]) and g[5] == float(sums[26])


def test_the_match_is_align_laws():
    source, target, _, _ = law.wavy_pair()
    sets = _one(source, target)
    anchor, shift = align_law.frame(target, sets[3], GATE)
    T = np.concatenate([align_law.rotation((1, 2, 3), 0.1), [[0.01], [0.02], [0.0]]], axis=1).astype(f32).reshape(1, 1, 12)
    got = law.step(*sets, law.normals_of(), T, GATE, anchor, shift)
    want = align_law.step(*sets, T, GATE, anchor, shift)
    assert np.array_equal(got["index"], want["index"]) and np.array_equal(got["dist2"].view(np.uint32), want["dist2"].view(np.uint32))
    assert got["moments"][0, 0, 0] == want["moments"][0, 0, 0] and got["moments"][0, 0, 1] == want["moments"][0, 0, 1]
    again = law.step(*sets, law.normals_of(), T, GATE, anchor, shift, match=want)
    assert np.array_equal(again["moments"], got["moments"])


def test_the_quantised_step_against_fp64():
    source, target, _, _ = law.wavy_pair(noise=0.002)
    sets, normals = _one(source, target), law.normals_of()
    anchor, shift = align_law.frame(target, sets[3], GATE)
    T, worst = np.eye(3, 4), {"first": [0.0, 0.0], "later": [0.0, 0.0]}
    for it in range(6):
        mom = law.step(*sets, normals, T.astype(f32).reshape(1, 1, 12), GATE, anchor, shift)["moments"]
        x, ok, _ = law.solve_plane(mom[0, 0])
        ref = law.reference_fp64_step(source, target, normals, T.astype(f32), GATE, anchor[0], shift[0])
        dw, dt = np.linalg.norm(x[:3] - ref[:3]), np.linalg.norm(np.ldexp(x[3:], int(shift[0]) - 19) - ref[3:])
        print(f"step {it + 1}: |omega| {np.linalg.norm(x[:3]):.3e}, |d omega| {dw:.3e} rad, |d t| {dt:.3e}")
        key = "first" if it == 0 else "later"
        worst[key] = [max(worst[key][0], dw), max(worst[key][1], dt)]
        assert ok
        delta, _, _ = law.rigid_from_plane_moments(mom, shift, anchor)
        T = align_law.compose(delta[0, 0], T)
    assert worst["first"][0] <= 4 * STEP_FIRST[0] and worst["first"][1] <= 4 * STEP_FIRST[1], worst
    assert worst["later"][0] <= 4 * STEP_LATER[0] and worst["later"][1] <= 4 * STEP_LATER[1], worst


@pytest.mark.parametrize("degrees", [8.0, 15.0])
def test_three_steps_reach_what_thirty_point_to_point_steps_do_not(degrees):
    for seed in (0, 1, 2):
        source, target, R, t = law.wavy_pair(seed=seed, degrees=degrees)
        T, ok, rms, matched = law.align_plane(*_one(source, target), law.normals_of(seed=seed), GATE, iters=3)
        angle, move = law.pose_error(T[0], R, t)
        print(f"{degrees} degrees, seed {seed}, point-to-plane, 3 steps: {angle:.3e} rad, {move:.3e}; rms {rms[0]:.3e}, matched {matched[0]}")
        assert ok[0] and matched[0] > 1400 and angle <= POSE_ROT and move <= POSE_MOVE, (seed, angle, move)
        assert 0.5 * 0.002 < rms[0] < 2 * 0.002                        # the rms point-to-plane distance is the noise
    source, target, R, t = law.wavy_pair(degrees=degrees)
    T, ok, _, _, _ = align_law.align(*_one(source, target), GATE, iters=30)
    angle, move = law.pose_error(T[0], R, t)
    print(f"{degrees} degrees, seed 0, point-to-point, 30 steps: {angle:.3e} rad, {move:.3e}")
    assert ok[0] and angle > 10 * POSE_ROT and move > 10 * POSE_MOVE, (angle, move)


def test_a_plane_is_refused_and_the_sheet_accepted():
    ratios = {}
    for name, (source, target, normals) in {"slab": law.slab_pair(), "wavy": law.wavy_pair()[:2] + (law.normals_of(),)}.items():
        out, anchor, shift = _first_step(source, target, normals)
        x, ok, ratios[name] = law.solve_plane(out["moments"][0, 0])
        delta, ok2, rms = law.rigid_from_plane_moments(out["moments"], shift, anchor)
        print(f"{name}: lambda_min / lambda_max = {ratios[name]:.3e}, ok {ok}, used {out['moments'][0, 0, 0]}")
        assert ok == ok2[0, 0] == (name == "wavy") and np.isfinite(rms[0, 0])
        if name == "slab":
            assert np.array_equal(delta[0, 0], np.eye(3, 4)) and not x.any()
    assert 0.75 * RATIO_SLAB < ratios["slab"] < 1.25 * RATIO_SLAB and 0.75 * RATIO_WAVY < ratios["wavy"] < 1.25 * RATIO_WAVY
    assert ratios["wavy"] / ratios["slab"] >= 100                        # far enough apart for a constant between them
    mean = np.sqrt(ratios["slab"] * ratios["wavy"])
    assert law.DEGENERATE_PLANE == 2.0 ** np.round(np.log2(mean)) == 2.0 ** -11
    # measured and not used: normals_law.slab() at noise 0.02 is as constrained as the sheet (see DEGENERATE_PLANE)
    source, target, normals = law.slab_pair(noise=0.02)
    assert np.array_equal(target, normals_law.slab()[0])
    ratio = law.solve_plane(_first_step(source, target, normals)[0]["moments"][0, 0])[2]
    print(f"normals_law.slab() (noise 0.02): lambda_min / lambda_max = {ratio:.3e}")
    assert ratio > 0.5 * ratios["wavy"]
    # an exact plane: the normals are one integer vector, three diagonal entries are exactly zero
    flat = np.array(law.slab_pair()[1])
    flat[:, 1] = 0
    normals = np.tile(np.array([0, 1, 0], f32), (len(flat), 1))
    out, anchor, shift = _first_step(flat + f32(0.001), flat, normals)
    assert out["moments"][0, 0, 0] == len(flat) and not law.rigid_from_plane_moments(out["moments"], shift, anchor)[1][0, 0]


def test_fewer_than_six_rows_are_refused():
    source, target, _, _ = law.wavy_pair()
    normals = law.normals_of()
    for n in (5, 6, 40):
        out, anchor, shift = _first_step(source[:n], target, normals)
        delta, ok, rms = law.rigid_from_plane_moments(out["moments"], shift, anchor)
        print(f"{n} rows: used {out['moments'][0, 0, 0]}, ok {ok[0, 0]}, ratio {law.solve_plane(out['moments'][0, 0])[2]:.3e}")
        assert out["moments"][0, 0, 0] == n and np.isfinite(rms[0, 0])
        if n < 6:
            assert not ok[0, 0] and np.array_equal(delta[0, 0], np.eye(3, 4))
        if n == 40:
            assert ok[0, 0]
    empty = np.zeros((2, 3, law.MOMENTS), np.int64)
    delta, ok, rms = law.rigid_from_plane_moments(empty, np.zeros(2, np.int32), np.zeros((2, 3), f32))
    assert delta.shape == (2, 3, 3, 4) and not ok.any() and np.isinf(rms).all()


def test_rows_without_a_normal_are_counted_and_not_summed():
    source, target, _, _ = law.wavy_pair()
    sets = _one(source, target)
    anchor, shift = align_law.frame(target, sets[3], GATE)
    base = align_law.step(*sets, _identity(), GATE, anchor, shift)
    gated = int(base["moments"][0, 0, 0])
    out = law.step(*sets, np.full((1500, 3), np.nan, f32), _identity(), GATE, anchor, shift)
    assert out["moments"][0, 0, :4].tolist() == [0, 0, gated, 0] and not out["moments"][0, 0, 4:].any() and gated > 1000
    # every kind of row without a normal, and the rows around them untouched
    normals = np.array(law.normals_of())
    kinds = {"nan": (np.nan, 0, 1), "inf": (0, np.inf, 0), "zero": (0, 0, 0), "tiny": (1e-3, -1e-3, 1e-3), "long": (0, 1.5, 0),
             "huge": (3e38, 0, 0), "just over": (0, 0, 1.004)}
    hit = np.unique(base["index"][0][base["index"][0] >= 0])[:len(kinds)]
    for row, value in zip(hit, kinds.values()):
        normals[row] = value
    assert not law.normal_ints(normals[hit])[1].any()
    assert law.normal_ints(np.array([[1, 0, 0], [0, 0, -1], [0, 1.0039, 0], [0.6, 0, 0.8]], f32))[1].all()      # axis-aligned and just under
    some = law.step(*sets, normals, _identity(), GATE, anchor, shift)
    lost = int(np.isin(base["index"][0], hit).sum())
    assert some["moments"][0, 0, :3].tolist() == [gated - lost, 0, lost]
    keep = ~np.isin(base["index"][0], hit)
    rest = law.step(source[keep], [0, int(keep.sum())], target, sets[3], law.normals_of(), _identity(), GATE, anchor, shift)
    assert np.array_equal(rest["moments"][0, 0, 3:], some["moments"][0, 0, 3:])
    # clipped comes first: a row outside the frame is clipped whatever its normal
    out = law.step(source + f32(9), sets[1], target, sets[3], np.full((1500, 3), np.nan, f32), _identity(), INF,
                   *align_law.frame(target, sets[3], 0.0))
    assert out["moments"][0, 0, :3].tolist() == [0, 1500, 0]

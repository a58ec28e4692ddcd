"""CPU suite for tests/depth_law.py, the yardstick of ops.depth_points: the vectorised form against the per-pixel loop bit for
bit, the law's small cases with their exact expectations, and an analytic round trip — a slanted plane and a sphere rendered to
fp32 depth by this file's own ray formulas come back as points on the surface with the surface's normals."""
import numpy as np
import pytest

import depth_law as law

f32, f64 = np.float32, np.float64
EPS = 2.0 ** -24                                                   # half an fp32 ulp, relative


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == f32 else a              # signed zeros count


def _same(got, want, what):
    assert set(got) == set(want)
    for name in want:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        wrong = np.argwhere(_bits(g) != _bits(w))
        assert len(wrong) == 0, (what, name, len(wrong), wrong[0].tolist(), g[tuple(wrong[0])], w[tuple(wrong[0])])


def _pose(seed):
    """A real rotation and translation as (3,4) float32."""
    q = np.random.RandomState(seed).standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return np.concatenate([np.array(R), [[0.3], [-1.25], [2.0]]], 1).astype(f32)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (67, 3), (33, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_vectorised_law_equals_the_loop(shape, dtype):
    H, W = shape
    B = 2
    depth = law.lattice_images(H * 100 + W, B, H, W, dtype)
    scale = 1 / 64 if dtype == np.uint16 else None
    K = np.array([[40.0, 37.5, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.7], [55.25, 60.0, W / 3, H / 1.7]])
    poses = np.stack([_pose(1), _pose(2)])
    masks = (np.random.RandomState(5).rand(B, H, W) < 0.8).astype(np.uint8)
    kept = 0
    for w in range(5):
        for m, jump in ((masks, (1 / 64, 0.0)), (None, (1 / 128, 1 / 32))):
            kw = dict(poses=poses, masks=m, scale=scale, near=1.0 + 1 / 64, far=1.0 + 40 / 64, jump=jump, w=w)
            got = law.depth_law(depth, K, **kw)
            _same(got, law.depth_law_loop(depth, K, **kw), (shape, w, m is not None))
            kept += int(got["offsets"][-1])
            if w == 4 and H * W > 100:                             # the cases are not empty ones: rows survive the widest window
                assert 0 < got["offsets"][-1] < B * H * W and np.abs(got["normals"]).sum() > 0
    assert kept > 0


def _plane(H, W, value=1500):
    return np.full((1, H, W), value, np.uint16)


def test_frontal_plane_has_the_normal_minus_z_with_signed_zeros():
    for fn in (law.depth_law, law.depth_law_loop):
        got = fn(_plane(5, 7), (50.0, 50.0, 3.0, 2.0))
        assert got["offsets"].tolist() == [0, 35] and got["pixel"].tolist() == list(range(35))
        want = np.tile(np.array([-0.0, -0.0, -1.0], f32), (35, 1))
        assert (_bits(got["normals"]) == _bits(want)).all()
        assert (got["points"][:, 2] == f32(1.5)).all() and got["points"][17].tolist() == [0.0, 0.0, 1.5]


def test_a_hole_and_a_far_pixel_take_themselves_and_the_far_pixels_neighbours():
    depth = _plane(5, 7)
    depth[0, 2, 3] = 0                                             # a hole: it goes, its neighbours stay
    depth[0, 0, 0] = 4000                                          # beyond far, in the corner: it goes, with its three neighbours
    gone = {2 * 7 + 3, 0, 1, 7, 8}
    for fn in (law.depth_law, law.depth_law_loop):
        got = fn(depth, (50.0, 50.0, 3.0, 2.0), far=3.0, w=1)
        assert got["offsets"].tolist() == [0, 30]
        assert got["pixel"].tolist() == [i for i in range(35) if i not in gone]
        # without the edge test only the two go; the far pixel is a witness although it is out of range
        assert fn(depth, (50.0, 50.0, 3.0, 2.0), far=3.0, w=0)["offsets"].tolist() == [0, 33]


def test_a_tie_of_the_jump_test_is_no_jump():
    depth = np.array([[[1.0, 1.0 + 1 / 64, 1.0 + 3 / 64]]], f32)
    for fn in (law.depth_law, law.depth_law_loop):
        got = fn(depth, (10.0, 10.0, 1.0, 0.0), jump=(1 / 64, 0.0), w=1)
        assert got["pixel"].tolist() == [0]
        assert fn(depth, (10.0, 10.0, 1.0, 0.0), jump=(2 / 64, 0.0), w=1)["pixel"].tolist() == [0, 1, 2]
        assert fn(depth, (10.0, 10.0, 1.0, 0.0), jump=(1 / 64, 0.0), w=0)["pixel"].tolist() == [0, 1, 2]


def test_near_and_far_are_inclusive():
    depth = np.array([[[0.5, 1.0, 2.0, 4.0]]], f32)
    for fn in (law.depth_law, law.depth_law_loop):
        run = lambda near, far: fn(depth, (10.0, 10.0, 0.0, 0.0), near=near, far=far, w=0)["pixel"].tolist()
        assert run(0.5, 2.0) == [0, 1, 2] and run(0.5 + 2.0 ** -30, 2.0 - 2.0 ** -30) == [1]
        assert run(0.0, np.inf) == [0, 1, 2, 3] and run(4.0, 4.0) == [3]
    mm = np.array([[[500, 1000, 2000]]], np.uint16)                # in units of 1/1024: exactly representable
    assert law.depth_law(mm, (10.0, 10.0, 0.0, 0.0), scale=1 / 1024, near=500 / 1024, far=1000 / 1024, w=0)["pixel"].tolist() == [0, 1]


def test_an_image_of_holes_keeps_nothing():
    holes = np.array([[[0.0, -1.0, np.nan], [np.inf, -np.inf, -0.0]]], f32)
    for fn in (law.depth_law, law.depth_law_loop):
        for depth in (holes, np.zeros((2, 3, 4), np.uint16)):
            got = fn(depth, (10.0, 10.0, 0.0, 0.0))
            assert got["points"].shape == got["normals"].shape == (0, 3) and got["pixel"].shape == (0,)
            assert got["offsets"].tolist() == [0] * (len(depth) + 1) and got["pixel"].dtype == np.int64


def test_a_quarter_turn_about_z_and_a_shift_permute_the_points_exactly():
    r = np.random.RandomState(3)
    depth = (r.randint(8, 17, (1, 6, 5)) / 8.0).astype(f32)        # dyadic depths, fx = fy = 2, cx, cy on the half grid:
    K = (2.0, 2.0, 2.5, 1.5)                                       # every camera coordinate is exact in fp32
    pose = np.array([[0, -1, 0, 1.0], [1, 0, 0, 2.0], [0, 0, 1, 3.0]], f32)
    for fn in (law.depth_law, law.depth_law_loop):
        cam, world = fn(depth, K, jump=(10.0, 0.0)), fn(depth, K, poses=pose, jump=(10.0, 0.0))
        assert len(cam["points"]) == 30 and (cam["pixel"] == world["pixel"]).all()
        p, n = cam["points"].astype(f64), cam["normals"]
        assert (world["points"] == np.stack([-p[:, 1] + 1.0, p[:, 0] + 2.0, p[:, 2] + 3.0], 1)).all()
        assert (world["normals"] == np.stack([-n[:, 1], n[:, 0], n[:, 2]], 1)).all()
        assert np.allclose(np.linalg.norm(n.astype(f64), axis=1), 1.0, atol=4 * EPS)


# ---- analytic round trip -----------------------------------------------------------------------------------------------------
# The test renders a surface along the rays d = ((u - cx) / fx, (v - cy) / fy, 1) in fp64: the exact point is P = t d with depth
# t, and the image holds float32(t).  The law's point is float32(d * float32(t)):
#   |float32(t) - t| <= EPS t moves the point along its ray by at most EPS |P| <= sqrt(3) EPS M, M the largest |coordinate|;
#   the cast of the three coordinates adds at most sqrt(3) EPS M; the fp64 operations in between err by 2^-53 relative, nothing.
# So a point lies within 2 sqrt(3) EPS M < 4 EPS M of the surface.
# The normal is (a x b) normalised with a = P_right - P_left and b = P_down - P_up.  With da, db the errors of a and b,
# |d(a x b)| <= |da| |b| + |a| |db| to first order and the direction turns by at most |d(a x b)| / |a x b| =
# (|da| / |a| + |db| / |b|) / sin(phi), phi the angle between a and b.  |da| <= 2 sqrt(3) EPS M (two points, moved along their
# rays; these are not cast), so the rounding term is 2 sqrt(3) EPS M (1 / |a| + 1 / |b|) / sin(phi); the factor 2 sqrt(3) < 4 is
# doubled to 8 for the terms of second order.  The cast of the unit normal adds sqrt(3) EPS < 2 EPS.
# On a plane a and b of exact points lie in the plane: nothing else.  On a sphere of radius r about c the chord a is
# perpendicular to (m_a - c), m_a the midpoint of its ends, so a . (P - c) = a . (P - m_a) and a leaves the tangent plane at P
# by an angle of at most |P - m_a| / r; b likewise: (|P - m_a| + |P - m_b|) / (r sin(phi)) is the discretisation term, computed
# from the exact points.
H, W, K = 24, 32, (40.0, 40.0, 15.5, 11.5)


def _rays():
    u, v = np.meshgrid(np.arange(W, dtype=f64), np.arange(H, dtype=f64))
    return np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones((H, W))], -1)


def _round_trip(t, hit, normal_of, curvature):
    """t (H,W) exact depths, hit (H,W) where the ray meets the surface -> the law's rows, checked."""
    depth = np.where(hit, t, 0.0).astype(f32)[None]
    P = _rays() * np.where(hit, t, 0.0)[..., None]
    for fn in (law.depth_law, law.depth_law_loop):
        got = fn(depth, K, jump=(10.0, 0.0), w=0)
        v, u = np.divmod(got["pixel"], W)
        assert (got["pixel"] == np.flatnonzero(hit)).all()
        p, n = got["points"].astype(f64), got["normals"].astype(f64)
        M = np.abs(P).max()
        assert np.abs(p - P[v, u]).max() <= 4 * EPS * M             # on the surface: within the bound of the exact point
        inner = np.zeros_like(hit)
        inner[1:-1, 1:-1] = hit[1:-1, 1:-1] & hit[1:-1, 2:] & hit[1:-1, :-2] & hit[2:, 1:-1] & hit[:-2, 1:-1]
        sel = inner[v, u]
        v, u = v[sel], u[sel]
        a, b = P[v, u + 1] - P[v, u - 1], P[v + 1, u] - P[v - 1, u]
        la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
        sin = np.linalg.norm(np.cross(a, b), axis=1) / (la * lb)
        bound = 8 * EPS * M * (1 / la + 1 / lb) / sin + 2 * EPS
        if curvature is not None:
            ma, mb = (P[v, u + 1] + P[v, u - 1]) / 2, (P[v + 1, u] + P[v - 1, u]) / 2
            bound = bound + (np.linalg.norm(P[v, u] - ma, axis=1) + np.linalg.norm(P[v, u] - mb, axis=1)) / (curvature * sin)
        err = np.linalg.norm(n[sel] - normal_of(P[v, u]), axis=1)
        assert sel.sum() > 50 and (err <= bound).all(), (err.max(), bound.min(), (err / bound).max())
        assert (np.sum(n[sel] * P[v, u], axis=1) < 0).all()        # facing the sensor at the origin


def test_a_slanted_plane_comes_back_with_its_normal():
    d = _rays()
    t = 1.0 / (1.0 - 0.2 * d[..., 0])                               # z = 1 + 0.2 x along the ray: t = 1 + 0.2 t d_x
    m = np.array([0.2, 0.0, -1.0]) / np.sqrt(1.04)                  # the plane's unit normal, towards the sensor
    _round_trip(t, np.ones((H, W), bool), lambda P: np.broadcast_to(m, P.shape), None)
    got = law.depth_law(t.astype(f32)[None], K, jump=(10.0, 0.0), w=0)
    assert np.abs((got["points"].astype(f64) @ [0.2, 0.0, -1.0]) + 1.0).max() <= 4 * EPS * np.abs(got["points"]).max() * np.sqrt(1.04)


def test_a_sphere_comes_back_with_its_normals():
    d, c, r = _rays(), np.array([0.05, -0.03, 2.0]), 0.5
    dd, dc = (d * d).sum(-1), d @ c
    disc = dc * dc - dd * (c @ c - r * r)
    hit = disc > 0
    t = (dc - np.sqrt(np.where(hit, disc, 0.0))) / dd
    _round_trip(t, hit, lambda P: (P - c) / r, r)
    got = law.depth_law(np.where(hit, t, 0.0).astype(f32)[None], K, jump=(10.0, 0.0), w=0)
    off = np.abs(np.linalg.norm(got["points"].astype(f64) - c, axis=1) - r)
    assert off.max() <= 4 * EPS * np.abs(got["points"]).max()

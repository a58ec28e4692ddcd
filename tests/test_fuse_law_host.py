"""CPU suite for the law of volumetric fusion (tests/fuse_law.py): the vectorised form that the GPU tests call against the
per-voxel loop in Python floats, bit for bit; the small cases worked by hand; and what the law is for — two noisy views of a
plane fuse to the plane, what one view records in free space is carved by the others, a slanted plane comes back within a bound
derived from the pixel footprint and the slope."""
import functools
import math

import numpy as np
import pytest

import depth_law
import fuse_law as law

f32, f64 = np.float32, np.float64
GRIDS = [(1, 1, 1), (1, 1, 70), (5, 3, 67), (33, 17, 9)]
SURFACE = ("offsets", "cell", "points", "normals")


def _bits(a):
    return a.view(np.uint32) if a.dtype == f32 else a


def _same(got, want, names, what):
    for name in names:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert (_bits(g) == _bits(w)).all(), (what, name)


def _rotation(q):
    w, x, y, z = np.asarray(q, f64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def _images(dtype):
    """Five images of 9 x 13 pixels on the 1/64 lattice about one place, image 0 through an axis-aligned pose on the lattice."""
    r = np.random.RandomState(3)
    B, H, W = 5, 9, 13
    depth = depth_law.lattice_images(17, B, H, W, dtype, holes=0.15)
    K = np.array([[12.0 + b, 11.5 + b, (W - 1) / 2 + 0.3 - 0.1 * b, (H - 1) / 2 - 0.7 + 0.1 * b] for b in range(B)])
    K[0] = [8.0, 8.0, (W - 1) / 2, (H - 1) / 2]
    R0, t0 = _rotation(r.standard_normal(4)), np.array([0.3, -1.25, 2.0])
    poses = np.stack([np.concatenate([R0 @ _rotation([1.0, *(0.04 * r.standard_normal(3))]), (t0 + 0.05 * r.standard_normal(3))[:, None]], 1)
                      for _ in range(B)])
    poses[0] = np.array([[0.0, 0, 1, 0.25], [1, 0, 0, -1.5], [0, 1, 0, 2.0]])
    masks = (r.rand(B, H, W) < 0.8).astype(np.uint8)
    return depth, K, poses.astype(f32), masks


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("dims", GRIDS, ids=str)
def test_the_two_forms_agree_bit_for_bit(dims, dtype):
    depth, K, poses, masks = _images(dtype)
    scale = 1 / 64 if dtype == np.uint16 else None
    observed = rows = 0
    for count in (1, 2, 5):
        groups = [list(range(count)), [count - 1]]
        pts = depth_law.depth_law(depth[:count], K[:count], poses[:count], scale=scale, w=0)["points"].astype(f64)
        lo, hi = pts.min(0) - 1 / 16, pts.max(0) + 1 / 16
        voxel = 2.0 ** math.ceil(math.log2(((hi - lo) / np.array(dims)).min()))
        lattice = max(64.0, 1 / voxel)
        origin = np.floor(((lo + hi) / 2 - np.array(dims) * voxel / 2) * lattice) / lattice
        for w, m in ((0, None), (1, masks), (1, None), (0, masks)):
            kw = dict(masks=m, scale=scale, near=1.0 + 1 / 64, far=1.0 + 44 / 64, jump=(1 / 64, 0.0), w=w)
            args = (depth, K, poses, groups, origin, dims, voxel, None if w else 3 * voxel)
            a, b = law.fuse_volume_law(*args, **kw), law.fuse_volume_law_loop(*args, **kw)
            _same(a, b, ("weight", "tsdf"), (count, w, m is not None))
            assert a["tsdf"].shape == (2, dims[2], dims[1], dims[0]) and a["weight"].dtype == np.int32
            observed += int(a["weight"].sum())
            for min_weight in (1, 2):
                sa = law.fuse_surface_law(a["tsdf"], a["weight"], origin, voxel, min_weight)
                _same(sa, law.fuse_surface_law_loop(a["tsdf"], a["weight"], origin, voxel, min_weight), SURFACE, (count, w, min_weight))
                rows += int(sa["offsets"][-1])
    assert observed > 0 and (rows > 0 or dims == (1, 1, 1))


@pytest.mark.parametrize("dims", GRIDS + [(70, 1, 1), (2, 2, 2)], ids=str)
def test_the_two_surface_forms_agree_on_dense_random_fields(dims):
    r = np.random.RandomState(sum(dims))
    nx, ny, nz = dims
    tsdf = (r.randint(-8, 9, (2, nz, ny, nx)) / 8.0).astype(f32)
    tsdf[r.rand(*tsdf.shape) < 0.1] = -0.0
    weight = r.randint(0, 4, tsdf.shape).astype(np.int32)
    origin = np.array([[0.1, -0.2, 0.3], [5.0, 6.0, -7.0]])
    for min_weight in (1, 2, 3):
        a = law.fuse_surface_law(tsdf, weight, origin, 0.0625, min_weight)
        _same(a, law.fuse_surface_law_loop(tsdf, weight, origin, 0.0625, min_weight), SURFACE, min_weight)
        assert (np.diff(a["cell"]) > 0).all() and a["offsets"][0] == 0 and a["offsets"][-1] == len(a["cell"])


# ---- by hand: one camera at the origin looking along +z, 4 x 4 pixels, fx = fy = 4, the optical axis between pixels 1 and 2 -------
K4 = (4.0, 4.0, 1.5, 1.5)
BOTH = (law.fuse_volume_law, law.fuse_volume_law_loop)


def _one_voxel(form, depth, centre, truncation, voxel=0.25, **kw):
    origin = np.asarray(centre, f64) - voxel / 2
    out = form(np.asarray(depth, f32)[None], K4, None, None, origin, (1, 1, 1), voxel, truncation, w=0, **kw)
    return float(out["tsdf"][0, 0, 0, 0]), int(out["weight"][0, 0, 0, 0])


@pytest.mark.parametrize("form", BOTH, ids=["vectorised", "loop"])
def test_hand_cases_of_the_volume(form):
    flat = np.full((4, 4), 2.0, f32)
    assert _one_voxel(form, flat, (0.125, 0.125, -1.0), 1.0) == (1.0, 0)           # behind the camera: q2 < 0
    assert _one_voxel(form, flat, (0.125, 0.125, 0.0), 1.0) == (1.0, 0)            # in its plane: q2 = 0 is not > 0
    assert _one_voxel(form, flat, (0.125, 0.125, 1.5), 1.0) == (0.5, 1)            # s = 0.5
    assert _one_voxel(form, flat, (0.125, 0.125, 3.0), 1.0) == (-1.0, 1)           # s = -truncation: kept, f = -1
    assert _one_voxel(form, flat, (0.125, 0.125, 3.0 + 2.0 ** -40), 1.0) == (1.0, 0)   # a hair behind it: says nothing
    assert _one_voxel(form, flat, (0.125, 0.125, 1.0), 1.0) == (1.0, 1)            # f exactly 1
    assert _one_voxel(form, flat, (0.125, 0.125, 0.5), 1.0) == (1.0, 1)            # f = 1.5, cut off at 1
    assert _one_voxel(form, flat, (0.125, 0.125, 0.5), 2.0) == (0.75, 1)           # ... and not with a longer truncation
    # the +0.5 tie: pixel centres are at integers, so x = (0 * 4) / 1 + 1.5 = 1.5 lies exactly on the border of pixels 1 and 2,
    # and u = floor(x + 0.5) = 2 sends it to the upper one
    steps = np.tile(np.array([1.0, 1.25, 1.5, 1.75], f32), (4, 1))
    assert _one_voxel(form, steps, (0.125, 0.0, 1.0), 1.0) == (0.5, 1)             # x = 2.0, a pixel's centre: u = 2, z = 1.5
    assert _one_voxel(form, steps, (0.125 - 2.0 ** -30, 0.0, 1.0), 1.0) == (0.5, 1)    # x + 0.5 just below 2.5 still floors to 2
    assert _one_voxel(form, steps, (0.0, 0.0, 1.0), 1.0) == (0.5, 1)               # x = 1.5, the border: u = floor(2.0) = 2
    assert _one_voxel(form, steps, (-2.0 ** -30, 0.0, 1.0), 1.0) == (0.25, 1)      # a hair to the left: u = 1, z = 1.25
    assert _one_voxel(form, steps, (-0.5, 0.0, 1.0), 1.0) == (0.0, 1)              # x = -0.5: u = floor(0.0) = 0, the first column
    assert _one_voxel(form, steps, (-0.5 - 2.0 ** -30, 0.0, 1.0), 1.0) == (1.0, 0)     # ... and outside beyond it
    assert _one_voxel(form, steps, (0.5 - 2.0 ** -30, 0.0, 1.0), 1.0) == (0.75, 1)     # u = 3, the last column
    assert _one_voxel(form, steps, (0.5, 0.0, 1.0), 1.0) == (1.0, 0)               # x = 3.5: u = 4 is outside
    # a pixel that is not kept says nothing: a hole, out of range, masked out
    holes = flat.copy()
    holes[1:3, 1:3] = 0.0
    assert _one_voxel(form, holes, (0.125, 0.125, 1.5), 1.0) == (1.0, 0)
    assert _one_voxel(form, flat, (0.125, 0.125, 1.5), 1.0, near=2.5) == (1.0, 0)
    mask = np.ones((1, 4, 4), np.uint8)
    mask[0, 2, 2] = 0
    assert _one_voxel(form, flat, (0.125, 0.125, 1.5), 1.0, masks=mask) == (1.0, 0)
    # two images, the same pose: the average of 0.5 and -0.25, in list order, weight 2
    two = form(np.stack([flat, np.full((4, 4), 1.25, f32)]), K4, depth_law.IDENTITY, [[0, 1], [1]], [0.0, 0.0, 1.375], (1, 1, 1), 0.25,
               1.0, w=0)
    assert two["tsdf"].ravel().tolist() == [0.125, -0.25] and two["weight"].ravel().tolist() == [2, 1]


SURFACES = (law.fuse_surface_law, law.fuse_surface_law_loop)


@pytest.mark.parametrize("form", SURFACES, ids=["vectorised", "loop"])
def test_hand_cases_of_the_surface(form):
    line = lambda values: np.asarray(values, f32).reshape(1, 1, 1, -1)
    ones = lambda t: np.ones(t.shape, np.int32)
    # fa = 0 against fb < 0: 0 is not negative, so there is a row, with t = 0, at a's centre
    t = line([0.5, 0.0, -0.5])
    s = form(t, ones(t), [0.0, 0.0, 0.0], 0.5)
    assert s["cell"].tolist() == [3] and s["points"].tolist() == [[0.75, 0.25, 0.25]] and s["offsets"].tolist() == [0, 1]
    assert s["normals"].tolist() == [[-1.0, 0.0, 0.0]]                              # the field falls along +x: free space is at -x
    # -0.0 is not negative either; fa < 0 against fb = 0 gives t = 1, the row at b's centre
    s = form(line([-0.5, -0.0, 0.5]), ones(t), [0.0, 0.0, 0.0], 0.5)
    assert s["cell"].tolist() == [0] and s["points"].tolist() == [[0.75, 0.25, 0.25]] and s["normals"].tolist() == [[1.0, 0.0, 0.0]]
    # t = fa / (fa - fb) = 0.25 / 1 between the centres 0.25 and 0.75
    s = form(line([0.25, -0.75]), np.ones((1, 1, 1, 2), np.int32), [0.0, 0.0, 0.0], 0.5)
    assert s["points"].tolist() == [[0.375, 0.25, 0.25]]
    # an unobserved neighbour in the gradient takes the centre's value: g(a) = f(b) - f(a) where a's lower neighbour is unusable
    t, w = line([9.0, 0.5, -0.5, -0.75]), np.array([0, 1, 1, 1], np.int32).reshape(1, 1, 1, 4)
    s = form(t, w, [0.0, 0.0, 0.0], 1.0)
    assert s["cell"].tolist() == [3] and s["normals"].tolist() == [[-1.0, 0.0, 0.0]]
    # ... along y, where the slope counts: g_y(a) = 0.5 - 0.25 with the lower side unusable, g_y(b) = -0.5 - -0.5 = 0
    t = np.asarray([[[0.25, -0.5]], [[0.5, -0.5]]], f32).reshape(1, 1, 2, 2)           # (nz, ny, nx) = (1, 2, 2)
    s = form(t, np.ones(t.shape, np.int32), [0.0, 0.0, 0.0], 1.0)
    assert s["cell"].tolist() == [0, 6]
    ta = 0.25 / 0.75
    m = [(-0.5 - 0.25) + ta * ((-0.5 - 0.25) - (-0.5 - 0.25)), (0.5 - 0.25) + ta * (0.0 - (0.5 - 0.25)), 0.0]
    l = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    assert s["normals"][0].tolist() == [f32(m[0] / l), f32(m[1] / l), 0.0] and s["points"][0].tolist() == [f32(0.5 + ta), 0.5, 0.5]
    # min_weight 2: a voxel seen once is neither an end of a row nor a side of a gradient
    t, w = line([0.5, -0.5, 0.5, -0.5, -1.0]), np.array([2, 2, 1, 2, 2], np.int32).reshape(1, 1, 1, 5)
    assert form(t, w, [0.0, 0.0, 0.0], 1.0, 1)["cell"].tolist() == [0, 3, 6]
    s = form(t, w, [0.0, 0.0, 0.0], 1.0, 2)
    assert s["cell"].tolist() == [0] and form(t, w, [0.0, 0.0, 0.0], 1.0, 3)["cell"].tolist() == []
    # no usable difference at all: the normal is zero, the row stays
    t = np.asarray([0.5, -0.5], f32).reshape(1, 2, 1, 1)                              # along z
    s = form(t, np.ones(t.shape, np.int32), [1.0, 2.0, 3.0], 2.0)
    assert s["cell"].tolist() == [2] and s["points"].tolist() == [[2.0, 3.0, 5.0]] and s["normals"].tolist() == [[0.0, 0.0, -1.0]]
    # order: group, k, j, i, then axis; two groups
    t = np.asarray([[[[-1.0, 1.0], [1.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]]]] * 2, f32)
    s = form(t, np.ones(t.shape, np.int32), [[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]], 1.0)
    assert s["cell"].tolist() == [0, 1, 2, 24, 25, 26] and s["offsets"].tolist() == [0, 3, 6]
    assert s["points"][:3].tolist() == [[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0]] and s["points"][3].tolist() == [11.0, 0.5, 0.5]


def test_fuse_grid():
    origin, dims = law.fuse_grid([0.0, 1.0, 2.0], [1.0, 1.0, 2.26], 0.25, 0.5)
    assert origin.tolist() == [[-0.5, 0.5, 1.5]] and dims == (8, 4, 6)               # ceil(2 / .25), ceil(1 / .25), ceil(1.26 / .25)
    origin, dims = law.fuse_grid([[0.0, 0.0, 0.0], [5.0, 5.0, 5.0]], [[1.0, 0.0, 0.0], [5.0, 7.0, 5.0]], 0.5, 0.25)
    assert origin.tolist() == [[-0.25] * 3, [4.75] * 3] and dims == (3, 5, 1)        # the maximum over the groups, per axis
    assert law.fuse_grid([0.0] * 3, [0.0] * 3, 1.0, 1e-3)[1] == (1, 1, 1)


# ---- what the law is for ---------------------------------------------------------------------------------------------------------
def test_two_noisy_views_of_a_plane_fuse_to_the_plane():
    """Two frontal images of the plane z = z0, recorded at z0 + delta and z0 - delta — both exact in fp32 —, fuse to rows at z0.
    With s_i = z_i - c, f_i = s_i / T and F = (f_1 + f_2) / 2 the field is (z0 - c) / T up to the roundings of the two kinds of
    division: f = s / T and F / n and the cast are exact here (T a power of two, every value on a lattice of few bits), so fa and
    fb are exact and t = fa / (fa - fb) carries the one rounding of its division, relative 2^-53; the point c + t * voxel adds
    one fp64 rounding and the cast to fp32 half an ulp of fp32 at 1.  |z - z0| <= 2^-24 + 4 * 2^-53."""
    z0, delta, voxel = 1.0, 2.0 ** -7, 2.0 ** -5
    depth = np.stack([np.full((24, 32), z0 + delta, f32), np.full((24, 32), z0 - delta, f32)])
    assert float(depth[0, 0, 0]) - z0 == delta and z0 - float(depth[1, 0, 0]) == delta
    K = (30.0, 30.0, 15.5, 11.5)
    origin, dims = law.fuse_grid([-0.2, -0.15, z0 - delta], [0.2, 0.15, z0 + delta], voxel, 4 * voxel)
    origin = origin + np.array([0.0, 0.0, 0.3 * voxel])                               # the plane off the voxel centres and borders
    vol = law.fuse_volume_law(depth, K, depth_law.IDENTITY, [[0, 1], [0], [1]], origin, dims, voxel)
    s = law.fuse_surface_law(vol["tsdf"], vol["weight"], origin, voxel)
    o = s["offsets"]
    fused, far_one, near_one = s["points"][o[0]:o[1]], s["points"][o[1]:o[2]], s["points"][o[2]:o[3]]
    assert len(fused) > 100 and (s["cell"] % 3 == 2).all()                            # crossings along z only
    bound = 2.0 ** -24 + 4 * 2.0 ** -53
    assert np.abs(fused[:, 2].astype(f64) - z0).max() <= bound
    assert np.abs(far_one[:, 2].astype(f64) - (z0 + delta)).max() <= bound and np.abs(near_one[:, 2].astype(f64) - (z0 - delta)).max() <= bound
    n = s["normals"][o[0]:o[1]]
    assert (n == np.array([0.0, 0.0, -1.0], f32)).all()                               # towards the sensor, free space
    assert (vol["weight"][0] == 2).sum() > 0 and set(np.unique(vol["weight"][0])) <= {0, 2}


@functools.lru_cache(maxsize=None)
def _wall_and_blob():
    """A wall z = 1 seen by three cameras; the first also records a blob 0.4 in front of it that is not there."""
    H, W = 48, 64
    K = (60.0, 60.0, (W - 1) / 2, (H - 1) / 2)
    poses = np.stack([law.look_at(eye, (0.0, 0.0, 1.0), up=(0.0, -1.0, 0.0)) for eye in ((0.0, 0.0, 0.0), (0.35, 0.0, 0.05), (-0.3, 0.1, 0.0))])
    depth = np.stack([law.render(p, K, H, W, planes=[((0.0, 0.0, 1.0), 1.0)]) for p in poses]).astype(f32)
    depth[0, 18:30, 26:38] = 0.6
    return depth, K, poses


def test_what_one_view_records_in_free_space_is_carved_by_the_others():
    depth, K, poses = _wall_and_blob()
    voxel = 1 / 64
    truncation = 4 * voxel
    origin, dims = law.fuse_grid([-0.25, -0.2, 0.5], [0.25, 0.2, 1.0], voxel, truncation)
    vol = law.fuse_volume_law(depth, K, poses, [[0], [0, 1, 2]], origin, dims, voxel, truncation)
    s = law.fuse_surface_law(vol["tsdf"], vol["weight"], origin, voxel)
    alone, fused = s["points"][:s["offsets"][1]], s["points"][s["offsets"][1]:]
    assert (alone[:, 2] < 0.8).sum() > 0                                              # the blob's face, fused alone
    assert len(fused) > 1000 and (fused[:, 2] < 0.8).sum() == 0                       # seen through twice: (f + 1 + 1) / 3 > 0
    assert fused[:, 2].min() >= 1.0 - truncation                                      # nothing nearer than the wall's band


def test_a_slanted_plane_comes_back_within_a_derived_bound():
    """One view of the plane n . p = o, rendered analytically to fp32 depth.  With r = o - n . c, linear in the voxel centre c,
    the exact field is s(c) = kappa(c) r(c), kappa = c_z / (n . c) > 0.  The law reads the depth of the nearest pixel, not of c's
    own ray: the two are at most half a pixel apart along u and v, and the plane's depth changes by |dz/du| = z^2 |n_x| / (o fx)
    a pixel (dz/dv likewise), so the computed s is kappa (r + d) with |d| <= eps = (half-pixel change + roundings) / kappa_min.
    Over one grid edge kappa changes by the relative eta at most, which moves fb by eta (|D| + eps) more, D = r_a - r_b.  From
    t = (r_a + d_a) / (D + d_a - d_b), the row's residual is r_a - t D = (r_a (d_a - d_b) - D d_a) / (D + d_a - d_b), at most
    (|r_a| 2 e + |D| e) / (|D| - 2 e) with |r_a| <= |D| + e; and since the row lies between two voxels on either side of the
    computed zero it is never more than |D| + e.  The smaller of the two, over |n|, bounds the distance to the plane."""
    n, o = np.array([0.3, -0.2, 1.0]), 1.1
    H, W = 240, 320
    K = (400.0, 400.0, (W - 1) / 2, (H - 1) / 2)
    depth = law.render(depth_law.IDENTITY, K, H, W, planes=[(n, o)]).astype(f32)[None]
    voxel = 1 / 64
    truncation = 4 * voxel
    pts = depth_law.depth_law(depth, K)["points"].astype(f64)
    origin, dims = law.fuse_grid(pts.min(0), pts.max(0), voxel, truncation)
    vol = law.fuse_volume_law(depth, K, depth_law.IDENTITY, None, origin, dims, voxel, truncation)
    s = law.fuse_surface_law(vol["tsdf"], vol["weight"], origin, voxel)
    p = s["points"].astype(f64)
    assert len(p) > 3000
    zmin, zmax = float(depth.min()) - truncation - voxel, float(depth.max()) + truncation + voxel    # where observed voxels lie
    nc_min = o - np.abs(n).sum() * (truncation + voxel) * zmax / zmin                 # n . c of a voxel within the band, generously
    kappa_min, kappa_max = zmin / (o + (o - nc_min)), zmax / nc_min
    z_hi = 1.02 * float(depth.max())              # half a pixel beyond the border: the depth changes by less than 0.3 % a pixel
    half_pixel = 0.5 * z_hi * z_hi * (abs(n[0]) / K[0] + abs(n[1]) / K[1]) / o
    rounding = 2.0 ** -24 * zmax + 2.0 ** -24 * truncation                            # the fp32 depth, the fp32 field
    eps = (half_pixel + rounding) / kappa_min
    eta = voxel / zmin + voxel * np.abs(n).max() / nc_min
    residual = np.abs(o - p @ n)
    axis = s["cell"] % 3
    worst = 0.0
    for e in range(3):
        D = voxel * abs(n[e])
        e_b = eps + eta * (D + 2 * eps)
        fine = ((D + e_b) * 2 * e_b + D * e_b) / (D - 2 * e_b) if D > 2 * e_b else np.inf
        bound = min(fine, D + e_b) + 2.0 ** -24 * 3 * zmax                            # ... and the cast of the point
        assert residual[axis == e].max() <= bound, (e, residual[axis == e].max(), bound)
        worst = max(worst, bound)
    assert worst / np.linalg.norm(n) < voxel                                          # the bound says something: within a voxel
    # the normals: along n, into free space (towards the camera: n . normal < 0 as the plane faces -z)
    cos = s["normals"].astype(f64) @ (-n / np.linalg.norm(n))
    assert np.median(cos) > 0.99 and (cos > 0).all()
    assert kappa_max >= kappa_min > 0

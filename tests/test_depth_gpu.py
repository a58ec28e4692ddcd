"""GPU suite for the depth-image kernels (csrc/depth.hip): points, normals, pixel and offsets of ops.depth_points bit for bit
against tests/depth_law.py — a sweep of image shapes from one pixel to several chunks an image over windows, both depth types
and masks, on depths of a 1/64 lattice where ties of the jump test occur; a scan pass of two rounds; empty and full images;
every kind of hole; jumps at the border; poses and per-image intrinsics; reused buffers, the sentinel beyond offsets[B],
repeatability; and one batch of real-size images."""
import functools

import numpy as np
import pytest
import torch

import depth_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32 = np.float32
SENTINEL = -7.5
K0 = (40.0, 37.5, 3.3, 1.7)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(CUDA)


def _run(depth, K, poses=None, masks=None, scale=None, near=0.0, far=np.inf, jump=(0.0, 0.05), w=1, bufs=None):
    """ops.depth_points on buffers filled with a sentinel -> (numpy dict trimmed to offsets[B], the buffers)."""
    from hyperpocket_amd import ops
    B, H, W = depth.shape
    if bufs is None:
        bufs = ops.depth_points_buffers(B, H, W, CUDA)
    for name in ("points", "normals", "pixel"):
        bufs[name].fill_(SENTINEL if name != "pixel" else -7)
    res = ops.depth_points(_dev(depth), K, poses=poses, masks=None if masks is None else _dev(masks), depth_scale=scale, near=near,
                           far=far, jump=jump, window=w, out=bufs, ws=bufs["ws"])
    assert res is bufs
    T = int(res["offsets"][-1])
    for name, fill in (("points", SENTINEL), ("normals", SENTINEL), ("pixel", -7)):
        assert res[name].shape[0] == B * H * W and bool((res[name][T:] == fill).all()), name      # never written beyond offsets[B]
    got = {name: res[name][:T].cpu().numpy() for name in ("points", "normals", "pixel")}
    got["offsets"] = res["offsets"].cpu().numpy()
    return got, bufs


def _bits(a):
    return a.view(np.uint32) if a.dtype == f32 else a              # signed zeros count


def _same(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in ("offsets", "pixel", "points", "normals"):
        g, w = got[name], np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        wrong = np.argwhere(_bits(g) != _bits(w))
        assert len(wrong) == 0, (what, name, len(wrong), wrong[0].tolist(), g[tuple(wrong[0])], w[tuple(wrong[0])])


def _check(depth, K, what=None, bufs=None, **kw):
    got, bufs = _run(depth, K, bufs=bufs, **kw)
    _same(got, law.depth_law(depth, K, **kw), what)
    return got, bufs


def _pose(seed):
    q = np.random.RandomState(seed).standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return np.concatenate([np.array(R), [[0.3], [-1.25], [2.0]]], 1).astype(f32)


@functools.lru_cache(maxsize=None)
def _several_chunks():
    """The sweep's largest shape: 130 x 70 when that spans several chunks an image, else the smallest shape of 70 columns that does."""
    from hyperpocket_amd import ops
    threads, per_lane, chunks, _, _ = ops.depth_points_plan(3, 130, 70)
    if chunks > 1:
        return (130, 70)
    return (-(-(2 * threads * per_lane + 1) // 70), 70)


# ---- the sweep: B = 3 images on the 1/64 lattice, per-image intrinsics off the pixel grid and real poses ---------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (67, 3), (33, 65), "several chunks"], ids=str)
def test_shape_sweep(shape, dtype):
    from hyperpocket_amd import ops
    H, W = _several_chunks() if shape == "several chunks" else shape
    B = 3
    if shape == "several chunks":
        assert ops.depth_points_plan(B, H, W)[2] > 1
    depth = law.lattice_images(H * 100 + W, B, H, W, dtype)
    scale = 1 / 64 if dtype == np.uint16 else None
    K = np.array([[40.0, 37.5, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.7], [55.25, 60.0, W / 3, H / 1.7], [31.0, 29.5, 0.25, H + 2.5]])
    poses = np.stack([_pose(1), _pose(2), _pose(3)])
    masks = (np.random.RandomState(5).rand(B, H, W) < 0.8).astype(np.uint8)
    bufs, kept = None, 0
    for w in (0, 1, 2, 4):
        for m, jump in ((masks, (1 / 64, 0.0)), (None, (1 / 128, 1 / 32))):
            got, bufs = _check(depth, K, what=(H, W, w, m is not None), bufs=bufs, poses=poses, masks=m, scale=scale,
                               near=1.0 + 1 / 64, far=1.0 + 40 / 64, jump=jump, w=w)
            kept += int(got["offsets"][-1])
    assert kept > 0


def test_the_scan_pass_takes_a_second_round():
    """The smallest number of chunks beyond one round of the scan pass: images of one pixel, one chunk each."""
    from hyperpocket_amd import ops
    _, _, chunks, scan_threads, rounds = ops.depth_points_plan(1, 1, 1)
    assert chunks == 1 and rounds == 1
    B = scan_threads + 1
    assert ops.depth_points_plan(B, 1, 1)[4] == 2 and ops.depth_points_plan(B - 1, 1, 1)[4] == 1
    depth = law.lattice_images(11, B, 1, 1, np.uint16, holes=0.3)
    got, _ = _check(depth, K0, what="two rounds", scale=1 / 64, w=1)
    assert 0 < got["offsets"][-1] < B
    # ... and chunks of several images in both rounds
    H, W = 40, 60
    per = ops.depth_points_plan(1, H, W)[2]
    B = scan_threads // per + 2
    depth = law.lattice_images(12, B, H, W, np.uint16)
    assert ops.depth_points_plan(B, H, W)[4] == 2
    _check(depth, K0, what="two rounds of larger images", scale=1 / 64, jump=(1 / 64, 0.0), w=1)


def test_an_image_that_keeps_nothing_and_images_that_keep_all():
    depth = law.lattice_images(21, 3, 33, 65, np.uint16, holes=0.1)
    depth[1] = 0
    got, _ = _check(depth, K0, what="the middle image is empty", scale=1 / 64, jump=(1 / 64, 0.0), w=1)
    assert got["offsets"][1] == got["offsets"][2] and 0 < got["offsets"][1] < got["offsets"][3]
    full = np.full((3, 33, 65), 1500, np.uint16)
    got, _ = _check(full, K0, what="all kept", w=4)
    assert got["offsets"].tolist() == [0, 2145, 4290, 6435] and (got["pixel"] == np.arange(6435)).all()
    assert (_bits(got["normals"]) == _bits(np.tile(np.array([-0.0, -0.0, -1.0], f32), (6435, 1)))).all()
    got, _ = _check(np.zeros((2, 5, 7), f32), K0, what="nothing at all")
    assert got["offsets"].tolist() == [0, 0, 0]


def test_every_kind_of_hole():
    depth = law.lattice_images(31, 2, 33, 65, np.float32, holes=0.3)
    depth[0, 0, :7] = [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45]   # the last is measured: the smallest depth there is
    for w in (0, 1):
        got, _ = _check(depth, K0, what=("holes", w), jump=(1 / 64, 0.0), w=w)
    meas = np.isfinite(depth) & (depth > 0)
    got, _ = _check(depth, K0, what="holes, no edge test", jump=(1 / 64, 0.0), w=0)
    assert got["offsets"][-1] == meas.sum() and 6 in got["pixel"] and not set(range(6)) & set(got["pixel"].tolist())


def test_jumps_at_the_border_and_in_the_corner():
    depth = np.full((2, 9, 11), 1.0, f32)
    depth[0, 0, 0] = depth[0, 8, 10] = depth[0, 0, 10] = depth[0, 8, 0] = 2.0          # the corners
    depth[1, 0, 5] = depth[1, 8, 5] = depth[1, 4, 0] = depth[1, 4, 10] = 2.0            # the borders
    for w in (1, 2, 4):
        _check(depth, K0, what=("border", w), w=w)
    got, _ = _check(depth, K0, what="border, window 1", w=1)
    assert got["offsets"].tolist() == [0, 99 - 4 * 4, 2 * 99 - 4 * 4 - 4 * 6]


def test_poses_and_intrinsics():
    depth = law.lattice_images(41, 2, 20, 30, np.uint16, holes=0.05)
    kw = dict(scale=1 / 64, jump=(1 / 64, 0.0), w=1)
    K2 = np.array([[40.0, 37.5, 14.2, 9.9], [25.0, 80.0, -3.0, 40.0]])
    cam, _ = _check(depth, K0, what="camera frame", **kw)
    one, _ = _check(depth, K0, what="one pose for all", poses=_pose(7), **kw)
    two, _ = _check(depth, K2, what="per image", poses=np.stack([_pose(8), _pose(9)]), **kw)
    assert (cam["pixel"] == one["pixel"]).all() and (cam["pixel"] == two["pixel"]).all()
    assert not (cam["points"] == one["points"]).all() and not (one["normals"] == two["normals"]).all()
    # 4x4 matrices give what their upper rows give
    from hyperpocket_amd import ops
    M = np.concatenate([_pose(7), [[0, 0, 0, 1]]]).astype(f32)
    res = ops.depth_points(_dev(depth), torch.tensor(K0, dtype=torch.float64), poses=torch.from_numpy(M), depth_scale=1 / 64, jump=(1 / 64, 0.0))
    T = int(res["offsets"][-1])
    assert (_bits(res["points"][:T].cpu().numpy()) == _bits(one["points"])).all()
    assert (_bits(res["normals"][:T].cpu().numpy()) == _bits(one["normals"])).all()


def test_tables_prepared_on_the_device():
    """depth_points_tables' tensors are taken as they are and give the same bits; any other device tensor is refused."""
    from hyperpocket_amd import ops
    depth = law.lattice_images(43, 2, 20, 30, np.uint16, holes=0.05)
    K2 = np.array([[40.0, 37.5, 14.2, 9.9], [25.0, 80.0, -3.0, 40.0]])
    poses = np.stack([_pose(8), _pose(9)])
    want = law.depth_law(depth, K2, poses, scale=1 / 64, jump=(1 / 64, 0.0))
    Kd, Md = ops.depth_points_tables(2, K2, poses, CUDA)
    assert Kd.is_cuda and Kd.dtype == torch.float64 and Md.is_cuda and Md.dtype == torch.float32 and Md.shape == (2, 3, 4)
    d = _dev(depth)
    res = ops.depth_points(d, Kd, poses=Md, depth_scale=1 / 64, jump=(1 / 64, 0.0))
    T = int(res["offsets"][-1])
    got = {name: res[name][:T].cpu().numpy() for name in ("points", "normals", "pixel")}
    got["offsets"] = res["offsets"].cpu().numpy()
    _same(got, want, "prepared tables")
    for bad in (dict(intrinsics=Kd.float()), dict(intrinsics=Kd[:1]), dict(intrinsics=Kd.t().contiguous().t()),
                dict(poses=Md.double()), dict(poses=Md[0]), dict(poses=torch.eye(4, device=CUDA))):
        with pytest.raises(ValueError, match="depth_points_tables"):
            ops.depth_points(d, **{"intrinsics": Kd, "poses": Md, **bad})


def test_buffers_are_reused_and_two_runs_give_the_same_bits():
    a = law.lattice_images(51, 3, 33, 65, np.float32, holes=0.1)
    b = law.lattice_images(52, 3, 33, 65, np.float32, holes=0.6)   # fewer rows than the call before left behind
    kw = dict(jump=(1 / 64, 0.0), w=2, poses=_pose(4))
    first, bufs = _check(a, K0, what="first use", **kw)
    second, again = _check(b, K0, what="second use", bufs=bufs, **kw)
    assert again is bufs and second["offsets"][-1] < first["offsets"][-1]
    third, _ = _run(a, K0, bufs=bufs, **kw)
    _same(third, first, "two runs")
    fresh, _ = _run(a, K0, **kw)
    _same(fresh, first, "fresh buffers")


@functools.lru_cache(maxsize=None)
def _real_size():
    s = law.scene(0, 2, 480, 640)
    return s, law.depth_law(s["depth"], s["K"], s["poses"], s["masks"])


def test_real_size_images():
    s, want = _real_size()
    got, _ = _run(s["depth"], s["K"], poses=s["poses"], masks=s["masks"])
    _same(got, want, "2 x 480 x 640")
    assert 0.5 * s["depth"].size < got["offsets"][-1] < s["depth"].size

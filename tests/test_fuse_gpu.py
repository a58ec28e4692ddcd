"""GPU suite for the fusion kernels (csrc/fuse.hip): tsdf and weight of ops.fuse_volume, points, normals, cell and offsets of
ops.fuse_surface bit for bit against tests/fuse_law.py — three groups of 1, 2 and 5 images with one image shared and one in no
group, images of 33 x 65 pixels and of one, depths on a 1/64 lattice with holes and masks, real rotations next to an axis-aligned
pose on the lattice (where s = -truncation and f = 1 are met exactly), per-image intrinsics, grids from one voxel to more chunks
than one round of the scan pass takes, a volume where nothing is observed; dense random fields through the surface pass alone;
min_weight 1 and 2, capacities below the total, of zero and beyond it, reused buffers, prepared tables, repeatability."""
import functools

import numpy as np
import pytest
import torch

import depth_law
import fuse_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32, f64 = np.float32, np.float64
SENTINEL = -7.5
GROUPS = [[0], [1, 2], [2, 3, 4, 5, 6]]                    # image 2 serves two groups, image 7 none
GRIDS = [(1, 1, 1), (1, 1, 70), (5, 3, 67), (33, 17, 9)]
LARGE = (102, 101, 102)                                    # more than 1024 chunks: the scan pass takes a second round


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(CUDA)


def _bits(a):
    return a.view(np.uint32) if a.dtype == f32 else a      # signed zeros count


def _same(got, want, names, what):
    for name in names:
        g, w = got[name], np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        wrong = np.argwhere(_bits(g) != _bits(w))
        assert len(wrong) == 0, (what, name, len(wrong), wrong[0].tolist(), g[tuple(wrong[0])], w[tuple(wrong[0])])


def _rotation(q):
    w, x, y, z = np.asarray(q, f64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@functools.lru_cache(maxsize=None)
def _images(H, W, dtype):
    """Eight images about one place: image 0 through an axis-aligned pose whose translation lies on the 1/64 lattice, the others
    through real rotations a few degrees apart.  -> dict of depth, K (8,4), poses (8,3,4) float32, masks, the depth keywords and
    the world points of every image by the depth law."""
    r = np.random.RandomState(H * 100 + W)
    B = 8
    depth = depth_law.lattice_images(H * 7 + W, B, H, W, dtype, holes=0.15 if H * W > 1 else 0.0)
    K = np.array([[40.0 + 3 * b, 37.5 + 2 * b, (W - 1) / 2 + 0.3 - 0.1 * b, (H - 1) / 2 - 0.7 + 0.1 * b] for b in range(B)])
    K[0] = [32.0, 32.0, (W - 1) / 2, (H - 1) / 2]
    R0, t0 = _rotation(r.standard_normal(4)), np.array([0.3, -1.25, 2.0])
    poses = np.stack([np.concatenate([R0 @ _rotation([1.0, *(0.04 * r.standard_normal(3))]), (t0 + 0.05 * r.standard_normal(3))[:, None]], 1)
                      for _ in range(B)])
    poses[0] = np.array([[0.0, 0, 1, 0.25], [1, 0, 0, -1.5], [0, 1, 0, 2.0]])   # camera x, y, z along world y, z, x
    poses = poses.astype(f32)
    masks = np.ones((B, H, W), np.uint8)
    masks[1::2] = r.rand(len(masks[1::2]), H, W) < 0.8                           # every other image has a real mask
    kw = dict(masks=masks, scale=1 / 64 if dtype == np.uint16 else None, near=1.0 + 1 / 64, far=1.0 + 44 / 64, jump=(1 / 64, 0.0), w=1)
    rows = depth_law.depth_law(depth, K, poses, **kw)
    return {"depth": depth, "K": K, "poses": poses, "kw": kw, "points": rows["points"].astype(f64), "offsets": rows["offsets"]}


@functools.lru_cache(maxsize=None)
def _case(H, W, dtype, dims):
    """The images and three volumes of `dims` voxels: each group's about the middle of its images' points, its origin on the
    lattice of the depths (of the voxels where they are finer) and the voxel the power of two at which the grid's tightest axis spans the points, but for one
    group — which one goes round with the grids — whose volume lies behind every camera.  The voxel is a power of two, the
    truncation 3 or 4 voxels.  -> (the case, the law's volume, the law's surface at min_weight 1 and 2)."""
    im = _images(H, W, dtype)
    pad, away = 1 / 16, (GRIDS + [LARGE]).index(dims) % 3
    boxes = []
    for g, images in enumerate(GROUPS):
        pts = np.concatenate([im["points"][im["offsets"][b]:im["offsets"][b + 1]] for b in images])
        if len(pts) == 0:
            pts = im["points"] if len(im["points"]) else im["poses"][images, :, 3].astype(f64)
        boxes.append((pts.min(0) - pad, pts.max(0) + pad))
    voxel = 2.0 ** math_ceil_log2(min(((hi - lo) / np.array(dims)).min() for lo, hi in boxes))
    lattice = max(64.0, 1 / voxel)
    origin = np.stack([np.floor(((lo + hi) / 2 - np.array(dims) * voxel / 2) * lattice) / lattice for lo, hi in boxes])
    origin[away] = im["poses"][GROUPS[away][0], :, 3].astype(f64) - 1000.0 * im["poses"][GROUPS[away][0], :, 2].astype(f64)
    case = dict(im, groups=GROUPS, origin=origin, dims=dims, voxel=voxel, truncation=None if sum(dims) % 2 else 3 * voxel, away=away)
    volume = law.fuse_volume_law(im["depth"], im["K"], im["poses"], GROUPS, origin, dims, voxel, case["truncation"], **im["kw"])
    surfaces = {m: law.fuse_surface_law(volume["tsdf"], volume["weight"], origin, voxel, m) for m in (1, 2)}
    return case, volume, surfaces


def math_ceil_log2(x):
    return int(np.ceil(np.log2(x)))


def _volume(case, out=None, tables=None):
    from hyperpocket_amd import ops
    kw = case["kw"]
    K, M, origin = tables if tables is not None else (case["K"], case["poses"], case["origin"])
    return ops.fuse_volume(_dev(case["depth"]), K, M, case["groups"], origin, case["dims"], case["voxel"], case["truncation"],
                           masks=_dev(kw["masks"]), depth_scale=kw["scale"], near=kw["near"], far=kw["far"], jump=kw["jump"],
                           window=kw["w"], out=out, ws=None if out is None else out["ws"])


def _host(res, names, rows=None):
    return {name: (res[name] if rows is None or name == "offsets" else res[name][:rows]).cpu().numpy() for name in names}


SURFACE = ("offsets", "cell", "points", "normals")


def _check_case(H, W, dtype, dims):
    from hyperpocket_amd import ops
    case, want, surfaces = _case(H, W, dtype, dims)
    vol = _volume(case)
    assert vol["dims"] == dims and vol["voxel"] == case["voxel"] and vol["truncation"] == (case["truncation"] or 4 * case["voxel"])
    _same(_host(vol, ("weight", "tsdf")), want, ("weight", "tsdf"), (H, W, dims))
    for m in (1, 2):
        got = _host(ops.fuse_surface(vol, min_weight=m), SURFACE)
        _same(got, surfaces[m], SURFACE, (H, W, dims, m))
        assert got["offsets"][case["away"]] == got["offsets"][case["away"] + 1]            # nothing observed there: an empty scan
        assert got["points"].shape[0] == got["offsets"][-1]
    return want, surfaces


@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["uint16", "float32"])
@pytest.mark.parametrize("dims", GRIDS, ids=str)
@pytest.mark.parametrize("shape", [(33, 65), (1, 1)], ids=str)
def test_volume_and_surface_sweep(shape, dims, dtype):
    want, surfaces = _check_case(*shape, dtype, dims)
    if shape == (33, 65) and dims == (33, 17, 9):
        w = want["weight"]
        assert w[1].max() == 2 and w[2].max() == 5 and (w[2] == 1).any() and (want["tsdf"] < 0).any()
        assert surfaces[1]["offsets"][-1] > surfaces[2]["offsets"][-1] > 0
    if shape == (33, 65) and dims == (5, 3, 67):
        assert (want["tsdf"][0] == -1.0).any() and (want["tsdf"][0] == 1.0).any()           # s = -truncation, met on the lattice


def test_more_chunks_than_a_round_of_the_scan_pass():
    from hyperpocket_amd import ops
    _, _, chunks, scan_threads, rounds = ops.fuse_surface_plan(3, LARGE)
    assert chunks > scan_threads and rounds >= 2
    want, surfaces = _check_case(33, 65, np.uint16, LARGE)
    w = want["weight"]
    assert w[0].max() == 1 and w[2].max() == 5
    assert surfaces[1]["offsets"][-1] > 3 * 1024 and surfaces[1]["offsets"][1] > 0 == surfaces[2]["offsets"][1]


@functools.lru_cache(maxsize=None)
def _field(dims, seed):
    """A dense random field and weights 0 .. 3: crossings at most voxels, exact zeros of both signs."""
    r = np.random.RandomState(seed)
    nx, ny, nz = dims
    tsdf = (r.randint(-8, 9, (2, nz, ny, nx)) / 8.0).astype(f32)
    tsdf[r.rand(*tsdf.shape) < 0.1] = -0.0
    weight = r.randint(0, 4, tsdf.shape).astype(np.int32)
    origin = np.array([[0.1, -0.2, 0.3], [5.0, 6.0, -7.0]])
    return tsdf, weight, origin, 0.0625, {m: law.fuse_surface_law(tsdf, weight, origin, 0.0625, m) for m in (1, 2)}


def _as_volume(tsdf, weight, origin, voxel):
    return {"tsdf": _dev(tsdf), "weight": _dev(weight), "origin": _dev(origin), "voxel": voxel}


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 1, 70), (5, 3, 67), (33, 17, 9), (70, 1, 1)], ids=str)
def test_surface_of_dense_random_fields(dims):
    from hyperpocket_amd import ops
    tsdf, weight, origin, voxel, want = _field(dims, sum(dims))
    for m in (1, 2):
        got = _host(ops.fuse_surface(_as_volume(tsdf, weight, origin, voxel), min_weight=m), SURFACE)
        _same(got, want[m], SURFACE, (dims, m))
    if min(dims) > 1:
        assert want[1]["offsets"][-1] > tsdf.size // 2


def test_capacity_below_the_total_zero_and_beyond():
    from hyperpocket_amd import ops
    dims = (33, 17, 9)
    tsdf, weight, origin, voxel, want = _field(dims, sum(dims))
    vol, want = _as_volume(tsdf, weight, origin, voxel), want[1]
    total = int(want["offsets"][-1])
    for capacity in (total // 2, 1, total + 100):
        bufs = ops.fuse_surface_buffers(2, dims, capacity, CUDA)
        for name in ("points", "normals", "cell"):
            bufs[name].fill_(SENTINEL if name != "cell" else -7)
        res = ops.fuse_surface(vol, capacity=capacity, out=bufs, ws=bufs["ws"])
        assert res is bufs
        rows = min(capacity, total)
        _same(_host(res, SURFACE, rows), {k: v if k == "offsets" else v[:rows] for k, v in want.items()}, SURFACE, capacity)
        for name, fill in (("points", SENTINEL), ("normals", SENTINEL), ("cell", -7)):
            assert bool((res[name][rows:] == fill).all()), (capacity, name)                # later rows keep the sentinel
    res = ops.fuse_surface(vol, capacity=0)
    assert res["points"].shape == (0, 3) and res["cell"].shape == (0,)
    assert (res["offsets"].cpu().numpy() == want["offsets"]).all()                         # the true counts all the same
    by_out = ops.fuse_surface(vol, out=ops.fuse_surface_buffers(2, dims, 5, CUDA))         # capacity from the rows of `out`
    _same(_host(by_out, SURFACE, 5), {k: v if k == "offsets" else v[:5] for k, v in want.items()}, SURFACE, "out")


def test_buffers_are_reused_and_two_runs_give_the_same_bits():
    from hyperpocket_amd import ops
    a, want_a, surf_a = _case(33, 65, np.uint16, (33, 17, 9))
    b, want_b, surf_b = _case(33, 65, np.uint16, (5, 3, 67))
    bufs = ops.fuse_volume_buffers(8, 33, 65, 3, a["dims"], CUDA)
    first = _volume(a, out=bufs)
    assert first["tsdf"] is bufs["tsdf"] and first["weight"] is bufs["weight"]
    got = _host(first, ("weight", "tsdf"))
    _same(got, want_a, ("weight", "tsdf"), "first use")
    rows = _host(ops.fuse_surface(first), SURFACE)
    other = dict(a, kw=dict(a["kw"], w=0, jump=(0.0, 0.05)))                               # other verdicts into the same workspace
    changed = _host(_volume(other, out=bufs), ("weight", "tsdf"))
    assert (changed["weight"] != got["weight"]).any()
    again = _volume(a, out=bufs)
    _same(_host(again, ("weight", "tsdf")), got, ("weight", "tsdf"), "two runs")
    _same(_host(ops.fuse_surface(again), SURFACE), rows, SURFACE, "two runs")
    _same(_host(_volume(a), ("weight", "tsdf")), got, ("weight", "tsdf"), "fresh buffers")
    sbufs = ops.fuse_surface_buffers(3, a["dims"], int(surf_a[1]["offsets"][-1]), CUDA)
    for m in (1, 2, 1):                                                                    # fewer rows, then more again
        res = ops.fuse_surface(again, min_weight=m, out=sbufs, ws=sbufs["ws"])
        T = int(surf_a[m]["offsets"][-1])
        _same(_host(res, SURFACE, T), surf_a[m], SURFACE, ("reused", m))
    _same(_host(_volume(b), ("weight", "tsdf")), want_b, ("weight", "tsdf"), "another grid")


def test_tables_prepared_on_the_device():
    from hyperpocket_amd import ops
    case, want, _ = _case(33, 65, np.float32, (33, 17, 9))
    Kd, Md = ops.depth_points_tables(8, case["K"], case["poses"], CUDA)
    vol = _volume(case, tables=(Kd, Md, _dev(case["origin"])))
    _same(_host(vol, ("weight", "tsdf")), want, ("weight", "tsdf"), "prepared tables")
    for bad in ((Kd.float(), Md, case["origin"]), (Kd, Md.double(), case["origin"]), (Kd, Md, _dev(case["origin"]).float()),
                (Kd, Md, _dev(case["origin"])[:2])):
        with pytest.raises(ValueError):
            _volume(case, tables=bad)

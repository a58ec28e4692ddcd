"""CPU suite for the C entry points of csrc/fuse.hip and their Python wrappers (needs the built library, not a GPU): argument
checks come before any HIP call, the workspaces and the plans agree with the formulas stated in include/hyperpocket_hip.h, the
new symbols are declared there and exported, and ops.fuse_volume, ops.fuse_surface and ops.fuse_grid check dtype, shape, device
and range on the host and hand the entry points the argument lists recorded here."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest

import fuse_law as law
from conftest import PKG_DIR, ROOT

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
NULL = ctypes.c_void_p(0)
LL = ctypes.c_longlong
D = ctypes.c_double
INF, NAN = float("inf"), float("nan")
SYMBOLS = ("hp_fuse_volume", "hp_fuse_volume_workspace_bytes", "hp_fuse_volume_plan", "hp_fuse_surface",
           "hp_fuse_surface_workspace_bytes", "hp_fuse_surface_plan")


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(verbose=False))
    for name, n in (("hp_fuse_volume_workspace_bytes", 3), ("hp_fuse_surface_workspace_bytes", 4)):
        getattr(lib, name).restype = ctypes.c_longlong
        getattr(lib, name).argtypes = [ctypes.c_int] * n
    return lib


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def _volume(lib, B=3, H=48, W=64, depth=P, is_u16=1, scale=0.001, K=P, poses=P, mask=NULL, near=0.0, far=INF, jump_abs=0.0,
            jump_rel=0.05, w=1, G=2, images=(0, 1, 1, 2), offsets=(0, 1, 4), L=None, dev_images=P, dev_offsets=P, origin=P, nx=8, ny=9,
            nz=10, voxel=0.01, truncation=0.04, tsdf=P, weight=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.hp_fuse_volume_workspace_bytes(B, H, W), 0)
    host_images = NULL if images is None else _ints(images)
    host_offsets = NULL if offsets is None else _ints(offsets)
    if L is None:
        L = 4 if images is None else len(images)
    return lib.hp_fuse_volume(B, H, W, depth, is_u16, D(scale), K, poses, mask, D(near), D(far), D(jump_abs), D(jump_rel), w, G, L,
                              dev_images, dev_offsets, host_images, host_offsets, origin, nx, ny, nz, D(voxel), D(truncation), tsdf,
                              weight, ws, LL(ws_bytes), NULL)


@pytest.mark.parametrize("bad", [
    dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=2049, W=2048), dict(B=512, H=2048, W=2048), dict(depth=NULL), dict(is_u16=2),
    dict(is_u16=-1), dict(scale=0.0), dict(scale=NAN), dict(scale=INF), dict(K=NULL), dict(poses=NULL), dict(near=-0.5), dict(near=NAN),
    dict(far=NAN), dict(near=2.0, far=1.0), dict(jump_abs=-1.0), dict(jump_abs=NAN), dict(jump_abs=INF), dict(jump_rel=-1.0),
    dict(jump_rel=NAN), dict(jump_rel=INF), dict(w=-1), dict(w=5),
    dict(G=0, offsets=(0,), images=()), dict(G=-1), dict(nx=0), dict(ny=0), dict(nz=0), dict(nx=1025), dict(ny=1025), dict(nz=1025),
    dict(nx=1024, ny=1024, nz=1024), dict(G=3, offsets=(0, 1, 2, 4), nx=1024, ny=1024, nz=683),          # 3 * 2^20 * 683 > 2^31 - 1
    dict(L=0), dict(L=3), dict(L=5), dict(images=(), offsets=(0, 0, 0)), dict(offsets=(0, 0, 4)), dict(offsets=(0, 4, 4)),
    dict(offsets=(1, 2, 4)), dict(offsets=(0, 3, 2)), dict(offsets=(0, 1, 3)), dict(images=(0, 1, 1, 3)), dict(images=(-1, 1, 1, 2)),
    dict(images=None), dict(offsets=None), dict(dev_images=NULL), dict(dev_offsets=NULL), dict(origin=NULL),
    dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=NAN), dict(voxel=INF), dict(truncation=0.0), dict(truncation=-1.0),
    dict(truncation=NAN), dict(truncation=INF), dict(tsdf=NULL), dict(weight=NULL), dict(ws=NULL), dict(ws=ctypes.c_void_p(72)),
    dict(ws_bytes=0), dict(ws_bytes=3 * 48 * 8 - 1)], ids=str)
def test_fuse_volume_rejects_before_any_hip_call(lib, bad):
    assert _volume(lib, **bad) == -1


def _surface(lib, G=2, nx=8, ny=9, nz=10, tsdf=P, weight=P, origin=P, voxel=0.01, min_weight=1, capacity=100, points=P, normals=P,
             cell=P, offsets=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.hp_fuse_surface_workspace_bytes(G, nx, ny, nz), 0)
    return lib.hp_fuse_surface(G, nx, ny, nz, tsdf, weight, origin, D(voxel), min_weight, LL(capacity), points, normals, cell, offsets,
                               ws, LL(ws_bytes), NULL)


@pytest.mark.parametrize("bad", [
    dict(G=0), dict(G=-1), dict(nx=0), dict(ny=0), dict(nz=0), dict(nx=1025), dict(ny=1025), dict(nz=1025), dict(nx=1024, ny=1024, nz=1024),
    dict(G=3, nx=1024, ny=1024, nz=683), dict(tsdf=NULL), dict(weight=NULL), dict(origin=NULL), dict(voxel=0.0), dict(voxel=-1.0),
    dict(voxel=NAN), dict(voxel=INF), dict(min_weight=0), dict(min_weight=-1), dict(capacity=-1), dict(points=NULL), dict(normals=NULL),
    dict(cell=NULL), dict(offsets=NULL), dict(capacity=0, offsets=NULL), dict(ws=NULL), dict(ws=ctypes.c_void_p(72)), dict(ws_bytes=0),
    dict(ws_bytes=15)], ids=str)
def test_fuse_surface_rejects_before_any_hip_call(lib, bad):
    assert _surface(lib, **bad) == -1


def test_workspaces_and_plans_agree_with_the_header(lib):
    """Volume: roundup(8 * B * ceil(H * W / 64), 16) bytes; words = ceil(H * W / 64), blocks_per_group = ceil(V / threads), blocks =
    G * blocks_per_group.  Surface: roundup(8 * G * ceil(V / chunk), 16) bytes; chunk = threads * voxels_per_lane = 1024; rounds =
    ceil(G * chunks / scan_threads)."""
    size = lib.hp_fuse_volume_workspace_bytes
    v = [ctypes.c_int(0) for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    for B, H, W, G, nx, ny, nz in ((1, 1, 1, 1, 1, 1, 1), (3, 33, 65, 3, 5, 3, 67), (8, 480, 640, 1, 256, 256, 256), (2, 2048, 2048, 2, 1024, 1024, 1023),
                                   ((1 << 31) - 1, 1, 1, (1 << 31) - 1, 1, 1, 1)):
        assert lib.hp_fuse_volume_plan(B, H, W, G, nx, ny, nz, *refs) == 0
        threads, words, per_group, blocks = (x.value for x in v)
        assert threads % 64 == 0 and 64 <= threads <= 1024
        assert words == -(-H * W // 64) and per_group == -(-nx * ny * nz // threads) and blocks == G * per_group
        assert size(B, H, W) == -(-8 * B * words // 16) * 16
    assert size(8, 480, 640) == 8 * 8 * 4800 and size(1, 1, 1) == 16 and size(3, 1, 1) == 32
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 2049, 2048), (512, 2048, 2048)):
        assert size(*shape) == -1 and lib.hp_fuse_volume_plan(*shape, 1, 4, 4, 4, *refs) == -1
    for grid in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 4, 1025), (2, 1024, 1024, 1024)):
        assert lib.hp_fuse_volume_plan(1, 4, 4, *grid, *refs) == -1
    for k in range(4):
        assert lib.hp_fuse_volume_plan(1, 4, 4, 1, 4, 4, 4, *(None if i == k else r for i, r in enumerate(refs))) == -1
    size = lib.hp_fuse_surface_workspace_bytes
    v = [ctypes.c_int(0) for _ in range(5)]
    refs = [ctypes.byref(x) for x in v]
    for G, nx, ny, nz in ((1, 1, 1, 1), (3, 5, 3, 67), (3, 102, 101, 102), (1, 256, 256, 256), (1, 1024, 1024, 1024), ((1 << 31) - 1, 1, 1, 1)):
        assert lib.hp_fuse_surface_plan(G, nx, ny, nz, *refs) == 0
        threads, per_lane, chunks, scan_threads, rounds = (x.value for x in v)
        assert threads % 64 == 0 and 64 <= threads <= 1024 and threads * per_lane == 1024
        assert scan_threads % 64 == 0 and 64 <= scan_threads <= 1024
        assert chunks == -(-nx * ny * nz // 1024) and rounds == -(-G * chunks // scan_threads)
        assert size(G, nx, ny, nz) == -(-8 * G * chunks // 16) * 16
    assert size(1, 256, 256, 256) == 8 * 16384 and size(1, 1, 1, 1) == 16 and size((1 << 31) - 1, 1, 1, 1) == 1 << 34
    for grid in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (1, 1025, 1, 1), (2, 1024, 1024, 1024), (3, 1024, 1024, 683)):
        assert size(*grid) == -1 and lib.hp_fuse_surface_plan(*grid, *refs) == -1
    for k in range(5):
        assert lib.hp_fuse_surface_plan(1, 4, 4, 4, *(None if i == k else r for i, r in enumerate(refs))) == -1


def test_the_new_symbols_are_declared_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "hyperpocket_hip.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    for name in SYMBOLS:
        assert re.search(r"^(int|long long) " + name + r"\(", header, re.M), name
        assert re.search(r" T " + name + r"$", exported, re.M), name
    assert "#define HP_FUSE_MAX_DIM 1024" in header


STREAM = object()


@pytest.fixture
def recorded(monkeypatch):
    """ops with the device tests off, call recording and the stream a token: nothing is launched."""
    import torch

    from hyperpocket_amd import ops
    real = ops.check_input
    calls = []

    def no_device_check(t, name, dtype=torch.float32):
        if not t.is_contiguous() or t.dtype != dtype:
            real(t, name, dtype)                                   # raises its own message

    monkeypatch.setattr(ops, "check_input", no_device_check)
    monkeypatch.setattr(ops, "_depth_on_gpu", lambda depth, masks: None)
    monkeypatch.setattr(ops, "_fuse_on_gpu", lambda t, name: None)
    monkeypatch.setattr(ops, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(ops, "current_stream", lambda device=None: STREAM)
    return calls


def _plain(a):
    return a.value if isinstance(a, (ctypes.c_longlong, ctypes.c_double)) else a


def test_no_cpu_path_and_the_signatures():
    import torch

    from hyperpocket_amd import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.fuse_volume(torch.zeros((1, 4, 4)), (1.0, 1.0, 0.0, 0.0), None, None, (0.0, 0.0, 0.0), (2, 2, 2), 0.1)
    vol = {"tsdf": torch.ones((1, 2, 2, 2)), "weight": torch.ones((1, 2, 2, 2), dtype=torch.int32),
           "origin": torch.zeros((1, 3), dtype=torch.float64), "voxel": 0.1}
    with pytest.raises(ValueError, match="GPU"):
        ops.fuse_surface(vol)
    assert list(inspect.signature(ops.fuse_volume).parameters) == [
        "depth", "intrinsics", "poses", "groups", "origin", "dims", "voxel", "truncation", "masks", "depth_scale", "near", "far", "jump",
        "window", "out", "ws"]
    assert [p.default for p in inspect.signature(ops.fuse_volume).parameters.values()][7:] == [None, None, None, 0.0, INF, (0.0, 0.05), 1, None, None]
    assert list(inspect.signature(ops.fuse_surface).parameters) == ["volume", "min_weight", "capacity", "out", "ws"]
    assert [p.default for p in inspect.signature(ops.fuse_surface).parameters.values()][1:] == [1, None, None, None]
    assert ops.FUSE_MAX_DIM == 1024 and ops.FUSE_MAX_VOXELS == (1 << 31) - 1
    assert ops.fuse_surface_plan(3, (102, 101, 102))[2:] == (1027, 1024, 4) and ops.fuse_volume_plan(3, 33, 65, 3, (5, 3, 67))[1] == 34
    for G, dims in ((0, (4, 4, 4)), (1, (0, 4, 4)), (1, (4, 4, 1025)), (2, (1024, 1024, 1024)), (1, (4, 4)), (1, (4.5, 4, 4)), (1, 4)):
        for fn in (lambda: ops.fuse_surface_plan(G, dims), lambda: ops.fuse_volume_plan(1, 4, 4, G, dims),
                   lambda: ops.fuse_volume_buffers(1, 4, 4, G, dims, "cpu"), lambda: ops.fuse_surface_buffers(G, dims, 10, "cpu")):
            with pytest.raises(ValueError):
                fn()
    with pytest.raises(ValueError):
        ops.fuse_surface_buffers(1, (4, 4, 4), -1, "cpu")


def test_fuse_grid_is_the_laws():
    import numpy as np

    from hyperpocket_amd import ops
    r = np.random.RandomState(0)
    for G in (1, 3):
        lo = r.standard_normal((G, 3))
        hi = lo + r.rand(G, 3)
        for voxel, truncation in ((0.01, None), (0.037, 0.1), (1.0, 1e-3)):
            origin, dims = ops.fuse_grid(lo, hi, voxel, truncation)
            want_origin, want_dims = law.fuse_grid(lo, hi, voxel, 4 * voxel if truncation is None else truncation)
            assert origin.dtype.is_floating_point and origin.numpy().dtype == np.float64 and (origin.numpy() == want_origin).all()
            assert dims == want_dims and all(type(n) is int for n in dims)
    assert ops.fuse_grid([0.0, 1.0, 2.0], [1.0, 1.0, 2.26], 0.25, 0.5)[1] == (8, 4, 6)
    for bad in (dict(voxel=0.0), dict(voxel=NAN), dict(voxel=INF), dict(truncation=0.0), dict(truncation=-1.0), dict(hi=[0.0, 0.0, -1.0]),
                dict(lo=[NAN, 0.0, 0.0]), dict(hi=[[1.0] * 3] * 2)):
        with pytest.raises(ValueError):
            ops.fuse_grid(**{"lo": [0.0] * 3, "hi": [1.0] * 3, "voxel": 0.1, "truncation": None, **bad})


def test_every_refusal_of_fuse_volume_is_its_own_check(recorded):
    """With the device test off and the call recorded, host tensors pass for device tensors: each of these is refused by its
    own check — were one missing, the call would go through and be recorded."""
    import numpy as np
    import torch

    from hyperpocket_amd import ops
    depth, K = torch.ones((3, 4, 6)), (10.0, 10.0, 2.5, 1.5)
    turn = [[0.0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]]
    poses = torch.tensor([turn] * 3)
    good = dict(depth=depth, intrinsics=K, poses=poses, groups=[[0], [1, 2]], origin=(0.0, 0.0, 0.0), dims=(4, 5, 6), voxel=0.1)
    scaled, sheared = torch.tensor(turn), torch.tensor(turn)
    scaled[:, :3] *= 1.001
    sheared[0, 1] += 0.001
    for kw in (dict(depth=np.ones((3, 4, 6), np.float32)), dict(depth=torch.ones((4, 6))), dict(depth=torch.ones((3, 4, 6), dtype=torch.float64)),
               dict(masks=torch.ones((2, 4, 6), dtype=torch.uint8)), dict(depth_scale=0.0), dict(near=-1.0), dict(near=2.0, far=1.0),
               dict(jump=0.05), dict(jump=(-1.0, 0.0)), dict(window=5), dict(window=1.5),
               dict(intrinsics=(0.0, 10.0, 2.5, 1.5)), dict(intrinsics=torch.ones((2, 4))),
               dict(poses=None),                                                   # a group of two images and no poses
               dict(poses=scaled), dict(poses=sheared), dict(poses=torch.zeros((3, 4))), dict(poses=torch.eye(4) * 2),
               dict(poses=torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 0]]).mul(1.0 + 2.0 ** -16)),
               dict(groups=[]), dict(groups=[[0], []]), dict(groups=[[0], [3]]), dict(groups=[[-1]]), dict(groups=[[0.5]]), dict(groups=[0, 1]),
               dict(groups="ab"), dict(origin=(0.0, 0.0)), dict(origin=torch.zeros((3, 3))), dict(origin=(0.0, NAN, 0.0)), dict(origin=(INF, 0.0, 0.0)),
               dict(dims=(4, 5)), dict(dims=(4, 5, 0)), dict(dims=(4, 5, 6.5)), dict(dims=(1025, 1, 1)), dict(dims=(1024, 1024, 1024)), dict(dims=7),
               dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=NAN), dict(voxel=INF), dict(truncation=0.0), dict(truncation=-1.0),
               dict(truncation=NAN), dict(truncation=INF)):
        with pytest.raises(ValueError):
            ops.fuse_volume(**{**good, **kw})
        assert recorded == [], kw
    with pytest.raises(ValueError, match=r"try voxel >= 0\.2"):                     # 2048 voxels along x: twice the voxel fits
        ops.fuse_volume(**{**good, "dims": (2048, 4, 4)})
    with pytest.raises(ValueError, match=r"try voxel >= 0\.1[0-9]+"):               # 2^32 voxels in all: the cube root of 2 and a little
        ops.fuse_volume(**{**good, "dims": (1024, 1024, 1024), "groups": [[0], [1], [2], [0]]})
    assert recorded == []
    # within the tolerance: fp32 rounding of a real rotation, and one image per group needs no poses
    c, s = np.cos(0.3), np.sin(0.3)
    ops.fuse_volume(**{**good, "poses": torch.tensor([[c, -s, 0, 1], [s, c, 0, 2], [0, 0, 1, 3]], dtype=torch.float64)})
    ops.fuse_volume(**{**good, "poses": None, "groups": [[0], [1], [2]]})
    ops.fuse_volume(**{**good, "groups": None, "origin": (1.0, 2.0, 3.0)})
    assert len(recorded) == 3
    bufs = ops.fuse_volume_buffers(3, 4, 6, 2, (4, 5, 6), "cpu")
    assert set(bufs) == {"tsdf", "weight", "ws"} and bufs["tsdf"].shape == bufs["weight"].shape == (2, 6, 5, 4) and bufs["ws"].nbytes == 32
    for name, bad in (("tsdf", torch.empty((2, 4, 5, 6))), ("weight", torch.empty((2, 6, 5, 4))), ("tsdf", torch.empty((2, 6, 5, 8))[..., ::2])):
        with pytest.raises(ValueError):
            ops.fuse_volume(**good, out={**bufs, name: bad}, ws=bufs["ws"])
    with pytest.raises(ValueError):
        ops.fuse_volume(**good, ws=torch.empty(3, dtype=torch.int64))
    with pytest.raises(KeyError):
        ops.fuse_volume(**good, out={"tsdf": bufs["tsdf"]})
    assert len(recorded) == 3


def test_argument_order_reaching_hp_fuse_volume(recorded):
    import torch

    from hyperpocket_amd import ops
    depth = torch.ones((3, 4, 6), dtype=torch.uint16)
    masks = torch.ones((3, 4, 6), dtype=torch.uint8)
    pose = [[0.0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]]
    res = ops.fuse_volume(depth, (10.0, 12.0, 3.3, 1.5), torch.tensor(pose), [[2], [0, 2, 1]], [[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]], (4, 5, 6),
                          0.1, masks=masks, near=0.25, far=8.0, jump=(0.125, 0.5), window=2)
    (name, B, H, W, d, is_u16, scale, K, M, mask, near, far, jump_abs, jump_rel, w, G, L, images, ends, host_images, host_ends, origin, nx,
     ny, nz, voxel, truncation, tsdf, weight, ws, ws_bytes, stream), = recorded
    assert (name, B, H, W, is_u16, w, G, L, nx, ny, nz) == ("hp_fuse_volume", 3, 4, 6, 1, 2, 2, 4, 4, 5, 6) and d is depth and mask is masks
    assert [_plain(x) for x in (scale, near, far, jump_abs, jump_rel, voxel, truncation)] == [0.001, 0.25, 8.0, 0.125, 0.5, 0.1, 0.4]
    assert all(isinstance(x, ctypes.c_double) for x in (scale, near, far, jump_abs, jump_rel, voxel, truncation))
    assert K.dtype == torch.float64 and K.tolist() == [[10.0, 12.0, 3.3, 1.5]] * 3 and M.dtype == torch.float32 and M.tolist() == [pose] * 3
    for t, want in ((images, [2, 0, 2, 1]), (host_images, [2, 0, 2, 1]), (ends, [0, 1, 4]), (host_ends, [0, 1, 4])):
        assert t.dtype == torch.int32 and t.tolist() == want and t.is_contiguous()
    assert not host_images.is_cuda and not host_ends.is_cuda
    assert origin.dtype == torch.float64 and origin.tolist() == [[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]] and origin is res["origin"]
    assert tsdf is res["tsdf"] and weight is res["weight"] and tsdf.shape == (2, 6, 5, 4) and weight.dtype == torch.int32
    assert isinstance(ws_bytes, ctypes.c_longlong) and ws.nbytes == ws_bytes.value == 32 and stream is STREAM
    assert (res["dims"], res["voxel"], res["truncation"]) == ((4, 5, 6), 0.1, 0.4) and set(res) == {"tsdf", "weight", "origin", "dims", "voxel", "truncation"}


def test_fuse_surface_refusals_and_argument_order(recorded):
    import torch

    from hyperpocket_amd import ops
    vol = {"tsdf": torch.ones((2, 6, 5, 4)), "weight": torch.ones((2, 6, 5, 4), dtype=torch.int32),
           "origin": torch.zeros((2, 3), dtype=torch.float64), "voxel": 0.1}
    for bad in (None, {}, {**vol, "tsdf": torch.ones((6, 5, 4))}, {**vol, "tsdf": torch.ones((2, 6, 5, 4), dtype=torch.float64)},
                {**vol, "weight": torch.ones((2, 6, 5, 4))}, {**vol, "weight": torch.ones((2, 6, 5, 3), dtype=torch.int32)},
                {**vol, "origin": torch.zeros((2, 3))}, {**vol, "origin": torch.zeros((3, 3), dtype=torch.float64)}, {**vol, "voxel": 0.0},
                {**vol, "voxel": NAN}, {**vol, "tsdf": torch.ones((2, 6, 5, 1025)), "weight": torch.ones((2, 6, 5, 1025), dtype=torch.int32)}):
        with pytest.raises(ValueError):
            ops.fuse_surface(bad, capacity=10)
    for kw in (dict(min_weight=0), dict(min_weight=1.5), dict(capacity=-1), dict(capacity=2.5)):
        with pytest.raises(ValueError):
            ops.fuse_surface(vol, **{"capacity": 10, **kw})
    bufs = ops.fuse_surface_buffers(2, (4, 5, 6), 10, "cpu")
    assert set(bufs) == {"points", "normals", "cell", "offsets", "ws"} and bufs["ws"].nbytes == 16 and bufs["offsets"].shape == (3,)
    for name, bad in (("points", torch.empty((9, 3))), ("normals", torch.empty((10, 3), dtype=torch.float64)), ("cell", torch.empty((10,), dtype=torch.int32)),
                      ("offsets", torch.empty((2,), dtype=torch.int64))):
        with pytest.raises(ValueError):
            ops.fuse_surface(vol, capacity=10, out={**bufs, name: bad})
    with pytest.raises(ValueError):
        ops.fuse_surface(vol, capacity=10, ws=torch.empty(1, dtype=torch.int64))
    assert recorded == []
    res = ops.fuse_surface(vol, min_weight=2, capacity=10, out=bufs, ws=bufs["ws"])
    assert res is bufs
    (name, G, nx, ny, nz, tsdf, weight, origin, voxel, m, capacity, points, normals, cell, offsets, ws, ws_bytes, stream), = recorded
    assert (name, G, nx, ny, nz, m) == ("hp_fuse_surface", 2, 4, 5, 6, 2) and tsdf is vol["tsdf"] and weight is vol["weight"]
    assert origin is vol["origin"] and isinstance(voxel, ctypes.c_double) and voxel.value == 0.1
    assert isinstance(capacity, ctypes.c_longlong) and capacity.value == 10
    assert points is bufs["points"] and normals is bufs["normals"] and cell is bufs["cell"] and offsets is bufs["offsets"]
    assert ws is bufs["ws"] and ws_bytes.value == 16 and stream is STREAM
    recorded.clear()
    res = ops.fuse_surface(vol, capacity=0)                                         # counts only: no row pointers at all
    (_, *_, capacity, points, normals, cell, offsets, ws, ws_bytes, stream), = recorded
    assert capacity.value == 0 and points is None and normals is None and cell is None and offsets is res["offsets"]
    assert res["points"].shape == (0, 3) and res["cell"].shape == (0,)

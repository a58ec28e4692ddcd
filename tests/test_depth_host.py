"""CPU suite for the C entry points of csrc/depth.hip and their Python wrappers (needs the built library, not a GPU): argument
checks come before any HIP call, the workspace and the plan agree with the formula stated in include/hyperpocket_hip.h, and
ops.depth_points checks dtype, shape, device and range on the host and hands hp_depth_points the argument list recorded here."""
import ctypes
import importlib.util
import inspect
import os

import pytest

from conftest import PKG_DIR

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
NULL = ctypes.c_void_p(0)
LL = ctypes.c_longlong
D = ctypes.c_double
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(verbose=False))
    lib.hp_depth_points_workspace_bytes.restype = ctypes.c_longlong
    lib.hp_depth_points_workspace_bytes.argtypes = [ctypes.c_int] * 3
    return lib


def _depth(lib, B=2, H=48, W=64, depth=P, is_u16=1, scale=0.001, K=P, poses=P, mask=NULL, near=0.0, far=INF, jump_abs=0.0,
           jump_rel=0.05, w=1, points=P, normals=P, pixel=P, offsets=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.hp_depth_points_workspace_bytes(B, H, W), 0)
    return lib.hp_depth_points(B, H, W, depth, is_u16, D(scale), K, poses, mask, D(near), D(far), D(jump_abs), D(jump_rel), w,
                               points, normals, pixel, offsets, ws, LL(ws_bytes), NULL)


@pytest.mark.parametrize("bad", [
    dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-4), dict(W=-4), dict(H=2049, W=2048), dict(B=512, H=2048, W=2048),
    dict(depth=NULL), dict(is_u16=2), dict(is_u16=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=NAN), dict(scale=INF),
    dict(K=NULL), dict(poses=NULL), dict(near=-0.5), dict(near=NAN), dict(far=NAN), dict(near=2.0, far=1.0),
    dict(jump_abs=-1.0), dict(jump_abs=NAN), dict(jump_abs=INF), dict(jump_rel=-1.0), dict(jump_rel=NAN), dict(jump_rel=INF),
    dict(w=-1), dict(w=5), dict(points=NULL), dict(normals=NULL), dict(pixel=NULL), dict(offsets=NULL), dict(ws=NULL),
    dict(ws=ctypes.c_void_p(72)), dict(ws_bytes=0), dict(ws_bytes=2 * 3 * 4 - 1), dict(ws_bytes=31)])
def test_depth_points_rejects_before_any_hip_call(lib, bad):
    assert _depth(lib, **bad) == -1


def test_workspace_and_plan_agree_with_the_header(lib):
    """roundup(4 * B * ceil(H * W / chunk), 16) bytes; chunk = threads * pixels_per_lane; rounds = ceil(B * chunks / scan_threads)."""
    size = lib.hp_depth_points_workspace_bytes
    v = [ctypes.c_int(0) for _ in range(5)]
    refs = [ctypes.byref(x) for x in v]
    for B, H, W in ((1, 1, 1), (3, 130, 70), (8, 480, 640), (1025, 1, 1), (5, 2048, 2048), ((1 << 20) - 1, 32, 64), ((1 << 31) - 1, 1, 1)):
        assert lib.hp_depth_points_plan(B, H, W, *refs) == 0
        threads, per_lane, chunks, scan_threads, rounds = (x.value for x in v)
        assert threads % 64 == 0 and 64 <= threads <= 1024 and 1 <= per_lane <= 16 and threads * per_lane == 1024
        assert scan_threads % 64 == 0 and 64 <= scan_threads <= 1024
        assert chunks == -(-H * W // (threads * per_lane)) and rounds == -(-B * chunks // scan_threads)
        assert size(B, H, W) == -(-4 * B * chunks // 16) * 16
    assert size(8, 480, 640) == 9600 and size(1, 1, 1) == 16 and size((1 << 31) - 1, 1, 1) == 1 << 33     # beyond 32 bits
    for B, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 2049, 2048), (512, 2048, 2048), (1 << 30, 1, 2)):
        assert size(B, H, W) == -1 and lib.hp_depth_points_plan(B, H, W, *refs) == -1
    for k in range(5):
        assert lib.hp_depth_points_plan(1, 4, 4, *(None if i == k else r for i, r in enumerate(refs))) == -1


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
    monkeypatch.setattr(ops, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(ops, "current_stream", lambda device=None: STREAM)
    return calls


def _plain(a):
    return a.value if isinstance(a, (ctypes.c_longlong, ctypes.c_double)) else a


def test_no_cpu_path_and_the_signature():
    import torch

    from hyperpocket_amd import ops
    with pytest.raises(ValueError, match="GPU"):
        ops.depth_points(torch.zeros((1, 4, 4)), (1.0, 1.0, 0.0, 0.0))
    assert list(inspect.signature(ops.depth_points).parameters) == [
        "depth", "intrinsics", "poses", "masks", "depth_scale", "near", "far", "jump", "window", "out", "ws"]
    defaults = [p.default for p in inspect.signature(ops.depth_points).parameters.values()][2:]
    assert defaults == [None, None, None, 0.0, INF, (0.0, 0.05), 1, None, None]
    assert ops.DEPTH_MAX_WINDOW == 4 and ops.SCAN_MAX_POINTS == 1 << 22
    assert ops.depth_points_plan(3, 130, 70)[2] == 9 and ops.depth_points_plan(1025, 1, 1)[3:] == (1024, 2)
    for shape in ((0, 4, 4), (1, 0, 4), (1, 2049, 2048), (512, 2048, 2048)):
        with pytest.raises(ValueError):
            ops.depth_points_plan(*shape)
        with pytest.raises(ValueError):
            ops.depth_points_buffers(*shape, "cpu")


def test_every_refusal_is_its_own_check(recorded):
    """With the device test off and the call recorded, host tensors pass for device tensors: each of these is refused by its
    own check — were one missing, the call would go through and be recorded."""
    import numpy as np
    import torch

    from hyperpocket_amd import ops
    depth, K = torch.ones((2, 4, 6)), (10.0, 10.0, 2.5, 1.5)
    mask = torch.ones((2, 4, 6), dtype=torch.uint8)
    for bad in (np.ones((2, 4, 6), np.float32), torch.ones((4, 6)), torch.ones((2, 4, 6), dtype=torch.float64),
                torch.ones((2, 4, 6), dtype=torch.int16), torch.ones((0, 4, 6)), torch.ones((2, 0, 6)),
                torch.ones((1, 2049, 2048), dtype=torch.uint16)):
        with pytest.raises(ValueError):
            ops.depth_points(bad, K)
        assert recorded == []
    for kw in (dict(masks=mask[:1]), dict(masks=mask.to(torch.int32)), dict(masks=mask.numpy()), dict(depth_scale=0.0),
               dict(depth_scale=-1.0), dict(depth_scale=INF), dict(depth_scale=NAN), dict(near=-1.0), dict(near=NAN), dict(far=NAN),
               dict(near=2.0, far=1.0), dict(jump=0.05), dict(jump=(0.0,)), dict(jump=(0.0, 0.05, 1.0)), dict(jump=(-1.0, 0.0)),
               dict(jump=(0.0, -0.05)), dict(jump=(INF, 0.0)), dict(jump=(0.0, NAN)), dict(window=-1), dict(window=5),
               dict(window=1.5), dict(poses=torch.eye(3)), dict(poses=torch.zeros((3, 3, 4))), dict(poses=torch.zeros((2, 4, 3))),
               dict(poses=torch.ones((4, 4))), dict(poses=torch.eye(4) * 2),
               dict(poses=torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, NAN], [0, 0, 1, 0]])),
               dict(poses=np.array([[1.0, 0, 0, 0], [0, 1, 0, 1e39], [0, 0, 1, 0]])),      # finite, but not in float32
               dict(poses=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1e-9, 1]])):
        with pytest.raises(ValueError):
            ops.depth_points(depth, K, **kw)
        assert recorded == [], kw
    for bad_K in ((10.0, 10.0, 2.5), torch.ones((3, 4)), torch.ones((2, 5)), (0.0, 10.0, 2.5, 1.5), (10.0, -1.0, 2.5, 1.5),
                  (10.0, 10.0, NAN, 1.5), (INF, 10.0, 2.5, 1.5), torch.ones((2, 4), dtype=torch.bool)):
        with pytest.raises(ValueError):
            ops.depth_points(depth, bad_K)
        assert recorded == [], bad_K
    ops.depth_points(depth, K, masks=mask, poses=torch.eye(4), jump=(0.0, 0.0), window=0, near=1.0, far=1.0)     # the good call
    assert len(recorded) == 1
    for B, intrinsics, poses in ((0, K, None), (2, (10.0, 0.0, 2.5, 1.5), None), (2, K, torch.ones((4, 4))), (3, K, torch.zeros((2, 3, 4)))):
        with pytest.raises(ValueError):
            ops.depth_points_tables(B, intrinsics, poses, device="cpu")
    Kd, Md = ops.depth_points_tables(2, K, None, device="cpu")
    assert Kd.dtype == torch.float64 and Kd.shape == (2, 4) and Md.dtype == torch.float32 and Md.shape == (2, 3, 4)


def test_refused_buffers(recorded):
    import torch

    from hyperpocket_amd import ops
    depth, K = torch.ones((2, 4, 6)), (10.0, 10.0, 2.5, 1.5)
    good = ops.depth_points_buffers(2, 4, 6, "cpu")
    assert set(good) == {"points", "normals", "pixel", "offsets", "ws"} and good["ws"].nbytes == 16
    assert good["points"].shape == good["normals"].shape == (48, 3) and good["pixel"].shape == (48,) and good["offsets"].shape == (3,)
    for name, bad in (("points", torch.empty((47, 3))), ("normals", torch.empty((48, 3), dtype=torch.float64)),
                      ("pixel", torch.empty((48,), dtype=torch.int32)), ("offsets", torch.empty((2,), dtype=torch.int64)),
                      ("points", torch.empty((3, 48)).t())):
        with pytest.raises(ValueError):
            ops.depth_points(depth, K, out={**good, name: bad}, ws=good["ws"])
    with pytest.raises(ValueError):
        ops.depth_points(depth, K, ws=torch.empty(3, dtype=torch.int32))
    with pytest.raises(KeyError):
        ops.depth_points(depth, K, out={k: v for k, v in good.items() if k != "pixel"})
    assert recorded == []


def test_argument_order_reaching_the_entry_point(recorded):
    import torch

    from hyperpocket_amd import ops
    depth = torch.ones((2, 4, 6), dtype=torch.uint16)
    res = ops.depth_points(depth, (10.0, 12.0, 3.3, 1.5))          # Python floats are doubles: 3.3 arrives as written
    (name, B, H, W, d, is_u16, scale, K, M, mask, near, far, jump_abs, jump_rel, w, points, normals, pixel, offsets, ws, ws_bytes,
     stream), = recorded
    assert (name, B, H, W, is_u16, w) == ("hp_depth_points", 2, 4, 6, 1, 1) and d is depth and mask is None
    assert [_plain(x) for x in (scale, near, far, jump_abs, jump_rel)] == [0.001, 0.0, INF, 0.0, 0.05]
    assert all(isinstance(x, ctypes.c_double) for x in (scale, near, far, jump_abs, jump_rel))     # never cut to a float on the way
    assert K.dtype == torch.float64 and K.tolist() == [[10.0, 12.0, 3.3, 1.5]] * 2 and K.is_contiguous()
    assert M.dtype == torch.float32 and M.tolist() == [[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]] * 2 and M.is_contiguous()
    assert points is res["points"] and normals is res["normals"] and pixel is res["pixel"] and offsets is res["offsets"]
    assert isinstance(ws_bytes, ctypes.c_longlong) and ws.nbytes == ws_bytes.value == 16 and stream is STREAM
    recorded.clear()
    bufs = ops.depth_points_buffers(2, 4, 6, "cpu")
    masks = torch.ones((2, 4, 6), dtype=torch.uint8)
    pose = torch.tensor([[0.0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
    res = ops.depth_points(depth.to(torch.float32), torch.tensor([[10.0, 12.0, 2.5, 1.5], [20.0, 22.0, 3.0, 2.0]]), poses=pose,
                           masks=masks, depth_scale=0.5, near=0.25, far=8.0, jump=(0.125, 0.5), window=4, out=bufs, ws=bufs["ws"])
    assert res is bufs
    (_, _, _, _, _, is_u16, scale, K, M, mask, near, far, jump_abs, jump_rel, w, *_), = recorded
    assert (is_u16, w) == (0, 4) and mask is masks
    assert [_plain(x) for x in (scale, near, far, jump_abs, jump_rel)] == [0.5, 0.25, 8.0, 0.125, 0.5]
    assert K.tolist() == [[10.0, 12.0, 2.5, 1.5], [20.0, 22.0, 3.0, 2.0]] and M.tolist() == [pose[:3].tolist()] * 2

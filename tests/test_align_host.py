"""CPU suite for the C entry points of csrc/align.hip and their Python side (needs the built library, not a GPU): the symbols
are exported, argument checks come before any HIP call, the plan names the kernel's geometry, the host functions of ops equal
the law's, the wrappers have no CPU path, and the dataset gained methods but no constructor keyword."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import align_law
from conftest import PKG_DIR

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
NULL = ctypes.c_void_p(0)
CAP_H = 64
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(verbose=False))
    lib.hp_scan_align_workspace_bytes.restype = ctypes.c_long
    return lib


def test_symbols_are_exported(lib):
    for name in ("hp_scan_align_step", "hp_scan_align_plan", "hp_scan_align_workspace_bytes"):
        assert hasattr(lib, name), name


def _step(lib, S=1, H=1, T=8, points=P, offsets=P, U=8, tpoints=P, toffsets=P, transforms=P, max_dist=0.1, anchor=P, shift=P,
          moments=P, index=NULL, dist2=NULL):
    return lib.hp_scan_align_step(S, H, ctypes.c_longlong(T), points, offsets, ctypes.c_longlong(U), tpoints, toffsets, transforms,
                                  ctypes.c_float(max_dist), anchor, shift, moments, index, dist2, NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(S=-1), dict(H=0), dict(H=-3), dict(H=CAP_H + 1), dict(T=-1), dict(U=-1),
                                 dict(points=NULL), dict(offsets=NULL), dict(tpoints=NULL), dict(toffsets=NULL),
                                 dict(transforms=NULL), dict(anchor=NULL), dict(shift=NULL), dict(moments=NULL),
                                 dict(index=P), dict(dist2=P),                       # they come together
                                 dict(max_dist=-1.0), dict(max_dist=-1e-30), dict(max_dist=float("nan")),
                                 dict(max_dist=float("-inf"))])
def test_scan_align_step_rejects_before_any_hip_call(lib, bad):
    assert _step(lib, **bad) == -1


def test_plan_names_the_geometry(lib):
    v = [ctypes.c_int(0) for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    seen = set()
    for H in (1, 2, 24, CAP_H):
        assert lib.hp_scan_align_plan(H, *refs) == 0
        threads, rows, group, tile = (x.value for x in v)
        assert threads % 64 == 0 and 64 <= threads <= 1024 and 1 <= rows <= 8 and 64 <= tile and 16 * tile <= 64 * 1024
        assert group == 1 if H == 1 else 2 <= group <= 8
        seen.add((threads, tile, rows, group))
    assert len({g[:2] for g in seen}) == 1 and len(seen) == 2      # one workgroup size and tile; two instances: H == 1 and H > 1
    for H in (0, -1, CAP_H + 1):
        assert lib.hp_scan_align_plan(H, *refs) == -1
    for hole in range(4):
        args = list(refs)
        args[hole] = None
        assert lib.hp_scan_align_plan(8, *args) == -1
    assert lib.hp_scan_align_workspace_bytes(4, 24) == 0
    for S, H in ((0, 1), (1, 0), (1, CAP_H + 1)):
        assert lib.hp_scan_align_workspace_bytes(S, H) == -1


def test_python_wrappers_validate_on_the_host():
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    assert ops.ALIGN_MAX_POINTS == 65536 == align_law.MAX_POINTS and ops.ALIGN_MAX_HYPOTHESES == CAP_H == align_law.MAX_HYPOTHESES
    assert ops.KNN_MAX_POINTS == 65536 and ops.CLUSTER_MAX_POINTS == 32768          # the other caps stay where they were
    assert ops.scan_align_plan() == ops.scan_align_plan(1) and ops.scan_align_plan(2) == ops.scan_align_plan(CAP_H)
    with pytest.raises(HipExtensionError):
        ops.scan_align_plan(CAP_H + 1)
    cpu = torch.zeros((4, 3)), torch.tensor([0, 4]), torch.zeros((5, 3)), torch.tensor([0, 5])
    frame = torch.zeros((1, 3)), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(HipExtensionError):                         # no CPU path, no fallback
        ops.scan_align_step(*cpu, torch.zeros((1, 1, 12)), 0.1, *frame)
    with pytest.raises(HipExtensionError):
        ops.scan_align(*cpu, 0.1)
    with pytest.raises(HipExtensionError):
        ops.align_frame(cpu[2], cpu[3], 0.1)


def test_arguments_are_checked_before_the_launch(monkeypatch):
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    real = ops.check_input

    def no_device_check(t, name, dtype=torch.float32):
        if not t.is_contiguous() or t.dtype != dtype:
            real(t, name, dtype)

    monkeypatch.setattr(ops, "check_input", no_device_check)
    monkeypatch.setattr(ops, "call", lambda *a: (_ for _ in ()).throw(AssertionError("a launch was reached")))
    sets = torch.zeros((6, 3)), torch.tensor([0, 4, 6]), torch.zeros((5, 3)), torch.tensor([0, 2, 5])
    good = dict(transforms=torch.zeros((2, 3, 12)), max_dist=0.1, anchor=torch.zeros((2, 3)), shift=torch.zeros(2, dtype=torch.int32))
    for kw in (dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(transforms=torch.zeros((2, 3, 11))),
               dict(transforms=torch.zeros((3, 3, 12))), dict(transforms=torch.zeros((2, CAP_H + 1, 12))),
               dict(transforms=torch.zeros((2, 3, 12), dtype=torch.float64)), dict(anchor=torch.zeros((2, 4))),
               dict(shift=torch.zeros(2, dtype=torch.int64)), dict(shift=torch.zeros(3, dtype=torch.int32))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(HipExtensionError):
            ops.scan_align_step(*sets, **args)
    with pytest.raises(HipExtensionError):                         # a target set per source set
        ops.scan_align_step(sets[0], sets[1], sets[2], torch.tensor([0, 5]), **good)
    for name, wrong in (("moments", torch.empty((2, 3, 17), dtype=torch.int64)), ("moments", torch.empty((2, 3, 18), dtype=torch.int32)),
                        ("index", torch.empty((3, 5), dtype=torch.int32)), ("dist2", torch.empty((3, 6), dtype=torch.float64))):
        out = {"moments": torch.empty((2, 3, 18), dtype=torch.int64), "index": torch.empty((3, 6), dtype=torch.int32),
               "dist2": torch.empty((3, 6))}
        out[name] = wrong
        with pytest.raises(HipExtensionError):
            ops.scan_align_step(*sets, out=out, want_index=True, **good)
    # no rows on one side is served on the host: no launch, the empty result
    res = ops.scan_align_step(sets[0], sets[1], torch.zeros((0, 3)), torch.tensor([0, 0, 0]), want_index=True, **good)
    assert not res["moments"].any() and (res["index"] == -1).all() and torch.isinf(res["dist2"]).all()
    for kw in (dict(iters=-1), dict(yaw=CAP_H + 1), dict(tol=-1.0), dict(yaw=4, init=np.zeros((2, 3, 4)))):
        with pytest.raises(HipExtensionError):
            ops.scan_align(*sets, 0.1, **kw)


def test_the_host_functions_equal_the_laws():
    from hyperpocket_amd import ops
    r = np.random.RandomState(3)
    p = r.uniform(-1, 1, (3, 200, 3)).astype(f32)
    anchor, shift = r.uniform(-0.1, 0.1, (3, 3)).astype(f32), np.array([1, 2, 1], np.int32)
    moments = np.zeros((3, 2, 18), np.int64)
    for s in range(3):
        for h in range(2):
            R = align_law.rotation(r.normal(size=3), r.uniform(-0.5, 0.5))
            q = (p[s] @ R.T + r.uniform(-0.1, 0.1, 3)).astype(f32)
            n = (200, 2)[h] if s == 2 else 200                     # one job with too few rows
            moments[s, h] = align_law.moments_of(p[s, :n], q[:n], np.arange(n, dtype=np.int32), np.zeros(n, f32), f32(np.inf),
                                                 anchor[s], shift[s])
    want, got = align_law.rigid_from_moments(moments, shift, anchor), ops.rigid_from_moments(moments, shift, anchor)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    assert want[1].tolist() == [[True, True], [True, True], [True, False]]
    one = ops.rigid_from_moments(moments[:, 0], shift, anchor)
    assert one[0].shape == (3, 3, 4) and np.array_equal(one[0], want[0][:, 0])
    with pytest.raises(ValueError):
        ops.rigid_from_moments(moments[:2], shift, anchor)
    src, dst = r.normal(size=(4, 3)), r.normal(size=(4, 3))
    for axis in ((0, 1, 0), (0.2, -1, 3)):
        T = ops.yaw_transforms(24, axis, src, dst)
        assert np.array_equal(T, align_law.yaw_transforms(24, axis, src, dst))
        R = T[..., :3]
        assert np.allclose(R @ np.swapaxes(R, -1, -2), np.eye(3), atol=1e-14) and np.allclose(np.linalg.det(R), 1, atol=1e-14)
        assert np.allclose(np.einsum("shab,sb->sha", R, src) + T[..., 3], dst[:, None], atol=1e-13)
    assert ops.yaw_transforms(5, (0, 0, 2), src[0], dst[0]).shape == (5, 3, 4)
    with pytest.raises(ValueError):
        ops.yaw_transforms(4, (0, 0, 0), src, dst)


def test_the_dataset_gained_methods_and_no_keyword():
    import inspect

    import torch

    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    init = list(inspect.signature(DeviceScanDataset.__init__).parameters)
    assert init[-3:] == ["outliers", "clusters", "plane"]
    assert list(inspect.signature(DeviceScanDataset.from_npy_dir).parameters)[-3:] == ["outliers", "clusters", "plane"]
    for name in ("aligned_to", "merged_views"):
        method = inspect.signature(getattr(DeviceScanDataset, name)).parameters
        assert list(method)[1:] == [{"aligned_to": "targets", "merged_views": "groups"}[name], "max_dist", "iters", "yaw", "axis"]
        assert [method[k].default for k in list(method)[3:]] == [30, 0, (0, 1, 0)]
    data = DeviceScanDataset([torch.rand(50, 3), torch.rand(40, 3)], device="cpu")
    assert data.poses is None and data.pose_ok is None and data.pose_rms is None and data.view_rows is None
    with pytest.raises(HipExtensionError):                         # no CPU path
        data.aligned_to(torch.rand(30, 3), 0.1)
    with pytest.raises(HipExtensionError):
        data.merged_views([[0, 1]], 0.1)
    with pytest.raises(ValueError):
        data.merged_views([[0, 2]], 0.1)
    with pytest.raises(ValueError):
        data.merged_views([], 0.1)
    with pytest.raises(ValueError):
        data.aligned_to([torch.rand(30, 3)] * 3, 0.1)              # one target per scan, or one for all

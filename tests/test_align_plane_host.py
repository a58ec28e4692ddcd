"""CPU suite for the C entry points of csrc/align_plane.hip and their Python side (needs the built library, not a GPU): the
symbols are exported, argument checks come before any HIP call, the plan names the kernel's geometry, the host solve of ops
equals the law's bit for bit, the wrappers have no CPU path, and the dataset gained two methods and no constructor keyword."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest

import align_law
import align_plane_law as law
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
    lib.hp_scan_align_plane_workspace_bytes.restype = ctypes.c_long
    return lib


def test_symbols_are_exported(lib):
    for name in ("hp_scan_align_plane_step", "hp_scan_align_plane_plan", "hp_scan_align_plane_workspace_bytes"):
        assert hasattr(lib, name), name


def _step(lib, S=1, H=1, T=8, points=P, offsets=P, U=8, tpoints=P, toffsets=P, tnormals=P, transforms=P, max_dist=0.1, anchor=P,
          shift=P, moments=P, index=NULL, dist2=NULL):
    return lib.hp_scan_align_plane_step(S, H, ctypes.c_longlong(T), points, offsets, ctypes.c_longlong(U), tpoints, toffsets,
                                        tnormals, transforms, ctypes.c_float(max_dist), anchor, shift, moments, index, dist2, NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(S=-1), dict(H=0), dict(H=-3), dict(H=CAP_H + 1), dict(T=-1), dict(U=-1),
                                 dict(points=NULL), dict(offsets=NULL), dict(tpoints=NULL), dict(toffsets=NULL),
                                 dict(tnormals=NULL), dict(transforms=NULL), dict(anchor=NULL), dict(shift=NULL),
                                 dict(moments=NULL), dict(index=P), dict(dist2=P),   # they come together
                                 dict(max_dist=-1.0), dict(max_dist=-1e-30), dict(max_dist=float("nan")),
                                 dict(max_dist=float("-inf"))])
def test_the_step_rejects_before_any_hip_call(lib, bad):
    assert _step(lib, **bad) == -1


def test_plan_names_the_geometry(lib):
    v = [ctypes.c_int(0) for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    seen = set()
    for H in (1, 2, 24, CAP_H):
        assert lib.hp_scan_align_plane_plan(H, *refs) == 0
        threads, rows, group, tile = (x.value for x in v)
        assert threads % 64 == 0 and 64 <= threads <= 1024 and 1 <= rows <= 8 and 64 <= tile and 16 * tile <= 64 * 1024
        assert 1 <= group <= 8
        seen.add((threads, rows, group, tile))
    assert len(seen) == 1                                          # one instance serves every H
    for H in (0, -1, CAP_H + 1):
        assert lib.hp_scan_align_plane_plan(H, *refs) == -1
    for hole in range(4):
        args = list(refs)
        args[hole] = None
        assert lib.hp_scan_align_plane_plan(8, *args) == -1
    assert lib.hp_scan_align_plane_workspace_bytes(4, 24) == 0
    for S, H in ((0, 1), (1, 0), (1, CAP_H + 1)):
        assert lib.hp_scan_align_plane_workspace_bytes(S, H) == -1


def test_python_wrappers_validate_on_the_host():
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    assert ops.scan_align_plane_plan() == ops.scan_align_plane_plan(1) == ops.scan_align_plane_plan(CAP_H)
    assert ops.scan_align_plane_plan()[2] == 1
    with pytest.raises(HipExtensionError):
        ops.scan_align_plane_plan(CAP_H + 1)
    cpu = torch.zeros((4, 3)), torch.tensor([0, 4]), torch.zeros((5, 3)), torch.tensor([0, 5])
    frame = torch.zeros((1, 3)), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(HipExtensionError):                         # no CPU path, no fallback
        ops.scan_align_plane_step(*cpu, torch.zeros((5, 3)), torch.zeros((1, 1, 12)), 0.1, *frame)
    with pytest.raises(HipExtensionError):
        ops.scan_align_plane(*cpu, 0.1)
    with pytest.raises(HipExtensionError):
        ops.scan_align_plane(*cpu, 0.1, tnormals=torch.zeros((5, 3)))


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
    good = dict(tnormals=torch.zeros((5, 3)), transforms=torch.zeros((2, 3, 12)), max_dist=0.1, anchor=torch.zeros((2, 3)),
                shift=torch.zeros(2, dtype=torch.int32))
    for kw in (dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(transforms=torch.zeros((2, 3, 11))),
               dict(transforms=torch.zeros((3, 3, 12))), dict(transforms=torch.zeros((2, CAP_H + 1, 12))),
               dict(transforms=torch.zeros((2, 3, 12), dtype=torch.float64)), dict(anchor=torch.zeros((2, 4))),
               dict(shift=torch.zeros(2, dtype=torch.int64)), dict(shift=torch.zeros(3, dtype=torch.int32)),
               dict(tnormals=torch.zeros((6, 3))), dict(tnormals=torch.zeros((5, 4))),
               dict(tnormals=torch.zeros((5, 3), dtype=torch.float64))):
        args = dict(good)
        args.update(kw)
        with pytest.raises(HipExtensionError):
            ops.scan_align_plane_step(*sets, **args)
    with pytest.raises(HipExtensionError):                         # a target set per source set
        ops.scan_align_plane_step(sets[0], sets[1], sets[2], torch.tensor([0, 5]), **good)
    for name, wrong in (("moments", torch.empty((2, 3, 18), dtype=torch.int64)), ("moments", torch.empty((2, 3, 60), dtype=torch.int32)),
                        ("index", torch.empty((3, 5), dtype=torch.int32)), ("dist2", torch.empty((3, 6), dtype=torch.float64))):
        out = {"moments": torch.empty((2, 3, 60), dtype=torch.int64), "index": torch.empty((3, 6), dtype=torch.int32),
               "dist2": torch.empty((3, 6))}
        out[name] = wrong
        with pytest.raises(HipExtensionError):
            ops.scan_align_plane_step(*sets, out=out, want_index=True, **good)
    # no rows on one side is served on the host: no launch, the empty result
    empty = dict(good, tnormals=torch.zeros((0, 3)))
    res = ops.scan_align_plane_step(sets[0], sets[1], torch.zeros((0, 3)), torch.tensor([0, 0, 0]), want_index=True, **empty)
    assert tuple(res["moments"].shape) == (2, 3, 60) and not res["moments"].any()
    assert (res["index"] == -1).all() and torch.isinf(res["dist2"]).all()
    assert set(ops.scan_align_plane_step(sets[0], sets[1], torch.zeros((0, 3)), torch.tensor([0, 0, 0]), **empty)) == {"moments"}
    for kw in (dict(iters=-1), dict(tol=-1.0), dict(tol=float("nan")), dict(init=np.zeros((3, 3, 4)))):
        with pytest.raises(HipExtensionError):
            ops.scan_align_plane(*sets, 0.1, tnormals=good["tnormals"], **kw)


def test_the_host_solve_equals_the_law():
    from hyperpocket_amd import ops
    assert ops._ALIGN_PLANE_DEGENERATE == law.DEGENERATE_PLANE and ops._ALIGN_PLANE_MOMENTS == law.MOMENTS
    source, target, _, _ = law.wavy_pair()
    slab_source, slab_target, slab_normals = law.slab_pair()
    # three sets: the sheet, the plane (refused), the sheet again with too few rows in its second job
    points = np.concatenate([source, slab_source, source[:40]])
    offsets = np.array([0, 1500, 2524, 2564])
    tpoints = np.concatenate([target, slab_target, target])
    toffsets = np.array([0, 1500, 2524, 4024])
    tnormals = np.concatenate([law.normals_of(), slab_normals, law.normals_of()])
    anchor, shift = align_law.frame(tpoints, toffsets, 0.3)
    T = np.tile(np.eye(3, 4, dtype=f32).reshape(12), (3, 2, 1))
    T[:, 1] = np.concatenate([align_law.rotation((1, 2, 3), 0.05), [[0.01], [0.0], [-0.01]]], axis=1).astype(f32).reshape(12)
    T[2, 1, 3] = 50.0                                              # far away: nothing within the gate
    moments = law.step(points, offsets, tpoints, toffsets, tnormals, T, 0.3, anchor, shift)["moments"]
    assert moments[2, 1, 0] < 6
    want, got = law.rigid_from_plane_moments(moments, shift, anchor), ops.rigid_from_plane_moments(moments, shift, anchor)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g, w.view(np.uint64) if w.dtype == np.float64 else w)
    assert want[1].tolist() == [[True, True], [False, False], [True, False]]
    assert np.isinf(want[2][2, 1]) and np.array_equal(want[0][1, 0], np.eye(3, 4))
    R = want[0][0, 0, :, :3]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) < 1e-14      # an exact rotation, not I + [omega]x
    one = ops.rigid_from_plane_moments(moments[:, 0], shift, anchor)
    assert one[0].shape == (3, 3, 4) and np.array_equal(one[0], want[0][:, 0]) and one[1].shape == (3,)
    import torch
    tens = ops.rigid_from_plane_moments(torch.from_numpy(moments), torch.from_numpy(shift), torch.from_numpy(anchor))
    assert np.array_equal(tens[0], want[0])
    with pytest.raises(ValueError):
        ops.rigid_from_plane_moments(moments[:2], shift, anchor)
    with pytest.raises(ValueError):
        ops.rigid_from_plane_moments(moments[:, :, :18], shift, anchor)


def test_the_signatures():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(ops.scan_align_plane_plan) == [("hypotheses", 1)]
    assert sig(ops.scan_align_plane_step) == [(n, E) for n in ("points", "offsets", "tpoints", "toffsets", "tnormals", "transforms",
                                                               "max_dist", "anchor", "shift")] + [("out", None), ("want_index", False)]
    assert sig(ops.rigid_from_plane_moments) == [("moments", E), ("shift", E), ("anchor", E)]
    assert sig(ops.scan_align_plane) == [(n, E) for n in ("points", "offsets", "tpoints", "toffsets", "max_dist")] + \
        [("iters", 10), ("tol", 0.0), ("init", None), ("tnormals", None), ("k", 16)]
    tail = [("max_dist", E), ("iters", 10), ("yaw", 0), ("axis", (0, 1, 0)), ("k", 16), ("coarse", 5)]
    assert sig(DeviceScanDataset.aligned_to_surface) == [("self", E), ("targets", E)] + tail
    assert sig(DeviceScanDataset.merged_views_surface) == [("self", E), ("groups", E)] + tail
    # what was there stays as it was
    assert list(inspect.signature(DeviceScanDataset.__init__).parameters)[-3:] == ["outliers", "clusters", "plane"]
    assert list(inspect.signature(DeviceScanDataset.from_npy_dir).parameters)[-3:] == ["outliers", "clusters", "plane"]
    assert sig(DeviceScanDataset.aligned_to)[2:] == [("max_dist", E), ("iters", 30), ("yaw", 0), ("axis", (0, 1, 0))]
    assert sig(DeviceScanDataset.merged_views)[2:] == [("max_dist", E), ("iters", 30), ("yaw", 0), ("axis", (0, 1, 0))]


def test_the_dataset_methods_raise_as_their_point_to_point_twins():
    import torch

    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    data = DeviceScanDataset([torch.rand(50, 3), torch.rand(40, 3)], device="cpu")
    with pytest.raises(HipExtensionError):                         # no CPU path
        data.aligned_to_surface(torch.rand(30, 3), 0.1)
    with pytest.raises(HipExtensionError):
        data.merged_views_surface([[0, 1]], 0.1)
    with pytest.raises(ValueError):
        data.merged_views_surface([[0, 2]], 0.1)
    with pytest.raises(ValueError):
        data.merged_views_surface([], 0.1)
    with pytest.raises(ValueError):
        data.merged_views_surface([[0], []], 0.1)
    with pytest.raises(ValueError):
        data.aligned_to_surface([torch.rand(30, 3)] * 3, 0.1)      # one target per scan, or one for all
    with pytest.raises(ValueError):
        data.aligned_to_surface(torch.rand(30, 2), 0.1)

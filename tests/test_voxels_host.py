"""CPU suite for the C entry points of csrc/voxels.hip (needs the built library, not a GPU): the symbols are exported, argument
checks come before any HIP call, the plan names the kernels' geometry, the workspace grows with T and slots_per_row, and the
Python wrappers and DeviceScanDataset.thinned have no CPU path and check their arguments on the host."""
import ctypes
import importlib.util
import inspect
import os

import pytest

from conftest import PKG_DIR

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
NULL = ctypes.c_void_p(0)
MAX_ROWS = 1 << 28


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(verbose=False))
    lib.hp_scan_voxels_workspace_bytes.restype = ctypes.c_long
    lib.hp_scan_voxels_workspace_bytes.argtypes = [ctypes.c_longlong, ctypes.c_int]
    return lib


def test_symbols_are_exported(lib):
    for name in ("hp_scan_voxels", "hp_scan_voxels_plan", "hp_scan_voxels_workspace_bytes"):
        assert hasattr(lib, name), name


def _voxels(lib, S=1, T=16, points=P, offsets=P, voxel=P, origin=NULL, keep_mode=0, slots_per_row=2, label=P, size=P, keep=P,
            kept=P, beyond=P, ws=P):
    return lib.hp_scan_voxels(S, ctypes.c_longlong(T), points, offsets, voxel, origin, keep_mode, slots_per_row, label, size, keep,
                              kept, beyond, ws, NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(S=-3), dict(T=-1), dict(T=MAX_ROWS + 1), dict(T=1 << 40), dict(keep_mode=-1),
                                 dict(keep_mode=2), dict(slots_per_row=0), dict(slots_per_row=3), dict(slots_per_row=8),
                                 dict(slots_per_row=-1), dict(points=NULL), dict(offsets=NULL), dict(voxel=NULL), dict(label=NULL),
                                 dict(size=NULL), dict(keep=NULL), dict(kept=NULL), dict(beyond=NULL), dict(ws=NULL),
                                 dict(T=0, slots_per_row=3), dict(T=0, kept=NULL)])
def test_scan_voxels_rejects_before_any_hip_call(lib, bad):
    assert _voxels(lib, **bad) == -1


def test_plan_names_the_geometry(lib):
    threads, rows = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.hp_scan_voxels_plan(ctypes.byref(threads), ctypes.byref(rows)) == 0
    assert threads.value % 64 == 0 and 64 <= threads.value <= 1024 and 1 <= rows.value <= 16
    assert lib.hp_scan_voxels_plan(None, ctypes.byref(rows)) == -1
    assert lib.hp_scan_voxels_plan(ctypes.byref(threads), None) == -1


def test_workspace_grows_with_rows_and_slots(lib):
    size = lib.hp_scan_voxels_workspace_bytes
    assert size(0, 1) > 0 and size(1, 1) > 0 and size(1, 1) % 16 == 0
    assert size(1000, 4) > size(1000, 2) > size(1000, 1) > size(999, 1) > size(1, 1) >= size(0, 1)
    assert size(1000, 2) >= 2 * 1000 * 24                          # per slot: the key and the best rank, the first row and the count
    assert size(MAX_ROWS, 4) >= 4 * MAX_ROWS * 24                   # does not wrap
    for T, spr in ((-1, 2), (MAX_ROWS + 1, 2), (16, 0), (16, 3), (16, 5), (16, -2)):
        assert size(T, spr) == -1


def test_python_wrappers_have_no_cpu_path():
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    assert ops.VOXEL_GRID_HALF == 1 << 20
    threads, rows = ops.scan_voxels_plan()
    assert threads % 64 == 0 and rows >= 1
    cpu = torch.zeros((4, 3)), torch.tensor([0, 4])
    with pytest.raises(HipExtensionError):                         # no CPU path, no fallback
        ops.scan_voxels(*cpu, 0.1)
    with pytest.raises(HipExtensionError):
        ops.scan_voxels(*cpu, 0.1, keep="first", slots_per_row=4)


def test_arguments_are_checked_before_the_launch(monkeypatch):
    """Ranges and shapes: refused on the host with ValueError.  check_input's device test is switched off so that CPU tensors
    reach the checks behind it; nothing is launched, every call raises first (or is served on the host: T == 0)."""
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    real = ops.check_input

    def no_device_check(t, name, dtype=torch.float32):
        if not t.is_contiguous() or t.dtype != dtype:
            real(t, name, dtype)                                   # raises its own message

    monkeypatch.setattr(ops, "check_input", no_device_check)
    monkeypatch.setattr(ops, "call", lambda *a: (_ for _ in ()).throw(AssertionError("a launch was reached")))
    points, offsets = torch.zeros((6, 3)), torch.tensor([0, 4, 6])
    for kw in (dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(voxel=1e-60),
               dict(voxel=1e60), dict(voxel=torch.ones(3)), dict(keep="centroid"), dict(keep=0), dict(slots_per_row=3),
               dict(slots_per_row=0), dict(origin=torch.zeros((3, 3))), dict(origin=torch.zeros((2, 4)))):
        args = dict(voxel=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.scan_voxels(points, offsets, **args)
    with pytest.raises(HipExtensionError):                         # a dtype is check_input's
        ops.scan_voxels(points, offsets, torch.ones(2, dtype=torch.float64))
    bufs = ops.scan_voxels_buffers(2, 6, "cpu", slots_per_row=2)
    assert set(bufs) == {"label", "size", "keep", "kept", "beyond", "ws"}
    assert bufs["ws"].numel() * bufs["ws"].element_size() >= 2 * 6 * 24
    assert bufs["label"].shape == bufs["size"].shape == bufs["keep"].shape == (6,) and bufs["kept"].shape == bufs["beyond"].shape == (2,)
    for name, wrong in (("label", torch.empty(5, dtype=torch.int32)), ("size", torch.empty((6, 1), dtype=torch.int32)),
                        ("keep", torch.empty(7, dtype=torch.uint8)), ("kept", torch.empty(3, dtype=torch.int32)),
                        ("beyond", torch.empty(1, dtype=torch.int32))):
        bad = dict(bufs)
        bad[name] = wrong
        with pytest.raises(ValueError):
            ops.scan_voxels(points, offsets, 0.1, out=bad, ws=bufs["ws"])
    with pytest.raises(HipExtensionError):
        ops.scan_voxels(points, offsets, 0.1, out=dict(bufs, keep=torch.empty(6, dtype=torch.bool)))
    with pytest.raises(ValueError):                                # a workspace sized for fewer slots per row
        ops.scan_voxels(points, offsets, 0.1, slots_per_row=4, ws=bufs["ws"])
    for S, T, spr in ((0, 6, 2), (2, -1, 2), (2, MAX_ROWS + 1, 2), (2, 6, 3)):
        with pytest.raises(ValueError):
            ops.scan_voxels_buffers(S, T, "cpu", slots_per_row=spr)
    # T == 0 is served on the host: no launch, the empty result
    bufs = ops.scan_voxels_buffers(2, 0, "cpu")
    res = ops.scan_voxels(torch.zeros((0, 3)), torch.tensor([0, 0, 0]), 0.1, out=bufs, ws=bufs["ws"])
    assert res is bufs and res["kept"].tolist() == [0, 0] and res["beyond"].tolist() == [0, 0] and res["label"].numel() == 0


def test_thinned_checks_its_arguments_and_has_no_cpu_path():
    import torch

    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    data = DeviceScanDataset([torch.rand(50, 3), torch.rand(20, 3)], device="cpu")
    assert data.voxels is None
    for kw in (dict(), dict(voxel=0.1, max_points=64), dict(max_points=7), dict(max_points=0), dict(voxel=0.1, keep="mean"),
               dict(voxel=0.1, origin="corner"), dict(max_points=64, origin=(0, 0, 0))):
        with pytest.raises(ValueError):
            data.thinned(**kw)
    with pytest.raises(HipExtensionError):
        data.thinned(voxel=0.1)
    with pytest.raises(HipExtensionError):
        data.thinned(max_points=8, keep="first", origin="center")
    method = inspect.signature(DeviceScanDataset.thinned).parameters
    assert list(method)[1:] == ["voxel", "max_points", "keep", "origin"]
    assert [method[k].default for k in list(method)[1:]] == [None, None, "center", None]
    # thinning is a method only: the constructor's keywords are what they were
    assert list(inspect.signature(DeviceScanDataset.__init__).parameters)[-3:] == ["outliers", "clusters", "plane"]
    assert list(inspect.signature(DeviceScanDataset.from_npy_dir).parameters)[-3:] == ["outliers", "clusters", "plane"]

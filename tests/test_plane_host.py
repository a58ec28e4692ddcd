"""CPU suite for the C entry points of csrc/plane.hip (needs the built library, not a GPU): the symbols are exported, argument
checks come before any HIP call, the plan names the kernel's geometry, the workspace grows with S and trials, and the Python
wrappers have no CPU path."""
import ctypes
import importlib.util
import os

import pytest

from conftest import PKG_DIR

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
NULL = ctypes.c_void_p(0)
CAP = 4096


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(verbose=False))
    lib.hp_scan_plane_workspace_bytes.restype = ctypes.c_long
    return lib


def test_symbols_are_exported(lib):
    for name in ("hp_scan_plane", "hp_scan_plane_side", "hp_scan_plane_plan", "hp_scan_plane_workspace_bytes"):
        assert hasattr(lib, name), name


def _plane(lib, S=1, points=P, offsets=P, streams=NULL, seed=0, trials=512, threshold=0.01, min_inliers=3, min_share=0.2,
           trial=P, inliers=P, found=P, sample=P, sample_plane=P, inlier=P, moments=P, shift=P, ws=P):
    return lib.hp_scan_plane(S, points, offsets, streams, ctypes.c_ulonglong(seed), trials, ctypes.c_float(threshold), min_inliers,
                             ctypes.c_float(min_share), trial, inliers, found, sample, sample_plane, inlier, moments, shift, ws,
                             NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(S=-2), dict(points=NULL), dict(offsets=NULL), dict(trial=NULL), dict(inliers=NULL),
                                 dict(found=NULL), dict(sample=NULL), dict(sample_plane=NULL), dict(inlier=NULL),
                                 dict(moments=NULL), dict(shift=NULL), dict(ws=NULL), dict(trials=0), dict(trials=-1),
                                 dict(trials=CAP + 1), dict(threshold=-1.0), dict(threshold=-1e-30),
                                 dict(threshold=float("nan")), dict(threshold=float("inf")),
                                 dict(threshold=2e19),                              # its square overflows fp32
                                 dict(min_share=1.5), dict(min_share=-0.1), dict(min_share=float("nan")),
                                 dict(min_inliers=2), dict(min_inliers=0)])
def test_scan_plane_rejects_before_any_hip_call(lib, bad):
    assert _plane(lib, **bad) == -1


def _side(lib, S=1, points=P, offsets=P, planes=P, threshold=0.01, dist=P, keep=P, kept=P):
    return lib.hp_scan_plane_side(S, points, offsets, planes, ctypes.c_float(threshold), dist, keep, kept, NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(S=-1), dict(points=NULL), dict(offsets=NULL), dict(planes=NULL), dict(dist=NULL),
                                 dict(keep=NULL), dict(kept=NULL), dict(threshold=-1.0), dict(threshold=float("nan")),
                                 dict(threshold=float("inf")), dict(threshold=2e19)])
def test_scan_plane_side_rejects_before_any_hip_call(lib, bad):
    assert _side(lib, **bad) == -1


def test_plan_names_the_geometry(lib):
    threads, rows, tile = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    refs = (ctypes.byref(threads), ctypes.byref(rows), ctypes.byref(tile))
    seen = set()
    for trials in (1, 512, CAP):
        assert lib.hp_scan_plane_plan(trials, *refs) == 0
        assert threads.value % 64 == 0 and 64 <= threads.value <= 1024 and 1 <= rows.value <= 16
        assert 64 <= tile.value <= CAP and 32 * tile.value <= 64 * 1024            # a tile of 8-float hypotheses fits LDS
        seen.add((threads.value, rows.value, tile.value))
    assert len(seen) == 1                                          # one geometry: the tests walk its edges once
    for trials in (0, -1, CAP + 1):
        assert lib.hp_scan_plane_plan(trials, *refs) == -1
    for hole in range(3):
        args = list(refs)
        args[hole] = None
        assert lib.hp_scan_plane_plan(8, *args) == -1


def test_workspace_grows_with_scans_and_trials(lib):
    size = lib.hp_scan_plane_workspace_bytes
    assert size(1, 1) > 0 and size(1, 1) % 16 == 0
    assert size(2, 64) > size(1, 64) > size(1, 63) > 0
    assert size(8, CAP) >= 8 * CAP * (32 + 4)                      # the hypotheses and the counts
    for S, trials in ((0, 8), (-1, 8), (1, 0), (1, CAP + 1)):
        assert size(S, trials) == -1


def test_python_wrappers_validate_on_the_host():
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    assert ops.PLANE_MAX_TRIALS == CAP
    assert ops.scan_plane_plan() == ops.scan_plane_plan(1) == ops.scan_plane_plan(CAP)
    with pytest.raises(HipExtensionError):
        ops.scan_plane_plan(CAP + 1)
    cpu = torch.zeros((4, 3)), torch.tensor([0, 4])
    with pytest.raises(HipExtensionError):                         # no CPU path, no fallback
        ops.scan_plane(*cpu, 0.01)
    with pytest.raises(HipExtensionError):
        ops.scan_plane_side(*cpu, torch.zeros((1, 4)), 0.01)


def test_arguments_are_checked_before_the_launch(monkeypatch):
    """Ranges, shapes and dtypes: refused on the host.  check_input's device test is switched off so that CPU tensors reach
    the checks behind it; nothing is launched, every call raises first (or is served on the host: T == 0)."""
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    real = ops.check_input

    def no_device_check(t, name, dtype=torch.float32):
        if not t.is_contiguous() or t.dtype != dtype:
            real(t, name, dtype)                                   # raises its own message

    monkeypatch.setattr(ops, "check_input", no_device_check)
    monkeypatch.setattr(ops, "call", lambda *a: (_ for _ in ()).throw(AssertionError("a launch was reached")))
    points, offsets = torch.zeros((6, 3)), torch.tensor([0, 4, 6])
    for kw in (dict(trials=0), dict(trials=CAP + 1), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=2e19),
               dict(min_inliers=2), dict(min_share=1.5), dict(min_share=-0.5), dict(streams=torch.zeros(3, dtype=torch.int64)),
               dict(streams=torch.zeros(2, dtype=torch.int32))):
        args = dict(threshold=0.01)
        args.update(kw)
        with pytest.raises(HipExtensionError):
            ops.scan_plane(points, offsets, **args)
    out, ws = ops.scan_plane_buffers(2, 6, 64, "cpu")
    assert ws.numel() * ws.element_size() >= 2 * 64 * 36
    for name, wrong in (("trial", torch.empty(3, dtype=torch.int32)), ("inliers", torch.empty(2, dtype=torch.int64)),
                        ("sample", torch.empty((2, 4), dtype=torch.int32)), ("sample_plane", torch.empty((2, 3))),
                        ("inlier", torch.empty(5, dtype=torch.uint8)), ("inlier", torch.empty(6, dtype=torch.bool)),
                        ("moments", torch.empty((2, 10), dtype=torch.int32)), ("shift", torch.empty((2, 1), dtype=torch.int32))):
        bad = dict(out)
        bad[name] = wrong
        with pytest.raises(HipExtensionError):
            ops.scan_plane(points, offsets, 0.01, trials=64, out=bad, ws=ws)
    with pytest.raises(HipExtensionError):                         # a workspace sized for fewer trials
        ops.scan_plane(points, offsets, 0.01, trials=128, ws=ws)
    # the host-side length check: more rows than S scans at the cap could hold (a meta tensor: nothing is allocated)
    long = torch.empty((ops.SCAN_MAX_POINTS + 1, 3), device="meta")
    with pytest.raises(HipExtensionError, match="at most"):
        ops.scan_plane(long, torch.tensor([0, ops.SCAN_MAX_POINTS + 1]), 0.01)
    with pytest.raises(HipExtensionError):
        ops.scan_plane_side(points, offsets, torch.zeros((3, 4)), 0.01)
    with pytest.raises(HipExtensionError):
        ops.scan_plane_side(points, offsets, torch.zeros((2, 4)), -1.0)
    # T == 0 is served on the host: no launch, the empty result
    out, ws = ops.scan_plane_buffers(2, 0, 8, "cpu")
    res = ops.scan_plane(torch.zeros((0, 3)), torch.tensor([0, 0, 0]), 0.01, trials=8, out=out, ws=ws)
    assert res["trial"].tolist() == [-1, -1] and res["found"].tolist() == [0, 0] and res["inliers"].tolist() == [0, 0]
    assert (res["sample"] == -1).all() and torch.isnan(res["sample_plane"]).all() and (res["moments"] == 0).all()
    dist, keep, kept = ops.scan_plane_side(torch.zeros((0, 3)), torch.tensor([0, 0, 0]), torch.zeros((2, 4)), 0.01)
    assert kept.tolist() == [0, 0] and dist.numel() == 0 and keep.numel() == 0


def test_the_dataset_method_has_no_cpu_path_and_the_keyword_comes_last():
    import inspect

    import torch

    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    data = DeviceScanDataset([torch.rand(50, 3)], device="cpu")
    assert data.planes is None and data.plane_found is None
    with pytest.raises(HipExtensionError):
        data.without_plane(0.01)
    with pytest.raises(HipExtensionError):
        DeviceScanDataset([torch.rand(50, 3)], device="cpu", plane=(0.01, 64))
    init = list(inspect.signature(DeviceScanDataset.__init__).parameters)
    assert init[-3:] == ["outliers", "clusters", "plane"]           # the earlier keywords keep their places
    assert list(inspect.signature(DeviceScanDataset.from_npy_dir).parameters)[-3:] == ["outliers", "clusters", "plane"]
    method = inspect.signature(DeviceScanDataset.without_plane).parameters
    assert list(method)[1:] == ["threshold", "trials", "seed", "min_inliers", "min_share", "refine"]
    assert [method[k].default for k in list(method)[2:]] == [512, 0, 3, 0.2, True]

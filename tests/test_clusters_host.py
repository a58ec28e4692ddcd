"""CPU suite for the C entry points of csrc/clusters.hip (needs the built library, not a GPU): the symbols are exported,
argument checks come before any HIP call, the plan names the kernel's geometry, and the Python wrapper has no CPU path."""
import ctypes
import importlib.util
import os

import pytest

from conftest import PKG_DIR

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
NULL = ctypes.c_void_p(0)
CAP = 32768


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build(verbose=False))


def test_symbols_are_exported(lib):
    for name in ("hp_scan_clusters", "hp_scan_clusters_plan"):
        assert hasattr(lib, name), name


def _clusters(lib, S=1, points=P, offsets=P, radius=0.5, max_points=CAP, label=P, size=P, clusters=P, largest=P):
    return lib.hp_scan_clusters(S, points, offsets, ctypes.c_float(radius), max_points, label, size, clusters, largest, NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(S=-2), dict(points=NULL), dict(offsets=NULL), dict(label=NULL), dict(size=NULL),
                                 dict(clusters=NULL), dict(largest=NULL), dict(radius=-1.0), dict(radius=-1e-30),
                                 dict(radius=float("nan")), dict(radius=float("inf")),
                                 dict(radius=2e19),                                 # its square overflows fp32
                                 dict(max_points=0), dict(max_points=-1), dict(max_points=CAP + 1)])
def test_scan_clusters_rejects_before_any_hip_call(lib, bad):
    assert _clusters(lib, **bad) == -1


def test_plan_names_the_geometry(lib):
    threads, tile, lds = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    refs = (ctypes.byref(threads), ctypes.byref(tile), ctypes.byref(lds))
    seen = set()
    for n in (1, 2048, CAP):
        assert lib.hp_scan_clusters_plan(n, *refs) == 0
        assert threads.value % 64 == 0 and 64 <= threads.value <= 1024 and tile.value >= 1
        assert lds.value >= 4 * n + 16 * tile.value and lds.value <= 160 * 1024       # the forest and the tile fit a compute unit
        seen.add((threads.value, tile.value))
    assert len(seen) == 1                                          # one geometry: the tests walk its edges once
    for n in (0, -1, CAP + 1):
        assert lib.hp_scan_clusters_plan(n, *refs) == -1
    assert lib.hp_scan_clusters_plan(8, None, refs[1], refs[2]) == -1


def test_python_wrapper_validates_on_the_host():
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    assert ops.CLUSTER_MAX_POINTS == CAP
    assert ops.scan_clusters_plan() == ops.scan_clusters_plan(CAP)
    with pytest.raises(HipExtensionError):
        ops.scan_clusters_plan(CAP + 1)
    cpu = torch.zeros((4, 3)), torch.tensor([0, 4])
    with pytest.raises(HipExtensionError):                         # no CPU path, no fallback
        ops.scan_clusters(*cpu, 0.5)
    with pytest.raises(HipExtensionError):
        ops.scan_clusters(*cpu, 0.5, max_points=4, out={})


def test_out_is_checked_before_the_launch(monkeypatch):
    """Shapes and dtypes of `out`, the radius and max_points: refused on the host.  check_input's device test is switched off
    so that CPU tensors reach the checks behind it; nothing is launched, every call raises first."""
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    real = ops.check_input

    def no_device_check(t, name, dtype=torch.float32):
        if not t.is_contiguous() or t.dtype != dtype:
            real(t, name, dtype)                                   # raises its own message

    monkeypatch.setattr(ops, "check_input", no_device_check)
    monkeypatch.setattr(ops, "call", lambda *a: (_ for _ in ()).throw(AssertionError("a launch was reached")))
    points, offsets = torch.zeros((6, 3)), torch.tensor([0, 4, 6])
    good = lambda: {"label": torch.empty(6, dtype=torch.int32), "size": torch.empty(6, dtype=torch.int32),
                    "clusters": torch.empty(2, dtype=torch.int32), "largest": torch.empty(2, dtype=torch.int32)}
    for name, wrong in (("label", torch.empty(5, dtype=torch.int32)), ("label", torch.empty(6, dtype=torch.int64)),
                        ("size", torch.empty((6, 1), dtype=torch.int32)), ("size", torch.empty(6, dtype=torch.float32)),
                        ("clusters", torch.empty(3, dtype=torch.int32)), ("clusters", torch.empty(2, dtype=torch.int64)),
                        ("largest", torch.empty(6, dtype=torch.int32)), ("largest", torch.empty(2, dtype=torch.uint8)),
                        ("label", torch.empty(12, dtype=torch.int32)[::2])):
        out = good()
        out[name] = wrong
        with pytest.raises(HipExtensionError):
            ops.scan_clusters(points, offsets, 0.5, out=out)
    for radius in (-1.0, float("nan"), float("inf"), 2e19):
        with pytest.raises(HipExtensionError):
            ops.scan_clusters(points, offsets, radius, out=good())
    for max_points in (0, -3, CAP + 1):
        with pytest.raises(HipExtensionError):
            ops.scan_clusters(points, offsets, 0.5, max_points=max_points, out=good())
    with pytest.raises(HipExtensionError):
        ops.scan_clusters(torch.zeros((6, 2)), offsets, 0.5)
    with pytest.raises(HipExtensionError):
        ops.scan_clusters(points, offsets.to(torch.int32), 0.5)
    # T == 0 is served on the host: no launch, clusters 0 and largest -1
    out = {"label": torch.empty(0, dtype=torch.int32), "size": torch.empty(0, dtype=torch.int32),
           "clusters": torch.full((2,), 7, dtype=torch.int32), "largest": torch.full((2,), 7, dtype=torch.int32)}
    label, size, clusters, largest = ops.scan_clusters(torch.zeros((0, 3)), torch.tensor([0, 0, 0]), 0.5, out=out)
    assert clusters.tolist() == [0, 0] and largest.tolist() == [-1, -1] and label.numel() == 0 and size.numel() == 0

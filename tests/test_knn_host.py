"""CPU suite for the C entry points of csrc/knn.hip (needs the built library, not a GPU): the symbols are exported, argument
checks come before any HIP call, and the plan names the instance that serves every k."""
import ctypes
import importlib.util
import os

import pytest

from conftest import PKG_DIR

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build(verbose=False))


def test_symbols_are_exported(lib):
    for name in ("hp_knn_points", "hp_knn_points_plan", "hp_scan_outliers"):
        assert hasattr(lib, name), name


def _knn(lib, S=1, points=P, offsets=P, queries=NULL, query_offsets=NULL, k=8, exclude_self=1, index=P, dist2=P):
    return lib.hp_knn_points(S, points, offsets, queries, query_offsets, k, exclude_self, index, dist2, NULL)


def _sor(lib, S=1, points=P, offsets=P, k=8, ratio=2.0, keep=P, mean_dist=P, kept=P):
    return lib.hp_scan_outliers(S, points, offsets, k, ctypes.c_float(ratio), keep, mean_dist, kept, NULL)


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=33), dict(k=-1), dict(S=0), dict(S=-3), dict(points=NULL), dict(offsets=NULL),
                                 dict(index=NULL), dict(dist2=NULL), dict(exclude_self=2),
                                 dict(queries=P), dict(query_offsets=P),                    # the two come together
                                 dict(exclude_self=0),                                      # the scan itself, self not excluded
                                 dict(queries=P, query_offsets=P, exclude_self=0)])         # queries == points: the same
def test_knn_points_rejects_before_any_hip_call(lib, bad):
    assert _knn(lib, **bad) == -1


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=33), dict(S=0), dict(points=NULL), dict(offsets=NULL), dict(keep=NULL),
                                 dict(mean_dist=NULL), dict(kept=NULL), dict(ratio=-1.0), dict(ratio=float("nan")),
                                 dict(ratio=float("inf"))])
def test_scan_outliers_rejects_before_any_hip_call(lib, bad):
    assert _sor(lib, **bad) == -1


def test_plan_names_the_instance_of_every_k(lib):
    inst, threads, tile = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    refs = (ctypes.byref(inst), ctypes.byref(threads), ctypes.byref(tile))
    seen = set()
    for k in range(1, 33):
        assert lib.hp_knn_points_plan(k, *refs) == 0
        assert inst.value == (8 if k <= 8 else 16 if k <= 16 else 32), k
        assert threads.value >= 64 and threads.value % 64 == 0 and tile.value >= 1
        seen.add((threads.value, tile.value))
    assert len(seen) == 1                                          # one geometry: the tests walk its tile once
    for k in (0, 33, -1):
        assert lib.hp_knn_points_plan(k, *refs) == -1
    assert lib.hp_knn_points_plan(8, None, refs[1], refs[2]) == -1


def test_python_wrappers_validate_on_the_host():
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    assert ops.KNN_MAX_POINTS == 65536
    assert ops.knn_points_plan(9)[0] == 16
    with pytest.raises(HipExtensionError):
        ops.knn_points_plan(33)
    cpu = torch.zeros((4, 3)), torch.tensor([0, 4])
    with pytest.raises(HipExtensionError):                         # no CPU path
        ops.knn_points(*cpu, 2)
    with pytest.raises(HipExtensionError):
        ops.scan_outliers(*cpu)

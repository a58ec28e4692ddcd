"""CPU suite for the C entry points of csrc/knn_grid.hip (needs the built library, not a GPU): the symbols are exported,
argument checks come before any HIP call, the workspace grows with the rows, the plan names the instance that serves every k,
and the Python wrappers and the dataset's search setting validate on the host."""
import ctypes
import importlib.util
import os

import pytest

from conftest import PKG_DIR

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
ODD = ctypes.c_void_p(72)
NULL = ctypes.c_void_p(0)
LL = ctypes.c_longlong


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(verbose=False))
    lib.hp_knn_grid_workspace_bytes.restype = LL
    return lib


def test_symbols_are_exported(lib):
    for name in ("hp_knn_grid", "hp_knn_grid_plan", "hp_knn_grid_workspace_bytes", "hp_outlier_keep", "hp_scan_outliers_grid"):
        assert hasattr(lib, name), name


def _knn(lib, S=1, points=P, offsets=P, queries=NULL, query_offsets=NULL, k=8, exclude_self=1, cell=NULL, index=P, dist2=P,
         mean_dist=NULL, grid=NULL, ws=P, ws_bytes=1 << 20):
    return lib.hp_knn_grid(S, points, offsets, queries, query_offsets, k, exclude_self, cell, index, dist2, mean_dist, grid, ws,
                           LL(ws_bytes), NULL)


def _keep(lib, S=1, mean_dist=P, offsets=P, ratio=2.0, keep=P, kept=P):
    return lib.hp_outlier_keep(S, mean_dist, offsets, ctypes.c_float(ratio), keep, kept, NULL)


def _sor(lib, S=1, points=P, offsets=P, k=8, ratio=2.0, cell=NULL, keep=P, mean_dist=P, kept=P, ws=P, ws_bytes=1 << 20):
    return lib.hp_scan_outliers_grid(S, points, offsets, k, ctypes.c_float(ratio), cell, keep, mean_dist, kept, ws, LL(ws_bytes), NULL)


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=33), dict(k=-1), dict(S=0), dict(S=-3), dict(points=NULL), dict(offsets=NULL),
                                 dict(index=NULL), dict(dist2=NULL), dict(exclude_self=2),
                                 dict(queries=P), dict(query_offsets=P),                    # the two come together
                                 dict(exclude_self=0),                                      # the scan itself, self not excluded
                                 dict(queries=P, query_offsets=P, exclude_self=0),          # queries == points: the same
                                 dict(ws=NULL), dict(ws=ODD), dict(ws_bytes=0), dict(ws_bytes=-16),
                                 dict(mean_dist=P),                                         # lists or m_i, not both
                                 dict(index=NULL, dist2=NULL)])                             # ... and not neither
def test_knn_grid_rejects_before_any_hip_call(lib, bad):
    assert _knn(lib, **bad) == -1


@pytest.mark.parametrize("bad", [dict(S=0), dict(mean_dist=NULL), dict(offsets=NULL), dict(keep=NULL), dict(kept=NULL),
                                 dict(ratio=-1.0), dict(ratio=float("nan")), dict(ratio=float("inf"))])
def test_outlier_keep_rejects_before_any_hip_call(lib, bad):
    assert _keep(lib, **bad) == -1


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=33), dict(S=0), dict(points=NULL), dict(offsets=NULL), dict(keep=NULL),
                                 dict(mean_dist=NULL), dict(kept=NULL), dict(ratio=-1.0), dict(ratio=float("nan")),
                                 dict(ratio=float("inf")), dict(ws=NULL), dict(ws=ODD), dict(ws_bytes=0)])
def test_scan_outliers_grid_rejects_before_any_hip_call(lib, bad):
    assert _sor(lib, **bad) == -1


def test_workspace_is_monotone_and_holds_what_the_kernels_keep(lib):
    need = lib.hp_knn_grid_workspace_bytes
    for S in (1, 3, 64):
        last = 0
        for T in (0, 1, 63, 64, 1000, 65536, 65537, 500000, 1 << 22, 8 << 22):
            own, cross = need(S, LL(T), LL(0)), need(S, LL(T), LL(1000))
            assert own % 16 == 0 and own > last and cross > own
            # the rows in cell order (16 bytes each) and 2 n_s + 64 cell counters per scan
            assert own >= 16 * T + 4 * (2 * T + 64 * S) and own <= 16 * T + 4 * (2 * T + 65 * S) + 32 * S + 64
            assert need(S, LL(T), LL(2000)) - cross == 16 * 1000 and need(S, LL(T), LL(-1)) == own
            last = own
    for bad in ((0, 10, 0), (-1, 10, 0), (1, -1, 0)):
        assert need(bad[0], LL(bad[1]), LL(bad[2])) == -1


def test_plan_names_the_instance_of_every_k(lib):
    inst, threads, tile = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    refs = (ctypes.byref(inst), ctypes.byref(threads), ctypes.byref(tile))
    seen = set()
    for k in range(1, 33):
        assert lib.hp_knn_grid_plan(k, *refs) == 0
        assert inst.value == (8 if k <= 8 else 16 if k <= 16 else 32), k
        assert threads.value >= 64 and threads.value % 64 == 0 and tile.value >= 1
        seen.add((threads.value, tile.value))
    assert len(seen) == 1
    for k in (0, 33, -1):
        assert lib.hp_knn_grid_plan(k, *refs) == -1
    assert lib.hp_knn_grid_plan(8, None, refs[1], refs[2]) == -1


def test_python_wrappers_validate_on_the_host():
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    assert ops.KNN_GRID_MAX_POINTS == 1 << 22 and ops.KNN_MAX_POINTS == 65536
    assert ops.knn_grid_plan(9)[0] == 16 and ops.knn_grid_plan(32)[0] == 32
    with pytest.raises(HipExtensionError):
        ops.knn_grid_plan(33)
    cpu = torch.zeros((4, 3)), torch.tensor([0, 4])
    for call in (lambda: ops.knn_points_grid(*cpu, 2), lambda: ops.scan_outliers_grid(*cpu),
                 lambda: ops.outlier_keep(torch.zeros(4), cpu[1])):                # no CPU path
        with pytest.raises(HipExtensionError):
            call()
    with pytest.raises(HipExtensionError):
        ops.knn_grid_buffers(0, 10, "cpu")
    assert ops.knn_grid_buffers(2, 1000, "cpu").numel() * 8 >= 16 * 1000 + 8 * 1000
    assert ops.knn_grid_buffers(2, 1000, "cpu", Q=50).numel() > ops.knn_grid_buffers(2, 1000, "cpu").numel()


def test_the_datasets_search_argument():
    import inspect

    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    assert inspect.signature(DeviceScanDataset.without_outliers).parameters["search"].default is None      # the dataset's setting
    assert list(inspect.signature(DeviceScanDataset.with_search).parameters) == ["self", "search"]
    data = object.__new__(DeviceScanDataset)                       # the check reads lengths, names and the setting only
    import torch
    data.lengths, data.names, data.search = torch.tensor([10, (1 << 22) + 1]), ["a", "b"], "brute"
    assert data._search_cap("brute", "x") is False and data._search_cap(None, "x") is False
    for bad in ("hash", "Grid", 1):
        with pytest.raises(ValueError, match="search"):
            data._search_cap(bad, "x")
        with pytest.raises(ValueError, match="search"):
            data.with_search(bad)
    grid = data.with_search("grid")
    assert grid.search == "grid" and data.search == "brute" and grid.lengths is data.lengths
    with pytest.raises(ValueError, match=r"1 \(b\).*4194304"):
        grid._search_cap(None, "edge removal")
    with pytest.raises(ValueError, match=r"1 \(b\).*4194304"):
        data._search_cap("grid", "normal estimation")
    data.lengths = torch.tensor([10, 1 << 22])
    assert data._search_cap("grid", "x") is True

"""CPU suite for farthest-point sampling: the law itself (tests/fps_law.py) against an independent float64 brute force, its
structure (covering radius, short clouds, ties), the launcher's plan over every P, and the argument checks of the entry
points (no GPU call is made)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fps_law
from conftest import PKG_DIR


def _grid_cloud(n, seed, steps=1024):
    """Rows on a grid of 1/64 in [0,16)^3: differences, squares (< 2^20 grid units) and their sums are exact in float32, so
    float32 and float64 see the same distances — and two different distances are at least one grid unit^2 apart."""
    return (np.random.RandomState(seed).randint(0, steps, size=(n, 3)) / 64.0).astype(np.float32)


def _brute_force(cloud, k, start=0):
    """Farthest-point picks from the full float64 distance matrix, the covering radius recomputed from the chosen set."""
    c = cloud.astype(np.float64)
    dist = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    chosen, radius2 = [int(start)], []
    for j in range(k):
        cover = dist[:, chosen].min(axis=1)                  # every row's distance to the chosen set
        radius2.append(cover.max())
        chosen.append(int(np.flatnonzero(cover == cover.max())[0]))
    return np.array(chosen[:k]), np.array(radius2)


@pytest.mark.parametrize("n,k,start", [(200, 60, 0), (333, 333, 7), (64, 10, 63)])
def test_law_agrees_with_a_float64_brute_force(n, k, start):
    cloud = _grid_cloud(n, n + k)
    index, radius2 = fps_law.fps_law(cloud, k, start=start)
    want_index, want_radius2 = _brute_force(cloud, k, start)
    assert index.dtype == np.int64 and radius2.dtype == np.float32
    assert np.array_equal(index, want_index)
    assert np.array_equal(radius2.astype(np.float64), want_radius2)       # the covering radius of picks 0..j, exactly
    assert np.all(np.diff(radius2) <= 0)                                  # non-increasing
    assert index[0] == start


def test_radius_is_non_increasing_on_a_plain_random_cloud():
    cloud = np.random.RandomState(3).rand(500, 3).astype(np.float32) - np.float32(0.5)
    index, radius2 = fps_law.fps_law(cloud, 200)
    assert np.all(np.diff(radius2) <= 0) and radius2[-1] > 0
    assert len(set(index.tolist())) == 200                                # distinct while the radius is positive
    # the covering radius in float64 agrees to rounding
    c = cloud.astype(np.float64)
    cover = ((c[:, None, :] - c[None, index, :]) ** 2).sum(-1).min(axis=1).max()
    np.testing.assert_allclose(radius2[-1], cover, rtol=1e-6)


def test_a_short_cloud_repeats_row_zero():
    cloud = _grid_cloud(50, 5)
    for count, k in ((1, 4), (7, 7), (7, 20), (50, 64)):
        index, radius2 = fps_law.fps_law(cloud, k, count=count, start=count - 1)
        assert sorted(index[:count].tolist()) == list(range(count))       # every row once (the rows are distinct)
        assert np.all(index[count:] == 0) and np.all(radius2[count - 1:] == 0)
        assert np.all(radius2[:count - 1] > 0)
        assert index.max() < count
    # rows at or beyond count take no part, whatever they hold
    other = cloud.copy()
    other[7:] = np.float32(1e30)
    a, b = fps_law.fps_law(cloud, 20, count=7), fps_law.fps_law(other, 20, count=7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_equal_distances_go_to_the_lowest_row():
    r = np.random.RandomState(11)
    lattice = r.randint(0, 4, size=(257, 3)).astype(np.float32)            # 64 places, 257 rows: duplicates everywhere
    index, radius2 = fps_law.fps_law(lattice, 257)
    want_index, want_radius2 = _brute_force(lattice, 257)                  # exact arithmetic: the same ties
    assert np.array_equal(index, want_index) and np.array_equal(radius2.astype(np.float64), want_radius2)
    places = len({tuple(p) for p in lattice.tolist()})
    first = {}
    for i, p in enumerate(lattice.tolist()):
        first.setdefault(tuple(p), i)
    assert sorted(index[:places].tolist()) == sorted(first.values())       # of equal rows, the first is the one picked
    assert np.all(index[places:] == 0) and np.all(radius2[places - 1:] == 0)
    # by hand: from row 0 = (0,0,0), rows 1 and 2 are equally far; the lower wins, then the other
    tiny = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 0, 0]], dtype=np.float32)
    index, radius2 = fps_law.fps_law(tiny, 4)
    assert index.tolist() == [0, 1, 2, 3] and radius2.tolist() == [4.0, 4.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------
# the library, without a GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build(verbose=False))


def test_plan_covers_every_size_without_gaps(lib):
    threads, per_lane = ctypes.c_int(0), ctypes.c_int(0)
    seen = []
    for P in range(1, 8193):
        assert lib.hp_farthest_points_plan(P, ctypes.byref(threads), ctypes.byref(per_lane)) == 0, P
        t, r = threads.value, per_lane.value
        assert t * r >= P, (P, t, r)
        assert t % 64 == 0 and 64 <= t <= 1024 and 1 <= r, (P, t, r)
        if not seen or seen[-1] != (t, r):
            seen.append((t, r))
    assert len(seen) == len(set(seen))                                     # an instance serves one range of P
    assert all(a[0] * a[1] < b[0] * b[1] for a, b in zip(seen, seen[1:]))  # and the ranges ascend
    for P in (0, -1, 8193):
        assert lib.hp_farthest_points_plan(P, ctypes.byref(threads), ctypes.byref(per_lane)) == -1
    assert lib.hp_farthest_points_plan(64, None, ctypes.byref(per_lane)) == -1
    assert lib.hp_farthest_points_plan(64, ctypes.byref(threads), None) == -1


def test_entry_point_rejects_bad_arguments_before_any_gpu_call(lib):
    p = ctypes.c_void_p(64)            # never dereferenced: every call below fails its argument check
    null = ctypes.c_void_p(0)

    def fps(B=2, P=16, clouds=p, k=4, index=p, failed=p):
        return lib.hp_farthest_points(B, P, clouds, null, null, k, index, null, failed, null)

    assert fps(B=-1) == -1
    assert fps(P=0) == -1
    assert fps(P=8193) == -1
    assert fps(k=0) == -1
    assert fps(k=8193) == -1
    assert fps(clouds=null) == -1
    assert fps(index=null) == -1
    assert fps(failed=null) == -1


def test_ops_and_batcher_refuse_what_they_cannot_do():
    from hyperpocket_amd import HipExtensionError, ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    assert ops.FPS_MAX_POINTS == 8192 == ops.SCAN_MAX_TARGET
    with pytest.raises(HipExtensionError):
        ops.farthest_points(torch.rand(2, 16, 3), 4)                       # CPU tensors: there is no CPU path
    d = DeviceScanDataset([np.random.RandomState(0).rand(9, 3).astype(np.float32)], device="cpu")
    with pytest.raises(ValueError):
        ScanBatcher(d, 1, resample="farthest", replace=True)
    with pytest.raises(ValueError):
        ScanBatcher(d, 1, resample="nearest")
    with pytest.raises(HipExtensionError):
        ScanBatcher(d, 1, resample="farthest")

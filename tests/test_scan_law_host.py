"""CPU suite for scan preparation: the sampling law itself (tests/scan_law.py) — uniformity and structure —, the argument
checks of the three entry points (no GPU call is made), and DeviceScanDataset's packing and validation on device="cpu"."""
import ctypes

import numpy as np
import pytest
import torch

import scan_law
from conftest import PKG_DIR


# ------------------------------------------------------------------------------------------------
# the law
# ------------------------------------------------------------------------------------------------
def _words_many(seed, streams, tag, count):
    """words() for many streams at once: (len(streams), count)."""
    streams = np.asarray(streams, dtype=np.uint64)[:, None]
    q = np.arange((count + 3) // 4, dtype=np.uint64)[None, :]
    out = scan_law.philox4x32_10(streams & scan_law.MASK, streams >> scan_law.S32, q, tag, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(out, axis=2).reshape(len(streams), -1)[:, :count]


def test_subsets_without_replacement_are_uniform():
    n, target, seed, streams = 40, 10, 1234, np.arange(20000)
    k = _words_many(seed, streams, 0, n)
    order = np.argsort(k, axis=1, kind="stable")[:, :target]           # by key, equal keys by index
    for s in (0, 1, 777, 19999):                                       # the vectorised form is index_law
        assert np.array_equal(np.sort(order[s]), scan_law.index_law(seed, s, n, target, False))
    counts = np.bincount(order.reshape(-1), minlength=n)
    # Binomial(20000, 1/4): sigma = sqrt(20000 * 0.25 * 0.75) = 61.2; 5 sigma = 306
    print("inclusion counts: max deviation", np.abs(counts - 5000).max())
    assert np.abs(counts - 5000).max() <= 306


def test_draws_are_uniform():
    n, per, seed, streams = 7, 16, 1234, np.arange(20000)
    d = (_words_many(seed, streams, 1, per) * np.uint64(n)) >> scan_law.S32
    for s in (0, 5, 19999):
        assert np.array_equal(d[s].astype(np.int64), scan_law.draws(seed, s, n, per))
    counts = np.bincount(d.reshape(-1).astype(np.int64), minlength=n)
    assert counts.size == n
    # Binomial(320000, 1/7): sigma = sqrt(320000 * (1/7) * (6/7)) = 197.9; 5 sigma = 990
    print("draw counts: max deviation", np.abs(counts - 320000 / 7).max())
    assert np.abs(counts - 320000 / 7).max() <= 990


@pytest.mark.parametrize("replace", [False, True])
def test_structure_of_the_law(replace):
    for n in (1, 5, 16):
        assert np.array_equal(scan_law.index_law(3, 9, n, n, replace), np.arange(n))           # n == target: the scan itself
    for n, target in ((1, 16), (5, 16), (15, 16), (100, 1024)):
        idx = scan_law.index_law(3, 9, n, target, replace)
        assert idx.shape == (target,) and np.array_equal(idx[:n], np.arange(n))
        assert idx.min() >= 0 and idx.max() < n
        assert np.array_equal(idx[n:], scan_law.draws(3, 9, n, target - n))
    for n, target in ((17, 16), (1000, 16), (5000, 1024)):
        idx = scan_law.index_law(3, 9, n, target, replace)
        assert idx.shape == (target,) and idx.min() >= 0 and idx.max() < n
        if replace:
            assert np.array_equal(idx, scan_law.draws(3, 9, n, target))
        else:
            assert np.all(np.diff(idx) > 0)                                                    # ascending, hence distinct
            k = scan_law.keys(3, 9, n)
            rest = np.setdiff1d(np.arange(n), idx)
            assert k[idx].max() <= k[rest].min()
    assert not np.array_equal(scan_law.index_law(3, 9, 1000, 16, False), scan_law.index_law(3, 10, 1000, 16, False))
    assert not np.array_equal(scan_law.index_law(3, 9, 1000, 16, False), scan_law.index_law(4, 9, 1000, 16, False))


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(w) for w in scan_law.philox4x32_10(*ctr, *key))
        assert got == want, (ctr, key)


def test_boxes_and_restore_are_float32():
    cloud = np.array([[-1.0, 0.5, 2.0], [3.0, 0.25, -7.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    center, scale = scan_law.boxes_fp32(cloud)
    assert np.array_equal(center, np.array([1.0, 0.25, -2.5], dtype=np.float32))
    assert scale == np.float32(9.0) / np.float32(0.9)
    back = scan_law.restore_fp32((cloud - center) / scale, np.float32(1.0), center, scale)
    np.testing.assert_allclose(back, cloud, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------
# the library, without a GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build(verbose=False))


def test_entry_points_reject_bad_arguments_before_any_gpu_call(lib):
    p = ctypes.c_void_p(64)            # never dereferenced: every call below fails its argument check
    null = ctypes.c_void_p(0)
    seed = ctypes.c_ulonglong(1)

    def prepare(B=2, points=p, target=16, S=3, replace=0, center=null, scale=null):
        return lib.hp_prepare_scans(B, points, p, S, p, p, seed, target, replace, center, scale, p, p, p, null)

    assert prepare(target=0) == -1
    assert prepare(target=8193) == -1
    assert prepare(B=-1) == -1
    assert prepare(B=0) == -1
    assert prepare(points=null) == -1
    assert prepare(S=0) == -1
    assert prepare(replace=2) == -1
    assert prepare(center=p) == -1                      # center without scale
    assert lib.hp_scan_boxes(-1, p, p, p, p, null) == -1
    assert lib.hp_scan_boxes(0, p, p, p, p, null) == -1
    assert lib.hp_scan_boxes(2, null, p, p, p, null) == -1
    assert lib.hp_restore_scans(-1, 8, p, p, p, p, p, null) == -1
    assert lib.hp_restore_scans(2, 0, p, p, p, p, p, null) == -1
    assert lib.hp_restore_scans(2, 8, null, p, p, p, p, null) == -1


# ------------------------------------------------------------------------------------------------
# DeviceScanDataset on the CPU: packing and validation (boxes are lazy: no kernel runs)
# ------------------------------------------------------------------------------------------------
def _scans(lengths, seed=0):
    r = np.random.RandomState(seed)
    return [r.rand(n, 3).astype(np.float32) - 0.5 for n in lengths]


def test_dataset_packs_a_list_once():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    scans = _scans([5, 1, 12])
    d = DeviceScanDataset(scans, names=["a", "b", "c"], device="cpu")
    assert len(d) == 3 and d.points.dtype == torch.float32 and d.offsets.dtype == torch.int64
    assert d.offsets.tolist() == [0, 5, 6, 18] and d.lengths.tolist() == [5, 1, 12]
    assert np.array_equal(d.points.numpy(), np.concatenate(scans))
    for i, s in enumerate(scans):
        assert np.array_equal(d.scan(i).numpy(), s)
    assert d._boxes is None                              # nothing computed yet
    pair = DeviceScanDataset((np.concatenate(scans), [0, 5, 6, 18]), device="cpu")
    assert torch.equal(pair.points, d.points) and torch.equal(pair.offsets, d.offsets)
    ints = DeviceScanDataset([np.arange(6).reshape(2, 3)], device="cpu")
    assert ints.points.dtype == torch.float32


def test_dataset_applies_the_transform_once_and_keeps_gt():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    scans = _scans([4, 7], 1)
    swap = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], dtype=np.float32)          # (x, y, z) -> (z, y, x)
    gt = np.random.RandomState(2).rand(2, 9, 3).astype(np.float32)
    d = DeviceScanDataset(scans, gt=gt, transform=swap, device="cpu")
    assert np.array_equal(d.points.numpy(), np.concatenate(scans)[:, ::-1])
    assert np.array_equal(d.gt.numpy(), gt)


def test_dataset_rejects_what_it_cannot_hold():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    good = _scans([4, 7], 3)
    with pytest.raises(ValueError):
        DeviceScanDataset([], device="cpu")
    with pytest.raises(ValueError):
        DeviceScanDataset([good[0], np.zeros((0, 3), np.float32)], device="cpu")               # an empty scan
    with pytest.raises(ValueError):
        DeviceScanDataset([good[0], np.zeros((4, 2), np.float32)], device="cpu")
    bad = good[1].copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        DeviceScanDataset([good[0], bad], device="cpu")
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        DeviceScanDataset([good[0], bad], device="cpu")
    with pytest.raises(ValueError):
        DeviceScanDataset((np.concatenate(good), [0, 4, 10]), device="cpu")                    # offsets stop short
    with pytest.raises(ValueError):
        DeviceScanDataset((np.concatenate(good), [0, 4, 4, 11]), device="cpu")                 # a scan of no points
    with pytest.raises(ValueError):
        DeviceScanDataset(good, gt=np.zeros((3, 8, 3), np.float32), device="cpu")
    with pytest.raises(ValueError):
        DeviceScanDataset(good, names=["one"], device="cpu")
    with pytest.raises(ValueError):
        DeviceScanDataset(good, transform=np.eye(4), device="cpu")


def test_batcher_and_boxes_need_the_gpu():
    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    d = DeviceScanDataset(_scans([4, 7], 4), device="cpu")
    with pytest.raises(HipExtensionError):
        d.boxes()
    with pytest.raises(HipExtensionError):
        ScanBatcher(d, 2)
    with pytest.raises(TypeError):
        ScanBatcher([1, 2], 2)

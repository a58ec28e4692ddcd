"""CPU suite for the cut by coordinate rank: the law (tests/axis_split_law.py) against numpy's stable argsort on everything an
order can get wrong, against the reference's own expressions where those are defined, and the argument checks of
hp_axis_split (no GPU call is made)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import axis_split_law
from conftest import PKG_DIR


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_key_order_by_hand():
    f = lambda *bits: np.array(bits, dtype=np.uint32).view(np.float32)
    nan_a, nan_b, nan_c = 0x7FC00001, 0xFFC00002, 0x7F800003
    c = f(nan_a, 0x7F800000, 0x00000000, 0x80000000, 0xFF800000, nan_b, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000, nan_c,
          0x00000000)
    #      NaN   +inf        +0          -0          -inf        NaN    +denorm     -denorm     1           -1          NaN  +0
    k = axis_split_law.keys(c)
    assert k[0] == k[5] == k[10] == 0xFFFFFFFF and k[1] < k[0]                # every NaN alike, above +inf
    assert k[2] == k[3] == k[11]                                              # the two zeros are one value
    assert k[4] < k[9] < k[7] < k[2] < k[6] < k[8] < k[1]                     # -inf < -1 < -denorm < 0 < +denorm < 1 < +inf
    cloud = np.stack([c, c[::-1], np.zeros_like(c)], 1)
    lower, upper, order = axis_split_law.split(cloud, 5, 0)
    assert order.tolist() == [4, 9, 7, 2, 3, 11, 6, 8, 1, 0, 5, 10]           # equal keys in row order, NaNs too
    assert np.array_equal(_bits(lower), _bits(cloud[order[:5]])) and np.array_equal(_bits(upper), _bits(cloud[order[5:]]))
    assert _bits(upper)[-3:, 0].tolist() == [nan_a, nan_b, nan_c]             # payloads intact


@pytest.mark.parametrize("n", [2, 3, 64, 65, 1000, 8192])
def test_law_is_numpys_stable_argsort(n):
    cloud = axis_split_law.awkward_cloud(n, 7 * n)
    assert np.isnan(cloud).any() or n < 8
    if n >= 1000:
        for a in range(3):
            col = _bits(cloud[:, a])
            assert {0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001} <= set(col.tolist())
            assert len(set(col[np.isnan(cloud[:, a])].tolist())) == int(np.isnan(cloud[:, a]).sum()) > 1   # distinct payloads
    for axis in range(3):
        for k in sorted({1, n // 2, n - 1} - {0, n}):
            lower, upper, order = axis_split_law.split(cloud, k, axis)
            want = np.argsort(cloud[:, axis], kind='stable')
            assert np.array_equal(order, want), (n, axis, k)
            assert lower.shape == (k, 3) and upper.shape == (n - k, 3)
            assert np.array_equal(_bits(np.concatenate([lower, upper])), _bits(cloud)[want])


def test_a_constant_coordinate_keeps_the_rows_in_place():
    cloud = np.random.RandomState(1).rand(100, 3).astype(np.float32)
    cloud[:, 1] = np.float32(0.25)
    cloud[::2, 2] = np.float32(0.0)
    cloud[1::2, 2] = np.float32(-0.0)
    for axis in (1, 2):
        lower, upper, order = axis_split_law.split(cloud, 37, axis)
        assert np.array_equal(order, np.arange(100))
        assert np.array_equal(_bits(lower), _bits(cloud[:37])) and np.array_equal(_bits(upper), _bits(cloud[37:]))


@pytest.mark.parametrize("n,k", [(2048, 1024), (64, 32), (101, 50)])
def test_without_ties_it_is_the_references_expressions(n, k):
    """core/experiments.py:149-152 of the reference cuts with numpy's default argsort: gt[gt.T[0].argsort()[k:]] and [:k]."""
    gt = np.random.RandomState(n).permutation(3 * n).reshape(n, 3).astype(np.float32) / np.float32(3 * n) - np.float32(0.5)
    for a in range(3):
        assert len(np.unique(gt[:, a])) == n                                  # no ties: the default argsort is defined
        lower, upper, order = axis_split_law.split(gt, k, a)
        assert np.array_equal(upper, gt[gt.T[a].argsort()[k:]])
        assert np.array_equal(lower, gt[gt.T[a].argsort()[:k]])
        assert np.array_equal(order, gt.T[a].argsort())


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


def test_entry_point_rejects_bad_arguments_before_any_gpu_call(lib):
    p = ctypes.c_void_p(64)            # never dereferenced: every call below ends at its argument check
    null = ctypes.c_void_p(0)

    def cut(B=2, n=16, clouds=p, axis=0, k=8, lower=p, upper=p, order=p):
        return lib.hp_axis_split(B, n, clouds, axis, k, lower, upper, order, null)

    assert cut(n=1, k=1) == -1
    assert cut(n=1, k=0) == -1
    assert cut(n=8193, k=4096) == -1
    assert cut(k=0) == -1
    assert cut(k=16) == -1
    assert cut(axis=3) == -1
    assert cut(axis=-1) == -1
    assert cut(B=-1) == -1
    assert cut(clouds=null) == -1
    assert cut(lower=null) == -1
    assert cut(upper=null) == -1
    assert cut(B=0) == 0               # nothing to do, nothing launched
    assert cut(B=0, order=null) == 0


def test_ops_refuse_what_they_cannot_do():
    from hyperpocket_amd import ops
    assert ops.AXIS_SPLIT_MAX_POINTS == 8192
    with pytest.raises(ValueError):
        ops.axis_split(torch.rand(2, 16, 3), 8)                               # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        ops.axis_split(np.zeros((2, 16, 3), np.float32), 8)

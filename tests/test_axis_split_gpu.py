"""GPU suite for the cut by coordinate rank (csrc/axis_split.hip): order, lower and upper bit for bit against
tests/axis_split_law.py at sizes around the wave, off the power of two the network pads to, at both ends of the size range and
with more clouds than compute units; on constant coordinates, duplicates across the cut, signed zeros, infinities, NaNs with
payloads and denormals; independence of the batch; the call without `order`; and caller-owned buffers."""
import numpy as np
import pytest
import torch

import axis_split_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(clouds, k, axis, **kw):
    from hyperpocket_amd import ops
    lower, upper, order = ops.axis_split(torch.from_numpy(np.ascontiguousarray(clouds)).to(CUDA), k, axis, **kw)
    return lower.cpu().numpy(), upper.cpu().numpy(), None if order is None else order.cpu().numpy()


def _check(got, cloud, k, axis, what):
    lower, upper, order = got
    want_lower, want_upper, want_order = axis_split_law.split(cloud, k, axis)
    assert order.dtype == np.int32
    wrong = int((order != want_order).sum())
    assert wrong == 0, (what, "order", wrong, int(np.flatnonzero(order != want_order)[0]))
    assert np.array_equal(_bits(lower), _bits(want_lower)), (what, "lower")
    assert np.array_equal(_bits(upper), _bits(want_upper)), (what, "upper")


def _plain(n, seed):
    return np.random.RandomState(seed).rand(n, 3).astype(np.float32) - np.float32(0.5)


@pytest.mark.parametrize("B,n,k", [(1, 2, 1), (3, 63, 31), (3, 64, 1), (3, 65, 64), (2, 1000, 333), (4, 2048, 1024), (2, 8192, 1),
                                   (2, 8192, 8191)])
def test_every_size_on_every_axis(B, n, k):
    """Cloud 0 is plain random (ties are rare), the others are awkward_cloud: duplicates everywhere — hence across the cut —,
    -0.0 with +0.0, both infinities, denormals, NaNs of both signs with distinct payloads."""
    clouds = np.stack([_plain(n, 10 * n + c) if c == 0 else axis_split_law.awkward_cloud(n, 10 * n + c) for c in range(B)])
    for axis in range(3):
        lower, upper, order = _run(clouds, k, axis)
        assert lower.shape == (B, k, 3) and upper.shape == (B, n - k, 3) and order.shape == (B, n)
        for c in range(B):
            _check((lower[c], upper[c], order[c]), clouds[c], k, axis, (B, n, k, axis, c))


def test_more_clouds_than_compute_units():
    clouds = np.stack([axis_split_law.awkward_cloud(17, 500 + c) if c % 2 else _plain(17, 500 + c) for c in range(300)])
    lower, upper, order = _run(clouds, 5, 1)
    for c in range(300):
        _check((lower[c], upper[c], order[c]), clouds[c], 5, 1, c)


def test_special_values_by_construction():
    n, k = 200, 100
    cloud = _plain(n, 3)
    cloud[:, 0] = np.float32(0.125)                                           # constant: the identity
    half = np.repeat(np.arange(n // 4, dtype=np.float32), 4)                  # runs of four equal values
    cloud[:, 1] = half[np.random.RandomState(4).permutation(n)]
    bits = _bits(cloud).copy()
    z = np.random.RandomState(5)
    col = np.where(z.rand(n) < 0.5, np.uint32(0x80000000), np.uint32(0)).astype(np.uint32)   # -0.0 mixed with +0.0
    col[[7, 150]] = 0x7F800000                                                # +inf
    col[[8, 151]] = 0xFF800000                                                # -inf
    col[[3, 90, 91, 199]] = [0x7FC00123, 0xFFC00001, 0x7F800001, 0xFFFFFFFF]  # NaNs, distinct payloads, both signs
    col[[20, 21, 22]] = [0x00000001, 0x80000001, 0x007FFFFF]                  # denormals
    bits[:, 2] = col
    cloud = bits.view(np.float32)
    lower, upper, order = _run(cloud[None], k, 0)
    assert np.array_equal(order[0], np.arange(n))
    assert np.array_equal(_bits(lower[0]), bits[:k]) and np.array_equal(_bits(upper[0]), bits[k:])
    for cut in (k, k + 1, k + 2, k + 3):                                      # k + 1 .. k + 3 cut through a run of equal values
        got = _run(cloud[None], cut, 1)
        _check((got[0][0], got[1][0], got[2][0]), cloud, cut, 1, ("duplicates", cut))
        assert np.all(np.diff(got[2][0].reshape(-1, 4), axis=1) > 0)          # within a run: ascending row
    lower, upper, order = _run(cloud[None], k, 2)
    _check((lower[0], upper[0], order[0]), cloud, k, 2, "specials")
    assert order[0][:2].tolist() == [8, 151] and order[0][-6:].tolist() == [7, 150, 3, 90, 91, 199]
    assert _bits(upper[0])[-4:, 2].tolist() == [0x7FC00123, 0xFFC00001, 0x7F800001, 0xFFFFFFFF]      # payloads intact
    assert order[0][2] == 21 and order[0][-8:-6].tolist() == [20, 22]         # denormals: below and above every zero
    zeros = order[0][3:-8]                                                    # the zeros of either sign: one value, row order
    assert np.all(np.diff(zeros) > 0) and len(zeros) == n - 11


def test_a_cloud_does_not_depend_on_its_batch():
    n, k = 333, 100
    clouds = np.stack([axis_split_law.awkward_cloud(n, 900 + c) for c in range(6)])
    batch = _run(clouds, k, 2)
    for pos in (0, 3, 5):
        alone = _run(clouds[pos:pos + 1], k, 2)
        for b, a in zip(batch, alone):
            assert np.array_equal(_bits(b[pos]), _bits(a[0])), pos
    moved = _run(clouds[::-1], k, 2)                                          # the same clouds at other places
    for b, m in zip(batch, moved):
        assert np.array_equal(_bits(b), _bits(m[::-1]))


def test_without_order_and_with_the_callers_buffers():
    from hyperpocket_amd import HipExtensionError, ops
    n, k = 777, 300
    clouds = torch.from_numpy(np.stack([axis_split_law.awkward_cloud(n, 70 + c) for c in range(3)])).to(CUDA)
    lower, upper, order = ops.axis_split(clouds, k, 1)
    out = ops.axis_split_buffers(3, n, k, CUDA)
    assert out["order"].dtype == torch.int32
    got = ops.axis_split(clouds, k, 1, out=out)
    assert got[0] is out["lower"] and got[1] is out["upper"] and got[2] is out["order"]
    for g, w in zip(got, (lower, upper, order)):
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(w.cpu().numpy()))
    bare = {"lower": torch.zeros_like(lower), "upper": torch.zeros_like(upper), "order": None}
    got = ops.axis_split(clouds, k, 1, out=bare)
    assert got[2] is None and got[0] is bare["lower"] and got[1] is bare["upper"]
    assert np.array_equal(_bits(got[0].cpu().numpy()), _bits(lower.cpu().numpy()))
    assert np.array_equal(_bits(got[1].cpu().numpy()), _bits(upper.cpu().numpy()))
    with pytest.raises(HipExtensionError):
        ops.axis_split(clouds, k + 1, 1, out=out)                             # buffers of another k
    for bad in (clouds.transpose(1, 2), clouds.double(), clouds[:, :, :2], clouds.cpu(), clouds[0]):
        with pytest.raises(ValueError):
            ops.axis_split(bad, 1, 0)
    for kw in ({"k": 0}, {"k": n}, {"k": 5, "axis": 3}):
        with pytest.raises(ValueError):
            ops.axis_split(clouds, **kw)
    empty = ops.axis_split(clouds[:0], k, 0)
    assert empty[0].shape == (0, k, 3) and empty[1].shape == (0, n - k, 3) and empty[2].shape == (0, n)

"""GPU suite for farthest-point sampling (csrc/fps.hip): index and radius2 bit for bit against tests/fps_law.py at every
instance of the kernel and around each of its boundaries, ragged counts over rows the kernel must not read, start rows,
ties, independence of the batch, bad items as values, and the call without radii."""
import ctypes

import numpy as np
import pytest
import torch

import fps_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"


def _plan(P):
    from hyperpocket_amd import ops
    threads, per_lane = ctypes.c_int(0), ctypes.c_int(0)
    assert ops.load_library().hp_farthest_points_plan(P, ctypes.byref(threads), ctypes.byref(per_lane)) == 0
    return threads.value, per_lane.value


def _sizes():
    """+-1 around every P at which the launcher changes its instance, and the sizes at which lane ownership, the wave-partial
    stage and the last partial wave can go wrong."""
    sizes = {1, 2, 63, 64, 65, 8191, 8192}
    last = _plan(1)
    for P in range(2, 8193):
        now = _plan(P)
        if now != last:                                        # P - 1 is the last size of an instance
            sizes |= {P - 2, P - 1, P}
            last = now
    return sorted(s for s in sizes if 1 <= s <= 8192)


def _cloud(n, seed):
    return (np.random.RandomState(seed).rand(n, 3).astype(np.float32) - np.float32(0.5)) * np.float32(2.0)


def _run(clouds, k, counts=None, start=None, **kw):
    from hyperpocket_amd import ops
    dev = lambda a: None if a is None else torch.tensor(a, dtype=torch.int32, device=CUDA)
    failed = torch.zeros((1,), dtype=torch.int32, device=CUDA)
    index, radius2 = ops.farthest_points(torch.from_numpy(np.ascontiguousarray(clouds)).to(CUDA), k, dev(counts), dev(start),
                                         failed=failed, **kw)
    return index.cpu().numpy(), None if radius2 is None else radius2.cpu().numpy(), int(failed.item())


def _check(got_index, got_radius2, cloud, k, count=None, start=0, what=None):
    want_index, want_radius2 = fps_law.fps_law(cloud, k, count=count, start=start)
    wrong = int((got_index != want_index).sum())
    assert wrong == 0, (what, "index", wrong, int(np.flatnonzero(got_index != want_index)[0]))
    assert np.array_equal(got_radius2.view(np.uint32), want_radius2.view(np.uint32)), (what, "radius2")


def test_every_instance_and_its_boundaries():
    sizes = _sizes()
    print("sizes", sizes, "instances", sorted({_plan(P) for P in sizes}))
    assert {1, 2, 63, 64, 65, 8191, 8192} <= set(sizes)
    for P in sizes:
        clouds = np.stack([_cloud(P, 1000 + 3 * P + c) for c in range(3)])
        k = min(P, 1024)
        index, radius2, failed = _run(clouds, k)
        assert failed == 0 and index.shape == (3, k) and radius2.shape == (3, k)
        for c in range(3):
            _check(index[c], radius2[c], clouds[c], k, what=(P, c))


def test_as_many_picks_as_the_largest_cloud_has_rows():
    clouds = np.stack([_cloud(8192, 77 + c) for c in range(3)])
    index, radius2, failed = _run(clouds, 8192)
    assert failed == 0
    for c in range(3):
        _check(index[c], radius2[c], clouds[c], 8192, what=c)
        assert sorted(index[c].tolist()) == list(range(8192))      # distinct rows: each exactly once


def test_ragged_counts_never_read_the_rows_beyond():
    P, k, counts = 1025, 130, [1, 2, 64, 1000, 1025]
    clouds = np.stack([_cloud(P, 200 + c) for c in range(len(counts))])
    for c, n in enumerate(counts):
        clouds[c, n:] = np.float32(1e30)                           # a kernel that reads them picks them
    index, radius2, failed = _run(clouds, k, counts=counts)
    assert failed == 0
    for c, n in enumerate(counts):
        assert index[c].max() < n
        _check(index[c], radius2[c], clouds[c], k, count=n, what=n)
        if n < k:
            assert np.all(index[c, n:] == 0) and np.all(radius2[c, n - 1:] == 0)


def test_start_rows():
    P, k = 300, 40
    counts, start = [300, 200, 64, 18, 300], [0, 199, 17, 17, 299]
    clouds = np.stack([_cloud(P, 300 + c) for c in range(len(counts))])
    index, radius2, failed = _run(clouds, k, counts=counts, start=start)
    assert failed == 0
    for c, (n, s) in enumerate(zip(counts, start)):
        assert index[c, 0] == s
        _check(index[c], radius2[c], clouds[c], k, count=n, start=s, what=(n, s))
    index, radius2, failed = _run(clouds, k, start=start)         # start without counts
    for c, s in enumerate(start):
        _check(index[c], radius2[c], clouds[c], k, start=s, what=("all rows", s))


def test_ties_go_to_the_lowest_row():
    r = np.random.RandomState(11)
    clouds = r.randint(0, 4, size=(3, 257, 3)).astype(np.float32)  # {0..3}^3: 64 places, 257 rows
    index, radius2, failed = _run(clouds, 257)
    assert failed == 0
    for c in range(3):
        _check(index[c], radius2[c], clouds[c], 257, what=c)
        places = len({tuple(p) for p in clouds[c].tolist()})
        assert np.all(index[c, places:] == 0) and np.all(radius2[c, places - 1:] == 0)


@pytest.mark.parametrize("P", [200, 5000])
def test_a_cloud_does_not_depend_on_its_batch(P):
    k = 100
    cloud = _cloud(P, 400 + P)
    alone = _run(cloud[None], k)
    batch = np.stack([_cloud(P, 500 + c) for c in range(9)])
    batch[5] = cloud
    counts = [P, 1, P // 2, P, 7, P, P - 1, 3, P]
    among = _run(batch, k, counts=counts)
    assert np.array_equal(among[0][5], alone[0][0])
    assert np.array_equal(among[1][5].view(np.uint32), alone[1][0].view(np.uint32))
    _check(alone[0][0], alone[1][0], cloud, k, what=P)


def test_bad_items_are_values():
    P, k = 40, 12
    clouds = np.stack([_cloud(P, 600 + c) for c in range(4)])
    counts, start = [0, 3, P + 1, P], [0, 3, 0, 5]                 # no rows; a start at count; too many rows; a good item
    from hyperpocket_amd import ops
    dev = lambda a: torch.tensor(a, dtype=torch.int32, device=CUDA)
    failed = torch.full((1,), 5, dtype=torch.int32, device=CUDA)   # the caller's counter is added to, never reset
    index, radius2 = ops.farthest_points(torch.from_numpy(clouds).to(CUDA), k, dev(counts), dev(start), failed=failed)
    index, radius2 = index.cpu().numpy(), radius2.cpu().numpy()
    assert int(failed.item()) == 5 + 3
    assert np.all(index[:3] == -1) and np.all(radius2[:3] == 0)
    _check(index[3], radius2[3], clouds[3], k, start=5, what="good row")
    index, radius2, count = _run(clouds, k, counts=[-1, P, P, P], start=[0, -1, P, P - 1])
    assert count == 3 and np.all(index[:3] == -1) and np.all(radius2[:3] == 0)
    _check(index[3], radius2[3], clouds[3], k, start=P - 1, what="last row")


def test_radii_are_optional():
    from hyperpocket_amd import ops
    clouds = np.stack([_cloud(700, 700 + c) for c in range(2)])
    with_radii = _run(clouds, 64)
    out = {"index": torch.empty((2, 64), dtype=torch.int32, device=CUDA), "radius2": None}
    index, radius2, failed = _run(clouds, 64, out=out)
    assert radius2 is None and failed == 0
    assert np.array_equal(index, with_radii[0]) and np.array_equal(out["index"].cpu().numpy(), index)
    reuse = ops.farthest_points_buffers(2, 64, CUDA)
    index, radius2, _ = _run(clouds, 64, out=reuse)
    assert np.array_equal(index, with_radii[0]) and np.array_equal(radius2, with_radii[1])


def test_inputs_are_checked():
    from hyperpocket_amd import HipExtensionError, ops
    clouds = torch.zeros((2, 16, 3), device=CUDA)
    for bad in (lambda: ops.farthest_points(clouds, 0), lambda: ops.farthest_points(clouds, 8193),
                lambda: ops.farthest_points(torch.zeros((2, 8193, 3), device=CUDA), 4),
                lambda: ops.farthest_points(torch.zeros((2, 16, 2), device=CUDA), 4),
                lambda: ops.farthest_points(clouds.double(), 4),
                lambda: ops.farthest_points(clouds, 4, counts=torch.ones(3, dtype=torch.int32, device=CUDA)),
                lambda: ops.farthest_points(clouds, 4, start=torch.zeros(2, dtype=torch.int64, device=CUDA)),
                lambda: ops.farthest_points(clouds, 4, out=ops.farthest_points_buffers(2, 5, CUDA))):
        with pytest.raises(HipExtensionError):
            bad()
    index, radius2 = ops.farthest_points(torch.zeros((0, 16, 3), device=CUDA), 4)      # B = 0: nothing to do
    assert index.shape == (0, 4) and radius2.shape == (0, 4)

"""GPU suite for the cluster kernel (csrc/clusters.hip): label, size, clusters and largest bit for bit against
tests/cluster_law.py — a ragged mix whose scan lengths sit on the wave, workgroup and tile edges at three radii; isolation of
the scans; numberings that make long parent chains; interleaved clusters; ties; absent rows and overflowed distances; the
cap and max_points; reuse and streams."""
import functools

import numpy as np
import pytest
import torch

import cluster_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
NAMES = ("label", "size", "clusters", "largest")


def _run(points, offsets, radius, **kw):
    from hyperpocket_amd import ops
    p = torch.from_numpy(np.array(points, dtype=np.float32)).to(CUDA)
    o = torch.as_tensor(np.asarray(offsets), dtype=torch.int64, device=CUDA)
    return tuple(t.cpu().numpy() for t in ops.scan_clusters(p, o, radius, **kw))


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name)
        wrong = np.flatnonzero(g != w)
        assert len(wrong) == 0, (what, name, len(wrong), int(wrong[0]), int(g[wrong[0]]), int(w[wrong[0]]))


def _check(points, offsets, radius, what=None, **kw):
    got = _run(points, offsets, radius, **kw)
    _same(got, cluster_law.cluster_law(points, offsets, radius, **kw), what)
    return got


def _geometry():
    from hyperpocket_amd import ops
    threads, tile, _ = ops.scan_clusters_plan()
    assert (threads, tile) == ops.scan_clusters_plan(1)[:2]
    return threads, tile


@functools.lru_cache(maxsize=None)
def _mix(threads, tile):
    """Scans of 0 .. 4097 rows on the wave, workgroup and tile edges, in mixed order: each a union of 1-5 Gaussian blobs
    (sigma 0.05, centres in [-1, 1]^3) plus uniform strays.  Read-only."""
    lengths = sorted({0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097,
                      threads - 1, threads, threads + 1, 2 * threads - 1, 2 * threads, 2 * threads + 1,
                      tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1})
    r = np.random.RandomState(23)
    lengths = [lengths[i] for i in r.permutation(len(lengths))]
    clouds = []
    for n in lengths:
        blobs = r.randint(1, 6)
        centre = r.uniform(-1, 1, (blobs, 3))
        c = centre[r.randint(0, blobs, n)] + r.normal(0, 0.05, (n, 3))
        stray = r.rand(n) < 0.05
        c[stray] = r.uniform(-1.5, 1.5, (int(stray.sum()), 3))
        clouds.append(c.astype(np.float32))
    points = np.concatenate(clouds)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    points.setflags(write=False)
    offsets.setflags(write=False)
    return points, offsets, tuple(lengths)


@functools.lru_cache(maxsize=None)
def _mix_law(threads, tile, radius):
    points, offsets, _ = _mix(threads, tile)
    return cluster_law.cluster_law(points, offsets, radius)


MIX_RADII = (1e-4, 0.03, 8.0)      # every row alone / blobs in pieces, strays alone / one component per scan


@pytest.mark.parametrize("radius", MIX_RADII)
def test_ragged_mix(radius):
    threads, tile = _geometry()
    points, offsets, lengths = _mix(threads, tile)
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097} <= set(lengths)
    want = _mix_law(threads, tile, radius)
    _same(_run(points, offsets, radius), want, radius)
    present = np.array(lengths) > 0
    if radius == MIX_RADII[0]:
        assert np.array_equal(want[2], np.array(lengths))                   # the range the radii are meant to span
    if radius == MIX_RADII[-1]:
        assert np.array_equal(want[2], present.astype(np.int32))
    if radius == MIX_RADII[1]:
        assert ((want[2] > 1) & (want[2] < np.array(lengths)))[np.array(lengths) > 64].all()


def test_scans_are_isolated():
    r = np.random.RandomState(5)
    cloud = r.uniform(-1, 1, (300, 3)).astype(np.float32)
    points, offsets = np.concatenate([cloud, cloud]), [0, 300, 600]         # identical coordinates, stored side by side
    label, size, clusters, largest = _check(points, offsets, 0.2, what="twins")
    alone = _run(cloud, [0, 300], 0.2)
    assert np.array_equal(label[:300], alone[0]) and np.array_equal(label[300:], alone[0])
    assert np.array_equal(size[:300], alone[1]) and np.array_equal(size[300:], alone[1])
    assert clusters.tolist() == [alone[2][0]] * 2 and largest.tolist() == [alone[3][0]] * 2
    assert size.max() < 300 and clusters[0] > 1                             # the radius splits the scan: labels could leak
    label, size, clusters, _ = _check(points, offsets, 0.0, what="twins at radius 0")
    assert np.array_equal(label, np.tile(np.arange(300), 2)) and (size == 1).all()       # a row's twin is in the other scan


def _bit_reversed(n):
    bits = n.bit_length() - 1
    assert 1 << bits == n
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])


def test_adversarial_numbering_of_a_chain():
    n, step = 2048, np.float32(0.0078125)
    r = np.random.RandomState(8)
    orders = {"reverse": np.arange(n)[::-1], "bit-reversed": _bit_reversed(n), "random": r.permutation(n)}
    below = np.nextafter(step, np.float32(0))
    for what, order in orders.items():
        chain = np.zeros((n, 3), dtype=np.float32)
        chain[:, 2] = order.astype(np.float32) * step                       # row i sits at place order[i] of the chain
        label, size, clusters, largest = _run(chain, [0, n], float(step))
        assert (label == 0).all() and (size == n).all() and clusters.tolist() == [1] and largest.tolist() == [0], what
        label, size, clusters, largest = _run(chain, [0, n], float(below))
        assert np.array_equal(label, np.arange(n)) and (size == 1).all() and clusters.tolist() == [n] and largest.tolist() == [0], what
    # pieces: the chain cut at every 100th place; the components are the same sets of places under every numbering, each
    # named by the smallest row it holds
    for what, order in orders.items():
        place = order.astype(np.float32) * step + (order // 100).astype(np.float32)
        chain = np.zeros((n, 3), dtype=np.float32)
        chain[:, 0] = place
        label, size, clusters, largest = _run(chain, [0, n], float(step))   # against the closed form
        assert clusters.tolist() == [21] and largest.tolist() == [int(np.flatnonzero(order // 100 < 20).min())] and np.array_equal(size, np.where(order // 100 == 20, 48, 100))
        first_of_piece = np.full(21, n)
        np.minimum.at(first_of_piece, order // 100, np.arange(n))           # relabelling by smallest row
        assert np.array_equal(label, first_of_piece[order // 100])


def test_two_interleaved_clusters():
    r = np.random.RandomState(6)
    n = 3001
    cloud = r.normal(0, 0.05, (n, 3)).astype(np.float32)
    cloud[1::2] += np.float32(50.0)                                         # odd rows in a blob far away
    label, size, clusters, largest = _check(cloud, [0, n], 1.0, what="interleaved")
    assert np.array_equal(label, np.arange(n) % 2) and clusters.tolist() == [2] and largest.tolist() == [0]
    assert np.array_equal(size, np.where(np.arange(n) % 2 == 0, 1501, 1500))
    label, _, _, largest = _check(cloud[1:], [0, n - 1], 1.0, what="interleaved, equal sizes")
    assert largest.tolist() == [0]                                          # 1500 and 1500: the smaller label


def test_ties():
    same = np.full((300, 3), 0.375, dtype=np.float32)
    label, size, clusters, largest = _check(same, [0, 300], 0.0, what="identical")
    assert (label == 0).all() and (size == 300).all() and clusters.tolist() == [1]
    g = np.arange(7, dtype=np.float32) * np.float32(0.25)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    label, size, clusters, _ = _check(lattice, [0, 343], 0.25, what="lattice at the spacing")
    assert clusters.tolist() == [1] and (label == 0).all()
    below = float(np.nextafter(np.float32(0.25), np.float32(0)))
    label, size, clusters, _ = _check(lattice, [0, 343], below, what="lattice below the spacing")
    assert clusters.tolist() == [343] and np.array_equal(label, np.arange(343))
    label, size, clusters, _ = _check(lattice, [0, 343], 0.25 * np.sqrt(2.0), what="lattice at the face diagonal")
    assert clusters.tolist() == [1]
    _check(np.concatenate([lattice[::-1], same, lattice]), [0, 343, 643, 986], 0.25, what="lattice, identical, lattice")


def test_non_finite_rows_are_absent_and_overflow_never_joins():
    r = np.random.RandomState(9)
    cloud = r.uniform(-1, 1, (1500, 3)).astype(np.float32)
    bad = r.permutation(1500)[:90]
    cloud[bad[:30], r.randint(0, 3, 30)] = np.nan
    cloud[bad[30:60], r.randint(0, 3, 30)] = np.inf
    cloud[bad[60:], r.randint(0, 3, 30)] = -np.inf
    for radius in (0.08, 0.3):
        label, size, clusters, largest = _check(cloud, [0, 1500], radius, what=("non-finite", radius))
        assert (label[bad] == -1).all() and (size[bad] == 0).all() and (np.delete(label, bad) >= 0).all()
        assert not np.isin(label, bad).any()
    huge = r.uniform(-1, 1, (200, 3)).astype(np.float32)
    huge[::2, 0] = 1e30                                                     # two groups an overflowed distance apart
    huge[5] = (3e38, 3e38, 3e38)
    label, size, clusters, _ = _check(huge, [0, 200], 4.0, what="huge")
    assert clusters.tolist() == [3] and sorted(set(label.tolist())) == [0, 1, 5]
    _check(huge, [0, 200], 1.8e19, what="huge, a radius whose square is near the largest float")
    nothing = np.full((70, 3), np.nan, dtype=np.float32)
    label, size, clusters, largest = _check(np.concatenate([nothing, cloud[:5]]), [0, 70, 75], 0.5, what="a scan of NaN")
    assert (label[:70] == -1).all() and clusters[0] == 0 and largest[0] == -1


def test_the_cap():
    from hyperpocket_amd import ops
    n = ops.CLUSTER_MAX_POINTS
    assert n == 32768
    r = np.random.RandomState(12)
    cuts = np.sort(r.permutation(np.arange(1, n))[:40])                     # a gap in front of these places
    cuts = np.concatenate([cuts, [5000, 5001, 5002]])                       # ... and three pieces of one row
    cuts = np.unique(cuts)
    piece = np.searchsorted(cuts, np.arange(n), side="right")
    line = np.zeros((n, 3), dtype=np.float32)
    line[:, 1] = (np.arange(n) + piece * 2).astype(np.float32)              # spacing 1 inside a piece, 3 across a cut
    starts = np.concatenate([[0], cuts])
    sizes = np.diff(np.concatenate([starts, [n]]))
    label, size, clusters, largest = _run(line, [0, n], 1.0)
    assert np.array_equal(label, starts[piece]) and np.array_equal(size, sizes[piece])
    assert clusters.tolist() == [len(starts)] and largest.tolist() == [starts[np.argmax(sizes)]]
    # max_points smaller than a scan: the empty result for that scan alone
    chain = np.zeros((1300, 3), dtype=np.float32)
    chain[:, 2] = np.arange(1300)
    three = np.concatenate([chain[:700], chain, chain[:701]])
    offsets = [0, 700, 2000, 2701]
    got = _check(three, offsets, 1.0, what="max_points 701", max_points=701)
    assert got[2].tolist() == [1, 0, 1] and got[3].tolist() == [0, -1, 0] and (got[0][700:2000] == -1).all()
    assert (got[1][700:2000] == 0).all() and (got[1][:700] == 700).all() and (got[1][2000:] == 701).all()
    got = _check(three, offsets, 1.0, what="max_points 700", max_points=700)
    assert got[2].tolist() == [1, 0, 0]
    _check(three, offsets, 1.0, what="max_points 1300", max_points=1300)


def test_the_cap_through_the_dataset():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    n = ops.CLUSTER_MAX_POINTS + 1
    long = torch.zeros((n, 3))
    long[:, 0] = torch.arange(n)
    data = DeviceScanDataset([torch.rand(50, 3), long], names=["small", "too-long"])
    for call in (lambda: data.keep_clusters(1.0), lambda: data.split_clusters(1.0)):
        with pytest.raises(ValueError, match=r"scan 1 \(too-long\) holds 32769 points"):
            call()


def test_reuse_and_streams():
    from hyperpocket_amd import ops
    threads, tile = _geometry()
    points, offsets, _ = _mix(threads, tile)
    p, o = torch.from_numpy(points).to(CUDA), torch.from_numpy(offsets).to(CUDA)
    T, S = len(points), len(offsets) - 1
    out = {"label": torch.full((T,), 123456, dtype=torch.int32, device=CUDA),
           "size": torch.full((T,), -7, dtype=torch.int32, device=CUDA),
           "clusters": torch.full((S,), -7, dtype=torch.int32, device=CUDA),
           "largest": torch.full((S,), 99, dtype=torch.int32, device=CUDA)}
    cpu = lambda ts: tuple(t.cpu().numpy() for t in ts)
    got = ops.scan_clusters(p, o, MIX_RADII[2], out=out)                    # one component per scan first ...
    assert all(g.data_ptr() == out[name].data_ptr() for g, name in zip(got, NAMES))
    _same(cpu(got), _mix_law(threads, tile, MIX_RADII[2]), "poisoned out")
    got = ops.scan_clusters(p, o, MIX_RADII[1], out=out)                    # ... then pieces: nothing is left of the first call
    _same(cpu(got), _mix_law(threads, tile, MIX_RADII[1]), "second call, another radius")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.scan_clusters(p, o, MIX_RADII[1])
    side.synchronize()
    _same(cpu(other), _mix_law(threads, tile, MIX_RADII[1]), "another stream")

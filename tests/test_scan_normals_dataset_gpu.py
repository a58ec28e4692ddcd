"""GPU suite for DeviceScanDataset.normals and .without_edges (csrc/normals.hip through the dataset): normals() against
ops.scan_normals and the law, the motivating scene — a row of mixed pixels between two planes goes, the planes stay —,
composition with an earlier filter, and the cap."""
import functools

import numpy as np
import pytest
import torch

import knn_law
import normals_law as law

pytestmark = pytest.mark.gpu

K = 8


def _dataset(scans, **kw):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    return DeviceScanDataset([np.array(s) for s in scans], **kw)


@functools.lru_cache(maxsize=None)
def _edges():
    """The fixture, the law's curvature on it at k = 8 and the threshold it gives: half the smallest curvature of a planted
    row.  The planes' interior is exactly flat, so it passes any threshold."""
    cloud, planted, interior = law.edge_fixture()
    _, curvature, _ = law.normals_scan(cloud, knn_law.knn_scan(cloud, K)[0])
    assert not np.isnan(curvature).any() and (curvature[interior] == 0).all() and interior.sum() == 864 and planted.sum() == 24
    threshold = float(curvature[planted].min()) / 2
    assert 0.01 < threshold < 1 / 3
    for a in (cloud, planted, interior, curvature):
        a.setflags(write=False)
    return cloud, planted, interior, curvature, threshold


def test_normals_equal_the_op_and_change_nothing():
    from hyperpocket_amd import ops
    cloud, _, _, _, _ = _edges()
    shell = law.shell()[0]
    data = _dataset([cloud, shell], names=["edges", "shell"])
    before = data.points.clone()
    normal, curvature = data.normals()
    want = ops.scan_normals(data.points, data.offsets, 16)
    assert torch.equal(normal.view(torch.int32), want[0].view(torch.int32)) and torch.equal(curvature.view(torch.int32), want[1].view(torch.int32))
    assert tuple(normal.shape) == (len(cloud) + 1024, 3) and tuple(curvature.shape) == (len(cloud) + 1024,)
    views = torch.tensor([[0.5, 5.0, 0.5], [0.0, 0.0, 0.0]], device="cuda")
    for v in (views, views.cpu().numpy(), (0.5, 5.0, 0.5)):
        n, c = data.normals(k=K, viewpoint=v)
        w = ops.scan_normals(data.points, data.offsets, K, viewpoints=views if not isinstance(v, tuple) else views[0].contiguous())
        assert torch.equal(n.view(torch.int32), w[0].view(torch.int32)) and torch.equal(c.view(torch.int32), w[1].view(torch.int32))
    # ... which is the law's
    lists = np.concatenate([knn_law.knn_scan(cloud, K)[0], knn_law.knn_scan(shell, K)[0]])
    ln, lc, _ = law.normals_law(np.concatenate([cloud, shell]), [0, len(cloud), len(cloud) + 1024], lists, views.cpu().numpy())
    n, c = data.normals(k=K, viewpoint=views)
    assert np.array_equal(n.cpu().numpy().view(np.uint32), ln.view(np.uint32)) and np.array_equal(c.cpu().numpy().view(np.uint32), lc.view(np.uint32))
    # seen from above the planes face up; from its centre the shell faces inwards
    n = n.cpu().numpy()
    flat = np.flatnonzero(_edges()[2])
    assert (n[flat] == np.array([0, 1, 0], np.float32)).all()
    assert ((n[len(cloud):] * shell).sum(axis=1) < 0).all()
    assert torch.equal(data.points, before) and data.source_rows is None and data.kept is None


def test_mixed_pixels_between_two_planes_go():
    cloud, planted, interior, curvature, threshold = _edges()
    data = _dataset([cloud], names=["edge"])
    clean = data.without_edges(k=K, max_curvature=threshold)
    keep = curvature <= np.float32(threshold)
    assert not keep[planted].any() and keep[interior].all()         # the law: every planted row goes, the interior stays
    assert keep.sum() == 1126                                       # 864 interior rows and 262 of the 288 near the planted row
    assert clean.kept.tolist() == [int(keep.sum())] and clean.lengths.tolist() == [int(keep.sum())]
    assert np.array_equal(clean.source_rows.cpu().numpy(), np.flatnonzero(keep))
    assert np.array_equal(clean.points.cpu().numpy(), cloud[keep])
    assert clean.names == ["edge"] and data.lengths.tolist() == [len(cloud)] and data.source_rows is None     # a new dataset
    # the whole range of the threshold: 1/3 keeps every row with a curvature, 0 the exactly flat ones
    assert data.without_edges(k=K, max_curvature=1 / 3).lengths.tolist() == [len(cloud)]
    assert data.without_edges(k=K, max_curvature=0.0).lengths.tolist() == [int((curvature == 0).sum())]


def test_source_rows_compose_and_nan_rows_go():
    cloud, planted, interior, curvature, threshold = _edges()
    r = np.random.RandomState(4)
    box = r.uniform(-1, 1, (300, 3)).astype(np.float32)
    with_nan = cloud.copy()
    with_nan[5] = np.nan
    data = _dataset([with_nan, box], gt=np.zeros((2, 8, 3), np.float32), names=["a", "b"], outliers=(K, 3.0))
    assert data.source_rows is not None and 5 not in data.source_rows.tolist()
    first = data.source_rows.cpu().numpy()
    clean = data.without_edges(k=K, max_curvature=0.2)
    rows = clean.source_rows.cpu().numpy()
    assert (np.diff(rows) > 0).all() and np.isin(rows, first).all() and clean.kept.tolist() == clean.lengths.tolist()
    both = np.concatenate([with_nan, box])
    assert np.array_equal(clean.points.cpu().numpy(), both[rows])
    _, c, _ = law.normals_law(both[first], [0, int(data.lengths[0]), len(first)],
                              knn_law.knn_law(both[first], [0, int(data.lengths[0]), len(first)], K)[0])
    assert np.array_equal(rows, first[c <= np.float32(0.2)])
    assert clean.gt is data.gt and clean.names == ["a", "b"]
    with pytest.raises(ValueError, match=r"scan 1 \(b\) would be left without points by edge removal"):
        data.without_edges(k=K, max_curvature=0.0)                  # no neighbourhood of a random box is exactly flat


def test_the_cap_and_the_arguments():
    from hyperpocket_amd import ops
    n = ops.KNN_MAX_POINTS + 1
    big = torch.zeros((n, 3))
    big[:, 0] = torch.arange(n)
    data = _dataset([np.random.RandomState(0).rand(50, 3).astype(np.float32), big.numpy()], names=["small", "big"])
    with pytest.raises(ValueError, match=r"scan 1 \(big\) holds 65537 points: normal estimation takes scans of at most 65536 .* thin it first"):
        data.normals()
    with pytest.raises(ValueError, match=r"scan 1 \(big\) holds 65537 points: edge removal .* thin it first"):
        data.without_edges(max_curvature=0.1)
    for bad in (-0.1, 0.5):
        with pytest.raises(ValueError, match="max_curvature"):
            data.without_edges(max_curvature=bad)
    with pytest.raises(TypeError):
        data.without_edges()

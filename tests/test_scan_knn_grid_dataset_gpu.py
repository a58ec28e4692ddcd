"""GPU suite for the grid-backed search of DeviceScanDataset — with_search("grid"), and search="grid" of without_outliers — (csrc/knn_grid.hip through the dataset): the same rows and tensors as the
brute-force search on a small dataset, and a scan beyond the brute-force cap — refused by the default as before, served by the
grid with normals that are the law's, refused past the grid's own cap with the scan named."""
import numpy as np
import pytest
import torch

import knn_grid_law
import knn_law
import normals_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"


def _small():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    recipe, _ = knn_law.shell_with_strays(1024, seed=0)
    r = np.random.RandomState(8)
    sheet = r.uniform(-1, 1, (900, 3)).astype(np.float32)
    sheet[:, 2] = (0.05 * np.sin(4 * sheet[:, 0])).astype(np.float32)
    sheet[:40, 2] += r.uniform(0.2, 0.6, 40).astype(np.float32)                  # mixed pixels off the surface
    patch = np.concatenate([r.uniform(0, 1, (33, 2)), np.zeros((33, 1))], axis=1).astype(np.float32)       # flat: it stays
    scans = [recipe[np.isfinite(recipe).all(axis=1)], sheet, patch]
    return DeviceScanDataset(scans, names=["shell", "sheet", "few"], device=CUDA)


def test_grid_equals_brute_on_a_small_dataset():
    data = _small()
    grid = data.with_search("grid")
    assert data.search == "brute" and grid.search == "grid" and grid.points.data_ptr() == data.points.data_ptr()
    assert grid.with_search("brute").search == "brute"
    pairs = [(data.without_outliers(k=16, ratio=2.0), data.without_outliers(k=16, ratio=2.0, search="grid")),
             (data.without_outliers(k=16, ratio=2.0), grid.without_outliers(k=16, ratio=2.0)),
             (data.without_outliers(k=5, ratio=1.0, search="brute"), data.without_outliers(k=5, ratio=1.0, search="grid")),
             (grid.without_outliers(k=5, ratio=1.0, search="brute"), grid.without_outliers(k=5, ratio=1.0)),
             (data.without_edges(k=12, max_curvature=0.05), grid.without_edges(k=12, max_curvature=0.05))]
    assert pairs[1][1].search == "grid" and pairs[0][1].search == "brute"            # the setting travels; an argument does not set it
    for a, b in pairs:
        assert torch.equal(a.points.view(torch.int32), b.points.view(torch.int32)) and torch.equal(a.source_rows, b.source_rows)
        assert torch.equal(a.kept, b.kept) and torch.equal(a.offsets, b.offsets) and int(a.kept.sum()) < data.points.size(0)
    for kw in (dict(), dict(k=8, viewpoint=(0.0, 0.0, 5.0))):
        a, b = data.normals(**kw), grid.normals(**kw)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    for method in (lambda s: data.without_outliers(search=s), lambda s: data.with_search(s)):
        for bad in ("hash", 1, "GRID"):
            with pytest.raises(ValueError, match="search"):
                method(bad)
    with pytest.raises(ValueError, match="search"):
        data.with_search(None)


def bumpy_sheet(n, seed=0):
    r = np.random.RandomState(seed)
    xy = r.uniform(-1, 1, (n, 2))
    z = 0.1 * np.sin(5 * xy[:, 0]) * np.cos(3 * xy[:, 1]) + r.normal(0, 0.002, n)
    return np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)


def test_a_scan_beyond_the_brute_force_cap():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    k, view = 12, (0.0, 0.0, 3.0)
    sheet = bumpy_sheet(ops.KNN_MAX_POINTS + 2000)
    other = np.random.RandomState(1).uniform(-1, 1, (50, 3)).astype(np.float32)
    data = DeviceScanDataset([other, sheet], names=["small", "sensor"], device=CUDA)
    for method in (lambda: data.without_outliers(), lambda: data.normals(), lambda: data.without_edges(max_curvature=0.1)):
        with pytest.raises(ValueError, match=f"sensor.*{ops.KNN_MAX_POINTS} points \\(brute-force neighbours\\).*thin it first"):
            method()
    grid = data.with_search("grid")
    normal, curvature = grid.normals(k=k, viewpoint=view)
    rows = np.random.RandomState(3).permutation(len(sheet))[:256]
    lists = np.full((len(sheet), k), -1, dtype=np.int32)
    lists[rows] = knn_grid_law.knn_rows(sheet, k, rows)[0]
    ln, lc, _ = normals_law.normals_law(sheet, [0, len(sheet)], lists, np.array([view], np.float32))
    got_n, got_c = normal[50:].cpu().numpy(), curvature[50:].cpu().numpy()
    assert np.array_equal(got_n[rows].view(np.uint32), ln[rows].view(np.uint32))
    assert np.array_equal(got_c[rows].view(np.uint32), lc[rows].view(np.uint32))
    assert not np.isnan(got_c).any() and (got_n[:, 2] > 0.5).mean() > 0.99        # the sheet faces the viewpoint
    clean = data.without_outliers(search="grid")
    assert int(clean.kept[1]) > 0.9 * len(sheet) and clean.source_rows is not None
    thin = grid.without_edges(k=k, max_curvature=0.1)
    assert int(thin.kept[1]) > 0.9 * len(sheet)


def test_past_the_grid_cap_the_scan_is_named():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    assert ops.KNN_GRID_MAX_POINTS == ops.SCAN_MAX_POINTS                        # a dataset cannot hold a longer scan ...
    data = DeviceScanDataset([np.zeros((40, 3), np.float32), np.ones((60, 3), np.float32)], names=["a", "long one"], device=CUDA)
    data.lengths = data.lengths.clone()
    data.lengths[1] = ops.KNN_GRID_MAX_POINTS + 1                                # ... so the check is met with the length it reads
    grid = data.with_search("grid")
    for method in (lambda: data.without_outliers(search="grid"), lambda: grid.without_outliers(), lambda: grid.normals(),
                   lambda: grid.without_edges(max_curvature=0.1)):
        with pytest.raises(ValueError, match=f"long one.*{ops.KNN_GRID_MAX_POINTS}"):
            method()

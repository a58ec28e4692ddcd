"""GPU suite for the grid-backed outlier removal (csrc/knn_grid.hip): scan_outliers_grid bit for bit against
knn_law.outliers_law and against ops.scan_outliers, outlier_keep on sums that pass 64 bits against the long law, and the
recipe of the outlier tests at 70 000 rows — beyond the brute-force cap — as one scan."""
import numpy as np
import pytest
import torch

import knn_grid_law
import knn_law
from test_knn_grid_law_host import long_means

pytestmark = pytest.mark.gpu

CUDA = "cuda"


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(CUDA) if dtype is None else torch.as_tensor(np.array(a), dtype=dtype, device=CUDA)


@pytest.mark.parametrize("ratio", (0.0, 1.0, 2.0))
@pytest.mark.parametrize("k", (1, 16, 32))
def test_keep_mean_and_kept_equal_the_law_and_the_brute_force_op(k, ratio):
    from hyperpocket_amd import ops
    points, offsets, _, lists = knn_law.ragged_mix(ops.knn_grid_plan(k)[2])
    p, o = _dev(points), _dev(offsets)
    keep, mean, kept = ops.scan_outliers_grid(p, o, k, ratio)
    assert keep.dtype == torch.uint8 and mean.dtype == torch.float32 and kept.dtype == torch.int32
    wk, wm, wn = knn_law.outliers_law(points, offsets, k, ratio, lists=lists)
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), wm.view(np.uint32)), (k, ratio, "mean_dist")
    assert np.array_equal(keep.cpu().numpy().astype(bool), wk) and set(np.unique(keep.cpu().numpy())) <= {0, 1}, (k, ratio, "keep")
    assert np.array_equal(kept.cpu().numpy().astype(np.int64), wn), (k, ratio, "kept")
    brute = ops.scan_outliers(p, o, k, ratio)
    assert torch.equal(keep, brute[0]) and torch.equal(mean.view(torch.int32), brute[1].view(torch.int32)) and torch.equal(kept, brute[2])
    for cell in (0.25, 4.0):
        other = ops.scan_outliers_grid(p, o, k, ratio, cell=cell)
        assert torch.equal(keep, other[0]) and torch.equal(mean.view(torch.int32), other[1].view(torch.int32)) and torch.equal(kept, other[2])


def test_outlier_keep_beyond_64_bits():
    from hyperpocket_amd import ops
    m = long_means()
    part = np.isfinite(m)
    q = np.trunc(np.ldexp(m[part].astype(np.float64), 23)).astype(np.int64)       # M = 1.75: e = 0
    assert sum(int(v) * int(v) for v in q) >= 1 << 64                             # knn.hip's 64-bit sum would have wrapped
    short = np.random.RandomState(4).uniform(0, 2, 1000).astype(np.float32)
    short[::9] = np.inf
    means = np.concatenate([short, m, np.full(3, np.inf, np.float32), np.zeros(7, np.float32)])
    offsets = np.concatenate([[0], np.cumsum([len(short), len(m), 3, 7])])
    for ratio in (0.0, 0.5, 2.0):
        keep, kept = ops.outlier_keep(_dev(means), _dev(offsets, torch.int64), ratio)
        assert keep.dtype == torch.uint8 and kept.dtype == torch.int32
        keep, kept = keep.cpu().numpy(), kept.cpu().numpy()
        for s in range(4):
            wk, wn = knn_grid_law.keep_law_long(means[offsets[s]:offsets[s + 1]], ratio)
            assert np.array_equal(keep[offsets[s]:offsets[s + 1]].astype(bool), wk) and kept[s] == wn, (ratio, s)
        wk, wn = knn_law.keep_law(short, ratio)                                   # ... which is the short law where that is defined
        assert np.array_equal(keep[:len(short)].astype(bool), wk) and kept[0] == wn and kept[2] == 0 and kept[3] == 7
        assert 0 < kept[1] <= part.sum()


def test_the_recipe_at_70000_rows_as_one_scan():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    recipe, shell = knn_law.shell_with_strays(70000, seed=0)
    n = len(recipe)
    assert n == 70006 > ops.KNN_MAX_POINTS
    keep, mean, kept = ops.scan_outliers_grid(_dev(recipe), _dev([0, n], torch.int64), 16, 2.0)
    rows = np.concatenate([np.random.RandomState(2).permutation(n)[:250], np.setdiff1d(np.arange(n), shell)])      # the strays too
    want = knn_law.mean_dist_law(*knn_grid_law.knn_rows(recipe, 16, rows))
    assert np.array_equal(mean.cpu().numpy()[rows].view(np.uint32), want.view(np.uint32))
    wk, wn = knn_grid_law.keep_law_long(mean.cpu().numpy(), 2.0)
    assert np.array_equal(keep.cpu().numpy().astype(bool), wk) and int(kept[0]) == wn
    assert np.array_equal(np.flatnonzero(keep.cpu().numpy()), shell) and int(kept[0]) == 70000      # only the strays and the NaN row go
    clean = DeviceScanDataset([recipe[np.isfinite(recipe).all(axis=1)]], device=CUDA).without_outliers(search="grid")
    assert clean.points.size(0) == 70000 and clean.boxes()[1].item() == np.float32(1.1111112)

"""GPU suite for statistical outlier removal (csrc/knn.hip hp_scan_outliers, DeviceScanDataset.without_outliers): keep and
kept equal to tests/knn_law.py, mean_dist bit for bit, over every ratio and every instance of k; the dataset built on it; and
a dataset built without it is what it was."""
import numpy as np
import pytest
import torch

import knn_law
import scan_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(CUDA) if dtype is None else torch.as_tensor(np.array(a), dtype=dtype, device=CUDA)


def _run(points, offsets, k, ratio, **kw):
    from hyperpocket_amd import ops
    keep, mean, kept = ops.scan_outliers(_dev(np.asarray(points, np.float32)), _dev(offsets, torch.int64), k, ratio, **kw)
    assert keep.dtype == torch.uint8 and mean.dtype == torch.float32 and kept.dtype == torch.int32
    return keep.cpu().numpy(), mean.cpu().numpy(), kept.cpu().numpy()


def _same(got, want, what):
    (gk, gm, gn), (wk, wm, wn) = got, want
    assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32)), (what, "mean_dist", int((gm.view(np.uint32) != wm.view(np.uint32)).sum()))
    assert np.array_equal(gk.astype(bool), wk) and set(np.unique(gk)) <= {0, 1}, (what, "keep", int((gk.astype(bool) != wk).sum()))
    assert np.array_equal(gn.astype(np.int64), wn), (what, "kept")


def _edge_set():
    """The recipe, M == 0, a scan that is all NaN, single points, a pair, and a line with a gap, as one ragged set."""
    recipe, shell = knn_law.shell_with_strays(1024, seed=0)
    x = np.array([0, 1, 2, 3, 4, 5, 6, 16], dtype=np.float32)
    scans = [np.full((1, 3), 2.0, np.float32), recipe, np.full((90, 3), -0.75, np.float32), np.full((70, 3), np.nan, np.float32),
             np.zeros((1, 3), np.float32), np.array([[0, 0, 0], [0, 3, 4]], np.float32),
             np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)]
    lengths = [len(s) for s in scans]
    return np.concatenate(scans), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), shell


@pytest.mark.parametrize("ratio", (0.0, 1.0, 2.0))
@pytest.mark.parametrize("k", (1, 16, 32))
def test_keep_mean_and_kept_equal_the_law(k, ratio):
    from hyperpocket_amd import ops
    points, offsets, _, lists = knn_law.ragged_mix(ops.knn_points_plan(k)[2])
    _same(_run(points, offsets, k, ratio), knn_law.outliers_law(points, offsets, k, ratio, lists=lists), ("mix", k, ratio))
    points, offsets, shell = _edge_set()
    got = _run(points, offsets, k, ratio)
    _same(got, knn_law.outliers_law(points, offsets, k, ratio), ("edges", k, ratio))
    keep, mean, kept = got
    assert kept[[0, 2, 3, 4, 5]].tolist() == [0, 90, 0, 0, 2]      # a lone point has no neighbour; M == 0 keeps all; all NaN none
    assert np.isinf(mean[offsets[3]:offsets[4]]).all() and (mean[offsets[2]:offsets[3]] == 0).all()
    if (k, ratio) == (16, 2.0):
        assert kept[1] == 1024 and np.array_equal(np.flatnonzero(keep[offsets[1]:offsets[2]]), shell)
    if (k, ratio) == (1, 0.0):
        assert keep[offsets[6]:].tolist() == [1] * 7 + [0]


def test_out_buffers_are_reused_and_fully_written():
    from hyperpocket_amd import ops
    points, offsets, _ = _edge_set()
    T, S = len(points), len(offsets) - 1
    out = {"keep": torch.full((T,), 77, dtype=torch.uint8, device=CUDA), "mean_dist": torch.full((T,), float("nan"), device=CUDA),
           "kept": torch.full((S,), -5, dtype=torch.int32, device=CUDA)}
    want = knn_law.outliers_law(points, offsets, 16, 2.0)
    for _ in range(2):
        got = _run(points, offsets, 16, 2.0, out=out)
        _same(got, want, "out")
    assert np.array_equal(out["keep"].cpu().numpy(), got[0])


def _recipe_dataset(**kw):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    recipe, shell = knn_law.shell_with_strays(1024, seed=0)
    finite = recipe[np.isfinite(recipe).all(axis=1)]               # a dataset without the filter refuses non-finite rows
    r = np.random.RandomState(8)
    other = r.uniform(-2, 2, (500, 3)).astype(np.float32)
    other[7] = (40, 0, 0)
    scans = [finite, other, r.uniform(0, 1, (33, 3)).astype(np.float32)]
    gt = r.uniform(-1, 1, (3, 16, 3)).astype(np.float32)
    return DeviceScanDataset(scans, gt=gt, names=["a", "b", "c"], device=CUDA, **kw), scans


def test_dataset_without_outliers():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import ScanBatcher
    data, scans = _recipe_dataset()
    clean = data.without_outliers(k=16, ratio=2.0)
    points, offsets = np.concatenate(scans), data.offsets_host.numpy()
    keep, _, kept = knn_law.outliers_law(points, offsets, 16, 2.0)
    rows = np.flatnonzero(keep)
    assert clean.source_rows.dtype == torch.int64 and np.array_equal(clean.source_rows.cpu().numpy(), rows)
    assert np.array_equal(clean.points.cpu().numpy().view(np.uint32), points[rows].view(np.uint32))
    want_offsets = np.concatenate([[0], np.cumsum(kept)])
    assert np.array_equal(clean.kept.numpy(), kept) and np.array_equal(clean.offsets.cpu().numpy(), want_offsets)
    assert np.array_equal(clean.offsets_host.numpy(), want_offsets) and np.array_equal(clean.lengths.numpy(), kept)
    assert clean.names == data.names and clean.gt is data.gt and len(clean) == 3 and kept[0] == 1024 and not keep[offsets[1] + 7]
    assert data.source_rows is None and data.kept is None and data.points.size(0) == len(points)     # the original is untouched
    # boxes of the filtered set = scan_boxes of the law's kept rows; on the recipe the stray box 10.0 becomes the object's
    center, scale = clean.boxes()
    wc, ws = ops.scan_boxes(torch.from_numpy(points[rows]).to(CUDA), torch.from_numpy(want_offsets).to(CUDA))
    assert torch.equal(center, wc) and torch.equal(scale, ws)
    law = [scan_law.boxes_fp32(points[rows][want_offsets[s]:want_offsets[s + 1]]) for s in range(3)]
    lc, ls = np.stack([c for c, _ in law]), np.array([sc for _, sc in law], dtype=np.float32)
    assert np.array_equal(center.cpu().numpy(), lc) and np.array_equal(scale.cpu().numpy(), ls)
    assert float(data.boxes()[1][0]) == 10.0 and scale[0].item() == np.float32(1.1111112)
    # batches over the filtered set hold kept rows only
    batcher = ScanBatcher(clean, 2, target=64, normalize=True, seed=3)
    seen = 0
    for existing, ids, gt in batcher:
        index = batcher.last_index.cpu().numpy()
        for b, s in enumerate(ids.cpu().numpy()):
            source = clean.source_rows.cpu().numpy()[want_offsets[s] + index[b]]
            assert keep[source].all() and (source >= offsets[s]).all() and (source < offsets[s + 1]).all()
            want = (points[source] - lc[s]) / ls[s]
            assert np.array_equal(existing[b].cpu().numpy(), want.astype(np.float32))
            seen += 1
    assert seen == 3 and batcher.failures() == 0
    # filtering again composes source_rows
    twice = clean.without_outliers(k=16, ratio=2.0)
    assert np.array_equal(points[twice.source_rows.cpu().numpy()].view(np.uint32), twice.points.cpu().numpy().view(np.uint32))


def test_constructor_argument_equals_the_method():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    data, scans = _recipe_dataset()
    clean = data.without_outliers(k=8, ratio=1.0)
    built, _ = _recipe_dataset(outliers=(8, 1.0))
    for name in ("points", "offsets", "source_rows"):
        assert torch.equal(getattr(built, name), getattr(clean, name)), name
    assert torch.equal(built.kept, clean.kept) and torch.equal(built.lengths, clean.lengths)
    assert torch.equal(built.boxes()[0], clean.boxes()[0]) and torch.equal(built.boxes()[1], clean.boxes()[1])
    # with the filter the constructor takes the recipe as it is: the NaN row goes with the strays
    recipe, shell = knn_law.shell_with_strays(1024, seed=0)
    raw = DeviceScanDataset([recipe], device=CUDA, outliers=(16, 2.0))
    assert np.array_equal(raw.source_rows.cpu().numpy(), shell) and raw.boxes()[1].item() == np.float32(1.1111112)
    with pytest.raises(ValueError):
        DeviceScanDataset([recipe], device=CUDA)


def test_an_emptied_or_oversized_scan_raises():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    lone = [np.random.RandomState(1).uniform(-1, 1, (50, 3)).astype(np.float32), np.ones((1, 3), np.float32)]
    data = DeviceScanDataset(lone, names=["fine", "lonely"], device=CUDA)
    with pytest.raises(ValueError, match="lonely"):                # a single point has no neighbour: nothing would be left
        data.without_outliers()
    with pytest.raises(ValueError, match="lonely"):
        DeviceScanDataset(lone, names=["fine", "lonely"], device=CUDA, outliers=(16, 2.0))
    big = DeviceScanDataset([np.zeros((ops.KNN_MAX_POINTS + 1, 3), np.float32), lone[0]], device=CUDA)
    with pytest.raises(ValueError, match=str(ops.KNN_MAX_POINTS)):
        big.without_outliers()


def test_a_dataset_without_the_argument_is_what_it_was():
    """The parent's code path, restated: pack, upload, the finite check, the transform; boxes by ops.scan_boxes."""
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    r = np.random.RandomState(6)
    scans = [r.uniform(-3, 3, (n, 3)).astype(np.float32) for n in (5, 700, 64, 1)]
    m = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    for transform in (None, m):
        data = DeviceScanDataset(scans, transform=transform, device=CUDA)
        points = torch.cat([torch.from_numpy(s) for s in scans]).to(CUDA)
        if transform is not None:
            points = points @ torch.from_numpy(m).to(CUDA).t()
        offsets = torch.tensor([0, 5, 705, 769, 770], dtype=torch.int64)
        assert torch.equal(data.points, points.contiguous()) and torch.equal(data.offsets.cpu(), offsets)
        assert torch.equal(data.offsets_host, offsets) and torch.equal(data.lengths, offsets[1:] - offsets[:-1])
        center, scale = ops.scan_boxes(points.contiguous(), offsets.to(CUDA))
        assert torch.equal(data.boxes()[0], center) and torch.equal(data.boxes()[1], scale)
        assert data.source_rows is None and data.kept is None

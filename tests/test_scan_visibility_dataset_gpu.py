"""GPU suite for what is built on ops.scan_visibility: DeviceScanDataset.seen_from and virtual_scans, and
utils/evaluation/visibility.completion_consistency — against tests/visibility_law.py on the sphere shell of DESIGN.md 3t."""
import numpy as np
import pytest
import torch

import visibility_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32 = np.float32
SCANS = (law.shell(2048), law.shell(500, seed=4, radius=0.5) + f32(0.25))
VIEWS = np.array([law.SHELL_VIEW, [-2.0, 0.5, 0.25]], f32)


def _dataset(**kw):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    return DeviceScanDataset([torch.from_numpy(s) for s in SCANS], names=["shell", "ball"], device=CUDA, **kw)


@pytest.fixture(scope="module")
def want():
    return [law.visibility_scan(s, v, 32, 2, 0.01, 2.0) for s, v in zip(SCANS, VIEWS)]


def test_seen_from_keeps_the_law_s_rows(want):
    data = _dataset(gt=np.stack([law.shell(64), law.shell(64, seed=9)]))
    assert data.viewpoints is None
    seen = data.seen_from(VIEWS, window=2)
    rows = [np.flatnonzero(r["label"] == law.ON_SURFACE) for r in want]
    assert seen.kept.tolist() == [len(r) for r in rows] and seen.lengths.tolist() == seen.kept.tolist()
    assert (seen.source_rows.cpu().numpy() == np.concatenate([rows[0], rows[1] + len(SCANS[0])])).all()
    assert (seen.points.cpu().numpy() == np.concatenate([SCANS[0][rows[0]], SCANS[1][rows[1]]])).all()
    assert seen.viewpoints.dtype == torch.float32 and seen.viewpoints.is_cuda and (seen.viewpoints.cpu().numpy() == VIEWS).all()
    assert seen.names == ["shell", "ball"] and seen.gt is data.gt and data.viewpoints is None and data.kept is None
    assert 0.25 < len(rows[0]) / 2048 < 0.4                # a sensor sees about a third of a sphere from 2.7 radii
    again = seen.without_outliers(k=8, ratio=3.0)          # the viewpoints travel with what is filtered from it
    assert again.viewpoints is seen.viewpoints
    one = data.seen_from(tuple(VIEWS[0]), window=2)         # one triple for all scans
    assert (one.viewpoints.cpu().numpy() == VIEWS[[0, 0]]).all() and one.kept[0] == seen.kept[0]


def test_nearest_leaves_at_most_one_row_per_pixel(want):
    near = _dataset().seen_from(VIEWS, window=2, keep="nearest")
    rows = [np.flatnonzero((r["label"] == law.ON_SURFACE) & (r["winner"] != 0)) for r in want]
    assert near.kept.tolist() == [len(r) for r in rows]
    assert (near.source_rows.cpu().numpy() == np.concatenate([rows[0], rows[1] + len(SCANS[0])])).all()
    for s in range(2):
        pixel = law.project(near.scan(s).cpu().numpy(), VIEWS[s], 32)[1]
        assert len(np.unique(pixel)) == len(pixel) > 50


def test_a_scan_left_empty_is_named():
    """Of finite rows the nearest one is never hidden, so keep="visible" cannot empty a scan; a scan that is nothing but its
    own sensor position owns no pixel, and keep="nearest" has nothing to keep of it."""
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    data = DeviceScanDataset([torch.from_numpy(SCANS[1]), torch.tensor([[1.0, 2.0, 3.0]] * 3)], names=["ball", "sensor"], device=CUDA)
    views = np.array([VIEWS[1], [1.0, 2.0, 3.0]], f32)
    assert data.seen_from(views).kept.tolist()[1] == 3     # at the viewpoint: label 1
    with pytest.raises(ValueError, match=r"scan 1 \(sensor\) would be left without points"):
        data.seen_from(views, keep="nearest")


def test_virtual_scans_feed_the_batcher():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher, viewpoints_on_sphere
    clouds = np.stack([law.shell(2048), law.shell(2048, seed=5) * f32([1.0, 0.5, 0.25])])
    views = viewpoints_on_sphere(6, 2.5, seed=1).reshape(2, 3, 3)
    data = DeviceScanDataset.virtual_scans(torch.from_numpy(clouds).to(CUDA), views, names=["sphere", "disc"], window=2)
    assert len(data) == 6 and data.names == ["sphere~0", "sphere~1", "sphere~2", "disc~0", "disc~1", "disc~2"]
    assert tuple(data.gt.shape) == (6, 2048, 3) and (data.gt.cpu().numpy() == clouds[[0, 0, 0, 1, 1, 1]]).all()
    assert (data.viewpoints.cpu().numpy() == views.reshape(6, 3)).all()
    for i in range(6):
        r = law.visibility_scan(clouds[i // 3], views[i // 3, i % 3], 32, 2, 0.01, 2.0)
        assert (data.scan(i).cpu().numpy() == clouds[i // 3][r["label"] == law.ON_SURFACE]).all(), i
        assert 0 < int(data.kept[i]) < 2048
    flat = DeviceScanDataset.virtual_scans(clouds, views[:, 0], window=2)        # (S,3) viewpoints, host clouds, no names
    assert len(flat) == 2 and flat.names == ["0~0", "1~0"] and flat.kept.tolist() == [int(data.kept[0]), int(data.kept[3])]
    batches = list(ScanBatcher(data, 4))
    assert [tuple(b[0].shape) for b in batches] == [(4, 1024, 3), (2, 1024, 3)]
    existing, ids, gt = batches[1]
    assert ids.tolist() == [4, 5] and (gt.cpu().numpy() == clouds[[1, 1]]).all()
    part = set(map(tuple, data.scan(4).cpu().numpy().tolist()))
    assert set(map(tuple, existing[0].cpu().numpy().tolist())) <= part


def test_completion_consistency_shares_are_the_law_s_counts(want):
    from hyperpocket_amd.utils.evaluation.visibility import LABELS, completion_consistency
    seen = _dataset().seen_from(VIEWS, window=2)
    M = 1024
    completions = np.stack([law.shell(M, seed=1, radius=1.4), law.shell(M, seed=2, radius=0.3) + f32(0.25)])
    res = completion_consistency(seen, torch.from_numpy(completions))
    counts = []
    for s in range(2):
        visible = SCANS[s][want[s]["label"] == law.ON_SURFACE]
        r = law.visibility_scan(visible, VIEWS[s], 32, 1, 0.01, 2.0, queries=completions[s])
        assert (res["label"].cpu().numpy()[s * M:(s + 1) * M] == r["label"]).all()
        counts.append(np.bincount(r["label"], minlength=5)[:4])
    counts = np.array(counts)
    assert LABELS == ("seen_through", "on_surface", "hidden", "unobserved") and counts[0, 0] > 0 and counts[1, 2] > M // 2
    assert res["shares"].is_cuda and (res["shares"].cpu().numpy() == counts / float(M)).all()
    assert not res["mean"].is_cuda and (res["mean"].numpy() == (counts / float(M)).mean(0)).all()
    # a ragged pair, other viewpoints and parameters
    ragged = (np.concatenate([completions[0][:100], completions[1]]), [0, 100, 100 + M])
    res = completion_consistency(seen, (torch.from_numpy(ragged[0]), torch.tensor(ragged[1])), viewpoints=VIEWS[::-1].copy(),
                                 resolution=16, window=2)
    kept = [SCANS[s][want[s]["label"] == law.ON_SURFACE] for s in range(2)]
    r = law.visibility_law(np.concatenate(kept), [0, len(kept[0]), len(kept[0]) + len(kept[1])], VIEWS[::-1], 16, 2,
                           queries=ragged[0], query_offsets=ragged[1])
    assert (res["label"].cpu().numpy() == r["label"]).all()
    want_counts = np.array([np.bincount(r["label"][:100], minlength=5)[:4] / 100.0, np.bincount(r["label"][100:], minlength=5)[:4] / M])
    assert (res["shares"].cpu().numpy() == want_counts).all()

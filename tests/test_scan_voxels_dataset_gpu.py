"""GPU suite for DeviceScanDataset.thinned (csrc/voxels.hip through the dataset): the kept rows against tests/voxel_law.py,
composition with an earlier filter, what is carried over, the refusal of rows beyond the grid, and the chain that motivates
the stage — a scene too long for the cluster kernel, thinned to a row budget, then clustered."""
import functools

import numpy as np
import pytest
import torch

import voxel_law

pytestmark = pytest.mark.gpu

f32 = np.float32


def _dataset(scans, **kw):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    return DeviceScanDataset([np.array(s) for s in scans], **kw)


@functools.lru_cache(maxsize=None)
def _scans():
    """Two scans, read-only: 3000 rows in three blobs with 30 far strays, and 500 uniform rows."""
    r = np.random.RandomState(21)
    centre = np.array([[-0.5, 0.0, 0.2], [0.4, 0.3, -0.1], [0.1, -0.6, 0.5]])
    a = centre[r.randint(0, 3, 3000)] + r.normal(0, 0.06, (3000, 3))
    a[r.choice(3000, 30, replace=False)] = r.uniform(-3, 3, (30, 3))
    b = r.uniform(-1, 1, (500, 3))
    out = a.astype(f32), b.astype(f32)
    for c in out:
        c.setflags(write=False)
    return out


@pytest.mark.parametrize("keep", voxel_law.KEEPS)
def test_thinned_keeps_the_laws_rows(keep):
    a, b = _scans()
    gt = np.random.RandomState(1).rand(2, 16, 3).astype(f32)
    data = _dataset([a, b], names=["blobs", "box"], gt=gt)
    assert data.voxels is None
    thin = data.thinned(voxel=0.05, keep=keep)
    want = [voxel_law.voxel_scan(c, 0.05, None, keep) for c in (a, b)]
    masks = [w["keep"].astype(bool) for w in want]
    assert thin.lengths.tolist() == thin.kept.tolist() == [w["kept"] for w in want] and thin.kept.dtype == torch.int64
    assert np.array_equal(thin.points.cpu().numpy(), np.concatenate([a[masks[0]], b[masks[1]]]))     # rows of the scans, bit for bit
    assert np.array_equal(thin.source_rows.cpu().numpy(), np.flatnonzero(np.concatenate(masks)))
    assert thin.offsets_host.tolist() == [0, want[0]["kept"], want[0]["kept"] + want[1]["kept"]]
    assert thin.offsets.cpu().tolist() == thin.offsets_host.tolist()
    assert thin.voxels.dtype == torch.float32 and thin.voxels.cpu().tolist() == [float(f32(0.05))] * 2
    assert thin.names == ["blobs", "box"] and np.array_equal(thin.gt.cpu().numpy(), gt)
    assert data.lengths.tolist() == [3000, 500] and data.source_rows is None and data.voxels is None      # a new dataset
    # the grid hangs on the coordinate origin: thinning again at the same voxel changes nothing
    again = thin.thinned(voxel=0.05, keep=keep)
    assert np.array_equal(again.points.cpu().numpy(), thin.points.cpu().numpy())
    assert np.array_equal(again.source_rows.cpu().numpy(), thin.source_rows.cpu().numpy())


def test_thinned_composes_with_the_other_filters():
    a, b = _scans()
    floor = np.random.RandomState(2).uniform(-1, 1, (4000, 3)) * [1, 0, 1] + [0, -0.9, 0]      # a plane y = -0.9 under the blobs
    scene = np.concatenate([a, floor.astype(f32)])
    data = _dataset([scene, b], names=["scene", "box"]).without_plane(0.01)
    clean = data.without_outliers(k=8, ratio=2.0)
    assert clean.lengths[0] < data.lengths[0]
    thin = clean.thinned(voxel=0.25, origin="center")
    pts = clean.points.cpu().numpy()
    off = clean.offsets_host.numpy()
    centre = np.stack([voxel_law.box(pts[off[s]:off[s + 1]])[0] for s in range(2)])
    want = voxel_law.voxel_law(pts, off, 0.25, centre, "center")
    mask = want["keep"].astype(bool)
    assert thin.kept.tolist() == want["kept"].tolist() and (want["kept"] < clean.lengths.numpy()).all()
    assert np.array_equal(thin.source_rows.cpu().numpy(), clean.source_rows.cpu().numpy()[mask])          # composed
    assert np.array_equal(thin.points.cpu().numpy(), pts[mask])
    assert np.array_equal(scene[thin.source_rows.cpu().numpy()[:int(thin.kept[0])]], thin.scan(0).cpu().numpy())     # down to the file's rows
    assert thin.planes is data.planes and thin.plane_found is data.plane_found and thin.plane_found.tolist() == [True, False]
    assert thin.names == ["scene", "box"]


def test_rows_beyond_the_grid_are_refused_by_name():
    a, b = _scans()
    far = (b.astype(np.float64) + 1e6).astype(f32)                 # extent 2 at +1e6: at voxel 0.01 the cells run past 2^20
    data = _dataset([a, far], names=["near", "far.npy"])
    with pytest.raises(ValueError, match=r"scan 1 \(far\.npy\).*voxel is too small.*origin=\"center\".*larger voxel"):
        data.thinned(voxel=0.01)
    thin = data.thinned(voxel=0.01, origin="center")               # the remedy the message names
    want = voxel_law.voxel_scan(far, 0.01, voxel_law.box(far)[0])
    assert thin.kept.tolist()[1] == want["kept"] and want["beyond"] == 0
    assert data.thinned(voxel=4.0).kept.tolist()[1] >= 1            # ... and the other one


@functools.lru_cache(maxsize=None)
def _scene():
    """40 000 rows, more than the cluster kernel takes: four objects of 10 000 rows, Gaussian with sigma 0.05, one metre
    apart, rows shuffled.  Read-only."""
    r = np.random.RandomState(22)
    centre = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], dtype=np.float64)
    cloud = (np.repeat(centre, 10000, axis=0) + r.normal(0, 0.05, (40000, 3)))[r.permutation(40000)].astype(f32)
    cloud.setflags(write=False)
    return cloud


def test_a_scene_too_long_for_the_cluster_kernel_is_thinned_and_then_clustered():
    from hyperpocket_amd import ops
    scene, (_, small) = _scene(), _scans()
    small = small.copy()
    small = np.concatenate([small, small[:500]])                    # 1000 rows, left whole
    assert len(scene) > ops.CLUSTER_MAX_POINTS
    data = _dataset([scene, small], names=["scene", "small"])
    with pytest.raises(ValueError, match="thin it first"):
        data.keep_clusters(radius=0.1)
    thin = data.thinned(max_points=4096)
    edge, want = voxel_law.thin_to(scene, 4096)
    assert thin.lengths.tolist() == [want["kept"], 1000] and want["kept"] <= 4096
    voxels = thin.voxels.cpu().numpy()
    assert voxels.dtype == f32 and voxels[:1].view(np.uint32) == np.array([edge]).view(np.uint32) and np.isnan(voxels[1])
    assert np.array_equal(thin.scan(0).cpu().numpy(), scene[want["keep"].astype(bool)])
    assert np.array_equal(thin.scan(1).cpu().numpy(), small)        # bit for bit
    assert np.array_equal(thin.source_rows.cpu().numpy(),
                          np.concatenate([np.flatnonzero(want["keep"]), len(scene) + np.arange(1000)]))
    main = thin.keep_clusters(radius=0.1)                           # runs now: the objects are a metre apart
    assert 1 <= main.lengths[0] <= want["kept"] and main.lengths[0] >= want["kept"] // 8
    pieces = thin.split_clusters(radius=0.1, min_points=want["kept"] // 8)
    assert (pieces.source_scan == 0).sum() == 4 and tuple(pieces.voxels.shape) == (len(pieces),)


def test_scans_within_the_budget_are_all_left_whole():
    a, b = _scans()
    data = _dataset([a, b], names=["blobs", "box"])
    thin = data.thinned(max_points=3000, keep="first", origin="center")
    assert thin.lengths.tolist() == [3000, 500] and torch.isnan(thin.voxels).all() and thin.voxels.dtype == torch.float32
    assert np.array_equal(thin.points.cpu().numpy(), np.concatenate([a, b]))
    assert np.array_equal(thin.source_rows.cpu().numpy(), np.arange(3500))
    one_more = data.thinned(max_points=2999)                        # the budget is inclusive: now scan 0 is thinned
    assert one_more.lengths.tolist()[0] == voxel_law.thin_to(a, 2999)[1]["kept"] <= 2999 and one_more.lengths.tolist()[1] == 500


def test_a_scan_no_grid_fits_is_refused_by_name():
    """1500 rows on one point at 3e6: the box scale is 0, so the bisection runs between 0 and 1, and without an origin every
    edge it tries leaves the rows beyond 2^20 cells — refused, naming the scan.  Anchored at the scan's centre u = 0: one cell
    at every edge, all 16 rounds are accepted and the edge is 2^-16."""
    a, _ = _scans()
    far = np.full((1500, 3), 3e6, dtype=f32)
    data = _dataset([a, far], names=["near", "far"])
    with pytest.raises(ValueError, match=r"scan 1 \(far\) cannot be thinned to 1024 rows"):
        data.thinned(max_points=1024)
    thin = data.thinned(max_points=1024, origin="center")
    centres = [voxel_law.box(c)[0] for c in (a, far)]
    want = [voxel_law.thin_to(c, 1024, origin=o) for c, o in zip((a, far), centres)]
    assert thin.lengths.tolist() == [want[0][1]["kept"], 1] and want[0][1]["kept"] <= 1024
    assert np.array_equal(thin.voxels.cpu().numpy().view(np.uint32), np.array([want[0][0], want[1][0]], f32).view(np.uint32))
    assert want[1][0] == f32(2.0 ** -16)
    assert np.array_equal(thin.source_rows.cpu().numpy(), np.concatenate([np.flatnonzero(want[0][1]["keep"]), [3000]]))

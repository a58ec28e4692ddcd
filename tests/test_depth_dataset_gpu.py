"""GPU suite for DeviceScanDataset.from_depth_images: the synthetic scene of tests/depth_law.py (a floor, a box and a sphere)
comes in as depth images and leaves as a dataset with viewpoints, pixel numbers and pixel-grid normals that follow the rows
through the filters; the chain down to one object; the free-space check without viewpoints given; the refusals."""
import functools

import numpy as np
import pytest
import torch

import depth_law as law

pytestmark = pytest.mark.gpu

B, H, W = 2, 120, 160


@functools.lru_cache(maxsize=None)
def _scene():
    s = law.scene(0, B, H, W)
    return s, law.depth_law(s["depth"], s["K"], s["poses"], s["masks"])


@functools.lru_cache(maxsize=None)
def _data():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    s, _ = _scene()
    return DeviceScanDataset.from_depth_images(s["depth"], s["K"], poses=s["poses"], masks=s["masks"], names=["left", "right"])


def test_the_dataset_as_built():
    (s, want), data = _scene(), _data()
    assert len(data) == B and data.names == ["left", "right"] and data.search == "brute" and data.source_rows is None
    assert data.lengths.tolist() == np.diff(want["offsets"]).tolist() and data.offsets_host.tolist() == want["offsets"].tolist()
    assert data.offsets.cpu().tolist() == want["offsets"].tolist() and data.points.is_cuda
    assert (data.viewpoints.cpu().numpy() == s["poses"][:, :, 3]).all() and data.viewpoints.dtype == torch.float32
    for got, name in ((data.points, "points"), (data.pixel_normals, "normals"), (data.pixels, "pixel")):
        assert got.is_contiguous() and got.shape == want[name].shape and (got.cpu().numpy() == want[name]).all(), name
    assert data.row_pixels() is data.pixels and data.row_normals() is data.pixel_normals
    assert data.boxes()[0].shape == (B, 3)                          # the rest of the dataset works on it


def _back_projects(ds, s):
    """The rows of `ds` against the images themselves: row_pixels() decodes to (b, v, u) inside the row's scan, whose depth
    back-projects to the row; row_normals() is unit or zero and faces the sensor.  Independent of source_rows."""
    pixel = ds.row_pixels().cpu().numpy()
    assert len(pixel) == ds.points.size(0) and len(np.unique(pixel)) == len(pixel)
    b, rest = np.divmod(pixel, H * W)
    v, u = np.divmod(rest, W)
    assert (b == np.repeat(np.arange(B), ds.lengths.numpy())).all()
    z = s["depth"][b, v, u] * 0.001
    assert (z > 0).all() and (s["masks"][b, v, u] != 0).all()
    fx, fy, cx, cy = s["K"]
    q = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    M = s["poses"].astype(np.float64)[b]
    p = np.einsum("nij,nj->ni", M[:, :, :3], q) + M[:, :, 3]
    assert np.abs(ds.points.cpu().numpy() - p).max() <= 2.0 ** -22 * np.abs(p).max()         # a few fp32 roundings of the largest coordinate
    n = ds.row_normals().cpu().numpy().astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    has = length > 0                                               # a pixel without a usable pair of neighbours has the zero normal
    assert has.mean() > 0.9 and np.abs(length[has] - 1.0).max() < 1e-6 and (n[~has] == 0).all()
    to_sensor = ds.viewpoints.cpu().numpy().astype(np.float64)[b] - p
    assert (np.sum(n * to_sensor, axis=1)[has] > 0).all()          # facing the sensor


def test_pixels_and_normals_follow_the_rows_through_a_filter():
    (s, _), data = _scene(), _data()
    clean = data.without_outliers()
    assert clean.source_rows is not None and 0 < clean.points.size(0) < data.points.size(0)
    assert torch.equal(clean.row_pixels(), data.pixels[clean.source_rows])
    assert torch.equal(clean.row_normals(), data.pixel_normals[clean.source_rows])
    assert torch.equal(clean.viewpoints, data.viewpoints)
    _back_projects(clean, s)


def test_the_lineage_ends_where_rows_are_reordered_or_moved():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    data = _data()
    objects = data.without_plane(0.01)
    pieces = objects.split_clusters(0.05, min_points=50)
    assert pieces.pixels is None and pieces.pixel_normals is None and pieces.viewpoints is not None
    for broken in (pieces, objects.merged_views([[0, 1]], max_dist=0.05, iters=2), objects.aligned_to(objects, max_dist=0.05, iters=2),
                   DeviceScanDataset([torch.rand(50, 3)])):
        with pytest.raises(ValueError, match="from_depth_images"):
            broken.row_normals()
        with pytest.raises(ValueError, match="from_depth_images"):
            broken.row_pixels()
    assert torch.equal(objects.row_pixels(), data.pixels[objects.source_rows])


def test_the_chain_leaves_one_object():
    data = _data()
    main = data.without_plane(0.01).keep_clusters(0.05)
    p = main.points.cpu().numpy().astype(np.float64)
    assert (main.lengths > 200).all()
    lo, hi, tol = np.array([-0.45, 0.0, 1.3]), np.array([-0.15, 0.3, 1.6]), 0.005
    for s in range(B):
        rows = p[main.offsets_host[s]:main.offsets_host[s + 1]]
        on_box = ((rows >= lo - tol) & (rows <= hi + tol)).all(1)
        on_sphere = np.abs(np.linalg.norm(rows - [0.3, 0.2, 1.5], axis=1) - 0.2) <= tol
        assert on_box.all() or on_sphere.all(), (s, on_box.mean(), on_sphere.mean())
    assert torch.equal(main.row_pixels(), data.pixels[main.source_rows]) and main.planes is not None
    _back_projects(main, _scene()[0])                               # two filters composed: the rows still are their pixels' points
    _back_projects(main.without_outliers(), _scene()[0])            # ... and three


def test_completion_consistency_needs_no_viewpoints():
    from hyperpocket_amd.utils.evaluation.visibility import completion_consistency
    data = _data()
    own = completion_consistency(data, (data.points, data.offsets))
    assert own["shares"].shape == (B, 4) and own["label"].shape == (data.points.size(0),)
    assert (own["shares"][:, 0] == 0).all()                         # a recorded row never lies in front of everything recorded
    scan = torch.repeat_interleave(torch.arange(B, device=data.device), data.lengths.to(data.device))
    halfway = (data.points + data.viewpoints[scan]) * 0.5           # in the sensor's free space
    free = completion_consistency(data, (halfway, data.offsets))
    assert (free["shares"][:, 0] > 0.5).all()
    assert torch.equal(completion_consistency(data, (halfway, data.offsets), viewpoints=data.viewpoints)["label"], free["label"])


def test_refusals():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    s, _ = _scene()
    depth = s["depth"].copy()
    depth[1] = 0
    with pytest.raises(ValueError, match=r"image 1 \(right\)"):
        DeviceScanDataset.from_depth_images(depth, s["K"], poses=s["poses"], names=["left", "right"])
    with pytest.raises(ValueError, match="image 0"):
        DeviceScanDataset.from_depth_images(s["depth"], s["K"], near=50.0, far=60.0)
    with pytest.raises(ValueError):
        DeviceScanDataset.from_depth_images(s["depth"], s["K"], names=["one"])
    with pytest.raises(ValueError):
        DeviceScanDataset.from_depth_images(s["depth"].astype(np.int32), s["K"])
    # a whole sensor image is beyond the brute-force searches: the dataset says so
    big = np.full((1, 300, 300), 1500, np.uint16)
    assert 300 * 300 > ops.KNN_MAX_POINTS
    data = DeviceScanDataset.from_depth_images(big, (250.0, 250.0, 149.5, 149.5))
    assert data.search == "grid" and data.lengths.tolist() == [90000] and data.viewpoints.tolist() == [[0.0, 0.0, 0.0]]

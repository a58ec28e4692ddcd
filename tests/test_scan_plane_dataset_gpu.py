"""GPU suite for DeviceScanDataset.without_plane (csrc/plane.hip through the dataset): the motivating scene — objects on a
floor are one component until the floor goes —, the fitted plane against the planted one, composition with the other
filters, refine=False against the law, scans without a plane, the constructor keyword and the upright transform."""
import functools

import numpy as np
import pytest
import torch

import plane_law

pytestmark = pytest.mark.gpu

NORMAL = np.array([0.2, 0.95, -0.15]) / np.linalg.norm([0.2, 0.95, -0.15])
ORIGIN = np.array([0.3, -0.2, 0.5])
SIGMA, HALF, FLOOR, BLOB = 0.002, 0.6, 3000, 400
CENTRES = ((-0.35, -0.3), (0.4, -0.25), (0.0, 0.4))


@functools.lru_cache(maxsize=None)
def _scene():
    """(cloud (4200,3) float32, is_floor (4200) bool, unit normal, d): a floor patch of 3000 rows, 1.2 x 1.2, Gaussian noise
    of sigma 0.002 along the normal, tilted and moved off the origin; three blobs of 400 rows, cylinders of radius 0.08
    and height 0.3 whose lowest rows hover 0.03 above the floor — closer than the cluster radius 0.05, so each is joined to
    the floor, and further than the threshold 0.01, so no blob row is a matter of rounding.  Shuffled.  Read-only."""
    r = np.random.RandomState(17)
    q, _ = np.linalg.qr(np.stack([NORMAL, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], axis=1))
    e1, e2 = q[:, 1], q[:, 2]                                       # an orthonormal pair in the plane
    uv = r.uniform(-HALF, HALF, (FLOOR, 2))
    noise = r.normal(0, SIGMA, FLOOR)
    assert np.abs(noise).max() < 0.009                              # 4.5 sigma: every floor row is inside the band for good
    local = [np.stack([uv[:, 0], noise, uv[:, 1]], axis=1)]
    for cu, cv in CENTRES:
        rad, ang = 0.08 * np.sqrt(r.rand(BLOB)), r.uniform(0, 2 * np.pi, BLOB)
        local.append(np.stack([cu + rad * np.cos(ang), r.uniform(0.03, 0.33, BLOB), cv + rad * np.sin(ang)], axis=1))
    local = np.concatenate(local)
    cloud = ORIGIN + local[:, [0]] * e1 + local[:, [1]] * NORMAL + local[:, [2]] * e2
    is_floor = np.arange(len(cloud)) < FLOOR
    order = r.permutation(len(cloud))
    cloud, is_floor = cloud[order].astype(np.float32), is_floor[order]
    for a in (cloud, is_floor):
        a.setflags(write=False)
    return cloud, is_floor, NORMAL, -float(NORMAL @ ORIGIN)


def _dataset(scans, **kw):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    return DeviceScanDataset([np.array(s) for s in scans], **kw)


def _angle_deg(a, b):
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)))


def test_objects_on_a_floor_come_apart_once_the_floor_is_gone():
    cloud, is_floor, normal, d = _scene()
    data = _dataset([cloud], names=["scene"])
    assert len(data.split_clusters(radius=0.05, min_points=200)) == 1          # the floor joins everything
    assert data.planes is None and data.plane_found is None
    off = data.without_plane(0.01)
    pieces = off.split_clusters(radius=0.05, min_points=200)
    assert len(pieces) == 3 and pieces.lengths.tolist() == [BLOB] * 3
    assert off.plane_found.tolist() == [True] and off.kept.tolist() == [3 * BLOB] and off.lengths.tolist() == [3 * BLOB]
    assert np.array_equal(off.source_rows.cpu().numpy(), np.flatnonzero(~is_floor))    # exactly the blobs, in scan order
    assert np.array_equal(off.points.cpu().numpy(), cloud[~is_floor])
    assert off.names == ["scene"] and data.lengths.tolist() == [len(cloud)] and data.source_rows is None      # a new dataset
    # The refit is least squares over the 3000 floor rows (no blob row comes within 0.01): the normal's angle has a standard
    # deviation of sigma / (sqrt(N) * rms lever) = 0.002 / (54.8 * 0.6 / sqrt(3)) = 1.1e-4 rad = 0.006 degrees per in-plane
    # axis, and d one of sigma / sqrt(N) = 3.7e-5 plus that angle times the patch centre's distance from the origin (0.62):
    # 1 degree and 0.005 are more than a hundred of either.
    plane = off.planes.cpu().numpy().astype(np.float64)[0]
    assert off.planes.dtype == torch.float32 and tuple(off.planes.shape) == (1, 4)
    assert abs(np.linalg.norm(plane[:3]) - 1) < 1e-6
    assert _angle_deg(plane[:3], normal) < 1.0 and abs(plane[3] - d) < 0.005
    assert (cloud[~is_floor].astype(np.float64) @ plane[:3] + plane[3] > 0.02).all()   # it points towards the blobs
    # pieces of a dataset with planes carry their scan's
    assert tuple(pieces.planes.shape) == (3, 4) and bool((pieces.planes == off.planes[0]).all()) and pieces.plane_found.tolist() == [True] * 3
    # the other way up: the plane turns with the blobs
    below = cloud.astype(np.float64) - 2 * ((cloud.astype(np.float64) @ normal + d)[:, None]) * normal
    flipped = _dataset([below.astype(np.float32)]).without_plane(0.01).planes.cpu().numpy().astype(np.float64)[0]
    assert _angle_deg(flipped[:3], -normal) < 1.0 and abs(flipped[3] + d) < 0.005


def test_source_rows_compose_with_outlier_removal():
    cloud, is_floor, _, _ = _scene()
    data = _dataset([cloud, cloud[::-1]], gt=np.zeros((2, 8, 3), np.float32), names=["a", "b"])
    clean = data.without_outliers(k=16, ratio=2.0)
    assert 0 < int(clean.kept.sum()) < 2 * len(cloud)
    off = clean.without_plane(0.01)
    rows = off.source_rows.cpu().numpy()
    assert np.array_equal(off.points.cpu().numpy(), data.points.cpu().numpy()[rows]) and (np.diff(rows) > 0).all()
    assert np.isin(rows, clean.source_rows.cpu().numpy()).all() and off.kept.tolist() == off.lengths.tolist()
    both = np.concatenate([is_floor, is_floor[::-1]])
    assert not both[rows].any() and off.lengths.sum() > 2 * 3 * BLOB * 0.75            # the floor went, the blobs stayed
    assert off.gt is data.gt and off.names == ["a", "b"] and clean.planes is None


def test_refine_false_keeps_the_laws_non_inliers():
    cloud, _, _, _ = _scene()
    other = plane_law.planted_scan(np.random.RandomState(3), 900)[0]
    data = _dataset([cloud, other])
    off = data.without_plane(0.01, trials=128, seed=5, refine=False)
    want = plane_law.plane_law(np.concatenate([cloud, other]), [0, len(cloud), len(cloud) + 900], 0.01, trials=128, seed=5,
                               min_share=0.2)
    assert want["found"].tolist() == [1, 1]
    assert np.array_equal(off.source_rows.cpu().numpy(), np.flatnonzero(want["inlier"] == 0))
    sample = want["sample_plane"].astype(np.float64)
    unit = sample / np.linalg.norm(sample[:, :3], axis=1, keepdims=True)
    got = off.planes.cpu().numpy().astype(np.float64)
    assert np.minimum(np.abs(got - unit).max(axis=1), np.abs(got + unit).max(axis=1)).max() < 1e-6     # the sample's, oriented


def test_a_scan_without_a_plane_stays_whole():
    cloud, _, _, _ = _scene()
    box = np.random.RandomState(8).uniform(-1, 1, (500, 3)).astype(np.float32)  # a band of 0.02 holds about 1 % of a box
    off = _dataset([box, cloud, box[:2]], names=["box", "scene", "pair"]).without_plane(0.01)
    assert off.plane_found.tolist() == [False, True, False] and off.lengths.tolist() == [500, 3 * BLOB, 2]
    planes = off.planes.cpu().numpy()
    assert np.isnan(planes[[0, 2]]).all() and np.isfinite(planes[1]).all()
    assert np.array_equal(off.scan(0).cpu().numpy(), box) and np.array_equal(off.scan(2).cpu().numpy(), box[:2])
    assert off.source_rows[:500].tolist() == list(range(500))


def test_a_scan_that_is_all_plane_is_an_error():
    cloud, is_floor, _, _ = _scene()
    data = _dataset([cloud, cloud[is_floor]], names=["scene", "floor-only"])
    with pytest.raises(ValueError, match=r"scan 1 \(floor-only\) would be left without points by plane removal"):
        data.without_plane(0.01)
    assert data.without_plane(0.01, min_inliers=FLOOR + 1).lengths.tolist() == [len(cloud), FLOOR]   # no plane that large: whole


def test_the_constructor_keyword_equals_the_method():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    cloud, _, _, _ = _scene()
    other = plane_law.planted_scan(np.random.RandomState(3), 900)[0]
    built = _dataset([cloud, other], plane=(0.01, 256))
    method = _dataset([cloud, other]).without_plane(0.01, trials=256)
    for name in ("points", "offsets", "source_rows", "planes", "plane_found"):
        a, b = getattr(built, name).cpu().numpy(), getattr(method, name).cpu().numpy()
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name
    assert built.kept.tolist() == method.kept.tolist()
    # before `outliers` and `clusters`: the clusters see the scene without its floor
    chained = _dataset([cloud], plane=(0.01, 256), outliers=(16, 2.0), clusters=(0.05, None))
    assert 0.7 * BLOB <= int(chained.lengths[0]) <= BLOB
    import inspect
    assert list(inspect.signature(DeviceScanDataset.__init__).parameters)[-1] == "plane"
    assert list(inspect.signature(DeviceScanDataset.from_npy_dir).parameters)[-1] == "plane"


def test_the_fitted_normal_stands_the_scan_upright():
    from hyperpocket_amd import ops
    cloud, _, normal, _ = _scene()
    first = _dataset([cloud]).without_plane(0.01)
    fitted = first.planes.cpu().numpy().astype(np.float64)[0, :3]
    upright = _dataset([cloud], transform=ops.rotation_to_axis(fitted)).without_plane(0.01)
    again = upright.planes.cpu().numpy().astype(np.float64)[0]
    assert np.abs(again[:3] - [0.0, 1.0, 0.0]).max() <= 1e-5
    assert upright.lengths.tolist() == [3 * BLOB] and float(upright.points[:, 1].min()) > -again[3]      # the blobs are above

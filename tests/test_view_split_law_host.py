"""CPU: the viewpoint batch maker's law (tests/view_split_law.py, include/hyperpocket_hip.h hp_make_view_batch) does what it is
for — the near side of a shell, the front one of two plates — and decides its corner cases as the text says; ops.view_frames and
ops.view_half_extent; and the entry point and the wrapper refuse bad arguments before any GPU call."""
import ctypes
import os

import numpy as np
import pytest
import torch

import view_split_law as law
from conftest import PKG_DIR

EYE = np.eye(3, dtype=np.float32)


def half_extent(radius, distance=3.0):
    from hyperpocket_amd import ops
    return ops.view_half_extent(radius, distance)


def split(cloud, frame=EYE, R=32, w=1, target=None, radius=0.5, dist=3.0):
    n = len(cloud)
    return law.view_split(cloud, frame, dist, law.scale_of(R, half_extent(radius, dist)), R, w, n // 2 if target is None else target)


# ------------------------------------------------------------------------------------------------
# what the law is for
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shell", [law.sphere_shell, law.lattice_shell], ids=["random", "lattice"])
def test_existing_is_the_sensors_half_of_a_shell(shell):
    """Radius 0.5, distance 3, the image fitted to the shell, target N/2: of `existing`, the share on the sensor's half
    (c_2 > 0) is >= 0.98 at (N, R, w) = (2048, 32, 1) over the 8 frames of view_frames(8, 3).  The strictly visible cap is
    (1 - r/d)/2 = 41.7 % of the rows; the ranking fills up with the least occluded rows at the limb.  Without the window the far
    side shows through the holes of the near one."""
    from hyperpocket_amd import ops
    cloud = shell(2048)
    frames = ops.view_frames(8, 3).numpy()
    shares = {1: [], 0: []}
    for f in frames:
        c2 = cloud.astype(np.float64) @ f[2].astype(np.float64)
        for w in shares:
            r = split(cloud, f, 32, w)
            assert int(r["side"].sum()) == 1024 and len(r["existing"]) == 1024 and len(r["missing"]) == 1024
            shares[w].append(float((c2[r["side"] == 1] > 0).mean()))
    print("shares, w = 1:", np.round(shares[1], 4), "w = 0:", np.round(shares[0], 4))
    assert min(shares[1]) >= 0.98
    assert max(shares[0]) < 0.85                     # why the window exists


PLATES_EXACT = [(2048, 16, 1), (2048, 32, 1), (2048, 64, 1), (2048, 8, 0), (2048, 8, 1), (2048, 8, 2),
                (128, 8, 0), (128, 8, 1), (128, 8, 2), (128, 16, 1)]


@pytest.mark.parametrize("n,R,w", PLATES_EXACT)
def test_existing_is_exactly_the_front_plate(n, R, w):
    """Two parallel plates at z = +-0.2, rows alternating, the identity frame, distance 3, the image fitted to a radius of 0.75."""
    cloud = law.two_plates(n)
    r = split(cloud, EYE, R, w, radius=0.75)
    front = (np.arange(n) % 2 == 0).astype(np.uint8)
    assert np.array_equal(r["side"], front)
    assert np.array_equal(r["existing"], cloud[0::2]) and np.array_equal(r["missing"], cloud[1::2])


@pytest.mark.parametrize("n,R", [(2048, 64), (128, 16)])
def test_a_pixel_finer_than_the_spacing_and_no_window_lets_the_back_plate_through(n, R):
    cloud = law.two_plates(n)
    r = split(cloud, EYE, R, 0, radius=0.75)
    front = np.arange(n) % 2 == 0
    assert int(r["side"].sum()) == n // 2
    share = float(r["side"][front].mean())
    print("front share", share)
    assert not np.array_equal(r["side"], front.astype(np.uint8)) and share < 0.8


# ------------------------------------------------------------------------------------------------
# the corner cases, decided as the text says
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [1, 7, 99])
def test_equal_occlusions_go_to_the_first_rows(target):
    """A plate perpendicular to the axis, w = 0: equal z, so o = +0 everywhere and the first `target` rows win."""
    r = np.random.default_rng(2)
    cloud = np.zeros((100, 3), np.float32)
    cloud[:, :2] = r.uniform(-0.4, 0.4, (100, 2))
    cloud[:, 2] = 0.125
    got = split(cloud, EYE, 16, 0, target)
    assert np.array_equal(got["occlusion"].view(np.uint32), np.zeros(100, np.uint32))       # +0, not -0
    assert np.array_equal(got["side"], (np.arange(100) < target).astype(np.uint8))
    assert int(got["side"].sum()) == target


def test_absent_rows_rank_last_and_fill_in_row_order():
    r = np.random.default_rng(3)
    cloud = r.uniform(-0.4, 0.4, (40, 3)).astype(np.float32)
    cloud[1, 0] = np.nan
    cloud[4, 2] = np.inf
    cloud[9, 1] = -np.inf
    cloud[12] = (0.0, 0.0, 3.0)                      # at the sensor: delta = 0
    cloud[20] = (0.1, 0.0, 5.0)                      # behind it: delta < 0
    absent = [1, 4, 9, 12, 20]
    got = split(cloud, EYE, 8, 1, 36)
    assert np.array_equal(np.nonzero(~got["present"])[0], absent)
    assert np.isposinf(got["occlusion"][absent]).all() and np.isfinite(np.delete(got["occlusion"], absent)).all()
    assert int(got["side"].sum()) == 36
    assert np.array_equal(np.nonzero(got["side"] == 0)[0], [4, 9, 12, 20])      # the 35 rows that project, then absent row 1
    # fewer rows project than `target`: all of them, then absent rows in row order
    cloud[5:] = np.nan
    cloud[2] = (0.0, 0.0, 4.0)
    got = split(cloud, EYE, 8, 1, 6)
    assert np.array_equal(np.nonzero(got["present"])[0], [0, 3])
    assert np.array_equal(np.nonzero(got["side"])[0], [0, 1, 2, 3, 4, 5])
    assert len(got["existing"]) == 6 and len(got["missing"]) == 34


def test_rows_outside_the_image_land_in_border_pixels():
    cloud = np.float32([[0.0, 0.0, 0.0], [9.0, 0.0, 0.0], [-9.0, 0.0, 0.0], [0.0, 9.0, 0.0], [0.0, -9.0, 0.0], [9.0, 9.0, 0.0],
                        [0.05, -0.05, 0.0]])
    present, pixel, _ = law.project(cloud, EYE, 3.0, law.scale_of(8, half_extent(0.5)), 8)
    assert present.all()
    assert pixel.tolist() == [4 * 8 + 4, 4 * 8 + 7, 4 * 8 + 0, 7 * 8 + 4, 0 * 8 + 4, 7 * 8 + 7, 3 * 8 + 4]
    got = split(cloud, EYE, 8, 0, 3)
    assert int(got["side"].sum()) == 3 and np.isfinite(got["occlusion"]).all()


def test_the_two_statements_of_the_law_agree():
    from hyperpocket_amd import ops
    r = np.random.default_rng(5)
    cloud = r.uniform(-0.5, 0.5, (257, 3)).astype(np.float32)
    cloud[3] = np.nan
    cloud[7, 1] = np.inf
    cloud[100] = cloud[101] = cloud[50]
    skew = np.float32([[1.0, 0.25, 0.0], [0.0, 0.5, 0.125], [0.25, 0.0, 2.0]])
    for f in list(ops.view_frames(2, 11).numpy()) + [skew]:
        for R, w, h in ((5, 0, 0.1), (5, 4, 0.3), (32, 1, 0.2)):
            a = law.view_split(cloud, f, 3.0, law.scale_of(R, h), R, w, 100)
            b = law.view_split_naive(cloud, f, 3.0, law.scale_of(R, h), R, w, 100)
            assert np.array_equal(a["side"], b["side"]) and np.array_equal(a["buffer"], b["buffer"])
            assert np.array_equal(a["occlusion"].view(np.uint32), b["occlusion"].view(np.uint32))
            assert int(a["side"].sum()) == 100


# ------------------------------------------------------------------------------------------------
# frames and the image's half-angle
# ------------------------------------------------------------------------------------------------
def test_view_frames_are_rotations_and_a_function_of_their_arguments():
    from hyperpocket_amd import ops
    f = ops.view_frames(64, 3)
    assert f.dtype == torch.float32 and tuple(f.shape) == (64, 3, 3) and not f.is_cuda
    m = f.numpy().astype(np.float64)
    assert np.abs(m @ m.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    assert np.abs(np.linalg.det(m) - 1.0).max() <= 1e-6
    assert torch.equal(f, ops.view_frames(64, 3)) and torch.equal(f[:8], ops.view_frames(8, 3))
    assert not torch.equal(f, ops.view_frames(64, 4))
    assert torch.equal(ops.view_frames(5, (3, 1)), ops.view_frames(5, (3, 1)))
    assert not torch.equal(ops.view_frames(5, (3, 1)), ops.view_frames(5, (3, 2)))
    # by hand: the unit quaternion (w, x, y, z) of the first draw
    q = np.random.default_rng(3).standard_normal((64, 4))[0]
    w, x, y, z = q / np.linalg.norm(q)
    want = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).astype(np.float32)
    assert np.array_equal(f[0].numpy(), want)
    assert tuple(ops.view_frames(0, 1).shape) == (0, 3, 3)
    # uniform over the rotations: the sensor's axis has no preferred direction
    axis = ops.view_frames(4096, 0).numpy()[:, 2].astype(np.float64)
    assert np.abs(axis.mean(0)).max() < 0.05


def test_view_half_extent():
    from hyperpocket_amd import ops
    assert ops.view_half_extent(0.5, 3.0) == 0.5 / (9.0 - 0.25) ** 0.5
    assert ops.view_half_extent(3.0, 5.0) == 0.75
    for bad in ((1.0, 1.0), (2.0, 1.0), (0.0, 1.0), (-1.0, 3.0), (1.0, float("inf")), (float("nan"), 3.0)):
        with pytest.raises(ValueError):
            ops.view_half_extent(*bad)


# ------------------------------------------------------------------------------------------------
# the library, without a GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build(verbose=False))


def test_entry_point_rejects_bad_arguments_before_any_gpu_call(lib):
    p = ctypes.c_void_p(64)            # never dereferenced: every call below ends at its argument check
    null = ctypes.c_void_p(0)
    inf, nan = float("inf"), float("nan")

    def make(M=4, N=64, target=32, clouds=p, B=2, ids=p, frames=p, degrees=null, rot=null, dist=3.0, scale=90.0, R=32, w=1,
             existing=p, missing=p, gt=p, side=p, occlusion=p):
        return lib.hp_make_view_batch(M, N, target, clouds, B, ids, frames, degrees, rot, ctypes.c_double(dist),
                                      ctypes.c_double(scale), R, w, existing, missing, gt, side, occlusion, null)

    for bad in (dict(M=0), dict(B=0), dict(B=65536), dict(N=1, target=1), dict(N=8193, target=4096), dict(target=0),
                dict(target=64), dict(target=-1), dict(R=3), dict(R=129), dict(w=-1), dict(w=5), dict(dist=0.0), dict(dist=-1.0),
                dict(dist=inf), dict(dist=nan), dict(scale=0.0), dict(scale=inf), dict(scale=nan), dict(clouds=null),
                dict(ids=null), dict(frames=null), dict(existing=null), dict(missing=null), dict(gt=null),
                dict(degrees=p, rot=null)):
        assert make(**bad) == -1, bad

    threads, lds = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.hp_make_view_batch_plan(8192, 128, ctypes.byref(threads), ctypes.byref(lds)) == 0
    assert threads.value % 64 == 0 and lds.value == 4 * 128 * 128 + 6 * 8192
    assert lds.value + 16 * 1024 <= 160 * 1024                   # the largest shape fits the 160 KiB of a compute unit
    assert lib.hp_make_view_batch_plan(65, 4, ctypes.byref(threads), ctypes.byref(lds)) == 0 and lds.value == 64 + 6 * 128
    for N, R in ((1, 32), (8193, 32), (64, 3), (64, 129)):
        assert lib.hp_make_view_batch_plan(N, R, ctypes.byref(threads), ctypes.byref(lds)) == -1


def test_ops_refuse_what_they_cannot_do():
    from hyperpocket_amd import HipExtensionError, ops
    assert (ops.VIEW_SPLIT_MAX_POINTS, ops.VIEW_SPLIT_MIN_RESOLUTION, ops.VIEW_SPLIT_MAX_RESOLUTION,
            ops.VIEW_SPLIT_MAX_WINDOW) == (8192, 4, 128, 4)
    clouds, ids, frames = torch.rand(4, 64, 3), torch.zeros(2, dtype=torch.int32), ops.view_frames(2, 0)
    with pytest.raises(HipExtensionError):
        ops.make_view_batch(clouds, ids, frames, target=32)                 # CPU tensors: there is no CPU path
    for kw in (dict(resolution=3), dict(resolution=129), dict(resolution=32.5), dict(window=-1), dict(window=5),
               dict(distance=0.0), dict(distance=float("inf")), dict(half_extent=0.0), dict(half_extent=-1.0),
               dict(half_extent=float("nan")), dict(distance=0.4)):         # 0.4: inside the default sphere of radius 0.5
        with pytest.raises(ValueError):
            ops.make_view_batch(clouds, ids, frames, target=32, **kw)
    for n, target in ((1, 1), (8193, 10), (64, 0), (64, 64)):
        with pytest.raises(ValueError):
            ops.make_view_batch_buffers(2, n, target, "cpu")
    bufs = ops.make_view_batch_buffers(3, 64, 20, "cpu", occlusion=False)
    assert {k: tuple(v.shape) for k, v in bufs.items()} == {"existing": (3, 20, 3), "missing": (3, 44, 3), "gt": (3, 64, 3),
                                                           "side": (3, 64)}
    assert bufs["side"].dtype == torch.uint8


def test_the_view_batcher_needs_a_device_dataset():
    from hyperpocket_amd.datasets.device_dataset import DeviceBatcher, DeviceViewBatcher, _EpochBatcher
    assert issubclass(DeviceViewBatcher, _EpochBatcher) and issubclass(DeviceBatcher, _EpochBatcher)
    for name in ("__iter__", "__len__", "set_epoch"):                       # one epoch plan, one prefetch machinery
        assert name not in vars(DeviceViewBatcher) and name not in vars(DeviceBatcher)
    with pytest.raises(TypeError):
        DeviceViewBatcher(np.zeros((4, 64, 3), np.float32), 2, target=32)

"""GPU suite for the global registration chain (ops.scan_align_global, DeviceScanDataset.aligned_globally and
merged_views_globally): the start is the laws' bit for bit, the refined pose lands where the laws' chain lands, and on the
same fixture the local aligners — from the identity and with the yaw search — end more than 90 degrees off."""
import functools

import numpy as np
import pytest
import torch

import feature_law
import pose_trials_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
MAX_DIST = 0.05
# Measured with the laws on the CPU (pose_trials_law.global_start_law, then refine_law), bumpy_sheet(1500, seed 0): the winning
# trial is 2.71 degrees and 0.0434 off, the refined pose 0.0198 degrees and 0.00027; sheet_views(1500, seed 0): 1.77 degrees and
# 0.0772, refined 0.134 degrees and 0.00051.  The refined error is asserted at 4 x the law's figure, the margin of DESIGN.md
# 3m and 3o: the figure is one seed's.
SHEET_REFINED = (0.0198, 0.00027)
VIEWS_REFINED = (0.134, 0.00051)


@functools.lru_cache(maxsize=None)
def _sheet():
    source, target, R, t = feature_law.bumpy_sheet(1500, seed=0)
    vs, vt = feature_law.sheet_viewpoints(R, t)
    off = np.array([0, 1500], dtype=np.int64)
    want = law.global_start_law(source, off, target, off, MAX_DIST, viewpoints=vs, tviewpoints=vt)
    return source, target, R, t, vs, vt, want


@functools.lru_cache(maxsize=None)
def _views():
    v0, v1, R, t = feature_law.sheet_views(1500, seed=0)
    want = law.global_start_law(v1, np.array([0, len(v1)]), v0, np.array([0, len(v0)]), MAX_DIST, viewpoints=(0, 0, 0),
                                tviewpoints=(0, 0, 0))
    return v0, v1, R, t, want


def _dev(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype, device=CUDA)


def _start(source, target, vs, vt):
    from hyperpocket_amd import ops
    off = lambda c: _dev([0, len(c)], torch.int64)
    return ops.scan_align_global(_dev(source), off(source), _dev(target), off(target), MAX_DIST, viewpoints=_dev(vs, torch.float32),
                                 tviewpoints=_dev(vt, torch.float32))


def _same_start(got, want):
    poses, found, inliers, valid = got
    assert poses.shape == (1, 3, 4) and poses.dtype == np.float64 and found.dtype == bool
    assert found.tolist() == [bool(want["found"][0])] and inliers.tolist() == want["inliers"].tolist()
    assert valid.tolist() == want["valid"].tolist()
    assert np.array_equal(poses[0], want["transform"][0].astype(np.float64).reshape(3, 4))      # bit for bit: fp32 widens exactly


def test_the_start_is_the_laws_bit_for_bit():
    source, target, R, t, vs, vt, want = _sheet()
    assert want["found"][0] == 1 and want["valid"][0] > 100 and want["inliers"][0] >= 20
    angle, move = law.pose_error(want["transform"][0], R, t)
    print("the law's start:", angle, move, {k: v.tolist() for k, v in want.items() if k not in ("transform", "match")})
    assert angle < 15.0                                            # within the reach of the point-to-plane refinement
    _same_start(_start(source, target, vs, vt), want)


def test_aligned_globally_lands_where_the_laws_chain_lands():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    source, target, R, t, vs, vt, want = _sheet()
    data = DeviceScanDataset([torch.from_numpy(source)], device=CUDA)
    new = data.aligned_globally(torch.from_numpy(target), MAX_DIST, viewpoint=tuple(vs.tolist()), target_viewpoint=tuple(vt.tolist()))
    angle, move = law.pose_error(new.poses[0], R, t)
    print("refined on the device:", angle, move)
    assert new.pose_found.tolist() == [True] and new.pose_ok.tolist() == [True]
    assert angle <= 4 * SHEET_REFINED[0] and move <= 4 * SHEET_REFINED[1]
    moved = new.points.cpu().numpy().astype(np.float64)
    assert np.abs(moved - (source.astype(np.float64) @ R.T + t)).max() < 0.01      # the rows went with the pose


def test_the_local_aligners_do_not_reach_it():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    source, target, R, t, _, _, _ = _sheet()
    data = DeviceScanDataset([torch.from_numpy(source)], device=CUDA)
    for yaw in (0, 24):                                            # the laws on the CPU: 139.0 and 137.5 degrees off
        new = data.aligned_to_surface(torch.from_numpy(target), MAX_DIST, yaw=yaw)
        angle, _ = law.pose_error(new.poses[0], R, t)
        print("aligned_to_surface, yaw", yaw, "ends", angle, "degrees off")
        assert angle > 90.0


def test_merged_views_globally():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    v0, v1, R, t, want = _views()
    assert want["found"][0] == 1
    zero = np.zeros(3, dtype=np.float32)
    _same_start(_start(v1, v0, zero, zero), want)
    data = DeviceScanDataset([torch.from_numpy(v0), torch.from_numpy(v1)], device=CUDA)
    new = data.merged_views_globally([[0, 1]], MAX_DIST)
    assert len(new) == 1 and new.view_rows == [[len(v0), len(v1)]]
    assert new.pose_found[0].tolist() == [True, True] and new.pose_ok[0].tolist() == [True, True]
    assert np.array_equal(new.poses[0][0], np.eye(3, 4))
    angle, move = law.pose_error(new.poses[0][1], R, t)
    print("merged views, refined on the device:", angle, move)
    assert angle <= 4 * VIEWS_REFINED[0] and move <= 4 * VIEWS_REFINED[1]
    merged = new.points.cpu().numpy()
    assert np.array_equal(merged[:len(v0)], v0)                    # the first view is the frame: bit for bit
    assert np.abs(merged[len(v0):].astype(np.float64) - (v1.astype(np.float64) @ R.T + t)).max() < 0.02

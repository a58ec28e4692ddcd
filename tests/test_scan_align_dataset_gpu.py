"""GPU suite for DeviceScanDataset.aligned_to and merged_views (ops.scan_align, csrc/align.hip): two overlapping views of an
object merged into one scan, scans posed onto one shared target and onto a target each, scans that do not align, and the
caps."""
import numpy as np
import pytest
import torch

import align_law
import scan_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32 = np.float32
INF = float("inf")
ROT_TOL, MOVE_TOL = 4 * 4.27e-7, 4 * 2.79e-7           # as tests/test_align_gpu.py: 4 x the solve's error at seed 0
MERGED_SCALE_GAP = 0.00732                             # measured with the law on the CPU, see test_two_views_merge_into_one_scan


def _dataset(scans, **kw):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    return DeviceScanDataset([torch.from_numpy(np.array(s)) for s in scans], device=CUDA, **kw)


def _error(T, R, t):
    return align_law.motion(np.concatenate([T[:, :3] @ R.T, np.zeros((3, 1))], axis=1))[0], float(np.linalg.norm(T[:, 3] - t))


def test_two_views_merge_into_one_scan():
    """align_law.two_views at seed 2: an object of 2000 rows, view 0 its x < 0.2 (1463 rows), view 1 its x > -0.2 (1676 rows)
    turned 25 degrees about y and shifted.  Measured with the law on the CPU (max_dist +inf, 30 iterations): plain ICP on two
    40 %-overlap views of a uniformly filled block stalls 5.7 degrees and 0.125 from the planted motion, and the merged scan's
    box scale lies 0.00732 from the whole object's 0.99852; the test asserts 4 x that figure, and the poses bit for bit."""
    obj, view0, view1, R, t = align_law.two_views(2)
    data = _dataset([view0, view1, obj], names=["front", "back", "whole"])
    merged = data.merged_views([[0, 1], [2]], INF)
    n0, n1 = len(view0), len(view1)
    assert len(merged) == 2 and merged.lengths.tolist() == [n0 + n1, len(obj)] and merged.view_rows == [[n0, n1], [len(obj)]]
    assert merged.source_scan.tolist() == [0, 2] and merged.names == ["front", "whole"]
    assert merged.offsets.tolist() == [0, n0 + n1, n0 + n1 + len(obj)] and merged.source_rows is None and merged.kept is None
    points = merged.points.cpu().numpy()
    assert np.array_equal(points[:n0], view0) and np.array_equal(points[n0 + n1:], obj)           # a group's frame is its first view
    want = align_law.align(view1, [0, n1], view0, [0, n0], INF)
    assert np.array_equal(merged.poses[0][1], want[0][0]) and np.array_equal(merged.poses[0][0], np.eye(3, 4))
    assert merged.pose_ok[0].tolist() == [True, True] and merged.pose_ok[1].tolist() == [True]
    assert merged.pose_rms[0][1] == want[2][0]
    scale, whole = float(merged.boxes()[1][0]), float(scan_law.boxes_fp32(obj)[1])
    angle, move = _error(merged.poses[0][1], R, t)
    print(f"merged scale {scale:.5f} against {whole:.5f}: gap {abs(scale - whole):.5f}; pose error {np.degrees(angle):.2f} degrees, {move:.3f}")
    assert abs(scale - whole) <= 4 * MERGED_SCALE_GAP
    assert float(merged.boxes()[1][1]) == whole and data.points.data_ptr() != merged.points.data_ptr()
    # the chain's last stage feeds the batcher
    from hyperpocket_amd.datasets.scan_dataset import ScanBatcher
    existing, ids, _ = next(iter(ScanBatcher(merged, 2, target=512, normalize=True)))
    assert tuple(existing.shape) == (2, 512, 3) and bool(torch.isfinite(existing).all())


def test_aligned_to_one_target_and_to_a_target_each():
    source0, target0, R0, t0, rows0 = align_law.planted_pair(0)
    source1, target1, R1, t1, _ = align_law.planted_pair(1)
    # one cloud for all scans: two parts of the same target, moved differently
    R2, t2 = align_law.rotation((1, 0.2, 0.1), np.radians(-15.0)), np.array([0.02, -0.05, 0.04])
    source2 = ((target0[100:500].astype(np.float64) - t2) @ R2).astype(f32)
    data = _dataset([source0, source2], names=["a", "b"])
    posed = data.aligned_to(target0, INF)
    want = align_law.align(np.concatenate([source0, source2]), [0, 400, 800], np.concatenate([target0, target0]), [0, 600, 1200], INF)
    assert np.array_equal(posed.poses, want[0]) and posed.pose_ok.tolist() == [True, True] and np.array_equal(posed.pose_rms, want[2])
    for s, (R, t) in enumerate(((R0, t0), (R2, t2))):
        angle, move = _error(posed.poses[s], R, t)
        assert angle <= ROT_TOL and move <= MOVE_TOL, (s, angle, move)
    gap = np.abs(posed.points.cpu().numpy() - np.concatenate([target0[rows0], target0[100:500]]))      # every row on its own target row
    assert gap.max() < 1e-5 and posed.lengths.tolist() == [400, 400] and posed.names == ["a", "b"]
    assert posed.source_rows is None and np.array_equal(data.points.cpu().numpy(), np.concatenate([source0, source2]))
    # a target each: a list, a ragged pair, another dataset
    data = _dataset([source0, source1])
    want = align_law.align(np.concatenate([source0, source1]), [0, 400, 800], np.concatenate([target0, target1]), [0, 600, 1200], INF)
    ragged = (torch.from_numpy(np.concatenate([target0, target1])), torch.tensor([0, 600, 1200]))
    for targets in ([target0, target1], ragged, _dataset([target0, target1])):
        posed = data.aligned_to(targets, INF)
        assert np.array_equal(posed.poses, want[0]) and posed.pose_ok.all()
        for s, (R, t) in enumerate(((R0, t0), (R1, t1))):
            angle, move = _error(posed.poses[s], R, t)
            assert angle <= ROT_TOL and move <= MOVE_TOL, (s, angle, move)
    filtered = _dataset([source0, source1], outliers=(8, 50.0))     # source_rows and kept pass through unchanged
    posed = filtered.aligned_to([target0, target1], INF)
    assert torch.equal(posed.source_rows, filtered.source_rows) and torch.equal(posed.kept, filtered.kept)
    yawed = data.aligned_to([target0, target1], INF, yaw=6, axis=(0.3, 0.9, -0.4))
    assert yawed.pose_ok.all() and _error(yawed.poses[0], R0, t0)[0] <= ROT_TOL


def test_unaligned_scans_stay_and_the_caps_name_the_scan():
    from hyperpocket_amd import ops
    source0, target0, R0, t0, _ = align_law.planted_pair(0)
    far = (source0 + f32(50)).astype(f32)                           # no target row within the gate
    two = np.array([[0, 0, 0], [0.5, 0.5, 0.5]], f32)               # two correspondences at the most
    data = _dataset([source0, far, two])
    posed = data.aligned_to(target0, 0.5)
    assert posed.pose_ok.tolist() == [True, False, False]
    assert np.array_equal(posed.poses[1], np.eye(3, 4)) and np.array_equal(posed.poses[2], np.eye(3, 4))
    points = posed.points.cpu().numpy()
    assert np.array_equal(points[400:800], far) and np.array_equal(points[800:], two) and not np.array_equal(points[:400], source0)
    merged = data.merged_views([[0, 1]], 0.5)
    assert merged.pose_ok[0].tolist() == [True, False] and np.array_equal(merged.points.cpu().numpy()[400:], far)
    cap = ops.ALIGN_MAX_POINTS
    big = np.random.RandomState(0).uniform(-1, 1, (cap + 1, 3)).astype(f32)
    data = _dataset([source0, big], names=["small", "big"])
    with pytest.raises(ValueError, match=r"scan 1 \(big\).*thin it first"):
        data.aligned_to(target0, 0.5)
    with pytest.raises(ValueError, match=r"target 0.*thin it first"):
        _dataset([source0]).aligned_to(big, 0.5)
    with pytest.raises(ValueError, match=r"scan 1 \(big\) of group 0.*thin it first"):
        data.merged_views([[0, 1]], 0.5)
    with pytest.raises(ValueError, match=r"group 1 would merge.*thin first"):
        data.merged_views([[0], [1] * 64], 0.5)

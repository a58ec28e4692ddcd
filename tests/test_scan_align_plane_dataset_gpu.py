"""GPU suite for DeviceScanDataset.aligned_to_surface and merged_views_surface (ops.scan_align_plane, csrc/align_plane.hip):
captures of a wavy sheet posed onto independent samplings of it within the noise floor, where thirty point-to-point steps stay
degrees away; a scan against one plane keeps its coarse pose; two views merged; the caps; and aligned_to / merged_views
untouched by the helpers they now share."""
import numpy as np
import pytest
import torch

import align_law
import align_plane_law as law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
f32 = np.float32
GATE = 0.3
# the pose error of three point-to-plane steps on wavy_pair, measured with the law on the CPU (test_align_plane_law_host.py asserts 4 x)
POSE_ROT, POSE_MOVE = 4 * 1.27e-3, 4 * 3.73e-4
WAVY = ((0, 8.0), (1, 8.0), (2, 15.0))                 # (seed, planted turn in degrees)


def _dataset(scans, **kw):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    return DeviceScanDataset([torch.from_numpy(np.array(s)) for s in scans], device=CUDA, **kw)


def _offsets(clouds):
    return np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)


def _two_stage(sources, targets, normals, coarse=5, iters=3):
    """The laws' two stages over S pairs: (poses, coarse ok, fine ok, rms)."""
    sets = (np.concatenate(sources), _offsets(sources), np.concatenate(targets), _offsets(targets))
    start, start_ok, _, _, _ = align_law.align(*sets, GATE, iters=coarse)
    start[~start_ok] = np.eye(3, 4)
    poses, ok, rms, _ = law.align_plane(*sets, np.concatenate(normals), GATE, iters=iters, init=start)
    poses[~ok] = start[~ok]
    return poses, start_ok, ok, rms


def _posed_by(got, rows, pose):
    """got is p' = R p + t of rows under the pose at its fp32 rounding: within a few fp32 roundings of the fp64 value (the
    coordinates stay below 2, the order of the three products is the device's)."""
    m = pose.astype(f32).astype(np.float64)
    return np.abs(got - (rows.astype(np.float64) @ m[:, :3].T + m[:, 3])).max() < 1e-6


def test_three_surface_steps_reach_what_thirty_point_to_point_steps_do_not():
    """Measured with the laws on the CPU, (rotation error in rad, translation error) against the planted motion:
        seed 0,  8 degrees: 5 coarse + 3 surface steps 9.6e-4 / 4.0e-4;  30 point-to-point steps 7.4e-2 / 3.3e-2
        seed 1,  8 degrees:                            1.4e-4 / 3.1e-4;                          5.0e-2 / 3.6e-2
        seed 2, 15 degrees:                            2.2e-4 / 2.7e-4;                          1.3e-1 / 4.6e-2"""
    pairs = [law.wavy_pair(seed=seed, degrees=degrees) for seed, degrees in WAVY]
    sources, targets = [p[0] for p in pairs], [np.array(p[1]) for p in pairs]      # copies: the fixtures are read-only
    data = _dataset(sources, names=["a", "b", "c"])
    posed = data.aligned_to_surface(targets, GATE, iters=3)
    want, _, fine_ok, rms = _two_stage(sources, targets, [law.normals_of(seed=seed) for seed, _ in WAVY])
    assert np.array_equal(posed.poses, want) and fine_ok.all() and posed.pose_ok.tolist() == [True] * 3
    assert np.array_equal(posed.pose_rms, rms) and posed.pose_ok.dtype == bool and posed.poses.dtype == np.float64
    plain = data.aligned_to(targets, GATE, iters=30)
    for s, (_, _, R, t) in enumerate(pairs):
        angle, move = law.pose_error(posed.poses[s], R, t)
        slow = law.pose_error(plain.poses[s], R, t)
        print(f"scan {s}: surface {angle:.3e} rad / {move:.3e}, rms {posed.pose_rms[s]:.3e}; point-to-point, 30 steps: {slow[0]:.3e} rad / {slow[1]:.3e}")
        assert angle <= POSE_ROT and move <= POSE_MOVE, (s, angle, move)
        assert slow[0] > POSE_ROT and slow[1] > POSE_MOVE and plain.pose_ok[s], (s, slow)
        assert 0.5 * 0.002 < posed.pose_rms[s] < 2 * 0.002          # the distance to the surface that is left is the noise
    points = posed.points.cpu().numpy()
    assert _posed_by(points[:1500], sources[0], want[0]) and posed.lengths.tolist() == [1500] * 3
    assert posed.names == ["a", "b", "c"] and np.array_equal(data.points.cpu().numpy(), np.concatenate(sources))
    # the forms of the targets, and a start without the coarse stage: three more steps from the identity are the law's chain itself
    ragged = (torch.from_numpy(np.concatenate(targets)), torch.from_numpy(_offsets(targets)))
    for form in (ragged, _dataset(targets)):
        assert np.array_equal(data.aligned_to_surface(form, GATE, iters=3).poses, want)
    bare = _dataset(sources[:1]).aligned_to_surface(targets[0], GATE, iters=3, coarse=0)
    direct = law.align_plane(sources[0], [0, 1500], targets[0], [0, 1500], law.normals_of(seed=0), GATE, iters=3)
    assert np.array_equal(bare.poses, direct[0]) and bare.pose_ok.tolist() == [True]


def test_a_plane_keeps_its_coarse_pose():
    slab_source, slab_target, slab_normals = law.slab_pair()
    wavy_source, wavy_target, _, _ = law.wavy_pair()
    far = (wavy_source + f32(50)).astype(f32)                       # no target row within the gate: neither stage is ok
    sources, targets = [slab_source, wavy_source, far], [np.array(slab_target), np.array(wavy_target), np.array(wavy_target)]
    normals = [slab_normals, law.normals_of(), law.normals_of()]
    data = _dataset(sources)
    posed = data.aligned_to_surface(targets, GATE, iters=3)
    want, start_ok, fine_ok, rms = _two_stage(sources, targets, normals)
    assert start_ok.tolist() == [True, True, False] and fine_ok.tolist() == [False, True, False]
    assert posed.pose_ok.tolist() == [True, True, False] and np.array_equal(posed.poses, want)
    coarse = align_law.align(slab_source, [0, 1024], slab_target, [0, 1024], GATE, iters=5)[0][0]
    assert np.array_equal(posed.poses[0], coarse) and not np.array_equal(coarse, np.eye(3, 4))     # the slide was refused, the coarse pose stays
    assert np.array_equal(posed.poses[2], np.eye(3, 4)) and np.isinf(posed.pose_rms[2]) and np.isfinite(posed.pose_rms[:2]).all()
    points = posed.points.cpu().numpy()
    assert _posed_by(points[:1024], slab_source, coarse) and np.array_equal(points[2524:], far)
    skipped = data.aligned_to_surface(targets, GATE, iters=3, coarse=0)    # without the coarse stage the plane has nothing to keep
    assert skipped.pose_ok.tolist() == [False, True, False] and np.array_equal(skipped.points.cpu().numpy()[:1024], slab_source)


def test_two_views_merge_along_the_surface():
    from hyperpocket_amd import ops
    source, target, R, t = law.wavy_pair()
    extra = law.wavy_pair(seed=1)[1]
    data = _dataset([target, source, extra], names=["front", "back", "other"])
    merged = data.merged_views_surface([[0, 1], [2]], GATE, iters=3)
    assert len(merged) == 2 and merged.lengths.tolist() == [3000, 1500] and merged.view_rows == [[1500, 1500], [1500]]
    assert merged.source_scan.tolist() == [0, 2] and merged.names == ["front", "other"]
    assert merged.offsets.tolist() == [0, 3000, 4500] and merged.source_rows is None and merged.kept is None
    want, _, fine_ok, rms = _two_stage([source], [target], [law.normals_of()])
    assert np.array_equal(merged.poses[0][0], np.eye(3, 4)) and np.array_equal(merged.poses[0][1], want[0]) and fine_ok[0]
    assert merged.pose_ok[0].tolist() == [True, True] and merged.pose_ok[1].tolist() == [True]
    assert merged.pose_rms[0][0] == 0 and merged.pose_rms[0][1] == rms[0] and merged.pose_rms[1].tolist() == [0.0]
    points = merged.points.cpu().numpy()
    assert np.array_equal(points[:1500], target) and np.array_equal(points[3000:], extra)         # a group's frame is its first view
    assert _posed_by(points[1500:3000], source, want[0])
    angle, move = law.pose_error(merged.poses[0][1], R, t)
    assert angle <= POSE_ROT and move <= POSE_MOVE, (angle, move)
    # the caps name the scan, as for the point-to-point twins
    cap = ops.ALIGN_MAX_POINTS
    big = np.random.RandomState(0).uniform(-1, 1, (cap + 1, 3)).astype(f32)
    data = _dataset([source, big], names=["small", "big"])
    with pytest.raises(ValueError, match=r"scan 1 \(big\).*thin it first"):
        data.aligned_to_surface(target, GATE)
    with pytest.raises(ValueError, match=r"target 0.*thin it first"):
        _dataset([source]).aligned_to_surface(big, GATE)
    with pytest.raises(ValueError, match=r"scan 1 \(big\) of group 0.*thin it first"):
        data.merged_views_surface([[0, 1]], GATE)
    with pytest.raises(ValueError, match=r"group 1 would merge.*thin first"):
        data.merged_views_surface([[0], [1] * 64], GATE)
    with pytest.raises(ValueError):
        data.aligned_to_surface([target] * 3, GATE)


def test_the_point_to_point_methods_are_untouched():
    obj, view0, view1, _, _ = align_law.two_views(2)
    data = _dataset([view0, view1, obj])
    INF = float("inf")

    def both():
        posed, merged = data.aligned_to(view0, INF, iters=10), data.merged_views([[0, 1], [2]], INF, iters=10)
        return [posed.points.cpu().numpy(), posed.poses, posed.pose_ok, posed.pose_rms, merged.points.cpu().numpy(),
                np.concatenate(merged.poses), np.concatenate(merged.pose_ok), np.concatenate(merged.pose_rms)]

    before = both()
    data.aligned_to_surface(view0, INF, iters=2)
    data.merged_views_surface([[0, 1], [2]], INF, iters=2)
    after = both()
    for b, a in zip(before, after):
        assert b.dtype == a.dtype and np.array_equal(b.view(np.uint8), a.view(np.uint8))
    sets = (np.concatenate([view0, view1, obj]), _offsets([view0, view1, obj]), np.concatenate([view0] * 3), _offsets([view0] * 3))
    want = align_law.align(*sets, INF, iters=10)                    # and they are what the law says they were
    assert np.array_equal(before[1], np.where(want[1][:, None, None], want[0], np.eye(3, 4))) and np.array_equal(before[2], want[1])
    assert _posed_by(before[0][:len(view0)], view0, before[1][0])

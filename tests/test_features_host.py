"""CPU suite for the C entry points of csrc/features.hip and csrc/pose_trials.hip and their Python side (needs the built library,
not a GPU): the symbols are exported, argument checks come before any HIP call, the plan queries answer, the wrappers have the
signatures of the issue and no CPU path, and the pinned dataset signatures are what they were."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest

import feature_law
import pose_trials_law
from conftest import PKG_DIR

# device pointers are never followed by an argument check: any non-null, aligned value stands for one
P = ctypes.c_void_p(64)
NULL = ctypes.c_void_p(0)
LL = ctypes.c_longlong


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(verbose=False))
    lib.hp_scan_features_workspace_bytes.restype = ctypes.c_long
    lib.hp_scan_pose_trials_workspace_bytes.restype = ctypes.c_long
    return lib


def test_symbols_are_exported(lib):
    for name in ("hp_scan_features", "hp_scan_features_plan", "hp_scan_features_workspace_bytes", "hp_scan_feature_match",
                 "hp_scan_feature_match_plan", "hp_scan_pose_trials", "hp_scan_pose_trials_plan",
                 "hp_scan_pose_trials_workspace_bytes"):
        assert hasattr(lib, name), name


def _features(lib, S=1, T=8, points=P, offsets=P, normals=P, k=8, index=P, features=P, count=P, ws=P):
    return lib.hp_scan_features(S, LL(T), points, offsets, normals, k, index, features, count, ws, NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(S=-1), dict(T=-1), dict(k=0), dict(k=33), dict(k=-4), dict(points=NULL),
                                 dict(offsets=NULL), dict(normals=NULL), dict(index=NULL), dict(features=NULL), dict(count=NULL),
                                 dict(ws=NULL), dict(features=ctypes.c_void_p(66)), dict(ws=ctypes.c_void_p(65))])
def test_features_rejects_before_any_hip_call(lib, bad):
    assert _features(lib, **bad) == -1


def _match(lib, S=1, T=8, features=P, offsets=P, U=8, tfeatures=P, toffsets=P, counts=P, tcounts=P, match=P, dist=P):
    return lib.hp_scan_feature_match(S, LL(T), features, offsets, LL(U), tfeatures, toffsets, counts, tcounts, match, dist, NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(T=-1), dict(U=-1), dict(features=NULL), dict(offsets=NULL), dict(tfeatures=NULL),
                                 dict(toffsets=NULL), dict(counts=NULL), dict(tcounts=NULL), dict(match=NULL), dict(dist=NULL),
                                 dict(features=ctypes.c_void_p(65)), dict(tfeatures=ctypes.c_void_p(70))])
def test_match_rejects_before_any_hip_call(lib, bad):
    assert _match(lib, **bad) == -1


def _trials(lib, S=1, T=8, points=P, offsets=P, U=8, tpoints=P, toffsets=P, match=P, streams=NULL, seed=0, trials=64, keep=16,
            rho2=0.81, inlier_dist=0.1, min_inliers=6, trial=P, inliers=P, found=P, transform=P, valid=P, kept=P, ws=P):
    return lib.hp_scan_pose_trials(S, LL(T), points, offsets, LL(U), tpoints, toffsets, match, streams, ctypes.c_ulonglong(seed),
                                   trials, keep, ctypes.c_float(rho2), ctypes.c_float(inlier_dist), min_inliers, trial, inliers,
                                   found, transform, valid, kept, ws, NULL)


@pytest.mark.parametrize("bad", [dict(S=0), dict(T=-1), dict(U=-1), dict(points=NULL), dict(offsets=NULL), dict(tpoints=NULL),
                                 dict(toffsets=NULL), dict(match=NULL), dict(trials=0), dict(trials=65537), dict(keep=0),
                                 dict(keep=4097), dict(rho2=-0.1), dict(rho2=1.5), dict(rho2=float("nan")), dict(inlier_dist=-1.0),
                                 dict(inlier_dist=float("nan")), dict(min_inliers=-1), dict(trial=NULL), dict(inliers=NULL),
                                 dict(found=NULL), dict(transform=NULL), dict(valid=NULL), dict(kept=NULL), dict(ws=NULL),
                                 dict(ws=ctypes.c_void_p(72))])
def test_pose_trials_rejects_before_any_hip_call(lib, bad):
    assert _trials(lib, **bad) == -1


def test_plans_name_the_geometry(lib):
    v = [ctypes.c_int(0) for _ in range(3)]
    refs = [ctypes.byref(x) for x in v]
    for k, inst in ((1, 8), (4, 8), (7, 8), (8, 8), (9, 16), (16, 16), (17, 32), (31, 32), (32, 32)):
        assert lib.hp_scan_features_plan(k, *refs) == 0
        assert [x.value for x in v] == [inst, 256, feature_law.WIDTH]
    for k in (0, -1, 33):
        assert lib.hp_scan_features_plan(k, *refs) == -1
    assert lib.hp_scan_features_plan(8, None, refs[1], refs[2]) == -1
    assert lib.hp_scan_features_workspace_bytes(LL(1000)) == 36000 and lib.hp_scan_features_workspace_bytes(LL(0)) == 0
    assert lib.hp_scan_features_workspace_bytes(LL(-1)) == -1
    assert lib.hp_scan_feature_match_plan(*refs) == 0
    threads, rows, tile = (x.value for x in v)
    assert threads % 64 == 0 and 64 <= threads <= 1024 and 1 <= rows <= 8 and 64 <= tile and 48 * tile <= 64 * 1024
    assert lib.hp_scan_feature_match_plan(refs[0], None, refs[2]) == -1
    assert lib.hp_scan_pose_trials_plan(32768, 1024, *refs) == 0
    threads, rows, tile = (x.value for x in v)
    assert threads % 64 == 0 and 1 <= rows <= 8 and tile == threads and 48 * tile <= 64 * 1024
    for trials, keep in ((0, 1), (65537, 1), (1, 0), (1, 4097)):
        assert lib.hp_scan_pose_trials_plan(trials, keep, *refs) == -1
    assert lib.hp_scan_pose_trials_workspace_bytes(3, 1024) == 3 * 1024 * 56
    for S, keep in ((0, 1), (1, 0), (1, 4097)):
        assert lib.hp_scan_pose_trials_workspace_bytes(S, keep) == -1


def test_python_constants_and_plans_agree_with_the_laws():
    from hyperpocket_amd import HipExtensionError, ops
    assert ops.FEATURE_WIDTH == feature_law.WIDTH and ops.POSE_MAX_TRIALS == pose_trials_law.MAX_TRIALS == 65536
    assert ops.POSE_MAX_KEEP == pose_trials_law.MAX_KEEP and ops.ALIGN_MAX_POINTS == feature_law.MAX_POINTS
    assert ops.scan_features_plan(32) == (32, 256, 36) and ops.scan_features_plan(5)[0] == 8
    assert len(ops.scan_feature_match_plan()) == 3 and len(ops.scan_pose_trials_plan()) == 3
    for bad in (0, 33):
        with pytest.raises(HipExtensionError):
            ops.scan_features_plan(bad)
    with pytest.raises(HipExtensionError):
        ops.scan_pose_trials_plan(trials=65537)
    with pytest.raises(HipExtensionError):
        ops.scan_pose_trials_plan(keep=4097)


def test_python_wrappers_have_no_cpu_path():
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    pts, off = torch.zeros((4, 3)), torch.tensor([0, 4])
    with pytest.raises(HipExtensionError):
        ops.scan_features(pts, off, torch.zeros((4, 3)), torch.zeros((4, 8), dtype=torch.int32))
    feat, cnt = torch.zeros((4, 36), dtype=torch.uint8), torch.ones(4, dtype=torch.int32)
    with pytest.raises(HipExtensionError):
        ops.scan_feature_match(feat, off, feat, off, cnt, cnt)
    with pytest.raises(HipExtensionError):
        ops.scan_pose_trials(pts, off, pts, off, torch.zeros(4, dtype=torch.int32), 0.1)
    with pytest.raises(HipExtensionError):
        ops.scan_align_global(pts, off, pts, off, 0.1)


def test_arguments_are_checked_before_the_launch(monkeypatch):
    import torch

    from hyperpocket_amd import HipExtensionError, ops
    real = ops.check_input

    def no_device_check(t, name, dtype=torch.float32):
        if not t.is_contiguous() or t.dtype != dtype:
            real(t, name, dtype)

    monkeypatch.setattr(ops, "check_input", no_device_check)
    monkeypatch.setattr(ops, "call", lambda *a: (_ for _ in ()).throw(AssertionError("a launch was reached")))
    pts, off = torch.zeros((6, 3)), torch.tensor([0, 4, 6])
    good = dict(normals=torch.zeros((6, 3)), index=torch.zeros((6, 8), dtype=torch.int32))
    for kw in (dict(normals=torch.zeros((5, 3))), dict(normals=torch.zeros((6, 3), dtype=torch.float64)),
               dict(index=torch.zeros((6, 8), dtype=torch.int64)), dict(index=torch.zeros((5, 8), dtype=torch.int32)),
               dict(index=torch.zeros((6, 33), dtype=torch.int32)), dict(index=torch.zeros((6, 0), dtype=torch.int32)),
               dict(out={"features": torch.zeros((6, 33), dtype=torch.uint8), "count": torch.zeros(6, dtype=torch.int32),
                         "ws": torch.zeros(216, dtype=torch.uint8)})):
        with pytest.raises(HipExtensionError):
            ops.scan_features(pts, off, **dict(good, **kw))
    feat, cnt = torch.zeros((6, 36), dtype=torch.uint8), torch.ones(6, dtype=torch.int32)
    tfeat, toff, tcnt = torch.zeros((5, 36), dtype=torch.uint8), torch.tensor([0, 2, 5]), torch.ones(5, dtype=torch.int32)
    for args in ((feat[:, :33].contiguous(), off, tfeat, toff, cnt, tcnt), (feat, off, tfeat, torch.tensor([0, 5]), cnt, tcnt),
                 (feat, off, tfeat, toff, cnt[:5], tcnt), (feat, off, tfeat, toff, cnt, tcnt.long()),
                 (feat.int(), off, tfeat, toff, cnt, tcnt)):
        with pytest.raises(HipExtensionError):
            ops.scan_feature_match(*args)
    # no rows on one side is served on the host: no launch, the empty result
    match, dist = ops.scan_feature_match(feat, off, tfeat[:0], torch.tensor([0, 0, 0]), cnt, tcnt[:0])
    assert (match == -1).all() and (dist == -1).all() and match.dtype == torch.int32
    tpts = torch.zeros((5, 3))
    m = torch.zeros(6, dtype=torch.int32)
    for kw in (dict(trials=0), dict(trials=65537), dict(keep=0), dict(keep=4097), dict(edge_ratio=-0.1), dict(edge_ratio=1.1),
               dict(min_inliers=-1), dict(inlier_dist=-1.0), dict(inlier_dist=float("nan")), dict(match=m[:5]), dict(match=m.long()),
               dict(streams=torch.zeros(3, dtype=torch.int64)), dict(streams=torch.zeros(2, dtype=torch.int32))):
        args = dict(match=m, inlier_dist=0.1)
        args.update(kw)
        with pytest.raises(HipExtensionError):
            ops.scan_pose_trials(pts, off, tpts, toff, **args)
    for kw in (dict(k=1), dict(k=33), dict(trials=0), dict(keep=5000), dict(max_dist=-1.0), dict(inlier_dist=-2.0),
               dict(normals=torch.zeros((5, 3)))):
        args = dict(max_dist=0.1)
        args.update(kw)
        with pytest.raises(HipExtensionError):
            ops.scan_align_global(pts, off, tpts, toff, **args)


def test_the_signatures():
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(ops.scan_features) == [("points", E), ("offsets", E), ("normals", E), ("index", E), ("out", None)]
    assert sig(ops.scan_feature_match) == [(n, E) for n in ("features", "offsets", "tfeatures", "toffsets", "counts", "tcounts")] + \
        [("out", None)]
    assert sig(ops.scan_pose_trials)[:6] == [(n, E) for n in ("points", "offsets", "tpoints", "toffsets", "match", "inlier_dist")]
    assert sig(ops.scan_pose_trials)[6:] == [("trials", 32768), ("keep", 1024), ("seed", 0), ("streams", None), ("edge_ratio", 0.9),
                                             ("min_inliers", 6), ("out", None), ("ws", None)]
    assert sig(ops.scan_align_global) == [(n, E) for n in ("points", "offsets", "tpoints", "toffsets", "max_dist")] + \
        [("k", 32), ("trials", 32768), ("keep", 1024), ("seed", 0), ("streams", None), ("edge_ratio", 0.9), ("inlier_dist", None),
         ("min_inliers", 6), ("normals", None), ("tnormals", None), ("viewpoints", None), ("tviewpoints", None)]
    assert sig(DeviceScanDataset.aligned_globally) == [("self", E), ("targets", E), ("max_dist", E), ("iters", 10), ("k", 32),
                                                       ("trials", 32768), ("seed", 0), ("viewpoint", (0, 0, 0)),
                                                       ("target_viewpoint", None), ("surface", True), ("coarse", 5)]
    assert sig(DeviceScanDataset.merged_views_globally)[:3] == [("self", E), ("groups", E), ("max_dist", E)]
    # what was there stays as it was: no constructor keyword, the four aligners and the three ops they rest on
    assert list(inspect.signature(DeviceScanDataset.__init__).parameters)[-3:] == ["outliers", "clusters", "plane"]
    assert list(inspect.signature(DeviceScanDataset.from_npy_dir).parameters)[-3:] == ["outliers", "clusters", "plane"]
    assert sig(DeviceScanDataset.aligned_to)[2:] == [("max_dist", E), ("iters", 30), ("yaw", 0), ("axis", (0, 1, 0))]
    assert sig(DeviceScanDataset.merged_views)[2:] == [("max_dist", E), ("iters", 30), ("yaw", 0), ("axis", (0, 1, 0))]
    tail = [("max_dist", E), ("iters", 10), ("yaw", 0), ("axis", (0, 1, 0)), ("k", 16), ("coarse", 5)]
    assert sig(DeviceScanDataset.aligned_to_surface)[2:] == tail and sig(DeviceScanDataset.merged_views_surface)[2:] == tail
    assert sig(ops.scan_normals) == [("points", E), ("offsets", E), ("k", 16), ("viewpoints", None), ("index", None), ("out", None)]
    assert [n for n, _ in sig(ops.scan_align)][:5] == ["points", "offsets", "tpoints", "toffsets", "max_dist"]
    assert ("init", None) in sig(ops.scan_align) and ("init", None) in sig(ops.scan_align_plane)


def test_the_dataset_methods_raise_as_their_twins():
    import torch

    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    data = DeviceScanDataset([torch.rand(50, 3), torch.rand(40, 3)], device="cpu")
    with pytest.raises(HipExtensionError):                         # no CPU path
        data.aligned_globally(torch.rand(30, 3), 0.1)
    with pytest.raises(HipExtensionError):
        data.merged_views_globally([[0, 1]], 0.1)
    with pytest.raises(ValueError):
        data.merged_views_globally([[0, 2]], 0.1)
    with pytest.raises(ValueError):
        data.aligned_globally([torch.rand(30, 3)] * 3, 0.1)


def test_the_fixture_is_what_the_issue_describes():
    source, target, R, t = feature_law.bumpy_sheet(800, seed=0)
    assert source.shape == target.shape == (800, 3) and source.dtype == np.float32
    angle = np.degrees(np.arccos((np.trace(R) - 1) / 2))
    assert abs(angle - 140.0) < 1e-9 and np.allclose(R @ np.array([1.0, 2.0, 3.0]), [1.0, 2.0, 3.0])
    assert np.array_equal(t, [0.3, -0.2, 0.5])
    moved = source.astype(np.float64) @ R.T + t                   # the two samplings are independent: same sheet, other rows
    assert np.abs(moved[:, :2]).max() < 1.02 and not np.allclose(moved, target, atol=1e-3)

"""CPU suite for the completion metrics: the `fixed/` directory protocol of the process() drivers, host-side argument
checks of hp_cloud_pairs / hp_cloud_pairs_workspace_floats (nothing reaches a GPU), and the numpy-only helpers."""
import ctypes
import glob
import importlib.util
import os

import numpy as np
import pytest

from conftest import PKG_DIR, golden

c_int, c_long, c_float, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
CHAMFER, HAUSDORFF, COVERED = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = ctypes.CDLL(mod.build(verbose=False))
    so.hp_cloud_pairs_workspace_floats.restype = c_long
    so.hp_cloud_pairs_workspace_floats.argtypes = [c_int, c_int, c_int, c_long]
    so.hp_cloud_pairs.restype = c_int
    so.hp_cloud_pairs.argtypes = [c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_float,
                                  c_void_p, c_void_p, c_void_p]
    return so


def _touch(d, names):
    for n in names:
        np.save(os.path.join(d, n), np.zeros((3, 2), np.float32))


def _fixed_names(shapes, k=10):
    names = []
    for cat, count in shapes:
        for i in range(count):
            names.append(f"{cat}_{i}_existing.npy")
            names += [f"{cat}_{i}_{j}_reconstruction.npy" for j in range(k)]
    return names


def test_grouping_follows_sorted_glob_in_tens(tmp_path):
    from hyperpocket_amd.utils.evaluation.shape_dir import grouped_paths
    _touch(tmp_path, _fixed_names([("chair", 12), ("lamp", 3)]))
    groups, existing = grouped_paths(str(tmp_path), with_existing=True)
    assert len(groups) == len(existing) == 15 and all(len(g) == 10 for g in groups)
    base = [os.path.basename(p) for p in existing]
    assert base == sorted(base)
    # lexicographic, not numeric: chair_10_ and chair_11_ come before chair_1_ and chair_2_
    assert base[:4] == ["chair_0_existing.npy", "chair_10_existing.npy", "chair_11_existing.npy", "chair_1_existing.npy"]
    for g, e in zip(groups, base):
        prefix = e[:-len("existing.npy")]
        assert [os.path.basename(p) for p in g] == [f"{prefix}{j}_reconstruction.npy" for j in range(10)]
    groups2, none = grouped_paths(str(tmp_path), with_existing=False)
    assert groups2 == groups and none is None


def test_grouping_rejects_mismatched_counts(tmp_path):
    from hyperpocket_amd.utils.evaluation.shape_dir import grouped_paths
    with pytest.raises(ValueError):
        grouped_paths(str(tmp_path), with_existing=False)              # empty
    _touch(tmp_path, _fixed_names([("car", 3)]))
    os.remove(os.path.join(tmp_path, "car_2_existing.npy"))
    with pytest.raises(ValueError):
        grouped_paths(str(tmp_path), with_existing=True)               # 3 groups, 2 inputs
    grouped_paths(str(tmp_path), with_existing=False)                  # TMD needs no inputs
    os.remove(os.path.join(tmp_path, "car_2_9_reconstruction.npy"))
    with pytest.raises(ValueError):
        grouped_paths(str(tmp_path), with_existing=False)              # 29 reconstructions


def test_load_points_transposes_the_stored_layout(tmp_path):
    from hyperpocket_amd.utils.evaluation.shape_dir import load_points
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    np.save(os.path.join(tmp_path, "x.npy"), a)
    got = load_points([os.path.join(tmp_path, "x.npy")] * 2)
    assert got.shape == (2, 4, 3) and got.dtype == np.float32 and got.flags.c_contiguous
    assert np.array_equal(got[1], a.T)


def test_scale_to_unit_sphere_matches_the_reference():
    from hyperpocket_amd.utils.evaluation.chamfer import scale_to_unit_sphere
    g = golden("completion")
    np.testing.assert_allclose(scale_to_unit_sphere(g["nn_ref"]), g["unit_sphere"], rtol=1e-6, atol=1e-7)


def test_workspace_query_on_host(lib):
    # TMD at S=64, k=10, N=2048: 2880 pairs, 4 queries per lane -> 2 query tiles per direction, one double per tile
    assert lib.hp_cloud_pairs_workspace_floats(CHAMFER, 2048, 2048, 2880) == 2 * 2880 * 4
    # UHD at Ne=1024: 640 pairs x 1 tile would be under 1024 workgroups -> 2 queries per lane, 2 tiles
    assert lib.hp_cloud_pairs_workspace_floats(HAUSDORFF, 1024, 2048, 640) == 2 * 640 * 2
    assert lib.hp_cloud_pairs_workspace_floats(COVERED, 5, 7, 0) == 0
    for bad in [(3, 8, 8, 1), (-1, 8, 8, 1), (CHAMFER, 0, 8, 1), (CHAMFER, 8, 0, 1), (CHAMFER, 8, 8, -1)]:
        assert lib.hp_cloud_pairs_workspace_floats(*bad) == -1, bad


def test_invalid_arguments_are_rejected_without_a_gpu(lib):
    def call(mode=CHAMFER, na=2, n=8, nb=2, m=8, pairs=1, thres=0.03):
        return lib.hp_cloud_pairs(mode, na, n, None, nb, m, None, pairs, None, thres, None, None, None)

    for kw in [dict(mode=3), dict(mode=-1), dict(na=0), dict(nb=-1), dict(n=0), dict(m=0), dict(pairs=-1),
               dict(mode=COVERED, thres=-1.0), dict(mode=COVERED, n=1 << 24),
               dict(), dict(mode=HAUSDORFF), dict(mode=COVERED)]:     # the last three: NULL pointers
        assert call(**kw) == -1, kw
    for mode in (CHAMFER, HAUSDORFF, COVERED):
        assert call(mode=mode, pairs=0) == 0                           # nothing to do: no pointer is touched


def test_completion_modules_stay_off_scipy_ray_and_the_oracle():
    pkg = os.path.join(PKG_DIR, "hyperpocket_amd")
    files = glob.glob(os.path.join(pkg, "utils", "evaluation", "*.py")) + [os.path.join(pkg, "core", "experiments.py")]
    assert len(files) >= 7
    for f in files:
        src = open(f).read()
        for mod in ("scipy", "ray", "oracle", "sklearn"):
            assert f"import {mod}" not in src and f"from {mod}" not in src, (f, mod)

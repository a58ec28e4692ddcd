"""CPU suite for the occupancy-grid JSD (hyperpocket_amd.utils.metrics, csrc/occupancy.hip): the host functions against
the reference-generated fixture (tests/golden/jsd.npz, make_golden_jsd.py), the argument checks of hp_occupancy_grid, and
the kernel's cell decision run on the host (hp_occupancy_cells_host: the same source the device compiles) against the
fixture's integers.  Nothing here reaches a GPU."""
import ctypes
import importlib.util
import os
import warnings
from ctypes import c_int, c_long, c_void_p

import numpy as np
import pytest
import torch

from conftest import PKG_DIR, golden

RESOLUTIONS = (28, 8, 13)
SETS = ("ball45", "ball50", "cube50", "sphere50", "cube60", "one_point", "n1000")


def tag(R, clip):
    return f"R{R}_{'sphere' if clip else 'cube'}"


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = ctypes.CDLL(mod.build(verbose=False))
    so.hp_occupancy_grid.restype = c_int
    so.hp_occupancy_grid.argtypes = [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p]
    so.hp_occupancy_cells_host.restype = c_int
    so.hp_occupancy_cells_host.argtypes = [c_long, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    return so


@pytest.fixture(scope="module")
def g():
    return golden("jsd")


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("R", RESOLUTIONS)
def test_grid_and_spacing_equal_the_references_bit_for_bit(g, R, clip):
    from hyperpocket_amd.utils.metrics import unit_cube_grid_point_cloud
    grid, spacing = unit_cube_grid_point_cloud(R, clip)
    want = g["grid__" + tag(R, clip)]
    assert grid.dtype == np.float32 and grid.shape == want.shape
    assert np.array_equal(grid.view(np.uint32), want.view(np.uint32))
    assert isinstance(spacing, float) and spacing == float(g["spacing__" + tag(R, clip)])
    if R == 28 and clip:
        assert len(grid) == 10144


def test_fixture_has_no_tie_between_the_two_nearest_centres(g):
    assert float(g["min_gap"]) > 0.0


def test_jensen_shannon_divergence_equals_the_references(g):
    from hyperpocket_amd.utils.metrics import jensen_shannon_divergence
    pairs = [(a, b, 28) for a, b in zip(SETS[:4], SETS[1:5])] + [("n1000", "cube60", 13)]
    for a, b, R in pairs:
        key = f"jsd__{a}__{b}" + ("" if R == 28 else f"__R{R}")
        P = g[f"counters__{a}__{tag(R, True)}"].astype(np.float64)
        Q = g[f"counters__{b}__{tag(R, True)}"].astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = jensen_shannon_divergence(P, Q)
        print(key, got, float(g[key]))
        np.testing.assert_allclose(got, float(g[key]), rtol=1e-10, atol=0)
    assert jensen_shannon_divergence(P, P) == pytest.approx(0.0, abs=1e-12)


def test_jensen_shannon_divergence_rejects_what_the_reference_rejects():
    from hyperpocket_amd.utils.metrics import jensen_shannon_divergence
    with pytest.raises(ValueError, match="Negative values."):
        jensen_shannon_divergence(np.array([1.0, -1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match="Non equal size."):
        jensen_shannon_divergence(np.array([1.0, 2.0]), np.array([1.0, 1.0, 3.0]))


def test_entropy_from_the_fixtures_hit_counts(g, monkeypatch):
    """The host half of entropy_of_occupancy_grid (everything after the kernel) on the fixture's integers."""
    from hyperpocket_amd.utils import metrics
    for name in SETS:
        for R in RESOLUTIONS:
            for clip in (False, True):
                t = tag(R, clip)
                counts, hit = g[f"counters__{name}__{t}"], g[f"clouds_hit__{name}__{t}"]
                monkeypatch.setattr(metrics, "_occupancy_counts", lambda *a, c=counts, h=hit: (c, h))
                ent, counters = metrics.entropy_of_occupancy_grid(g["set__" + name], R, clip)
                np.testing.assert_allclose(ent, float(g[f"entropy__{name}__{t}"]), rtol=1e-10, atol=0)
                assert counters.dtype == np.float64 and np.array_equal(counters, counts)


def _tables(R, clip):
    from hyperpocket_amd.utils.metrics import _grid_columns
    axis, columns, cells = _grid_columns(R, clip)
    assert axis.dtype == np.float32 and columns.dtype == np.uint32 and columns.shape == (R * R,)
    return np.ascontiguousarray(axis), np.ascontiguousarray(columns), cells


def _p(a):
    return a.ctypes.data_as(c_void_p)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("R", RESOLUTIONS)
def test_column_tables_describe_the_references_kept_cells(g, R, clip):
    """kept index base + (k - klo) of every kept cell, unpacked from the column words, numbers the fixture's grid rows."""
    axis, columns, cells = _tables(R, clip)
    grid = g["grid__" + tag(R, clip)].reshape(-1, 3)
    assert cells == len(grid)
    klo, khi, base = columns & 63, (columns >> 6) & 63, columns >> 12
    rows = []
    for c in range(R * R):
        for k in range(int(klo[c]), int(khi[c]) + 1):
            assert int(base[c]) + k - int(klo[c]) == len(rows)
            rows.append((axis[c // R], axis[c % R], axis[k]))
    assert np.array_equal(np.array(rows, np.float32), grid)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("R", RESOLUTIONS)
def test_cell_decision_on_the_host_equals_the_fixture_exactly(lib, g, R, clip):
    axis, columns, cells = _tables(R, clip)
    for name in SETS:
        pts = np.ascontiguousarray(g["set__" + name])
        S, n = pts.shape[:2]
        cell = np.full(S * n, -7, np.int32)
        assert lib.hp_occupancy_cells_host(S * n, _p(pts), R, _p(axis), _p(columns), _p(cell)) == 0
        assert cell.min() >= 0 and cell.max() < cells
        counters = np.bincount(cell, minlength=cells)
        hit = sum(np.bincount(np.unique(row), minlength=cells) for row in cell.reshape(S, n))
        t = tag(R, clip)
        assert np.array_equal(counters, g[f"counters__{name}__{t}"]), (name, t)
        assert np.array_equal(hit, g[f"clouds_hit__{name}__{t}"]), (name, t)


def test_cell_decision_on_the_host_equals_an_exhaustive_fp64_search(lib):
    """Seeded points in and well outside the cube, R = 28 clipped: the column search against the arg-min over all
    10 144 kept centres in fp64."""
    from hyperpocket_amd.utils.metrics import unit_cube_grid_point_cloud
    axis, columns, cells = _tables(28, True)
    grid = unit_cube_grid_point_cloud(28, True)[0].astype(np.float64)
    r = np.random.RandomState(7)
    pts = np.concatenate([r.uniform(-0.75, 0.75, (1500, 3)), r.standard_normal((500, 3)) * 3.0,
                          grid[r.randint(0, cells, 200)], [[1e3, -1e3, 0.01]]]).astype(np.float32)
    cell = np.empty(len(pts), np.int32)
    assert lib.hp_occupancy_cells_host(len(pts), _p(pts), 28, _p(axis), _p(columns), _p(cell)) == 0
    p64 = pts.astype(np.float64)
    for s in range(0, len(pts), 256):
        d2 = ((grid[None, :, :] - p64[s:s + 256, None, :]) ** 2).sum(axis=2)
        # seeded continuous points: the two smallest distances differ by far more than an fp64 rounding, so the
        # summation order of the three squares cannot move the arg-min
        assert np.array_equal(cell[s:s + 256], d2.argmin(axis=1))
    nan = np.array([[0.1, np.nan, 0.0], [np.inf, 0.0, 0.0], [0.1, 0.1, 0.1]], np.float32)
    out = np.empty(3, np.int32)
    assert lib.hp_occupancy_cells_host(3, _p(nan), 28, _p(axis), _p(columns), _p(out)) == 0
    assert out[0] == -1 and out[1] == -1 and out[2] >= 0


def test_invalid_arguments_are_rejected_without_a_gpu(lib):
    """hp_occupancy_grid checks its arguments before any HIP call: -1, no GPU needed.  Non-NULL pointers are host buffers
    that a passing check would hand to the device, so every case below must fail a check."""
    buf = np.zeros(64 * 64, np.int32)
    ok = dict(S=2, n=4, clouds=_p(buf), R=28, axis=_p(buf), columns=_p(buf), cells=10144, counters=_p(buf),
              clouds_hit=_p(buf), nonfinite=_p(buf))

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.hp_occupancy_grid(a["S"], a["n"], a["clouds"], a["R"], a["axis"], a["columns"], a["cells"], a["counters"],
                                     a["clouds_hit"], a["nonfinite"], None)
    for name in ("clouds", "axis", "columns", "counters", "clouds_hit", "nonfinite"):
        assert rc(**{name: None}) == -1, name
    for bad in (dict(S=0), dict(S=-1), dict(n=0), dict(R=1), dict(R=0), dict(R=65), dict(cells=0), dict(cells=28 ** 3 + 1),
                dict(S=1 << 16, n=1 << 15), dict(S=2, n=1 << 30)):
        assert rc(**bad) == -1, bad
    assert lib.hp_occupancy_cells_host(1, None, 28, None, None, None) == -1
    assert lib.hp_occupancy_cells_host(1, _p(buf), 1, _p(buf), _p(buf), _p(buf)) == -1


def test_occupancy_grid_has_no_cpu_fallback():
    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.utils.metrics import entropy_of_occupancy_grid, jsd_between_point_cloud_sets
    a = torch.rand(2, 16, 3) - 0.5
    with pytest.raises(HipExtensionError):
        entropy_of_occupancy_grid(a, 8, True)
    with pytest.raises(HipExtensionError):
        jsd_between_point_cloud_sets(a, a)


def test_resolution_outside_the_kernels_range_raises():
    from hyperpocket_amd.utils.metrics import OCCUPANCY_MAX_RESOLUTION, entropy_of_occupancy_grid
    a = torch.rand(2, 16, 3) - 0.5
    for R in (1, 0, OCCUPANCY_MAX_RESOLUTION + 1):
        with pytest.raises(ValueError):
            entropy_of_occupancy_grid(a, R, True)


def test_sample_completions_refuses_training_mode_and_a_model_without_noise():
    import copy
    from hyperpocket_amd.model.full_model import FullModel
    cfg = {"random_encoder": {"output_size": 8, "use_bias": True, "relu_slope": 0.2},
           "real_encoder": {"output_size": 8, "use_bias": True, "relu_slope": 0.2},
           "hyper_network": {"use_bias": True, "relu_slope": 0.2},
           "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                              "layer_out_channels": [32, 64, 128, 64]},
           "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}
    model = FullModel(copy.deepcopy(cfg))
    with pytest.raises(RuntimeError):
        model.train().sample_completions(torch.zeros(1, 4, 3), torch.zeros(2, 8), 16, 1)
    with pytest.raises(ValueError):
        model.eval().sample_completions(torch.zeros(3, 4, 3), torch.zeros(2, 8), 16, 1)       # 3 clouds, 2 noises
    rec_cfg = copy.deepcopy(cfg)
    rec_cfg["random_encoder"]["output_size"] = 0
    with pytest.raises(ValueError):
        FullModel(rec_cfg).eval().sample_completions(torch.zeros(1, 4, 3), torch.zeros(2, 0), 16, 1)

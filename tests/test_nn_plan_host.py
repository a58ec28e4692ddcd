"""CPU suite for the nearest-neighbour kernels' host side: the queries-per-lane hook of nn_distance_kernel
(hp_nn_set_queries_per_lane) and the two plan queries (hp_nn_queries_per_lane, hp_cloud_pairs_plan) that let the GPU suites
assert which kernel instance a case runs.  Nothing here reaches a GPU."""
import ctypes
import importlib.util
import os
from ctypes import c_int, c_long, POINTER

import pytest

from conftest import PKG_DIR


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = ctypes.CDLL(mod.build(verbose=False))
    so.hp_nn_set_queries_per_lane.restype = c_int
    so.hp_nn_set_queries_per_lane.argtypes = [c_int]
    so.hp_nn_queries_per_lane.restype = c_int
    so.hp_nn_queries_per_lane.argtypes = [c_int, c_int, c_int]
    so.hp_cloud_pairs_plan.restype = c_int
    so.hp_cloud_pairs_plan.argtypes = [c_int, c_int, c_int, c_long, POINTER(c_int), POINTER(c_int)]
    so.hp_chamfer_workspace_floats.restype = c_long
    return so


def test_library_exports_the_hook_and_the_plan_queries(lib):
    for name in ("hp_nn_set_queries_per_lane", "hp_nn_queries_per_lane", "hp_cloud_pairs_plan"):
        assert hasattr(lib, name), name


# the operating points the kernel comment names (structural_losses.hip, nn_pick_r) and the thresholds around them:
# 4 while b * (ceil(n / 1024) + ceil(m / 1024)) >= 512, else 2 while b * (ceil(n / 512) + ceil(m / 512)) >= 512, else 1
@pytest.mark.parametrize("b,n,m,want", [(64, 2048, 2048, 2), (32, 2048, 2048, 1), (64, 8192, 8192, 4),
                                         (256, 64, 64, 4), (255, 64, 64, 1), (300, 40, 1100, 4), (128, 600, 1000, 2),
                                         (70, 64, 64, 1), (1, 1, 1, 1), (128, 2048, 2048, 4), (127, 2048, 2048, 2)])
def test_nn_heuristic_on_the_host(lib, b, n, m, want):
    assert lib.hp_nn_queries_per_lane(b, n, m) == want
    blocks = lambda r: b * (-(-n // (256 * r)) + -(-m // (256 * r)))
    assert want == (4 if blocks(4) >= 512 else 2 if blocks(2) >= 512 else 1)


def test_nn_heuristic_rejects_negative_sizes(lib):
    assert lib.hp_nn_queries_per_lane(-1, 1, 1) == -1


def _plan(lib, mode, n, m, P):
    r, group = c_int(-1), c_int(-1)
    assert lib.hp_cloud_pairs_plan(mode, n, m, P, ctypes.byref(r), ctypes.byref(group)) == 0
    return r.value, group.value


def test_cloud_pairs_plan_of_every_documented_case(lib):
    """The plan recorded next to the GPU suite's cases (tests/test_completion_metrics_gpu.py: PLANS, ORACLE_CASES), mode by mode,
    and that together they reach 1, 2, 4 queries per lane and 1, 2, 4, 8 pairs per workgroup."""
    import test_completion_metrics_gpu as gpu_suite
    seen_r, seen_g = set(), set()
    assert {(n, m, P) for n, m, _, _, P, _ in gpu_suite.CASES} == set(gpu_suite.PLANS)
    for (n, m, P), per_mode in gpu_suite.PLANS.items():
        for mode, want in enumerate(per_mode):
            assert _plan(lib, mode, n, m, P) == want, (n, m, P, mode)
            seen_r.add(want[0])
            seen_g.add(want[1])
    assert seen_r == {1, 2, 4} and seen_g == {1, 2, 4, 8}
    for n, m, _, _, P, rs in gpu_suite.ORACLE_CASES:
        for mode in range(3):
            assert _plan(lib, mode, n, m, P)[0] == rs[mode], (n, m, P, mode)


def test_cloud_pairs_plan_follows_its_rule(lib):
    """4 queries per lane while the launch keeps 1024 workgroups, else 2, else 1; then 8, 4 or 2 pairs per workgroup while 2048
    workgroups remain (cloud_pairs.hip: plan) — restated here and compared over a grid of sizes."""
    tiles = lambda n, r: -(-n // (256 * r))
    for mode in range(3):
        for n, m in [(1, 1), (20, 20), (300, 1025), (600, 100), (2048, 2048), (5000, 700)]:
            for P in (0, 1, 3, 100, 511, 512, 1023, 1024, 2047, 2048, 4096, 10000, 70001):
                for r in (4, 2, 1):
                    t = tiles(n, r) + (tiles(m, r) if mode == 0 else 0)
                    if P * t >= 1024:
                        break
                group = next((g for g in (8, 4, 2) if -(-P // g) * t >= 2048), 1)
                assert _plan(lib, mode, n, m, P) == (r, group), (mode, n, m, P)


def test_cloud_pairs_plan_checks_its_arguments(lib):
    assert lib.hp_cloud_pairs_plan(3, 8, 8, 1, None, None) == -1
    assert lib.hp_cloud_pairs_plan(0, 0, 8, 1, None, None) == -1
    assert lib.hp_cloud_pairs_plan(0, 8, 8, -1, None, None) == -1
    assert lib.hp_cloud_pairs_plan(0, 8, 8, 1, None, None) == 0          # either output may be NULL


def test_queries_per_lane_hook_round_trips(lib):
    load = lib.hp_nn_set_queries_per_lane(-1)        # whatever the setting was: now the load-time value
    try:
        assert lib.hp_nn_set_queries_per_lane(-1) == load
        assert load == 0 or "HP_NN_QUERIES_PER_LANE" in os.environ      # the default is the size heuristic
        prev = load
        for r in (1, 2, 4, 0, 4):
            assert lib.hp_nn_set_queries_per_lane(r) == prev          # returns the previous setting
            prev = r
        for bad in (3, 5, 8, 1 << 20):
            assert lib.hp_nn_set_queries_per_lane(bad) == -1            # rejected ...
            assert lib.hp_nn_set_queries_per_lane(4) == 4               # ... and nothing changed
        assert lib.hp_nn_set_queries_per_lane(-7) == 4                  # any negative value restores the load-time value
        assert lib.hp_nn_set_queries_per_lane(2) == load
        # the heuristic's answer does not depend on the hook
        assert lib.hp_nn_queries_per_lane(64, 8192, 8192) == 4 and lib.hp_nn_queries_per_lane(32, 2048, 2048) == 1
    finally:
        lib.hp_nn_set_queries_per_lane(-1)


def test_chamfer_workspace_covers_every_instance(lib):
    """hp_chamfer_workspace_floats sizes for one query per lane, the instance with the most workgroups: it covers the
    b * (ceil(n / (256 R)) + ceil(m / (256 R))) partials of every R, and does not depend on the hook."""
    try:
        for b, n, m in [(3, 255, 257), (2, 1324, 2079), (300, 40, 1100), (64, 2048, 2048), (1, 1, 1)]:
            sizes = set()
            for r in (0, 1, 2, 4):
                lib.hp_nn_set_queries_per_lane(r)
                sizes.add(lib.hp_chamfer_workspace_floats(b, n, m))
            assert sizes == {b * (-(-n // 256) + -(-m // 256))}
    finally:
        lib.hp_nn_set_queries_per_lane(-1)

"""CPU suite for the exact-assignment law (tests/assign_law.py, the checker of csrc/assign.hip): the auction returns scipy's
optimum on its own integer costs to the last unit, its round counts stay an eighth below the library's default bound, its
outputs do not depend on list or set order, and hp_assign_pairs checks its arguments before any HIP call."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from conftest import PKG_DIR

from assign_law import FAMILIES, OK, CAPPED, OVERFLOW, assign_law, assign_pairs_law, family_pair, quantised_costs

SMALL_N = (1, 2, 3, 64, 65, 256)
SEEDS = (0, 1, 2)
BIG = (("grid", 1024, 0), ("clustered", 2048, 0))       # the slow ones: one seed each


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(verbose=False))
    lib.hp_assign_default_max_rounds.restype = ctypes.c_long
    return lib


_SOLVED = {}


def solved(family, n, seed):
    """(a, b, q, assignment, cost, rounds) of one case, computed once for the module."""
    key = (family, n, seed)
    if key not in _SOLVED:
        a, b = family_pair(family, n, seed)
        q, overflow = quantised_costs(a, b)
        assert not overflow
        assignment, cost, rounds, status = assign_law(a, b)
        assert status == OK
        _SOLVED[key] = (a, b, q, assignment, cost, rounds)
    return _SOLVED[key]


def check_optimal(q, assignment, cost):
    n = len(q)
    assert sorted(assignment.tolist()) == list(range(n)), "not a permutation"
    assert int(q[np.arange(n), assignment].sum()) == int(cost)
    rows, cols = linear_sum_assignment(q)
    assert int(cost) == int(q[rows, cols].sum())


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("family", ["uniform", "clustered", "near", "grid"])
def test_law_reaches_scipys_optimum(family, n):
    for seed in SEEDS:
        _, _, q, assignment, cost, _ = solved(family, n, seed)
        check_optimal(q, assignment, cost)


@pytest.mark.parametrize("family,n,seed", BIG)
def test_law_reaches_scipys_optimum_on_large_clouds(family, n, seed):
    _, _, q, assignment, cost, _ = solved(family, n, seed)
    check_optimal(q, assignment, cost)


@pytest.mark.parametrize("n", SMALL_N)
def test_identical_clouds_under_a_permutation_cost_nothing(n):
    for seed in SEEDS:
        a, b, q, assignment, cost, _ = solved("identical", n, seed)
        assert int(cost) == 0
        assert np.array_equal(b[assignment], a)             # distinct points: the inverse permutation, and unique
        check_optimal(q, assignment, cost)


def test_tie_heavy_grid_has_ties():
    """The 4^3 grid of eighths: most distances occur many times, so the lowest-index rules are exercised."""
    _, _, q, _, _, _ = solved("grid", 256, 0)
    assert len(np.unique(q)) < 64


def test_costs_round_to_nearest_even_and_flag_overflow():
    a = np.zeros((2, 3), np.float32)
    b = np.array([[0.5, 0, 0], [2.5, 0, 0]], np.float32)
    q, overflow = quantised_costs(a, b, scale_log2=0)       # 0.5 -> 0, 2.5 -> 2
    assert not overflow and q.tolist() == [[0, 2], [0, 2]]
    q, overflow = quantised_costs(a, b * 4096, scale_log2=24)
    assert overflow
    assert assign_law(a, b * 4096, scale_log2=24)[3] == OVERFLOW
    assert assign_law(a, np.full((2, 3), np.nan, np.float32))[3] == OVERFLOW
    assert not quantised_costs(a, np.array([[64, 0, 0], [0, 0, 0]], np.float32), scale_log2=24)[1]   # 2^30 itself is allowed


def test_round_bound_stops_a_pair():
    a, b = family_pair("uniform", 64, 0)
    assignment, cost, rounds, status = assign_law(a, b, max_rounds=3)
    assert status == CAPPED and rounds == -1 and cost == -1 and (assignment == -1).all()
    full = solved("uniform", 64, 0)
    again = assign_law(a, b, max_rounds=full[5])            # exactly enough rounds is enough
    assert again[3] == OK and again[2] == full[5] and np.array_equal(again[0], full[3])
    assert assign_law(a, b, max_rounds=full[5] - 1)[3] == CAPPED


def test_default_round_bound_is_eight_times_the_largest_count_seen(lib):
    """hp_assign_default_max_rounds(n) against the law's round counts over every family at every n of this suite."""
    seen = {}
    for n in SMALL_N:
        for family in FAMILIES:
            for seed in SEEDS:
                seen[n] = max(seen.get(n, 0), solved(family, n, seed)[5])
    for family, n, seed in BIG:
        seen[n] = max(seen.get(n, 0), solved(family, n, seed)[5])
    print("largest round counts:", seen)
    for n, rounds in seen.items():
        bound = lib.hp_assign_default_max_rounds(n)
        assert bound >= 8 * rounds, (n, rounds, bound)
        assert bound == 256 * n + 1024
    assert lib.hp_assign_default_max_rounds(0) == -1
    assert lib.hp_assign_default_max_rounds(2049) == -1


def test_invalid_arguments_are_rejected_without_a_gpu(lib):
    f = lib.hp_assign_pairs
    L = ctypes.c_long
    buf = (ctypes.c_float * 12)()
    ints = (ctypes.c_int * 8)()
    cost = (ctypes.c_longlong * 2)()
    good = dict(na=1, n=2, A=buf, nb=1, B=buf, pairs=L(1), ab=ints, scale=20, cap=L(0), asg=ints, cost=cost, rounds=ints)

    def run(**kw):
        a = dict(good, **kw)
        return f(a["na"], a["n"], a["A"], a["nb"], a["B"], a["pairs"], a["ab"], a["scale"], a["cap"], a["asg"], a["cost"],
                 a["rounds"], None)

    for bad in (dict(na=0), dict(nb=0), dict(n=0), dict(n=2049), dict(pairs=L(-1)), dict(scale=-1), dict(scale=25),
                dict(cap=L(-1)), dict(cap=L(1 << 31)), dict(A=None), dict(B=None), dict(ab=None), dict(cost=None),
                dict(rounds=None)):
        assert run(**bad) == -1, bad
    assert run(pairs=L(0), A=None, B=None, ab=None, cost=None, rounds=None) == 0      # a no-op before any pointer is looked at


def test_outputs_follow_the_pair_list_and_the_set_order():
    rng = np.random.default_rng(5)
    A = rng.uniform(-0.5, 0.5, (3, 16, 3)).astype(np.float32)
    B = rng.uniform(-0.5, 0.5, (4, 16, 3)).astype(np.float32)
    pairs = np.array([(i, j) for i in range(3) for j in range(4)] + [(3, 0), (0, -1)])
    asg, cost, rounds = assign_pairs_law(A, B, pairs)
    assert (rounds[-2:] == -2).all() and (cost[-2:] == -1).all() and (asg[-2:] == -1).all() and (rounds[:-2] > 0).all()
    r_asg, r_cost, r_rounds = assign_pairs_law(A, B, pairs[::-1])
    assert np.array_equal(r_asg, asg[::-1]) and np.array_equal(r_cost, cost[::-1]) and np.array_equal(r_rounds, rounds[::-1])
    perm = np.array([2, 0, 1])                              # A[perm][k] = A[perm[k]]: pair (k, j) now names the old (perm[k], j)
    moved = np.array([(int(np.where(perm == i)[0][0]), j) if 0 <= i < 3 else (i, j) for i, j in pairs.tolist()])
    p_asg, p_cost, p_rounds = assign_pairs_law(A[perm], B, moved)
    assert np.array_equal(p_asg, asg) and np.array_equal(p_cost, cost) and np.array_equal(p_rounds, rounds)

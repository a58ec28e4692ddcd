"""CPU suite for tests/knn_grid_law.py: the model of the grid search (cell assignment by edges, block growth, stopping rule)
gives knn_law.knn_scan's lists bit for bit over clouds and grids chosen to sit on every edge of the rule — the proof, before
any GPU run, that the stopping rule is conservative under fp32 rounding; and the long statistics law equals keep_law where
that is defined and an independent exact evaluation beyond it."""
from fractions import Fraction

import numpy as np
import pytest

import knn_grid_law
import knn_law

K = 9


def _lattice():
    g = np.arange(7, dtype=np.float32) * np.float32(0.5)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.float32(-1.5)


def _clouds():
    r = np.random.RandomState(3)
    out = {"uniform": r.uniform(-1, 1, (500, 3)).astype(np.float32),
           "identical": np.full((300, 3), 0.375, dtype=np.float32),
           "lattice": _lattice()}
    far = (1e6 + r.randint(0, 64, (400, 3)) * 0.0625).astype(np.float32)          # on the fp32 grid at 10^6
    out["offset"] = far
    huge = r.uniform(-1, 1, (200, 3)).astype(np.float32)
    huge[:6, 0] = (3e38, -3e38, 3e38, -3e38, 3e38, -3e38)
    huge[6:9, 2] = (3e38, -3e38, 3e38)
    out["huge"] = huge
    line = np.zeros((400, 3), dtype=np.float32)
    line[:, 1] = r.permutation(400) * 0.25
    out["line"] = line
    bad = r.uniform(-1, 1, (300, 3)).astype(np.float32)
    rows = r.permutation(300)[:45]
    bad[rows[:15], r.randint(0, 3, 15)] = np.nan
    bad[rows[15:30], r.randint(0, 3, 15)] = np.inf
    bad[rows[30:], r.randint(0, 3, 15)] = -np.inf
    out["non-finite"] = bad
    for n in (1, 2, K - 1):
        out[f"short{n}"] = r.uniform(-1, 1, (n, 3)).astype(np.float32)
    return out


CLOUDS = _clouds()


def _box(cloud):
    ok = cloud[np.isfinite(cloud).all(axis=1)]
    return ok.min(axis=0), ok.max(axis=0)


def _grids(name, cloud):
    """(what, lo, h, G) for one cloud: one cell; 2-3 cells per axis; h below the point spacing; a lo that is not the box
    minimum; and the cloud's own edge case."""
    lo, hi = _box(cloud)
    with np.errstate(over="ignore"):
        ext = (hi - lo).astype(np.float32)
    good = np.isfinite(ext) & (ext > 0)
    emax = float(ext[good].max()) if good.any() else 1.0

    def cells(h, cap=1024):
        return [min(cap, int(ext[c] / np.float32(h)) + 1) if good[c] else 1 for c in range(3)]

    yield "one cell", lo, emax * 2, (1, 1, 1)
    yield "two to three", lo, emax / 2.5, cells(emax / 2.5)
    yield "fine", lo, emax / 40, cells(emax / 40)                   # many empty shells
    yield "shifted lo", lo + np.float32(0.37 * emax), emax / 5, cells(emax / 5)   # rows below lo: the first cell is unbounded
    yield "too few cells", lo, emax / 20, cells(emax / 20, cap=7)   # rows beyond the last edge: the last cell is unbounded
    if name == "lattice":
        yield "edges on rows", lo, 0.5, (7, 7, 7)                   # spacing == h, lo on a lattice point
        yield "edges on rows, short", lo, 0.5, (5, 6, 7)
    if name == "offset":
        yield "h = 0.25 at 1e6", lo, 0.25, cells(0.25)
        yield "h below the ulp at 1e6", lo, 0.01, cells(0.01)       # equal consecutive edges: empty cells


CASES = [(name, what, lo, h, G) for name, cloud in CLOUDS.items() for what, lo, h, G in _grids(name, cloud)]


@pytest.mark.parametrize("name,what,lo,h,G", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_the_model_equals_the_law(name, what, lo, h, G):
    cloud = CLOUDS[name]
    want = knn_law.knn_scan(cloud, K)
    for group in (1, 64):
        stats = {}
        got = knn_grid_law.grid_search_model(cloud, K, lo, h, G, group=group, stats=stats)
        assert np.array_equal(got[0], want[0]), (name, what, group)
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (name, what, group)
    if what == "fine" and name == "uniform":
        assert min(G) >= 8 and stats["sweeps"] > len(cloud) // 64   # the case ran on many cells and grew its blocks ...
        assert stats["early"] == stats["groups"] >= len(cloud) // 64    # ... and the rule, not the grid's end, stopped every group


@pytest.mark.parametrize("name", ["uniform", "lattice", "offset", "huge", "non-finite", "short2"])
def test_cross_set_queries_inside_and_far_outside(name):
    cloud = CLOUDS[name]
    lo, hi = _box(cloud)
    r = np.random.RandomState(8)
    mid = (lo / 2 + hi / 2).astype(np.float32)
    inside = (mid + r.uniform(-0.4, 0.4, (40, 3))).astype(np.float32)
    outside = (mid + r.choice([-1e4, 1e4, 0.0], (40, 3)) + r.uniform(-1, 1, (40, 3))).astype(np.float32)
    queries = np.concatenate([inside, outside, cloud[:10], np.full((1, 3), np.nan, np.float32),
                              np.array([[3e38, -3e38, 0]], np.float32)])
    for what, glo, h, G in _grids(name, cloud):
        for ex in (False, True):
            want = knn_law.knn_scan(cloud, K, queries, exclude_self=ex)
            got = knn_grid_law.grid_search_model(cloud, K, glo, h, G, queries=queries, exclude_self=ex, group=16)
            assert np.array_equal(got[0], want[0]), (name, what, ex)
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (name, what, ex)


def test_knn_rows_is_the_law_at_the_sampled_rows():
    cloud = CLOUDS["non-finite"]
    rows = np.random.RandomState(1).permutation(len(cloud))[:80]
    want = knn_law.knn_scan(cloud, 16)
    got = knn_grid_law.knn_rows(cloud, 16, rows)
    assert np.array_equal(got[0], want[0][rows]) and np.array_equal(got[1].view(np.uint32), want[1][rows].view(np.uint32))


def test_the_long_statistics_equal_the_short_ones_where_those_are_defined():
    points, _ = knn_law.shell_with_strays()
    _, m, _ = knn_law.outliers_law(points, [0, len(points)], 16, 2.0)
    r = np.random.RandomState(6)
    sets = [m, r.uniform(0, 3, 65536).astype(np.float32), r.uniform(1, 2, 65536).astype(np.float32),
            np.full(65536, 7.0, np.float32), r.uniform(0, 1e-40, 5000).astype(np.float32), np.zeros(10, np.float32),
            np.array([np.inf, 2.0], np.float32), np.array([np.inf, np.nan], np.float32)]
    sets[1][::7] = np.inf
    for m in sets:
        for ratio in (0.0, 1.0, 2.0):
            a, b = knn_law.keep_law(m, ratio), knn_grid_law.keep_law_long(m, ratio)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def long_means(n=300000, seed=12):
    """n synthetic m_i in [M/2, M] whose S2 passes 2^64 — the 64-bit sum of knn.hip would have wrapped — with a few absent."""
    r = np.random.RandomState(seed)
    m = r.uniform(0.5, 1.0, n).astype(np.float32) * np.float32(1.75)
    m[0] = np.float32(1.75)
    m[r.randint(1, n, 20)] = np.inf
    return m


def test_the_long_statistics_beyond_64_bits_against_exact_fractions():
    m = long_means()
    part = np.isfinite(m)
    q = [int(v) for v in np.trunc(np.ldexp(m[part].astype(np.float64), 23 - 0))]       # M = 1.75: e = 0
    assert max(q) < (1 << 24) and max(q) == int(1.75 * 2 ** 23)
    S1, S2, n_p = sum(q), sum(v * v for v in q), len(q)
    assert S2 >= 1 << 64
    for ratio in (0.0, 0.5, 1.0, 2.0):
        keep, kept = knn_grid_law.keep_law_long(m, ratio)
        # the same lines, each operation rounded once: Fraction arithmetic rounded by float() is a correctly rounded double
        f1, f2 = float(Fraction(S1)), float(Fraction(S2))
        mu = float(Fraction(f1) / n_p)
        prod = float(Fraction(mu) * Fraction(f1))
        var = max(0.0, float(Fraction(float(Fraction(f2) - Fraction(prod))) / (n_p - 1)))
        thr = float(Fraction(mu) + Fraction(float(Fraction(float(np.float32(ratio))) * Fraction(float(np.sqrt(np.float64(var)))))))
        want = np.zeros(len(m), dtype=bool)
        want[np.flatnonzero(part)] = [Fraction(v) <= Fraction(thr) for v in q]
        assert np.array_equal(keep, want) and kept == int(want.sum()) and not keep[~part].any()
        assert 0 < kept <= n_p and (ratio > 0 or kept < n_p)

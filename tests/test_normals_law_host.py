"""CPU suite for the surface-normal law (tests/normals_law.py): the law against numpy.linalg.eigh of the unquantised fp64
scatter, against geometry — a plane, a sphere —, its undefined results, the sweep count and the exactness bound."""
import functools

import numpy as np
import pytest

import knn_law
import normals_law as law

f32 = np.float32
QNAN_BITS = 0x7FC00000

# The largest value the law measures on the three fixtures, in this file's own run (printed by the test): the angle to the fp64
# eigenvector times the relative gap (l1 - l0) / l2, and the curvature's absolute difference.  Both come from the 2^-19
# quantisation of the differences.  Measured: shell 1.28e-6 / 9.5e-8, slab 1.10e-6 / 4.8e-7, mix 1.22e-6 / 6.2e-7.
ANGLE_GAP_MEASURED = 1.28e-6
CURVATURE_MEASURED = 6.2e-7


@functools.lru_cache(maxsize=None)
def _fixture(name):
    if name == "mix":
        points, offsets, index = law.mix()
    else:
        points, index = getattr(law, name)()
        offsets = np.array([0, len(points)], dtype=np.int64)
    assert len(points) == 1024 and index.shape == (1024, 16)
    return points, offsets, index, law.reference_law(points, offsets, index)


def _errors(got, ref):
    (normal, curvature, _), (rn, rc, gap, ok) = got, ref
    live = ~np.isnan(curvature)
    assert np.array_equal(live, ok) and live.sum() > 1000
    return (law.angle(normal[live], rn[live]) * gap[live]).max(), np.abs(curvature[live].astype(np.float64) - rc[live]).max()


@pytest.mark.parametrize("name", ["shell", "slab", "mix"])
def test_the_law_against_fp64_eigh(name):
    points, offsets, index, ref = _fixture(name)
    got = law.normals_law(points, offsets, index)
    ang, curv = _errors(got, ref)
    print(f"{name}: angle x gap {ang:.3e}, curvature {curv:.3e}")
    assert ang <= 4 * ANGLE_GAP_MEASURED and curv <= 4 * CURVATURE_MEASURED
    live = ~np.isnan(got[1])
    assert np.abs(np.linalg.norm(got[0][live].astype(np.float64), axis=1) - 1).max() < 1e-7       # unit, to fp32 rounding
    assert (got[1][live] >= 0).all() and (got[1][live] <= f32(1 / 3)).all()
    assert (np.abs(got[0][live]).max(axis=1) == got[0][live].max(axis=1)).all()                     # the sign rule
    if name == "shell":                                             # the normal of a sphere is the radius
        assert law.angle(got[0], points).max() < 0.15
    if name == "slab":                                              # sigma / spacing = 0.02 / 0.06: flat, up to the jitter
        assert np.median(np.abs(got[0][:, 1])) > 0.9 and np.median(got[1]) < 0.1


@pytest.mark.parametrize("name", ["shell", "slab", "mix"])
def test_four_sweeps_agree_with_six(name):
    points, offsets, index, ref = _fixture(name)
    six, four = law.normals_law(points, offsets, index), law.normals_law(points, offsets, index, sweeps=4)
    assert law.SWEEPS == 6
    ang, curv = _errors(four, ref)
    assert ang <= 4 * ANGLE_GAP_MEASURED and curv <= 4 * CURVATURE_MEASURED
    live = ~np.isnan(six[1])
    gap = ref[2][live]
    assert (law.angle(four[0][live], six[0][live]) * gap).max() <= 4 * ANGLE_GAP_MEASURED
    assert np.abs(four[1][live].astype(np.float64) - six[1][live]).max() <= 4 * CURVATURE_MEASURED
    three = law.normals_law(points, offsets, index, sweeps=3)      # ... and three do not always: that is why the count is fixed
    print(f"{name}: 3 sweeps vs 6, angle x gap {(law.angle(three[0][live], six[0][live]) * gap).max():.3e}")


def test_a_plane_is_exact_and_the_viewpoint_turns_it():
    r = np.random.RandomState(5)
    cloud = np.stack([r.uniform(-1, 1, 500), np.full(500, 0.25), r.uniform(-1, 1, 500)], axis=1).astype(f32)
    index = knn_law.knn_scan(cloud, 16)[0]
    normal, curvature, count = law.normals_scan(cloud, index)
    assert (normal == np.array([0, 1, 0], f32)).all() and (curvature == 0).all() and (count == 17).all()
    above, _, _ = law.normals_scan(cloud, index, viewpoint=(0.0, 3.0, 0.0))
    below, _, _ = law.normals_scan(cloud, index, viewpoint=(0.0, -3.0, 0.0))
    assert np.array_equal(above.view(np.uint32), normal.view(np.uint32))
    assert (below == np.array([0, -1, 0], f32)).all()
    on, _, _ = law.normals_scan(cloud, index, viewpoint=(0.0, 0.25, 0.0))      # dot == 0: not < 0, no flip
    nan, _, _ = law.normals_scan(cloud, index, viewpoint=(np.nan, 0.0, 0.0))   # a NaN dot never flips
    assert (on == normal).all() and (nan == normal).all()
    # per scan: the second scan's viewpoint is its own
    two = np.concatenate([cloud, cloud])
    n2, _, _ = law.normals_law(two, [0, 500, 1000], np.concatenate([index, index]), viewpoints=[[0, 3, 0], [0, -3, 0]])
    assert (n2[:500, 1] == 1).all() and (n2[500:, 1] == -1).all()


def _undefined(normal, curvature, rows):
    return (normal[rows].view(np.uint32) == QNAN_BITS).all() and (curvature[rows].view(np.uint32) == QNAN_BITS).all()


def test_undefined_results_and_counts():
    r = np.random.RandomState(7)
    a, b, c = r.uniform(-1, 1, (1, 3)), r.uniform(-1, 1, (2, 3)), r.uniform(-1, 1, (40, 3))
    same = np.full((6, 3), 0.375)                                   # every neighbour on the row itself: M == 0
    huge = np.array([[3e38, 0, 0], [-3e38, 0, 0], [0, 1, 0], [1, 0, 1]])       # dq overflows for rows 0 and 1
    points = np.concatenate([a, b, c, same, huge]).astype(f32)
    points[3 + 5] = np.nan                                          # an absent row of the third scan
    offsets = np.array([0, 1, 3, 43, 49, 53])
    index = knn_law.knn_law(points, offsets, 8)[0]
    normal, curvature, count = law.normals_law(points, offsets, index)
    assert count[:3].tolist() == [1, 2, 2] and _undefined(normal, curvature, slice(0, 3))
    assert count[8] == 0 and _undefined(normal, curvature, [8])
    rest = np.setdiff1d(np.arange(3, 43), [8])
    assert (count[rest] == 9).all() and np.isfinite(normal[rest]).all() and not np.isin(index[3:43], 5).any()
    assert (count[43:49] == 6).all() and _undefined(normal, curvature, slice(43, 49))
    assert (count[49:53] == 4).all() and _undefined(normal, curvature, [49, 50]) and np.isfinite(normal[51:53]).all()
    # an absent row as a listed neighbour is left out; an out-of-range slot is ignored
    idx = index.copy()
    idx[3:43, 0] = 5
    idx[3:43, 1] = np.where(np.arange(40) % 2 == 0, 40, -7)
    idx[3:43, 2] = 1 << 30
    n2, c2, cnt2 = law.normals_law(points, offsets, idx)
    assert (cnt2[rest] == 6).all() and cnt2[8] == 0
    idx[3:43, :3] = -1
    n3, c3, cnt3 = law.normals_law(points, offsets, idx)
    assert np.array_equal(n2.view(np.uint32), n3.view(np.uint32)) and np.array_equal(c2.view(np.uint32), c3.view(np.uint32))
    assert np.array_equal(cnt2, cnt3)
    # duplicates and the row itself count as listed
    idx = index[3:43].copy()
    idx[:, 7] = idx[:, 0]
    idx[:, 6] = np.arange(40)
    _, _, cnt4 = law.normals_scan(points[3:43], idx)
    assert (cnt4[np.arange(40) != 5] == 9).all()
    # two present neighbours are enough, one is not
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    n5, c5, cnt5 = law.normals_scan(tri, np.array([[1, 2], [0, 2], [0, -1]], np.int32))
    assert cnt5.tolist() == [3, 3, 2] and (n5[:2] == np.array([0, 0, 1], f32)).all() and (c5[:2] == 0).all()
    assert _undefined(n5, c5, [2])


def test_the_scatter_is_exact_at_33_rows_of_extreme_q():
    top = (1 << 20) - 1
    worst = 0
    for signs in ((1, 1, 1), (1, -1, 1), (-1, -1, -1)):
        for k_pos in (32, 16, 31):                                  # every q at the edge; half on each side; one against the rest
            q = np.full((1, 32, 3), top, dtype=np.int64) * np.array(signs)
            q[0, k_pos:] *= -1
            C = law.scatter(q, np.array([33]))[0]
            m, S1 = 33, [sum(int(v) for v in q[0, :, a]) for a in range(3)]
            for a in range(3):
                for b in range(3):
                    exact = m * sum(int(x) * int(y) for x, y in zip(q[0, :, a], q[0, :, b])) - S1[a] * S1[b]
                    assert int(C[a, b]) == exact and abs(exact) < 1 << 53
                    assert float(np.float64(C[a, b])) == exact      # the conversion is exact
                    worst = max(worst, abs(exact))
            assert 0 <= int(np.trace(C)) < 1 << 53
    assert worst == 33 * 32 * top * top and worst < 1 << 52         # half the rows on each side: S_a = 0, the largest entry
    with pytest.raises(AssertionError):                             # a 34th row is outside the bound's premise
        law.scatter(np.zeros((1, 33, 3), np.int64), np.array([34]))


def test_rotation_formulas_diagonalise():
    """Six sweeps leave nothing off the diagonal and keep V orthogonal and A's spectrum."""
    r = np.random.RandomState(1)
    q = r.randint(-(1 << 20) + 1, 1 << 20, (200, 16, 3)).astype(np.int64)
    q[:50, :, 2] = q[:50, :, 0] // 1024                             # nearly flat
    q[50:100, :, 1:] = q[50:100, :, :1] // 4096                     # nearly collinear
    C = law.scatter(q, np.full(200, 17))
    lam, V = law.jacobi(C)
    want = np.linalg.eigvalsh(C.astype(np.float64))
    scale = want[:, 2:]
    assert (np.abs(np.sort(lam, axis=1) - want) <= 1e-14 * scale).all()
    assert np.abs(np.einsum("nki,nkj->nij", V, V) - np.eye(3)).max() < 1e-14
    back = np.einsum("nik,nk,njk->nij", V, lam, V)
    assert (np.abs(back - C) <= 1e-14 * scale[:, :, None]).all()

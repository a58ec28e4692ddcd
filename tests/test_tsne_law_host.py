"""CPU suite of the exact t-SNE: the law of tests/tsne_law.py against scikit-learn, its behaviour on degenerate inputs, the
classical-scaling start against SVD PCA scores, and what the library answers on the host — the plan query and the argument
checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

import tsne_law as law


@pytest.fixture(scope="module")
def three_clusters():
    X, labels = law.clusters(3, 96, 64)
    D = law.sqdist(X).astype(np.float32)
    return X, D, labels


def test_joint_probabilities_match_scikit_learn(three_clusters):
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    _, D, _ = three_clusters
    want = squareform(_t_sne._joint_probabilities(D, 10.0, 0))
    C, beta, steps, H = law.conditional(D, 10.0)
    P = law.joint(C)
    gap = np.abs(P - want)[~np.eye(len(D), dtype=bool)].max() / want.max()
    print("joint P against scikit-learn's float32 search, largest gap over max P:", gap)
    assert gap <= 1e-5
    assert steps.max() < law.SEARCH_STEPS and np.abs(H - math.log(10.0)).max() <= law.SEARCH_TOL
    assert np.array_equal(P, P.T) and not P.diagonal().any() and abs(P.sum() - 1) <= len(D) ** 2 * law.EPS64 + 1e-13


def test_gradient_matches_scikit_learn(three_clusters):
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    _, D, _ = three_clusters
    n = len(D)
    P32 = law.joint(law.conditional(D, 10.0)[0]).astype(np.float32)
    r = np.random.RandomState(5)
    for scale in (1e-4, 1.0):
        Y = (r.randn(n, 2) * scale).astype(np.float32)
        kl, grad = _t_sne._kl_divergence(Y.astype(np.float64).ravel(), squareform(P32.astype(np.float64)), 1, n, 2)
        got = law.gradient(P32, Y)
        gap = np.abs(got["g"].ravel() - grad).max() / np.abs(grad).max()
        print("gradient against scikit-learn at scale", scale, ":", gap, "kl", abs(got["kl"] - kl) / abs(kl))
        assert gap <= 1e-12 and abs(got["kl"] - kl) <= 1e-12 * abs(kl)
        assert np.all(got["A"] >= np.abs(got["g"]))


def test_identical_points_give_a_uniform_finite_P():
    n = 40
    C, beta, steps, H = law.conditional(law.identical_points(n), 10.0)
    assert np.all(steps == law.SEARCH_STEPS) and np.all(np.isfinite(beta)) and np.all(np.isfinite(C))
    P = law.joint(C)
    off = ~np.eye(n, dtype=bool)
    assert np.allclose(P[off], 1.0 / (n * (n - 1)), rtol=1e-12, atol=0) and not P.diagonal().any()


def test_duplicates_and_a_far_outlier_converge_on_every_row():
    D = law.duplicates_and_outlier()
    C, beta, steps, H = law.conditional(D, 2.0)
    assert np.all(steps < law.SEARCH_STEPS) and np.abs(H - math.log(2.0)).max() <= law.SEARCH_TOL
    assert np.all(np.isfinite(C)) and np.all(np.isfinite(law.joint(C))) and np.allclose(C.sum(1), 1.0)
    at = law.conditional_at(D, beta)
    assert np.allclose(at["C"], C, rtol=1e-12, atol=0) and np.allclose(at["H"], H, rtol=0, atol=1e-12)
    assert np.all(np.isfinite(at["H_bar"])) and np.all(np.isfinite(law.joint_bar(at)))


def test_update_is_float32_and_keeps_the_stated_order():
    r = np.random.RandomState(1)
    g, upd, gains, Y = (r.randn(9, 2).astype(np.float32) for _ in range(4))
    gains = np.abs(gains) + np.float32(0.01)
    upd[0], g[1] = 0, 0
    Y1, u1, g1 = law.update(g, upd, gains, Y, 0.5, 200.0)
    assert Y1.dtype == u1.dtype == g1.dtype == np.float32
    inc = upd * g < 0
    want_gains = np.maximum(np.where(inc, gains + np.float32(0.2), gains * np.float32(0.8)), np.float32(0.01))
    assert np.array_equal(g1, want_gains) and not inc[0].any() and not inc[1].any()
    assert np.array_equal(u1, np.float32(0.5) * upd - np.float32(200.0) * (g * want_gains)) and np.array_equal(Y1, Y + u1)


def test_descent_lowers_the_kl_in_both_state_types(three_clusters):
    _, D, _ = three_clusters
    P = law.joint(law.conditional(D, 10.0)[0]).astype(np.float32)
    Y0 = (np.random.RandomState(2).randn(len(D), 2) * 1e-4).astype(np.float32)
    lr = max(len(D) / 12.0 / 4.0, 50.0)
    for dtype in (np.float64, np.float32):
        Y = law.descend(P, Y0, 60, 20, 12.0, lr, dtype=dtype)
        assert Y.dtype == dtype and law.kl_of(P, Y) < law.kl_of(P, Y0)


def test_classical_scaling_gives_the_svd_pca_scores():
    from hyperpocket_amd.utils.tsne import classical_scaling
    X = (np.random.RandomState(7).randn(50, 300) * np.linspace(3.0, 0.1, 300)).astype(np.float32)
    got = classical_scaling(torch.from_numpy(law.sqdist(X))).numpy().astype(np.float64)
    want = law.pca_scores(X)
    want = want * np.where(want[np.abs(want).argmax(0), np.arange(2)] < 0, -1.0, 1.0)
    want = want / want[:, 0].std() * 1e-4
    gap = np.abs(got - want).max() / np.abs(want).max()
    print("classical scaling against SVD PCA scores:", gap)
    assert gap <= 1e-6                                       # the result is rounded to float32: 6e-8 of an entry
    assert abs(got[:, 0].std() - 1e-4) <= 1e-10 and np.all(got[np.abs(got).argmax(0), np.arange(2)] > 0)
    with pytest.raises(ValueError):
        from hyperpocket_amd.utils.tsne import initial_embedding
        initial_embedding("spectral", 50, None, 0, "cpu")


def test_plan_query_and_argument_checks_run_on_the_host():
    lib = law.library()
    assert law.plan(5000, 19011) == law.plan(2, 1) and min(law.plan(2, 1)) >= 1
    tile, kchunk = law.plan(5000, 19011)
    assert law.sqdist_bar(19011, kchunk) == (kchunk + -(-19011 // kchunk) + 4) * law.U
    t, c = ctypes.c_int(0), ctypes.c_int(0)
    for n, d in ((1, 4), (16385, 4), (8, 0), (-3, 4)):
        assert lib.hp_pairwise_sqdist_plan(n, d, ctypes.byref(t), ctypes.byref(c)) == -1
    assert lib.hp_tsne_affinities_workspace_floats(100) == 100 * 100 + 101 and lib.hp_tsne_affinities_workspace_floats(1) == -1
    one = (ctypes.c_float * 64)()
    p = ctypes.cast(one, ctypes.c_void_p)
    f, L = ctypes.c_float, ctypes.c_long
    for n in (1, 16385):
        assert lib.hp_pairwise_sqdist(n, 4, p, L(4), p, None) == -1
        assert lib.hp_tsne_affinities(n, p, f(0.5), p, p, p, p, None) == -1
        assert lib.hp_tsne_gradient(n, p, f(1.0), p, p, None, None) == -1
        assert lib.hp_tsne_update(n, p, p, p, p, f(0.5), f(1.0), f(0.01), None, None) == -1
        assert lib.hp_tsne_descend(n, p, p, p, p, p, 0, 1, 1, f(12.0), f(1.0), None, None) == -1
    assert lib.hp_pairwise_sqdist(4, 0, p, L(4), p, None) == -1 and lib.hp_pairwise_sqdist(4, 4, p, L(3), p, None) == -1
    assert lib.hp_pairwise_sqdist(4, 4, None, L(4), p, None) == -1
    for perplexity in (0.0, -1.0, 4.0, 5.0):
        assert lib.hp_tsne_affinities(4, p, f(perplexity), p, p, p, p, None) == -1
    assert lib.hp_tsne_affinities(4, p, f(2.0), p, p, p, None, None) == -1
    assert lib.hp_tsne_gradient(4, p, f(1.0), None, p, None, None) == -1
    assert lib.hp_tsne_update(4, p, p, None, p, f(0.5), f(1.0), f(0.01), None, None) == -1
    assert lib.hp_tsne_descend(4, p, p, p, p, p, -1, 1, 1, f(12.0), f(1.0), None, None) == -1

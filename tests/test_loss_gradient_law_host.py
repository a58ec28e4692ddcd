"""Host test of tests/loss_gradient_law.py: each law equals torch float64 autograd of the plain statement of its loss, and the
case tables of tests/test_loss_gradients_gpu.py reach every edge of the kernels.  No GPU."""
import numpy as np
import torch

import loss_gradient_law as law

_B, _N, _M = 2, 40, 55


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _pairwise(x, y):
    return ((x[:, :, None, :] - y[:, None, :, :]) ** 2).sum(-1)          # (b, n, m)


def test_nn_grad_law_equals_autograd_of_the_weighted_minima():
    """sum_i w1_i min_j |x_i - y_j|^2 + sum_j w2_j min_i |x_i - y_j|^2 in float64: its autograd is nn_grad_law on both sides
    with the arg-min indices handed in; with w1 = w2 = g it is chamfer_backward_law."""
    a, c = law.clouds(1, _B, _N, _M)
    r = np.random.RandomState(2)
    w1, w2 = r.randn(_B, _N).astype(np.float32), r.randn(_B, _M).astype(np.float32)
    x, y = torch.from_numpy(a).double().requires_grad_(True), torch.from_numpy(c).double().requires_grad_(True)
    d = _pairwise(x, y)
    m1, i1 = d.min(2)
    m2, i2 = d.min(1)
    (m1 * torch.from_numpy(w1).double()).sum().add((m2 * torch.from_numpy(w2).double()).sum()).backward()
    s1 = law.nn_grad_law(a, i1.numpy(), w1, c, i2.numpy(), w2)
    s2 = law.nn_grad_law(c, i2.numpy(), w2, a, i1.numpy(), w1)
    assert _rel(s1["out"], x.grad.numpy()) <= 1e-12 and _rel(s2["out"], y.grad.numpy()) <= 1e-12
    # the by-products: counts, absolute sums, direct term
    assert s1["cnt"].sum() == _B * _M and s2["cnt"].sum() == _B * _N
    assert np.all(s1["A"] >= np.abs(s1["out"] - s1["direct"]) * (1 - 1e-12))
    assert np.array_equal(s1["A"][s1["cnt"] == 0], np.zeros_like(s1["A"][s1["cnt"] == 0]))
    assert np.all(s1["M"] > 0) and np.all(s1["M"] == s1["M"][:, :1])     # one tile per cloud

    x.grad = y.grad = None
    d = _pairwise(x, y)
    g = np.float32(-0.37)
    ((d.min(2)[0].sum() + d.min(1)[0].sum()) * float(g)).backward()
    assert _rel(law.chamfer_backward_law(a, i1.numpy(), c, i2.numpy(), g)["out"], x.grad.numpy()) <= 1e-12
    assert _rel(law.chamfer_backward_law(c, i2.numpy(), a, i1.numpy(), g)["out"], y.grad.numpy()) <= 1e-12


def test_nn_grad_law_tile_maximum_and_non_finite_terms():
    """M is per 2048-target tile and over the finite fp32 terms; a non-finite upstream reaches exactly the chosen target."""
    b, n, m = 1, 6, 2050
    t, s = np.zeros((b, m, 3), np.float32), np.ones((b, n, 3), np.float32)
    idx_s = np.array([[0, 0, 2047, 2048, 2049, 2049]], np.int32)
    g_s = np.array([[1, 2, 3, 0.5, np.inf, 0.25]], np.float32)
    out = law.nn_grad_law(t, np.zeros((b, m), np.int32), np.zeros((b, m), np.float32), s, idx_s, g_s)
    assert np.all(out["M"][0, :2048] == 6.0) and np.all(out["M"][0, 2048:] == 1.0)
    assert np.array_equal(out["cnt"][0, [0, 1, 2047, 2048, 2049]], [2, 0, 1, 1, 2])
    assert np.all(out["out"][0, 2049] == -np.inf) and np.isfinite(np.delete(out["out"][0], 2049, 0)).all()
    assert np.array_equal(out["out"][0, 0], [-6.0] * 3)
    bar = law.nn_grad_bar(out, n)
    assert np.isfinite(bar[0, :2049]).all() and bar[0, 0, 0] == 4 * law.U * 6 + 2 * 6 * 2.0 ** (3 - 60)


def test_matchcost_laws_equal_autograd_with_match_held_constant():
    a, c = law.clouds(3, _B, _N, _M)
    match = law.synthetic_match(4, _B, _N, _M)
    x, y = torch.from_numpy(a).double().requires_grad_(True), torch.from_numpy(c).double().requires_grad_(True)
    cost = (torch.from_numpy(match).double() * _pairwise(x, y).sqrt().transpose(1, 2)).sum((1, 2))
    cost.sum().backward()
    got, S = law.matchcost_law(a, c, match)
    assert _rel(got, cost.detach().numpy()) <= 1e-12 and np.all(S == got)
    g1, g2, A1, A2 = law.matchcostgrad_law(a, c, match)
    assert _rel(g1, x.grad.numpy()) <= 1e-12 and _rel(g2, y.grad.numpy()) <= 1e-12
    assert np.all(A1 >= np.abs(g1) * (1 - 1e-12)) and np.all(A2 >= np.abs(g2) * (1 - 1e-12))
    # the clamp (approxmatch.cu: e / max(|e|, 1e-10)): a coincident pair gives 0, a pair 1e-12 apart gives match * e / 1e-10
    p, q = np.zeros((1, 1, 3), np.float32), np.zeros((1, 1, 3), np.float32)
    one = np.ones((1, 1, 1), np.float32)
    assert not law.matchcostgrad_law(p, q, one)[0].any()
    p[0, 0, 0] = 1e-12
    assert abs(law.matchcostgrad_law(p, q, one)[0][0, 0, 0] - float(np.float32(1e-12)) / 1e-10) < 1e-15


def test_synthetic_match_is_half_zero_and_spans_six_decades():
    match = law.synthetic_match(5, 3, 257, 65)
    assert match.min() >= 0 and 0.4 < (match == 0).mean() < 0.6
    rows = match.max(2)
    assert rows.max() / rows.min() > 1e4


def test_case_tables_reach_every_edge():
    law.check_tables_reach_every_edge()

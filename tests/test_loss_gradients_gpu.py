"""GPU suite: the gradient and match-cost kernels of csrc/structural_losses.hip against their float64 laws.

  * nn_grad_side_kernel through hp_nndistancegrad (per-point upstreams) and hp_chamfer_backward (one scalar, either output
    NULL): every tile edge, source stride and bits(n) step, worst-case accumulation, magnitudes over sixty decades, mixed
    magnitudes in one tile, order independence bit for bit, non-finite and overflowing terms;
  * matchcost_kernel / matchcost_cloud_kernel / matchcostgrad1_kernel / matchcostgrad2_kernel through hp_matchcost_ws,
    hp_matchcost and hp_matchcostgrad on synthetic `match` at every edge of every kernel.

Laws, bars (derived, with their counts of roundings), case tables and drivers: tests/loss_gradient_law.py.  Every figure is
printed before it is asserted, as a fraction of its bar.  Every index a test passes is in range.
"""
import functools

import numpy as np
import pytest
import torch

import loss_gradient_law as law
from loss_gradient_law import dev

pytestmark = pytest.mark.gpu


def _nn(a, c):
    from hyperpocket_amd.utils.pytorch_structural_losses.StructuralLossesBackend import NNDistance
    return NNDistance(a, c)


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ----------------------------------------------------------------------------------------------------------- nn gradient
def _check_side(got, L, n_src, t, idx_t, g_t, s, what):
    """One side's kernel output against the law L = nn_grad_law(...) of it:
      * where the law is NaN the kernel is NaN; where it is +-Inf or beyond FLT_MAX the kernel is that infinity;
      * every other element is finite and within nn_grad_bar;
      * a target no source chose holds exactly its direct term as fp32 forms it.
    Returns the largest error as a fraction of its bar."""
    got = _np64(got)
    want, bar = L["out"], law.nn_grad_bar(L, n_src)
    nan = np.isnan(want)
    with np.errstate(invalid="ignore"):
        inf = ~nan & (np.abs(want) > law.FLT_MAX)
    fin = ~nan & ~inf
    print(f"{what}: {int(nan.sum())} NaN and {int(inf.sum())} infinite elements in the law; kernel non-finite at "
          f"{int((~np.isfinite(got[nan | inf])).sum())} of them")
    assert np.isnan(got[nan]).all(), (what, "law NaN, kernel", got[nan][~np.isnan(got[nan])][:4])
    assert np.array_equal(got[inf], np.sign(want[inf]) * np.inf), (what, "law overflows, kernel", got[inf][:4], want[inf][:4])
    assert np.isfinite(got[fin]).all(), (what, "kernel not finite where the law is", int((~np.isfinite(got[fin])).sum()))
    err = np.abs(got[fin] - want[fin])
    ratio = float(np.max(err / np.maximum(bar[fin], 1e-300), initial=0.0))
    worst = int(np.argmax(err / np.maximum(bar[fin], 1e-300))) if err.size else 0
    print(f"PARITY {what}: max err/bar = {ratio:.4f}" + (f" (err {err[worst]:.3e}, bar {bar[fin][worst]:.3e})" if err.size else ""))
    assert np.all(err <= bar[fin]), (what, ratio)
    t32, s32, g32 = np.asarray(t, np.float32), np.asarray(s, np.float32), np.asarray(g_t, np.float32)
    rows = np.arange(t32.shape[0])[:, None]
    with np.errstate(all="ignore"):
        direct32 = (g32 * np.float32(2))[..., None] * (t32 - s32[rows, np.asarray(idx_t, np.int64)])
    lone = (L["cnt"] == 0) & np.isfinite(direct32).all(-1)
    assert np.array_equal(got[lone], direct32[lone].astype(np.float64)), (what, "unchosen target differs from its direct term")
    return ratio


def _check_call(x1, x2, g1, i1, g2, i2, what):
    """hp_nndistancegrad on (x1, x2) with the given indices and upstreams, both sides against the law."""
    o1, o2 = law.run_nndistancegrad(dev(x1), dev(x2), dev(g1), dev(i1), dev(g2), dev(i2))
    n, m = x1.shape[1], x2.shape[1]
    r1 = _check_side(o1, law.nn_grad_law(x1, i1, g1, x2, i2, g2), m, x1, i1, g1, x2, what + " side 1")
    r2 = _check_side(o2, law.nn_grad_law(x2, i2, g2, x1, i1, g1), n, x2, i2, g2, x1, what + " side 2")
    return o1, o2, max(r1, r2)


def _check_chamfer(x1, x2, i1, i2, g, what):
    """hp_chamfer_backward with the scalar g against the law, and bit for bit against hp_nndistancegrad fed the constant."""
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    X1, X2, I1, I2 = dev(x1), dev(x2), dev(i1), dev(i2)
    G = torch.tensor([g], dtype=torch.float32, device="cuda")
    c1, c2 = law.run_chamfer_backward(X1, X2, I1, I2, G)
    g1, g2 = np.full((b, n), g, np.float32), np.full((b, m), g, np.float32)
    _check_side(c1, law.chamfer_backward_law(x1, i1, x2, i2, g), m, x1, i1, g1, x2, what + f" chamfer g={g} side 1")
    _check_side(c2, law.chamfer_backward_law(x2, i2, x1, i1, g), n, x2, i2, g2, x1, what + f" chamfer g={g} side 2")
    p1, p2 = law.run_nndistancegrad(X1, X2, dev(g1), I1, dev(g2), I2)
    assert torch.equal(c1, p1) and torch.equal(c2, p2), (what, g, "scalar and per-point routes differ")
    only1, none2 = law.run_chamfer_backward(X1, X2, I1, I2, G, want2=False)
    none1, only2 = law.run_chamfer_backward(X1, X2, I1, I2, G, want1=False)
    assert none1 is None and none2 is None and torch.equal(only1, c1) and torch.equal(only2, c2), (what, g, "NULL output")


def _synthetic(seed, b, n, m, gscale=1.0):
    """clouds, synthetic in-range indices with every tile seam planted, upstreams of both signs"""
    x1, x2 = law.clouds(seed, b, n, m)
    i1, i2 = law.nn_idx_s(seed + 1, b, n, m), law.nn_idx_s(seed + 2, b, m, n)
    r = np.random.RandomState(seed + 3)
    g1 = (r.uniform(0.5, 1.5, (b, n)) * r.choice([-1, 1], (b, n)) * gscale).astype(np.float32)
    g2 = (r.uniform(0.5, 1.5, (b, m)) * r.choice([-1, 1], (b, m)) * gscale).astype(np.float32)
    return x1, x2, g1, i1, g2, i2


@pytest.mark.parametrize("b,n,m", law.NN_TILE_CASES + law.NN_STRIDE_CASES)
def test_nn_gradient_tile_edges_and_source_stride(b, n, m):
    """Targets on either side of the 2048-target tile (and of its second seam) at 257 sources, and 64 targets at sources on
    either side of the 256-thread stride and of every bits(n) step; idx_s holds 0, j0 - 1, j0 and m - 1 for every tile start.
    Both sides of the call (the kernel runs twice with the roles swapped), both entry points, every element."""
    x1, x2, g1, i1, g2, i2 = _synthetic(1000 + n * 7 + m, b, n, m)
    _check_call(x1, x2, g1, i1, g2, i2, f"tile/stride n={n} m={m}")
    _check_chamfer(x1, x2, i1, i2, 0.05, f"tile/stride n={n} m={m}")


@pytest.mark.parametrize("n,m,j,k", law.NN_WORST_CASES)
def test_nn_gradient_worst_case_accumulation(n, m, j, k):
    """n identical sources all choose target j (the last of tile 0 or the first of tile 1) with terms of one sign and size
    1.9999 * 2^k (x), half and a quarter of it (y, z): the fixed-point sum comes as close to its 61 bits as the rule allows.
    The terms are exact in fp32 and their float64 sum is exact, so the law is the true value."""
    r = np.random.RandomState(n + j + k)
    x = np.float32(1.9999)
    x1 = np.tile(np.array([x, x / 2, -x / 4], np.float32), (1, n, 1))
    x2 = (r.rand(1, m, 3).astype(np.float32) - 0.5)
    x2[0, j] = 0
    g1 = np.full((1, n), 2.0 ** (k - 1), np.float32)
    g2 = (r.uniform(0.5, 1.5, (1, m)) * 2.0 ** (k - 1)).astype(np.float32)
    i1 = np.full((1, n), j, np.int32)
    i2 = r.randint(0, n, (1, m)).astype(np.int32)
    L = law.nn_grad_law(x2, i2, g2, x1, i1, g1)
    assert np.array_equal(L["A"][0, j], n * 2.0 ** k * np.abs(x1[0, 0].astype(np.float64)))     # exact
    _, o2, _ = _check_call(x1, x2, g1, i1, g2, i2, f"worst n={n} j={j} k={k}")
    got, bar = _np64(o2)[0, j], law.nn_grad_bar(L, n)[0, j]
    print(f"worst n={n} j={j} k={k}: kernel {got}, law {L['out'][0, j]}, err/bar {np.abs(got - L['out'][0, j]) / bar}")
    assert np.all(np.abs(got - L["out"][0, j]) <= bar)


@functools.lru_cache(maxsize=None)
def _gridded(scale):
    """clouds of NN_MAGNITUDE_SHAPE on a 1024^3 lattice times `scale`, and their real nearest-neighbour indices: coordinate
    differences are 0 or at least ~scale / 1024, which keeps every term clear of the fp32 denormals at every upstream scale"""
    b, n, m = law.NN_MAGNITUDE_SHAPE
    r = np.random.RandomState(int(np.log10(scale)) + 50)
    x1 = (r.randint(-512, 512, (b, n, 3)) / 1024.0 * scale).astype(np.float32)
    x2 = (r.randint(-512, 512, (b, m, 3)) / 1024.0 * scale).astype(np.float32)
    _, i1, _, i2 = _nn(dev(x1), dev(x2))
    out = (x1, x2, i1.cpu().numpy(), i2.cpu().numpy())
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("scale", law.NN_CLOUD_SCALES)
@pytest.mark.parametrize("gscale", law.NN_UPSTREAM_SCALES)
def test_nn_gradient_magnitudes(gscale, scale):
    """Upstream gradients of 1e-30 ... 1e30 on clouds of 1e-3 ... 1e3, with the real indices of hp_nndistance: the grid step
    follows the data, so the bar — relative throughout — holds at every magnitude."""
    x1, x2, i1, i2 = _gridded(scale)
    b, n, m = law.NN_MAGNITUDE_SHAPE
    r = np.random.RandomState(7)
    g1 = (r.uniform(0.5, 1.5, (b, n)) * r.choice([-1, 1], (b, n)) * gscale).astype(np.float32)
    g2 = (r.uniform(0.5, 1.5, (b, m)) * r.choice([-1, 1], (b, m)) * gscale).astype(np.float32)
    smallest = 2 * 0.5 * gscale * scale / 1024
    assert smallest > 50 * float(np.finfo(np.float32).tiny), smallest
    _check_call(x1, x2, g1, i1, g2, i2, f"magnitudes upstream {gscale:g} cloud {scale:g}")
    if gscale in (1e-30, 0.05, 1e30):
        _check_chamfer(x1, x2, i1, i2, gscale, f"magnitudes cloud {scale:g}")


def test_nn_gradient_mixed_magnitudes_in_one_tile():
    """Target 3 receives 300 terms of size 1, target 7 of the same tile 300 terms of size 1e-9: the grid step follows the
    largest term, so the small target's error is the grid term of the bar, cnt M 2^(bits(n) - 60) — both inside it."""
    b, n, m = 1, 600, 100
    r = np.random.RandomState(11)
    x2 = r.rand(b, m, 3).astype(np.float32) - 0.5
    x1 = np.empty((b, n, 3), np.float32)
    off = (r.uniform(0.5, 1.0, (n, 3)) * r.choice([-1, 1], (n, 3))).astype(np.float32)
    x1[0, :300], x1[0, 300:] = x2[0, 3] + off[:300], x2[0, 7] + off[300:]
    i1 = np.r_[np.full(300, 3), np.full(300, 7)].astype(np.int32)[None]
    g1 = np.r_[np.full(300, 0.5), np.full(300, 0.5e-9)].astype(np.float32)[None]
    i2 = r.randint(0, n, (b, m)).astype(np.int32)
    g2 = np.full((b, m), 1e-9, np.float32)
    _, o2, _ = _check_call(x1, x2, g1, i1, g2, i2, "mixed magnitudes")
    L = law.nn_grad_law(x2, i2, g2, x1, i1, g1)
    bar = law.nn_grad_bar(L, n)
    for j in (3, 7):
        err = np.abs(_np64(o2)[0, j] - L["out"][0, j])
        print(f"mixed magnitudes target {j}: |out| {np.abs(L['out'][0, j])}, err {err}, bar {bar[0, j]}, "
              f"of which grid {(L['cnt'] * L['M'])[0, j] * 2.0 ** (n.bit_length() - 60):.3e}")
        assert np.all(err <= bar[0, j])
    assert L["cnt"][0, 3] == 300 and L["cnt"][0, 7] == 300 and 0.9 < L["M"][0, 0] <= 1.0


def test_nn_gradient_does_not_depend_on_the_order_of_the_sources():
    """Sources permuted (with their idx and upstream; the targets' idx renamed): the targets' gradient is torch.equal, the
    sources' gradient is the permuted one, and three repeated calls are torch.equal — integer accumulation and an
    order-independent maximum."""
    b, n, m = 2, 1000, 2300
    x1, x2, g1, i1, g2, i2 = _synthetic(21, b, n, m)
    i1[:, ::3] = i1[:, :1]                                            # a hot target: a third of the sources on one address
    base = law.run_nndistancegrad(dev(x1), dev(x2), dev(g1), dev(i1), dev(g2), dev(i2))
    for _ in range(2):
        again = law.run_nndistancegrad(dev(x1), dev(x2), dev(g1), dev(i1), dev(g2), dev(i2))
        assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])
    perm = np.random.RandomState(22).permutation(n)
    inv = np.argsort(perm)
    o1, o2 = law.run_nndistancegrad(dev(x1[:, perm]), dev(x2), dev(g1[:, perm]), dev(i1[:, perm]), dev(g2),
                                    dev(inv[i2].astype(np.int32)))
    assert torch.equal(o2, base[1]), int((o2 != base[1]).sum())
    assert torch.equal(o1, base[0][:, torch.from_numpy(perm).cuda()])
    # ... and the other launch: permute the sources of side 1
    perm = np.random.RandomState(23).permutation(m)
    inv = np.argsort(perm)
    o1, o2 = law.run_nndistancegrad(dev(x1), dev(x2[:, perm]), dev(g1), dev(inv[i1].astype(np.int32)), dev(g2[:, perm]),
                                    dev(i2[:, perm]))
    assert torch.equal(o1, base[0]) and torch.equal(o2, base[1][:, torch.from_numpy(perm).cuda()])


@pytest.mark.parametrize("g", [-2.5, 0.0, 0.05, 1.0])
def test_chamfer_backward_scalar_route(g):
    """hp_chamfer_backward on three distinct clouds with the real indices: the law; torch.equal with hp_nndistancegrad fed the
    constant; with either output NULL the other is unchanged bit for bit; upstreams of both signs and 0."""
    x1, x2 = law.clouds(31, 3, 300, 2100)
    _, i1, _, i2 = _nn(dev(x1), dev(x2))
    _check_chamfer(x1, x2, i1.cpu().numpy(), i2.cpu().numpy(), g, "chamfer backward (3, 300, 2100)")


def test_chamfer_loss_module_backward_vs_law():
    """ChamferLoss with (loss * w).backward(): both gradients against the law at upstream w, indices from hp_nndistance (the
    fused forward's own, tests/test_nn_instances_gpu.py)."""
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    x1, x2 = law.clouds(41, 3, 300, 2100)
    w = np.float32(-0.7)
    preds, gts = dev(x1).requires_grad_(True), dev(x2).requires_grad_(True)
    (ChamferLoss()(preds, gts) * float(w)).backward()
    torch.cuda.synchronize()
    _, i1, _, i2 = _nn(dev(x1), dev(x2))
    i1, i2 = i1.cpu().numpy(), i2.cpu().numpy()
    g1, g2 = np.full((3, 300), w, np.float32), np.full((3, 2100), w, np.float32)
    _check_side(preds.grad, law.chamfer_backward_law(x1, i1, x2, i2, w), 2100, x1, i1, g1, x2, "ChamferLoss preds.grad")
    _check_side(gts.grad, law.chamfer_backward_law(x2, i2, x1, i1, w), 300, x2, i2, g2, x1, "ChamferLoss gts.grad")


def test_nn_gradient_non_finite_upstreams_reach_their_targets():
    """A NaN, a +Inf and a -Inf upstream on single sources of either side, a +Inf and a -Inf meeting on one target: the chosen
    targets are non-finite as the reference's float atomicAdd leaves them (the law's NaN or infinity), the sources' own
    elements too, and every other element of the tile stays inside its bar.  Scalar NaN on the Chamfer route: all NaN."""
    b, n, m = 2, 300, 2100
    x1, x2, g1, i1, g2, i2 = _synthetic(51, b, n, m)
    i1[:, 61], x1[:, 61] = i1[:, 60], x1[:, 60]                      # +Inf and -Inf terms, component for component, on one target: NaN
    g1[0, 5], g1[0, 17], g1[0, 40], g1[1, 60], g1[1, 61] = np.nan, np.inf, -np.inf, np.inf, -np.inf
    g2[0, 2050], g2[1, 100], g2[1, 2047] = np.nan, np.inf, -np.inf
    o1, o2, _ = _check_call(x1, x2, g1, i1, g2, i2, "non-finite upstreams")
    o1, o2 = _np64(o1), _np64(o2)
    # stated on the inputs: the target each marked source chose
    assert np.isnan(o2[0, i1[0, 5]]).all() and np.isinf(o2[0, i1[0, 17]]).all() and np.isinf(o2[0, i1[0, 40]]).all()
    assert np.isnan(o2[1, i1[1, 60]]).all()
    assert np.isnan(o1[0, i2[0, 2050]]).all() and np.isinf(o1[1, i2[1, 100]]).all() and np.isinf(o1[1, i2[1, 2047]]).all()
    assert np.isfinite(o2).sum() >= o2.size - 3 * 8 and np.isfinite(o1).sum() >= o1.size - 3 * 8
    nan = torch.tensor([float("nan")], device="cuda")
    c1, c2 = law.run_chamfer_backward(dev(x1), dev(x2), dev(i1), dev(i2), nan)
    assert torch.isnan(c1).all() and torch.isnan(c2).all()


def test_nn_gradient_sums_at_and_beyond_flt_max():
    """1025 sources on target 2048 of 2049 with terms -1.9999 * 2^118 * (1, 1/2, -1/4): the exact sums of x and y exceed
    FLT_MAX and must come out as -Inf, the sum of z (2^127.0007) lies within a factor two of FLT_MAX and must stay inside its
    bar — the rule asks for a grid step of 2^69 here.  And a single term of 1.9 * 2^127 (above 3e38, below FLT_MAX) arrives
    as itself."""
    n, m, j = 1025, 2049, 2048
    r = np.random.RandomState(61)
    x = np.float32(1.9999)
    x1 = np.tile(np.array([x, x / 2, -x / 4], np.float32), (1, n, 1))
    x2 = r.rand(1, m, 3).astype(np.float32) - 0.5
    x2[0, j] = 0
    g1, i1 = np.full((1, n), 2.0 ** 117, np.float32), np.full((1, n), j, np.int32)
    g2, i2 = np.full((1, m), 0.25, np.float32), r.randint(0, n, (1, m)).astype(np.int32)
    L = law.nn_grad_law(x2, i2, g2, x1, i1, g1)
    assert L["out"][0, j, 0] < -law.FLT_MAX and L["out"][0, j, 1] < -law.FLT_MAX and law.FLT_MAX / 2 < L["out"][0, j, 2] < law.FLT_MAX
    _, o2, _ = _check_call(x1, x2, g1, i1, g2, i2, "sum beyond FLT_MAX")
    print("sum beyond FLT_MAX: kernel", _np64(o2)[0, j], "law", L["out"][0, j])
    assert np.array_equal(_np64(o2)[0, j, :2], [-np.inf, -np.inf]) and np.isfinite(_np64(o2)[0, j, 2])

    n, m = 5, 70
    x1 = r.rand(1, n, 3).astype(np.float32) - 0.5
    x2 = r.rand(1, m, 3).astype(np.float32) - 0.5
    x2[0, 9] = 0
    x1[0, 2] = [-1.9, 0.5, 0.25]
    g1, i1 = np.full((1, n), 0.5, np.float32), np.array([[1, 4, 9, 30, 69]], np.int32)
    g1[0, 2] = 2.0 ** 126
    g2, i2 = np.full((1, m), 0.25, np.float32), r.randint(0, n, (1, m)).astype(np.int32)
    L = law.nn_grad_law(x2, i2, g2, x1, i1, g1)
    assert 3.0e38 < L["out"][0, 9, 0] < law.FLT_MAX
    _, o2, _ = _check_call(x1, x2, g1, i1, g2, i2, "one term above 3e38")
    print("one term above 3e38: kernel", _np64(o2)[0, 9], "law", L["out"][0, 9])


# ----------------------------------------------------------------------------------------------------------- match cost
@functools.lru_cache(maxsize=None)
def _match_case(b, n, m):
    """inputs and their laws, computed once per shape and never modified"""
    x1, x2 = law.clouds(b * 7919 + n * 31 + m, b, n, m)
    match = law.synthetic_match(b + n + m, b, n, m)
    cost, S = law.matchcost_law(x1, x2, match)
    g1, g2, A1, A2 = law.matchcostgrad_law(x1, x2, match)
    out = (x1, x2, match, cost, S, g1, g2, A1, A2)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("b,n,m", law.MATCH_CASES)
def test_matchcost_and_gradients_vs_law(b, n, m):
    """hp_matchcost_ws, hp_matchcost and hp_matchcostgrad on a synthetic match at (b, n, m): each cost against the law within
    k u sum|match d| (k: loss_gradient_law.k_matchcost_ws / k_matchcost_cloud), the two against each other within the sum of
    their bars; both gradients within ((k + 1) u + RSQ_BAR) sum|terms| (matchcostgrad_bars); repeated calls torch.equal."""
    x1, x2, match, cost, S, g1, g2, A1, A2 = _match_case(b, n, m)
    X1, X2, Mt = dev(x1), dev(x2), dev(match)
    ws, cl = law.run_matchcost(X1, X2, Mt, True), law.run_matchcost(X1, X2, Mt, False)
    bar_ws, bar_cl = law.k_matchcost_ws() * law.U * S, law.k_matchcost_cloud(m) * law.U * S
    e_ws, e_cl, e_x = np.abs(_np64(ws) - cost), np.abs(_np64(cl) - cost), np.abs(_np64(ws) - _np64(cl))
    print(f"PARITY matchcost ({b}, {n}, {m}): ws err/bar {np.max(e_ws / np.maximum(bar_ws, 1e-300)):.4f}, cloud err/bar "
          f"{np.max(e_cl / np.maximum(bar_cl, 1e-300)):.4f}; relative errors {np.max(e_ws / np.maximum(S, 1e-300)):.3e} "
          f"{np.max(e_cl / np.maximum(S, 1e-300)):.3e}")
    assert np.all(e_ws <= bar_ws) and np.all(e_cl <= bar_cl) and np.all(e_x <= bar_ws + bar_cl)
    o1, o2 = law.run_matchcostgrad(X1, X2, Mt)
    bar1, bar2 = law.matchcostgrad_bars(A1, A2, n, m)
    e1, e2 = np.abs(_np64(o1) - g1), np.abs(_np64(o2) - g2)
    print(f"PARITY matchcostgrad ({b}, {n}, {m}): grad1 err/bar {np.max(e1 / np.maximum(bar1, 1e-300)):.4f}, grad2 err/bar "
          f"{np.max(e2 / np.maximum(bar2, 1e-300)):.4f}")
    assert np.all(e1 <= bar1) and np.all(e2 <= bar2)
    assert torch.equal(law.run_matchcost(X1, X2, Mt, True), ws) and torch.equal(law.run_matchcost(X1, X2, Mt, False), cl)
    p1, p2 = law.run_matchcostgrad(X1, X2, Mt)
    assert torch.equal(p1, o1) and torch.equal(p2, o2)


def test_rsq_probe_through_matchcostgrad():
    """The hardware reciprocal square root, measured through the kernel itself: m = 1, match = 1, q = 0 and p_j = (a_j, 1, 0),
    so grad1[j].y = fl(1 * rsq(arg_j)) * 1 + 0 = rsq(arg_j) with arg_j = fl(1 + fl(a_j^2)) known exactly; 4096 distinct
    arguments over [1, 4), both binades of the mantissa.  The figure is recorded in profiles/loss_gradients_parity.md and
    the bars use RSQ_BAR = twice that record; here the live figure is printed and must not exceed RSQ_BAR."""
    n = 4096
    a = (np.sqrt(3.0) * (np.arange(n) + 0.37) / n).astype(np.float32)
    x1 = np.stack([a, np.ones(n, np.float32), np.zeros(n, np.float32)], -1)[None]
    x2 = np.zeros((1, 1, 3), np.float32)
    arg = ((a * a).astype(np.float64) + 1.0).astype(np.float32)       # the fma rounds 1 + fl(a^2) once
    assert len(np.unique(arg)) > 4000 and arg.min() >= 1 and arg.max() < 4
    o1, _ = law.run_matchcostgrad(dev(x1), dev(x2), dev(np.ones((1, 1, n), np.float32)))
    got = _np64(o1)[0, :, 1]
    rel = np.abs(got * np.sqrt(arg.astype(np.float64)) - 1.0)
    print(f"PARITY rsq: max relative error {rel.max():.4e} = {rel.max() / law.U:.3f} u at arg {arg[np.argmax(rel)]!r}; "
          f"RSQ_MEASURED {law.RSQ_MEASURED:.4e}, RSQ_BAR {law.RSQ_BAR:.4e}")
    assert rel.max() <= law.RSQ_BAR


@pytest.mark.parametrize("k,l", law.ONE_HOT_AT)
def test_matchcostgrad_one_hot_match(k, l):
    """A single 1 at (row k, column l) in each of the three clouds: grad1[l] is the unit vector from q_k to p_l, grad2[k] its
    negative, every other element exactly 0."""
    b, n, m = law.ONE_HOT_SHAPE
    x1, x2 = law.clouds(71, b, n, m)
    match = torch.zeros((b, m, n), device="cuda")
    match[:, k, l] = 1
    o1, o2 = law.run_matchcostgrad(dev(x1), dev(x2), match)
    e = x1[:, l].astype(np.float64) - x2[:, k].astype(np.float64)
    unit = e / np.sqrt((e ** 2).sum(-1, keepdims=True))
    bar = ((law.k_grad_term() + 2) * law.U + law.RSQ_BAR) * np.abs(unit)
    e1, e2 = np.abs(_np64(o1)[:, l] - unit), np.abs(_np64(o2)[:, k] + unit)
    print(f"PARITY one-hot ({k}, {l}): grad1 err/bar {np.max(e1 / bar):.4f}, grad2 err/bar {np.max(e2 / bar):.4f}")
    assert np.all(e1 <= bar) and np.all(e2 <= bar)
    o1[:, l], o2[:, k] = 0, 0
    assert not o1.any() and not o2.any()


def test_matchcostgrad_clamp_and_zero_match():
    """approxmatch.cu's e / max(|e|, 1e-10): a coincident pair contributes exactly 0 (to both gradients and to the cost), a
    pair 1e-12 apart next to the origin follows the clamped law, match * e / 1e-10.  match = 0: exact zeros everywhere."""
    x1 = np.array([[[0.25, -0.5, 0.125], [1e-12, 0, 0], [0.3, 0.2, 0.1]]], np.float32)
    x2 = np.array([[[0.25, -0.5, 0.125], [0, 0, 0]]], np.float32)
    match = np.zeros((1, 2, 3), np.float32)
    match[0, 0, 0], match[0, 1, 1] = 3.0, 0.75
    o1, o2 = law.run_matchcostgrad(dev(x1), dev(x2), dev(match))
    g1, g2, A1, A2 = law.matchcostgrad_law(x1, x2, match)
    bar1, bar2 = law.matchcostgrad_bars(A1, A2, 3, 2)
    print("clamp: grad1", _np64(o1)[0].tolist(), "law", g1[0].tolist(), "grad2", _np64(o2)[0].tolist())
    assert not o1[0, 0].any() and not o2[0, 0].any() and not o1[0, 2].any()
    assert abs(g1[0, 1, 0] - 0.75 * float(np.float32(1e-12)) / 1e-10) < 1e-12
    assert np.all(np.abs(_np64(o1) - g1) <= bar1) and np.all(np.abs(_np64(o2) - g2) <= bar2)
    for ws in (True, False):
        c = _np64(law.run_matchcost(dev(x1), dev(x2), dev(match), ws))[0]
        want = 0.75 * float(np.float32(1e-12))
        print(f"clamp: cost ws={ws} {c!r} law {want!r}")
        assert abs(c - want) <= (law.K_DIST + 3) * law.U * want       # the distance, one fma, the conversion of the sum, + 1
    b, n, m = 3, 257, 65
    x1, x2 = law.clouds(81, b, n, m)
    zero = torch.zeros((b, m, n), device="cuda")
    o1, o2 = law.run_matchcostgrad(dev(x1), dev(x2), zero)
    assert not o1.any() and not o2.any()
    assert not law.run_matchcost(dev(x1), dev(x2), zero, True).any() and not law.run_matchcost(dev(x1), dev(x2), zero, False).any()


def test_matchcostgrad_validates_its_arguments():
    """b = 65536 exceeds the grid's y dimension and a NULL pointer cannot be launched on: -1 like hp_matchcost_ws and
    hp_nndistancegrad, outputs untouched."""
    import ctypes
    from hyperpocket_amd._lib import current_stream, load_library, ptr
    fn = load_library().hp_matchcostgrad
    b = 65536
    x1, x2 = torch.zeros((b, 1, 3), device="cuda"), torch.ones((b, 1, 3), device="cuda")
    match = torch.ones((b, 1, 1), device="cuda")
    o1, o2 = torch.full((b, 1, 3), -7.0, device="cuda"), torch.full((b, 1, 3), -7.0, device="cuda")
    st = current_stream(x1.device)
    i = ctypes.c_int
    assert fn(i(b), i(1), i(1), ptr(x1), ptr(x2), ptr(match), ptr(o1), ptr(o2), st) == -1
    for drop in range(5):
        args = [ptr(None) if k == drop else ptr(t) for k, t in enumerate((x1, x2, match, o1, o2))]
        assert fn(i(3), i(1), i(1), *args, st) == -1, drop
    torch.cuda.synchronize()
    assert bool((o1 == -7.0).all()) and bool((o2 == -7.0).all())
    assert fn(i(3), i(1), i(1), ptr(x1), ptr(x2), ptr(match), ptr(o1), ptr(o2), st) == 0
    torch.cuda.synchronize()
    assert bool((o1[:3] != -7.0).all()) and bool((o1[3:] == -7.0).all())

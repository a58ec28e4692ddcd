"""CPU suite for tests/aux_law.py: the laws are the reference's laws (the sampler's distribution and push-out rule, the slicer
against oracle/slicer_ref.py fed the law's own planes, the KLD and loss scalars against plain float64), and the case tables
that tests/test_aux_kernels_gpu.py runs would notice a wrong kernel: they reach the attempt depth, the pushed and unpushed
points, the late candidates, the same-round second acceptors, the ties of sides and the loop boundaries that each of the
mutations below needs in order to show."""
import functools

import numpy as np
import pytest
import torch

import aux_law as law
from oracle.slicer_ref import slice_with_planes

F32 = np.float32
POINTS = 200000


@functools.lru_cache(maxsize=None)
def sample(coef, seed=7, offset=1):
    return law.sampler_law(POINTS, coef, seed, offset, return_attempts=True)


@functools.lru_cache(maxsize=None)
def sliced(N, target, seed):
    return law.slice_law(law.slice_clouds_of(N, target), target, seed, law.SLICE_LIMIT // law.WAVES)


def every_slice_case():
    return [(N, target, seed) for seed in law.SLICE_SEEDS for N, target in law.SLICE_CASES]


# ---------------------------------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------------------------------
def test_sampler_law_is_uniform_in_the_ball():
    p, _ = sample(0.0)
    assert p.dtype == F32 and p.shape == (POINTS, 3)
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    assert (r < 1).all()
    for t in (0.3, 0.5, 0.8):
        q = t ** 3
        assert abs((r < t).mean() - q) <= 4 * np.sqrt(q * (1 - q) / POINTS), t
    # a coordinate of a uniform ball point has variance 1/5
    assert np.abs(p.astype(np.float64).mean(0)).max() <= 4 * np.sqrt(0.2 / POINTS)
    # every coordinate is an integer multiple of 2^-23
    assert np.array_equal(p.astype(np.float64) * 2.0 ** 23, np.round(p.astype(np.float64) * 2.0 ** 23))


@pytest.mark.parametrize("coef", [c for c in law.SAMPLER_COEFS if 0 < c < 1])
def test_sampler_law_pushes_as_the_reference_does(coef):
    """utils/points.py:24-33: rows with |p| < c become c * (p / |p|), the norms through numpy on the fp32 values, the
    division and the product in fp32 (torch).  The law scales by fl(c / |p|) instead: two roundings each way, on norms that
    are themselves rounded differently.  "Within 2 ulp" is taken at the point's scale — every coordinate within 2 ulp32(c)
    of the reference's, c being the pushed point's radius.  (Measured per coordinate at its own scale the two differ by up to
    3 ulp, in 50 of 28 671 coordinates at c = 36/99, all of them small beside c; each formula is then up to 2.8 ulp from the
    float64 value itself.)"""
    raw, _ = sample(0.0)
    got, _ = sample(coef)
    moved = (got != raw).any(1)
    q = coef ** 3
    assert abs(moved.mean() - q) <= 4 * np.sqrt(q * (1 - q) / POINTS)
    assert moved.any() and not moved.all()
    rows = torch.from_numpy(raw[moved])
    radius = torch.from_numpy(np.linalg.norm(raw[moved], axis=1)).float()
    want = (coef * (rows.T / radius).T).numpy()
    assert want.dtype == F32
    assert (np.abs(got[moved].astype(np.float64) - want) <= 2 * float(np.spacing(F32(coef)))).all()
    # the reference pushes exactly the rows whose numpy norm is below c; the law's set may differ from it only where the
    # two fp32 norms straddle c
    ref_moved = np.linalg.norm(raw, axis=1) < coef
    differ = moved != ref_moved
    exact = np.linalg.norm(raw.astype(np.float64), axis=1)
    assert (np.abs(exact[differ] - coef) <= 2 * np.spacing(F32(coef))).all()
    # unpushed rows are the raw draw, bit for bit, and lie at or beyond c
    assert np.array_equal(got[~moved], raw[~moved]) and (exact[~moved] >= coef * (1 - 2.0 ** -23)).all()


def test_sampler_law_at_coef_one_puts_every_point_on_the_sphere():
    got, _ = sample(1.0)
    r = np.linalg.norm(got.astype(np.float64), axis=1)
    assert (np.abs(r - 1) <= 2 * 2.0 ** -23).all()                 # within 2 ulp of 1
    # "|p| < 1" does not hold after the push-out, in the law as in the reference: about two thirds of the fp32 norms
    # (numpy's, which the reference takes, and the plain fp32 expression) come out >= 1, none beyond the next float
    for n32 in (np.linalg.norm(got, axis=1), np.sqrt((got[:, 0] * got[:, 0] + got[:, 1] * got[:, 1]) + got[:, 2] * got[:, 2])):
        assert n32.dtype == F32 and (n32 <= F32(1 + 2.0 ** -23)).all()
        assert 0.5 <= (n32 >= 1).mean() <= 0.8


def test_sampler_case_table_reaches_deep_attempts_and_both_kinds_of_point():
    deepest = 0
    for seed, offset in law.SAMPLER_SEEDS:
        raw, attempts = law.sampler_law(max(law.SAMPLER_TOTALS), 0.0, seed, offset, return_attempts=True)
        assert attempts.max() < law.ATTEMPTS                      # no feasible draw exhausts its attempts
        deepest = max(deepest, int(attempts.max()))
        for coef in law.SAMPLER_COEFS:
            if 0 < coef < 1:
                moved = (law.sampler_law(max(law.SAMPLER_TOTALS), coef, seed, offset) != raw).any(1)
                assert moved.any() and not moved.all(), (seed, offset, coef)
    assert deepest + 1 >= 12, deepest


def test_sampler_branches_no_feasible_draw_reaches():
    z = np.zeros((1, 3), F32)
    assert np.array_equal(law.push_out(z, np.zeros(1, F32), 0.37), np.array([[F32(0.37), 0, 0]], F32))
    assert np.array_equal(law.push_out(z, np.zeros(1, F32), 0.0), z)
    assert np.array_equal(law.exhausted_point(0.5), np.array([0.5, 0, 0], F32))
    assert np.array_equal(law.exhausted_point(0.0), np.zeros(3, F32))
    # a point exactly at radius coef is not moved: the rule is a strict <
    p = np.array([[0.5, 0, 0]], F32)
    assert np.array_equal(law.push_out(p, np.array([0.25], F32), 0.5), p)


def test_sampler_mutations_show_on_the_case_table():
    total = 257
    high_seed = high_offset = 0
    for seed, offset in law.SAMPLER_SEEDS:
        want = law.sampler_law(total, 0.37, seed, offset)
        if seed >> 32:
            high_seed += 1
            assert not np.array_equal(law.sampler_law(total, 0.37, seed & 0xFFFFFFFF, offset), want), (seed, offset)
        if offset >> 32:
            high_offset += 1
            assert not np.array_equal(law.sampler_law(total, 0.37, seed, offset & 0xFFFFFFFF), want), (seed, offset)
    assert high_seed >= 2 and high_offset >= 2

    # an attempt mixed into the counter where it collides with the point index: attempt a of point i would be attempt 0
    # of point i ^ (a << 8), so two points 256 apart share draws.  The law keeps them apart:
    i = np.arange(1024, dtype=np.uint64)
    first = law.sampler_attempt(i, 0, 7, 1)[0]
    second = law.sampler_attempt(i, 1, 7, 1)[0]
    assert not np.array_equal(second, law.sampler_attempt(i ^ np.uint64(256), 0, 7, 1)[0])
    assert not (first == second).all(1).any()


# ---------------------------------------------------------------------------------------------------------------------
# slicer
# ---------------------------------------------------------------------------------------------------------------------
def test_slice_law_is_the_reference_split_with_its_own_planes():
    """oracle/slicer_ref.slice_with_planes (pinned by the reference's fixture) classifies in float64; the law in fp32.  Fed
    the law's candidates 0..accepted as float64 it must accept the same candidate and return the same parts, unless a point
    lies within fp32 rounding of a counted plane — no shipped case does (a case that did would be drawn again)."""
    left_out = 0
    for N, target, seed in every_slice_case():
        pts = law.slice_clouds_of(N, target)
        part_a, part_b, plane, status, index = sliced(N, target, seed)
        assert (status == 0).all() and (index >= 0).all() and index.max() < law.SLICE_LIMIT, (N, target, seed, index)
        for b in range(law.SLICE_CLOUDS):
            planes = law.slice_candidates(b, seed, 0, int(index[b]) + 1).astype(np.float64)
            assert np.array_equal(planes[-1].astype(F32), plane[b])
            a, rest, idx = slice_with_planes(pts[b], planes, target)
            same = idx == index[b] and np.array_equal(a, part_a[b]) and np.array_equal(rest, part_b[b])
            left_out += not same
    assert left_out == 0


def test_slice_law_parts_are_a_partition_in_point_order():
    for N, target, seed in every_slice_case():
        pts = law.slice_clouds_of(N, target)
        part_a, part_b, plane, _, _ = sliced(N, target, seed)
        for b in range(law.SLICE_CLOUDS):
            assert part_a[b].shape == (target, 3) and part_b[b].shape == (N - target, 3)
            m = law.under_mask(pts[b], plane[b])
            if not (m.sum() == target and np.array_equal(pts[b][m], part_a[b])):
                m = ~m
            assert np.array_equal(pts[b][m], part_a[b]) and np.array_equal(pts[b][~m], part_b[b])


def test_slice_case_table_has_what_the_mutations_need():
    second_acceptor, ties, a_under, a_other, latest = [], 0, 0, 0, 0
    for N, target, seed in every_slice_case():
        pts = law.slice_clouds_of(N, target)
        part_a, _, plane, _, index = sliced(N, target, seed)
        latest = max(latest, int(index.max()))
        for b in range(law.SLICE_CLOUDS):
            c = int(index[b])
            rest_of_round = np.arange(c + 1, (c // law.WAVES + 1) * law.WAVES)
            if rest_of_round.size:
                cnt = law.under_counts(pts[b], law.slice_candidates(b, seed, c + 1, rest_of_round.size))
                if ((cnt == target) | (N - cnt == target)).any():
                    second_acceptor.append((N, target))
            under = int(law.under_mask(pts[b], plane[b]).sum())
            if N == 2 * target and under == target:
                ties += 1
            if under == target:
                a_under += 1
            else:
                a_other += 1
    assert (2, 1) in second_acceptor and len(set(second_acceptor)) >= 2
    assert ties > 0 and a_under > 0 and a_other > 0
    assert latest >= 10000                      # late candidates: a round counter cut to 8 or 12 bits would show


def test_slice_mutations_show_on_the_case_table():
    shown = {"any": 0, "other": 0, "swapped": 0, "seed": 0}
    for N, target, seed in every_slice_case():
        pts = law.slice_clouds_of(N, target)
        want = sliced(N, target, seed)
        rounds = law.SLICE_LIMIT // law.WAVES

        def differs(got):
            return not all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want))

        if N <= 333:                             # (the small cases already show each of them; the large ones cost seconds)
            shown["any"] += differs(law.slice_law(pts, target, seed, rounds, rule="any"))
            shown["other"] += differs(law.slice_law(pts, target, seed, rounds, prefer="other"))
            shown["swapped"] += differs(law.slice_law(pts, target, seed, rounds, order=("round", "cloud")))
            if seed >> 32:
                shown["seed"] += differs(law.slice_law(pts, target, seed & 0xFFFFFFFF, rounds))
    assert all(n > 0 for n in shown.values()), shown


def test_slice_law_reports_a_failed_cloud_alone():
    for seed in law.SLICE_SEEDS:
        for N, target in law.STATUS_CASES:
            pts = law.slice_clouds_of(N, target)
            want = sliced(N, target, seed)
            index = want[4]
            slow = int(np.argmax(index))
            rounds = int(index[slow]) // law.WAVES + 1
            assert rounds >= 2 and sorted(index // law.WAVES)[-2] < rounds - 1     # one cloud alone needs the last round
            assert all(np.array_equal(g, w) for g, w in zip(law.slice_law(pts, target, seed, rounds), want))
            part_a, part_b, plane, status, idx = law.slice_law(pts, target, seed, rounds - 1)
            assert status.tolist() == [int(b == slow) for b in range(law.SLICE_CLOUDS)] and idx[slow] == -1
            assert np.isnan(part_a[slow]).all() and np.isnan(part_b[slow]).all() and np.isnan(plane[slow]).all()
            for b in range(law.SLICE_CLOUDS):
                if b != slow:
                    assert np.array_equal(part_a[b], want[0][b]) and np.array_equal(plane[b], want[2][b])


def test_the_ball_clouds_split_within_the_wrapper_default():
    ball = law.ball_clouds()
    assert ball.shape == (law.SLICE_CLOUDS,) + law.BALL_CASE[:1] + (3,) and np.abs(ball.astype(np.float64).mean(1)).max() < 0.05
    assert (np.linalg.norm(ball.astype(np.float64), axis=2) < 0.5).all()
    for seed in law.SLICE_SEEDS:
        assert (law.slice_law(ball, law.BALL_CASE[1], seed, 100000)[3] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# KLD
# ---------------------------------------------------------------------------------------------------------------------
def boundaries(n):
    """Elements at which a 1024-wide, 4-deep loop nest could lose or repeat one: the ends and the multiples of 1024."""
    at = {0, n - 1}
    for edge in range(1024, n + 1, 1024):
        at |= {edge - 1, edge} if edge < n else {edge - 1}
    return sorted(i for i in at if 0 <= i < n)


def test_kld_f64_is_the_reference_expression():
    rs = np.random.RandomState(0)
    v, mu = torch.from_numpy(rs.rand(5, 7) * 0.5).requires_grad_(True), torch.from_numpy(rs.randn(5, 7)).requires_grad_(True)
    ref = 0.5 * (torch.exp(v) + torch.square(mu) - 1 - v).sum() / 5              # core/epoch_loops.py:29-30
    (ref * 3).backward()
    value, gv, gm = law.kld_f64(v.detach().numpy(), mu.detach().numpy(), 5, g=3.0)
    assert abs(value - ref.item()) <= 1e-15 * abs(ref.item())
    assert np.allclose(gv, v.grad.numpy(), rtol=1e-14, atol=0) and np.allclose(gm, mu.grad.numpy(), rtol=1e-14, atol=0)


def test_kld_exact_form_is_exact_and_notices_one_element():
    for n in law.KLD_N:
        mu = law.kld_exact_mu(n)
        k = np.abs(mu.astype(np.float64)) * 64
        assert np.array_equal(k, np.round(k)) and k.min() >= 1 and k.max() <= 1021 and (n == 1 or len(set(k.tolist())) > 1)
        assert np.array_equal(law.kld_exact_terms(mu), mu.astype(np.float64) ** 2)       # every fp32 term is exact
        for batch in law.KLD_BATCH:
            want = law.kld_exact_v0(mu, batch)
            f64 = law.kld_f64(np.zeros(n), mu, batch)[0]
            assert abs(float(want) - f64) <= 2 * law.U * f64                               # fl32(1/B) and the final rounding
            for i in boundaries(n):
                assert law.kld_exact_v0(mu, batch, twice=i) != want, (n, batch, i)
                if n > 1:
                    assert law.kld_exact_v0(mu, batch, skip=i) != want, (n, batch, i)
            if n > 1:
                assert law.kld_exact_v0(mu, batch, skip=0, twice=n - 1) != want            # one swapped for another


def test_kld_bound_holds_for_the_reference_fp32_evaluation_and_is_not_slack():
    """torch's fp32 evaluation on the CPU (its expf is within 1 ulp) must pass the bound; the bound itself stays within a
    small multiple of fp32's resolution of the terms, so a dropped element (1/n of the value and more) fails it."""
    for regime in law.KLD_REGIMES:
        for n in (257, 4097, 12289):
            v, mu = law.kld_inputs(n, 64, regime)
            value = law.kld_f64(v, mu, 64)[0]
            bound = law.kld_bound(v, mu, 64)
            tv, tm = torch.from_numpy(v), torch.from_numpy(mu)
            terms = (torch.exp(tv) + tm * tm - 1 - tv).double()
            got = float(np.float32(0.5 * terms.sum().item() * float(F32(1) / F32(64))))
            assert abs(got - value) <= bound, (regime, n)
            scale = 0.5 / 64 * float(np.sum(np.exp(v.astype(np.float64)) + mu.astype(np.float64) ** 2 + 1 + np.abs(v)))
            assert bound <= 11 * law.U * scale, (regime, n)
    v, mu = law.kld_inputs(8192, 64, "workload")
    terms = np.exp(v.astype(np.float64)) + mu.astype(np.float64) ** 2 - 1 - v
    assert np.median(terms) * 0.5 / 64 > 20 * law.kld_bound(v, mu, 64)          # a typical element is far above the bar


def test_kld_gradient_laws():
    v, mu = law.kld_inputs(1025, 3, "workload")
    for g in law.KLD_G:
        _, gv, gm = law.kld_f64(v, mu, 3, g)
        got = law.kld_grad_mu_law(mu, 3, g)
        assert got.dtype == F32 and np.all(np.abs(got - gm) <= 3 * law.U * np.abs(gm))
        tv = torch.from_numpy(v)
        scale = torch.tensor(g, dtype=torch.float32) * (torch.tensor(1.0) / torch.tensor(3.0))
        fp32 = (0.5 * scale * (torch.exp(tv) - 1)).numpy()
        assert np.all(np.abs(fp32 - gv) <= law.kld_grad_v_bound(v, 3, g))


# ---------------------------------------------------------------------------------------------------------------------
# step losses
# ---------------------------------------------------------------------------------------------------------------------
def test_step_losses_law_and_its_summation_order():
    for b in law.STEP_B:
        cd, kld, cost = law.step_inputs(b)
        for with_kld in (True, False):
            for with_cost in (True, False):
                out = law.step_losses_law(cd, kld if with_kld else None, cost if with_cost else None, law.STEP_C_CD, law.STEP_C_EMD)
                assert out.dtype == F32 and out.shape == (4,)
                e = float(np.sum(cost.astype(np.float64))) if with_cost else 0.0
                want = [law.STEP_C_CD * float(cd), float(kld) if with_kld else 0.0, law.STEP_C_EMD * e]
                want.append(sum(want))
                assert np.all(np.abs(out - np.array(want)) <= (b + 4) * law.U * np.abs(want))
                assert out[1] == (kld if with_kld else 0) and (with_cost or out[2] == 0)
        if b >= 9:
            assert not np.array_equal(law.step_losses_law(cd, kld, cost, law.STEP_C_CD, law.STEP_C_EMD, pairwise=True),
                                      law.step_losses_law(cd, kld, cost, law.STEP_C_CD, law.STEP_C_EMD)), b


# ---------------------------------------------------------------------------------------------------------------------
# ops.slice_clouds on an empty batch (no library call: nothing to launch, nothing to reduce)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_planes", [False, True])
def test_slice_clouds_serves_an_empty_batch_on_the_host(with_planes):
    from hyperpocket_amd import ops
    real = ops.check_input, ops.call, ops.current_stream
    calls = []
    ops.check_input, ops.call, ops.current_stream = (lambda t, name, dtype=torch.float32: None), (lambda *a: calls.append(a)), \
        (lambda device=None: None)
    try:
        planes = torch.zeros((0, 5, 4), dtype=torch.float64) if with_planes else None
        a, b, plane = ops.slice_clouds(torch.zeros((0, 10, 3)), 4, seed=3, planes=planes)
    finally:
        ops.check_input, ops.call, ops.current_stream = real
    assert calls == []
    assert a.shape == (0, 4, 3) and b.shape == (0, 6, 3) and a.dtype == b.dtype == torch.float32
    assert (plane.shape, plane.dtype) == (((0,), torch.int32) if with_planes else ((0, 4), torch.float32))

"""GPU suite for the exact EMD: hp_assign_pairs (csrc/assign.hip) against the law (tests/assign_law.py) bit for bit —
assignment, cost and rounds — at the wave and slice edges, on tie-heavy and identical clouds, at n = 1024 and 2048; pair
lists longer than the grid; bad, capped and overflowing pairs; emd_exact_pairs / emd_exact_loss; the `emd` keyword of the
metrics; another stream.

Bars.  Kernel against law: torch.equal, the law is the specification.  Cost against scipy on the law's q: equal integers.
emd_exact_loss against the kernel's cost: see test_loss_value_and_gradient.  pairwise_EMD_CD(emd="exact") against scipy:
one fp32 rounding (the final cast)."""
import ctypes

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from assign_law import FAMILIES, assign_pairs_law, family_pair, quantised_costs

pytestmark = pytest.mark.gpu


def _c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_kernel(A, B, pairs, scale_log2=20, max_rounds=0, want_assignment=True):
    """hp_assign_pairs as it is: -> (assignment (P,n) int32 or None, cost (P,) int64, rounds (P,) int32) on the device."""
    from hyperpocket_amd._lib import call, current_stream
    pairs = torch.as_tensor(np.asarray(pairs, dtype=np.int32)).reshape(-1, 2).cuda().contiguous()
    P, n = pairs.size(0), A.size(1)
    asg = torch.full((P, n), -7, dtype=torch.int32, device="cuda") if want_assignment else None
    cost = torch.full((P,), -7, dtype=torch.int64, device="cuda")
    rounds = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    call("hp_assign_pairs", A.size(0), n, A, B.size(0), B, ctypes.c_long(P), pairs, scale_log2, ctypes.c_long(max_rounds), asg,
         cost, rounds, current_stream(A.device))
    return asg, cost, rounds


def assert_equals_law(A, B, pairs, **kw):
    """A, B numpy sets: the kernel's three outputs are the law's."""
    asg, cost, rounds = run_kernel(_c(A), _c(B), pairs, **kw)
    l_asg, l_cost, l_rounds = assign_pairs_law(A, B, pairs, kw.get("scale_log2", 20), kw.get("max_rounds") or None)
    assert torch.equal(rounds.cpu(), torch.from_numpy(l_rounds))
    assert torch.equal(cost.cpu(), torch.from_numpy(l_cost))
    assert torch.equal(asg.cpu(), torch.from_numpy(l_asg))
    return l_asg, l_cost, l_rounds


def family_sets(n, families=FAMILIES, seed=0):
    """One (a, b) per family stacked into two sets; pair (k, k) is family k's."""
    ab = [family_pair(f, n, seed) for f in families]
    return np.stack([a for a, _ in ab]), np.stack([b for _, b in ab])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 200, 256])
def test_kernel_equals_law_at_the_wave_and_slice_edges(n):
    """Every family (tie-heavy grid and identical clouds among them) on the diagonal, two mixed pairs next to it."""
    A, B = family_sets(n)
    pairs = [(k, k) for k in range(len(FAMILIES))] + [(0, 1), (3, 2)]
    _, cost, rounds = assert_equals_law(A, B, pairs)
    assert (rounds > 0).all()
    assert cost[FAMILIES.index("identical")] == 0


def test_kernel_equals_law_at_1024():
    A, B = family_sets(1024, ("uniform", "clustered", "identical"))
    assert_equals_law(A, B, [(0, 0), (1, 1), (2, 2)])


def test_kernel_equals_law_and_scipy_at_2048():
    A, B = family_sets(2048, ("uniform", "identical"))
    _, cost, _ = assert_equals_law(A, B, [(0, 0), (1, 1)])
    q, overflow = quantised_costs(A[0], B[0])
    assert not overflow
    rows, cols = linear_sum_assignment(q)
    assert int(cost[0]) == int(q[rows, cols].sum())
    assert int(cost[1]) == 0


@pytest.mark.parametrize("count,n,repeat", [(30, 16, 1), (8, 8, 40)])
def test_many_small_pairs_and_the_reversed_list(count, n, repeat):
    """900 pairs (the whole 30 x 30 set at n = 16) and 2560 pairs (the 8 x 8 set at n = 8, forty times over: more than the
    2048 workgroups a launch has at the most, so workgroups take several pairs): every pair is the law's, and the reversed
    list gives the reversed outputs."""
    rng = np.random.default_rng(count)
    A = rng.uniform(-0.5, 0.5, (count, n, 3)).astype(np.float32)
    B = rng.uniform(-0.5, 0.5, (count, n, 3)).astype(np.float32)
    B[3] = A[5][rng.permutation(n)]
    pairs = np.array([(i, j) for i in range(count) for j in range(count)] * repeat)
    pairs = pairs[rng.permutation(len(pairs))]
    assert_equals_law(A, B, pairs)
    asg, cost, rounds = run_kernel(_c(A), _c(B), pairs)
    r_asg, r_cost, r_rounds = run_kernel(_c(A), _c(B), pairs[::-1].copy())
    assert torch.equal(r_asg, asg.flip(0)) and torch.equal(r_cost, cost.flip(0)) and torch.equal(r_rounds, rounds.flip(0))


def test_out_of_range_pairs_are_flagged_and_their_neighbours_untouched():
    A, B = family_sets(64, ("uniform", "clustered", "grid"))
    na = len(A)
    pairs = [(0, 0), (-1, 0), (1, 1), (na, 1), (2, 2), (0, 2 ** 31 - 1), (2, -1), (2, 1)]
    asg, cost, rounds = assert_equals_law(A, B, pairs)
    bad = np.array([1, 3, 5, 6])
    assert (rounds[bad] == -2).all() and (cost[bad] == -1).all() and (asg[bad] == -1).all()
    good = np.array([0, 2, 4, 7])
    assert (rounds[good] > 0).all()
    from hyperpocket_amd.utils.evaluation.emd_exact import emd_exact_pairs
    out = emd_exact_pairs(_c(A), _c(B), torch.tensor(pairs, dtype=torch.int64))         # NaN, no exception
    assert torch.equal(out.isnan().cpu(), torch.from_numpy(rounds < 0))
    assert torch.equal(out[good].cpu(), torch.from_numpy(cost[good] / 2.0 ** 20))


def test_a_capped_call_stops_and_the_next_call_is_correct():
    """max_rounds = 3 at n = 64: the bounded exit, then an ordinary call on the same stream."""
    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.utils.evaluation.emd_exact import emd_exact_pairs
    A, B = family_sets(64, ("uniform", "clustered"))
    pairs = [(0, 0), (1, 1), (0, 1)]
    asg, cost, rounds = assert_equals_law(A, B, pairs, max_rounds=3)
    assert (rounds == -1).all() and (cost == -1).all() and (asg == -1).all()
    assert_equals_law(A, B, pairs)
    with pytest.raises(HipExtensionError, match="3 of 3 pairs exhausted"):
        emd_exact_pairs(_c(A), _c(B), pairs, max_rounds=3)
    _, _, rounds = assign_pairs_law(A, B, [(0, 0)])
    exactly = int(rounds[0])
    assert_equals_law(A, B, [(0, 0)], max_rounds=exactly)
    assert (assert_equals_law(A, B, [(0, 0)], max_rounds=exactly - 1)[2] == -1).all()


def test_overflowing_distances_are_flagged():
    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.utils.evaluation.emd_exact import emd_exact_pairs
    A = np.zeros((2, 8, 3), np.float32)
    B = np.zeros((2, 8, 3), np.float32)
    B[1] = 4096.0
    B[0, :, 0] = np.arange(8) * 8.0                          # 56 * 2^24 < 2^30: fine
    _, cost, rounds = assert_equals_law(A, B, [(0, 0), (0, 1), (1, 0)], scale_log2=24)
    assert rounds[1] == -3 and cost[1] == -1 and rounds[0] > 0 and rounds[2] > 0
    with pytest.raises(HipExtensionError, match="1 overflowed"):
        emd_exact_pairs(_c(A), _c(B), [(0, 0), (0, 1)], scale_log2=24)
    B[0, 0, 0] = np.nan
    assert assert_equals_law(A, B, [(0, 0)])[2][0] == -3


def test_no_assignment_buffer_is_needed():
    A, B = family_sets(65, ("uniform", "grid"))
    asg, cost, rounds = run_kernel(_c(A), _c(B), [(0, 0), (1, 1), (5, 5)])
    none, cost2, rounds2 = run_kernel(_c(A), _c(B), [(0, 0), (1, 1), (5, 5)], want_assignment=False)
    assert none is None and torch.equal(cost, cost2) and torch.equal(rounds, rounds2)


def test_loss_value_and_gradient():
    """emd_exact_loss at n = 100, b = 3.

    Value against the kernel's cost / 2^20.  Every q is within half a unit of sqrt_f32(d2_f32) 2^20, so the cost is within
    n 2^-21 of the sum of those fp32 distances.  A distance formed in fp32 from the fp32 coordinates by either route (three
    differences, three squares, two additions, one root) is within 4 u of the exact one relatively, u = 2^-24, and an n-term
    fp32 sum in any order adds at most (n - 1) u of the sum of the terms: together n 2^-21 + (n + 8) u cost.
    Gradient: (a_i - b_sigma(i)) / |a_i - b_sigma(i)| recomputed in fp64 on the host, 1e-6 absolute."""
    from hyperpocket_amd.utils.evaluation.emd_exact import emd_exact_loss, emd_exact_pairs
    n, batch = 100, 3
    A, B = family_sets(n, ("uniform", "clustered", "near"))
    a = _c(A).requires_grad_(True)
    b = _c(B).requires_grad_(True)
    loss = emd_exact_loss(a, b)
    assert loss.shape == (batch,) and loss.dtype == torch.float32
    cost, asg, rounds = emd_exact_pairs(_c(A), _c(B), [(k, k) for k in range(batch)], return_assignment=True)
    l_asg, _, _ = assign_pairs_law(A, B, [(k, k) for k in range(batch)])
    assert torch.equal(asg.cpu(), torch.from_numpy(l_asg))
    tol = n * 2.0 ** -21 + (n + 8) * 2.0 ** -24 * cost
    diff = (loss.double() - cost).abs()
    print("loss - cost:", diff.tolist(), "bound:", tol.tolist())
    assert (diff <= tol).all()
    loss.sum().backward()
    matched = np.stack([B[k][l_asg[k]] for k in range(batch)]).astype(np.float64)
    d = A.astype(np.float64) - matched
    unit = d / np.linalg.norm(d, axis=-1, keepdims=True)
    print("gradient error:", np.abs(a.grad.cpu().numpy() - unit).max())
    assert np.abs(a.grad.cpu().numpy() - unit).max() <= 1e-6
    want_b = np.zeros_like(unit)
    for k in range(batch):
        want_b[k][l_asg[k]] = -unit[k]
    assert np.abs(b.grad.cpu().numpy() - want_b).max() <= 1e-6


def test_pairwise_matrices_exact_and_approx():
    """5 x 7 clouds of 64 points: emd="exact" is scipy's optimum per pair on the law's q, / 2^20 / n, cast to fp32 once;
    emd="approx" is today's call, bit for bit, and the Chamfer matrix is the same in all three."""
    from hyperpocket_amd.utils.metrics import pairwise_EMD_CD
    rng = np.random.default_rng(11)
    S = rng.uniform(-0.5, 0.5, (5, 64, 3)).astype(np.float32)
    R = rng.uniform(-0.5, 0.5, (7, 64, 3)).astype(np.float32)
    cd0, emd0 = pairwise_EMD_CD(_c(S), _c(R))
    cd1, emd1 = pairwise_EMD_CD(_c(S), _c(R), emd="approx")
    assert torch.equal(cd0, cd1) and torch.equal(emd0, emd1)
    cd2, emd2 = pairwise_EMD_CD(_c(S), _c(R), emd="exact")
    assert torch.equal(cd0, cd2) and emd2.shape == (5, 7) and emd2.dtype == torch.float32
    want = np.empty((5, 7))
    for i in range(5):
        for j in range(7):
            q, _ = quantised_costs(S[i], R[j])
            rows, cols = linear_sum_assignment(q)
            want[i, j] = int(q[rows, cols].sum()) / 2.0 ** 20 / 64
    err = np.abs(emd2.cpu().numpy().astype(np.float64) - want)
    assert (err <= 2.0 ** -24 * want).all()
    with pytest.raises(ValueError):
        pairwise_EMD_CD(_c(S), _c(R), emd="both")


def test_metrics_take_the_keyword():
    from hyperpocket_amd.utils.metrics import earth_mover_distance, emd_approx, emd_exact, pairwise_EMD_CD, two_sample_metrics
    rng = np.random.default_rng(12)
    S = _c(rng.uniform(-0.5, 0.5, (6, 64, 3)).astype(np.float32))
    R = _c(rng.uniform(-0.5, 0.5, (6, 64, 3)).astype(np.float32))
    exact = emd_exact(S, R)
    assert torch.equal(exact, pairwise_EMD_CD(S, R, emd="exact")[1].diagonal())
    assert torch.equal(earth_mover_distance(S, R, emd="exact"), exact)
    assert torch.equal(earth_mover_distance(S, R), emd_approx(S, R))
    res = two_sample_metrics(S, R, emd="exact")
    M = pairwise_EMD_CD(R, S, emd="exact")[1]
    assert torch.equal(res["mmd(Fidelity)-EMD"], M.t().min(dim=0)[0].mean())
    assert set(res) == set(two_sample_metrics(S, R))
    with pytest.raises(ValueError):
        from hyperpocket_amd.utils.evaluation.emd_exact import emd_exact_pairs
        emd_exact_pairs(S, R[:, :32].contiguous(), [(0, 0)])


def test_another_stream_gives_the_same_bits():
    A, B = family_sets(200, ("uniform", "clustered", "grid"))
    pairs = [(0, 0), (1, 1), (2, 2), (2, 0)]
    dA, dB = _c(A), _c(B)
    ref = run_kernel(dA, dB, pairs)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = run_kernel(dA, dB, pairs)
    side.synchronize()
    for x, y in zip(ref, out):
        assert torch.equal(x, y)


def test_evaluate_generativity_takes_the_keyword(tmp_path):
    """emd="exact": the EMD keys are those of the exact matrices (recomputed here from the public pieces), the CD keys and
    the JSD are the default run's (1e-5: the pair kernel's fp64 Chamfer sums against the loop's), one_nn adds its keys
    without changing the six; emd="approx" is the default run."""
    from test_jsd_gpu import synthetic_datasets, trained_model
    from hyperpocket_amd.core.experiments import evaluate_generativity, lowest_y_half
    from hyperpocket_amd.utils.metrics import mmd_cov, pairwise_EMD_CD
    datasets, device, seed = synthetic_datasets(), torch.device("cuda"), 77

    def run(name, **kw):
        model, gm = trained_model()
        torch.manual_seed(seed)
        return evaluate_generativity(model, device, datasets, str(tmp_path / name), int(gm["epoch"]), 2, 0, **kw)

    plain, approx, exact = run("plain"), run("approx", emd="approx"), run("exact", emd="exact")
    assert plain == approx
    both = run("both", emd="exact", one_nn=True)
    with pytest.raises(ValueError):
        run("bad", emd="true")
    model, gm = trained_model()
    torch.manual_seed(seed)
    with torch.no_grad():
        for cat, items in datasets.items():
            cat_gt = torch.from_numpy(np.stack([it[1] for it in items])).cuda()
            K, want = len(items), {}
            for existing, _, _, _ in items:
                noise = torch.empty(K, model.get_noise_size()).normal_(mean=0.0, std=0.005).cuda()
                recs = lowest_y_half(model.sample_completions(torch.from_numpy(existing)[None].cuda(), noise, 2048, int(gm["epoch"])))
                for k, v in mmd_cov(pairwise_EMD_CD(cat_gt, recs, emd="exact")[1].t()).items():
                    want[k + "-EMD"] = want.get(k + "-EMD", 0.0) + v.item()
            assert set(exact[cat]) == set(plain[cat])
            for k, v in want.items():
                assert exact[cat][k] == v, (cat, k)
                assert both[cat][k] == v, (cat, k)
            for k in set(plain[cat]) - set(want):
                assert abs(exact[cat][k] - plain[cat][k]) <= 1e-5 * abs(plain[cat][k]), (cat, k)
            assert exact[cat]["mmd(Fidelity)-EMD"] != plain[cat]["mmd(Fidelity)-EMD"]
            assert set(both[cat]) > set(exact[cat])

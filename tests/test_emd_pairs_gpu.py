"""GPU suite for the pair form of the approximate EMD: hp_emd_pairs / emd_pairs() against the batched path on gathered clouds
(bit for bit: the pair list only changes where the set-up kernels read), the chunking, out-of-range pairs, the distance matrices
on it (pairwise_EMD_CD), the 1-NN two-sample accuracy (two_sample_metrics) against the CPU oracle, and evaluate_generativity's
one_nn switch.

Bars.  Bit identity is torch.equal.  Values against the fixture, the oracle, the Python-loop path and between chunk sizes: rtol
1e-5, the suite's EMD bar (tests/test_metrics_gpu.py); the regrouping of the cost partials between calls of different sizes is
stated as 2e-6 (csrc/emd.hip above emd_forward_impl).  The 1-NN accuracies are ratios of small integer counts (1e-6); the test
first proves on the oracle's matrices that every discrete decision behind them has a relative margin above 1e-4, ten times the
bar on the matrices."""
import contextlib
import json

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

RTOL = 1e-5


@pytest.fixture(scope="module")
def g():
    return golden("metrics")


def _c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lib():
    from hyperpocket_amd._lib import load_library
    return load_library()


class switch:
    """A process-wide library switch (hp_emd_set_*) at `value` inside the block, its previous value afterwards."""

    def __init__(self, name, value):
        self.fn, self.value = getattr(_lib(), name), value

    def __enter__(self):
        self.prev = self.fn(self.value)

    def __exit__(self, *exc):
        self.fn(self.prev)


def _rand(count, points, seed):
    return (torch.rand(count, points, 3, generator=torch.Generator().manual_seed(seed)) - 0.5).cuda()


def _all_pairs(na, nb):
    return torch.stack([torch.arange(na).repeat_interleave(nb), torch.arange(nb).repeat(na)], 1)


def _case(name, g):
    """-> (A, B, pairs (P,2) int64 on the host)"""
    if name == "a":          # the fixture's clouds: all 35 pairs in a scrambled order, and one of them a second time
        A, B = _c(g["sample"]), _c(g["ref"])
        pairs = _all_pairs(5, 7)[torch.randperm(35, generator=torch.Generator().manual_seed(35))]
        return A, B, torch.cat([pairs, pairs[11:12]])
    if name == "b":          # padding (neither size a multiple of 64) and n != m
        return _rand(3, 100, 1), _rand(4, 37, 2), _all_pairs(3, 4)
    assert name == "c"       # 130 pairs of 1024 points: two chains (fills_chip(65, 1024, 1)), an odd number of pairs per chain
    pairs = _all_pairs(12, 12)[torch.randperm(144, generator=torch.Generator().manual_seed(144))[:130]]
    return _rand(12, 1024, 3), _rand(12, 1024, 4), pairs


def _gathered(A, B, pairs):
    """The batched path on gathered copies: what a chunk of the pair form must equal bit for bit."""
    from hyperpocket_amd.utils.pytorch_structural_losses.match_cost import match_cost
    pairs = torch.as_tensor(pairs)
    return match_cost(A[pairs[:, 0].cuda()].contiguous(), B[pairs[:, 1].cuda()].contiguous())


# ---- 1: bit identity with the batched path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,switches", [
    ("a", ()), ("a", (("hp_emd_set_cull", 0),)), ("a", (("hp_emd_set_chains", 1),)),
    ("b", ()), ("b", (("hp_emd_set_cull", 0),)),
    ("c", ()), ("c", (("hp_emd_set_cull", 0),)),
])
def test_pair_costs_are_the_batched_paths_bits(g, name, switches):
    from hyperpocket_amd.utils.evaluation.emd_pairs import emd_pairs
    A, B, pairs = _case(name, g)
    assert pairs.size(0) == {"a": 36, "b": 12, "c": 130}[name]
    held = [switch(s, v) for s, v in switches]
    with contextlib.ExitStack() as stack:
        for sw in held:
            stack.enter_context(sw)
        got = emd_pairs(A, B, pairs)
        want = _gathered(A, B, pairs)
        torch.cuda.synchronize()
    for sw in held:          # restored: setting the previous value again finds it there
        assert sw.fn(sw.prev) == sw.prev
    assert got.shape == (pairs.size(0),) and got.dtype == torch.float32
    assert torch.isfinite(want).all() and (want > 0).all()
    print(name, switches, "max |pair - batched|", (got - want).abs().max().item(), "cost range", want.min().item(), want.max().item())
    assert torch.equal(got, want)
    if name == "a":          # the repeated pair
        assert got[35].item() == got[11].item()


# ---- 2: chunking ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [35, 36])
def test_chunks_equal_the_batched_path_chunk_by_chunk(g, count):
    """Chunks of 3 pairs over case (a): its 35 scrambled pairs make 12 chunks of which the last holds 2; with the repeated pair,
    36, the last chunk is full."""
    from hyperpocket_amd.utils.evaluation.emd_pairs import emd_pairs, emd_pairs_buffer_floats, emd_pairs_chunk
    A, B, pairs = _case("a", g)
    pairs = pairs[:count]
    budget = 4 * sum(emd_pairs_buffer_floats(3, 96, 96))
    assert emd_pairs_chunk(96, 96, budget) == 3
    got = emd_pairs(A, B, pairs, workspace_bytes=budget)
    starts = list(range(0, count, 3))
    assert len(starts) == 12 and count - starts[-1] == (2 if count == 35 else 3)
    for s in starts:
        assert torch.equal(got[s:s + 3], _gathered(A, B, pairs[s:s + 3])), s
    whole = emd_pairs(A, B, pairs)
    rel = ((got - whole).abs() / whole.abs()).max().item()
    print("chunks of 3 against one chunk: max relative difference", rel)
    np.testing.assert_allclose(got.cpu().numpy(), whole.cpu().numpy(), rtol=RTOL, atol=0)


# ---- 3: out-of-range pairs, edge cases ----------------------------------------------------------------------------------------
def test_out_of_range_pairs_cost_nan_and_leave_the_others_alone(g):
    from hyperpocket_amd.utils.evaluation.emd_pairs import emd_pairs
    A, B = _c(g["sample"]), _c(g["ref"])
    nb = B.size(0)
    good = [(0, 0), (2, 3), (4, 6), (1, 5)]
    mixed = [good[0], (-1, 0), good[1], (0, nb), good[2], good[3]]
    for sw in ((), (("hp_emd_set_cull", 0),)):          # both set-up kernels clamp
        with contextlib.ExitStack() as stack:
            for s, v in sw:
                stack.enter_context(switch(s, v))
            got = emd_pairs(A, B, mixed).cpu()
            want = emd_pairs(A, B, good).cpu()
        assert torch.isnan(got).tolist() == [False, True, False, True, False, False]
        assert torch.equal(got[[0, 2, 4, 5]], want) and torch.isfinite(want).all()
    # every pair out of range, on either side and far out
    bad = emd_pairs(A, B, [(5, 0), (0, -1), (2 ** 31 - 1, 0), (-2 ** 31, 7)])
    assert torch.isnan(bad).all()
    # int64 indices that would wrap into the sets if they were cut to int32: 2^32 -> 0, 2^32 + 1 -> 1, -2^32 + 2 -> 2
    wide = torch.tensor([(2 ** 32, 0), (1, 2 ** 32 + 1), (-2 ** 32 + 2, 2), (2, 3)], dtype=torch.int64)
    want = emd_pairs(A, B, good).cpu()          # under the default switches
    for p in (wide, wide.cuda()):
        got = emd_pairs(A, B, p).cpu()
        assert torch.isnan(got).tolist() == [True, True, True, False] and got[3].item() == want[1].item()
    with pytest.raises(ValueError):
        emd_pairs(A, B, torch.tensor([(0.0, 1.0)]))


def test_zero_pairs_repeat_calls_and_another_stream(g):
    from hyperpocket_amd.utils.evaluation.emd_pairs import emd_pairs
    A, B, pairs = _case("a", g)
    empty = emd_pairs(A, B, torch.empty((0, 2), dtype=torch.int64))
    assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.is_cuda
    first = emd_pairs(A, B, pairs)
    again = emd_pairs(A, B, pairs.to(torch.int32).cuda())          # a device int32 list is taken as it is
    assert torch.equal(first, again)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = emd_pairs(A, B, pairs)
    side.synchronize()
    assert torch.equal(on_side, first)
    from hyperpocket_amd import HipExtensionError
    with pytest.raises(HipExtensionError):
        emd_pairs(A.cpu(), B, pairs)
    with pytest.raises(ValueError):
        emd_pairs(A[0], B, pairs)


# ---- 4: the matrices ----------------------------------------------------------------------------------------------------------
def test_pairwise_matrices_equal_the_fixture_and_the_loop(g):
    from hyperpocket_amd.utils import metrics as M
    s, r = _c(g["sample"]), _c(g["ref"])
    cd, emd = M.pairwise_EMD_CD(s, r)
    assert cd.shape == (5, 7) and emd.shape == (5, 7) and cd.dtype == torch.float32 and emd.dtype == torch.float32
    np.testing.assert_allclose(cd.cpu().numpy(), g["pairwise_cd"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(emd.cpu().numpy(), g["pairwise_emd"], rtol=RTOL, atol=0)
    loop_cd, loop_emd = M._pairwise_EMD_CD_(s, r, 3)
    print("pair form against the loop: CD", ((cd - loop_cd).abs() / loop_cd).max().item(), "EMD", ((emd - loop_emd).abs() / loop_emd).max().item())
    np.testing.assert_allclose(cd.cpu().numpy(), loop_cd.cpu().numpy(), rtol=RTOL, atol=0)
    np.testing.assert_allclose(emd.cpu().numpy(), loop_emd.cpu().numpy(), rtol=RTOL, atol=0)
    small_cd, small_emd = M.pairwise_EMD_CD(s, r, workspace_bytes=0)          # one pair per chunk
    np.testing.assert_allclose(small_emd.cpu().numpy(), emd.cpu().numpy(), rtol=RTOL, atol=0)
    assert torch.equal(small_cd, cd)
    with pytest.raises(AssertionError):
        M.pairwise_EMD_CD(s[:, :50].contiguous(), r)


# ---- 5: 1-NN two-sample accuracy against the CPU oracle ------------------------------------------------------------------------
def _oracle_matrices(oracle_lib, X, Y):
    """(len(X), len(Y)) fp32 CD and EMD matrices of two numpy cloud sets: numpy brute force in fp64 / the C oracle's approxmatch and
    matchcost divided by the number of points."""
    nx, ny, n = len(X), len(Y), X.shape[1]
    ia, ib = np.repeat(np.arange(nx), ny), np.tile(np.arange(ny), nx)
    a, b = np.ascontiguousarray(X[ia]), np.ascontiguousarray(Y[ib])
    match, _ = oracle_lib.approxmatch(a, b)
    emd = oracle_lib.matchcost(a, b, match) / np.float32(n)
    d2 = ((a[:, :, None, :].astype(np.float64) - b[:, None, :, :].astype(np.float64)) ** 2).sum(-1)
    cd = d2.min(2).mean(1) + d2.min(1).mean(1)
    return cd.astype(np.float32).reshape(nx, ny), emd.astype(np.float32).reshape(nx, ny)


def _smallest_gap(M, dim):
    """Smallest relative gap between the smallest and the second smallest entry along `dim` of a matrix."""
    two = torch.as_tensor(M).double().topk(2, dim, largest=False).values
    lo, hi = two.select(dim, 0), two.select(dim, 1)
    return ((hi - lo) / lo).min().item()


def test_two_sample_metrics_equal_the_oracles(g, oracle_lib):
    from hyperpocket_amd.utils import metrics as M
    sample, ref = g["sample"], g["ref"]
    rs, rr, ss = (_oracle_matrices(oracle_lib, x, y) for x, y in ((ref, sample), (ref, ref), (sample, sample)))
    want = {}
    for d, name in ((0, "CD"), (1, "EMD")):
        m_rs, m_rr, m_ss = (torch.from_numpy(m[d]) for m in (rs, rr, ss))
        # the discrete decisions: each column's nearest neighbour in the matrix knn builds, each sample's nearest reference
        n0, n1 = m_rr.size(0), m_ss.size(0)
        full = torch.cat((torch.cat((m_rr, m_rs), 1), torch.cat((m_rs.t(), m_ss), 1)), 0) + torch.diag(torch.full((n0 + n1,), float("inf")))
        gap_knn, gap_cov = _smallest_gap(full, 0), _smallest_gap(m_rs.t(), 1)
        print(name, "smallest relative gap: 1-NN columns", gap_knn, "coverage arg-min", gap_cov)
        assert gap_knn > 1e-4 and gap_cov > 1e-4, "a near-tie: the discrete outcomes are not defined at the 1e-5 agreement of the matrices"
        want.update({f"{k}-{name}": v.item() for k, v in M.mmd_cov(m_rs.t()).items()})
        want.update({f"1-NN-{name}-{k}": v.item() for k, v in M.knn(m_rr, m_rs, m_ss, 1, sqrt=False).items() if "acc" in k})
    s, r = _c(sample), _c(ref)
    got = {k: v.item() for k, v in M.two_sample_metrics(s, r).items()}
    print("two_sample_metrics", got)
    assert set(got) == set(want) and len(got) == 12
    assert {k for k in got if k.startswith("1-NN")} == {f"1-NN-{d}-{k}" for d in ("CD", "EMD") for k in ("acc", "acc_t", "acc_f")}
    for k, v in want.items():
        if k.startswith("1-NN"):
            assert abs(got[k] - v) <= 1e-6, (k, got[k], v)
        else:
            assert abs(got[k] - v) <= RTOL * abs(v), (k, got[k], v)
    within = M.pairwise_EMD_CD(r, r)
    assert {k: v.item() for k, v in M.two_sample_metrics(s, r, ref_within=within).items()} == got


# ---- 6: the experiment --------------------------------------------------------------------------------------------------------
BASE_KEYS = {f"{k}-{d}" for k in ("mmd(Fidelity)", "cov(Coverage)", "mmd_smp") for d in ("CD", "EMD")} | {"jsd"}
ONE_NN_KEYS = {f"1-NN-{d}-{k}" for d in ("CD", "EMD") for k in ("acc", "acc_t", "acc_f")}


def test_evaluate_generativity_one_nn(tmp_path):
    from test_jsd_gpu import synthetic_datasets, trained_model
    from hyperpocket_amd.core.experiments import evaluate_generativity, lowest_y_half
    from hyperpocket_amd.utils.metrics import jsd_between_point_cloud_sets, two_sample_metrics
    datasets, device, batch_size, seed = synthetic_datasets(), torch.device("cuda"), 2, 77

    def run(name, **kw):
        model, gm = trained_model()
        epoch = int(gm["epoch"])
        torch.manual_seed(seed)
        res = evaluate_generativity(model, device, datasets, str(tmp_path / name), epoch, batch_size, 0, **kw)
        on_disk = json.loads((tmp_path / name / "evaluate_generativity" / f"{epoch}eval_gen_by_cat.json").read_text())
        assert on_disk == res
        return res

    # the default: no new keys, and the values of an explicit one_nn=False run
    plain, explicit = run("plain"), run("explicit", one_nn=False)
    assert plain == explicit and set(plain) == set(datasets) and all(set(v) == BASE_KEYS for v in plain.values())

    res = run("one_nn", one_nn=True)
    assert set(res) == set(datasets) and all(set(v) == BASE_KEYS | ONE_NN_KEYS for v in res.values())
    model, gm = trained_model()          # a second, identically built and seeded model: the experiment's has advanced its sampler
    epoch = int(gm["epoch"])
    torch.manual_seed(seed)
    with torch.no_grad():
        for cat, items in datasets.items():
            cat_gt = torch.from_numpy(np.stack([it[1] for it in items])).cuda()
            K, want = len(items), {}
            assert K == 3
            for existing, _, _, _ in items:
                noise = torch.empty(K, model.get_noise_size()).normal_(mean=0.0, std=0.005).cuda()
                obj_recs = lowest_y_half(model.sample_completions(torch.from_numpy(existing)[None].cuda(), noise, 2048, epoch))
                for k, v in two_sample_metrics(obj_recs, cat_gt).items():
                    want[k] = want.get(k, 0.0) + v.item()
                want["jsd"] = want.get("jsd", 0.0) + jsd_between_point_cloud_sets(obj_recs, cat_gt)
            print(cat, res[cat], want)
            assert set(want) == set(res[cat])
            for k, v in want.items():
                assert abs(res[cat][k] - v) <= 1e-6 * abs(v), (cat, k, res[cat][k], v)
            assert np.isfinite(list(want.values())).all()
            assert all(0.0 <= want[k] <= K for k in ONE_NN_KEYS)          # K accuracies summed
            # the six shared keys: the pair kernels against the loop of the default path, to the regrouping of sums
            for k in BASE_KEYS - {"jsd"}:
                assert abs(res[cat][k] - plain[cat][k]) <= RTOL * abs(plain[cat][k]), (cat, k, res[cat][k], plain[cat][k])
            assert res[cat]["jsd"] == plain[cat]["jsd"]

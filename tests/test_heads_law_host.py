"""CPU suite for tests/heads_law.py and the heads' route query.

  * hp_hypernet_heads_plan (host only, follows no data pointer: the addresses here are made up) reports every route for the case
    meant to reach it and flips at every boundary of the dispatch: B 64 | 65, total 15 | 16, W and t aligned | + 4 bytes,
    heads contiguous | not, hp_hypernet_set_heads_stream 1 | 0; the case tables of tests/test_heads_gpu.py reach all of them.
  * The laws admit a correct fp32 implementation: a plain float32 numpy evaluation of each operation sits inside every
    bound (equals the integers in family E), no element left out.
  * The laws catch what they are for: each named mutant of a REFERENCE (heads_law.MUTANTS; never of GPU code) leaves the
    bound on at least 1 % of the elements of one of its listed cases.  A mutant counts as caught at an element where it is
    more than TWICE the bound from the reference (or differs from the integer, family E): an fp32 implementation of the
    mutant, itself within one bound of it, would still fail there.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import PKG_DIR

import heads_law as law


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build(verbose=False))


# ------------------------------------------------------------------------------------------------ the route query
def test_cases_reach_every_route(lib):
    law.check_cases_reach_every_route(lib)


def test_plan_reports_every_route_and_flips_at_every_boundary(lib):
    T, A = 1 << 32, 1 << 30
    one = lambda n, **kw: law.fake_heads((n,), **kw)
    fwd = lambda B, w, t=T: law.plan(lib, B, w, None, t, None)[:2]
    with law.stream_switch(lib, 1):
        w, gr = one(81)
        assert law.plan(lib, 17, w, gr, T, A) == (0, law.FWD_STREAM, law.DW_DIRECT, law.DW_DIRECT)
        assert law.plan(lib, 17, w, None, T, None) == (0, law.FWD_STREAM, -1, -1)
        # B 64 | 65 (and 1: the lower end)
        assert [fwd(B, w) for B in (1, 64, 65)] == [(0, law.FWD_STREAM), (0, law.FWD_STREAM), (0, law.FWD_GEMM)]
        # total 15 | 16: one head, and three heads that make it up together
        assert fwd(17, one(15)[0]) == (0, law.FWD_GEMM) and fwd(17, one(16)[0]) == (0, law.FWD_STREAM)
        assert fwd(17, law.fake_heads((7, 3, 5))[0]) == (0, law.FWD_GEMM) and fwd(17, law.fake_heads((7, 3, 6))[0]) == (0, law.FWD_STREAM)
        # W aligned | + 4 bytes; t aligned | + 4 bytes (the t5 block and the split workspace inherit t's phase at every B)
        assert fwd(17, one(81, w0=A + 4)[0]) == (0, law.FWD_GEMM) and fwd(17, one(81, w0=A + 16)[0]) == (0, law.FWD_STREAM)
        for B in (1, 2, 3, 17, 64):
            assert fwd(B, w, T) == (0, law.FWD_STREAM) and fwd(B, w, T + 4) == (0, law.FWD_GEMM), B
        # contiguous | not: weights apart, or only the biases apart
        assert fwd(17, law.fake_heads((16, 3, 45))[0]) == (0, law.FWD_STREAM)
        assert fwd(17, law.fake_heads((16, 3, 45), contiguous=False)[0]) == (0, law.FWD_PER_HEAD)
        wb, _ = law.fake_heads((16, 3, 45))
        wb.head_b[2] += 4
        assert fwd(17, wb) == (0, law.FWD_PER_HEAD)
        assert fwd(65, law.fake_heads((16, 3, 45), contiguous=False)[0]) == (0, law.FWD_PER_HEAD)
    # switch 1 | 0: the forward alone
    with law.stream_switch(lib, 0):
        assert law.plan(lib, 17, w, gr, T, A) == (0, law.FWD_GEMM, law.DW_DIRECT, law.DW_DIRECT)
    with law.stream_switch(lib, 1):
        assert fwd(17, w) == (0, law.FWD_STREAM)


def test_plan_dw_routes(lib):
    T, A = 1 << 32, 1 << 30
    dw = lambda w, gr, t=T, B=9: law.plan(lib, B, w, gr, t, None)
    w, gr = law.fake_heads((33,))
    assert dw(w, gr)[2] == law.DW_DIRECT and dw(w, gr, B=130)[2] == law.DW_DIRECT           # no limit on the batch
    assert dw(w, gr, T + 4)[2] == law.DW_GEMM                                              # t5 off its boundary
    gr.head_w[0] += 4
    assert dw(w, gr)[2] == law.DW_GEMM                                                     # the gradient off its boundary
    gr.head_w[0] = None
    assert dw(w, gr)[::2] == (0, law.DW_SKIPPED)
    w3, g3 = law.fake_heads((16, 3, 45))
    assert dw(w3, g3)[2] == law.DW_DIRECT
    g3.head_b[1] += 4                                                                       # gradients not back to back
    assert dw(w3, g3)[2] == law.DW_PER_HEAD
    g3.head_w[0] = None
    assert dw(w3, g3)[0] == -1                                                              # a skipped dW needs them back to back
    w3, g3 = law.fake_heads((16, 3, 45), contiguous=False)
    assert dw(w3, g3)[2] == law.DW_PER_HEAD
    g3.head_w[0] = None
    assert dw(w3, g3)[0] == -1
    # the row-slice call: either operand off its boundary
    assert law.rows_route(lib, T, A) == law.DW_DIRECT
    assert law.rows_route(lib, T, A + 4) == law.DW_GEMM and law.rows_route(lib, T + 4, A) == law.DW_GEMM
    assert law.rows_route(lib, T + 16, A + 16) == law.DW_DIRECT
    # what the query refuses
    p = law.HeadsPlan()
    assert lib.hp_hypernet_heads_plan(0, ctypes.byref(w), None, ctypes.c_void_p(T), None, ctypes.byref(p)) == -1
    assert lib.hp_hypernet_heads_plan(4, None, None, ctypes.c_void_p(T), None, ctypes.byref(p)) == -1
    assert lib.hp_hypernet_heads_plan(4, ctypes.byref(w), None, None, None, ctypes.byref(p)) == -1
    assert lib.hp_hypernet_heads_plan(4, ctypes.byref(w), None, ctypes.c_void_p(T), None, None) == -1
    w.n_heads = law.HP_MAX_HEADS + 1
    assert lib.hp_hypernet_heads_plan(4, ctypes.byref(w), None, ctypes.c_void_p(T), None, ctypes.byref(p)) == -1


# ------------------------------------------------------------------------------------------------ fixtures
def _fwd_fixture(fam, B, N):
    t5 = law.trunk64(fam, B)
    W, b = law.head_weights(fam)
    return t5, W[:N], b[:N]


def test_family_e_premise_holds_on_the_fixtures():
    for B in (1, 17, 64):
        t5 = law.trunk64("E", B)
        assert law.is_family_e(t5), B
    W, b = law.head_weights("E")
    assert law.is_family_e(W) and bool((b == b.round()).all())
    d, t = law.dw_operands("E", 7, 40)
    assert law.is_family_e(d) and law.is_family_e(t)
    # family R: the significands are full (the low mantissa bits are in use), so the second and third bf16 pieces are not zeros
    W, _ = law.head_weights("R")
    p1, p2, p3 = law.split3(W[:64])
    assert bool((p1 + p2 + p3 == W[:64].double()).all()) and float((p3 != 0).double().mean()) > 0.9


# ------------------------------------------------------------------------------------------------ fp32 sits inside the bounds
@pytest.mark.parametrize("fam", ["E", "R"])
def test_fp32_forward_sits_inside_the_law(fam):
    for B, N in [(17, 17), (17, 81), (64, 81), (49, 81), (64, 2561)]:
        t5, W, b = _fwd_fixture(fam, B, N)
        got = torch.from_numpy(t5.numpy() @ W.numpy().T + b.numpy())
        assert got.dtype == torch.float32
        if fam == "E":
            law.check_exact(f"fp32 {fam} B={B} N={N}", "theta", got, law.int_mm(t5, W.t(), b))
        else:
            want, bound = law.fwd64(t5, W, b)
            assert law.check(f"fp32 {fam} B={B} N={N}", "theta", got, want, bound) < 1.0


@pytest.mark.parametrize("fam", ["E", "R"])
def test_fp32_dw_sits_inside_the_law(fam):
    for Kc, rows in [(1, 33), (3, 33), (7, 33), (64, 65), (65, 33), (130, 33)]:
        dth, t5 = law.dw_operands(fam, Kc, rows)
        got = torch.from_numpy(dth.numpy().T @ t5.numpy())
        gdb = torch.from_numpy(dth.numpy().sum(0, dtype=np.float32))
        tag = f"fp32 {fam} Kc={Kc} rows={rows}"
        if fam == "E":
            law.check_exact(tag, "dW", got, law.int_mm(dth.t(), t5))
            law.check_exact(tag, "db", gdb, dth.to(torch.int64).sum(0))
        else:
            want, bound, wdb, bdb = law.dw64(dth, t5)
            law.check(tag, "dW", got, want, bound)
            law.check(tag, "db", gdb, wdb, bdb)


def test_fp32_adam_sits_inside_the_law():
    worst = 0.0
    for n in (1, 5, 1025, 70001):
        for step in law.ADAM_STEPS:
            for scale in law.ADAM_SCALES:
                fx = law.adam_fixture(n, scale)
                ref = law.adam64(fx["p"], fx["g"], fx["m"], fx["v"], step, scale, **law.HYPER)
                got = law.f32_adam(fx["p"], fx["g"], fx["m"], fx["v"], step, scale, **law.HYPER)
                worst = max(worst, law.check_adam(f"fp32 adam n={n} step={step} scale={scale}", got, ref))
                z = fx["zero"]
                for k in "pmv":
                    assert torch.equal(got[k][z], fx[k][z]), (k, n)
    assert 0.0 < worst <= 1.0


def test_adam64_is_torch_optim_adam_in_float64():
    """The reference is the optimiser the kernel's comment cites: torch.optim.Adam (single tensor, wd = 0, amsgrad off) on
    float64 copies of the fixture, its state set to (step - 1, m, v).  Agreement to fp64 rounding."""
    fx = law.adam_fixture(1025)
    lr, b1, b2, eps = (law.f32(law.HYPER[k]) for k in ("lr", "b1", "b2", "eps"))
    for step in law.ADAM_STEPS:
        p = torch.nn.Parameter(fx["p"].double().clone())
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=0.0, amsgrad=False, foreach=False)
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": fx["m"].double().clone(),
                        "exp_avg_sq": fx["v"].double().clone()}
        p.grad = fx["g"].double().clone()
        opt.step()
        ref = law.adam64(fx["p"], fx["g"], fx["m"], fx["v"], step, 1.0, **law.HYPER)
        for k, t in (("p", p.detach()), ("m", opt.state[p]["exp_avg"]), ("v", opt.state[p]["exp_avg_sq"])):
            err = (ref[k] - t).abs()
            assert bool((err <= 1e-3 * ref["b" + k]).all()), (step, k, float(err.max()))


# ------------------------------------------------------------------------------------------------ mutants
def _caught_share(kind, name, case):
    """Share of the case's elements at which the mutant is outside the law."""
    if kind == "fwd":
        fam, B, N = case
        t5, W, b = _fwd_fixture(fam, B, N)
        mut = law.fwd_mutant(name, t5, W, b)
        if fam == "E":
            return float((mut != law.int_mm(t5, W.t(), b).double()).double().mean())
        want, bound = law.fwd64(t5, W, b)
        return float(((mut - want).abs() > 2 * bound).double().mean())
    if kind == "dw":
        fam, Kc, rows = case
        dth, t5 = law.dw_operands(fam, Kc, rows)
        mw, mb = law.dw_mutant(name, dth, t5)
        want, bound, wdb, bdb = law.dw64(dth, t5)
        if fam == "E":
            bound, bdb = torch.zeros_like(bound), torch.zeros_like(bdb)
        if name.startswith("db_"):                 # the bias gradient is the output under test
            return float(((mb - wdb).abs() > 2 * bdb).double().mean())
        return float(((mw - want).abs() > 2 * bound).double().mean())
    n, step, scale = case
    fx = law.adam_fixture(n, scale)
    ref = law.adam64(fx["p"], fx["g"], fx["m"], fx["v"], step, scale, **law.HYPER)
    mut = law.adam64(fx["p"], fx["g"], fx["m"], fx["v"], step, scale, mutant=name, **law.HYPER)
    bad = torch.zeros(n, dtype=torch.bool)
    for k in "pmv":
        bad |= (mut[k] - ref[k]).abs() > 2 * ref["b" + k]
    return float(bad.double().mean())


@pytest.mark.parametrize("name", sorted(law.MUTANTS))
def test_the_laws_catch_the_mutant(name):
    kind, cases = law.MUTANTS[name]
    shares = {case: _caught_share(kind, name, case) for case in cases}
    print(f"MUTANT {name}: " + ", ".join(f"{c} {100 * s:.1f} %" for c, s in shares.items()))
    assert all(s >= 0.01 for s in shares.values()), (name, shares)


def test_the_piece_mutant_is_invisible_to_family_e_by_construction():
    """An integer of size <= 8 is one bf16 piece: the second pieces are zeros and a dropped b1 c2 product changes nothing.
    That is why family R is run at every case as well."""
    t5, W, b = _fwd_fixture("E", 17, 81)
    assert torch.equal(law.fwd_mutant("fwd_piece_b1c2_dropped", t5, W, b), law.int_mm(t5, W.t(), b).double())

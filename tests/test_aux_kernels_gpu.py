"""GPU: csrc/aux_kernels.hip against tests/aux_law.py — the point sampler, the device-drawn random-plane slicer, the KLD
term and the step's loss scalars.  Every comparison is of bits (float32 viewed as int32), except the KLD value and grad_explv
for general v, where expf enters: those are held to the per-call bound of aux_law.kld_bound / kld_grad_v_bound (E = 2 ulp for
expf, the header's 1 ulp for the hardware exponential times two for the range reduction), and print error / bound beside the
same figure for torch's fp32 evaluation on the CPU.  tests/test_aux_law_host.py proves on the CPU what the case tables cover.
One PARITY line per family is printed before anything is asserted (profiles/aux_kernels_parity.md holds a run's lines)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import aux_law as law

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = 77.0
U64 = ctypes.c_ulonglong


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype == F32 and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def sliced(N, target, seed):
    return law.slice_law(law.slice_clouds_of(N, target), target, seed, law.SLICE_LIMIT // law.WAVES)


# ---------------------------------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------------------------------
def test_sampler_is_the_law_draw_for_draw():
    from hyperpocket_amd._lib import call, current_stream
    from hyperpocket_amd.ops import sample_points
    wrong, runs, points = [], 0, 0
    for seed, offset in law.SAMPLER_SEEDS:
        for coef in law.SAMPLER_COEFS:
            for total in law.SAMPLER_TOTALS:
                got = sample_points(1, total, coef, seed, offset, "cuda").cpu().numpy()[0]
                want = law.sampler_law(total, coef, seed, offset)
                runs, points = runs + 1, points + total
                if not same_bits(got, want):
                    rows = np.flatnonzero((got.view(np.int32) != want.view(np.int32)).any(1))
                    wrong.append((seed, offset, coef, total, rows.size, int(rows[0])))
    # total = 0: nothing is written
    out = torch.full((4, 3), SENTINEL, device="cuda")
    call("hp_sample_points", ctypes.c_long(0), 0.5, U64(7), U64(1), out, current_stream(out.device))
    torch.cuda.synchronize()
    untouched = bool((out == SENTINEL).all())
    print(f"PARITY sampler: {runs} runs, {points} points, {len(wrong)} runs with a differing point (bit for bit); "
          f"total = 0 writes nothing: {untouched}")
    assert not wrong, wrong[:5]
    assert untouched


def test_full_model_draws_its_points_by_the_law():
    """FullModel._draw_points: Philox key = torch.initial_seed() (above 2^32 by default), offset = the number of the call,
    coef = float32(normalization_coef(config, epoch))."""
    import copy
    from hyperpocket_amd.model.full_model import FullModel
    from hyperpocket_amd.utils.points import normalization_coef
    cfg = {"random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "hyper_network": {"use_bias": True, "relu_slope": 0.2},
           "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                              "layer_out_channels": [32, 64, 128, 64]},
           "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}
    B, N = 3, 100
    state = torch.get_rng_state()
    wrong = []
    try:
        torch.manual_seed(67280421310721)                          # torch's default seed: the high word is in use
        model = FullModel(copy.deepcopy(cfg))
        for epoch in (1, 37, 250):
            model._sampler_seed, model._sampler_calls = None, 0
            coef = F32(normalization_coef(model.point_generator_config, epoch))
            for offset in (1, 2):
                got = model._draw_points(epoch, B, N, "cuda").cpu().numpy()
                want = law.sampler_law(B * N, coef, torch.initial_seed(), offset).reshape(B, N, 3)
                if not same_bits(got, want):
                    wrong.append((epoch, offset))
        seed = torch.initial_seed()
    finally:
        torch.set_rng_state(state)
    print(f"PARITY sampler through FullModel._draw_points: seed {seed}, epochs 1 / 37 / 250, calls 1 and 2: "
          f"{len(wrong)} of 6 draws differ")
    assert seed >> 32 and not wrong, wrong


# ---------------------------------------------------------------------------------------------------------------------
# device-drawn slicer
# ---------------------------------------------------------------------------------------------------------------------
def test_slicer_is_the_law_split_for_split():
    from hyperpocket_amd.ops import slice_clouds
    wrong, clouds, latest, sides = [], 0, 0, [0, 0]
    for seed in law.SLICE_SEEDS:
        for N, target in law.SLICE_CASES:
            pts = law.slice_clouds_of(N, target)
            want_a, want_b, want_plane, status, index = sliced(N, target, seed)
            assert (status == 0).all()
            a, b, plane = slice_clouds(dev(pts), target, seed=seed, max_rounds=law.SLICE_LIMIT // law.WAVES)
            a, b, plane = a.cpu().numpy(), b.cpu().numpy(), plane.cpu().numpy()
            clouds, latest = clouds + law.SLICE_CLOUDS, max(latest, int(index.max()))
            for c in range(law.SLICE_CLOUDS):
                under = law.under_mask(pts[c], want_plane[c])
                sides[0 if np.array_equal(pts[c][under], want_a[c]) else 1] += 1
            if not (same_bits(a, want_a) and same_bits(b, want_b) and same_bits(plane, want_plane)):
                wrong.append((seed, N, target, same_bits(plane, want_plane), same_bits(a, want_a), same_bits(b, want_b)))
    # a centred ball, as the shapes of the workload are, through the wrapper's default max_rounds
    ball = law.ball_clouds()
    for seed in law.SLICE_SEEDS:
        want_a, want_b, want_plane, status, index = law.slice_law(ball, law.BALL_CASE[1], seed, 100000)
        assert (status == 0).all()
        a, b, plane = slice_clouds(dev(ball), law.BALL_CASE[1], seed=seed)
        clouds, latest = clouds + law.SLICE_CLOUDS, max(latest, int(index.max()))
        if not (same_bits(a.cpu().numpy(), want_a) and same_bits(b.cpu().numpy(), want_b) and same_bits(plane.cpu().numpy(), want_plane)):
            wrong.append((seed, "ball"))
    print(f"PARITY slicer (device-drawn planes): {clouds} clouds, N = 2 .. 8192, latest accepted candidate {latest}, "
          f"part_a the under / the other side {sides[0]} / {sides[1]}: {len(wrong)} calls with a differing part or plane (bit for bit)")
    assert not wrong, wrong


def raw_slice(lib, pts, target, seed, max_rounds):
    """hp_slice_clouds through the C ABI on sentinel-filled outputs -> (rc, part_a, part_b, plane, status) as numpy."""
    B, N = pts.shape[:2]
    P = dev(pts)
    a = torch.full((B, target, 3), SENTINEL, device="cuda")
    b = torch.full((B, N - target, 3), SENTINEL, device="cuda")
    plane = torch.full((B, 4), SENTINEL, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.hp_slice_clouds(B, N, target, p(P), U64(seed), max_rounds, p(a), p(b), p(plane), p(status), None)
    torch.cuda.synchronize()
    return rc, a.cpu().numpy(), b.cpu().numpy(), plane.cpu().numpy(), status.cpu().numpy()


def test_slicer_status_is_per_cloud_and_a_failed_cloud_is_left_alone():
    from hyperpocket_amd import load_library
    lib = load_library()
    wrong, calls = [], 0
    for seed in law.SLICE_SEEDS:
        for N, target in law.STATUS_CASES:
            pts = law.slice_clouds_of(N, target)
            index = sliced(N, target, seed)[4]
            slow = int(np.argmax(index))
            rounds = int(index[slow]) // law.WAVES + 1
            assert rounds >= 2 and sorted(index // law.WAVES)[-2] < rounds - 1          # one cloud alone needs the last round
            for max_rounds in (rounds, rounds - 1):
                want_a, want_b, want_plane, want_status, _ = law.slice_law(pts, target, seed, max_rounds)
                assert want_status.tolist() == [int(max_rounds < rounds and c == slow) for c in range(law.SLICE_CLOUDS)]
                rc, a, b, plane, status = raw_slice(lib, pts, target, seed, max_rounds)
                calls += 1
                ok = rc == 0 and status.tolist() == want_status.tolist()
                for c in range(law.SLICE_CLOUDS):
                    if want_status[c]:
                        ok = ok and (a[c] == SENTINEL).all() and (b[c] == SENTINEL).all() and (plane[c] == SENTINEL).all()
                    else:
                        ok = ok and same_bits(a[c], want_a[c]) and same_bits(b[c], want_b[c]) and same_bits(plane[c], want_plane[c])
                if not ok:
                    wrong.append((seed, N, target, max_rounds, rc, status.tolist()))
    pts = np.zeros((1, 8193, 3), F32)
    beyond = raw_slice(lib, pts, 4096, 7, 4)
    print(f"PARITY slicer status: {calls} calls at the winning round + 1 and one fewer: {len(wrong)} wrong; "
          f"N = 8193 returns {beyond[0]}")
    assert not wrong, wrong
    assert beyond[0] == -1 and (beyond[1] == SENTINEL).all() and (beyond[4] == -7).all()


# ---------------------------------------------------------------------------------------------------------------------
# KLD
# ---------------------------------------------------------------------------------------------------------------------
def kld_forward(v, mu, batch):
    from hyperpocket_amd._lib import call, current_stream
    out = torch.full((1,), SENTINEL, device="cuda")
    call("hp_kld_forward", ctypes.c_long(mu.numel()), batch, v, mu, out, current_stream(out.device))
    return out.cpu().numpy()[0]


def kld_backward(v, mu, batch, g):
    from hyperpocket_amd._lib import call, current_stream
    gv, gm = torch.full_like(v, SENTINEL), torch.full_like(mu, SENTINEL)
    gout = torch.tensor([g], dtype=torch.float32, device="cuda")
    call("hp_kld_backward", ctypes.c_long(mu.numel()), batch, v, mu, gout, gv, gm, current_stream(gv.device))
    return gv.cpu().numpy(), gm.cpu().numpy()


def test_kld_is_exact_where_expf_is():
    """v = 0, mu = +-k/64: every fp32 term and the float64 sum are exact, so no summation order excuses a difference —
    an element dropped or counted twice at a loop boundary changes the result (tests/test_aux_law_host.py)."""
    wrong_fwd, wrong_mu, wrong_v, runs = [], [], [], 0
    for n in law.KLD_N:
        mu = law.kld_exact_mu(n)
        v_d, mu_d = torch.zeros(n, device="cuda"), dev(mu)
        for batch in law.KLD_BATCH:
            runs += 1
            got, want = kld_forward(v_d, mu_d, batch), law.kld_exact_v0(mu, batch)
            if not same_bits(np.array([got]), np.array([want])):
                wrong_fwd.append((n, batch, float(got), float(want)))
            for g in law.KLD_G:
                gv, gm = kld_backward(v_d, mu_d, batch, g)
                if not same_bits(gm, law.kld_grad_mu_law(mu, batch, g)):
                    wrong_mu.append((n, batch, g))
                if gv.view(np.int32).any():                                    # exactly +0
                    wrong_v.append((n, batch, g))
    print(f"PARITY kld exact (v = 0): {runs} (n, batch) pairs, n = 1 .. 12289: forward differs in {len(wrong_fwd)}, "
          f"grad_mu in {len(wrong_mu)} of {3 * runs}, grad_explv not +0 in {len(wrong_v)} (bit for bit)")
    assert not wrong_fwd, wrong_fwd[:5]
    assert not wrong_mu and not wrong_v, (wrong_mu[:5], wrong_v[:5])


@pytest.mark.parametrize("regime", law.KLD_REGIMES)
def test_kld_is_within_the_derived_bound_of_float64(regime):
    g = 3.0
    worst = {"fwd": (0.0, None), "fwd_cpu_fp32": (0.0, None), "gv": (0.0, None), "gv_cpu_fp32": (0.0, None)}
    wrong_mu = []

    def note(key, ratio, case):
        if ratio > worst[key][0]:
            worst[key] = (float(ratio), case)

    for n in law.KLD_N:
        for batch in law.KLD_BATCH:
            v, mu = law.kld_inputs(n, batch, regime)
            value, gv64, _ = law.kld_f64(v, mu, batch, g)
            bound, gv_bound = law.kld_bound(v, mu, batch), law.kld_grad_v_bound(v, batch, g)
            v_d, mu_d = dev(v), dev(mu)
            note("fwd", abs(float(kld_forward(v_d, mu_d, batch)) - value) / bound, (n, batch))
            gv, gm = kld_backward(v_d, mu_d, batch, g)
            note("gv", np.max(np.abs(gv.astype(np.float64) - gv64) / gv_bound), (n, batch))
            if not same_bits(gm, law.kld_grad_mu_law(mu, batch, g)):
                wrong_mu.append((n, batch))
            # the yardstick: the reference's own expression in fp32 (torch on the CPU)
            tv, tm = torch.from_numpy(v), torch.from_numpy(mu)
            cpu = (0.5 * (torch.exp(tv) + torch.square(tm) - 1 - tv).sum() / batch).item()
            note("fwd_cpu_fp32", abs(cpu - value) / bound, (n, batch))
            cpu_gv = (0.5 * (torch.tensor(g) / batch) * (torch.exp(tv) - 1)).numpy()
            note("gv_cpu_fp32", np.max(np.abs(cpu_gv.astype(np.float64) - gv64) / gv_bound), (n, batch))
    print(f"PARITY kld bounded ({regime}): error / bound, worst of {len(law.KLD_N) * len(law.KLD_BATCH)} (n, batch) pairs: "
          f"forward {worst['fwd'][0]:.4f} at {worst['fwd'][1]} (torch CPU fp32: {worst['fwd_cpu_fp32'][0]:.4f}), "
          f"grad_explv {worst['gv'][0]:.4f} at {worst['gv'][1]} (torch CPU fp32: {worst['gv_cpu_fp32'][0]:.4f}); "
          f"grad_mu differs from the law in {len(wrong_mu)} (bit for bit)")
    assert worst["fwd"][0] <= 1.0 and worst["gv"][0] <= 1.0, worst
    assert not wrong_mu, wrong_mu[:5]


def test_kld_loss_takes_views_as_it_takes_their_copies():
    from hyperpocket_amd.ops import kld_loss
    v, mu = law.kld_inputs(128 * 64, 64, "workload")
    outs = []
    for copy in (False, True):
        vt, mt = dev(v).view(128, 64).t(), dev(mu).view(128, 64).t()
        assert not vt.is_contiguous()
        if copy:
            vt, mt = vt.contiguous(), mt.contiguous()
        vt.requires_grad_(True), mt.requires_grad_(True)
        k = kld_loss(vt, mt)
        (k * 3).backward()
        outs.append((k.detach().cpu().numpy().reshape(1), vt.grad.cpu().numpy(), mt.grad.cpu().numpy()))
    same = [same_bits(a, b) for a, b in zip(*outs)]
    value = law.kld_f64(v, mu, 64)[0]
    print(f"PARITY kld views: transposed (64, 128) views against their copies — value, grad_explv, grad_mu equal: {same}")
    assert all(same) and abs(float(outs[0][0][0]) - value) <= law.kld_bound(v, mu, 64)


# ---------------------------------------------------------------------------------------------------------------------
# step losses
# ---------------------------------------------------------------------------------------------------------------------
def test_step_losses_are_the_law_bit_for_bit():
    from hyperpocket_amd._lib import call, current_stream
    wrong, runs = [], 0
    for b in law.STEP_B:
        cd, kld, cost = law.step_inputs(b)
        cd_d, kld_d, cost_d = dev(np.array([cd])), dev(np.array([kld])), dev(cost)
        for with_kld in (True, False):
            for with_cost in (True, False):
                out = torch.full((4,), SENTINEL, device="cuda")
                call("hp_step_losses", b, cd_d, kld_d if with_kld else None, cost_d if with_cost else None,
                     law.STEP_C_CD, law.STEP_C_EMD, out, current_stream(out.device))
                want = law.step_losses_law(cd, kld if with_kld else None, cost if with_cost else None,
                                           law.STEP_C_CD, law.STEP_C_EMD)
                runs += 1
                if not same_bits(out.cpu().numpy(), want):
                    wrong.append((b, with_kld, with_cost, out.cpu().tolist(), want.tolist()))
    print(f"PARITY step losses: {runs} calls, b = 0 .. 64, kld / cost present or NULL: {len(wrong)} differ (bit for bit)")
    assert not wrong, wrong[:5]

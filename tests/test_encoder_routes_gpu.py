"""GPU parity of the encoder (csrc/model.hip: hp_encoder_forward / _backward_ld and the pair calls) on every launch route,
at the shapes where encoder_forward_impl and encoder_backward_impl change route.

The routes are named by hp_encoder_plan (the query answered by the functions those two decide with); the first test proves,
through it, that the case tables of tests/encoder_law.py reach every combination of routes the dispatch can produce.  Then
each case is held against the float64 evaluation of model/encoder.py:14-53 (encoder_law.encoder_law and its autograd) with the
bars the project already uses:

  forward   z, mu: 1e-5 (rtol + atol); exp(logvar): rtol 2e-5 — test_encoder_forward_backward_vs_oracle's;
            pooled g: 2e-6 of its scale, the rows at argidx: 4e-6 — against layer 5 in fp64 over the call's own h4, as
            test_conv_stack_split_f16_is_as_close_to_fp64_as_the_fp32_chain measures them
  backward  fp32 chain: 2e-4 of each gradient's scale (grad_close's default); f16 chain: e16 <= 2.5 e32 + 2e-7 scale, e32 the
            fp32 chain's error at the same case; each chain run twice, torch.equal
  pair      torch.equal with two single calls, every output and every parameter gradient
  ties      exact ties are built (and checked to be exact): the first point attaining the maximum wins on every route

Every figure is printed before it is asserted (pytest -s shows them; profiles/encoder_routes_parity.md records a run)."""
import functools

import pytest
import torch

import encoder_law as law
from test_model_gpu import close, grad_close

pytestmark = pytest.mark.gpu

OUT = 128


@functools.lru_cache(maxsize=None)
def _params(out_size, is_vae):
    return tuple(law.make_params(41 + out_size + int(is_vae), out_size, is_vae))


@functools.lru_cache(maxsize=None)
def _inputs(B, Np, out_size=OUT):
    g = torch.Generator().manual_seed(1000 * B + Np)
    return torch.rand(B, Np, 3, generator=g) - 0.5, torch.randn(B, out_size, generator=g)


@functools.lru_cache(maxsize=None)
def _law_forward(B, Np, is_vae):
    x, eps = _inputs(B, Np)
    with torch.no_grad():
        o = law.encoder_law([p.double() for p in _params(OUT, is_vae)], x.double(), eps.double())
    return {k: v for k, v in o.items() if k in ("z", "mu", "explv", "arg")}


@functools.lru_cache(maxsize=None)
def _law_grads(B, Np, is_vae, out_size=OUT, use=(True, True, True)):
    x, eps = _inputs(B, Np, out_size)
    return law.law_gradients(_params(out_size, is_vae), x, eps if is_vae else None, use)


def _names(n):
    names = [f"conv{l}.w" for l in range(1, 6)] + [f"conv{l}.b" for l in range(1, 6)] + ["fc.w", "fc.b", "mu.w", "mu.b", "std.w", "std.b"]
    return names[:n]


def _route_of(B, Np):
    return "fp32" if (B, Np) in law.FP32_ONLY else "default"


def test_cases_reach_every_plan():
    """The tables below reach every forward combination (conv format x fused pool x tile rows x tails) and every backward
    combination (fused | layered x row ranges x tails) hp_encoder_plan can report, each listed boundary from both sides; the
    combinations no case reaches are those the dispatch cannot produce (encoder_law.FORWARD_UNREACHABLE, with the reasons)."""
    law.check_cases_reach_every_route()
    assert len(law.FORWARD_UNREACHABLE) == 3


# ------------------------------------------------------------------------------------------------ a. forward
@pytest.mark.parametrize("is_vae", [True, False], ids=["vae", "plain"])
@pytest.mark.parametrize("route,B,Np", law.routes_of(law.ALL_CASES), ids=lambda v: str(v))
def test_forward_matches_fp64_on_every_route(route, B, Np, is_vae):
    x, eps = _inputs(B, Np)
    params = _params(OUT, is_vae)
    split, presplit = law.CONV_ROUTES[route]
    with law.switches(split, presplit):
        plan = law.plan_of(route, B, Np, is_vae=(is_vae,))
        s = law.Side(B, Np, OUT, x, params, eps if is_vae else None).forward()
        got = s.outputs()
        hs = s.hidden()
    want = _law_forward(B, Np, is_vae)
    # layer 5 and the pool in fp64 over the call's own h4: the pooled value, and the row the call names must attain it
    P = [p.cuda().double() for p in s.params]
    h5 = (hs[3].double() @ P[4].t() + P[9]).view(B, Np, 512)
    want_g = h5.max(dim=1)[0]
    scale = want_g.abs().max().item()
    arg = got["argidx"].long()
    assert arg.min().item() >= 0 and arg.max().item() < Np
    e_g = (got["g"].double() - want_g).abs().max().item()
    e_arg = (torch.gather(h5, 1, arg.unsqueeze(1)).squeeze(1) - want_g).abs().max().item()
    e_mu, s_mu = law.err_of_scale(got["mu"], want["mu"])
    print(f"PARITY fwd {route} B={B} Np={Np} {'vae' if is_vae else 'plain'} {law.forward_combo(plan)}: g {e_g / scale:.2e} "
          f"argrow {e_arg / scale:.2e} mu {e_mu:.2e} (scale {s_mu:.2e})", end="")
    if is_vae:
        e_z, _ = law.err_of_scale(got["z"], want["z"])
        rel = ((got["explv"].double().cpu() - want["explv"]).abs() / want["explv"].abs()).max().item()
        print(f" z {e_z:.2e} explv rel {rel:.2e}", end="")
    print()
    assert e_g <= 2e-6 * scale, "g"
    assert e_arg <= 4e-6 * scale, "argidx"
    close(got["mu"], want["mu"])
    if is_vae:
        close(got["z"], want["z"])
        close(got["explv"], want["explv"], rtol=2e-5)


# ------------------------------------------------------------------------------------------------ b. backward
# The forward takes discrete decisions: which point a channel's maximum names, and on which side of zero a pre-activation
# lies.  Where float64 puts a pre-activation of a critical row within fp32 rounding of zero, any fp32 forward may mask it the
# other way, and that row's delta then enters (or leaves) one layer's weight and bias gradient whole — a difference of one
# term, not of rounding.  Two cases hit this ON THE fp32 ROUTE (fp32 GEMM conv stack, fp32 chain: the reference measurement),
# both chains alike, with every row named as the law names it:
#   (64, 192): the law has a layer-4 pre-activation of +2.4e-9 with dL/dh = -0.33303 at a critical row; the call masks it out:
#              conv4.b is off by 0.33305 = 3.05e-4 of its scale, conv4.w by 2.60e-4
#   (96, 128): a layer-3 pre-activation of +2.4e-9 with dL/dh = 0.30985: conv3.w is off by 2.33e-4 of its scale
# (found by listing the law's critical pre-activations below 3e-6 next to their dL/dh; at B >= 64 there are ~80 of them per
# layer and the smallest is expected around 1e-9).  As the fp32 route misses grad_close's 2e-4 there, the bar against the law
# at these two shapes is that measured error times the project's 2.5x margin (profiles/encoder_routes_parity.md); every other
# case keeps 2e-4.  Against the law differentiated AT THE CALL'S OWN DECISIONS (the rows it named, which
# test_forward_matches_fp64_on_every_route holds to the maximum within 4e-6, and the signs of its stored h1..h4) every case keeps
# every bar.
MOVED_FP32_BARS = {(64, 192): 2.5 * 3.05e-4, (96, 128): 2.5 * 2.33e-4}


def _assert_backward_bars(tag, route, run, want, chains=(1, 0), at=None, bar=2e-4):
    """run() -> (outputs, gradients) under the current switches; want: the law's gradients; at(argidx, masks) -> the law's
    gradients at the call's own rows and ReLU masks.  Both chains twice; the bars of the module docstring — `bar` (the fp32
    chain's, 2e-4 unless moved) against `want`, 2e-4 against at(...)."""
    split, presplit = law.CONV_ROUTES[route]
    got, arg = {}, None
    for c in chains:
        with law.switches(split, presplit, chain16=c):
            (o, a), (_, b) = run(), run()
            got[c], arg, masks = (a, b), o["argidx"], o.get("masks")
    refs = [("law", want, bar)] + ([("law at the call's decisions", at(arg, masks), 2e-4)] if at is not None else [])
    fails, line = [], []
    for what, ref, fp32_bar in refs:
        worst = {c: 0.0 for c in chains}
        for i, (k, w) in enumerate(zip(_names(len(ref)), ref)):
            errs = {}
            for c in chains:
                assert torch.equal(got[c][0][i], got[c][1][i]), (tag, k, "chain16", c, "two runs differ")
                assert tuple(got[c][0][i].shape) == tuple(w.shape)
                errs[c], scale = law.err_of_scale(got[c][0][i], w)
                worst[c] = max(worst[c], errs[c] / max(scale, 1e-30))
            if 0 in errs and errs[0] > fp32_bar * max(scale, 1e-30):
                fails.append((what, k, "fp32 chain", errs[0], scale))
            if 0 in errs and 1 in errs and errs[1] > 2.5 * errs[0] + 2e-7 * scale:
                fails.append((what, k, "f16 chain", errs[1], errs[0], scale))
            if 0 not in errs and errs[1] > fp32_bar * max(scale, 1e-30):      # the layered sequence: no f16 chain, the fp32 bar
                fails.append((what, k, "layered", errs[1], scale))
        line.append(f"vs {what}: " + " ".join(f"chain16={c} {worst[c]:.2e}" for c in chains))
    print(f"PARITY bwd {tag} {route}: worst error / scale " + " | ".join(line))
    assert not fails, (tag, fails)
    return {c: v for c, v in got.items()}


def _flips(route, B, Np, is_vae=True):
    """Rows the forward names differently from the float64 law (near-ties), for the record."""
    split, presplit = law.CONV_ROUTES[route]
    x, eps = _inputs(B, Np)
    with law.switches(split, presplit):
        arg = law.Side(B, Np, OUT, x, _params(OUT, is_vae), eps if is_vae else None).forward().outputs()["argidx"]
    return int((arg.cpu().long() != _law_forward(B, Np, is_vae)["arg"]).sum())


@pytest.mark.parametrize("B,Np", law.ALL_CASES, ids=lambda v: str(v))
def test_backward_matches_fp64_on_both_chains(B, Np):
    x, eps = _inputs(B, Np)
    route = _route_of(B, Np)
    params = _params(OUT, True)
    tag = f"B={B} Np={Np} vae S={law.plan_of(route, B, Np)['bwd_splits']} rows named differently {_flips(route, B, Np)}/{B * 512}"
    _assert_backward_bars(tag, route, lambda: law.single(B, Np, OUT, x, params, eps), _law_grads(B, Np, True),
                          at=lambda arg, masks: law.law_gradients(params, x, eps, arg=arg, masks=masks),
                          bar=MOVED_FP32_BARS.get((B, Np), 2e-4))


@pytest.mark.parametrize("B,Np", [(1, 128), (21, 100), (65, 128)], ids=lambda v: str(v))
def test_backward_of_a_plain_encoder_with_only_grad_out(B, Np):
    x, _ = _inputs(B, Np)
    params = _params(OUT, False)
    _assert_backward_bars(f"B={B} Np={Np} plain", "default", lambda: law.single(B, Np, OUT, x, params), _law_grads(B, Np, False),
                          at=lambda arg, masks: law.law_gradients(params, x, arg=arg, masks=masks))


# ------------------------------------------------------------------------------------------------ c. pair == two singles
def _assert_same(a, b, what):
    for z in (0, 1):
        for k in a[z][0]:
            assert torch.equal(a[z][0][k], b[z][0][k]), (what, "encoder", z, k)
        for k, ga, gb in zip(_names(len(a[z][1])), a[z][1], b[z][1]):
            assert not torch.isnan(ga).any(), (what, "encoder", z, k, "unwritten")
            assert torch.equal(ga, gb), (what, "encoder", z, k)


@pytest.mark.parametrize("chain16", [1, 0], ids=["f16chain", "fp32chain"])
@pytest.mark.parametrize("split", [1, 0], ids=["split", "fp32conv"])
@pytest.mark.parametrize("B,Np", law.PAIR_CASES, ids=lambda v: str(v))
def test_pair_equals_two_single_calls_bit_for_bit(B, Np, split, chain16):
    """VAE + plain encoder as EncoderPairFunction lays them out (the plain one's mu in the latent's second column block, the halves
    of d latent read in place): every output and every parameter gradient of the pair calls equals the single calls' — with
    separately allocated buffers, and with everything carved from ONE allocation in reverse order (encoder 1's inputs,
    weights, outputs, workspaces and gradients below encoder 0's: the batched launches' strides are negative)."""
    x0, eps = _inputs(B, Np)
    x1 = _inputs(B + 1, Np)[0][1:]
    p0, p1 = _params(OUT, True), _params(OUT, False)
    with law.switches(split, 1, chain16=chain16):
        plan = law.plan_of("default" if split else "fp32", B, Np, is_vae=(True, False), ld=2 * OUT)
        assert plan["bwd_fused"] and plan["bwd_tails_skinny"] == (B <= 64, B <= 64)
        ones = law.pair_as_singles(B, Np, OUT, x0, p0, eps, x1, p1)
        two = law.pair(B, Np, OUT, x0, p0, eps, x1, p1)
        _assert_same(two, ones, "pair")
        back = law.pair(B, Np, OUT, x0, p0, eps, x1, p1, reverse=True, alloc=law.Arena(law.pair_arena_bytes(B, Np, OUT)))
        _assert_same(back, ones, "pair, reverse order")


# ------------------------------------------------------------------------------------------------ d. arg-max ties
def _tie_cloud(kind, Np, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "point":
        return (torch.rand(1, 3, generator=g) - 0.5).expand(Np, 3).clone()
    if kind == "halves":
        h = torch.rand(Np // 2, 3, generator=g) - 0.5
        return torch.cat([h, h])
    return torch.rand(Np, 3, generator=g) - 0.5


# (route, Np, the clouds of the batch).  Halves of whole 128-point tiles: whole tiles repeat, so the per-tile scales of the split
# routes agree; on the fp32 route no per-tile scale exists and any half will do.  Np = 200 and 37 end colmax_kernel's four row
# segments (50 / 10 rows each) inside the cloud.
TIE_CASES = [
    ("default", 256, ("halves",)), ("default", 1024, ("halves",)),                 # fused pool: ties across tiles
    ("default", 128, ("point",)), ("default", 1024, ("point",)),                   # ... within a tile and across tiles
    ("default", 256, ("halves", "point", "plain")),                                # a batch that mixes both with an ordinary cloud
    ("r3", 256, ("halves", "point", "plain")),
    ("fp32", 256, ("halves", "point", "plain")),                                   # fused pool, 64-row tiles
    ("fp32", 200, ("point",)), ("fp32", 200, ("halves", "point", "plain")),        # colmax_kernel: ties across its segments
    ("fp32", 37, ("point",)),
    ("default", 200, ("point",)), ("default", 37, ("point", "plain")),             # ... behind the ragged split route
]


@pytest.mark.parametrize("route,Np,kinds", TIE_CASES, ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_first_point_wins_arg_max_ties_on_every_route(route, Np, kinds):
    """colmax_kernel and colmax_tiles_kernel (and the COLMAX epilogues before the latter) promise the FIRST point attaining a
    channel's maximum.  Premise, asserted: the repeated points' h4 rows come back bit-equal, so their h5 values tie exactly."""
    B = len(kinds)
    x = torch.stack([_tie_cloud(k, Np, 7 + i) for i, k in enumerate(kinds)])
    eps = _inputs(B, Np)[1]
    params, plain = _params(OUT, True), _params(OUT, False)
    split, presplit = law.CONV_ROUTES[route]
    with law.switches(split, presplit):
        plan = law.plan_of(route, B, Np)
        assert plan["pool_fused"] == (Np % plan["tile_rows"] == 0)
        runs = [law.Side(B, Np, OUT, x, params, eps).forward() for _ in range(2)]
        outs = [r.outputs() for r in runs]
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), (k, "two runs differ")
        h4 = runs[0].hidden()[3].view(B, Np, 512)
        arg = outs[0]["argidx"].cpu()
        for b, kind in enumerate(kinds):
            if kind == "point":
                assert torch.equal(h4[b], h4[b, :1].expand(Np, 512)), "invalid case: the repeated point's rows differ"
                assert (arg[b] == 0).all(), (kind, arg[b].unique().tolist())
            elif kind == "halves":
                assert torch.equal(h4[b, :Np // 2], h4[b, Np // 2:]), "invalid case: the repeated half's rows differ"
                assert (arg[b] < Np // 2).all(), (kind, arg[b].max().item())
        # the pair call chooses the same rows (and computes the same outputs) as the single call
        two = law.pair(B, Np, OUT, x, params, eps, x, plain)
        for k in outs[0]:
            assert torch.equal(two[0][0][k], outs[0][k]), ("pair", k)
        assert torch.equal(two[1][0]["argidx"], law.Side(B, Np, OUT, x, plain, None).forward().outputs()["argidx"])
    # gradients of the tie clouds: the bars of the backward tests (the law's max sends a channel's gradient to ONE of the equal
    # rows; which one does not matter to a parameter gradient), and merged critical rows equal per-channel rows
    want = law.law_gradients(params, x, eps)
    run = lambda: law.single(B, Np, OUT, x, params, eps)
    got = _assert_backward_bars(f"ties {'+'.join(kinds)} Np={Np}", route, run, want)
    with law.switches(split, presplit, chain16=1):
        per_channel = law.single(B, Np, OUT, x, params, eps, dedup=0)[1]
    for k, a, b in zip(_names(16), got[1][0], per_channel):
        grad_close(a, b, tol=2e-5)


# ------------------------------------------------------------------------------------------------ e. fall-backs
@pytest.mark.parametrize("case", law.FALLBACK_CASES, ids=lambda c: c[0])
def test_backward_fallbacks_match_fp64(case):
    """Each fall-back is first shown to be one (hp_encoder_plan), then held to the backward bars.  The layered sequence has no
    f16 chain: it is held to the fp32 bar alone.  unaligned: the backward's workspace and the forward's (a copy of it, brought
    to fp32 rows first) start one float past a 16-byte boundary; its gradients also agree with the aligned call's."""
    name, B, Np, out, vae, pad, aligned, says = case
    x, eps = _inputs(B, Np, out)
    params = _params(out, vae)
    plan = law.plan_of("default", B, Np, out, (vae,), ld=out + pad, aligned=aligned)
    for k, v in says.items():
        assert plan[k] == v, (k, plan)
    want = _law_grads(B, Np, vae, out)

    def run():
        if aligned:
            return law.single(B, Np, out, x, params, eps if vae else None, ld=out + pad)
        s = law.Side(B, Np, out, x, params, eps).forward()
        o = s.outputs()
        s.hidden()
        moved = law._off16(law.fresh, s.ws.numel(), 1)
        assert moved.data_ptr() % 16 == 4
        moved.copy_(s.ws)
        gz, gmu, gex = law.upstream(B, out)
        return o, s.backward(gz, None, gmu, gex, fwd_ws=moved, ws_off=1)

    got = _assert_backward_bars(name, "default", run, want, chains=(1, 0) if plan["bwd_fused"] else (1,))
    if not aligned:
        fused = law.single(B, Np, out, x, params, eps)[1]
        for a, b in zip(got[1][0], fused):
            grad_close(a, b, tol=2e-5)


def test_backward_of_a_vae_encoder_with_only_the_kld_gradients():
    """grad_out = NULL, grad_mu and grad_explv alone (the KLD term's gradient): fused and layered."""
    B, Np = 3, 128
    x, eps = _inputs(B, Np)
    params = _params(OUT, True)
    want = _law_grads(B, Np, True, OUT, (False, True, True))

    def run(dedup=1):
        s = law.Side(B, Np, OUT, x, params, eps).forward()
        _, gmu, gex = law.upstream(B, OUT, use=(False, True, True))
        return s.outputs(), s.backward(None, None, gmu, gex, dedup=dedup)

    assert law.plan_of("default", B, Np)["bwd_fused"] and not law.plan_of("default", B, Np, dedup=False)["bwd_fused"]
    _assert_backward_bars("kld only", "default", run, want)
    _assert_backward_bars("kld only, layered", "default", lambda: run(0), want, chains=(1,))

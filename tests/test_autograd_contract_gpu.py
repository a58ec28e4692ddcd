"""GPU suite: the autograd nodes (ops.EncoderFunction, EncoderPairFunction, HyperNetFunction, TargetNetworkFunction,
KLDFunction, losses._ChamferFunction, NNDistanceFunction, MatchCostFunction) and the gradient-placement registry
(ops._grad_buffer) held to autograd's contract under accumulation, weight sharing, replay, partial use, odd layouts,
inputs that require grad, double backward and frozen sub-networks.

Reference: the float64 evaluation of oracle/hyperpocket_ref.py with double leaves on the CPU; match_cost through the C
oracle as tests/test_structural_losses_gpu.py does (cost rtol 1e-5; gradients atol 5e-5, rtol 1e-3: that file's bars for
this operation).  Bars: test_model_gpu's `close` (1e-5) for forward values, `grad_close` (2e-4 of each gradient's scale)
for parameter and input gradients; torch.equal where two GPU results are the same computation (the kernels are
run-to-run identical: test_train_engine_steps_are_bit_identical_run_to_run).  Every figure is printed before it is
asserted (pytest -s shows them; profiles/autograd_contract.md records one run).

Routes: "plain" — plain parameters, fresh gradient tensors; "flat" — FlatParameters registered through
FlatAdam(model, fuse_heads=False); "fused" — FlatAdam's default, where it applies (one backward per step).

Shapes: the smallest that take every route — encoders at B=3, Np=128 (pair node, fused backward) and at B=2 with 100
existing / 128 missing points (two nodes on two streams, ragged tiles), the hypernetwork at its published size
(19011 x 2048 heads) with B=3, the decoder on 64 points, the losses at (b, n, m) = (3, 64, 64) and (2, 100, 37).

Premise of the accumulation and sharing cases: before any GPU result is judged, the float64 gradients themselves show
that each wrong answer a broken placement gives (2*g2, g1 alone, g2 alone) lies at least ten bars from g1 + g2.
"""
import types

import numpy as np
import pytest
import torch

from test_model_gpu import build_model, close

pytestmark = pytest.mark.gpu

OUT = 128
BAR = 2e-4
SHAPES = {"pair": dict(B=3, n_ex=128, n_mi=128), "two_node": dict(B=2, n_ex=100, n_mi=128)}
LOSS_SHAPES = [(3, 64, 64), (2, 100, 37)]


# ------------------------------------------------------------------------------------------------ figures
def _scale_err(got, want):
    """grad_close's figure: max|got - want| over the scale max|want| (floored at 1e-30)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def _grads_meet(tag, got, want, bar=BAR):
    """grad_close (test_model_gpu: max|got - want| <= bar * max|want|) over a dict, every figure printed first.
    got / want: name -> gradient (None: the loss does not reach it; then asserted None, never skipped)."""
    figures = {}
    for n, w in want.items():
        if w is None:
            assert got[n] is None, f"{tag}: {n} has a gradient the loss cannot reach"
            continue
        assert got[n] is not None, f"{tag}: {n} has no gradient"
        figures[n] = _scale_err(got[n], w)
        print(f"{tag:44s} {n:40s} err/scale {figures[n]:.3e}")
    worst = max(figures, key=figures.get)
    print(f"{tag:44s} WORST {worst} {figures[worst]:.3e} (bar {bar:.0e})")
    for n, e in figures.items():
        assert e <= bar, f"{tag}: {n}: max err {e:.3e} of scale (bar {bar:.0e})"


def _premise(tag, want, wrongs):
    """float64 only: each wrong answer lies at least ten bars from the right one, for every tensor compared."""
    for n, w in want.items():
        if w is None:
            continue
        scale = w.abs().max().item()
        for what, g in wrongs.items():
            d = (g[n] - w).abs().max().item() / scale
            assert d >= 10 * BAR, f"{tag}: {what} is only {d:.2e} of scale from the right {n}: the case cannot tell them apart"


def _sum(g1, g2):
    return {n: None if g1[n] is None else g1[n] + g2[n] for n in g1}


def _scaled(g, c):
    return {n: None if v is None else c * v for n, v in g.items()}


# ------------------------------------------------------------------------------------------------ the model, its routes
def _batch(seed, B, n_ex, n_mi, N=64):
    g = torch.Generator().manual_seed(seed)
    ex, mi = torch.rand(B, n_ex, 3, generator=g) - 0.5, torch.rand(B, n_mi, 3, generator=g) - 0.5
    pts = torch.rand(B, N, 3, generator=g) * 2 - 1
    eps = torch.randn(B, OUT, generator=g)
    return types.SimpleNamespace(seed=seed, ex=ex, mi=mi, gt=torch.cat([ex, mi], 1), pts=pts, eps=eps)


def _P64(state, prefix=""):
    return {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in state.items() if k.startswith(prefix)}


def _grads_of(P):
    return {k: p.grad for k, p in P.items()}


def _oracle_step(ref, state, b):
    """(loss, name -> float64 gradient) of 0.05 * Chamfer + KLD at `state` for batch b."""
    P = _P64(state)
    rec, explv, mu, _ = ref.full_forward(P, b.ex.double(), b.mi.double(), b.pts.double(), b.eps.double())
    loss = 0.05 * ref.chamfer_loss(b.gt.double(), rec.permute(0, 2, 1)) \
        + 0.5 * (torch.exp(explv) + torch.square(mu) - 1 - explv).sum() / b.ex.shape[0]
    loss.backward()
    return loss.item(), _grads_of(P)


@pytest.fixture(scope="module")
def world(ref):
    from hyperpocket_amd import ops
    model = build_model(4242).train()
    w = types.SimpleNamespace(model=model, ref=ref, cache={},
                              state0={k: v.detach().clone() for k, v in model.state_dict().items()})

    def oracle(b, shape):
        if (b.seed, shape) not in w.cache:
            w.cache[(b.seed, shape)] = _oracle_step(ref, w.state0, b)
        return w.cache[(b.seed, shape)]
    w.oracle = oracle
    yield w
    ops.clear_grad_views()


def _route(w, route, frozen=()):
    """The module's one model, back at its first state, on `route`; returns the FlatAdam (None on "plain")."""
    from hyperpocket_amd import ops
    from hyperpocket_amd.optim import FlatAdam
    ops.clear_grad_views()
    m = w.model
    m.hyper_network._heads_exchange = None
    for p in torch.nn.Module.parameters(m):
        p.requires_grad_(True)
        p.grad = None
    m.load_state_dict(w.state0)
    m.train()
    for name in frozen:
        getattr(m, name).requires_grad_(False)
    if route == "plain":
        return None
    return FlatAdam(m, lr=1e-4, fuse_heads=(route == "fused"))


def _clear(w, opt):
    if opt is not None:
        opt.zero_grad()
    else:
        for p in torch.nn.Module.parameters(w.model):
            p.grad = None


def _named_grads(m, prefix=""):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in torch.nn.Module.named_parameters(m)
            if n.startswith(prefix)}


def _gpu_loss(m, b, node=None):
    from hyperpocket_amd import ops
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    dev = torch.device("cuda")
    gt = b.gt.cuda()
    rec, explv, mu = m(b.ex.cuda().clone(), b.mi.cuda().clone(), list(gt.shape), 1, dev, points=b.pts.cuda(), eps=b.eps.cuda())
    if node is not None:
        assert type(m._last_latent.grad_fn).__name__.startswith(node), type(m._last_latent.grad_fn).__name__
    return 0.05 * ChamferLoss()(gt, rec.permute(0, 2, 1)) + ops.kld_loss(explv, mu)


NODE_OF = {"pair": "EncoderPairFunction", "two_node": "Cat"}


# ------------------------------------------------------------------------------------------------ A. accumulation
@pytest.mark.parametrize("shape", ["pair", "two_node"])
def test_accumulation_two_backwards_without_clearing(world, shape):
    """g1 + g2 against float64 on routes plain and flat, bit-equal to the fp32 sum of the two single-backward gradients;
    then one Adam step on the accumulated pair: FlatAdam(fuse_heads=False) against torch.optim.Adam, at the bars of
    test_dropin_route_equals_engine_and_flat_adam_equals_torch_adam scaled from its three steps to one (tol = 2e-6 max|w| +
    1e-5, share over tol <= 1e-4, largest <= 6.1e-4 / 3, mean <= 1e-7)."""
    m = world.model
    b1, b2 = _batch(11, **SHAPES[shape]), _batch(12, **SHAPES[shape])
    (l1, g1), (l2, g2) = world.oracle(b1, shape), world.oracle(b2, shape)
    want = _sum(g1, g2)
    assert want["real_encoder.std_layer.weight"] is None and want["random_encoder.std_layer.weight"] is not None
    _premise(f"A {shape}", want, {"2*g2": _scaled(g2, 2), "g1 alone": g1, "g2 alone": g2})
    after = {}
    for route in ("plain", "flat"):
        opt = _route(world, route)
        singles = []
        for b, l in ((b1, l1), (b2, l2)):
            _clear(world, opt)
            loss = _gpu_loss(m, b, NODE_OF[shape])
            print(f"A {shape} {route}: loss {loss.item():.8g} (float64 {l:.8g})")
            close(loss, np.float64(l))
            loss.backward()
            singles.append(_named_grads(m))
        _clear(world, opt)
        _gpu_loss(m, b1).backward()
        _gpu_loss(m, b2).backward()
        got = _named_grads(m)
        _grads_meet(f"A {shape} {route} g1+g2", got, want)
        for n, g in got.items():
            if g is not None:
                assert torch.equal(g, singles[0][n] + singles[1][n]), f"A {shape} {route}: {n} is not the fp32 sum of its two gradients"
        if opt is not None:          # the sum landed in the flat slice: the step finds it in place
            for p, ptr in zip(opt.flat.params, opt._grad_ptrs):
                assert p.grad is None or p.grad.data_ptr() == ptr
        (opt or torch.optim.Adam(m.parameters(), lr=1e-4)).step()
        torch.cuda.synchronize()
        after[route] = {n: p.detach().clone() for n, p in torch.nn.Module.named_parameters(m)}
    for n, w in after["plain"].items():
        d = (after["flat"][n] - w).abs()
        tol = 2e-6 * w.abs().max().item() + 1e-5
        share, largest, mean = (d > tol).float().mean().item(), d.max().item(), d.mean().item()
        print(f"A {shape} Adam step, flat vs torch {n:40s} share {share:.2e} max {largest:.3e} mean {mean:.3e}")
        assert share <= 1e-4 and largest <= 6.1e-4 / 3 and mean <= 1e-7, (n, share, largest, mean)
        moved = (w - world.state0[n]).abs().max().item()
        assert moved > 0 or g1[n] is None, n


@pytest.mark.parametrize("route", ["flat", "fused"])
def test_in_place_zero_grad_between_two_ordinary_steps(world, route):
    """model.zero_grad(set_to_none=False) leaves every .grad set (zeroed in place): the next backward must add onto the
    zeros, not write the slice and add it onto itself.  The second step's gradients, read before step(), against float64
    at the parameters the first step left."""
    m = world.model
    opt = _route(world, route)
    b1, b2 = _batch(11, **SHAPES["pair"]), _batch(12, **SHAPES["pair"])
    opt.zero_grad()
    _gpu_loss(m, b1).backward()
    opt.step()
    m.zero_grad(set_to_none=False)
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    loss = _gpu_loss(m, b2)
    loss.backward()
    got = _named_grads(m)
    opt.step()
    torch.cuda.synchronize()
    l, want = _oracle_step(world.ref, state, b2)
    if route == "fused":             # the heads' weight gradient is never stored on this route
        want = {n: (None if n.startswith("hyper_network.output") and n.endswith(".weight") else g) for n, g in want.items()}
    print(f"A zero_grad(set_to_none=False) {route}: loss {loss.item():.8g} (float64 {l:.8g})")
    close(loss, np.float64(l))
    _grads_meet(f"A zero_grad(set_to_none=False) {route}", got, want)      # (2*g is 5000 bars from g)


def test_ordinary_iterations_stay_copy_free(world):
    """After an ordinary FlatAdam iteration and an ordinary TrainEngine.step every trained parameter's .grad is its slice
    of the flat gradient buffer — on the first iteration and on the ones after it."""
    from hyperpocket_amd.core.engine import TrainEngine
    m = world.model
    b = _batch(11, **SHAPES["pair"])
    for route in ("flat", "fused"):
        opt = _route(world, route)
        for it in range(3):
            opt.zero_grad()
            _gpu_loss(m, b).backward()
            opt.step()
            n = 0
            for p, ptr in zip(opt.flat.params, opt._grad_ptrs):
                assert p.grad is None or p.grad.data_ptr() == ptr, (route, it)
                n += p.grad is not None
            assert n >= len(opt.flat.params) - 7, (route, it, n)      # all but real_encoder.std_layer and (fused) the 5 heads
    _route(world, "plain")
    b = _batch(11, N=256, **SHAPES["pair"])          # the engine's losses want as many decoded points as gt has
    eng = TrainEngine(m)
    try:
        for it in range(3):
            eng.step(b.ex.cuda(), b.mi.cuda(), b.gt.cuda(), 1, points=b.pts.cuda(), eps_noise=b.eps.cuda())
            n = 0
            for p, o in zip(eng.flat.params, eng.flat.offsets):
                assert p.grad is None or p.grad.data_ptr() == eng.flat.grad.data_ptr() + 4 * o, it
                n += p.grad is not None
            assert n >= len(eng.flat.params) - 7, (it, n)
        eng.synchronize()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ node-level helpers
def _weights(seed, *shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in shapes]


def _cloud(seed, B, Np):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, Np, 3, generator=g) - 0.5, torch.randn(B, OUT, generator=g)


def _dot(outs, ws, use=(True, True, True, True)):
    return sum((o * w.to(o)).sum() for o, w, u in zip(outs, ws, use) if u)


def _enc64(ref, P, prefix, x, eps):
    return ref.encoder_forward(P, prefix, x.double(), True, eps.double())


def _enc_gpu(enc, x, eps):
    return enc(x.cuda().transpose(1, 2), eps.cuda())          # the channels-first view FullModel makes


def _outputs_close(tag, outs, outs64, names=("z", "mu", "explv")):
    """Forward values at `close`; exp(logvar) at the rtol test_encoder_forward_backward_vs_oracle gives it (2e-5)."""
    for name, o, o64 in zip(names, outs, outs64):
        print(f"{tag:44s} {name:40s} err/scale {_scale_err(o, o64):.3e}")
        close(o, o64.detach(), rtol=2e-5 if name == "explv" else 1e-5)


def _oracle_of(P, loss):
    for p in P.values():
        p.grad = None
    loss.backward()
    return loss.item(), _grads_of(P)


# ------------------------------------------------------------------------------------------------ B. weight sharing
@pytest.mark.parametrize("route", ["plain", "flat"])
def test_encoder_applied_to_two_batches_in_one_graph(world, route):
    m, ref = world.model, world.ref
    (xa, ea), (xb, eb) = _cloud(21, 3, 128), _cloud(22, 3, 128)
    wsa, wsb = _weights(23, (3, OUT), (3, OUT), (3, OUT)), _weights(24, (3, OUT), (3, OUT), (3, OUT))
    P = _P64(world.state0, "random_encoder.")
    oa, ob = _enc64(ref, P, "random_encoder", xa, ea), _enc64(ref, P, "random_encoder", xb, eb)
    _, ga = _oracle_of(P, _dot(oa, wsa))
    _, gb = _oracle_of(P, _dot(ob, wsb))
    want = _sum(ga, gb)
    _premise("B encoder", want, {"2*gB": _scaled(gb, 2), "2*gA": _scaled(ga, 2), "gA alone": ga, "gB alone": gb})
    opt = _route(world, route)
    _clear(world, opt)
    da, db = _enc_gpu(m.random_encoder, xa, ea), _enc_gpu(m.random_encoder, xb, eb)
    _outputs_close(f"B encoder twice {route} A", da, oa)
    _outputs_close(f"B encoder twice {route} B", db, ob)
    (_dot(da, wsa) + _dot(db, wsb)).backward()
    _grads_meet(f"B encoder twice {route}", _named_grads(m, "random_encoder."), want)


@pytest.mark.parametrize("route", ["plain", "flat"])
def test_hypernetwork_applied_to_two_latents_in_one_graph(world, route):
    m, ref = world.model, world.ref
    la_, lb_, wa, wb = _weights(31, (3, 2 * OUT), (3, 2 * OUT), (3, 19011), (3, 19011))
    P = _P64(world.state0, "hyper_network.")
    lat = [t.double().requires_grad_(True) for t in (la_, lb_)]
    ta, tb = ref.hypernet_forward(P, lat[0]), ref.hypernet_forward(P, lat[1])
    _, ga = _oracle_of(P, (ta * wa.double()).sum())
    _, gb = _oracle_of(P, (tb * wb.double()).sum())
    want = _sum(ga, gb)
    _premise("B hypernetwork", want, {"2*gB": _scaled(gb, 2), "2*gA": _scaled(ga, 2), "gA alone": ga, "gB alone": gb})
    opt = _route(world, route)
    _clear(world, opt)
    dl = [t.cuda().requires_grad_(True) for t in (la_, lb_)]
    da, db = m.hyper_network(dl[0]), m.hyper_network(dl[1])
    _outputs_close(f"B hypernetwork twice {route}", (da, db), (ta, tb), ("theta A", "theta B"))
    ((da * wa.cuda()).sum() + (db * wb.cuda()).sum()).backward()
    got = _named_grads(m, "hyper_network.")
    got.update({"latent A": dl[0].grad, "latent B": dl[1].grad})
    want.update({"latent A": lat[0].grad, "latent B": lat[1].grad})
    _grads_meet(f"B hypernetwork twice {route}", got, want)


def _theta(seed, B=3):
    return _weights(seed, (B, 19011))[0] * 0.1


def _target64(ref, theta, pts):
    return torch.stack([ref.target_forward(theta[j], pts[j].double()) for j in range(theta.shape[0])])


@pytest.mark.parametrize("fused", [True, False])
def test_decoder_on_one_theta_with_two_point_sets(world, fused):
    from hyperpocket_amd import ops
    from hyperpocket_amd.model.target_network import target_network_batched
    ref, cfg = world.ref, world.model.target_network_config
    th = _theta(41)
    pa, pb, wa, wb = _weights(42, (3, 64, 3), (3, 64, 3), (3, 64, 3), (3, 64, 3))
    pa, pb = pa.clamp(-1, 1), pb.clamp(-1, 1)
    t64 = th.double().requires_grad_(True)
    ga, = torch.autograd.grad((_target64(ref, t64, pa) * wa.double()).sum(), t64)
    gb, = torch.autograd.grad((_target64(ref, t64, pb) * wb.double()).sum(), t64)
    want = {"theta": ga + gb}
    _premise("B decoder", want, {"2*gB": {"theta": 2 * gb}, "2*gA": {"theta": 2 * ga}, "gA": {"theta": ga}, "gB": {"theta": gb}})
    was, ops.FUSED_TARGET_NETWORK = ops.FUSED_TARGET_NETWORK, fused
    try:
        t = th.cuda().requires_grad_(True)
        ya, yb = target_network_batched(cfg, t, pa.cuda()), target_network_batched(cfg, t, pb.cuda())
        _outputs_close(f"B decoder fused={fused}", (ya, yb), (_target64(ref, t64, pa), _target64(ref, t64, pb)), ("y A", "y B"))
        ((ya * wa.cuda()).sum() + (yb * wb.cuda()).sum()).backward()
        _grads_meet(f"B decoder one theta, two point sets fused={fused}", {"theta": t.grad}, want)
    finally:
        ops.FUSED_TARGET_NETWORK = was


# ------------------------------------------------------------------------------------------------ C. replay
@pytest.mark.parametrize("route", ["plain", "flat"])
@pytest.mark.parametrize("node,B,Np", [("single", 3, 128), ("single", 2, 100), ("pair", 3, 128)])
def test_encoder_second_backward_through_a_retained_graph(world, route, node, B, Np):
    """The first backward drops the forward's workspace: the second one recomputes the critical rows.  It is the same
    computation as one backward with ops.KEEP_ENCODER_ACTIVATIONS = False, bit for bit; both runs meet float64."""
    from hyperpocket_amd import ops
    m, ref = world.model, world.ref
    (x0, eps), (x1, _) = _cloud(51, B, Np), _cloud(52, B, Np)
    ws = _weights(53, (B, OUT), (B, OUT), (B, OUT), (B, OUT))
    P = _P64(world.state0, "r")
    if node == "single":
        prefix = "random_encoder."
        o64 = _enc64(ref, P, "random_encoder", x0, eps)

        def build():
            return _enc_gpu(m.random_encoder, x0, eps)
    else:
        prefix = "r"
        o64 = _enc64(ref, P, "random_encoder", x0, eps) + (ref.encoder_forward(P, "real_encoder", x1.double(), False),)

        def build():
            latent, mu, explv = m._pair_latent(x1.cuda().transpose(1, 2), x0.cuda().transpose(1, 2), eps.cuda())
            assert type(latent.grad_fn).__name__.startswith("EncoderPairFunction")
            return latent[:, :OUT], mu, explv, latent[:, OUT:]
    _, want = _oracle_of(P, _dot(o64, ws))
    want = {n: g for n, g in want.items() if n.startswith(prefix)}
    opt = _route(world, route)
    _clear(world, opt)
    outs = build()
    _outputs_close(f"C encoder {node} B={B} Np={Np} {route}", outs, o64, ("z", "mu", "explv", "real mu"))
    loss = _dot(outs, ws)
    loss.backward(retain_graph=True)
    first = _named_grads(m, prefix)
    _clear(world, opt)
    loss.backward()
    second = _named_grads(m, prefix)
    was, ops.KEEP_ENCODER_ACTIVATIONS = ops.KEEP_ENCODER_ACTIVATIONS, False
    try:
        _clear(world, opt)
        _dot(build(), ws).backward()
        recomputed = _named_grads(m, prefix)
    finally:
        ops.KEEP_ENCODER_ACTIVATIONS = was
    tag = f"C encoder {node} B={B} Np={Np} {route}"
    _grads_meet(tag + " first", first, want)
    _grads_meet(tag + " second", second, want)
    for n, g in second.items():
        assert (g is None) == (recomputed[n] is None)
        if g is not None:
            assert torch.equal(g, recomputed[n]), f"{tag}: {n}: the replay is not the recompute path's result"


@pytest.mark.parametrize("route", ["plain", "flat"])
def test_hypernetwork_second_backward_equals_the_first(world, route):
    m, ref = world.model, world.ref
    la_, wa = _weights(31, (3, 2 * OUT), (3, 19011))
    P = _P64(world.state0, "hyper_network.")
    lat = la_.double().requires_grad_(True)
    _, want = _oracle_of(P, (ref.hypernet_forward(P, lat) * wa.double()).sum())
    want["latent"] = lat.grad
    opt = _route(world, route)
    dl = la_.cuda().requires_grad_(True)
    loss = (m.hyper_network(dl) * wa.cuda()).sum()
    runs = []
    for retain in (True, False):
        _clear(world, opt)
        dl.grad = None
        loss.backward(retain_graph=retain)
        runs.append(dict(_named_grads(m, "hyper_network."), latent=dl.grad.clone()))
    _grads_meet(f"C hypernetwork replay {route}", runs[1], want)
    for n, g in runs[0].items():
        assert torch.equal(g, runs[1][n]), n


@pytest.mark.parametrize("fused", [True, False])
def test_decoder_second_backward_equals_the_first(world, fused):
    from hyperpocket_amd import ops
    from hyperpocket_amd.model.target_network import target_network_batched
    ref, cfg = world.ref, world.model.target_network_config
    th = _theta(41)
    pa, wa = _weights(42, (3, 64, 3), (3, 64, 3))
    pa = pa.clamp(-1, 1)
    t64 = th.double().requires_grad_(True)
    want, = torch.autograd.grad((_target64(ref, t64, pa) * wa.double()).sum(), t64)
    was, ops.FUSED_TARGET_NETWORK = ops.FUSED_TARGET_NETWORK, fused
    try:
        t = th.cuda().requires_grad_(True)
        loss = (target_network_batched(cfg, t, pa.cuda()) * wa.cuda()).sum()
        first, = torch.autograd.grad(loss, t, retain_graph=True)
        second, = torch.autograd.grad(loss, t)
        _grads_meet(f"C decoder replay fused={fused}", {"theta": second}, {"theta": want})
        assert torch.equal(first, second)
    finally:
        ops.FUSED_TARGET_NETWORK = was


def _clouds(seed, b, n, m):
    r = np.random.RandomState(seed)
    return (r.rand(b, n, 3).astype(np.float32) - 0.5), (r.rand(b, m, 3).astype(np.float32) - 0.5)


@pytest.mark.parametrize("b,n,m", LOSS_SHAPES)
def test_match_cost_backward_twice_with_two_upstream_vectors(oracle_lib, b, n, m):
    """The node keeps d cost / d sets from its forward: every backward is that stored gradient times its own vector."""
    from hyperpocket_amd.utils.pytorch_structural_losses.match_cost import match_cost
    a, c = _clouds(61, b, n, m)
    A, C = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(c).cuda().requires_grad_(True)
    cost = match_cost(A, C)
    om, _ = oracle_lib.approxmatch(a, c)
    o1, o2 = oracle_lib.matchcostgrad(a, c, om)
    np.testing.assert_allclose(cost.detach().cpu().numpy(), oracle_lib.matchcost(a, c, om), rtol=1e-5)
    unit = torch.autograd.grad(cost, [A, C], grad_outputs=torch.ones(b, device="cuda"), retain_graph=True)
    for k, w in enumerate(_weights(62, (b,), (b,))):
        got = torch.autograd.grad(cost, [A, C], grad_outputs=w.cuda(), retain_graph=True)
        for g, u, o, name in zip(got, unit, (o1, o2), ("seta", "setb")):
            assert torch.equal(g, u * w.cuda().view(-1, 1, 1)), name
            e = np.abs(g.cpu().numpy() - o * w.numpy()[:, None, None]).max() / np.abs(o * w.numpy()[:, None, None]).max()
            print(f"C match_cost ({b},{n},{m}) vector {k} {name}: err/scale {e:.3e}")
            np.testing.assert_allclose(g.cpu().numpy(), o * w.numpy()[:, None, None], atol=5e-5, rtol=1e-3)


# ------------------------------------------------------------------------------------------------ D. partial use
@pytest.mark.parametrize("route", ["plain", "flat"])
@pytest.mark.parametrize("use", [(False, True, False), (True, False, False), (False, False, True)], ids=["mu", "z", "explv"])
def test_vae_encoder_with_one_output_used(world, route, use):
    m, ref = world.model, world.ref
    x, eps = _cloud(71, 3, 128)
    ws = _weights(72, (3, OUT), (3, OUT), (3, OUT))
    P = _P64(world.state0, "random_encoder.")
    o64 = _enc64(ref, P, "random_encoder", x, eps)
    _, want = _oracle_of(P, _dot(o64, ws, use))
    assert (want["random_encoder.std_layer.weight"] is None) == (use == (False, True, False))
    assert (want["random_encoder.mu_layer.weight"] is None) == (use == (False, False, True))
    opt = _route(world, route)
    _clear(world, opt)
    outs = _enc_gpu(m.random_encoder, x, eps)
    _outputs_close(f"D encoder {route}", outs, o64)
    _dot(outs, ws, use).backward()
    _grads_meet(f"D encoder, only {'z mu explv'.split()[use.index(True)]} used, {route}", _named_grads(m, "random_encoder."), want)


@pytest.mark.parametrize("route", ["plain", "flat"])
@pytest.mark.parametrize("half", [0, 1])
def test_pair_node_with_one_latent_half_used(world, half, route):
    """(Plain autograd sends zeros, not None, down the unused half of a concatenation: so does the float64 graph here.)"""
    m, ref = world.model, world.ref
    (x0, eps), (x1, _) = _cloud(51, 3, 128), _cloud(52, 3, 128)
    w, = _weights(73, (3, OUT))
    P = _P64(world.state0, "r")
    z, _, _ = ref.encoder_forward(P, "random_encoder", x0.double(), True, eps.double())
    lat64 = torch.cat([z, ref.encoder_forward(P, "real_encoder", x1.double(), False)], 1)
    _, want = _oracle_of(P, (lat64[:, half * OUT:(half + 1) * OUT] * w.double()).sum())
    assert want["real_encoder.std_layer.weight"] is None and want["random_encoder.conv.0.weight"] is not None
    opt = _route(world, route)
    _clear(world, opt)
    latent, _, _ = m._pair_latent(x1.cuda().transpose(1, 2), x0.cuda().transpose(1, 2), eps.cuda())
    _outputs_close("D pair node", (latent,), (lat64,), ("latent",))
    (latent[:, half * OUT:(half + 1) * OUT] * w.cuda()).sum().backward()
    _grads_meet(f"D pair node, latent half {half} used, {route}", _named_grads(m, "r"), want)


def _nn_dist64(a, c):
    d = ((a[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1)
    return d.min(2)[0], d.min(1)[0]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("b,n,m", LOSS_SHAPES)
def test_nn_distance_with_one_distance_used(b, n, m, which):
    from hyperpocket_amd.utils.pytorch_structural_losses.nn_distance import nn_distance
    a, c = (torch.from_numpy(t) for t in _clouds(74, b, n, m))
    w, = _weights(75, (b, (n, m)[which]))
    a64, c64 = a.double().requires_grad_(True), c.double().requires_grad_(True)
    d64 = _nn_dist64(a64, c64)[which]
    (d64 * w.double()).sum().backward()
    A, C = a.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    d = nn_distance(A, C)[which]
    close(d, d64.detach())
    (d * w.cuda()).sum().backward()
    _grads_meet(f"D nn_distance ({b},{n},{m}) dist{which + 1} only", {"seta": A.grad, "setb": C.grad}, {"seta": a64.grad, "setb": c64.grad})


@pytest.mark.parametrize("side", ["preds", "gts"])
@pytest.mark.parametrize("b,n,m", LOSS_SHAPES)
def test_chamfer_loss_with_one_side_requiring_grad(world, b, n, m, side):
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    a, c = (torch.from_numpy(t) for t in _clouds(76, b, n, m))
    a64, c64 = a.double().requires_grad_(side == "preds"), c.double().requires_grad_(side == "gts")
    l64 = world.ref.chamfer_loss(a64, c64)
    l64.backward()
    A, C = a.cuda().requires_grad_(side == "preds"), c.cuda().requires_grad_(side == "gts")
    loss = ChamferLoss()(A, C)
    close(loss, l64.detach())
    loss.backward()
    _grads_meet(f"D chamfer ({b},{n},{m}) only {side}", {"preds": A.grad, "gts": C.grad}, {"preds": a64.grad, "gts": c64.grad})


# ------------------------------------------------------------------------------------------------ E. layouts
def _off16(t):
    """t's values in a contiguous device tensor that starts 4 bytes past a 16-byte boundary."""
    big = torch.empty(t.numel() + 1, dtype=torch.float32, device="cuda")
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _terms(outs, ws, layout):
    """sum_i (out_i * w_i).sum(), built so that the gradient autograd hands each out_i's node has the layout asked for:
    transposed — a transposed view; expanded — a stride-0 expansion (ws are ones there); sliced — a slice of one larger
    tensor that starts off a 16-byte boundary."""
    if layout == "transposed":
        return sum((o.transpose(0, -1) * w.cuda().transpose(0, -1).contiguous()).sum() for o, w in zip(outs, ws))
    if layout == "expanded":
        return sum(o.sum() for o in outs)
    pad = torch.zeros(1, device="cuda")
    wcat = torch.cat([pad] + [w.cuda().reshape(-1) for w in ws])
    return (torch.cat([pad] + [o.reshape(-1) for o in outs]) * wcat).sum()


LAYOUTS = ["transposed", "expanded", "sliced", "input off 16 bytes"]


def _layout_weights(layout, ws):
    return [torch.ones_like(w) for w in ws] if layout == "expanded" else ws


@pytest.mark.parametrize("route", ["plain", "flat"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_encoder_gradient_and_input_layouts(world, layout, route):
    m, ref = world.model, world.ref
    x, eps = _cloud(81, 3, 128)
    ws = _layout_weights(layout, _weights(82, (3, OUT), (3, OUT), (3, OUT)))
    P = _P64(world.state0, "random_encoder.")
    o64 = _enc64(ref, P, "random_encoder", x, eps)
    _, want = _oracle_of(P, _dot(o64, ws))
    _clear(world, _route(world, route))
    if layout == "input off 16 bytes":
        outs = m.random_encoder(_off16(x).transpose(1, 2), _off16(eps))
        loss = _dot(outs, ws)
    else:
        outs = _enc_gpu(m.random_encoder, x, eps)
        loss = _terms(outs, ws, layout)
    _outputs_close(f"E encoder, {layout}, {route}", outs, o64)
    loss.backward()
    _grads_meet(f"E encoder, {layout}, {route}", _named_grads(m, "random_encoder."), want)


@pytest.mark.parametrize("route", ["plain", "flat"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_hypernetwork_gradient_and_input_layouts(world, layout, route):
    m, ref = world.model, world.ref
    la_, wa = _weights(31, (3, 2 * OUT), (3, 19011))
    wa, = _layout_weights(layout, [wa])
    P = _P64(world.state0, "hyper_network.")
    lat = la_.double().requires_grad_(True)
    t64 = ref.hypernet_forward(P, lat)
    _, want = _oracle_of(P, (t64 * wa.double()).sum())
    want["latent"] = lat.grad
    _clear(world, _route(world, route))
    dl = (_off16(la_) if layout == "input off 16 bytes" else la_.cuda()).requires_grad_(True)
    theta = m.hyper_network(dl)
    _outputs_close(f"E hypernetwork, {layout}, {route}", (theta,), (t64,), ("theta",))
    ((theta * wa.cuda()).sum() if layout == "input off 16 bytes" else _terms([theta], [wa], layout)).backward()
    _grads_meet(f"E hypernetwork, {layout}, {route}", dict(_named_grads(m, "hyper_network."), latent=dl.grad), want)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_decoder_gradient_and_input_layouts(world, layout, fused):
    from hyperpocket_amd import ops
    from hyperpocket_amd.model.target_network import target_network_batched
    ref, cfg = world.ref, world.model.target_network_config
    th = _theta(41)
    pa, wa = _weights(42, (3, 64, 3), (3, 64, 3))
    pa = pa.clamp(-1, 1)
    wa, = _layout_weights(layout, [wa])
    t64 = th.double().requires_grad_(True)
    y64 = _target64(ref, t64, pa)
    want, = torch.autograd.grad((y64 * wa.double()).sum(), t64)
    was, ops.FUSED_TARGET_NETWORK = ops.FUSED_TARGET_NETWORK, fused
    try:
        off = layout == "input off 16 bytes"
        t = (_off16(th) if off else th.cuda()).requires_grad_(True)
        y = target_network_batched(cfg, t, _off16(pa) if off else pa.cuda())
        _outputs_close(f"E decoder fused={fused}, {layout}", (y,), (y64,), ("y",))
        ((y * wa.cuda()).sum() if off else _terms([y], [wa], layout)).backward()
        _grads_meet(f"E decoder fused={fused}, {layout}", {"theta": t.grad}, {"theta": want})
    finally:
        ops.FUSED_TARGET_NETWORK = was


@pytest.mark.parametrize("b,n,m", LOSS_SHAPES)
def test_chamfer_loss_on_a_permuted_reconstruction(world, b, n, m):
    """core/epoch_loops.py:26: loss(gt, rec.permute(0, 2, 1)) with rec (B, 3, N)."""
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    a, c = (torch.from_numpy(t) for t in _clouds(83, b, n, m))
    rec64 = c.double().permute(0, 2, 1).contiguous().requires_grad_(True)
    l64 = world.ref.chamfer_loss(a.double(), rec64.permute(0, 2, 1))
    l64.backward()
    rec = c.cuda().permute(0, 2, 1).contiguous().requires_grad_(True)
    loss = ChamferLoss()(a.cuda(), rec.permute(0, 2, 1))
    close(loss, l64.detach())
    loss.backward()
    assert rec.grad.shape == rec.shape
    _grads_meet(f"E chamfer ({b},{n},{m}) rec.permute", {"rec": rec.grad}, {"rec": rec64.grad})


@pytest.mark.parametrize("b,n,m", LOSS_SHAPES)
def test_match_cost_on_non_contiguous_sets(oracle_lib, b, n, m):
    from hyperpocket_amd.utils.pytorch_structural_losses.match_cost import match_cost
    a, c = _clouds(84, b, n, m)
    At = torch.from_numpy(a).cuda().permute(0, 2, 1).contiguous().requires_grad_(True)      # (b, 3, n) leaves
    Ct = torch.from_numpy(c).cuda().permute(0, 2, 1).contiguous().requires_grad_(True)
    w, = _weights(85, (b,))
    cost = match_cost(At.permute(0, 2, 1), Ct.permute(0, 2, 1))
    om, _ = oracle_lib.approxmatch(a, c)
    o1, o2 = oracle_lib.matchcostgrad(a, c, om)
    np.testing.assert_allclose(cost.detach().cpu().numpy(), oracle_lib.matchcost(a, c, om), rtol=1e-5)
    (cost * w.cuda()).sum().backward()
    for g, o, name in ((At.grad, o1, "seta"), (Ct.grad, o2, "setb")):
        o = (o * w.numpy()[:, None, None]).transpose(0, 2, 1)
        print(f"E match_cost ({b},{n},{m}) non-contiguous {name}: err/scale {np.abs(g.cpu().numpy() - o).max() / np.abs(o).max():.3e}")
        np.testing.assert_allclose(g.cpu().numpy(), o, atol=5e-5, rtol=1e-3)


# ------------------------------------------------------------------------------------------------ F. inputs that require grad
def test_inputs_whose_gradient_is_not_formed_are_refused_in_the_forward(world):
    """The reference's modules differentiate x and points.  These nodes do not: a silent None would be wrong, so the
    forward raises, naming the argument — and stays quiet where no graph is recorded."""
    from hyperpocket_amd._lib import HipExtensionError
    from hyperpocket_amd.model.target_network import target_network_batched
    m, cfg = world.model, world.model.target_network_config
    _route(world, "plain")
    (x0, eps), (x1, _) = _cloud(51, 3, 128), _cloud(52, 3, 128)
    leaf = lambda t: t.cuda().requires_grad_(True)
    cf = lambda t: t.transpose(1, 2)
    with pytest.raises(HipExtensionError, match=r"`x` requires grad.*not formed"):
        m.random_encoder(cf(leaf(x0)), eps.cuda())
    with pytest.raises(HipExtensionError, match=r"`x` requires grad.*not formed"):
        m.real_encoder(cf(leaf(x0)))
    with pytest.raises(HipExtensionError, match=r"`eps` requires grad.*not formed"):
        m.random_encoder(cf(x0.cuda()), leaf(eps))
    with pytest.raises(HipExtensionError, match=r"`x \(VAE encoder\)` requires grad.*not formed"):
        m._pair_latent(cf(x1.cuda()), cf(leaf(x0)), eps.cuda())
    with pytest.raises(HipExtensionError, match=r"`x \(plain encoder\)` requires grad.*not formed"):
        m._pair_latent(cf(leaf(x1)), cf(x0.cuda()), eps.cuda())
    with pytest.raises(HipExtensionError, match=r"`eps` requires grad.*not formed"):
        m._pair_latent(cf(x1.cuda()), cf(x0.cuda()), leaf(eps))
    th, pts = _theta(41), _weights(42, (3, 64, 3))[0]
    with pytest.raises(HipExtensionError, match=r"`points` requires grad.*not formed"):
        target_network_batched(cfg, leaf(th), leaf(pts))
    with torch.no_grad():
        z, _, _ = m.random_encoder(cf(leaf(x0)), leaf(eps))
        y = target_network_batched(cfg, th.cuda(), leaf(pts))
    assert not z.requires_grad and not y.requires_grad


# ------------------------------------------------------------------------------------------------ G. double backward
def test_double_backward_is_refused_by_every_node(world):
    from hyperpocket_amd import ops
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    from hyperpocket_amd.model.target_network import target_network_batched
    from hyperpocket_amd.utils.pytorch_structural_losses.match_cost import match_cost
    from hyperpocket_amd.utils.pytorch_structural_losses.nn_distance import nn_distance
    m, cfg = world.model, world.model.target_network_config
    _route(world, "plain")
    (x0, eps), (x1, _) = _cloud(51, 3, 128), _cloud(52, 3, 128)
    cf = lambda t: t.cuda().transpose(1, 2)
    leaf = lambda t: t.cuda().requires_grad_(True)
    a, c = (torch.from_numpy(t) for t in _clouds(91, 3, 64, 64))
    th, lat, A, C, mu, explv = leaf(_theta(41)), leaf(_weights(31, (3, 2 * OUT))[0]), leaf(a), leaf(c), leaf(eps), leaf(eps.abs())
    # every loss is built so that the gradient arriving at the node carries a graph (d out^2 = 2 out): the node's backward
    # is then asked for a differentiable result, which once_differentiable refuses when that result is differentiated.
    cases = {
        "EncoderFunction": lambda: (m.random_encoder(cf(x0), eps.cuda())[0].square().sum(), m.random_encoder.mu_layer.weight),
        "EncoderPairFunction": lambda: (m._pair_latent(cf(x1), cf(x0), eps.cuda())[0].square().sum(), m.real_encoder.fc[0].weight),
        "HyperNetFunction": lambda: (m.hyper_network(lat).square().sum(), lat),
        "TargetNetworkFunction": lambda: (target_network_batched(cfg, th, _weights(42, (3, 64, 3))[0].cuda()).square().sum(), th),
        "KLDFunction": lambda: (ops.kld_loss(explv, mu).square(), mu),
        "_ChamferFunction": lambda: (ChamferLoss()(A, C).square(), A),
        "NNDistanceFunction": lambda: (nn_distance(A, C)[0].square().sum(), A),
        "MatchCostFunction": lambda: (match_cost(A, C).square().sum(), A),
    }
    for name, build in cases.items():
        loss, p = build()
        g, = torch.autograd.grad(loss, p, create_graph=True)
        assert g.requires_grad, name
        # a term built on the gradient (a gradient penalty): without the marking it would differentiate to zero, silently
        with pytest.raises(RuntimeError, match="once_differentiable") as err:
            (loss + g.square().sum()).backward()
        print(f"G {name}: double backward refused: {str(err.value)[:90]}")


# ------------------------------------------------------------------------------------------------ H. frozen sub-network
def test_frozen_real_encoder_under_flat_adam(world):
    m = world.model
    b = _batch(11, **SHAPES["pair"])
    l, g = world.oracle(b, "pair")
    want = {n: (None if n.startswith("real_encoder.") else v) for n, v in g.items()}
    opt = _route(world, "flat", frozen=("real_encoder",))
    assert not any(p is q for p in m.real_encoder.parameters() for q in opt.flat.params)
    before = {n: p.detach().clone() for n, p in m.real_encoder.named_parameters()}
    opt.zero_grad()
    loss = _gpu_loss(m, b, "EncoderPairFunction")
    close(loss, np.float64(l))
    loss.backward()
    _grads_meet("H frozen real_encoder", _named_grads(m), want)
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.real_encoder.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), before[n]), n
    assert not torch.equal(m.random_encoder.fc[0].weight.detach(), world.state0["random_encoder.fc.0.weight"])

"""CPU suite: the gradient-placement registry (ops._grad_buffer / parallel.FlatParameters) held to autograd's contract.

The HIP autograd nodes OVERWRITE the buffers `ops._grad_buffer(p)` hands them and return those buffers.  With a
FlatParameters owner the buffer may be a view of the owner's flat gradient, which autograd adopts as `p.grad` without a
copy.  That is only right while nobody else reads the slice: a second backward onto a set `.grad`, a parameter used by two
nodes of one graph, or a gradient a caller of torch.autograd.grad kept must get a fresh tensor instead.  A stub Function
that takes its buffers from the registry exactly as the real nodes do (overwrite, return) stands in for the kernels; the
reference is plain torch autograd on a float64 copy.  Every case runs with the registry in force and after
ops.clear_grad_views() (fresh tensors).

Bar: the stub's gradients are sums of at most 8 fp32 products of O(1) numbers (error <= 8 * 2^-24 ~ 5e-7 of their scale),
so 1e-5 of each gradient's scale; every wrong answer the cases are after (2*g2, g1 alone, g2 alone, the last node's
gradient twice) is asserted to lie at least 1000 bars away in float64 first.
"""
import gc
import weakref

import pytest
import torch
from torch import nn

import conftest  # noqa: F401  (import paths)

BAR = 1e-5


class _LinearStub(torch.autograd.Function):
    """y = x W^T + b with the placement protocol of the HIP nodes: the backward asks ops._grad_buffer for each parameter's
    buffer, overwrites it with the analytic gradient and returns it."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w, b)
        return x @ w.t() + b

    @staticmethod
    def backward(ctx, gy):
        from hyperpocket_amd import ops
        x, w, b = ctx.saved_tensors
        gw, gb = ops._grad_buffer(w), ops._grad_buffer(b)
        gw.copy_(gy.t() @ x)          # overwritten, never accumulated: what a kernel does
        gb.copy_(gy.sum(0))
        return gy @ w, gw, gb


class _Tiny(nn.Module):
    def __init__(self, linear=_LinearStub.apply):
        super().__init__()
        self.l1, self.l2 = nn.Linear(5, 7), nn.Linear(7, 3)
        self._linear = linear

    def forward(self, x):
        h = torch.tanh(self._linear(x, self.l1.weight, self.l1.bias))
        return self._linear(h, self.l2.weight, self.l2.bias)

    def twice(self, xa, xb):
        """l1 used by two nodes of one graph."""
        ya = self._linear(xa, self.l1.weight, self.l1.bias)
        yb = self._linear(xb, self.l1.weight, self.l1.bias)
        return torch.tanh(ya) * 1.5 + torch.sin(yb)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(8, 5, generator=g), torch.randn(8, 3, generator=g), torch.randn(8, 7, generator=g)


def _loss(model, seed):
    x, t, _ = _batch(seed)
    return (model(x) * t).sum()


def _loss_twice(model, seed_a, seed_b):
    (xa, _, ta), (xb, _, _) = _batch(seed_a), _batch(seed_b)
    return (model.twice(xa, xb) * ta).sum()


def _ref64(model, build):
    """name -> float64 gradient of build(m64) by plain torch autograd (None where the loss does not reach)."""
    m64 = _Tiny(nn.functional.linear).double()
    m64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    build(m64).backward()
    return {n: p.grad for n, p in m64.named_parameters()}


def _loss64(seed):
    def build(m):
        x, t, _ = _batch(seed)
        return (m(x.double()) * t.double()).sum()
    return build


def _twice64(seed_a, seed_b):
    def build(m):
        (xa, _, ta), (xb, _, _) = _batch(seed_a), _batch(seed_b)
        return (m.twice(xa.double(), xb.double()) * ta.double()).sum()
    return build


def _err(got, want):
    return (got.double() - want).abs().max().item() / want.abs().max().item()


def _far(wrong, want, what):
    """The premise of a case: the wrong answer it is after is far from the right one (float64, no code under test)."""
    d = (wrong - want).abs().max().item() / want.abs().max().item()
    assert d >= 1000 * BAR, (what, d)


def _check(model, want, what, flat=None):
    for n, p in model.named_parameters():
        if want[n] is None:
            assert p.grad is None, (what, n)
            continue
        e = _err(p.grad, want[n])
        print(f"{what:28s} {n:10s} p.grad    err/scale {e:.3e}")
        assert e <= BAR, (what, n, e)
        if flat is not None:
            e = _err(flat.grad_of(n), want[n])
            print(f"{what:28s} {n:10s} flat.grad err/scale {e:.3e}")
            assert e <= BAR, (what, n, "flat.grad", e)


@pytest.fixture(params=["registered", "fresh"])
def owner(request):
    from hyperpocket_amd import ops
    from hyperpocket_amd.parallel import FlatParameters
    ops.clear_grad_views()
    torch.manual_seed(3)
    model = _Tiny()
    flat = FlatParameters(model)
    if request.param == "fresh":
        ops.clear_grad_views()
    yield model, flat, request.param == "registered"
    ops.clear_grad_views()


def _slice_ptrs(flat):
    return {n: flat.grad.data_ptr() + 4 * o for n, o in zip(flat.names, flat.offsets)}


def test_single_backward_lands_in_the_flat_slice_without_a_copy(owner):
    model, flat, registered = owner
    want = _ref64(model, _loss64(1))
    for step in range(2):            # the second ordinary iteration (after the owner's clear) is as copy-free as the first
        flat.clear_param_grads()
        _loss(model, 1).backward()
        _check(model, want, f"single backward #{step}", flat if registered else None)
        if registered:
            for n, p in model.named_parameters():
                assert p.grad.data_ptr() == _slice_ptrs(flat)[n], n


def test_two_backwards_without_clearing_accumulate(owner):
    model, flat, registered = owner
    g1, g2 = _ref64(model, _loss64(1)), _ref64(model, _loss64(2))
    want = {n: g1[n] + g2[n] for n in g1}
    for n in want:
        _far(2 * g2[n], want[n], "2*g2")
        _far(g1[n], want[n], "g1")
        _far(g2[n], want[n], "g2")
    flat.clear_param_grads()
    _loss(model, 1).backward()
    _loss(model, 2).backward()
    _check(model, want, "accumulation", flat if registered else None)
    if registered:                   # the sum landed in the slice: FlatAdam.step's pointer check finds it in place
        for n, p in model.named_parameters():
            assert p.grad.data_ptr() == _slice_ptrs(flat)[n], n


def test_backward_after_in_place_zeroing(owner):
    """p.grad.zero_() is what zero_grad(set_to_none=False) does."""
    model, flat, registered = owner
    want = _ref64(model, _loss64(2))
    for n in want:
        _far(2 * want[n], want[n], "2*g")
    flat.clear_param_grads()
    _loss(model, 1).backward()
    for p in model.parameters():
        p.grad.zero_()
    _loss(model, 2).backward()
    _check(model, want, "in-place zeroing", flat if registered else None)


def test_parameter_shared_by_two_nodes_of_one_graph(owner):
    model, flat, registered = owner
    want = _ref64(model, _twice64(1, 2))
    ga = _ref64(model, lambda m: (torch.tanh(nn.functional.linear(_batch(1)[0].double(), m.l1.weight, m.l1.bias)) * 1.5
                                  * _batch(1)[2].double()).sum())
    gb = _ref64(model, lambda m: (torch.sin(nn.functional.linear(_batch(2)[0].double(), m.l1.weight, m.l1.bias))
                                  * _batch(1)[2].double()).sum())
    for n in ("l1.weight", "l1.bias"):
        assert _err(ga[n] + gb[n], want[n]) <= 1e-12
        for wrong, what in ((2 * ga[n], "2*gA"), (2 * gb[n], "2*gB"), (ga[n], "gA"), (gb[n], "gB")):
            _far(wrong, want[n], what)
    flat.clear_param_grads()
    _loss_twice(model, 1, 2).backward()
    assert want["l2.weight"] is None and model.l2.weight.grad is None
    _check(model, want, "shared parameter")
    # the owner's step reads p.grad (copying it into its slot when it lives elsewhere): whichever tensor holds the sum,
    # it is the sum
    flat.clear_param_grads()
    _loss_twice(model, 1, 2).backward()
    _check(model, want, "shared parameter, again")


def test_gradient_the_caller_keeps_survives_a_later_backward(owner):
    model, flat, registered = owner
    g1, g2 = _ref64(model, _loss64(1)), _ref64(model, _loss64(2))
    for n in g1:
        _far(g2[n], g1[n], "g2 for g1")
    flat.clear_param_grads()
    names = [n for n, _ in model.named_parameters()]
    kept = torch.autograd.grad(_loss(model, 1), list(model.parameters()))
    snap = [k.clone() for k in kept]
    _loss(model, 2).backward()
    for n, k, s in zip(names, kept, snap):
        assert torch.equal(k, s), n
        e = _err(k, g1[n])
        print(f"{'kept gradient':28s} {n:10s} kept      err/scale {e:.3e}")
        assert e <= BAR, (n, e)
    _check(model, g2, "backward after a kept one")


def test_owner_gone_drops_its_entries_and_backward_returns_fresh_tensors():
    from hyperpocket_amd import ops
    from hyperpocket_amd.parallel import FlatParameters
    ops.clear_grad_views()
    try:
        torch.manual_seed(3)
        model = _Tiny()
        flat = FlatParameters(model)
        keys = [p.data_ptr() for p in model.parameters()]
        assert all(k in ops._GRAD_VIEWS for k in keys)
        flat.clear_param_grads()
        _loss(model, 1).backward()                       # views handed out and adopted
        buf = weakref.ref(flat.grad)
        for p in model.parameters():
            p.grad = None
        del flat
        gc.collect()
        assert not any(k in ops._GRAD_VIEWS for k in keys)
        assert buf() is None                             # the registry no longer pins the dead owner's buffer
        for p in model.parameters():
            assert ops._grad_buffer(p)._base is None     # a fresh tensor, not a view of anything
        want = _ref64(model, _loss64(2))
        _loss(model, 2).backward()
        _loss(model, 2).backward()
        _check(model, {n: 2 * g for n, g in want.items()}, "owner gone")
    finally:
        ops.clear_grad_views()


def test_heads_get_one_contiguous_block_when_their_views_are_taken():
    """The hypernetwork's launches are chosen by whether the heads' gradient buffers lie back to back (and a skipped dW
    refuses bias gradients that do not): where registered views that lie back to back may not be handed out,
    ops._grad_block hands out slices of ONE fresh block, so an accumulating backward takes the launches of an ordinary
    one.  Views with gaps between them (these biases: 4, 6, 3 floats on 16-byte slots) get one fresh tensor each."""
    from hyperpocket_amd import ops
    from hyperpocket_amd.parallel import FlatParameters
    ops.clear_grad_views()
    try:
        hyper = nn.Module()
        hyper.output = nn.ModuleList([nn.Linear(8, 4), nn.Linear(8, 6), nn.Linear(8, 3)])
        model = nn.Module()
        model.hyper_network = hyper
        flat = FlatParameters(model)
        assert flat.heads is not None and flat.heads["rows"] == 13
        lo, hi = flat.grad.data_ptr(), flat.grad.data_ptr() + 4 * flat.total
        inside = lambda ts: [lo <= t.data_ptr() < hi for t in ts]
        gaps = lambda ts: [b.data_ptr() - a.data_ptr() - 4 * a.numel() for a, b in zip(ts, ts[1:])]
        for params, packed in (([h.weight for h in hyper.output], True), ([h.bias for h in hyper.output], False)):
            first = ops._grad_block(params)
            assert all(inside(first)) and (gaps(first) == [0, 0]) == packed                # in place
            again = ops._grad_block(params)                                                # taken: fresh tensors
            assert not any(inside(again))
            assert [t.shape for t in again] == [p.shape for p in params] and all(t.is_contiguous() for t in again)
            if packed:
                assert gaps(again) == [0, 0] and again[0]._base is not None                # one block, laid out alike
            else:
                assert all(t._base is None for t in again)                                 # one tensor each
            flat.clear_param_grads()
            assert all(inside(ops._grad_block(params)))                                    # cleared: in place again
            flat.clear_param_grads()
    finally:
        ops.clear_grad_views()

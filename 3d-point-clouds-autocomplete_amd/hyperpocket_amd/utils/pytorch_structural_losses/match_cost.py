"""Drop-in for utils/pytorch_structural_losses/match_cost.py:5-48.

Same call and results as the reference's ApproxMatch -> MatchCost (forward) and MatchCostGrad x grad_output
(backward), computed match-free: the nine per-level scaling vectors are kept instead of the (b,m,n) match
tensor and cost / gradients re-evaluate the match entries on the fly, in the reference's summation order
(hp_emd_forward / hp_emd_backward).  At B=64, N=2048 that removes a 1 GB tensor from `ctx` and its traffic.
The materialising functions stay available in StructuralLossesBackend.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from ..._lib import call, check_input, current_stream, load_library


class MatchCostFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seta, setb):
        seta, setb = seta.contiguous(), setb.contiguous()
        check_input(seta, "seta")
        check_input(setb, "setb")
        b, n, m = seta.size(0), seta.size(1), setb.size(1)
        dev = seta.device
        lib = load_library()
        f32 = dict(dtype=torch.float32, device=dev)
        temp = torch.empty((b, (n + m) * 2), **f32)
        ws = torch.empty((max(1, lib.hp_approxmatch_workspace_floats(b, n, m)),), **f32)
        lib.hp_emd_partials_floats.restype = ctypes.c_long
        part = torch.empty((max(1, lib.hp_emd_partials_floats(b, n, m)),), **f32)
        cost = torch.empty((b,), **f32)
        # gradients are by-products of the sweeps that produce the cost: take the ones autograd will ask for now
        grada = torch.empty((b, n, 3), **f32) if ctx.needs_input_grad[0] else None
        gradb = torch.empty((b, m, 3), **f32) if ctx.needs_input_grad[1] else None
        call("hp_emd_forward", b, n, m, seta, setb, temp, ws, part, cost, grada, gradb, current_stream(dev))
        ctx.grada, ctx.gradb = grada, gradb
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        per_cloud = grad_output.reshape(-1, 1, 1)        # d(loss)/d(cost_b), broadcast over that cloud's points
        return tuple(None if g is None else g * per_cloud for g in (ctx.grada, ctx.gradb))


match_cost = MatchCostFunction.apply

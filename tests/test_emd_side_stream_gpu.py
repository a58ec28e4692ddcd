"""GPU: hp_emd_forward_acc behind a gradient that another stream is still writing (the training step's arrangement).

The engine fills the reconstruction's gradient with the Chamfer term on a high-priority side stream and passes that stream as
`after`; the EMD's level sweeps run beside it and only the final sweep, which accumulates into that gradient, waits.  Since round 13
the sweeps' waves outrank the side stream's on the vector pipes (emd.hip HP_EMD_WAVE_PRIO), so Chamfer finishes later relative to
the level sweeps than it used to: what this file guards is that the final sweep still starts behind it.  For each shape the
Chamfer forward + backward write g_rec on a second stream and hp_emd_forward_acc runs on the first with the second as `after`;
cost and the accumulated gradient must equal, bit for bit, those of the same calls on one stream, and a second run of either must
equal the first.  g_rec starts as NaN, so a sweep that ran ahead of the Chamfer gradient (overwritten afterwards) or a Chamfer
gradient that never landed shows.  Shapes: (3, 200, 264) — one chain, ordered records, ragged tiles — and (64, 1024, 1024), the
smallest batch at which two chains run.  Inputs: the noisy-copy regime the EMD is timed in (bench.emd_regime_noisy_copy, restated).
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 200, 264), (64, 1024, 1024)]
_SIDE = []


def _side_stream():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(priority=-1))
    return _SIDE[0]


def _noisy_copy(b, n, m):
    """gt ~ U(-0.5, 0.5)^3 (b, n, 3); rec (b, m, 3) = points of gt in shuffled order (every one, where m >= n) + N(0, sigma^2),
    sigma cycling over 0.002 / 0.01 / 0.02 / 0.05 from cloud to cloud."""
    g = torch.Generator(device="cuda").manual_seed(7)
    f32 = dict(dtype=torch.float32, device="cuda")
    gt = torch.rand(b, n, 3, generator=g, **f32) - 0.5
    pick = torch.stack([torch.randperm(m, generator=g, device="cuda") % n for _ in range(b)])
    sig = torch.tensor([0.002, 0.01, 0.02, 0.05], **f32)[torch.arange(b, device="cuda") % 4].view(b, 1, 1)
    rec = torch.gather(gt, 1, pick.unsqueeze(-1).expand(-1, -1, 3)) + sig * torch.randn(b, m, 3, generator=g, **f32)
    return gt.contiguous(), rec.contiguous()


def _step_losses(gt, rec, two_streams):
    """g_rec = 0.05 * d Chamfer / d rec, then += (0.05 / m) * d EMD / d rec inside hp_emd_forward_acc; returns (cost, g_rec)."""
    from hyperpocket_amd._lib import call, current_stream, load_library
    lib = load_library()
    lib.hp_emd_partials_floats.restype = ctypes.c_long
    b, n, m = gt.size(0), gt.size(1), rec.size(1)
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    cur = torch.cuda.current_stream()
    # everything is allocated on the compute stream and lives until the synchronize below
    g_rec = torch.full((b, m, 3), float("nan"), **f32)
    dist1, dist2 = torch.empty((b, n), **f32), torch.empty((b, m), **f32)
    idx1, idx2 = torch.empty((b, n), **i32), torch.empty((b, m), **i32)
    part = torch.empty((lib.hp_chamfer_workspace_floats(b, n, m),), **f32)
    cd, c_cd = torch.empty((), **f32), torch.full((), 0.05, **f32)
    temp = torch.empty((b, 2 * (n + m)), **f32)
    ws = torch.empty((lib.hp_approxmatch_workspace_floats(b, n, m),), **f32)
    epart = torch.empty((lib.hp_emd_partials_floats(b, n, m),), **f32)
    cost = torch.full((b,), float("nan"), **f32)
    side = _side_stream() if two_streams else cur
    if two_streams:
        side.wait_stream(cur)
    with torch.cuda.stream(side):
        st = current_stream(gt.device)
        call("hp_chamfer_forward", b, n, gt, m, rec, dist1, idx1, dist2, idx2, part, cd, st)
        call("hp_chamfer_backward", b, n, gt, m, rec, idx1, idx2, c_cd, None, g_rec, st)
    call("hp_emd_forward_acc", b, n, m, gt, rec, temp, ws, epart, cost, g_rec, 0.05 / m, current_stream(gt.device),
         ctypes.c_void_p(side.cuda_stream) if two_streams else None)
    torch.cuda.synchronize()
    return cost, g_rec


_ONE_STREAM = {}


def _one_stream(shape):
    """the one-stream results of a shape: computed once, shared by the tests, never written"""
    if shape not in _ONE_STREAM:
        gt, rec = _noisy_copy(*shape)
        _ONE_STREAM[shape] = (gt, rec) + _step_losses(gt, rec, False)
    return _ONE_STREAM[shape]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_final_sweep_waits_for_the_side_streams_gradient(shape):
    gt, rec, cost1, g1 = _one_stream(shape)
    assert torch.isfinite(cost1).all() and torch.isfinite(g1).all()
    assert (cost1 > 0).all()      # every cloud carries mass in this regime
    for run in range(2):
        cost2, g2 = _step_losses(gt, rec, True)
        assert torch.equal(_bits(cost2), _bits(cost1)), f"cost differs from the one-stream call (run {run})"
        assert torch.equal(_bits(g2), _bits(g1)), f"accumulated gradient differs from the one-stream call (run {run})"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_stream_call_repeats(shape):
    gt, rec, cost1, g1 = _one_stream(shape)
    cost2, g2 = _step_losses(gt, rec, False)
    assert torch.equal(_bits(cost2), _bits(cost1)) and torch.equal(_bits(g2), _bits(g1))

"""utils/evaluation/completeness.py — unidirectional Hausdorff distance (UHD) from the partial input to its completions,
and the completeness ratio, on the HIP pair kernel (hp_cloud_pairs) instead of a (B,3,N,M) CPU tensor, a KD-tree and
ray workers.  Same names, arguments and results.
"""
import torch

from ..pytorch_structural_losses import StructuralLossesBackend as backend
from .cloud_pairs import COVERED, HAUSDORFF, cloud_pairs
from .shape_dir import grouped_paths, load_points


def _gpu(x):
    """numpy array or tensor (any device) -> contiguous fp32 tensor on the current GPU (or the tensor's own GPU)."""
    t = torch.as_tensor(x)
    dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.to(device=dev, dtype=torch.float32).contiguous()


def uhd_pairs(partial, completions, pairs):
    """sqrt(max_i min_j |partial[a]_i - completions[b]_j|^2) per (a, b) pair: the directed Hausdorff distance."""
    return cloud_pairs(HAUSDORFF, partial, completions, pairs).sqrt()


def directed_hausdorff(point_cloud1, point_cloud2, reduce_mean=True):
    """point_cloud1 (B, 3, N), point_cloud2 (B, 3, M) -> (B,) max over cloud-1 points of the distance to the nearest
    cloud-2 point (A -> B), or its mean.  The result lives on point_cloud1's device."""
    if point_cloud1.dim() != 3 or point_cloud2.dim() != 3 or point_cloud1.size(0) != point_cloud2.size(0):
        raise ValueError(f"expected (B,3,N) and (B,3,M), got {tuple(point_cloud1.shape)} {tuple(point_cloud2.shape)}")
    a = _gpu(torch.as_tensor(point_cloud1).transpose(1, 2))
    b = _gpu(torch.as_tensor(point_cloud2).transpose(1, 2)).to(a.device)
    idx = torch.arange(a.size(0), device=a.device)
    d = uhd_pairs(a, b, torch.stack([idx, idx], 1))
    if reduce_mean:
        d = d.mean()
    return d.to(point_cloud1.device)


def nn_distance(query_points, ref_points):
    """(N,3), (M,3) numpy -> (N,) float64: distance of every query point to its nearest reference point."""
    q, r = _gpu(query_points).unsqueeze(0), _gpu(ref_points).unsqueeze(0)
    dist, _, _, _ = backend.NNDistance(q, r.to(q.device))
    return dist[0].double().sqrt().cpu().numpy()


def completeness(query_points, ref_points, thres=0.03):
    """Share of the query points whose nearest reference point lies closer than `thres`."""
    q, r = _gpu(query_points).unsqueeze(0), _gpu(ref_points).unsqueeze(0)
    covered = cloud_pairs(COVERED, q, r.to(q.device), [[0, 0]], thres)
    return covered.item() / q.size(1)


def uhd_per_input(existing, generated):
    """existing (S, Ne, 3), generated (S, k, N, 3) on one GPU -> (S,) fp64: each input's mean directed Hausdorff
    distance to its k completions (the reference's process_one_uhd)."""
    S, k = generated.size(0), generated.size(1)
    if existing.size(0) != S:
        raise ValueError(f"{existing.size(0)} inputs for {S} groups of completions")
    dev = existing.device
    s = torch.arange(S, device=dev).repeat_interleave(k)
    pairs = torch.stack([s, torch.arange(S * k, device=dev)], 1)
    gen = generated.reshape(S * k, generated.size(2), 3).contiguous()
    return uhd_pairs(existing.contiguous(), gen, pairs).double().view(S, k).mean(1)


def process(shape_dir):
    """Mean UHD over the inputs of a `fixed/` directory (see shape_dir.py for the file protocol)."""
    groups, existing = grouped_paths(shape_dir, with_existing=True)
    ex = _gpu(load_points(existing))
    gen = _gpu(load_points([p for g in groups for p in g])).to(ex.device)
    return uhd_per_input(ex, gen.view(len(groups), len(groups[0]), gen.size(1), 3)).mean().item()

"""utils/evaluation/total_mutual_diff.py — total mutual difference (TMD) of the k completions of one partial input:
Σ_{j<l} CD(j, l) · 2/(k−1), CD = chamfer.compute_trimesh_chamfer.  All S·k(k−1)/2 pairs go to the HIP pair kernel in
one launch, instead of a serial loop over scipy KD-trees.
"""
import torch

from .cloud_pairs import CHAMFER, cloud_pairs
from .completeness import _gpu
from .shape_dir import grouped_paths, load_points


def total_mutual_difference(gen):
    """gen (S, k, N, 3) fp32 on a GPU -> (S,) fp64 TMD of every group."""
    if gen.dim() != 4 or gen.size(3) != 3 or gen.size(1) < 2:
        raise ValueError(f"expected (S, k >= 2, N, 3), got {tuple(gen.shape)}")
    S, k, N = gen.size(0), gen.size(1), gen.size(2)
    j, l = torch.triu_indices(k, k, 1, device=gen.device)
    base = (torch.arange(S, device=gen.device) * k).view(S, 1)
    pairs = torch.stack([(base + j).reshape(-1), (base + l).reshape(-1)], 1)
    flat = gen.reshape(S * k, N, 3).contiguous()
    cd = cloud_pairs(CHAMFER, flat, flat, pairs).double().sum(1) / N
    return cd.view(S, -1).sum(1) * (2.0 / (k - 1))


def process(shape_dir):
    """Mean TMD over the inputs of a `fixed/` directory (see shape_dir.py for the file protocol)."""
    groups, _ = grouped_paths(shape_dir, with_existing=False)
    gen = _gpu(load_points([p for g in groups for p in g]))
    return total_mutual_difference(gen.view(len(groups), len(groups[0]), gen.size(1), 3)).mean().item()

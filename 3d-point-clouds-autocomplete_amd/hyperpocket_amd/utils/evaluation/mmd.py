"""utils/evaluation/mmd.py:23-47 — minimum matching distance of a reference set against generated samples,
over the HIP nearest-neighbour kernel.

Faithful to the reference including its quirk: ``nn_distance(ref (1,N,3), chunk (<=batch,N,3))`` takes
the batch size from its FIRST argument, so only the first cloud of every chunk is ever compared.

``minimum_matching_distance_all_pairs`` is the true minimum-matching distance over ALL (reference, sample) pairs, on the
HIP pair kernel (hp_cloud_pairs) in one launch.
"""
import numpy as np
import torch

from ..pytorch_structural_losses.nn_distance import nn_distance
from .cloud_pairs import CHAMFER, cloud_pairs
from .shape_dir import load_points, reconstruction_paths


def iterate_in_chunks(seq, n):
    for i in range(0, len(seq), n):
        yield seq[i:i + n]


def minimum_mathing_distance(sample_pcs, ref_pcs, batch_size, device=None):
    n_ref, n_pc_points, pc_dim = ref_pcs.shape
    _, n_pc_points_s, pc_dim_s = sample_pcs.shape
    if n_pc_points != n_pc_points_s or pc_dim != pc_dim_s:
        raise ValueError('Incompatible size of point-clouds.')
    matched_dists = []
    for i in range(n_ref):
        ref = torch.from_numpy(ref_pcs[i]).unsqueeze(0).to(device).contiguous()
        best = []
        for chunk_np in iterate_in_chunks(sample_pcs, batch_size):
            chunk = torch.from_numpy(chunk_np).to(device).contiguous()
            ref_to_s, s_to_ref = nn_distance(ref, chunk)       # b = 1: chunk[0] only (reference behaviour)
            best.append(torch.min(ref_to_s.mean(dim=1) + s_to_ref.mean(dim=1)).item())
        matched_dists.append(np.min(best))
    return np.mean(matched_dists), matched_dists


def chamfer_pairs(A, B, pairs):
    """Per (a, b) pair: mean over A[a] of the squared distance to the nearest point of B[b] plus the mirrored mean,
    fp64 — the per-pair value minimum_mathing_distance takes the minimum of."""
    s = cloud_pairs(CHAMFER, A, B, pairs).double()
    return s[:, 0] / A.size(1) + s[:, 1] / B.size(1)


def minimum_matching_distance_all_pairs(sample, ref):
    """sample (Ns, N, 3), ref (Nr, N, 3) fp32 on one GPU -> (mmd, per_ref): per_ref (Nr,) fp64 is, for every reference
    cloud, the smallest Chamfer distance to ANY sample cloud; mmd their mean (a 0-dim fp64 tensor)."""
    if sample.dim() != 3 or ref.dim() != 3 or sample.shape[1:] != ref.shape[1:]:
        raise ValueError('Incompatible size of point-clouds.')
    ns, nr = sample.size(0), ref.size(0)
    dev = ref.device
    pairs = torch.stack([torch.arange(nr, device=dev).repeat_interleave(ns), torch.arange(ns, device=dev).repeat(nr)], 1)
    per_ref = chamfer_pairs(ref.contiguous(), sample.contiguous(), pairs).view(nr, ns).min(1).values
    return per_ref.mean(), per_ref


def minimum_matching_distance_chunked(sample, ref, batch_size):
    """minimum_mathing_distance's result (the reference's chunk[0]-only semantics) on device tensors, in one
    launch: reference cloud r meets sample clouds 0, batch_size, 2*batch_size, ...  -> (mmd, per_ref) as above."""
    if sample.dim() != 3 or ref.dim() != 3 or sample.shape[1:] != ref.shape[1:]:
        raise ValueError('Incompatible size of point-clouds.')
    firsts = torch.arange(0, sample.size(0), batch_size, device=ref.device)
    nr, nc = ref.size(0), firsts.numel()
    pairs = torch.stack([torch.arange(nr, device=ref.device).repeat_interleave(nc), firsts.repeat(nr)], 1)
    per_ref = chamfer_pairs(ref.contiguous(), sample.contiguous(), pairs).view(nr, nc).min(1).values
    return per_ref.mean(), per_ref


def process(shape_dir, dataset, device, batch_size=64):
    """MMD of every reconstruction in a `fixed/` directory against the dataset's complete clouds (each item's third
    field), with the reference's semantics (minimum_mathing_distance above)."""
    ref_pcs = np.stack([np.asarray(item[2], dtype=np.float32) for item in dataset], axis=0)
    paths = reconstruction_paths(shape_dir)
    if not paths:
        raise ValueError(f"{shape_dir}: no reconstruction files")
    mmd, _ = minimum_mathing_distance(load_points(paths), ref_pcs, batch_size, device)
    return mmd

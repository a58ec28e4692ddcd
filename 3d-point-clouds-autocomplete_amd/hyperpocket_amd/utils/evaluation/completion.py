"""Completion metrics in one call on device tensors — UHD, TMD and MMD without the reference's `.npy` round trip.
Every distance comes from the HIP pair kernel (hp_cloud_pairs)."""
from .completeness import uhd_per_input
from .mmd import minimum_matching_distance_all_pairs, minimum_matching_distance_chunked
from .total_mutual_diff import total_mutual_difference


def completion_metrics(existing, generated, ref=None, batch_size=64):
    """existing (S, Ne, 3): the partial inputs; generated (S, k, N, 3): k completions of each; ref (R, N, 3): complete
    reference clouds, optional.  fp32 tensors on one GPU.  Returns floats:
      'UHD'            mean directed Hausdorff distance input -> completion   (completeness.process)
      'TMD'            mean total mutual difference of each input's completions   (total_mutual_diff.process)
      'MMD'            minimum matching distance of ref against all S*k completions, over all pairs
      'MMD_reference'  the same with the reference's chunk semantics at `batch_size` (mmd.process)."""
    if generated.dim() != 4 or existing.dim() != 3 or existing.size(0) != generated.size(0):
        raise ValueError(f"expected existing (S,Ne,3), generated (S,k,N,3); got {tuple(existing.shape)}, "
                         f"{tuple(generated.shape)}")
    out = {"UHD": uhd_per_input(existing, generated).mean(), "TMD": total_mutual_difference(generated).mean()}
    if ref is not None:
        sample = generated.reshape(-1, generated.size(2), 3)
        out["MMD"] = minimum_matching_distance_all_pairs(sample, ref)[0]
        out["MMD_reference"] = minimum_matching_distance_chunked(sample, ref, batch_size)[0]
    return {k: v.item() for k, v in out.items()}

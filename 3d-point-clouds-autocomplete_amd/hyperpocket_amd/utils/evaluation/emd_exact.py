"""``emd_exact_pairs`` / ``emd_exact_loss``: the true earth mover's distance of equal-sized clouds — the minimum over
one-to-one matchings of the summed point distances — on the HIP auction solver (hp_assign_pairs, csrc/assign.hip), next
to the approximate ``emd_pairs``.

The solver works on distances quantised to 2^-scale_log2 and is exact on those integers, so a cost is
within n * 2^-(scale_log2 + 1) of the optimum over the fp32 distances.  One workgroup per pair, no scratch buffers, any
number of pairs in one call, on the caller's current stream.  Bit-identical from run to run and independent of where a pair
stands in the list.
"""
import ctypes

import torch

from ..._lib import HipExtensionError, call, check_input, current_stream

INT32_MAX = (1 << 31) - 1
CAPPED, BAD_PAIR, OVERFLOW = -1, -2, -3          # hp_assign_pairs' per-pair status, in `rounds`


def emd_exact_pairs(A, B, pairs, scale_log2=20, max_rounds=None, return_assignment=False):
    """A (na, n, 3), B (nb, n, 3) fp32 contiguous on one GPU; pairs (P, 2) integer (a, b) indices -> cost (P,) fp64: the
    minimum over one-to-one matchings of (A[a], B[b]) of the summed point distances, not divided by n (emd_pairs' convention),
    as cost_int / 2^scale_log2 — exact in fp64.  return_assignment: -> (cost, assignment (P, n) int32: the point of B[b]
    matched to every point of A[a], rounds (P,) int32: auction rounds, or the pair's status).

    A pair with an index outside its set gets NaN (rounds -2), whatever the integer type of `pairs`.  A pair that exhausted
    `max_rounds` (None: the library's default for n) or whose quantised distances overflow 2^30 (coordinates times
    2^scale_log2 too large, or not finite) gets NaN as well, and the call then raises HipExtensionError once it has run,
    naming how many.  No gradients: see emd_exact_loss."""
    if max_rounds is not None and max_rounds < 1:
        raise ValueError(f"max_rounds must be positive, got {max_rounds}")
    check_input(A, "A")
    check_input(B, "B")
    if A.dim() != 3 or A.size(2) != 3 or B.dim() != 3 or B.size(2) != 3:
        raise ValueError(f"clouds must be (count, points, 3), got {tuple(A.shape)} and {tuple(B.shape)}")
    if A.device != B.device:
        raise ValueError("A and B must be on the same device")
    if A.size(1) != B.size(1):
        raise ValueError(f"the exact EMD needs equal point counts, got {A.size(1)} and {B.size(1)}")
    dev = A.device
    pairs = torch.as_tensor(pairs)
    if pairs.is_floating_point() or pairs.is_complex() or pairs.dtype == torch.bool:
        raise ValueError(f"pairs must hold integer indices, got {pairs.dtype}")
    if pairs.dtype != torch.int32:
        # an index that does not fit int32 must stay out of range, not wrap into it: -1 and 2^31 - 1 are outside every set
        pairs = pairs.to(device=dev, dtype=torch.int64).clamp(-1, INT32_MAX)
    pairs = pairs.to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    P, n = pairs.size(0), A.size(1)
    cost_int = torch.empty((P,), dtype=torch.int64, device=dev)
    rounds = torch.empty((P,), dtype=torch.int32, device=dev)
    assignment = torch.empty((P, n), dtype=torch.int32, device=dev) if return_assignment else None
    if P and min(A.size(0), n, B.size(0)) < 1:
        raise ValueError(f"empty cloud sets: {tuple(A.shape)} and {tuple(B.shape)}")
    if P:
        call("hp_assign_pairs", A.size(0), n, A, B.size(0), B, ctypes.c_long(P), pairs, int(scale_log2),
             ctypes.c_long(0 if max_rounds is None else int(max_rounds)), assignment, cost_int, rounds, current_stream(dev))
    cost = cost_int.double() / float(1 << scale_log2)
    cost = torch.where(rounds < 0, torch.full_like(cost, float("nan")), cost)
    if P:
        capped, overflow = int((rounds == CAPPED).sum()), int((rounds == OVERFLOW).sum())
        if capped or overflow:
            raise HipExtensionError(f"exact EMD: {capped} of {rounds.numel()} pairs exhausted the round bound, "
                                    f"{overflow} overflowed the distance quantisation (scale_log2={scale_log2})")
    return (cost, assignment, rounds) if return_assignment else cost


def emd_exact_loss(a, b):
    """a, b (batch, n, 3) fp32 on the GPU -> (batch,) fp32: sum_i |a_i - b_sigma(i)| under the optimal matching sigma of cloud
    k of `a` against cloud k of `b`.  The matching comes from the kernel without gradients; the distances are plain torch, so
    autograd gives d/da_i = (a_i - b_sigma(i)) / |a_i - b_sigma(i)| and the opposite for b (the loss of MSN-style training).
    The value equals the kernel's cost up to its quantisation and the fp32 summation."""
    if a.shape != b.shape:
        raise ValueError(f"the exact EMD needs equal shapes, got {tuple(a.shape)} and {tuple(b.shape)}")
    batch = a.size(0)
    pairs = torch.arange(batch, device=a.device, dtype=torch.int32).view(-1, 1).expand(-1, 2)
    _, assignment, _ = emd_exact_pairs(a.detach().contiguous(), b.detach().contiguous(), pairs, return_assignment=True)
    matched = b.gather(1, assignment.long().unsqueeze(2).expand(-1, -1, 3))
    return (a - matched).norm(dim=-1).sum(-1)

"""``cloud_pairs``: nearest-neighbour reductions over a list of (a, b) cloud pairs on the HIP pair kernel
(hp_cloud_pairs, csrc/cloud_pairs.hip) — the one distance primitive under every completion metric here.

No clouds are copied per pair: A and B are indexed through the pair list, and one launch covers any number of pairs.
Per-point minima are hp_nndistance's bit for bit; the reductions are deterministic.
"""
import ctypes

import torch

from ..._lib import call, check_input, current_stream, load_library

CHAMFER, HAUSDORFF, COVERED = 0, 1, 2


def cloud_pairs(mode, A, B, pairs, thres=0.0):
    """A (na, n, 3), B (nb, m, 3) fp32 contiguous on one GPU; pairs (P, 2) integer (a, b) indices.

    CHAMFER   -> (P, 2): (sum_i min_j d^2 over A[a]'s points, sum_j min_i d^2 over B[b]'s points)
    HAUSDORFF -> (P,):   max_i min_j d^2, A[a] -> B[b]
    COVERED   -> (P,):   #{i : sqrt(min_j d^2) < thres}, A[a] -> B[b]
    d^2 are squared distances; sums are fp64 accumulations rounded to fp32 once."""
    check_input(A, "A")
    check_input(B, "B")
    if A.dim() != 3 or A.size(2) != 3 or B.dim() != 3 or B.size(2) != 3:
        raise ValueError(f"clouds must be (count, points, 3), got {tuple(A.shape)} and {tuple(B.shape)}")
    if A.device != B.device:
        raise ValueError("A and B must be on the same device")
    dev = A.device
    pairs = torch.as_tensor(pairs).to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    P = pairs.size(0)
    out = torch.empty((P, 2) if mode == CHAMFER else (P,), dtype=torch.float32, device=dev)
    if P == 0:
        return out
    na, n = A.size(0), A.size(1)
    nb, m = B.size(0), B.size(1)
    wsf = load_library().hp_cloud_pairs_workspace_floats(mode, n, m, ctypes.c_long(P))
    if wsf < 0:
        raise ValueError(f"hp_cloud_pairs: bad mode {mode} or sizes n={n} m={m}")
    ws = torch.empty((max(2, wsf) // 2,), dtype=torch.float64, device=dev)    # 8-byte aligned
    call("hp_cloud_pairs", mode, na, n, A, nb, m, B, ctypes.c_long(P), pairs, float(thres), ws, out, current_stream(dev))
    return out

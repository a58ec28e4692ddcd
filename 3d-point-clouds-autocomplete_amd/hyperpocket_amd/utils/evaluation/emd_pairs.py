"""``emd_pairs``: the approximate EMD (match cost) over a list of (a, b) cloud pairs on the HIP pair entry point
(hp_emd_pairs, csrc/emd.hip) — the EMD half of every cloud-set against cloud-set metric, next to ``cloud_pairs``.

No clouds are copied per pair: the EMD's set-up kernels read A and B through the pair list, everything behind them is
the batched path's.  Any number of pairs: the call runs in chunks of at most 65 535 pairs that share one allocation of
the three scratch buffers, in order, on the caller's current stream.

Reproducibility contract:
  * the costs of one chunk are bit-identical to ``match_cost(A[a].contiguous(), B[b].contiguous())`` on that chunk's
    pairs under the same library switches (hp_emd_set_*);
  * between different chunk sizes (another ``workspace_bytes``, another P) the costs agree only to the regrouping of the
    cost partials: the rows-per-lane instance of the sweeps and the split into chains depend on the number of clouds in
    a call (2e-6 relative, the figure stated above emd_forward_impl in csrc/emd.hip).
"""
import torch

from ..._lib import call, check_input, current_stream, load_library

MAX_CHUNK = 65535           # hp_emd_pairs: the pairs are a grid dimension
DEFAULT_WORKSPACE_BYTES = 1 << 30
INT32_MAX = (1 << 31) - 1


def emd_pairs_buffer_floats(chunk, n, m):
    """-> (temp, ws, partials) floats hp_emd_pairs needs for `chunk` pairs of n against m points (host only)."""
    lib = load_library()
    return (chunk * (n + m) * 2, lib.hp_approxmatch_workspace_floats(chunk, n, m), lib.hp_emd_partials_floats(chunk, n, m))


def emd_pairs_chunk(n, m, workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """The largest number of pairs <= 65 535 whose three buffers fit `workspace_bytes` together, and at least 1 (one pair
    is always run, whatever the budget).  Pure host arithmetic over the library's size queries."""
    if n <= 0 or m <= 0:
        raise ValueError(f"clouds need points: n={n} m={m}")
    fits = lambda c: 4 * sum(emd_pairs_buffer_floats(c, n, m)) <= workspace_bytes
    if fits(MAX_CHUNK):
        return MAX_CHUNK
    lo, hi = 1, MAX_CHUNK           # lo fits (or is the floor of 1), hi does not; the sizes grow with the chunk
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    return lo


def emd_pairs(A, B, pairs, workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """A (na, n, 3), B (nb, m, 3) fp32 contiguous on one GPU; pairs (P, 2) integer (a, b) indices -> (P,) fp32: the
    match cost of (A[a], B[b]), not divided by the number of points (match_cost's value).  A pair with an index outside
    its set gets NaN, whatever the integer type of `pairs` (an index beyond int32 counts as outside).  No gradients.  `workspace_bytes` bounds the scratch of a chunk (see emd_pairs_chunk)."""
    check_input(A, "A")
    check_input(B, "B")
    if A.dim() != 3 or A.size(2) != 3 or B.dim() != 3 or B.size(2) != 3:
        raise ValueError(f"clouds must be (count, points, 3), got {tuple(A.shape)} and {tuple(B.shape)}")
    if A.device != B.device:
        raise ValueError("A and B must be on the same device")
    dev = A.device
    pairs = torch.as_tensor(pairs)
    if pairs.is_floating_point() or pairs.is_complex() or pairs.dtype == torch.bool:
        raise ValueError(f"pairs must hold integer indices, got {pairs.dtype}")
    if pairs.dtype != torch.int32:
        # an index that does not fit int32 must stay out of range, not wrap into it: -1 and 2^31 - 1 are outside every set
        pairs = pairs.to(device=dev, dtype=torch.int64).clamp(-1, INT32_MAX)
    pairs = pairs.to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    P = pairs.size(0)
    out = torch.empty((P,), dtype=torch.float32, device=dev)
    if P == 0:
        return out
    na, n = A.size(0), A.size(1)
    nb, m = B.size(0), B.size(1)
    if min(na, n, nb, m) < 1:
        raise ValueError(f"empty cloud sets: {tuple(A.shape)} and {tuple(B.shape)}")
    chunk = min(P, emd_pairs_chunk(n, m, workspace_bytes))
    f32 = dict(dtype=torch.float32, device=dev)
    temp, ws, part = (torch.empty((max(1, f),), **f32) for f in emd_pairs_buffer_floats(chunk, n, m))
    stream = current_stream(dev)
    for s in range(0, P, chunk):
        c = min(chunk, P - s)
        call("hp_emd_pairs", na, n, A, nb, m, B, c, pairs[s:s + c], temp, ws, part, out[s:s + c], stream)
    return out

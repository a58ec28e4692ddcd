"""utils/evaluation/visibility.py — the one check of a completion that a depth capture allows without ground truth: the sensor
looked through all the space in front of what it recorded, so a completion that puts points there contradicts the scan, and
one that puts them behind the recorded surface does not.  On the HIP visibility kernels (ops.scan_visibility,
csrc/visibility.hip): the scans' depth buffers from their sensor positions, and the completions' rows as queries against them.
"""
import torch

from ... import ops
from ...datasets.scan_dataset import DeviceScanDataset

LABELS = ops.VISIBILITY_LABELS          # the columns of `shares`: seen through, on the surface, hidden, unobserved


def completion_consistency(dataset, completions, viewpoints=None, **visibility):
    """How the completions of a DeviceScanDataset's scans stand to what the sensor recorded.
    completions: (S,M,3), or a ragged (points (Q,3), offsets (S+1)) pair, in the scans' frame — what dataset.inverse_scale
    returns, not the normalised output of the model; viewpoints: where the sensor stood, one triple or (S,3), default
    dataset.viewpoints (seen_from, virtual_scans and from_depth_images set it); **visibility: resolution, window, margin, slope of
    ops.scan_visibility.
    Returns a dict: shares (S,4) float64 on the device — per scan the share of its completion's rows that are seen through
    (label 0: in the sensor's free space, the contradiction), on the surface (1), hidden (2) and unobserved (3: the sensor
    recorded nothing that way); rows with non-finite values (label 4) count in the denominator only, and a scan without rows
    has NaNs —, mean (4) float64 on the host, the shares' mean over the scans, and label (Q) uint8 on the device, aligned with
    the completions' rows, so a caller can carve the contradicted points out (label != 0) before inverse_scale_to_scene.
    One host transfer, for the means."""
    if not isinstance(dataset, DeviceScanDataset):
        raise TypeError("dataset must be a DeviceScanDataset")
    if viewpoints is None:
        viewpoints = dataset.viewpoints
    if viewpoints is None:
        raise ValueError("the dataset holds no viewpoints (seen_from, virtual_scans and from_depth_images set them): pass viewpoints")
    S, dev = len(dataset), dataset.device
    if isinstance(completions, tuple):
        points, offsets = completions
        points = torch.as_tensor(points, dtype=torch.float32).to(dev).contiguous()
        offsets = torch.as_tensor(offsets).to(device=dev, dtype=torch.int64).contiguous()
        if points.dim() != 2 or points.size(1) != 3 or tuple(offsets.shape) != (S + 1,):
            raise ValueError(f"a ragged completion set is points (Q,3) and offsets (S+1) with S = {S}")
    else:
        c = torch.as_tensor(completions, dtype=torch.float32)
        if c.dim() != 3 or c.size(0) != S or c.size(2) != 3:
            raise ValueError(f"completions must be (S,M,3) with S = {S}, got {tuple(c.shape)}")
        points = c.to(dev).reshape(-1, 3).contiguous()
        offsets = torch.arange(S + 1, dtype=torch.int64, device=dev) * c.size(1)
    label = ops.scan_visibility(dataset.points, dataset.offsets, viewpoints, queries=points, query_offsets=offsets,
                                **visibility)["label"]
    lengths = offsets[1:] - offsets[:-1]
    scan = torch.repeat_interleave(torch.arange(S, device=dev), lengths, output_size=points.size(0))
    counts = torch.zeros(S * 5, dtype=torch.int64, device=dev).index_add_(0, scan * 5 + label.to(torch.int64),
                                                                          torch.ones_like(scan)).view(S, 5)
    shares = counts[:, :4].to(torch.float64) / lengths.to(torch.float64).unsqueeze(1)
    return {"shares": shares, "mean": shares.mean(0).cpu(), "label": label}

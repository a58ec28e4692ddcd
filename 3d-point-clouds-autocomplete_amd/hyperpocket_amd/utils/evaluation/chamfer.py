"""utils/evaluation/chamfer.py — symmetric Chamfer distance of two point sets (the pair distance of TMD) on the HIP pair
kernel instead of two scipy KD-trees, and the unit-sphere normalisation.
"""
import numpy as np
import torch

from .cloud_pairs import CHAMFER, cloud_pairs


def compute_trimesh_chamfer(gt_points, gen_points, offset=0, scale=1):
    """gt_points (n, 3), gen_points (m, 3) numpy -> float: mean over gt of the squared distance to the nearest gen point
    plus mean over gen of the squared distance to the nearest gt point; gen is first mapped to gen / scale - offset."""
    gen = np.asarray(gen_points) / scale - offset
    dev = torch.device("cuda", torch.cuda.current_device())
    a = torch.as_tensor(np.asarray(gt_points), dtype=torch.float32, device=dev).unsqueeze(0).contiguous()
    b = torch.as_tensor(gen, dtype=torch.float32, device=dev).unsqueeze(0).contiguous()
    s = cloud_pairs(CHAMFER, a, b, [[0, 0]]).double()[0]
    return (s[0] / a.size(1) + s[1] / b.size(1)).item()


def scale_to_unit_sphere(points):
    """(n, 3) numpy: centre the bounding box at the origin, then divide by the largest norm."""
    centre = 0.5 * (points.max(axis=0) + points.min(axis=0))
    centred = points - centre
    return centred / np.linalg.norm(centred, axis=1).max()

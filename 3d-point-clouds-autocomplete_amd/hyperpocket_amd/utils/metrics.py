"""Evaluation consumers of the structural losses and the occupancy-grid JSD — the reference's
utils/metrics.py:44-359, same names, arguments and results, over the HIP kernels.

What is different underneath: Chamfer distances come from the fused nearest-neighbour kernel
(hp_nndistance) instead of the (B,N,N) `batch_pairwise_dist` tensor, EMD from the match-free path
(hp_emd_forward).  The JSD's occupancy histograms (the reference: sklearn NearestNeighbors plus a Python loop over every
point) come from hp_occupancy_grid (csrc/occupancy.hip); only the two integer vectors of at most R^3 entries cross to the
host, where entropy and divergence are fp64 numpy.
"""
import warnings

import numpy as np
import torch

from .._lib import HipExtensionError, call, check_input, current_stream
from .pytorch_structural_losses.match_cost import match_cost
from .evaluation.emd_exact import emd_exact_pairs
from .evaluation.emd_pairs import DEFAULT_WORKSPACE_BYTES, emd_pairs
from .evaluation.mmd import chamfer_pairs
from .pytorch_structural_losses.nn_distance import nn_distance


def emd_approx(sample, ref):
    """utils/metrics.py:71-76 — per-cloud approximate EMD divided by the number of points."""
    n, n_ref = sample.size(1), ref.size(1)
    assert n == n_ref, "Not sure what would EMD do in this case"
    return match_cost(sample.contiguous(), ref.contiguous()) / float(n)


def emd_exact(sample, ref):
    """emd_approx's figure from the exact assignment: per cloud the minimum over one-to-one matchings of the summed point
    distances (hp_assign_pairs), divided by the number of points.  (b, n, 3) against (b, n, 3) -> (b,) fp32, no gradients."""
    n, n_ref = sample.size(1), ref.size(1)
    assert n == n_ref, "Not sure what would EMD do in this case"
    b = sample.size(0)
    pairs = torch.arange(b, device=sample.device, dtype=torch.int32).view(-1, 1).expand(-1, 2)
    return (emd_exact_pairs(sample.contiguous(), ref.contiguous(), pairs) / float(n)).float()


def _emd_choice(emd):
    if emd not in ("approx", "exact"):
        raise ValueError(f"emd must be 'approx' or 'exact', got {emd!r}")
    return emd == "exact"


def earth_mover_distance(sample_pcs, ref_pcs, batch_size=None, emd="approx"):
    """utils/metrics.py:44-68; emd="exact": the exact assignment's cost (emd_exact) instead of the approximate matching's."""
    per_batch = emd_exact if _emd_choice(emd) else emd_approx
    sample_pcs, ref_pcs = sample_pcs.contiguous(), ref_pcs.contiguous()
    if sample_pcs.dim() == 2:
        sample_pcs = sample_pcs.unsqueeze(0)
    if ref_pcs.dim() == 2:
        ref_pcs = ref_pcs.unsqueeze(0)
    n_sample, n_ref = sample_pcs.shape[0], ref_pcs.shape[0]
    assert n_sample == n_ref, f'REF:{n_ref} SMP:{n_sample}'
    step = min(batch_size or n_sample, 300)
    return torch.cat([per_batch(sample_pcs[s:s + step], ref_pcs[s:s + step]) for s in range(0, n_sample, step)])


def dist_chamfer(x, y, chamfer_loss=None):
    """utils/metrics.py:78-83: (for every point of y its squared distance to the nearest point of x,
    for every point of x the same towards y).  `chamfer_loss` is accepted for signature parity and unused: the
    distances come from the NN kernel, not from its (B,Nx,Ny) matrix (they agree to ~1e-7)."""
    d_x, d_y = nn_distance(x.contiguous(), y.contiguous())
    return d_y, d_x


def EMD_CD(sample_pcs, ref_pcs, batch_size, reduced=True, chamfer_loss=None):
    """utils/metrics.py:86-118 (the reference calls dist_chamfer without its third argument there and would raise;
    the evident intent — element-wise CD and EMD of matching clouds — is what this computes)."""
    n_sample, n_ref = sample_pcs.shape[0], ref_pcs.shape[0]
    assert n_sample == n_ref, f'REF:{n_ref} SMP:{n_sample}'
    cd_lst, emd_lst = [], []
    for s in range(0, n_sample, batch_size):
        a, b = sample_pcs[s:s + batch_size].contiguous(), ref_pcs[s:s + batch_size].contiguous()
        dl, dr = dist_chamfer(a, b, chamfer_loss)
        cd_lst.append(dl.mean(dim=1) + dr.mean(dim=1))
        emd_lst.append(emd_approx(a, b))
    cd, emd = torch.cat(cd_lst), torch.cat(emd_lst)
    if reduced:
        cd, emd = cd.mean(), emd.mean()
    return {'MMD-CD': cd, 'MMD-EMD': emd}


def _pairwise_EMD_CD_(sample_pcs, ref_pcs, batch_size, chamfer_loss=None):
    """utils/metrics.py:121-158 — all (sample, ref) pairs: returns (N_sample, N_ref) CD and EMD matrices.  One kernel
    batch per (sample, ref chunk): the sample cloud is expanded against up to `batch_size` reference clouds."""
    n_sample, n_ref = sample_pcs.shape[0], ref_pcs.shape[0]
    all_cd, all_emd = [], []
    for i in range(n_sample):
        cd_row, emd_row = [], []
        for r in range(0, n_ref, batch_size):
            ref_batch = ref_pcs[r:r + batch_size].contiguous()
            sample_exp = sample_pcs[i].view(1, -1, 3).expand(ref_batch.size(0), -1, -1).contiguous()
            dl, dr = dist_chamfer(sample_exp, ref_batch, chamfer_loss)
            cd_row.append((dl.mean(dim=1) + dr.mean(dim=1)).view(1, -1))
            emd_row.append(emd_approx(sample_exp, ref_batch).view(1, -1))
        all_cd.append(torch.cat(cd_row, dim=1))
        all_emd.append(torch.cat(emd_row, dim=1))
    return torch.cat(all_cd, dim=0), torch.cat(all_emd, dim=0)


def knn(Mxx, Mxy, Myy, k, sqrt=False):
    """utils/metrics.py:162-191 — leave-one-out k-NN two-sample test on precomputed distance matrices."""
    n0, n1 = Mxx.size(0), Myy.size(0)
    label = torch.cat((torch.ones(n0), torch.zeros(n1))).to(Mxx)
    M = torch.cat((torch.cat((Mxx, Mxy), 1), torch.cat((Mxy.t(), Myy), 1)), 0)
    if sqrt:
        M = M.abs().sqrt()
    M = M + torch.diag(torch.full((n0 + n1,), float('inf')).to(Mxx))
    _, idx = M.topk(k, 0, False)
    votes = torch.zeros(n0 + n1).to(Mxx)
    for i in range(k):
        votes = votes + label.index_select(0, idx[i])
    pred = (votes >= float(k) / 2).float()
    s = {'tp': (pred * label).sum(), 'fp': (pred * (1 - label)).sum(),
         'fn': ((1 - pred) * label).sum(), 'tn': ((1 - pred) * (1 - label)).sum()}
    s.update({
        'precision': s['tp'] / (s['tp'] + s['fp'] + 1e-10),
        'recall': s['tp'] / (s['tp'] + s['fn'] + 1e-10),
        'acc_t': s['tp'] / (s['tp'] + s['fn'] + 1e-10),
        'acc_f': s['tn'] / (s['tn'] + s['fp'] + 1e-10),
        'acc': torch.eq(label, pred).float().mean(),
    })
    return s


def mmd_cov(all_dist):
    """utils/metrics.py:194-206 on an (N_sample, N_ref) distance matrix."""
    n_ref = all_dist.size(1)
    min_from_sample, min_idx = torch.min(all_dist, dim=1)
    min_to_ref, _ = torch.min(all_dist, dim=0)
    cov = torch.tensor(float(min_idx.unique().numel()) / float(n_ref)).to(all_dist)
    return {'mmd(Fidelity)': min_to_ref.mean(), 'cov(Coverage)': cov, 'mmd_smp': min_from_sample.mean()}


def compute_all_metrics(sample_pcs, ref_pcs, batch_size, chamfer_loss=None):
    """utils/metrics.py:209-238 (the 1-NN block is commented out in the reference as well)."""
    results = {}
    M_rs_cd, M_rs_emd = _pairwise_EMD_CD_(ref_pcs, sample_pcs, batch_size, chamfer_loss)
    results.update({"%s-CD" % k: v for k, v in mmd_cov(M_rs_cd.t()).items()})
    results.update({"%s-EMD" % k: v for k, v in mmd_cov(M_rs_emd.t()).items()})
    return results


# ---- the pair form: whole distance matrices in two calls, and the 1-NN two-sample accuracy on them --------------------------------
def pairwise_EMD_CD(sample_pcs, ref_pcs, workspace_bytes=None, emd="approx"):
    """_pairwise_EMD_CD_'s matrices — (N_sample, N_ref) fp32 CD and EMD, the EMD divided by the number of points — from ONE
    Chamfer call (hp_cloud_pairs) and ONE EMD call (hp_emd_pairs) over all N_sample * N_ref pairs: no expanded copy of a cloud,
    no Python loop over the samples.  `workspace_bytes` bounds the EMD's scratch (utils/evaluation/emd_pairs.py; None: its
    default).  The values agree with _pairwise_EMD_CD_'s to the regrouping of sums (1e-5), not bit for bit: the EMD runs another
    number of clouds per call, the Chamfer sums are fp64 here.
    emd="exact": the EMD matrix holds the exact assignment's cost per pair (hp_assign_pairs through emd_exact_pairs, fp64
    cast to fp32 once) divided by the number of points; `workspace_bytes` is then unused, the exact solver has no scratch."""
    exact = _emd_choice(emd)
    sample_pcs, ref_pcs = sample_pcs.contiguous(), ref_pcs.contiguous()
    n_sample, n_ref = sample_pcs.size(0), ref_pcs.size(0)
    n, n_of_ref = sample_pcs.size(1), ref_pcs.size(1)
    assert n == n_of_ref, "Not sure what would EMD do in this case"
    dev = sample_pcs.device
    pairs = torch.stack([torch.arange(n_sample, device=dev).repeat_interleave(n_ref),
                         torch.arange(n_ref, device=dev).repeat(n_sample)], 1).to(torch.int32)
    cd = chamfer_pairs(sample_pcs, ref_pcs, pairs).float()
    if exact:
        emd = (emd_exact_pairs(sample_pcs, ref_pcs, pairs) / float(n)).float()
    else:
        emd = emd_pairs(sample_pcs, ref_pcs, pairs, DEFAULT_WORKSPACE_BYTES if workspace_bytes is None else workspace_bytes) / float(n)
    return cd.view(n_sample, n_ref), emd.view(n_sample, n_ref)


def two_sample_metrics(sample_pcs, ref_pcs, ref_within=None, workspace_bytes=None, emd="approx"):
    """compute_all_metrics' six numbers plus the block the reference keeps commented out (utils/metrics.py:224-237): the
    leave-one-out 1-NN two-sample accuracy of arXiv:1707.02392 on the CD and on the EMD matrices, as keys "1-NN-CD-acc",
    "-acc_t", "-acc_f" and the same for EMD.  All matrices come from pairwise_EMD_CD.  `ref_within` = (M_rr_cd, M_rr_emd), the
    reference set's own matrices (pairwise_EMD_CD(ref_pcs, ref_pcs)), lets a caller with many sample sets compute them once.
    `emd` is pairwise_EMD_CD's: "exact" puts the exact assignment behind every EMD key (ref_within must then be exact too)."""
    results = {}
    M_rs_cd, M_rs_emd = pairwise_EMD_CD(ref_pcs, sample_pcs, workspace_bytes, emd)
    results.update({"%s-CD" % k: v for k, v in mmd_cov(M_rs_cd.t()).items()})
    results.update({"%s-EMD" % k: v for k, v in mmd_cov(M_rs_emd.t()).items()})
    M_rr_cd, M_rr_emd = pairwise_EMD_CD(ref_pcs, ref_pcs, workspace_bytes, emd) if ref_within is None else ref_within
    M_ss_cd, M_ss_emd = pairwise_EMD_CD(sample_pcs, sample_pcs, workspace_bytes, emd)
    one_nn_cd = knn(M_rr_cd, M_rs_cd, M_ss_cd, 1, sqrt=False)
    results.update({"1-NN-CD-%s" % k: v for k, v in one_nn_cd.items() if 'acc' in k})
    one_nn_emd = knn(M_rr_emd, M_rs_emd, M_ss_emd, 1, sqrt=False)
    results.update({"1-NN-EMD-%s" % k: v for k, v in one_nn_emd.items() if 'acc' in k})
    return results


# ---- JSD over occupancy grids (utils/metrics.py:244-359; the measure of arXiv:1707.02392) -----------------------------------
OCCUPANCY_MAX_RESOLUTION = 64      # HP_OCCUPANCY_MAX_R: klo / khi of a column are 6-bit fields


def _grid_axis(resolution):
    """One axis of cell centres, the reference's numbers bit for bit: i * spacing - 0.5 formed in fp64, stored as fp32."""
    spacing = 1.0 / float(resolution - 1)
    return (np.arange(resolution) * spacing - 0.5).astype(np.float32), spacing


def _grid_cells(resolution):
    """-> (centres (R^3, 3) fp32 in (i, j, k) row-major order, inside (R^3,) bool: centre within the sphere r = 0.5)."""
    axis, _ = _grid_axis(resolution)
    centres = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
    return centres, np.linalg.norm(centres, axis=1) <= 0.5


def unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """Centres of the resolution^3 cells of a grid over the cube [-0.5, 0.5]^3 and the cell spacing.  Unclipped: an
    (R, R, R, 3) fp32 array; clip_sphere: the (cells, 3) centres whose fp32 norm is at most 0.5, in row-major order."""
    _, spacing = _grid_axis(resolution)
    centres, inside = _grid_cells(resolution)
    if clip_sphere:
        return centres[inside], spacing
    return centres.reshape(resolution, resolution, resolution, 3), spacing


def _grid_columns(resolution, in_sphere):
    """The kernel's view of the kept cells (csrc/hp_occupancy.h): -> (axis (R,) fp32, columns (R*R,) uint32, cells).
    Column (i, j) keeps k in [klo, khi] with kept indices base + (k - klo); packed klo | khi << 6 | base << 12, klo > khi if
    it keeps nothing.  Membership is the numpy test of _grid_cells; that every column's kept cells are one run of k is
    checked here, not assumed."""
    R = resolution
    axis, _ = _grid_axis(R)
    kept = _grid_cells(R)[1].reshape(R * R, R) if in_sphere else np.ones((R * R, R), bool)
    count = kept.sum(axis=1)
    klo = np.where(count > 0, kept.argmax(axis=1), 1)
    khi = np.where(count > 0, R - 1 - kept[:, ::-1].argmax(axis=1), 0)
    if not np.array_equal(np.where(count > 0, khi - klo + 1, 0), count):
        raise AssertionError(f"kept cells of a grid column are not contiguous at resolution {R}")
    base = np.cumsum(count) - count          # row-major numbering of the kept cells
    columns = (klo | khi << 6 | base << 12).astype(np.uint32)
    return axis, columns, int(count.sum())


_GRID_TABLES = {}       # (resolution, in_sphere, device) -> (axis, columns, cells) with the two tables on the device


def _occupancy_counts(pclouds, grid_resolution, in_sphere):
    """-> (counters, clouds_hit): int32 numpy vectors over the kept cells, from hp_occupancy_grid.  `pclouds` (S, n, 3): a
    CUDA fp32 tensor (read in place) or anything numpy can view (converted to fp32 and uploaded once)."""
    R = int(grid_resolution)
    if R < 2 or R > OCCUPANCY_MAX_RESOLUTION:
        raise ValueError(f"grid resolution must be in [2, {OCCUPANCY_MAX_RESOLUTION}], got {grid_resolution}")
    if not isinstance(pclouds, torch.Tensor):
        host = np.ascontiguousarray(pclouds, dtype=np.float32)
        if not torch.cuda.is_available():
            raise HipExtensionError("the occupancy grid runs on the HIP kernel only: no GPU to upload the clouds to")
        pclouds = torch.from_numpy(host).cuda()
    if pclouds.dim() != 3 or pclouds.size(2) != 3 or pclouds.size(0) < 1 or pclouds.size(1) < 1:
        raise ValueError(f"clouds must be (count, points, 3) and not empty, got {tuple(pclouds.shape)}")
    if pclouds.is_cuda:
        pclouds = pclouds.contiguous()
    check_input(pclouds, "pclouds")
    dev = pclouds.device
    key = (R, bool(in_sphere), dev)
    if key not in _GRID_TABLES:
        axis, columns, cells = _grid_columns(R, bool(in_sphere))
        if cells == 0:
            raise ValueError(f"no cell centre of a resolution-{R} grid lies inside the sphere")
        _GRID_TABLES[key] = (torch.from_numpy(axis).to(dev), torch.from_numpy(columns.view(np.int32)).to(dev), cells)
    axis, columns, cells = _GRID_TABLES[key]
    out = torch.empty((2 * cells + 1,), dtype=torch.int32, device=dev)      # counters | clouds_hit | non-finite flag
    call("hp_occupancy_grid", pclouds.size(0), pclouds.size(1), pclouds, R, axis, columns, cells,
         out[:cells], out[cells:2 * cells], out[2 * cells:], current_stream(dev))
    host = out.cpu().numpy()
    if host[-1]:
        raise ValueError("point clouds contain NaN or infinity")
    return host[:cells], host[cells:2 * cells]


def entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False, verbose=False):
    """utils/metrics.py:279-318.  -> (mean over the cells of the entropy of "cell is hit by a cloud" estimated over the
    clouds, counters): counters[c] = points, over all clouds, whose nearest cell centre is c, as float64 numpy like the
    reference's.  Points outside the cube or sphere are counted at their nearest cell, not dropped; `verbose` warns about
    them (bounds with the reference's 1e-3 slack).  Non-finite coordinates raise ValueError."""
    counters, clouds_hit = _occupancy_counts(pclouds, grid_resolution, in_sphere)
    if verbose:
        pts = torch.as_tensor(pclouds)
        limit = 0.5 + 10e-4
        if pts.abs().max().item() > limit:
            warnings.warn('Point-clouds are not in unit cube.')
        if in_sphere and pts.double().pow(2).sum(dim=2).max().sqrt().item() > limit:
            warnings.warn('Point-clouds are not in unit sphere.')
    p = clouds_hit[clouds_hit > 0].astype(np.float64) / float(len(pclouds))
    q = 1.0 - p
    with np.errstate(divide='ignore', invalid='ignore'):
        per_cell = -(p * np.log(p) + np.where(q > 0, q * np.log(q), 0.0))
    return float(per_cell.sum()) / len(counters), counters.astype(np.float64)


def _entropy_bits(p):
    """Shannon entropy in bits of a probability vector (0 log 0 = 0)."""
    nz = p[p > 0]
    return float(-(nz * np.log2(nz)).sum())


def _kl_bits(a, b):
    both = np.logical_and(a > 0, b > 0)
    return float((a[both] * np.log2(a[both] / b[both])).sum())


def jensen_shannon_divergence(P, Q):
    """utils/metrics.py:321-359: JSD in bits of two non-negative count vectors, as H(M) - (H(P) + H(Q)) / 2 with
    M = (P + Q) / 2; the KL form is computed next to it and a disagreement beyond 1e-4 warns."""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    if np.any(P < 0) or np.any(Q < 0):
        raise ValueError('Negative values.')
    if len(P) != len(Q):
        raise ValueError('Non equal size.')
    p, q = P / P.sum(), Q / Q.sum()
    m = 0.5 * (p + q)
    res = _entropy_bits(m) - 0.5 * (_entropy_bits(p) + _entropy_bits(q))
    if abs(res - 0.5 * (_kl_bits(p, m) + _kl_bits(q, m))) > 10e-5:
        warnings.warn('Numerical values of two JSD methods don\'t agree.')
    return res


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, resolution=28):
    """utils/metrics.py:265-276: JSD between the occupancy histograms of two sets of clouds, (S1, n1, 3) and (S2, n2, 3),
    on the resolution^3 grid clipped to the sphere.  CUDA tensors stay on the device."""
    sample_counts = entropy_of_occupancy_grid(sample_pcs, resolution, True)[1]
    ref_counts = entropy_of_occupancy_grid(ref_pcs, resolution, True)[1]
    return jensen_shannon_divergence(sample_counts, ref_counts)

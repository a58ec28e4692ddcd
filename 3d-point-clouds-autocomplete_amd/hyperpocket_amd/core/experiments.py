"""Three experiments of the reference's core/experiments.py, results written under its paths, names and keys:
fixed (:23-60) — noises_per_item completions of every test input, written as the `fixed/` directory the completion metrics
read —, evaluate_generativity (:63-104) — per category MMD / coverage (CD and EMD) and JSD of K sampled completions of every test
object against the category's missing parts — and compute_mmd_tmd_uhd (:107-128) — the three completion numbers for a
`fixed/` directory of reconstructions.  The other experiments of that file (plots, t-SNE, submissions) are out of scope."""
import json
import os
import shutil

import numpy as np

import torch
from torch.utils.data import DataLoader

from ..datasets.scan_dataset import DeviceScanDataset, ScanBatcher
from ..utils.metrics import compute_all_metrics, jsd_between_point_cloud_sets, pairwise_EMD_CD, two_sample_metrics
from ..utils.evaluation.completeness import process as uhd_process
from ..utils.evaluation.mmd import process as mmd_process
from ..utils.evaluation.total_mutual_diff import process as tmd_process


FIXED_POINTS = 2048         # points per completion of fixed()


def _fixed_batches(source, batch_size, device):
    """(existing (B,n,3) on `device`, rows per batch) of one category: a ScanBatcher as it is, a DeviceScanDataset through a
    ScanBatcher of its own, any other dataset of (existing, missing, gt, idx) items through a DataLoader in item order."""
    if isinstance(source, DeviceScanDataset):
        source = ScanBatcher(source, batch_size)
    if isinstance(source, ScanBatcher):
        return (batch[0] for batch in source), source.batch_size
    loader = DataLoader(source, batch_size=batch_size, generator=torch.Generator())
    return (batch[0].to(device, torch.float32) for batch in loader), batch_size


def fixed(full_model, device, datasets_dict, results_dir, epoch, amount=30, mean=0.0, std=0.015, noises_per_item=10,
          batch_size=8, save_plots=False, triangulation_config=None):
    """Clears and refills results_dir/fixed with the files utils/evaluation/shape_dir.py describes: per category `cat`, batch i
    and row k, with item = i * batch_size + k, `<cat>_<item>_<j>_reconstruction.npy` (3, 2048) for j < noises_per_item and
    `<cat>_<item>_existing.npy` (3, n).  `datasets_dict`: category -> DeviceScanDataset (batched by a ScanBatcher with its
    defaults: 1024 points, not normalised), a ScanBatcher (its own batch size and resampling), or any map-style dataset of
    (existing, missing, gt, idx) items (batched by a DataLoader).  For density-biased scans pass
    ScanBatcher(..., resample="farthest"): every kept point is then a farthest-point pick, still a row of its scan.

    Random numbers: per batch, noises_per_item draws of (B, noise_size) normal(mean, std) rows on the CPU from torch's
    global generator, in j order — the reference's calls; the data loader has a generator of its own.  The batch is encoded
    once (FullModel.encode_existing) and decoded once per noise; the completions of a batch reach the host in one copy.
    `amount` and `triangulation_config` are accepted for signature parity and unused, as in the reference; so is
    `save_plots` — plotting is out of scope.

    Returns (existing_list, generated): one (n,3) device tensor per item in writing order, and all completions as one
    (items, noises_per_item, 2048, 3) device tensor — torch.stack(existing_list) and `generated` are completion_metrics' inputs."""
    out_dir = os.path.join(results_dir, 'fixed')
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    conditioned = full_model.mode.conditioned
    existing_list, generated = [], []
    was_training = full_model.training
    full_model.eval()
    try:
        with torch.no_grad():
            for cat_name, source in datasets_dict.items():
                batches, rows = _fixed_batches(source, batch_size, device)
                for i, existing in enumerate(batches):
                    B = existing.size(0)
                    noises = [torch.empty(B, full_model.get_noise_size()).normal_(mean=mean, std=std)
                              for _ in range(noises_per_item)]
                    code = full_model.encode_existing(existing) if conditioned else None
                    recs = torch.stack([full_model.sample_completions(existing, noise.to(device), FIXED_POINTS, epoch, code=code)
                                        for noise in noises], 1)                        # (B, noises, 3, 2048)
                    recs_host, existing_host = recs.cpu().numpy(), existing.transpose(1, 2).contiguous().cpu().numpy()
                    for k in range(B):
                        stem = os.path.join(out_dir, f'{cat_name}_{i * rows + k}')
                        for j in range(noises_per_item):
                            np.save(f'{stem}_{j}_reconstruction', recs_host[k, j])
                        np.save(f'{stem}_existing', existing_host[k])
                        existing_list.append(existing[k].clone())
                    generated.append(recs.permute(0, 1, 3, 2).contiguous())
    finally:
        full_model.train(was_training)
    return existing_list, torch.cat(generated)


def compute_mmd_tmd_uhd(full_model, device, dataset, results_dir, epoch, batch_size=64):
    """Reads results_dir/fixed, writes results_dir/compute_mmd_tmd_uhd/<epoch>res.json and returns the same dict.
    `full_model` is unused (signature parity: the reconstructions are already on disk)."""
    shape_dir = os.path.join(results_dir, 'fixed')
    res = {}
    for key, scale, value in (('MMD * 1000', 1000, lambda: mmd_process(shape_dir, dataset, device, batch_size)),
                              ('UHD * 100', 100, lambda: uhd_process(shape_dir)),
                              ('TMD * 100', 100, lambda: tmd_process(shape_dir))):
        res[key] = float(value()) * scale
        print(key, res[key])
    out_dir = os.path.join(results_dir, 'compute_mmd_tmd_uhd')
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, str(epoch) + 'res.json'), mode='w') as f:
        json.dump(res, f)
    return res


SAMPLE_CHUNK = 64           # completions decoded per sample_completions call
SAMPLE_POINTS = 2048        # points per completion, of which the KEPT_POINTS with the smallest y are evaluated
KEPT_POINTS = 1024


def lowest_y_half(recs, keep=KEPT_POINTS):
    """recs (K, 3, N) -> (K, keep, 3): of every cloud the `keep` points with the smallest y, ascending in y (equal y in
    their original order), selected on the device."""
    order = torch.argsort(recs[:, 1, :], dim=1, stable=True)[:, :keep]
    return torch.gather(recs.permute(0, 2, 1), 1, order.unsqueeze(2).expand(-1, -1, 3)).contiguous()


def evaluate_generativity(full_model, device, datasets_dict, results_dir, epoch, batch_size, num_workers, mean=0.0,
                          std=0.005, one_nn=False):
    """`datasets_dict`: category -> dataset of (existing, missing, gt, idx) items.  Per category, with cat_gt the missing
    parts of all its objects: every object gets K = len(cat_gt) completions of 2048 points, each cut to its 1024 lowest-y
    points, and compute_all_metrics(completions, cat_gt, batch_size) plus jsd_between_point_cloud_sets(completions, cat_gt)
    are summed over the objects (summed, as the reference does, not averaged).  Writes
    results_dir/evaluate_generativity/<epoch>eval_gen_by_cat.json and returns the same dict.

    Random numbers: the K noises of an object are one (K, noise_size) normal(mean, std) draw on the CPU from torch's global
    generator (the reference makes K draws of one row each: the same distribution, another stream); the data loader has a
    generator of its own, so the global stream holds the noise draws only, in category and object order.  The partial cloud
    is encoded once per chunk of at most 64 completions (FullModel.sample_completions), everything stays on the device
    until the per-object scalars.

    one_nn=True: every object goes through two_sample_metrics(completions, cat_gt) instead of compute_all_metrics — the same six
    keys (from the pair kernels: values equal to the regrouping of sums, `batch_size` unused) plus the 1-NN two-sample accuracies
    "1-NN-CD-acc" / "-acc_t" / "-acc_f" and the same for EMD, summed over the objects like the others.  The category's own
    matrices (cat_gt against cat_gt) are computed once per category."""
    was_training = full_model.training
    full_model.eval()
    results = {}
    try:
        with torch.no_grad():
            for cat_name, cat_ds in datasets_dict.items():
                loader = DataLoader(cat_ds, batch_size=1, num_workers=num_workers, generator=torch.Generator())
                partial, cat_gt = [], []
                for existing, missing, _, _ in loader:
                    partial.append(existing.to(device, torch.float32))
                    cat_gt.append(missing.to(device, torch.float32))
                cat_gt = torch.cat(cat_gt).contiguous()
                K = cat_gt.size(0)
                cat_results = {}
                ref_within = pairwise_EMD_CD(cat_gt, cat_gt) if one_nn else None
                for existing in partial:
                    noise = torch.empty(K, full_model.get_noise_size()).normal_(mean=mean, std=std).to(device)
                    obj_recs = torch.cat([
                        lowest_y_half(full_model.sample_completions(existing, noise[s:s + SAMPLE_CHUNK], SAMPLE_POINTS, epoch))
                        for s in range(0, K, SAMPLE_CHUNK)])
                    if one_nn:
                        for k, v in two_sample_metrics(obj_recs, cat_gt, ref_within).items():
                            cat_results[k] = cat_results.get(k, 0.0) + v.item()
                        cat_results['jsd'] = cat_results.get('jsd', 0.0) + jsd_between_point_cloud_sets(obj_recs, cat_gt)
                        continue
                    for k, v in compute_all_metrics(obj_recs, cat_gt, batch_size).items():
                        cat_results[k] = cat_results.get(k, 0.0) + v.item()
                    cat_results['jsd'] = cat_results.get('jsd', 0.0) + jsd_between_point_cloud_sets(obj_recs, cat_gt)
                results[cat_name] = cat_results
                print(cat_name, cat_results)
    finally:
        full_model.train(was_training)
    out_dir = os.path.join(results_dir, 'evaluate_generativity')
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, str(epoch) + 'eval_gen_by_cat.json'), mode='w') as f:
        json.dump(results, f)
    return results

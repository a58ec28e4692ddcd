"""The two evaluation experiments of the reference's core/experiments.py, results written as JSON under its paths and keys:
evaluate_generativity (:63-104) — per category MMD / coverage (CD and EMD) and JSD of K sampled completions of every test
object against the category's missing parts — and compute_mmd_tmd_uhd (:107-128) — the three completion numbers for a
`fixed/` directory of reconstructions.  The other experiments of that file (plots, t-SNE, submissions) are out of scope."""
import json
import os

import torch
from torch.utils.data import DataLoader

from ..utils.metrics import compute_all_metrics, jsd_between_point_cloud_sets
from ..utils.evaluation.completeness import process as uhd_process
from ..utils.evaluation.mmd import process as mmd_process
from ..utils.evaluation.total_mutual_diff import process as tmd_process


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
                          std=0.005):
    """`datasets_dict`: category -> dataset of (existing, missing, gt, idx) items.  Per category, with cat_gt the missing
    parts of all its objects: every object gets K = len(cat_gt) completions of 2048 points, each cut to its 1024 lowest-y
    points, and compute_all_metrics(completions, cat_gt, batch_size) plus jsd_between_point_cloud_sets(completions, cat_gt)
    are summed over the objects (summed, as the reference does, not averaged).  Writes
    results_dir/evaluate_generativity/<epoch>eval_gen_by_cat.json and returns the same dict.

    Random numbers: the K noises of an object are one (K, noise_size) normal(mean, std) draw on the CPU from torch's global
    generator (the reference makes K draws of one row each: the same distribution, another stream); the data loader has a
    generator of its own, so the global stream holds the noise draws only, in category and object order.  The partial cloud
    is encoded once per chunk of at most 64 completions (FullModel.sample_completions), everything stays on the device
    until the per-object scalars."""
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
                for existing in partial:
                    noise = torch.empty(K, full_model.get_noise_size()).normal_(mean=mean, std=std).to(device)
                    obj_recs = torch.cat([
                        lowest_y_half(full_model.sample_completions(existing, noise[s:s + SAMPLE_CHUNK], SAMPLE_POINTS, epoch))
                        for s in range(0, K, SAMPLE_CHUNK)])
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

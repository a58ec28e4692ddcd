"""core/experiments.py:107-128 — compute_mmd_tmd_uhd: the paper's three completion numbers for a `fixed/` directory of
reconstructions, written as JSON under the reference's keys.  The other experiments of that file (generation, plots,
t-SNE) are out of scope."""
import json
import os

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

"""Five experiments of the reference's core/experiments.py, results written under its paths, names and keys:
fixed (:23-60) — noises_per_item completions of every test input, written as the `fixed/` directory the completion metrics
read —, evaluate_generativity (:63-104) — per category MMD / coverage (CD and EMD) and JSD of K sampled completions of every test
object against the category's missing parts —, compute_mmd_tmd_uhd (:107-128) — the three completion numbers for a
`fixed/` directory of reconstructions —, merge_different_categories (:131-191) — shapes of two categories cut in two along an
axis, every kept half completed with the latent of every removed half — and same_model_different_slices (:194-225) — both
sides of several random-plane cuts of a shape, each completed under a noise of its own.  fixed's `triangulation_config`, which
the reference accepts and ignores, is carried out here: mesh_completions decodes a triangulated sphere into a watertight mesh of
every completion and samples its surface.  The PNGs the reference draws with matplotlib — fixed(save_plots=True), every
same_model_different_slices run — are rendered on the device here (utils/render.py: depth-shaded splats under the reference's
camera, no titles or axes) behind `save_plots`.  What remains out of scope is the t-SNE scatter plot and the submission zip."""
import json
import os
import shutil

import numpy as np

import torch
from torch.utils.data import DataLoader

from .. import ops
from ..datasets.scan_dataset import DeviceScanDataset, ScanBatcher
from ..utils.render import render_clouds, write_png
from ..utils.sphere_mesh import SphereMesh, sphere_mesh
from ..utils.tsne import tsne
from ..utils.metrics import (compute_all_metrics, jsd_between_point_cloud_sets, mmd_cov, pairwise_EMD_CD,
                             two_sample_metrics)
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


def mesh_to_device(mesh, device):
    """A utils/sphere_mesh.py SphereMesh of numpy arrays as one of device tensors: uploaded once, used for every completion."""
    if isinstance(mesh.vertices, torch.Tensor):
        return mesh
    up = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(device, dtype)
    return SphereMesh(up(mesh.vertices, torch.float32), up(mesh.faces, torch.int32),
                      tuple(up(a, torch.int32) for a in mesh.vertex_faces))


def mesh_completions(full_model, existing, noises, mesh, epoch, n_surface=2048, seed=0, code=None, streams=None):
    """K completions as watertight meshes with their surfaces sampled, eval mode only.  `mesh`: a SphereMesh (mesh_to_device's
    result, or numpy arrays, uploaded here); `noises` (K, noise_size) on the device; existing / code as sample_completions
    takes them.  The sphere's V vertices go through each noise row's target network (FullModel.sample_meshes: no random
    numbers), ops.mesh_normals gives area-weighted vertex normals over the shared face list, and ops.mesh_sample draws
    n_surface points per mesh uniformly by area under (seed, streams — default arange(K)): what CD, EMD, UHD, TMD and JSD of a
    mesh should be computed on, since the decoded vertices themselves crowd where the map contracts.
    Returns {"vertices" (K,V,3), "vertex_normals" (K,V,3), "surface" (K,n_surface,3), "surface_face" (K,n_surface) int32,
    "area" (K) float64, "failed" (K) int32}, all on the device; nothing is synchronised once the mesh has been seen."""
    mesh = mesh_to_device(mesh, noises.device)
    with torch.no_grad():
        vertices = full_model.sample_meshes(existing, noises, mesh.vertices, epoch, code=code).contiguous()
        normals = ops.mesh_normals(vertices, mesh.faces, mesh.vertex_faces)
        surface, surface_face, area, failed = ops.mesh_sample(vertices, mesh.faces, n_surface, seed, streams)
    return {"vertices": vertices, "vertex_normals": normals, "surface": surface, "surface_face": surface_face, "area": area,
            "failed": failed}


def write_obj(path, vertices, normals, faces_text):
    """A Wavefront file of one mesh: `v` and `vn` lines of float32 values in 9 significant digits (they read back to the same
    bits), then `faces_text`, the `f a//a b//b c//c` lines (1-based) shared by every mesh of a sphere (obj_faces_text)."""
    with open(path, 'w') as f:
        f.write(''.join('v %.9g %.9g %.9g\n' % tuple(r) for r in vertices.tolist()))
        f.write(''.join('vn %.9g %.9g %.9g\n' % tuple(r) for r in normals.tolist()))
        f.write(faces_text)


def obj_faces_text(faces):
    return ''.join('f %d//%d %d//%d %d//%d\n' % (a, a, b, b, c, c) for a, b, c in (np.asarray(faces) + 1).tolist())


def _write_plots(stems, clouds):
    """One PNG per cloud of `clouds` (N,n,3) on the device, `stems[i] + '.png'`: one render launch, one host copy, no random
    numbers."""
    images = render_clouds(clouds)[:, 0].cpu().numpy()
    for stem, image in zip(stems, images):
        write_png(stem + '.png', image)


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
    `amount` is accepted for signature parity and unused, as in the reference.

    save_plots=True adds the reference's pictures under its names: `<cat>_<item>_<j>_fixed_reconstructed.png` and
    `<cat>_<item>_existing.png`, each utils/render.py's default rendering of the array saved beside it.  A batch's completions
    are drawn in one launch from the tensors already on the device.  Drawing takes no random numbers: every other file, both
    global generators and the return value are the same with and without it.

    `triangulation_config` = {'execute': True, 'method': m, 'depth': d} (the reference's sample configs carry it; the
    reference ignores it) adds, per completion j of an item, `<cat>_<item>_<j>_mesh.obj` — the sphere sphere_mesh(m, d, outward=True) decoded
    under the noise and code of `..._<j>_reconstruction.npy`, with vertex normals (write_obj) — and
    `<cat>_<item>_<j>_surface.npy` (3, 2048), ops.mesh_sample's points under seed triangulation_config.get('seed', 0) and
    stream = the completion's running number, item * noises_per_item + j with items counted over all categories in writing
    order.  Neither name matches shape_dir.py's globs.  The mesh pass draws no random numbers, so every other file, the global
    generator and the return value are the same with and without it; absent or with 'execute' false nothing is added.

    Returns (existing_list, generated): one (n,3) device tensor per item in writing order, and all completions as one
    (items, noises_per_item, 2048, 3) device tensor — torch.stack(existing_list) and `generated` are completion_metrics' inputs."""
    out_dir = os.path.join(results_dir, 'fixed')
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    conditioned = full_model.mode.conditioned
    existing_list, generated = [], []
    mesh = None
    if triangulation_config and triangulation_config.get('execute'):
        mesh = mesh_to_device(sphere_mesh(triangulation_config['method'], int(triangulation_config['depth']), outward=True), device)
        faces_text, mesh_seed = obj_faces_text(mesh.faces.cpu().numpy()), int(triangulation_config.get('seed', 0))
    was_training = full_model.training
    full_model.eval()
    try:
        with torch.no_grad():
            for cat_name, source in datasets_dict.items():
                batches, rows = _fixed_batches(source, batch_size, device)
                for i, existing in enumerate(batches):
                    B = existing.size(0)
                    first = len(existing_list)                                          # running number of the batch's first item
                    noises = [torch.empty(B, full_model.get_noise_size()).normal_(mean=mean, std=std)
                              for _ in range(noises_per_item)]
                    code = full_model.encode_existing(existing) if conditioned else None
                    recs = torch.stack([full_model.sample_completions(existing, noise.to(device), FIXED_POINTS, epoch, code=code)
                                        for noise in noises], 1)                        # (B, noises, 3, 2048)
                    clouds = recs.permute(0, 1, 3, 2).contiguous()                      # (B, noises, 2048, 3)
                    if save_plots:
                        stems = [os.path.join(out_dir, f'{cat_name}_{i * rows + k}') for k in range(B)]
                        _write_plots([f'{stem}_{j}_fixed_reconstructed' for stem in stems for j in range(noises_per_item)],
                                     clouds.flatten(0, 1))
                        _write_plots([f'{stem}_existing' for stem in stems], existing)
                    recs_host, existing_host = recs.cpu().numpy(), existing.transpose(1, 2).contiguous().cpu().numpy()
                    if mesh is not None:
                        item = torch.arange(first, first + B, dtype=torch.int64, device=device)
                        meshes = [mesh_completions(full_model, existing, noise.to(device), mesh, epoch, FIXED_POINTS, mesh_seed,
                                                   code, item * noises_per_item + j) for j, noise in enumerate(noises)]
                        verts_host, normals_host, surface_host = (
                            torch.stack([m[name] for m in meshes], 1).cpu().numpy()     # (B, noises, ..)
                            for name in ('vertices', 'vertex_normals', 'surface'))
                    for k in range(B):
                        stem = os.path.join(out_dir, f'{cat_name}_{i * rows + k}')
                        for j in range(noises_per_item):
                            np.save(f'{stem}_{j}_reconstruction', recs_host[k, j])
                            if mesh is not None:
                                write_obj(f'{stem}_{j}_mesh.obj', verts_host[k, j], normals_host[k, j], faces_text)
                                np.save(f'{stem}_{j}_surface', np.ascontiguousarray(surface_host[k, j].T))
                        np.save(f'{stem}_existing', existing_host[k])
                        existing_list.append(existing[k].clone())
                    generated.append(clouds)
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
                          std=0.005, one_nn=False, emd="approx"):
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
    matrices (cat_gt against cat_gt) are computed once per category.

    emd="exact": every EMD figure comes from the exact assignment (utils/evaluation/emd_exact.py) instead of the approximate
    matching; without one_nn the six keys then come from pairwise_EMD_CD's matrices, as they do with it.  The default leaves
    every result as it was."""
    if emd not in ("approx", "exact"):
        raise ValueError(f"emd must be 'approx' or 'exact', got {emd!r}")
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
                ref_within = pairwise_EMD_CD(cat_gt, cat_gt, emd=emd) if one_nn else None
                for existing in partial:
                    noise = torch.empty(K, full_model.get_noise_size()).normal_(mean=mean, std=std).to(device)
                    obj_recs = torch.cat([
                        lowest_y_half(full_model.sample_completions(existing, noise[s:s + SAMPLE_CHUNK], SAMPLE_POINTS, epoch))
                        for s in range(0, K, SAMPLE_CHUNK)])
                    if one_nn:
                        for k, v in two_sample_metrics(obj_recs, cat_gt, ref_within, emd=emd).items():
                            cat_results[k] = cat_results.get(k, 0.0) + v.item()
                        cat_results['jsd'] = cat_results.get('jsd', 0.0) + jsd_between_point_cloud_sets(obj_recs, cat_gt)
                        continue
                    if emd == "exact":
                        M_cd, M_emd = pairwise_EMD_CD(cat_gt, obj_recs, emd=emd)
                        six = {"%s-CD" % k: v for k, v in mmd_cov(M_cd.t()).items()}
                        six.update({"%s-EMD" % k: v for k, v in mmd_cov(M_emd.t()).items()})
                    else:
                        six = compute_all_metrics(obj_recs, cat_gt, batch_size)
                    for k, v in six.items():
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


def mix_completions(full_model, existing, missing, pairs, n_points, epoch, *, points=None):
    """Completions of kept parts under the latents of removed parts, eval mode only: existing (E,n,3), missing (M,n',3) and
    pairs (P,2) integer rows (existing row i, missing row j) -> (P, 3, n_points), row p being what forward(existing[i],
    missing[j]) decodes.  Each encoder runs once, over all its rows (FullModel.encode_existing / encode_missing); the pairs
    are decoded in chunks of at most SAMPLE_CHUNK by sample_completions(None, mean[j], ..., code=code[i]).  `points`
    (P, n_points, 3) injects the decoder's input, otherwise the model's sampler draws once per chunk."""
    pairs = torch.as_tensor(pairs, dtype=torch.long, device=existing.device)
    if pairs.dim() != 2 or pairs.size(1) != 2:
        raise ValueError(f"pairs must be (P, 2), got {tuple(pairs.shape)}")
    with torch.no_grad():
        code, mean = full_model.encode_existing(existing), full_model.encode_missing(missing)
        recs = [full_model.sample_completions(None, mean[chunk[:, 1]], n_points, epoch, code=code[chunk[:, 0]],
                                              points=None if points is None else points[s:s + SAMPLE_CHUNK])
                for s, chunk in ((s, pairs[s:s + SAMPLE_CHUNK]) for s in range(0, pairs.size(0), SAMPLE_CHUNK))]
    return torch.cat(recs)


def _gt_clouds(dataset, ids, device):
    """The gt clouds (third field) of the items `ids` of a map-style dataset, stacked (len(ids), n, 3) on `device`."""
    return torch.stack([torch.as_tensor(np.asarray(dataset[int(i)][2]), dtype=torch.float32) for i in ids]).to(device)


def merge_different_categories(full_model, device, dataset, results_dir, epoch, amount=10, first_cat='car',
                               second_cat='airplane', axis=0, as_reference=False):
    """Clears and refills results_dir/merge_different_categories.  `dataset`: category -> map-style dataset of (existing,
    missing, gt, idx) items, of which only gt (n,3) is read.  `amount` items of each of the two categories are drawn
    (np.random.choice without replacement on numpy's global generator, first category first), and every gt is cut in two by
    the rank of its `axis` coordinate in one ops.axis_split call with k = n // 2: the k lowest rows are its missing part, the
    others its existing part, both in rank order (equal coordinates in row order — the reference's argsort leaves those
    unspecified).  Every existing part is then completed with the posterior mean of every missing part, within and across the
    categories: 4 * amount**2 completions of 2048 points from one mix_completions call, so each encoder runs once where the
    reference runs both at batch 1 for every pair.  Each kind of result reaches the host in one copy.

    Files, with a, b the two category names and i, j < amount: `<a>_<i>_existing.npy` (n-k,3), `<a>_<i>_missing.npy` (k,3),
    `<a>_<i>_gt.npy` (n,3) and `<a>_<i>~<b>_<j>_rec.npy` (2048,3), the existing part of a's item i under the missing part of
    b's item j.

    The reference has two slips here.  It draws the second category's ids from the first category's length (:141); ours come
    from the second's.  And its second~second completion is decoded from the first category's missing part (:189), a copy of
    second~first up to the decoder's point draw; ours uses the second's, and as_reference=True reproduces that slip for a
    user comparing files.  A category with fewer than `amount` items is a ValueError, as in the reference.

    Returns (parts, recs): parts = {"existing": (2, amount, n-k, 3), "missing": (2, amount, k, 3), "gt": (2, amount, n, 3)}
    device tensors, recs (2, 2, amount, amount, 2048, 3) indexed [existing category, missing category, i, j]."""
    cats = (first_cat, second_cat)
    sizes = [len(dataset[cat]) for cat in cats]
    if min(sizes) < amount:
        raise ValueError(f'with current dataset config the max amount value is {min(sizes)}')
    ids = [np.random.choice(size, amount, replace=False) for size in sizes]
    out_dir = os.path.join(results_dir, 'merge_different_categories')
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    was_training = full_model.training
    full_model.eval()
    try:
        with torch.no_grad():
            gt = torch.cat([_gt_clouds(dataset[cat], chosen, device) for cat, chosen in zip(cats, ids)])
            n = gt.size(1)
            missing, existing, _ = ops.axis_split(gt, n // 2, axis)
            # row of category c, item i: c * amount + i
            pairs = [(a * amount + i, (0 if as_reference and a == b == 1 else b) * amount + j)
                     for a in range(2) for b in range(2) for i in range(amount) for j in range(amount)]
            recs = mix_completions(full_model, existing, missing, pairs, FIXED_POINTS, epoch)
            recs = recs.permute(0, 2, 1).contiguous().view(2, 2, amount, amount, FIXED_POINTS, 3)
    finally:
        full_model.train(was_training)
    parts = {name: t.view(2, amount, t.size(1), 3) for name, t in (('existing', existing), ('missing', missing), ('gt', gt))}
    recs_host = recs.cpu().numpy()
    for name, t in parts.items():
        host = t.cpu().numpy()
        for c, cat in enumerate(cats):
            for i in range(amount):
                np.save(os.path.join(out_dir, f'{cat}_{i}_{name}'), host[c, i])
    for a, b in ((a, b) for a in range(2) for b in range(2)):
        for i in range(amount):
            for j in range(amount):
                np.save(os.path.join(out_dir, f'{cats[a]}_{i}~{cats[b]}_{j}_rec'), recs_host[a, b, i, j])
    return parts, recs


def same_model_different_slices(full_model, device, datasets_dict, results_dir, epoch, amount=10, slices_number=10,
                                mean=0.0, std=0.015, seed=0, save_plots=False):
    """Clears and refills results_dir/same_model_different_slices.  `datasets_dict`: category -> map-style dataset of
    (existing, missing, gt, idx) items, of which only gt (n,3), n even, is read.  Per category `amount` items are drawn
    (np.random.choice without replacement on numpy's global generator); item i gets slices_number random-plane cuts into
    two halves of n // 2 points (1024 of the reference's 2048) from one ops.slice_clouds call on the item repeated, and both
    sides of every cut are completed to 2048 points under one noise each.

    Random numbers: the planes are the device's Philox planes of slice_clouds (datasets/utils/dataset_generator.py) under
    seed + the item's running number over all categories, so items do not share their candidates; the reference draws them
    from numpy's global generator.  The noises are (1, noise_size) normal(mean, std) draws on the CPU from torch's global
    generator in the reference's order: item i, cut j, side f then s.  The 2 * slices_number parts of an item are encoded in
    one pass and decoded by one sample_completions call with one part per noise row.

    Files, with j < slices_number and side f (the half slice_clouds returns first) or s: `<cat>_<i>_gt.npy` (n,3),
    `<cat>_<i>_<j>_<side>_pcd.npy` (n/2,3), `..._noise.npy` (1, noise_size) and `..._rec.npy` (3,2048).  save_plots=True adds
    the reference's pictures, which it draws unconditionally: `<cat>_<i>_gt.png` and `<cat>_<i>_<j>_<side>_rec.png`, each
    utils/render.py's default rendering of the array saved beside it, an item's completions in one launch.  Drawing takes no
    random numbers: every other file, both global generators and the return value are the same with and without it.

    Returns the completions as one (categories * amount, slices_number, 2, 2048, 3) device tensor in writing order."""
    out_dir = os.path.join(results_dir, 'same_model_different_slices')
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    conditioned = full_model.mode.conditioned
    generated = []
    was_training = full_model.training
    full_model.eval()
    try:
        with torch.no_grad():
            for cat_name, ds in datasets_dict.items():
                ids = np.random.choice(len(ds), amount, replace=False)
                for i, idx in enumerate(ids):
                    gt = _gt_clouds(ds, [idx], device)
                    n = gt.size(1)
                    if n % 2:
                        raise ValueError(f"gt clouds must have an even number of points to cut in halves, got {n}")
                    first, second, _ = ops.slice_clouds(gt.expand(slices_number, -1, -1), n // 2, seed + len(generated))
                    sides = torch.stack([first, second], 1).flatten(0, 1)               # (2 * slices, n/2, 3): j major, f then s
                    noises = torch.cat([torch.empty(1, full_model.get_noise_size()).normal_(mean=mean, std=std)
                                        for _ in range(2 * slices_number)])
                    code = full_model.encode_existing(sides) if conditioned else None
                    recs = full_model.sample_completions(sides, noises.to(device), FIXED_POINTS, epoch, code=code)
                    stem = os.path.join(out_dir, f'{cat_name}_{i}')
                    np.save(f'{stem}_gt', gt[0].cpu().numpy())
                    sides_host, noises_host, recs_host = sides.cpu().numpy(), noises.numpy(), recs.cpu().numpy()
                    for j in range(slices_number):
                        for s, side in enumerate('fs'):
                            np.save(f'{stem}_{j}_{side}_pcd', sides_host[2 * j + s])
                            np.save(f'{stem}_{j}_{side}_noise', noises_host[2 * j + s:2 * j + s + 1])
                            np.save(f'{stem}_{j}_{side}_rec', recs_host[2 * j + s])
                    clouds = recs.permute(0, 2, 1).contiguous()                         # (2 * slices, 2048, 3)
                    if save_plots:
                        _write_plots([f'{stem}_gt'], gt)
                        _write_plots([f'{stem}_{j}_{side}_rec' for j in range(slices_number) for side in 'fs'], clouds)
                    generated.append(clouds.view(slices_number, 2, FIXED_POINTS, 3))
    finally:
        full_model.train(was_training)
    return torch.stack(generated)


ENCODE_CHUNK = 64           # rows per latent_and_weights call of make_tsne_reduction


def _latents_and_weights(full_model, existing, missing):
    """latent_and_weights over the rows of (existing, missing) in batches of at most ENCODE_CHUNK -> (latents, weights)."""
    parts = [full_model.latent_and_weights(existing[s:s + ENCODE_CHUNK], missing[s:s + ENCODE_CHUNK])
             for s in range(0, existing.size(0), ENCODE_CHUNK)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def make_tsne_reduction(full_model, device, dataset_dict, results_dir, epoch, train_dataset_dict=None, cat_name='car',
                        amount=100, perplexity=30.0, max_iter=1000, seed=0):
    """Do two different cuts of one shape land close together — in the latent space, and in the space of the decoder weights
    the hypernetwork generates?  Fills results_dir/temp_exp (created if missing, other files left alone).  `dataset_dict`
    and `train_dataset_dict`: category -> map-style dataset of (existing, missing, gt, idx) items.

    `amount` items of dataset_dict[cat_name] are drawn (np.random.choice without replacement on numpy's global generator)
    and every gt (n, 3) is cut twice, by the rank of its x and of its y coordinate (ops.axis_split with k = n // 2, axes 0
    and 1): the lower half is the missing part, the upper half the existing part.  Row 2i of the test rows is item i's x
    cut, row 2i + 1 its y cut.  With train_dataset_dict, the (existing, missing) parts of every item of its cat_name are the
    background rows, in dataset order, in front of the test rows.  All rows go through FullModel.latent_and_weights in
    batches of at most ENCODE_CHUNK — the reference runs forward() at batch 1 and has its user edit it to return these —
    and the latents and the weight vectors are each embedded by utils/tsne.py's exact t-SNE (init 'pca', `seed` unused by
    it) where the reference runs scikit-learn's Barnes-Hut on the CPU.  `epoch` is not read: nothing is decoded.

    Files: `<cat>_latent1.npy`, `<cat>_tnw1.npy` (the background rows; only with train_dataset_dict), `gts/<cat>_<i>.npy`,
    `<cat>_latent_tsne.npy`, `<cat>_tnw_tsne.npy` (all rows, (rows, 2)) and `<cat>_latent_dist.npy`, `<cat>_tnw_dist.npy`
    (amount): the embedded distance between each item's two cuts, which the reference computes and drops.  Its scatter
    plots of the embeddings are not drawn: utils/render.py draws clouds, not charts.  Fewer rows than the perplexity allows
    (rows <= perplexity) is a ValueError, as is a category with fewer than `amount` items.

    Returns (latent_tsne, tnw_tsne, latent_dist, tnw_dist) as device tensors."""
    ds = dataset_dict[cat_name]
    if len(ds) < amount:
        raise ValueError(f'with current dataset config the max amount value is {len(ds)}')
    background = train_dataset_dict[cat_name] if train_dataset_dict is not None else []
    total = len(background) + 2 * amount
    if not 0 < perplexity < total:
        raise ValueError(f'{total} rows cannot carry perplexity {perplexity}')
    ids = np.random.choice(len(ds), amount, replace=False)
    out_dir = os.path.join(results_dir, 'temp_exp')
    os.makedirs(os.path.join(out_dir, 'gts'), exist_ok=True)
    was_training = full_model.training
    full_model.eval()
    try:
        with torch.no_grad():
            gt = _gt_clouds(ds, ids, device)
            k = gt.size(1) // 2
            cuts = [ops.axis_split(gt, k, axis) for axis in (0, 1)]
            # (amount, 2, ., 3) -> rows 2i, 2i + 1
            missing = torch.stack([c[0] for c in cuts], 1).flatten(0, 1)
            existing = torch.stack([c[1] for c in cuts], 1).flatten(0, 1)
            latents, weights = _latents_and_weights(full_model, existing, missing)
            if len(background):
                part = lambda f: torch.stack([torch.as_tensor(np.asarray(background[i][f]), dtype=torch.float32)
                                              for i in range(len(background))]).to(device)
                bg_latents, bg_weights = _latents_and_weights(full_model, part(0), part(1))
                np.save(os.path.join(out_dir, f'{cat_name}_latent1'), bg_latents.cpu().numpy())
                np.save(os.path.join(out_dir, f'{cat_name}_tnw1'), bg_weights.cpu().numpy())
                latents, weights = torch.cat([bg_latents, latents]), torch.cat([bg_weights, weights])
            results = []
            for name, rows in (('latent', latents), ('tnw', weights)):
                embedding = tsne(rows.contiguous(), perplexity=perplexity, max_iter=max_iter, seed=seed).embedding
                test = embedding[-2 * amount:].view(amount, 2, 2)
                dist = (test[:, 0] - test[:, 1]).norm(dim=1)
                np.save(os.path.join(out_dir, f'{cat_name}_{name}_tsne'), embedding.cpu().numpy())
                np.save(os.path.join(out_dir, f'{cat_name}_{name}_dist'), dist.cpu().numpy())
                results.append((embedding, dist))
    finally:
        full_model.train(was_training)
    gt_host = gt.cpu().numpy()
    for i in range(amount):
        np.save(os.path.join(out_dir, 'gts', f'{cat_name}_{i}'), gt_host[i])
    return results[0][0], results[1][0], results[0][1], results[1][1]

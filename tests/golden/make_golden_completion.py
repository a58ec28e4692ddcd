#!/usr/bin/env python3
"""Golden fixtures for the completion metrics (UHD, TMD, MMD and their helpers), produced by running the REFERENCE's
own host code on CPU: utils/evaluation/completeness.py (process, directed_hausdorff, nn_distance, completeness),
utils/evaluation/total_mutual_diff.py (process), utils/evaluation/chamfer.py (compute_trimesh_chamfer,
scale_to_unit_sphere), utils/evaluation/mmd.py (process) and core/experiments.py (compute_mmd_tmd_uhd).

Stand-ins, below the reference's code only:
  * `ray`: remote(f) gives f a `.remote` that calls it, get() is the identity, init()/shutdown() do nothing — the
    reference's UHD process() then runs its tasks serially on the CPU;
  * `StructuralLossesBackend` (mmd.process's nn_distance): the CPU oracle, as in make_golden_metrics.py;
  * third-party modules core/experiments.py imports for its OTHER experiments and that this container lacks (h5py,
    trimesh, ...): empty modules — compute_mmd_tmd_uhd uses none of them.
Input: a synthetic `fixed/` directory (two categories, 15 inputs, so `chair_10_` sorts before `chair_2_`; k = 10;
existing (3,128), reconstructions (3,256)).  The arrays and file names are stored so the GPU test rebuilds it.
Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_completion.py
"""
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
from conftest import OracleLib  # noqa: E402

REF = os.environ.get("HP_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
OUT = os.path.dirname(os.path.abspath(__file__))
lib = OracleLib()

ray = types.ModuleType("ray")


def _remote(f):
    f.remote = f
    return f


ray.remote, ray.get = _remote, (lambda x: x)
ray.init = ray.shutdown = (lambda *a, **k: None)
sys.modules["ray"] = ray



def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


backend = types.ModuleType("utils.pytorch_structural_losses.StructuralLossesBackend")
backend.ApproxMatch = lambda a, b: [_t(x) for x in lib.approxmatch(a.numpy(), b.numpy())]
backend.MatchCost = lambda a, b, m: _t(lib.matchcost(a.numpy(), b.numpy(), m.numpy()))
backend.MatchCostGrad = lambda a, b, m: [_t(x) for x in lib.matchcostgrad(a.numpy(), b.numpy(), m.numpy())]
# b and n come from the first argument (structural_loss.cpp:86-93) — the oracle wrapper does the same
backend.NNDistance = lambda a, b: [_t(x) for x in lib.nndistance(a.numpy(), b.numpy()[:a.shape[0]])]
backend.NNDistanceGrad = lambda a, b, i1, i2, g1, g2: [_t(x) for x in lib.nndistancegrad(
    a.numpy(), b.numpy(), g1.numpy(), i1.numpy(), g2.numpy(), i2.numpy())]
sys.modules[backend.__name__] = backend


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything(self.__name__ + "." + name)

    def __call__(self, *a, **k):
        return self


_REF_PACKAGES = ("core", "utils", "datasets", "model", "losses")


def _import_with_stand_ins(module, tries=20):
    for _ in range(tries):
        try:
            return importlib.import_module(module)
        except ModuleNotFoundError as e:     # a third-party module this container lacks: an empty stand-in
            if e.name is None or e.name.split(".")[0] in _REF_PACKAGES:
                raise
            sys.modules[e.name] = _Anything(e.name)
            for k in [k for k in sys.modules if k.split(".")[0] in _REF_PACKAGES and k != backend.__name__]:
                del sys.modules[k]     # half-imported reference packages: import them afresh
    raise ImportError(module)


ref_experiments = _import_with_stand_ins("core.experiments")
import utils.evaluation.chamfer as ref_chamfer  # noqa: E402
import utils.evaluation.completeness as ref_completeness  # noqa: E402
import utils.evaluation.mmd as ref_mmd  # noqa: E402
import utils.evaluation.total_mutual_diff as ref_tmd  # noqa: E402

K, NE, N, BATCH = 10, 128, 256, 4
SHAPES = [("chair", 12), ("lamp", 3)]


def make_inputs(r):
    """{file name: (3, points) fp32}: a noisy partial sphere per input and k noisy completions of it."""
    files = {}
    for cat, count in SHAPES:
        for i in range(count):
            centre = r.uniform(-0.2, 0.2, 3)
            u = r.normal(size=(N, 3))
            sphere = u / np.linalg.norm(u, axis=1, keepdims=True) * r.uniform(0.3, 0.5) + centre
            part = sphere[sphere[:, 2] > np.median(sphere[:, 2])][:NE]
            part = np.concatenate([part, part[:NE - len(part)]], 0) if len(part) < NE else part
            files[f"{cat}_{i}_existing.npy"] = (part + r.normal(scale=0.01, size=part.shape)).T.astype(np.float32)
            for j in range(K):
                rec = sphere + r.normal(scale=0.02 + 0.01 * j, size=sphere.shape)
                files[f"{cat}_{i}_{j}_reconstruction.npy"] = rec.T.astype(np.float32)
    return files


def main():
    r = np.random.RandomState(2022)
    files = make_inputs(r)
    refs = (r.rand(6, N, 3).astype(np.float32) - 0.5) * 0.9
    dataset = [(None, None, refs[i], i) for i in range(len(refs))]
    out = {"names": np.array(sorted(files)), "ref_pcs": refs, "batch_size": np.int64(BATCH)}
    for i, name in enumerate(sorted(files)):
        out[f"file_{i}"] = files[name]
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "fixed"))
        os.makedirs(os.path.join(d, "compute_mmd_tmd_uhd"))
        for name, a in files.items():
            np.save(os.path.join(d, "fixed", name), a)
        shape_dir = os.path.join(d, "fixed")
        out["uhd_process"] = np.float64(ref_completeness.process(shape_dir))
        out["tmd_process"] = np.float64(ref_tmd.process(shape_dir))
        out["mmd_process"] = np.float64(ref_mmd.process(shape_dir, dataset, torch.device("cpu"), BATCH))
        ref_experiments.compute_mmd_tmd_uhd(None, torch.device("cpu"), dataset, d, 7, BATCH)
        with open(os.path.join(d, "compute_mmd_tmd_uhd", "7res.json")) as f:
            out["experiments_json"] = np.array(json.dumps(json.load(f)))
    # helpers on a few clouds of the same directory
    ex = np.stack([files[f"chair_{i}_existing.npy"] for i in range(4)])           # (4, 3, NE)
    gen = np.stack([files[f"chair_{i}_{i}_reconstruction.npy"] for i in range(4)])  # (4, 3, N)
    out["dh_pc1"], out["dh_pc2"] = ex, gen
    for red in (True, False):
        v = ref_completeness.directed_hausdorff(torch.from_numpy(ex), torch.from_numpy(gen), reduce_mean=red)
        out[f"directed_hausdorff_{int(red)}"] = v.numpy()
    q, c = ex[0].T.copy(), gen[1].T.copy()
    out["nn_query"], out["nn_ref"] = q, c
    out["nn_distance"] = ref_completeness.nn_distance(q, c)
    for t in (0.03, 0.1, 0.2):
        out[f"completeness_{t}"] = np.float64(ref_completeness.completeness(q, c, thres=t))
    out["chamfer_default"] = np.float64(ref_chamfer.compute_trimesh_chamfer(q, c))
    out["chamfer_offset_scale"] = np.float64(ref_chamfer.compute_trimesh_chamfer(q, c, offset=0.05, scale=1.5))
    out["unit_sphere"] = ref_chamfer.scale_to_unit_sphere(c)
    np.savez_compressed(os.path.join(OUT, "completion.npz"), **out)
    print({k: (v.shape if getattr(v, "ndim", 0) else v) for k, v in out.items() if not k.startswith("file_")})


if __name__ == "__main__":
    main()

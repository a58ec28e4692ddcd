#!/usr/bin/env python3
"""Golden fixture for the occupancy-grid JSD (utils/metrics.py:244-359 of the reference), produced by running the
REFERENCE's own host code on the CPU: unit_cube_grid_point_cloud, entropy_of_occupancy_grid, jensen_shannon_divergence
(through jsd_between_point_cloud_sets), with sklearn's NearestNeighbors underneath as the reference has it.

The reference's compiled module `StructuralLossesBackend` cannot be built here and the JSD never touches it: an empty
stand-in module satisfies the import.

Per (cloud set, R, in_sphere) the file holds `counters` and the entropy as entropy_of_occupancy_grid returns them, and
`clouds_hit` (the reference's grid_bernoulli_rvars, which it does not return): recomputed here with the reference's grid and
NearestNeighbors, cloud by cloud — the same recomputation also yields counters and is asserted equal to the reference's.
The one-point clouds (n = 1) are beyond the reference's function (it iterates a squeezed 0-d index array): their entries
come from the recomputation alone, the entropy from the reference's formula on it.

The generator asserts, for every point and grid, that the fp64 squared distances to the nearest and second-nearest kept
centre differ (no exact tie) and stores the smallest gap: tie-breaking is not under test.
Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_jsd.py
"""
import os
import sys
import types

import numpy as np
from scipy.stats import entropy
from sklearn.neighbors import NearestNeighbors

sys.dont_write_bytecode = True
REF = os.environ.get("HP_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
OUT = os.path.dirname(os.path.abspath(__file__))

backend = types.ModuleType("utils.pytorch_structural_losses.StructuralLossesBackend")
for _name in ("ApproxMatch", "MatchCost", "MatchCostGrad", "NNDistance", "NNDistanceGrad"):
    setattr(backend, _name, None)
sys.modules[backend.__name__] = backend

import utils.metrics as ref_metrics  # noqa: E402

RESOLUTIONS = (28, 8, 13)
DISTRIBUTIONS = ("ball45", "ball50", "cube50", "sphere50", "cube60")     # neighbouring pairs get a JSD


def _directions(r, shape):
    v = r.standard_normal(shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def cloud_sets():
    r = np.random.RandomState(2024)
    shape = (16, 384)
    ball = lambda radius: _directions(r, shape) * (radius * r.uniform(size=shape + (1,)) ** (1.0 / 3.0))
    sets = {
        "ball45": ball(0.45),                                   # uniform in the ball r = 0.45: no point needs the search
        "ball50": ball(0.5),
        "cube50": r.uniform(-0.5, 0.5, shape + (3,)),
        "sphere50": _directions(r, shape) * 0.5,                # on the sphere's surface
        "cube60": r.uniform(-0.6, 0.6, shape + (3,)),           # points outside cube and sphere are not dropped
        "one_point": r.uniform(-0.5, 0.5, (3, 1, 3)),
        "n1000": r.uniform(-0.55, 0.55, (3, 1000, 3)),
    }
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sets.items()}


def recompute(pclouds, grid):
    """counters, clouds_hit and the smallest fp64 gap between nearest and second-nearest squared distance."""
    nn = NearestNeighbors(n_neighbors=2).fit(grid)
    counters, hit, gap = np.zeros(len(grid), np.int64), np.zeros(len(grid), np.int64), np.inf
    g64 = grid.astype(np.float64)
    for pc in pclouds:
        _, idx = nn.kneighbors(pc)
        d2 = ((g64[idx] - pc.astype(np.float64)[:, None, :]) ** 2).sum(axis=2)
        assert np.all(d2[:, 1] > d2[:, 0]), "exact fp64 tie between the two nearest centres"
        gap = min(gap, float((d2[:, 1] - d2[:, 0]).min()))
        np.add.at(counters, idx[:, 0], 1)
        hit[np.unique(idx[:, 0])] += 1
    return counters, hit, gap


def main():
    sets = cloud_sets()
    out = {"set__" + k: v for k, v in sets.items()}
    min_gap = np.inf
    for R in RESOLUTIONS:
        for clip in (False, True):
            grid, spacing = ref_metrics.unit_cube_grid_point_cloud(R, clip)
            tag = f"R{R}_{'sphere' if clip else 'cube'}"
            out["grid__" + tag], out["spacing__" + tag] = grid, np.float64(spacing)
            flat = grid.reshape(-1, 3)
            for name, pcs in sets.items():
                counters, hit, gap = recompute(pcs, flat)
                min_gap = min(min_gap, gap)
                if pcs.shape[1] > 1:
                    ent, ref_counters = ref_metrics.entropy_of_occupancy_grid(pcs, R, clip)
                    assert np.array_equal(ref_counters, counters), (name, tag)
                else:
                    ent = sum(entropy([g / len(pcs), 1.0 - g / len(pcs)]) for g in hit if g > 0) / len(flat)
                assert counters.sum() == pcs.shape[0] * pcs.shape[1]
                out[f"counters__{name}__{tag}"] = counters.astype(np.int32)
                out[f"clouds_hit__{name}__{tag}"] = hit.astype(np.int32)
                out[f"entropy__{name}__{tag}"] = np.float64(ent)
    for a, b in zip(DISTRIBUTIONS[:-1], DISTRIBUTIONS[1:]):
        out[f"jsd__{a}__{b}"] = np.float64(ref_metrics.jsd_between_point_cloud_sets(sets[a], sets[b]))
    out["jsd__n1000__cube60__R13"] = np.float64(ref_metrics.jsd_between_point_cloud_sets(sets["n1000"], sets["cube60"], 13))
    out["min_gap"] = np.float64(min_gap)
    path = os.path.join(OUT, "jsd.npz")
    np.savez_compressed(path, **out)
    print("min fp64 gap", min_gap, "bytes", os.path.getsize(path))
    print({k: v for k, v in out.items() if k.startswith("jsd__")})


if __name__ == "__main__":
    main()

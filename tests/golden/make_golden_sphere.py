"""Writes tests/golden/sphere_meshes.npz: the points of the reference's utils/sphere_triangles.py generate(method, depth) as
float32 (3F,3) arrays, for `edge` at depths 0-3 and every other method at depths 1-3 — recorded output only, the check of
hyperpocket_amd/utils/sphere_mesh.py.

    python tests/golden/make_golden_sphere.py /path/to/reference
"""
import os
import sys

import numpy as np

CASES = [("edge", d) for d in range(4)] + [(m, d) for m in ("centroid", "midpoint", "midpoint2", "hybrid", "hybrid2", "hybrid3")
                                           for d in (1, 2, 3)]


def main(reference):
    sys.path.insert(0, reference)
    from utils import sphere_triangles
    out = {}
    for method, depth in CASES:
        points, _ = sphere_triangles.generate(method, depth)
        out[f"{method}_{depth}"] = points.numpy().astype(np.float32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sphere_meshes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", sum(v.shape[0] // 3 for v in out.values()), "triangles")


if __name__ == "__main__":
    main(sys.argv[1])

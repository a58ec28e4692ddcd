"""The mesh laws in numpy and Python integers — the checker of csrc/mesh.hip, written from the law itself
(include/hyperpocket_hip.h): fp64 arrays for the geometry, every operation a separate numpy operation and so one IEEE rounding;
Python ints for the weights' prefix sums and for mulhi64.  One mesh at a time: vertices (V,3) float32, faces (F,3) integers.
"""
import math

import numpy as np

from scan_law import words

TAG = 3                 # of the (stream, q, tag) Philox counter: 0 and 1 are scan preparation's, 0-2 the batch maker's


def corners(vertices, faces):
    x = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    return x[faces[:, 0]], x[faces[:, 1]], x[faces[:, 2]]


def cross_products(vertices, faces):
    """((F,3) fp64 cross products (b - a) x (c - a), a, e1, e2): products rounded, then the difference."""
    a, b, c = corners(vertices, faces)
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.stack([cx, cy, cz], 1), a, e1, e2


def lengths(c):
    with np.errstate(all="ignore"):
        return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


def weights(vertices, faces):
    """(w: a list of F Python ints, e) or (None, None) for a mesh without a face of finite non-zero area."""
    d = lengths(cross_products(vertices, faces)[0])
    d = np.where(np.isfinite(d), d, 0.0)
    d_max = float(d.max())
    if d_max == 0.0:
        return None, None
    e = math.frexp(d_max)[1]
    return [int(math.floor(math.ldexp(v, 40 - e))) for v in d.tolist()], e


def sample(vertices, faces, n, seed, stream):
    """(points (n,3) float32, face (n) int32, area float, failed int) of one mesh."""
    w, e = weights(vertices, faces)
    if w is None:
        return np.zeros((n, 3), np.float32), np.zeros(n, np.int32), 0.0, 1
    prefix, total = [], 0
    for v in w:
        total += v
        prefix.append(total)                           # inclusive, exact
    assert 2 ** 39 <= max(w) < 2 ** 40 and total < 2 ** 55
    area = math.ldexp(float(total), e - 41)            # float(int) rounds to nearest even: the one rounding of the law
    x = words(seed, stream, TAG, 4 * n).reshape(n, 4)
    r = [((int(a) << 32 | int(b)) * total) >> 64 for a, b in zip(x[:, 0].tolist(), x[:, 1].tolist())]
    # the smallest f with prefix[f] > r: prefix is non-decreasing, so this is a right-sided search
    face = np.searchsorted(np.array(prefix, dtype=np.uint64), np.array(r, dtype=np.uint64), side="right").astype(np.int64)
    assert all(prefix[f] > q and (f == 0 or prefix[f - 1] <= q) for f, q in zip(face.tolist(), r))
    u, v = x[:, 2].astype(np.float64) * 2.0 ** -32, x[:, 3].astype(np.float64) * 2.0 ** -32
    fold = u + v > 1.0
    u, v = np.where(fold, 1.0 - u, u), np.where(fold, 1.0 - v, v)
    _, a, e1, e2 = cross_products(vertices, faces)
    with np.errstate(all="ignore"):
        p = (a[face] + u[:, None] * e1[face]) + v[:, None] * e2[face]
        points = p.astype(np.float32)
    return points, face.astype(np.int32), area, 0


def fold_uv(seed, stream, n):
    """The (u, v) of samples 0..n-1 after the fold, fp64."""
    x = words(seed, stream, TAG, 4 * n).reshape(n, 4)
    u, v = x[:, 2].astype(np.float64) * 2.0 ** -32, x[:, 3].astype(np.float64) * 2.0 ** -32
    fold = u + v > 1.0
    return np.where(fold, 1.0 - u, u), np.where(fold, 1.0 - v, v)


def unit(s):
    """Rows of s (R,3) fp64 over their length, rounded to float32; rows of zero or non-finite length become +0."""
    length = lengths(s)
    ok = np.isfinite(length) & (length != 0.0)
    with np.errstate(all="ignore"):
        out = (s / length[:, None]).astype(np.float32)
    out[~ok] = 0.0
    return out


def normals(vertices, faces, vertex_faces):
    """(vertex_normal (V,3), face_normal (F,3)) float32 of one mesh; vertex_faces = (offsets, incident) CSR lists."""
    c = cross_products(vertices, faces)[0]
    offsets, incident = (np.asarray(a, dtype=np.int64) for a in vertex_faces)
    start, degree = offsets[:-1], np.diff(offsets)
    s = np.zeros((start.size, 3), np.float64)          # from +0
    with np.errstate(all="ignore"):
        for r in range(int(degree.max()) if degree.size else 0):
            has = degree > r                           # the r-th face of every list that has one: lists are ascending, so
            s[has] = s[has] + c[incident[start[has] + r]]      # each vertex adds its faces in that order, one rounding each
    return unit(s), unit(c)

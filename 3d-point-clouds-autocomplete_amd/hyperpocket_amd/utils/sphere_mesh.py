"""Triangulations of the unit sphere, as indexed meshes (host, numpy): the input of FullModel.sample_meshes.

The target network is a continuous map of the unit ball, so a closed triangulation of the sphere pushed through one cloud's
weights is a watertight mesh of that completion.  The seed is an octahedron; every level replaces each triangle by its
children, in place and in order, so the triangle order is the depth-first order of a recursive generator.  The rules, on a
triangle (p0, p1, p2) with mXY the normalised midpoint of pX pY and c the normalised centroid:

    edge        (p0, m01, m02) (m01, p1, m12) (m02, m12, p2) (m01, m02, m12)
    midpoint    (m12, p0, p1) (m12, p2, p0)
    midpoint2   (p0, m12, p1) (p0, p2, m12)           the second child is wound the other way; kept as the reference has it
    centroid    (p0, p1, c) (p2, c, p0) (c, p1, p2)

`hybrid` alternates edge, centroid, ..; `hybrid2` centroid, edge, ..; `hybrid3` cycles (midpoint twice), centroid, edge — each
item of a cycle uses one unit of depth.  All arithmetic is in doubles in the order (a + b) / 2, ((a + b) + c) / 3 and
u / (((x*x + y*y) + z*z) ** 0.5), and the result is rounded to float32 once.  New vertices are put back on the sphere but the
old ones stay, so `centroid`, `hybrid2` and `midpoint2` do not tend to area 4 pi; that is how the reference defines them.

Winding is the reference's too, and it is not consistent: the middle child of the edge rule, (m01, m02, m12), runs against its
parent, as does midpoint2's second child.  Sampling by area does not care; normals do.  `outward=True` swaps the last two
corners of every face whose normal points into the sphere, which makes the welded meshes consistently oriented.
"""
from collections import namedtuple

import numpy as np

METHODS = ("edge", "centroid", "midpoint", "midpoint2", "hybrid", "hybrid2", "hybrid3")

SphereMesh = namedtuple("SphereMesh", "vertices faces vertex_faces")


def _unit(p):
    """Rows of p (T,3) over their length; the power is Python's `** 0.5`, which is not sqrt in the last bit for every input."""
    s = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    s = np.array([v ** 0.5 for v in s.tolist()], dtype=np.float64)
    return p / s[:, None]


def _mid(a, b):
    return _unit((a + b) / 2)


def _children(tris, *corners):
    """tris (T,3,3) -> (T * len(corners), 3, 3): child k of every triangle has the three (T,3) arrays corners[k]."""
    kids = np.stack([np.stack(c, 1) for c in corners], 1)
    return kids.reshape(-1, 3, 3)


def _edge(t):
    p0, p1, p2 = t[:, 0], t[:, 1], t[:, 2]
    m01, m02, m12 = _mid(p0, p1), _mid(p0, p2), _mid(p1, p2)
    return _children(t, (p0, m01, m02), (m01, p1, m12), (m02, m12, p2), (m01, m02, m12))


def _midpoint(t):
    p0, p1, p2 = t[:, 0], t[:, 1], t[:, 2]
    m12 = _mid(p1, p2)
    return _children(t, (m12, p0, p1), (m12, p2, p0))


def _midpoint2(t):
    p0, p1, p2 = t[:, 0], t[:, 1], t[:, 2]
    m12 = _mid(p1, p2)
    return _children(t, (p0, m12, p1), (p0, p2, m12))


def _centroid(t):
    p0, p1, p2 = t[:, 0], t[:, 1], t[:, 2]
    c = _unit(((p0 + p1) + p2) / 3)
    return _children(t, (p0, p1, c), (p2, c, p0), (c, p1, p2))


def _twice(rule):
    return lambda t: rule(rule(t))


_CYCLES = {"edge": (_edge,), "centroid": (_centroid,), "midpoint": (_midpoint,), "midpoint2": (_midpoint2,),
           "hybrid": (_edge, _centroid), "hybrid2": (_centroid, _edge), "hybrid3": (_twice(_midpoint), _centroid, _edge)}


def _octahedron():
    p = 2 ** 0.5 / 2
    top, bottom = (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)
    ring = [(-p, 0.0, p), (p, 0.0, p), (p, 0.0, -p), (-p, 0.0, -p)]
    tris = [(top, ring[i], ring[(i + 1) % 4]) for i in range(4)] + [(bottom, ring[(i + 1) % 4], ring[i]) for i in range(4)]
    return np.array(tris, dtype=np.float64)


def triangle_soup(method, depth):
    """(F,3,3) float32: the triangles of `method` at `depth`, three private corners each."""
    if method not in _CYCLES:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    depth = int(depth)
    if depth < 0:
        raise ValueError(f"depth must be >= 0, got {depth}")
    tris, cycle = _octahedron(), _CYCLES[method]
    for level in range(depth):
        tris = cycle[level % len(cycle)](tris)
    return tris.astype(np.float32)


def vertex_faces(faces, n_vertices):
    """The faces around every vertex as CSR lists: (offsets (V+1) int32, incident (offsets[V]) int32), vertex v's faces being
    incident[offsets[v]:offsets[v+1]] in ascending order, each once even where a face names v twice."""
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be (F,3), got {faces.shape}")
    if faces.size and (faces.min() < 0 or faces.max() >= n_vertices):
        raise ValueError("a face names a vertex outside [0, V)")
    pairs = np.unique(faces.astype(np.int64).reshape(-1) * faces.shape[0] + np.repeat(np.arange(faces.shape[0]), 3))
    vertex, incident = pairs // max(faces.shape[0], 1), pairs % max(faces.shape[0], 1)
    offsets = np.zeros(n_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(vertex, minlength=n_vertices), out=offsets[1:])
    return offsets.astype(np.int32), incident.astype(np.int32)


def weld_corners(soup):
    """(F,3,3) float32 -> (vertices (V,3) float32, faces (F,3) int32): corners with equal float32 bit patterns become one
    vertex, numbered in order of first appearance, so vertices[faces] is the soup bit for bit."""
    corners = np.ascontiguousarray(soup, dtype=np.float32).reshape(-1, 3)
    _, first, inverse = np.unique(corners.view(np.dtype((np.void, 12))).reshape(-1), return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")            # unique value u is vertex rank[u]
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return corners[first[order]], rank[inverse.reshape(-1)].reshape(-1, 3).astype(np.int32)


def wind_outwards(vertices, faces):
    """`faces` with the last two corners swapped wherever (b - a) x (c - a) points against a + b + c, i.e. into the sphere."""
    a, b, c = (vertices[faces[:, i]].astype(np.float64) for i in range(3))
    inward = (np.cross(b - a, c - a) * (a + b + c)).sum(1) < 0
    out = faces.copy()
    out[inward] = faces[inward][:, [0, 2, 1]]
    return out


def sphere_mesh(method, depth, weld=True, outward=False):
    """SphereMesh(vertices (V,3) float32, faces (F,3) int32, vertex_faces): the sphere triangulated by `method` (one of
    METHODS) at `depth`.  weld=True merges corners by their float32 bits — a closed genus-0 mesh, V = F/2 + 2 — and
    weld=False keeps the three private corners of every triangle: vertices (3F,3), faces [[3i, 3i+1, 3i+2]].  Either way
    vertices[faces] is the same array — the reference generator's points, in its order — unless outward=True rewinds the
    faces that point inwards (wind_outwards; the vertices and their numbering stay).  vertex_faces is the CSR pair of the function of that name: the topology is the same
    for every mesh decoded from these vertices, so it is built here, once."""
    soup = triangle_soup(method, depth)
    if weld:
        vertices, faces = weld_corners(soup)
    else:
        vertices, faces = soup.reshape(-1, 3), np.arange(3 * soup.shape[0], dtype=np.int32).reshape(-1, 3)
    if outward:
        faces = wind_outwards(vertices, faces)
    return SphereMesh(vertices, faces, vertex_faces(faces, vertices.shape[0]))

"""CPU suite for the mesh layer: utils/sphere_mesh.py against the reference generator's recorded points
(tests/golden/sphere_meshes.npz), the welded meshes' topology, the sampling and normal laws (tests/mesh_law.py) on cases small
enough to work out by hand, and the argument checks of hp_mesh_sample / hp_mesh_normals (no GPU call is made)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_law
from conftest import PKG_DIR, golden
from scan_law import words

from hyperpocket_amd.utils.sphere_mesh import METHODS, sphere_mesh, vertex_faces

CASES = [("edge", d) for d in range(4)] + [(m, d) for m in METHODS if m != "edge" for d in (1, 2, 3)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def recorded():
    return golden("sphere_meshes")


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(f"{m}_{d}" for m, d in CASES)
    assert sum(v.shape[0] for v in recorded.values()) % 3 == 0


@pytest.mark.parametrize("method,depth", CASES)
def test_unwelded_is_the_references_points_by_bits(recorded, method, depth):
    want = recorded[f"{method}_{depth}"]
    mesh = sphere_mesh(method, depth, weld=False)
    assert mesh.vertices.dtype == np.float32 and mesh.faces.dtype == np.int32
    assert np.array_equal(_bits(mesh.vertices), _bits(want))
    F = want.shape[0] // 3
    assert np.array_equal(mesh.faces, np.arange(3 * F).reshape(F, 3))


@pytest.mark.parametrize("method,depth", CASES + [("edge", 4), ("edge", 5), ("hybrid", 4), ("centroid", 5)])
def test_welded_is_the_same_triangles_on_a_closed_genus_0_mesh(recorded, method, depth):
    mesh = sphere_mesh(method, depth)
    v, f = mesh.vertices, mesh.faces
    soup = sphere_mesh(method, depth, weld=False).vertices
    if f"{method}_{depth}" in recorded:
        soup = recorded[f"{method}_{depth}"]
    assert np.array_equal(_bits(v[f].reshape(-1, 3)), _bits(soup))            # same triangles, same order, same bits
    F, V = f.shape[0], v.shape[0]
    assert V == F // 2 + 2                                                    # Euler: V - 3F/2 + F = 2
    assert len({r.tobytes() for r in v}) == V                                 # welded: no two vertices share their bits
    first = np.full(V, -1)
    for pos, idx in enumerate(f.reshape(-1).tolist()):
        if first[idx] < 0:
            first[idx] = pos
    assert (np.diff(first) > 0).all() and first[0] == 0                       # numbered by first appearance
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all()                                                # every edge has exactly two faces
    assert not (v == 0).all(axis=1).any() and not np.signbit(v[v == 0]).any() # no signed-zero twins to weld
    offsets, incident = mesh.vertex_faces
    assert offsets.dtype == np.int32 and incident.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == 3 * F
    for vert in range(V):
        mine = incident[offsets[vert]:offsets[vert + 1]]
        assert (np.diff(mine) > 0).all()                                      # ascending, none twice
        assert np.array_equal(mine, np.nonzero((f == vert).any(axis=1))[0])   # complete


def test_the_sizes_the_design_quotes():
    sizes = {("edge", 0): (8, 6), ("edge", 2): (128, 66), ("edge", 4): (2048, 1026), ("edge", 5): (8192, 4098),
             ("centroid", 3): (216, 110), ("hybrid", 3): (384, 194)}
    for (method, depth), (F, V) in sizes.items():
        mesh = sphere_mesh(method, depth)
        assert (mesh.faces.shape[0], mesh.vertices.shape[0]) == (F, V)
    with pytest.raises(ValueError):
        sphere_mesh("loop", 2)
    with pytest.raises(ValueError):
        sphere_mesh("edge", -1)


def test_vertex_faces_of_a_face_list_with_repeats():
    faces = np.array([[0, 1, 2], [2, 2, 3], [3, 0, 0], [1, 1, 1]], np.int32)
    offsets, incident = vertex_faces(faces, 5)
    assert offsets.tolist() == [0, 2, 4, 6, 8, 8] and incident.tolist() == [0, 2, 0, 3, 0, 1, 1, 2]
    with pytest.raises(ValueError):
        vertex_faces(faces, 3)


# ------------------------------------------------------------------------------------------------
# the law, by hand
# ------------------------------------------------------------------------------------------------
def test_a_single_triangle():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32)
    points, face, area, failed = mesh_law.sample(v, [[0, 1, 2]], 500, 3, 9)
    assert failed == 0 and area == 1.0 and (face == 0).all()                  # |e1 x e2| / 2
    assert points.dtype == np.float32 and (points[:, 2] == 0).all()
    assert (points[:, 0] >= 0).all() and (points[:, 1] >= 0).all() and (points[:, 0] / 2 + points[:, 1] <= 1 + 1e-6).all()
    # the same stream gives the same points; another stream or seed does not
    again = mesh_law.sample(v, [[0, 1, 2]], 500, 3, 9)[0]
    assert np.array_equal(_bits(points), _bits(again))
    assert not np.array_equal(points, mesh_law.sample(v, [[0, 1, 2]], 500, 3, 10)[0])
    assert not np.array_equal(points, mesh_law.sample(v, [[0, 1, 2]], 500, 4, 9)[0])
    # sample j is a function of j alone: a longer run starts with the shorter one
    assert np.array_equal(_bits(points[:77]), _bits(mesh_law.sample(v, [[0, 1, 2]], 77, 3, 9)[0]))


def test_areas_one_to_three_are_the_integer_thresholds():
    """d = (1, 3): frexp(3) = (0.75, 2), so w = (2^38, 3 * 2^38), W = 2^40 and r = x >> 24: face 0 exactly when the first
    word of the block is below 2^30."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 3, 0]], np.float32)
    faces = [[0, 1, 2], [0, 1, 3]]
    w, e = mesh_law.weights(v, faces)
    assert e == 2 and w == [2 ** 38, 3 * 2 ** 38]
    n = 4000
    _, face, area, failed = mesh_law.sample(v, faces, n, 11, 5)
    word0 = words(11, 5, mesh_law.TAG, 4 * n).reshape(n, 4)[:, 0]
    assert np.array_equal(face == 0, word0 < 2 ** 30)
    assert area == 2.0 and failed == 0
    assert abs(int((face == 0).sum()) - n // 4) < 4 * (n * 3 / 16) ** 0.5      # and a quarter of them, to four sigma


def test_a_zero_area_face_is_never_picked():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 1]], np.float32)
    faces = [[0, 1, 3], [0, 1, 2], [1, 1, 4], [2, 2, 2], [0, 2, 4], [0, 3, 1]]   # 0, 2, 3, 5: collinear or repeated corners
    w, _ = mesh_law.weights(v, faces)
    assert [x == 0 for x in w] == [True, False, True, True, False, True]
    _, face, _, failed = mesh_law.sample(v, faces, 3000, 0, 0)
    assert failed == 0 and set(face.tolist()) == {1, 4}


def test_an_all_degenerate_mesh_fails():
    v = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)
    points, face, area, failed = mesh_law.sample(v, [[0, 1, 2], [1, 1, 2]], 10, 0, 0)
    assert failed == 1 and area == 0.0 and not points.any() and not face.any()
    assert mesh_law.sample(np.zeros((3, 3), np.float32), [[0, 1, 2]], 4, 0, 0)[3] == 1


def test_a_nan_vertex_zeroes_only_its_faces():
    mesh = sphere_mesh("edge", 2)
    v = mesh.vertices.copy()
    v[7] = np.nan
    v[20, 1] = np.inf
    w, _ = mesh_law.weights(v, mesh.faces)
    touched = (mesh.faces == 7).any(axis=1) | (mesh.faces == 20).any(axis=1)
    assert touched.sum() >= 8 and np.array_equal(np.array(w) == 0, touched)
    points, face, area, failed = mesh_law.sample(v, mesh.faces, 2000, 1, 2)
    assert failed == 0 and not touched[face].any() and np.isfinite(points).all() and 0 < area < 4 * np.pi


def test_uv_stay_in_the_triangle_after_the_fold():
    u, v = mesh_law.fold_uv(5, 6, 20000)
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1.0).all()
    raw = words(5, 6, mesh_law.TAG, 80000).reshape(-1, 4).astype(np.float64) * 2.0 ** -32
    folded = raw[:, 2] + raw[:, 3] > 1
    assert 0.4 < folded.mean() < 0.6 and np.array_equal(u[folded], 1 - raw[folded, 2])


@pytest.mark.parametrize("scale", [1.0, 2.0 ** 20, 2.0 ** -20])
def test_points_lie_in_their_faces_plane(scale):
    mesh = sphere_mesh("hybrid", 3)
    r = np.random.RandomState(3)
    v = ((mesh.vertices * (1 + 0.3 * r.rand(mesh.vertices.shape[0], 1))).astype(np.float32) * np.float32(scale)).astype(np.float32)
    points, face, area, failed = mesh_law.sample(v, mesh.faces, 3000, 8, 1)
    assert failed == 0
    c, a, e1, e2 = mesh_law.cross_products(v, mesh.faces)
    normal = c[face] / np.linalg.norm(c[face], axis=1, keepdims=True)
    off = np.abs(((points.astype(np.float64) - a[face]) * normal).sum(1))
    # the fp64 point is in the plane to fp64 rounding; rounding it to fp32 moves each coordinate by at most half an ulp
    bound = np.abs(points.astype(np.float64)).max(1) * 2.0 ** -24 * 3 ** 0.5 * 1.01
    assert (off <= bound).all()
    # scale-free: the faces drawn do not move under an exact power-of-two scaling
    base = mesh_law.sample((v / np.float32(scale)).astype(np.float32), mesh.faces, 3000, 8, 1)
    assert np.array_equal(face, base[1]) and area == base[2] * scale * scale
    assert np.array_equal(_bits(points), _bits(base[0] * np.float32(scale)))
    assert len(set(face.tolist())) > 300                                      # and it does draw all over the mesh


def test_area_of_the_edge_sphere_tends_to_4_pi():
    mesh = sphere_mesh("edge", 4)
    _, _, area, _ = mesh_law.sample(mesh.vertices, mesh.faces, 1, 0, 0)
    exact = 0.5 * mesh_law.lengths(mesh_law.cross_products(mesh.vertices, mesh.faces)[0]).sum()
    assert abs(area - exact) <= exact * 2.0 ** -38                            # 40-bit weights, truncated
    assert 0.99 * 4 * np.pi < area < 4 * np.pi


@pytest.mark.parametrize("method", METHODS)
def test_outward_rewinds_faces_and_nothing_else(method):
    plain, mesh = sphere_mesh(method, 3), sphere_mesh(method, 3, outward=True)
    assert np.array_equal(_bits(plain.vertices), _bits(mesh.vertices))
    assert np.array_equal(plain.faces[:, 0], mesh.faces[:, 0])
    swapped = (plain.faces != mesh.faces).any(axis=1)
    assert np.array_equal(mesh.faces[swapped], plain.faces[swapped][:, [0, 2, 1]])
    assert all(np.array_equal(a, b) for a, b in zip(plain.vertex_faces, mesh.vertex_faces))
    c = mesh_law.cross_products(mesh.vertices, mesh.faces)[0]
    assert ((c * mesh.vertices[mesh.faces].astype(np.float64).sum(1)).sum(1) > 0).all()
    # consistently oriented: every directed edge is used once, its reverse by the neighbour
    f = mesh.faces
    directed = {(a, b) for tri in f.tolist() for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0]))}
    assert len(directed) == 3 * f.shape[0] and all((b, a) in directed for a, b in directed)
    if method in ("edge", "midpoint2", "hybrid"):
        assert swapped.any()                                                  # the reference's winding is mixed there


def test_normals_of_a_sphere_point_outwards():
    mesh = sphere_mesh("edge", 3, outward=True)
    vn, fn = mesh_law.normals(mesh.vertices, mesh.faces, mesh.vertex_faces)
    assert vn.dtype == np.float32 and vn.shape == mesh.vertices.shape and fn.shape == (512, 3)
    assert np.allclose(np.linalg.norm(vn, axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(fn, axis=1), 1, atol=1e-6)
    assert ((vn * mesh.vertices).sum(1) > 0.99).all()                         # the octahedron's faces are wound outwards
    centre = mesh.vertices[mesh.faces].mean(1)
    assert ((fn * centre).sum(1) > 0.97).all()                                # |centre| is a little under 1
    flat = np.zeros((3, 3), np.float32)
    vn, fn = mesh_law.normals(flat, [[0, 1, 2]], vertex_faces(np.array([[0, 1, 2]]), 3))
    assert not vn.any() and not fn.any() and not np.signbit(vn).any()         # zero length: +0, not NaN


# ------------------------------------------------------------------------------------------------
# the library, without a GPU
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = ctypes.CDLL(mod.build(verbose=False))
    so.hp_mesh_sample_workspace_bytes.restype = ctypes.c_long
    return so


def test_entry_points_reject_bad_arguments_before_any_gpu_call(lib):
    p = ctypes.c_void_p(64)            # never dereferenced: every call below ends at its argument check
    null = ctypes.c_void_p(0)
    seed = ctypes.c_ulonglong(1)

    def draw(K=2, V=6, verts=p, F=8, faces=p, n=16, streams=p, points=p, face=p, area=p, failed=p, ws=null):
        return lib.hp_mesh_sample(K, V, verts, F, faces, n, seed, streams, points, face, area, failed, ws, null)

    for bad in (dict(K=-1), dict(K=65536), dict(V=0), dict(F=0), dict(F=32769), dict(n=0), dict(n=(1 << 24) + 1),
                dict(verts=null), dict(faces=null), dict(streams=null), dict(points=null), dict(face=null), dict(area=null),
                dict(failed=null), dict(F=8193, ws=null), dict(F=32768, ws=null)):
        assert draw(**bad) == -1, bad
    assert draw(K=0) == 0 and draw(K=0, F=32768, ws=p) == 0                   # nothing to do, nothing launched

    def normals(K=2, V=6, verts=p, F=8, faces=p, offsets=p, incident=p, face_normal=null, vertex_normal=p):
        return lib.hp_mesh_normals(K, V, verts, F, faces, offsets, incident, face_normal, vertex_normal, null)

    for bad in (dict(K=-1), dict(V=0), dict(F=0), dict(F=32769), dict(verts=null), dict(faces=null), dict(offsets=null),
                dict(incident=null), dict(vertex_normal=null)):
        assert normals(**bad) == -1, bad
    assert normals(K=0) == 0 and normals(K=0, face_normal=p) == 0


def test_plan_workspace_and_hooks(lib):
    threads, slices, in_lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    plan = lambda K, F, n: (lib.hp_mesh_sample_plan(K, F, n, ctypes.byref(threads), ctypes.byref(slices), ctypes.byref(in_lds)),
                            threads.value, slices.value, in_lds.value)
    try:
        assert lib.hp_mesh_sample_set_slices(0) >= 0 and lib.hp_mesh_sample_set_lds_faces(8192) >= 0
        assert plan(640, 8192, 2048) == (0, 1024, 2, 1) and lib.hp_mesh_sample_workspace_bytes(640, 8192, 2048) == 0
        assert plan(8, 32768, 2048) == (0, 1024, 8, 0) and lib.hp_mesh_sample_workspace_bytes(8, 32768, 2048) == 8 * 8 * 32768 * 8
        assert plan(1, 8, 1) == (0, 256, 1, 1) and plan(2, 8193, 5)[3] == 0
        assert plan(3, 128, 65)[2] == 1 and plan(1, 2048, 100000)[2] == 391   # never fewer than 256 samples a slice
        assert plan(0, 8, 0)[0] == -1 and lib.hp_mesh_sample_workspace_bytes(1, 0, 1) == -1
        assert lib.hp_mesh_sample_plan(1, 8, 1, None, ctypes.byref(slices), ctypes.byref(in_lds)) == -1
        assert lib.hp_mesh_sample_set_slices(7) == 0 and plan(3, 128, 65)[2] == 7 and plan(3, 128, 3)[2] == 3
        assert lib.hp_mesh_sample_set_slices(-1) == -1 and lib.hp_mesh_sample_set_slices(1025) == -1
        assert lib.hp_mesh_sample_set_slices(0) == 7                          # a refused value changed nothing
        assert lib.hp_mesh_sample_set_lds_faces(100) == 8192 and plan(3, 128, 65)[3] == 0 and plan(3, 100, 65)[3] == 1
        assert lib.hp_mesh_sample_workspace_bytes(3, 128, 65) == 3 * 1 * 128 * 8
        assert lib.hp_mesh_sample_set_lds_faces(8193) == -1 and lib.hp_mesh_sample_set_lds_faces(-1) == -1
        assert lib.hp_mesh_sample_set_lds_faces(8192) == 100
    finally:
        lib.hp_mesh_sample_set_slices(0)
        lib.hp_mesh_sample_set_lds_faces(8192)


def test_ops_refuse_what_they_cannot_do():
    from hyperpocket_amd import HipExtensionError, ops
    assert ops.MESH_MAX_FACES == 32768
    faces = torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(HipExtensionError):
        ops.mesh_sample(torch.rand(2, 6, 3), faces, 8)                        # CPU tensors: there is no CPU path
    with pytest.raises(HipExtensionError):
        ops.mesh_normals(torch.rand(2, 6, 3), faces, (torch.zeros(7, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)))

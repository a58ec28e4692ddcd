"""GPU suite for the mesh layer: hp_mesh_sample and hp_mesh_normals against the law (tests/mesh_law.py) bit for bit — points,
face, area, failed and both kinds of normals — at the smallest shapes that can go wrong and under every forced launch
geometry; then FullModel.sample_meshes against sample_completions, and fixed() with and without its triangulation."""
import copy
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import mesh_law
from conftest import fixture_state_, golden

from hyperpocket_amd.utils.sphere_mesh import sphere_mesh, vertex_faces

pytestmark = pytest.mark.gpu

CUDA = "cuda"
SEED = 0x1234_5678_9ABC_DEF1
SCALES = (1.0, 2.0 ** 20, 2.0 ** -20)

#          name: (faces from, K, n, streams)
CASES = {"a": (("edge", 0), 1, 1, (5,)),                        # fewer faces than a wave
         "b": (("edge", 2), 3, 65, (7, 2 ** 40 + 3, 0)),        # more than a wave, less than a workgroup; odd n; distinct streams
         "c": (("edge", 4), 2, 2048, (0, 1)),                   # several faces per lane
         "d0": (("edge", 5), 2, 300, (3, 4)),                   # 8192 faces: the last size whose table is in LDS
         "d1": (("random", 8193, 4098), 2, 300, (3, 4)),        # 8193: the first in the workspace
         "e": (("edge", 6), 2, 257, (11, 12)),                  # 32768 faces: the largest
         "f": (("random", 1000, 300), 3, 500, (0, 1, 2))}       # non-manifold, repeated corners, a zero mesh, a NaN vertex


def _bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@functools.lru_cache(maxsize=None)
def topology(spec):
    """(faces (F,3) int32, V, vertex_faces) of a case."""
    if spec[0] == "random":
        _, F, V = spec
        r = np.random.RandomState(F)
        faces = r.randint(0, V, size=(F, 3)).astype(np.int32)
        faces[::7, 1] = faces[::7, 0]                           # repeated corners: faces of no area
        faces[5] = faces[4]                                     # a face twice
        return faces, V, vertex_faces(faces, V)
    mesh = sphere_mesh(*spec)
    return mesh.faces, mesh.vertices.shape[0], mesh.vertex_faces


@functools.lru_cache(maxsize=None)
def vertices_of(name, scale):
    """(K,V,3) float32, decoded-looking: randn * 0.3, times an exact power of two."""
    spec, K, n, _ = CASES[name]
    _, V, _ = topology(spec)
    v = (np.random.RandomState(ord(name[0]) + len(name)).standard_normal((K, V, 3)) * 0.3).astype(np.float32)
    if name == "f":
        v[1] = 0.0                                              # a mesh with nothing to draw from, between two valid ones
        v[2, 17] = np.nan                                       # removes its own faces only
        v[2, 40, 2] = np.inf
    out = (v * np.float32(scale)).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def law(name, scale):
    """The law's (points, face, area, failed) of a case, stacked over its meshes: computed once, shared, left unchanged."""
    spec, K, n, streams = CASES[name]
    faces, _, _ = topology(spec)
    per_mesh = [mesh_law.sample(vertices_of(name, scale)[k], faces, n, SEED, streams[k]) for k in range(K)]
    return tuple(np.stack([np.asarray(m[i]) for m in per_mesh]) for i in range(4))


def _device(name, scale):
    spec, K, n, streams = CASES[name]
    faces, V, vf = topology(spec)
    return (torch.from_numpy(vertices_of(name, scale).copy()).to(CUDA), torch.from_numpy(faces).to(CUDA),
            tuple(torch.from_numpy(a).to(CUDA) for a in vf), n, torch.tensor(streams, dtype=torch.int64, device=CUDA))


def _check_sample(name, scale, got):
    want = law(name, scale)
    points, face, area, failed = got
    assert np.array_equal(failed.cpu().numpy(), want[3]), (name, scale)
    assert np.array_equal(face.cpu().numpy(), want[1]), (name, scale)
    assert np.array_equal(_bits(area), _bits(want[2].astype(np.float64))), (name, scale)
    assert np.array_equal(_bits(points), _bits(want[0])), (name, scale)


class Geometry:
    """`with Geometry(slices, lds_faces):` forces the launch geometry of hp_mesh_sample inside the block."""

    def __init__(self, slices, lds_faces):
        self.want = (slices, lds_faces)

    def __enter__(self):
        from hyperpocket_amd import ops
        lib = ops.load_library()
        self.prev = (lib.hp_mesh_sample_set_slices(self.want[0]), lib.hp_mesh_sample_set_lds_faces(self.want[1]))
        assert min(self.prev) >= 0
        return self

    def __exit__(self, *exc):
        from hyperpocket_amd import ops
        lib = ops.load_library()
        lib.hp_mesh_sample_set_slices(self.prev[0])
        lib.hp_mesh_sample_set_lds_faces(self.prev[1])


def _plan(K, F, n):
    from hyperpocket_amd import ops
    t, s, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert ops.load_library().hp_mesh_sample_plan(K, F, n, ctypes.byref(t), ctypes.byref(s), ctypes.byref(l)) == 0
    return t.value, s.value, l.value


@pytest.mark.parametrize("name", list(CASES))
def test_sample_is_the_law_and_scale_free(name):
    from hyperpocket_amd import ops
    spec, K, n, _ = CASES[name]
    F = topology(spec)[0].shape[0]
    assert _plan(K, F, n)[2] == (1 if F <= 8192 else 0)                       # the default: LDS up to 8192 faces
    base_face = None
    for scale in SCALES:
        verts, faces, _, n, streams = _device(name, scale)
        got = ops.mesh_sample(verts, faces, n, SEED, streams)
        _check_sample(name, scale, got)
        if base_face is None:
            base_face = got[1].clone()
        assert torch.equal(got[1], base_face), scale                          # the faces drawn do not move with the scale
    want = law(name, 1.0)
    if name == "f":
        assert want[3].tolist() == [0, 1, 0] and want[2][1] == 0 and not want[0][1].any()
        touched = (topology(spec)[0] == 17).any(axis=1) | (topology(spec)[0] == 40).any(axis=1)
        assert touched.sum() > 10 and not touched[want[1][2]].any() and np.isfinite(want[0]).all()
    else:
        assert not want[3].any() and len({tuple(r) for r in want[1].tolist()}) == K   # distinct streams, distinct draws


GEOMETRIES = [(1, 8192), (3, 8192), (64, 8192), (0, 0), (5, 0), (1, 128)]


@pytest.mark.parametrize("slices,lds_faces", GEOMETRIES)
@pytest.mark.parametrize("name", ["b", "c", "d0", "d1", "e"])
def test_every_forced_geometry_gives_the_same_bits(name, slices, lds_faces):
    from hyperpocket_amd import ops
    verts, faces, _, n, streams = _device(name, 1.0)
    K, F = verts.size(0), faces.size(0)
    with Geometry(slices, lds_faces):
        threads, got_slices, in_lds = _plan(K, F, n)
        assert in_lds == (1 if F <= lds_faces else 0)
        if slices:
            assert got_slices == -(-n // -(-n // min(slices, n)))              # `slices` of them, fewer where they would be empty
        out = ops.mesh_sample_buffers(K, F, n, CUDA)
        assert (out["ws"] is None) == bool(in_lds)
        for t in (out["points"], out["face"], out["failed"]):
            t.fill_(-1)                                                       # every output is written in full
        out["area"].fill_(-1.0)
        got = ops.mesh_sample(verts, faces, n, SEED, streams, out=out)
        assert got[0] is out["points"]
        _check_sample(name, 1.0, got)


def test_two_calls_agree_and_streams_default_to_the_mesh_number():
    from hyperpocket_amd import ops
    verts, faces, _, n, _ = _device("b", 1.0)
    one = ops.mesh_sample(verts, faces, n, 9)
    two = ops.mesh_sample(verts, faces, n, 9, torch.arange(3, dtype=torch.int64, device=CUDA))
    for a, b in zip(one, two):
        assert np.array_equal(_bits(a), _bits(b))
    want = mesh_law.sample(vertices_of("b", 1.0)[2], topology(CASES["b"][0])[0], n, 9, 2)
    assert np.array_equal(_bits(one[0][2]), _bits(want[0])) and np.array_equal(one[1][2].cpu().numpy(), want[1])
    other = ops.mesh_sample(verts, faces, n, 10)
    assert not torch.equal(one[1], other[1])
    # a mesh's result does not depend on its neighbours or its place in the batch
    alone = ops.mesh_sample(verts[1:2].contiguous(), faces, n, 9, torch.tensor([1], dtype=torch.int64, device=CUDA))
    assert np.array_equal(_bits(alone[0][0]), _bits(one[0][1])) and np.array_equal(_bits(alone[2]), _bits(one[2][1:2]))


def test_ops_check_a_face_list_once_and_refuse_a_bad_one():
    from hyperpocket_amd import HipExtensionError, ops
    verts, faces, vf, n, streams = _device("b", 1.0)
    ops.mesh_sample(verts, faces, n)
    assert faces._hp_mesh_checked == (faces._version, int(faces.max()) + 1)
    with pytest.raises(HipExtensionError):
        ops.mesh_sample(verts[:, :60].contiguous(), faces, n)                 # the same list over too few vertices
    bad = faces.clone()
    bad[3, 1] = 66
    with pytest.raises(HipExtensionError):
        ops.mesh_sample(verts, bad, n)
    faces[3, 1] = -1                                                          # modified in place: seen again
    with pytest.raises(HipExtensionError):
        ops.mesh_normals(verts, faces, vf)
    with pytest.raises(HipExtensionError):
        ops.mesh_sample(verts, bad.long(), n)
    with pytest.raises(HipExtensionError):
        ops.mesh_sample(verts, _device("b", 1.0)[1], n, streams=streams[:2])
    good = _device("b", 1.0)[1]
    with pytest.raises(HipExtensionError):
        ops.mesh_normals(verts, good, (vf[0], vf[1] + 1000))


@pytest.mark.parametrize("name", list(CASES))
def test_normals_are_the_law(name):
    from hyperpocket_amd import ops
    spec, K, _, _ = CASES[name]
    host_faces, V, host_vf = topology(spec)
    for scale in SCALES[:2] if name != "f" else SCALES:
        verts, faces, vf, _, _ = _device(name, scale)
        vn, fn = ops.mesh_normals(verts, faces, vf, face_normals=True)
        only_vn = ops.mesh_normals(verts, faces, vf)
        assert vn.shape == (K, V, 3) and fn.shape == (K, host_faces.shape[0], 3)
        for k in range(K):
            want_vn, want_fn = mesh_law.normals(vertices_of(name, scale)[k], host_faces, host_vf)
            assert np.array_equal(_bits(vn[k]), _bits(want_vn)), (name, scale, k)
            assert np.array_equal(_bits(fn[k]), _bits(want_fn)), (name, scale, k)
        assert np.array_equal(_bits(only_vn), _bits(vn))
    if name == "f":
        assert not vn[1].any() and not fn[1].any() and torch.isfinite(vn).all() and torch.isfinite(fn).all()


# ------------------------------------------------------------------------------------------------
# the model and the experiment
# ------------------------------------------------------------------------------------------------
CFG = {"random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
       "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
       "hyper_network": {"use_bias": True, "relu_slope": 0.2},
       "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                          "layer_out_channels": [32, 64, 128, 64]},
       "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}


def _model(fixture):
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    g = golden(fixture)
    torch.manual_seed(int(g["seed"]))
    model = FullModel(copy.deepcopy(CFG))
    model.apply(weights_init)
    model = model.cuda()
    fixture_state_(model.state_dict(), g)
    return model.eval(), g


def test_sample_meshes_is_sample_completions_on_the_spheres_vertices():
    model, g = _model("model_small")
    mesh = sphere_mesh("hybrid", 3)
    V = mesh.vertices.shape[0]
    existing = torch.from_numpy(g["existing"]).cuda()
    K = existing.size(0)
    noise = (torch.randn(K, model.get_noise_size(), generator=torch.Generator().manual_seed(3)) * 0.2).cuda()
    sphere = torch.from_numpy(mesh.vertices).cuda()
    calls, state, kept = model._sampler_calls, torch.get_rng_state(), existing.clone()
    with torch.no_grad():
        got = model.sample_meshes(existing, noise, sphere, 1)
        want = model.sample_completions(existing, noise, V, 1, points=sphere.unsqueeze(0).expand(K, V, 3).contiguous())
        code = model.encode_existing(existing)
        again = model.sample_meshes(None, noise, sphere, 1, code=code)
    assert got.shape == (K, V, 3) and got.is_contiguous() and want.shape == (K, 3, V)
    assert np.array_equal(_bits(got), _bits(want.permute(0, 2, 1).contiguous()))
    assert np.array_equal(_bits(again), _bits(got))
    assert model._sampler_calls == calls and torch.equal(torch.get_rng_state(), state)    # nothing drawn
    assert torch.equal(existing, kept)
    assert not torch.equal(got[0], got[1]) and torch.isfinite(got).all()
    with pytest.raises(ValueError):
        model.sample_meshes(existing, noise, sphere.t(), 1)
    model.train()
    with pytest.raises(RuntimeError):
        model.sample_meshes(existing, noise, sphere, 1)


def _scan(n, seed, centre=(0.0, 0.0, 0.0)):
    r = np.random.RandomState(seed)
    return (r.standard_normal((n, 3)) * 0.1 + np.asarray(centre)).astype(np.float32)


def _categories():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    sets = {"blob": [_scan(n, 20 + n) for n in (50, 64, 300)], "shifted": [_scan(n, 40 + n, (0.1, -0.05, 0.0)) for n in (90, 33)]}
    return {cat: ScanBatcher(DeviceScanDataset(scans, device=CUDA), 2, target=64, seed=5) for cat, scans in sets.items()}


NOISES = 10              # shape_dir.py groups reconstructions by tens
TRI = {"execute": True, "method": "hybrid", "depth": 2, "seed": 21}


def _parse_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        tag, *rest = line.split()
        if tag == "v":
            v.append([np.float32(x) for x in rest])
        elif tag == "vn":
            vn.append([np.float32(x) for x in rest])
        else:
            assert tag == "f"
            corners = [c.split("//") for c in rest]
            assert all(a == b for a, b in corners)
            f.append([int(a) - 1 for a, _ in corners])
    return np.array(v, np.float32), np.array(vn, np.float32), np.array(f, np.int32)


def test_fixed_with_its_triangulation(tmp_path):
    from hyperpocket_amd.core.experiments import fixed, mesh_completions
    from hyperpocket_amd.utils.evaluation.shape_dir import grouped_paths
    model, g = _model("model_trained")
    epoch, dev = int(g["epoch"]), torch.device(CUDA)
    runs = {}
    for name, tri in (("plain", None), ("off", dict(TRI, execute=False)), ("mesh", TRI)):
        torch.manual_seed(31)
        model._sampler_seed, model._sampler_calls = None, 0
        out = fixed(model, dev, _categories(), str(tmp_path / name), epoch, std=0.2, noises_per_item=NOISES, batch_size=2,
                    triangulation_config=tri)
        runs[name] = (out, torch.get_rng_state(), sorted(os.listdir(tmp_path / name / "fixed")))
    plain, off, mesh_run = runs["plain"], runs["off"], runs["mesh"]
    assert off[2] == plain[2] and len(plain[2]) == 5 * (NOISES + 1)
    extra = sorted(f"{cat}_{i}_{j}_{kind}" for cat, items in (("blob", 3), ("shifted", 2)) for i in range(items)
                   for j in range(NOISES) for kind in ("mesh.obj", "surface.npy"))
    assert sorted(set(mesh_run[2]) - set(plain[2])) == extra and set(plain[2]) <= set(mesh_run[2])
    for other in ("off", "mesh"):                                             # the common files, the generator, the return value
        for f in plain[2]:
            assert (tmp_path / "plain" / "fixed" / f).read_bytes() == (tmp_path / other / "fixed" / f).read_bytes(), (other, f)
        assert torch.equal(runs[other][1], plain[1])
        assert all(torch.equal(a, b) for a, b in zip(runs[other][0][0], plain[0][0])) and torch.equal(runs[other][0][1], plain[0][1])
    groups, ex = grouped_paths(str(tmp_path / "mesh" / "fixed"), True)        # the new names stay out of the metrics' globs
    assert len(ex) == 5 and all(len(grp) == NOISES for grp in groups)

    sphere = sphere_mesh(TRI["method"], TRI["depth"], outward=True)
    d = tmp_path / "mesh" / "fixed"
    torch.manual_seed(31)
    item = 0
    for cat, batcher in _categories().items():
        for i, batch in enumerate(batcher):
            existing = batch[0]
            B = existing.size(0)
            noises = [torch.empty(B, model.get_noise_size()).normal_(mean=0.0, std=0.2) for _ in range(NOISES)]
            for j, noise in enumerate(noises):
                streams = (torch.arange(item, item + B, device=CUDA) * NOISES + j).long()
                res = mesh_completions(model, existing, noise.cuda(), sphere, epoch, 2048, TRI["seed"], streams=streams)
                assert not res["failed"].any() and (res["area"] > 0).all()
                for k in range(B):
                    stem = f"{cat}_{i * 2 + k}_{j}"
                    v, vn, f = _parse_obj(d / f"{stem}_mesh.obj")
                    assert np.array_equal(f, sphere.faces)
                    assert np.array_equal(_bits(v), _bits(res["vertices"][k]))             # text and back: the same bits
                    assert np.array_equal(_bits(vn), _bits(res["vertex_normals"][k]))
                    assert np.array_equal(_bits(vn), _bits(mesh_law.normals(v, f, sphere.vertex_faces)[0]))
                    surface = np.load(d / f"{stem}_surface.npy")
                    assert surface.shape == (3, 2048) and surface.dtype == np.float32
                    want = mesh_law.sample(v, f, 2048, TRI["seed"], (item + k) * NOISES + j)
                    assert want[3] == 0 and np.array_equal(_bits(surface.T), _bits(want[0]))
                    assert np.array_equal(res["surface_face"][k].cpu().numpy(), want[1])
            item += B
    assert item == 5

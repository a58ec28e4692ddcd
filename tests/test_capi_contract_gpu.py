"""GPU suite: every call the package makes into libhyperpocket_hip.so, held to include/hyperpocket_hip.h as the compiler
reads it (tests/capi_law.py).  The package sets no argtypes, so each call site chooses the ctypes object of every argument and
the restype of the function object; capi_law.checked_library() puts a proxy in front of a freshly loaded library that checks
the argument count, every argument's class and the restype of each call, records it and forwards the very objects.

These are no numeric tests — the laws own the numerics.  Each family is driven once at the smallest shape its route accepts;
the last tests close the set: every hp_* name in the package's Python source was observed (here, or in the host record of
tests/golden/ops_wrapper_calls.json), or is exempt because every call site of it belongs to the multi-rank exchange and is
checked statically.  The module's tests build on one another's record: run the module whole."""
import ast
import contextlib
import ctypes
import glob
import os
import types

import numpy as np
import pytest
import torch

import capi_law
from conftest import PKG_DIR, golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
PACKAGE = os.path.join(PKG_DIR, "hyperpocket_amd")
# Call sites that run only inside the multi-rank exchange (a process group): (file, enclosing function or Class.method).  Everything
# in parallel.py counts as well.  An entry point is exempt from the GPU record only if ALL of its call sites are of these.
MULTI_RANK_SITES = {("core/engine.py", "HeadsShard.begin")}
EXEMPT = {"hp_hypernet_heads_dw_workspace_floats": ["core/engine.py:65", "core/engine.py:67"]}


@pytest.fixture(scope="module")
def book():
    return types.SimpleNamespace(log=capi_law.CallLog(), families={}, gpu_error=None)


@contextlib.contextmanager
def checked(book, family):
    """The family's calls under the proxy; afterwards the violations it added, all of them, fail the test."""
    if book.gpu_error:                                         # after a GPU error nothing more is started on the device
        pytest.fail(f"not run: an earlier family ended in a GPU error ({book.gpu_error})")
    first_call, first_bad = len(book.log.calls), len(book.log.violations)
    try:
        # the drivers draw from torch's generators (the engine's own eps and points): later modules find them as they were
        with torch.random.fork_rng(devices=[torch.cuda.current_device()]), capi_law.checked_library(book.log):
            yield
            torch.cuda.synchronize()
    except Exception as e:
        if any(word in str(e) for word in ("HIP error", "hipError", "illegal memory access", "HIP kernel failed")):
            book.gpu_error = f"{family}: {str(e)[:200]}"
        raise
    finally:
        names = sorted({n for n, _ in book.log.calls[first_call:]})
        book.families[family] = names
        print(f"{family}: {len(book.log.calls) - first_call} calls of {len(names)} entry points")
        for v in book.log.violations[first_bad:]:
            print("VIOLATION", v)
    assert book.log.violations[first_bad:] == []
    assert names, family


def rand(*shape, seed=0, scale=1.0, shift=-0.5):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g) + shift) * scale).cuda()


def small_batch(seed, B=2, n_ex=128, n_mi=128, N=64, out=128):
    g = torch.Generator().manual_seed(seed)
    ex, mi = torch.rand(B, n_ex, 3, generator=g) - 0.5, torch.rand(B, n_mi, 3, generator=g) - 0.5
    return types.SimpleNamespace(ex=ex.cuda(), mi=mi.cuda(), gt=torch.cat([ex, mi], 1).cuda(),
                                 pts=(torch.rand(B, N, 3, generator=g) * 2 - 1).cuda(), eps=torch.randn(B, out, generator=g).cuda())


def model_loss(model, b):
    from hyperpocket_amd import ops
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    rec, explv, mu = model(b.ex.clone(), b.mi.clone(), list(b.gt.shape), 1, torch.device("cuda"), points=b.pts, eps=b.eps)
    return 0.05 * ChamferLoss()(b.gt, rec.permute(0, 2, 1)) + ops.kld_loss(explv, mu)


# ============================================================================================ the autograd nodes, the losses
def drive_nodes_and_losses():
    from hyperpocket_amd import ops
    from hyperpocket_amd.utils.pytorch_structural_losses import StructuralLossesBackend as backend
    from hyperpocket_amd.utils.pytorch_structural_losses.match_cost import match_cost
    from hyperpocket_amd.utils.pytorch_structural_losses.nn_distance import nn_distance
    from test_model_gpu import build_model
    model = build_model(5).train()
    try:
        model_loss(model, small_batch(1)).backward()                       # the pair node, the fused decoder, the plain heads
        model_loss(model, small_batch(2, n_ex=100)).backward()             # two encoder nodes on two streams
        fused, ops.FUSED_TARGET_NETWORK = ops.FUSED_TARGET_NETWORK, False
        try:
            model_loss(model, small_batch(3)).backward()                   # the layered decoder
        finally:
            ops.FUSED_TARGET_NETWORK = fused
        model.eval()
        with torch.no_grad():
            b = small_batch(4)
            model(b.ex.clone(), b.mi.clone(), list(b.gt.shape), 1, torch.device("cuda"), points=b.pts)
        model.train()
    finally:
        ops.clear_grad_views()
    a, c = rand(2, 100, 3, seed=5).requires_grad_(True), rand(2, 37, 3, seed=6).requires_grad_(True)
    d1, d2 = nn_distance(a, c)
    (d1.sum() + d2.sum()).backward()
    match_cost(a, c).sum().backward()
    with torch.no_grad():
        match_cost(a, c)
        match, _ = backend.ApproxMatch(a, c)
        backend.MatchCost(a, c, match)
        backend.MatchCostGrad(a, c, match)
        dist1, idx1, dist2, idx2 = backend.NNDistance(a, c)
        backend.NNDistanceGrad(a, c, idx1, idx2, torch.ones_like(dist1), torch.ones_like(dist2))


@pytest.mark.parametrize("arithmetic", ["pieces", "strict_fp32"])
def test_autograd_nodes_and_loss_functions(book, arithmetic):
    from hyperpocket_amd import ops
    with checked(book, f"nodes and losses, {arithmetic}"):
        if arithmetic == "strict_fp32":
            with ops.strict_fp32():
                drive_nodes_and_losses()
        else:
            drive_nodes_and_losses()


# ======================================================================================================== the optimizers
def test_optimizers(book):
    from hyperpocket_amd import ops
    from hyperpocket_amd.optim import FlatAdam
    from test_model_gpu import build_model
    with checked(book, "optimizers"):
        p, g, m, v = (rand(1000, seed=s) for s in range(4))
        ops.adam_step(p, g, m, v.abs(), 1e-3, 0.9, 0.999, 1e-8, 1, grad_scale=0.5)
        for fuse in (True, False):
            model = build_model(6).train()
            try:
                opt = FlatAdam(model, lr=1e-4, fuse_heads=fuse)
                opt.zero_grad()
                model_loss(model, small_batch(7)).backward()
                opt.step()
                torch.cuda.synchronize()
            finally:
                ops.clear_grad_views()


# ============================================================================================================ the engine
@pytest.mark.parametrize("term", ["chamfer", "emd"])
def test_one_engine_step(book, term):
    from hyperpocket_amd import ops
    from hyperpocket_amd.core.engine import TrainEngine
    from test_model_gpu import build_model
    with checked(book, f"engine step, {term}"):
        model = build_model(8).train()
        b = small_batch(9, N=256)                                          # the engine's Chamfer term wants as many points as gt has
        eng = TrainEngine(model, emd_coef=0.05 if term == "emd" else 0.0)
        try:
            eng.step(b.ex.clone(), b.mi.clone(), b.gt.clone(), 50, points=b.pts, eps_noise=b.eps)
            eng.step(b.ex.clone(), b.mi.clone(), b.gt.clone(), 50)                                 # the engine's own draws, pre-drawn beside the step
            eng.finish_pending()
            eng.synchronize()
            # the rows update of the sharded heads (HeadsShard hands it the gathered factors): here on the first 64 rows
            h = eng.flat.heads
            eng._adam_heads_rows(rand(2, h["rows"], seed=1), rand(2, 2048, seed=2), 0, 64, h["lo"], h["lo"] + 64 * h["cols"])
        finally:
            eng.close()
            ops.clear_grad_views()


# ============================================================================================================== the GEMMs
def test_gemm_and_colsum_wrappers(book):
    from hyperpocket_amd import ops
    with checked(book, "gemm and colsum"):
        A, B, bias = rand(130, 70, seed=1), rand(50, 70, seed=2), rand(50, seed=3)
        mask, add = rand(130, 50, seed=4), rand(130, 50, seed=5)
        ops.gemm(A, B)
        ops.gemm(A, B, bias=bias, relu=True, mask=mask, add=add, ksplit=2, rowsum=True)
        ops.gemm(rand(2, 130, 70, seed=6), rand(2, 70, 50, seed=7), trans_b=False, out=torch.empty(2, 130, 50, device=DEV))
        ops.gemm(rand(70, 130, seed=8), B, trans_a=True, dyn_rows=torch.tensor([100], dtype=torch.int32, device=DEV))
        ops.gemm(A, B, dyn_k=torch.tensor([60], dtype=torch.int32, device=DEV))
        ops.gemm(rand(128, 8, seed=9), rand(70, 8, seed=10), colmax=64)
        ops.gemm_plan(A.cpu(), B.cpu(), bias=bias.cpu(), ksplit=2)
        X = rand(2, 130, 50, seed=10)
        ops.colsum(X)
        ops.colsum(X, mask=rand(2, 130, 50, seed=11), use_ws=False)
        W = rand(128, 64, seed=12)
        ops.GemmF16x2(rand(300, 64, seed=13), W, rand(128, seed=14), relu=True).run()
        pp = ops.GemmPP(rand(300, 64, seed=15), W, rand(128, seed=16), relu=True, xcb=64)
        pp.run(0)
        pp.result()
        pp.run(1)
        pp.partials()


# ================================================================================= the samplers, the slicer, the batch makers
def test_samplers_slicer_and_batch_makers(book):
    from hyperpocket_amd import ops
    with checked(book, "samplers, slicer, batch makers"):
        ops.sample_points(2, 64, 0.5, 2020, 1, DEV)
        clouds = rand(3, 64, 3, seed=1)
        ops.slice_clouds(clouds, target=32, seed=3)
        g = golden("slicer")                                               # a cloud with the candidate planes it was cut by
        name = g["cases"][0]
        ops.slice_clouds(torch.from_numpy(g[f"{name}_points"]).cuda().unsqueeze(0), g[f"{name}_part_a"].shape[0],
                         planes=g[f"{name}_planes"])
        ids = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
        streams = torch.tensor([5, 6], dtype=torch.int64, device=DEV)
        degrees = torch.tensor([90, 7], dtype=torch.int32, device=DEV)
        ops.make_batch(clouds, ids, streams, target=32, degrees=degrees, seed=2 ** 64 - 3)
        ops.make_batch(clouds, ids, streams, target=32, out=ops.make_batch_buffers(2, 64, 32, DEV),
                       ws=ops.make_batch_workspace(2, 64, DEV))
        frames = ops.view_frames(2, 1).cuda()
        ops.make_view_batch(clouds, ids, frames, target=32, degrees=degrees, resolution=8)
        ops.make_view_batch(clouds, ids, frames, target=32, resolution=8,
                            out=ops.make_view_batch_buffers(2, 64, 32, DEV, side=False, occlusion=False))


# ================================================================================================ the evaluation utilities
def test_evaluation_utilities(book):
    from hyperpocket_amd import ops
    from hyperpocket_amd.utils import metrics
    from hyperpocket_amd.utils import tsne as tsne_utils
    from hyperpocket_amd.utils.evaluation.cloud_pairs import cloud_pairs
    from hyperpocket_amd.utils.evaluation.emd_exact import emd_exact_pairs
    from hyperpocket_amd.utils.evaluation.emd_pairs import emd_pairs
    from hyperpocket_amd.utils.render import render_clouds
    from hyperpocket_amd.utils.sphere_mesh import sphere_mesh
    with checked(book, "evaluation utilities"):
        A, B = rand(2, 64, 3, seed=1), rand(3, 48, 3, seed=2)
        pairs = torch.tensor([[0, 0], [1, 2], [0, 1]])
        for mode in (0, 1, 2):
            cloud_pairs(mode, A, B, pairs, thres=0.1)
        emd_pairs(A, B, pairs)
        C = rand(3, 64, 3, seed=3)
        emd_exact_pairs(A, C, pairs, return_assignment=True)
        metrics.emd_approx(A, C[:2])
        metrics.emd_exact(A, C[:2])
        metrics.jsd_between_point_cloud_sets(A.cpu().numpy(), C.cpu().numpy(), resolution=4)
        metrics.entropy_of_occupancy_grid(A, 4, in_sphere=True)
        X = rand(12, 5, seed=4)
        tsne_utils.tsne(X, perplexity=3.0, max_iter=4, explore=2)
        D = ops.pairwise_sqdist(X)
        P, _, _ = ops.tsne_affinities(D, 3.0)
        tsne_utils.tsne_gradient(P, rand(12, 2, seed=5), kl=True)
        render_clouds(A, overlay=A[:, :4], size=(16, 8))
        ops.render_points(A, [64], [(10, 20, 30)], [2], torch.eye(3, 4).reshape(1, 3, 4).cuda(), (8, 8), ids=True)
        mesh = sphere_mesh("hybrid", 1)
        verts = torch.from_numpy(np.stack([mesh.vertices, mesh.vertices * 0.5])).cuda()
        faces = torch.from_numpy(mesh.faces).cuda()
        vf = tuple(torch.as_tensor(t).to(torch.int32).cuda() for t in mesh.vertex_faces)
        ops.mesh_normals(verts, faces, vf, face_normals=True)
        ops.mesh_sample(verts, faces, 5, seed=1)


# ======================================================================================================= the scan wrappers
HOST_TABLES = {"depth_points": ("intrinsics",), "fuse_volume": ("intrinsics", "poses", "origin")}     # host data by contract


def on_gpu(tensors, stay=()):
    return {k: (v.cuda() if torch.is_tensor(v) and k not in stay else v) for k, v in tensors.items()}


def test_every_scan_wrapper_with_and_without_caller_buffers(book):
    """The cases of tests/test_ops_wrappers_host.py (six rows in two scans, two clouds, two meshes), on the device: once with
    the wrapper's own buffers and once with the caller's."""
    import test_ops_wrappers_host as host
    from hyperpocket_amd import ops
    with checked(book, "scan wrappers"):
        for case in host.CASES:
            x = on_gpu(case.inputs(host.SIZES), HOST_TABLES.get(case.name, ()))
            case.run(ops, x, None, None)
            ws = case.workspace(ops, host.SIZES)
            case.run(ops, x, on_gpu(case.out(host.SIZES)), None if ws is None else ws.cuda())
        pts, offs = rand(6, 3, seed=1), torch.tensor([0, 4, 6]).cuda()
        center, scale = ops.scan_boxes(pts, offs)
        ops.restore_scans(rand(2, 8, 3, seed=2), torch.ones(2).cuda(), center, scale)
    assert {"hp_scan_boxes", "hp_restore_scans", "hp_knn_points", "hp_scan_visibility", "hp_depth_points", "hp_fuse_volume",
            "hp_fuse_surface"} <= set(book.families["scan wrappers"])


# ========================================================================================= the plan and workspace queries
def test_every_plan_and_workspace_query(book):
    from hyperpocket_amd import ops
    with checked(book, "plans and workspaces"):
        ops.encoder_plan(2, 128)
        ops.encoder_plan(2, 128, 128, (True, False), ld=(256, 256))
        ops.knn_points_plan(4)
        ops.knn_grid_plan(4)
        ops.knn_grid_buffers(2, 6, DEV, Q=3)
        ops.scan_normals_plan(4)
        ops.scan_clusters_plan()
        ops.scan_plane_plan(16)
        ops.scan_plane_buffers(2, 6, 16, DEV)
        ops.scan_align_plan(2)
        ops.scan_align_plane_plan(2)
        ops.scan_features_plan(4)
        ops.scan_feature_match_plan()
        ops.scan_pose_trials_plan(64, 8)
        ops.scan_voxels_plan()
        ops.scan_voxels_buffers(2, 6, DEV)
        ops.scan_visibility_plan(6)
        ops.scan_visibility_plan(6, 3)
        ops.scan_visibility_buffers(2, 8, DEV, Q=3)
        ops.depth_points_plan(2, 8, 8)
        ops.depth_points_buffers(2, 8, 8, DEV)
        ops.fuse_volume_plan(2, 8, 8, 1, (8, 8, 8))
        ops.fuse_volume_buffers(2, 8, 8, 1, (8, 8, 8), DEV)
        ops.fuse_surface_plan(1, (8, 8, 8))
        ops.fuse_surface_buffers(1, (8, 8, 8), 16, DEV)
        ops.mesh_sample_buffers(2, 2, 3, DEV)
        ops.mesh_sample_buffers(1, 8200, 2, DEV)
        ops.make_batch_workspace(2, 64, DEV)
        ops.pairwise_sqdist_plan(12, 5)
        ops.render_points_plan(1, 1, (8, 8))
        ops.gemm_plan(torch.zeros(130, 70), torch.zeros(50, 70))


# ====================================================================================================== the proxy changes nothing
def test_the_proxy_changes_nothing(book):
    """One wrapper of each family, with and without the proxy: the same bits (the kernels are run-to-run identical)."""
    from hyperpocket_amd import ops
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    from hyperpocket_amd.utils.evaluation.cloud_pairs import cloud_pairs
    a, c = rand(2, 100, 3, seed=1), rand(2, 37, 3, seed=2)
    offs = torch.tensor([0, 40, 100]).cuda()

    def adam():
        p, g, m, v = (rand(1000, seed=s) for s in range(4))
        ops.adam_step(p, g, m, v.abs(), 1e-3, 0.9, 0.999, 1e-8, 3)
        return p

    runs = {"losses": lambda: ChamferLoss()(a, c),
            "optimizers": adam,
            "gemm": lambda: ops.gemm(a[0], c[0], relu=True),
            "samplers": lambda: ops.sample_points(2, 64, 0.5, 7, 1, DEV),
            "evaluation": lambda: cloud_pairs(0, a, c, torch.tensor([[0, 1], [1, 0]])),
            "scans": lambda: torch.cat([t.float().reshape(-1) for t in ops.knn_points(a[0], offs, 3)])}
    plain = {k: fn() for k, fn in runs.items()}
    with checked(book, "with and without the proxy"):
        behind = {k: fn() for k, fn in runs.items()}
    for k in runs:
        assert torch.equal(plain[k], behind[k]), k


# =========================================================================================================== nothing slips by
def source_sites():
    """{entry: [(file, line, enclosing top-level name, ast.Call or None)]} for every hp_* name in the package's code: an
    attribute (lib.hp_x) or a whole string constant ("hp_x") that is no docstring."""
    sites = {}
    for path in sorted(glob.glob(os.path.join(PACKAGE, "**", "*.py"), recursive=True)):
        rel = os.path.relpath(path, PACKAGE)
        tree = ast.parse(open(path).read())
        tops = []
        for node in tree.body:                                     # a class is taken method by method
            if isinstance(node, ast.ClassDef):
                tops += [(f"{node.name}.{getattr(item, 'name', '<body>')}", item) for item in node.body]
            else:
                tops.append((getattr(node, "name", "<module>"), node))
        for owner, top in tops:
            docstrings = {id(n.body[0].value) for n in ast.walk(top)
                          if isinstance(n, (ast.FunctionDef, ast.ClassDef, ast.AsyncFunctionDef)) and n.body
                          and isinstance(n.body[0], ast.Expr) and isinstance(n.body[0].value, ast.Constant)}
            if isinstance(top, ast.Expr) and isinstance(top.value, ast.Constant):
                docstrings.add(id(top.value))
            calls = {}
            for n in ast.walk(top):
                if isinstance(n, ast.Call):
                    if isinstance(n.func, ast.Attribute) and n.func.attr.startswith("hp_"):
                        calls[id(n.func)] = n                      # lib.hp_x(...)
                    for a in n.args[:1]:
                        if isinstance(a, ast.Constant):
                            calls[id(a)] = n                       # call("hp_x", ...), _long_fn("hp_x", ...)
            for n in ast.walk(top):
                name = None
                if isinstance(n, ast.Attribute) and n.attr.startswith("hp_"):
                    name = n.attr
                elif isinstance(n, ast.Constant) and isinstance(n.value, str) and id(n) not in docstrings \
                        and n.value.startswith("hp_") and n.value.replace("_", "").isalnum():
                    name = n.value
                if name:
                    sites.setdefault(name, []).append((rel, n.lineno, owner, calls.get(id(n))))
    return sites


def is_multi_rank(site):
    rel, _, owner, _ = site
    return rel == "parallel.py" or (rel, owner) in MULTI_RANK_SITES


WIDE_CONSTRUCTORS = {"c_long", "c_longlong", "c_ulong", "c_ulonglong", "c_int64", "c_uint64", "c_size_t"}


def static_argument(node):
    """What the outermost constructor of an argument expression says about the object ctypes gets: a stand-in object for
    compatible(), or None where the expression does not tell (a tensor, a name)."""
    if isinstance(node, ast.Call):
        f = node.func
        ctor = f.attr if isinstance(f, ast.Attribute) else getattr(f, "id", "")
        if ctor in WIDE_CONSTRUCTORS:
            return ctypes.c_longlong(0)
        if ctor in ("c_double", "c_float", "c_int", "c_void_p"):
            return getattr(ctypes, ctor)(0)
        if ctor == "float":
            return ctypes.c_float(0.0)                             # _lib.call's conversion
        if ctor in ("int", "bool", "len"):
            return ctypes.c_int(0)
        if ctor in ("current_stream", "ptr"):
            return ctypes.c_void_p(0)
        if ctor == "byref":
            return ctypes.byref(ctypes.c_int(0))
    return None


def test_nothing_slips_by(book):
    """Run after every family above.  Source names = observed names (GPU record + host record) + exempt names, and every
    declared entry point is observed, exempt or absent from the package."""
    from test_capi_contract_host import recorded_calls
    table = capi_law.prototypes()
    sites = source_sites()
    in_source = set(sites)
    assert in_source <= set(table), sorted(in_source - set(table))           # no name the header does not declare
    on_gpu_names = book.log.names()
    on_host = {entry for _, _, entry, _ in recorded_calls()}
    observed = on_gpu_names | on_host
    exempt = set(EXEMPT)
    # an exemption holds only while every call site of the name is a multi-rank one, and names its sites
    for name in exempt:
        assert name in sites and all(is_multi_rank(s) for s in sites[name]), (name, sites.get(name))
        assert sorted(f"{rel}:{line}" for rel, line, _, _ in sites[name]) == sorted(EXEMPT[name]), (name, sites[name])
    should_be_exempt = {n for n in in_source - observed if all(is_multi_rank(s) for s in sites[n])}
    assert should_be_exempt <= exempt, sorted(should_be_exempt - exempt)
    unseen = in_source - observed - exempt
    print("entry points declared", len(table), "| in the package's source", len(in_source), "| observed on the GPU",
          len(on_gpu_names), "| in the host record", len(on_host), "| exempt", sorted(exempt))
    for name in sorted(unseen):
        print("NOT OBSERVED", name, [(rel, line) for rel, line, _, _ in sites[name]])
    assert not unseen
    assert observed & exempt == set(), sorted(observed & exempt)             # an exempt name that ran needs no exemption
    assert observed - exempt <= in_source | on_host
    absent = sorted(set(table) - in_source)
    print("declared, absent from the package:", len(absent), absent)
    assert "hp_gemm_workspace_floats" in absent
    assert set(table) == (observed & set(table)) | exempt | set(absent)
    assert book.log.violations == []


def test_the_exempt_call_sites_statically():
    """The multi-rank call sites (a second GPU, a process group) by the text of the call: the argument count, and each
    argument whose outermost constructor tells its class, against the rule; an 8-byte return needs its restype set on the
    function object in the same function."""
    table = capi_law.prototypes()
    sites = source_sites()
    checked_calls = 0
    for name, where in sites.items():
        for site in where:
            rel, line, owner, call = site
            if not is_multi_rank(site) or call is None:
                continue
            ret, params = table[name]
            by_name = bool(call.args) and isinstance(call.args[0], ast.Constant) and call.args[0].value == name
            args = call.args[1:] if by_name else call.args             # call("hp_x", ...) or lib.hp_x(...)
            assert not any(isinstance(a, ast.Starred) for a in args), (rel, line)
            assert len(args) == len(params), (name, rel, line, len(args), len(params))
            for i, (p, a) in enumerate(zip(params, args)):
                stand_in = static_argument(a)
                if stand_in is not None:
                    assert capi_law.compatible(p, stand_in), (name, rel, line, i, p, ast.dump(a))
                else:
                    assert p == "ptr" or p == "i32", (name, rel, line, i, p, "a wide parameter needs its constructor at the call")
            if ret == "i64":
                text = open(os.path.join(PACKAGE, rel)).read()
                assert f"{name}.restype = ctypes.c_long" in text or f'_long_fn("{name}"' in text, (name, rel, line)
            checked_calls += 1
    assert checked_calls >= 1                                                # HeadsShard.begin's workspace query

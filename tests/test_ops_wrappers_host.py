"""CPU suite for the Python wrappers of the scan, mesh and resampling kernels in hyperpocket_amd/ops.py (needs the built
library for the workspace and plan queries, not a GPU): what each wrapper allocates, which caller's buffers it refuses and
with which exception type, what it serves on the host for empty input, and the exact argument list it hands to its entry
point.  check_input's device test is switched off so that CPU tensors reach the checks behind it, and ops.call is replaced by
a recorder: nothing is launched.

The argument lists are compared with tests/golden/ops_wrapper_calls.json.  `python tests/test_ops_wrappers_host.py` writes
that file from the checked-out ops.py: do that only when an entry point's signature changes on purpose."""
import contextlib
import ctypes
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import GOLDEN, PKG_DIR  # noqa: E402  (also puts the package on sys.path)

RECORD = os.path.join(GOLDEN, "ops_wrapper_calls.json")
S, K, H, TRIALS, KEEP = 2, 2, 2, 4, 2
SIZES = {"T": 6, "U": 5, "Q": 3, "B": 2, "M": 2}           # rows of the sets, clouds of a batch, meshes
OFFSETS = {6: [0, 4, 6], 5: [0, 3, 5], 3: [0, 2, 3], 0: [0, 0, 0]}
STREAM = object()
POISON = 77
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


class FakeDevice(torch.Tensor):
    """axis_split tests is_cuda itself: a CPU tensor that says yes."""
    is_cuda = property(lambda self: True)


@pytest.fixture(scope="module", autouse=True)
def built_library():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)


@contextlib.contextmanager
def recording():
    """ops with check_input's device test off, call recording and the stream a token; yields the list of recorded calls."""
    from hyperpocket_amd import ops
    real = ops.check_input, ops.call, ops.current_stream
    calls = []

    def no_device_check(t, name, dtype=torch.float32):
        if not t.is_contiguous() or t.dtype != dtype:
            real[0](t, name, dtype)                                # raises its own message

    ops.check_input, ops.call, ops.current_stream = no_device_check, lambda *a: calls.append(a), lambda device=None: STREAM
    try:
        yield calls
    finally:
        ops.check_input, ops.call, ops.current_stream = real


def rows(n, width=3, dtype=F32):
    return torch.arange(n * width, dtype=F32).reshape(n, width).to(dtype)


def offsets(n):
    return torch.tensor(OFFSETS[n])


class Case:
    """inputs(d) -> named tensors for the sizes d; run(ops, x, out, ws) calls the wrapper; members: (name, dtype, shape(d));
    returns: "dict" or the names of the returned tuple; exc: the type a buffer of the wrong shape or size is refused with; ws:
    (bytes(ops, d), dtype) of a workspace passed beside out; empty: the sizes of the host-served run and fills: what its
    members hold then; optional: members a fresh dict does not get or the wrapper does not return; derived: inputs the entry
    point gets a rearranged copy of; dtype_exc: see __init__."""

    def __init__(self, name, inputs, run, members, returns, exc=None, ws=None, empty=None, fills=None, empty_calls=0,
                 optional=(), derived=(), dtype_exc=None):
        self.name, self.inputs, self.run, self.members, self.returns = name, inputs, run, members, returns
        self.exc, self.ws, self.empty, self.fills, self.empty_calls = exc, ws, empty, fills or {}, empty_calls
        self.optional, self.derived = optional, derived
        self.dtype_exc = dtype_exc                                 # the type a member of the wrong dtype is refused with, if not HipExtensionError

    def out(self, d):
        return {name: torch.full(shape(d), POISON, dtype=dtype) for name, dtype, shape in self.members}

    def workspace(self, ops, d):
        if self.ws is None:
            return None
        need, dtype = self.ws[0](ops, d), self.ws[1]
        return torch.empty((need // torch.empty((), dtype=dtype).element_size(),), dtype=dtype)

    def named(self, result):
        if result is None:
            return {}
        return dict(result) if self.returns == "dict" else dict(zip(self.returns, result))


def ragged(d):
    return {"points": rows(d["T"]), "offsets": offsets(d["T"])}


def queried(d):
    return dict(ragged(d), queries=rows(d["Q"]), query_offsets=offsets(d["Q"]))


def two_sets(d):
    return dict(ragged(d), tpoints=rows(d["U"]), toffsets=offsets(d["U"]))


def align_sets(d):
    return dict(two_sets(d), transforms=rows(S * H, 12).reshape(S, H, 12), anchor=rows(S), shift=torch.zeros(S, dtype=I32))


def grid_bytes(ops, d, Q=None):
    fn = ops.load_library().hp_knn_grid_workspace_bytes
    fn.restype = ctypes.c_longlong
    return fn(S, ctypes.c_longlong(d["T"]), ctypes.c_longlong(0 if Q is None else Q))


KNN_OUT = [("index", I32, lambda d: (d["T"], K)), ("dist2", F32, lambda d: (d["T"], K))]
KNN_Q_OUT = [("index", I32, lambda d: (d["Q"], K)), ("dist2", F32, lambda d: (d["Q"], K))]
GRID = [("grid", F32, lambda d: (S, 4))]
KNN_FILLS = {"index": -1, "dist2": float("inf"), "grid": 0}
OUTLIER_OUT = [("keep", U8, lambda d: (d["T"],)), ("mean_dist", F32, lambda d: (d["T"],)), ("kept", I32, lambda d: (S,))]
PLANE_OUT = [("trial", I32, lambda d: (S,)), ("inliers", I32, lambda d: (S,)), ("found", I32, lambda d: (S,)),
             ("sample", I32, lambda d: (S, 3)), ("sample_plane", F32, lambda d: (S, 4)), ("inlier", U8, lambda d: (d["T"],)),
             ("moments", I64, lambda d: (S, 10)), ("shift", I32, lambda d: (S,))]
POSE_OUT = [("trial", I32, lambda d: (S,)), ("inliers", I32, lambda d: (S,)), ("found", I32, lambda d: (S,)),
            ("transform", F32, lambda d: (S, 12)), ("valid", I32, lambda d: (S,)), ("kept", I32, lambda d: (S,))]
VOXEL_OUT = [("label", I32, lambda d: (d["T"],)), ("size", I32, lambda d: (d["T"],)), ("keep", U8, lambda d: (d["T"],)),
             ("kept", I32, lambda d: (S,)), ("beyond", I32, lambda d: (S,))]


def align_out(width):
    return [("moments", I64, lambda d: (S, H, width)), ("index", I32, lambda d: (H, d["T"])), ("dist2", F32, lambda d: (H, d["T"]))]


ALIGN_FILLS = {"moments": 0, "index": -1, "dist2": float("inf")}
NO_TARGETS = dict(SIZES, U=0)
NO_ROWS = dict(SIZES, T=0)

CASES = [
    Case("knn_points", ragged, lambda ops, x, out, ws: ops.knn_points(x["points"], x["offsets"], K, out=out),
         KNN_OUT, ("index", "dist2"), empty=NO_ROWS, fills=KNN_FILLS),
    Case("knn_points_queries", queried,
         lambda ops, x, out, ws: ops.knn_points(x["points"], x["offsets"], K, x["queries"], x["query_offsets"], out=out),
         KNN_Q_OUT, ("index", "dist2"), empty=NO_ROWS, fills=KNN_FILLS),
    Case("knn_points_grid", ragged, lambda ops, x, out, ws: ops.knn_points_grid(x["points"], x["offsets"], K, out=out, ws=ws),
         KNN_OUT + GRID, ("index", "dist2"), ws=(grid_bytes, I64), empty=NO_ROWS, fills=KNN_FILLS, optional=("grid",)),
    Case("knn_points_grid_queries", queried,
         lambda ops, x, out, ws: ops.knn_points_grid(x["points"], x["offsets"], K, x["queries"], x["query_offsets"], True, 0.5,
                                                     out=out, ws=ws),
         KNN_Q_OUT + GRID, ("index", "dist2"), ws=(lambda ops, d: grid_bytes(ops, d, d["Q"]), I64), empty=NO_ROWS,
         fills=KNN_FILLS, optional=("grid",)),
    Case("scan_outliers", ragged, lambda ops, x, out, ws: ops.scan_outliers(x["points"], x["offsets"], K, 1.5, out=out),
         OUTLIER_OUT, ("keep", "mean_dist", "kept"), empty=NO_ROWS, fills={"kept": 0}),
    Case("outlier_keep", lambda d: {"mean_dist": rows(d["T"], 1).reshape(-1), "offsets": offsets(d["T"])},
         lambda ops, x, out, ws: ops.outlier_keep(x["mean_dist"], x["offsets"], 1.5, out=out),
         [OUTLIER_OUT[0], OUTLIER_OUT[2]], ("keep", "kept"), empty=NO_ROWS, fills={"kept": 0}),
    Case("scan_outliers_grid", lambda d: dict(ragged(d), cell=torch.full((S,), 0.25)),
         lambda ops, x, out, ws: ops.scan_outliers_grid(x["points"], x["offsets"], K, 1.5, x["cell"], out=out, ws=ws),
         OUTLIER_OUT, ("keep", "mean_dist", "kept"), ws=(grid_bytes, I64), empty=NO_ROWS, fills={"kept": 0}),
    Case("scan_normals", lambda d: dict(ragged(d), viewpoints=torch.ones(3)),
         lambda ops, x, out, ws: ops.scan_normals(x["points"], x["offsets"], K, x["viewpoints"], out=out),
         [("normal", F32, lambda d: (d["T"], 3)), ("curvature", F32, lambda d: (d["T"],)), ("count", I32, lambda d: (d["T"],))],
         ("normal", "curvature", "count"), empty=NO_ROWS, derived=("viewpoints",)),
    Case("scan_normals_index", lambda d: dict(ragged(d), viewpoints=torch.ones((S, 3)), index=torch.zeros((d["T"], K), dtype=I32)),
         lambda ops, x, out, ws: ops.scan_normals(x["points"], x["offsets"], K, x["viewpoints"], x["index"], out=out),
         [("normal", F32, lambda d: (d["T"], 3)), ("curvature", F32, lambda d: (d["T"],)), ("count", I32, lambda d: (d["T"],))],
         ("normal", "curvature", "count"), empty=NO_ROWS),
    Case("scan_clusters", ragged, lambda ops, x, out, ws: ops.scan_clusters(x["points"], x["offsets"], 0.125, 64, out=out),
         [("label", I32, lambda d: (d["T"],)), ("size", I32, lambda d: (d["T"],)), ("clusters", I32, lambda d: (S,)),
          ("largest", I32, lambda d: (S,))], ("label", "size", "clusters", "largest"), empty=NO_ROWS,
         fills={"clusters": 0, "largest": -1}),
    Case("scan_plane", lambda d: dict(ragged(d), streams=torch.tensor([7, 9])),
         lambda ops, x, out, ws: ops.scan_plane(x["points"], x["offsets"], 0.0625, TRIALS, -1, x["streams"], 4, 0.5, out=out, ws=ws),
         PLANE_OUT, "dict", ws=(lambda ops, d: ops._long_fn("hp_scan_plane_workspace_bytes", S, TRIALS), I64), empty=NO_ROWS,
         fills={"trial": -1, "inliers": 0, "found": 0, "sample": -1, "sample_plane": float("nan"), "moments": 0, "shift": 0}),
    Case("scan_plane_side", lambda d: dict(ragged(d), planes=rows(S, 4)),
         lambda ops, x, out, ws: ops.scan_plane_side(x["points"], x["offsets"], x["planes"], 0.0625, out=out),
         [("dist", F32, lambda d: (d["T"],)), ("keep", U8, lambda d: (d["T"],)), ("kept", I32, lambda d: (S,))],
         ("dist", "keep", "kept"), empty=NO_ROWS, fills={"kept": 0}),
    Case("scan_align_step", align_sets,
         lambda ops, x, out, ws: ops.scan_align_step(x["points"], x["offsets"], x["tpoints"], x["toffsets"], x["transforms"], 0.5,
                                                     x["anchor"], x["shift"], out=out, want_index=True),
         align_out(18), "dict", empty=NO_TARGETS, fills=ALIGN_FILLS),
    Case("scan_align_step_moments", align_sets,
         lambda ops, x, out, ws: ops.scan_align_step(x["points"], x["offsets"], x["tpoints"], x["toffsets"], x["transforms"], 0.5,
                                                     x["anchor"], x["shift"], out=out),
         align_out(18)[:1], "dict", empty=NO_TARGETS, fills=ALIGN_FILLS),
    Case("scan_align_plane_step", lambda d: dict(align_sets(d), tnormals=rows(d["U"])),
         lambda ops, x, out, ws: ops.scan_align_plane_step(x["points"], x["offsets"], x["tpoints"], x["toffsets"], x["tnormals"],
                                                           x["transforms"], float("inf"), x["anchor"], x["shift"], out=out,
                                                           want_index=True),
         align_out(60), "dict", empty=NO_TARGETS, fills=ALIGN_FILLS),
    Case("scan_features", lambda d: dict(ragged(d), normals=rows(d["T"]), index=torch.zeros((d["T"], K), dtype=I32)),
         lambda ops, x, out, ws: ops.scan_features(x["points"], x["offsets"], x["normals"], x["index"], out=out),
         [("features", U8, lambda d: (d["T"], 36)), ("count", I32, lambda d: (d["T"],)), ("ws", U8, lambda d: (d["T"] * 36,))],
         ("features", "count"), empty=NO_ROWS, optional=("ws",)),
    Case("scan_feature_match",
         lambda d: {"features": rows(d["T"], 36, U8), "offsets": offsets(d["T"]), "tfeatures": rows(d["U"], 36, U8),
                    "toffsets": offsets(d["U"]), "counts": torch.ones(d["T"], dtype=I32), "tcounts": torch.ones(d["U"], dtype=I32)},
         lambda ops, x, out, ws: ops.scan_feature_match(x["features"], x["offsets"], x["tfeatures"], x["toffsets"], x["counts"],
                                                        x["tcounts"], out=out),
         [("match", I32, lambda d: (d["T"],)), ("dist", I32, lambda d: (d["T"],))], ("match", "dist"), empty=NO_TARGETS,
         fills={"match": -1, "dist": -1}),
    # no host-served result here: the entry point itself answers empty sets, so the call is made
    Case("scan_pose_trials", lambda d: dict(two_sets(d), match=torch.zeros(d["T"], dtype=I32), streams=torch.tensor([3, 1])),
         lambda ops, x, out, ws: ops.scan_pose_trials(x["points"], x["offsets"], x["tpoints"], x["toffsets"], x["match"], 0.25,
                                                      TRIALS, KEEP, 2 ** 64 + 5, x["streams"], 0.9, 3, out=out, ws=ws),
         POSE_OUT, "dict", ws=(lambda ops, d: ops._long_fn("hp_scan_pose_trials_workspace_bytes", S, KEEP), I32), empty=NO_ROWS,
         empty_calls=1),
    Case("scan_voxels", lambda d: dict(ragged(d), origin=rows(S)),
         lambda ops, x, out, ws: ops.scan_voxels(x["points"], x["offsets"], 0.1, x["origin"], "first", 2, out=out, ws=ws),
         VOXEL_OUT, "dict", exc=ValueError,
         ws=(lambda ops, d: ops._long_fn("hp_scan_voxels_workspace_bytes", ctypes.c_longlong(d["T"]), 2), I64), empty=NO_ROWS,
         fills={"kept": 0, "beyond": 0}),
    Case("scan_voxels_tensor", lambda d: dict(ragged(d), voxel=torch.full((S,), 0.5)),
         lambda ops, x, out, ws: ops.scan_voxels(x["points"], x["offsets"], x["voxel"], slots_per_row=4, out=out, ws=ws),
         VOXEL_OUT, "dict", exc=ValueError,
         ws=(lambda ops, d: ops._long_fn("hp_scan_voxels_workspace_bytes", ctypes.c_longlong(d["T"]), 4), I64), empty=NO_ROWS,
         fills={"kept": 0, "beyond": 0}),
    Case("mesh_sample",
         lambda d: {"vertices": rows(d["M"] * 4).reshape(d["M"], 4, 3), "faces": torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=I32),
                    "streams": torch.arange(d["M"]) + 4},
         lambda ops, x, out, ws: ops.mesh_sample(x["vertices"], x["faces"], 3, -2, x["streams"], out=out),
         [("points", F32, lambda d: (d["M"], 3, 3)), ("face", I32, lambda d: (d["M"], 3)), ("area", F64, lambda d: (d["M"],)),
          ("failed", I32, lambda d: (d["M"],))], ("points", "face", "area", "failed"), empty=dict(SIZES, M=0)),
    Case("prepare_scans",
         lambda d: dict(ragged(d), ids=torch.tensor([1, 0, 1], dtype=I32), streams=torch.tensor([5, 6, 7]), center=rows(S),
                        scale=torch.ones(S)),
         lambda ops, x, out, ws: ops.prepare_scans(x["points"], x["offsets"], x["ids"], x["streams"], 4, True, 11, x["center"],
                                                   x["scale"], out=out),
         [("existing", F32, lambda d: (3, 4, 3)), ("index", I32, lambda d: (3, 4))], ("existing", "index", "failed"),
         optional=("failed",)),
    Case("farthest_points",
         lambda d: {"clouds": rows(d["B"] * 5).reshape(d["B"], 5, 3), "counts": torch.full((d["B"],), 5, dtype=I32),
                    "start": torch.zeros(d["B"], dtype=I32)},
         lambda ops, x, out, ws: ops.farthest_points(x["clouds"], K, x["counts"], x["start"], out=out),
         [("index", I32, lambda d: (d["B"], K)), ("radius2", F32, lambda d: (d["B"], K))], ("index", "radius2"),
         empty=dict(SIZES, B=0)),
    Case("axis_split", lambda d: {"clouds": rows(d["B"] * 5).reshape(d["B"], 5, 3).as_subclass(FakeDevice)},
         lambda ops, x, out, ws: ops.axis_split(x["clouds"], K, 1, out=out),
         [("lower", F32, lambda d: (d["B"], K, 3)), ("upper", F32, lambda d: (d["B"], 5 - K, 3)), ("order", I32, lambda d: (d["B"], 5))],
         ("lower", "upper", "order"), empty=dict(SIZES, B=0)),
]
# ---- the depth, fusion, visibility and view wrappers: images of IMG x IMG pixels, volumes of VOX^3 voxels, a depth buffer of
# RES pixels per edge.  depth_points, fuse_volume and fuse_surface look at is_cuda themselves.
IMG, VOX, RES, CAP = 2, 2, 8, 4


def on_device(t):
    return t.as_subclass(FakeDevice)


def images(d):
    return {"depth": on_device(rows(d["B"] * IMG * IMG, 1).reshape(d["B"], IMG, IMG) + 1), "intrinsics": torch.tensor([2.0, 2.0, 0.5, 0.5]),
            "masks": on_device(torch.ones((d["B"], IMG, IMG), dtype=U8))}


def posed_images(d):
    return dict(images(d), poses=torch.eye(3, 4, dtype=F64).expand(d["B"], 3, 4).contiguous(), origin=torch.zeros(3, dtype=F64))


def volume(d):
    return {"tsdf": on_device(rows(VOX ** 3, 1).reshape(1, VOX, VOX, VOX) - 3.5), "weight": on_device(torch.ones((1, VOX, VOX, VOX), dtype=I32)),
            "origin": on_device(torch.zeros((1, 3), dtype=F64))}


def fuse_bytes(entry, *shape):
    return lambda ops, d: ops._fuse_workspace_bytes(entry, *[d["B"] if x == "B" else x for x in shape])


def tensors_of(result, names):
    return {n: result[n] for n in names}


def views(d):
    return {"clouds": rows(3 * 5).reshape(3, 5, 3), "ids": torch.tensor([2, 0], dtype=I32)[:d["B"]],
            "frames": torch.eye(3).expand(d["B"], 3, 3).contiguous(), "degrees": torch.tensor([90, 7], dtype=I32)[:d["B"]],
            "rot": rows(360, 2)}


DEPTH_OUT = [("points", F32, lambda d: (d["B"] * IMG * IMG, 3)), ("normals", F32, lambda d: (d["B"] * IMG * IMG, 3)),
             ("pixel", I64, lambda d: (d["B"] * IMG * IMG,)), ("offsets", I64, lambda d: (d["B"] + 1,))]
VOLUME_OUT = [("tsdf", F32, lambda d: (1, VOX, VOX, VOX)), ("weight", I32, lambda d: (1, VOX, VOX, VOX))]
SURFACE_OUT = [("points", F32, lambda d: (CAP, 3)), ("normals", F32, lambda d: (CAP, 3)), ("cell", I64, lambda d: (CAP,)),
               ("offsets", I64, lambda d: (2,))]
VIEW_OUT = [("existing", F32, lambda d: (d["B"], 2, 3)), ("missing", F32, lambda d: (d["B"], 3, 3)), ("gt", F32, lambda d: (d["B"], 5, 3)),
            ("side", U8, lambda d: (d["B"], 5)), ("occlusion", F32, lambda d: (d["B"], 5))]

CASES += [
    Case("scan_visibility", lambda d: dict(ragged(d), viewpoints=torch.ones(3)),
         lambda ops, x, out, ws: ops.scan_visibility(x["points"], x["offsets"], x["viewpoints"], RES, 1, 0.01, 2.0, out=out, ws=ws),
         [("label", U8, lambda d: (d["T"],)), ("winner", U8, lambda d: (d["T"],))], "dict", exc=ValueError,
         ws=(lambda ops, d: ops._visibility_workspace_bytes(S, RES), I64), empty=NO_ROWS, derived=("viewpoints",)),
    Case("scan_visibility_queries", lambda d: dict(queried(d), viewpoints=torch.ones((S, 3))),
         lambda ops, x, out, ws: ops.scan_visibility(x["points"], x["offsets"], x["viewpoints"], RES, 2, 0.0, 1.5, x["queries"],
                                                     x["query_offsets"], out=out, ws=ws),
         [("label", U8, lambda d: (d["Q"],))], "dict", exc=ValueError,
         ws=(lambda ops, d: ops._visibility_workspace_bytes(S, RES), I64), empty=dict(SIZES, Q=0)),
    Case("depth_points", images,
         lambda ops, x, out, ws: ops.depth_points(x["depth"], x["intrinsics"], None, x["masks"], 0.5, 0.25, 100.0, (0.125, 0.5), 1,
                                                  out=out, ws=ws),
         DEPTH_OUT, "dict", exc=ValueError, dtype_exc=ValueError,
         ws=(lambda ops, d: ops._depth_workspace_bytes(d["B"], IMG, IMG), I32), derived=("intrinsics",)),
    Case("fuse_volume", posed_images,
         lambda ops, x, out, ws: tensors_of(ops.fuse_volume(x["depth"], x["intrinsics"], x["poses"], None, x["origin"], (VOX, VOX, VOX),
                                                            0.5, 1.5, x["masks"], 0.5, 0.25, 100.0, (0.125, 0.5), 1, out=out, ws=ws),
                                            ("tsdf", "weight")),
         VOLUME_OUT, "dict", exc=ValueError, dtype_exc=ValueError,
         ws=(fuse_bytes("hp_fuse_volume_workspace_bytes", "B", IMG, IMG), I64), derived=("intrinsics", "poses")),
    Case("fuse_surface", volume,
         lambda ops, x, out, ws: ops.fuse_surface(dict(x, voxel=0.5), 1, CAP, out=out, ws=ws),
         SURFACE_OUT, "dict", exc=ValueError, dtype_exc=ValueError,
         ws=(fuse_bytes("hp_fuse_surface_workspace_bytes", 1, VOX, VOX, VOX), I64)),
    Case("make_view_batch", views,
         lambda ops, x, out, ws: ops.make_view_batch(x["clouds"], x["ids"], x["frames"], 2, x["degrees"], x["rot"], 3.0, 0.25, RES, 1,
                                                     out=out),
         VIEW_OUT, ("existing", "missing", "gt", "side", "occlusion")),
    Case("restore_scans",
         lambda d: {"completions": rows(d["B"] * 5).reshape(d["B"], 5, 3), "s_scale": torch.ones(d["B"]), "center": rows(d["B"]),
                    "scale": torch.full((d["B"],), 2.0)},
         lambda ops, x, out, ws: (ops.restore_scans(x["completions"], x["s_scale"], x["center"], x["scale"]),),
         [], ("restored",), optional=("restored",)),
]
BY_NAME = {c.name: c for c in CASES}
each_case = pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])


def holds(t, value):
    return bool(torch.isnan(t).all()) if value != value else bool((t == value).all())


def describe(a, labels):
    if isinstance(a, torch.Tensor):
        label = labels.get(a.data_ptr()) if a.numel() else None
        return label or f"new:{str(a.dtype)[6:]}{list(a.shape)}"
    if a is None:
        return "null"
    if a is STREAM:
        return "stream"
    if isinstance(a, ctypes._SimpleCData):
        return f"{type(a).__name__}:{a.value!r}"
    return f"{type(a).__name__}:{a!r}"


def recorded(case, fresh):
    """The calls of one run as [entry, [argument, ...]] lists: a tensor is named after the input or the output member it is
    (by address), another one after its dtype and shape, a scalar after its type and value."""
    from hyperpocket_amd import ops
    with recording() as calls:
        x = case.inputs(SIZES)
        out, ws = (None, None) if fresh else (case.out(SIZES), case.workspace(ops, SIZES))
        result = case.named(case.run(ops, x, out, ws))
    labels = {t.data_ptr(): f"in:{name}" for name, t in x.items()}
    labels.update({t.data_ptr(): f"out:{name}" for name, t in dict(result, **(out or {})).items() if t is not None})
    if ws is not None:
        labels[ws.data_ptr()] = "ws"
    return [[c[0], [describe(a, labels) for a in c[1:]]] for c in calls]


def record_all():
    return {case.name: {"given": recorded(case, False), "fresh": recorded(case, True)} for case in CASES}


@each_case
def test_a_fresh_call_allocates_the_documented_members(case):
    from hyperpocket_amd import ops
    with recording():
        result = case.named(case.run(ops, case.inputs(SIZES), None, None))
    want = {name: (dtype, shape(SIZES)) for name, dtype, shape in case.members if name not in case.optional}
    assert {n for n in result if n not in case.optional} == set(want)
    for name, (dtype, shape) in want.items():
        assert result[name].dtype == dtype and tuple(result[name].shape) == shape, name


@each_case
def test_a_buffer_of_the_wrong_shape_or_dtype_is_refused(case):
    from hyperpocket_amd import HipExtensionError, ops
    exc = case.exc or HipExtensionError
    with recording() as calls:
        x, good, ws = case.inputs(SIZES), case.out(SIZES), case.workspace(ops, SIZES)
        case.run(ops, x, dict(good), ws)                           # the buffers themselves are fine
        assert len(calls) >= 1
        del calls[:]
        for name, dtype, shape in case.members:
            longer = (shape(SIZES)[0] + 1,) + shape(SIZES)[1:]
            with pytest.raises(exc) as e:
                case.run(ops, x, dict(good, **{name: torch.empty(longer, dtype=dtype)}), ws)
            assert type(e.value) is exc, name
            with pytest.raises(case.dtype_exc or HipExtensionError):
                case.run(ops, x, dict(good, **{name: torch.empty(shape(SIZES), dtype=torch.int16)}), ws)
        if ws is not None:
            # too small; large enough but 8 (int64) or 4 (int32) bytes off a 16-byte boundary; on another device
            roomy = torch.empty(ws.numel() + 4, dtype=ws.dtype)
            assert roomy.data_ptr() % 16 == 0 and roomy[1:].data_ptr() % 16 != 0
            for bad in (ws[:-1], roomy[1:], torch.empty(ws.shape, dtype=ws.dtype, device="meta")):
                with pytest.raises(exc) as e:
                    case.run(ops, x, dict(good), bad)
                assert type(e.value) is exc and f"ws must hold {ws.numel() * ws.element_size()} bytes" in str(e.value)
            case.run(ops, x, dict(good), roomy[4:] if ws.dtype == I32 else roomy[2:])      # aligned again: accepted
            assert len(calls) == 1
            del calls[:]
        assert calls == []


@pytest.mark.parametrize("case", [c for c in CASES if c.empty], ids=[c.name for c in CASES if c.empty])
def test_empty_input_is_served_on_the_host(case):
    from hyperpocket_amd import ops
    for fresh in (False, True):
        with recording() as calls:
            x = case.inputs(case.empty)
            out = None if fresh else case.out(case.empty)
            result = case.named(case.run(ops, x, out, None if fresh else case.workspace(ops, case.empty)))
        assert len(calls) == case.empty_calls
        members = result if fresh else out
        for name, dtype, shape in case.members:
            if name in members and members[name] is not None:
                assert tuple(members[name].shape) == shape(case.empty)
                if name in case.fills:
                    assert holds(members[name], case.fills[name]), name
                elif not fresh and not case.empty_calls:
                    assert holds(members[name], POISON), name          # nothing is written


@each_case
def test_the_entry_point_gets_the_recorded_arguments(case):
    with open(RECORD) as f:
        want = json.load(f)[case.name]
    assert recorded(case, False) == want["given"]
    assert recorded(case, True) == want["fresh"]


def test_the_record_names_every_case_and_every_argument():
    with open(RECORD) as f:
        want = json.load(f)
    assert set(want) == set(BY_NAME)
    for name, runs in want.items():
        case = BY_NAME[name]
        for call in runs["given"]:
            assert call[0].startswith("hp_") and call[1][-1] == "stream"
        given = [a for call in runs["given"] for a in call[1]]
        for member, _, _ in case.members:
            assert f"out:{member}" in given, (name, member)
        for x in case.inputs(SIZES):
            assert (f"in:{x}" in given) == (x not in case.derived), (name, x)
        assert ("ws" in given) == (case.ws is not None)


def test_rows_are_checked_in_order_where_the_types_differ():
    """scan_voxels refuses a shape with ValueError and a dtype with HipExtensionError: the first bad member decides."""
    from hyperpocket_amd import HipExtensionError, ops
    case = BY_NAME["scan_voxels"]
    with recording() as calls:
        x, good, ws = case.inputs(SIZES), case.out(SIZES), case.workspace(ops, SIZES)
        with pytest.raises(ValueError):
            case.run(ops, x, dict(good, label=torch.empty(7, dtype=I32), size=torch.empty(6, dtype=I64)), ws)
        with pytest.raises(HipExtensionError):
            case.run(ops, x, dict(good, label=torch.empty(6, dtype=I64), size=torch.empty(7, dtype=I32)), ws)
        assert calls == []


def test_a_table_knows_its_letters_and_its_labels():
    from hyperpocket_amd import ops
    table = ops._table(("a", F32, ("T", 3), None), ("b", I32, ("S",), 0), ("c", U8, ("T", 3), None))
    assert tuple(table) == (("a", F32, ("T", 3), None), ("b", I32, ("S",), 0), ("c", U8, ("T", 3), None))
    assert table.resolve({"S": 2, "T": 6, "unused": 9}) == ((6, 3), (2,))
    assert table.checks == (("a", "out['a']", F32, 0), ("b", "out['b']", I32, 1), ("c", "out['c']", U8, 0))
    with pytest.raises(KeyError):                                  # a letter the wrapper did not hand over
        ops._outputs(None, table, {"T": 6}, "cpu", "the scans")
    assert [(n, tail) for n, _, tail in ops._POSE_OUT] == [(n, shape[1:]) for n, _, shape, _ in ops._POSE_ROWS]


def test_members_a_caller_may_leave_out():
    from hyperpocket_amd import HipExtensionError, ops
    with recording() as calls:
        case = BY_NAME["farthest_points"]
        out = dict(case.out(SIZES), radius2=None)
        index, radius2 = case.run(ops, case.inputs(SIZES), out, None)
        assert index is out["index"] and radius2 is None and calls[-1][8] is None
        case = BY_NAME["axis_split"]
        out = dict(case.out(SIZES), order=None)
        lower, upper, order = case.run(ops, case.inputs(SIZES), out, None)
        assert lower is out["lower"] and upper is out["upper"] and order is None and calls[-1][8] is None
        case = BY_NAME["knn_points_grid"]
        out = case.out(SIZES)
        del out["grid"]
        case.run(ops, case.inputs(SIZES), out, None)
        assert calls[-1][0] == "hp_knn_grid" and calls[-1][12] is None
        case = BY_NAME["scan_align_step_moments"]                  # index and dist2 of an earlier call are left alone
        out = BY_NAME["scan_align_step"].out(SIZES)
        case.run(ops, case.inputs(SIZES), out, None)
        assert calls[-1][-3] is None and calls[-1][-2] is None and holds(out["index"], POISON)
        with pytest.raises(HipExtensionError):
            BY_NAME["scan_align_step"].run(ops, case.inputs(SIZES), {"moments": out["moments"], "index": out["index"][:1],
                                                                     "dist2": out["dist2"]}, None)


def test_scalars_become_per_scan_tensors_and_seed_words():
    from hyperpocket_amd import ops
    with recording() as calls:
        BY_NAME["scan_voxels"].run(ops, BY_NAME["scan_voxels"].inputs(SIZES), None, None)
        voxel = calls[-1][5]
        assert voxel.dtype == F32 and voxel.tolist() == [torch.tensor(0.1).item()] * S
        BY_NAME["knn_points_grid_queries"].run(ops, BY_NAME["knn_points_grid_queries"].inputs(SIZES), None, None)
        assert calls[-1][8].dtype == F32 and calls[-1][8].tolist() == [0.5, 0.5]
        BY_NAME["knn_points_grid"].run(ops, BY_NAME["knn_points_grid"].inputs(SIZES), None, None)
        assert calls[-1][8] is None
        BY_NAME["scan_plane"].run(ops, BY_NAME["scan_plane"].inputs(SIZES), None, None)
        assert type(calls[-1][5]) is ctypes.c_ulonglong and calls[-1][5].value == 2 ** 64 - 1
        BY_NAME["scan_pose_trials"].run(ops, BY_NAME["scan_pose_trials"].inputs(SIZES), None, None)
        assert type(calls[-1][10]) is ctypes.c_ulonglong and calls[-1][10].value == 5
        assert calls[-1][13].value == torch.tensor(0.9 * 0.9).item()     # edge_ratio^2 at its fp32 rounding


def test_scalar_checks_decide_as_fp32_arithmetic_does():
    """A radius or threshold needs a finite fp32 square, a cell or voxel edge a positive finite fp32 value: the checkers
    against torch's own float32 arithmetic, at the ends of the range."""
    from hyperpocket_amd import HipExtensionError, ops
    top = torch.tensor(torch.finfo(F32).max).sqrt()
    values = [0.0, -0.0, 1e-60, 1e-46, 1e-40, 1.0, 1e20, 3.4e38, 3.5e38, 1e60, float("inf"), float("nan"), -1.0, -1e-50,
              1.8446743e19, 1.8446744e19, 1.844674352395373e19, 1.8446744073709552e19]
    for towards in (0.0, float("inf")):
        x = top
        for _ in range(6):
            values.append(float(x))
            x = torch.nextafter(x, torch.tensor(towards))
    for v in values:
        v32 = torch.tensor(v, dtype=F32)
        square_ok = bool(v >= 0.0 and torch.isfinite(v32.square()))
        edge_ok = bool(torch.isfinite(v32)) and float(v32) > 0.0
        for ok, check in ((square_ok, lambda: ops._check_fp32_square(v, "radius")), (edge_ok, lambda: ops._per_scan(v, "cell", S, "cpu"))):
            if ok:
                check()
            else:
                with pytest.raises(HipExtensionError):
                    check()
        if edge_ok:
            assert ops._per_scan(v, "cell", S, "cpu").tolist() == [float(v32)] * S


def test_buffer_functions_follow_the_same_tables():
    from hyperpocket_amd import ops
    out, ws = ops.scan_plane_buffers(S, 6, TRIALS, "cpu")
    assert {n: (t.dtype, tuple(t.shape)) for n, t in out.items()} == {n: (dt, sh(SIZES)) for n, dt, sh in PLANE_OUT}
    assert ws.dtype == I64 and ws.numel() * 8 == ops._long_fn("hp_scan_plane_workspace_bytes", S, TRIALS)
    bufs = ops.scan_voxels_buffers(S, 6, "cpu", slots_per_row=4)
    assert list(bufs) == [n for n, _, _ in VOXEL_OUT] + ["ws"]
    assert {n: (bufs[n].dtype, tuple(bufs[n].shape)) for n, _, _ in VOXEL_OUT} == {n: (dt, sh(SIZES)) for n, dt, sh in VOXEL_OUT}
    assert bufs["ws"].dtype == I64 and bufs["ws"].numel() * 8 == ops._long_fn("hp_scan_voxels_workspace_bytes",
                                                                              ctypes.c_longlong(6), 4)
    for bufs, case, d in ((ops.mesh_sample_buffers(2, 2, 3, "cpu"), BY_NAME["mesh_sample"], SIZES),
                          (ops.farthest_points_buffers(2, K, "cpu"), BY_NAME["farthest_points"], SIZES),
                          (ops.axis_split_buffers(2, 5, K, "cpu"), BY_NAME["axis_split"], SIZES),
                          (ops.prepare_scans_buffers(3, 4, "cpu"), BY_NAME["prepare_scans"], SIZES)):
        got = {n: (t.dtype, tuple(t.shape)) for n, t in bufs.items() if n != "ws"}
        assert got == {n: (dt, sh(d)) for n, dt, sh in case.members}, case.name
    assert ops.mesh_sample_buffers(2, 2, 3, "cpu")["ws"] is None   # up to 8192 faces the table of a mesh lives in LDS
    assert ops.scan_voxels_buffers(S, 0, "cpu")["ws"].dtype == I64 and ops.scan_plane_buffers(S, 0, TRIALS, "cpu")[1].dtype == I64
    ws = ops.knn_grid_buffers(S, 6, "cpu", Q=3)
    assert ws.dtype == I64 and ws.numel() * 8 >= grid_bytes(ops, SIZES, 3)


def test_mesh_sample_wants_its_workspace_above_the_lds_table():
    from hyperpocket_amd import HipExtensionError, ops
    faces = torch.tensor([[0, 1, 2]], dtype=I32).repeat(8200, 1)
    vertices = rows(4).reshape(1, 4, 3)
    with recording() as calls:
        bufs = ops.mesh_sample_buffers(1, 8200, 2, "cpu")
        need = ops._mesh_sample_workspace_bytes(1, 8200, 2)
        assert need > 0 and bufs["ws"].dtype == I64 and bufs["ws"].numel() * 8 == need
        ops.mesh_sample(vertices, faces, 2, out=bufs)
        assert calls[-1][0] == "hp_mesh_sample" and calls[-1][13] is bufs["ws"]
        del calls[:]
        roomy = torch.empty(bufs["ws"].numel() + 2, dtype=I64)
        for bad in (bufs["ws"][:-1], None, roomy[1:], torch.empty(bufs["ws"].shape, dtype=I64, device="meta")):
            with pytest.raises(HipExtensionError) as e:        # too small, left out, off a 16-byte boundary, another device
                ops.mesh_sample(vertices, faces, 2, out=dict(bufs, ws=bad))
            assert f"must hold {need} bytes" in str(e.value) and calls == []
        with pytest.raises(HipExtensionError):                 # the members are looked at before the workspace
            ops.mesh_sample(vertices, faces, 2, out=dict(bufs, ws=None, face=bufs["face"].long()))
        ops.mesh_sample(vertices, faces, 2)                    # without out the wrapper brings its own
        assert calls[-1][13].dtype == I64 and calls[-1][13].numel() * 8 == need


if __name__ == "__main__":
    with open(RECORD, "w") as f:
        json.dump(record_all(), f, indent=1)
        f.write("\n")
    print("wrote", RECORD)

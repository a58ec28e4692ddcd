"""CPU suite: the several hand-written statements of the C ABI against include/hyperpocket_hip.h as the compiler reads it
(tests/capi_law.py).  a. every struct of the header against its restatement in csrc and every ctypes mirror; b. every
extern "C" definition in csrc compiled behind the header's prototypes, with planted mismatches to show that the compiler
does refuse one; c. the recorded argument lists of tests/golden/ops_wrapper_calls.json against the declared parameter
classes; d. the rule itself, row by row.  Needs the built library at most, never a GPU."""
import concurrent.futures
import ctypes
import glob
import importlib
import inspect
import json
import os
import re
import subprocess
import types

import pytest

import capi_law
from conftest import GOLDEN, PKG_DIR, ROOT

PUBLIC = ('#include "hyperpocket_hip.h"',)
# where csrc states the structs again: the two headers that say "mirrored in include/hyperpocket_hip.h", and render.hip
CSRC_STATEMENTS = {
    ('#include "hp_common.h"', '#include "hp_model.h"', '#include "hp_gemm.h"'):
        ("HpGemmDesc", "HpEncoderWeights", "HpEncoderGrads", "HpHyperWeights", "HpHyperGrads", "HpEncoderIO", "HpEncoderBwdIO",
         "HpEncoderPlan", "HpHeadsPlan"),
    ('#include "render.hip"',): ("HpRenderPlan",),
}
# C name -> every ctypes.Structure that mirrors it, as (module, class); package modules first
MIRRORS = {
    "HpGemmDesc": [("hyperpocket_amd.ops", "_GemmDesc")],
    "HpEncoderWeights": [("hyperpocket_amd.ops", "_EncoderPtrs")],
    "HpEncoderGrads": [("hyperpocket_amd.ops", "_EncoderPtrs")],
    "HpHyperWeights": [("hyperpocket_amd.ops", "_HyperWeights"), ("heads_law", "HyperWeights")],
    "HpHyperGrads": [("hyperpocket_amd.ops", "_HyperGrads"), ("heads_law", "HyperGrads")],
    "HpEncoderIO": [("hyperpocket_amd.ops", "_EncoderIO")],
    "HpEncoderBwdIO": [("hyperpocket_amd.ops", "_EncoderBwdIO")],
    "HpEncoderPlan": [("hyperpocket_amd.ops", "_EncoderPlan")],
    "HpHeadsPlan": [("heads_law", "HeadsPlan")],
    "HpRenderPlan": [("hyperpocket_amd.ops", "RenderPlan"), ("test_render_host", "Plan")],
}
NO_MIRROR_IN_THE_PACKAGE = {"HpHeadsPlan"}


# ======================================================================================================= a. struct mirrors
@pytest.fixture(scope="module")
def public_layouts():
    layouts = capi_law.struct_layouts(PUBLIC)
    assert set(layouts) == set(capi_law.STRUCTS)
    return layouts


def test_the_header_has_these_ten_structs_and_no_other():
    text = capi_law._strip_comments(open(capi_law.HEADER).read())
    assert sorted(re.findall(r"typedef\s+struct\s+(\w+)\s*\{", text)) == sorted(capi_law.STRUCTS)
    assert set(MIRRORS) == set(capi_law.STRUCTS)


@pytest.mark.parametrize("lines", list(CSRC_STATEMENTS), ids=["hp_model.h+hp_gemm.h", "render.hip"])
def test_csrc_states_each_struct_as_the_header_does(public_layouts, lines):
    private = capi_law.struct_layouts(lines)
    assert set(private) == set(CSRC_STATEMENTS[lines])
    for name, layout in private.items():
        assert layout == public_layouts[name], name


def test_every_struct_is_restated_in_csrc_exactly_where_the_table_says():
    stated = [s for structs in CSRC_STATEMENTS.values() for s in structs]
    assert sorted(stated) == sorted(capi_law.STRUCTS)
    elsewhere = []
    for path in glob.glob(os.path.join(capi_law.CSRC, "*")):
        text = capi_law._strip_comments(open(path).read())
        for s in capi_law.STRUCTS:
            if re.search(r"\bstruct\s+%s\s*\{" % s, text):
                elsewhere.append((os.path.basename(path), s))
    expected = [(re.search(r'"(.+)"', line).group(1), s) for lines, structs in CSRC_STATEMENTS.items() for line in lines
                for s in structs if capi_law.struct_fields(capi_law._included_text((line,)), s) is not None]
    assert sorted(elsewhere) == sorted(expected)


@pytest.mark.parametrize("struct", capi_law.STRUCTS)
def test_every_ctypes_mirror_is_the_header_struct(public_layouts, struct):
    assert MIRRORS[struct], struct
    for module, cls in MIRRORS[struct]:
        mirror = getattr(importlib.import_module(module), cls)
        assert capi_law.ctypes_layout(mirror) == public_layouts[struct], (struct, module, cls)
    in_package = [m for m, _ in MIRRORS[struct] if m.startswith("hyperpocket_amd")]
    assert (not in_package) == (struct in NO_MIRROR_IN_THE_PACKAGE), struct


def _package_modules():
    top = os.path.join(PKG_DIR, "hyperpocket_amd")
    for path in sorted(glob.glob(os.path.join(top, "**", "*.py"), recursive=True)):
        name = os.path.relpath(path, PKG_DIR)[:-3].replace(os.sep, ".")
        yield importlib.import_module(name[:-len(".__init__")] if name.endswith(".__init__") else name)


def test_no_structure_of_the_package_is_outside_the_table():
    listed = {(m, c) for rows in MIRRORS.values() for m, c in rows}
    found = set()
    for mod in _package_modules():
        for name, obj in vars(mod).items():
            if inspect.isclass(obj) and issubclass(obj, (ctypes.Structure, ctypes.Union)) and obj.__module__ == mod.__name__:
                found.add((mod.__name__, name))
    assert found == {row for row in listed if row[0].startswith("hyperpocket_amd")}
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):      # the suite's own mirrors: by text, nothing is imported
        module = os.path.basename(path)[:-3]
        for cls in re.findall(r"^class\s+(\w+)\(ctypes\.(?:Structure|Union)\)", open(path).read(), flags=re.M):
            assert (module, cls) in listed, (module, cls)


# ================================================================================= b. definitions against declarations
def prototypes_only(header_text):
    """The header with each struct body and every value macro and enum taken out: what is left declares the types' names and the
    entry points, and can stand in front of the csrc text that states the bodies itself."""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{.*?\}\s*\1\s*;", r"typedef struct \1 \1;", header_text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*define[ \t]+HP_\w+[ \t]+\S.*$", "", text, flags=re.M)
    text = re.sub(r"\benum\s*\w*\s*\{.*?\}\s*;", "", text, flags=re.S)
    return text


def syntax_pass(header_copies):
    """{copy: {file: (return code, stderr)}} of a host-only syntax pass of every csrc/*.hip behind each of `header_copies`
    ({name: path}); one pool for all of it, so that no more than JOBS compilers run at a time."""
    files = sorted(glob.glob(os.path.join(capi_law.CSRC, "*.hip")))

    def one(job):
        copy, path = job
        cmd = [capi_law.HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", "-std=c++17", "-I", capi_law.CSRC,
               "-include", header_copies[copy], path]
        done = subprocess.run(cmd, capture_output=True, text=True)
        return copy, os.path.basename(path), (done.returncode, done.stderr)

    results = {copy: {} for copy in header_copies}
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(capi_law.JOBS, os.cpu_count() or 1)) as pool:
        for copy, name, outcome in pool.map(one, [(c, f) for c in header_copies for f in files]):
            results[copy][name] = outcome
    return results


def narrowed(text, entry, old, new):
    """`text` with the first `old` in the declaration of `entry` (return type included) rewritten to `new`."""
    m = re.search(r"(?:^|(?<=[;/\n]))[^;{}#]*?\b%s\s*\([^;]*;" % entry, text, flags=re.S)
    assert m is not None, entry
    decl = m.group(0)
    assert re.search(r"\b%s\b" % old, decl), (entry, decl)
    return text[:m.start()] + re.sub(r"\b%s\b" % old, new, decl, count=1) + text[m.end():]


# model.hip and emd.hip declare no 8-byte parameter: what is wide in their entry points is the `long` a size query returns,
# and a C-linkage definition that returns another type than its declaration is refused like one that takes another.  The
# 8-byte parameter is planted in visibility.hip.
PLANTED = {"model.hip": ("hp_encoder_forward_workspace_floats", "long", "int"),
           "emd.hip": ("hp_emd_partials_floats", "long", "int"),
           "visibility.hip": ("hp_scan_visibility", "long long", "int")}


@pytest.fixture(scope="module")
def passes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("capi_header")
    clean = prototypes_only(open(capi_law.HEADER).read())
    assert "typedef struct HpGemmDesc HpGemmDesc;" in clean and "workgroups;" not in clean and "#define HP_" not in clean
    planted = clean
    for entry, old, new in PLANTED.values():
        planted = narrowed(planted, entry, old, new)
    assert planted != clean
    (tmp / "clean.h").write_text(clean)
    (tmp / "planted.h").write_text(planted)
    results = syntax_pass({"clean": str(tmp / "clean.h"), "planted": str(tmp / "planted.h")})
    return results["clean"], results["planted"]


def test_every_definition_compiles_against_the_headers_declaration(passes):
    clean, _ = passes
    assert len(clean) == len(glob.glob(os.path.join(capi_law.CSRC, "*.hip"))) >= 38
    failed = {f: err[-2000:] for f, (rc, err) in clean.items() if rc != 0}
    assert not failed, failed


def test_every_entry_point_is_defined_with_c_linkage_in_csrc():
    """The pass above proves nothing about a name that no file defines as extern "C"."""
    defined = set()
    for path in glob.glob(os.path.join(capi_law.CSRC, "*.hip")):
        defined |= set(re.findall(r"\bHP_API\b[^;{(]*?\b(hp_\w+)\s*\(", capi_law._strip_comments(open(path).read())))
    assert set(capi_law.declared()) <= defined, sorted(set(capi_law.declared()) - defined)


def test_a_planted_mismatch_is_refused_by_name(passes):
    _, planted = passes
    failed = {f for f, (rc, _) in planted.items() if rc != 0}
    assert failed == set(PLANTED)
    for f, (entry, _, _) in PLANTED.items():
        assert entry in planted[f][1], (f, planted[f][1][-2000:])


# ============================================================================================ c. the recorded argument lists
def from_record(described):
    """The object ctypes is handed for one described argument of the record (after _lib.call's conversion)."""
    if described in ("null", "stream") or described == "ws" or described.split(":")[0] in ("in", "out", "new"):
        return ctypes.c_void_p(4096) if described != "null" else None      # call() makes c_void_p of a tensor and of None
    kind, _, value = described.partition(":")
    if kind == "int":
        v = int(value)
        return ctypes.c_longlong(v) if abs(v) > 0x7FFFFFFF else ctypes.c_int(v)
    if kind == "bool":
        return ctypes.c_int(value == "True")
    if kind == "float":
        return ctypes.c_float(float(value))
    if kind.startswith("c_") and isinstance(getattr(ctypes, kind, None), type):       # stands as it is
        return getattr(ctypes, kind)(float(value) if kind in ("c_double", "c_float") else int(value))
    raise AssertionError(f"the record holds {described!r}: no rule for it")


def recorded_calls():
    with open(os.path.join(GOLDEN, "ops_wrapper_calls.json")) as f:
        record = json.load(f)
    return [(case, run, entry, args) for case, runs in sorted(record.items()) for run in ("given", "fresh")
            for entry, args in runs[run]]


def test_the_recorded_argument_lists_keep_the_declared_classes():
    table = capi_law.prototypes()
    bad = []
    for case, run, entry, args in recorded_calls():
        # the record is of _lib.call, which reads an int return
        bad += [f"{case}/{run}: {v}" for v in capi_law.check_call(entry, [from_record(a) for a in args], ctypes.c_int, table)]
    assert not bad, "\n".join(bad)


def test_the_record_reaches_the_newest_wrappers():
    entries = {entry for _, _, entry, _ in recorded_calls()}
    for entry in ("hp_scan_visibility", "hp_depth_points", "hp_fuse_volume", "hp_fuse_surface", "hp_make_view_batch",
                  "hp_restore_scans", "hp_knn_grid"):
        assert entry in entries, entry


# ======================================================================================================== d. the rule
I8 = [ctypes.c_longlong(5), ctypes.c_ulonglong(5), ctypes.c_long(5), ctypes.c_ulong(5), ctypes.c_int64(5), ctypes.c_size_t(5)]
POINTERS = [ctypes.c_void_p(0), ctypes.c_void_p(4096), None, ctypes.pointer(ctypes.c_int(1)), (ctypes.c_int * 4)(),
            ctypes.byref(ctypes.c_int(1)), ctypes.cast(ctypes.pointer(ctypes.c_int(1)), ctypes.POINTER(ctypes.c_float))]
NARROW = [ctypes.c_int(5), ctypes.c_uint(5), ctypes.c_bool(True), 5, 0, -2 ** 31, 2 ** 31 - 1, True]
FLOATS = [ctypes.c_float(0.5), ctypes.c_double(0.5), 0.5]


def test_the_rule_row_by_row():
    ok = capi_law.compatible
    assert ctypes.sizeof(ctypes.c_long) == 8                     # LP64: `long` of the header is an 8-byte integer
    for a in NARROW:                                             # i32: c_int, c_uint, c_bool, a bare int within int32
        assert ok("i32", a), a
    for a in I8 + POINTERS + FLOATS + [2 ** 31, -2 ** 31 - 1, ctypes.c_short(1), ctypes.c_char(b"a")]:
        assert not ok("i32", a), a
    for a in I8:                                                 # i64: an 8-byte ctypes integer only
        assert ok("i64", a), a
    for a in NARROW + POINTERS + FLOATS + [2 ** 40, ctypes.c_int32(5), ctypes.c_uint32(5), ctypes.c_short(1)]:
        assert not ok("i64", a), a
    assert ok("f32", ctypes.c_float(0.5))                        # f32: c_float only
    for a in [ctypes.c_double(0.5), 0.5] + NARROW + I8 + POINTERS:
        assert not ok("f32", a), a
    assert ok("f64", ctypes.c_double(0.5))                       # f64: c_double only
    for a in [ctypes.c_float(0.5), 0.5] + NARROW + I8 + POINTERS:
        assert not ok("f64", a), a
    for a in POINTERS + I8:                                      # ptr: c_void_p, None, pointer, array, byref, 8-byte integer
        assert ok("ptr", a), a
    for a in NARROW + FLOATS:                                    # ... never a bare int (0 included) or c_int
        assert not ok("ptr", a), a
    with pytest.raises(ValueError):
        ok("i16", 1)


def test_the_rule_for_returns():
    ok = capi_law.returns_ok
    default = ctypes.CDLL(None).getpid.restype                   # what a fresh function object holds
    assert default is ctypes.c_int
    assert ok("i32", default) and ok("i32", ctypes.c_int) and not ok("i32", ctypes.c_long) and not ok("i32", None)
    for restype in (ctypes.c_long, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int64):
        assert ok("i64", restype), restype
    for restype in (default, ctypes.c_int, ctypes.c_uint, ctypes.c_double, ctypes.c_void_p, None):
        assert not ok("i64", restype), restype
    assert ok("f64", ctypes.c_double) and not ok("f64", ctypes.c_float) and not ok("f64", default)
    assert ok("f32", ctypes.c_float) and not ok("f32", ctypes.c_double)
    assert ok("ptr", ctypes.c_void_p) and ok("ptr", ctypes.POINTER(ctypes.c_int)) and not ok("ptr", default)
    assert ok("void", None) and ok("void", default)


def test_a_call_is_held_to_count_classes_and_return():
    table = {"hp_x": ("i64", ("i32", "i64", "f64", "ptr"))}
    good = [3, ctypes.c_longlong(4), ctypes.c_double(0.5), None]
    assert capi_law.check_call("hp_x", good, ctypes.c_long, table) == []
    assert len(capi_law.check_call("hp_x", good, ctypes.c_int, table)) == 1                  # the return is cut in half
    assert len(capi_law.check_call("hp_x", good[:3], ctypes.c_long, table)) == 1             # an argument short
    assert len(capi_law.check_call("hp_x", good + [None], ctypes.c_long, table)) == 1        # one too many
    bad = capi_law.check_call("hp_x", [3, 4, ctypes.c_float(0.5), 0], ctypes.c_long, table)
    assert len(bad) == 3 and "argument 1 is declared i64 and gets int(4)" in bad[0] and "c_float" in bad[1], bad
    assert capi_law.check_call("hp_y", [], ctypes.c_int, table) == ["hp_y: not declared in the header"]


# ========================================================================================================= the proxy
class _FakeFunction:
    """Stands for a ctypes function object: a restype, and a record of what it was called with."""

    def __init__(self):
        self.restype, self.got = ctypes.c_int, []

    def __call__(self, *args):
        self.got.append(args)
        return 7


def test_the_checking_library_checks_records_and_forwards():
    fake = types.SimpleNamespace(hp_knn_grid_workspace_bytes=_FakeFunction(), other=object())
    log = capi_law.CallLog()
    lib = capi_law._CheckedLibrary(fake, log)
    assert lib.other is fake.other                                               # only hp_* names are wrapped
    wide = ctypes.c_longlong(6)
    assert lib.hp_knn_grid_workspace_bytes(2, wide, 0) == 7                      # a bare int for a long long, restype c_int
    assert fake.hp_knn_grid_workspace_bytes.got[0][1] is wide                    # the very object
    assert len(log.violations) == 2 and "argument 2 is declared i64 and gets int(0)" in log.violations[0] \
        and "restype c_int" in log.violations[1], log.violations
    lib.hp_knn_grid_workspace_bytes.restype = ctypes.c_longlong                  # reaches the real function object
    assert fake.hp_knn_grid_workspace_bytes.restype is ctypes.c_longlong
    assert lib.hp_knn_grid_workspace_bytes.restype is ctypes.c_longlong
    lib.hp_knn_grid_workspace_bytes(2, wide, ctypes.c_longlong(0))
    assert len(log.violations) == 2
    assert log.calls == [("hp_knn_grid_workspace_bytes", ("int(2)", "c_long", "int(0)")),
                         ("hp_knn_grid_workspace_bytes", ("int(2)", "c_long", "c_long"))]


@pytest.fixture(scope="module")
def built_library():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)


def test_checked_library_installs_a_fresh_library_and_restores_the_old_one(built_library):
    from hyperpocket_amd import _lib
    before = _lib.load_library()
    before.hp_emd_partials_floats.restype = ctypes.c_long
    kept = dict(_lib._FN)
    with capi_law.checked_library() as log:
        inside = _lib.load_library()
        assert isinstance(inside, capi_law._CheckedLibrary) and inside._real is not before
        assert _lib._FN == {}
        assert inside.hp_hypernet_t5_offset.restype is ctypes.c_int              # fresh function objects: the default
        assert inside.hp_emd_partials_floats.restype is ctypes.c_long            # load_library's own five
        assert inside.hp_nn_queries_per_lane(1, 64, 64) in (1, 2, 4)
    assert log.names() == {"hp_nn_queries_per_lane"} and log.violations == []
    assert _lib.load_library() is before and _lib._FN == kept


# ======================================================================================= the compiler's reading, spot-checked
def test_prototypes_reads_the_header_as_the_compiler_does():
    table = capi_law.prototypes()
    assert sorted(table) == capi_law.declared() and len(table) >= 160
    assert table["hp_nndistance"] == ("i32", ("i32", "i32", "ptr", "i32", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"))
    assert table["hp_approxmatch_workspace_floats"] == ("i64", ("i32", "i32", "i32"))
    assert table["hp_sample_points"] == ("i32", ("i64", "f32", "i64", "i64", "ptr", "ptr"))
    assert table["hp_scan_visibility"][1][7:10] == ("f64", "f64", "i64") and len(table["hp_scan_visibility"][1]) == 17
    assert table["hp_hypernet_heads_dw_workspace_floats"] == ("i64", ())
    assert table["hp_gemm_pp_plan"][1][-1] == "ptr"               # `int out[6]` is a pointer

"""CPU suite for the general fp32 GEMM's host side: hp_gemm_plan, the query that tells which tile and which staging-loader
instance hp_gemm_f32 launches for a descriptor.  It proves from the case tables of tests/test_gemm_paths_gpu.py alone that
the GPU suite reaches every tile x loader instance and the listed paths, and that the query refuses what the launcher
refuses.  Nothing here reaches a GPU: the cases' operands are laid out in host memory (the query reads strides and the
alignment of the base pointers, never the data)."""
import ctypes
import importlib.util
import os
from ctypes import c_int, POINTER

import pytest

from conftest import PKG_DIR

import test_gemm_paths_gpu as gpu_suite

MODES = {0, 1, 2, 3, 4, 7, 8}
ALL_PAIRS = {(t, m) for t in range(4) for m in MODES}


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = ctypes.CDLL(mod.build(verbose=False))
    from hyperpocket_amd.ops import _GemmDesc
    so.hp_gemm_plan.restype = c_int
    so.hp_gemm_plan.argtypes = [POINTER(_GemmDesc), POINTER(c_int), POINTER(c_int)]
    so.hp_gemm_tile_rows.restype = c_int
    so.hp_gemm_tile_rows.argtypes = [POINTER(_GemmDesc)]
    return so


def plan_of(c):
    from hyperpocket_amd import ops
    x = gpu_suite.make(c, "cpu")
    return ops.gemm_plan(x.A.view(), x.B.view(), **x.kw)


def pairs(table):
    return {(c["tile"], c["mode"]) for c in table}


@pytest.mark.parametrize("name", sorted(gpu_suite.GEMM_TABLES))
def test_every_case_runs_the_instance_its_table_records(lib, name):
    for c in gpu_suite.GEMM_TABLES[name]:
        assert plan_of(c) == (c["tile"], c["mode"]), gpu_suite.case_id(c)


def test_the_tables_reach_every_tile_and_loader_instance(lib):
    assert pairs(gpu_suite.LOADER_CASES) == ALL_PAIRS                 # the loader table alone: all 28 kernels
    loaders = {(c["tile"], c["am"], c["bm"]) for c in gpu_suite.LOADER_CASES}
    assert loaders >= {(t, am, bm) for t in range(4) for am in range(3) for bm in range(3)}
    for c in gpu_suite.LOADER_CASES:                                   # what the table calls a loader pair is what launches
        if c["M"] > 1 and c["K"] > 1:
            assert c["mode"] == gpu_suite.MODE_OF[c["am"], c["bm"]]
    # loader 1 with a K tail (K = 37 on row stride 40) on the tiles that have tail loaders
    assert {c["tile"] for c in gpu_suite.LOADER_CASES if c["am"] == 1 and c["K"] % 4} >= {0, 2}
    assert any(c["K"] == 0 for c in gpu_suite.LOADER_CASES)
    tiles = lambda table, pick=lambda c: True: {c["tile"] for c in table if pick(c)}
    assert tiles(gpu_suite.EPILOGUE_CASES) == {0, 1, 2, 3}
    for flag in ("bias", "relu", "mask", "add"):
        assert tiles(gpu_suite.EPILOGUE_CASES, lambda c: c[flag]) == {0, 1, 2, 3}, flag
    assert tiles(gpu_suite.EPILOGUE_CASES, lambda c: len({0, *c["pads"]}) == 4) == {0, 1, 2, 3}
    assert tiles(gpu_suite.ROWSUM_CASES) == {0, 1, 2, 3} and all(c["ksplit"] == 1 for c in gpu_suite.ROWSUM_CASES)
    assert tiles(gpu_suite.SPLITK_CASES) == {0, 1, 2, 3} and tiles(gpu_suite.SPLITK_CASES, lambda c: c["rowsum"]) == {0, 1, 2, 3}
    assert len(tiles(gpu_suite.COLMAX_CASES)) >= 3
    assert tiles(gpu_suite.DYN_CASES, lambda c: c["dyn"][0] == "rows") == {1, 3}
    assert tiles(gpu_suite.DYN_CASES, lambda c: c["dyn"][0] == "k" and c["ksplit"] > 1 and c["rowsum"]) == {2}
    assert tiles(gpu_suite.REAL_CASES, lambda c: c["ksplit"] == 1) == tiles(gpu_suite.REAL_CASES, lambda c: c["ksplit"] > 1) == {0, 1, 2, 3}


def test_splitk_cases_reach_both_reduce_paths_and_every_slab_loop(lib):
    """splitk_reduce_kernel takes its float4 path for a dense C without addend or mask, M N % 4 == 0 and at most 8 slabs;
    slab_sum adds 16, then 4, then single slabs.  Split ranges are multiples of 32 deep."""
    f4, scalar, loops, empty = set(), set(), set(), False
    for c in gpu_suite.SPLITK_CASES:
        fast = not (c["add"] or c["mask"] or c["pads"][0]) and (c["M"] * c["N"]) % 4 == 0 and c["ksplit"] <= 8
        (f4 if fast else scalar).add(c["tile"])
        if not fast:
            ks = c["ksplit"]
            loops |= {n for n, hit in ((16, ks >= 16), (4, ks % 16 >= 4), (1, ks % 4 > 0)) if hit}
        chunk = -(-(-(-c["K"] // c["ksplit"])) // 32) * 32
        empty |= chunk * (c["ksplit"] - 1) >= c["K"]
    assert f4 >= {0, 1} and scalar >= {1, 2, 3} and loops == {16, 4, 1} and empty


def _desc(M=100, N=130, K=70, batch=2, ksplit=1, flags=0):
    """A descriptor hp_gemm_f32 accepts: dense row-major A (M, K) and B (N, K), dummy pointers (non-null, 16-byte aligned)."""
    from hyperpocket_amd.ops import _GemmDesc
    d = _GemmDesc()
    d.A, d.B, d.C, d.ws = 4096, 8192, 12288, 16384
    d.sAz, d.sBz, d.sCz = M * K, N * K, M * N
    d.sAi, d.sAk, d.sBk, d.sBj = K, 1, 1, K
    d.ldc, d.M, d.N, d.K, d.batch, d.ksplit, d.flags = N, M, N, K, batch, ksplit, flags
    return d


def _plan(lib, d):
    tile, mode = c_int(-9), c_int(-9)
    rc = lib.hp_gemm_plan(ctypes.byref(d), ctypes.byref(tile), ctypes.byref(mode))
    return rc, tile.value, mode.value


def test_plan_refuses_what_the_launcher_refuses(lib):
    assert _plan(lib, _desc())[0] == 0
    assert lib.hp_gemm_plan(None, None, None) == -1
    assert lib.hp_gemm_plan(ctypes.byref(_desc()), None, None) == 0    # either output may be NULL
    d = _desc()
    d.sAi, d.sAk = 70, 2                                               # both strides of A non-unit
    assert _plan(lib, d)[0] == -1
    d = _desc()
    d.sBk, d.sBj = 3, 70                                               # ... of B
    assert _plan(lib, d)[0] == -1
    d = _desc(M=128, flags=16)                                         # COLMAX ...
    d.cmax, d.cidx, d.group_rows = 4096, 8192, 64
    assert _plan(lib, d)[0] == 0
    d.ksplit = 2                                                       # ... with split-K
    assert _plan(lib, d)[0] == -1
    d.ksplit, d.group_rows = 1, 48                                     # ... with groups that are no whole tiles
    assert _plan(lib, d)[0] == -1
    assert _plan(lib, _desc(batch=65535))[0] == 0
    assert _plan(lib, _desc(batch=65536))[0] == -1                     # batch * ksplit > 65535
    assert _plan(lib, _desc(batch=6554, ksplit=10))[0] == -1
    d = _desc(ksplit=4)
    d.dyn_count, d.dyn_kind = 4096, 2
    assert _plan(lib, d)[0] == 0
    d.dyn_kind = 1                                                     # a device-side row count with split-K
    assert _plan(lib, d)[0] == -1
    d = _desc(ksplit=4)
    d.ws = None                                                        # split-K without a workspace
    assert _plan(lib, d)[0] == -1
    d = _desc(flags=1)                                                 # BIAS without a bias
    assert _plan(lib, d)[0] == -1
    assert _plan(lib, _desc(M=0)) == (0, -1, -1)                       # nothing to do: nothing is launched


def test_tile_rows_agrees_with_the_plan(lib):
    """Over a grid of sizes around the thresholds: the plan's tile follows choose_cfg's rule (csrc/gemm.hip) restated here —
    128x32 for N <= 32; 128x128 for whole 16-deep k-tiles, more than 64 rows and columns and >= 384 workgroups; 64x128 for
    more than 64 columns and >= 512 workgroups; else 64x64 — hp_gemm_tile_rows answers that tile's rows, and the mode is the
    16-byte loader exactly where every row of every batch starts 16-byte aligned."""
    rows = gpu_suite.TILE_ROWS
    seen = set()
    for M, N, K, batch, ksplit in [(130, 19, 37, 3, 1), (130, 130, 48, 96, 1), (130, 130, 48, 95, 1), (100, 200, 37, 128, 1),
                                   (100, 200, 37, 127, 1), (100, 130, 70, 2, 1), (130, 132, 256, 12, 8), (64, 130, 48, 4000, 1),
                                   (65, 130, 48, 96, 1), (130, 130, 40, 96, 1), (70, 130, 200, 32, 16), (1, 1, 1, 1, 1),
                                   (130, 64, 48, 4000, 1), (130, 65, 48, 4000, 1), (4000, 32, 48, 96, 1), (4000, 33, 8, 96, 1)]:
        d = _desc(M, N, K, batch, ksplit)
        wgs = lambda bm, bn: -(-M // bm) * -(-N // bn) * batch * ksplit
        want = (0 if N <= 32 else 1 if K >= 16 and K % 16 == 0 and M > 64 and N > 64 and wgs(128, 128) >= 384
                else 2 if N > 64 and wgs(64, 128) >= 512 else 3)
        loader = lambda r: 1 if K % 4 == 0 and (r * K) % 4 == 0 else 2
        assert _plan(lib, d) == (0, want, gpu_suite.MODE_OF[loader(M), loader(N)]), (M, N, K, batch, ksplit)
        assert lib.hp_gemm_tile_rows(ctypes.byref(d)) == rows[want], (M, N, K, batch, ksplit)
        seen.add(want)
    assert seen == {0, 1, 2, 3}
    for c in gpu_suite.COLMAX_CASES:                                   # the COLMAX partial layout follows the recorded tile
        assert c["colmax"] % rows[c["tile"]] == 0 and c["M"] % c["colmax"] == 0

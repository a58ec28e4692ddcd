"""CPU suite behind tests/test_split_gemm_gpu.py.  From that file's case tables, tests/split_gemm_law.py and the host query
hp_gemm_pp_plan alone (nothing here reaches a GPU) it proves
  * that each case runs the plan its table records, and that the tables together reach every kernel instance, tiles_n in
    {1, 2, 4, 8}, grids of 1, 2, 4, multiples of 8 below the cap and the cap, walks with and without a remainder, a single
    tile and every listed M % 256;
  * that the kernel's XCD remap is a bijection for every grid size and that a workgroup keeps its column tile along its walk;
  * the preconditions under which the kernels must be exact, for every case: the restated three-product sum equals the plain
    product, lo pieces occur in both operands in every k-block and never at the same k, every partial sum stays below 2^24,
    mode 0's outputs are piece pairs under their block's exponent, exponents differ between neighbouring blocks;
  * that the cases would notice: each mutation of the law (a dropped hi lo or lo hi product, no rescale along k, the last
    row of a tie, a clamped row >= M that wins, a walk that skips its last tile) changes the result of at least one case;
  * the constant of the real-valued pass: the law's fp32 simulation against the rounding bound."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from conftest import PKG_DIR

import split_gemm_law as law
import test_split_gemm_gpu as gpu_suite

INSTANCES = {(0, 128, 256), (0, 256, 512), (1, 128, 512), (1, 256, 512)}          # (mode, bn, threads): <0,1,1> <0,2,2> <1,1,2> <1,2,2>


@pytest.fixture(scope="module")
def lib():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = ctypes.CDLL(mod.build(verbose=False))
    so.hp_gemm_pp_plan.restype = ctypes.c_int
    so.hp_gemm_pp_plan.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return so


def lib_plan(lib, M, N, mode, n=1):
    out = (ctypes.c_int * 6)(*([-9] * 6))
    rc = lib.hp_gemm_pp_plan(M, N, mode, n, out)
    return tuple(out) if rc == 0 else None


_OPS = {}


def ops_of(c):
    key = gpu_suite.case_id(c)
    if key not in _OPS:
        _OPS.clear()                                   # one case at a time: the largest operands are hundreds of MB
        _OPS[key] = law.operands(c)
    return _OPS[key]


# ------------------------------------------------------------------------------------------------------------- the plan
def test_every_case_runs_the_plan_its_table_records(lib):
    for c in gpu_suite.EXACT_PP_CASES:
        assert lib_plan(lib, c["M"], c["N"], c["mode"]) == c["plan"] == law.plan(c["M"], c["N"], c["mode"]), gpu_suite.case_id(c)


def test_plan_query_follows_the_law_and_refuses_what_the_launch_refuses(lib):
    for mode in (0, 1):
        for n in (1, 2, 3):
            for N in (128, 256, 512, 1024, 2048):
                for M in (1, 127, 128, 129, 255, 256, 257, 1000, 4097, 8449, 33000, 65663, 140000, 2 ** 31 - 1):
                    got = lib_plan(lib, M, N, mode, n)
                    assert got == law.plan(M, N, mode, n), (mode, n, N, M)
                    bn, bm, tiles_n, tiles, wgs, threads = got
                    assert N == bn * tiles_n and tiles == -(-M // bm) * tiles_n and 1 <= wgs <= tiles
                    assert wgs % tiles_n == 0 and (wgs % 8 == 0 or wgs == tiles_n)
                    assert wgs <= max(256 * (512 // threads) // n, tiles_n)
    for N in (384, 640, 100, 0, -128):
        assert lib_plan(lib, 300, N, 0) is None and law.plan(300, N, 0) is None
    assert lib_plan(lib, 0, 128, 0) is None and lib_plan(lib, -5, 128, 1) is None and lib_plan(lib, 2 ** 31, 128, 1) is None
    assert lib_plan(lib, 300, 128, 2) is None and lib_plan(lib, 300, 128, -1) is None and lib_plan(lib, 300, 128, 0, 0) is None
    assert lib.hp_gemm_pp_plan(300, 128, 0, 1, None) != 0


def test_the_tables_reach_every_instance_grid_and_walk():
    walk = gpu_suite.WALK_CASES
    assert all(c["K"] == 64 for c in walk)
    assert {(c["mode"], c["plan"][0], c["plan"][5]) for c in walk} == INSTANCES
    assert {(c["mode"], c["plan"][0], c["plan"][5]) for c in gpu_suite.K_CASES} == INSTANCES
    for mode in (0, 1):
        cs = [c for c in walk if c["mode"] == mode]
        assert {c["plan"][2] for c in cs} == {1, 2, 4, 8}
        grids = {c["plan"][4] for c in cs}
        assert grids >= {1, 2, 4, 8, 16, 24, 256}, grids
        assert any(c["plan"][3] == 1 for c in cs)                                              # a single tile
        even = [c for c in cs if c["plan"][3] > c["plan"][4] and c["plan"][3] % c["plan"][4] == 0]
        ragged = [c for c in cs if c["plan"][3] > c["plan"][4] and c["plan"][3] % c["plan"][4]]
        assert even and ragged, mode         # every workgroup has a next tile to prefetch until its last / only some have
        assert any(c["plan"][4] == 256 and c["plan"][3] % 256 for c in cs)                     # ... at the cap too
        assert {c["M"] % 256 for c in cs} >= {0, 1, 127, 128, 129, 255}
        for bn in (128, 256):                                                                  # each instance: one tile, a walk, a grid
            inst = [c["plan"] for c in cs if c["plan"][0] == bn]
            assert any(p[3] == 1 for p in inst) and any(p[4] == 1 and p[3] > 1 for p in inst) and any(p[4] >= 8 and p[3] % p[4] for p in inst)
    assert any(c["plan"][4] == 512 for c in walk if c["mode"] == 0)                            # the 4-wave instance's cap
    assert {c["N"] for c in walk} == {128, 256, 512, 1024, 2048}


def test_k_cases_cover_every_admitted_block_width():
    want = {(K, xcb) for K in (64, 128, 256, 512) for xcb in range(32, K + 1, 32) if K % xcb == 0 and K // xcb <= 16}
    for mode in (0, 1):
        assert {(c["K"], c["xcb"]) for c in gpu_suite.K_CASES if c["mode"] == mode} == want
    assert (512, 32) in want                                                                   # 16 blocks along k


def test_xcd_remap_is_a_bijection_for_every_grid():
    for nwg in range(1, 521):
        assert sorted(law.xcd_remap(b, nwg) for b in range(nwg)) == list(range(nwg)), nwg


def test_a_workgroup_keeps_its_column_tile_and_the_walks_cover_every_tile_once():
    plans = {c["plan"] for c in gpu_suite.EXACT_PP_CASES}
    plans |= {law.plan(M, N, mode, n) for mode in (0, 1) for n in (1, 2) for N in (128, 256, 512, 1024, 2048)
              for M in (1, 300, 1153, 5120, 8449, 33000, 70000)}
    for pl in plans:
        _, _, tiles_n, tiles, wgs, _ = pl
        seen = []
        for wg, tl in law.walks(pl).items():
            assert all(t % tiles_n == wg % tiles_n for t in tl), pl
            seen += tl
        assert sorted(seen) == list(range(tiles)), pl


# ------------------------------------------------------------------------------------------------ operand preconditions
def check_operands(c, ops, act_cb, clamp):
    M, N, K = c["M"], c["N"], c["K"]
    X, W, b = ops["X"], ops["W"], ops["b"]
    for t in (X, W, b):
        assert np.array_equal(t, np.rint(t))                                  # integer-valued
    assert law.sum_bound(ops) < 2 ** 24, gpu_suite.case_id(c)
    ah, al, aexp = law.pack_act(X, act_cb, clamp)
    wh, wl, wexp = law.pack_rows(W)
    # the pieces carry the operands exactly
    assert np.array_equal(law.unpack(ah, al, np.repeat(np.repeat(aexp, 128, axis=0)[:M], act_cb, axis=1)), X)
    assert np.array_equal(law.unpack(wh, wl, wexp[:, None]), W)
    # lo pieces: somewhere in every 32-deep k-tile (so in every exponent block) of both operands, never at the same k
    la, lw = (al != 0).any(axis=0), (wl != 0).any(axis=0)
    assert la.reshape(-1, 32).any(axis=1).all() and lw.reshape(-1, 32).any(axis=1).all(), gpu_suite.case_id(c)
    assert not (la & lw).any(), gpu_suite.case_id(c)
    # zero blocks, zero rows, a power-of-two block maximum
    assert (np.abs(W).max(axis=1) == 0).any()
    if clamp:
        assert np.frexp(np.abs(X[:128, :act_cb]).max())[0] == 0.5
    if clamp and M > 128:
        pad = np.zeros((len(aexp) * 128, K), np.float32)
        pad[:M] = np.abs(X)
        assert (pad.reshape(len(aexp), 128, K // act_cb, act_cb).max(axis=(1, 3)) == 0).any()
    # exponents differ between neighbouring blocks: along k, from row tile to row tile, from weight row to weight row
    assert (np.diff(wexp) != 0).any()
    if aexp.shape[1] > 1:
        assert (np.diff(aexp, axis=1) != 0).any()
    if aexp.shape[0] > 2:
        assert (np.diff(aexp, axis=0) != 0).any()
    return (ah, al, aexp), (wh, wl, wexp)


@pytest.mark.parametrize("c", gpu_suite.EXACT_PP_CASES, ids=gpu_suite.case_id)
def test_exact_case_preconditions(c):
    """... and the law's walk of the launch, with the restated three-product sum and (mode 0) the store's re-split, gives the
    plain product: every tile is visited, every output is a piece pair under its block's exponent."""
    ops = ops_of(c)
    check_operands(c, ops, c["xcb"], True)
    C, cmax, cidx = law.expected(c, ops)
    got = law.simulate(c, ops, c["mode"])
    if c["mode"] == 0:
        assert np.array_equal(got, C), gpu_suite.case_id(c)
        assert np.abs(C).max() < 2 ** 24
    else:
        assert np.array_equal(got[0], cmax) and np.array_equal(got[1], cidx), gpu_suite.case_id(c)


@pytest.mark.parametrize("c", gpu_suite.F16X2_CASES, ids=gpu_suite.case_id)
def test_f16x2_case_preconditions(c):
    """conv_split_kernel: one activation exponent per 128-row tile over all of K (not clamped), the same weight split."""
    ops = ops_of(c)
    (ah, al, aexp), (wh, wl, wexp) = check_operands(c, ops, c["K"], False)
    got = law.three_product(ah, al, aexp, c["K"], wh, wl, wexp) + ops["b"].astype(np.float64)[None, :]
    want = ops["X"].astype(np.float64) @ ops["W"].astype(np.float64).T + ops["b"].astype(np.float64)[None, :]
    assert np.array_equal(got, want)
    assert {c["M"] for c in gpu_suite.F16X2_CASES} == {1, 127, 128, 129, 300}
    assert {c["N"] for c in gpu_suite.F16X2_CASES} == {128, 256, 384} and {c["K"] for c in gpu_suite.F16X2_CASES} == {32, 96, 512}


def test_exponent_patterns_of_the_k_cases():
    """Along k the exponent rises at one boundary, falls at the next and stays at a third (row tile 0), and a zero block
    sits between two non-zero ones (row tile 1), wherever there are four blocks or more."""
    for c in gpu_suite.K_CASES:
        ncb = c["K"] // c["xcb"]
        if ncb < 4 or c["mode"]:
            continue
        X = ops_of(c)["X"]
        _, _, aexp = law.pack_act(X, c["xcb"])
        d = np.diff(aexp[0])
        assert (d > 0).any() and (d < 0).any() and (d == 0).any(), gpu_suite.case_id(c)
        blkmax = np.abs(X[128:256]).reshape(128, ncb, c["xcb"]).max(axis=(0, 2))
        z = ncb // 2
        assert blkmax[z] == 0 and blkmax[z - 1] > 0 and blkmax[z + 1] > 0, gpu_suite.case_id(c)


def test_epilogue_cases_are_what_their_names_say():
    for c in gpu_suite.EPI0_CASES:
        ops = ops_of(c)
        C, _, _ = law.expected(c, ops)
        raw = ops["X"].astype(np.float64) @ ops["W"].astype(np.float64).T + ops["b"].astype(np.float64)[None, :]
        bn = law.pp_bn(c["N"])
        if c["bias"] == "zero":
            assert not ops["b"].any() and c["relu"] and (raw < 0).any()
        if c["bias"] == "neg0":
            assert c["relu"] and not C[:, :bn].any() and (C[:, bn:] > 0).any()          # ReLU empties whole output blocks
        if c["bias"] == "neg":
            assert not c["relu"] and (C < 0).all()
        if c["bias"] == "pow2":
            assert np.abs(C[128:256]).max() == 1024 and np.array_equal(C[128], ops["b"].astype(np.float64))
    assert {(c["bias"] != "zero", c["relu"]) for c in gpu_suite.EPI0_CASES} >= {(True, 0), (False, 1), (True, 1)}
    assert {c["group_rows"] for c in gpu_suite.EPI1_CASES} == {128, 256, 384, 1280}
    for c in gpu_suite.EPI1_CASES:
        M, g = c["M"], c["group_rows"]
        assert M > 3 * g or g == 1280 and g == 128 * -(-M // 128)                       # several groups per call
        ops = ops_of(c)
        _, cmax, cidx = law.expected(c, ops)
        raw = ops["X"].astype(np.float64) @ ops["W"].astype(np.float64).T + ops["b"].astype(np.float64)[None, :]
        live = np.abs(ops["W"]).max(axis=1) > 0
        assert M % 128 and M - 1 == 1188
        for row, twin in ((0, None), (255, None), (261, 333), (1188, None)):             # first row, last row, two at once, M - 1
            t = row // 128
            blk = raw[t * 128:min(M, (t + 1) * 128)][:, live]
            hits = blk == blk.max(axis=0)[None, :]
            want = np.zeros(len(blk), bool)
            want[[r - t * 128 for r in (row, twin) if r is not None]] = True
            assert (hits == want[:, None]).all(), (row, gpu_suite.case_id(c))
            assert (cidx[t][live] == row % g).all()


# ------------------------------------------------------------------------------------------------------------ mutations
def _differs(c, **mut):
    ops = ops_of(c)
    C, cmax, cidx = law.expected(c, ops)
    got = law.simulate(c, ops, c["mode"], **mut)
    if c["mode"] == 0:
        return not np.array_equal(got, C)
    return not (np.array_equal(got[0], cmax) and np.array_equal(got[1], cidx))


SMALL = [c for c in gpu_suite.EXACT_PP_CASES if c["M"] * c["N"] <= 1100 * 512]


@pytest.mark.parametrize("mut", [dict(drop="hilo"), dict(drop="lohi")], ids=lambda m: m["drop"])
def test_a_dropped_product_changes_every_case(mut):
    for c in SMALL:
        assert _differs(c, **mut), gpu_suite.case_id(c)


def test_a_skipped_rescale_changes_every_case_with_blocks_along_k():
    for c in SMALL:
        if c["K"] // c["xcb"] > 1:
            assert _differs(c, rescale=False), gpu_suite.case_id(c)


def test_the_last_row_of_a_tie_changes_every_mode_1_case():
    for c in SMALL:
        if c["mode"] == 1:
            assert _differs(c, tie="last"), gpu_suite.case_id(c)


def test_a_clamped_row_that_wins_changes_the_ragged_mode_1_cases():
    hit = [c for c in SMALL if c["mode"] == 1 and c["M"] % 128 and _differs(c, clamped_wins=True)]
    assert {gpu_suite.case_id(c) for c in hit} >= {gpu_suite.case_id(c) for c in gpu_suite.EPI1_CASES}


def test_a_walk_that_skips_its_last_tile_changes_every_case_with_a_walk():
    for c in SMALL:
        if c["plan"][3] > c["plan"][4]:
            assert _differs(c, skip_last=True), gpu_suite.case_id(c)
    assert sum(c["plan"][3] > c["plan"][4] for c in SMALL) >= 10


# ------------------------------------------------------------------------------------------------------ real-valued pass
def test_the_laws_fp32_simulation_reaches_the_share_of_the_bound_each_real_case_records():
    for c in gpu_suite.REAL_CASES:
        ops = law.real_operands(c)
        want = ops["X"].astype(np.float64) @ ops["W"].astype(np.float64).T + ops["b"].astype(np.float64)[None, :]
        want = np.maximum(want, 0.0) if c["relu"] else want
        ratio = (np.abs(law.simulate_f32(c, ops).astype(np.float64) - want) / law.real_bound(c, ops, want)).max()
        print(f"{gpu_suite.case_id(c)}: law error / bound = {ratio:.4f}")
        assert 0.8 * c["law_ratio"] <= ratio <= c["law_ratio"], gpu_suite.case_id(c)
        rows = np.abs(ops["X"]).max(axis=1)
        assert rows.max() / rows.min() > np.exp(4) and c["xcb"] <= c["K"] // 2
    assert gpu_suite.REAL_MARGIN == 2


# ------------------------------------------------------------------------------------------------------ the real layers
@pytest.mark.parametrize("seed", gpu_suite.ENC_SEEDS)
def test_encoder_operands_keep_every_layer_exact(seed):
    """Per point (every cloud of the encoder cases draws its points from this base set): every partial sum of every layer stays
    below 2^24, h1..h4 stay below 2^22 (an integer below 2^22 is a piece pair under any block exponent its block can have:
    hi keeps 11 bits of at most 14 above the binary point, the remainder has at most 11), the weights have no lo piece and the
    activations have; and over the base cloud the law's three-product sum of each layer is the plain product."""
    Ws, bs = law.encoder_weights(seed)
    x = law.encoder_base_points(gpu_suite.ENC_CLOUD_SEED)
    hs, sums = law.encoder_chain(x, Ws, bs)
    assert max(sums) < 2 ** 24 and max(h.max() for h in hs[:4]) < 2 ** 22 and np.abs(hs[4]).max() < 2 ** 24
    exps = []
    for l in range(1, 5):                                               # layer l + 1 contracts h_l with W_{l+1}
        W = Ws[l]
        assert np.array_equal(W, np.rint(W)) and np.abs(W).max() < 2 ** 11
        wh, wl, wexp = law.pack_rows(W)
        assert not wl.any()
        cb = (64, 128, 256, 256)[l - 1]                                 # the producing layer's column tile
        h = hs[l - 1].astype(np.float32)
        ah, al, aexp = law.pack_act(h, cb)
        assert np.array_equal(law.unpack(ah, al, np.repeat(np.repeat(aexp, 128, axis=0), cb, axis=1)), h)
        assert al.any() and (np.diff(aexp, axis=0) != 0).any()
        got = law.three_product(ah, al, aexp, cb, wh, wl, wexp) + bs[l].astype(np.float64)[None, :]
        want = hs[l] if l == 4 else None
        pre = hs[l - 1] @ W.astype(np.float64).T + bs[l].astype(np.float64)[None, :]
        assert np.array_equal(got, pre) and (want is None or np.array_equal(pre, want))
        exps.append(aexp)
    assert (exps[3][:, 0] != exps[3][:, 1]).any()                       # h4's two exponent blocks: layer 5 rescales along k
    # every cloud consists of these points; the zero tile ties all of its points
    for B, Np in gpu_suite.ENC_SHAPES:
        assert Np % 128 == 0
    c = law.encoder_cloud(2, 256, gpu_suite.ENC_CLOUD_SEED).reshape(-1, 3)
    assert {tuple(p) for p in c} <= {tuple(p) for p in x}
    assert {B * Np for B, Np in gpu_suite.ENC_SHAPES} >= {128, 384, 5 * 256 + 128} and max(B * Np for B, Np in gpu_suite.ENC_SHAPES) > 32768

"""CPU suite for the encoder's host side: hp_encoder_plan, the query that tells which launches hp_encoder_forward[_pair] and
hp_encoder_backward[_ld|_pair] take for a shape under the current switches.  It is answered by the functions
encoder_forward_impl / encoder_backward_impl (csrc/model.hip) decide with; here it must flip exactly where that code's
conditions flip, refuse what the calls refuse, and show that the case tables of tests/test_encoder_routes_gpu.py
(tests/encoder_law.py) reach every route combination.  Nothing here reaches a GPU: the query follows no pointer."""
import ctypes
import importlib.util
import os

import pytest

from conftest import PKG_DIR

import encoder_law as law


@pytest.fixture(scope="module")
def ops():
    spec = importlib.util.spec_from_file_location("hp_build", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from hyperpocket_amd import ops
    return ops


def test_cases_reach_every_route(ops):
    law.check_cases_reach_every_route()


def test_forward_tails_flip_with_the_slab_condition(ops):
    """Behind the fused pool the h5 slot (R*512 floats) holds 2 * tiles * 512 floats of partials; the tails' slabs
    (4*64*512 + 8*64*out_size floats) fit behind them from R = 512 on at out_size = 128 — whatever B and Np make up R."""
    need = lambda out: 4 * 64 * 512 + 8 * 64 * out
    for route, tile in (("default", 128), ("r3", 128)):
        for B, Np in [(1, 128), (2, 128), (3, 128), (1, 256), (1, 384), (4, 128), (2, 256), (1, 512), (5, 128), (1, 640)]:
            p = law.plan_of(route, B, Np)
            R = B * Np
            assert p["pool_fused"] and p["tile_rows"] == tile
            assert p["fwd_tails_skinny"] == (R * 512 - 2 * (R // tile) * 512 >= need(128)) == (R >= 512), (route, B, Np)
    assert not law.plan_of("default", 3, 128)["fwd_tails_skinny"] and law.plan_of("default", 4, 128)["fwd_tails_skinny"]   # 384 | 512
    # a wider output needs more room: out_size = 512 from R = 896 on
    assert [law.plan_of("default", 1, Np, 512)["fwd_tails_skinny"] for Np in (640, 768, 896)] == [False, False, True]
    # 64-row tiles (fp32 route) keep twice the partials per row: the slabs fit from R = 448 on
    assert [law.plan_of("fp32", B, 64)["fwd_tails_skinny"] for B in (5, 6, 7, 8)] == \
           [B * 64 * 512 - 2 * B * 512 >= need(128) for B in (5, 6, 7, 8)] == [False, False, True, True]
    # ragged clouds: no fused pool on the split route, so no skinny tails at any size
    for B, Np in [(1, 1), (1, 129), (2, 127), (3, 200), (64, 100)]:
        p = law.plan_of("default", B, Np)
        assert (p["conv"], p["pool_fused"], p["fwd_tails_skinny"]) == ("split_f32", False, False)
    # whole tiles: the P-format unless switched off
    assert law.plan_of("default", 4, 128)["conv"] == "pformat" and law.plan_of("r3", 4, 128)["conv"] == "split_f32"
    assert law.plan_of("fp32", 4, 128)["conv"] == "gemm_f32"


def test_fp32_route_tile_rows_flip_with_the_workgroup_count(ops):
    """hp_gemm_tile_rows for layer 5 (N = K = 512): 128-row tiles once ceil(R / 128) * 4 * n workgroups reach 384 — with one
    encoder from R = 12161 on (96 row tiles), i.e. for whole 64-row clouds between R = 12160 and 12224; the first R that is
    also whole 128-row tiles is 12288.  Below it 64-row tiles (64x128 needs 512 workgroups: R >= 8129; else 64x64)."""
    tile = lambda B, Np, n=1: law.plan_of("fp32", B, Np, is_vae=(True, False)[:n] if n > 1 else (True,))
    assert tile(1, 12160)["tile_rows"] == 64 and tile(1, 12161)["tile_rows"] == 128
    assert tile(1, 12287)["tile_rows"] == 128 and tile(1, 12288)["tile_rows"] == 128
    # what the pool makes of it: Np = 192 is whole 64-row tiles only
    assert [tile(B, 192)["pool_fused"] for B in (62, 63, 64)] == [True, True, False]          # R = 11904, 12096 | 12288
    assert [tile(B, 128)["tile_rows"] for B in (94, 95, 96)] == [64, 64, 128]                 # R = 12032, 12160 | 12288
    assert all(tile(B, 128)["pool_fused"] for B in (94, 95, 96))
    # the pair batches both encoders into one launch: twice the workgroups, the flip at half the rows
    assert tile(1, 6016, 2)["tile_rows"] == 64 and tile(1, 6017, 2)["tile_rows"] == 128
    assert [tile(B, 192, 2)["pool_fused"] for B in (31, 32)] == [True, False]


def test_skinny_limit_is_64_clouds(ops):
    for route in ("default", "fp32"):
        a, b = law.plan_of(route, 64, 128), law.plan_of(route, 65, 128)
        assert a["fwd_tails_skinny"] and a["bwd_tails_skinny"] == (True,)
        assert not b["fwd_tails_skinny"] and b["bwd_tails_skinny"] == (False,)
        assert a["bwd_fused"] and b["bwd_fused"]
    with law.switches(skinny=0):
        p = law.plan_of("default", 8, 128)
        assert not p["fwd_tails_skinny"] and p["bwd_tails_skinny"] == (False,)


@pytest.mark.parametrize("chain16,cap", [(1, 20), (0, 23)])
def test_backward_row_ranges_are_min_B_cap_for_one_and_two_encoders(ops, chain16, cap):
    """S = max(1, min(B, cap)): 20 ranges on the f16 chain, 23 on the fp32 chain — the same for a single encoder and for a pair
    (hp_encoder_backward_pair promises the gradients of two single calls bit for bit; the ranges fix the summation order)."""
    with law.switches(chain16=chain16):
        for B in (1, 2, 19, 20, 21, 22, 23, 24, 64, 65, 2048):
            one = law.plan_of("default", B, 128)
            two = law.plan_of("default", B, 128, is_vae=(True, False), ld=256)
            assert one["bwd_fused"] and two["bwd_fused"]
            assert one["bwd_splits"] == two["bwd_splits"] == min(B, cap), B
        assert not law.plan_of("default", 2049, 128)["bwd_fused"]                            # hp_enc_bwd_max_clouds


def test_backward_fallbacks(ops):
    plan = lambda **kw: law.plan_of("default", 4, 128, **kw)
    assert plan(out_size=512)["bwd_fused"] and not plan(out_size=544)["bwd_fused"]
    assert plan(out_size=544)["bwd_splits"] == 0
    assert plan(aligned=True)["bwd_fused"] and not plan(aligned=False)["bwd_fused"]
    assert plan(aligned=False)["bwd_tails_skinny"] == (False,)                               # the slabs are not 16-byte aligned either
    assert plan(dedup=True)["bwd_fused"] and not plan(dedup=False)["bwd_fused"]
    assert plan(dedup=False)["bwd_tails_skinny"] == (True,)
    # grad_out_ld % 4 decides for a plain encoder (the tail reads grad_out in place); a VAE's d mu is formed in the workspace
    for ld, ok in ((128, True), (129, False), (130, False), (131, False), (132, True), (256, True)):
        assert plan(is_vae=(False,), ld=ld)["bwd_tails_skinny"] == (ok,), ld
        assert plan(is_vae=(True,), ld=ld)["bwd_tails_skinny"] == (True,), ld
    # in a pair one encoder's stride sends both tails to the GEMM launches (they share the program)
    assert plan(is_vae=(True, False), ld=(256, 256))["bwd_tails_skinny"] == (True, True)
    assert plan(is_vae=(True, False), ld=(256, 258))["bwd_tails_skinny"] == (False, False)
    # ... unless the backward is layered: one program per encoder
    assert plan(is_vae=(True, False), ld=(256, 258), dedup=False)["bwd_tails_skinny"] == (True, False)
    # widths: 96 is served forward (three strips per head) and refused backward (48-deep ranges); 32 with one head has one range
    assert plan(out_size=96)["fwd_tails_skinny"] and plan(out_size=96)["bwd_tails_skinny"] == (False,)
    assert plan(out_size=32)["bwd_tails_skinny"] == (True,) and plan(out_size=32, is_vae=(False,))["bwd_tails_skinny"] == (False,)
    assert not plan(out_size=100)["fwd_tails_skinny"] and plan(out_size=100)["bwd_tails_skinny"] == (False,)


def test_plan_refuses_what_the_calls_refuse(ops):
    lib = ops.load_library()
    p = ops._EncoderPlan()
    vae = (ctypes.c_int * 2)(1, 0)
    ld = (ctypes.c_int * 2)(0, 0)
    q = lambda B, Np, out, n, v=vae, l=ld, pl=p: lib.hp_encoder_plan(B, Np, out, n, v, l, 1, 1, ctypes.byref(pl) if pl is not None else None)
    assert q(4, 128, 128, 1) == 0 and q(4, 128, 128, 2) == 0
    assert q(4, 128, 128, 1, l=None) == 0                                # no strides: dense
    for bad in [(0, 128, 128, 1), (4, 0, 128, 1), (4, 128, 0, 1), (-1, 128, 128, 1), (4, 128, 128, 0), (4, 128, 128, 3)]:
        assert q(*bad) == -1, bad
    assert q(4, 128, 128, 1, v=None) == -1 and q(4, 128, 128, 1, pl=None) == -1
    assert q(65535, 1, 128, 1) == 0 and q(65536, 1, 128, 1) == -1        # one encoder: the grid's y limit
    assert q(32767, 1, 128, 2) == 0 and q(32768, 1, 128, 2) == -1        # a pair: ... halved
    assert lib.hp_encoder_plan(2, 1 << 30, 128, 1, vae, ld, 1, 0, ctypes.byref(p)) == -1    # B * Np = 2^31 rows
    assert lib.hp_encoder_plan(1, 1 << 22, 128, 1, vae, ld, 1, 1, ctypes.byref(p)) == -1    # dedup with Np * 512 = 2^31
    assert lib.hp_encoder_plan(1, 1 << 22, 128, 1, vae, ld, 1, 0, ctypes.byref(p)) == 0
    short = (ctypes.c_int * 2)(127, 0)
    assert q(4, 128, 128, 1, l=short) == -1                              # grad_out_ld < out_size
    with pytest.raises(ops.HipExtensionError):
        ops.encoder_plan(0, 128)

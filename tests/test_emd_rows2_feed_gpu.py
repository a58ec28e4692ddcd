"""GPU: the two candidate feeds of the list-driven EMD phase-2 sweeps (hp_emd_set_rows2_feed, emd.hip emd_rows2_kernel FEED), bit for bit.

Feed 0 fetches the set1 records on the scalar path, stage by stage; feed 1 has each workgroup copy them into LDS once and its waves
read them from there.  Only the operand source differs: per row and per (candidate range, parity) class the same terms enter the same
fma chain in the same order, so nothing may move.  Feed 1 is compared with feed 0 as raw 32-bit patterns on cost, grad1 / grad2 (and
hp_emd_forward_acc's accumulated gradient), the whole of `temp` and the workspace from the final records on (the helpers restate
those of test_emd_compact_fused_gpu.py): over regimes in which set2 empties at once, slowly or not at all, the smallest shapes at
which the staging can go wrong, set1 sizes around the staged block's bound (2048 padded points; past it a call takes feed 0), both
list-driven compaction modes, every forced rows-per-lane instance, cull placements, and one and two chains.  Every output buffer
starts as NaN and the workspace as zeros, so a record the new feed failed to stage shows.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FEED_MAX_NP = 2048      # emd.hip kFeedMaxNP


def _lib():
    from hyperpocket_amd._lib import load_library
    lib = load_library()
    lib.hp_emd_partials_floats.restype = ctypes.c_long
    return lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tail_offset(n, m):
    """float offset of the final records of set1 (flp) in a cloud's workspace (emd.hip ws_layout): everything from there on
    (flp, frp, permutations, block / tile boxes, flag) is read after the forward."""
    NP, MP = (n + 63) // 64 * 64, (m + 63) // 64 * 64
    return (NP + 8) * 4 + (MP + 8) * 4 + (MP + 8)


def _forward(a, c, feed, compact=2, grad1=True, acc=None):
    """hp_emd_forward (acc None) or hp_emd_forward_acc (acc = (initial grad2, scale)) under the given feed and compaction mode;
    every output buffer and the partials start as NaN, the workspace as zeros."""
    from hyperpocket_amd._lib import call, current_stream
    lib = _lib()
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    f32 = dict(device=a.device, dtype=torch.float32)
    temp = torch.full((b, 2 * (n + m)), float("nan"), **f32)
    ws = torch.zeros((lib.hp_approxmatch_workspace_floats(b, n, m),), **f32)
    part = torch.full((lib.hp_emd_partials_floats(b, n, m),), float("nan"), **f32)
    cost = torch.full((b,), float("nan"), **f32)
    g1 = torch.full((b, n, 3), float("nan"), **f32) if grad1 else None
    prev_feed = lib.hp_emd_set_rows2_feed(feed)
    prev = lib.hp_emd_set_compact(compact)
    try:
        if acc is None:
            g2 = torch.full((b, m, 3), float("nan"), **f32)
            call("hp_emd_forward", b, n, m, a, c, temp, ws, part, cost, g1, g2, current_stream(a.device))
        else:
            g2 = acc[0].clone()
            call("hp_emd_forward_acc", b, n, m, a, c, temp, ws, part, cost, g2, float(acc[1]), current_stream(a.device), None)
        torch.cuda.synchronize()
    finally:
        lib.hp_emd_set_compact(prev)
        lib.hp_emd_set_rows2_feed(prev_feed)
    per = ws.numel() // b
    tail = ws.view(b, per)[:, _tail_offset(n, m):]
    return {"cost": cost, "grad1": g1, "grad2": g2, "temp": temp, "ws_tail": tail}


def _assert_same(got, want, what):
    for k in ("cost", "grad1", "grad2", "temp", "ws_tail"):
        if got[k] is None:
            continue
        assert torch.equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs"
    assert torch.isfinite(got["cost"]).all() and torch.isfinite(got["grad2"]).all(), what


def _assert_feeds_same(a, c, what, **kw):
    """feed 1 against feed 0, the same call otherwise"""
    got = _forward(a, c, 1, **kw)
    _assert_same(got, _forward(a, c, 0, **kw), f"{what}, LDS feed against the scalar feed")
    return got


def _regime(name, b, n, m, seed):
    r = np.random.RandomState(seed)
    u = lambda k: r.rand(b, k, 3).astype(np.float32) - 0.5
    if name == "uniform":
        x, y = u(n), u(m)
    elif name == "normal_029":          # rec's spread at the bench operating point
        x, y = u(n), (0.29 * r.randn(b, m, 3)).astype(np.float32)
    elif name == "noisy_copy_0002":     # permuted set1 + N(0, 0.002^2)
        x = u(max(n, m))
        y = np.stack([xi[r.permutation(len(xi))][:m] for xi in x]) + (0.002 * r.randn(b, m, 3)).astype(np.float32)
        x = x[:, :n]
    elif name == "identical":           # the lists empty at once
        x = u(n)
        y = x[:, :m].copy()
    elif name == "far_apart":           # nothing dies until the late levels: every segment full
        x, y = u(n), u(m) + np.float32(3.0)
    elif name == "degenerate":          # every point of set2 the same
        x, y = u(n), np.repeat(u(1), m, 1)
    else:
        raise ValueError(name)
    return (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda())


@pytest.mark.parametrize("name", ["uniform", "normal_029", "noisy_copy_0002", "identical", "far_apart", "degenerate"])
def test_feeds_are_bit_identical_across_regimes(name):
    a, c = _regime(name, 3, 2048, 2048, 11)
    _assert_feeds_same(a, c, name)


@pytest.mark.parametrize("b,n,m", [(1, 64, 64), (5, 96, 130), (2, 200, 330), (3, 330, 200), (1, 2048, 100)])
def test_feeds_smallest_shapes(b, n, m):
    """(1, 64, 64): 16 candidates per range, one loop iteration per wave; (5, 96, 130): n and m no multiples of 64, padded records
    are staged (and a cloud's workspace starts 8 bytes off a 16-byte boundary); (1, 2048, 100): the largest staged block, one row
    tile."""
    for name in ("uniform", "normal_029"):
        a, c = _regime(name, b, n, m, 100 + n + m)
        _assert_feeds_same(a, c, f"{name} {b}x{n}x{m}")


@pytest.mark.parametrize("n", [FEED_MAX_NP - 64, FEED_MAX_NP - 1, FEED_MAX_NP, FEED_MAX_NP + 1])
def test_feeds_around_the_staging_bound(n):
    """set1 one tile below the bound, just below it, at it (the block is full) and just above (NP = 2112: the call takes the scalar
    feed, whatever the switch says)."""
    a, c = _regime("normal_029", 1, n, 100, 7 + n)
    _assert_feeds_same(a, c, f"n={n}")


@pytest.mark.parametrize("compact", [1, 2])
def test_each_list_driven_mode_under_the_lds_feed_equals_the_full_sweeps(compact):
    """hp_emd_set_compact(1) (the rows from emd_compact_kernel's list) and (2) (from the workgroup's own scan) under feed 1, each
    against the sweeps over every point, which no feed switch reaches."""
    for b, n, m in ((3, 2048, 2048), (2, 200, 330)):
        a, c = _regime("normal_029", b, n, m, 17 + m)
        _assert_same(_forward(a, c, 1, compact=compact), _forward(a, c, 0, compact=0), f"compact={compact} {b}x{n}x{m}")


@pytest.mark.parametrize("r1,r2,g2", [(1, 1, 1), (2, 2, 2), (4, 4, 1)])
def test_feeds_forced_rows_per_lane(r1, r2, g2):
    from hyperpocket_amd._lib import call
    a, c = _regime("normal_029", 3, 1000, 2048, 31)
    call("hp_emd_set_rows_per_lane", r1, r2, g2)
    try:
        for compact in (1, 2):
            _assert_feeds_same(a, c, f"rows {r1},{r2},{g2} compact={compact}", compact=compact)
    finally:
        call("hp_emd_set_rows_per_lane", 0, 0, 0)


@pytest.mark.parametrize("cull", [0, 3, 8])
def test_feeds_under_cull(cull):
    """cull 0: the list-driven sweeps start at level 1; 3: the default; 8: only the last level's sweep is list-driven."""
    lib = _lib()
    a, c = _regime("noisy_copy_0002", 3, 2048, 2048, 21)
    prev = lib.hp_emd_set_cull(cull)
    try:
        _assert_feeds_same(a, c, f"cull={cull}")
    finally:
        lib.hp_emd_set_cull(prev)


@pytest.mark.parametrize("chains", [1, 2])
def test_feeds_chains_odd_batch_and_accumulated_gradient(chains):
    """B = 5: two chains of 2 and 3 clouds, or one; then hp_emd_forward_acc's form on a non-zero initial gradient."""
    lib = _lib()
    a, c = _regime("normal_029", 5, 2048, 2048, 5)
    g0 = torch.from_numpy(np.random.RandomState(9).randn(5, 2048, 3).astype(np.float32)).cuda()
    prev = lib.hp_emd_set_chains(chains)
    try:
        _assert_feeds_same(a, c, f"chains={chains}")
        _assert_feeds_same(a, c, f"forward_acc chains={chains}", grad1=False, acc=(g0, 0.05 / 2048))
    finally:
        lib.hp_emd_set_chains(prev)


def test_feed_switch_takes_two_values():
    lib = _lib()
    prev = lib.hp_emd_set_rows2_feed(0)
    try:
        assert lib.hp_emd_set_rows2_feed(1) == 0       # returns the previous value
        assert lib.hp_emd_set_rows2_feed(0) == 1
        assert lib.hp_emd_set_rows2_feed(7) == 0       # above 1: clamped to 1
        assert lib.hp_emd_set_rows2_feed(-1) == 1
        load = lib.hp_emd_set_rows2_feed(1 - prev)     # -1 restored the load-time value
        assert load in (0, 1)
        assert lib.hp_emd_set_rows2_feed(-1) == 1 - prev and lib.hp_emd_set_rows2_feed(0) == load
    finally:
        lib.hp_emd_set_rows2_feed(prev)

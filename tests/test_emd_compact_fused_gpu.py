"""GPU: the fused compaction of the EMD level sweeps (hp_emd_set_compact(2), emd.hip fused_scan) against the full sweeps (0) and
against emd_compact_kernel (1), bit for bit.

In the fused form no compaction kernel runs: every phase-2 launch leaves its live rows in its own segment of the cloud's row list
(-1 in the unused slots) and each row's record in a slot fixed by the list it was launched from, and the next phase-2 launch scans
that list in its prologue.  The candidates it leaves for the merged launches are a superset of emd_compact_kernel's (the extra ones
carry zero weights), each class in the full sweep's order, so nothing may move: cost, grad1 / grad2 (and hp_emd_forward_acc's
accumulated gradient), the whole of `temp` and the workspace from the final records on are compared as raw 32-bit patterns (the
helpers restate those of test_emd_compact_gpu.py), over regimes in which set2 empties fast, slowly or not at all, ragged sizes up
to the fused form's limit (MP = 4096) and past it, every forced rows-per-lane instance, every placement of the culling levels,
and one and two chains.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


def _forward(a, c, compact, grad1=True, acc=None):
    """hp_emd_forward (acc None) or hp_emd_forward_acc (acc = (initial grad2, scale)) with the compaction switch at `compact`;
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
    per = ws.numel() // b
    tail = ws.view(b, per)[:, _tail_offset(n, m):]
    return {"cost": cost, "grad1": g1, "grad2": g2, "temp": temp, "ws_tail": tail, "ws": ws, "part": part}


def _assert_same(got, want, what):
    for k in ("cost", "grad1", "grad2", "temp", "ws_tail"):
        if got[k] is None:
            continue
        assert torch.equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs"
    assert torch.isfinite(got["cost"]).all() and torch.isfinite(got["grad2"]).all(), what


def _assert_fused_same(a, c, what, **kw):
    """mode 2 against mode 0 and against mode 1"""
    fused = _forward(a, c, 2, **kw)
    _assert_same(fused, _forward(a, c, 0, **kw), f"{what}, fused against the full sweeps")
    _assert_same(fused, _forward(a, c, 1, **kw), f"{what}, fused against the compaction kernel")
    return fused


def _regime(name, b, n, m, seed):
    r = np.random.RandomState(seed)
    u = lambda k: r.rand(b, k, 3).astype(np.float32) - 0.5
    if name == "uniform":
        x, y = u(n), u(m)
    elif name == "normal_029":          # rec's spread at the bench operating point
        x, y = u(n), (0.29 * r.randn(b, m, 3)).astype(np.float32)
    elif name.startswith("noisy_copy"):  # permuted set1 + N(0, sigma^2)
        sig = {"noisy_copy_003": 0.03, "noisy_copy_0002": 0.002}[name]
        x = u(max(n, m))
        y = np.stack([xi[r.permutation(len(xi))][:m] for xi in x]) + (sig * r.randn(b, m, 3)).astype(np.float32)
        x = x[:, :n]
    elif name == "identical":           # the lists empty fast
        x = u(n)
        y = x[:, :m].copy()
    elif name == "far_apart":           # every exponential underflows until the late levels: no point dies early, every segment full
        x, y = u(n), u(m) + np.float32(3.0)
    elif name == "degenerate":          # every point of set2 the same
        x, y = u(n), np.repeat(u(1), m, 1)
    else:
        raise ValueError(name)
    return (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda())


@pytest.mark.parametrize("name", ["uniform", "normal_029", "noisy_copy_003", "noisy_copy_0002", "identical", "far_apart",
                                  "degenerate"])
def test_fused_sweeps_are_bit_identical_across_regimes(name):
    a, c = _regime(name, 3, 2048, 2048, 11)
    _assert_fused_same(a, c, name)


@pytest.mark.parametrize("b,n,m", [(1, 64, 64), (5, 96, 130), (3, 330, 200), (2, 200, 330), (2, 2048, 700), (2, 1000, 2048),
                                   (1, 100, 4096), (1, 100, 4100)])
def test_fused_sweeps_ragged_sizes(b, n, m):
    """(1, 64, 64): one segment, one workgroup; (5, 96, 130): m no multiple of 64; (2, 2048, 700): every set2 point starts with
    remainR = multiR = 2; (1, 100, 4096): the largest set the fused form takes; (1, 100, 4100): past it, the call runs as mode 1."""
    for name in ("uniform", "normal_029"):
        a, c = _regime(name, b, n, m, 100 + n + m)
        _assert_fused_same(a, c, f"{name} {b}x{n}x{m}")


@pytest.mark.parametrize("r1,r2,g2", [(1, 1, 1), (2, 2, 2), (4, 4, 1), (1, 4, 0), (4, 1, 2)])
def test_fused_sweeps_forced_rows_per_lane(r1, r2, g2):
    """Every rows-per-lane instance: the segments a launch writes and the window the next one reads then differ in size from the
    heuristic's."""
    from hyperpocket_amd._lib import call
    a, c = _regime("normal_029", 3, 1000, 2048, 31)
    call("hp_emd_set_rows_per_lane", r1, r2, g2)
    try:
        _assert_fused_same(a, c, f"rows {r1},{r2},{g2}")
    finally:
        call("hp_emd_set_rows_per_lane", 0, 0, 0)


@pytest.mark.parametrize("cull", [0, 1, 2, 3, 8, 9])
def test_fused_sweeps_under_every_cull(cull):
    """cull 0: the plain full sweep of level 0 leaves the first list; 1: the culling sweep of level 0 does; 2, 3, 8: the culling
    sweep of the last culled level reads a list and leaves one; 9: no plain level is left."""
    lib = _lib()
    a, c = _regime("noisy_copy_003", 3, 2048, 2048, 21)
    prev = lib.hp_emd_set_cull(cull)
    try:
        _assert_fused_same(a, c, f"cull={cull}")
    finally:
        lib.hp_emd_set_cull(prev)


@pytest.mark.parametrize("chains", [1, 2])
def test_fused_sweeps_chains_odd_batch_and_accumulated_gradient(chains):
    """B = 5: two chains of 2 and 3 clouds, or one; then hp_emd_forward_acc's form."""
    lib = _lib()
    a, c = _regime("normal_029", 5, 2048, 2048, 5)
    g0 = torch.from_numpy(np.random.RandomState(9).randn(5, 2048, 3).astype(np.float32)).cuda()
    prev = lib.hp_emd_set_chains(chains)
    try:
        _assert_fused_same(a, c, f"chains={chains}")
        _assert_fused_same(a, c, f"forward_acc chains={chains}", grad1=False, acc=(g0, 0.05 / 2048))
    finally:
        lib.hp_emd_set_chains(prev)


def test_backward_on_a_workspace_written_by_the_fused_sweeps():
    from hyperpocket_amd._lib import call, current_stream
    a, c = _regime("normal_029", 3, 2048, 2048, 41)
    b, n, m = 3, 2048, 2048

    def backward(ws):
        g2 = torch.full((b, m, 3), float("nan"), device=a.device, dtype=torch.float32)
        call("hp_emd_backward", b, n, m, a, c, ws, g2, current_stream(a.device))
        torch.cuda.synchronize()
        return g2
    want = backward(_forward(a, c, 0)["ws"])
    assert torch.isfinite(want).all()
    assert torch.equal(_bits(backward(_forward(a, c, 2)["ws"])), _bits(want))


def _row_lists(part, b, n, m):
    """Each cloud's row lists 0 and 1 in `partials`, behind the cost partials (emd.hip CsLayout), as int32."""
    a16 = lambda x: (x + 15) // 16 * 16
    MP = (m + 63) // 64 * 64
    base = a16(b * ((max(n, m) + 63) // 64))
    w = a16((MP + 8) * 4)
    l0 = a16(w + MP + 8)
    l1 = a16(l0 + MP)
    cnt = a16(l1 + MP)
    per = a16(cnt + 16)
    assert part.numel() == base + b * per
    v = part[base:].view(torch.int32).view(b, per)
    return v[:, l0:l0 + MP], v[:, l1:l1 + MP]


def test_the_fused_path_runs_and_lists_the_live_points():
    """At cull 3 the phase-2 launches of levels 1..7 leave the lists 1, 0, 1, 0, 1, 0, 1, so list 1 ends as L_8, the points phase 2
    of the last level sweeps.  Every slot of it was written by the launch of level 7 (the buffer starts as NaN words): a point or
    -1, in segments of 64 x 2 row slots (rows per lane forced to 2) with the live entries first.  Without the -1 entries it holds,
    strictly ascending, exactly the points whose level-8 ratioR (final records) is non-zero — some, but fewer than m."""
    from hyperpocket_amd._lib import call
    lib = _lib()
    b, n, m = 3, 2048, 2048
    a, c = _regime("uniform", b, n, m, 11)
    prev = lib.hp_emd_set_cull(3)
    call("hp_emd_set_rows_per_lane", 0, 2, 0)
    try:
        on = _forward(a, c, 2)
    finally:
        call("hp_emd_set_rows_per_lane", 0, 0, 0)
        lib.hp_emd_set_cull(prev)
    _, last = _row_lists(on["part"], b, n, m)
    NP, MP = (n + 63) // 64 * 64, (m + 63) // 64 * 64
    frp = _tail_offset(n, m) + (NP + 8) * 16
    rec = on["ws"].view(b, -1)[:, frp:frp + (MP + 8) * 16].reshape(b, (MP + 8) // 2, 32)
    ratio8 = rec[:, :, 3 * 2 + 2 * 8:3 * 2 + 2 * 8 + 2].reshape(b, -1)[:, :m]      # [x0 x1 y0 y1 z0 z1 | r(lev)0 r(lev)1 ...]
    for i in range(b):
        lst = last[i]
        assert bool(((lst == -1) | ((lst >= 0) & (lst < m))).all())
        seg = (lst >= 0).view(-1, 128).to(torch.int32)
        assert bool((seg[:, 1:] <= seg[:, :-1]).all()), "a live entry behind a -1 inside a segment"
        live = lst[lst >= 0]
        assert 0 < live.numel() < m, live.numel()
        assert bool((live[1:] > live[:-1]).all())
        assert torch.equal(live, torch.nonzero(ratio8[i] != 0).flatten().to(torch.int32))


def test_compact_switch_takes_three_values():
    lib = _lib()
    prev = lib.hp_emd_set_compact(0)
    try:
        assert lib.hp_emd_set_compact(2) == 0       # returns the previous value
        assert lib.hp_emd_set_compact(1) == 2
        assert lib.hp_emd_set_compact(7) == 1       # above 2: clamped to 2
        assert lib.hp_emd_set_compact(-1) == 2
        load = lib.hp_emd_set_compact(0)            # -1 restored the load-time value
        assert lib.hp_emd_set_compact(-1) == 0 and lib.hp_emd_set_compact(3) == load
        assert lib.hp_emd_set_compact(prev) == 2
    finally:
        lib.hp_emd_set_compact(prev)

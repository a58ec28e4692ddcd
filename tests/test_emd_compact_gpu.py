"""GPU: the compacted EMD level sweeps (hp_emd_set_compact, emd.hip emd_compact_kernel) against the full sweeps, bit for bit.

A set2 point whose remainR has been clamped to +0 adds only exact zeros from then on, so leaving it out of the plain level sweeps
must not move a single bit: cost, grad1 / grad2 (and the accumulated gradient of hp_emd_forward_acc), the whole of `temp`, and the
workspace regions read after the call (final records, permutations, boxes, flag) are compared as raw 32-bit patterns with the
switch on and off, over regimes in which set2 empties fast, slowly or not at all, ragged sizes, one and two chains, the caller's
order (sets past 4096 points) and every forced rows-per-lane instance.
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


def _assert_same(on, off, what):
    for k in ("cost", "grad1", "grad2", "temp", "ws_tail"):
        if on[k] is None:
            continue
        assert torch.equal(_bits(on[k]), _bits(off[k])), f"{what}: {k} differs with the compaction on"
    assert torch.isfinite(on["cost"]).all() and torch.isfinite(on["grad2"]).all(), what


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
    elif name == "identical":
        x = u(n)
        y = x[:, :m].copy()
    elif name == "far_apart":           # every exponential underflows until the late levels: no point dies early
        x, y = u(n), u(m) + np.float32(3.0)
    elif name == "degenerate":          # every point of set2 the same
        x, y = u(n), np.repeat(u(1), m, 1)
    else:
        raise ValueError(name)
    return (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).cuda())


@pytest.mark.parametrize("name", ["uniform", "normal_029", "noisy_copy_003", "noisy_copy_0002", "identical", "far_apart",
                                  "degenerate"])
def test_compact_sweeps_are_bit_identical_across_regimes(name):
    a, c = _regime(name, 3, 2048, 2048, 11)
    _assert_same(_forward(a, c, 1), _forward(a, c, 0), name)


@pytest.mark.parametrize("b,n,m", [(2, 1000, 2048), (3, 330, 200), (2, 200, 330), (2, 2048, 700), (1, 64, 64), (5, 96, 130)])
def test_compact_sweeps_ragged_sizes(b, n, m):
    """Ragged sizes; (2, 2048, 700): n > 2m, so every set2 point starts with remainR = multiR = 2."""
    for name in ("uniform", "normal_029"):
        a, c = _regime(name, b, n, m, 100 + n + m)
        _assert_same(_forward(a, c, 1), _forward(a, c, 0), f"{name} {b}x{n}x{m}")


def test_compact_sweeps_two_chains_odd_batch_and_accumulated_gradient():
    """B = 33 at N = 2048: two chains of 16 and 17 clouds (each still fills the chip) or one, then hp_emd_forward_acc's form."""
    lib = _lib()
    a, c = _regime("normal_029", 33, 2048, 2048, 5)
    g0 = torch.from_numpy(np.random.RandomState(9).randn(33, 2048, 3).astype(np.float32)).cuda()
    for chains in (1, 2):
        prev = lib.hp_emd_set_chains(chains)
        try:
            _assert_same(_forward(a, c, 1), _forward(a, c, 0), f"chains={chains}")
            _assert_same(_forward(a, c, 1, grad1=False, acc=(g0, 0.05 / 2048)), _forward(a, c, 0, grad1=False, acc=(g0, 0.05 / 2048)),
                         f"forward_acc chains={chains}")
        finally:
            lib.hp_emd_set_chains(prev)


@pytest.mark.parametrize("b,n,m", [(2, 600, 4500), (1, 4200, 4100)])
def test_compact_sweeps_on_unordered_records(b, n, m):
    """A set past 4096 points: the records stay in the caller's order and no level culls, so compaction starts behind the phase-2
    sweep of level 0 (and the compaction kernel walks more than one chunk of its workgroup)."""
    for name in ("uniform", "noisy_copy_003"):
        a, c = _regime(name, b, n, m, 7 + m)
        _assert_same(_forward(a, c, 1), _forward(a, c, 0), f"{name} {b}x{n}x{m}")


@pytest.mark.parametrize("cull", [0, 1, 3, 8, 9])
def test_compact_sweeps_under_every_cull(cull):
    lib = _lib()
    a, c = _regime("noisy_copy_003", 3, 2048, 2048, 21)
    prev = lib.hp_emd_set_cull(cull)
    try:
        _assert_same(_forward(a, c, 1), _forward(a, c, 0), f"cull={cull}")
    finally:
        lib.hp_emd_set_cull(prev)


@pytest.mark.parametrize("r1,r2,g2", [(1, 1, 1), (2, 2, 2), (4, 4, 1), (1, 4, 0), (4, 1, 2)])
def test_compact_sweeps_forced_rows_per_lane(r1, r2, g2):
    """Every rows-per-lane instance of the compacted sweeps (the phase-2 one follows hp_emd_set_rows_per_lane's rows2) against
    the full sweeps under the same forcing."""
    from hyperpocket_amd._lib import call
    a, c = _regime("normal_029", 3, 1000, 2048, 31)
    call("hp_emd_set_rows_per_lane", r1, r2, g2)
    try:
        on, off = _forward(a, c, 1), _forward(a, c, 0)
    finally:
        call("hp_emd_set_rows_per_lane", 0, 0, 0)
    _assert_same(on, off, f"rows {r1},{r2},{g2}")


def _compaction_words(part, b, n, m):
    """Each cloud's compaction scratch in `partials`, behind the cost partials (emd.hip CsLayout): row lists 0 and 1 and the
    count block ([0] / [1]: the lists' lengths), as int32."""
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
    return v[:, l0:l0 + MP], v[:, l1:l1 + MP], v[:, cnt:cnt + 16]


def test_compaction_runs_and_lists_the_live_points():
    """The compacted sweeps are the ones that run: at the default cull of 3 the six compaction launches behind phase 2 of levels
    2..7 write row lists 0, 1, 0, 1, 0, 1, so list 1 ends as L_8, the points phase 2 of the last level sweeps.  It must hold, in
    ascending order, exactly the points whose level-8 ratioR (final records) is non-zero — fewer than m of them in this regime."""
    lib = _lib()
    b, n, m = 3, 2048, 2048
    a, c = _regime("uniform", b, n, m, 11)
    prev = lib.hp_emd_set_cull(3)
    try:
        on = _forward(a, c, 1)
    finally:
        lib.hp_emd_set_cull(prev)
    _, live_lists, cnt = _compaction_words(on["part"], b, n, m)
    NP, MP = (n + 63) // 64 * 64, (m + 63) // 64 * 64
    frp = _tail_offset(n, m) + (NP + 8) * 16
    rec = on["ws"].view(b, -1)[:, frp:frp + (MP + 8) * 16].reshape(b, (MP + 8) // 2, 32)
    ratio8 = rec[:, :, 3 * 2 + 2 * 8:3 * 2 + 2 * 8 + 2].reshape(b, -1)[:, :m]      # [x0 x1 y0 y1 z0 z1 | r(lev)0 r(lev)1 ...]
    for i in range(b):
        k = int(cnt[i, 1])
        assert 0 < k < m, k
        live = live_lists[i, :k]
        assert bool((live[1:] > live[:-1]).all()) and int(live[-1]) < m
        assert torch.equal(live, torch.nonzero(ratio8[i] != 0).flatten().to(torch.int32))


def test_backward_on_a_compacted_workspace():
    """hp_emd_backward reads the final records, permutations, boxes and flag of the forward's workspace: the same grad2, bit for
    bit, from a workspace written with the compaction on as from one written with it off."""
    from hyperpocket_amd._lib import call, current_stream
    a, c = _regime("normal_029", 3, 2048, 2048, 41)
    b, n, m = 3, 2048, 2048

    def backward(ws):
        g2 = torch.full((b, m, 3), float("nan"), device=a.device, dtype=torch.float32)
        call("hp_emd_backward", b, n, m, a, c, ws, g2, current_stream(a.device))
        torch.cuda.synchronize()
        return g2
    on, off = _forward(a, c, 1), _forward(a, c, 0)
    got, want = backward(on["ws"]), backward(off["ws"])
    assert torch.isfinite(want).all()
    assert torch.equal(_bits(got), _bits(want))


def test_compact_switch_returns_the_previous_setting():
    lib = _lib()
    prev = lib.hp_emd_set_compact(0)
    try:
        assert lib.hp_emd_set_compact(1) == 0
        assert lib.hp_emd_set_compact(-1) == 1      # -1: back to the load-time value (on)
    finally:
        lib.hp_emd_set_compact(prev)

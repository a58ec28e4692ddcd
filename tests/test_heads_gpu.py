"""The hypernetwork heads' kernels and the Adam kernels against tests/heads_law.py, through the C ABI alone.

  heads_t5_split_kernel + heads_fwd_kernel (csrc/heads_fwd.hip)        hp_hypernet_forward, one layer of heads
  heads_dw_kernel<false> and the bias gradient (csrc/hypernet.hip)     hp_hypernet_heads_dw_rows, hp_hypernet_backward
  adam_kernel (csrc/aux_kernels.hip)                                   hp_adam_step
  heads_dw_kernel<true>, heads_dw_persist_kernel<true>                 hp_hypernet_heads_dw_adam, hp_hypernet_heads_dw_adam_bg

LAWS (heads_law.py, nothing measured on the code under test): family E — integer operands, the result equals the int64 product
bit for bit; family R — full significands at three scales, every element within (L + 16) u (forward, L = 2048) or (Kc + 8) u
(dW, db) of the fp64 result, times the product of the absolute operands; Adam — every element of p, m, v within the bounds
counted from the roundings, against torch.optim.Adam's update in float64; the fused pass the same from the exact integer
gradient.  The forward's reference is formed from the t5 the call left in `t`: the trunk's own error does not enter.

ROUTES.  Every case of the heads first asserts, through hp_hypernet_heads_plan on the very pointers of the call, which launch
serves it (the Adam calls have one launch sequence and no route).  The fall-backs (one GEMM, per-head GEMMs, the skipped dW's
column sums) are held to the same two families.  heads_law.check_cases_reach_every_route shows that the tables reach every
route and both sides of every boundary of the dispatch.

Every buffer a call writes is NaN (or a sentinel) first: columns N .. theta_ld - 1 of theta, the floats around an unaligned
view and the rows around a row slice must come back untouched, everything else finite.  A second run is bit-identical.
A NULL bias is admitted by the forward (n_heads = 1) and a NULL bias gradient by the backward; both are run.

WORST err / bound MEASURED (one run of this file on an MI355X, 2026-10-20, the tree on top of commit e4f418d; the tests print a line
`HEADSLAW ...` per case before they assert).  Family E was equal bit for bit everywhere.  Family R and Adam, worst case per route:
    forward   stream kernel 0.0020 (B = 64, N = 2561)   one GEMM 0.0004 (N = 2561, switch off)   per-head GEMMs 0.0002
              — the bf16 pipe's fp32 accumulation shows no truncation: the bound stays at 2^-24
    dW, db    fragment-direct 0.250 (Kc = 7, rows = 64; dw_rows and the backward alike)   one GEMM 0.210 (Kc = 7, rows = 33)
              per-head GEMMs 0.154   skipped dW, column sums only 0.045
    Adam      hp_adam_step 0.9987 (n = 2 097 157)   fused dW + Adam 0.9952 (rows = 65, Kc = 8) — both in p, where |p| = 1 and the
              final subtraction's rounding, the bound's first term u |p64|, is attained; m and v stay below 0.49 in both
"""
import ctypes

import pytest
import torch

import heads_law as law

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p


# ------------------------------------------------------------------------------------------------ plumbing
def _lib():
    from hyperpocket_amd._lib import load_library
    lib = load_library()
    for n in ("hp_hypernet_saved_floats", "hp_hypernet_backward_workspace_floats", "hp_hypernet_t5_offset",
              "hp_hypernet_heads_dw_workspace_floats"):
        getattr(lib, n).restype = ctypes.c_long
    return lib


def _stream(t):
    from hyperpocket_amd._lib import current_stream
    return current_stream(t.device)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _view(x, off=0):
    """A copy of x on the GPU as a view `4 + off` floats into a buffer of sentinels: off = 0 sits on a 16-byte boundary, 1..3 past
    it.  -> (buffer, view)."""
    buf = torch.full((x.numel() + 12,), 123.0, dtype=torch.float32, device="cuda")
    v = buf[4 + off:4 + off + x.numel()].view(x.shape)
    v.copy_(x)
    assert (v.data_ptr() - off * 4) % 16 == 0
    return buf, v


def _guards_untouched(buf, v, off, what):
    n = v.numel()
    assert bool((buf[:4 + off] == 123.0).all()) and bool((buf[4 + off + n:] == 123.0).all()), f"{what}: a float outside the view was written"


_DEV = {}


def _dev(key, make):
    if key not in _DEV:
        _DEV[key] = make()
    return _DEV[key]


def _trunk_dev(fam):
    return _dev(("trunk", fam), lambda: tuple([t.cuda() for t in part] for part in law.trunk(fam)))


def _heads_dev(fam, outs, quirk):
    """The heads of a case on the GPU: [(W view, b view, rows)], back to back in one buffer — from a 16-byte boundary, or one
    float past it ("w+1") — or with 64 floats between them ("split")."""
    def make():
        W, b = law.head_weights(fam)
        gap = 64 if quirk == "split" else 0
        lead = 5 if quirk == "w+1" else 4
        n = sum(outs)
        wbuf = torch.zeros(lead + n * law.K + gap * len(outs) + 4, device="cuda")
        bbuf = torch.zeros(4 + n + gap * len(outs), device="cuda")
        heads, r, ow, ob = [], 0, lead, 4
        for h in outs:
            wv, bv = wbuf[ow:ow + h * law.K].view(h, law.K), bbuf[ob:ob + h]
            wv.copy_(W[r:r + h])
            bv.copy_(b[r:r + h])
            heads.append((wv, bv, h))
            r, ow, ob = r + h, ow + h * law.K + gap, ob + h + gap
        return heads, (wbuf, bbuf)
    return _dev(("heads", fam, outs, quirk), make)[0]


def _weights_struct(fam, heads, bias=True):
    tw, tb = _trunk_dev(fam)
    w = law.HyperWeights()
    for l in range(5):
        w.trunk_w[l], w.trunk_b[l] = tw[l].data_ptr(), tb[l].data_ptr()
    w.n_heads = len(heads)
    for h, (wv, bv, n) in enumerate(heads):
        w.head_out[h], w.head_w[h], w.head_b[h] = n, wv.data_ptr(), bv.data_ptr() if bias else None
    return w


# ================================================================================================ 1. forward
def _forward(lib, fam, B, heads, route, pad, bias):
    from hyperpocket_amd._lib import call
    N = sum(n for *_, n in heads)
    w = _weights_struct(fam, heads, bias)
    t = _nan(lib.hp_hypernet_saved_floats(B))
    theta = _nan(B, N + pad)
    lat = law.latent(fam, B).cuda()
    got = law.plan(lib, B, w, None, t.data_ptr(), None)
    assert got[:2] == (0, route), f"route {got}, expected {route}"
    call("hp_hypernet_forward", B, law.IN_SIZE, lat, ctypes.byref(w), t, theta, N + pad, _stream(t))
    torch.cuda.synchronize()
    o5 = lib.hp_hypernet_t5_offset(B)
    return t[o5:o5 + B * law.K].view(B, law.K).cpu(), theta.cpu()


def _forward_case(fam, B, outs, route, quirk):
    lib = _lib()
    tag = f"fwd {fam} B={B} heads={outs} {quirk or ''}"
    heads = _heads_dev(fam, outs, quirk)
    N = sum(outs)
    Wc, bc = law.head_weights(fam)
    Wc, bc = Wc[:N], bc[:N]
    worst = 0.0
    with law.stream_switch(lib, 0 if quirk == "switch0" else 1):
        first = None
        for pad, bias in ((0, True), (3, True), (3, False), (0, True)):
            t5, theta = _forward(lib, fam, B, heads, route if bias or len(outs) == 1 else law.FWD_PER_HEAD, pad, bias)
            assert torch.isfinite(t5).all(), tag
            assert torch.isnan(theta[:, N:]).all(), f"{tag}: a column past N was written"
            got = theta[:, :N]
            b = bc if bias else None
            if fam == "E":
                assert law.is_family_e(t5), f"{tag}: t5 is not small varying integers — the exact family's premise"
                law.check_exact(tag, "theta", got, law.int_mm(t5, Wc.t(), b))
            else:
                want, bound = law.fwd64(t5, Wc, b)
                worst = max(worst, law.check(tag, "theta", got, want, bound))
            if (pad, bias) == (0, True):
                if first is None:
                    first = (t5, theta)
                else:
                    assert torch.equal(first[0], t5) and torch.equal(first[1], theta), f"{tag}: the second run differs"
    if fam == "R":
        print(f"HEADSLAW fwd route={route} {tag} worst err/bound = {worst:.4f}")


@pytest.mark.parametrize("fam", ["E", "R"])
@pytest.mark.parametrize("name,B,outs,route,quirk", law.FWD_CASES, ids=[c[0] for c in law.FWD_CASES])
def test_heads_forward_stream_kernel(fam, name, B, outs, route, quirk):
    """N at the tile edges (16 = one tile, 17 / 81 ragged, 79 / 95 one row short, 80 / 96 whole tiles and whole workgroups of
    five waves; fewer tiles than waves up to N = 64; 2561 = 34 workgroups: the stage rotation wraps and the last tile is
    ragged) and B at the cloud-tile edges, each with theta_ld = N and N + 3, with and without a bias."""
    _forward_case(fam, B, outs, route, quirk)


@pytest.mark.parametrize("fam", ["E", "R"])
@pytest.mark.parametrize("name,B,outs,route,quirk", law.FWD_FALLBACKS + law.FWD_SWITCHED,
                         ids=[c[0] for c in law.FWD_FALLBACKS + law.FWD_SWITCHED])
def test_heads_forward_fallbacks(fam, name, B, outs, route, quirk):
    """What the stream kernel does not serve goes to one GEMM (N < 16, B > 64, W off its 16-byte boundary, the switch off) or to
    a GEMM per head (heads not back to back): route asserted, same laws."""
    _forward_case(fam, B, outs, route, quirk)


def test_cases_reach_every_route():
    law.check_cases_reach_every_route(_lib())


# ================================================================================================ 2. dW and db
def _dw_check(tag, fam, got_dw, got_db, dth, t5):
    """dth: the (Kc x rows) columns the pass contracts.  -> worst err / bound."""
    worst = 0.0
    if fam == "E":
        if got_dw is not None:
            law.check_exact(tag, "dW", got_dw, law.int_mm(dth.t(), t5))
        if got_db is not None:
            law.check_exact(tag, "db", got_db, dth.to(torch.int64).sum(0))
        return worst
    want, bound, wdb, bdb = law.dw64(dth, t5)
    if got_dw is not None:
        worst = max(worst, law.check(tag, "dW", got_dw, want, bound))
    if got_db is not None:
        worst = max(worst, law.check(tag, "db", got_db, wdb, bdb))
    return worst


@pytest.mark.parametrize("fam", ["E", "R"])
@pytest.mark.parametrize("Kc,rows,r0,pad,route", law.DW_ROWS_CASES)
def test_heads_dw_rows(fam, Kc, rows, r0, pad, route):
    """hp_hypernet_heads_dw_rows: odd Kc (the half step whose h == 1 lanes load nothing), Kc around the prefetch depth (a step
    of kPref = 4 k-steps is 8 clouds) and past one GPU's batch, rows around the 32-row unit, a row offset, a padded stride;
    with `out` one float past its boundary the GEMM."""
    from hyperpocket_amd._lib import call
    lib = _lib()
    tag = f"dw_rows {fam} Kc={Kc} rows={rows} r0={r0} ld={r0 + rows + pad} route={route}"
    ld = r0 + rows + pad
    dth, t5 = law.dw_operands(fam, Kc, ld)
    dth_d, t5_d = dth.cuda(), t5.cuda()
    ws = _nan(lib.hp_hypernet_heads_dw_workspace_floats())
    off = 1 if route == law.DW_GEMM else 0
    runs = []
    for _ in range(2):
        buf = _nan(rows * law.K + 12)
        out = buf[4 + off:4 + off + rows * law.K].view(rows, law.K)
        assert law.rows_route(lib, t5_d.data_ptr(), out.data_ptr()) == route, tag
        call("hp_hypernet_heads_dw_rows", Kc, rows, r0, dth_d, ld, t5_d, out, ws, _stream(out))
        torch.cuda.synchronize()
        assert torch.isnan(buf[:4 + off]).all() and torch.isnan(buf[4 + off + rows * law.K:]).all(), f"{tag}: written outside dW_rows"
        runs.append(out.cpu())
    assert torch.equal(runs[0], runs[1]), f"{tag}: the second run differs"
    worst = _dw_check(tag, fam, runs[0], None, dth[:, r0:r0 + rows], t5)
    if fam == "R":
        print(f"HEADSLAW {tag} worst err/bound = {worst:.4f}")


def test_heads_dw_rows_of_no_rows_writes_nothing():
    from hyperpocket_amd._lib import call
    lib = _lib()
    dth, t5 = (x.cuda() for x in law.dw_operands("E", 7, 40))
    out, ws = _nan(64, law.K), _nan(lib.hp_hypernet_heads_dw_workspace_floats())
    call("hp_hypernet_heads_dw_rows", 7, 0, 5, dth, 40, t5, out, ws, _stream(out))
    call("hp_hypernet_heads_dw_rows", 7, 0, 40, dth, 40, t5, None, ws, _stream(out))
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all()


@pytest.mark.parametrize("fam", ["E", "R"])
@pytest.mark.parametrize("Kc,outs,pad,route,quirk", law.BWD_CASES)
def test_heads_dw_and_db_through_the_backward(fam, Kc, outs, pad, route, quirk):
    """hp_hypernet_backward at B = Kc with t5 and d theta supplied: the only way to the bias gradient and to the c0 == 0
    lanes that write it.  Fall-backs: the gradient one float past its boundary (one GEMM with row sums), heads not back to
    back (per-head GEMMs), grads->head_w[0] == NULL (column sums only); a NULL bias gradient beside the direct kernel."""
    from hyperpocket_amd._lib import call
    lib = _lib()
    tag = f"bwd {fam} Kc={Kc} heads={outs} pad={pad} route={route} {quirk or ''}"
    B, N = Kc, sum(outs)
    ld = N + pad
    dth, t5 = law.dw_operands(fam, Kc, ld)
    heads = _heads_dev("R", outs, "split" if quirk == "split" else None)
    w = _weights_struct("R", heads)
    tw, tb = _trunk_dev("R")
    t = torch.zeros(lib.hp_hypernet_saved_floats(B), device="cuda")
    o5 = lib.hp_hypernet_t5_offset(B)
    t[o5:o5 + B * law.K] = t5.cuda().view(-1)
    lat, dth_d = torch.zeros(B, law.IN_SIZE, device="cuda"), dth.cuda()
    worst = 0.0
    for with_db in ((True, False) if quirk is None and Kc in (7, 64) else (True,)):
        runs = []
        for _ in range(2):
            gr = law.HyperGrads()
            keep = [[_nan(*x.shape) for x in tw], [_nan(*x.shape) for x in tb]]
            for l in range(5):
                gr.trunk_w[l], gr.trunk_b[l] = keep[0][l].data_ptr(), keep[1][l].data_ptr()
            gap = 64 if quirk == "split" else 0
            lead = 5 if quirk == "out+1" else 4
            gw, gb = _nan(lead + N * law.K + gap * len(outs) + 4), _nan(4 + N + gap * len(outs))
            dws, dbs, ow, ob = [], [], lead, 4
            for h, n in enumerate(outs):
                dws.append(gw[ow:ow + n * law.K].view(n, law.K))
                dbs.append(gb[ob:ob + n])
                gr.head_w[h] = None if quirk == "skip" else dws[h].data_ptr()
                gr.head_b[h] = dbs[h].data_ptr() if with_db else None
                ow, ob = ow + n * law.K + gap, ob + n + gap
            got = law.plan(lib, B, w, gr, t.data_ptr(), None)
            assert (got[0], got[2]) == (0, route), f"{tag}: route {got}"
            ws = _nan(lib.hp_hypernet_backward_workspace_floats(B))
            call("hp_hypernet_backward", B, law.IN_SIZE, lat, ctypes.byref(w), t, dth_d, ld, ctypes.byref(gr), None, ws, _stream(ws))
            torch.cuda.synchronize()
            dW = None if quirk == "skip" else torch.cat([x.cpu() for x in dws])
            db = torch.cat([x.cpu() for x in dbs]) if with_db else None
            if quirk == "skip":
                assert torch.isnan(gw).all(), f"{tag}: a skipped dW was written"
            else:
                used = torch.zeros_like(gw, dtype=torch.bool)
                o = lead
                for n in outs:
                    used[o:o + n * law.K] = True
                    o += n * law.K + gap
                assert torch.isnan(gw[~used]).all() and torch.isfinite(gw[used]).all(), f"{tag}: dW written outside its rows, or not all of it"
            if not with_db:
                assert torch.isnan(gb).all(), f"{tag}: a NULL bias gradient was written"
            runs.append((dW, db))
        for a, b in zip(*runs):
            assert (a is None and b is None) or torch.equal(a, b), f"{tag}: the second run differs"
        worst = max(worst, _dw_check(tag, fam, runs[0][0], runs[0][1], dth[:, :N], t5))
    if fam == "R":
        print(f"HEADSLAW {tag} worst err/bound = {worst:.4f}")


# ================================================================================================ 3. hp_adam_step
def _adam_call(lib, n, p, g, m, v, step, scale, stream, hyper=law.HYPER):
    F = ctypes.c_float
    ptr = lambda x: P(x) if isinstance(x, int) else P(x.data_ptr())
    return lib.hp_adam_step(ctypes.c_long(n), ptr(p), ptr(g), ptr(m), ptr(v), F(hyper["lr"]), F(hyper["b1"]), F(hyper["b2"]),
                            F(hyper["eps"]), ctypes.c_int(step), F(scale), stream)


def _adam_case(n, step, scale, off=0):
    lib = _lib()
    tag = f"adam n={n} step={step} scale={scale} off={off}"
    fx = law.adam_fixture(n, scale)
    bufs = {k: _view(fx[k], off) for k in "pgmv"}
    d = {k: bufs[k][1] for k in "pgmv"}
    rc = _adam_call(lib, n, d["p"], d["g"], d["m"], d["v"], step, scale, _stream(d["p"]))
    torch.cuda.synchronize()
    assert rc == 0, (tag, rc)
    for k in "pgmv":
        _guards_untouched(*bufs[k], off, f"{tag} {k}")
    assert torch.equal(d["g"].cpu(), fx["g"]), f"{tag}: the gradient was written"
    got = {k: d[k].cpu() for k in "pmv"}
    if n == 0:
        return 0.0
    ref = law.adam64(fx["p"], fx["g"], fx["m"], fx["v"], step, scale, **law.HYPER)
    worst = law.check_adam(tag, got, ref, parts=True)
    z = fx["zero"]
    for k in "pmv":
        assert torch.equal(got[k][z], fx[k][z]), f"{tag}: {k} of the all-zero block changed"
    print(f"HEADSLAW {tag} worst err/bound = {max(worst.values()):.4f} (p {worst['p']:.4f} m {worst['m']:.4f} v {worst['v']:.4f})")
    return max(worst.values())


@pytest.mark.parametrize("n", law.ADAM_N)
def test_adam_step_sizes(n):
    """n around the float4 group and the 256-lane block (the scalar tail, one and two blocks) and 2 097 152 + 5: past the
    2048-block cap, so the grid-stride loop runs a second round — which ends in the scalar tail."""
    _adam_case(n, 1, 1.0)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", law.ADAM_VIEW_N)
def test_adam_step_views_off_the_16_byte_boundary(n, off):
    """All four arrays 0..3 floats past a boundary: a head launch of up to three elements, then the aligned body; the floats
    in front of and behind every view stay what they were."""
    _adam_case(n, 2, 0.5, off)


@pytest.mark.parametrize("scale", law.ADAM_SCALES)
@pytest.mark.parametrize("step", law.ADAM_STEPS)
def test_adam_step_bias_corrections_and_grad_scale(step, scale):
    _adam_case(1025, step, scale)


def test_adam_step_refuses_mismatched_phases():
    lib = _lib()
    fx = law.adam_fixture(1025)
    for odd in "pgmv":
        for off in (1, 2, 3):
            bufs = {k: _view(fx[k], off if k == odd else 0) for k in "pgmv"}
            before = {k: bufs[k][0].clone() for k in "pgmv"}
            rc = _adam_call(lib, 1025, *(bufs[k][1] for k in "pgmv"), 1, 1.0, _stream(before["p"]))
            torch.cuda.synchronize()
            assert rc == -1, (odd, off, rc)
            for k in "pgmv":
                assert torch.equal(bufs[k][0], before[k]), (odd, off, k)


# ================================================================================================ 4. fused dW + Adam
def _fused_call(lib, Kc, rows, r0, dth, ld, t5, W, m, v, step, cus, stream, hyper=law.HYPER):
    F = ctypes.c_float
    ptr = lambda x: P(x) if isinstance(x, int) else P(x.data_ptr())
    head = (Kc, rows, r0, ptr(dth), ld, ptr(t5), ptr(W), ptr(m), ptr(v), F(hyper["lr"]), F(hyper["b1"]), F(hyper["b2"]), F(hyper["eps"]), step)
    if cus is None:
        return lib.hp_hypernet_heads_dw_adam(*head, stream)
    return lib.hp_hypernet_heads_dw_adam_bg(*head, cus, stream)


def _fused_operands(rows, Kc, r0):
    """Family-E factors (the gradient is exact: the epilogue alone is under test; with more than one row the middle row's d theta
    is zero, so a whole row of g, m, v is 0) and the Adam fixture over the slice, inside buffers with two sentinel rows behind
    and r0 in front."""
    ld = r0 + rows + 3
    dth, t5 = law.dw_operands("E", Kc, ld)
    dth = dth.clone()
    if rows > 1:
        dth[:, r0 + rows // 2] = 0.0
    g = law.int_mm(dth[:, r0:r0 + rows].t(), t5)
    assert int(g.abs().max()) < 2 ** 24
    fx = law.adam_fixture(rows * law.K, g=g.float())
    full = {}
    for k, name in (("p", "W"), ("m", "m"), ("v", "v")):
        full[name] = torch.full((r0 + rows + 2, law.K), 123.0)
        full[name][r0:r0 + rows] = fx[k].view(rows, law.K)
    return ld, dth, t5, fx, full


@pytest.mark.parametrize("rows,Kc,pairs", law.FUSED_CASES)
def test_fused_heads_dw_adam_plain_and_persistent(rows, Kc, pairs):
    """hp_hypernet_heads_dw_adam and hp_hypernet_heads_dw_adam_bg with cus = 0 (the default 176), 1 and 3.  97 rows are 64 units:
    at cus = 1 one workgroup of 16 waves walks them in four rounds, at cus = 3 three walk them in two, the second ragged
    (16 of 48 waves have a unit).  All four agree bit for bit; the rows around the slice are untouched."""
    lib = _lib()
    for r0, step in pairs:
        tag = f"fused rows={rows} Kc={Kc} r0={r0} step={step}"
        ld, dth, t5, fx, full = _fused_operands(rows, Kc, r0)
        dth_d, t5_d = dth.cuda(), t5.cuda()
        ref = law.adam64(fx["p"], fx["g"], fx["m"], fx["v"], step, 1.0, **law.HYPER)
        results = []
        for cus in (None,) + law.FUSED_CUS:
            dev = {k: x.cuda() for k, x in full.items()}
            rc = _fused_call(lib, Kc, rows, r0, dth_d, ld, t5_d, dev["W"][r0:], dev["m"][r0:], dev["v"][r0:], step, cus, _stream(dth_d))
            torch.cuda.synchronize()
            assert rc == 0, (tag, cus, rc)
            out = {k: x.cpu() for k, x in dev.items()}
            for k in out:
                assert torch.equal(out[k][:r0], full[k][:r0]) and torch.equal(out[k][r0 + rows:], full[k][r0 + rows:]), \
                    f"{tag} cus={cus}: rows of {k} outside [r0, r0 + rows) changed"
            results.append(out)
        for cus, out in zip(law.FUSED_CUS, results[1:]):
            for k in out:
                assert torch.equal(out[k], results[0][k]), f"{tag}: {k} of the persistent pass (cus = {cus}) differs from the plain pass"
        got = {k: results[0][name][r0:r0 + rows].reshape(-1) for k, name in (("p", "W"), ("m", "m"), ("v", "v"))}
        worst = law.check_adam(tag, got, ref, parts=True)
        z = fx["zero"]
        assert int(z.sum()) >= (law.K if rows > 1 else 0) and int((~z).sum()) >= law.K // 2      # (an integer g is 0 by chance too)
        for k in "pmv":
            assert torch.equal(got[k][z], fx[k][z]), f"{tag}: {k} changed where g = m = v = 0"
        print(f"HEADSLAW {tag} worst err/bound = {max(worst.values()):.4f} (p {worst['p']:.4f} m {worst['m']:.4f} v {worst['v']:.4f})")


def test_fused_heads_dw_adam_refuses_misaligned_rows():
    lib = _lib()
    rows, Kc, r0 = 33, 8, 5
    ld, dth, t5, fx, full = _fused_operands(rows, Kc, r0)
    dth_d, t5_d = dth.cuda(), t5.cuda()
    for odd in ("W", "m", "v"):
        for cus in (None, 1):
            dev = {k: x.cuda() for k, x in full.items()}
            ptrs = {k: dev[k][r0:].data_ptr() + (4 if k == odd else 0) for k in dev}
            rc = _fused_call(lib, Kc, rows, r0, dth_d, ld, t5_d, ptrs["W"], ptrs["m"], ptrs["v"], 1, cus, _stream(dth_d))
            torch.cuda.synchronize()
            assert rc == -1, (odd, cus, rc)
            for k in dev:
                assert torch.equal(dev[k].cpu(), full[k]), (odd, cus, k)
    dev = {k: x.cuda() for k, x in full.items()}
    assert _fused_call(lib, Kc, 0, r0, dth_d, ld, t5_d, dev["W"], dev["m"], dev["v"], 1, None, _stream(dth_d)) == 0     # no rows
    torch.cuda.synchronize()
    assert all(torch.equal(dev[k].cpu(), full[k]) for k in dev)

"""Skinny layer programs (csrc/skinny.hip) phase by phase against fp64, at every batch size and width they serve.

The four program builders of csrc/model.hip (trunk forward / backward, encoder tail forward / backward) are driven through
the C ABI, so that every phase's input and output is a tensor the test can read: the saved trunk activations, dt[0..4] at the
head of the hypernetwork's backward workspace, the encoder's g / f / mu / lv, and dmu / dlv / dfc / dg in the encoder's
backward workspace (`_enc_bwd_offsets` mirrors enc_bwd_layout).

REFERENCE.  Each phase is recomputed in float64 on the CPU from the fp32 tensors that very phase consumed on the GPU (the
layer-l activation from the GPU's act(l-1), dt(l-1) from the GPU's dt(l) and the GPU's saved mask, ...): errors do not
compound and a ReLU sign that differs between fp32 and fp64 cannot flip a mask in the reference.

BOUND, per element, nothing to tune:  |got - want64| <= (L + 8) * 2^-24 * (|A| |W|^T + |bias|),  the right-hand side in fp64
from the same operands.  It is the gamma_L bound of a length-L fp32 sum in any order ((L + 8) u stands for gamma_(L+8): the two
differ by a factor 1 + O(1e-4) at L <= 1024, and every element measured sits far inside); the 8 covers the adds of up to four
slabs, the cross-wave reduce and the bias.  L is the contraction length: K for F, N for X (nh * N where the two heads of a VAE
tail are contracted into one dfc), M for W and its column sums; a FIN output carries the L of the phase that produced its
slabs.  A dropped or doubled product, a slab summed twice or a row read one off exceeds it.  The tiled-GEMM path
(hp_skinny_set_enabled(0)) is held to the same bound in every case; it has not violated it anywhere.

PATH.  hp_skinny_programs_run() counts the programs hp_skinny_run launched; every case asserts how far a forward and a
backward moved it, so no case passes by silently exercising the GEMM fallback.  Where it did not move, the results equal the
skinny-off run bit for bit.

YARDSTICK (measured on an MI355X over every case of this file, 803 tensors; profiles/r10_skinny_error_ratio.md).  Both
paths' maximum error against the fp64 reference of their own inputs, per tensor (the two backward paths start from the same
saved activations).  Worst e_skinny / e_gemm per task kind:
    F 1.23 (trunk act1, B = 1)   X 1.15 (trunk dt3, B = 1)   W 2.40 (the VAE tail's d mu_b, B = 64)   FIN 0.99 (the tail's dg)
W's worst is a bias gradient: task_w adds a column's 32 rows per half-wave one after the other where the GEMM path's column
sum adds them as a tree; both stay below a tenth of the bound.  No kind is above 4.  The assertion is
e_skinny <= r * e_gemm + 1e-7 * scale  with r twice the worst measured ratio, rounded up to one digit: 3, 3, 5, 2.

SENSITIVITY (checked once by perturbing csrc/skinny.hip): SrcChunk::store summing one slab fewer fails 64 of the 66 cases
(all but the two in which no program runs); task_w zeroing av from row M + 1 instead of row M fails every case with B < 64
that a backward program serves (44).  Dropping SrcChunk::store's `row >= M` zeroing fails NOTHING, and cannot: an MFMA
output row depends on its own A row only, and reduce_store never stores rows >= M, so the staged rows >= M are never observed.

Every buffer a call writes or uses as scratch is filled with NaN before the call (`t` with its slab area, both workspaces,
every output and gradient): whatever comes back must be finite, so a slab slot or a row that is read without having been
written in this call shows.  A second run on the same inputs must be bit-identical (the file claims no atomics).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KT = (64, 128, 512, 1024, 2048)          # trunk widths (csrc/model.hip kTrunk)
KE = (3, 64, 128, 256, 512, 512)         # encoder conv widths (kEnc)
HEAD = 64                                # ONE head of 64 rows: the heads are not under test

# e_skinny <= r * e_gemm + 1e-7 * scale, r per task kind = twice the worst measured ratio (1.23, 1.15, 2.40, 0.99: the
# module docstring, profiles/r10_skinny_error_ratio.md) rounded up to one digit.
_RATIO = {"F": 3.0, "X": 3.0, "W": 5.0, "FIN": 2.0}


# ------------------------------------------------------------------------------------------------ plumbing
def _lib():
    from hyperpocket_amd._lib import load_library
    lib = load_library()
    lib.hp_skinny_programs_run.restype = ctypes.c_long
    for n in ("hp_hypernet_saved_floats", "hp_hypernet_backward_workspace_floats", "hp_encoder_forward_workspace_floats",
              "hp_encoder_backward_workspace_floats"):
        getattr(lib, n).restype = ctypes.c_long
    return lib


class _Skinny:
    """with _Skinny(on): the switch set for the block, restored afterwards."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = _lib().hp_skinny_set_enabled(self.on)

    def __exit__(self, *a):
        _lib().hp_skinny_set_enabled(self.prev)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _mm(A, Bm, L, bias=None):
    """want = A . Bm (+ bias) in fp64 and the per-element bound (L + 8) u (|A| |Bm| + |bias|)."""
    A, Bm = A.double(), Bm.double()
    want, mag = A @ Bm, A.abs() @ Bm.abs()
    if bias is not None:
        want, mag = want + bias.double(), mag + bias.double().abs()
    return want, (L + 8) * U * mag


def _colsum(A, L):
    A = A.double()
    return A.sum(0), (L + 8) * U * A.abs().sum(0)


def _check(rec, kind, name, got, want, bound, tag):
    """Every element finite and inside its bound; records (max error, scale) for the yardstick."""
    assert got.shape == want.shape, (tag, name, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{tag} {name}: non-finite values (a slot read before it was written?)"
    err = (got.double() - want).abs()
    over = err - bound
    if (over > 0).any():
        i = int(over.argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(err.shape)))
        raise AssertionError(f"{tag} {name}{list(idx)}: |got - want64| = {err.flatten()[i]:.3e} > bound {bound.flatten()[i]:.3e} "
                             f"(got {got.flatten()[i]:.9e}, want {want.flatten()[i]:.9e}); {int((over > 0).sum())} elements over")
    rec[(kind, name)] = (err.max().item(), want.abs().max().item())


def _mask_agrees(tag, name, act, z64, bound):
    """The GPU's saved ReLU mask (act > 0) has the fp64 pre-activation's sign wherever |z64| exceeds the bound."""
    sure = z64.abs() > bound
    bad = sure & ((act > 0) != (z64 > 0))
    assert not bad.any(), f"{tag} {name}: {int(bad.sum())} mask entries differ from the fp64 sign outside the rounding bound"


def _yardstick(tag, rec_on, rec_off):
    for (kind, name), (e_s, scale) in rec_on.items():
        e_g = rec_off[(kind, name)][0]
        print(f"SKRATIO {tag} {kind} {name} e_skinny={e_s:.4e} e_gemm={e_g:.4e} scale={scale:.4e}")
    for (kind, name), (e_s, scale) in rec_on.items():
        e_g = rec_off[(kind, name)][0]
        assert e_s <= _RATIO[kind] * e_g + 1e-7 * scale, \
            f"{tag} {name} ({kind}): e_skinny {e_s:.3e} > {_RATIO[kind]} * e_gemm {e_g:.3e} + 1e-7 * {scale:.3e}"


def _same(tag, a, b, names=None):
    for k in (names or a.keys()):
        x, y = a[k], b[k]
        if isinstance(x, (list, tuple)):
            for i, (p, q) in enumerate(zip(x, y)):
                assert torch.equal(p, q), f"{tag}: {k}[{i}] differs"
        elif torch.is_tensor(x):
            assert torch.equal(x, y), f"{tag}: {k} differs"


# ------------------------------------------------------------------------------------------------ trunk
_TRUNK_W = {}


def _trunk_weights(in_size):
    """Trunk weights / biases and the one 64-row head, drawn once (layers 1..4 shared by every width)."""
    if "shared" not in _TRUNK_W:
        g = torch.Generator().manual_seed(1234)
        w = [None] + [torch.randn(KT[l], KT[l - 1], generator=g) / math.sqrt(KT[l - 1]) for l in range(1, 5)]
        b = [(torch.rand(KT[l], generator=g) - 0.5) * 0.1 for l in range(5)]
        hw = torch.randn(HEAD, 2048, generator=g) / math.sqrt(2048.0)
        hb = (torch.rand(HEAD, generator=g) - 0.5) * 0.1
        _TRUNK_W["shared"] = (w, b, hw, hb, [None] + [t.cuda() for t in w[1:]], [t.cuda() for t in b], hw.cuda(), hb.cuda())
    if in_size not in _TRUNK_W:
        g = torch.Generator().manual_seed(77 + in_size)
        w0 = torch.randn(KT[0], in_size, generator=g) / math.sqrt(in_size)
        _TRUNK_W[in_size] = (w0, w0.cuda())
    w, b, hw, hb, wd, bd, hwd, hbd = _TRUNK_W["shared"]
    w0, w0d = _TRUNK_W[in_size]
    return dict(w=[w0] + w[1:], b=b, hw=hw, hb=hb, wd=[w0d] + wd[1:], bd=bd, hwd=hwd, hbd=hbd)


def _hyper_struct(P):
    from hyperpocket_amd.ops import _HyperWeights
    w = _HyperWeights()
    for l in range(5):
        w.trunk_w[l], w.trunk_b[l] = P["wd"][l].data_ptr(), P["bd"][l].data_ptr()
    w.n_heads = 1
    w.head_out[0], w.head_w[0], w.head_b[0] = HEAD, P["hwd"].data_ptr(), P["hbd"].data_ptr()
    return w


def _trunk_forward(B, in_size, P, latent_d, skinny):
    from hyperpocket_amd._lib import call, current_stream
    lib = _lib()
    w = _hyper_struct(P)
    t = _nan(lib.hp_hypernet_saved_floats(B))
    theta = _nan(B, HEAD)
    with _Skinny(skinny):
        c0 = lib.hp_skinny_programs_run()
        call("hp_hypernet_forward", B, in_size, latent_d, ctypes.byref(w), t, theta, HEAD, current_stream(t.device))
        progs = lib.hp_skinny_programs_run() - c0
    torch.cuda.synchronize()
    acts, off = [], 0
    for l in range(5):
        acts.append(t[off:off + B * KT[l]].view(B, KT[l]).cpu())
        off += B * KT[l]
    return dict(t=t, act=acts, theta=theta.cpu(), progs=progs)


def _trunk_backward(B, in_size, P, latent_d, gtheta_d, fwd, skinny, want_latent=True):
    from hyperpocket_amd._lib import call, current_stream
    from hyperpocket_amd.ops import _HyperGrads
    lib = _lib()
    w, gr = _hyper_struct(P), _HyperGrads()
    dW = [_nan(*P["w"][l].shape) for l in range(5)]
    db = [_nan(KT[l]) for l in range(5)]
    dhw, dhb = _nan(HEAD, 2048), _nan(HEAD)
    for l in range(5):
        gr.trunk_w[l], gr.trunk_b[l] = dW[l].data_ptr(), db[l].data_ptr()
    gr.head_w[0], gr.head_b[0] = dhw.data_ptr(), dhb.data_ptr()
    glat = _nan(B, in_size) if want_latent else None
    ws = _nan(lib.hp_hypernet_backward_workspace_floats(B))
    with _Skinny(skinny):
        c0 = lib.hp_skinny_programs_run()
        call("hp_hypernet_backward", B, in_size, latent_d, ctypes.byref(w), fwd["t"], gtheta_d, HEAD, ctypes.byref(gr), glat, ws,
             current_stream(ws.device))
        progs = lib.hp_skinny_programs_run() - c0
    torch.cuda.synchronize()
    dt, off = [], 0
    for l in range(5):
        dt.append(ws[off:off + B * KT[l]].view(B, KT[l]).cpu())
        off += B * KT[l]
    return dict(dt=dt, dW=[x.cpu() for x in dW], db=[x.cpu() for x in db], glat=None if glat is None else glat.cpu(), progs=progs)


def _trunk_forward_parity(tag, P, latent, fwd, served):
    rec = {}
    for l in range(5):
        inp = latent if l == 0 else fwd["act"][l - 1]
        z, bound = _mm(inp, P["w"][l].t(), inp.shape[1], P["b"][l])
        # (the last layer's slabs are finished by a FIN op; the layers below by the next layer's readers)
        kind = "FIN" if l == 4 else "F"
        _check(rec, kind, f"act{l}", fwd["act"][l], torch.relu(z) if l < 4 else z, bound, tag)
        if l < 4:
            _mask_agrees(tag, f"act{l}", fwd["act"][l], z, bound)
    return rec


def _trunk_backward_parity(tag, P, latent, fwd, bwd):
    rec = {}
    B = latent.shape[0]
    assert all(torch.isfinite(d).all() for d in bwd["dt"]), f"{tag}: dt holds non-finite values"
    for l in range(4, -1, -1):
        below = latent if l == 0 else fwd["act"][l - 1]
        dt = bwd["dt"][l]
        want, bound = _mm(dt.t(), below, B)
        _check(rec, "W", f"dW{l}", bwd["dW"][l], want, bound, tag)
        want, bound = _colsum(dt, B)
        _check(rec, "W", f"db{l}", bwd["db"][l], want, bound, tag)
        if l > 0:
            want, bound = _mm(dt, P["w"][l], KT[l])
            mask = below > 0                      # the GPU's saved activation, as the kernel reads it
            _check(rec, "X", f"dt{l - 1}", bwd["dt"][l - 1], want * mask, bound, tag)
            assert (bwd["dt"][l - 1][~mask] == 0).all(), f"{tag} dt{l - 1}: a masked entry is not zero"
        elif bwd["glat"] is not None:
            want, bound = _mm(dt, P["w"][0], KT[0])
            _check(rec, "FIN", "grad_latent", bwd["glat"], want, bound, tag)
    return rec


def _trunk_case(B, in_size, fwd_progs, bwd_progs, no_latent=False):
    tag = f"trunk B={B} in={in_size}"
    P = _trunk_weights(in_size)
    g = torch.Generator().manual_seed(B * 4099 + in_size)
    latent = torch.randn(B, in_size, generator=g)
    gtheta = torch.randn(B, HEAD, generator=g)
    latent_d, gtheta_d = latent.cuda(), gtheta.cuda()

    on = _trunk_forward(B, in_size, P, latent_d, 1)
    assert on["progs"] == fwd_progs, f"{tag}: the forward launched {on['progs']} layer programs, expected {fwd_progs}"
    again = _trunk_forward(B, in_size, P, latent_d, 1)
    _same(tag + " forward, run to run", on, again, ("act", "theta"))
    off = _trunk_forward(B, in_size, P, latent_d, 0)
    assert off["progs"] == 0, tag
    rec_on = _trunk_forward_parity(tag + " forward", P, latent, on, True)
    rec_off = _trunk_forward_parity(tag + " forward (GEMM path)", P, latent, off, False)
    if on["progs"]:
        _yardstick(tag + " forward", rec_on, rec_off)
    else:
        _same(tag + " forward fell back: must be the GEMM path's result", on, off, ("act", "theta"))

    # both backward paths start from the SAME saved activations (the skinny-on forward's)
    bon = _trunk_backward(B, in_size, P, latent_d, gtheta_d, on, 1)
    assert bon["progs"] == bwd_progs, f"{tag}: the backward launched {bon['progs']} layer programs, expected {bwd_progs}"
    bagain = _trunk_backward(B, in_size, P, latent_d, gtheta_d, on, 1)
    _same(tag + " backward, run to run", bon, bagain, ("dt", "dW", "db", "glat"))
    boff = _trunk_backward(B, in_size, P, latent_d, gtheta_d, on, 0)
    assert boff["progs"] == 0, tag
    assert torch.equal(bon["dt"][4], boff["dt"][4]), f"{tag}: dt4 (the heads' dX, not a layer program) differs between the paths"
    rec_on = _trunk_backward_parity(tag + " backward", P, latent, on, bon)
    rec_off = _trunk_backward_parity(tag + " backward (GEMM path)", P, latent, on, boff)
    if bon["progs"]:
        _yardstick(tag + " backward", rec_on, rec_off)
    else:
        _same(tag + " backward fell back: must be the GEMM path's result", bon, boff, ("dt", "dW", "db", "glat"))

    if no_latent:
        # grad_latent == NULL: a FIN op for dt0 stands in for the last X op; every other output is the with-latent run's
        bnl = _trunk_backward(B, in_size, P, latent_d, gtheta_d, on, 1, want_latent=False)
        assert bnl["progs"] == bwd_progs, f"{tag}: without grad_latent the backward launched {bnl['progs']} programs"
        _same(tag + " backward without grad_latent", bon, bnl, ("dt", "dW", "db"))
        bnl2 = _trunk_backward(B, in_size, P, latent_d, gtheta_d, on, 1, want_latent=False)
        _same(tag + " backward without grad_latent, run to run", bnl, bnl2, ("dt", "dW", "db"))


@pytest.mark.parametrize("B", [1, 2, 31, 32, 33, 63, 64])
def test_trunk_programs_batch_sweep(B):
    """in_size 256 at every batch size where the 32-row MFMA tiles can mishandle rows (rows >= M re-read row M-1 and are
    zeroed after staging; task_w zeroes av for 2s+h >= M; FIN has M*N/1024 tasks), with and without grad_latent."""
    _trunk_case(B, 256, 1, 1, no_latent=True)


@pytest.mark.parametrize("in_size", [32, 64, 128, 512, 1024])
@pytest.mark.parametrize("B", [1, 33, 64])
def test_trunk_programs_width_sweep(B, in_size):
    """Layer 0 at every template instance: 32 = a single range with the producer's direct bias + ReLU epilogue, 64 =
    task_f<2,1> and a two-slab source, 128 = four 32-deep ranges, 512 / 1024 = 128-deep chunks (1024: two per range)."""
    _trunk_case(B, in_size, 1, 1)


@pytest.mark.parametrize("B,in_size,fwd_progs,bwd_progs", [(33, 96, 0, 1), (33, 100, 0, 0), (65, 256, 0, 0)])
def test_trunk_programs_fallback(B, in_size, fwd_progs, bwd_progs):
    """Shapes the builders refuse: in_size 96 has no power-of-two range for the forward's layer 0 (CL = 48) while the
    backward's X / W ops over it are served; in_size 100 and B = 65 fall back in both directions.  Whatever ran meets the
    same parity, and a direction that fell back equals the skinny-off run bit for bit (nothing half-launched)."""
    _trunk_case(B, in_size, fwd_progs, bwd_progs)


# ------------------------------------------------------------------------------------------------ encoder tail
_ENC_W = {}


def _enc_params(out_size, vae, seed=0):
    """conv_w x5, conv_b x5, fc_w, fc_b, mu_w, mu_b[, std_w, std_b] (CPU); conv stack and fc drawn once per seed."""
    if ("conv", seed) not in _ENC_W:
        g = torch.Generator().manual_seed(4321 + seed)
        cw = [torch.randn(KE[l + 1], KE[l], generator=g) * math.sqrt(2.0 / KE[l]) for l in range(5)]
        cb = [(torch.rand(KE[l + 1], generator=g) - 0.5) * 0.1 for l in range(5)]
        fc_w = torch.randn(512, 512, generator=g) / math.sqrt(512.0)
        fc_b = (torch.rand(512, generator=g) - 0.5) * 0.1
        _ENC_W[("conv", seed)] = cw + cb + [fc_w, fc_b]
    key = ("head", seed, out_size)
    if key not in _ENC_W:
        g = torch.Generator().manual_seed(99 + 7 * seed + out_size)
        _ENC_W[key] = [torch.randn(out_size, 512, generator=g) / math.sqrt(512.0), (torch.rand(out_size, generator=g) - 0.5) * 0.1,
                       torch.randn(out_size, 512, generator=g) / math.sqrt(512.0), (torch.rand(out_size, generator=g) - 0.5) * 0.1]
    return _ENC_W[("conv", seed)] + (_ENC_W[key] if vae else _ENC_W[key][:2])


def _enc_bwd_offsets(B, out_size):
    """dmu, dlv, dfc, dg inside the hp_encoder_backward workspace (csrc/model.hip enc_bwd_layout)."""
    up4 = lambda n: (n + 3) // 4 * 4
    Rc = B * 512
    off = up4(Rc * 3) + 2 * sum(up4(Rc * KE[l]) for l in range(1, 5))
    o = {}
    for name, n in (("dmu", B * out_size), ("dlv", B * out_size), ("tmp", B * 512), ("dfc", B * 512), ("dg", B * 512)):
        o[name] = (off, n)
        off += up4(n)
    return o


def _enc_forward(B, Np, out_size, vae, params_d, x_d, eps_d, skinny):
    from hyperpocket_amd._lib import call, current_stream
    from hyperpocket_amd.ops import _encoder_struct
    lib = _lib()
    w = _encoder_struct(params_d)
    argidx = torch.full((B, 512), -1, dtype=torch.int32, device="cuda")
    g, f, mu = _nan(B, 512), _nan(B, 512), _nan(B, out_size)
    lv, z, explv = (_nan(B, out_size), _nan(B, out_size), _nan(B, out_size)) if vae else (None, None, None)
    ws = _nan(lib.hp_encoder_forward_workspace_floats(B, Np))
    with _Skinny(skinny):
        c0 = lib.hp_skinny_programs_run()
        call("hp_encoder_forward", B, Np, x_d, ctypes.byref(w), out_size, int(vae), eps_d if vae else None, argidx, g, f, mu, lv, z,
             explv, ws, current_stream(ws.device))
        progs = lib.hp_skinny_programs_run() - c0
    torch.cuda.synchronize()
    dev = dict(argidx=argidx, g=g, f=f, mu=mu, lv=lv, ws=ws)
    out = dict(dev=dev, progs=progs, argidx=argidx.cpu(), g=g.cpu(), f=f.cpu(), mu=mu.cpu())
    if vae:
        out.update(lv=lv.cpu(), z=z.cpu(), explv=explv.cpu())
    return out


def _enc_backward(B, Np, out_size, vae, params_d, x_d, eps_d, fwd, grads_d, skinny):
    from hyperpocket_amd._lib import call, current_stream
    from hyperpocket_amd.ops import _encoder_struct
    lib = _lib()
    w = _encoder_struct(params_d)
    out = [_nan(*p.shape) for p in params_d]
    gr = _encoder_struct(out)
    ws = _nan(lib.hp_encoder_backward_workspace_floats(B, out_size))
    d = fwd["dev"]
    gout, gmu, gexplv = grads_d
    with _Skinny(skinny):
        c0 = lib.hp_skinny_programs_run()
        call("hp_encoder_backward", B, Np, x_d, ctypes.byref(w), out_size, int(vae), eps_d if vae else None, d["argidx"], d["g"],
             d["f"], d["lv"], gout, gmu, gexplv, ctypes.byref(gr), ws, d["ws"], 1, current_stream(ws.device))
        progs = lib.hp_skinny_programs_run() - c0
    torch.cuda.synchronize()
    o = _enc_bwd_offsets(B, out_size)
    take = lambda name, cols: ws[o[name][0]:o[name][0] + o[name][1]].view(B, cols).cpu()
    res = dict(progs=progs, grads=[t.cpu() for t in out], dfc=take("dfc", 512), dg=take("dg", 512))
    if vae:
        res.update(dmu=take("dmu", out_size), dlv=take("dlv", out_size))
    else:
        res.update(dmu=gout.cpu(), dlv=None)
    return res


def _enc_forward_parity(tag, params, vae, fwd):
    rec = {}
    fc_w, fc_b, mu_w, mu_b = params[10:14]
    z, bound = _mm(fwd["g"], fc_w.t(), 512, fc_b)
    _check(rec, "F", "f", fwd["f"], torch.relu(z), bound, tag)
    _mask_agrees(tag, "f", fwd["f"], z, bound)
    want, bound = _mm(fwd["f"], mu_w.t(), 512, mu_b)
    _check(rec, "FIN", "mu", fwd["mu"], want, bound, tag)
    if vae:
        want, bound = _mm(fwd["f"], params[14].t(), 512, params[15])
        _check(rec, "FIN", "lv", fwd["lv"], want, bound, tag)
        assert torch.isfinite(fwd["z"]).all() and torch.isfinite(fwd["explv"]).all(), tag
    return rec


def _enc_backward_parity(tag, params, vae, fwd, bwd):
    rec = {}
    B, out_size = fwd["mu"].shape
    fc_w, mu_w = params[10], params[12]
    g, f, gr = fwd["g"], fwd["f"], bwd["grads"]
    dmu, dlv, dfc = bwd["dmu"], bwd["dlv"], bwd["dfc"]
    assert all(torch.isfinite(t).all() for t in gr), f"{tag}: a parameter gradient holds non-finite values"
    assert torch.isfinite(dmu).all() and (dlv is None or torch.isfinite(dlv).all()), tag
    for name, d, iw, ib in (("mu", dmu, 12, 13), ("std", dlv, 14, 15)):
        if d is None:
            continue
        want, bound = _mm(d.t(), f, B)
        _check(rec, "W", f"d{name}_w", gr[iw], want, bound, tag)
        want, bound = _colsum(d, B)
        _check(rec, "W", f"d{name}_b", gr[ib], want, bound, tag)
    # dfc = (dmu . mu_w + dlv . std_w) * (f > 0): ONE contraction over the heads' concatenated columns, length nh * out
    nh = 2 if vae else 1
    want, bound = _mm(dmu, mu_w, nh * out_size)
    if vae:
        w2, b2 = _mm(dlv, params[14], nh * out_size)
        want, bound = want + w2, bound + b2
    mask = f > 0
    _check(rec, "X", "dfc", dfc, want * mask, bound, tag)
    assert (dfc[~mask] == 0).all(), f"{tag} dfc: a masked entry is not zero"
    want, bound = _mm(dfc.t(), g, B)
    _check(rec, "W", "dfc_w", gr[10], want, bound, tag)
    want, bound = _colsum(dfc, B)
    _check(rec, "W", "dfc_b", gr[11], want, bound, tag)
    want, bound = _mm(dfc, fc_w, 512)
    _check(rec, "FIN", "dg", bwd["dg"], want, bound, tag)
    return rec


def _grad_close(got, want, tol):
    got, want = got.double(), want.double()
    scale = max(want.abs().max().item(), 1e-30)
    err = (got - want).abs().max().item()
    assert err <= tol * scale, f"max err {err:.3e} vs scale {scale:.3e}"


def _enc_case(B, Np, out_size, vae, fwd_progs, bwd_progs):
    tag = f"encoder {'vae' if vae else 'plain'} B={B} Np={Np} out={out_size}"
    params = _enc_params(out_size, vae)
    params_d = [p.cuda() for p in params]
    g = torch.Generator().manual_seed(B * 8191 + out_size * 3 + int(vae))
    x = torch.rand(B, Np, 3, generator=g) * 2 - 1
    eps = torch.randn(B, out_size, generator=g)
    grads = [torch.randn(B, out_size, generator=g) for _ in range(3)]
    x_d, eps_d = x.cuda(), eps.cuda()
    grads_d = [t.cuda() for t in grads] if vae else [grads[0].cuda(), None, None]

    on = _enc_forward(B, Np, out_size, vae, params_d, x_d, eps_d, 1)
    assert on["progs"] == fwd_progs, f"{tag}: the forward launched {on['progs']} layer programs, expected {fwd_progs}"
    names = ("argidx", "g", "f", "mu") + (("lv", "z", "explv") if vae else ())
    again = _enc_forward(B, Np, out_size, vae, params_d, x_d, eps_d, 1)
    _same(tag + " forward, run to run", on, again, names)
    off = _enc_forward(B, Np, out_size, vae, params_d, x_d, eps_d, 0)
    assert off["progs"] == 0, tag
    _same(tag + ": the conv stack does not depend on the tail's path", on, off, ("argidx", "g"))   # the tail's reference starts from this g
    assert torch.isfinite(on["g"]).all() and (on["argidx"] >= 0).all() and (on["argidx"] < Np).all(), tag
    rec_on = _enc_forward_parity(tag + " forward", params, vae, on)
    rec_off = _enc_forward_parity(tag + " forward (GEMM path)", params, vae, off)
    if on["progs"]:
        _yardstick(tag + " forward", rec_on, rec_off)
    else:
        _same(tag + " forward fell back: must be the GEMM path's result", on, off, names)

    # both backward paths start from the SAME forward state (the skinny-on forward's)
    bon = _enc_backward(B, Np, out_size, vae, params_d, x_d, eps_d, on, grads_d, 1)
    assert bon["progs"] == bwd_progs, f"{tag}: the backward launched {bon['progs']} layer programs, expected {bwd_progs}"
    bagain = _enc_backward(B, Np, out_size, vae, params_d, x_d, eps_d, on, grads_d, 1)
    _same(tag + " backward, run to run", bon, bagain, ("grads", "dfc", "dg", "dmu"))
    boff = _enc_backward(B, Np, out_size, vae, params_d, x_d, eps_d, on, grads_d, 0)
    assert boff["progs"] == 0, tag
    assert torch.equal(bon["dmu"], boff["dmu"]), tag
    rec_on = _enc_backward_parity(tag + " backward", params, vae, on, bon)
    rec_off = _enc_backward_parity(tag + " backward (GEMM path)", params, vae, on, boff)
    if bon["progs"]:
        _yardstick(tag + " backward", rec_on, rec_off)
        # dg through the layer it feeds: the conv5 weight gradient, skinny on against off (the suite's grad_close)
        _grad_close(bon["grads"][4], boff["grads"][4], tol=2e-5)
    else:
        _same(tag + " backward fell back: must be the GEMM path's result", bon, boff, ("grads", "dfc", "dg"))


def _np_for(B):
    # the slabs live in the h5 slot behind the fused max-pool's partials: small B*Np leaves no room and falls back
    return 1024 if B <= 2 else 128


@pytest.mark.parametrize("vae", [True, False], ids=["vae", "plain"])
@pytest.mark.parametrize("B", [1, 2, 31, 32, 33, 63, 64])
def test_encoder_tail_programs_batch_sweep(B, vae):
    """out_size 128 at every batch size around the 32-row tiles; Np chosen so that the counter confirms the skinny tail ran."""
    _enc_case(B, _np_for(B), 128, vae, 1, 1)


@pytest.mark.parametrize("vae", [True, False], ids=["vae", "plain"])
@pytest.mark.parametrize("out_size", [32, 64, 256, 512])
@pytest.mark.parametrize("B", [1, 33, 64])
def test_encoder_tail_programs_width_sweep(B, out_size, vae):
    """Head widths 32 .. 512: one to sixteen strips per head in the forward; in the backward one range per head (VAE at 32:
    nh * S == 2, task_x<2,1>) up to 256-deep ranges (VAE at 512).  The plain encoder's backward at 32 would be a single
    range, which applies no mask: it is not built and falls back."""
    _enc_case(B, _np_for(B), out_size, vae, 1, 0 if (out_size == 32 and not vae) else 1)


@pytest.mark.parametrize("vae", [True, False], ids=["vae", "plain"])
def test_encoder_tail_programs_fallback_width_96(vae):
    """out_size 96: the forward is served (three strips per head), the backward's ranges would be 48 deep — refused by
    hp_skinny_run before its first launch, so the GEMM launches give the skinny-off result bit for bit."""
    _enc_case(33, 128, 96, vae, 1, 0)


def test_encoder_pair_program_equals_two_single_programs():
    """EncoderPairFunction (both tails in ONE program per direction; the plain encoder writes mu into, and reads d mu from,
    a column block of the latent: the strided mu_ld / dmu_ld operands) against two EncoderFunction calls, bit for bit: every
    output and every parameter gradient, the conv stack's included (B = 33 is past the 20 row ranges of the fused backward's
    dW launch: the pair and the single call must split the critical rows alike for their partial sums to add up alike)."""
    from hyperpocket_amd.ops import EncoderFunction, EncoderPairFunction
    lib = _lib()
    B, Np, out_size = 33, 128, 64
    g = torch.Generator().manual_seed(5)
    x0, x1 = (torch.rand(B, Np, 3, generator=g) * 2 - 1).cuda(), (torch.rand(B, Np, 3, generator=g) * 2 - 1).cuda()
    eps = torch.randn(B, out_size, generator=g).cuda()
    glat, gmu, gexplv = torch.randn(B, 2 * out_size, generator=g).cuda(), torch.randn(B, out_size, generator=g).cuda(), \
        torch.randn(B, out_size, generator=g).cuda()

    def leaves(seed, vae):
        return [p.cuda().requires_grad_(True) for p in _enc_params(out_size, vae, seed)]

    with _Skinny(1):
        p0, p1 = leaves(0, True), leaves(1, False)
        c0 = lib.hp_skinny_programs_run()
        latent, mu, explv = EncoderPairFunction.apply(x0, eps, x1, out_size, *p0, *p1)
        c1 = lib.hp_skinny_programs_run()
        ((latent * glat).sum() + (mu * gmu).sum() + (explv * gexplv).sum()).backward()
        c2 = lib.hp_skinny_programs_run()
        assert (c1 - c0, c2 - c1) == (1, 1), f"the pair ran {c1 - c0} forward and {c2 - c1} backward programs, expected one shared each"

        q0, q1 = leaves(0, True), leaves(1, False)
        z_s, mu_s, explv_s = EncoderFunction.apply(x0, eps, out_size, *q0)
        real_s = EncoderFunction.apply(x1, None, out_size, *q1)
        c3 = lib.hp_skinny_programs_run()
        ((z_s * glat[:, :out_size]).sum() + (real_s * glat[:, out_size:]).sum() + (mu_s * gmu).sum() + (explv_s * gexplv).sum()).backward()
        c4 = lib.hp_skinny_programs_run()
        assert (c3 - c2, c4 - c3) == (2, 2), "the single-encoder calls must run one program each per direction"
    torch.cuda.synchronize()
    assert torch.equal(latent[:, :out_size], z_s) and torch.equal(latent[:, out_size:], real_s)
    assert torch.equal(mu, mu_s) and torch.equal(explv, explv_s)
    for i, (a, b) in enumerate(zip(p0 + p1, q0 + q1)):
        assert torch.isfinite(a.grad).all(), i
        assert torch.equal(a.grad, b.grad), f"parameter {i}: the pair's gradient differs from the single call's"

"""The encoder's law and the drivers of its C entry points, shared by tests/test_encoder_routes_gpu.py and
tests/test_encoder_plan_host.py.

Law: model/encoder.py:14-53 restated over torch ops on a flat parameter list (the order of the C entry points: five conv
weights (Cout, Cin), five conv biases, fc, mu[, std]) — any dtype, eps handed in instead of drawn; in float64 it is the
yardstick, its autograd the yardstick of the backward.

Drivers: hp_encoder_forward / hp_encoder_backward_ld and the pair calls through the C ABI over buffers the tests own, so a
test decides where each buffer lies (one arena carved in either encoder order), how grad_out is strided, whether the
workspaces sit on 16-byte boundaries and which upstream gradients exist.

Route tables: the case tables of the GPU suite and the check, through hp_encoder_plan, that they reach every combination
of launch routes the dispatch of csrc/model.hip can produce.
"""
import contextlib
import ctypes

import torch

WIDTHS = (3, 64, 128, 256, 512, 512)


# ------------------------------------------------------------------------------------------------ the law
def make_params(seed, out_size, is_vae):
    """A seeded encoder's parameters (xavier weights as the training setup draws them, biases off zero so that their paths
    and gradients are exercised) as the flat fp32 list of the C entry points, on the CPU."""
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.encoder import Encoder
    torch.manual_seed(seed)
    enc = Encoder({"output_size": out_size, "use_bias": True, "relu_slope": 0.2}, is_vae=is_vae).apply(weights_init)
    for p in enc.parameters():
        if p.dim() == 1:
            torch.nn.init.uniform_(p, -0.1, 0.1)
    return [(p.detach().reshape(p.shape[0], -1) if p.dim() == 3 else p.detach()).clone().contiguous() for p in enc._params()]


def encoder_law(params, x, eps=None, arg=None, masks=None):
    """model/encoder.py:43-53 over torch ops: x (B, Np, 3); returns a dict with h4 (B, Np, 512), h5, the pooled g and its
    arg-max, f, mu and — for 16 parameters — lv, explv = exp(lv) (what the reference returns as "logvar"), z = eps explv + mu.
    arg (B, 512): the pool takes these rows instead of choosing (the same function wherever they attain the maximum; it fixes
    which of two nearly equal points carries a channel's gradient).  masks: four (B, Np, C_l) boolean tensors — layer l's ReLU
    passes where its mask says instead of where its own pre-activation is positive (the same function except where a
    pre-activation lies within rounding of zero; it fixes on which side of the kink such a value is differentiated)."""
    h = x
    out = {}
    for l in range(5):
        h = h @ params[l].t() + params[5 + l]
        if l < 4:
            h = torch.relu(h) if masks is None else h * masks[l].to(h.dtype)
        if l == 3:
            out["h4"] = h
    out["h5"] = h
    if arg is None:
        out["g"], out["arg"] = h.max(dim=1)
    else:
        out["g"], out["arg"] = torch.gather(h, 1, arg.long().unsqueeze(1)).squeeze(1), arg
    out["f"] = torch.relu(out["g"] @ params[10].t() + params[11])
    out["mu"] = out["f"] @ params[12].t() + params[13]
    if len(params) == 16:
        out["lv"] = out["f"] @ params[14].t() + params[15]
        out["explv"] = torch.exp(out["lv"])
        out["z"] = eps * out["explv"] + out["mu"]
    return out


# upstream gradients in the mixed form of test_encoder_backward_chain_on_the_f16_pipe...: sum_i (out_i * (i + 1.5)).sum() over
# (z, mu, exp(logvar)) of a VAE encoder / (mu,) of a plain one
UPSTREAM = (1.5, 2.5, 3.5)


def law_gradients(params, x, eps=None, use=(True, True, True), gscale=1.0, arg=None, masks=None):
    """float64 autograd of the law: d/d params of gscale * (1.5 z.sum() + 2.5 mu.sum() + 3.5 explv.sum()) (VAE; `use` drops
    terms) or of gscale * 1.5 mu.sum() (plain); arg and masks as in encoder_law.  Returns the float64 gradients in parameter order."""
    P = [p.detach().double().cpu().requires_grad_(True) for p in params]
    o = encoder_law(P, x.detach().double().cpu(), None if eps is None else eps.detach().double().cpu(),
                    None if arg is None else arg.detach().cpu(), None if masks is None else [m.cpu() for m in masks])
    outs = (o["z"], o["mu"], o["explv"]) if len(P) == 16 else (o["mu"],)
    loss = sum((t * c).sum() for t, c, u in zip(outs, UPSTREAM, use) if u) * gscale
    return list(torch.autograd.grad(loss, P))


# ------------------------------------------------------------------------------------------------ buffers
def fresh(numel, dtype=torch.float32):
    return torch.empty((numel,), dtype=dtype, device="cuda")


class Arena:
    """One device allocation carved front to back in 256-byte steps: whoever asks first lies lowest."""

    def __init__(self, nbytes):
        self.buf = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        self.off = 0

    def __call__(self, numel, dtype=torch.float32):
        size = torch.empty((), dtype=dtype).element_size() * numel
        assert self.off + size <= self.buf.numel(), "arena too small"
        t = self.buf[self.off:self.off + size].view(dtype)
        self.off += (size + 255) // 256 * 256
        return t


def _filled(alloc, shape, dtype=torch.float32, like=None):
    """A buffer from `alloc`: a copy of `like`, else NaN (floats) / -1 (ints) so that what a call leaves unwritten shows."""
    n = 1
    for s in shape:
        n *= s
    t = alloc(n, dtype).view(*shape)
    if like is not None:
        t.copy_(like)
    elif dtype == torch.float32:
        t.fill_(float("nan"))
    else:
        t.fill_(-1)
    return t


def _off16(alloc, numel, off):
    """`numel` floats that start `off` floats past a 16-byte boundary."""
    return alloc(numel + 4)[off:off + numel]


def _lib():
    from hyperpocket_amd import _lib as L
    return L


def fwd_ws_floats(B, Np):
    from hyperpocket_amd import ops
    return ops._long_fn("hp_encoder_forward_workspace_floats", B, Np)


def bwd_ws_floats(B, out_size):
    from hyperpocket_amd import ops
    return ops._long_fn("hp_encoder_backward_workspace_floats", B, out_size)


@contextlib.contextmanager
def switches(split=1, presplit=1, chain16=None, skinny=None):
    """The library's process-wide route switches for the block; restored on exit."""
    lib = _lib().load_library()
    was = [("hp_conv_split_set", lib.hp_conv_split_set(int(split))), ("hp_conv_presplit_set", lib.hp_conv_presplit_set(int(presplit)))]
    if chain16 is not None:
        was.append(("hp_encoder_backward_set_chain_f16", lib.hp_encoder_backward_set_chain_f16(int(chain16))))
    if skinny is not None:
        was.append(("hp_skinny_set_enabled", lib.hp_skinny_set_enabled(int(skinny))))
    try:
        yield
    finally:
        for name, prev in was:
            getattr(lib, name)(prev)


# the three conv routes of the forward as switch settings (split, presplit); "r3" is round 3's route: split-f16 kernels fed
# fp32 activations at whole tiles too
CONV_ROUTES = {"default": (1, 1), "r3": (1, 0), "fp32": (0, 1)}


# ------------------------------------------------------------------------------------------------ drivers
class Side:
    """One encoder's device buffers for the C calls: inputs, parameters, outputs, workspaces, gradients."""

    def __init__(self, B, Np, out_size, x, params, eps, alloc=fresh, latent=None):
        from hyperpocket_amd import ops
        self.B, self.Np, self.out, self.vae = B, Np, out_size, len(params) == 16
        self.x = _filled(alloc, (B, Np, 3), like=x)
        self.params = [_filled(alloc, tuple(p.shape), like=p) for p in params]
        self.eps = _filled(alloc, (B, out_size), like=eps) if self.vae else None
        self.argidx = _filled(alloc, (B, 512), torch.int32)
        self.g, self.f = _filled(alloc, (B, 512)), _filled(alloc, (B, 512))
        self.lv = self.z = self.explv = None
        self.out_ld = 0
        if latent is None:
            self.mu = _filled(alloc, (B, out_size))
            if self.vae:
                self.z = _filled(alloc, (B, out_size))
        else:                                                  # the pair's latent [z | real mu], as EncoderPairFunction lays it out
            self.out_ld = 2 * out_size
            if self.vae:
                self.mu, self.z = _filled(alloc, (B, out_size)), latent
            else:
                self.mu = latent[:, out_size:]
        if self.vae:
            self.lv, self.explv = _filled(alloc, (B, out_size)), _filled(alloc, (B, out_size))
        self.ws = _filled(alloc, (fwd_ws_floats(B, Np),))
        self.w = ops._encoder_struct(self.params)
        self.grads = self.gr = self.bws = None

    def io(self):
        from hyperpocket_amd import ops
        e = ops._EncoderIO()
        e.x, e.w, e.eps, e.argidx = self.x.data_ptr(), ctypes.pointer(self.w), ops._dp(self.eps), self.argidx.data_ptr()
        e.g, e.f, e.mu, e.lv, e.z, e.explv = (ops._dp(t) for t in (self.g, self.f, self.mu, self.lv, self.z, self.explv))
        e.ws, e.is_vae, e.out_ld = self.ws.data_ptr(), int(self.vae), self.out_ld
        return e

    def forward(self):
        L = _lib()
        L.call("hp_encoder_forward", self.B, self.Np, self.x, ctypes.byref(self.w), self.out, int(self.vae), self.eps, self.argidx,
               self.g, self.f, self.mu, self.lv, self.z, self.explv, self.ws, L.current_stream(self.x.device))
        return self

    def hidden(self):
        """h1..h4 as fp32 rows (views of the workspace, converted in place by hp_encoder_workspace_to_f32 where the forward left
        them in the P-format)."""
        L = _lib()
        L.call("hp_encoder_workspace_to_f32", self.B, self.Np, self.ws, L.current_stream(self.x.device))
        torch.cuda.synchronize()
        R, hs, off = self.B * self.Np, [], 0
        for c in WIDTHS[1:5]:
            hs.append(self.ws[off:off + R * c].view(R, c))
            off += R * c
        return hs

    def masks(self):
        """Where the stored h1..h4 are positive, (B, Np, C) each: the ReLU masks a backward over this workspace applies."""
        return [(h > 0).view(self.B, self.Np, -1).cpu() for h in self.hidden()]

    def outputs(self):
        o = {"argidx": self.argidx, "g": self.g, "f": self.f, "mu": self.mu}
        if self.vae:
            o.update(lv=self.lv, z=self.z[:, :self.out], explv=self.explv)
        return {k: v.clone() for k, v in o.items()}

    def prepare_backward(self, alloc=fresh, ws_off=0):
        from hyperpocket_amd import ops
        self.grads = [_filled(alloc, tuple(p.shape)) for p in self.params]
        self.gr = ops._encoder_struct(self.grads)
        self.bws = _off16(alloc, bwd_ws_floats(self.B, self.out), ws_off)
        self.bws.fill_(float("nan"))

    def bwd_io(self, gout, gout_ld, gmu, gexplv, fwd_ws):
        from hyperpocket_amd import ops
        e = ops._EncoderBwdIO()
        e.x, e.w, e.eps, e.argidx = self.x.data_ptr(), ctypes.pointer(self.w), ops._dp(self.eps), self.argidx.data_ptr()
        e.g, e.f, e.lv = self.g.data_ptr(), self.f.data_ptr(), ops._dp(self.lv)
        e.grad_out, e.grad_mu, e.grad_explv = ops._dp(gout), ops._dp(gmu), ops._dp(gexplv)
        e.gr, e.ws, e.fwd_ws = ctypes.pointer(self.gr), self.bws.data_ptr(), ops._dp(fwd_ws)
        e.is_vae, e.grad_out_ld = int(self.vae), gout_ld
        return e

    def backward(self, gout, gout_ld=None, gmu=None, gexplv=None, dedup=1, fwd_ws="own", alloc=fresh, ws_off=0):
        """hp_encoder_backward_ld; fwd_ws: "own" (the workspace the forward ran in), a tensor, or None.  Returns the gradients
        (clones, parameter order)."""
        L = _lib()
        self.prepare_backward(alloc, ws_off)
        fw = self.ws if isinstance(fwd_ws, str) else fwd_ws
        L.call("hp_encoder_backward_ld", self.B, self.Np, self.x, ctypes.byref(self.w), self.out, int(self.vae), self.eps, self.argidx,
               self.g, self.f, self.lv, gout, self.out if gout_ld is None else gout_ld, gmu, gexplv, ctypes.byref(self.gr),
               self.bws, fw, int(dedup), L.current_stream(self.x.device))
        torch.cuda.synchronize()
        return [t.clone() for t in self.grads]


def upstream(B, out_size, ld=None, use=(True, True, True), gscale=1.0, alloc=fresh):
    """The constant upstream gradients of UPSTREAM as device tensors (gz with row stride ld, gmu, gexplv); None where dropped."""
    ld = out_size if ld is None else ld
    full = lambda c: _filled(alloc, (B, out_size), like=torch.full((B, out_size), c * gscale))
    gz = None
    if use[0]:
        gz = _filled(alloc, (B, ld))                            # the padding columns stay NaN: nothing may read them
        gz[:, :out_size] = UPSTREAM[0] * gscale
    return gz, (full(UPSTREAM[1]) if use[1] else None), (full(UPSTREAM[2]) if use[2] else None)


def single(B, Np, out_size, x, params, eps=None, gscale=1.0, ld=None, dedup=1, alloc=fresh):
    """One encoder forward and backward (every upstream gradient present) through the single-encoder calls: (outputs, gradients)."""
    s = Side(B, Np, out_size, x, params, eps, alloc).forward()
    gz, gmu, gex = upstream(B, out_size, ld, gscale=gscale, alloc=alloc)
    grads = s.backward(gz, ld, gmu if s.vae else None, gex if s.vae else None, dedup=dedup, alloc=alloc)
    out = s.outputs()
    out["masks"] = s.masks()
    return out, grads


def pair(B, Np, out_size, x0, p0, eps, x1, p1, reverse=False, alloc=fresh, dedup=1):
    """The VAE encoder (x0, p0, eps) and the plain one (x1, p1) through hp_encoder_forward_pair and hp_encoder_backward_pair,
    the plain encoder's mu in the latent's second column block and the halves of d latent read in place, as
    ops.EncoderPairFunction does it.  reverse: encoder 1's buffers are carved before (below) encoder 0's.
    Returns ((outputs0, grads0), (outputs1, grads1))."""
    from hyperpocket_amd import ops
    L = _lib()
    latent = _filled(alloc, (B, 2 * out_size))
    glat = _filled(alloc, (B, 2 * out_size), like=torch.full((B, 2 * out_size), UPSTREAM[0]))
    gmu = _filled(alloc, (B, out_size), like=torch.full((B, out_size), UPSTREAM[1]))
    gex = _filled(alloc, (B, out_size), like=torch.full((B, out_size), UPSTREAM[2]))
    sides = [None, None]
    for z in ((1, 0) if reverse else (0, 1)):
        sides[z] = Side(B, Np, out_size, (x0, x1)[z], (p0, p1)[z], eps if z == 0 else None, alloc, latent=latent)
        sides[z].prepare_backward(alloc)
    if reverse:
        assert sides[1].ws.data_ptr() < sides[0].ws.data_ptr() and sides[1].bws.data_ptr() < sides[0].bws.data_ptr()
        assert sides[1].grads[0].data_ptr() < sides[0].grads[0].data_ptr() and sides[1].g.data_ptr() < sides[0].g.data_ptr()
    io = (ops._EncoderIO * 2)(sides[0].io(), sides[1].io())
    L.call("hp_encoder_forward_pair", B, Np, out_size, io, L.current_stream(latent.device))
    outs = [s.outputs() for s in sides]
    bio = (ops._EncoderBwdIO * 2)(sides[0].bwd_io(glat, 2 * out_size, gmu, gex, sides[0].ws),
                                  sides[1].bwd_io(glat[:, out_size:], 2 * out_size, None, None, sides[1].ws))
    L.call("hp_encoder_backward_pair", B, Np, out_size, bio, int(dedup), L.current_stream(latent.device))
    torch.cuda.synchronize()
    return tuple((o, [t.clone() for t in s.grads]) for o, s in zip(outs, sides))


def pair_as_singles(B, Np, out_size, x0, p0, eps, x1, p1, dedup=1):
    """The same two encoders through two hp_encoder_forward / hp_encoder_backward_ld calls each: d latent is handed over the
    same way (row stride 2 out_size); a single forward writes a dense mu."""
    res = []
    glat = torch.full((B, 2 * out_size), UPSTREAM[0], device="cuda")
    gmu, gex = torch.full((B, out_size), UPSTREAM[1], device="cuda"), torch.full((B, out_size), UPSTREAM[2], device="cuda")
    for z, (x, p) in enumerate(((x0, p0), (x1, p1))):
        s = Side(B, Np, out_size, x, p, eps if z == 0 else None).forward()
        o = s.outputs()
        gout = glat if z == 0 else glat[:, out_size:]
        res.append((o, s.backward(gout, 2 * out_size, gmu if z == 0 else None, gex if z == 0 else None, dedup=dedup)))
    return tuple(res)


def pair_arena_bytes(B, Np, out_size):
    per = 4 * (fwd_ws_floats(B, Np) + bwd_ws_floats(B, out_size) + B * Np * 3 + 2 * 1_100_000 + B * (4 * 512 + 8 * out_size)) + 256 * 80
    return 2 * per + 4 * 8 * B * out_size + 256 * 8


# ------------------------------------------------------------------------------------------------ error measures
def err_of_scale(got, want):
    """max |got - want| and max |want| (float64)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (got - want).abs().max().item(), want.abs().max().item()


# ------------------------------------------------------------------------------------------------ the case tables
# (B, Np) at out_size = 128, by what they sit next to in encoder_forward_impl / encoder_backward_impl (csrc/model.hip)
POOL_SLAB_CASES = [(1, 128), (3, 128), (1, 384), (4, 128), (1, 512)]       # fused pool; the slabs fit from R = 512 on
RAGGED_CASES = [(1, 1), (1, 129), (2, 127), (3, 200)]                      # ragged split route: smallest, across a tile seam
FP32_TILE64_CASES = [(2, 64), (3, 192)]                                    # fp32 route only: 64-row tiles fused
FP32_TILE128_CASES = [(64, 192), (96, 128), (32, 384)]                     # ... the tile flips to 128: unfused | fused, B > 64 | fused, skinny tails
OVER_SKINNY_CASES = [(65, 128), (70, 100)]                                 # B over the skinny limit
S_BOUNDARY_CASES = [(B, Np) for Np in (128, 100) for B in (1, 19, 20, 21, 23, 24)]

FP32_ONLY = set(FP32_TILE64_CASES + FP32_TILE128_CASES)
ALL_CASES = list(dict.fromkeys(POOL_SLAB_CASES + RAGGED_CASES + FP32_TILE64_CASES + FP32_TILE128_CASES + OVER_SKINNY_CASES +
                               S_BOUNDARY_CASES))
PAIR_CASES = [(1, 128), (20, 128), (21, 128), (24, 100), (65, 128), (3, 200)]
# fall-backs: (name, B, Np, out_size, is_vae, grad_out_ld - out_size, aligned, what the plan must say of the backward)
FALLBACK_CASES = [
    ("out32_vae", 3, 128, 32, True, 0, True, dict(bwd_fused=True, bwd_tails_skinny=(True,))),
    ("out32_plain", 3, 128, 32, False, 0, True, dict(bwd_fused=True, bwd_tails_skinny=(False,))),   # one head, one range: not built
    ("out512", 3, 128, 512, True, 0, True, dict(bwd_fused=True, bwd_tails_skinny=(True,))),
    ("out544", 3, 128, 544, True, 0, True, dict(bwd_fused=False, bwd_tails_skinny=(False,))),
    ("out96", 5, 128, 96, True, 0, True, dict(fwd_tails_skinny=True, bwd_fused=True, bwd_tails_skinny=(False,))),
    ("ld_plus2", 3, 128, 128, False, 2, True, dict(bwd_fused=True, bwd_tails_skinny=(False,))),
    ("ld_plus2_vae", 3, 128, 128, True, 2, True, dict(bwd_fused=True, bwd_tails_skinny=(True,))),   # the head kernel reads the stride
    ("unaligned", 3, 128, 128, True, 0, False, dict(bwd_fused=False, bwd_tails_skinny=(False,))),
]


def routes_of(cases):
    """Forward cases as (route, B, Np): every case on the fp32 route, all but the fp32-only ones on the default route, the
    whole-tile ones of the slab group on round 3's route too."""
    out = []
    for B, Np in cases:
        if (B, Np) not in FP32_ONLY:
            out.append(("default", B, Np))
        if (B, Np) in POOL_SLAB_CASES:
            out.append(("r3", B, Np))
        out.append(("fp32", B, Np))
    return out


def forward_combo(plan):
    return plan["conv"], plan["pool_fused"], plan["tile_rows"] if plan["pool_fused"] else None, plan["fwd_tails_skinny"]


# every forward combination the dispatch can produce ...
FORWARD_COMBOS = {
    ("pformat", True, 128, True), ("pformat", True, 128, False),
    ("split_f32", True, 128, True), ("split_f32", True, 128, False), ("split_f32", False, None, False),
    ("gemm_f32", True, 64, True), ("gemm_f32", True, 64, False), ("gemm_f32", True, 128, True), ("gemm_f32", True, 128, False),
    ("gemm_f32", False, None, False),
}
# ... and why the others cannot occur
FORWARD_UNREACHABLE = {
    "unfused pool with skinny tails": "the tails' slabs live in the h5 slot, which holds h5 itself when the pool is not fused",
    "pformat with an unfused pool": "the P-format needs Np % 128 == 0, which is the fused-pool condition at its 128-row tiles",
    "pformat / split_f32 with 64-row tiles": "the split-f16 kernels have 128-row tiles only",
}


def backward_combo(plan, B):
    s = plan["bwd_splits"]
    return plan["bwd_fused"], (None if not plan["bwd_fused"] else "B" if s == B else "cap"), plan["bwd_tails_skinny"][0]


BACKWARD_COMBOS = {(True, "B", True), (True, "B", False), (True, "cap", True), (True, "cap", False),
                   (False, None, True), (False, None, False)}


def plan_of(route, B, Np, out_size=128, is_vae=(True,), **kw):
    from hyperpocket_amd import ops
    split, presplit = CONV_ROUTES[route]
    with switches(split, presplit):
        return ops.encoder_plan(B, Np, out_size, is_vae, **kw)


def check_cases_reach_every_route():
    """Through hp_encoder_plan: the case tables reach every forward combination (conv format x pool x tile x tails) and every
    backward combination (fused | layered x row ranges = B | capped x tails) on both chains, every listed boundary from
    both sides, and nothing the tables of unreachable combinations exclude."""
    seen = {forward_combo(plan_of(r, B, Np)) for r, B, Np in routes_of(ALL_CASES)}
    assert seen == FORWARD_COMBOS, (sorted(map(str, seen - FORWARD_COMBOS)), sorted(map(str, FORWARD_COMBOS - seen)))
    for combo in seen:
        assert not (not combo[1] and combo[3]) and not (combo[0] == "pformat" and not combo[1])
        assert not (combo[0] != "gemm_f32" and combo[2] == 64)
    for chain16, cap in ((1, 20), (0, 23)):
        with switches(chain16=chain16):
            plans = {(B, Np): plan_of("default" if (B, Np) not in FP32_ONLY else "fp32", B, Np) for B, Np in ALL_CASES}
            back = {backward_combo(p, B) for (B, Np), p in plans.items()}
            for name, B, Np, out, vae, pad, aligned, want in FALLBACK_CASES:
                p = plan_of("default", B, Np, out, (vae,), ld=out + pad, aligned=aligned)
                for k, v in want.items():
                    assert p[k] == v, (name, k, p)
                back.add(backward_combo(p, B))
            back.add(backward_combo(plan_of("default", 3, 128, dedup=False), 3))          # per-channel rows: layered, skinny tails
            assert back == BACKWARD_COMBOS, (chain16, back ^ BACKWARD_COMBOS)
            for Np in (128, 100):                                                          # the row ranges on either side of each cap
                assert [plans[B, Np]["bwd_splits"] for B in (1, 19, 20, 21, 23, 24)] == [min(B, cap) for B in (1, 19, 20, 21, 23, 24)]
    # the forward's boundaries from both sides
    tails = lambda r, B, Np: plan_of(r, B, Np)["fwd_tails_skinny"]
    assert [tails("default", B, Np) for B, Np in POOL_SLAB_CASES] == [False, False, False, True, True]
    assert not tails("default", 65, 128) and tails("default", 24, 128)
    assert plan_of("fp32", 64, 192)["tile_rows"] == 128 and plan_of("fp32", 3, 192)["tile_rows"] == 64
    assert max(B * Np for B, Np in ALL_CASES) == 12288

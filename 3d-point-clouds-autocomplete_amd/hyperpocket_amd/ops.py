"""autograd bridges between PyTorch tensors and the model entry points of the C ABI.

Each Function's forward/backward is ONE call into libhyperpocket_hip.so (which issues the whole
launch sequence on the current stream); PyTorch only owns the memory and the autograd wiring.
"""
import contextlib
import ctypes
from ctypes import c_int, c_long, c_void_p

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import HipExtensionError, call, check_input, current_stream, load_library, ptr

HP_MAX_HEADS = 8


class _NodeFunction(Function):
    """The nodes form the gradients of the parameters and of `latent` / `theta` only.  REFUSED lists (position, name) of
    the inputs whose gradient the HIP backward does not form: one of them requiring grad while a graph is recorded is an
    error at the call — the backward would hand the caller a silent None.  (Checked here, not in forward: a Function's
    forward always runs with grad mode off.)"""
    REFUSED = ()

    @classmethod
    def apply(cls, *args):
        if torch.is_grad_enabled():
            for i, name in cls.REFUSED:
                if isinstance(args[i], torch.Tensor) and args[i].requires_grad:
                    raise HipExtensionError(f"{cls.__name__}: `{name}` requires grad, but the gradient of `{name}` is not "
                                            f"formed by the HIP backward; detach it (or run under torch.no_grad())")
        return super().apply(*args)


class _EncoderPtrs(ctypes.Structure):  # HpEncoderWeights / HpEncoderGrads (csrc/hp_model.h)
    _fields_ = [("conv_w", c_void_p * 5), ("conv_b", c_void_p * 5), ("fc_w", c_void_p), ("fc_b", c_void_p),
                ("mu_w", c_void_p), ("mu_b", c_void_p), ("std_w", c_void_p), ("std_b", c_void_p)]


class _EncoderIO(ctypes.Structure):  # HpEncoderIO (one encoder's buffers for hp_encoder_forward_pair)
    _fields_ = [("x", c_void_p), ("w", ctypes.POINTER(_EncoderPtrs)), ("eps", c_void_p), ("argidx", c_void_p),
                ("g", c_void_p), ("f", c_void_p), ("mu", c_void_p), ("lv", c_void_p), ("z", c_void_p), ("explv", c_void_p),
                ("ws", c_void_p), ("is_vae", c_int), ("out_ld", c_int)]


class _EncoderBwdIO(ctypes.Structure):  # HpEncoderBwdIO (one encoder's buffers for hp_encoder_backward_pair)
    _fields_ = [("x", c_void_p), ("w", ctypes.POINTER(_EncoderPtrs)), ("eps", c_void_p), ("argidx", c_void_p),
                ("g", c_void_p), ("f", c_void_p), ("lv", c_void_p), ("grad_out", c_void_p), ("grad_mu", c_void_p),
                ("grad_explv", c_void_p), ("gr", ctypes.POINTER(_EncoderPtrs)), ("ws", c_void_p), ("fwd_ws", c_void_p),
                ("is_vae", c_int), ("grad_out_ld", c_int)]


class _HyperWeights(ctypes.Structure):  # HpHyperWeights
    _fields_ = [("trunk_w", c_void_p * 5), ("trunk_b", c_void_p * 5), ("n_heads", c_int),
                ("head_out", c_int * HP_MAX_HEADS), ("head_w", c_void_p * HP_MAX_HEADS),
                ("head_b", c_void_p * HP_MAX_HEADS)]


class _HyperGrads(ctypes.Structure):  # HpHyperGrads
    _fields_ = [("trunk_w", c_void_p * 5), ("trunk_b", c_void_p * 5), ("head_w", c_void_p * HP_MAX_HEADS),
                ("head_b", c_void_p * HP_MAX_HEADS)]


def _dp(t):
    return None if t is None else t.data_ptr()


def _long_fn(name, *args):
    fn = getattr(load_library(), name)
    fn.restype = c_long
    return fn(*args)


# ---------------------------------------------------------------------------------------------
# Arithmetic: by default the wide GEMM-shaped kernels form each fp32 product on the f16 / bf16 matrix pipe from
# exact pieces of the fp32 operands (fp32 accumulation; see bench.py config.arithmetic).  Every one of them has an
# IEEE-fp32 form (v_mfma_f32_* / VALU fma) behind a process-wide switch of the library.
# ---------------------------------------------------------------------------------------------
_PIECE_SWITCHES = ("hp_conv_split_set",                   # encoder conv stack: two f16 pieces per operand
                   "hp_conv_presplit_set",                # ... hidden activations stored as piece pairs
                   "hp_encoder_backward_set_chain_f16",   # encoder backward: delta chain + dW launch
                   "hp_hypernet_set_heads_stream",        # hypernetwork heads' forward: three bf16 pieces
                   "hp_target_fused_set_f16")             # fused decoder forward


@contextlib.contextmanager
def strict_fp32():
    """Inside the block every kernel computes its products in fp32 (no f16 / bf16 pieces): the arithmetic the
    reference states.  The switches are process-wide (not per stream or thread) and restored on exit."""
    lib = load_library()
    was = [getattr(lib, name)(0) for name in _PIECE_SWITCHES]
    try:
        yield
    finally:
        for name, prev in zip(_PIECE_SWITCHES, was):
            getattr(lib, name)(prev)


# ---------------------------------------------------------------------------------------------
# Gradient placement: a FlatParameters owner (parallel.py) may register, per parameter, a view of
# its flat gradient buffer; backward then writes gradients straight into it (no copy before the
# RCCL all-reduce / fused Adam).  Default: fresh tensors.
# ---------------------------------------------------------------------------------------------
_GRAD_VIEWS = {}
_GRAD_VIEWS_OUT = set()     # keys whose view a backward has been handed since the owner last cleared its gradients


def register_grad_view(param, view):
    """Returns the registry key; the owner drops its keys when it dies (parallel.FlatParameters does, through a
    weakref finalizer), so a dead engine's flat gradient buffer is not pinned by this table."""
    _GRAD_VIEWS[param.data_ptr()] = view
    _GRAD_VIEWS_OUT.discard(param.data_ptr())
    return param.data_ptr()


def drop_grad_views(keys):
    for k in keys:
        _GRAD_VIEWS.pop(k, None)
        _GRAD_VIEWS_OUT.discard(k)


def clear_grad_views():
    _GRAD_VIEWS.clear()
    _GRAD_VIEWS_OUT.clear()


def reset_grad_views(keys):
    """The owner has cleared its parameters' gradients (FlatParameters.clear_param_grads): nothing aliases its flat
    gradient buffer any more, the next backward may be handed the registered views again."""
    _GRAD_VIEWS_OUT.difference_update(keys)


def _grad_buffer(param):
    """The tensor a backward kernel OVERWRITES with param's gradient and the node returns.  The registered view is handed
    out only where autograd adopting it is right: param.grad is unset and no backward since the owner's last clear holds
    the view already.  Every other case — a second backward onto a set .grad, a parameter used by two nodes of one
    graph, a gradient the caller of torch.autograd.grad kept — would have this kernel overwrite a gradient somebody
    still reads; it gets a fresh tensor, and AccumulateGrad's own in-place add lands the sum in the flat slice."""
    k = param.data_ptr()
    v = _GRAD_VIEWS.get(k)
    if v is not None and v.shape == param.shape and param.grad is None and k not in _GRAD_VIEWS_OUT:
        _GRAD_VIEWS_OUT.add(k)
        # a FRESH view object: autograd's AccumulateGrad keeps (instead of cloning) a gradient nobody else references,
        # so param.grad ends up aliasing the flat buffer with no copy
        return v.view(v.shape)
    return torch.empty_like(param, memory_format=torch.contiguous_format)


def _grad_block(params):
    """_grad_buffer for parameters whose registered views lie back to back (the hypernetwork heads' weights; their
    biases).  The library picks the heads' launches by whether these buffers are contiguous, and refuses a skipped dW
    without contiguous bias gradients: so where such views exist but may not be handed out, the fresh tensors are slices
    of ONE block — the same launches, hence the same bits, as a backward that writes in place.  Views that do not lie
    back to back (or none): one _grad_buffer each."""
    keys = [p.data_ptr() for p in params]
    views = [_GRAD_VIEWS.get(k) for k in keys]
    if any(v is None or v.shape != p.shape for v, p in zip(views, params)) or \
            any(b.data_ptr() != a.data_ptr() + 4 * a.numel() for a, b in zip(views, views[1:])):
        return [_grad_buffer(p) for p in params]
    if all(p.grad is None and k not in _GRAD_VIEWS_OUT for p, k in zip(params, keys)):
        _GRAD_VIEWS_OUT.update(keys)
        return [v.view(v.shape) for v in views]
    block = torch.empty((sum(p.numel() for p in params),), dtype=torch.float32, device=params[0].device)
    return [t.view(p.shape) for t, p in zip(block.split([p.numel() for p in params]), params)]


# The encoder backward copies the critical rows' activations out of the forward's workspace (15 KB per point, kept
# alive by the autograd node).  False: drop the workspace after the forward and recompute those rows instead.
KEEP_ENCODER_ACTIVATIONS = True
# Channels whose max-pool peaks at the same point share every activation below it: the encoder backward runs its
# layers 4..1 on the distinct critical points (~170 of 512 per cloud).  False: one row per (cloud, channel).
DEDUP_CRITICAL_ROWS = True


def _encoder_struct(params, cls=_EncoderPtrs):
    # params: conv_w x5, conv_b x5, fc_w, fc_b, mu_w, mu_b[, std_w, std_b]
    s = cls()
    for i in range(5):
        s.conv_w[i] = _dp(params[i])
        s.conv_b[i] = _dp(params[5 + i])
    s.fc_w, s.fc_b, s.mu_w, s.mu_b = (_dp(p) for p in params[10:14])
    if len(params) > 14:
        s.std_w, s.std_b = _dp(params[14]), _dp(params[15])
    return s


class EncoderFunction(_NodeFunction):
    """model/encoder.py:43-53.  x: (B, Np, 3) contiguous.  params as listed in _encoder_struct.
    Returns mu (plain) or (z, mu, exp(logvar)) (VAE)."""
    REFUSED = ((0, "x"), (1, "eps"))

    @staticmethod
    def forward(ctx, x, eps, out_size, *params):
        check_input(x, "x")
        is_vae = len(params) == 16
        for i, p in enumerate(params):
            check_input(p, f"encoder param {i}")
        B, Np = x.size(0), x.size(1)
        dev = x.device
        f32 = dict(dtype=torch.float32, device=dev)
        argidx = torch.empty((B, 512), dtype=torch.int32, device=dev)
        g = torch.empty((B, 512), **f32)
        f = torch.empty((B, 512), **f32)
        mu = torch.empty((B, out_size), **f32)
        lv = z = explv = None
        if is_vae:
            check_input(eps, "eps")
            lv, z, explv = (torch.empty((B, out_size), **f32) for _ in range(3))
        ws = torch.empty((_long_fn("hp_encoder_forward_workspace_floats", B, Np),), **f32)
        w = _encoder_struct(params)
        call("hp_encoder_forward", B, Np, x, ctypes.byref(w), out_size, int(is_vae), eps, argidx, g, f, mu, lv, z, explv,
             ws, current_stream(dev))
        ctx.is_vae, ctx.out_size = is_vae, out_size
        ctx.fwd_ws = ws if KEEP_ENCODER_ACTIVATIONS else None
        ctx.save_for_backward(x, eps, argidx, g, f, lv, *params)
        # an output the loss does not use arrives as None in backward: the heads it alone feeds get no gradient
        ctx.set_materialize_grads(False)
        if is_vae:
            return z, mu, explv
        return mu

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        x, eps, argidx, g, f, lv, *params = ctx.saved_tensors
        B, Np = x.size(0), x.size(1)
        dev = x.device
        if all(t is None for t in grads):
            return (None,) * (3 + len(params))
        reached = [True] * len(params)
        if ctx.is_vae:
            # mu_layer feeds z and mu, std_layer z and exp(logvar): a head none of whose outputs the loss uses has no gradient
            # (.grad stays None, as under plain autograd).  The kernels see zeros for an unused output, as they always have.
            reached[12:14] = [grads[0] is not None or grads[1] is not None] * 2
            reached[14:16] = [grads[0] is not None or grads[2] is not None] * 2
            gz, gmu, gexplv = (torch.zeros((B, ctx.out_size), dtype=torch.float32, device=dev) if t is None else t.contiguous()
                               for t in grads)
            gout = gz
        else:
            gout, gmu, gexplv = grads[0].contiguous(), None, None
        out = [_grad_buffer(p) if r else torch.empty_like(p) for p, r in zip(params, reached)]
        ws = torch.empty((_long_fn("hp_encoder_backward_workspace_floats", B, ctx.out_size),), dtype=torch.float32,
                         device=dev)
        w, gr = _encoder_struct(params), _encoder_struct(out)
        call("hp_encoder_backward", B, Np, x, ctypes.byref(w), ctx.out_size, int(ctx.is_vae), eps, argidx, g, f, lv,
             gout, gmu, gexplv, ctypes.byref(gr), ws, ctx.fwd_ws, int(DEDUP_CRITICAL_ROWS), current_stream(dev))
        ctx.fwd_ws = None
        return (None, None, None, *(o if r else None for o, r in zip(out, reached)))


class EncoderPairFunction(_NodeFunction):
    """The two encoders of a HyperPocket training step (model/full_model.py:106-112) as ONE node: the conv stacks of both run
    as batched launches (hp_encoder_forward_pair), and so do their backward's (hp_encoder_backward_pair, one stream).  Arguments:
    x_vae (missing), eps, x_plain (existing), out_size, then the VAE encoder's 16 parameters and the plain encoder's 14.
    Returns (latent, mu, exp(logvar)) with latent = [z | real_mu] (B, 2*out): the two encoders write its halves directly (no
    torch.cat) and the backward reads the halves of d latent in place."""

    N_VAE = 16
    REFUSED = ((0, "x (VAE encoder)"), (1, "eps"), (2, "x (plain encoder)"))

    @staticmethod
    def forward(ctx, x0, eps, x1, out_size, *params):
        p0, p1 = params[:EncoderPairFunction.N_VAE], params[EncoderPairFunction.N_VAE:]
        check_input(x0, "x (VAE encoder)")
        check_input(x1, "x (plain encoder)")
        check_input(eps, "eps")
        for i, p in enumerate(params):
            check_input(p, f"encoder param {i}")
        if x0.shape != x1.shape or len(p1) != 14:
            raise HipExtensionError("EncoderPairFunction: both encoders must see the same (B, N, 3) shape")
        B, Np = x0.size(0), x0.size(1)
        dev = x0.device
        f32 = dict(dtype=torch.float32, device=dev)
        nws = _long_fn("hp_encoder_forward_workspace_floats", B, Np)
        io = (_EncoderIO * 2)()
        keep, structs = [], []
        latent = torch.empty((B, 2 * out_size), **f32)
        for e, (x, ps, vae) in enumerate(((x0, p0, True), (x1, p1, False))):
            argidx = torch.empty((B, 512), dtype=torch.int32, device=dev)
            g, f = torch.empty((B, 512), **f32), torch.empty((B, 512), **f32)
            lv = z = explv = None
            if vae:
                mu = torch.empty((B, out_size), **f32)
                lv, explv = (torch.empty((B, out_size), **f32) for _ in range(2))
                z = latent                                   # columns [0, out)
            else:
                mu = latent[:, out_size:]                    # columns [out, 2*out): data_ptr() is the block's first element
            ws = torch.empty((nws,), **f32)
            w = _encoder_struct(ps)
            structs.append(w)
            io[e].x, io[e].w, io[e].eps, io[e].argidx = x.data_ptr(), ctypes.pointer(w), _dp(eps if vae else None), argidx.data_ptr()
            io[e].g, io[e].f, io[e].mu, io[e].lv, io[e].z, io[e].explv = (_dp(t) for t in (g, f, mu, lv, z, explv))
            io[e].ws, io[e].is_vae, io[e].out_ld = ws.data_ptr(), int(vae), 2 * out_size
            keep.append((argidx, g, f, mu, lv, z, explv, ws))
        call("hp_encoder_forward_pair", B, Np, out_size, io, current_stream(dev))
        ctx.out_size = out_size
        ctx.fwd_ws = [k[7] if KEEP_ENCODER_ACTIVATIONS else None for k in keep]
        ctx.save_for_backward(x0, eps, x1, keep[0][0], keep[0][1], keep[0][2], keep[0][4], keep[1][0], keep[1][1], keep[1][2],
                              *params)
        return latent, keep[0][3], keep[0][6]

    @staticmethod
    @once_differentiable
    def backward(ctx, glat, gmu, gexplv):
        x0, eps, x1, arg0, g0, f0, lv0, arg1, g1, f1, *params = ctx.saved_tensors
        p0, p1 = params[:EncoderPairFunction.N_VAE], params[EncoderPairFunction.N_VAE:]
        B, Np = x0.size(0), x0.size(1)
        dev = x0.device
        nws = _long_fn("hp_encoder_backward_workspace_floats", B, ctx.out_size)
        glat, gmu, gexplv = (None if t is None else t.contiguous() for t in (glat, gmu, gexplv))
        if glat is None:
            glat = torch.zeros((B, 2 * ctx.out_size), dtype=torch.float32, device=dev)
        out0, out1 = [_grad_buffer(p) for p in p0], [_grad_buffer(p) for p in p1]
        gz, greal = glat, glat[:, ctx.out_size:]             # the halves of d latent, read in place (row stride 2*out)
        # one call, one stream: the conv stacks of both encoders in four shared launches, the tails in three
        io = (_EncoderBwdIO * 2)()
        keep = []
        for e, (x, ps, outs, vae, argidx, g, f, lv, gout, gm, ge, fwd_ws) in enumerate((
                (x0, p0, out0, True, arg0, g0, f0, lv0, gz, gmu, gexplv, ctx.fwd_ws[0]),
                (x1, p1, out1, False, arg1, g1, f1, None, greal, None, None, ctx.fwd_ws[1]))):
            ws = torch.empty((nws,), dtype=torch.float32, device=dev)
            w, gr = _encoder_struct(ps), _encoder_struct(outs)
            keep.append((ws, w, gr))
            io[e].x, io[e].w, io[e].eps, io[e].argidx = x.data_ptr(), ctypes.pointer(w), _dp(eps if vae else None), argidx.data_ptr()
            io[e].g, io[e].f, io[e].lv = g.data_ptr(), f.data_ptr(), _dp(lv)
            io[e].grad_out, io[e].grad_mu, io[e].grad_explv = gout.data_ptr(), _dp(gm), _dp(ge)
            io[e].gr, io[e].ws, io[e].fwd_ws = ctypes.pointer(gr), ws.data_ptr(), _dp(fwd_ws)
            io[e].is_vae, io[e].grad_out_ld = int(vae), 2 * ctx.out_size
        call("hp_encoder_backward_pair", B, Np, ctx.out_size, io, int(DEDUP_CRITICAL_ROWS), current_stream(dev))
        ctx.fwd_ws = [None, None]                            # a second backward (retain_graph) recomputes the critical rows
        return (None, None, None, None, *out0, *out1)


class _EncoderPlan(ctypes.Structure):  # HpEncoderPlan
    _fields_ = [("conv_format", c_int), ("pool_fused", c_int), ("tile_rows", c_int), ("fwd_tails_skinny", c_int),
                ("bwd_fused", c_int), ("bwd_splits", c_int), ("bwd_tails_skinny", c_int * 2)]


ENC_CONV_FORMATS = ("pformat", "split_f32", "gemm_f32")     # HP_ENC_CONV_*


def encoder_plan(B, Np, out_size=128, is_vae=(True,), ld=None, aligned=True, dedup=True):
    """The launches the encoder calls take for these shapes under the library's current switches (hp_encoder_plan; host
    only): one encoder (hp_encoder_forward / hp_encoder_backward_ld) or the two of a pair, `ld` the row stride(s) of grad_out.
    Returns a dict: conv ('pformat' | 'split_f32' | 'gemm_f32'), pool_fused, tile_rows, fwd_tails_skinny, bwd_fused,
    bwd_splits, bwd_tails_skinny (a tuple, one entry per encoder).  Shapes the calls refuse raise HipExtensionError."""
    n = len(is_vae)
    vae = (c_int * 2)(*[int(v) for v in is_vae])
    lds = None if ld is None else (c_int * 2)(*([int(v) for v in ld] if isinstance(ld, (tuple, list)) else [int(ld)] * n))
    p = _EncoderPlan()
    call("hp_encoder_plan", int(B), int(Np), int(out_size), n, vae, lds, int(bool(aligned)), int(bool(dedup)), ctypes.byref(p))
    return {"conv": ENC_CONV_FORMATS[p.conv_format], "pool_fused": bool(p.pool_fused), "tile_rows": p.tile_rows,
            "fwd_tails_skinny": bool(p.fwd_tails_skinny), "bwd_fused": bool(p.bwd_fused), "bwd_splits": p.bwd_splits,
            "bwd_tails_skinny": tuple(bool(v) for v in p.bwd_tails_skinny[:n])}


# The heads' weight gradient may be left to an exchange object with `accepts(head_weights) -> bool`, `begin(grad_theta, t5)`
# and optionally `finish(grad_theta, t5)` (core/engine.py: HeadsShard under data parallelism, FusedHeadsAdam on one GPU): the
# ranks then exchange the gradient's two factors (d theta, t5) instead of the 156 MB matrix / one kernel forms the gradient
# and applies Adam without storing it.  The object travels with the autograd node: HyperNetwork.forward reads it from its
# module (`hyper_network._heads_exchange`, set by the engine for the forward of the step it drives) and hands it to
# HyperNetFunction.apply — no process-global state, two engines in one process do not see each other's.


class HyperNetFunction(Function):
    """model/hyper_network.py:41-43.  params: trunk_w x5, trunk_b x5, head_w x H, head_b x H."""

    @staticmethod
    def forward(ctx, latent, n_heads, exchange, *params):
        latent = latent.contiguous()
        check_input(latent, "latent")
        # raw pointers go to the kernels: a head left on the CPU (`freeze_layers_learning` keeps `output` a plain list,
        # which .cuda() does not move — model/hyper_network.py:38-39), a .half() / .double() model or a foreign device must
        # fail here, not as a GPU memory fault
        for i, p in enumerate(params):
            check_input(p, f"hypernetwork param {i}")
            if p.device != latent.device:
                raise HipExtensionError(f"hypernetwork param {i} is on {p.device}, the latent on {latent.device}")
        B, in_size = latent.shape
        dev = latent.device
        w = _HyperWeights()
        for i in range(5):
            w.trunk_w[i], w.trunk_b[i] = _dp(params[i]), _dp(params[5 + i])
        w.n_heads = n_heads
        total = 0
        for h in range(n_heads):
            hw, hb = params[10 + h], params[10 + n_heads + h]
            w.head_w[h], w.head_b[h], w.head_out[h] = _dp(hw), _dp(hb), hw.size(0)
            total += hw.size(0)
        t = torch.empty((_long_fn("hp_hypernet_saved_floats", B),), dtype=torch.float32, device=dev)
        theta = torch.empty((B, total), dtype=torch.float32, device=dev)
        call("hp_hypernet_forward", B, in_size, latent, ctypes.byref(w), t, theta, total, current_stream(dev))
        ctx.n_heads, ctx.exchange = n_heads, exchange
        ctx.save_for_backward(latent, t, *params)
        return theta

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_theta):
        latent, t, *params = ctx.saved_tensors
        n_heads = ctx.n_heads
        grad_theta = grad_theta.contiguous()
        B, in_size = latent.shape
        dev = latent.device
        w, gr = _HyperWeights(), _HyperGrads()
        exch, ctx.exchange = ctx.exchange, None
        external_dw = exch is not None and exch.accepts(params[10:10 + n_heads])
        out = [_grad_buffer(p) for p in params[:10]] \
            + ([None] * n_heads if external_dw else _grad_block(params[10:10 + n_heads])) \
            + _grad_block(params[10 + n_heads:])
        for i in range(5):
            w.trunk_w[i], w.trunk_b[i] = _dp(params[i]), _dp(params[5 + i])
            gr.trunk_w[i], gr.trunk_b[i] = _dp(out[i]), _dp(out[5 + i])
        w.n_heads = n_heads
        for h in range(n_heads):
            w.head_w[h], w.head_b[h], w.head_out[h] = _dp(params[10 + h]), _dp(params[10 + n_heads + h]), params[10 + h].size(0)
            gr.head_w[h], gr.head_b[h] = _dp(out[10 + h]), _dp(out[10 + n_heads + h])
        if external_dw:
            # issued before this rank's backward launches, so the gathers travel under them
            o5 = _long_fn("hp_hypernet_t5_offset", B)
            exch.begin(grad_theta, t[o5:o5 + B * 2048].view(B, 2048))
        grad_latent = torch.empty_like(latent) if ctx.needs_input_grad[0] else None
        ws = torch.empty((_long_fn("hp_hypernet_backward_workspace_floats", B),), dtype=torch.float32, device=dev)
        # An exchange object with a stream of its own (core/engine.py FusedHeadsAdam) gets that stream ordered behind the LAST
        # READER of the heads' weights inside the call (d t5 = d theta . W): its in-place dW + Adam pass then starts beside the
        # trunk's backward launches, on the CUs its persistent grid occupies.
        if external_dw and getattr(exch, "stream", None) is not None:
            call("hp_hypernet_backward_ordered", B, in_size, latent, ctypes.byref(w), t, grad_theta, grad_theta.size(1),
                 ctypes.byref(gr), grad_latent, ws, current_stream(dev), ctypes.c_void_p(exch.stream.cuda_stream))
        else:
            call("hp_hypernet_backward", B, in_size, latent, ctypes.byref(w), t, grad_theta, grad_theta.size(1), ctypes.byref(gr),
                 grad_latent, ws, current_stream(dev))
        if external_dw and hasattr(exch, "finish"):
            # in-place consumers of the heads' weights (the fused dW + Adam pass) go behind the backward that reads them
            o5 = _long_fn("hp_hypernet_t5_offset", B)
            exch.finish(grad_theta, t[o5:o5 + B * 2048].view(B, 2048))
        return (grad_latent, None, None, *out)


# The published decoder (3-32-64-128-64-3) runs as one fused kernel per direction (csrc/target_fused.hip: weights in
# LDS, activations in registers, nothing saved for the backward).  False: the layered batched-GEMM path, which serves
# every other architecture anyway.
FUSED_TARGET_NETWORK = True


class TargetNetworkFunction(_NodeFunction):
    """All B per-cloud target networks at once (model/full_model.py:70-74 + model/target_network.py).
    theta (B, T), points (B, N, 3) -> y (B, N, 3)."""
    REFUSED = ((1, "points"),)

    @staticmethod
    def forward(ctx, theta, points, channels):
        theta = theta.contiguous()
        points = points.contiguous()
        check_input(theta, "theta")
        check_input(points, "points")
        B, N = points.size(0), points.size(1)
        dev = theta.device
        ch = (c_int * len(channels))(*channels)
        need = _long_fn("hp_target_theta_size", len(channels), ch)
        if need != theta.size(1) or theta.size(0) != B:
            # model/target_network.py:29 `assert split_index == len(weights)`
            raise HipExtensionError(f"target network expects {need} weights per cloud, got {tuple(theta.shape)}")
        y = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        ctx.channels = tuple(channels)
        ctx.fused = bool(FUSED_TARGET_NETWORK and load_library().hp_target_fused_supported(len(channels), ch))
        if ctx.fused:
            call("hp_target_fused_forward", B, N, theta, theta.size(1), points, y, current_stream(dev))
            ctx.save_for_backward(theta, points)
            return y
        acts = torch.empty((_long_fn("hp_target_saved_floats", B, N, len(channels), ch),), dtype=torch.float32, device=dev)
        call("hp_target_forward", B, N, len(channels), ch, theta, theta.size(1), points, acts, y, current_stream(dev))
        ctx.save_for_backward(theta, points, acts)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        grad_y = grad_y.contiguous()
        theta, points = ctx.saved_tensors[:2]
        B, N = points.size(0), points.size(1)
        dev = theta.device
        grad_theta = torch.empty_like(theta)
        if ctx.fused:
            ws = torch.empty((_long_fn("hp_target_fused_workspace_floats", B, N),), dtype=torch.float32, device=dev)
            call("hp_target_fused_backward", B, N, theta, theta.size(1), points, grad_y, grad_theta, ws, current_stream(dev))
            return grad_theta, None, None
        acts = ctx.saved_tensors[2]
        ch = (c_int * len(ctx.channels))(*ctx.channels)
        ws = torch.empty((_long_fn("hp_target_backward_workspace_floats", B, N, len(ctx.channels), ch),), dtype=torch.float32,
                         device=dev)
        call("hp_target_backward", B, N, len(ctx.channels), ch, theta, theta.size(1), points,
             acts, grad_y, grad_theta, ws, current_stream(dev))
        return grad_theta, None, None


class KLDFunction(Function):
    """core/epoch_loops.py:29-30: 0.5*sum(exp(v)+mu^2-1-v)/B with v = the encoder's exp(logvar)."""

    @staticmethod
    def forward(ctx, explv, mu, batch):
        explv, mu = explv.contiguous(), mu.contiguous()
        check_input(explv, "explv")
        check_input(mu, "mu")
        out = torch.empty((), dtype=torch.float32, device=mu.device)
        call("hp_kld_forward", c_long(mu.numel()), batch, explv, mu, out, current_stream(mu.device))
        ctx.batch = batch
        ctx.save_for_backward(explv, mu)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        explv, mu = ctx.saved_tensors
        gv, gm = torch.empty_like(explv), torch.empty_like(mu)
        call("hp_kld_backward", c_long(mu.numel()), ctx.batch, explv, mu, g.contiguous(), gv, gm, current_stream(mu.device))
        return gv, gm, None


def kld_loss(explv, mu, batch=None):
    return KLDFunction.apply(explv, mu, mu.size(0) if batch is None else batch)


def sample_points(B, N, coef, seed, offset, device):
    """Decoder input points for B clouds (utils/points.py distribution) drawn on the device."""
    out = torch.empty((B, N, 3), dtype=torch.float32, device=device)
    call("hp_sample_points", c_long(B * N), float(coef), ctypes.c_ulonglong(seed & (2 ** 64 - 1)),
         ctypes.c_ulonglong(offset & (2 ** 64 - 1)), out, current_stream(device))
    return out


def slice_clouds(points, target=1024, seed=0, max_rounds=100000, planes=None):
    """Random-plane slicer (datasets/utils/dataset_generator.py:26-39) for a batch of clouds on the device.
    points (B,N,3) -> (part_with_target_points (B,target,3), rest (B,N-target,3), plane).
    planes=None: candidate planes are drawn on the device (Philox(seed)), fp32 classification; plane = (B,4) float32, the
    accepted plane.  planes = (B,R,4) or (R,4) float64 candidate (params, bias) rows — e.g. the sequence numpy's generator
    gives the reference: float64 classification exactly as HyperPlane.check_point, the reference's own split; plane = (B,)
    int32, the index of the accepted candidate."""
    points = points.contiguous()
    check_input(points, "points")
    B, N = points.size(0), points.size(1)
    dev = points.device
    a = torch.empty((B, target, 3), dtype=torch.float32, device=dev)
    b = torch.empty((B, N - target, 3), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:                            # nothing to launch, and status has no maximum: the empty parts
        return a, b, (torch.empty((0, 4), dtype=torch.float32, device=dev) if planes is None else
                      torch.empty((0,), dtype=torch.int32, device=dev))
    if planes is not None:
        planes = torch.as_tensor(planes, dtype=torch.float64).to(dev)
        if planes.dim() == 2:
            planes = planes.unsqueeze(0).expand(B, -1, -1)
        if planes.dim() != 3 or planes.size(0) != B or planes.size(2) != 4 or planes.size(1) == 0:
            raise HipExtensionError("planes must be (B,R,4) or (R,4) float64 with R > 0")
        planes = planes.contiguous()
        plane = torch.empty((B,), dtype=torch.int32, device=dev)
        call("hp_slice_clouds_planes", B, N, target, points, planes, planes.size(1), a, b, plane, status, current_stream(dev))
    else:
        plane = torch.empty((B, 4), dtype=torch.float32, device=dev)
        call("hp_slice_clouds", B, N, target, points, ctypes.c_ulonglong(seed & (2 ** 64 - 1)), max_rounds, a, b, plane, status,
             current_stream(dev))
    if int(status.max().item()) != 0:     # data preparation, not the training step: a host sync is fine here
        raise HipExtensionError(f"no plane with a {target}-point side found for {int((status != 0).sum())} cloud(s)")
    return a, b, plane


def rotation_table(device=None):
    """(360, 2) float32 rows (cos, sin) of a z-rotation by 0..359 degrees: the [0,0] and [1,0] entries of
    Rotation.from_euler('z', deg, degrees=True).as_matrix().astype(float32) (datasets/shapenet.py:73-92).  scipy goes through
    the unit quaternion (0, 0, sin(a/2), cos(a/2)), so the entries are w*w - z*z and 2*z*w in float64 — the same route here,
    which reproduces its float32 table in every row (cos(a) itself differs from it at 90 and 270 degrees)."""
    import numpy as np
    half = np.deg2rad(np.arange(360, dtype=np.float64)) / 2
    z, w = np.sin(half), np.cos(half)
    t = torch.from_numpy(np.stack([w * w - z * z, 2 * z * w], 1).astype(np.float32))
    return t if device is None else t.to(device)


def make_batch_default_groups(batch_size):
    """Workgroups per item: twice what fills the chip (256 CUs x 4 resident 4-wave workgroups at the 2048-point kernel's
    register count), over the items of the batch.  A call ends with its slowest item; the workgroups of the items that are
    done leave, and the second helping then shares that item's candidates in finer pieces (measured at B = 64: 32 groups
    9-20 % under 16, 64 slower again — DESIGN.md 3c)."""
    return max(1, min(64, -(-2048 // max(1, int(batch_size)))))


def make_batch_buffers(batch_size, n_points, target, device):
    """The output tensors of one make_batch call, allocated once by a caller that reuses them."""
    f = dict(dtype=torch.float32, device=device)
    return {"existing": torch.empty((batch_size, target, 3), **f), "missing": torch.empty((batch_size, n_points - target, 3), **f),
            "gt": torch.empty((batch_size, n_points, 3), **f), "plane": torch.empty((batch_size, 4), **f),
            "index": torch.empty((batch_size,), dtype=torch.int32, device=device)}


def make_batch_workspace(batch_size, n_points, device):
    nbytes = _long_fn("hp_make_batch_workspace_bytes", int(batch_size), int(n_points))
    if nbytes < 0:
        raise HipExtensionError(f"make_batch: unsupported shape B={batch_size}, N={n_points}")
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def make_batch(clouds, ids, streams, target=1024, degrees=None, rot=None, seed=0, max_candidates=400_000, groups=None,
               out=None, ws=None, failed=None):
    """One training batch from a device-resident dataset (csrc/batch_maker.hip) — asynchronous, no host synchronisation.
    clouds (M,N,3) float32; ids (B) int32 cloud numbers; streams (B) int64 RNG stream ids; degrees (B) int32 z-rotations
    (None: none) with rot = rotation_table(device).  Item b is split by the first accepted candidate plane of the sequence
    (seed, streams[b]) — whatever its place in the batch and whatever `groups`.
    Returns (existing (B,target,3), missing (B,N-target,3), gt (B,N,3), plane (B,4), index (B) int32, failed (1) int32):
    index -1 marks an item with no accepted plane below max_candidates (outputs: first `target` points / the rest), and
    `failed` — the caller's counter if given, never reset here — has risen by the number of such items.
    out / ws: make_batch_buffers / make_batch_workspace results to reuse."""
    check_input(clouds, "clouds")
    check_input(ids, "ids", torch.int32)
    check_input(streams, "streams", torch.int64)
    if clouds.dim() != 3 or clouds.size(2) != 3:
        raise HipExtensionError("clouds must be (M,N,3)")
    M, N, B = clouds.size(0), clouds.size(1), ids.numel()
    if streams.numel() != B:
        raise HipExtensionError("ids and streams must have one entry per item")
    dev = clouds.device
    if degrees is not None:
        check_input(degrees, "degrees", torch.int32)
        if degrees.numel() != B:
            raise HipExtensionError("degrees must have one entry per item")
        if rot is None:
            rot = rotation_table(dev)
        check_input(rot, "rot")
        if tuple(rot.shape) != (360, 2):
            raise HipExtensionError("rot must be (360,2)")
    if groups is None:
        groups = make_batch_default_groups(B)
    if out is None:
        out = make_batch_buffers(B, N, target, dev) if 0 < target < N and B > 0 else None
    if ws is None and out is not None:
        ws = make_batch_workspace(B, N, dev)
    if failed is None:
        failed = torch.zeros((1,), dtype=torch.int32, device=dev)
    o = out or {}
    call("hp_make_batch", M, N, int(target), clouds, B, ids, streams, degrees, rot if degrees is not None else None,
         ctypes.c_ulonglong(seed & (2 ** 64 - 1)), int(max_candidates), int(groups), o.get("existing"), o.get("missing"),
         o.get("gt"), o.get("plane"), o.get("index"), failed, ws, current_stream(dev))
    return out["existing"], out["missing"], out["gt"], out["plane"], out["index"], failed


SCAN_MAX_POINTS = 1 << 22      # HP_SCAN_MAX_POINTS
SCAN_MAX_TARGET = 8192


def _check_ragged(points, offsets):
    check_input(points, "points")
    check_input(offsets, "offsets", torch.int64)
    if points.dim() != 2 or points.size(1) != 3 or offsets.dim() != 1 or offsets.numel() < 2:
        raise HipExtensionError("a ragged set is points (T,3) and offsets (S+1) with S >= 1")
    return offsets.numel() - 1


# ---------------------------------------------------------------------------------------------
# What every wrapper below does around its call, stated once.  An output table has one row per member of the wrapper's
# `out` dict: (name, dtype, shape, empty) — shape a tuple of ints and dimension letters, resolved from the dict of sizes
# the wrapper hands to _outputs; empty the fill of the result served on the host when there is nothing to launch (None:
# nothing is written).
# ---------------------------------------------------------------------------------------------
class _Table(tuple):
    """The rows of an output table, with what _outputs needs of them that no call changes: `checks`, a (name, label, dtype,
    number of the shape) per row, and `resolve`, which turns the call's sizes into the table's distinct shapes."""


def _table(*rows):
    table = _Table(rows)
    shapes = list(dict.fromkeys(shape for _, _, shape, _ in rows))
    sizes = ["(" + "".join(f"d[{x!r}], " if type(x) is str else f"{x}, " for x in shape) + ")" for shape in shapes]
    table.resolve = eval("lambda d: (" + ", ".join(sizes) + ",)")      # e.g. lambda d: ((d['T'], ), (d['S'], 4, ),)
    table.checks = tuple((name, f"out['{name}']", dtype, shapes.index(shape)) for name, dtype, shape, _ in rows)
    return table


def _outputs(out, table, dims, device, what, exc=HipExtensionError, optional=None):
    """The `out` dict of one call: fresh tensors for the table's rows when out is None, else the caller's, each member
    through check_input and then the shape test, in row order.  optional: {name: allocate} — members a caller may set to
    None or leave out (they are then skipped), and whether a fresh dict gets them."""
    want = table.resolve(dims)
    if out is None:
        return {name: torch.empty(want[i], dtype=dtype, device=device) for name, _, dtype, i in table.checks
                if not optional or optional.get(name, True)}
    for name, label, dtype, i in table.checks:
        t = out.get(name)
        if t is None:
            if optional and name in optional:
                continue
            raise KeyError(name)
        check_input(t, label, dtype)
        if t.shape != want[i]:
            raise exc(f"out does not fit {what}")
    return out


def _serve_empty(out, rows):
    """The result of a call with nothing to launch (an empty tensor has no address): every member gets its row's fill."""
    for name, _, _, empty in rows:
        if empty is not None and out.get(name) is not None:
            out[name].fill_(empty)


def _workspace(ws, need, device, dtype, exc=HipExtensionError):
    """(ws, its bytes): a fresh workspace of `need` bytes, or the caller's — on the device, 16-byte aligned and large
    enough."""
    if ws is None:
        return torch.empty((need // dtype.itemsize,), dtype=dtype, device=device), need
    check_input(ws, "ws", ws.dtype)
    held = ws.nbytes
    if held < need or ws.device != device or ws.data_ptr() % 16:
        raise exc(f"ws must hold {need} bytes on the inputs' device, 16-byte aligned")
    return ws, held


def _plan(entry, args, n, message):
    """The n ints an hp_*_plan entry point answers `args` with; `message` where it refuses them."""
    v = [c_int(0) for _ in range(n)]
    if getattr(load_library(), entry)(*args, *[ctypes.byref(x) for x in v]) != 0:
        raise HipExtensionError(message)
    return tuple(x.value for x in v)


def _check_k(k, least=1):
    n = int(k)
    if not least <= n <= KNN_MAX_K:
        raise HipExtensionError(f"{least} <= k <= {KNN_MAX_K} is required, got k = {k}")
    return n


def _check_ratio(ratio):
    ratio = float(ratio)
    if not 0.0 <= ratio <= 3.0e38:
        raise HipExtensionError(f"0 <= ratio (finite) is required, got {ratio}")
    return ratio


_FP32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103       # the least double that fp32 rounds to +inf


def _check_fp32_square(value, name):
    """A radius or threshold the kernels square in fp32: non-negative, and the square finite.  The product of two fp32
    values is exact in a double, so it is finite in fp32 iff it stays below the rounding boundary."""
    value = float(value)
    v32 = ctypes.c_float(value).value
    if not (value >= 0.0 and v32 * v32 < _FP32_OVERFLOW):
        raise HipExtensionError(f"0 <= {name} with a finite fp32 square is required, got {value}")
    return value


def _check_streams(streams, n, per):
    if streams is not None:
        check_input(streams, "streams", torch.int64)
        if tuple(streams.shape) != (n,):
            raise HipExtensionError(f"streams must have one entry per {per}")


def _seed_word(seed):
    return ctypes.c_ulonglong(int(seed) & (2 ** 64 - 1))


def _per_scan(value, name, S, device, exc=HipExtensionError, none_too=False):
    """A positive edge length for every scan as the (S) float32 tensor the kernels read: one float for all, or the caller's
    tensor; with none_too, None stays None."""
    if isinstance(value, torch.Tensor):
        check_input(value, name)
        if value.shape != (S,) or value.device != device:
            raise exc(f"{name} must be a float or an (S) tensor on the points' device")
        return value
    if value is None and none_too:
        return None
    v32 = ctypes.c_float(float(value)).value
    if not 0.0 < v32 < float("inf"):
        raise exc(f"{name} must be a positive finite float (in fp32 too){', an (S) tensor or None' if none_too else ''}, got {value}")
    return torch.full((S,), v32, dtype=torch.float32, device=device)


def _check_queries(points, T, S, queries, query_offsets, exclude_self):
    """The query set of the nearest-neighbour wrappers -> (own, exclude_self, Q): whether the scans (T rows) query
    themselves, the resolved default of exclude_self and the number of queries."""
    if (queries is None) != (query_offsets is None):
        raise HipExtensionError("queries and query_offsets come together")
    own = queries is None or queries.data_ptr() == points.data_ptr()
    if exclude_self is None:
        exclude_self = queries is None
    if own and not exclude_self:
        raise HipExtensionError("a scan queried with itself needs exclude_self: every row would find itself first")
    if queries is None:
        return own, exclude_self, T
    if _check_ragged(queries, query_offsets) != S:
        raise HipExtensionError("query_offsets must have one entry per scan, plus one")
    if queries.device != points.device:
        raise HipExtensionError("queries and points must be on one device")
    return own, exclude_self, queries.size(0)


def scan_boxes(points, offsets):
    """Bounding boxes of S ragged scans (csrc/scan_prep.hip): points (T,3) float32, offsets (S+1) int64; scan s is rows
    offsets[s] .. offsets[s+1].  Returns (center (S,3), scale (S)): the box's middle and its largest side / 0.9, in fp32 as
    datasets/real_data.py:26-33.  For (K,N,3) clouds pass points.view(-1,3) and offsets = arange(K+1) * N."""
    S = _check_ragged(points, offsets)
    center = torch.empty((S, 3), dtype=torch.float32, device=points.device)
    scale = torch.empty((S,), dtype=torch.float32, device=points.device)
    call("hp_scan_boxes", S, points, offsets, center, scale, current_stream(points.device))
    return center, scale


_PREPARE_OUT = _table(("existing", torch.float32, ("B", "target", 3), None), ("index", torch.int32, ("B", "target"), None))


def prepare_scans_buffers(batch_size, target, device):
    """The output tensors of one prepare_scans call, allocated once by a caller that reuses them."""
    return _outputs(None, _PREPARE_OUT, {"B": batch_size, "target": target}, device, "B and target")


def prepare_scans(points, offsets, ids, streams, target=1024, replace=False, seed=0, center=None, scale=None, out=None,
                  failed=None):
    """B fixed-size clouds from ragged scans in one call (csrc/scan_prep.hip) — asynchronous, no host synchronisation.
    points (T,3) float32 and offsets (S+1) int64 as scan_boxes; ids (B) int32 scan numbers; streams (B) int64 RNG stream ids.
    Item b is scan ids[b] brought to `target` points by the law of include/hyperpocket_hip.h, a pure function of
    (seed, streams[b], n, target, replace): the whole scan plus drawn repeats when it is short; when it is long, a uniform
    subset in scan order (replace=False) or `target` draws with replacement (replace=True).  center (S,3) / scale (S)
    — scan_boxes' results — normalise the rows as (p - center) / scale; without them the rows are copied bit for bit.
    Returns (existing (B,target,3), index (B,target) int32 rows of the scan, failed (1) int32): an id outside [0,S) gives
    zero rows, index -1 and raises `failed` — the caller's counter if given, never reset here — by one.
    out: a prepare_scans_buffers result to reuse."""
    S = _check_ragged(points, offsets)
    check_input(ids, "ids", torch.int32)
    check_input(streams, "streams", torch.int64)
    B = ids.numel()
    if streams.numel() != B:
        raise HipExtensionError("ids and streams must have one entry per item")
    if (center is None) != (scale is None):
        raise HipExtensionError("center and scale come together")
    if center is not None:
        check_input(center, "center")
        check_input(scale, "scale")
        if tuple(center.shape) != (S, 3) or tuple(scale.shape) != (S,):
            raise HipExtensionError("center must be (S,3) and scale (S)")
    if not (B >= 1 and 1 <= target <= SCAN_MAX_TARGET):
        raise HipExtensionError(f"B >= 1 items and 1 <= target <= {SCAN_MAX_TARGET} are required, got B = {B}, target = {target}")
    dev = points.device
    out = _outputs(out, _PREPARE_OUT, {"B": B, "target": target}, dev, "B and target")
    if failed is None:
        failed = torch.zeros((1,), dtype=torch.int32, device=dev)
    call("hp_prepare_scans", B, points, offsets, S, ids, streams, _seed_word(seed), int(target),
         bool(replace), center, scale, out["existing"], out["index"], failed, current_stream(dev))
    return out["existing"], out["index"], failed


def restore_scans(completions, s_scale, center, scale):
    """Completions of normalised scans back in the scans' coordinates (datasets/real_data.py:63-67):
    (c / s_scale) * scale + center, one fp32 rounding per operation.  completions (K,N,3); s_scale (K) = scan_boxes'
    scale of the completions themselves; center (K,3) or (3) and scale (K) or () = the scans' boxes, per row or one for all."""
    check_input(completions, "completions")
    if completions.dim() != 3 or completions.size(2) != 3:
        raise HipExtensionError("completions must be (K,N,3)")
    K, N = completions.size(0), completions.size(1)
    center = center.expand(K, 3).contiguous()
    scale, s_scale = scale.expand(K).contiguous(), s_scale.expand(K).contiguous()
    for t, n in ((s_scale, "s_scale"), (center, "center"), (scale, "scale")):
        check_input(t, n)
    out = torch.empty_like(completions)
    call("hp_restore_scans", K, N, completions, s_scale, center, scale, out, current_stream(completions.device))
    return out


FPS_MAX_POINTS = 8192          # HP_FPS_MAX_POINTS


_FPS_OUT = _table(("index", torch.int32, ("B", "k"), None), ("radius2", torch.float32, ("B", "k"), None))


def farthest_points_buffers(batch_size, k, device):
    """The output tensors of one farthest_points call, allocated once by a caller that reuses them."""
    return _outputs(None, _FPS_OUT, {"B": batch_size, "k": k}, device, "B and k")


def farthest_points(clouds, k, counts=None, start=None, out=None, failed=None):
    """k farthest-point picks out of each of B clouds in one launch (csrc/fps.hip) — asynchronous, no host synchronisation.
    clouds (B,P,3) float32 with 1 <= P <= FPS_MAX_POINTS; counts (B) int32: the valid rows of each cloud (default P), rows at
    or beyond them are never read; start (B) int32: the first pick (default row 0); 1 <= k <= 8192.  The law is in
    include/hyperpocket_hip.h: pick_j is the row farthest from picks 0..j-1 (fp32 squared distance, one rounding per
    operation, equal distances broken by the lowest row); with fewer than k distinct rows the tail repeats row 0.
    Returns (index (B,k) int32, radius2 (B,k) float32): radius2[b,j] is the squared covering radius of the first j+1 picks
    over the cloud.  counts[b] outside [1,P] or start[b] outside [0,counts[b]) gives an index row of -1, a radius2 row of 0
    and raises `failed` — the caller's (1) int32 counter if given, never reset here — by one.
    out: a farthest_points_buffers result to reuse; with its "radius2" None no radii are written and None is returned."""
    check_input(clouds, "clouds")
    if clouds.dim() != 3 or clouds.size(2) != 3:
        raise HipExtensionError("clouds must be (B,P,3)")
    B, P, k = clouds.size(0), clouds.size(1), int(k)
    if not (1 <= P <= FPS_MAX_POINTS and 1 <= k <= FPS_MAX_POINTS):
        raise HipExtensionError(f"1 <= P <= {FPS_MAX_POINTS} and 1 <= k <= {FPS_MAX_POINTS} are required, got P = {P}, k = {k}")
    for t, name in ((counts, "counts"), (start, "start")):
        if t is not None:
            check_input(t, name, torch.int32)
            if tuple(t.shape) != (B,):
                raise HipExtensionError(f"{name} must have one entry per cloud")
    dev = clouds.device
    out = _outputs(out, _FPS_OUT, {"B": B, "k": k}, dev, "B and k", optional={"radius2": True})   # None: no radii wanted
    if failed is None:
        failed = torch.zeros((1,), dtype=torch.int32, device=dev)
    else:
        check_input(failed, "failed", torch.int32)
    if B == 0:                                             # nothing to launch (and an empty tensor has no address)
        return out["index"], out.get("radius2")
    call("hp_farthest_points", B, P, clouds, counts, start, k, out["index"], out.get("radius2"), failed, current_stream(dev))
    return out["index"], out.get("radius2")


KNN_MAX_POINTS = 65536         # HP_KNN_MAX_POINTS
KNN_MAX_K = 32


def knn_points_plan(k):
    """(instance_k, threads, tile) of the kernel instance that serves k (hp_knn_points_plan): the compile-time list length
    (8, 16 or 32), the queries per workgroup and the candidates per LDS tile.  Host only."""
    return _plan("hp_knn_points_plan", (int(k),), 3, f"1 <= k <= {KNN_MAX_K} is required, got k = {k}")


_KNN_OUT = _table(("index", torch.int32, ("Q", "k"), -1), ("dist2", torch.float32, ("Q", "k"), float("inf")))
_KNN_GRID_OUT = _table(*_KNN_OUT, ("grid", torch.float32, ("S", 4), 0))           # grid: only where the caller brings it


def _check_knn(points, offsets, k):
    """-> (S, k as an int, T)"""
    S, k, T = _check_ragged(points, offsets), _check_k(k), points.size(0)
    if T > S * KNN_MAX_POINTS:                             # known without reading the offsets: some scan is beyond the cap
        raise HipExtensionError(f"a scan holds at most {KNN_MAX_POINTS} points for the nearest-neighbour kernels, "
                                f"got {T} rows in {S} scan(s)")
    return S, k, T


def knn_points(points, offsets, k, queries=None, query_offsets=None, exclude_self=None, out=None):
    """The k nearest rows of its scan for every query (csrc/knn.hip) — asynchronous, no host synchronisation.
    points (T,3) float32 and offsets (S+1) int64 as scan_boxes; queries (Q,3) / query_offsets (S+1): a second ragged set over
    the same S scans, default the scans themselves; 1 <= k <= 32; a scan holds at most KNN_MAX_POINTS rows (brute force).
    The law is in include/hyperpocket_hip.h, per scan: d2 = ((dx*dx + dy*dy) + dz*dz) with one fp32 rounding per operation;
    a row with a non-finite coordinate is absent (nobody's neighbour, and as a query it gets the empty result); the
    candidates of a query are the present rows of its scan — without row i itself under exclude_self — ordered by
    (d2, row), equal distances to the lower row; the first k are the result.
    exclude_self: default True for the scans themselves (False is refused there: every row would find itself) and False
    for given queries; with given queries it skips the candidate with the query's own row number.
    Returns (index (Q,k) int32 rows within the scan, dist2 (Q,k) float32); slots beyond the number of candidates hold -1
    and +inf, and so do all slots of the queries of a scan longer than KNN_MAX_POINTS (its length lives on the device).
    out: {"index", "dist2"} tensors to reuse; both are fully overwritten."""
    S, k, T = _check_knn(points, offsets, k)
    own, exclude_self, Q = _check_queries(points, T, S, queries, query_offsets, exclude_self)
    dev = points.device
    out = _outputs(out, _KNN_OUT, {"Q": Q, "k": k}, dev, "the queries and k")
    if Q == 0 or T == 0:                      # nothing to launch (and an empty tensor has no address)
        _serve_empty(out, _KNN_OUT)
        return out["index"], out["dist2"]
    call("hp_knn_points", S, points, offsets, queries, query_offsets, k, bool(exclude_self), out["index"], out["dist2"],
         current_stream(dev))
    return out["index"], out["dist2"]


_OUTLIER_OUT = _table(("keep", torch.uint8, ("T",), None), ("mean_dist", torch.float32, ("T",), None), ("kept", torch.int32, ("S",), 0))
_KEEP_OUT = _table(("keep", torch.uint8, ("T",), None), ("kept", torch.int32, ("S",), 0))     # outlier_keep's


def scan_outliers(points, offsets, k=16, ratio=2.0, out=None):
    """Statistical outlier removal of S ragged scans (csrc/knn.hip) — asynchronous, no host synchronisation, bit-reproducible.
    points (T,3) float32, offsets (S+1) int64 as scan_boxes; 1 <= k <= 32; 0 <= ratio; a scan holds at most KNN_MAX_POINTS rows.
    The law is in include/hyperpocket_hip.h, per scan: m_i = the mean distance of row i to its (up to) k nearest
    neighbours (knn_points' law; the roots summed in fp64 in slot order, the mean rounded to fp32); rows with a non-finite
    coordinate, without a neighbour or with a non-finite m_i are absent.  With M the largest m_i, the m_i are cut to 24-bit
    integers q_i = trunc(m_i * 2^(23 - floor(log2 M))), their sums S1 and S2 are exact, and row i stays iff
    q_i <= mu + ratio * sqrt(var) with mu = S1 / n_p and var = max(0, (S2 - mu * S1) / (n_p - 1)) in fp64; a scan with at
    most one participating row, or with M == 0, keeps its participants.
    Returns (keep (T) uint8, mean_dist (T) float32 — +inf for absent rows, kept (S) int32 rows kept per scan).
    out: {"keep", "mean_dist", "kept"} tensors to reuse."""
    S, _, T = _check_knn(points, offsets, k)
    ratio, dev = _check_ratio(ratio), points.device
    out = _outputs(out, _OUTLIER_OUT, {"S": S, "T": T}, dev, "the scans")
    if T == 0:
        _serve_empty(out, _OUTLIER_OUT)
        return out["keep"], out["mean_dist"], out["kept"]
    call("hp_scan_outliers", S, points, offsets, int(k), ratio, out["keep"], out["mean_dist"], out["kept"], current_stream(dev))
    return out["keep"], out["mean_dist"], out["kept"]


KNN_GRID_MAX_POINTS = 1 << 22  # HP_KNN_GRID_MAX_POINTS (= SCAN_MAX_POINTS)


def knn_grid_plan(k):
    """(instance_k, threads, tile) of the kernel instance of knn_points_grid that serves k (hp_knn_grid_plan): the compile-time
    list length (8, 16 or 32), the threads per workgroup (one wave: 64 queries share a block of cells) and the candidates per
    LDS tile.  Host only."""
    return _plan("hp_knn_grid_plan", (int(k),), 3, f"1 <= k <= {KNN_MAX_K} is required, got k = {k}")


def _knn_grid_workspace_bytes(S, T, Q=None):
    fn = load_library().hp_knn_grid_workspace_bytes
    fn.restype = ctypes.c_longlong
    need = fn(int(S), ctypes.c_longlong(int(T)), ctypes.c_longlong(0 if Q is None else int(Q)))
    if need < 0:
        raise HipExtensionError(f"S >= 1 scans and 0 <= T, Q rows are required, got S = {S}, T = {T}, Q = {Q}")
    return need


def knn_grid_buffers(S, T, device, Q=None):
    """The workspace of one knn_points_grid / scan_outliers_grid call over S scans of T rows in all (Q: the rows of a second
    query set, None without one), allocated once by a caller that reuses it: pass it as `ws`."""
    return _workspace(None, max(_knn_grid_workspace_bytes(S, T, Q), 16), device, torch.int64)[0]


def _check_knn_grid(points, offsets, k, cell):
    S = _check_ragged(points, offsets)
    _check_k(k)
    return S, _per_scan(cell, "cell", S, points.device, none_too=True)                # None: the default edge


def knn_points_grid(points, offsets, k, queries=None, query_offsets=None, exclude_self=None, cell=None, out=None, ws=None):
    """knn_points behind a uniform grid (csrc/knn_grid.hip) — the same lists, bit for bit, for scans of up to
    KNN_GRID_MAX_POINTS rows; asynchronous, no host synchronisation.
    Arguments and law as knn_points: the grid only decides which rows a query looks at, and nothing of it shows in the
    result.  cell: None for the default edge (from the scan's occupied surface, about k/2 rows per occupied cell), a positive
    float for all scans or an (S) float32 device tensor (an entry that is not positive and finite means the default) — a
    request, raised on the device as far as 1024 cells per axis and 2 n_s + 64 cells per scan demand.
    Returns (index (Q,k) int32 rows within the scan, dist2 (Q,k) float32); slots beyond the number of candidates hold -1 and
    +inf, and so do all slots of the queries of a scan longer than KNN_GRID_MAX_POINTS (its length lives on the device).
    out: {"index", "dist2"} tensors to reuse, both fully overwritten; with a "grid" (S,4) float32 tensor in it, that receives
    (h, G_x, G_y, G_z) per scan — zeros for a scan that is not searched.  ws: a knn_grid_buffers result to reuse."""
    S, cell = _check_knn_grid(points, offsets, k, cell)
    k = int(k)
    T, dev = points.size(0), points.device
    own, exclude_self, Q = _check_queries(points, T, S, queries, query_offsets, exclude_self)
    out = _outputs(out, _KNN_GRID_OUT, {"S": S, "Q": Q, "k": k}, dev, "the queries and k", optional={"grid": False})
    grid = out.get("grid")
    if grid is not None and grid.device != dev:
        raise HipExtensionError("out['grid'] must be on the points' device")
    ws, ws_bytes = _workspace(ws, _knn_grid_workspace_bytes(S, T, None if own else Q), dev, torch.int64)
    if Q == 0 or T == 0:                                   # nothing to launch (and an empty tensor has no address)
        _serve_empty(out, _KNN_GRID_OUT)
        return out["index"], out["dist2"]
    call("hp_knn_grid", S, points, offsets, None if own else queries, None if own else query_offsets, k, bool(exclude_self),
         cell, out["index"], out["dist2"], None, grid, ws, ctypes.c_longlong(ws_bytes), current_stream(dev))
    return out["index"], out["dist2"]


def outlier_keep(mean_dist, offsets, ratio=2.0, out=None):
    """The statistics half of scan_outliers over given m_i (csrc/knn_grid.hip) — asynchronous, no host synchronisation.
    mean_dist (T) float32: the rows' mean neighbour distances, +inf (or any non-finite value) for an absent row; offsets
    (S+1) int64; scans of up to KNN_GRID_MAX_POINTS rows (a longer one keeps nothing).  scan_outliers' law with S2 an exact
    integer of up to 70 bits, rounded to double to nearest even: equal to scan_outliers' keep wherever that is defined.
    Returns (keep (T) uint8, kept (S) int32).  out: {"keep", "kept"} tensors to reuse."""
    check_input(mean_dist, "mean_dist")
    check_input(offsets, "offsets", torch.int64)
    if mean_dist.dim() != 1 or offsets.dim() != 1 or offsets.numel() < 2:
        raise HipExtensionError("mean_dist must be (T) and offsets (S+1) with S >= 1")
    ratio = _check_ratio(ratio)
    S, T, dev = offsets.numel() - 1, mean_dist.size(0), mean_dist.device
    out = _outputs(out, _KEEP_OUT, {"S": S, "T": T}, dev, "the scans")
    if T == 0:
        _serve_empty(out, _KEEP_OUT)
        return out["keep"], out["kept"]
    call("hp_outlier_keep", S, mean_dist, offsets, ratio, out["keep"], out["kept"], current_stream(dev))
    return out["keep"], out["kept"]


def scan_outliers_grid(points, offsets, k=16, ratio=2.0, cell=None, out=None, ws=None):
    """scan_outliers behind knn_points_grid's search (csrc/knn_grid.hip) — the same keep, mean_dist and kept, bit for bit, for
    scans of up to KNN_GRID_MAX_POINTS rows; asynchronous, no host synchronisation.  Arguments as scan_outliers; cell and ws
    as knn_points_grid.  A scan beyond the cap keeps nothing (all its rows absent).
    Returns (keep (T) uint8, mean_dist (T) float32, kept (S) int32).  out: {"keep", "mean_dist", "kept"} tensors to reuse."""
    S, cell = _check_knn_grid(points, offsets, k, cell)
    ratio = _check_ratio(ratio)
    T, dev = points.size(0), points.device
    out = _outputs(out, _OUTLIER_OUT, {"S": S, "T": T}, dev, "the scans")
    ws, ws_bytes = _workspace(ws, _knn_grid_workspace_bytes(S, T, None), dev, torch.int64)
    if T == 0:
        _serve_empty(out, _OUTLIER_OUT)
        return out["keep"], out["mean_dist"], out["kept"]
    call("hp_scan_outliers_grid", S, points, offsets, int(k), ratio, cell, out["keep"], out["mean_dist"], out["kept"], ws,
         ctypes.c_longlong(ws_bytes), current_stream(dev))
    return out["keep"], out["mean_dist"], out["kept"]


def scan_normals_plan(k):
    """(instance_k, threads, sweeps) of the kernel instance that serves k (hp_scan_normals_plan): the compile-time list length
    (8, 16 or 32), the rows per workgroup and the Jacobi sweeps of the law.  Host only."""
    return _plan("hp_scan_normals_plan", (int(k),), 3, f"2 <= k <= {KNN_MAX_K} is required, got k = {k}")


_NORMALS_OUT = _table(("normal", torch.float32, ("T", 3), None), ("curvature", torch.float32, ("T",), None),
                ("count", torch.int32, ("T",), None))


def scan_normals(points, offsets, k=16, viewpoints=None, index=None, out=None):
    """Surface normals and surface variation of S ragged scans by local principal components (csrc/normals.hip) —
    asynchronous, no host synchronisation, bit-reproducible.
    points (T,3) float32, offsets (S+1) int64 as scan_boxes; 2 <= k <= 32.  index None: the lists come from knn_points(k)
    first, so a scan holds at most KNN_MAX_POINTS rows; a given index must be int32 (T,k) on the same device — rows within
    the scan, knn_points' format — and skips the search, for callers that hold lists already or bring their own (then
    scans of any length).  viewpoints: (S,3), or one (3,) for all scans — where the sensor stood; None leaves the sign rule.
    The law is in include/hyperpocket_hip.h, per row i: its neighbourhood is row i plus every slot of its list that names a
    present (finite) row of the scan, 0 <= index < n_s — any other slot is empty; count is its size, 0 for an absent row.
    The differences p_j - p_i (fp32) are cut to 21-bit integers q = trunc(dq * 2^(19 - e)), e the exponent of the largest
    |dq_c| (scan_plane's frame); C = count * sum(q q^T) - sum(q) sum(q)^T is exact in int64 and in fp64; six cyclic Jacobi
    sweeps in fp64 (pairs (0,1), (0,2), (1,2), one rounding per operation, no convergence exit) diagonalise it.  The normal
    is the column of the smallest diagonal entry, normalised, its largest component made positive, then negated where it
    points away from the viewpoint (n . (v - p_i) < 0), rounded to fp32.  The curvature is the surface variation
    max(lambda_min, 0) / trace(C): 0 on a plane, 1/3 for an isotropic neighbourhood.  A row with count < 3, with all its
    neighbours on itself or with an overflowed difference has no normal: three NaNs and a NaN curvature — so has every
    row of a scan beyond KNN_MAX_POINTS under index=None (its lists are empty, count 1).
    Returns (normal (T,3) float32, curvature (T) float32, count (T) int32).
    out: {"normal", "curvature", "count"} tensors to reuse; all are fully overwritten."""
    k = _check_k(k, 2)
    S = _check_knn(points, offsets, k)[0] if index is None else _check_ragged(points, offsets)
    T, dev = points.size(0), points.device
    if index is not None:
        check_input(index, "index", torch.int32)
        if index.device != dev or tuple(index.shape) != (T, k):
            raise HipExtensionError(f"index must be (T,k) = ({T},{k}) int32 on the points' device, got {tuple(index.shape)}")
    if viewpoints is not None:
        check_input(viewpoints, "viewpoints")
        if viewpoints.device != dev or tuple(viewpoints.shape) not in ((3,), (S, 3)):
            raise HipExtensionError(f"viewpoints must be (S,3) = ({S},3) or (3,) on the points' device, got {tuple(viewpoints.shape)}")
        if viewpoints.dim() == 1:
            viewpoints = viewpoints.expand(S, 3).contiguous()
    out = _outputs(out, _NORMALS_OUT, {"T": T}, dev, "the scans")
    if T == 0:                                             # nothing to launch (and an empty tensor has no address)
        return out["normal"], out["curvature"], out["count"]
    if index is None:
        index, _ = knn_points(points, offsets, k)
    call("hp_scan_normals", S, points, offsets, k, index, viewpoints, out["normal"], out["curvature"], out["count"],
         current_stream(dev))
    return out["normal"], out["curvature"], out["count"]


CLUSTER_MAX_POINTS = 32768     # HP_CLUSTER_MAX_POINTS


def scan_clusters_plan(max_points=None):
    """(threads, tile, lds_bytes) of the cluster kernel for a bound on the longest scan (hp_scan_clusters_plan): rows per
    block of a scan, candidates per LDS tile and the LDS a workgroup takes.  Host only."""
    max_points = CLUSTER_MAX_POINTS if max_points is None else int(max_points)
    return _plan("hp_scan_clusters_plan", (max_points,), 3, f"1 <= max_points <= {CLUSTER_MAX_POINTS} is required, got {max_points}")


_CLUSTER_OUT = _table(("label", torch.int32, ("T",), None), ("size", torch.int32, ("T",), None), ("clusters", torch.int32, ("S",), 0),
                ("largest", torch.int32, ("S",), -1))


def scan_clusters(points, offsets, radius, max_points=None, out=None):
    """Euclidean clusters of S ragged scans (csrc/clusters.hip) — asynchronous, no host synchronisation, bit-reproducible.
    points (T,3) float32, offsets (S+1) int64 as scan_boxes; 0 <= radius with a finite square; max_points: the caller's bound
    on the longest scan, 1 <= max_points <= CLUSTER_MAX_POINTS, default the cap (a smaller one lets more scans share a
    compute unit).
    The law is in include/hyperpocket_hip.h, per scan: rows i != j are joined iff both are present (finite) and
    d2(i, j) = ((dx*dx + dy*dy) + dz*dz) <= radius * radius, each operation one fp32 rounding, the test inclusive;
    label is the smallest row of the row's connected component (-1 for an absent row), size the component's rows (0),
    clusters the components per scan, largest the label of the one with the most rows (ties to the smaller label, -1 when no
    row is present).  A scan longer than max_points gets the empty result — its length lives on the device.
    Returns (label (T) int32 rows within the scan, size (T) int32, clusters (S) int32, largest (S) int32).
    out: {"label", "size", "clusters", "largest"} tensors to reuse; all are fully overwritten."""
    S = _check_ragged(points, offsets)
    max_points = CLUSTER_MAX_POINTS if max_points is None else int(max_points)
    if not 1 <= max_points <= CLUSTER_MAX_POINTS:
        raise HipExtensionError(f"1 <= max_points <= {CLUSTER_MAX_POINTS} is required, got {max_points}")
    radius = _check_fp32_square(radius, "radius")
    T, dev = points.size(0), points.device
    out = _outputs(out, _CLUSTER_OUT, {"S": S, "T": T}, dev, "the scans")
    if T == 0:                                             # nothing to launch (and an empty tensor has no address)
        _serve_empty(out, _CLUSTER_OUT)
        return out["label"], out["size"], out["clusters"], out["largest"]
    call("hp_scan_clusters", S, points, offsets, radius, max_points, out["label"], out["size"], out["clusters"], out["largest"],
         current_stream(dev))
    return out["label"], out["size"], out["clusters"], out["largest"]


PLANE_MAX_TRIALS = 4096        # HP_PLANE_MAX_TRIALS

_PLANE_OUT = _table(("trial", torch.int32, ("S",), -1), ("inliers", torch.int32, ("S",), 0), ("found", torch.int32, ("S",), 0),
              ("sample", torch.int32, ("S", 3), -1), ("sample_plane", torch.float32, ("S", 4), float("nan")),
              ("inlier", torch.uint8, ("T",), None), ("moments", torch.int64, ("S", 10), 0), ("shift", torch.int32, ("S",), 0))
_PLANE_SIDE_OUT = _table(("dist", torch.float32, ("T",), None), ("keep", torch.uint8, ("T",), None), ("kept", torch.int32, ("S",), 0))


def scan_plane_plan(trials=512):
    """(threads, rows_per_lane, trial_tile) of the consensus kernel (hp_scan_plane_plan): a workgroup of `threads` lanes
    holds threads * rows_per_lane consecutive rows of the ragged set and walks a scan's hypotheses trial_tile at a time
    through LDS.  Host only."""
    return _plan("hp_scan_plane_plan", (int(trials),), 3, f"1 <= trials <= {PLANE_MAX_TRIALS} is required, got {trials}")


def _check_plane_trials(trials):
    if not 1 <= int(trials) <= PLANE_MAX_TRIALS:
        raise HipExtensionError(f"1 <= trials <= {PLANE_MAX_TRIALS} is required, got {trials}")
    return int(trials)


def scan_plane_buffers(S, T, trials, device):
    """(out, ws) of one scan_plane call over S scans of T rows in all, allocated once by a caller that reuses them."""
    need = _long_fn("hp_scan_plane_workspace_bytes", int(S), _check_plane_trials(trials))
    if need < 0:
        raise HipExtensionError(f"S >= 1 is required, got {S}")
    return (_outputs(None, _PLANE_OUT, {"S": int(S), "T": int(T)}, device, "the scans"),
            _workspace(None, need, device, torch.int64)[0])


def _check_plane_lengths(points, S):
    if points.size(0) > S * SCAN_MAX_POINTS:               # known without reading the offsets: some scan is beyond the cap
        raise HipExtensionError(f"a scan holds at most {SCAN_MAX_POINTS} points, got {points.size(0)} rows in {S} scan(s)")


def scan_plane(points, offsets, threshold, trials=512, seed=0, streams=None, min_inliers=3, min_share=0.0, out=None, ws=None):
    """The dominant plane of each of S ragged scans by random sample consensus (csrc/plane.hip) — asynchronous, no host
    synchronisation, bit-reproducible.  points (T,3) float32, offsets (S+1) int64 as scan_boxes; 0 <= threshold with a finite
    square, the half width of the plane's band; 1 <= trials <= PLANE_MAX_TRIALS; streams (S) int64 RNG stream ids, default
    the scan's number; min_inliers >= 3 and 0 <= min_share <= 1 decide `found`.  A scan holds up to SCAN_MAX_POINTS rows: the
    cost is O(n * trials), so this stage takes whole scenes, before the capped neighbour and cluster kernels.
    The law is in include/hyperpocket_hip.h, per scan: trial h samples three rows by Philox (seed, stream, tag 4),
    nrm = (b - a) x (c - a), and row p is an inlier iff e*e <= threshold^2 * |nrm|^2 with e = nrm . (p - a), every operation
    one fp32 rounding, the test inclusive, no root and no division; rows with a non-finite coordinate are absent; a trial
    with a repeated, collinear or absent sample is invalid; the winner is the valid trial with the most inliers, ties to the
    lower trial.
    Returns a dict: trial (S) int32 (-1: no valid trial, then the rest is empty), inliers (S) int32, found (S) int32
    (inliers >= min_inliers and inliers >= min_share * n), sample (S,3) int32 rows within the scan, sample_plane (S,4)
    float32 (nx, ny, nz, d) not normalised, inlier (T) uint8 the winner's mask, moments (S,10) int64
    [cnt, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz] of the inliers' q = trunc((p - a) * 2^(19 - shift)) — exact integers, for
    plane_from_moments — and shift (S) int32.  A scan shorter than 3 rows or longer than SCAN_MAX_POINTS gets the empty
    result — its length lives on the device.
    out, ws: a scan_plane_buffers(S, T, trials, device) pair to reuse; all outputs are fully overwritten."""
    S = _check_ragged(points, offsets)
    trials, threshold = _check_plane_trials(trials), _check_fp32_square(threshold, "threshold")
    min_inliers, min_share = int(min_inliers), float(min_share)
    if min_inliers < 3 or not 0.0 <= min_share <= 1.0:
        raise HipExtensionError(f"min_inliers >= 3 and 0 <= min_share <= 1 are required, got {min_inliers} and {min_share}")
    _check_plane_lengths(points, S)
    T, dev = points.size(0), points.device
    _check_streams(streams, S, "scan")
    out = _outputs(out, _PLANE_OUT, {"S": S, "T": T}, dev, "the scans")
    ws, _ = _workspace(ws, _long_fn("hp_scan_plane_workspace_bytes", S, trials), dev, torch.int64)
    if T == 0:                                             # nothing to launch (and an empty tensor has no address)
        _serve_empty(out, _PLANE_OUT)
        return out
    call("hp_scan_plane", S, points, offsets, streams, _seed_word(seed), trials,
         ctypes.c_float(threshold), min_inliers, ctypes.c_float(min_share), out["trial"], out["inliers"], out["found"],
         out["sample"], out["sample_plane"], out["inlier"], out["moments"], out["shift"], ws, current_stream(dev))
    return out


def scan_plane_side(points, offsets, planes, threshold, out=None):
    """Every row of S ragged scans against its scan's plane (csrc/plane.hip) — asynchronous, no host synchronisation.
    planes (S,4) float32 (nx, ny, nz, d), given and not sampled — a refitted plane_from_moments result rounded to fp32;
    dist = ((nx*x + ny*y) + nz*z) + d, one fp32 rounding per operation, NaN for a row with a non-finite coordinate;
    keep = the row is present and not |dist| <= threshold (a NaN plane keeps every present row).
    Returns (dist (T) float32, keep (T) uint8, kept (S) int32 rows kept per scan).  out: {"dist", "keep", "kept"} to reuse."""
    S = _check_ragged(points, offsets)
    threshold = _check_fp32_square(threshold, "threshold")
    check_input(planes, "planes")
    if tuple(planes.shape) != (S, 4) or planes.device != points.device:
        raise HipExtensionError("planes must be (S,4) on the points' device")
    T, dev = points.size(0), points.device
    out = _outputs(out, _PLANE_SIDE_OUT, {"S": S, "T": T}, dev, "the scans")
    if T == 0:
        _serve_empty(out, _PLANE_SIDE_OUT)
        return out["dist"], out["keep"], out["kept"]
    call("hp_scan_plane_side", S, points, offsets, planes, ctypes.c_float(threshold), out["dist"], out["keep"], out["kept"],
         current_stream(dev))
    return out["dist"], out["keep"], out["kept"]


def plane_from_moments(moments, shift, sample_plane, anchor):
    """The least-squares plane of each scan's inliers from scan_plane's integer moments — a host function, numpy fp64 over
    S small problems.  moments (S,10), shift (S), sample_plane (S,4): scan_plane's; anchor (S,3): the coordinates of the
    sample row a (sample[:, 0]) the q's are measured from.  The scatter matrix cnt * Sqq - Sq Sq^T is formed in exact Python
    integers and only then converted; its eigenvector of the smallest eigenvalue (numpy.linalg.eigh) is the unit normal,
    oriented along the sample's normal; the centroid is anchor + mean * 2^(shift - 19) and d = -normal . centroid.
    With cnt < 3 or a middle eigenvalue of 0 (the inliers lie on a line) it is the normalised sample_plane (NaN where the
    scan has none).  Returns (S,4) float64 (nx, ny, nz, d)."""
    import numpy as np
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    moments, shift = host(moments).reshape(-1, 10), host(shift).reshape(-1)
    sample_plane = host(sample_plane).astype(np.float64).reshape(-1, 4)
    anchor = host(anchor).astype(np.float64).reshape(-1, 3)
    S = len(moments)
    if not (len(shift) == len(sample_plane) == len(anchor) == S):
        raise ValueError("moments, shift, sample_plane and anchor must have one row per scan")
    out = np.empty((S, 4), dtype=np.float64)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for s in range(S):
        m = [int(v) for v in moments[s]]
        with np.errstate(all="ignore"):
            out[s] = sample_plane[s] / np.sqrt((sample_plane[s, :3] ** 2).sum())      # the fallback
        if m[0] < 3:
            continue
        scatter = np.empty((3, 3), dtype=np.float64)
        for k, (i, j) in enumerate(pairs):
            scatter[i, j] = scatter[j, i] = float(m[0] * m[4 + k] - m[1 + i] * m[1 + j])
        values, vectors = np.linalg.eigh(scatter)
        if not values[1] > 0:
            continue
        normal = vectors[:, 0]
        if normal @ sample_plane[s, :3] < 0:
            normal = -normal
        centroid = anchor[s] + np.ldexp(np.array(m[1:4], dtype=np.float64) / m[0], int(shift[s]) - 19)
        out[s, :3] = normal
        out[s, 3] = -(normal @ centroid)
    return out


def rotation_to_axis(normal, axis=(0, 1, 0)):
    """The minimal rotation (3,3) float64 that takes `normal` to `axis` (both are normalised here): the rotation in the plane
    of the two, Rodrigues' I + K + K^2 / (1 + c) with K the cross-product matrix of normal x axis and c their cosine — a host
    function.  Where c < 0 the formula loses its digits (1 + c -> 0), so the turn is made in two steps about the same axis
    k = normal x axis: the half-turn 2 k k^T - I, which takes the normal to its opposite, then Rodrigues for the small rest.
    Exactly antiparallel, k is any perpendicular.
    Meant for DeviceScanDataset(transform=...): a scan's fitted plane normal becomes the training data's up axis."""
    import numpy as np
    n, a = np.asarray(normal, dtype=np.float64).reshape(3), np.asarray(axis, dtype=np.float64).reshape(3)
    ln, la = np.linalg.norm(n), np.linalg.norm(a)
    if not (np.isfinite(ln) and np.isfinite(la) and ln > 0 and la > 0):
        raise ValueError("normal and axis must be finite and non-zero")
    n, a = n / ln, a / la
    half = np.eye(3)
    if n @ a < 0:
        k = np.cross(n, a)
        if np.linalg.norm(k) < 1e-150:
            k = np.zeros(3)
            k[np.argmin(np.abs(n))] = 1.0
            k = np.cross(n, k)
        k /= np.linalg.norm(k)
        k -= (k @ n) * n                                   # exactly perpendicular to n: the half-turn is exact on it
        k /= np.linalg.norm(k)
        half = 2.0 * np.outer(k, k) - np.eye(3)
        n = half @ n
    v = np.cross(n, a)
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return (np.eye(3) + K + K @ K / (1.0 + n @ a)) @ half


ALIGN_MAX_POINTS = 65536       # HP_ALIGN_MAX_POINTS: rows per source set and per target set
ALIGN_MAX_HYPOTHESES = 64      # HP_ALIGN_MAX_HYPOTHESES
_ALIGN_SHIFT = (-100, 128)     # the range of align_frame's shift
_ALIGN_DEGENERATE = 2.0 ** -40


def scan_align_plan(hypotheses=1):
    """(threads, rows_per_lane, hypothesis_group, tile) of the sweep of scan_align_step for H hypotheses
    (hp_scan_align_plan): a workgroup of `threads` lanes holds threads * rows_per_lane consecutive source rows of the ragged
    set, each moved under hypothesis_group transforms (1 for H == 1), and walks the targets `tile` at a time through LDS.
    Host only."""
    return _plan("hp_scan_align_plan", (int(hypotheses),), 4,
                 f"1 <= hypotheses <= {ALIGN_MAX_HYPOTHESES} is required, got {hypotheses}")


def _check_max_dist(max_dist):
    max_dist = float(max_dist)
    if not max_dist >= 0.0:
        raise HipExtensionError(f"max_dist >= 0 (+inf: no gate) is required, got {max_dist}")
    return max_dist


def _check_align_sets(points, offsets, tpoints, toffsets):
    S = _check_ragged(points, offsets)
    if _check_ragged(tpoints, toffsets) != S:
        raise HipExtensionError("toffsets must have one entry per set, plus one")
    if tpoints.device != points.device:
        raise HipExtensionError("the sources and the targets must be on one device")
    return S


_ALIGN_OUT = _table(("moments", torch.int64, ("S", "H", "width"), 0), ("index", torch.int32, ("H", "T"), -1),
              ("dist2", torch.float32, ("H", "T"), float("inf")))
_ALIGN_MOMENTS_OUT = _table(_ALIGN_OUT[0])     # without want_index


def _align_step(entry, width, points, offsets, tpoints, toffsets, transforms, max_dist, anchor, shift, out, want_index, extra=()):
    """The body of scan_align_step and scan_align_plane_step: the checks of the sets, the transforms and the frame, the out
    dict with moments (S,H,width), the empty result on the host, and the call of `entry`, `extra` (further arrays of the
    targets) behind toffsets."""
    S = _check_align_sets(points, offsets, tpoints, toffsets)
    max_dist = _check_max_dist(max_dist)
    dev, T, U = points.device, points.size(0), tpoints.size(0)
    check_input(transforms, "transforms")
    if transforms.dim() != 3 or transforms.size(0) != S or transforms.size(2) != 12 \
            or not 1 <= transforms.size(1) <= ALIGN_MAX_HYPOTHESES:
        raise HipExtensionError(f"transforms must be (S,H,12) with 1 <= H <= {ALIGN_MAX_HYPOTHESES}")
    H = transforms.size(1)
    check_input(anchor, "anchor")
    check_input(shift, "shift", torch.int32)
    if tuple(anchor.shape) != (S, 3) or tuple(shift.shape) != (S,):
        raise HipExtensionError("anchor must be (S,3) and shift (S)")
    rows = _ALIGN_OUT if want_index else _ALIGN_MOMENTS_OUT
    out = _outputs(out, rows, {"S": S, "H": H, "T": T, "width": width}, dev, "the sets and the hypotheses")
    if T == 0 or U == 0:                                   # nothing to launch (and an empty tensor has no address)
        _serve_empty(out, rows)
        return out
    call(entry, S, H, ctypes.c_longlong(T), points, offsets, ctypes.c_longlong(U), tpoints, toffsets, *extra, transforms,
         ctypes.c_float(max_dist), anchor, shift, out["moments"], out["index"] if want_index else None,
         out["dist2"] if want_index else None, current_stream(dev))
    return out


def scan_align_step(points, offsets, tpoints, toffsets, transforms, max_dist, anchor, shift, out=None, want_index=False):
    """One step of point-to-point rigid registration for S x H jobs (csrc/align.hip) — asynchronous, no host synchronisation,
    bit-reproducible.  points (T,3) float32 / offsets (S+1) int64: the sources; tpoints (U,3) / toffsets (S+1): the targets,
    a second ragged set over the same S sets; transforms (S,H,12) float32, row-major [R | t], 1 <= H <=
    ALIGN_MAX_HYPOTHESES; 0 <= max_dist, +inf for no gate; anchor (S,3) float32 and shift (S) int32: align_frame's.
    The law is in include/hyperpocket_hip.h, per job (s, h): every source row is moved, p' = R p + t with one fp32 rounding
    per operation, and matched with the finite target row of set s at the smallest d2 = ((dx*dx + dy*dy) + dz*dz), ties to
    the lower row; it is a correspondence iff d2 <= max_dist^2; u and v are p' and the target row as integers of the frame,
    trunc((. - anchor) * 2^(19 - shift)), clipped (counted, not summed) at 2^20.
    Returns a dict: moments (S,H,18) int64 = [used, clipped, sum u (3), sum v (3), sum u_a v_b (9), sum |u - v|^2] — exact
    integers, for rigid_from_moments — and, with want_index, index (H,T) int32 (the matched row within the target set, -1
    for none) and dist2 (H,T) float32 (+inf for none).  A set that is empty, holds more than ALIGN_MAX_POINTS rows on either
    side or reaches beyond its tensor gets the empty result — its length lives on the device.
    out: the dict of an earlier call to reuse; all of it is fully overwritten."""
    return _align_step("hp_scan_align_step", 18, points, offsets, tpoints, toffsets, transforms, max_dist, anchor, shift, out,
                       want_index)


def align_frame(tpoints, toffsets, max_dist):
    """The integer frame of an alignment from the targets' boxes (scan_boxes) — one host read, at the start of an alignment.
    anchor (S,3) float32 is the target box centre (0 where it is not finite).  With half = float64(scale) * 0.45, half the
    box's longest side, and x = half + min(max_dist, half): shift (S) int32 is the smallest integer e with x < 2^e, clamped
    to [-100, 128], 0 for a set without a box.  scan_align_step clips a component at 2^(shift + 1), twice that bound: no
    target row is ever clipped, and no gated correspondence while max_dist <= 3 * half.  Returns (anchor, shift) on the
    targets' device."""
    import numpy as np
    max_dist = float(np.float32(_check_max_dist(max_dist)))
    center, scale = scan_boxes(tpoints, toffsets)
    center, scale = center.cpu().numpy(), scale.cpu().numpy()      # the host read
    anchor = np.where(np.isfinite(center), center, np.float32(0)).astype(np.float32)
    shift = np.zeros(len(scale), dtype=np.int32)
    for s in range(len(scale)):
        half = float(scale[s]) * 0.45
        x = half + min(max_dist, half)
        if np.isnan(x):
            continue
        e = _ALIGN_SHIFT[1] if x == np.inf else _ALIGN_SHIFT[0] if x <= 0 else int(np.frexp(x)[1])   # 2^(e-1) <= x < 2^e
        shift[s] = min(max(e, _ALIGN_SHIFT[0]), _ALIGN_SHIFT[1])
    return torch.from_numpy(anchor).to(tpoints.device), torch.from_numpy(shift).to(tpoints.device)


def _solve_jobs(moments, shift, anchor, width, solve_one):
    """The frame of rigid_from_moments and rigid_from_plane_moments: moments (S,width) or (S,H,width), shift (S), anchor (S,3)
    from tensors or arrays, and solve_one(m, back, anchor_s) for every job — m the job's moments as Python integers, back =
    shift - 19 — which returns (rms, (R, t)), or (rms, None) where there is no motion to be had: the identity, ok False."""
    import numpy as np
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    moments, shift, anchor = host(moments), host(shift).reshape(-1), host(anchor).astype(np.float64).reshape(-1, 3)
    lead = moments.shape[:-1]
    S = len(shift)
    if moments.shape[-1] != width or not lead or lead[0] != S or len(anchor) != S:
        raise ValueError(f"moments must be (S,{width}) or (S,H,{width}), shift (S) and anchor (S,3)")
    mom = moments.reshape(S, -1, width)
    J = mom.shape[1]
    delta = np.zeros((S, J, 3, 4), dtype=np.float64)
    delta[:, :, :, :3] = np.eye(3)
    ok, rms = np.zeros((S, J), dtype=bool), np.full((S, J), np.inf, dtype=np.float64)
    for s in range(S):
        for j in range(J):
            rms[s, j], motion = solve_one([int(x) for x in mom[s, j]], int(shift[s]) - 19, anchor[s])
            if motion is not None:
                delta[s, j, :, :3], delta[s, j, :, 3] = motion
                ok[s, j] = True
    return delta.reshape(lead + (3, 4)), ok.reshape(lead), rms.reshape(lead)


def rigid_from_moments(moments, shift, anchor):
    """The least-squares rigid motion of each job from scan_align_step's integer moments — a host function, numpy fp64 over
    S x H small problems, the counterpart of plane_from_moments.  moments (S,18) or (S,H,18); shift (S), anchor (S,3): the
    frame.  The cross-covariance cnt * Suv - Su Sv^T and Horn's symmetric 4x4 matrix are formed in exact Python integers
    (they reach 2^72) and only then converted; the eigenvector of its largest eigenvalue (numpy.linalg.eigh) is the unit
    quaternion of R, and t = c_v - R c_u with c = anchor + mean * 2^(shift - 19).  With cnt < 3, or the two largest
    eigenvalues equal (within 2^-40 of the largest magnitude: the rows lie on a line), the motion is the identity and ok is
    False.  Returns (delta (...,3,4) float64, ok (...) bool, rms (...) float64 = sqrt([17] / cnt) * 2^(shift - 19), +inf
    without a correspondence)."""
    import numpy as np

    def solve_one(m, back, anchor_s):
        cnt = m[0]
        rms = np.ldexp(np.sqrt(m[17] / cnt), back) if cnt > 0 else np.inf
        if cnt < 3:
            return rms, None
        c = [[cnt * m[8 + 3 * a + b] - m[2 + a] * m[5 + b] for b in range(3)] for a in range(3)]
        N = np.array([[c[0][0] + c[1][1] + c[2][2], c[1][2] - c[2][1], c[2][0] - c[0][2], c[0][1] - c[1][0]],
                      [c[1][2] - c[2][1], c[0][0] - c[1][1] - c[2][2], c[0][1] + c[1][0], c[2][0] + c[0][2]],
                      [c[2][0] - c[0][2], c[0][1] + c[1][0], c[1][1] - c[0][0] - c[2][2], c[1][2] + c[2][1]],
                      [c[0][1] - c[1][0], c[2][0] + c[0][2], c[1][2] + c[2][1], c[2][2] - c[0][0] - c[1][1]]],
                     dtype=object).astype(np.float64)
        values, vectors = np.linalg.eigh(N)
        if not values[3] - values[2] > _ALIGN_DEGENERATE * max(abs(values[0]), abs(values[3])):
            return rms, None
        w, x, y, z = vectors[:, 3] / np.linalg.norm(vectors[:, 3])
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        cu = anchor_s + np.ldexp(np.array(m[2:5], dtype=np.float64) / cnt, back)
        cv = anchor_s + np.ldexp(np.array(m[5:8], dtype=np.float64) / cnt, back)
        return rms, (R, cv - R @ cu)

    return _solve_jobs(moments, shift, anchor, 18, solve_one)


def yaw_transforms(H, axis, src_center, dst_center):
    """H starts of a yaw search — a host function, float64: the rotation by 2 pi h / H about `axis` (normalised here,
    Rodrigues' formula) that takes src_center to dst_center, t = dst - R src.  src_center, dst_center: (3) or (S,3).
    Returns (H,3,4) or (S,H,3,4) float64, row-major [R | t]."""
    import numpy as np
    k = np.asarray(axis, dtype=np.float64).reshape(3)
    if not (np.isfinite(k).all() and np.linalg.norm(k) > 0) or int(H) < 1:
        raise ValueError("axis must be finite and non-zero and H >= 1")
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    src, dst = np.asarray(src_center, dtype=np.float64), np.asarray(dst_center, dtype=np.float64)
    out = np.empty(src.shape[:-1] + (int(H), 3, 4), dtype=np.float64)
    for h in range(int(H)):
        angle = 2.0 * np.pi * h / int(H)
        R = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
        out[..., h, :, :3] = R
        out[..., h, :, 3] = dst - src @ R.T
    return out


def _compose(delta, T):
    import numpy as np
    out = np.empty((3, 4), dtype=np.float64)
    out[:, :3] = delta[:, :3] @ T[:, :3]
    out[:, 3] = delta[:, :3] @ T[:, 3] + delta[:, 3]
    return out


def _align_start(init, S):
    """The (S,3,4) float64 starts of a refinement: `init`, or the identity."""
    import numpy as np
    if init is None:
        T = np.zeros((S, 3, 4), dtype=np.float64)
        T[:, :, :3] = np.eye(3)
        return T
    T = np.array(init.cpu().numpy() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
    if T.shape != (S, 3, 4):
        raise HipExtensionError("init must be (S,3,4)")
    return T


def _align_refine(run, solve, T, shift, anchor, iters, tol):
    """The refinement of scan_align and scan_align_plane.  run(T (S,H,3,4) float64) is one step on the device at T's float32
    rounding and returns its moments on the host; solve is the step's rigid_from_*_moments.  `iters` times T <- delta o T
    wherever the solve is ok, fewer once every set's delta is within tol of the identity (rotation angle in radians,
    translation over the frame's 2^shift; tol = 0 never stops); one more step measures the result.  T is updated in place.
    Returns (T, ok (S), rms (S), matched (S) int64)."""
    import numpy as np
    for _ in range(iters):
        delta, ok, _ = solve(run(T[:, None]), shift, anchor)
        still = False
        for s in range(len(T)):
            if ok[s, 0]:
                T[s] = _compose(delta[s, 0], T[s])
                R = delta[s, 0, :, :3]
                twist = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
                angle = float(np.arctan2(np.linalg.norm(twist) / 2, (np.trace(R) - 1) / 2))
                move = float(np.ldexp(np.linalg.norm(delta[s, 0, :, 3]), -int(shift[s])))
                still = still or not (angle <= tol and move <= tol)
        if tol > 0 and not still:
            break
    mom = run(T[:, None])
    _, ok, rms = solve(mom, shift, anchor)
    return T, ok[:, 0], rms[:, 0], mom[:, 0, 0].astype(np.int64)


def scan_align(points, offsets, tpoints, toffsets, max_dist, iters=30, tol=0.0, init=None, yaw=0, axis=(0, 1, 0), coarse_iters=3):
    """Point-to-point ICP of S source sets onto their target sets: scan_align_step on the device, rigid_from_moments on the
    host.  The host reads one (S,H,18) block of moments per iteration, because the solve is a host function — 144 bytes a
    job; nothing else crosses, the rows stay on the device — and the targets' boxes once, for align_frame.
    The transforms are kept in float64; each step runs at their float32 rounding and T <- delta o T wherever the solve is ok.
    init: (S,3,4) starts, default the identity.  yaw = H > 0 (not with init): H starts turned by 2 pi h / H about `axis`
    through the box centres (yaw_transforms: the source box centre goes to the target's) run coarse_iters steps together,
    each refined on its own; one more step scores them and each set keeps the hypothesis with the most correspondences,
    then the lower sum |u - v|^2, then the lower h.  The refinement runs `iters` steps with H = 1, fewer once every set's
    delta is within tol of the identity (rotation angle in radians, translation over the frame's 2^shift; tol = 0 never
    stops); one more step measures the result.
    Returns (transforms (S,3,4) float64 source -> target, ok (S) bool — at least three correspondences in general position
    at the end —, rms (S) float64 of the quantised correspondences, matched (S) int64 their number, hypothesis (S) int64 the
    chosen h, -1 without yaw): numpy arrays on the host.  A set beyond ALIGN_MAX_POINTS rows on either side matches nothing
    (ok False): thin it first."""
    import numpy as np
    S = _check_align_sets(points, offsets, tpoints, toffsets)
    max_dist = _check_max_dist(max_dist)
    yaw, iters, coarse_iters, tol = int(yaw), int(iters), int(coarse_iters), float(tol)
    if iters < 0 or coarse_iters < 0 or not 0 <= yaw <= ALIGN_MAX_HYPOTHESES or not tol >= 0:
        raise HipExtensionError(f"iters >= 0, coarse_iters >= 0, 0 <= yaw <= {ALIGN_MAX_HYPOTHESES} and tol >= 0 are required")
    if yaw and init is not None:
        raise HipExtensionError("yaw makes its own starts: init cannot be given with it")
    dev = points.device
    anchor_d, shift_d = align_frame(tpoints, toffsets, max_dist)
    anchor, shift = anchor_d.cpu().numpy(), shift_d.cpu().numpy()
    bufs = {}

    def run(T):
        t32 = torch.from_numpy(np.ascontiguousarray(T.astype(np.float32).reshape(S, -1, 12))).to(dev)
        H = t32.size(1)
        bufs[H] = scan_align_step(points, offsets, tpoints, toffsets, t32, max_dist, anchor_d, shift_d, out=bufs.get(H))
        return bufs[H]["moments"].cpu().numpy()                    # the host read of the iteration

    hypothesis = np.full(S, -1, dtype=np.int64)
    if yaw:
        centres = [np.nan_to_num(scan_boxes(p, o)[0].cpu().numpy().astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
                   for p, o in ((points, offsets), (tpoints, toffsets))]
        TH = yaw_transforms(yaw, axis, centres[0], centres[1])
        for _ in range(coarse_iters):
            delta, ok, _ = rigid_from_moments(run(TH), shift, anchor)
            for s in range(S):
                for h in range(yaw):
                    if ok[s, h]:
                        TH[s, h] = _compose(delta[s, h], TH[s, h])
        mom = run(TH)
        T = np.empty((S, 3, 4), dtype=np.float64)
        for s in range(S):
            hypothesis[s] = min(range(yaw), key=lambda h: (-int(mom[s, h, 0]), int(mom[s, h, 17]), h))
            T[s] = TH[s, hypothesis[s]]
    else:
        T = _align_start(init, S)
    return _align_refine(run, rigid_from_moments, T, shift, anchor, iters, tol) + (hypothesis,)


_ALIGN_PLANE_MOMENTS = 60
_ALIGN_PLANE_DEGENERATE = 2.0 ** -11       # lambda_min / lambda_max of the block-scaled system (tests/align_plane_law.py has the measurement)


def scan_align_plane_plan(hypotheses=1):
    """(threads, rows_per_lane, hypothesis_group, tile) of the sweep of scan_align_plane_step for H hypotheses
    (hp_scan_align_plane_plan), as scan_align_plan; hypothesis_group is 1 for every H.  Host only."""
    return _plan("hp_scan_align_plane_plan", (int(hypotheses),), 4,
                 f"1 <= hypotheses <= {ALIGN_MAX_HYPOTHESES} is required, got {hypotheses}")


def scan_align_plane_step(points, offsets, tpoints, toffsets, tnormals, transforms, max_dist, anchor, shift, out=None,
                          want_index=False):
    """One step of point-to-plane rigid registration for S x H jobs (csrc/align_plane.hip) — asynchronous, no host
    synchronisation, bit-reproducible.  The arguments are scan_align_step's, plus tnormals (U,3) float32, the targets'
    normals row for row (scan_normals' output); the transform, the match, the gate and the integer frame are its rules, so
    index and dist2 are its bit for bit.
    The law is in include/hyperpocket_hip.h.  A correspondence matched to target row j takes w = trunc(n_j * 2^9); it is
    without normal (counted, not summed) when n_j is not finite, rounds to zero or is no unit vector (w.w > 2^18 + 2^11);
    otherwise, with u and v the moved row and the target row as integers of the frame, a = (u x w, w) and b = -(u - v).w.
    Returns a dict: moments (S,H,60) int64 = [used, clipped, without normal, 0, then (hi, lo) of 28 sums: the 21 a_i a_j
    (i <= j, row-major), the 6 a_i b, b b] with every term split as lo = term & (2^31 - 1), hi = term >> 31 — exact
    integers, for rigid_from_plane_moments — and, with want_index, index (H,T) int32 and dist2 (H,T) float32 as
    scan_align_step's.  Sets with the empty result are scan_align_step's.
    out: the dict of an earlier call to reuse; all of it is fully overwritten."""
    check_input(tnormals, "tnormals")
    if tnormals.device != points.device or tuple(tnormals.shape) != (tpoints.size(0), 3):
        raise HipExtensionError(f"tnormals must be (U,3) = ({tpoints.size(0)},3) on the points' device, got {tuple(tnormals.shape)}")
    return _align_step("hp_scan_align_plane_step", _ALIGN_PLANE_MOMENTS, points, offsets, tpoints, toffsets, transforms, max_dist,
                       anchor, shift, out, want_index, extra=(tnormals,))


def rigid_from_plane_moments(moments, shift, anchor):
    """The Gauss-Newton step of the point-to-plane error of each job from scan_align_plane_step's integer moments — a host
    function, numpy fp64 over S x H small problems, the counterpart of rigid_from_moments.  moments (S,60) or (S,H,60);
    shift (S), anchor (S,3): the frame.  The 28 sums are rebuilt as hi * 2^31 + lo in Python integers (they reach 2^78) and
    only then converted: A (6x6) = sum a a^T, g = sum a b.  A x = g, x = (omega, t'), is solved in the scaling D^-1 A D^-1,
    D = (r, r, r, m, m, m), r^2 and m^2 the mean diagonal of the rotation and of the translation block — one scale per block
    takes the units out and leaves the anisotropy within a block to be seen.  The motion is the exact rotation by |omega|
    about omega through the anchor and t = t' * 2^(shift - 19).  With fewer than 6 used correspondences, a zero on A's
    diagonal, or lambda_min <= 2^-11 lambda_max of the scaled matrix (numpy.linalg.eigh: the surface lets the source
    slide, as a plane, a sphere or a cylinder does) the motion is the identity and ok is False.  Returns (delta (...,3,4)
    float64, ok (...) bool, rms (...) float64 = sqrt(sum b b / used) * 2^(shift - 28), the rms point-to-plane distance, +inf
    without a used correspondence)."""
    import numpy as np
    pairs = [(i, j) for i in range(6) for j in range(i, 6)]

    def solve_one(m, back, anchor_s):
        used = m[0]
        sums = [m[4 + 2 * i] * (1 << 31) + m[5 + 2 * i] for i in range(28)]
        rms = np.ldexp(np.sqrt(sums[27] / used), back - 9) if used > 0 else np.inf
        if used < 6:
            return rms, None
        A = [[0] * 6 for _ in range(6)]
        for k, (a, b) in enumerate(pairs):
            A[a][b] = A[b][a] = sums[k]
        A = np.array(A, dtype=object).astype(np.float64)
        g = np.array(sums[21:27], dtype=object).astype(np.float64)
        diag = np.diagonal(A)
        if not (diag > 0).all():
            return rms, None
        r, t = np.sqrt((diag[0] + diag[1] + diag[2]) / 3.0), np.sqrt((diag[3] + diag[4] + diag[5]) / 3.0)
        D = np.array([r, r, r, t, t, t])
        scaled = A / D[:, None] / D[None, :]
        values = np.linalg.eigh(scaled)[0]
        if not values[0] > _ALIGN_PLANE_DEGENERATE * values[5]:
            return rms, None
        x = np.linalg.solve(scaled, g / D) / D
        angle = float(np.linalg.norm(x[:3]))
        R = np.eye(3)
        if angle != 0:
            k = x[:3] / np.linalg.norm(x[:3])
            K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
            R = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
        return rms, (R, anchor_s - R @ anchor_s + np.ldexp(x[3:], back))

    return _solve_jobs(moments, shift, anchor, _ALIGN_PLANE_MOMENTS, solve_one)


def scan_align_plane(points, offsets, tpoints, toffsets, max_dist, iters=10, tol=0.0, init=None, tnormals=None, k=16):
    """Point-to-plane ICP of S source sets onto their target sets: scan_align_plane_step on the device,
    rigid_from_plane_moments on the host — the refinement for surfaces: where scan_align's point-to-point error pulls every
    row to its nearest sample and the pose crawls along the surface, this one reaches the noise floor in about three steps
    from a start within some 15 degrees.  tnormals None: the targets' normals come from scan_normals(tpoints, toffsets, k)
    once, before the first step; they are not recomputed.  The host reads one (S,1,60) block of moments per iteration —
    480 bytes a job — and the targets' boxes once, for align_frame.
    The transforms are kept in float64; each step runs at their float32 rounding and T <- delta o T wherever the solve is
    ok.  init: (S,3,4) starts, default the identity (there is no yaw search here: give scan_align's poses).  `iters` steps,
    fewer once every set's delta is within tol of the identity (as scan_align); one more step measures the result.
    Returns (transforms (S,3,4) float64 source -> target, ok (S) bool — at least six used correspondences on a surface that
    holds all six freedoms at the end —, rms (S) float64 the rms point-to-plane distance, matched (S) int64 the used
    correspondences): numpy arrays on the host."""
    import numpy as np
    S = _check_align_sets(points, offsets, tpoints, toffsets)
    max_dist = _check_max_dist(max_dist)
    iters, tol = int(iters), float(tol)
    if iters < 0 or not tol >= 0:
        raise HipExtensionError("iters >= 0 and tol >= 0 are required")
    dev = points.device
    T = _align_start(init, S)
    if tnormals is None:
        tnormals = scan_normals(tpoints, toffsets, k)[0]
    anchor_d, shift_d = align_frame(tpoints, toffsets, max_dist)
    anchor, shift = anchor_d.cpu().numpy(), shift_d.cpu().numpy()
    buf = [None]

    def run(T):
        t32 = torch.from_numpy(np.ascontiguousarray(T.astype(np.float32).reshape(S, 1, 12))).to(dev)
        buf[0] = scan_align_plane_step(points, offsets, tpoints, toffsets, tnormals, t32, max_dist, anchor_d, shift_d, out=buf[0])
        return buf[0]["moments"].cpu().numpy()                     # the host read of the iteration

    return _align_refine(run, rigid_from_plane_moments, T, shift, anchor, iters, tol)


FEATURE_WIDTH = 36             # bytes of a descriptor: 3 x 11 bins and 3 zero bytes
POSE_MAX_TRIALS = 65536        # HP_POSE_MAX_TRIALS
POSE_MAX_KEEP = 4096           # HP_POSE_MAX_KEEP

_FEATURE_OUT = _table(("features", torch.uint8, ("T", FEATURE_WIDTH), None), ("count", torch.int32, ("T",), None),
                ("ws", torch.uint8, ("bytes",), None))
_MATCH_OUT = _table(("match", torch.int32, ("T",), -1), ("dist", torch.int32, ("T",), -1))
_POSE_OUT = (("trial", torch.int32, ()), ("inliers", torch.int32, ()), ("found", torch.int32, ()),
             ("transform", torch.float32, (12,)), ("valid", torch.int32, ()), ("kept", torch.int32, ()))     # name, dtype, tail
_POSE_ROWS = _table(*((name, dtype, ("S",) + tail, None) for name, dtype, tail in _POSE_OUT))   # no fills: the entry point
#                                                                                                  answers empty sets itself


def scan_features_plan(k):
    """(instance_k, threads, width) of the kernel instance that serves k (hp_scan_features_plan): the compile-time list length
    (8, 16 or 32), the rows per workgroup and the bytes of a descriptor.  Host only."""
    return _plan("hp_scan_features_plan", (int(k),), 3, f"1 <= k <= {KNN_MAX_K} is required, got k = {k}")


def scan_features(points, offsets, normals, index, out=None):
    """Fast point feature histograms of S ragged scans from given normals and neighbour lists (csrc/features.hip) —
    asynchronous, no host synchronisation, bit-reproducible.
    points (T,3) float32, offsets (S+1) int64 as scan_boxes; normals (T,3) float32 row for row (scan_normals' output: unit
    length, and consistently oriented — towards the sensor — or descriptors of two scans do not compare); index (T,k) int32,
    1 <= k <= 32, rows within the scan: knn_points' format, scan_normals' slot rules (a slot outside [0, n_s), the row
    itself, or a row without finite coordinates and a finite non-zero normal is empty).
    The law is in include/hyperpocket_hip.h, per row i with its listed neighbours j: d = p_j - p_i in fp32, then fp64 with one
    rounding per operation.  The end whose normal has the larger |n . d| is the source; phi = ns . d / |d|,
    v = (d x ns) / |d x ns|, w = ns x v, alpha = v . nt, theta the angle of (ns . nt, w . nt); a pair with d = 0 or d along ns
    is skipped.  alpha and phi fall into floor(11 (f + 1) / 2), theta into 11 bins of (-pi, pi] decided by sign tests against
    ten tabulated directions — no library function decides a bit.  SPFH(i) is the 33 counts over m_i pairs;
    FPFH(i) = SPFH(i) / m_i + (sum_j (w_j / m_j) SPFH(j)) / sum_j w_j with w_j = 1 / |d|^2 over the listed neighbours with
    m_j > 0 in list order; each group of 11 bins is scaled to trunc(255 F_b / sum F).
    Returns (features (T,36) uint8 — bytes 33..35 are zero —, count (T) int32 = m_i).  A row with count 0 (absent, without a
    normal, without a valid pair, or of no scan) has all-zero bytes and no descriptor for scan_feature_match.
    out: {"features", "count", "ws"} tensors to reuse (ws: T * 36 bytes of uint8); features and count are fully overwritten."""
    S = _check_ragged(points, offsets)
    T, dev = points.size(0), points.device
    check_input(normals, "normals")
    check_input(index, "index", torch.int32)
    if normals.device != dev or tuple(normals.shape) != (T, 3):
        raise HipExtensionError(f"normals must be (T,3) = ({T},3) on the points' device, got {tuple(normals.shape)}")
    if index.device != dev or index.dim() != 2 or index.size(0) != T or not 1 <= index.size(1) <= KNN_MAX_K:
        raise HipExtensionError(f"index must be (T,k) int32 with 1 <= k <= {KNN_MAX_K} on the points' device, got {tuple(index.shape)}")
    out = _outputs(out, _FEATURE_OUT, {"T": T, "bytes": T * FEATURE_WIDTH}, dev, "the scans")
    if T == 0:                                             # nothing to launch (and an empty tensor has no address)
        return out["features"], out["count"]
    call("hp_scan_features", S, ctypes.c_longlong(T), points, offsets, normals, index.size(1), index, out["features"], out["count"],
         out["ws"], current_stream(dev))
    return out["features"], out["count"]


def scan_feature_match_plan():
    """(threads, rows_per_lane, tile) of scan_feature_match's sweep (hp_scan_feature_match_plan): a workgroup of `threads`
    lanes holds threads * rows_per_lane consecutive source rows and walks the target descriptors `tile` at a time through
    LDS.  Host only."""
    return _plan("hp_scan_feature_match_plan", (), 3, "hp_scan_feature_match_plan failed")


def _check_descriptors(features, offsets, counts, name):
    check_input(features, name, torch.uint8)
    check_input(offsets, f"{name}' offsets", torch.int64)
    check_input(counts, f"{name}' counts", torch.int32)
    if features.dim() != 2 or features.size(1) != FEATURE_WIDTH or offsets.dim() != 1 or offsets.numel() < 2 \
            or tuple(counts.shape) != (features.size(0),) or offsets.device != features.device or counts.device != features.device:
        raise HipExtensionError(f"{name} must be (T,{FEATURE_WIDTH}) uint8 with offsets (S+1) and counts (T) on one device")
    return offsets.numel() - 1


def scan_feature_match(features, offsets, tfeatures, toffsets, counts, tcounts, out=None):
    """The nearest target descriptor of every source row, set by set (csrc/features.hip) — asynchronous, no host
    synchronisation, bit-reproducible.  features (T,36) uint8 / offsets (S+1) int64 / counts (T) int32: the sources,
    scan_features' output; tfeatures (U,36) / toffsets (S+1) / tcounts (U): the targets, a second ragged set over the same S
    sets.  A row with count <= 0 has no descriptor: it is matched to nothing and nothing is matched to it.
    The law is in include/hyperpocket_hip.h: the squared distance over the 36 bytes, an exact integer (at most
    33 * 255^2 < 2^22, formed as |a|^2 + |b|^2 - 2 a . b from nine 4 x 8-bit dot products a pair), the smallest one of the set,
    ties to the lower target row.  No ratio test and no mutual filter: scan_pose_trials' edge test does the sifting.
    Returns (match (T) int32 the target row within the set, -1 for none; dist (T) int32, -1 for none).  A set that is empty,
    holds more than ALIGN_MAX_POINTS rows on either side or reaches beyond its tensor gets the empty result — its length
    lives on the device.  out: {"match", "dist"} tensors to reuse; both are fully overwritten."""
    S = _check_descriptors(features, offsets, counts, "features")
    if _check_descriptors(tfeatures, toffsets, tcounts, "tfeatures") != S:
        raise HipExtensionError("toffsets must have one entry per set, plus one")
    if tfeatures.device != features.device:
        raise HipExtensionError("the sources and the targets must be on one device")
    T, U, dev = features.size(0), tfeatures.size(0), features.device
    out = _outputs(out, _MATCH_OUT, {"T": T}, dev, "the sources")
    if T == 0 or U == 0:                                   # nothing to launch (and an empty tensor has no address)
        _serve_empty(out, _MATCH_OUT)
        return out["match"], out["dist"]
    call("hp_scan_feature_match", S, ctypes.c_longlong(T), features, offsets, ctypes.c_longlong(U), tfeatures, toffsets, counts,
         tcounts, out["match"], out["dist"], current_stream(dev))
    return out["match"], out["dist"]


def _check_pose_trials(trials, keep):
    trials, keep = int(trials), int(keep)
    if not (1 <= trials <= POSE_MAX_TRIALS and 1 <= keep <= POSE_MAX_KEEP):
        raise HipExtensionError(f"1 <= trials <= {POSE_MAX_TRIALS} and 1 <= keep <= {POSE_MAX_KEEP} are required, "
                                f"got {trials} and {keep}")
    return trials, keep


def scan_pose_trials_plan(trials=32768, keep=1024):
    """(threads, rows_per_lane, tile) of the score kernel of scan_pose_trials (hp_scan_pose_trials_plan): a workgroup of
    `threads` lanes holds threads * rows_per_lane consecutive source rows and walks a set's kept transforms `tile` at a time
    through LDS; the draw walks the trials `threads` at a time.  Host only."""
    return _plan("hp_scan_pose_trials_plan", (int(trials), int(keep)), 3,
                 f"1 <= trials <= {POSE_MAX_TRIALS} and 1 <= keep <= {POSE_MAX_KEEP} are required, got {trials} and {keep}")


def scan_pose_trials(points, offsets, tpoints, toffsets, match, inlier_dist, trials=32768, keep=1024, seed=0, streams=None,
                     edge_ratio=0.9, min_inliers=6, out=None, ws=None):
    """A rigid start of each of S source sets onto its target set by sample consensus over matched triples
    (csrc/pose_trials.hip) — asynchronous, no host synchronisation, bit-reproducible.  points (T,3) float32 / offsets (S+1)
    int64 and tpoints (U,3) / toffsets (S+1) as scan_align_step; match (T) int32: a target row within the set for every
    source row, or -1 (scan_feature_match's output); 0 <= inlier_dist, +inf for no gate; 1 <= trials <= POSE_MAX_TRIALS;
    1 <= keep <= POSE_MAX_KEEP; streams (S) int64 RNG stream ids, default the set's number; 0 <= edge_ratio <= 1.
    The law is in include/hyperpocket_hip.h, per set: trial h samples three source rows by Philox (seed, stream, tag 5).  It
    is valid iff the rows are matched (finite, as their targets) and differ, their targets differ, every side of the two
    triangles agrees in length — fp32 squared lengths, ls2 >= rho2 * lt2 and lt2 >= rho2 * ls2 with rho2 = fp32(edge_ratio^2) —
    and neither triangle is collinear.  Its transform takes the source triangle's triad frame and centroid onto the target's
    (fp64, rounded to the 12 fp32 of a scan_align_step transform): a start, not a least-squares fit.  The first `keep` valid
    trials in ascending h are kept — an ordered compaction, so the kept list is a function of the inputs — and scored: the
    matched rows with |T p - q|^2 <= inlier_dist^2 in scan_align_step's fp32 formulas.  The winner has the most inliers, ties to
    the lower trial.  The cost is O(trials) + O(n * kept).
    Returns a dict of (S) int32 — trial (-1: no valid trial), inliers, found (inliers >= min_inliers), valid (the valid
    trials, counted before the cap) and kept — and transform (S,12) float32, NaN without a trial.  Sets with the empty
    result are scan_align_step's.  out, ws: the dict of an earlier call and its workspace to reuse."""
    S = _check_align_sets(points, offsets, tpoints, toffsets)
    trials, keep = _check_pose_trials(trials, keep)
    inlier_dist, edge_ratio, min_inliers = _check_max_dist(inlier_dist), float(edge_ratio), int(min_inliers)
    if not 0.0 <= edge_ratio <= 1.0 or min_inliers < 0:
        raise HipExtensionError(f"0 <= edge_ratio <= 1 and min_inliers >= 0 are required, got {edge_ratio} and {min_inliers}")
    T, U, dev = points.size(0), tpoints.size(0), points.device
    check_input(match, "match", torch.int32)
    if match.device != dev or tuple(match.shape) != (T,):
        raise HipExtensionError(f"match must be (T) = ({T}) int32 on the points' device, got {tuple(match.shape)}")
    _check_streams(streams, S, "set")
    out = _outputs(out, _POSE_ROWS, {"S": S}, dev, "the sets")
    ws, _ = _workspace(ws, _long_fn("hp_scan_pose_trials_workspace_bytes", S, keep), dev, torch.int32)
    rho2 = ctypes.c_float(edge_ratio * edge_ratio).value       # at its fp32 rounding
    call("hp_scan_pose_trials", S, ctypes.c_longlong(T), points, offsets, ctypes.c_longlong(U), tpoints, toffsets, match, streams,
         _seed_word(seed), trials, keep, ctypes.c_float(rho2), ctypes.c_float(inlier_dist), min_inliers,
         out["trial"], out["inliers"], out["found"], out["transform"], out["valid"], out["kept"], ws, current_stream(dev))
    return out


def scan_align_global(points, offsets, tpoints, toffsets, max_dist, k=32, trials=32768, keep=1024, seed=0, streams=None,
                      edge_ratio=0.9, inlier_dist=None, min_inliers=6, normals=None, tnormals=None, viewpoints=None,
                      tviewpoints=None):
    """A global start for scan_align / scan_align_plane: descriptors, their matches and a consensus over matched triples, all
    on the device — for two sets in arbitrary relative pose, where the local aligners and the yaw search do not reach.
    The chain, on either side wherever normals are not given: knn_points(k) and scan_normals(k, viewpoints) — then
    scan_features on the same lists, scan_feature_match source -> target and scan_pose_trials (trials, keep, seed, streams,
    edge_ratio, min_inliers) with inlier_dist, default max_dist.  One host read, at the end.
    Descriptors need consistently oriented normals: a capture is oriented towards its sensor, so say where each sensor stood —
    viewpoints / tviewpoints, (S,3) or one (3,), in each side's own frame.  Without them scan_normals' sign rule (the largest
    component positive) is not invariant under rotation and the matches of a turned scan are poor.  Given normals are taken
    as they are.
    Returns (poses (S,3,4) float64 source -> target — the identity where nothing was found —, found (S) bool, inliers (S)
    int64, valid (S) int64 the valid trials): numpy arrays on the host; hand poses to scan_align(init=) or
    scan_align_plane(init=)."""
    import numpy as np
    S = _check_align_sets(points, offsets, tpoints, toffsets)
    max_dist = _check_max_dist(max_dist)
    inlier_dist = max_dist if inlier_dist is None else _check_max_dist(inlier_dist)
    trials, keep = _check_pose_trials(trials, keep)
    k = int(k)
    if not 2 <= k <= KNN_MAX_K:
        raise HipExtensionError(f"2 <= k <= {KNN_MAX_K} is required, got k = {k}")
    for side, side_offsets, given in ((points, offsets, normals), (tpoints, toffsets, tnormals)):
        _check_knn(side, side_offsets, k)
        if given is not None:
            check_input(given, "normals")
            if given.device != side.device or tuple(given.shape) != tuple(side.shape):
                raise HipExtensionError("given normals must match their points row for row")

    def describe(p, o, n, v):
        if p.size(0) == 0:
            return (torch.empty((0, FEATURE_WIDTH), dtype=torch.uint8, device=p.device),
                    torch.empty((0,), dtype=torch.int32, device=p.device))
        index, _ = knn_points(p, o, k)
        if n is None:
            n = scan_normals(p, o, k, viewpoints=v, index=index)[0]
        return scan_features(p, o, n, index)

    feat, cnt = describe(points, offsets, normals, viewpoints)
    tfeat, tcnt = describe(tpoints, toffsets, tnormals, tviewpoints)
    match, _ = scan_feature_match(feat, offsets, tfeat, toffsets, cnt, tcnt)
    res = scan_pose_trials(points, offsets, tpoints, toffsets, match, inlier_dist, trials=trials, keep=keep, seed=seed,
                           streams=streams, edge_ratio=edge_ratio, min_inliers=min_inliers)
    packed = torch.cat([res["transform"], res["found"].float().unsqueeze(1), res["inliers"].float().unsqueeze(1),
                        res["valid"].float().unsqueeze(1)], dim=1).cpu().numpy()      # the host read; the counts are below 2^24
    found = packed[:, 12] != 0
    poses = np.tile(np.eye(3, 4), (S, 1, 1))
    poses[found] = packed[found, :12].astype(np.float64).reshape(-1, 3, 4)
    return poses, found, packed[:, 13].astype(np.int64), packed[:, 14].astype(np.int64)


VOXEL_GRID_HALF = 1 << 20      # HP_VOXEL_GRID_HALF
VOXEL_MAX_ROWS = 1 << 28       # rows of one scan_voxels call

_VOXEL_OUT = _table(("label", torch.int32, ("T",), None), ("size", torch.int32, ("T",), None), ("keep", torch.uint8, ("T",), None),
              ("kept", torch.int32, ("S",), 0), ("beyond", torch.int32, ("S",), 0))
_VOXEL_KEEP = {"center": 0, "first": 1}


def scan_voxels_plan():
    """(threads, rows_per_lane) of the voxel kernels (hp_scan_voxels_plan): a workgroup of `threads` lanes covers
    threads * rows_per_lane consecutive rows of the ragged set.  Host only."""
    return _plan("hp_scan_voxels_plan", (), 2, "hp_scan_voxels_plan failed")


def _voxel_workspace_bytes(T, slots_per_row):
    if slots_per_row not in (1, 2, 4):
        raise ValueError(f"slots_per_row must be 1, 2 or 4, got {slots_per_row!r}")
    need = _long_fn("hp_scan_voxels_workspace_bytes", ctypes.c_longlong(int(T)), int(slots_per_row))
    if need < 0:
        raise ValueError(f"0 <= T <= {VOXEL_MAX_ROWS} rows are required, got {T}")
    return need


def scan_voxels_buffers(S, T, device, slots_per_row=2):
    """The outputs of one scan_voxels call over S scans of T rows in all plus its workspace, as one dict (label, size, keep,
    kept, beyond, ws), allocated once by a caller that reuses them: pass it as `out`, and its "ws" as `ws`."""
    if int(S) < 1:
        raise ValueError(f"S >= 1 is required, got {S}")
    need = _voxel_workspace_bytes(T, slots_per_row)
    return dict(_outputs(None, _VOXEL_OUT, {"S": int(S), "T": int(T)}, device, "the scans"),
                ws=_workspace(None, need, device, torch.int64)[0])


def scan_voxels(points, offsets, voxel, origin=None, keep="center", slots_per_row=2, out=None, ws=None):
    """Voxel-grid thinning of S ragged scans (csrc/voxels.hip): one representative row per occupied cell of a regular grid —
    asynchronous, no host synchronisation, bit-reproducible.  points (T,3) float32, offsets (S+1) int64 as scan_boxes, a scan
    of up to SCAN_MAX_POINTS rows and T <= VOXEL_MAX_ROWS; voxel: the cell edge, a positive finite float for all scans or an
    (S) float32 device tensor (a scan whose entry is not finite or not > 0 gets the empty result); origin: None anchors the
    grid at the coordinate origin (u = p, no operation), an (S,3) float32 device tensor anchors scan s at origin[s]
    (u = p - origin[s]).
    The law is in include/hyperpocket_hip.h, per scan: q = floor(u / voxel) per axis, one correctly rounded fp32 division; a
    row is inside iff -VOXEL_GRID_HALF <= q < VOXEL_GRID_HALF on all axes, absent with a non-finite coordinate, beyond the
    grid otherwise; keep="center" keeps the row of each cell nearest the cell's centre (q + 0.5) * voxel by (the bits of d2,
    the row), keep="first" the cell's first row.
    Returns a dict: label (T) int32 the smallest row within the scan of the row's cell (-1: absent or beyond), size (T) int32
    the cell's rows (0), keep (T) uint8 exactly one row per occupied cell, kept (S) int32 the occupied cells, beyond (S) int32
    the present rows outside the grid.  label is what a caller needs to average per cell with one index_add_.
    out: a dict with these five tensors to reuse (a scan_voxels_buffers result; returned as it is), ws: its "ws"; all outputs
    are fully overwritten.  slots_per_row in (1, 2, 4) sizes the hash table; the result does not depend on it."""
    S = _check_ragged(points, offsets)
    if keep not in _VOXEL_KEEP:
        raise ValueError(f'keep must be "center" or "first", got {keep!r}')
    T, dev = points.size(0), points.device
    need = _voxel_workspace_bytes(T, slots_per_row)
    voxel = _per_scan(voxel, "voxel", S, dev, ValueError)
    if origin is not None:
        check_input(origin, "origin")
        if tuple(origin.shape) != (S, 3) or origin.device != dev:
            raise ValueError("origin must be (S,3) on the points' device")
    out = _outputs(out, _VOXEL_OUT, {"S": S, "T": T}, dev, "the scans", ValueError)
    ws, _ = _workspace(ws, need, dev, torch.int64, ValueError)
    if T == 0:                                             # nothing to launch (and an empty tensor has no address)
        _serve_empty(out, _VOXEL_OUT)
        return out
    call("hp_scan_voxels", S, ctypes.c_longlong(T), points, offsets, voxel, origin, _VOXEL_KEEP[keep], int(slots_per_row),
         out["label"], out["size"], out["keep"], out["kept"], out["beyond"], ws, current_stream(dev))
    return out


VISIBILITY_MIN_RESOLUTION, VISIBILITY_MAX_RESOLUTION = 4, 1024     # HP_VISIBILITY_MIN_RESOLUTION, HP_VISIBILITY_MAX_RESOLUTION
VISIBILITY_MAX_WINDOW = 4                                          # HP_VISIBILITY_MAX_WINDOW
VISIBILITY_MAX_WORKSPACE = 1 << 32     # bytes of depth buffers one scan_visibility call may hold: 64 scans at resolution 1024 fit
VISIBILITY_LABELS = ("seen_through", "on_surface", "hidden", "unobserved")      # labels 0 .. 3; 4: a non-finite row

_VISIBILITY_OUT = _table(("label", torch.uint8, ("Q",), None), ("winner", torch.uint8, ("Q",), None))


def scan_visibility_plan(T, Q=None):
    """(threads, rows_per_lane, scatter_groups, classify_groups) of a scan_visibility call over T rows that labels Q rows (None:
    the T rows themselves) — hp_scan_visibility_plan: a workgroup of `threads` lanes covers threads * rows_per_lane consecutive
    rows, and the two launches run that many workgroups (0: not launched).  Host only."""
    T, Q = int(T), int(T if Q is None else Q)
    return _plan("hp_scan_visibility_plan", (ctypes.c_longlong(T), ctypes.c_longlong(Q)), 4,
                 f"0 <= T, Q <= 2^31 - 1 rows are required, got T = {T}, Q = {Q}")


def _check_visibility(resolution, window, margin, slope):
    """-> (R, w, margin, pitch): the integers, and the two doubles the kernels take; pitch = 2 * slope / R in fp64."""
    R, w, margin, slope = int(resolution), int(window), float(margin), float(slope)
    if not VISIBILITY_MIN_RESOLUTION <= R <= VISIBILITY_MAX_RESOLUTION or R != resolution:
        raise ValueError(f"{VISIBILITY_MIN_RESOLUTION} <= resolution <= {VISIBILITY_MAX_RESOLUTION} (an integer) is required, "
                         f"got {resolution!r}")
    if not 0 <= w <= VISIBILITY_MAX_WINDOW or w != window:
        raise ValueError(f"0 <= window <= {VISIBILITY_MAX_WINDOW} (an integer) is required, got {window!r}")
    pitch = 2.0 * slope / R
    if not (0.0 <= margin < float("inf") and 0.0 <= slope and pitch < float("inf")):
        raise ValueError(f"margin >= 0 and slope >= 0, both finite, are required, got margin = {margin}, slope = {slope}")
    return R, w, margin, pitch


def _visibility_workspace_bytes(S, R):
    fn = load_library().hp_scan_visibility_workspace_bytes
    fn.restype = ctypes.c_longlong
    need = fn(int(S), int(R))
    if need < 0:
        raise ValueError(f"S >= 1 scans and {VISIBILITY_MIN_RESOLUTION} <= resolution <= {VISIBILITY_MAX_RESOLUTION} are required, "
                         f"got S = {S}, resolution = {R}")
    if need > VISIBILITY_MAX_WORKSPACE:
        fit = VISIBILITY_MAX_WORKSPACE // (need // int(S))
        raise ValueError(f"the depth buffers of {S} scans at resolution {R} take {need} bytes, more than the {VISIBILITY_MAX_WORKSPACE} "
                         f"one call may hold: {fit} scans fit, call it on chunks of the scans")
    return need


def scan_visibility_buffers(S, R, device, Q=None):
    """The workspace of one scan_visibility call over S scans at resolution R — and, with Q, the rows it labels (the scans' T, or
    the queries' Q), its label tensor — as one dict (ws, label), allocated once by a caller that reuses them: pass it as `out`,
    and its "ws" as `ws`.  After a call, ws.view(S, 6, R, R) is the scans' range image."""
    bufs = {"ws": _workspace(None, _visibility_workspace_bytes(S, R), device, torch.int64)[0]}
    if Q is not None:
        if int(Q) < 0:
            raise ValueError(f"Q >= 0 is required, got {Q}")
        bufs["label"] = torch.empty((int(Q),), dtype=torch.uint8, device=device)
    return bufs


def _viewpoints(viewpoints, S, device):
    """One triple or (S,3), on any device -> the (S,3) float32 tensor the kernels read."""
    v = torch.as_tensor(viewpoints, dtype=torch.float32)
    if tuple(v.shape) not in ((3,), (S, 3)):
        raise ValueError(f"viewpoints must be one triple or (S,3) with S = {S}, got {tuple(v.shape)}")
    return v.to(device).expand(S, 3).contiguous()


def scan_visibility(points, offsets, viewpoints, resolution=32, window=1, margin=0.01, slope=2.0, queries=None,
                    query_offsets=None, out=None, ws=None):
    """What of S ragged scans is visible from their sensor positions, and how a second set of rows stands to what the sensor
    recorded (csrc/visibility.hip) — asynchronous, no host synchronisation, bit-reproducible.  points (T,3) float32, offsets (S+1)
    int64 as scan_boxes, a scan of up to SCAN_MAX_POINTS rows; viewpoints: one triple for all scans or (S,3), in the scans' frame;
    queries (Q,3) / query_offsets (S+1): a second ragged set over the same S scans, default the scans' own rows.
    The law is in include/hyperpocket_hip.h, per scan: a depth buffer on the six faces of a cube about the viewpoint,
    `resolution` pixels per edge (gnomonic: no trigonometry, a sensor inside the scene is covered), the nearest z-depth per pixel
    and equal depths to the lowest row; a query looks at the pixels within `window` of its own on its face, each with the
    tolerance margin + z * (2 * slope / resolution) * (max(|dx|,|dy|) + 1) — a recorded point shadows a cone.  The pixel must be
    about the sample spacing or coarser, or the far side shows through.  A window does not reach across a cube
    edge.
    Returns a dict: label (T) or (Q) uint8 — 0 seen through (everything recorded there lies behind the row: it stands in the
    sensor's free space), 1 on the surface / visible, 2 hidden (something recorded is in front), 3 unobserved (nothing recorded
    there), 4 a row with a non-finite coordinate; a scan's own rows get 1, 2 or 4 — and, without queries, winner (T) uint8: 1 for
    the row that owns its pixel, one row per pixel.
    out: a dict with "label" (and "winner", which may be left out) to reuse, ws: a scan_visibility_buffers "ws"; after the call
    ws.view(S, 6, resolution, resolution) of its first S * 6 * resolution^2 words is the range image: (depth bits << 32 | row),
    -1 where empty.  The depth buffers take S * 6 * resolution^2 * 8 bytes; more than VISIBILITY_MAX_WORKSPACE is refused with
    the number of scans that fit."""
    S = _check_ragged(points, offsets)
    R, w, margin, pitch = _check_visibility(resolution, window, margin, slope)
    T, dev = points.size(0), points.device
    if T > S * SCAN_MAX_POINTS:                            # known without reading the offsets: some scan is beyond the cap
        raise ValueError(f"a scan holds at most {SCAN_MAX_POINTS} points, got {T} rows in {S} scan(s)")
    if (queries is None) != (query_offsets is None):
        raise ValueError("queries and query_offsets come together")
    own, Q = queries is None, T
    if not own:
        if _check_ragged(queries, query_offsets) != S:
            raise ValueError("query_offsets must have one entry per scan, plus one")
        if queries.device != dev:
            raise ValueError("queries and points must be on one device")
        Q = queries.size(0)
        if out is not None and out.get("winner") is not None:
            raise ValueError("winner belongs to a scan's own rows: it cannot be asked for together with queries")
    need = _visibility_workspace_bytes(S, R)
    views = _viewpoints(viewpoints, S, dev)
    out = _outputs(out, _VISIBILITY_OUT, {"Q": Q}, dev, "the rows to label", ValueError, optional={"winner": own})
    ws, ws_bytes = _workspace(ws, need, dev, torch.int64, ValueError)
    if Q == 0:                                             # nothing to label (and an empty tensor has no address)
        return out
    call("hp_scan_visibility", S, ctypes.c_longlong(T), points if T else None, offsets, views, R, w, ctypes.c_double(margin),
         ctypes.c_double(pitch), ctypes.c_longlong(Q), queries, query_offsets, out["label"], out.get("winner"), ws,
         ctypes.c_longlong(ws_bytes), current_stream(dev))
    return out


DEPTH_MAX_WINDOW = 4               # HP_DEPTH_MAX_WINDOW
DEPTH_MAX_PIXELS = (1 << 31) - 1   # B * H * W of one depth_points call; an image holds at most SCAN_MAX_POINTS pixels

_DEPTH_OUT = _table(("points", torch.float32, ("P", 3), None), ("normals", torch.float32, ("P", 3), None),
                    ("pixel", torch.int64, ("P",), None), ("offsets", torch.int64, ("B1",), None))


def _check_depth_shape(B, H, W):
    B, H, W = int(B), int(H), int(W)
    if B < 1 or H < 1 or W < 1 or H * W > SCAN_MAX_POINTS or B * H * W > DEPTH_MAX_PIXELS:
        raise ValueError(f"B, H, W >= 1, H * W <= {SCAN_MAX_POINTS} and B * H * W <= {DEPTH_MAX_PIXELS} are required, got "
                         f"B = {B}, H = {H}, W = {W}")
    return B, H, W


def depth_points_plan(B, H, W):
    """(threads, pixels_per_lane, chunks, scan_threads, scan_rounds) of a depth_points call over B images of H x W —
    hp_depth_points_plan: a workgroup of `threads` lanes takes a chunk of threads * pixels_per_lane consecutive row-major pixels
    of one image, an image has `chunks` of them, and the scan pass takes scan_threads chunks a round.  Host only."""
    B, H, W = _check_depth_shape(B, H, W)
    return _plan("hp_depth_points_plan", (B, H, W), 5, f"no plan for B = {B}, H = {H}, W = {W}")


def _depth_workspace_bytes(B, H, W):
    fn = load_library().hp_depth_points_workspace_bytes
    fn.restype = ctypes.c_longlong
    return fn(B, H, W)


def depth_points_buffers(B, H, W, device):
    """The outputs and the workspace of one depth_points call over B images of H x W as one dict (points, normals, pixel of
    capacity B * H * W rows, offsets, ws), allocated once by a caller that reuses them: pass it as `out`, and its "ws" as `ws`."""
    B, H, W = _check_depth_shape(B, H, W)
    bufs = _outputs(None, _DEPTH_OUT, {"P": B * H * W, "B1": B + 1}, device, "the images")
    bufs["ws"] = _workspace(None, _depth_workspace_bytes(B, H, W), device, torch.int32)[0]
    return bufs


def _depth_table(value, B, row, name, forms):
    """A per-image table of host data, given once for all images or per image -> the host float64 tensor (B, *row)."""
    import numpy as np
    if not torch.is_tensor(value):                         # Python floats are doubles: never through torch's default float32
        value = np.asarray(value)
        if value.dtype.kind not in "iuf":
            raise ValueError(f"{name} must hold real numbers, got {value.dtype}")
        value = value.astype(np.float64)
    t = torch.as_tensor(value)
    if t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{name} must hold real numbers, got {t.dtype}")
    if t.is_cuda:                                          # reading it would be a host synchronisation
        raise ValueError(f"{name} on the device must be a depth_points_tables result; anything else is host data")
    t = t.detach().to(torch.float64)
    if tuple(t.shape) == row:
        t = t.expand(B, *row)
    if tuple(t.shape) != (B, *row):
        raise ValueError(f"{name} must be {forms} with B = {B}, got {tuple(t.shape)}")
    return t.contiguous()


def _depth_poses(poses, B):
    """None, (3,4), (4,4), (B,3,4) or (B,4,4) camera-to-world matrices -> (B,3,4) float32 on the host; a 4x4's last row must
    be (0, 0, 0, 1)."""
    if poses is None:
        return torch.eye(3, 4, dtype=torch.float32).expand(B, 3, 4).contiguous()
    t = torch.as_tensor(poses)
    if t.dim() not in (2, 3) or tuple(t.shape[-2:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"poses must be (3,4), (4,4), (B,3,4) or (B,4,4) with B = {B}, got {tuple(t.shape)}")
    p = _depth_table(t, B, tuple(t.shape[-2:]), "poses", "(3,4), (4,4), (B,3,4) or (B,4,4)")
    if p.size(1) == 4:
        if not bool((p[:, 3] == torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).all()):
            raise ValueError("the last row of a 4x4 pose must be (0, 0, 0, 1)")
        p = p[:, :3]
    p = p.to(torch.float32).contiguous()
    if not bool(torch.isfinite(p).all()):                  # after the cast: a double beyond the fp32 range is not finite there
        raise ValueError("poses must be finite in float32")
    return p


def _depth_intrinsics(intrinsics, B):
    """(4,) or (B,4) host data -> (B,4) float64 on the host: finite, fx and fy > 0."""
    K = _depth_table(intrinsics, B, (4,), "intrinsics", "(4,) or (B,4)")
    if not bool((torch.isfinite(K).all(1) & (K[:, 0] > 0) & (K[:, 1] > 0)).all()):
        raise ValueError("intrinsics (fx, fy, cx, cy) must be finite with fx, fy > 0")
    return K


def depth_points_tables(B, intrinsics, poses=None, device="cuda"):
    """(K (B,4) float64, M (B,3,4) float32) on the device: the intrinsics and poses of B images as depth_points' kernels read
    them, checked on the host and uploaded once by a caller that calls depth_points again and again — pass them as
    `intrinsics` and `poses`, and a call makes no copy and reads no value."""
    B = int(B)
    if B < 1:
        raise ValueError(f"B >= 1 is required, got {B}")
    return _depth_intrinsics(intrinsics, B).to(device), _depth_poses(poses, B).to(device)


def _depth_prepared(t, dev, dtype, shape, name):
    """A table already on the device is taken as it is — its values are the caller's promise (depth_points_tables checked
    them) — when it has the kernels' form."""
    if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{name} on the device must be the contiguous {dtype} tensor {shape} of depth_points_tables on the "
                         f"depth's device, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _depth_on_gpu(depth, masks):
    """The device test of depth_points, after every check the host can make without one."""
    if not depth.is_cuda or not depth.is_contiguous():
        raise ValueError("depth must be a contiguous tensor on the GPU — the kernels have no CPU path")
    if masks is not None and (masks.device != depth.device or not masks.is_contiguous()):
        raise ValueError("masks must be contiguous and on the depth's device")


def _depth_arguments(depth, masks, depth_scale, near, far, jump, window):
    """The checks of what depth_points and fuse_volume share, before the device is looked at -> (B, H, W, is_u16, scale, near,
    far, jump_abs, jump_rel, w)."""
    if not (torch.is_tensor(depth) and depth.dim() == 3 and depth.dtype in (torch.uint16, torch.float32)):
        raise ValueError("depth must be a (B,H,W) uint16 or float32 tensor")
    B, H, W = _check_depth_shape(*depth.shape)
    if masks is not None and not (torch.is_tensor(masks) and masks.dtype == torch.uint8 and masks.shape == depth.shape):
        raise ValueError(f"masks must be a uint8 tensor of the depth's shape {tuple(depth.shape)}")
    is_u16 = depth.dtype == torch.uint16
    scale = (0.001 if is_u16 else 1.0) if depth_scale is None else float(depth_scale)
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"depth_scale > 0 (finite) is required, got {depth_scale!r}")
    near, far = float(near), float(far)
    if not 0.0 <= near <= far:
        raise ValueError(f"0 <= near <= far is required (far may be inf), got near = {near}, far = {far}")
    try:
        jump_abs, jump_rel = (float(x) for x in jump)
    except (TypeError, ValueError):
        raise ValueError(f"jump must be a pair (absolute, relative), got {jump!r}") from None
    if not (0.0 <= jump_abs < float("inf") and 0.0 <= jump_rel < float("inf")):
        raise ValueError(f"jump = (absolute, relative), both >= 0 and finite, is required, got {jump!r}")
    w = int(window)
    if not 0 <= w <= DEPTH_MAX_WINDOW or w != window:
        raise ValueError(f"0 <= window <= {DEPTH_MAX_WINDOW} (an integer) is required, got {window!r}")
    return B, H, W, is_u16, scale, near, far, jump_abs, jump_rel, w


def depth_points(depth, intrinsics, poses=None, masks=None, depth_scale=None, near=0.0, far=float("inf"), jump=(0.0, 0.05),
                 window=1, out=None, ws=None):
    """A batch of depth images back-projected and cleaned into one ragged set (csrc/depth.hip) — asynchronous, three launches, no
    host synchronisation, bit-equal to tests/depth_law.py.  depth (B,H,W) uint16 or float32 on the device; intrinsics (4,) or
    (B,4) = (fx, fy, cx, cy), pixel centres at integer coordinates, the camera looking along +z with x right and y down; poses:
    camera-to-world, (3,4) / (B,3,4) [R | t] or 4x4 matrices with the last row (0, 0, 0, 1), None for the camera frame; masks
    (B,H,W) uint8 on the device or None: pixels with 0 go.  intrinsics and poses are host data (numbers, arrays, host tensors):
    they are checked here and uploaded with every call, two small copies from pageable memory; a caller in a loop passes the
    device tensors of depth_points_tables instead, which are taken as they are.  Any other device tensor is refused: reading it
    would synchronise.  depth_scale: metres per unit, None for 0.001 (uint16) or 1.0 (float32).  The law is in include/hyperpocket_hip.h: a pixel is kept when its depth z is measured (finite, > 0), near <= z <=
    far, masked in and not at a depth edge — no measured pixel within `window` (0 .. DEPTH_MAX_WINDOW, 0: no edge test) of it
    differs by more than jump[0] + jump[1] * (the nearer of the two depths), whichever side it is on.
    Returns a dict: points (B*H*W,3) float32 in the world frame, normals (B*H*W,3) float32 (unit, facing the sensor, from the
    four neighbours that do not jump; zero where there is none), pixel (B*H*W) int64 = (b * H + v) * W + u, offsets (B+1) int64.
    The first offsets[B] rows are written, in image, row, column order; the rest keep what they held.
    out: a depth_points_buffers dict to reuse, ws: its "ws".  A wrong dtype, shape, device or range is a ValueError before any
    GPU call."""
    B, H, W, is_u16, scale, near, far, jump_abs, jump_rel, w = _depth_arguments(depth, masks, depth_scale, near, far, jump, window)
    dev = depth.device
    on_device = lambda t: torch.is_tensor(t) and t.is_cuda
    K = _depth_prepared(intrinsics, dev, torch.float64, (B, 4), "intrinsics") if on_device(intrinsics) \
        else _depth_intrinsics(intrinsics, B)
    M = _depth_prepared(poses, dev, torch.float32, (B, 3, 4), "poses") if on_device(poses) else _depth_poses(poses, B)
    need = _depth_workspace_bytes(B, H, W)
    _depth_on_gpu(depth, masks)
    try:
        out = _outputs(out, _DEPTH_OUT, {"P": B * H * W, "B1": B + 1}, dev, "the images", ValueError)
        ws, ws_bytes = _workspace(ws, need, dev, torch.int32, ValueError)
    except HipExtensionError as e:                         # check_input's: a dtype, a device, a stride
        raise ValueError(str(e)) from None
    if any(out[name].device != dev for name, _, _, _ in _DEPTH_OUT.checks):
        raise ValueError("out must be on the depth's device")
    call("hp_depth_points", B, H, W, depth, int(is_u16), ctypes.c_double(scale), K.to(dev), M.to(dev), masks,
         ctypes.c_double(near), ctypes.c_double(far), ctypes.c_double(jump_abs), ctypes.c_double(jump_rel), w, out["points"],
         out["normals"], out["pixel"], out["offsets"], ws, ctypes.c_longlong(ws_bytes), current_stream(dev))
    return out


FUSE_MAX_DIM = 1024                # HP_FUSE_MAX_DIM: voxels along an axis
FUSE_MAX_VOXELS = (1 << 31) - 1    # G * nx * ny * nz of one call
FUSE_ROTATION_TOLERANCE = 2.0 ** -16

_FUSE_VOLUME_OUT = _table(("tsdf", torch.float32, ("G", "nz", "ny", "nx"), None), ("weight", torch.int32, ("G", "nz", "ny", "nx"), None))
_FUSE_SURFACE_OUT = _table(("points", torch.float32, ("C", 3), None), ("normals", torch.float32, ("C", 3), None),
                           ("cell", torch.int64, ("C",), None), ("offsets", torch.int64, ("G1",), None))


def fuse_grid(lo, hi, voxel, truncation=None):
    """(origin (G,3) float64 host tensor, (nx, ny, nz)): the default grid of fuse_volume around the boxes lo, hi (G,3) — origin =
    lo - truncation, n = max(1, ceil(((hi - lo) + 2 * truncation) / voxel)) per axis in float64, the shared dims the maximum over
    the groups (tests/fuse_law.py states the same rule).  truncation None: 4 * voxel."""
    voxel, truncation = _check_fuse_lengths(voxel, truncation)
    lo = torch.as_tensor(lo, dtype=torch.float64).reshape(-1, 3)
    hi = torch.as_tensor(hi, dtype=torch.float64).reshape(-1, 3)
    if lo.shape != hi.shape or lo.size(0) < 1 or not bool((torch.isfinite(lo) & torch.isfinite(hi) & (lo <= hi)).all()):
        raise ValueError("lo and hi must be finite (G,3) boxes with lo <= hi")
    n = torch.ceil(((hi - lo) + 2 * truncation) / voxel).clamp(min=1).amax(0)
    return lo - truncation, tuple(int(x) for x in n)


def _check_fuse_lengths(voxel, truncation):
    voxel = float(voxel)
    if not 0.0 < voxel < float("inf"):
        raise ValueError(f"voxel > 0 (finite) is required, got {voxel!r}")
    truncation = 4 * voxel if truncation is None else float(truncation)
    if not 0.0 < truncation < float("inf"):
        raise ValueError(f"truncation > 0 (finite) is required, got {truncation!r}")
    return voxel, truncation


def _check_fuse_dims(G, dims, voxel=None):
    """(G, nx, ny, nz) within the kernels' limits; the message names the voxel size to try where the caller's is known."""
    try:
        nx, ny, nz = (int(x) for x in dims)
        exact = (nx, ny, nz) == tuple(dims)
    except (TypeError, ValueError):
        exact = False
    if not exact:
        raise ValueError(f"dims must be three integers (nx, ny, nz), got {dims!r}")
    G = int(G)
    if G < 1 or min(nx, ny, nz) < 1:
        raise ValueError(f"G >= 1 and nx, ny, nz >= 1 are required, got G = {G}, dims = {(nx, ny, nz)}")
    if max(nx, ny, nz) > FUSE_MAX_DIM or G * nx * ny * nz > FUSE_MAX_VOXELS:
        grow = max(max(nx, ny, nz) / FUSE_MAX_DIM, (G * nx * ny * nz / FUSE_MAX_VOXELS) ** (1.0 / 3.0)) * 1.01
        hint = f": try voxel >= {voxel * grow:.6g}" if voxel is not None else ""
        raise ValueError(f"a grid of {nx} x {ny} x {nz} voxels in {G} volumes is beyond nx, ny, nz <= {FUSE_MAX_DIM} and "
                         f"G * nx * ny * nz <= {FUSE_MAX_VOXELS}{hint}")
    return G, nx, ny, nz


def _fuse_groups(groups, B):
    """None (one group of all images) or a list of lists of image numbers -> (images (L) int32, offsets (G+1) int32) on the host."""
    if groups is None:
        groups = [range(B)]
    try:
        lists = [[int(b) for b in g] for g in groups]
        exact = all(a == b for g, l in zip(groups, lists) for a, b in zip(g, l))
    except (TypeError, ValueError):
        exact = False
    if not exact or not lists:
        raise ValueError("groups must be a non-empty list of lists of image numbers")
    for g, l in enumerate(lists):
        if not l:
            raise ValueError(f"group {g} has no image")
        if min(l) < 0 or max(l) >= B:
            raise ValueError(f"group {g} names an image outside 0 .. {B - 1}")
    ends = [0]
    for l in lists:
        ends.append(ends[-1] + len(l))
    if ends[-1] > FUSE_MAX_VOXELS:
        raise ValueError("too many images in the groups")
    return torch.tensor([b for l in lists for b in l], dtype=torch.int32), torch.tensor(ends, dtype=torch.int32)


def _check_rotations(M):
    """The fp32 R of every pose (B,3,4) on the host is a rotation: |R^T R - I| <= 2^-16 entry by entry, evaluated in float64 — far
    above fp32 rounding (about 3 * 2^-24), far below any scale or shear.  The volume's projection inverts R by its transpose."""
    R = M[:, :, :3].to(torch.float64)
    err = (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().amax((1, 2))
    bad = torch.nonzero(~(err <= FUSE_ROTATION_TOLERANCE))
    if bad.numel():
        b = int(bad[0])
        raise ValueError(f"pose {b} is not a rotation and a translation: |R^T R - I| reaches {float(err[b]):.3g}, beyond 2^-16")


def _fuse_workspace_bytes(entry, *shape):
    fn = getattr(load_library(), entry)
    fn.restype = ctypes.c_longlong
    return fn(*shape)


def fuse_volume_plan(B, H, W, G, dims):
    """(threads, words, blocks_per_group, blocks) of a fuse_volume call — hp_fuse_volume_plan: workgroups of `threads` lanes, an
    image's keep verdicts in `words` 64-bit ballot words, a group's voxels in blocks_per_group workgroups.  Host only."""
    B, H, W = _check_depth_shape(B, H, W)
    G, nx, ny, nz = _check_fuse_dims(G, dims)
    return _plan("hp_fuse_volume_plan", (B, H, W, G, nx, ny, nz), 4, f"no plan for {(B, H, W, G, nx, ny, nz)}")


def fuse_surface_plan(G, dims):
    """(threads, voxels_per_lane, chunks, scan_threads, scan_rounds) of a fuse_surface call — hp_fuse_surface_plan: a chunk is
    threads * voxels_per_lane consecutive voxels of one group, a group has `chunks` of them.  Host only."""
    G, nx, ny, nz = _check_fuse_dims(G, dims)
    return _plan("hp_fuse_surface_plan", (G, nx, ny, nz), 5, f"no plan for {(G, nx, ny, nz)}")


def fuse_volume_buffers(B, H, W, G, dims, device):
    """The outputs and the workspace of one fuse_volume call as one dict (tsdf, weight (G,nz,ny,nx), ws) for a caller that reuses
    them: pass it as `out`, and its "ws" as `ws`."""
    B, H, W = _check_depth_shape(B, H, W)
    G, nx, ny, nz = _check_fuse_dims(G, dims)
    bufs = _outputs(None, _FUSE_VOLUME_OUT, {"G": G, "nx": nx, "ny": ny, "nz": nz}, device, "the volumes")
    bufs["ws"] = _workspace(None, _fuse_workspace_bytes("hp_fuse_volume_workspace_bytes", B, H, W), device, torch.int64)[0]
    return bufs


def fuse_surface_buffers(G, dims, capacity, device):
    """The outputs and the workspace of one fuse_surface call as one dict (points, normals, cell of `capacity` rows, offsets, ws)."""
    G, nx, ny, nz = _check_fuse_dims(G, dims)
    capacity = _check_capacity(capacity)
    bufs = _outputs(None, _FUSE_SURFACE_OUT, {"C": capacity, "G1": G + 1}, device, "the volumes")
    bufs["ws"] = _workspace(None, _fuse_workspace_bytes("hp_fuse_surface_workspace_bytes", G, nx, ny, nz), device, torch.int64)[0]
    return bufs


def _check_capacity(capacity):
    c = int(capacity)
    if c < 0 or c != capacity:
        raise ValueError(f"capacity >= 0 (an integer) is required, got {capacity!r}")
    return c


def _fuse_on_gpu(t, name):
    """The device test of the fuse wrappers, after every check the host can make without one."""
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous tensor on the GPU — the kernels have no CPU path")


def fuse_volume(depth, intrinsics, poses, groups, origin, dims, voxel, truncation=None, masks=None, depth_scale=None, near=0.0,
                far=float("inf"), jump=(0.0, 0.05), window=1, out=None, ws=None):
    """Posed depth images fused into truncated signed distance volumes (csrc/fuse.hip) — asynchronous, two launches, no host
    synchronisation, no atomics, bit-equal to tests/fuse_law.py.  depth, intrinsics, poses, masks, depth_scale, near, far, jump and
    window are depth_points' (host tables are checked and uploaded per call, depth_points_tables' device tensors are taken as they
    are); a host pose must be a rotation with a translation, |R^T R - I| <= 2^-16, and poses are required when a group has more
    than one image.  groups: a list of lists of image numbers, one volume each, in the order their images are averaged — an image
    may serve several groups or none; None: one group of all images.  origin (3,) or (G,3): the corner of voxel (0, 0, 0) of each
    volume (host data, or a contiguous float64 (G,3) device tensor); dims = (nx, ny, nz) shared by the groups, each <=
    FUSE_MAX_DIM, G * nx * ny * nz <= FUSE_MAX_VOXELS; voxel: the edge of a voxel; truncation: None for 4 * voxel.
    Every voxel averages, over the images of its group whose kept pixel it projects to, the distance along the optical axis from
    the voxel to the measured surface, divided by truncation and cut off at 1; an image that sees the voxel more than truncation
    behind its surface says nothing.  Returns a dict: tsdf (G,nz,ny,nx) float32 (1.0 where no image counts), weight (G,nz,ny,nx)
    int32 (the images that count), origin (G,3) float64 on the device, dims, voxel, truncation — what fuse_surface takes.
    out: a fuse_volume_buffers dict to reuse, ws: its "ws".  A wrong dtype, shape, device or range is a ValueError before any GPU
    call."""
    B, H, W, is_u16, scale, near, far, jump_abs, jump_rel, w = _depth_arguments(depth, masks, depth_scale, near, far, jump, window)
    dev = depth.device
    voxel, truncation = _check_fuse_lengths(voxel, truncation)
    images, ends = _fuse_groups(groups, B)
    G, nx, ny, nz = _check_fuse_dims(ends.numel() - 1, dims, voxel)
    if poses is None and int((ends[1:] - ends[:-1]).max()) > 1:
        raise ValueError("poses are required when a group has more than one image: without them every image is its own frame")
    on_device = lambda t: torch.is_tensor(t) and t.is_cuda
    K = _depth_prepared(intrinsics, dev, torch.float64, (B, 4), "intrinsics") if on_device(intrinsics) \
        else _depth_intrinsics(intrinsics, B)
    if on_device(poses):
        M = _depth_prepared(poses, dev, torch.float32, (B, 3, 4), "poses")
    else:
        M = _depth_poses(poses, B)
        _check_rotations(M)
    if on_device(origin):
        if origin.dtype != torch.float64 or tuple(origin.shape) != (G, 3) or origin.device != dev or not origin.is_contiguous():
            raise ValueError(f"origin on the device must be a contiguous float64 ({G},3) tensor on the depth's device")
    else:
        origin = _depth_table(origin, G, (3,), "origin", "(3,) or (G,3)")
        if not bool(torch.isfinite(origin).all()):
            raise ValueError("origin must be finite")
    need = _fuse_workspace_bytes("hp_fuse_volume_workspace_bytes", B, H, W)
    _depth_on_gpu(depth, masks)
    try:
        out = _outputs(out, _FUSE_VOLUME_OUT, {"G": G, "nx": nx, "ny": ny, "nz": nz}, dev, "the volumes", ValueError)
        ws, ws_bytes = _workspace(ws, need, dev, torch.int64, ValueError)
    except HipExtensionError as e:                         # check_input's: a dtype, a device, a stride
        raise ValueError(str(e)) from None
    if any(out[name].device != dev for name, _, _, _ in _FUSE_VOLUME_OUT.checks):
        raise ValueError("out must be on the depth's device")
    origin = origin.to(dev)
    call("hp_fuse_volume", B, H, W, depth, int(is_u16), ctypes.c_double(scale), K.to(dev), M.to(dev), masks, ctypes.c_double(near),
         ctypes.c_double(far), ctypes.c_double(jump_abs), ctypes.c_double(jump_rel), w, G, int(images.numel()), images.to(dev),
         ends.to(dev), images, ends, origin, nx, ny, nz, ctypes.c_double(voxel), ctypes.c_double(truncation), out["tsdf"],
         out["weight"], ws, ctypes.c_longlong(ws_bytes), current_stream(dev))
    return {"tsdf": out["tsdf"], "weight": out["weight"], "origin": origin, "dims": (nx, ny, nz), "voxel": voxel,
            "truncation": truncation}


def fuse_surface(volume, min_weight=1, capacity=None, out=None, ws=None):
    """The surface of fused volumes as one ragged set (csrc/fuse.hip) — count, scan and emit launches, no atomics, bit-equal to
    tests/fuse_law.py.  volume: a fuse_volume result (tsdf, weight (G,nz,ny,nx), origin (G,3) float64 on the device, voxel).
    There is a row wherever the field changes sign between a voxel and its next neighbour along x, y or z, both observed by at
    least min_weight images: the point interpolated between the two centres, the unit normal from the field's central differences,
    pointing into free space, and cell = (((g * nz + k) * ny + j) * nx + i) * 3 + axis; rows in order of group, k, j, i, axis.
    Returns a dict: points (C,3), normals (C,3) float32, cell (C) int64, offsets (G+1) int64 — offsets always holds the true
    counts, rows at and beyond min(offsets[G], C) keep what they held.  capacity None without `out`: the count runs first,
    offsets[G] is read — the one host synchronisation — and exactly that many rows are emitted; with `out`, its rows are the
    capacity.  capacity 0 counts only.  out: a fuse_surface_buffers dict to reuse, ws: its "ws"."""
    try:
        tsdf, weight, origin, voxel = volume["tsdf"], volume["weight"], volume["origin"], volume["voxel"]
    except (TypeError, KeyError):
        raise ValueError("volume must be a fuse_volume result: a dict of tsdf, weight, origin, voxel") from None
    if not (torch.is_tensor(tsdf) and tsdf.dim() == 4 and tsdf.dtype == torch.float32):
        raise ValueError("volume['tsdf'] must be a (G,nz,ny,nx) float32 tensor")
    G, nx, ny, nz = _check_fuse_dims(tsdf.size(0), (tsdf.size(3), tsdf.size(2), tsdf.size(1)))
    if not (torch.is_tensor(weight) and weight.dtype == torch.int32 and weight.shape == tsdf.shape):
        raise ValueError("volume['weight'] must be an int32 tensor of the tsdf's shape")
    if not (torch.is_tensor(origin) and origin.dtype == torch.float64 and tuple(origin.shape) == (G, 3)):
        raise ValueError(f"volume['origin'] must be a float64 ({G},3) tensor")
    voxel, _ = _check_fuse_lengths(voxel, None)
    m = int(min_weight)
    if m < 1 or m != min_weight:
        raise ValueError(f"min_weight >= 1 (an integer) is required, got {min_weight!r}")
    if capacity is not None:
        capacity = _check_capacity(capacity)
    elif out is not None:
        capacity = _check_capacity(out["points"].shape[0]) if torch.is_tensor(out.get("points")) else 0
    dev = tsdf.device
    need = _fuse_workspace_bytes("hp_fuse_surface_workspace_bytes", G, nx, ny, nz)
    for t, name in ((tsdf, "volume['tsdf']"), (weight, "volume['weight']"), (origin, "volume['origin']")):
        _fuse_on_gpu(t, name)
        if t.device != dev:
            raise ValueError("the volume's tensors must be on one device")

    def run(capacity, out):
        try:
            out = _outputs(out, _FUSE_SURFACE_OUT, {"C": capacity, "G1": G + 1}, dev, "the capacity", ValueError)
            w, w_bytes = _workspace(ws, need, dev, torch.int64, ValueError)
        except HipExtensionError as e:
            raise ValueError(str(e)) from None
        if any(out[name].device != dev for name, _, _, _ in _FUSE_SURFACE_OUT.checks):
            raise ValueError("out must be on the volume's device")
        rows = [out[name] if capacity else None for name in ("points", "normals", "cell")]    # an empty tensor has no address
        call("hp_fuse_surface", G, nx, ny, nz, tsdf, weight, origin, ctypes.c_double(voxel), m, ctypes.c_longlong(capacity), *rows,
             out["offsets"], w, ctypes.c_longlong(w_bytes), current_stream(dev))
        return out

    if capacity is not None:
        return run(capacity, out)
    total = int(run(0, None)["offsets"][G])                # the host synchronisation
    return run(total, None)


VIEW_SPLIT_MAX_POINTS = 8192       # HP_VIEW_SPLIT_MAX_POINTS
VIEW_SPLIT_MIN_RESOLUTION = 4      # HP_VIEW_SPLIT_MIN_RESOLUTION
VIEW_SPLIT_MAX_RESOLUTION = 128    # HP_VIEW_SPLIT_MAX_RESOLUTION
VIEW_SPLIT_MAX_WINDOW = 4          # HP_VIEW_SPLIT_MAX_WINDOW

_VIEW_BATCH_OUT = _table(("existing", torch.float32, ("B", "target", 3), None), ("missing", torch.float32, ("B", "rest", 3), None),
                         ("gt", torch.float32, ("B", "N", 3), None), ("side", torch.uint8, ("B", "N"), None),
                         ("occlusion", torch.float32, ("B", "N"), None))


def view_frames(count, seed):
    """(count,3,3) float32 camera frames on the host, uniformly random rotations: the rows of
    numpy.random.default_rng(seed).standard_normal((count, 4)) as unit quaternions (w, x, y, z), the matrix built in float64.
    Rows of a frame: the camera's right, up and towards-the-sensor axes.  A function of its arguments alone."""
    import numpy as np
    count = int(count)
    if count < 0:
        raise ValueError(f"count >= 0 is required, got {count}")
    q = np.random.default_rng(seed).standard_normal((count, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(count, 3, 3)
    return torch.from_numpy(m.astype(np.float32))


def view_half_extent(radius, distance):
    """The tangent of the half-angle under which a sphere of `radius` about the origin is seen from `distance`:
    radius / sqrt(distance^2 - radius^2) — the image of make_view_batch fitted to an object of that radius."""
    radius, distance = float(radius), float(distance)
    if not (0.0 < radius < distance < float("inf")):
        raise ValueError(f"0 < radius < distance (finite) is required, got radius = {radius}, distance = {distance}")
    return radius / (distance * distance - radius * radius) ** 0.5


def _check_view(distance, half_extent, resolution, window):
    """-> (dist, scale, R, w): the two doubles and the two ints the kernel takes; scale = (0.5 R) / half_extent in fp64."""
    R, w, dist = int(resolution), int(window), float(distance)
    if not VIEW_SPLIT_MIN_RESOLUTION <= R <= VIEW_SPLIT_MAX_RESOLUTION or R != resolution:
        raise ValueError(f"{VIEW_SPLIT_MIN_RESOLUTION} <= resolution <= {VIEW_SPLIT_MAX_RESOLUTION} (an integer) is required, "
                         f"got {resolution!r}")
    if not 0 <= w <= VIEW_SPLIT_MAX_WINDOW or w != window:
        raise ValueError(f"0 <= window <= {VIEW_SPLIT_MAX_WINDOW} (an integer) is required, got {window!r}")
    if not 0.0 < dist < float("inf"):
        raise ValueError(f"a finite distance > 0 is required, got {distance!r}")
    h = view_half_extent(0.5, dist) if half_extent is None else float(half_extent)
    scale = (0.5 * R) / h if h > 0.0 else float("inf")
    if not (0.0 < h < float("inf") and 0.0 < scale < float("inf")):
        raise ValueError(f"a finite half_extent > 0 is required, got {half_extent!r}")
    return dist, scale, R, w


def _check_view_shape(n_points, target):
    if not (2 <= n_points <= VIEW_SPLIT_MAX_POINTS and 0 < target < n_points):
        raise ValueError(f"2 <= N <= {VIEW_SPLIT_MAX_POINTS} and 0 < target < N are required, got N = {n_points}, target = {target}")


def make_view_batch_buffers(batch_size, n_points, target, device, side=True, occlusion=True):
    """The output tensors of one make_view_batch call, allocated once by a caller that reuses them; side / occlusion False leave
    that member out (it is then not written)."""
    _check_view_shape(int(n_points), int(target))
    return _outputs(None, _VIEW_BATCH_OUT, {"B": int(batch_size), "N": int(n_points), "target": int(target),
                                            "rest": int(n_points) - int(target)}, device, "B, N and target",
                    optional={"side": side, "occlusion": occlusion})


def make_view_batch(clouds, ids, frames, target=1024, degrees=None, rot=None, distance=3.0, half_extent=None, resolution=32,
                    window=1, out=None):
    """One training batch of self-occluded views from a device-resident dataset (csrc/view_split.hip) — make_batch's interface
    with a sensor in place of the random plane; one launch, asynchronous, no host synchronisation, bit-reproducible.
    clouds (M,N,3) float32 with 2 <= N <= VIEW_SPLIT_MAX_POINTS; ids (B) int32 cloud numbers; frames (B,3,3) float32, rows the
    camera's right, up and towards-the-sensor axes (view_frames draws them); degrees (B) int32 z-rotations (None: none) with
    rot = rotation_table(device), applied to the output rows after the split.
    The law is in include/hyperpocket_hip.h: the sensor sits at `distance` along the frame's third row and looks at the origin
    through an image of resolution^2 pixels whose half-angle has the tangent half_extent (None: view_half_extent(0.5, distance),
    a sphere of radius 0.5; rows outside the image count in its border pixels); a pixel keeps its nearest depth, a row's
    occlusion is its depth minus the nearest depth within `window` pixels of its own, and the `target` rows of least
    (occlusion, row) are `existing`, the rest `missing`, both in the cloud's row order.  There is no failed item.  The pixel must
    be about the sample spacing or coarser, or the far side shows through: 32 with window 1 for 2048 rows.
    Returns (existing (B,target,3), missing (B,N-target,3), gt (B,N,3), side (B,N) uint8 — 1 = existing —, occlusion (B,N)
    float32); an id outside [0,M) gets zeros.
    out: a make_view_batch_buffers result to reuse; with its "side" / "occlusion" None or left out that one is not written and
    None is returned in its place."""
    dist, scale, R, w = _check_view(distance, half_extent, resolution, window)
    check_input(clouds, "clouds")
    check_input(ids, "ids", torch.int32)
    check_input(frames, "frames")
    if clouds.dim() != 3 or clouds.size(2) != 3:
        raise HipExtensionError("clouds must be (M,N,3)")
    M, N, B, target = clouds.size(0), clouds.size(1), ids.numel(), int(target)
    _check_view_shape(N, target)
    if M < 1 or not 1 <= B <= 65535 or ids.dim() != 1:
        raise ValueError(f"M >= 1 clouds and 1 <= B <= 65535 ids (B) are required, got M = {M}, B = {B}")
    if tuple(frames.shape) != (B, 3, 3):
        raise ValueError(f"frames must be (B,3,3) with B = {B}, got {tuple(frames.shape)}")
    dev = clouds.device
    if degrees is not None:
        check_input(degrees, "degrees", torch.int32)
        if degrees.numel() != B:
            raise HipExtensionError("degrees must have one entry per item")
        if rot is None:
            rot = rotation_table(dev)
        check_input(rot, "rot")
        if tuple(rot.shape) != (360, 2):
            raise HipExtensionError("rot must be (360,2)")
    out = _outputs(out, _VIEW_BATCH_OUT, {"B": B, "N": N, "target": target, "rest": N - target}, dev, "B, N and target",
                   optional={"side": True, "occlusion": True})
    call("hp_make_view_batch", M, N, target, clouds, B, ids, frames, degrees, rot if degrees is not None else None,
         ctypes.c_double(dist), ctypes.c_double(scale), R, w, out["existing"], out["missing"], out["gt"], out.get("side"),
         out.get("occlusion"), current_stream(dev))
    return out["existing"], out["missing"], out["gt"], out.get("side"), out.get("occlusion")


AXIS_SPLIT_MAX_POINTS = 8192   # HP_AXIS_SPLIT_MAX_POINTS


_AXIS_SPLIT_OUT = _table(("lower", torch.float32, ("B", "k", 3), None), ("upper", torch.float32, ("B", "rest", 3), None),
                   ("order", torch.int32, ("B", "n"), None))


def axis_split_buffers(batch_size, n, k, device):
    """The output tensors of one axis_split call, allocated once by a caller that reuses them."""
    return _outputs(None, _AXIS_SPLIT_OUT, {"B": batch_size, "n": n, "k": k, "rest": n - k}, device, "B, n and k")


def axis_split(clouds, k, axis=0, out=None):
    """Each of B clouds sorted along one coordinate and cut at row k, in one launch (csrc/axis_split.hip) — asynchronous, no
    host synchronisation.  clouds (B,n,3) float32 with 2 <= n <= AXIS_SPLIT_MAX_POINTS; 1 <= k <= n-1; axis 0, 1 or 2.
    The law is in include/hyperpocket_hip.h: order = np.argsort(clouds[b,:,axis], kind='stable') — numpy's float32 order,
    -0.0 equal to +0.0, NaNs last, equal values in row order —, lower = the rows order[:k], upper = the rows order[k:], each
    copied bit for bit.  Returns (lower (B,k,3), upper (B,n-k,3), order (B,n) int32).
    out: an axis_split_buffers result to reuse; with its "order" None the permutation is not written and None is returned."""
    if not isinstance(clouds, torch.Tensor) or not clouds.is_cuda or clouds.dtype != torch.float32 or clouds.dim() != 3 \
            or clouds.size(2) != 3 or not clouds.is_contiguous():
        raise ValueError("clouds must be a contiguous (B,n,3) float32 CUDA (HIP) tensor — there is no CPU path")
    B, n, k, axis = clouds.size(0), clouds.size(1), int(k), int(axis)
    if not (2 <= n <= AXIS_SPLIT_MAX_POINTS and 1 <= k <= n - 1 and 0 <= axis <= 2):
        raise ValueError(f"2 <= n <= {AXIS_SPLIT_MAX_POINTS}, 1 <= k <= n-1 and axis in (0, 1, 2) are required, "
                         f"got n = {n}, k = {k}, axis = {axis}")
    load_library()                                         # a product path: no library, no result
    dev = clouds.device
    out = _outputs(out, _AXIS_SPLIT_OUT, {"B": B, "n": n, "k": k, "rest": n - k}, dev, "B, n and k",
                   optional={"order": True})               # None: no permutation wanted
    if B > 0:                                              # an empty tensor has no address
        call("hp_axis_split", B, n, clouds, axis, k, out["lower"], out["upper"], out.get("order"), current_stream(dev))
    return out["lower"], out["upper"], out.get("order")


MESH_MAX_FACES = 32768         # HP_MESH_MAX_FACES


def _check_meshes(vertices, faces):
    """(K, V, F) of vertices (K,V,3) float32 and a shared face list (F,3) int32, both on the device.  The kernels trust the
    face indices, so a face list is read back and checked against V the first time it is seen — the one host synchronisation of
    the mesh calls — and marked; later calls with the same tensor, unmodified, go straight through."""
    check_input(vertices, "vertices")
    check_input(faces, "faces", torch.int32)
    if vertices.dim() != 3 or vertices.size(2) != 3 or vertices.size(1) < 1:
        raise HipExtensionError("vertices must be (K,V,3) with V >= 1")
    if faces.dim() != 2 or faces.size(1) != 3 or not 1 <= faces.size(0) <= MESH_MAX_FACES:
        raise HipExtensionError(f"faces must be (F,3) with 1 <= F <= {MESH_MAX_FACES}")
    if faces.device != vertices.device:
        raise HipExtensionError("vertices and faces must be on one device")
    V = vertices.size(1)
    seen = getattr(faces, "_hp_mesh_checked", None)
    if seen is None or seen[0] != faces._version or seen[1] > V:
        lo, hi = torch.aminmax(faces)
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= V:
            raise HipExtensionError(f"faces name vertices {lo} .. {hi}, outside [0, {V})")
        faces._hp_mesh_checked = (faces._version, hi + 1)      # good for every V above the largest index
    return vertices.size(0), V, faces.size(0)


def _mesh_sample_workspace_bytes(K, F, n):
    fn = load_library().hp_mesh_sample_workspace_bytes
    fn.restype = c_long
    return fn(K, F, n)


_MESH_OUT = _table(("points", torch.float32, ("K", "n", 3), None), ("face", torch.int32, ("K", "n"), None),
             ("area", torch.float64, ("K",), None), ("failed", torch.int32, ("K",), None))


def mesh_sample_buffers(K, F, n, device):
    """The output tensors and the workspace of one mesh_sample call, allocated once by a caller that reuses them."""
    need = _mesh_sample_workspace_bytes(K, F, n) if K > 0 else 0
    return dict(_outputs(None, _MESH_OUT, {"K": K, "n": n}, device, "K and n"),
                ws=_workspace(None, need, device, torch.int64)[0] if need > 0 else None)      # up to 8192 faces: none needed


def mesh_sample(vertices, faces, n, seed=0, streams=None, out=None):
    """n points on each of K triangle meshes, uniform by area, in one launch (csrc/mesh.hip) — asynchronous; no host
    synchronisation once `faces` has been seen (_check_meshes).  vertices (K,V,3) float32: K meshes over the one face list
    faces (F,3) int32, 1 <= F <= MESH_MAX_FACES, as FullModel.sample_meshes decodes them from a utils/sphere_mesh.py sphere;
    streams (K) int64 RNG stream ids, default arange(K).  The law is in include/hyperpocket_hip.h: a face is drawn by its
    area quantised to 40 bits against the mesh's largest, a point in it by the folded (u, v) of the same Philox block, every
    operation one fp64 rounding, the point rounded to fp32 once; the result is a pure function of (the mesh, n, seed,
    streams[k]) and does not move under power-of-two scaling.
    Returns (points (K,n,3) float32, face (K,n) int32 — the face each point lies in —, area (K) float64, failed (K) int32):
    a mesh without any face of finite non-zero area has failed 1 and zero rows; NaN vertices only remove their own faces.
    out: a mesh_sample_buffers(K, F, n, device) result to reuse."""
    K, V, F = _check_meshes(vertices, faces)
    n = int(n)
    if not 1 <= n <= 1 << 24:
        raise HipExtensionError(f"1 <= n <= 2**24 is required, got {n}")
    dev = vertices.device
    _check_streams(streams, K, "mesh")
    if streams is None:
        streams = torch.arange(K, dtype=torch.int64, device=dev)
    given = out is not None
    out = _outputs(out, _MESH_OUT, {"K": K, "n": n}, dev, "K and n")
    ws, need = out.get("ws"), _mesh_sample_workspace_bytes(K, F, n) if K > 0 else 0
    if need > 0:                                           # up to 8192 faces none is needed, and none is looked at
        if given and ws is None:
            raise HipExtensionError(f"out['ws'] must hold {need} bytes")
        ws, _ = _workspace(ws, need, dev, torch.int64)
    if K > 0:                                              # an empty tensor has no address
        call("hp_mesh_sample", K, V, vertices, F, faces, n, _seed_word(seed), streams,
             out["points"], out["face"], out["area"], out["failed"], ws, current_stream(dev))
    return out["points"], out["face"], out["area"], out["failed"]


def mesh_normals(vertices, faces, vertex_faces, face_normals=False):
    """Unit vertex normals of K meshes over one face list (csrc/mesh.hip) — asynchronous, as mesh_sample.  vertex_faces:
    (offsets (V+1), incident) int32 device tensors, the CSR lists utils/sphere_mesh.py builds with a mesh.  A vertex normal is
    the fp64 sum of its incident faces' cross products (b - a) x (c - a) in list order — area-weighted, no atomics, one
    result — over its length, rounded to fp32; zero or non-finite sums give (0,0,0).
    Returns vertex_normal (K,V,3), or (vertex_normal, face_normal (K,F,3)) with face_normals=True."""
    K, V, F = _check_meshes(vertices, faces)
    offsets, incident = vertex_faces
    check_input(offsets, "vertex_faces[0]", torch.int32)
    check_input(incident, "vertex_faces[1]", torch.int32)
    if tuple(offsets.shape) != (V + 1,) or incident.dim() != 1:
        raise HipExtensionError("vertex_faces must be (offsets (V+1), incident faces)")
    seen = getattr(offsets, "_hp_mesh_checked", None)
    if seen is None or seen != (offsets._version, incident._version, incident.data_ptr(), F):
        o = offsets.cpu()
        ok = int(o[0]) == 0 and int(o[-1]) == incident.numel() and bool((o[1:] >= o[:-1]).all())
        if ok and incident.numel():
            lo, hi = torch.aminmax(incident)
            ok = int(lo) >= 0 and int(hi) < F
        if not ok:
            raise HipExtensionError("vertex_faces is not a CSR list of faces in [0, F)")
        offsets._hp_mesh_checked = (offsets._version, incident._version, incident.data_ptr(), F)
    dev = vertices.device
    vertex_normal = torch.empty((K, V, 3), dtype=torch.float32, device=dev)
    face_normal = torch.empty((K, F, 3), dtype=torch.float32, device=dev) if face_normals else None
    if K > 0:
        call("hp_mesh_normals", K, V, vertices, F, faces, offsets, incident if incident.numel() else offsets, face_normal,
             vertex_normal, current_stream(dev))
    return (vertex_normal, face_normal) if face_normals else vertex_normal


TSNE_MAX_POINTS = 16384        # HP_TSNE_MAX_POINTS
TSNE_MIN_GAIN = 0.01


def _check_square(t, name, n=None):
    check_input(t, name)
    if t.dim() != 2 or t.size(0) != t.size(1) or (n is not None and t.size(0) != n):
        raise HipExtensionError(f"{name} must be (n, n)" + ("" if n is None else f" with n = {n}") + f", got {tuple(t.shape)}")
    if not 2 <= t.size(0) <= TSNE_MAX_POINTS:
        raise HipExtensionError(f"2 <= n <= {TSNE_MAX_POINTS} is required, got n = {t.size(0)}")
    return t.size(0)


def _check_embedding(t, name, n):
    check_input(t, name)
    if tuple(t.shape) != (n, 2):
        raise HipExtensionError(f"{name} must be ({n}, 2), got {tuple(t.shape)}")


def pairwise_sqdist_plan(n, d):
    """(tile, kchunk) of hp_pairwise_sqdist: rows per workgroup side and columns per inner sum.  Host only."""
    tile, kchunk = c_int(0), c_int(0)
    if load_library().hp_pairwise_sqdist_plan(int(n), int(d), ctypes.byref(tile), ctypes.byref(kchunk)) != 0:
        raise HipExtensionError(f"2 <= n <= {TSNE_MAX_POINTS} and d >= 1 are required, got n = {n}, d = {d}")
    return tile.value, kchunk.value


def pairwise_sqdist(X, out=None):
    """All-pairs squared distances of the rows of X (n, d) float32, rows contiguous, any row stride -> D (n, n) float32 in
    one asynchronous launch (csrc/tsne.hip): differences first, bit-symmetric, zero diagonal (include/hyperpocket_hip.h)."""
    if not isinstance(X, torch.Tensor) or not X.is_cuda or X.dtype != torch.float32 or X.dim() != 2 or X.size(1) < 1 \
            or X.stride(1) != 1 or X.stride(0) < X.size(1):
        raise HipExtensionError("X must be a (n, d) float32 CUDA (HIP) tensor with contiguous rows — there is no CPU path")
    n, d = X.shape
    if not 2 <= n <= TSNE_MAX_POINTS:
        raise HipExtensionError(f"2 <= n <= {TSNE_MAX_POINTS} is required, got n = {n}")
    if out is None:
        out = torch.empty((n, n), dtype=torch.float32, device=X.device)
    else:
        _check_square(out, "out", n)
    call("hp_pairwise_sqdist", n, d, X, ctypes.c_long(X.stride(0)), out, current_stream(X.device))
    return out


def tsne_affinities(D, perplexity, ws=None):
    """The joint probabilities of exact t-SNE from squared distances D (n, n) float32 (csrc/tsne.hip) — asynchronous.  Per
    row the precision beta is searched until the row's entropy is log(perplexity) within 1e-5, at most 100 evaluations, on
    the row shifted by its smallest off-diagonal entry (include/hyperpocket_hip.h); then
    P = max((C + C^T) / sum(C + C^T), 2^-52) with a zero diagonal.  Returns (P (n, n) float32, beta (n) float32, steps (n)
    int32).  ws: float32 workspace of at least n * n + n + 1 elements to reuse; it holds the conditional matrix afterwards."""
    n = _check_square(D, "D")
    perplexity = float(perplexity)
    if not 0.0 < perplexity < n:
        raise HipExtensionError(f"0 < perplexity < n = {n} is required, got {perplexity}")
    need = n * n + n + 1
    if ws is None:
        ws = torch.empty((need,), dtype=torch.float32, device=D.device)
    else:
        check_input(ws, "ws")
        if ws.numel() < need:
            raise HipExtensionError(f"ws must hold {need} floats")
    P = torch.empty((n, n), dtype=torch.float32, device=D.device)
    beta = torch.empty((n,), dtype=torch.float32, device=D.device)
    steps = torch.empty((n,), dtype=torch.int32, device=D.device)
    call("hp_tsne_affinities", n, D, perplexity, P, beta, steps, ws, current_stream(D.device))
    return P, beta, steps


def tsne_state(Y):
    """(update, gains, rowacc) of a descent starting at Y (n, 2): zeros, ones and the gradient pass's per-row sums."""
    n = Y.size(0)
    return torch.zeros_like(Y), torch.ones_like(Y), torch.zeros((n, 8), dtype=torch.float32, device=Y.device)


def tsne_gradient_rows(P, Y, exaggeration=1.0, rowacc=None, kl=None):
    """hp_tsne_gradient: the per-row sums (n, 8) of one pass over the pairs — [0:2] attractive, [2:4] repulsive, [4] z and, with
    kl a (3) float32 tensor, [5] and [6] the KL terms, kl itself receiving (KL, Z, sum P).  Asynchronous."""
    n = _check_square(P, "P")
    _check_embedding(Y, "Y", n)
    if rowacc is None:
        rowacc = torch.zeros((n, 8), dtype=torch.float32, device=Y.device)
    else:
        check_input(rowacc, "rowacc")
        if tuple(rowacc.shape) != (n, 8):
            raise HipExtensionError(f"rowacc must be ({n}, 8)")
    if kl is not None:
        check_input(kl, "kl")
        if kl.numel() != 3:
            raise HipExtensionError("kl must hold 3 floats")
    call("hp_tsne_gradient", n, P, float(exaggeration), Y, rowacc, kl, current_stream(Y.device))
    return rowacc


def tsne_update(rowacc, Y, update, gains, momentum, lr, min_gain=TSNE_MIN_GAIN, grad=None):
    """hp_tsne_update: Y, update and gains (n, 2) moved in place by one step from a gradient pass's rowacc; grad (n, 2)
    receives g = 4 (attractive - repulsive / Z) when given.  Asynchronous."""
    n = Y.size(0) if Y.dim() == 2 else 0
    if not 2 <= n <= TSNE_MAX_POINTS:
        raise HipExtensionError(f"2 <= n <= {TSNE_MAX_POINTS} is required, got n = {n}")
    for t, name in ((Y, "Y"), (update, "update"), (gains, "gains")) + (((grad, "grad"),) if grad is not None else ()):
        _check_embedding(t, name, n)
    check_input(rowacc, "rowacc")
    if tuple(rowacc.shape) != (n, 8):
        raise HipExtensionError(f"rowacc must be ({n}, 8)")
    call("hp_tsne_update", n, rowacc, Y, update, gains, float(momentum), float(lr), float(min_gain), grad,
         current_stream(Y.device))


def tsne_descend(P, Y, update, gains, rowacc, it0, iters, explore, exaggeration, lr, kl=None):
    """hp_tsne_descend: iterations it0 .. it0 + iters - 1 enqueued back to back, no host synchronisation; below `explore`
    under `exaggeration` and momentum 0.5, afterwards 1 and 0.8.  kl (3) float32 receives (KL, Z, sum P) of the final Y."""
    n = _check_square(P, "P")
    for t, name in ((Y, "Y"), (update, "update"), (gains, "gains")):
        _check_embedding(t, name, n)
    check_input(rowacc, "rowacc")
    if tuple(rowacc.shape) != (n, 8):
        raise HipExtensionError(f"rowacc must be ({n}, 8)")
    if kl is not None:
        check_input(kl, "kl")
        if kl.numel() != 3:
            raise HipExtensionError("kl must hold 3 floats")
    if int(it0) < 0 or int(iters) < 0:
        raise HipExtensionError("it0 >= 0 and iters >= 0 are required")
    call("hp_tsne_descend", n, P, Y, update, gains, rowacc, int(it0), int(iters), int(explore), float(exaggeration), float(lr),
         kl, current_stream(Y.device))


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """In-place fused Adam over flat fp32 tensors (torch.optim.Adam semantics, wd=0, amsgrad=False)."""
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        check_input(t, n)
    call("hp_adam_step", c_long(p.numel()), p, g, m, v, float(lr), float(beta1), float(beta2), float(eps), int(step),
         float(grad_scale), current_stream(p.device))


class _GemmDesc(ctypes.Structure):
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p), ("bias", c_void_p), ("mask", c_void_p),
                ("add", c_void_p), ("ws", c_void_p),
                ("sAz", c_long), ("sBz", c_long), ("sCz", c_long), ("sBiasz", c_long), ("sMaskz", c_long), ("sAddz", c_long),
                ("sAi", c_long), ("sAk", c_long), ("sBk", c_long), ("sBj", c_long),
                ("ldc", c_int), ("ldmask", c_int), ("ldadd", c_int),
                ("M", c_int), ("N", c_int), ("K", c_int), ("batch", c_int), ("ksplit", c_int), ("flags", c_int),
                ("cmax", c_void_p), ("cidx", c_void_p), ("group_rows", c_int), ("rsum", c_void_p), ("sRsumz", c_long),
                ("dyn_count", c_void_p), ("dyn_kind", c_int)]


class GemmF16x2:
    """Test / bench hook over hp_gemm_f16x2_*: C = act(X W^T + b) on the f16 matrix pipe with every fp32 operand split into
    two f16 pieces (csrc/conv_split.hip — the kernel the encoders' conv stack runs).  The constructor prepares (max|X|, the
    pieces of W), `run()` is the GEMM launch alone."""

    def __init__(self, X, W, bias, relu=False, out=None):
        for t, n in ((X, "X"), (W, "W"), (bias, "bias")):
            check_input(t, n)
        self.M, self.K = X.shape
        self.N = W.shape[0]
        if W.shape[1] != self.K or bias.numel() != self.N:
            raise HipExtensionError("GemmF16x2: X (M,K), W (N,K), bias (N)")
        self.X, self.W, self.bias, self.relu = X, W, bias, int(relu)
        self.ws = torch.empty((_long_fn("hp_gemm_f16x2_workspace_floats", c_long(self.M), self.N, self.K),), dtype=torch.float32, device=X.device)
        self.C = out if out is not None else torch.empty((self.M, self.N), dtype=torch.float32, device=X.device)
        call("hp_gemm_f16x2_prepare", c_long(self.M), self.N, self.K, X, W, self.ws, current_stream(X.device))

    def run(self):
        call("hp_gemm_f16x2_run", c_long(self.M), self.N, self.K, self.X, self.bias, self.C, self.relu, self.ws,
             current_stream(self.X.device))
        return self.C


class GemmPP:
    """Test / bench hook over hp_gemm_pp_*: C = act(X W^T + b) with BOTH operands in the piece format (csrc/conv_pp.hip — the
    kernel layers 2..5 of the encoders' conv stack run since round 4): X and W are packed once by the constructor (one exponent
    per 128 rows x `xcb` channels of X, one per row of W), `run(mode)` is the matrix-core launch alone — mode 0: the layer form
    (P-format C inside the workspace; `result()` brings it to fp32), mode 1: the fused max-pool's first stage (per-128-row-tile
    column maxima of X W^T + b and their rows; `partials()`)."""

    def __init__(self, X, W, bias, relu=False, xcb=None, group_rows=None):
        for t, n in ((X, "X"), (W, "W"), (bias, "bias")):
            check_input(t, n)
        self.M, self.K = X.shape
        self.N = W.shape[0]
        self.xcb = int(xcb or min(self.K, 256))
        self.bias, self.relu = bias, int(relu)
        self.group_rows = int(group_rows or 128 * ((self.M + 127) // 128))
        self.ws = torch.empty((_long_fn("hp_gemm_pp_workspace_floats", c_long(self.M), self.N, self.K),), dtype=torch.float32,
                              device=X.device)
        self.dev = X.device
        call("hp_gemm_pp_prepare", c_long(self.M), self.N, self.K, self.xcb, X, W, self.ws, current_stream(self.dev))

    def run(self, mode=0):
        call("hp_gemm_pp_run", c_long(self.M), self.N, self.K, self.xcb, self.bias, self.relu, int(mode), self.group_rows, self.ws,
             current_stream(self.dev))

    def result(self):
        C = torch.empty((self.M, self.N), dtype=torch.float32, device=self.dev)
        call("hp_gemm_pp_unpack", c_long(self.M), self.N, self.K, self.ws, C, current_stream(self.dev))
        return C

    def partials(self):
        tiles = (self.M + 127) // 128
        cmax = torch.empty((tiles, self.N), dtype=torch.float32, device=self.dev)
        cidx = torch.empty((tiles, self.N), dtype=torch.int32, device=self.dev)
        call("hp_gemm_pp_partials", c_long(self.M), self.N, self.K, self.ws, cmax, cidx, current_stream(self.dev))
        return cmax, cidx


def _rows3(t, name, host):
    """A 2-D / 3-D fp32 matrix operand of the GEMM hooks as (3-D view, row stride, batch stride): contiguous, or a view of
    a wider buffer whose rows are dense (inner stride 1, row stride >= width).  A contiguous tensor is described by its
    sizes.  host: a plan query, which reads no memory, also takes CPU tensors."""
    t3 = t if t.dim() == 3 else t.unsqueeze(0)
    if t3.dim() != 3 or t3.dtype != torch.float32 or not (host or t3.is_cuda):
        raise HipExtensionError(f"{name} must be a 2-D or 3-D fp32 CUDA (HIP) tensor")
    if t3.is_contiguous():
        return t3, t3.size(2), t3.size(1) * t3.size(2)
    if t3.stride(2) != 1 or t3.stride(1) < t3.size(2):
        raise HipExtensionError(f"{name} must have dense rows (inner stride 1, row stride >= width)")
    return t3, t3.stride(1), t3.stride(0)


def _base(t):
    """Address of a tensor's first element.  torch answers NULL for a tensor without elements (K = 0); its place in the
    storage it views still has an address, which is what the descriptor wants (the library refuses a NULL operand)."""
    return t.data_ptr() or (t.untyped_storage().data_ptr() and t.untyped_storage().data_ptr() + 4 * t.storage_offset())


_PLAN_PTR = 64     # stands for the buffers a plan query would otherwise allocate: non-null, 16-byte aligned, never followed


def gemm(A, B, bias=None, relu=False, trans_a=False, trans_b=True, mask=None, add=None, ksplit=1, rowsum=False, out=None,
         dyn_rows=None, dyn_k=None, colmax=None, plan=False):
    """Thin test hook over hp_gemm_f32 for 2-D / 3-D (batched) fp32 tensors:
    C = epi(op(A) @ op(B)); trans_b=True means B is stored (N, K) like an nn.Linear weight.
    A, B, mask, add and out may be views with padded rows (inner stride 1, row stride >= width) or an offset base: the
    descriptor carries their strides.  colmax=group_rows: HP_GEMM_COLMAX, returns (cmax, cidx) of shape
    (batch, M / tile_rows, N) and no C.  plan=True: fill the same descriptor and return hp_gemm_plan's (tile, mode) without
    launching or allocating anything (CPU tensors are accepted there)."""
    batched = A.dim() == 3
    A3, lda, _ = _rows3(A, "A", plan)
    B3, ldb, _ = _rows3(B, "B", plan)
    batch = A3.size(0)
    M, K = (A3.size(2), A3.size(1)) if trans_a else (A3.size(1), A3.size(2))
    N = B3.size(1) if trans_b else B3.size(2)
    dev = A.device
    d = _GemmDesc()
    d.A, d.B = _base(A3), _base(B3)
    d.sAz = A3.stride(0)
    d.sBz = B3.stride(0) if B3.size(0) > 1 else 0
    d.sAi, d.sAk = (1, lda) if trans_a else (lda, 1)
    d.sBk, d.sBj = (1, ldb) if trans_b else (ldb, 1)
    d.ldc, d.sCz = N, M * N
    d.M, d.N, d.K, d.batch, d.ksplit = M, N, K, batch, ksplit
    C = None
    if out is not None:
        C, d.ldc, d.sCz = _rows3(out, "out", plan)
        if tuple(C.shape) != (batch, M, N):
            raise RuntimeError(f"out must have shape {(batch, M, N)}")
    elif colmax is None and not plan:
        C = torch.empty((batch, M, N), dtype=torch.float32, device=dev)
    if colmax is None:
        d.C = C.data_ptr() if C is not None else _PLAN_PTR
    flags = 0
    if bias is not None:
        if bias.dtype != torch.float32 or not bias.is_contiguous() or not (plan or bias.is_cuda):
            raise HipExtensionError("bias must be a contiguous fp32 CUDA (HIP) tensor")
        d.bias, d.sBiasz = bias.data_ptr(), (bias.stride(0) if bias.dim() == 2 else 0)
        flags |= 1
    if relu:
        flags |= 2
    if mask is not None:
        mask3, d.ldmask, d.sMaskz = _rows3(mask, "mask", plan)
        d.mask = mask3.data_ptr()
        flags |= 4
    if add is not None:
        add3, d.ldadd, d.sAddz = _rows3(add, "add", plan)
        d.add = add3.data_ptr()
        flags |= 8
    rs = None
    if rowsum:
        if not plan:
            rs = torch.empty((batch, M), dtype=torch.float32, device=dev)
        d.rsum, d.sRsumz = (rs.data_ptr() if rs is not None else _PLAN_PTR), M
        flags |= 32
    if colmax is not None:
        flags |= 16
        d.group_rows = int(colmax)
        d.cmax = d.cidx = _PLAN_PTR
    d.flags = flags
    if dyn_rows is not None:      # int32 device tensor with one element: the real number of rows of A / C
        d.dyn_count, d.dyn_kind = dyn_rows.data_ptr(), 1
    if dyn_k is not None:         # ... the real contraction length
        d.dyn_count, d.dyn_kind = dyn_k.data_ptr(), 2
    ws = None
    if ksplit > 1:
        if not plan:
            ws = torch.empty((batch * ksplit * (M * N + M),), dtype=torch.float32, device=dev)
        d.ws = ws.data_ptr() if ws is not None else _PLAN_PTR
    if plan:
        tile, mode = c_int(-1), c_int(-1)
        call("hp_gemm_plan", ctypes.byref(d), ctypes.byref(tile), ctypes.byref(mode))
        return tile.value, mode.value
    cmax = cidx = None
    if colmax is not None:
        tile_rows = load_library().hp_gemm_tile_rows(ctypes.byref(d))
        cmax = torch.empty((batch, M // tile_rows, N), dtype=torch.float32, device=dev)
        cidx = torch.empty((batch, M // tile_rows, N), dtype=torch.int32, device=dev)
        d.cmax, d.cidx, d.sCz = cmax.data_ptr(), cidx.data_ptr(), (M // tile_rows) * N
    call("hp_gemm_f32", ctypes.byref(d), current_stream(dev))
    if colmax is not None:
        return cmax, cidx
    res = out if out is not None else (C if batched else C[0])
    if rowsum:
        return res, (rs if batched else rs[0])
    return res


def gemm_plan(A, B, **kw):
    """(tile, mode) of the kernel instance gemm(A, B, **kw) would run (hp_gemm_plan): tile 0: 128x32, 1: 128x128, 2: 64x128,
    3: 64x64; mode = the staging loaders of A and B (csrc/gemm.hip)."""
    return gemm(A, B, plan=True, **kw)


def colsum(X, mask=None, use_ws=True):
    """Thin test hook over hp_colsum_f32: out[z][j] = sum_i (mask(i,j) > 0 ? X(i,j) : 0) for a 2-D / 3-D fp32 X (rows may be
    padded).  use_ws=False withholds the workspace, so the rows are not split across workgroups."""
    X3, ldx, sXz = _rows3(X, "X", False)
    batch, M, N = X3.shape
    mask3, ldmask, sMaskz = _rows3(mask, "mask", False) if mask is not None else (None, 0, 0)
    if mask3 is not None and tuple(mask3.shape) != (batch, M, N):
        raise RuntimeError(f"mask must have shape {(batch, M, N)}")
    res = torch.empty((batch, N), dtype=torch.float32, device=X.device)
    ws = None
    if use_ws:
        ws = torch.empty((_long_fn("hp_colsum_workspace_floats", batch, M, N),), dtype=torch.float32, device=X.device)
    call("hp_colsum_f32", batch, M, N, X3, c_long(sXz), ldx, mask3, c_long(sMaskz), ldmask, res, c_long(N), ws,
         current_stream(X.device))
    return res if X.dim() == 3 else res[0]


RENDER_MAX_LAYERS, RENDER_MAX_RADIUS2, RENDER_MAX_SIDE = 8, 64, 4096   # HP_RENDER_MAX_*


class RenderPlan(ctypes.Structure):  # HpRenderPlan
    _fields_ = [("tile_w", c_int), ("tile_h", c_int), ("tiles_x", c_int), ("tiles_y", c_int), ("tiles", c_int),
                ("threads", c_int), ("lds_bytes", c_int), ("workgroups", ctypes.c_longlong)]


def render_points_plan(B, V, size):
    """The launch render_points makes for B clouds, V views and size (W, H) (hp_render_points_plan; host only)."""
    plan = RenderPlan()
    call("hp_render_points_plan", int(B), int(V), int(size[0]), int(size[1]), ctypes.byref(plan))
    return plan


def render_points(points, layer_ends, palette, radius2, views, size, fog=96, background=(255, 255, 255), out=None, ids=False):
    """B clouds under V views as depth-buffered splats, in one launch (csrc/render.hip) — asynchronous, no host
    synchronisation.  points (B,n,3) float32 and views (V,3,4) float32 on the device; layer_ends (L) cumulative ends of the
    L <= 8 layers the n points fall into (non-decreasing, the last one n), palette (L,3) colours 0..255 and radius2 (L)
    integers in [0, 64] on the host; size (W, H) with sides in [1, 4096]; fog in [0, 255]; background 3 values 0..255.
    The law is in include/hyperpocket_hip.h and, executable, in tests/render_law.py: project in fp32, one rounding per
    operation; drop what is not finite or more than 9 pixels outside; quantise the depth w to 24 bits; splat the disc
    dx^2 + dy^2 <= radius2 with the key (depth << 32 | index); the smallest key of a pixel wins and is shaded by its depth.
    Returns image (B,V,H,W,3) uint8, or (image, ids (B,V,H,W) int32 — the winning point of every pixel, -1 for the
    background) with ids=True.  out: an image tensor, or an (image, ids) pair with ids=True, to write into."""
    check_input(points, "points")
    check_input(views, "views")
    if points.dim() != 3 or points.size(2) != 3 or points.size(1) < 1:
        raise HipExtensionError("points must be (B,n,3) with n >= 1")
    if views.dim() != 3 or tuple(views.shape[1:]) != (3, 4) or views.size(0) < 1 or views.device != points.device:
        raise HipExtensionError("views must be (V,3,4) with V >= 1, on the device of points")
    B, n, V = points.size(0), points.size(1), views.size(0)
    W, H = (int(s) for s in size)
    layer_ends, radius2 = [int(e) for e in layer_ends], [int(r) for r in radius2]
    palette = [[int(c) for c in rgb] for rgb in palette]
    background, fog, L = [int(c) for c in background], int(fog), len(layer_ends)
    if not (1 <= W <= RENDER_MAX_SIDE and 1 <= H <= RENDER_MAX_SIDE):
        raise HipExtensionError(f"size must be (W, H) with sides in [1, {RENDER_MAX_SIDE}], got {(W, H)}")
    if not 1 <= L <= RENDER_MAX_LAYERS or len(palette) != L or len(radius2) != L:
        raise HipExtensionError(f"1 <= L <= {RENDER_MAX_LAYERS} layers with one colour and one radius2 each are required")
    if layer_ends[-1] != n or any(a > b for a, b in zip([0] + layer_ends, layer_ends)):
        raise HipExtensionError(f"layer_ends must be non-decreasing from 0 and end at n = {n}, got {layer_ends}")
    if any(not 0 <= r <= RENDER_MAX_RADIUS2 for r in radius2) or not 0 <= fog <= 255:
        raise HipExtensionError(f"radius2 must lie in [0, {RENDER_MAX_RADIUS2}] and fog in [0, 255]")
    if any(len(rgb) != 3 or any(not 0 <= c <= 255 for c in rgb) for rgb in palette + [background]):
        raise HipExtensionError("colours must be 3 values in [0, 255]")
    load_library()                                         # a product path: no library, no result
    dev = points.device
    image, id_map = (out if ids else (out, None)) if out is not None else (None, None)
    if image is None:
        image = torch.empty((B, V, H, W, 3), dtype=torch.uint8, device=dev)
    else:
        check_input(image, "out image", torch.uint8)
        if tuple(image.shape) != (B, V, H, W, 3):
            raise HipExtensionError("out does not fit B, V and size")
    if ids and id_map is None:
        id_map = torch.empty((B, V, H, W), dtype=torch.int32, device=dev)
    elif ids:
        check_input(id_map, "out ids", torch.int32)
        if tuple(id_map.shape) != (B, V, H, W):
            raise HipExtensionError("out does not fit B, V and size")
    if B > 0:                                              # an empty tensor has no address
        call("hp_render_points", B, n, points, V, views, L, (c_int * L)(*layer_ends),
             (ctypes.c_ubyte * (3 * L))(*[c for rgb in palette for c in rgb]), (c_int * L)(*radius2), fog,
             (ctypes.c_ubyte * 3)(*background), W, H, image, id_map, current_stream(dev))
    return (image, id_map) if ids else image

"""What the hypernetwork heads' kernels and the Adam kernels are held to: references, bounds, fixtures, case tables, mutants.

Everything here runs on the CPU in float64 / int64 (the float32 evaluations of `f32_*` are the one exception: they are the
check that a correct fp32 implementation fits the bounds).  tests/test_heads_gpu.py holds the GPU kernels to these laws through
the C ABI; tests/test_heads_law_host.py shows on the same fixtures that the laws catch what they are for, and that the route
query (hp_hypernet_heads_plan) reports every route and flips at every boundary.

TWO OPERAND FAMILIES for the three contractions (theta = t5 W^T + b;  dW = dtheta^T t5;  db = column sums of dtheta):
  E (exact)    small integers (|.| <= 8).  Every product and every partial sum is an integer below 2^24 (2048 * 64 = 2^17 for the
               forward, Kc * 64 for dW), so the fp32 result is the int64 result whatever the summation order, the split into bf16
               pieces (an integer <= 8 is one piece) or the rounding mode: equality bit for bit.
  R (rounded)  full 24-bit significands at three scales (rows cycle through 1e-3, 1, 300).  Per element, in fp64 from the same
               operands:   forward  |got - want64| <= (2048 + 16) u (|t5| |W|^T + |b|)
                           dW       |got - want64| <= (Kc + 8) u (|dtheta|^T |t5|),      db likewise with the column sums of |dtheta|
               u = 2^-24: the gamma_L bound of tests/test_skinny_gpu.py; the forward has 8 more units for the three piece
               products its kernel drops (<= 2^-23 |x y| in all: csrc/heads_fwd.hip).

ADAM (torch.optim.Adam's single-tensor update, wd = 0, amsgrad off; csrc/aux_kernels.hip adam_kernel and the epilogue of
csrc/hypernet.hip's fused dW + Adam kernels, same operation order), with s = grad_scale:
    m' = b1 m + (1 - b1) g s        v' = b2 v + (1 - b2) (g s)^2
    p' = p - step_size * m' / (sqrt(v') * inv_sqrt_bc2 + eps),     step_size = lr / (1 - b1^step),  inv_sqrt_bc2 = (1 - b2^step)^-1/2
`adam64` evaluates this in float64 from the fp32 inputs, with lr, b1, b2, eps, s the fp32 values the C ABI receives.  The
bounds count roundings, one per fp32 operation (products and sums rounded apart; a contracted fma has fewer), one each for the
host's step_size and inv_sqrt_bc2; division and square root are correctly rounded (hipcc's default for fp32):
    m'   b1 m: product, sum = 2;  (1 - b1) g s: g s, 1 - b1, product, sum = 4                                     c_m = 4
    v'   b2 v: 2;  (1 - b2) (g s)^2: g s twice, 1 - b2, two products, sum = 6; all terms >= 0, so relative to v64  c_v = 6
    update: denom carries v' (6 / 2 = 3 under the root), the root, inv_sqrt_bc2, the product, the sum = 7 (the eps term only
         the sum); the quotient, step_size and the product with it = 3                                             c_d = 10
    |m' - m64| <= c_m u (|b1 m| + |(1 - b1) g s|)
    |v' - v64| <= c_v u v64
    |p' - p64| <= u |p64| + (step_size / denom64) (m' bound) + c_d u |update64|
each right-hand side times (1 + 2^-18) for the products of two of these terms (the largest, c_d u times the m' term, is
1e-6 of it).  Nothing is fitted.  The fixtures keep every value where fp32 neither overflows nor leaves the normal range in
v' (v >= 1e-12, |g s| >= 1e-6 or exactly 0); m' may cancel to a small number but its bound is absolute.
"""
import ctypes
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
KT = (64, 128, 512, 1024, 2048)          # trunk widths (csrc/model.hip kTrunk)
K = 2048
IN_SIZE = 32                             # the latent's width in every forward / backward case
L_FWD = 2048 + 16
C_M, C_V, C_D = 4, 6, 10
SECOND_ORDER = 1.0 + 2.0 ** -18
SCALES = (1e-3, 1.0, 300.0)
HP_MAX_HEADS = 8

FWD_STREAM, FWD_GEMM, FWD_PER_HEAD = 0, 1, 2
DW_DIRECT, DW_GEMM, DW_PER_HEAD, DW_SKIPPED = 0, 1, 2, 3


# ================================================================================================ route query
class HyperWeights(ctypes.Structure):    # HpHyperWeights
    _fields_ = [("trunk_w", ctypes.c_void_p * 5), ("trunk_b", ctypes.c_void_p * 5), ("n_heads", ctypes.c_int),
                ("head_out", ctypes.c_int * HP_MAX_HEADS), ("head_w", ctypes.c_void_p * HP_MAX_HEADS),
                ("head_b", ctypes.c_void_p * HP_MAX_HEADS)]


class HyperGrads(ctypes.Structure):      # HpHyperGrads
    _fields_ = [("trunk_w", ctypes.c_void_p * 5), ("trunk_b", ctypes.c_void_p * 5), ("head_w", ctypes.c_void_p * HP_MAX_HEADS),
                ("head_b", ctypes.c_void_p * HP_MAX_HEADS)]


class HeadsPlan(ctypes.Structure):       # HpHeadsPlan
    _fields_ = [("fwd_route", ctypes.c_int), ("dw_route", ctypes.c_int), ("dw_rows_route", ctypes.c_int)]


def plan(lib, B, w, gr, t, dW_rows):
    """hp_hypernet_heads_plan -> (return code, fwd_route, dw_route, dw_rows_route); t and dW_rows are addresses (ints)."""
    p = HeadsPlan(-9, -9, -9)
    rc = lib.hp_hypernet_heads_plan(int(B), ctypes.byref(w), ctypes.byref(gr) if gr is not None else None,
                                    ctypes.c_void_p(t), ctypes.c_void_p(dW_rows) if dW_rows else None, ctypes.byref(p))
    return rc, p.fwd_route, p.dw_route, p.dw_rows_route


def rows_route(lib, t5_addr, out_addr):
    """The route hp_hypernet_heads_dw_rows takes for these two addresses (the query names t5_all through the `t` it is a block of)."""
    w = HyperWeights()
    w.n_heads, w.head_out[0], w.head_w[0] = 1, 16, 1 << 20
    B = 1
    return plan(lib, B, w, None, t5_addr - 4 * B * sum(KT[:4]), out_addr)[3]


def fake_heads(outs, w0=1 << 30, b0=1 << 28, contiguous=True, gap=64):
    """A HyperWeights / HyperGrads pair over made-up addresses: heads of `outs` rows back to back from w0 / b0 (the gradients
    at twice those addresses), or with `gap` floats between them."""
    w, gr = HyperWeights(), HyperGrads()
    w.n_heads = len(outs)
    aw, ab = w0, b0
    for h, n in enumerate(outs):
        w.head_out[h], w.head_w[h], w.head_b[h] = n, aw, ab
        gr.head_w[h], gr.head_b[h] = 2 * w0 + (aw - w0), 2 * b0 + (ab - b0)
        aw += 4 * (n * K + (0 if contiguous else gap))
        ab += 4 * (n + (0 if contiguous else gap))
    return w, gr


# ================================================================================================ the three contractions
def mm64(A, Bm, L, bias=None):
    """want = A . Bm (+ bias) in fp64 and the per-element bound L u (|A| |Bm| + |bias|)."""
    A, Bm = A.double(), Bm.double()
    want, mag = A @ Bm, A.abs() @ Bm.abs()
    if bias is not None:
        want, mag = want + bias.double(), mag + bias.double().abs()
    return want, L * U * mag


def fwd64(t5, W, b):
    return mm64(t5, W.t(), L_FWD, b)


def dw64(dth, t5):
    """dW = dth^T t5 (dth: Kc x rows), db = column sums; bounds with L = Kc + 8."""
    Kc = dth.shape[0]
    want, bound = mm64(dth.t(), t5, Kc + 8)
    d = dth.double()
    return want, bound, d.sum(0), (Kc + 8) * U * d.abs().sum(0)


def int_mm(A, Bm, bias=None):
    out = A.to(torch.int64) @ Bm.to(torch.int64)
    return out if bias is None else out + bias.to(torch.int64)


def is_family_e(x, lim=8):
    """The premise of the exact family, on the tensor the kernel consumed: integral, small, not constant along either axis."""
    x = x.double()
    ok = bool((x == x.round()).all()) and bool((x.abs() <= lim).all())
    if x.shape[0] > 1:
        ok = ok and bool((x != x[:1]).any())
    return ok and bool((x != x[:, :1]).any())


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def trunk(fam):
    """Trunk weights / biases (CPU fp32), drawn once.  E: 0 / +-1 selection matrices and integer biases — layer 0 keeps
    relu(x) and relu(-x) side by side, layers 1-3 copy (layer 1 adds 0 / 1), the last layer, which has no ReLU, takes them
    back with either sign and adds an integer in [-2, 2]: t5 is small signed integers that vary by cloud and column.
    R: random, as tests/test_skinny_gpu.py draws them."""
    def make():
        if fam == "R":
            g = torch.Generator().manual_seed(1234)
            w = [torch.randn(KT[l], KT[l - 1] if l else IN_SIZE, generator=g) / math.sqrt(KT[l - 1] if l else IN_SIZE) for l in range(5)]
            b = [(torch.rand(KT[l], generator=g) - 0.5) * 0.1 for l in range(5)]
            return w, b
        w, b = [], []
        for l in range(5):
            kin = KT[l - 1] if l else IN_SIZE
            j = torch.arange(KT[l])
            m = torch.zeros(KT[l], kin)
            if l == 0:
                sign = torch.where(j < IN_SIZE, 1.0, -1.0)
            elif l == 4:
                sign = torch.where((j % 64 < IN_SIZE) ^ (j % 3 == 0), 1.0, -1.0)
            else:
                sign = torch.ones(KT[l])
            m[j, j % kin] = sign
            w.append(m)
            b.append((j % 2).float() if l == 1 else ((j * 7) % 5 - 2).float() if l == 4 else torch.zeros(KT[l]))
        return w, b
    return _cached(("trunk", fam), make)


def latent(fam, B):
    g = _gen("latent", fam, B)
    if fam == "E":
        return torch.randint(-3, 4, (B, IN_SIZE), generator=g).float()
    return torch.randn(B, IN_SIZE, generator=g)


def trunk64(fam, B):
    """t5 of the fixture as the CPU makes it (fp64 layers, rounded to fp32 once): what the host suite uses where the GPU suite
    reads t5 back."""
    w, b = trunk(fam)
    x = latent(fam, B).double()
    for l in range(5):
        x = x @ w[l].double().t() + b[l].double()
        if l < 4:
            x = torch.relu(x)
    return x.float()


NMAX = 2561


def head_weights(fam):
    """(NMAX x 2048) head weights and NMAX biases; a case takes the first N rows."""
    def make():
        g = _gen("heads", fam)
        if fam == "E":
            return torch.randint(-8, 9, (NMAX, K), generator=g).float(), torch.randint(-8, 9, (NMAX,), generator=g).float()
        s = torch.tensor(SCALES)[torch.arange(NMAX) % 3]
        return torch.randn(NMAX, K, generator=g) * s[:, None], torch.randn(NMAX, generator=g) * s
    return _cached(("heads", fam), make)


def dw_operands(fam, Kc, width):
    """dtheta (Kc x width) and t5 (Kc x 2048)."""
    g = _gen("dw", fam, Kc, width)
    if fam == "E":
        return torch.randint(-8, 9, (Kc, width), generator=g).float(), torch.randint(-8, 9, (Kc, K), generator=g).float()
    s = torch.tensor(SCALES)[torch.arange(width) % 3]
    return torch.randn(Kc, width, generator=g) * s, torch.randn(Kc, K, generator=g)


# ------------------------------------------------------------------------------------------------ case tables
# forward: (name, B, head rows, route, quirk); quirk: None | "w+1" (weights one float past a 16-byte boundary) | "split" (heads not
# back to back) | "switch0" (hp_hypernet_set_heads_stream(0))
N_SWEEP = (16, 17, 79, 80, 81, 95, 96, 2561)
B_SWEEP = (1, 15, 16, 17, 33, 48, 49, 64)
FWD_CASES = [(f"N{N}-B{B}", B, (N,), FWD_STREAM, None) for B in (17, 64) for N in N_SWEEP] + \
            [(f"N81-B{B}", B, (81,), FWD_STREAM, None) for B in B_SWEEP if B not in (17, 64)]
FWD_FALLBACKS = [("N1", 17, (1,), FWD_GEMM, None), ("N15", 17, (15,), FWD_GEMM, None), ("B65", 65, (81,), FWD_GEMM, None),
                 ("W+1", 17, (81,), FWD_GEMM, "w+1"), ("three-heads", 17, (16, 3, 45), FWD_PER_HEAD, "split"),
                 ("three-heads-B64", 64, (16, 3, 45), FWD_PER_HEAD, "split")]
FWD_SWITCHED = [("N17-B17-off", 17, (17,), FWD_GEMM, "switch0"), ("N81-B64-off", 64, (81,), FWD_GEMM, "switch0"),
                ("N2561-B17-off", 17, (2561,), FWD_GEMM, "switch0")]

# dW through hp_hypernet_heads_dw_rows: (Kc, rows, r0, pad of theta_ld, route); every Kc at rows = 33, every rows at Kc in {7, 64}
KC_SWEEP = (1, 2, 3, 7, 8, 9, 16, 63, 64, 65, 130)
ROWS_SWEEP = (1, 31, 32, 33, 64, 65)


def _dw_rows_cases():
    out, i = [], 0
    for Kc, rows in [(Kc, 33) for Kc in KC_SWEEP] + [(Kc, rows) for Kc in (7, 64) for rows in ROWS_SWEEP if rows != 33]:
        out.append((Kc, rows, (0, 5)[i % 2], (0, 7)[(i // 2) % 2], DW_DIRECT))
        i += 1
    # r0 and the stride's pad from both sides at the ragged unit, and the GEMM fall-back (out one float past alignment)
    out += [(7, 33, 5, 0, DW_DIRECT), (7, 33, 0, 7, DW_DIRECT), (64, 65, 0, 0, DW_DIRECT), (64, 65, 5, 7, DW_DIRECT)]
    out += [(3, 33, 5, 7, DW_GEMM), (64, 65, 0, 0, DW_GEMM), (9, 1, 0, 7, DW_GEMM)]
    return sorted(set(out))


DW_ROWS_CASES = _dw_rows_cases()
# dW and db through hp_hypernet_backward, one head of `rows` rows at B = Kc: (Kc, head rows, pad, route, quirk);
# quirk: None | "out+1" | "split" | "skip" (grads->head_w[0] == NULL)
BWD_CASES = [(Kc, (33,), (0, 7)[i % 2], DW_DIRECT, None) for i, Kc in enumerate(KC_SWEEP)] + \
            [(Kc, (rows,), (7, 0)[i % 2], DW_DIRECT, None) for Kc in (7, 64) for i, rows in enumerate(ROWS_SWEEP) if rows != 33] + \
            [(7, (33,), 7, DW_GEMM, "out+1"), (64, (65,), 0, DW_GEMM, "out+1"), (17, (16, 3, 45), 3, DW_PER_HEAD, "split"),
             (9, (33,), 7, DW_SKIPPED, "skip"), (64, (16, 3, 45), 0, DW_SKIPPED, "skip")]

# fused dW + Adam: rows x Kc, each with two of the four (r0, step) pairs so that every value meets every rows and every Kc
FUSED_ROWS, FUSED_KC = (1, 33, 65, 97), (3, 8, 64, 65)
FUSED_CASES = [(rows, Kc, ((0, 1), (5, 1000)) if (i + j) % 2 == 0 else ((0, 1000), (5, 1)))
               for i, rows in enumerate(FUSED_ROWS) for j, Kc in enumerate(FUSED_KC)]
FUSED_CUS = (0, 1, 3)

ADAM_N = (0, 1, 3, 4, 5, 1023, 1024, 1025, 2097152 + 5)
ADAM_VIEW_N = (1, 2, 5, 1025)
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_SCALES = (1.0, 0.5, 1.0 / 64)
HYPER = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)


def fake_fwd_case(B, outs, quirk, t=1 << 32):
    """The addresses a forward case of the tables hands to the query, made up: (w, gr, t)."""
    w, gr = fake_heads(outs, contiguous=quirk != "split", w0=(1 << 30) + (4 if quirk == "w+1" else 0))
    return w, gr, t


def fake_bwd_case(outs, quirk, t=1 << 32):
    w, gr = fake_heads(outs, contiguous=quirk != "split")
    if quirk == "out+1":
        for h in range(len(outs)):
            gr.head_w[h] += 4
    if quirk == "skip":
        gr.head_w[0] = None
    return w, gr, t


class stream_switch:
    """with stream_switch(lib, on): hp_hypernet_set_heads_stream for the block, restored afterwards."""

    def __init__(self, lib, on):
        self.lib, self.on = lib, on

    def __enter__(self):
        self.prev = self.lib.hp_hypernet_set_heads_stream(self.on)

    def __exit__(self, *a):
        self.lib.hp_hypernet_set_heads_stream(self.prev)


def check_cases_reach_every_route(lib):
    """Through hp_hypernet_heads_plan on made-up addresses: every case of the tables takes the route it names, the tables reach
    every route, and both sides of every boundary: B 64 | 65, total 15 | 16, W aligned | + 4 bytes, contiguous | not, switch 1 | 0."""
    seen_f, seen_d, seen_r = set(), set(), set()
    for name, B, outs, route, quirk in FWD_CASES + FWD_FALLBACKS + FWD_SWITCHED:
        w, gr, t = fake_fwd_case(B, outs, quirk)
        with stream_switch(lib, 0 if quirk == "switch0" else 1):
            got = plan(lib, B, w, None, t, None)
        assert got[:2] == (0, route), (name, got)
        seen_f.add((route, quirk, B, sum(outs)))
    for Kc, outs, pad, route, quirk in BWD_CASES:
        w, gr, t = fake_bwd_case(outs, quirk)
        got = plan(lib, Kc, w, gr, t, None)
        assert (got[0], got[2]) == (0, route), (Kc, outs, quirk, got)
        seen_d.add(route)
    for Kc, rows, r0, pad, route in DW_ROWS_CASES:
        assert rows_route(lib, 1 << 32, (1 << 30) + (4 if route == DW_GEMM else 0)) == route
        seen_r.add(route)
    assert {r for r, *_ in seen_f} == {FWD_STREAM, FWD_GEMM, FWD_PER_HEAD}
    assert seen_d == {DW_DIRECT, DW_GEMM, DW_PER_HEAD, DW_SKIPPED} and seen_r == {DW_DIRECT, DW_GEMM}
    sides = lambda pred: {r for r, q, B, n in seen_f if pred(q, B, n)}
    assert sides(lambda q, B, n: q is None and B == 64) == {FWD_STREAM} and sides(lambda q, B, n: B == 65) == {FWD_GEMM}
    assert sides(lambda q, B, n: q is None and n == 16) == {FWD_STREAM} and sides(lambda q, B, n: n == 15) == {FWD_GEMM}
    assert sides(lambda q, B, n: q == "w+1") == {FWD_GEMM} and sides(lambda q, B, n: q == "split") == {FWD_PER_HEAD}
    assert sides(lambda q, B, n: q == "switch0") == {FWD_GEMM}


# ================================================================================================ Adam
def f32(x):
    return float(np.float32(x))


def adam_consts(step, lr, b1, b2, eps):
    """The constants as the C ABI receives them (fp32) and as the host forms them from those (fp64)."""
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    return lr, b1, b2, eps, lr / (1.0 - b1 ** step), 1.0 / math.sqrt(1.0 - b2 ** step)


def adam64(p, g, m, v, step, scale=1.0, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, mutant=None):
    """-> dict(p, m, v: float64 results; bp, bm, bv: per-element bounds).  Inputs are fp32 tensors.  `mutant` names a wrong
    variant (MUTANTS): the results are then the wrong ones; the bounds stay those of the right ones."""
    lr, b1, b2, eps, ss, isb = adam_consts(step, lr, b1, b2, eps)
    s = f32(scale)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gs = g * s
    ta, tb = b1 * m, (1.0 - b1) * gs
    m2 = ta + tb
    v2 = b2 * v + (1.0 - b2) * gs * gs
    denom = v2.sqrt() * isb + eps
    upd = ss * m2 / denom
    p2 = p - upd
    bm = C_M * U * (ta.abs() + tb.abs()) * SECOND_ORDER
    bv = C_V * U * v2 * SECOND_ORDER
    bp = (U * p2.abs() + ss / denom * bm + C_D * U * upd.abs()) * SECOND_ORDER
    out = dict(p=p2, m=m2, v=v2, bp=bp, bm=bm, bv=bv)
    if mutant is None:
        return out
    if mutant == "adam_bias_correction_step_minus_1":
        _, _, _, _, ss, isb = adam_consts(step - 1, lr, b1, b2, eps)
    if mutant == "adam_betas_swapped":
        b1, b2 = b2, b1
    if mutant == "adam_grad_scale_ignored":
        gs = g
    mm = b1 * m + (1.0 - b1) * gs
    vv = b2 * v + (1.0 - b2) * (gs if mutant == "adam_g_not_squared" else gs * gs)
    den = (vv * isb * isb + eps).sqrt() if mutant == "adam_eps_inside_sqrt" else vv.sqrt() * isb + eps
    out.update(p=p - ss * (m if mutant == "adam_old_m_in_update" else mm) / den, m=mm, v=vv)
    return out


def f32_adam(p, g, m, v, step, scale=1.0, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8):
    """The update in plain float32 numpy, one rounding per operation: a correct fp32 implementation."""
    _, b1, b2, eps, ss, isb = adam_consts(step, lr, b1, b2, eps)
    F = np.float32
    b1, b2, eps, ss, isb, s = F(b1), F(b2), F(eps), F(ss), F(isb), F(scale)
    p, g, m, v = (x.numpy().astype(F) for x in (p, g, m, v))
    gr = g * s
    m2 = b1 * m + (F(1) - b1) * gr
    v2 = b2 * v + (F(1) - b2) * gr * gr
    p2 = p - ss * (m2 / (np.sqrt(v2) * isb + eps))
    return dict(p=torch.from_numpy(p2), m=torch.from_numpy(m2), v=torch.from_numpy(v2))


def adam_fixture(n, scale=1.0, seed=0, g=None):
    """p, g, m, v (fp32, n elements).  p: a third exactly 0, a third of size 1e-3, a third of size 1 (so that the bound resolves
    the update, 1e-4 at the most, and not merely p).  g: both signs, 1e-3 .. 1 in size (or the given one).  m: both signs; every
    fifth nearly cancels (1 - b1) g s in m'.  v: 1e-12 .. 1, log-uniform.  Where g is 0 — eight elements from n // 2 on when
    n >= 16, or wherever a given g is — m = v = 0 too: the update there is 0 / eps and p, m, v must come back bit for bit
    (`zero` is the mask)."""
    gen = _gen("adam", n, seed)
    i = torch.arange(n)
    sign = lambda: torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    mag = (1.0 + torch.rand(n, generator=gen)) * sign()
    p = torch.where(i % 3 == 0, torch.zeros(n), torch.where(i % 3 == 1, 1e-3 * mag, mag)).float()
    if g is None:
        g = (10.0 ** (-3.0 * torch.rand(n, generator=gen)) * sign()).float()
        if n >= 16:
            g[n // 2:n // 2 + 8] = 0.0
    else:
        g = g.reshape(-1).float().clone()
    m = (torch.randn(n, generator=gen) * 0.1 * g.abs()).float()
    b1 = f32(0.9)
    cancel = (-(1.0 - b1) / b1 * g.double() * f32(scale) * (1.0 + 1e-4 * torch.randn(n, generator=gen).double())).float()
    m = torch.where(i % 5 == 2, cancel, m)
    v = (10.0 ** (-12.0 * torch.rand(n, generator=gen))).float()
    zero = g == 0
    m[zero], v[zero] = 0.0, 0.0
    return dict(p=p, g=g, m=m, v=v, zero=zero)


# ================================================================================================ what a check reports
def over(got, want, bound):
    """Elements of `got` outside the bound (non-finite ones included)."""
    got = got.double()
    return ~((got - want).abs() <= bound)


def check(tag, name, got, want, bound):
    """Every element finite and inside its bound -> the worst err / bound (over the elements whose bound is not 0)."""
    assert tuple(got.shape) == tuple(want.shape), (tag, name, tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all(), f"{tag} {name}: non-finite values (read before written?)"
    err = (got.double() - want).abs()
    bad = err > bound
    if bad.any():
        i = int((err - bound).argmax())
        idx = tuple(int(x) for x in np.unravel_index(i, tuple(err.shape)))
        raise AssertionError(f"{tag} {name}{list(idx)}: |got - want64| = {err.flatten()[i]:.3e} > bound {bound.flatten()[i]:.3e} "
                             f"(got {got.flatten()[i]:.9e}, want {want.flatten()[i]:.9e}); {int(bad.sum())} elements over")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def check_exact(tag, name, got, want_int):
    assert tuple(got.shape) == tuple(want_int.shape), (tag, name, tuple(got.shape), tuple(want_int.shape))
    assert torch.isfinite(got).all(), f"{tag} {name}: non-finite values (read before written?)"
    bad = got.double() != want_int.double()
    if bad.any():
        idx = tuple(int(x) for x in bad.nonzero()[0])
        raise AssertionError(f"{tag} {name}{list(idx)}: got {got[idx].item()!r}, the integer product is {int(want_int[idx])}; "
                             f"{int(bad.sum())} elements differ")


def check_adam(tag, got, ref, parts=False):
    """got: dict(p, m, v) fp32 -> the worst err / bound of the three (parts: of each, as a dict)."""
    r = {k: check(tag, k, got[k], ref[k], ref["b" + k]) for k in "pmv"}
    return r if parts else max(r.values())


# ================================================================================================ mutants (of the references)
def split3(x):
    """x = p1 + p2 + p3 exactly: three bf16 pieces by truncation (csrc/heads_fwd.hip split3), as float64 tensors."""
    def top(a):
        return torch.from_numpy((a.numpy().view(np.uint32) & np.uint32(0xffff0000)).view(np.float32))
    x = x.float().contiguous()
    p1 = top(x)
    r = (x - p1).contiguous()
    p2 = top(r)
    return p1.double(), p2.double(), (r - p2).double()


def fwd_mutant(name, t5, W, b):
    """theta of a forward that is wrong in the named way, in fp64 / exact arithmetic."""
    B, N = t5.shape[0], W.shape[0]
    T, Wd, bd = t5.double(), W.double(), (b.double() if b is not None else torch.zeros(N, dtype=torch.float64))
    want = T @ Wd.t() + bd
    if name == "fwd_kstep_dropped":               # the k-step 37 of 64 never reaches the accumulators
        ks = slice(32 * 37, 32 * 38)
        return want - T[:, ks] @ Wd[:, ks].t()
    if name == "fwd_product_doubled":             # every element counts one of its 2048 products twice
        k0 = (torch.arange(B)[:, None] * 31 + torch.arange(N)[None, :] * 7) % K
        return want + torch.gather(T, 1, k0) * torch.gather(Wd.t().contiguous(), 0, k0)
    if name == "fwd_ragged_tile_row_off":         # the rows of a ragged last tile come from one row up
        out, r = want.clone(), 16 * (N // 16)
        if N % 16 and r > 0:
            out[:, r:] = T @ Wd[r - 1:N - 1].t() + bd[r:]
        return out
    if name == "fwd_last_cloud_dropped":          # cloud B - 1 is taken for padding: zeros in the product
        out = want.clone()
        out[B - 1] = bd
        return out
    if name == "fwd_piece_b1c2_dropped":          # of the six piece products the one of W's first and t5's second piece is missing
        return want - split3(t5)[1] @ split3(W)[0].t()
    if name == "fwd_bias_twice":
        return want + bd
    raise KeyError(name)


def dw_mutant(name, dth, t5):
    """(dW, db) of a dW pass that is wrong in the named way."""
    Kc = dth.shape[0]
    D, T = dth.double(), t5.double()
    if name == "dw_odd_last_cloud_dropped":       # an odd Kc's half step: the last cloud is never loaded
        keep = Kc - 1 if Kc % 2 else Kc
        return D[:keep].t() @ T[:keep], D[:keep].sum(0)
    if name == "db_odd_lanes_missing":            # the bias gradient keeps lanes 0-31 only: the even clouds
        return D.t() @ T, D[0::2].sum(0)
    raise KeyError(name)


# mutant -> (kind, the cases that are to catch it).  forward: (family, B, N); dW: (family, Kc, rows); Adam: (n, step, scale).
# fwd_piece_b1c2_dropped is family R only, by construction: an integer <= 8 is one bf16 piece, the second pieces are zeros.
MUTANTS = {
    "fwd_kstep_dropped": ("fwd", [("E", 17, 81), ("R", 17, 81), ("R", 64, 2561)]),
    "fwd_product_doubled": ("fwd", [("E", 17, 81), ("R", 17, 81)]),
    "fwd_ragged_tile_row_off": ("fwd", [("E", 17, 17), ("R", 17, 17), ("E", 64, 81), ("R", 64, 81)]),
    "fwd_last_cloud_dropped": ("fwd", [("E", 17, 81), ("R", 17, 81), ("E", 64, 81), ("R", 49, 81)]),
    "fwd_piece_b1c2_dropped": ("fwd", [("R", 17, 81), ("R", 64, 2561)]),
    "fwd_bias_twice": ("fwd", [("E", 17, 81), ("R", 17, 81)]),
    "dw_odd_last_cloud_dropped": ("dw", [("E", 7, 33), ("R", 7, 33), ("E", 65, 33), ("R", 3, 33)]),
    "db_odd_lanes_missing": ("dw", [("E", 7, 33), ("R", 7, 33), ("R", 64, 65)]),
    "adam_bias_correction_step_minus_1": ("adam", [(1025, 2, 1.0), (1025, 1000, 1.0)]),
    "adam_eps_inside_sqrt": ("adam", [(1025, 1, 1.0), (1025, 1000, 0.5)]),
    "adam_betas_swapped": ("adam", [(1025, 1, 1.0), (1025, 100000, 1.0)]),
    "adam_grad_scale_ignored": ("adam", [(1025, 1, 0.5), (1025, 1000, 1.0 / 64)]),
    "adam_g_not_squared": ("adam", [(1025, 1, 1.0)]),
    "adam_old_m_in_update": ("adam", [(1025, 1, 1.0), (1025, 1000, 1.0)]),
}

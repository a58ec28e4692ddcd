"""The laws of the exact t-SNE kernels of csrc/tsne.hip, their error bars, the shared inputs and the drivers of the C entry
points; shared by tests/test_tsne_gpu.py and tests/test_tsne_law_host.py.

Laws: plain numpy in float64 on the fp32 inputs (`update` alone is float32: the kernel's update is specified bit for bit).

Bars: derived from the kernels' operation counts and the precision of fp32 (u = 2^-24); nothing here is fitted to what the
kernels return, with the exceptions the project states nowhere else — the accuracy of the hardware reciprocal, exponential
and logarithm, each measured once through a kernel (RCP_MEASURED, EXP_MEASURED, LOG_MEASURED, profiles/tsne_parity.md).

One departure from scikit-learn's _binary_search_perplexity, in law and kernel alike: a row is shifted by its smallest
off-diagonal distance before the exponential, with the diagonal masked first.  The conditional probabilities p_j / sum p do
not change under the shift, H does not either, and sum p >= 1 always, where scikit-learn's sum underflows to 0 for a far
outlier and its search then sits on the underflow edge for all 100 steps.
"""
import ctypes
import math

import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32
EPS64 = 2.220446049250313e-16     # scikit-learn's MACHINE_EPSILON: the floor of the joint probabilities
TINY = 2.0 ** -126                # below it the hardware transcendentals flush: an absolute term of the bars
SEARCH_STEPS = 100
SEARCH_TOL = 1e-5
MIN_GAIN = 0.01

# the geometry of the kernels (csrc/tsne.hip)
COND_THREADS = 256                # lanes striding over a row of the calibration
GRAD_LANES = 64                   # lanes striding over a row of the gradient
GRAD_ROWS = 16                    # rows per workgroup of the gradient
GRAD_STAGE = 2048                 # points of Y staged in LDS at a time

# Largest errors of the hardware instructions against float64, measured on an MI355X through the kernels themselves
# (profiles/tsne_parity.md has the probes); the bars use twice each figure: the factor covers arguments the probes did not
# sample.
#   v_rcp_f32 through grad_kernel at n = 2, where z_0 = w_01 is the only term of its sum: 3000 arguments 1 + |y_0 - y_1|^2
#   in [1, 1e6], relative
RCP_MEASURED = 8.6307e-08         # 1.448 u, at the argument 15347.038
#   v_exp_f32 through cond_kernel's C at n = 3: C_02 / C_01 = exp(-t) for the t = fl(beta e_02) of the kernel's own beta,
#   relative, t in [0.46, 4.7], 600 samples.  The figure includes three roundings the bars count again (the product with
#   log2(e) and two divisions): an upper bound of the instruction's error, not the error itself
EXP_MEASURED = 2.6553e-07         # 4.455 u, at t = 3.0482538
#   v_log_f32 times ln 2 through grad_kernel's KL row at n = 2 with P_01 = 1: the row is -log w_01, and w_01 is z_0 of the
#   same launch; |error| / max(1, |log w|) over 3000 w in [1e-6, 1)
LOG_MEASURED = 1.4412e-07         # 2.418 u, at w = 0.22962973
RCP_BAR, EXP_BAR, LOG_BAR = 2 * RCP_MEASURED, 2 * EXP_MEASURED, 2 * LOG_MEASURED


def _f64(a):
    return np.asarray(np.asarray(a, np.float32), np.float64)


# ------------------------------------------------------------------------------------------------ distances
def sqdist(X):
    """D[i][j] = sum_k (x_ik - x_jk)^2 in float64 on the fp32 rows of X (n, d)."""
    X = _f64(X)
    n = X.shape[0]
    D = np.empty((n, n))
    for i in range(n):
        D[i] = ((X - X[i]) ** 2).sum(1)
    return D


def sqdist_bar(d, kchunk):
    """Relative: every term is non-negative.  Per term: the difference (u, 2u on its square) and the fmaf that rounds square
    plus sum once; the chain of a chunk has kchunk such roundings, the chunk sums ceil(d / kchunk) - 1 adds: 2 + kchunk +
    ceil(d / kchunk) - 1 roundings, and (1 + u)^k - 1 <= (k + 1) u.  Stated with the issue's ceiling of + 4."""
    return (kchunk + -(-d // kchunk) + 4) * U


# ------------------------------------------------------------------------------------------------ calibration
def _shifted(D):
    """(n, n) float64: each row minus its smallest off-diagonal entry, diagonal 0; and the off-diagonal mask."""
    D = _f64(D)
    n = D.shape[0]
    off = ~np.eye(n, dtype=bool)
    m = np.where(off, D, np.inf).min(1)
    return np.where(off, D - m[:, None], 0.0), off


def _entropy(e, beta):
    """One row: (H, p, S) for the shifted off-diagonal distances e under beta."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.where(e == 0, 0.0, beta * e)
    p = np.exp(-t)
    S = p.sum()
    return math.log(S) + np.where(p > 0, t * p, 0.0).sum() / S, p, S


def conditional(D, perplexity):
    """The search of hp_tsne_affinities per row -> (C (n, n), beta (n), steps (n), H (n)), everything float64."""
    E, off = _shifted(D)
    n = E.shape[0]
    target = math.log(perplexity)
    C, betas, steps, Hs = np.zeros((n, n)), np.empty(n), np.empty(n, np.int64), np.empty(n)
    for i in range(n):
        e = E[i][off[i]]
        beta, lo, hi = 1.0, -np.inf, np.inf
        for step in range(1, SEARCH_STEPS + 1):
            H, p, S = _entropy(e, beta)
            diff = H - target
            if abs(diff) <= SEARCH_TOL or step == SEARCH_STEPS:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2 if hi == np.inf else (beta + hi) / 2
            else:
                hi = beta
                beta = beta / 2 if lo == -np.inf else (beta + lo) / 2
        C[i][off[i]] = p / S
        betas[i], steps[i], Hs[i] = beta, step, H
    return C, betas, steps, Hs


def _sum_roundings(n):
    """A block-wide fp32 sum of cond_kernel over a row of n: a lane's ceil(n / 256) sequential adds, six shuffle levels, four
    wave partials."""
    return -(-n // COND_THREADS) + 6 + 4


def conditional_at(D, beta):
    """C and H at given per-row betas (float64 of the kernel's fp32 output), with the bars of the kernel's evaluation:
    -> dict C (n, n), H (n), H_bar (n), C_rel (n, n): the relative error bar of every C_ij.

    p_j: the shift e = D - m (u), the product with beta (u), the product with log2(e) and that constant's own rounding
    (1.5u) move the argument t = beta e by 3.5 t u <= 4 t u absolutely, p by as much relatively; the exponential adds EXP_BAR.
    eps_j = (4 t_j + 1) u + EXP_BAR.  S = sum p: a = sum p_j eps_j / S + k u relatively, k = _sum_roundings(n) + 1.
    T / S = sum t_j p_j / S: each term e_j p_j carries eps_j + u, the fmaf chain and the sums k u, the product with beta and the
    division 2u, and S's own a.  log S: a absolutely, plus LOG_BAR max(1, |log S|).  The final add: u |H|."""
    E, off = _shifted(D)
    beta = np.asarray(beta, np.float64)
    n = E.shape[0]
    k = _sum_roundings(n) + 1
    C, C_rel, H, H_bar = np.zeros((n, n)), np.zeros((n, n)), np.empty(n), np.empty(n)
    for i in range(n):
        e = E[i][off[i]]
        with np.errstate(over="ignore", invalid="ignore"):
            t = np.where(e == 0, 0.0, beta[i] * e)
        p = np.exp(-t)
        S = p.sum()
        tp = np.where(p > 0, t * p, 0.0)
        eps = (4 * np.minimum(t, 1e30) + 1) * U + EXP_BAR
        a = (p * eps).sum() / S + k * U
        logS, ts = math.log(S), tp.sum() / S
        H[i] = logS + ts
        H_bar[i] = (a + LOG_BAR * max(1.0, abs(logS)) + (tp * (eps + U)).sum() / S + ts * ((k + 2) * U + a)
                    + U * abs(H[i]) + 2 * U)
        C[i][off[i]] = p / S
        C_rel[i][off[i]] = eps + a + 2 * U
    return {"C": C, "H": H, "H_bar": H_bar, "C_rel": C_rel}


def joint(C):
    """P = max((C + C^T) / sum(C + C^T), EPS64) with a zero diagonal."""
    C = np.asarray(C, np.float64)
    S = C + C.T
    P = np.maximum(S / S.sum(), EPS64)
    np.fill_diagonal(P, 0.0)
    return P


def joint_bar(at):
    """Per element, from conditional_at's result: the two conditionals with their own relative bars; the total — row sums as
    block-wide fp32 sums, then fp64, one conversion — carries the C-weighted mean of those bars plus (k + 2) u; the add, the
    division and the linearisation 3u; the clamp is 1-Lipschitz; TINY for a flushed C."""
    C, rel = at["C"], at["C_rel"]
    n = C.shape[0]
    total = 2 * C.sum()
    s_rel = (C * rel).sum() / C.sum() + (_sum_roundings(n) + 3) * U
    cr = C * rel
    return (cr + cr.T) / total + joint(C) * (s_rel + 3 * U) + TINY


# ------------------------------------------------------------------------------------------------ gradient
def gradient(P, Y, exaggeration=1.0):
    """The pass of hp_tsne_gradient and the g of hp_tsne_update in float64 -> dict:
      g (n, 2) = 4 (attr - rep / Z);  A (n, 2) the sum of the absolute terms of g;  attr, rep (n, 2), z (n), Z;
      kl = sum_{P > 0} P (log P - log Q) with Q = w / Z left unclamped so that the pass separates into rows (scikit-learn
      clamps Q at EPS64, which no fp32 input reaches: w >= 1 / (1 + 8 FLT_MAX^2) never gets there before it overflows);
      kl_abs the sum of the absolute terms of kl; sum_p; and per pair logP, logw for the bars."""
    P, Y = _f64(P), _f64(Y)
    n = Y.shape[0]
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff ** 2).sum(-1))
    np.fill_diagonal(w, 0.0)
    z = w.sum(1)
    Z = z.sum()
    at, rt = (exaggeration * P * w)[..., None] * diff, (w * w)[..., None] * diff
    attr, rep = at.sum(1), rt.sum(1)
    pos = (P > 0) & ~np.eye(n, dtype=bool)
    logP = np.log(np.where(pos, P, 1.0))
    logw = np.log(np.where(pos, w, 1.0))
    Pm = np.where(pos, P, 0.0)
    sum_p = Pm.sum()
    kl = (Pm * (logP - logw)).sum() + math.log(Z) * sum_p
    kl_abs = (Pm * (np.abs(logP) + np.abs(logw))).sum() + abs(math.log(Z)) * sum_p
    return {"g": 4 * (attr - rep / Z), "A": 4 * (np.abs(at).sum(1) + np.abs(rt).sum(1) / Z), "attr": attr, "rep": rep, "z": z,
            "Z": Z, "kl": kl, "kl_abs": kl_abs, "sum_p": sum_p, "Pm": Pm, "logP": logP, "logw": logw}


def _chain(n):
    """A row of grad_kernel: a lane's ceil(n / 64) accumulations, then six shuffle levels."""
    return -(-n // GRAD_LANES) + 6


def w_bar():
    """w = rcp(1 + (dx dx + dy dy)): the differences (u each, 2u on a square), the squares (u) and their add (u) put 4u on the
    sum, which is at most the denominator; the add of 1 another u; the reciprocal RCP_BAR."""
    return 5 * U + RCP_BAR


def gradient_bar(n):
    """Relative to A, per element.  Attractive term: exaggeration P (u), times w (u + w_bar), the difference (u), the chain:
    (3 + chain) u + w_bar.  Repulsive term: w w (u + 2 w_bar), the difference (u), the chain; Z: w_bar, the chain, the fp64
    sum's one conversion (u); the division (u): (4 + 2 chain) u + 3 w_bar.  The larger of the two, the subtraction (u) and
    the linearisation (u); the product with 4 is exact."""
    return (6 + 2 * _chain(n)) * U + 3 * w_bar()


def z_bar(n):
    """Relative: w_bar, the chain, one conversion, the linearisation."""
    return w_bar() + (_chain(n) + 2) * U


def kl_bar(law, n):
    """Absolute.  Per pair P (log P - log w) in fp32: each logarithm LOG_BAR max(1, |log|), log w also w_bar for its
    argument; the difference and the product 2u on |log P| + |log w|, one more for the linearisation; the pair sums are fp64.
    The row's conversion to fp32 and the result's: 2u on kl_abs.  log Z sum P: z_bar on Z absolutely on its logarithm, u
    each on the row sums of P."""
    lp, lw, Pm = np.abs(law["logP"]), np.abs(law["logw"]), law["Pm"]
    pairs = (Pm * (LOG_BAR * (np.maximum(1.0, lp) + np.maximum(1.0, lw)) + w_bar() + 3 * U * (lp + lw))).sum()
    return pairs + 2 * U * law["kl_abs"] + law["sum_p"] * (z_bar(n) + U * abs(math.log(law["Z"]))) + TINY


# ------------------------------------------------------------------------------------------------ update and descent
def form_g32(attr, rep, Z):
    """g as update_kernel forms it from fp32 row sums: 4 (attr - rep / Z), each operation rounded to fp32."""
    attr, rep = np.asarray(attr, np.float32), np.asarray(rep, np.float32)
    return np.float32(4) * (attr - rep / np.float32(Z))


def update(g, upd, gains, Y, momentum, lr, min_gain=MIN_GAIN, dtype=np.float32):
    """hp_tsne_update's elementwise part in `dtype` (float32: the kernel's bits), in its order -> (Y, update, gains)."""
    f = dtype
    g, upd, gains, Y = (np.asarray(a, f) for a in (g, upd, gains, Y))
    inc = upd * g < 0
    gains = np.where(inc, gains + f(0.2), gains * f(0.8))
    gains = np.maximum(gains, f(min_gain)).astype(f)
    upd = (f(momentum) * upd - f(lr) * (g * gains)).astype(f)
    return (Y + upd).astype(f), upd, gains


def schedule(it, explore, exaggeration):
    """(exaggeration, momentum) of iteration `it`."""
    return (exaggeration, 0.5) if it < explore else (1.0, 0.8)


def descend(P, Y0, iters, explore, exaggeration, lr, it0=0, dtype=np.float64, trace=None):
    """hp_tsne_descend with the state (Y, update, gains) held in `dtype` and every gradient from the float64 law of the
    current Y -> Y.  trace: a list that receives (max |Y|, max A, max gains, max |g|) per iteration."""
    Y = np.asarray(np.asarray(Y0, np.float32), dtype)
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    for it in range(it0, it0 + iters):
        ex, momentum = schedule(it, explore, exaggeration)
        law = gradient(P, Y, ex)
        if trace is not None:
            trace.append((np.abs(Y).max(), law["A"].max(), gains.max(), np.abs(law["g"]).max()))
        Y, upd, gains = update(law["g"], upd, gains, Y, momentum, lr, dtype=dtype)
    return Y


def kl_of(P, Y):
    return gradient(P, Y)["kl"]


# ------------------------------------------------------------------------------------------------ init
def pca_scores(X):
    """The first two principal-component scores by SVD, float64."""
    X = _f64(X)
    Xc = X - X.mean(0)
    u, s, _ = np.linalg.svd(Xc, full_matrices=False)
    return u[:, :2] * s[:2]


# ------------------------------------------------------------------------------------------------ shared inputs
def clusters(seed, n, d, centres=3, spread=2.0):
    """Gaussian clusters of unit variance around centres drawn at `spread` per coordinate -> (X (n, d) fp32, labels (n))."""
    r = np.random.RandomState(seed)
    labels = np.arange(n) % centres
    mu = r.randn(centres, d) * spread
    return (mu[labels] + r.randn(n, d)).astype(np.float32), labels


def rows(seed, n, d, near=True):
    """Random rows of unit scale sharing a large common part, as decoder weights of similar shapes do; with `near`, rows 1
    and n - 1 are row 0 with its last bits moved."""
    r = np.random.RandomState(seed)
    X = (r.randn(1, d) * 3 + 0.05 * r.randn(n, d)).astype(np.float32)
    if near and n >= 2:
        X[1] = np.nextafter(X[0], np.float32(np.inf))
        X[n - 1] = X[0]
        X[n - 1, ::2] = np.nextafter(X[0, ::2], np.float32(-np.inf))
    return X


def identical_points(n):
    return np.zeros((n, n), np.float32)


def duplicates_and_outlier():
    """D of two duplicates and one point at 10^3."""
    x = np.array([[0.0], [0.0], [1e3]], np.float32)
    return sqdist(x).astype(np.float32)


# ------------------------------------------------------------------------------------------------ drivers
def library():
    from hyperpocket_amd._lib import load_library
    lib = load_library()
    lib.hp_tsne_affinities_workspace_floats.restype = ctypes.c_long
    return lib


def plan(n, d):
    """(tile, kchunk) of hp_pairwise_sqdist_plan; host only."""
    from hyperpocket_amd import ops
    return ops.pairwise_sqdist_plan(n, d)


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()

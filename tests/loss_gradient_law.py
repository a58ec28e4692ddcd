"""The laws of the loss-gradient and match-cost kernels of csrc/structural_losses.hip, their error bars, the case tables and the
drivers of their C entry points; shared by tests/test_loss_gradients_gpu.py and tests/test_loss_gradient_law_host.py.

Laws: plain numpy in float64 on the fp32 inputs.  They take the nearest-neighbour indices and the `match` as inputs, exactly
as the kernels do, so a test may hand law and kernel the same synthetic ones.

Bars: derived from the kernels' operation counts and the precision of fp32 (u = 2^-24); nothing here is fitted to what the
kernels return, with the one exception the project states nowhere else — the accuracy of the hardware reciprocal square
root, measured once through the kernel itself (RSQ_MEASURED, profiles/loss_gradients_parity.md).

Case tables: the shapes of the GPU suite, and the check that they sit on both sides of every edge of every kernel.
"""
import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32
FLT_MAX = float(np.finfo(np.float32).max)

# the geometry of the kernels (csrc/structural_losses.hip)
GRAD_TILE = 2048                  # kGradTile: targets per workgroup of nn_grad_side_kernel
GRAD_THREADS = 256                # its stride over the sources
COST_ROWS = 64                    # kLT: match rows per workgroup of matchcost_kernel
COST_COLS = 256                   # its columns (one per thread); also the columns of matchcostgrad1_kernel
COST_CLOUD_THREADS = 1024         # matchcost_cloud_kernel: columns per sweep of its one workgroup
GRAD1_TILE = 1024                 # kTile: candidates per LDS tile of matchcostgrad1_kernel
GRAD2_ROWS = 4                    # rows per workgroup of matchcostgrad2_kernel (one wave each)
GRAD2_LANES = 64                  # lanes striding over a row


# ------------------------------------------------------------------------------------------------ nearest-neighbour gradient
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def nn_grad_law(t, idx_t, g_t, s, idx_s, g_s):
    """Gradient of the targets t (b, m, 3) of a pair (nndistance.cu:137-153):

        out_T[j] = 2 g_t[j] (t_j - s_{idx_t[j]})  -  sum_{i : idx_s[i] = j} 2 g_s[i] (s_i - t_j)

    idx_t (b, m) indexes the sources s (b, n, 3), idx_s (b, n) the targets; g_t (b, m) and g_s (b, n) are the upstream
    gradients.  Returns a dict of float64 arrays:
      out    (b, m, 3)  the law
      direct (b, m, 3)  the first term
      A      (b, m, 3)  the sum of the absolute scattered terms
      cnt    (b, m)     how many sources scattered to the target
      M      (b, m)     the largest finite |term| — as the kernel forms its terms in fp32: fl(fl(2 g_s) fl(s - t)) — among
                        those scattered into the 2048-target tile the element lies in (0 for a tile nothing scatters to)
    Non-finite inputs propagate as IEEE arithmetic propagates them."""
    t32, s32 = np.asarray(t, np.float32), np.asarray(s, np.float32)
    gs32 = np.asarray(g_s, np.float32)
    t, s, g_t, g_s = _f64(t32), _f64(s32), _f64(np.asarray(g_t, np.float32)), _f64(gs32)
    idx_t, idx_s = np.asarray(idx_t, np.int64), np.asarray(idx_s, np.int64)
    b, m, n = t.shape[0], t.shape[1], s.shape[1]
    assert idx_t.shape == (b, m) and idx_s.shape == (b, n) and g_t.shape == (b, m) and g_s.shape == (b, n)
    assert n == 0 or m == 0 or (idx_t.min() >= 0 and idx_t.max() < n and idx_s.min() >= 0 and idx_s.max() < m)
    rows = np.arange(b)[:, None]
    with np.errstate(all="ignore"):
        direct = 2 * g_t[..., None] * (t - s[rows, idx_t])
        terms = -2 * g_s[..., None] * (s - t[rows, idx_s])                                  # (b, n, 3)
        terms32 = np.abs((gs32 * np.float32(2))[..., None] * (s32 - t32[rows, idx_s])).astype(np.float64)
        sc, A = np.zeros((b, m, 3)), np.zeros((b, m, 3))
        cnt = np.zeros((b, m))
        ntiles = -(-m // GRAD_TILE)
        tmax = np.zeros((b, max(ntiles, 1)))
        for i in range(b):
            np.add.at(sc[i], idx_s[i], terms[i])
            np.add.at(A[i], idx_s[i], np.abs(terms[i]))
            np.add.at(cnt[i], idx_s[i], 1.0)
            big = np.where(np.isfinite(terms32[i]), terms32[i], 0.0).max(axis=1) if n else np.zeros(0)
            np.maximum.at(tmax[i], idx_s[i] // GRAD_TILE, big)
        M = tmax[:, np.arange(m) // GRAD_TILE] if m else np.zeros((b, 0))
        return {"out": direct + sc, "direct": direct, "A": A, "cnt": cnt, "M": M}


def chamfer_backward_law(t, idx_t, s, idx_s, g):
    """nn_grad_law with the one scalar upstream g on both sides: the targets' gradient of g * (batch-sum Chamfer loss)."""
    t, s = np.asarray(t), np.asarray(s)
    g32 = np.float32(g)
    return nn_grad_law(t, idx_t, np.full(t.shape[:2], g32, np.float32), s, idx_s, np.full(s.shape[:2], g32, np.float32))


def nn_grad_bar(law, n):
    """Per element: 4u (A + |direct|) + cnt M 2^(bits(n) - 60), n = the number of sources, bits(n) = n.bit_length().

    First part, the fp32 roundings on the path of a term: two to form it (the difference and the product; doubling the
    upstream is exact), one when the fixed-point sum is converted to fp32, one in the final add of the direct term (which
    has two roundings of its own): <= 4 on anything.  Second part: the sum itself is exact integer arithmetic, but each
    scattered term is first rounded to the grid, half a step 2^-shift at most; the kernel's rule is shift = 61 - ex -
    bits(n) with M < 2^ex <= 2 M, so half a step is at most M 2^(bits(n) - 61) — stated here with a factor two to spare."""
    with np.errstate(all="ignore"):
        return 4 * U * (law["A"] + np.abs(law["direct"])) + (law["cnt"] * law["M"])[..., None] * 2.0 ** (int(n).bit_length() - 60)


# ------------------------------------------------------------------------------------------------ match cost and its gradients
def _pair_diff(p, q):
    """e[b, k, j, :] = p_j - q_k in float64: (b, m, n, 3)"""
    return _f64(np.asarray(p, np.float32))[:, None, :, :] - _f64(np.asarray(q, np.float32))[:, :, None, :]


def matchcost_law(p, q, match):
    """cost[b] = sum_k sum_j match[b, k, j] |p_j - q_k|  (approxmatch.cu:214-258); p (b, n, 3), q (b, m, 3), match (b, m, n).
    Returns (cost (b,), S (b,) = sum |match d|)."""
    d = np.sqrt((_pair_diff(p, q) ** 2).sum(-1))
    w = _f64(np.asarray(match, np.float32)) * d
    return w.sum((1, 2)), np.abs(w).sum((1, 2))


def matchcostgrad_law(p, q, match):
    """grad1[b, j] = sum_k match[b, k, j] e / max(|e|, 1e-10), e = p_j - q_k;  grad2[b, k] = - sum_j of the same terms
    (approxmatch.cu:260-322, the clamp included).  Returns (grad1 (b, n, 3), grad2 (b, m, 3), A1, A2): the gradients and the
    sums of their absolute terms."""
    e = _pair_diff(p, q)
    d = np.sqrt((e ** 2).sum(-1))
    terms = (_f64(np.asarray(match, np.float32)) / np.maximum(d, 1e-10))[..., None] * e          # (b, m, n, 3)
    return terms.sum(1), -terms.sum(2), np.abs(terms).sum(1), np.abs(terms).sum(2)


# Roundings on the longest path of a term, counted in csrc/structural_losses.hip; all terms of the cost are non-negative,
# so k roundings give a relative error of (1 + u)^k - 1 <= (k + 1) u for k u < 1e-3: each count below carries that + 1.
#   |p - q| as the kernels form it: three differences (u each; squaring doubles it: 2u on d^2), the chain
#   fma(dz, dz, fma(dy, dy, dx dx)) (3u on d^2) — 5u on d^2, 2.5u on d — and the square root (u): under 4.
K_DIST = 4


def k_matchcost_ws():
    """hp_matchcost_ws: matchcost_kernel adds the <= 64 rows of a tile by an fma chain (64), then hp::block_sum in fp32: six
    shuffle levels (6) and four wave partials (4); matchcost_finish_kernel adds the partials in fp64 and rounds once (1)."""
    return COST_ROWS + K_DIST + 6 + 4 + 1 + 1


def k_matchcost_cloud(m):
    """hp_matchcost: matchcost_cloud_kernel adds a whole column of m rows by an fma chain (m); everything after it is fp64
    until the one conversion of the result (1)."""
    return m + K_DIST + 1 + 1


# Largest relative error of the hardware reciprocal square root (v_rsq_f32 through __builtin_amdgcn_rsqf) against float64
# 1/sqrt, measured through matchcostgrad1_kernel on an MI355X over 4096 distinct arguments in [1, 4): see
# profiles/loss_gradients_parity.md.  The bars use twice the figure: the factor covers arguments the probe did not sample.
RSQ_MEASURED = 8.2653e-08             # 1.387 u, at the argument 3.6248806
RSQ_BAR = 2 * RSQ_MEASURED


def k_grad_term():
    """One term match e / |e| in fp32: the difference e (1), the argument of the reciprocal square root (5u on d^2, so 2.5u
    on its result: 3), the product with match (1); the reciprocal square root itself comes on top as RSQ_BAR."""
    return 1 + 3 + 1


def matchcostgrad_bars(A1, A2, n, m):
    """grad1: matchcostgrad1_kernel adds the m terms of a column by one fma chain across the LDS tiles (m roundings).
    grad2: matchcostgrad2_kernel gives each of 64 lanes every 64th term of the row's n (ceil(n / 64) fmas), then six shuffle
    levels.  Per element: ((k + 1) u + RSQ_BAR) * the sum of the absolute terms."""
    k1 = m + k_grad_term() + 1
    k2 = -(-n // GRAD2_LANES) + 6 + k_grad_term() + 1
    return (k1 * U + RSQ_BAR) * A1, (k2 * U + RSQ_BAR) * A2


def synthetic_match(seed, b, n, m):
    """(b, m, n) fp32, non-negative, about half the entries exactly 0, row magnitudes spread over six decades.  The kernels
    are linear in match, so no matching has to be computed."""
    r = np.random.RandomState(seed)
    rows = 10.0 ** r.uniform(-3, 3, size=(b, m, 1))
    return (r.rand(b, m, n) * rows * (r.rand(b, m, n) < 0.5)).astype(np.float32)


def clouds(seed, b, n, m, scale=1.0):
    r = np.random.RandomState(seed)
    return ((r.rand(b, n, 3) - 0.5) * scale).astype(np.float32), ((r.rand(b, m, 3) - 0.5) * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the case tables
# nearest-neighbour gradient, (b, sources, targets) of the side under test; the other side of each call has the roles swapped
NN_TILE_TARGETS = (1, 2047, 2048, 2049, 4096, 4097)
NN_TILE_CASES = [(2, 257, m) for m in NN_TILE_TARGETS]
NN_STRIDE_SOURCES = (1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
NN_STRIDE_CASES = [(2, n, 64) for n in NN_STRIDE_SOURCES]
# all sources on one target: (sources, targets, the target, exponent k of the terms 1.9999 * 2^k)
NN_WORST_CASES = [(n, 2049, j, k) for n in (1023, 1024, 1025) for j in (2047, 2048) for k in (-100, 0, 100)]
NN_UPSTREAM_SCALES = (1e-30, 1e-6, 0.05, 1.0, 1e6, 1e30)
NN_CLOUD_SCALES = (1e-3, 1.0, 1e3)
NN_MAGNITUDE_SHAPE = (2, 700, 2300)
NN_MAX_POINTS = 4100

# match cost and gradients, (b, n, m): n columns (xyz1), m rows (xyz2) of match (b, m, n)
MATCH_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
MATCH_M = (1, 3, 4, 5, 63, 64, 65, 129, 1023, 1024, 1025)
MATCH_CASES = [
    (1, 1, 1), (3, 1, 64), (3, 65, 1),
    (3, 63, 3), (3, 64, 4), (3, 65, 5),                      # grad2: 64 lanes per row, 4 rows per workgroup
    (3, 255, 63), (3, 256, 64), (3, 257, 65), (1, 257, 129),  # cost: 256-thread column, 64-row tile; grad1: 256-thread column
    (1, 63, 1023), (1, 64, 1024), (1, 65, 1025),              # grad1: 1024-candidate LDS tile
    (1, 1023, 5), (3, 1024, 4), (1, 1025, 3),                 # hp_matchcost: 1024 columns per sweep
    (1, 1023, 1025), (1, 1024, 1024), (1, 1025, 1023),
    (1, 2049, 129), (2, 2049, 1025),                          # three sweeps; the largest match allowed
]
MATCH_MAX_ELEMS = 2 * 1025 * 2049
# one-hot match: shape and the (row k, column l) positions — the corners, then the edges of grad2's rows and lanes and of
# grad1's LDS tile and thread column
ONE_HOT_SHAPE = (3, 300, 1030)
ONE_HOT_AT = [(0, 0), (0, 299), (1029, 0), (1029, 299), (3, 63), (4, 64), (1023, 255), (1024, 256)]


def _both_sides(values, edge):
    return {edge - 1, edge, edge + 1} <= set(values)


def nn_idx_s(seed, b, n, m):
    """Synthetic nearest-target indices (b, n) into m targets: random, with 0, m - 1 and j0 - 1, j0 for every tile start j0
    planted as far as n allows (the seams first)."""
    r = np.random.RandomState(seed)
    idx = r.randint(0, m, size=(b, n))
    plant = [0, m - 1]
    for j0 in range(GRAD_TILE, m, GRAD_TILE):
        plant += [j0 - 1, j0]
    plant = list(dict.fromkeys(plant))[:n]
    for i in range(b):
        idx[i, r.permutation(n)[:len(plant)]] = plant
    return idx.astype(np.int32)


def check_tables_reach_every_edge():
    """The tables above sit on both sides of every edge the kernels have, hold what the suite's limits allow, and nothing else."""
    # nn gradient: the 2048-target tile (and its second seam), the 256-thread stride and every bits(n) step up to 1025
    targets = [m for _, _, m in NN_TILE_CASES]
    assert _both_sides(targets, GRAD_TILE) and {2 * GRAD_TILE, 2 * GRAD_TILE + 1} <= set(targets) and 1 in targets
    sources = [n for _, n, _ in NN_STRIDE_CASES]
    for edge in (GRAD_THREADS, 2 * GRAD_THREADS, 4 * GRAD_THREADS):
        assert _both_sides(sources, edge), edge
    assert {n.bit_length() for n in sources} >= {1, 8, 9, 10, 11}
    for b, n, m in NN_TILE_CASES:
        idx = nn_idx_s(0, b, n, m)
        want = {0, m - 1} | {j for j0 in range(GRAD_TILE, m, GRAD_TILE) for j in (j0 - 1, j0)}
        assert all(want <= set(row.tolist()) for row in idx), (n, m)
        assert idx.min() >= 0 and idx.max() < m
    assert {n for n, _, _, _ in NN_WORST_CASES} == {1023, 1024, 1025}
    assert {j for _, _, j, _ in NN_WORST_CASES} == {GRAD_TILE - 1, GRAD_TILE}
    assert {k for _, _, _, k in NN_WORST_CASES} == {-100, 0, 100} and all(m == 2049 for _, m, _, _ in NN_WORST_CASES)
    assert max(max(n, m) for _, n, m in NN_TILE_CASES + NN_STRIDE_CASES + [NN_MAGNITUDE_SHAPE]) <= NN_MAX_POINTS
    # match cost and gradients
    ns, ms, bs = [n for _, n, _ in MATCH_CASES], [m for _, _, m in MATCH_CASES], {b for b, _, _ in MATCH_CASES}
    assert set(MATCH_N) <= set(ns) and set(MATCH_M) <= set(ms) and {1, 3} <= bs
    for edge in (GRAD2_LANES, COST_COLS, COST_CLOUD_THREADS):
        assert _both_sides(ns, edge), ("n", edge)
    assert 2 * COST_CLOUD_THREADS + 1 in ns
    for edge in (GRAD2_ROWS, COST_ROWS, GRAD1_TILE):
        assert _both_sides(ms, edge), ("m", edge)
    assert 2 * COST_ROWS + 1 in ms
    assert max(b * n * m for b, n, m in MATCH_CASES) <= MATCH_MAX_ELEMS
    assert sum(n != m for _, n, m in MATCH_CASES) > len(MATCH_CASES) // 2
    b, n, m = ONE_HOT_SHAPE
    ks, ls = {k for k, _ in ONE_HOT_AT}, {l for _, l in ONE_HOT_AT}
    assert {0, m - 1, GRAD2_ROWS - 1, GRAD2_ROWS, GRAD1_TILE - 1, GRAD1_TILE} <= ks
    assert {0, n - 1, GRAD2_LANES - 1, GRAD2_LANES, COST_COLS - 1, COST_COLS} <= ls
    assert all(0 <= k < m and 0 <= l < n for k, l in ONE_HOT_AT) and b * n * m <= MATCH_MAX_ELEMS


# ------------------------------------------------------------------------------------------------ drivers
_SENTINEL = -12345.0


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _out(shape):
    import torch
    return torch.full(shape, _SENTINEL, dtype=torch.float32, device="cuda")


def run_nndistancegrad(x1, x2, g1, i1, g2, i2):
    """hp_nndistancegrad on device tensors -> (grad_xyz1 (b, n, 3), grad_xyz2 (b, m, 3)); idx1 (b, n) indexes x2, idx2 x1."""
    import torch
    from hyperpocket_amd._lib import call, current_stream
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    o1, o2 = _out((b, n, 3)), _out((b, m, 3))
    call("hp_nndistancegrad", b, n, x1, m, x2, g1, i1, g2, i2, o1, o2, current_stream(x1.device))
    torch.cuda.synchronize()
    return o1, o2


def run_chamfer_backward(x1, x2, i1, i2, g, want1=True, want2=True):
    """hp_chamfer_backward with the device scalar g; an output not wanted is passed as NULL and returned as None."""
    import torch
    from hyperpocket_amd._lib import call, current_stream
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    o1, o2 = (_out((b, n, 3)) if want1 else None), (_out((b, m, 3)) if want2 else None)
    call("hp_chamfer_backward", b, n, x1, m, x2, i1, i2, g, o1, o2, current_stream(x1.device))
    torch.cuda.synchronize()
    return o1, o2


def run_matchcost(x1, x2, match, ws):
    """hp_matchcost_ws (ws=True) or hp_matchcost -> cost (b,)"""
    import torch
    from hyperpocket_amd._lib import call, current_stream, load_library
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    out = _out((b,))
    if ws:
        part = torch.full((max(1, load_library().hp_matchcost_workspace_floats(b, n, m)),), float("nan"), device="cuda")
        call("hp_matchcost_ws", b, n, m, x1, x2, match, out, part, current_stream(x1.device))
    else:
        call("hp_matchcost", b, n, m, x1, x2, match, out, current_stream(x1.device))
    torch.cuda.synchronize()
    return out


def run_matchcostgrad(x1, x2, match):
    import torch
    from hyperpocket_amd._lib import call, current_stream
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    o1, o2 = _out((b, n, 3)), _out((b, m, 3))
    call("hp_matchcostgrad", b, n, m, x1, x2, match, o1, o2, current_stream(x1.device))
    torch.cuda.synchronize()
    return o1, o2

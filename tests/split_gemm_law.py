"""The split-f16 ("piece format") GEMM kernels restated on the host, and operands for which they must be exact.

csrc/conv_pp.hip and csrc/conv_split.hip form, per output and in fp32 accumulators,
    sum_k (hi_a hi_w + hi_a lo_w + lo_a hi_w) 2^-(e_a + e_w)  [+ bias, ReLU]
from  hi = rne16(x 2^e),  lo = rne16(x 2^e - hi),  e = 14 - exponent(max over the operand's block)  (activations: one block per
128 rows x cb channels, clamped at 54; weights: one per output channel).  lo_a lo_w is never formed.

This file holds, in numpy (never the code under test):
  * the format: block_exp, the two roundings (split), the 128-byte line layout (lines), pack_act / pack_rows / unpack;
  * the arithmetic: three_product (fp64; exact for the operands below), with the switches the host suite mutates;
  * the launch: plan (launch_pp's arithmetic), xcd_remap and walks (the persistent workgroups' tile walk), simulate (what a
    launch leaves in C or cmax / cidx, tile by tile, wave row by wave row);
  * operands(case): integer-valued fp32 operands with
      - small entries +-1..4 (lo = 0) and, per row and 32-deep chunk, one odd entry in [2^11, 2^bigbits) (lo != 0): at an
        even k in the activations, at an odd k in the weights, so lo_a lo_w = 0 at every k and the absent product is exact;
      - whole exponent blocks times 1, 2 or 4 (amul: the activation blocks along k and from row tile to row tile; wmul: the
        weight rows), a zero activation block, a zero weight row, a block whose maximum is a power of two;
      - duplicated rows at distances 1, 4, 32 and 64 inside every 128-row tile (ties for the arg-max: across the registers
        of a lane, the two lane halves and the 32-row groups), planted maxima (mode 1), integer bias;
    so that sum_k |a w| + |bias| < 2^24: every partial sum in any order is an integer below 2^24, every rounding inside
    the kernel is exact, and the expected result is the plain product X W^T + b in fp64.
  * the real-valued pass: real_operands, simulate_f32 (the kernel's formats with one fp32 summation order) and real_bound
    (the per-element rounding bound derived in the header of tests/test_split_gemm_gpu.py);
  * the encoder's real layers: integer conv weights (no lo piece) and integer clouds drawn from a finite set of points, for
    which h1..h4 and layer 5 are exact per point (encoder_weights, encoder_base_points, encoder_cloud, encoder_chain).
tests/test_split_gemm_law_host.py proves these preconditions for every case of the tables in tests/test_split_gemm_gpu.py."""
import numpy as np

TARGET = 14
EXP_MAX = 54


# ---------------------------------------------------------------------------------------------------------------- format
def frexp_exp(m):
    """Exponent e of a non-negative fp32 m = f 2^e, f in [0.5, 1), from its bits; 0 for zero and subnormals."""
    E = (np.asarray(m, np.float32).view(np.uint32).astype(np.int64) >> 23) & 0xff
    return np.where(E > 0, E - 126, 0)


def block_exp(m, clamp=True):
    e = TARGET - frexp_exp(m)
    return np.minimum(e, EXP_MAX) if clamp else e


def pow2(e):
    return np.ldexp(np.float32(1), np.clip(e, -126, 127)).astype(np.float32)


def split(x, e):
    """The two roundings: x fp32, e the exponent(s) (broadcast) -> (hi, lo) f16."""
    xs = (np.asarray(x, np.float32) * pow2(e)).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def _rows_of(tile_vals, M):
    return np.repeat(tile_vals, 128, axis=0)[:M]


def pack_act(X, cb, clamp=True):
    """pp_pack_kernel: one exponent per 128 rows x cb channels -> (hi, lo (M, K) f16, exp (tiles, K / cb) int32).
    clamp=False, cb = K: conv_split_kernel's activation split (absmax_kernel's maximum per 128-row tile)."""
    X = np.asarray(X, np.float32)
    M, K = X.shape
    tiles, ncb = (M + 127) // 128, K // cb
    pad = np.zeros((tiles * 128, K), np.float32)
    pad[:M] = np.abs(X)
    m = pad.reshape(tiles, 128, ncb, cb).max(axis=(1, 3))
    e = block_exp(m, clamp).astype(np.int32)
    hi, lo = split(X, np.repeat(_rows_of(e, M), cb, axis=1))
    return hi, lo, e


def pack_rows(W):
    """split_rows_kernel: one exponent per row, not clamped."""
    W = np.asarray(W, np.float32)
    e = block_exp(np.abs(W).max(axis=1), clamp=False).astype(np.int32)
    hi, lo = split(W, e[:, None])
    return hi, lo, e


def lines(hi, lo):
    """The memory image: row r = K / 32 lines of 128 bytes, line kt = [hi of channels 32 kt .. 32 kt + 31 | lo of the same].
    -> uint16 (rows, 2 K), the same bytes as K fp32."""
    R, K = hi.shape
    img = np.stack([hi.reshape(R, K // 32, 32), lo.reshape(R, K // 32, 32)], axis=2)
    return np.ascontiguousarray(img).view(np.uint16).reshape(R, 2 * K)


def unlines(img, K):
    img = np.ascontiguousarray(img).view(np.float16).reshape(-1, K // 32, 2, 32)
    return img[:, :, 0].reshape(-1, K), img[:, :, 1].reshape(-1, K)


def unpack(hi, lo, e):
    """pp_unpack_kernel: (f32(hi) + f32(lo)) 2^-e in fp32; e broadcast to the elements."""
    return ((hi.astype(np.float32) + lo.astype(np.float32)) * pow2(-np.asarray(e))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ arithmetic
def three_product(ah, al, aexp, cb, wh, wl, wexp, drop=None, rescale=True):
    """sum over the k-blocks of (hi hi + hi lo + lo hi) 2^-e_a, times 2^-e_w, in fp64 (M, N); no bias.
    drop: "hilo" / "lohi" leaves that product out; rescale=False: the accumulators are not rescaled where the activation
    exponent changes along k (everything is unscaled by the first block's exponent)."""
    M, K = ah.shape
    Ah, Al, Wh, Wl = (t.astype(np.float64) for t in (ah, al, wh, wl))
    out = np.zeros((M, wh.shape[0]))
    for kb in range(K // cb):
        ks = slice(kb * cb, (kb + 1) * cb)
        S = Ah[:, ks] @ Wh[:, ks].T
        if drop != "hilo":
            S += Ah[:, ks] @ Wl[:, ks].T
        if drop != "lohi":
            S += Al[:, ks] @ Wh[:, ks].T
        e = _rows_of(aexp[:, kb if rescale else 0], M).astype(np.float64)
        out += S * np.exp2(-e)[:, None]
    return out * np.exp2(-wexp.astype(np.float64))[None, :]


# ---------------------------------------------------------------------------------------------------------------- launch
def pp_bn(N):
    return 256 if N >= 256 else 128


def plan(M, N, mode, n=1):
    """launch_pp's arithmetic: (bn, bm, tiles_n, tiles, workgroups, threads), or None where it refuses."""
    bn = pp_bn(N)
    if mode not in (0, 1) or n <= 0 or M <= 0 or N <= 0 or N % bn:
        return None
    tiles_n = N // bn
    small = mode == 0 and bn == 128
    bm = 128 if small else 256
    tiles = -(-M // bm) * tiles_n
    cap = max(256 * (2 if small else 1) // n, 1)
    wgs = min(tiles, cap)
    mult = 8 * tiles_n // (8 if tiles_n % 8 == 0 else (tiles_n if 8 % tiles_n == 0 else 1))
    if wgs >= mult:
        wgs = wgs // mult * mult
    elif tiles >= tiles_n:
        wgs = tiles_n
    return (bn, bm, tiles_n, tiles, wgs, 256 if small else 512)


def xcd_remap(b, nwg):
    """conv_pp_kernel's remap of blockIdx.x (hardware: workgroup b runs on XCD b % 8) to a tile-walk start."""
    q, r8, xcd = nwg >> 3, nwg & 7, b & 7
    return (xcd * (q + 1) if xcd < r8 else r8 * (q + 1) + (xcd - r8) * q) + (b >> 3)


def walks(pl, skip_last=False):
    """{wg: the tiles it visits}; skip_last: a walk that stops one tile early wherever it has more than one."""
    _, _, _, tiles, wgs, _ = pl
    out = {}
    for b in range(wgs):
        wg = xcd_remap(b, wgs)
        w = list(range(wg, tiles, wgs))
        out[wg] = w[:-1] if skip_last and len(w) > 1 else w
    return out


def simulate(c, ops, mode, drop=None, rescale=True, tie="first", clamped_wins=False, skip_last=False):
    """What hp_gemm_pp_prepare + hp_gemm_pp_run(mode) leave behind, walked tile by tile as the kernel walks them; what no
    workgroup writes stays NaN (cidx: -1).  mode 0 -> C (M, N) fp64 as hp_gemm_pp_unpack returns it; mode 1 -> (cmax, cidx).
    The keyword switches are the mutations of the host suite."""
    M, N, K, cb = c["M"], c["N"], c["K"], c["xcb"]
    X, W, b = ops["X"], ops["W"], ops["b"]
    ah, al, aexp = pack_act(X, cb)
    wh, wl, wexp = pack_rows(W)
    T = three_product(ah, al, aexp, cb, wh, wl, wexp, drop, rescale) + b.astype(np.float64)[None, :]
    bn, bm, tiles_n, tiles, wgs, _ = pl = plan(M, N, mode)
    t128 = (M + 127) // 128
    C = np.full((M, N), np.nan)
    cmax, cidx = np.full((t128, N), np.nan), np.full((t128, N), -1, np.int64)
    for wg, tl in walks(pl, skip_last).items():
        col0 = (wg % tiles_n) * bn                       # the kernel takes its column tile from wg, once
        for tile in tl:
            row0 = (tile // tiles_n) * bm
            for r0 in range(row0, min(row0 + bm, M), 128):
                rows = np.minimum(np.arange(r0, r0 + 128), M - 1)      # the DMA clamps: rows past M repeat row M - 1
                v = T[rows, col0:col0 + bn]
                live = np.arange(r0, r0 + 128) < M
                if mode == 1:
                    if not clamped_wins:
                        v = np.where(live[:, None], v, -np.inf)
                    mx = v.max(axis=0)
                    hit = v == mx[None, :]
                    first = hit.argmax(axis=0)
                    last = 127 - hit[::-1].argmax(axis=0)
                    at = last if tie == "last" or clamped_wins else first
                    cmax[r0 // 128, col0:col0 + bn] = mx
                    cidx[r0 // 128, col0:col0 + bn] = (r0 + at) % c.get("group_rows", 128 * t128)
                    continue
                if c["relu"]:
                    v = np.maximum(v, 0.0)
                e = int(block_exp(np.float32(np.abs(v).max())))
                hi, lo = split(v.astype(np.float32), e)
                nlive = min(128, M - r0)
                C[r0:r0 + nlive, col0:col0 + bn] = unpack(hi, lo, e)[:nlive]
    return C if mode == 0 else (cmax, cidx)


def expected(c, ops):
    """The plain product: fp64 X W^T + b (ReLU for mode 0's store) -> (C, cmax, cidx by the first-row rule)."""
    M = c["M"]
    want = ops["X"].astype(np.float64) @ ops["W"].astype(np.float64).T + ops["b"].astype(np.float64)[None, :]
    t128 = (M + 127) // 128
    pad = np.full((t128 * 128, c["N"]), -np.inf)
    pad[:M] = want
    pad = pad.reshape(t128, 128, -1)
    cmax = pad.max(axis=1)
    cidx = (pad == cmax[:, None, :]).argmax(axis=1) + 128 * np.arange(t128)[:, None]
    return (np.maximum(want, 0.0) if c["relu"] else want), cmax, cidx % c.get("group_rows", 128 * t128)


# -------------------------------------------------------------------------------------------------------------- operands
AMUL = (1, 4, 2, 2, 1, 4, 1, 2, 4, 2, 2, 1, 1, 4, 2, 1)     # along k: rises, falls, stays; row tile t starts at entry 3 t
DUP = (1, 4, 32, 64)                                         # distance of the duplicated rows in 128-row tile t % 4
PLANT_K, PLANT_A = 2, 256                                    # the channel and the activation value of a planted maximum


def amul_table(t128, ncb):
    a = np.array([[AMUL[(kb + 3 * t) % 16] for kb in range(ncb)] for t in range(t128)], np.int64)
    if t128 >= 2:
        a[1, ncb // 2] = 0                                   # a zero block (between two non-zero ones where ncb >= 3)
    return a


def operands(c):
    """Integer-valued fp32 X (M, K), W (N, K), b (N) of case c (see the header).  Keys read: M, N, K, xcb, seed and the
    optional bigbits (default 13 for K <= 128, else 12), bias ("rand" | "zero" | "neg" | "neg0": -2^21 on every column /
    on the first column tile | "pow2": rand with one entry exactly 1024), plants [(row, copy_of_row | None)]."""
    M, N, K, cb = c["M"], c["N"], c["K"], c["xcb"]
    rng = np.random.default_rng(c["seed"])
    bits = c.get("bigbits", 13 if K <= 128 else 12)
    nch, t128, ncb = K // 32, (M + 127) // 128, K // cb

    def ints(rows, parity):
        v = rng.integers(1, 5, (rows, K)) * rng.choice([-1, 1], (rows, K))
        pos = 2 * rng.integers(0, 16, (rows, nch)) + parity + 32 * np.arange(nch)[None, :]
        big = (2 * rng.integers(2 ** 10, 2 ** (bits - 1), (rows, nch)) + 1) * rng.choice([-1, 1], (rows, nch))
        v[np.arange(rows)[:, None], pos] = big
        return v

    A = ints(M, 0)
    r = np.arange(M)
    d = np.array(DUP)[(r // 128) % 4]
    A = A[np.where(((r % 128) // d) % 2 == 1, r - d, r)]                  # row r + d repeats row r
    plants = c.get("plants", ())
    if plants:
        A[:, PLANT_K] = 0
    for row, src in plants:
        if src is not None:
            A[row] = A[src]
        A[row, PLANT_K] = PLANT_A
    A[0, 0] = 2 ** bits                                                   # block (0, 0): a power-of-two maximum
    A *= np.repeat(_rows_of(amul_table(t128, ncb), M), cb, axis=1)

    Wt = ints(N, 1)
    if plants:
        Wt[:, PLANT_K] = 2 ** 11 + 1 + 2 * rng.integers(0, 8, N)
    Wt *= np.array([1, 2])[(np.arange(N) // 3) % 2][:, None]
    Wt[5] = 0                                                             # a row of zeros

    kind = c.get("bias", "rand")
    b = rng.integers(-1000, 1001, N)
    if kind == "zero":
        b[:] = 0
    elif kind == "neg":
        b[:] = -2 ** 21
    elif kind == "neg0":
        b[:pp_bn(N)] = -2 ** 21
    elif kind == "pow2":
        b[7] = 1024
    return {"X": A.astype(np.float32), "W": Wt.astype(np.float32), "b": b.astype(np.float32)}


def sum_bound(ops):
    """max over the outputs of sum_k |a w| (1 + 2^-9) + |b|: above every partial sum, in any order, of the piece products
    (|hi| <= |x| (1 + 2^-11), |lo| <= 2^-11 |x|) and the bias.  The operands are integers: the smallest term's unit is >= 1."""
    s = np.abs(ops["X"]).astype(np.float64) @ np.abs(ops["W"]).astype(np.float64).T
    return float((s * (1 + 2.0 ** -9) + np.abs(ops["b"]).astype(np.float64)[None, :]).max())


# ----------------------------------------------------------------------------------------------- the real-valued pass
def real_operands(c):
    """Real-valued operands: rows spanning e^+-4, 10^5 between the two halves of K (the column blocks of a row tile)."""
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.default_rng(c["seed"])
    X = rng.standard_normal((M, K)) * np.exp(2 * rng.standard_normal((M, 1)).clip(-2, 2))
    X[:, K // 2:] *= 1e-5
    W = rng.standard_normal((N, K)) * np.exp(rng.standard_normal((N, 1)))
    b = rng.standard_normal(N)
    return {"X": X.astype(np.float32), "W": W.astype(np.float32), "b": b.astype(np.float32)}


def simulate_f32(c, ops):
    """Mode 0 with the kernel's number formats for any operands: the piece products (exact in fp32) added one by one to an
    fp32 accumulator in k order (per 16-deep step hi hi, then hi lo, then lo hi), the exact rescale between k-blocks, the
    bias fma, ReLU, the store's split under the output block's exponent, the unpack.  -> fp32 (M, N).  One summation order
    out of many: the real-valued pass measures its error against real_bound, and allows the kernel twice that."""
    M, N, K, cb = c["M"], c["N"], c["K"], c["xcb"]
    ah, al, aexp = pack_act(ops["X"], cb)
    wh, wl, wexp = pack_rows(ops["W"])
    Ah, Al, Wh, Wl = (t.astype(np.float32) for t in (ah, al, wh, wl))
    acc = np.zeros((M, N), np.float32)
    for k0 in range(0, K, 16):
        if k0 and k0 % cb == 0:
            acc *= pow2(_rows_of(aexp[:, k0 // cb] - aexp[:, k0 // cb - 1], M))[:, None]
        for a, w in ((Ah, Wh), (Ah, Wl), (Al, Wh)):
            for k in range(k0, k0 + 16):
                acc += a[:, k, None] * w[None, :, k]
    e = _rows_of(aexp[:, -1], M).astype(np.float64)[:, None] + wexp.astype(np.float64)[None, :]
    v = (acc.astype(np.float64) * np.exp2(-e) + ops["b"].astype(np.float64)[None, :]).astype(np.float32)
    if c["relu"]:
        v = np.maximum(v, np.float32(0))
    out = np.empty_like(v)
    bn = pp_bn(N)
    for r0 in range(0, M, 128):
        for c0 in range(0, N, bn):
            blk = v[r0:r0 + 128, c0:c0 + bn]
            eo = int(block_exp(np.abs(blk).max()))
            out[r0:r0 + 128, c0:c0 + bn] = unpack(*split(blk, eo), eo)
    return out


def real_bound(c, ops, want):
    """The rounding bound of the header of tests/test_split_gemm_gpu.py, per element, from the reference `want` (fp64, after
    ReLU) and the operands: splits + absent lo lo + fp32 accumulation of 3 K products + the bias fma + the stored pair."""
    M, N, K, cb = c["M"], c["N"], c["K"], c["xcb"]
    aX, aW = np.abs(ops["X"]).astype(np.float64), np.abs(ops["W"]).astype(np.float64)
    t128, ncb = (M + 127) // 128, K // cb
    pad = np.zeros((t128 * 128, K))
    pad[:M] = aX
    amax = np.repeat(_rows_of(pad.reshape(t128, 128, ncb, cb).max(axis=(1, 3)), M), cb, axis=1)     # block maxima, per element
    wmax = aW.max(axis=1)
    dX = 2.0 ** -22 * aX + 2.0 ** -38 * amax            # |x - (hi + lo) 2^-e|: two roundings, or lo's subnormal floor
    dW = 2.0 ** -22 * aW + 2.0 ** -38 * wmax[:, None]
    S = aX @ aW.T
    splits = dX @ aW.T + aX @ dW.T + dX @ dW.T
    lolo = 2.0 ** -22 * S * (1 + 2.0 ** -10)
    accum = 3 * K * 2.0 ** -24 * S * (1 + 2.0 ** -9)
    v = np.abs(want)
    bn = pp_bn(N)
    vp = np.zeros((t128 * 128, N))
    vp[:M] = v
    cmaxb = np.repeat(_rows_of(vp.reshape(t128, 128, N // bn, bn).max(axis=(1, 3)), M), bn, axis=1)
    store = 2.0 ** -24 * v + 2.0 ** -22 * v + 2.0 ** -38 * cmaxb
    return splits + lolo + accum + store


# ------------------------------------------------------------------------------------------------- the encoder's layers
ENC_WIDTHS = (3, 64, 128, 256, 512, 512)
ENC_AMP = (40, 10, 20, 40, 5, 30, 40, 0, 15, 40, 25)        # coordinate range of the base cloud's 128-point tiles (one is all zero)


def encoder_weights(seed):
    """Integer conv weights and biases of the five layers for which the whole stack is exact on encoder_cloud's points:
    W1 dense in [-31, 31]; W2..W5 sparse (6 non-zeros per row, at most 11 significant bits: their lo pieces are zero), the
    second half of W4's rows larger than the first (h4's two exponent blocks differ); biases integers, growing with the layer.
    h1 already exceeds 2^11 with odd low bits, so every split activation has non-zero lo pieces."""
    rng = np.random.default_rng(seed)
    Ws = [rng.integers(-31, 32, (64, 3))]
    for l, top in ((2, 3), (3, 2), (4, 1), (5, 3)):
        cout, cin = ENC_WIDTHS[l], ENC_WIDTHS[l - 1]
        W = np.zeros((cout, cin), np.int64)
        for n in range(cout):
            W[n, rng.choice(cin, 6, replace=False)] = rng.integers(1, top + 1, 6) * rng.choice([-1, 1], 6)
        if l == 4:
            W[256:] *= 4
        Ws.append(W)
    bs = [rng.integers(-(4 ** l) * 8, (4 ** l) * 8 + 1, ENC_WIDTHS[l]) for l in range(1, 6)]
    return [W.astype(np.float32) for W in Ws], [b.astype(np.float32) for b in bs]


def encoder_base_points(seed):
    """11 tiles of 128 integer points, tile t within +-ENC_AMP[t]: the finite set every cloud of the encoder cases draws from."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.integers(-a, a + 1, (128, 3)) for a in ENC_AMP]).astype(np.float32)


def encoder_cloud(B, Np, seed):
    """(B, Np, 3): 128-row tile t of the flattened batch holds points of base tile t % 11, drawn with repetition (ties within
    a tile and, from 11 tiles on, across tiles) — every point is one of encoder_base_points(seed)."""
    base = encoder_base_points(seed)
    rng = np.random.default_rng(seed + 1)
    R = B * Np
    t = (np.arange(R) // 128) % len(ENC_AMP)
    return base[128 * t + rng.integers(0, 128, R)].reshape(B, Np, 3)


def encoder_chain(x, Ws, bs):
    """fp64: h1..h4 (after ReLU) and layer 5's values for points x (R, 3), and per layer max over the rows of sum |h| |w| + |b|."""
    h, hs, sums = x.astype(np.float64), [], []
    for l in range(5):
        W, b = Ws[l].astype(np.float64), bs[l].astype(np.float64)
        sums.append(float((np.abs(h) @ np.abs(W).T + np.abs(b)[None, :]).max()))
        h = h @ W.T + b[None, :]
        if l < 4:
            h = np.maximum(h, 0.0)
        hs.append(h)
    return hs, sums

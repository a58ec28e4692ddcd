"""The laws of csrc/aux_kernels.hip in numpy — the checker of the point sampler, the device-drawn random-plane slicer, the
KLD term and the step's loss scalars, written from what each kernel is documented to compute, not from how it
is launched: nothing here knows of blocks, waves, loop widths or LDS.

Every value these kernels write is a chain of single-rounding fp32 operations (the library is built with fp contraction off;
sqrt and division are IEEE) over Philox4x32-10 words, except where expf enters the KLD.  So the laws are numpy float32
expressions, one numpy operation per rounding, and the GPU suite compares bits; the KLD with general v is compared against
float64 within a bound derived per call (kld_bound).

    sampler_law      point i, attempt a = 0..63: Philox block with counter (i_lo, i_hi ^ (a << 8), offset_lo, offset_hi) and key
                     (seed_lo, seed_hi); coordinates (w >> 8) * 2^-23 - 1 of words 0..2 (exact); n2 = fma(z, z, fma(y, y, x*x));
                     the first attempt with n2 < 1 is the point; nrm = sqrt(n2); if nrm < float32(coef) the point is scaled by
                     float32(coef) / nrm.
    slice_law        candidate c = 4 * round + wave of cloud b: Philox blocks with counter (b, round, wave, k), k = 0, 1, 2, key =
                     seed; uniforms (w >> 8) * 2^-24; p0 from k = 0, u = p1 - p0, v = p2 - p0, normal f = u x v (products
                     rounded, then the difference), bias = (fx*p0x + fy*p0y) + fz*p0z; a point is "under" when
                     ((x*fx + y*fy) + z*fz) + bias > 0; the first candidate with under == target, or else N - under == target,
                     is accepted and its `target` side is part_a, both parts in the cloud's point order.
    kld_*            0.5 * sum(exp(v) + mu^2 - 1 - v) / B (core/epoch_loops.py:29-30) in float64, its error bound, and its exact
                     fp32 value where v == 0.
    step_losses_law  (c_cd * cd, kld, c_emd * (((cost0 + cost1) + cost2) + ...), (out0 + out1) + out2).
"""
import hashlib

import numpy as np

from scan_law import philox4x32_10

F32 = np.float32
U = 2.0 ** -24                       # unit roundoff of fp32
ATTEMPTS = 64                        # rejection attempts per point before the sampler gives up
WAVES = 4                            # candidates per round of the slicer
MASK64 = 2 ** 64 - 1


def _words(x):
    x = int(x) & MASK64
    return x & 0xFFFFFFFF, x >> 32


# ---------------------------------------------------------------------------------------------------------------------
# point sampler
# ---------------------------------------------------------------------------------------------------------------------
def push_out(xyz, n2, coef):
    """The sampler's last step on accepted points xyz (n, 3) float32 with squared norms n2 (n) float32: points with
    sqrt(n2) < float32(coef) are scaled by float32(coef) / sqrt(n2); a point AT the origin goes to (coef, 0, 0).  No feasible
    draw reaches the origin branch (it needs three words with (w >> 8) == 2^23 in one block, and then coef > 0): the host
    suite calls this function with such rows directly."""
    xyz = np.array(xyz, F32, copy=True).reshape(-1, 3)
    coef = F32(coef)
    nrm = np.sqrt(np.asarray(n2, F32))
    inner = nrm < coef
    at_origin = inner & ~(nrm > 0)
    scaled = inner & (nrm > 0)
    s = coef / nrm[scaled]
    xyz[scaled] = xyz[scaled] * s[:, None]
    xyz[at_origin] = (coef, F32(0), F32(0))
    return xyz


def exhausted_point(coef):
    """What the sampler writes for a point none of whose 64 attempts fell inside the ball (probability (1 - pi/6)^64 = 2e-21
    per point: no feasible draw reaches it, so the host suite calls this directly): the origin, then the push-out rule."""
    return push_out(np.zeros((1, 3), F32), np.zeros(1, F32), coef)[0]


def sampler_attempt(index, attempt, seed, offset):
    """(integer coordinates a (n, 3) int64 with coordinate = a / 2^23, n2 * 2^46 as float64 holding fp32 values) of
    attempt `attempt` of the points `index` (uint64)."""
    index = np.asarray(index, np.uint64)
    k0, k1 = _words(seed)
    o0, o1 = _words(offset)
    hi = (index >> np.uint64(32)) ^ np.uint64((int(attempt) << 8) & 0xFFFFFFFF)
    w = philox4x32_10(index & np.uint64(0xFFFFFFFF), hi, o0, o1, k0, k1)
    a = np.stack([(w[c] >> np.uint64(8)).astype(np.int64) - 2 ** 23 for c in range(3)], 1)
    # squares are integers < 2^47 and every partial sum an integer < 2^49: exact in float64, so each float32() below is
    # the single rounding of one fp32 multiply / fma (scaled by 2^46, a power of two: the same rounding)
    sq = (a * a).astype(np.float64)
    t = sq[:, 0].astype(F32).astype(np.float64)
    t = (sq[:, 1] + t).astype(F32).astype(np.float64)
    t = (sq[:, 2] + t).astype(F32).astype(np.float64)
    return a, t


def sampler_law(total, coef, seed, offset, return_attempts=False):
    """hp_sample_points(total, coef, seed, offset) -> (total, 3) float32 [, the accepted attempt of every point (total) int]."""
    total = int(total)
    out = np.zeros((total, 3), F32)
    n2 = np.zeros(total, F32)
    accepted = np.full(total, ATTEMPTS, np.int64)
    pending = np.arange(total, dtype=np.uint64)
    for attempt in range(ATTEMPTS):
        if pending.size == 0:
            break
        a, t = sampler_attempt(pending, attempt, seed, offset)
        ok = t < 2.0 ** 46
        rows = pending[ok].astype(np.int64)
        out[rows] = (a[ok].astype(np.float64) * 2.0 ** -23).astype(F32)          # exact: |a| <= 2^23
        n2[rows] = (t[ok] * 2.0 ** -46).astype(F32)                              # exact: t holds an fp32 value
        accepted[rows] = attempt
        pending = pending[~ok]
    out = push_out(out, n2, coef)                                                 # (rows left pending: exhausted_point)
    return (out, accepted) if return_attempts else out


# ---------------------------------------------------------------------------------------------------------------------
# device-drawn random-plane slicer
# ---------------------------------------------------------------------------------------------------------------------
def slice_candidates(cloud, seed, first, count, order=("cloud", "round")):
    """Candidates first .. first + count - 1 of cloud `cloud` as (count, 4) float32 rows (fx, fy, fz, bias).
    `order`: which of (cloud, round) is counter word 0 and which word 1 (the host suite's mutation swaps them)."""
    c = np.arange(first, first + count, dtype=np.uint64)
    rnd, wave = c // np.uint64(WAVES), c % np.uint64(WAVES)
    word = {"cloud": np.full(count, int(cloud), np.uint64), "round": rnd}
    k0, k1 = _words(seed)
    p = []
    for k in range(3):
        w = philox4x32_10(word[order[0]], word[order[1]], wave, k, k0, k1)
        p.append(np.stack([(w[j] >> np.uint64(8)).astype(F32) * F32(2.0 ** -24) for j in range(3)], 1))      # exact
    p0, u, v = p[0], p[1] - p[0], p[2] - p[0]
    f = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1],
                  u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                  u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    bias = (f[:, 0] * p0[:, 0] + f[:, 1] * p0[:, 1]) + f[:, 2] * p0[:, 2]
    out = np.concatenate([f, bias[:, None]], 1)
    assert out.dtype == F32
    return out


def under_counts(points, planes):
    """How many of points (N, 3) float32 each of planes (K, 4) float32 has "under" it, (K) int64."""
    x, y, z = (np.ascontiguousarray(points[:, j], F32)[None, :] for j in range(3))
    rows = max(1, (1 << 18) // points.shape[0])            # a cache-sized slab of candidates at a time
    out = np.empty(planes.shape[0], np.int64)
    for r in range(0, planes.shape[0], rows):
        pl = planes[r:r + rows]
        t = x * pl[:, 0:1]
        t += y * pl[:, 1:2]
        t += z * pl[:, 2:3]
        t += pl[:, 3:4]
        out[r:r + rows] = (t > 0).sum(1)
    return out


def under_mask(points, plane):
    points = np.asarray(points, F32)
    return ((points[:, 0] * plane[0] + points[:, 1] * plane[1]) + points[:, 2] * plane[2]) + plane[3] > 0


_FIRST = {}


def first_accepted(points, cloud, target, seed, limit, rule="lowest", order=("cloud", "round")):
    """(candidate number, under count) of the first accepted candidate below `limit` of one cloud, or (-1, -1).
    rule "lowest": candidates in order; "any": the HIGHEST accepting wave of the first accepting round (a mutation)."""
    points = np.ascontiguousarray(points, F32)
    n = points.shape[0]
    key = (hashlib.sha1(points.tobytes()).hexdigest(), int(cloud), int(target), int(seed) & MASK64, rule, order)
    found, searched = _FIRST.get(key, ((-1, -1), 0))
    if found[0] >= 0 or searched >= limit:
        return found if 0 <= found[0] < limit else (-1, -1)
    chunk = 64                                             # (a multiple of WAVES: a round never straddles two chunks)
    first = searched
    while first < limit:
        count = min(chunk, limit - first)
        chunk = min(2 * chunk, 4096)
        cnt = under_counts(points, slice_candidates(cloud, seed, first, count, order))
        ok = np.flatnonzero((cnt == target) | (n - cnt == target))
        if ok.size:
            j = int(ok[0])
            if rule == "any":
                same_round = ok[(ok + first) // WAVES == (j + first) // WAVES]
                j = int(same_round[-1])
            found = (first + j, int(cnt[j]))
            break
        first += count
    _FIRST[key] = (found, limit if found[0] < 0 else found[0] + 1)
    return found


def slice_law(points, target, seed, max_rounds, rule="lowest", prefer="under", order=("cloud", "round")):
    """hp_slice_clouds(B, N, target, points, seed, max_rounds) -> (part_a (B, target, 3), part_b (B, N - target, 3),
    plane (B, 4) float32, status (B) int32, index (B) int64 = the accepted candidate's number 4 * round + wave, -1 if none).
    The rows of a cloud with status 1 are NaN here: the kernel writes nothing for it.
    rule / prefer / order: the host suite's mutations ("any" accepting wave; the "other" side at a tie of sides; the
    counter words swapped)."""
    points = np.ascontiguousarray(points, F32)
    B, N = points.shape[:2]
    part_a = np.full((B, target, 3), np.nan, F32)
    part_b = np.full((B, N - target, 3), np.nan, F32)
    plane = np.full((B, 4), np.nan, F32)
    status = np.ones(B, np.int32)
    index = np.full(B, -1, np.int64)
    for b in range(B):
        c, under = first_accepted(points[b], b, target, seed, WAVES * int(max_rounds), rule=rule, order=order)
        if c < 0:
            continue
        pl = slice_candidates(b, seed, c, 1, order)[0]
        m = under_mask(points[b], pl)
        assert int(m.sum()) == under
        both = under == target and N - under == target
        a_is_under = (under == target) if prefer == "under" or not both else False
        if not a_is_under:
            m = ~m
        part_a[b], part_b[b], plane[b], status[b], index[b] = points[b][m], points[b][~m], pl, 0, c
    return part_a, part_b, plane, status, index


# ---------------------------------------------------------------------------------------------------------------------
# KLD
# ---------------------------------------------------------------------------------------------------------------------
def kld_f64(v, mu, batch, g=1.0):
    """core/epoch_loops.py:29-30 in float64: (value, d value * g / d v, d value * g / d mu)."""
    v, mu = np.asarray(v, np.float64), np.asarray(mu, np.float64)
    value = 0.5 * np.sum(np.exp(v) + mu * mu - 1.0 - v) / batch
    return value, 0.5 * g / batch * (np.exp(v) - 1.0), g / batch * mu


def ulp32(x):
    """Spacing of fp32 at |x| (float64 in, float64 out; normal range)."""
    return 2.0 ** (np.floor(np.log2(np.abs(np.asarray(x, np.float64)))) - 23)


def kld_bound(v, mu, batch, E=2.0):
    """Error bound of an fp32 evaluation of the forward value whose expf is within E ulp, whose products, sums and
    differences round once each and whose accumulation is exact (float64 against fp32 terms):
      sum_i [ E ulp32(exp v_i) + u (m_i^2 + |exp v_i + m_i^2| + |exp v_i + m_i^2 - 1| + |term_i|) ] * 0.5 / B + 3 u |value|
    (the four u terms: the roundings of m*m, of the sum, of the - 1 and of the - v; 3 u: fl32(1/B), the final rounding, and
    slack for second-order terms)."""
    v, mu = np.asarray(v, np.float64), np.asarray(mu, np.float64)
    e, m2 = np.exp(v), mu * mu
    term = e + m2 - 1.0 - v
    per = E * ulp32(e) + U * (m2 + np.abs(e + m2) + np.abs(e + m2 - 1.0) + np.abs(term))
    return float(np.sum(per) * 0.5 / batch + 3 * U * abs(0.5 * np.sum(term) / batch))


def kld_grad_v_bound(v, batch, g, E=2.0):
    """Element-wise error bound of 0.5 * fl(g * fl(1/B)) * fl(expf(v) - 1) against 0.5 * g / B * (exp(v) - 1):
      0.5 |g| / B * [ E ulp32(exp v_i) + u |exp v_i - 1| ] + 4 u |grad_i|
    (the expf error and the rounding of the - 1 scaled by the factor; 4 u: fl32(1/B), g * that, the final product — 0.5 * is
    exact — and slack for second-order terms)."""
    v = np.asarray(v, np.float64)
    e = np.exp(v)
    return 0.5 * abs(g) / batch * (E * ulp32(e) + U * np.abs(e - 1.0)) + 4 * U * np.abs(0.5 * g / batch * (e - 1.0))


def kld_exact_terms(mu):
    """The fp32 terms fl(fl(fl(1 + fl(m^2)) - 1) - 0) of the forward where v == 0 (expf(0) == 1), as float64."""
    mu = np.asarray(mu, F32)
    one, zero = F32(1), F32(0)
    return ((((one + mu * mu).astype(F32)) - one).astype(F32) - zero).astype(np.float64)


def kld_exact_v0(mu, batch, skip=None, twice=None):
    """hp_kld_forward where v == 0, to the bit: the fp32 terms summed in float64, times 0.5 and float64(float32(1/B)),
    rounded to fp32.  With mu = k/64, k <= 1021, every term and the float64 sum are exact, so the summation order does not
    matter.  skip / twice: the host suite's mutations (one element left out / counted twice)."""
    t = kld_exact_terms(mu).reshape(-1)
    total = float(np.sum(t))
    assert total < 2.0 ** 52                      # (with terms that are multiples of 2^-12: the float64 sum is exact)
    if skip is not None:
        total -= float(t[skip])
    if twice is not None:
        total += float(t[twice])
    inv_b = np.float64(F32(1) / F32(batch))
    return F32(0.5 * total * inv_b)


def kld_grad_mu_law(mu, batch, g):
    """grad_mu = fl(fl(g * fl(1/B)) * mu), float32."""
    scale = F32(F32(g) * (F32(1) / F32(batch)))
    return (scale * np.asarray(mu, F32)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# step losses
# ---------------------------------------------------------------------------------------------------------------------
def step_losses_law(cd, kld, cost, c_cd, c_emd, pairwise=False):
    """hp_step_losses -> (4) float32.  kld / cost None: the term is absent.  pairwise: the host suite's mutation (the cost
    sum taken as a balanced tree instead of left to right)."""
    e = F32(0)
    if cost is not None:
        cost = np.asarray(cost, F32)
        if pairwise:
            level = list(cost)
            while len(level) > 1:
                level = [F32(level[i] + level[i + 1]) if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
            e = level[0] if level else F32(0)
        else:
            for c in cost:
                e = F32(e + c)
    out0 = F32(F32(c_cd) * F32(cd))
    out1 = F32(kld) if kld is not None else F32(0)
    out2 = F32(F32(c_emd) * e)
    return np.array([out0, out1, out2, F32(F32(out0 + out1) + out2)], F32)


# ---------------------------------------------------------------------------------------------------------------------
# case tables, shared by tests/test_aux_law_host.py (which proves what they cover) and tests/test_aux_kernels_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
SAMPLER_TOTALS = (1, 255, 256, 257, 100000)
SAMPLER_COEFS = (0.0, float(np.linspace(0, 1, 100)[36]), 0.37, 1.0)
SAMPLER_SEEDS = ((7, 1), (2 ** 32 + 7, 1), (67280421310721, 3), (2 ** 64 - 1, 2 ** 32), (5, 2 ** 63 + 5))

SLICE_CASES = ((2, 1), (3, 1), (3, 2), (63, 1), (63, 31), (63, 62), (64, 32), (65, 1), (65, 33), (65, 64), (255, 127),
               (256, 1), (256, 128), (256, 255), (257, 129), (333, 100), (1000, 500), (2048, 1), (2048, 1024), (2048, 2047),
               (8192, 4096))
SLICE_SEEDS = (7, 2 ** 40 + 3)
SLICE_CLOUDS = 3                     # clouds per call: the cloud index is a counter word
SLICE_LIMIT = 40000                  # every table cloud's first accepted candidate lies below this
BALL_CASE = (2048, 1024)
STATUS_CASES = ((63, 1), (256, 128), (2048, 1024), (8192, 4096))   # one cloud alone needs the call's last round


RESEED = {(8192, 4096): 2}           # cases whose first clouds needed more than SLICE_LIMIT candidates: drawn again


def slice_clouds_of(N, target):
    """The table's clouds of a case: (3, N, 3) float32 uniform in [0, 1)^3."""
    rs = np.random.RandomState(100003 * N + target + RESEED.get((N, target), 0))
    return rs.random_sample((SLICE_CLOUDS, N, 3)).astype(F32)


def ball_clouds():
    """(3, 2048, 3) float32: clouds uniform in the ball of radius 1/2 about the origin (normalised shapes are centred)."""
    return (sampler_law(SLICE_CLOUDS * BALL_CASE[0], 0.0, 11, 1) * F32(0.5)).reshape(SLICE_CLOUDS, BALL_CASE[0], 3)


KLD_N = (1, 2, 255, 256, 257, 1023, 1024, 1025, 3072, 3073, 4095, 4096, 4097, 7169, 8192, 8193, 12289)
KLD_BATCH = (1, 3, 64)
KLD_G = (1.0, 3.0, 2.0 ** -20)
KLD_REGIMES = ("workload", "collapse", "wide")


def kld_exact_mu(n):
    """mu = +-k/64 with k in [512, 1021] varying by element: k <= 1021 keeps every term and the sum exact; k >= 512 keeps
    every term (>= 64) above the fp32 spacing of 0.5 * sum / B (sum <= 12289 * 255 < 2^22, spacing <= 0.25 at the sum's
    scale), so one element left out or counted twice always changes the fp32 result."""
    i = np.arange(n, dtype=np.int64)
    k = 512 + (i * 37) % 510
    return (np.where(i % 3 == 1, -k, k) / 64.0).astype(F32)


def kld_inputs(n, batch, regime):
    rs = np.random.RandomState(1000003 * KLD_REGIMES.index(regime) + 131 * n + batch)
    if regime == "workload":                                   # v = exp(logvar) of an early model in [0, 0.5), mu ~ N(0, 1)
        return (rs.random_sample(n) * 0.5).astype(F32), rs.standard_normal(n).astype(F32)
    if regime == "collapse":                                   # |v|, |mu| <= 1e-3: exp(v) - 1 - v cancels
        return ((rs.random_sample(n) * 2 - 1) * 1e-3).astype(F32), ((rs.random_sample(n) * 2 - 1) * 1e-3).astype(F32)
    return ((rs.random_sample(n) * 2 - 1) * 60).astype(F32), rs.standard_normal(n).astype(F32)       # wide


STEP_B = (0, 1, 7, 8, 9, 15, 16, 17, 37, 64)
STEP_C_CD, STEP_C_EMD = 0.05, 0.05 / 2048


STEP_RESEED = {15: 7, 37: 1}         # drawn again until the left-to-right fp32 sum differs from the pairwise one


def step_inputs(b):
    """(cd, kld, cost (b) float32): costs rand * 100, so that the order of their sum matters."""
    rs = np.random.RandomState(500 + b + 1000 * STEP_RESEED.get(b, 0))
    return F32(rs.random_sample() * 2000), F32(rs.random_sample()), (rs.random_sample(b) * 100).astype(F32)

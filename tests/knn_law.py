"""The nearest-neighbour and outlier laws in numpy — the checker of csrc/knn.hip, written from the law itself.

Everything is per scan (rows offsets[s] .. offsets[s+1] of points (T,3) float32); rows of other scans never take part.

Neighbours
    d2(i, j)   = ((dx*dx + dy*dy) + dz*dz) with dx = q_i.x - p_j.x etc., every operation one float32 rounding (fps_law's
                 formula).  A NaN d2 counts as +inf; an overflowed +inf is a legal value.
    absent     a row with a non-finite coordinate: nobody's candidate, and as a query it gets the empty result.
    candidates of query i: the present rows j of the same scan, and j != i under exclude_self (the default, and required when
                 the queries are the scan itself), ordered by the pair (d2 as its uint32 bit pattern, j), ascending.
    result     the first k candidates: index (k) rows within the scan, dist2 (k) float32; slots beyond the number of
                 candidates hold index -1 and dist2 +inf.
The result for k is the first k columns of the result for any larger k: a test may compute the largest once.

Outlier statistics (k, ratio), with c_i the number of valid slots of row i
    m_i        = float32((sum_t sqrt64(float64(dist2_t))) / c_i), the float64 sum sequential in slot order.  Rows with c_i = 0
                 or a non-finite m_i are absent too: never kept, not in the statistics.
    M          = the largest m_i of the n_p participating rows; n_p <= 1 or M == 0: all participating rows are kept.
    q_i        = trunc(m_i * 2^(23-e)), e = floor(log2 M) from the bits: exact, 0 <= q_i < 2^24
    S1, S2     = sum q_i, sum q_i^2, exact integers
    mu = double(S1) / n_p;  var = max(0, (double(S2) - mu * double(S1)) / (n_p - 1));  thr = mu + double(float32(ratio)) * sqrt(var)
    keep i iff double(q_i) <= thr      (each line one float64 operation per rounding; integers convert round-to-nearest-even)
"""
import functools

import numpy as np

INF = np.float32(np.inf)


def _f32(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    assert a.ndim == 2 and a.shape[1] == 3
    return a


def d2_block(queries, cloud):
    """d2(i, j) for every query i and every row j of the cloud, float32 (nq, n); NaN -> +inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = queries[:, None, :] - cloud[None, :, :]
        sq = d * d
        out = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    assert out.dtype == np.float32
    out[np.isnan(out)] = INF
    return out


def knn_scan(cloud, k, queries=None, exclude_self=True, block=512):
    """(index (nq,k) int32, dist2 (nq,k) float32) of one scan; queries None: the scan itself."""
    cloud = _f32(cloud)
    own = queries is None
    assert not (own and not exclude_self) and k >= 1
    queries = cloud if own else _f32(queries)
    n, nq = len(cloud), len(queries)
    index = np.full((nq, k), -1, dtype=np.int32)
    dist2 = np.full((nq, k), INF, dtype=np.float32)
    present = np.isfinite(cloud).all(axis=1)
    rows = np.flatnonzero(present)                              # ascending: a stable sort by d2 then orders by (d2, j)
    if len(rows) == 0:
        return index, dist2
    for lo in range(0, nq, block):
        q = queries[lo:lo + block]
        asks = np.flatnonzero(np.isfinite(q).all(axis=1))      # absent queries keep the empty result
        if len(asks) == 0:
            continue
        d2 = d2_block(q[asks], cloud[rows])
        bits = d2.view(np.uint32).astype(np.int64)              # d2 >= 0: the bit patterns order as the values do
        if exclude_self:
            me = lo + asks                                      # query i skips candidate row i
            pos = np.searchsorted(rows, me)
            hit = (pos < len(rows)) & (rows[np.minimum(pos, len(rows) - 1)] == me)
            bits[np.flatnonzero(hit), pos[hit]] = np.int64(1) << 40     # behind every candidate; cut off below
        order = np.argsort(bits, axis=1, kind="stable")[:, :k]
        took = np.take_along_axis(bits, order, axis=1) < (np.int64(1) << 40)
        idx = np.where(took, rows[order], -1).astype(np.int32)
        dd = np.where(took, np.take_along_axis(d2, order, axis=1), INF).astype(np.float32)
        index[lo + asks, :idx.shape[1]] = idx
        dist2[lo + asks, :dd.shape[1]] = dd
    return index, dist2


def knn_law(points, offsets, k, queries=None, query_offsets=None, exclude_self=None):
    """(index (Q,k) int32, dist2 (Q,k) float32) over a ragged set; queries / query_offsets: a second ragged set, default the
    scans themselves."""
    points, offsets = _f32(points), np.asarray(offsets, dtype=np.int64)
    if exclude_self is None:
        exclude_self = queries is None
    if queries is not None:
        queries, query_offsets = _f32(queries), np.asarray(query_offsets, dtype=np.int64)
        assert len(query_offsets) == len(offsets)
    qo = offsets if queries is None else query_offsets
    index = np.full((int(qo[-1]), k), -1, dtype=np.int32)
    dist2 = np.full((int(qo[-1]), k), INF, dtype=np.float32)
    for s in range(len(offsets) - 1):
        cloud = points[offsets[s]:offsets[s + 1]]
        q = None if queries is None else queries[qo[s]:qo[s + 1]]
        index[qo[s]:qo[s + 1]], dist2[qo[s]:qo[s + 1]] = knn_scan(cloud, k, q, exclude_self)
    return index, dist2


def mean_dist_law(index, dist2):
    """m_i (Q) float32 from the neighbour lists: +inf for rows without a valid slot or with a non-finite mean."""
    total = np.zeros(len(index), dtype=np.float64)
    count = np.zeros(len(index), dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(index.shape[1]):                         # slot order: the float64 sum is sequential
            valid = index[:, t] >= 0
            total = np.where(valid, total + np.sqrt(dist2[:, t].astype(np.float64)), total)
            count += valid
        m = (total / count).astype(np.float32)
    m[(count == 0) | ~np.isfinite(m)] = INF
    return m


def keep_law(m, ratio):
    """(keep (n) bool, kept) of one scan from its m_i."""
    m = np.asarray(m, dtype=np.float32)
    part = np.isfinite(m)
    n_p = int(part.sum())
    if n_p == 0:
        return part, 0
    M = m[part].max()
    if n_p <= 1 or M == 0:
        return part, n_p
    bits = int(M.view(np.uint32))
    field, mant = bits >> 23, bits & 0x7FFFFF
    e = field - 127 if field else (mant.bit_length() - 1) - 149
    scaled = np.ldexp(m[part].astype(np.float64), 23 - e)      # exact
    q = np.trunc(scaled).astype(np.int64)
    assert q.min() >= 0 and q.max() < (1 << 24)
    S1, S2 = sum(int(v) for v in q), sum(int(v) * int(v) for v in q)       # Python integers: exact
    assert S2 < (1 << 64)
    f1, f2 = np.float64(float(S1)), np.float64(float(S2))       # int -> float rounds to nearest even
    mu = f1 / np.float64(n_p)
    var = max(np.float64(0), (f2 - mu * f1) / np.float64(n_p - 1))
    thr = mu + np.float64(np.float32(ratio)) * np.sqrt(var)
    keep = np.zeros(len(m), dtype=bool)
    keep[np.flatnonzero(part)] = q.astype(np.float64) <= thr
    return keep, int(keep.sum())


def outliers_law(points, offsets, k=16, ratio=2.0, lists=None):
    """(keep (T) bool, mean_dist (T) float32, kept (S) int64) over a ragged set.  lists: knn_law's result for the same set
    and a k at least as large, if the caller has it already (its first k columns are the lists for k)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    index, dist2 = knn_law(points, offsets, k) if lists is None else (lists[0][:, :k], lists[1][:, :k])
    mean = mean_dist_law(index, dist2)
    keep = np.zeros(len(mean), dtype=bool)
    kept = np.zeros(len(offsets) - 1, dtype=np.int64)
    for s in range(len(offsets) - 1):
        keep[offsets[s]:offsets[s + 1]], kept[s] = keep_law(mean[offsets[s]:offsets[s + 1]], ratio)
    return keep, mean, kept


STRAYS = ((4.5, 0.0, 0.0), (-4.5, 0.0, 0.0), (0.0, 3.0, 0.0), (0.0, 0.0, -4.0), (2.0, 2.0, -2.0))


def shell_with_strays(n_shell=1024, seed=0):
    """The recipe of the outlier tests: n_shell points on the faces of the box [-0.5, 0.5]^3 (the first six one on each
    face, so the box is exact), five strays at 3 to 6 units that stretch the bounding box to a side of 9, and one NaN row,
    shuffled: (points (n_shell + 6, 3) float32, the shell's rows ascending)."""
    r = np.random.RandomState(seed)
    p = r.uniform(-0.5, 0.5, (n_shell, 3))
    face = r.randint(0, 6, n_shell)
    face[:6] = np.arange(6)
    p[np.arange(n_shell), face % 3] = np.where(face < 3, -0.5, 0.5)
    pts = np.concatenate([p, np.array(STRAYS), np.full((1, 3), np.nan)]).astype(np.float32)
    where = r.permutation(len(pts))                             # strays and the NaN row anywhere in the scan
    out = np.empty_like(pts)
    out[where] = pts
    return out, np.sort(where[:n_shell])


MIX_LENGTHS = (1, 2, 8, 9, 16, 17, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4097)


@functools.lru_cache(maxsize=None)
def ragged_mix(tile):
    """The ragged set of the GPU suites: scans of MIX_LENGTHS and of tile - 1, tile, tile + 1 points in mixed order, so that
    scan boundaries fall inside waves, chunks and tiles; uniform in [-1, 1]^3 with a few repeated points.  Returns
    (points, offsets, lengths, (index, dist2) of knn_law at k = 32) — computed once per process, read-only."""
    lengths = sorted(set(MIX_LENGTHS) | {tile - 1, tile, tile + 1})
    r = np.random.RandomState(11)
    lengths = [lengths[i] for i in r.permutation(len(lengths))]
    clouds = []
    for n in lengths:
        c = r.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        if n >= 8:
            c[r.randint(0, n, n // 8)] = c[r.randint(0, n, n // 8)]      # equal distances: the order by row matters
        clouds.append(c)
    points = np.concatenate(clouds)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    lists = knn_law(points, offsets, 32)
    for a in (points, offsets) + lists:
        a.setflags(write=False)
    return points, offsets, tuple(lengths), lists

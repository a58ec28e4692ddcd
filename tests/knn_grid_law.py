"""What the grid-backed neighbour search (csrc/knn_grid.hip) adds to tests/knn_law.py — nothing of that file is
restated here.

The lists are knn_law's, bit for bit: the grid is an acceleration structure and no property of it shows in any output.
keep_law_long is knn_law.keep_law with S2 as an exact integer of up to 70 bits (q_i < 2^24, n_p <= 2^22) converted to double
by round-to-nearest-even — Python's float(int) is correctly rounded — so it equals keep_law wherever that is defined.
knn_rows gives the law's lists for a sample of query rows of one long scan.  grid_search_model restates the kernel's cell
assignment, block growth and stopping rule for arbitrary grid parameters: run against knn_law.knn_scan on the CPU it shows
that the stopping rule is conservative under fp32 rounding before any GPU run.
"""
import numpy as np

import knn_law

INF = knn_law.INF
GRID_MAX_POINTS = 1 << 22


def keep_law_long(m, ratio):
    """(keep (n) bool, kept) of one scan of up to 2^22 rows from its m_i: knn_law.keep_law with an exact S2 of any size."""
    m = np.asarray(m, dtype=np.float32)
    part = np.isfinite(m)
    n_p = int(part.sum())
    assert n_p <= GRID_MAX_POINTS
    if n_p == 0:
        return part, 0
    M = m[part].max()
    if n_p <= 1 or M == 0:
        return part, n_p
    bits = int(M.view(np.uint32))
    field, mant = bits >> 23, bits & 0x7FFFFF
    e = field - 127 if field else (mant.bit_length() - 1) - 149
    q = np.trunc(np.ldexp(m[part].astype(np.float64), 23 - e)).astype(np.int64)      # exact
    assert q.min() >= 0 and q.max() < (1 << 24)
    S1 = int(q.sum())                                               # below 2^46: exact in int64
    sq = q * q                                                      # below 2^48
    S2 = (int((sq >> 32).sum()) << 32) + int((sq & 0xFFFFFFFF).sum())       # Python integers: exact, up to 70 bits
    f1, f2 = np.float64(float(S1)), np.float64(float(S2))           # int -> float rounds to nearest even
    mu = f1 / np.float64(n_p)
    var = max(np.float64(0), (f2 - mu * f1) / np.float64(n_p - 1))
    thr = mu + np.float64(np.float32(ratio)) * np.sqrt(var)
    keep = np.zeros(len(m), dtype=bool)
    keep[np.flatnonzero(part)] = q.astype(np.float64) <= thr
    return keep, int(keep.sum())


def _first_k(bits, rows, k):
    """The first k of every line of candidates by (bits, row): (index (nq,k) int32, dist2 (nq,k) float32).  bits (nq,c)
    int64 — 1 << 40 marks a candidate that does not count; rows (c) the candidates' row numbers, ascending."""
    nq = len(bits)
    index = np.full((nq, k), -1, dtype=np.int32)
    dist2 = np.full((nq, k), INF, dtype=np.float32)
    if bits.shape[1] == 0:
        return index, dist2
    assert (np.diff(rows) > 0).all()                                # ascending rows: a stable sort by bits orders by (bits, row)
    order = np.argsort(bits, axis=1, kind="stable")[:, :k]
    got = np.take_along_axis(bits, order, axis=1)
    took = got < (np.int64(1) << 40)
    index[:, :order.shape[1]] = np.where(took, rows[order], -1)
    dist2[:, :order.shape[1]] = np.where(took, got.astype(np.uint32).view(np.float32), INF)
    return index, dist2


def knn_rows(cloud, k, rows, block=64):
    """The law's lists of the query rows `rows` of one scan queried with itself (self excluded by row number):
    (index (len(rows),k) int32, dist2 (len(rows),k) float32) — what knn_law.knn_scan(cloud, k) holds at those rows."""
    cloud = knn_law._f32(cloud)
    rows = np.asarray(rows, dtype=np.int64)
    present = np.flatnonzero(np.isfinite(cloud).all(axis=1))
    index = np.full((len(rows), k), -1, dtype=np.int32)
    dist2 = np.full((len(rows), k), INF, dtype=np.float32)
    cand = cloud[present]
    for lo in range(0, len(rows), block):
        me = rows[lo:lo + block]
        asks = np.flatnonzero(np.isfinite(cloud[me]).all(axis=1))
        if len(asks) == 0 or len(present) == 0:
            continue
        bits = knn_law.d2_block(cloud[me[asks]], cand).view(np.uint32).astype(np.int64)
        bits[present[None, :] == me[asks][:, None]] = np.int64(1) << 40
        index[lo + asks], dist2[lo + asks] = _first_k(bits, present, k)
    return index, dist2


def edges(lo, h, G):
    """edge(j) = fl(lo + fl(float(j) * h)) for j = 0 .. G: float32, monotone in j."""
    j = np.arange(G + 1, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(lo) + j * np.float32(h)).astype(np.float32)


def cells_of(x, lo, h, G):
    """The cell of every coordinate: the largest j of [0, G) with edge(j) <= x, 0 if none — the first and the last cell are
    unbounded outwards."""
    e = edges(lo, h, G)[:G]
    return np.clip(np.searchsorted(e, x, side="right") - 1, 0, G - 1)


def grid_search_model(cloud, k, lo, h, G, queries=None, exclude_self=None, group=1, span=16, stats=None):
    """knn_law.knn_scan's lists of one scan by the kernel's search over the grid (lo (3), h, G (3)): rows binned by cells_of,
    the queries taken `group` at a time in cell order (a wave's lanes) and served in groups — the first lane not served yet
    and the lanes behind it on its (y, z) line of cells within `span` cells —, the block of cells that covers the group's
    cells grown by r shells, every lane done iff its list is full and its worst d2 is strictly below the smallest
    fl(fl(edge_face - q_c)^2) over the block's faces inside the grid, the block growing — doubling until the lists are full,
    then to the reach of the worst distance — until every lane is done or the block is the whole grid.
    stats: a dict that receives "sweeps" (the number of blocks swept), "groups" (their number), "early" (the groups the rule ended before the
    block was the whole grid) and "cells" (G)."""
    cloud = knn_law._f32(cloud)
    own = queries is None
    if exclude_self is None:
        exclude_self = own
    assert not (own and not exclude_self) and k >= 1
    queries = cloud if own else knn_law._f32(queries)
    lo, h, G = np.asarray(lo, dtype=np.float32), np.float32(h), [int(g) for g in G]
    nq = len(queries)
    index = np.full((nq, k), -1, dtype=np.int32)
    dist2 = np.full((nq, k), INF, dtype=np.float32)
    present = np.flatnonzero(np.isfinite(cloud).all(axis=1))
    asks = np.flatnonzero(np.isfinite(queries).all(axis=1))
    sweeps = early = 0
    groups = []
    if len(present) and len(asks):
        E = [edges(lo[c], h, G[c]) for c in range(3)]
        pc = np.stack([cells_of(cloud[present, c], lo[c], h, G[c]) for c in range(3)], axis=1)
        qc = np.stack([cells_of(queries[asks, c], lo[c], h, G[c]) for c in range(3)], axis=1)
        order = np.argsort((qc[:, 2] * G[1] + qc[:, 1]) * G[0] + qc[:, 0], kind="stable")
        top = np.array(G) - 1
        groups = []                                                 # a wave's lanes, served a line of cells at a time
        for g0 in range(0, len(asks), group):
            todo = list(order[g0:g0 + group])
            while todo:
                lead = qc[todo[0]]
                mine = [i for i in todo if qc[i][1] == lead[1] and qc[i][2] == lead[2] and 0 <= qc[i][0] - lead[0] < span]
                groups.append(np.array(mine))
                todo = [i for i in todo if i not in set(mine)]
        for lanes in groups:
            me, q = asks[lanes], queries[asks[lanes]]
            base0, base1 = qc[lanes].min(axis=0), qc[lanes].max(axis=0)
            r = 0
            while True:
                b0, b1 = np.maximum(base0 - r, 0), np.minimum(base1 + r, top)
                inside = np.flatnonzero(((pc >= b0) & (pc <= b1)).all(axis=1))
                rows = present[inside]
                bits = knn_law.d2_block(q, cloud[rows]).view(np.uint32).astype(np.int64)
                if exclude_self:
                    bits[rows[None, :] == me[:, None]] = np.int64(1) << 40
                idx, dd = _first_k(bits, rows, k)
                sweeps += 1
                if (b0 == 0).all() and (b1 == top).all():
                    break
                bound = np.full(len(lanes), INF, dtype=np.float32)
                with np.errstate(over="ignore"):
                    for c in range(3):
                        if b0[c] > 0:
                            t = (q[:, c] - E[c][b0[c]]).astype(np.float32)
                            bound = np.minimum(bound, (t * t).astype(np.float32))
                        if b1[c] < top[c]:
                            t = (E[c][b1[c] + 1] - q[:, c]).astype(np.float32)
                            bound = np.minimum(bound, (t * t).astype(np.float32))
                full = idx[:, k - 1] >= 0
                open_ = ~(full & (dd[:, k - 1].view(np.uint32) < bound.view(np.uint32)))
                if not open_.any():
                    early += 1
                    break
                if not full.all():
                    r = 2 * r if r else 1
                else:
                    with np.errstate(over="ignore", invalid="ignore"):
                        t = np.sqrt(dd[open_, k - 1]) / h
                    reach = np.where(t < 1023, np.where(t < 1023, t, 0).astype(np.int64) + 1, 1024)
                    r = max(r + 1, int(np.max(reach)))
            index[me], dist2[me] = idx, dd
    if stats is not None:
        stats["sweeps"], stats["early"], stats["groups"], stats["cells"] = sweeps, early, len(groups), tuple(G)
    return index, dist2

"""The exact-assignment law in numpy integers — the checker of csrc/assign.hip, written from the law itself.

Two clouds a (n,3) and b (n,3), float32.  Bidders are the points of a, objects the points of b.

Costs
    d2(i, j) = ((dx*dx + dy*dy) + dz*dz) with dx = a_i.x - b_j.x etc., every operation one float32 rounding (fps_law's)
    q(i, j)  = rint(sqrt_f32(d2) * 2^scale_log2) as an integer: the root float32 and correctly rounded, the product by the
               power of two float32 (exact short of overflow), rint to the nearest with ties to even
    a q that is not <= 2^30 (a NaN or infinity among the coordinates included) is an overflow: status -3

Auction (forward, Jacobi, eps-scaling), every quantity int64
    A(i, j) = -q(i, j) * (n + 1); price(j) = 0 at the start and kept from phase to phase
    eps     = max(max_ij q(i, j) * (n + 1) // 2, 1); after a phase eps = max(eps // THETA, 1); the phase run at eps = 1 is the last
    a phase starts with every bidder unassigned and runs rounds until none is

One round: every unassigned bidder i, all on the prices as they stood when the round began,
    v(j) = A(i, j) - price(j);  j1 = argmax_j v(j), the lowest j among equals;  v2 = max_{j != j1} v(j)  (n = 1: v2 = v1)
    bid  = price(j1) + (v(j1) - v2) + eps
then for every object that received a bid: the highest bid wins, the lowest bidder among equal bids; the previous owner, if
any, becomes unassigned; the price becomes the winning bid.

Nothing above depends on the order in which bidders or objects are visited: max, min and lowest-index rules only.

The rounds of all phases are counted together.  A pair that would need more than `max_rounds` rounds stops with status -1.
Since every A is a multiple of n + 1 and the last eps is 1, the final assignment is within n * eps < n + 1 of the optimum of
A, hence an exact optimum of q.

THETA = 4.  Measured on the host over the families below, rounds with 4 against 8: clustered n = 2048 22.1 k / 17.6 k, but
near-coincident n = 2048 32.1 k / 62.2 k, grid n = 2048 35.5 k / 43.7 k, near n = 256 3.5 k / 4.6 k, grid n = 256 2.3 k / 4.7 k:
8 gains a fifth on the easy family and loses up to half on the families that set the worst case, so 4 it is.
"""
import numpy as np

THETA = 4
Q_MAX = 1 << 30
OK, CAPPED, OVERFLOW = 0, -1, -3
_I64_MIN = np.iinfo(np.int64).min


def quantised_costs(a, b, scale_log2=20):
    """q (n,n) int64 and a flag: some q is not <= 2^30.  Entries that overflow hold Q_MAX + 1."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
    assert a.ndim == 2 and a.shape[1] == 3 and a.shape == b.shape and 0 <= scale_log2 <= 24
    with np.errstate(all="ignore"):
        d = a[:, None, :] - b[None, :, :]
        sq = d * d
        d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        r = np.rint(np.sqrt(d2) * np.float32(2.0 ** scale_log2))
        assert d.dtype == np.float32 and sq.dtype == np.float32 and d2.dtype == np.float32 and r.dtype == np.float32
        good = r <= np.float32(Q_MAX)                        # false for NaN
    q = np.where(good, r, np.float32(0)).astype(np.int64)
    q[~good] = Q_MAX + 1
    return q, bool((~good).any())


def assign_law(a, b, scale_log2=20, max_rounds=None, theta=THETA):
    """-> (assignment (n) int64: the object of each bidder, cost int64 = sum_i q(i, assignment_i), rounds int, status).
    Status CAPPED / OVERFLOW: assignment all -1, cost -1, rounds = the status (what the kernel writes)."""
    q, overflow = quantised_costs(a, b, scale_log2)
    n = len(q)
    fail = lambda s: (np.full(n, -1, dtype=np.int64), np.int64(-1), s, s)
    if overflow:
        return fail(OVERFLOW)
    A = -q * np.int64(n + 1)
    price = np.zeros(n, dtype=np.int64)
    eps = max(int(q.max()) * (n + 1) // 2, 1)
    rounds = 0
    while True:
        owner = np.full(n, -1, dtype=np.int64)               # of each object
        un = np.arange(n, dtype=np.int64)                    # unassigned bidders
        while len(un):
            if max_rounds is not None and rounds >= max_rounds:
                return fail(CAPPED)
            rounds += 1
            v = A[un] - price[None, :]
            rows = np.arange(len(un))
            j1 = np.argmax(v, axis=1)                        # the first of equal values: the lowest j
            v1 = v[rows, j1]
            if n > 1:
                v[rows, j1] = _I64_MIN
                v2 = v.max(axis=1)
            else:
                v2 = v1
            bid = price[j1] + (v1 - v2) + np.int64(eps)
            order = np.lexsort((un, -bid, j1))               # by object, then highest bid, then lowest bidder
            first = np.ones(len(un), dtype=bool)
            first[1:] = j1[order][1:] != j1[order][:-1]
            win = order[first]
            objs, winners = j1[win], un[win]
            displaced = owner[objs]
            owner[objs] = winners
            price[objs] = bid[win]
            lost = np.ones(len(un), dtype=bool)
            lost[win] = False
            un = np.concatenate([un[lost], displaced[displaced >= 0]])
        if eps == 1:
            break
        eps = max(eps // theta, 1)
    assignment = np.empty(n, dtype=np.int64)
    assignment[owner] = np.arange(n)
    cost = q[np.arange(n), assignment].sum(dtype=np.int64)
    return assignment, cost, rounds, OK


def assign_pairs_law(A, B, pairs, scale_log2=20, max_rounds=None):
    """The kernel's outputs for a pair list: (assignment (P,n) int32, cost (P) int64, rounds (P) int32); a pair whose index
    lies outside its set gets the -2 row."""
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    pairs = np.asarray(pairs).reshape(-1, 2)
    n = A.shape[1]
    asg = np.full((len(pairs), n), -1, dtype=np.int32)
    cost = np.full(len(pairs), -1, dtype=np.int64)
    rounds = np.full(len(pairs), -2, dtype=np.int32)
    memo = {}
    for p, (ia, ib) in enumerate(pairs.tolist()):
        if not (0 <= ia < len(A) and 0 <= ib < len(B)):
            continue
        if (ia, ib) not in memo:
            memo[(ia, ib)] = assign_law(A[ia], B[ib], scale_log2, max_rounds)
        s, c, r, _ = memo[(ia, ib)]
        asg[p], cost[p], rounds[p] = s, c, r
    return asg, cost, rounds


# ---- the input families of the host and GPU suites ---------------------------------------------------------------------
def uniform_cloud(rng, n):
    return rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)


def clustered_cloud(rng, n, clusters=8, spread=0.03):
    centres = rng.uniform(-0.4, 0.4, (clusters, 3))
    return (centres[rng.integers(0, clusters, n)] + rng.normal(0.0, spread, (n, 3))).astype(np.float32)


def grid_cloud(rng, n):
    """Points on the 4^3 grid of eighths, drawn with repetition: many exactly equal distances."""
    return (rng.integers(0, 4, (n, 3)) / 8.0).astype(np.float32)


def family_pair(family, n, seed):
    """(a, b) of one family: uniform, clustered, near (b shrunk to 1 %), grid (tie-heavy), identical (b = a permuted)."""
    rng = np.random.default_rng(seed)
    if family == "uniform":
        return uniform_cloud(rng, n), uniform_cloud(rng, n)
    if family == "clustered":
        return clustered_cloud(rng, n), clustered_cloud(rng, n)
    if family == "near":
        return uniform_cloud(rng, n), (uniform_cloud(rng, n) * np.float32(0.01)).astype(np.float32)
    if family == "grid":
        return grid_cloud(rng, n), grid_cloud(rng, n)
    if family == "identical":
        a = uniform_cloud(rng, n)
        assert len(np.unique(a, axis=0)) == n
        return a, a[rng.permutation(n)].copy()
    raise ValueError(family)


FAMILIES = ("uniform", "clustered", "near", "grid", "identical")

"""The cut by coordinate rank in numpy — the checker of csrc/axis_split.hip, written from the law itself.

One cloud of n rows, c_i the `axis` coordinate of row i:
    key(c)  = the order-preserving uint32 image of a float32: -0.0 first made +0.0, every NaN made 0xFFFFFFFF, then the sign
              bit flipped for c >= 0 and all bits flipped for c < 0 — numpy's float32 `<` order, -inf first, +inf last among
              the numbers, every NaN after +inf
    order   = the rows sorted by (key(c_i), i) ascending: equal keys, NaNs among themselves included, keep ascending i
    lower   = rows order[:k], upper = rows order[k:], copied bit for bit
The pairs (key, i) are distinct, so they are sorted as single uint64 integers: no float comparison, no np.argsort and no
question of stability enters.
"""
import numpy as np


def keys(c):
    """uint32 image of a float32 vector whose integer order is the law's order of the floats."""
    c = np.ascontiguousarray(c, dtype=np.float32)
    u = c.view(np.uint32).copy()
    mag = u & np.uint32(0x7FFFFFFF)
    u[u == np.uint32(0x80000000)] = 0                                    # -0.0 -> +0.0
    negative = (u & np.uint32(0x80000000)) != 0
    image = np.where(negative, ~u, u | np.uint32(0x80000000))
    image[mag > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)           # NaN, either sign, any payload
    return image.astype(np.uint32)


def split(cloud, k, axis=0):
    """(lower (k,3), upper (n-k,3), order (n) int64) of one float32 (n,3) cloud."""
    cloud = np.ascontiguousarray(cloud)
    assert cloud.dtype == np.float32 and cloud.ndim == 2 and cloud.shape[1] == 3 and axis in (0, 1, 2)
    n = len(cloud)
    assert 1 <= k <= n - 1
    packed = (keys(cloud[:, axis]).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    order = (np.sort(packed) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    rows = cloud.view(np.uint32)[order].view(np.float32)                 # integer copies: NaN payloads survive
    return rows[:k], rows[k:], order


def awkward_cloud(n, seed):
    """A float32 (n,3) cloud whose every coordinate mixes what an order can get wrong: plain values drawn from a few, so
    duplicates are everywhere, -0.0 next to +0.0, both infinities, denormals of both signs and NaNs of both signs with
    distinct payloads (the row number).  The special values land on random rows, a different set per coordinate."""
    r = np.random.RandomState(seed)
    bits = r.choice(np.linspace(-1, 1, max(n // 3, 2)).astype(np.float32), size=(n, 3)).view(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                        0x00800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32)
    for a in range(3):
        hit = r.rand(n) < 0.5
        bits[hit, a] = r.choice(special, size=int(hit.sum()))
        nan = r.rand(n) < 0.15
        rows = np.flatnonzero(nan).astype(np.uint32)
        bits[nan, a] = np.where(rows % 2 == 0, np.uint32(0x7FC00000), np.uint32(0xFF800001)) + (rows << np.uint32(1))
    return np.ascontiguousarray(bits).view(np.float32)

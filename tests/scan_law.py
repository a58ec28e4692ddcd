"""The scan-preparation law in numpy — the checker of csrc/scan_prep.hip, written from the law itself.

Philox4x32-10 with key = seed (lo, hi) and counter (stream_lo, stream_hi, q, tag); word i of a tag is lane i & 3 of block
q = i >> 2; key_i = word i of tag 0; draw_j = (uint64(word j of tag 1) * n) >> 32.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or scalars, values < 2**32) and the key -> the four output words as uint64 arrays < 2**32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = ((p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def words(seed, stream, tag, count):
    """The first `count` words of a tag of the sequence (seed, stream), as uint64 values < 2**32."""
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    q = np.arange((count + 3) // 4, dtype=np.uint64)
    out = philox4x32_10(stream & 0xFFFFFFFF, stream >> 32, q, tag, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(out, axis=1).reshape(-1)[:count]


def keys(seed, stream, n):
    return words(seed, stream, 0, n)


def draws(seed, stream, n, count):
    return ((words(seed, stream, 1, count) * np.uint64(n)) >> S32).astype(np.int64)


def index_law(seed, stream, n, target, replace):
    """The rows of an n-point scan that make its `target`-point version, as int64 (target)."""
    if n <= target:
        return np.concatenate([np.arange(n, dtype=np.int64), draws(seed, stream, n, target - n)])
    if replace:
        return draws(seed, stream, n, target)
    k = keys(seed, stream, n)
    order = np.lexsort((np.arange(n), k))              # by key, equal keys by index
    return np.sort(order[:target]).astype(np.int64)


def boxes_fp32(cloud):
    """(center (3), scale) of one (n, 3) cloud, every step in float32: the bounding box's middle and its largest side / 0.9."""
    cloud = np.asarray(cloud, dtype=np.float32)
    lo, hi = cloud.min(axis=0), cloud.max(axis=0)
    center = (hi + lo) / np.float32(2)
    scale = np.float32((hi - lo).max()) / np.float32(0.9)
    assert center.dtype == np.float32 and scale.dtype == np.float32
    return center, scale


def restore_fp32(completion, s_scale, center, scale):
    """(c / s_scale) * scale + center in float32, one rounding per operation."""
    c = np.asarray(completion, dtype=np.float32)
    out = c / np.float32(s_scale) * np.float32(scale) + np.asarray(center, dtype=np.float32)
    assert out.dtype == np.float32
    return out

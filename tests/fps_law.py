"""The farthest-point law in numpy float32 — the checker of csrc/fps.hip, written from the law itself.

A cloud of `count` valid rows p_0 .. p_{count-1}, k picks, a start row s:
    d2(i, j)   = ((dx*dx + dy*dy) + dz*dz) with dx = p_i.x - p_j.x etc., every operation one float32 rounding
    pick_0     = s, mind_i = d2(i, pick_0)
    pick_j     = argmax_i mind_i, equal values broken by the lowest i; then mind_i = min(mind_i, d2(i, pick_j))
    radius2[j] = max_i mind_i after picks 0..j
count < k is no special case: once every mind_i is 0 the arg-max is row 0.
"""
import numpy as np


def d2_to(cloud, j):
    """d2(i, j) for every row i of a float32 (n,3) cloud, as float32 (n)."""
    assert cloud.dtype == np.float32
    d = cloud - cloud[j]
    sq = d * d
    out = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    assert d.dtype == np.float32 and sq.dtype == np.float32 and out.dtype == np.float32
    return out


def fps_law(cloud, k, count=None, start=0):
    """(index (k) int64, radius2 (k) float32) of the first `count` rows (default: all) of one (n,3) cloud."""
    cloud = np.ascontiguousarray(np.asarray(cloud, dtype=np.float32))
    count = len(cloud) if count is None else int(count)
    assert cloud.ndim == 2 and cloud.shape[1] == 3 and 1 <= count <= len(cloud) and 0 <= start < count and k >= 1
    cloud = cloud[:count]                                    # rows at or beyond count take no part
    index, radius2 = np.empty(k, dtype=np.int64), np.empty(k, dtype=np.float32)
    pick, mind = int(start), None
    for j in range(k):
        index[j] = pick
        d = d2_to(cloud, pick)
        mind = d if mind is None else np.minimum(mind, d)
        assert mind.dtype == np.float32
        pick = int(np.argmax(mind))                          # the first of equal values: the lowest row
        radius2[j] = mind[pick]
    return index, radius2

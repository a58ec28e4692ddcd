"""CPU suite for tests/voxel_law.py, the checker of csrc/voxels.hip: the vectorised law against a plain dict of cells filled
row by row, the boundary rows worked out by hand, the ragged form, and the bisection of thinned(max_points=...)."""
import numpy as np
import pytest

import voxel_law

f32 = np.float32
HALF = 1 << 20


def _dict_of_cells(cloud, voxel, origin, keep):
    """The law once more, one row and one float32 operation at a time."""
    voxel = f32(voxel)
    cells, beyond = {}, 0
    with np.errstate(all="ignore"):
        for row, p in enumerate(cloud):
            if not all(np.isfinite(c) for c in p):
                continue
            u = [f32(c) if origin is None else f32(f32(c) - f32(o)) for c, o in zip(p, origin if origin is not None else p)]
            q = [np.floor(f32(c / voxel)) for c in u]
            if not all(-HALF <= c < HALF for c in q):
                beyond += 1
                continue
            q = tuple(int(c) for c in q)
            d = [f32(c - f32(f32(f32(k) + f32(0.5)) * voxel)) for c, k in zip(u, q)]
            d2 = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
            rank = (int(np.array(d2).view(np.uint32)), row) if keep == "center" else (row,)
            cells.setdefault(q, []).append((rank, row))
    n = len(cloud)
    label, size, mask = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    for members in cells.values():
        rows = [row for _, row in members]
        label[rows], size[rows] = min(rows), len(rows)
        mask[min(members)[1]] = 1
    return {"label": label, "size": size, "keep": mask, "kept": len(cells), "beyond": beyond}


def _same(got, want, what):
    for name in ("label", "size", "keep"):
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)
    assert int(got["kept"]) == int(want["kept"]) and int(got["beyond"]) == int(want["beyond"]), (what, got["kept"], got["beyond"])


@pytest.mark.parametrize("keep", voxel_law.KEEPS)
@pytest.mark.parametrize("voxel", [1e-3, 0.1, 0.5, 8.0])
def test_the_law_is_a_dict_of_cells(voxel, keep):
    r = np.random.RandomState(5)
    cloud = np.concatenate([r.uniform(-1.5, 1.5, (300, 3)), r.normal(0.3, 0.02, (200, 3))]).astype(f32)
    cloud[r.randint(0, 500, 20)] = cloud[r.randint(0, 500, 20)]                   # exact duplicates
    cloud[7, 1], cloud[90, 0], cloud[91, 2] = np.nan, np.inf, 3e9                  # absent, absent, beyond
    for origin in (None, np.array([0.37, -1.2, 0.05], dtype=f32)):
        got = voxel_law.voxel_scan(cloud, voxel, origin, keep)
        _same(got, _dict_of_cells(cloud, voxel, origin, keep), (voxel, keep, origin is None))
        assert got["keep"].sum() == got["kept"] == len(set(got["label"][got["label"] >= 0]))
        assert got["beyond"] == 1 and (got["label"][[7, 90, 91]] == -1).all()
    if voxel == 1e-3:
        assert got["kept"] > 450                                                   # the range the voxels are meant to span
    if voxel == 8.0:
        assert got["kept"] <= 8


def test_boundary_rows_by_hand():
    cloud, want = voxel_law.boundary_rows()
    for keep in voxel_law.KEEPS:
        got = voxel_law.voxel_scan(cloud, voxel_law.BOUNDARY_VOXEL, None, keep)
        hand = dict(want, keep=want[keep])
        _same(got, hand, keep)
        _same(_dict_of_cells(cloud, voxel_law.BOUNDARY_VOXEL, None, keep), hand, keep)


def test_bad_voxels_and_lengths_give_the_empty_result():
    cloud = np.random.RandomState(1).rand(40, 3).astype(f32)
    for voxel in (np.nan, np.inf, 0.0, -1.0, -0.0):
        got = voxel_law.voxel_scan(cloud, voxel)
        assert (got["label"] == -1).all() and not got["size"].any() and not got["keep"].any() and got["kept"] == got["beyond"] == 0
    got = voxel_law.voxel_scan(np.zeros((0, 3), f32), 0.1)
    assert got["label"].shape == (0,) and got["kept"] == 0


def test_the_ragged_form_is_the_scans_one_by_one():
    r = np.random.RandomState(9)
    lengths = [0, 37, 1, 200, 0, 64]
    points = r.uniform(-1, 1, (sum(lengths), 3)).astype(f32)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    voxel = np.array([0.1, 0.2, np.nan, 0.05, 0.1, 0.0], dtype=f32)
    origin = r.uniform(-1, 1, (len(lengths), 3)).astype(f32)
    got = voxel_law.voxel_law(points, offsets, voxel, origin, "center")
    for s, n in enumerate(lengths):
        lo, hi = offsets[s], offsets[s + 1]
        one = voxel_law.voxel_scan(points[lo:hi], voxel[s], origin[s], "center")
        _same({k: (got[k][lo:hi] if k in ("label", "size", "keep") else got[k][s]) for k in got}, one, s)
    assert got["kept"][2] == 0 and got["kept"][5] == 0 and got["kept"][3] > 0 and got["kept"].dtype == np.int32


def test_thin_to_ends_within_max_points():
    cloud = np.random.RandomState(3).normal(0, 0.3, (40000, 3)).astype(f32)
    for m in (8, 500, 4096):
        edge, res = voxel_law.thin_to(cloud, m)
        assert edge.dtype == f32 and 0 < edge <= voxel_law.box(cloud)[1]
        assert 1 <= res["kept"] <= m and res["beyond"] == 0 and res["keep"].sum() == res["kept"]
    assert res["kept"] > 4096 // 2                                   # 16 rounds come close to the finest grid that fits

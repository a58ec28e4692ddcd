"""CPU suite for the visibility law itself (tests/visibility_law.py): hand-made scenes whose answer is known
without the law, and the sphere shell of DESIGN.md 3t with the law's exact label counts recorded beside two conditions any
usable visibility test has to meet.  No GPU and no library: the GPU suite compares the kernels with this law bit for bit."""
import numpy as np
import pytest

import visibility_law as law

f32 = np.float32
GRID5 = np.linspace(-0.2, 0.2, 5)
NEAR_WALL = np.array([[x, y, 1.0] for y in GRID5 for x in GRID5], f32)
FAR_WALL = NEAR_WALL * f32(2)                              # the same rays from the origin: every far row behind a near one
WALLS = np.concatenate([NEAR_WALL, FAR_WALL])


@pytest.mark.parametrize("w", [0, 1, 2, 3, 4])
def test_far_wall_is_hidden_head_on(w):
    r = law.visibility_scan(WALLS, (0, 0, 0), 32, w, 0.01, 2.0)
    assert (r["label"][:25] == law.ON_SURFACE).all() and (r["label"][25:] == law.HIDDEN).all()
    assert r["winner"][:25].all() and not r["winner"][25:].any()
    keys = r["buffer"][r["buffer"] != law.EMPTY]
    assert len(keys) == 25 and ((keys >> np.uint64(32)) == f32(1).view(np.uint32)).all()       # the z-depth of a facing wall is constant
    assert sorted((keys & np.uint64(0xFFFFFFFF)).tolist()) == list(range(25))


def test_both_walls_are_visible_from_between_them():
    r = law.visibility_scan(WALLS, (0, 0, 1.5), 32, 1, 0.01, 2.0)
    assert (r["label"] == law.ON_SURFACE).all()
    faces = np.flatnonzero(r["buffer"] != law.EMPTY) // (32 * 32)
    assert set(faces.tolist()) == {4, 5}                   # +z and -z
    kind, pixel, _ = law.project(WALLS, (0, 0, 1.5), 32)
    assert (pixel[:25] // 1024 == 5).all() and (pixel[25:] // 1024 == 4).all() and (kind == 2).all()


def _slanted_wall():
    """A wall turned by 60 degrees about y, sampled five to ten times finer than the pixel's footprint at its depth."""
    xs, ys = np.arange(-0.5, 0.5001, 0.02), np.arange(-0.5, 0.5001, 0.05)
    return np.array([[x, y, 3.0 + np.tan(np.pi / 3) * x] for y in ys for x in xs], f32)


def test_slanted_wall_is_why_a_point_shadows_a_cone():
    wall = _slanted_wall()
    cone = law.visibility_scan(wall, (0, 0, 0), 32, 1, 0.01, 2.0)
    assert (cone["label"] == law.ON_SURFACE).all()
    cylinder = law.visibility_scan(wall, (0, 0, 0), 32, 1, 0.0, 0.0)
    assert (cylinder["label"] == law.HIDDEN).sum() > len(wall) // 2
    assert set(np.unique(cylinder["label"]).tolist()) == {law.ON_SURFACE, law.HIDDEN}
    assert (cone["winner"] == cylinder["winner"]).all() and (cone["buffer"] == cylinder["buffer"]).all()     # the buffer knows no tolerance


def test_special_rows():
    view = np.array([0.5, 0.25, -1.0], f32)
    cloud = np.array([[0.5, 0.25, -1.0], [np.nan, 0, 0], [0, np.inf, 0], [1.5, 1.25, 0.0], [1.5, 0.25, -1.0], [1.5, 0.25, -1.0],
                      [0.5, 1.25, 0.0], [-0.5, 0.25, -2.0]], f32)
    r = law.visibility_scan(cloud, view, 8, 0, 0.0, 0.0)
    #      at the viewpoint, NaN, Inf, |dx| = |dy| = |dz| -> +x, duplicates on +x (the lower row wins), dy = dz -> +y, dx = dz -> -x
    assert r["label"].tolist() == [1, 4, 4, 1, 1, 1, 1, 1]
    assert r["winner"].tolist() == [0, 0, 0, 1, 1, 0, 1, 1]
    kind, pixel, _ = law.project(cloud, view, 8)
    assert kind.tolist() == [1, 0, 0, 2, 2, 2, 2, 2]
    assert (pixel[3:] // 64).tolist() == [0, 0, 0, 2, 1]
    assert pixel[3] == 0 * 64 + 7 * 8 + 7                  # u = t = +1 exactly: clamped to the last pixel
    assert pixel[7] == 1 * 64 + 0 * 8 + 4                  # -x face: u = dy / a = 0 -> 4, t = dz / a = -1 -> 0
    assert (law.visibility_scan(cloud, (np.nan, 0, 0), 8)["label"] == law.ABSENT).all()


def test_overflowing_depths_stay_ordered():
    """6e38 is a double and rounds to +inf in fp32: rows 0 and 1 share a pixel with row 2 at 3e38, which wins it; rows 3 and
    4, duplicates, own a pixel at depth +inf — a key below the empty pixel's, the lower row first.  A row at depth +inf is
    never hidden: its tolerance is z0 * pitch = +inf, or NaN with pitch 0, and no comparison with either holds."""
    cloud = np.array([[3e38, 0, 0], [3e38, 1e37, 0], [0, 0, 0], [3e38, 3.2e38, 0], [3e38, 3.2e38, 0]], f32)
    r = law.visibility_scan(cloud, (-3e38, 0, 0), 4, 0, 0.0, 0.0)
    assert r["label"].tolist() == [1, 1, 1, 1, 1] and r["winner"].tolist() == [0, 0, 1, 1, 0]
    assert law.visibility_scan(cloud, (-3e38, 0, 0), 4, 0, 0.0, 2.0)["label"].tolist() == [1, 1, 1, 1, 1]
    keys = np.sort(r["buffer"][r["buffer"] != law.EMPTY])
    assert keys.tolist() == [(int(f32(3e38).view(np.uint32)) << 32) | 2, (0x7F800000 << 32) | 3]


# ---- the shell of DESIGN.md 3t: a unit sphere of seed 0 seen from (1.5, 2, 1) at R = 32, slope 2, margin 0.01 ---------------
SHELL_CASES = {(8192, 1): ([0, 2601, 5591, 0, 0], 309), (2048, 2): ([0, 685, 1363, 0, 0], 306)}


@pytest.fixture(scope="module")
def shells():
    out = {}
    for (n, w) in SHELL_CASES:
        cloud = law.shell(n)
        out[n, w] = cloud, law.visibility_scan(cloud, law.SHELL_VIEW, 32, w, 0.01, 2.0)
    return out


@pytest.mark.parametrize("case", sorted(SHELL_CASES))
def test_shell_counts_and_conditions(shells, case):
    cloud, r = shells[case]
    counts, winners = SHELL_CASES[case]
    assert np.bincount(r["label"], minlength=5).tolist() == counts and int(r["winner"].sum()) == winners
    v = law.SHELL_VIEW.astype(np.float64)
    D = np.linalg.norm(v)
    along = cloud.astype(np.float64) @ (v / D)             # a row is truly visible iff along > 1 / D
    assert not ((along < 0) & (r["label"] == law.ON_SURFACE)).any()
    near = along > 1 / D + 0.1
    assert (r["label"][near] == law.HIDDEN).mean() <= 0.05


# queries of seed 1, 1024 rows, against the visible part of the 8192-row shell
QUERY_COUNTS = {0.6: [0, 14, 1010, 0, 0], 1.4: [55, 35, 452, 482, 0]}


@pytest.fixture(scope="module")
def visible_part(shells):
    cloud, r = shells[8192, 1]
    return cloud[r["label"] == law.ON_SURFACE]


@pytest.mark.parametrize("radius", sorted(QUERY_COUNTS))
def test_query_shells(visible_part, radius):
    q = law.shell(1024, seed=1, radius=radius)
    counts = np.bincount(law.visibility_scan(visible_part, law.SHELL_VIEW, 32, 1, 0.01, 2.0, queries=q)["label"], minlength=5)
    assert counts.tolist() == QUERY_COUNTS[radius]
    if radius < 1:
        assert counts[law.HIDDEN] >= 0.95 * len(q) and counts[law.SEEN_THROUGH] == 0       # behind the recorded surface but for stragglers
    else:
        assert (counts[:4] > 0).all()                      # in front of it, on its rim, behind its rim and beside it


def test_a_second_sample_of_the_shell_lies_on_the_surface_where_it_is_near(visible_part):
    """Queries on the recorded surface itself: the share labelled on the surface is the share of the sphere the sensor sees,
    within 0.1.  Why 0.1: the labels can differ from the truth only near the silhouette.  At depth z ~ 2.7 the tolerance of the
    centre pixel is 0.01 + 2.7 * (2 * 2 / 32) = 0.35; rows of the far side whose ray leaves the near side less than that in
    front of them, a chord of 2 * sqrt(1 - b^2) < 0.35, lie within 0.175 of the silhouette's plane: 0.0875 of the sphere's area.
    On the other side at most 5 % of the near rows may be hidden (the condition above), 0.016 of the sphere."""
    q = law.shell(1024, seed=1)
    v = law.SHELL_VIEW.astype(np.float64)
    D = np.linalg.norm(v)
    truth = (q.astype(np.float64) @ (v / D) > 1 / D).mean()
    label = law.visibility_scan(visible_part, law.SHELL_VIEW, 32, 1, 0.01, 2.0, queries=q)["label"]
    share = (label == law.ON_SURFACE).mean()
    print("on the surface", share, "near side", truth, np.bincount(label, minlength=5))
    assert abs(share - truth) <= 0.1
    assert (label == law.SEEN_THROUGH).sum() == 0


def test_ragged_law_keeps_scans_apart():
    a, b = law.shell(300, seed=2), law.shell(200, seed=3)
    points, offsets = np.concatenate([a, np.zeros((0, 3), f32), b]), [0, 300, 300, 500]
    views = np.array([[2, 0, 0], [0, 0, 0], [0, 0, 0]], f32)
    r = law.visibility_law(points, offsets, views, 16, 1)
    ra, rb = law.visibility_scan(a, views[0], 16, 1), law.visibility_scan(b, views[2], 16, 1)
    assert (r["label"] == np.concatenate([ra["label"], rb["label"]])).all()
    assert (r["buffer"][0].ravel() == ra["buffer"]).all() and (r["buffer"][1] == law.EMPTY).all()
    assert (rb["label"] == law.ON_SURFACE).all() and len(set((np.flatnonzero(rb["buffer"] != law.EMPTY) // 256).tolist())) == 6
    q = law.visibility_law(points, offsets, views, 16, 1, queries=np.ones((3, 3), f32), query_offsets=[0, 1, 2, 3])
    assert q["label"][1] == law.UNOBSERVED and "winner" not in q

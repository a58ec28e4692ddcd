"""CPU suite for tests/feature_law.py, the law csrc/features.hip is checked against: hand-worked pairs, theta exactly on a bin
boundary, and the sign-test binning against a straightforward fp64 atan2 formulation."""
import numpy as np

import feature_law as law

f32, f64 = np.float32, np.float64


def _pair(d, ni, nj):
    ok, bt, ba, bp = law.pair_bins(np.asarray([d], dtype=f32), np.asarray([ni], dtype=f64), np.asarray([nj], dtype=f64))
    return bool(ok[0]), int(bt[0]), int(ba[0]), int(bp[0])


def test_the_table_is_the_ten_boundaries():
    assert len(law.THETA) == 10
    for k, (c, s) in enumerate(law.THETA):
        angle = -np.pi + 2 * np.pi * (k + 1) / 11
        assert c == float(np.cos(angle)) and s == float(np.sin(angle))        # the literals are these doubles, bit for bit
        assert c.hex() and abs(c * c + s * s - 1) < 1e-15


def test_a_pair_with_bins_known_by_construction():
    # i at the origin with normal +z, j one step along x with normal +z: |n . d| ties at 0, so i is the source.
    # phi = 0 -> bin 5;  v = d x ns = (1,0,0) x (0,0,1) = (0,-1,0);  w = ns x v = (1,0,0);  alpha = v . nt = 0 -> bin 5;
    # theta = atan2(w . nt, ns . nt) = atan2(0, 1) = 0 -> the middle bin 5.
    assert _pair((1, 0, 0), (0, 0, 1), (0, 0, 1)) == (True, 5, 5, 5)
    # the target's normal tilted towards +x by 45 degrees: nt = (s, 0, s); j's |n . d| = s > 0, so j is the source and d flips.
    # ns = (s,0,s), d = (-1,0,0): phi = -s -> floor(11 * (1 - 0.7071) / 2) = 1;  v = d x ns = (0, s, 0) / s = (0,1,0);
    # w = ns x v = (-s, 0, s);  nt = (0,0,1): alpha = 0 -> 5;  y = s, x = s: theta = pi/4 -> floor(11 * (pi/4 + pi) / (2 pi)) = 6.
    s = np.sqrt(0.5)
    assert _pair((1, 0, 0), (0, 0, 1), (s, 0, s)) == (True, 6, 5, 1)
    # a normal against the line on both ends: alpha = +-1 at the clamp
    assert _pair((0, 1, 0), (1, 0, 0), (0, 0, 1))[0]


def test_skipped_pairs():
    assert not _pair((0, 0, 0), (0, 0, 1), (0, 0, 1))[0]                      # d = 0: a duplicated point
    assert not _pair((0, 0, 2), (0, 0, 1), (0, 0, 1))[0]                      # d along the source's normal: no frame
    assert not _pair((np.inf, 0, 0), (0, 0, 1), (0, 0, 1))[0]                 # an overflowed difference
    assert _pair((1e-30, 0, 0), (0, 0, 1), (0, 0, 1))[0]                      # tiny is not zero: fp64 holds its square


def test_theta_exactly_on_a_boundary_and_next_to_it():
    for k, (c, s) in enumerate(law.THETA):
        on = int(law.theta_bin(f64(c), f64(s)))
        assert on == k + 1                                                    # the boundary belongs to the upper bin
        for eps in (1e-12, -1e-12):
            x, y = c - eps * s, s + eps * c                                   # a turn by eps about the boundary
            assert int(law.theta_bin(f64(x), f64(y))) == (k + 1 if eps > 0 else k)
        assert int(law.theta_bin(f64(3.5 * c), f64(3.5 * s))) in (k, k + 1)   # scale may round, only to a neighbour
        assert int(law.theta_bin(f64(4 * c), f64(4 * s))) == k + 1            # a power of two is exact
    assert int(law.theta_bin(f64(-1), f64(0.0))) == 10 and int(law.theta_bin(f64(-1), f64(-0.0))) == 10
    assert int(law.theta_bin(f64(-1), f64(-1e-300))) == 0
    assert int(law.theta_bin(f64(0), f64(0))) == 5 and int(law.theta_bin(f64(1), f64(0))) == 5


def test_unit_bins():
    got = law.unit_bin(np.array([-1.0, -0.82, -0.8181, 0.0, 0.999, 1.0, 1.5, -2.0], dtype=f64))
    assert got.tolist() == [0, 0, 1, 5, 10, 10, 10, 0]


MARGIN = 1e-9          # radians; the measured largest distance of a disagreeing pair from a boundary is asserted below it


def test_the_sign_tests_bin_as_atan2_does():
    """The law's bins against numpy's float64 arctan2 / dot / cross on random pairs.  The two may differ only where theta lies
    within MARGIN of a boundary (or alpha / phi within it of one of theirs): a condition on the law, stated and measured
    here — on these 600 pairs they do not differ at all, and the closest theta to a boundary is far above MARGIN."""
    r = np.random.RandomState(7)
    n = 600
    d = r.normal(size=(n, 3)).astype(f32)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    ni, nj = unit(r.normal(size=(n, 3))).astype(f32).astype(f64), unit(r.normal(size=(n, 3))).astype(f32).astype(f64)
    ok, bt, ba, bp = law.pair_bins(d, ni, nj)
    rok, theta, alpha, phi = law.reference_bins(d, ni, nj)
    assert ok.all() and rok.all()
    want_t = np.minimum(np.floor(11 * (theta + np.pi) / (2 * np.pi)), 10).astype(np.int64)
    want_a = np.clip(np.floor(11 * (alpha + 1) / 2), 0, 10).astype(np.int64)
    want_p = np.clip(np.floor(11 * (phi + 1) / 2), 0, 10).astype(np.int64)
    edges = -np.pi + 2 * np.pi * np.arange(12) / 11
    gap_t = np.abs(theta[:, None] - edges[None, :]).min(axis=1)
    unit_edges = -1 + 2 * np.arange(12) / 11
    gap_a = np.abs(alpha[:, None] - unit_edges[None, :]).min(axis=1)
    gap_p = np.abs(phi[:, None] - unit_edges[None, :]).min(axis=1)
    print("disagreeing pairs (theta, alpha, phi):", int((bt != want_t).sum()), int((ba != want_a).sum()), int((bp != want_p).sum()),
          " closest to a boundary:", float(gap_t.min()), float(gap_a.min()), float(gap_p.min()))
    for got, want, gap in ((bt, want_t, gap_t), (ba, want_a, gap_a), (bp, want_p, gap_p)):
        differ = got != want
        assert (np.abs(got - want)[differ] == 1).all() and (gap[differ] < MARGIN).all()
    assert len(set(bt.tolist())) == 11                                        # every theta bin is met


def test_spfh_and_fpfh_of_a_small_scan_by_hand():
    # three usable rows on a line in x with normals +z, a fourth without a normal, a fifth not finite
    cloud = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0], [1, 1, 0], [np.nan, 0, 0]], dtype=f32)
    normals = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1]], dtype=f32)
    index = np.array([[1, 2, 3, 4], [0, 2, 1, -1], [0, 1, 7, 0], [0, 1, 2, 4], [0, 1, 2, 3]], dtype=np.int32)
    feat, count, spfh = law.feature_law(cloud, [0, 5], normals, index)
    # every valid pair is the (5, 5, 5) pair of the construction above; row 2 lists row 0 twice
    assert count.tolist() == [2, 2, 3, 0, 0] and spfh[:, 33].tolist() == [2, 2, 3, 0, 0]
    for i in range(3):
        assert spfh[i, 5] == spfh[i, 16] == spfh[i, 27] == count[i] and spfh[i, :33].sum() == 3 * count[i]
        assert feat[i, 5] == feat[i, 16] == feat[i, 27] >= 254 and feat[i].sum() == 3 * int(feat[i, 5])   # one bin holds everything;
        # the quotient (255 * F) / F may round just below 255
    assert not feat[3:].any() and not spfh[3:].any() and not feat[:, 33:].any()


def test_fpfh_weights_by_hand():
    # SPFH records given; three neighbours at squared distances 1, 2 and 2: w = 1, 1/2, 1/2 and W = 2, all exact
    cloud = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 1]], dtype=f32)
    spfh = np.zeros((4, 36), dtype=np.uint8)
    spfh[0, [0, 11, 22]], spfh[0, 33] = 4, 4                                   # row 0: everything in bin 0
    spfh[1, [1, 12, 23]], spfh[1, 33] = 2, 2                                   # row 1: bin 1
    spfh[2, [2, 13, 24]], spfh[2, 33] = 1, 1                                   # row 2: bin 2
    spfh[3, [3, 14, 25]], spfh[3, 33] = 1, 1                                   # row 3: bin 3
    index = np.array([[1, 2, 3], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]], dtype=np.int32)
    feat, count = law.fpfh_scan(cloud, index, spfh)
    # F = (1, 1/2, 1/4, 1/4), sum 2: bytes trunc(255 * F / 2)
    assert feat[0, :4].tolist() == [127, 63, 31, 31] and feat[0, 11:15].tolist() == [127, 63, 31, 31]
    assert feat[1, 1] == 255 and feat[2, 2] == 255 and count.tolist() == [4, 2, 1, 1]


def test_match_law_ties_and_absent_rows():
    a = np.zeros((4, 36), dtype=np.uint8)
    a[:, 0] = [10, 20, 30, 40]
    b = np.zeros((5, 36), dtype=np.uint8)
    b[:, 0] = [25, 15, 15, 35, 35]
    match, dist = law.match_law(a, [0, 4], b, [0, 5], [1, 1, 0, 1], [1, 1, 1, 0, 1])
    assert match.tolist() == [1, 0, -1, 4] and dist.tolist() == [25, 25, -1, 25]      # 20 ties among rows 0-2: the lower; target 3 is absent
    match, dist = law.match_law(a, [0, 4], b, [0, 5], [1, 1, 1, 1], [0, 0, 0, 0, 0])
    assert (match == -1).all() and (dist == -1).all()
    match, _ = law.match_law(a, [0, 2, 4], b, [0, 0, 5], [1, 1, 1, 1], [1, 1, 1, 1, 1])
    assert match.tolist() == [-1, -1, 0, 3]                                    # an empty target set: the empty result

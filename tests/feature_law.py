"""The descriptor law in numpy — the checker of csrc/features.hip, written from the law itself.

Fast point feature histograms (Rusu et al. 2009) over given neighbour lists, and the nearest descriptor of another set.
Everything is per scan (rows offsets[s] .. offsets[s+1] of points (T,3) float32 with normals (T,3) float32, n_s rows) and per
row i, given a list index (T,k) int32 of rows within the scan (knn_law's format, normals_law's slot rules), k <= 32.
Only IEEE + - * / sqrt, comparisons and floor / trunc are used: no library function decides a bit.

    usable     a row with finite coordinates and a finite normal that is not (0, 0, 0).  Normals are taken as given: unit
               length is the caller's (scan_normals' are), and consistently oriented ones are what makes descriptors comparable.
    listed     slot t of row i with 0 <= j = index[i,t] < n_s, j != i and row j usable; duplicates count as often as listed.
    d          = p_j - p_i per component, one float32 rounding; everything below is float64, one rounding per operation, in
               the association written; dot(a, b) = (a0*b0 + a1*b1) + a2*b2, cross(a, b)_0 = a1*b2 - a2*b1 and cyclic.
    pair       of a usable row i and a listed j, with d2 = dot(d, d).  Skipped if a component of d is not finite or d2 == 0.
               The source is the end whose normal makes the smaller angle with the line: j iff |dot(n_j, d)| > |dot(n_i, d)|,
               and then d is negated; (ns, nt) are the source's and the target's normal.
                   phi = dot(ns, d) / sqrt(d2);   v = cross(d, ns);  vn = sqrt(dot(v, v));  skipped if vn == 0;  v = v / vn;
                   w = cross(ns, v);   alpha = dot(v, nt);   y = dot(w, nt);   x = dot(ns, nt);   theta = the angle of (x, y).
    bins       alpha and phi: floor((11 * (f + 1)) / 2), clamped to [0, 10].  theta over (-pi, pi] in 11 equal bins, decided by
               sign tests against the ten boundary directions THETA[k] = (cos, sin)(-pi + 2 pi (k + 1) / 11), tabulated once:
               with cr_k = c_k * y - s_k * x, the bin is 5 + #{k in 5..9: cr_k >= 0} where y >= 0 (-0.0 counts as 0) and
               #{k in 0..4: cr_k >= 0} where y < 0; x == 0 and y == 0 is bin 5.
    SPFH(i)    33 counts — bin theta, 11 + bin alpha, 22 + bin phi of every pair that is not skipped — and m_i, their number:
               36 bytes [33 counts, m_i, 0, 0].  A row that is not usable has m_i = 0.
    FPFH(i)    for a row with m_i > 0: over the slots in list order whose j is listed, has m_j > 0 and whose d is finite with
               d2 != 0:  w_j = 1 / d2;  W = W + w_j;  c_j = w_j / m_j;  A_b = A_b + c_j * SPFH(j)_b.  Then
               F_b = SPFH(i)_b / m_i + A_b / W (the second term only where a slot took part).  Each group of 11 bins is
               scaled by its own sum taken in bin order: byte_b = trunc((255 * F_b) / sum).  Bytes 33..35 are 0.
    count      m_i; a row with count 0 has 36 zero bytes and no descriptor.

    match      per set s of two ragged descriptor sets: for every source row with count > 0 the target row of set s with
               tcount > 0 at the smallest squared distance over the 36 bytes, an exact integer <= 33 * 255**2 < 2**22; ties to
               the lower row.  Without a descriptor or without a candidate: match -1, dist -1.  A set that is empty, holds more
               than MAX_POINTS rows on either side or whose offsets are not 0 <= lo < hi <= rows gets that empty result too.
"""
import numpy as np

f32, f64 = np.float32, np.float64
BINS = 11
WIDTH = 36
MAX_K = 32
MAX_POINTS = 65536
THETA = tuple((float.fromhex(c), float.fromhex(s)) for c, s in (
    ("-0x1.aeb8c8764f0b9p-1", "-0x1.14cedf8bb580dp-1"),
    ("-0x1.a9628d9c712b4p-2", "-0x1.d1bb48eee2c14p-1"),
    ("0x1.2375f640f44dap-3", "-0x1.fac9e043842efp-1"),
    ("0x1.4f49e7f775887p-1", "-0x1.82f19bb3a28a1p-1"),
    ("0x1.eb42a9bcd5058p-1", "-0x1.207e7fd768dbcp-2"),
    ("0x1.eb42a9bcd5058p-1", "0x1.207e7fd768dbcp-2"),
    ("0x1.4f49e7f775887p-1", "0x1.82f19bb3a28a1p-1"),
    ("0x1.2375f640f44dap-3", "0x1.fac9e043842efp-1"),
    ("-0x1.a9628d9c712b1p-2", "0x1.d1bb48eee2c15p-1"),
    ("-0x1.aeb8c8764f0bbp-1", "0x1.14cedf8bb580ap-1")))


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def theta_bin(x, y):
    """The bin of the angle of (x, y), float64 arrays, by sign tests alone."""
    x, y = np.asarray(x, dtype=f64), np.asarray(y, dtype=f64)
    up = y >= 0
    cnt = np.zeros(x.shape, dtype=np.int64)
    for k, (c, s) in enumerate(THETA):
        cr = f64(c) * y - f64(s) * x
        cnt += ((up if k >= 5 else ~up) & (cr >= 0)).astype(np.int64)
    return np.where((x == 0) & (y == 0), 5, np.where(up, 5 + cnt, cnt))


def unit_bin(f):
    """The bin of a feature of [-1, 1]."""
    with np.errstate(invalid="ignore"):                             # a NaN belongs to a pair that is skipped: its bin is unread
        return np.nan_to_num(np.clip(np.floor((f64(BINS) * (f + f64(1))) / f64(2)), 0, BINS - 1)).astype(np.int64)


def pair_features(d32, ni, nj):
    """(ok, x, y, alpha, phi) of pairs: d32 (...,3) float32 = p_j - p_i, ni and nj (...,3) float64 usable normals."""
    assert d32.dtype == f32 and ni.dtype == f64 and nj.dtype == f64
    with np.errstate(all="ignore"):
        d = d32.astype(f64)
        d2 = dot(d, d)
        ok = np.isfinite(d32).all(axis=-1) & (d2 != 0)
        d = np.where(ok[..., None], d, f64(1))                      # a skipped pair computes on, unread
        d2 = np.where(ok, d2, f64(3))
        swap = np.abs(dot(nj, d)) > np.abs(dot(ni, d))
        ns, nt = np.where(swap[..., None], nj, ni), np.where(swap[..., None], ni, nj)
        d = np.where(swap[..., None], -d, d)
        phi = dot(ns, d) / np.sqrt(d2)
        v = cross(d, ns)
        vn = np.sqrt(dot(v, v))
        ok = ok & (vn != 0)
        v = v / np.where(ok, vn, f64(1))[..., None]
        w = cross(ns, v)
        return ok, dot(ns, nt), dot(w, nt), dot(v, nt), phi


def pair_bins(d32, ni, nj):
    """(ok, bin theta, bin alpha, bin phi) of pairs."""
    ok, x, y, alpha, phi = pair_features(d32, ni, nj)
    return ok, theta_bin(x, y), unit_bin(alpha), unit_bin(phi)


def usable(cloud, normals):
    return np.isfinite(cloud).all(axis=1) & np.isfinite(normals).all(axis=1) & (normals != 0).any(axis=1)


def _listed(cloud, normals, index):
    n = len(cloud)
    good = usable(cloud, normals)
    inr = (index >= 0) & (index < n)
    safe = np.where(inr, index, 0)
    listed = inr & (safe != np.arange(n)[:, None]) & good[safe] & good[:, None]
    with np.errstate(all="ignore"):
        d32 = cloud[safe] - cloud[:, None, :]
    assert d32.dtype == f32
    return listed, safe, d32


def spfh_scan(cloud, normals, index):
    """(n,36) uint8 of one scan: 33 counts, m, 0, 0."""
    n, k = index.shape
    assert k <= MAX_K
    out = np.zeros((n, WIDTH), dtype=np.uint8)
    if n == 0:
        return out
    listed, safe, d32 = _listed(cloud, normals, index)
    nrm = normals.astype(f64)
    hist = np.zeros((n, 3 * BINS + 1), dtype=np.int64)
    rows = np.arange(n)
    for t in range(k):
        ok, bt, ba, bp = pair_bins(d32[:, t], nrm, nrm[safe[:, t]])
        ok = ok & listed[:, t]
        r = rows[ok]
        np.add.at(hist, (r, bt[ok]), 1)
        np.add.at(hist, (r, BINS + ba[ok]), 1)
        np.add.at(hist, (r, 2 * BINS + bp[ok]), 1)
        hist[r, 3 * BINS] += 1
    out[:, :3 * BINS + 1] = hist
    return out


def fpfh_scan(cloud, index, spfh):
    """(features (n,36) uint8, count (n) int32) of one scan from its SPFH records."""
    n, k = index.shape
    feat, count = np.zeros((n, WIDTH), dtype=np.uint8), spfh[:, 3 * BINS].astype(np.int32)
    if n == 0:
        return feat, count
    m = spfh[:, 3 * BINS].astype(f64)
    inr = (index >= 0) & (index < n)
    safe = np.where(inr, index, 0)
    with np.errstate(all="ignore"):
        d32 = cloud[safe] - cloud[:, None, :]
        d = d32.astype(f64)
        d2 = dot(d, d)
    take = inr & (safe != np.arange(n)[:, None]) & (m[safe] > 0) & (m[:, None] > 0) & np.isfinite(d32).all(axis=-1) & (d2 != 0)
    S = spfh[:, :3 * BINS].astype(f64)
    A, W = np.zeros((n, 3 * BINS), dtype=f64), np.zeros(n, dtype=f64)
    with np.errstate(all="ignore"):
        for t in range(k):
            on = take[:, t]
            w = f64(1) / np.where(on, d2[:, t], f64(1))
            c = w / np.where(on, m[safe[:, t]], f64(1))
            W = np.where(on, W + w, W)
            A = np.where(on[:, None], A + c[:, None] * S[safe[:, t]], A)
        have = m > 0
        F = S / np.where(have, m, f64(1))[:, None]
        F = np.where((W > 0)[:, None], F + A / np.where(W > 0, W, f64(1))[:, None], F)
        for g in range(3):
            G = F[:, g * BINS:(g + 1) * BINS]
            tot = G[:, 0].copy()
            for b in range(1, BINS):
                tot = tot + G[:, b]
            byte = np.trunc((f64(255) * G) / np.where(have, tot, f64(1))[:, None])
            feat[:, g * BINS:(g + 1) * BINS] = np.where(have[:, None], byte, 0).astype(np.uint8)
    return feat, count


def feature_law(points, offsets, normals, index):
    """(features (T,36) uint8, count (T) int32, spfh (T,36) uint8) over a ragged set."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    normals = np.ascontiguousarray(np.asarray(normals, dtype=f32)).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    index = np.asarray(index, dtype=np.int32).reshape(len(points), -1)
    T = len(points)
    feat, count, spfh = np.zeros((T, WIDTH), np.uint8), np.zeros(T, np.int32), np.zeros((T, WIDTH), np.uint8)
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        spfh[lo:hi] = spfh_scan(points[lo:hi], normals[lo:hi], index[lo:hi])
        feat[lo:hi], count[lo:hi] = fpfh_scan(points[lo:hi], index[lo:hi], spfh[lo:hi])
    return feat, count, spfh


def _valid_set(offsets, s, rows):
    lo, hi = int(offsets[s]), int(offsets[s + 1])
    return 0 <= lo < hi <= rows and hi - lo <= MAX_POINTS


def match_law(features, offsets, tfeatures, toffsets, counts, tcounts, block=64):
    """(match (T) int32, dist (T) int32): the nearest target descriptor of every source row."""
    features, tfeatures = np.asarray(features, dtype=np.uint8), np.asarray(tfeatures, dtype=np.uint8)
    offsets, toffsets = np.asarray(offsets, dtype=np.int64), np.asarray(toffsets, dtype=np.int64)
    counts, tcounts = np.asarray(counts), np.asarray(tcounts)
    T, U = len(features), len(tfeatures)
    match, dist = np.full(T, -1, dtype=np.int32), np.full(T, -1, dtype=np.int32)
    for s in range(len(offsets) - 1):
        if not (_valid_set(offsets, s, T) and _valid_set(toffsets, s, U)):
            continue
        lo, hi, tlo, thi = int(offsets[s]), int(offsets[s + 1]), int(toffsets[s]), int(toffsets[s + 1])
        cand = np.flatnonzero(tcounts[tlo:thi] > 0)
        if len(cand) == 0:
            continue
        b = tfeatures[tlo:thi][cand].astype(np.int64)
        for i0 in range(lo, hi, block):
            a = features[i0:min(i0 + block, hi)].astype(np.int64)
            d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
            j = np.argmin(d, axis=1)                                # the first of equals: the lower row
            have = counts[i0:i0 + len(a)] > 0
            match[i0:i0 + len(a)] = np.where(have, cand[j], -1)
            dist[i0:i0 + len(a)] = np.where(have, d[np.arange(len(a)), j], -1)
    return match, dist


def reference_bins(d32, ni, nj):
    """What the law approximates — the same pair features with numpy's own dot / cross / atan2 in float64, for the
    comparison of the host suite: (ok, theta, alpha, phi) as real numbers."""
    d = d32.astype(f64)
    ln = np.linalg.norm(d, axis=-1)
    swap = np.abs((nj * d).sum(-1)) > np.abs((ni * d).sum(-1))
    ns, nt = np.where(swap[..., None], nj, ni), np.where(swap[..., None], ni, nj)
    d = np.where(swap[..., None], -d, d)
    v = np.cross(d, ns)
    vn = np.linalg.norm(v, axis=-1)
    ok = (ln > 0) & (vn > 0)
    v = v / vn[..., None]
    w = np.cross(ns, v)
    return ok, np.arctan2((w * nt).sum(-1), (ns * nt).sum(-1)), (v * nt).sum(-1), (ns * d).sum(-1) / ln


# ---- fixtures of the suites, not of the law -------------------------------------------------------------------------------


def bumpy_sheet(rows=800, seed=0, noise=0.002, degrees=140.0, axis=(1.0, 2.0, 3.0), shift=(0.3, -0.2, 0.5)):
    """(source, target (rows,3) float32, R (3,3), t (3)): a bumpy sheet z = f(x, y) over [-1, 1]^2 sampled twice independently
    with Gaussian noise; the source is its second sampling moved by the inverse of (R, t), a turn of `degrees` about `axis`
    and a shift — so (R, t) takes the source onto the target.  Both sets are seen from above: the sensor of the target stands
    at (0, 0, 5), the source's at R^T ((0, 0, 5) - t)."""
    r = np.random.RandomState(seed)

    def sample():
        x, y = r.uniform(-1, 1, (2, rows))
        z = 0.25 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.15 * np.sin(3.3 * x * y + 1.0) + 0.2 * x * x - 0.1 * y
        return np.stack([x, y, z], axis=1) + noise * r.normal(size=(rows, 3))

    target, second = sample(), sample()
    k = np.asarray(axis, dtype=f64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    a = np.radians(degrees)
    R = np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)
    t = np.asarray(shift, dtype=f64)
    source = (second - t) @ R
    return source.astype(f32), target.astype(f32), R, t


def sheet_viewpoints(R, t, height=5.0):
    """(source viewpoint, target viewpoint) float32 of bumpy_sheet."""
    up = np.array([0.0, 0.0, height])
    return ((up - t) @ R).astype(f32), up.astype(f32)


def sheet_views(rows=1500, seed=0, cut=0.7, noise=0.002, degrees=140.0, axis=(1.0, 2.0, 3.0)):
    """(view 0, view 1 float32, R, t): two captures of bumpy_sheet's surface, each in the frame of its own sensor (the sensor
    at the origin).  View 0 is the part with x < cut of one sampling, seen from (0, 0, 3); view 1 the part with x > -cut of
    an independent one, seen from (0.5, 0.3, 3) by a sensor turned `degrees` about `axis`: (R, t) takes view 1 onto view 0."""
    _, first, R, _ = bumpy_sheet(rows, seed, noise, degrees, axis)
    _, second, _, _ = bumpy_sheet(rows, seed + 1000, noise, degrees, axis)
    c0, c1 = np.array([0.0, 0.0, 3.0]), np.array([0.5, 0.3, 3.0])
    view0 = first[first[:, 0] < cut].astype(f64) - c0
    view1 = (second[second[:, 0] > -cut].astype(f64) - c1) @ R
    return view0.astype(f32), view1.astype(f32), R, c1 - c0

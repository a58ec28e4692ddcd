"""The visibility law in numpy — the checker of csrc/visibility.hip, written from the law itself.

Everything is per scan (rows offsets[s] .. offsets[s+1] of points (T,3) float32) and its viewpoint v (3) float32; rows of other
scans never take part.  Every operation below is one float64 rounding in the association written; no library function decides
a bit (floor of a float64 is exact).

    parameters  resolution R, 4 <= R <= 1024 pixels per edge of a cube face; window w, 0 <= w <= 4; margin >= 0 in scan units;
                slope >= 0, which enters as pitch = 2 * slope / R, computed once in float64.
    project     d = float64(p) - float64(v) per component, a = |d|; the major axis m is the largest a, ties to the lowest axis;
                face = 2 m + (d_m < 0); u = d[(m+1) % 3] / a_m, t = d[(m+2) % 3] / a_m; iu = min(R - 1, int(floor((u + 1.0) *
                (0.5 * R)))), `it` likewise from t; the depth z = float32(a_m), round to nearest even, +inf where it overflows.
    absent      a row with a non-finite coordinate, or of a scan whose viewpoint has one: no pixel, label 4, winner 0.
    at v        a row with a_m == 0: no pixel, label 1, winner 0.
    buffer      one uint64 key per pixel, laid out (scan, face, it, iu): (the uint32 bits of z) << 32 | row within the scan; an
                empty pixel holds all ones; a pixel holds the smallest key of the rows that project to it.
    classify    a query q — a row of the scan, or of a second ragged set over the same scans — has its pixel (face, it, iu) and
                its depth z0 = float64(z).  Over the pixels (it + dy, iu + dx) of that face with |dx|, |dy| <= w that lie inside
                the face and are not empty: zz = float64(the pixel's depth), c = max(|dx|, |dy|) + 1,
                tol = margin + (z0 * pitch) * c.
                  3  unobserved     no such pixel
                  2  hidden         else, some pixel has zz + tol < z0
                  0  seen through   else, every pixel has zz - tol > z0
                  1  on the surface otherwise
    winner      for a scan's own rows: 1 iff the row's key is the key its pixel holds.
    A scan longer than MAX_POINTS writes no pixel; its rows and its queries are labelled 4.
"""
import numpy as np

MAX_POINTS = 1 << 22
MIN_RESOLUTION, MAX_RESOLUTION, MAX_WINDOW = 4, 1024, 4
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SEEN_THROUGH, ON_SURFACE, HIDDEN, UNOBSERVED, ABSENT = 0, 1, 2, 3, 4
f32, f64 = np.float32, np.float64


def pitch_of(slope, R):
    return 2.0 * float(slope) / int(R)


def project(cloud, view, R):
    """One set of rows against one viewpoint -> (kind (n) int: 0 absent, 1 at the viewpoint, 2 projected; pixel (n) int64
    within the scan's 6 R^2 pixels, 0 where not projected; zbits (n) uint32)."""
    cloud = np.ascontiguousarray(np.asarray(cloud, dtype=f32)).reshape(-1, 3)
    view = np.asarray(view, dtype=f32).reshape(3)
    n = len(cloud)
    finite = np.isfinite(cloud).all(axis=1) & bool(np.isfinite(view).all())
    with np.errstate(all="ignore"):
        d = np.where(finite[:, None], cloud.astype(f64) - view.astype(f64), 1.0)     # absent rows: any finite stand-in
        a = np.abs(d)
        m = np.argmax(a, axis=1)                                   # the first of equal maxima: the lowest axis
        rows = np.arange(n)
        am, dm = a[rows, m], d[rows, m]
        there = finite & (am > 0)
        am_safe = np.where(there, am, 1.0)
        u = d[rows, (m + 1) % 3] / am_safe
        t = d[rows, (m + 2) % 3] / am_safe
        half = 0.5 * R
        iu = np.minimum(R - 1, np.floor((u + 1.0) * half).astype(np.int64))
        it = np.minimum(R - 1, np.floor((t + 1.0) * half).astype(np.int64))
        z = am.astype(f32)
    assert d.dtype == f64 and u.dtype == f64 and z.dtype == f32
    face = 2 * m + (dm < 0)
    pixel = np.where(there, (face * R + it) * R + iu, 0).astype(np.int64)
    kind = np.where(there, 2, np.where(finite, 1, 0))
    return kind, pixel, z.view(np.uint32)


def scatter(cloud, view, R):
    """The buffer (6 R^2) uint64 of one scan and what project() gave for its rows."""
    kind, pixel, zbits = project(cloud, view, R)
    buf = np.full(6 * R * R, EMPTY, dtype=np.uint64)
    n = len(kind)
    if n > MAX_POINTS:
        return buf, kind, pixel, zbits
    rows = np.flatnonzero(kind == 2)
    key = (zbits[rows].astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    np.minimum.at(buf, pixel[rows], key)
    return buf, kind, pixel, zbits


def classify(buf, kind, pixel, zbits, R, w, margin, pitch):
    """Labels (n) uint8 of projected queries against one scan's buffer."""
    n = len(kind)
    margin, pitch = f64(margin), f64(pitch)
    iu, it, face = pixel % R, (pixel // R) % R, pixel // (R * R)
    z0 = zbits.view(f32).astype(f64)
    any_pixel = np.zeros(n, bool)
    hidden = np.zeros(n, bool)
    all_behind = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for dy in range(-w, w + 1):
            for dx in range(-w, w + 1):
                y, x = it + dy, iu + dx
                inside = (y >= 0) & (y < R) & (x >= 0) & (x < R)
                k = buf[np.where(inside, (face * R + y) * R + x, 0)]
                full = inside & (k != EMPTY)
                zz = (k >> np.uint64(32)).astype(np.uint32).view(f32).astype(f64)
                tol = margin + (z0 * pitch) * f64(max(abs(dx), abs(dy)) + 1)
                any_pixel |= full
                hidden |= full & (zz + tol < z0)
                all_behind &= ~full | (zz - tol > z0)
    label = np.where(~any_pixel, UNOBSERVED, np.where(hidden, HIDDEN, np.where(all_behind, SEEN_THROUGH, ON_SURFACE)))
    label = np.where(kind == 2, label, np.where(kind == 1, ON_SURFACE, ABSENT))
    return label.astype(np.uint8)


def check_parameters(R, w, margin, slope):
    assert MIN_RESOLUTION <= R <= MAX_RESOLUTION and 0 <= w <= MAX_WINDOW and margin >= 0 and slope >= 0


def visibility_scan(cloud, view, R=32, w=1, margin=0.01, slope=2.0, queries=None):
    """One scan -> dict(label (n or q) uint8, winner (n) uint8 — without queries —, buffer (6 R^2) uint64)."""
    check_parameters(R, w, margin, slope)
    buf, kind, pixel, zbits = scatter(cloud, view, R)
    too_long = len(kind) > MAX_POINTS
    res = {"buffer": buf}
    if queries is None:
        key = (zbits.astype(np.uint64) << np.uint64(32)) | np.arange(len(kind), dtype=np.uint64)
        res["winner"] = ((kind == 2) & (buf[pixel] == key) & (not too_long)).astype(np.uint8)
    else:
        kind, pixel, zbits = project(queries, view, R)
    res["label"] = classify(buf, kind, pixel, zbits, R, w, margin, pitch_of(slope, R))
    if too_long:
        res["label"][:] = ABSENT
    return res


def visibility_law(points, offsets, viewpoints, R=32, w=1, margin=0.01, slope=2.0, queries=None, query_offsets=None):
    """The ragged set -> dict(label (T or Q) uint8, winner (T) uint8 — without queries —, buffer (S, 6, R, R) uint64).
    viewpoints: one triple or (S,3)."""
    points = np.ascontiguousarray(np.asarray(points, dtype=f32)).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    S = len(offsets) - 1
    views = np.broadcast_to(np.asarray(viewpoints, dtype=f32).reshape(-1, 3), (S, 3))
    own = queries is None
    if not own:
        queries = np.ascontiguousarray(np.asarray(queries, dtype=f32)).reshape(-1, 3)
        query_offsets = np.asarray(query_offsets, dtype=np.int64)
    out = {"label": np.zeros(len(points) if own else len(queries), np.uint8), "buffer": np.zeros((S, 6, R, R), np.uint64)}
    if own:
        out["winner"] = np.zeros(len(points), np.uint8)
    for s in range(S):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        if own:
            r = visibility_scan(points[lo:hi], views[s], R, w, margin, slope)
            out["winner"][lo:hi] = r["winner"]
            out["label"][lo:hi] = r["label"]
        else:
            qlo, qhi = int(query_offsets[s]), int(query_offsets[s + 1])
            r = visibility_scan(points[lo:hi], views[s], R, w, margin, slope, queries[qlo:qhi])
            out["label"][qlo:qhi] = r["label"]
        out["buffer"][s] = r["buffer"].reshape(6, R, R)
    return out


def shell(n, seed=0, radius=1.0):
    """A fixture of the suites, not of the law: n rows on the sphere of `radius`, normalised normals of default_rng(seed)."""
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True) * radius).astype(f32)


SHELL_VIEW = np.array([1.5, 2.0, 1.0], dtype=f32)

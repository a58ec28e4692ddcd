"""GPU: hp_make_batch / ops.make_batch (csrc/batch_maker.hip) — one chip-wide call that cuts a training batch out of a
device-resident dataset: the reference's random-plane law (datasets/utils/dataset_generator.py:6-39) with a candidate
sequence keyed by (seed, stream id), the first accepted candidate whatever the number of workgroups, the z-rotation of
datasets/shapenet.py:73-92 applied while writing, and failure as a value.

Shapes (N, target, B): (64, 32, 8) and (100, 37, 8) — the smallest where chunk interleaving, early exit, a ragged last wave
and an uneven target all run — (2048, 1024, 8), the workload's, and (8192, 4096, 2), the LDS staging path.  Clouds are seeded
uniform draws from the cube of half-width 0.5: inside the unit ball, which the bounds below assume."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 2024
SMALL = [(64, 32), (100, 37)]
SHAPES = {(64, 32): 8, (100, 37): 8, (2048, 1024): 8, (8192, 4096): 2}
GROUPS = (1, 3, 16)
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatement of the candidate sequence: Philox4x32-10, counter (stream_lo, stream_hi, c, k), key = seed, uniforms
# (x >> 8) * 2^-24 (exact in fp64), the plane of dataset_generator.py:13-20 in fp64
# ---------------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) for x in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def candidate_planes(seed, stream, cs):
    """(len(cs), 4) float64: normal and bias of candidates `cs` of the sequence (seed, stream)."""
    cs = np.asarray(cs, np.uint64)
    seed, stream = int(seed) & (2 ** 64 - 1), int(stream) & (2 ** 64 - 1)
    pts = []
    for k in range(3):
        r = philox4x32_10(np.full_like(cs, stream & 0xFFFFFFFF), np.full_like(cs, stream >> 32), cs, np.full_like(cs, k),
                          seed & 0xFFFFFFFF, seed >> 32)
        pts.append(np.stack([(x >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 for x in r[:3]], 1))
    normal = np.cross(pts[1] - pts[0], pts[2] - pts[0])
    return np.concatenate([normal, (normal * pts[0]).sum(1, keepdims=True)], 1)


def restated_search(cloud, target, seed, stream, limit):
    """First candidate below `limit` whose fp64 counts accept unambiguously, and how many candidates before it are
    ambiguous (a point within 1e-5 of the plane) -> (index or -1, ambiguous candidates before it)."""
    pl = candidate_planes(seed, stream, np.arange(limit))
    v = cloud.astype(np.float64) @ pl[:, :3].T + pl[:, 3]            # (N, limit)
    lo, hi = (v > 1e-5).sum(0), (v > -1e-5).sum(0)
    n = cloud.shape[0]
    clear = lo == hi
    accept = clear & ((lo == target) | (n - lo == target))
    first = int(np.argmax(accept)) if accept.any() else -1
    upto = first if first >= 0 else limit
    return first, int((~clear[:upto]).sum())


def make_clouds(n_clouds, n, seed):
    return (np.random.RandomState(seed).rand(n_clouds, n, 3).astype(np.float32) - 0.5)


def split_of(gt, ex, mi):
    """Membership mask of the order-preserving partition gt -> (ex, mi); asserts that it is one."""
    n, i, j = gt.shape[0], 0, 0
    mask = np.zeros(n, bool)
    g, e, m = (np.ascontiguousarray(a).view(np.uint32) for a in (gt, ex, mi))
    for r in range(n):
        if i < e.shape[0] and np.array_equal(g[r], e[i]):
            mask[r], i = True, i + 1
        else:
            assert j < m.shape[0] and np.array_equal(g[r], m[j]), f"row {r} of gt is the next row of neither part"
            j += 1
    assert i == e.shape[0] and j == m.shape[0]
    return mask


def run(clouds, ids, streams, target, **kw):
    from hyperpocket_amd import ops
    dev = "cuda"
    C = clouds if torch.is_tensor(clouds) else torch.from_numpy(clouds).to(dev)
    deg = kw.pop("degrees", None)
    out = ops.make_batch(C, torch.tensor(ids, dtype=torch.int32, device=dev), torch.tensor(streams, dtype=torch.int64, device=dev),
                         target, degrees=None if deg is None else torch.tensor(deg, dtype=torch.int32, device=dev), **kw)
    names = ("existing", "missing", "gt", "plane", "index", "failed")
    return {k: v.cpu().numpy() for k, v in zip(names, out)}


def same(a, b, keys=("existing", "missing", "gt", "plane", "index")):
    return all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in keys)


def items_of(shape):
    """The B items of a shape: cloud numbers (one repeated) and stream ids (not their positions)."""
    B = SHAPES[shape]
    ids = [(3 * b + 1) % 10 for b in range(B)]
    streams = [1000 * shape[0] + 17 * b + 5 for b in range(B)]
    return ids, streams


@pytest.fixture(scope="module")
def runs():
    """Every shape once (default groups) and the small shapes at each of GROUPS — computed once, left unchanged."""
    out = {}
    for shape in SHAPES:
        n, target = shape
        clouds = make_clouds(10, n, seed=n)
        ids, streams = items_of(shape)
        out[shape] = (clouds, ids, streams, run(clouds, ids, streams, target, seed=SEED))
        if shape in SMALL:
            for g in GROUPS:
                out[shape, g] = run(clouds, ids, streams, target, seed=SEED, groups=g)
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_exact_ordered_partition(runs, shape):
    (n, target), B = shape, SHAPES[shape]
    clouds, ids, _, r = runs[shape]
    assert r["existing"].shape == (B, target, 3) and r["missing"].shape == (B, n - target, 3) and r["gt"].shape == (B, n, 3)
    assert np.array_equal(r["gt"].view(np.uint32), clouds[ids].view(np.uint32))
    assert (r["index"] >= 0).all() and r["failed"][0] == 0
    for b in range(B):
        mask = split_of(r["gt"][b], r["existing"][b], r["missing"][b])
        assert mask.sum() == target


@pytest.mark.parametrize("shape", list(SHAPES))
def test_parts_are_separated_by_the_returned_plane(runs, shape):
    """fp64 value of the returned fp32 plane at the fp32 points: one part on each side, except points with |value| <= 1e-5
    (a cross-product component is off by <= 4 * 2^-24 * 2, bias and dot add a few 2^-24 terms of magnitude <= 3: below 5e-6
    in the unit ball; 1e-5 is twice that)."""
    _, _, _, r = runs[shape]
    for b in range(SHAPES[shape]):
        mask = split_of(r["gt"][b], r["existing"][b], r["missing"][b])
        pl = r["plane"][b].astype(np.float64)
        v = r["gt"][b].astype(np.float64) @ pl[:3] + pl[3]
        above = (v[mask] > -1e-5).all() and (v[~mask] < 1e-5).all()
        below = (v[mask] < 1e-5).all() and (v[~mask] > -1e-5).all()
        assert above or below, b
        assert np.abs(v).max() > 1e-5


@pytest.mark.parametrize("shape", SMALL)
def test_result_does_not_depend_on_groups(runs, shape):
    base = runs[shape, GROUPS[0]]
    for g in GROUPS[1:]:
        assert same(base, runs[shape, g]), g
    assert same(base, runs[shape][3])


def test_it_is_the_first_accepted_candidate_of_the_restated_sequence(runs):
    """The numpy restatement above must give the returned plane (5e-6 per coefficient: pins the counter layout and the
    formula), and no candidate below the returned index may accept.  A candidate with a point within 1e-5 of its plane is
    ambiguous and skipped; at most 2 % of the candidates checked may be."""
    checked = skipped = 0
    for shape in SMALL:
        n, target = shape
        clouds, ids, streams, r = runs[shape]
        for b in range(SHAPES[shape]):
            idx = int(r["index"][b])
            pl = candidate_planes(SEED, streams[b], np.arange(idx + 1))
            assert np.abs(pl[idx] - r["plane"][b].astype(np.float64)).max() <= 5e-6, (shape, b)
            v = clouds[ids[b]].astype(np.float64) @ pl[:idx, :3].T + pl[:idx, 3]
            lo, hi = (v > 1e-5).sum(0), (v > -1e-5).sum(0)
            clear = lo == hi
            assert not (clear & ((lo == target) | (n - lo == target))).any(), (shape, b, np.nonzero(clear & ((lo == target) | (n - lo == target))))
            checked += idx
            skipped += int((~clear).sum())
    assert checked > 100
    assert skipped <= 0.02 * checked, (skipped, checked)


def test_keyed_by_stream_not_by_position():
    n, target = 64, 32
    clouds = make_clouds(10, n, seed=n)
    alone = run(clouds, [3], [77], target, seed=SEED)
    ids, streams = [5, 1, 3, 3, 8, 3, 0, 2], [11, 12, 78, 13, 14, 77, 15, 16]
    batch = run(clouds, ids, streams, target, seed=SEED)
    other = run(clouds, [3, 9], [77, 4], target, seed=SEED)
    for r, pos in ((batch, 5), (other, 0)):
        one = {k: r[k][pos:pos + 1] for k in ("existing", "missing", "gt", "plane", "index")}
        assert same(alone, one), pos
    # the same cloud under other streams / another seed: other planes
    assert not np.array_equal(batch["plane"][2], batch["plane"][5]) and not np.array_equal(batch["plane"][3], batch["plane"][5])
    reseeded = run(clouds, [3], [77], target, seed=SEED + 1)
    assert not np.array_equal(reseeded["plane"], alone["plane"])


def test_rotation_table_is_scipys():
    from hyperpocket_amd import ops
    tab = ops.rotation_table().numpy()
    assert tab.shape == (360, 2) and tab.dtype == np.float32
    try:
        from scipy.spatial.transform import Rotation
        m = np.stack([Rotation.from_euler("z", d, degrees=True).as_matrix().astype(np.float32) for d in range(360)])
        want = np.stack([m[:, 0, 0], m[:, 1, 0]], 1)
        assert np.array_equal(m[:, 1, 1], m[:, 0, 0]) and np.array_equal(m[:, 0, 1], -m[:, 1, 0])
    except ImportError:
        h = np.deg2rad(np.arange(360, dtype=np.float64)) / 2          # closed form, through the half angle as scipy's quaternion
        want = np.stack([np.cos(h) ** 2 - np.sin(h) ** 2, 2 * np.sin(h) * np.cos(h)], 1).astype(np.float32)
    assert np.array_equal(tab, want)
    assert tab[0, 0] == 1.0 and tab[0, 1] == 0.0


@pytest.mark.parametrize("shape", [(100, 37), (2048, 1024)])
def test_rotation(runs, shape):
    n, target = shape
    clouds, ids, streams, plain = runs[shape]
    B = SHAPES[shape]
    zero = run(clouds, ids, streams, target, seed=SEED, degrees=[0] * B)
    assert same(plain, zero)
    degs = [1, 90, 137, 359] * (B // 4)
    r = run(clouds, ids, streams, target, seed=SEED, degrees=degs)
    assert np.array_equal(r["index"], plain["index"]) and np.array_equal(r["plane"], plain["plane"])
    for b in range(B):
        a = np.deg2rad(np.float64(degs[b]))
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])       # from_euler('z', deg).as_matrix()
        want = clouds[ids[b]].astype(np.float64) @ R
        # three fp32 roundings on terms bounded by 1 in the unit ball, plus the table's own rounding
        assert np.abs(r["gt"][b].astype(np.float64) - want).max() <= 4e-7, b
        mask = split_of(r["gt"][b], r["existing"][b], r["missing"][b])
        assert np.array_equal(mask, split_of(plain["gt"][b], plain["existing"][b], plain["missing"][b])), b


def test_failure_is_a_value():
    """A cloud of N identical points lies on one side of every plane: it cannot split.  index -1, the counter rises by the
    number of such items (added to what it held), the fallback is first-target / rest, the other items are untouched."""
    from hyperpocket_amd import ops
    n, target, limit = 64, 32, 64
    clouds = make_clouds(10, n, seed=n)
    clouds[2] = np.float32([0.25, -0.125, 0.375])
    # the healthy items must accept below `limit`: take streams whose restated sequence does, with nothing ambiguous before
    healthy = []
    stream = 0
    while len(healthy) < 6:
        cloud = 1 + len(healthy)            # clouds 1, 3..7 (2 is the degenerate one)
        cloud += cloud >= 2
        first, ambiguous = restated_search(clouds[cloud], target, SEED, stream, limit)
        if 0 <= first < limit - 8 and ambiguous == 0:
            healthy.append((cloud, stream))
        stream += 1
        assert stream < 4000
    ids = [healthy[0][0], 2, healthy[1][0], healthy[2][0], 2, healthy[3][0], healthy[4][0], healthy[5][0]]
    streams = [healthy[0][1], 900, healthy[1][1], healthy[2][1], 901, healthy[3][1], healthy[4][1], healthy[5][1]]
    failed = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    r = run(clouds, ids, streams, target, seed=SEED, max_candidates=limit, failed=failed)     # returned: the call itself is fine
    assert r["failed"][0] == 5 + 2 and int(failed.item()) == 7
    assert r["index"].tolist()[1] == -1 and r["index"].tolist()[4] == -1
    good = [b for b in range(8) if b not in (1, 4)]
    assert (r["index"][good] >= 0).all() and (r["index"][good] < limit).all()
    for b in (1, 4):
        assert np.array_equal(r["gt"][b], clouds[2])
        assert np.array_equal(r["existing"][b], clouds[2][:target]) and np.array_equal(r["missing"][b], clouds[2][target:])
        assert not r["plane"][b].any()
    clean = run(clouds, [ids[b] for b in good], [streams[b] for b in good], target, seed=SEED, max_candidates=limit)
    assert clean["failed"][0] == 0
    assert same({k: r[k][good] for k in ("existing", "missing", "gt", "plane", "index")}, clean)
    for b, (cloud, s) in zip(good, healthy):
        assert int(r["index"][b]) == restated_search(clouds[cloud], target, SEED, s, limit)[0]
    # the fallback is rotated like everything else
    rot = run(clouds, [2], [900], target, seed=SEED, max_candidates=limit, degrees=[90])
    assert rot["index"][0] == -1
    assert np.abs(rot["gt"][0] - np.float32([-0.125, -0.25, 0.375])).max() <= 4e-7
    assert np.array_equal(rot["existing"][0], rot["gt"][0][:target]) and np.array_equal(rot["missing"][0], rot["gt"][0][target:])


def test_invalid_arguments_return_minus_one():
    from hyperpocket_amd import ops
    lib = ops.load_library()
    lib.hp_make_batch_workspace_bytes.restype = ctypes.c_long
    dev, B, M = "cuda", 2, 3
    buf = {"N": 64, "target": 32, "B": B, "groups": 4}

    def rc(**kw):
        a = dict(buf, **kw)
        n_alloc, b_alloc = 64, max(1, min(abs(a["B"]), 4))
        clouds = torch.zeros((M, n_alloc, 3), device=dev)
        ids = torch.zeros((b_alloc,), dtype=torch.int32, device=dev)
        streams = torch.zeros((b_alloc,), dtype=torch.int64, device=dev)
        f = [torch.zeros((b_alloc, n_alloc, 3), device=dev) for _ in range(3)]
        plane, index = torch.zeros((b_alloc, 4), device=dev), torch.zeros((b_alloc,), dtype=torch.int32, device=dev)
        failed, ws = torch.zeros((1,), dtype=torch.int32, device=dev), torch.zeros((1024,), dtype=torch.uint8, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        out = lib.hp_make_batch(M, a["N"], a["target"], p(clouds), a["B"], p(ids), p(streams), None, None, ctypes.c_ulonglong(1),
                                100, a["groups"], p(f[0]), p(f[1]), p(f[2]), p(plane), p(index), p(failed), p(ws), None)
        torch.cuda.synchronize()
        return out

    assert rc() == 0
    assert rc(target=64) == -1 and rc(target=65) == -1 and rc(target=0) == -1
    assert rc(N=8193, target=4096) == -1
    assert rc(B=0) == -1 and rc(B=-1) == -1
    assert rc(groups=0) == -1 and rc(groups=-3) == -1
    assert lib.hp_make_batch_workspace_bytes(64, 2048) >= 64 * 4
    assert lib.hp_make_batch_workspace_bytes(0, 2048) == -1 and lib.hp_make_batch_workspace_bytes(1, 8193) == -1
    with pytest.raises(ops.HipExtensionError):
        run(make_clouds(2, 64, 1), [0], [0], 64)

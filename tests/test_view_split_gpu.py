"""GPU: ops.make_view_batch (csrc/view_split.hip) against its numpy law (tests/view_split_law.py), bit for bit — existing, missing,
gt, side and occlusion — over the sizes at which the kernel takes another path (one row more or less than a wave, than the 512
rows of a sweep, than the LDS attribute's threshold), the smallest and largest images and windows, and the law's corner cases."""
import numpy as np
import pytest
import torch

import view_split_law as law

pytestmark = pytest.mark.gpu

DIST = 3.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run(clouds, ids, frames, target, R=32, w=1, h=None, degrees=None, out=None, dist=DIST):
    """One call -> dict of host arrays (side / occlusion None where `out` leaves them out)."""
    from hyperpocket_amd import ops
    dev = torch.device("cuda")
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    h = ops.view_half_extent(0.5, dist) if h is None else h
    got = ops.make_view_batch(t(clouds, torch.float32), t(ids, torch.int32), t(frames, torch.float32), target,
                              None if degrees is None else t(degrees, torch.int32), None, dist, h, R, w, out=out)
    return {k: None if v is None else v.cpu().numpy() for k, v in zip(("existing", "missing", "gt", "side", "occlusion"), got)}


def expect(clouds, ids, frames, target, R=32, w=1, h=None, dist=DIST):
    from hyperpocket_amd import ops
    h = ops.view_half_extent(0.5, dist) if h is None else h
    items = [law.view_split(clouds[i], f, dist, law.scale_of(R, h), R, w, target) for i, f in zip(ids, frames)]
    return {k: np.stack([it[k] for it in items]) for k in ("existing", "missing", "gt", "side", "occlusion")}


def assert_same(got, want, keys=("existing", "missing", "gt", "side", "occlusion"), what=""):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist())


def cube(m, n, seed):
    return (np.random.default_rng(seed).random((m, n, 3), dtype=np.float32) - np.float32(0.5))


def frames_of(count, seed):
    from hyperpocket_amd import ops
    return ops.view_frames(count, seed).numpy()


def target_of(n, kind):
    return {"one": 1, "half": max(1, n // 2), "all-but-one": n - 1}[kind]


# a sparse cross of N x R x w x target: every value of each list below appears, and every N next to a path's edge
CROSS = [(2, 4, 0, "one"), (2, 5, 1, "one"), (63, 5, 1, "half"), (64, 32, 4, "all-but-one"), (65, 4, 0, "one"),
         (255, 128, 1, "half"), (256, 5, 4, "one"), (257, 32, 0, "all-but-one"), (511, 32, 1, "half"), (512, 4, 4, "half"),
         (513, 32, 1, "one"), (2048, 32, 1, "half"), (2048, 128, 4, "one"), (2049, 4, 1, "all-but-one"), (2049, 32, 0, "half"),
         (8192, 128, 1, "half"), (8192, 32, 4, "all-but-one"), (8192, 5, 0, "one")]


def test_the_cross_covers_what_the_issue_lists():
    assert {c[0] for c in CROSS} >= {2, 63, 64, 65, 255, 256, 257, 2048, 2049, 8192}
    assert {c[1] for c in CROSS} == {4, 5, 32, 128} and {c[2] for c in CROSS} == {0, 1, 4}
    assert {c[3] for c in CROSS} == {"one", "half", "all-but-one"}


@pytest.mark.parametrize("n,R,w,kind", CROSS)
def test_bit_equal_to_the_law(n, R, w, kind):
    clouds, ids = cube(3, n, n + R), [2, 0, 2, 1]
    frames, target = frames_of(4, n), target_of(n, kind)
    got, want = run(clouds, ids, frames, target, R, w), expect(clouds, ids, frames, target, R, w)
    assert_same(got, want)
    assert (got["side"].sum(1) == target).all()
    for b in range(4):                                       # every row of existing / missing is bitwise a row of gt, in order
        assert np.array_equal(bits(got["existing"][b]), bits(got["gt"][b][got["side"][b] == 1]))
        assert np.array_equal(bits(got["missing"][b]), bits(got["gt"][b][got["side"][b] == 0]))


@pytest.fixture(scope="module")
def alone():
    """257 rows, 5 clouds: each cloud's item under one frame per cloud, computed alone (B = 1) and by the law."""
    clouds, frames = cube(5, 257, 21), frames_of(5, 22)
    got = [run(clouds, [i], frames[i:i + 1], 100) for i in range(5)]
    for i in range(5):
        assert_same(got[i], expect(clouds, [i], frames[i:i + 1], 100), what=i)
    return clouds, frames, got


@pytest.mark.parametrize("B", [1, 3, 70])
def test_an_items_bits_do_not_depend_on_the_batch(alone, B):
    clouds, frames, single = alone
    ids = [(7 * b + 3) % 5 for b in range(B)]                # repeated and unordered
    got = run(clouds, ids, frames[ids], 100)
    for b, i in enumerate(ids):
        for k in ("existing", "missing", "gt", "side", "occlusion"):
            assert np.array_equal(bits(got[k][b]), bits(single[i][k][0])), (b, i, k)


def test_two_runs_give_the_same_bits_and_the_optional_outputs_change_nothing(alone):
    from hyperpocket_amd import ops
    clouds, frames, _ = alone
    ids = [4, 4, 0, 3, 1, 2]
    a, b = run(clouds, ids, frames[ids], 100), run(clouds, ids, frames[ids], 100)
    assert_same(a, b)
    for side, occlusion in ((False, False), (True, False), (False, True)):
        bufs = ops.make_view_batch_buffers(6, 257, 100, "cuda", side=side, occlusion=occlusion)
        c = run(clouds, ids, frames[ids], 100, out=bufs)
        assert (c["side"] is None) == (not side) and (c["occlusion"] is None) == (not occlusion)
        assert_same(c, a, [k for k in a if c[k] is not None])
        c = run(clouds, ids, frames[ids], 100, out={**bufs, "side": None, "occlusion": None})
        assert c["side"] is None and c["occlusion"] is None
        assert_same(c, a, ("existing", "missing", "gt"))


def test_duplicated_rows_straddle_the_threshold():
    """Every row four times, shuffled: the copies have the same occlusion, and row order decides which of them are in.  And a
    plate perpendicular to the axis with w = 0: every o is +0, the first `target` rows win."""
    r = np.random.default_rng(31)
    base = cube(2, 150, 32)
    clouds = np.stack([np.repeat(c, 4, 0)[r.permutation(600)] for c in base])
    frames = frames_of(2, 33)
    for target in (1, 299, 300, 301, 599):
        got, want = run(clouds, [0, 1], frames, target, 16, 1), expect(clouds, [0, 1], frames, target, 16, 1)
        assert_same(got, want, what=target)
    want = expect(clouds, [0, 1], frames, 299, 16, 1)          # copies come in fours: 299 cuts through a group of them
    o = want["occlusion"][0]
    tie = o == np.sort(o, kind="stable")[298]
    assert tie.sum() >= 4 and 0 < want["side"][0][tie].sum() < tie.sum()
    plate = np.zeros((1, 1000, 3), np.float32)
    plate[0, :, :2] = r.uniform(-0.4, 0.4, (1000, 2))
    plate[0, :, 2] = 0.125
    for target in (1, 512, 513, 999):
        got = run(plate, [0], np.eye(3, dtype=np.float32)[None], target, 16, 0)
        assert_same(got, expect(plate, [0], np.eye(3, dtype=np.float32)[None], target, 16, 0), what=target)
        assert np.array_equal(got["side"][0], (np.arange(1000) < target).astype(np.uint8))
        assert not bits(got["occlusion"]).any()


def test_all_rows_in_one_pixel_and_most_rows_clamped():
    clouds, frames = cube(2, 700, 41), frames_of(3, 42)
    tiny = clouds * np.float32(1e-4)                          # the four pixels at the image's centre
    small = tiny + np.float32(0.001)                          # one pixel: a single word takes every atomicMin
    for c in (tiny, small):
        got, want = run(c, [1, 0, 1], frames, 350, 32, 1), expect(c, [1, 0, 1], frames, 350, 32, 1)
        assert_same(got, want)
    from hyperpocket_amd import ops
    one = law.project(small[0], frames[1], DIST, law.scale_of(32, ops.view_half_extent(0.5, DIST)), 32)[1]
    assert len(np.unique(one)) == 1
    # an image far smaller than the object: most rows land in the border pixels
    h = 0.02
    pix = law.project(clouds[0], frames[0], DIST, law.scale_of(8, h), 8)[1]
    edge = (pix // 8 == 0) | (pix // 8 == 7) | (pix % 8 == 0) | (pix % 8 == 7)
    assert edge.mean() > 0.9 and not edge.all()
    for w in (0, 2):
        assert_same(run(clouds, [0, 1, 1], frames, 200, 8, w, h), expect(clouds, [0, 1, 1], frames, 200, 8, w, h), what=w)


def test_absent_rows():
    """NaN and +-inf coordinates, rows at and behind the sensor: they rank last, and fill up in row order where fewer than
    `target` rows project (more absent rows than N - target)."""
    r = np.random.default_rng(51)
    clouds = cube(3, 300, 52)
    clouds[0, r.permutation(300)[:40], r.integers(0, 3, 40)] = np.nan
    clouds[0, 7, 0], clouds[0, 8, 1], clouds[0, 299, 2] = np.inf, -np.inf, np.inf
    frames = frames_of(3, 53)
    behind = r.permutation(300)[:120]                         # pushed along the sensor's axis past it
    clouds[1, behind] += (np.float32(4.0) * frames[1][2]).astype(np.float32)
    clouds[1, 5] = (np.float32(3.0) * frames[1][2]).astype(np.float32)
    clouds[2, 10:] = np.nan                                   # ten rows left
    clouds[2, 3] = np.float32([0.0, np.inf, 0.0])
    want = expect(clouds, [0, 1, 2], frames, 250)
    absent = np.isposinf(want["occlusion"]).sum(1)
    assert absent[0] >= 40 and absent[1] >= 120 and absent[2] == 291 and (absent > 300 - 250).any()
    for target in (1, 9, 10, 150, 250, 299):
        assert_same(run(clouds, [0, 1, 2], frames, target), expect(clouds, [0, 1, 2], frames, target), what=target)
    everything = np.full((1, 64, 3), np.nan, np.float32)      # nothing projects: the first rows in row order
    got = run(everything, [0], frames[:1], 20)
    assert_same(got, expect(everything, [0], frames[:1], 20))
    assert np.array_equal(got["side"][0], (np.arange(64) < 20).astype(np.uint8))


def test_a_frame_need_not_be_orthonormal():
    clouds = cube(2, 400, 61)
    frames = np.float32([[[1.0, 0.25, 0.0], [0.0, 0.5, 0.125], [0.25, 0.0, 8.0]],          # skewed and scaled: some rows behind
                         [[0.0, 0.0, 0.0], [3.0, 3.0, 3.0], [1e-3, 0.0, 1e-3]],            # degenerate: one column of pixels
                         [[-7.5, 0.1, 0.3], [0.2, 1e4, 0.0], [0.0, 0.0, -1.0]]])           # mirrored, one axis blown up
    absent = np.isposinf(expect(clouds, [0, 1, 0], frames, 200)["occlusion"]).sum(1)
    assert 0 < absent[0] < 200 and absent[1] == 0 and absent[2] == 0
    for R, w in ((32, 1), (5, 4)):
        assert_same(run(clouds, [0, 1, 0], frames, 200, R, w), expect(clouds, [0, 1, 0], frames, 200, R, w), what=(R, w))


def test_an_id_outside_the_dataset_gets_zeros():
    clouds, frames = cube(3, 130, 71), frames_of(4, 72)
    got = run(clouds, [1, 3, -1, 2], frames, 50)
    want = expect(clouds, [1, 0, 0, 2], frames, 50)
    for b in (0, 3):
        assert_same({k: v[b] for k, v in got.items()}, {k: v[b] for k, v in want.items()}, what=b)
    for b in (1, 2):
        assert not got["existing"][b].any() and not got["missing"][b].any() and not got["gt"][b].any()
        assert np.array_equal(got["side"][b], (np.arange(130) < 50).astype(np.uint8)) and np.isposinf(got["occlusion"][b]).all()


def test_rotation_is_the_batch_makers():
    """degrees given: gt is bitwise hp_make_batch's gt for the same ids and degrees, the split is the unrotated one, and every
    row of existing / missing is a row of gt."""
    from hyperpocket_amd import ops
    clouds, frames = cube(3, 257, 81), frames_of(6, 82)
    ids, degs = [2, 0, 1, 1, 0, 2], [0, 90, 359, -45, 720, 17]
    plain = run(clouds, ids, frames, 100)
    got = run(clouds, ids, frames, 100, degrees=degs)
    dev = torch.device("cuda")
    ref = ops.make_batch(torch.from_numpy(clouds).to(dev), torch.tensor(ids, dtype=torch.int32, device=dev),
                         torch.arange(6, dtype=torch.int64, device=dev), 100,
                         degrees=torch.tensor(degs, dtype=torch.int32, device=dev), seed=1)
    assert np.array_equal(bits(got["gt"]), bits(ref[2].cpu().numpy()))
    assert_same(got, plain, ("side", "occlusion"))
    for b in range(6):
        assert np.array_equal(bits(got["existing"][b]), bits(got["gt"][b][got["side"][b] == 1]))
        assert np.array_equal(bits(got["missing"][b]), bits(got["gt"][b][got["side"][b] == 0]))
    assert_same({k: v[[0, 4]] for k, v in got.items()}, {k: v[[0, 4]] for k, v in plain.items()})     # 0 and 720 degrees: the bits
    assert not np.array_equal(got["gt"][1], plain["gt"][1])


def test_the_wrapper_checks_shapes_on_the_device():
    from hyperpocket_amd import ops
    dev = torch.device("cuda")
    clouds = torch.from_numpy(cube(3, 64, 91)).to(dev)
    ids = torch.zeros(2, dtype=torch.int32, device=dev)
    frames = ops.view_frames(2, 0).to(dev)
    with pytest.raises(ValueError):
        ops.make_view_batch(clouds, ids, frames[:1], 32)
    with pytest.raises(ValueError):
        ops.make_view_batch(clouds, ids, frames, 64)
    with pytest.raises(ops.HipExtensionError):
        ops.make_view_batch(clouds, ids.long(), frames, 32)
    with pytest.raises(ops.HipExtensionError):
        ops.make_view_batch(clouds, ids, frames, 32, out=ops.make_view_batch_buffers(3, 64, 32, dev))
    assert ops._plan("hp_make_view_batch_plan", (8192, 128), 2, "")[1] == 4 * 128 * 128 + 6 * 8192

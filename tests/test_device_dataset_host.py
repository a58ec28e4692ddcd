"""CPU suite: the host side of the device-resident data path (datasets/device_dataset.py) — the epoch bookkeeping
(permutation, shards, drop_last, stream ids) on CPU tensors, constructor validation, and the rotation table."""
import os

import numpy as np
import pytest
import torch


def plan(**kw):
    from hyperpocket_amd.datasets.device_dataset import epoch_plan
    a = dict(n_clouds=10, num_samples=4, batch_size=8, epoch=0, seed=1, device="cpu")
    a.update(kw)
    return epoch_plan(**a)


def test_an_epoch_is_a_permutation_of_every_cloud_and_scan():
    ids, streams, degrees = plan()
    assert ids.dtype == torch.int32 and streams.dtype == torch.int64 and degrees is None
    assert ids.is_contiguous() and streams.is_contiguous()
    assert sorted(streams.tolist()) == list(range(40))                      # item = cloud * num_samples + scan, each once
    assert torch.equal(ids.long(), streams // 4)                            # stream id = cloud * num_samples + scan
    assert streams.tolist() != list(range(40))
    again = plan()
    assert torch.equal(again[0], ids) and torch.equal(again[1], streams)    # a function of (seed, epoch)
    assert not torch.equal(plan(epoch=1)[1], streams) and not torch.equal(plan(seed=2)[1], streams)
    assert plan(shuffle=False)[1].tolist() == list(range(40))


def test_fresh_slices_mix_the_epoch_into_the_stream_id():
    fixed0, fixed1 = plan(epoch=0), plan(epoch=5)
    assert sorted(fixed0[1].tolist()) == sorted(fixed1[1].tolist())         # the same split of a (cloud, scan) in every epoch
    ids, streams, _ = plan(epoch=5, fresh_slices=True)
    assert torch.equal(ids, fixed1[0])                                      # the same order of clouds ...
    assert torch.equal(streams, fixed1[1] + 5 * 40)                         # ... under stream ids no other epoch uses
    assert torch.equal(plan(epoch=0, fresh_slices=True)[1], fixed0[1])


def test_shards_are_disjoint_complete_and_of_equal_length():
    whole = plan(batch_size=4)[1].tolist()
    parts = [plan(batch_size=4, rank=r, world=3)[1].tolist() for r in range(3)]
    assert [len(p) for p in parts] == [12, 12, 12]                          # 40 // 3 = 13 -> 3 whole batches of 4 per rank
    flat = sum(parts, [])
    assert len(set(flat)) == 36 and set(flat) <= set(whole)
    parts = [plan(batch_size=4, rank=r, world=3, drop_last=False)[1].tolist() for r in range(3)]
    assert sorted(sum(parts, [])) == list(range(40)) and [len(p) for p in parts] == [14, 13, 13]
    assert len(plan(batch_size=16)[0]) == 32 and len(plan(batch_size=16, drop_last=False)[0]) == 40
    with pytest.raises(ValueError):
        plan(rank=2, world=2)


def test_degrees_are_drawn_per_item_once_per_epoch():
    ids, streams, degrees = plan(rotate=True)
    assert degrees.dtype == torch.int32 and degrees.shape == ids.shape
    assert int(degrees.min()) >= 0 and int(degrees.max()) < 360 and len(set(degrees.tolist())) > 10
    assert torch.equal(plan(rotate=True)[2], degrees) and not torch.equal(plan(rotate=True, epoch=1)[2], degrees)
    assert torch.equal(plan(rotate=True)[1], plan()[1])                     # rotating does not move the permutation
    both = [plan(rotate=True, rank=r, world=2, batch_size=4) for r in range(2)]
    full = plan(rotate=True, batch_size=4)
    lookup = dict(zip(full[1].tolist(), full[2].tolist()))
    for _, s, d in both:
        assert [lookup[i] for i in s.tolist()] == d.tolist()               # an item keeps its degree on whichever rank it lands


def test_constructor_validation(tmp_path):
    from hyperpocket_amd import HipExtensionError
    from hyperpocket_amd.datasets.device_dataset import DeviceBatcher, DeviceDataset
    good = np.random.RandomState(0).rand(5, 16, 3)                          # float64 in: stored as contiguous float32
    ds = DeviceDataset(good, labels=[0, 1, 0, 1, 1], names=["x", "y"], device="cpu")
    assert ds.clouds.dtype == torch.float32 and ds.clouds.is_contiguous() and len(ds) == 5 and ds.n_points == 16
    assert torch.equal(ds.clouds, torch.from_numpy(good.astype(np.float32)))
    views = ds.by_label()
    assert list(views) == ["x", "y"] and len(views["x"]) == 2 and len(views["y"]) == 3
    assert torch.equal(views["y"].clouds, ds.clouds[[1, 3, 4]])
    strided = torch.from_numpy(good.astype(np.float32)).transpose(0, 1)     # (16,5,3) non-contiguous
    assert DeviceDataset(strided, device="cpu").clouds.is_contiguous()
    for bad in (np.zeros((5, 16)), np.zeros((5, 16, 2)), np.zeros((0, 16, 3)), np.zeros((5, 1, 3))):
        with pytest.raises(ValueError):
            DeviceDataset(bad, device="cpu")
    for poison in (np.nan, np.inf):
        broken = good.copy()
        broken[3, 7, 1] = poison
        with pytest.raises(ValueError, match="non-finite"):
            DeviceDataset(broken, device="cpu")
    with pytest.raises(ValueError):
        DeviceDataset(good, labels=[0, 1], device="cpu")
    with pytest.raises(ValueError):
        DeviceDataset(good, labels=[0, 1, 0, 1, 2], names=["x", "y"], device="cpu")
    with pytest.raises(ValueError):
        DeviceDataset(good, device="cpu").by_label()
    # files: .npy is the array, .npz carries clouds [+ labels, names]
    np.save(tmp_path / "c.npy", good.astype(np.float32))
    np.savez(tmp_path / "c.npz", clouds=good.astype(np.float32), labels=np.array([0, 1, 0, 1, 1]), names=np.array(["x", "y"]))
    assert torch.equal(DeviceDataset(str(tmp_path / "c.npy"), device="cpu").clouds, ds.clouds)
    from_npz = DeviceDataset(tmp_path / "c.npz", device="cpu")
    assert torch.equal(from_npz.clouds, ds.clouds) and from_npz.names == ["x", "y"] and from_npz.labels.tolist() == [0, 1, 0, 1, 1]
    with pytest.raises(ValueError):
        DeviceDataset(os.path.join(str(tmp_path), "c.txt"), device="cpu")
    # the batcher has no CPU path
    with pytest.raises(HipExtensionError):
        DeviceBatcher(ds, 2, target=8)
    with pytest.raises(TypeError):
        DeviceBatcher(good, 2, target=8)


def test_rotation_table():
    """(cos, sin) per degree = the [0,0] and [1,0] entries of scipy's Rotation.from_euler('z', deg, degrees=True)
    .as_matrix().astype(float32); without scipy, the same half-angle closed form in fp64, cast."""
    from hyperpocket_amd import ops
    tab = ops.rotation_table().numpy()
    assert tab.shape == (360, 2) and tab.dtype == np.float32
    try:
        from scipy.spatial.transform import Rotation
        m = np.stack([Rotation.from_euler("z", d, degrees=True).as_matrix().astype(np.float32) for d in range(360)])
        want = np.stack([m[:, 0, 0], m[:, 1, 0]], 1)
    except ImportError:
        h = np.deg2rad(np.arange(360, dtype=np.float64)) / 2
        want = np.stack([np.cos(h) ** 2 - np.sin(h) ** 2, 2 * np.sin(h) * np.cos(h)], 1).astype(np.float32)
    assert np.array_equal(tab, want)
    a = np.deg2rad(np.arange(360, dtype=np.float64))
    assert np.abs(tab - np.stack([np.cos(a), np.sin(a)], 1)).max() <= 2.0 ** -24
    assert tab[0].tolist() == [1.0, 0.0] and tab[90, 1] == 1.0 and tab[180, 0] == -1.0


def test_default_groups_fill_the_chip_twice():
    from hyperpocket_amd import ops
    assert ops.make_batch_default_groups(64) == 32 and ops.make_batch_default_groups(8) == 64
    assert ops.make_batch_default_groups(4096) == 1 and ops.make_batch_default_groups(100) == 21


def test_make_batch_rejects_bad_shapes_on_the_host():
    from hyperpocket_amd import ops
    lib = ops.load_library()
    import ctypes
    lib.hp_make_batch_workspace_bytes.restype = ctypes.c_long
    assert lib.hp_make_batch_workspace_bytes(64, 2048) == 256
    assert lib.hp_make_batch_workspace_bytes(65, 2048) == 512
    assert lib.hp_make_batch_workspace_bytes(0, 64) == -1 and lib.hp_make_batch_workspace_bytes(2, 8193) == -1
    # validation precedes every HIP call: -1 without a GPU
    null = [None] * 7
    args = lambda M, N, target, B, groups: (M, N, target, None, B, None, None, None, None, ctypes.c_ulonglong(0), 10, groups, *null, None)
    for a in ((1, 64, 64, 1, 1), (1, 8193, 10, 1, 1), (1, 64, 32, 0, 1), (1, 64, 32, 1, 0), (1, 64, 32, 1, 1)):
        assert lib.hp_make_batch(*args(*a)) == -1, a

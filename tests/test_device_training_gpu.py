"""GPU: DeviceDataset / DeviceBatcher (datasets/device_dataset.py) and the epoch loops built on them (core/training.py):
an epoch is every (cloud, scan) once, sharded over ranks, reproducible per seed, identical with and without prefetch;
train_epoch is engine.step per batch with the means taken once; val_epoch is the reference's formula
(core/epoch_loops.py:49-83); a cloud that cannot be sliced surfaces at the end of the epoch."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = {"random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
       "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
       "hyper_network": {"use_bias": True, "relu_slope": 0.2},
       "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                          "layer_out_channels": [32, 64, 128, 64]},
       "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}


def small_clouds(m, n, seed):
    return np.random.RandomState(seed).rand(m, n, 3).astype(np.float32) - 0.5


def epoch_of(batcher):
    """[(existing, missing, gt, labels)] of one epoch as host arrays (a batch is only valid until the next one)."""
    return [tuple(None if t is None else t.cpu().numpy().copy() for t in batch) for batch in batcher]


def items_of(epoch, clouds):
    """Every item of an epoch as (cloud number, bytes of its `existing`)."""
    which = {c.tobytes(): i for i, c in enumerate(clouds)}
    return [(which[gt[b].tobytes()], ex[b].tobytes()) for ex, _, gt, _ in epoch for b in range(gt.shape[0])]


@pytest.fixture(scope="module")
def data():
    from hyperpocket_amd.datasets.device_dataset import DeviceDataset
    clouds = small_clouds(40, 64, 5)
    return clouds, DeviceDataset(clouds, labels=np.arange(40) % 4, names=["a", "b", "c", "d"])


def batcher_of(ds, **kw):
    from hyperpocket_amd.datasets.device_dataset import DeviceBatcher
    return DeviceBatcher(ds, 8, target=32, num_samples=4, **kw)


def test_an_epoch_is_every_cloud_and_scan_once(data):
    clouds, ds = data
    bt = batcher_of(ds, seed=1)
    assert len(bt) == 20
    first, second = epoch_of(bt), epoch_of(bt)
    assert len(first) == 20 and all(ex.shape == (8, 32, 3) and mi.shape == (8, 32, 3) and gt.shape == (8, 64, 3) for ex, mi, gt, _ in first)
    for ex, mi, gt, lab in first:
        for b in range(8):
            assert int(lab[b]) == {c.tobytes(): i for i, c in enumerate(clouds)}[gt[b].tobytes()] % 4
    a, b = items_of(first, clouds), items_of(second, clouds)
    assert sorted(c for c, _ in a) == sorted(list(range(40)) * 4)    # 40 clouds x 4 scans
    # ... four different splits per cloud (two of 240 pairs of random planes may cut 64 points alike: a handful at most)
    assert len(set(a)) >= 152
    assert sorted(a) == sorted(b) and a != b                         # fixed slices, another order in the next epoch
    assert bt.failures() == 0
    fresh = batcher_of(ds, seed=1, fresh_slices=True)
    f0, f1 = items_of(epoch_of(fresh), clouds), items_of(epoch_of(fresh), clouds)
    assert sorted(f0) == sorted(a)                                   # epoch 0 mixes nothing into the stream ids
    assert sorted(c for c, _ in f1) == sorted(c for c, _ in a) and len(set(f1) & set(f0)) <= 8      # epoch 1: new planes


def test_ranks_are_disjoint_and_complete(data):
    clouds, ds = data
    whole = items_of(epoch_of(batcher_of(ds, seed=1)), clouds)
    r0 = items_of(epoch_of(batcher_of(ds, seed=1, rank=0, world=2)), clouds)
    r1 = items_of(epoch_of(batcher_of(ds, seed=1, rank=1, world=2)), clouds)
    assert len(r0) == len(r1) == 80
    assert sorted(r0 + r1) == sorted(whole)                          # as multisets: nothing twice, nothing missing


def test_equal_seeds_equal_epochs_and_prefetch_changes_nothing(data):
    _, ds = data
    base = epoch_of(batcher_of(ds, seed=2, rotate=True))
    for kw in ({}, {"prefetch": True}, {"groups": 3}):
        other = epoch_of(batcher_of(ds, seed=2, rotate=True, **kw))
        assert len(other) == len(base)
        for x, y in zip(base, other):
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), kw
    another = epoch_of(batcher_of(ds, seed=3, rotate=True))
    assert not all(np.array_equal(x[2], y[2]) for x, y in zip(base, another))
    # a rotation about z: z kept, the distance from the axis kept; some batch really is rotated
    plain = epoch_of(batcher_of(ds, seed=2))
    assert all(np.array_equal(x[2][..., 2], y[2][..., 2]) for x, y in zip(base, plain))
    assert any(not np.array_equal(x[2], y[2]) for x, y in zip(base, plain))
    for x, y in zip(base, plain):
        assert np.abs(np.hypot(x[2][..., 0], x[2][..., 1]) - np.hypot(y[2][..., 0], y[2][..., 1])).max() <= 1e-6


def test_two_epochs_with_prefetch_and_a_ragged_last_batch(data):
    from hyperpocket_amd.datasets.device_dataset import DeviceBatcher
    clouds, ds = data
    kw = dict(target=32, num_samples=1, drop_last=False, seed=4)
    a, b = DeviceBatcher(ds, 12, **kw), DeviceBatcher(ds, 12, prefetch=True, **kw)
    assert len(a) == 4
    for _ in range(2):
        ea, eb = epoch_of(a), epoch_of(b)
        assert [x[2].shape[0] for x in ea] == [12, 12, 12, 4]
        assert sorted(c for c, _ in items_of(ea, clouds)) == list(range(40))
        for x, y in zip(ea, eb):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))


def build_model(seed):
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    torch.manual_seed(seed)
    model = FullModel(copy.deepcopy(CFG))
    model.apply(weights_init)
    return model.cuda()


def train_setup(clouds, **kw):
    from hyperpocket_amd.core.engine import TrainEngine
    from hyperpocket_amd.datasets.device_dataset import DeviceBatcher, DeviceDataset
    model = build_model(7)
    return TrainEngine(model), DeviceBatcher(DeviceDataset(clouds), 4, target=128, num_samples=1, seed=3, **kw)


def test_train_epoch_is_engine_step_per_batch():
    from hyperpocket_amd import ops
    from hyperpocket_amd.core.training import train_epoch
    clouds = small_clouds(12, 256, 9)
    try:
        engine, batcher = train_setup(clouds)
        got = train_epoch(1, engine, batcher)
        assert engine.steps == 3
        engine, batcher = train_setup(clouds)
        by_hand = [{k: v.item() for k, v in engine.step(ex, mi, gt, 1).items()} for ex, mi, gt, _ in batcher]
    finally:
        ops.clear_grad_views()
    assert len(by_hand) == 3 and set(got) == {"loss_all", "loss_r", "loss_kld"}
    for k, v in got.items():
        want = sum(s[k] for s in by_hand) / 3
        assert np.isfinite(v) and v > 0
        # the same kernels on the same inputs; 1e-5 = 100 fp32 ulps for reductions whose order the device may choose
        assert abs(v - want) <= 1e-5 * abs(want), (k, v, want)


def test_val_epoch_is_the_references_formula():
    from hyperpocket_amd.core.training import val_epoch
    from hyperpocket_amd.datasets.device_dataset import DeviceBatcher, DeviceDataset
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    clouds = small_clouds(12, 256, 10)
    sets = DeviceDataset(clouds, labels=[0] * 6 + [1] * 6, names=["chair", "table"]).by_label()
    assert list(sets) == ["chair", "table"] and all(len(s) == 6 for s in sets.values())
    batchers = lambda: {k: DeviceBatcher(s, 3, target=128, num_samples=1, seed=5, shuffle=False) for k, s in sets.items()}
    model = build_model(7)
    model.train()
    got = val_epoch(3, model, batchers())
    assert model.training
    model.eval()
    val_epoch(3, model, batchers())
    assert not model.training
    # by hand, on an identically seeded model (the decoder's input points follow the model's own draw counter)
    model = build_model(7)
    model.eval()
    want = {}
    with torch.no_grad():
        for name, bt in batchers().items():
            loss = 0.0
            for i, (ex, mi, gt, _) in enumerate(bt, 1):
                rec = model(ex.clone(), mi.clone(), list(gt.shape), 3, gt.device)
                loss += torch.mean(0.05 * ChamferLoss()(gt, rec.permute(0, 2, 1))).item()
            want[name] = loss / i
    want["total"] = sum(want.values()) / 2
    assert set(got) == {"chair", "table", "total"}
    for k in want:
        assert np.isfinite(got[k]) and abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), (k, got[k], want[k])


def test_a_cloud_that_cannot_be_sliced_surfaces_at_the_end_of_the_epoch():
    from hyperpocket_amd import HipExtensionError, ops
    from hyperpocket_amd.core.training import train_epoch
    clouds = small_clouds(12, 256, 11)
    clouds[7] = np.float32([0.1, 0.2, -0.3])                  # 256 identical points: on one side of every plane
    try:
        engine, batcher = train_setup(clouds, max_candidates=4096)
        with pytest.raises(HipExtensionError, match="1 item"):
            train_epoch(1, engine, batcher)
        assert engine.steps == 3                              # the whole epoch ran first
        assert batcher.failures() == 1
    finally:
        ops.clear_grad_views()

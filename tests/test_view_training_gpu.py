"""GPU: DeviceViewBatcher (datasets/device_dataset.py) — DeviceBatcher's epochs, ranks, rotation and prefetch over the viewpoint
batch maker: an epoch is every (cloud, scan) once with the view of its item, the same in every epoch unless fresh_slices asks
for new ones; and the epoch loops of core/training.py run over it unchanged."""
import copy

import numpy as np
import pytest
import torch

import view_split_law as law

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
    from hyperpocket_amd.datasets.device_dataset import DeviceViewBatcher
    return DeviceViewBatcher(ds, 8, target=32, num_samples=4, resolution=8, **kw)


def views_by_the_law(clouds, bt, epoch):
    """Every (cloud, scan) of an epoch as (cloud number, bytes of its `existing`), from the law and the batcher's own frames."""
    frames = bt.frames(epoch).numpy()
    scale = law.scale_of(bt.resolution, bt.half_extent)
    return [(item // 4, law.view_split(clouds[item // 4], frames[item], bt.distance, scale, bt.resolution, bt.window,
                                       bt.target)["existing"].tobytes()) for item in range(len(clouds) * 4)]


def test_an_epoch_is_every_cloud_and_scan_once_under_its_items_view(data):
    from hyperpocket_amd import ops
    clouds, ds = data
    bt = batcher_of(ds, seed=1)
    assert len(bt) == 20 and bt.failures() == 0
    assert abs(bt.radius - np.sqrt((clouds.astype(np.float64) ** 2).sum(-1).max())) <= 1e-6       # the largest point norm
    assert bt.half_extent == ops.view_half_extent(bt.radius, 3.0)
    assert torch.equal(bt.frames(0), ops.view_frames(160, 1)) and torch.equal(bt.frames(5), ops.view_frames(160, 1))
    first, second = epoch_of(bt), epoch_of(bt)
    assert len(first) == 20 and all(ex.shape == (8, 32, 3) and mi.shape == (8, 32, 3) and gt.shape == (8, 64, 3) for ex, mi, gt, _ in first)
    for ex, mi, gt, lab in first:
        for b in range(8):
            assert int(lab[b]) == {c.tobytes(): i for i, c in enumerate(clouds)}[gt[b].tobytes()] % 4
            rows = {r.tobytes() for r in gt[b]}
            assert all(r.tobytes() in rows for r in ex[b]) and all(r.tobytes() in rows for r in mi[b])
    a, b = items_of(first, clouds), items_of(second, clouds)
    assert sorted(c for c, _ in a) == sorted(list(range(40)) * 4)    # 40 clouds x 4 scans
    assert len(set(a)) == 160                                        # four different views per cloud
    assert sorted(a) == sorted(b) and a != b                         # the same views, another order in the next epoch
    assert sorted(a) == sorted(views_by_the_law(clouds, bt, 0))      # item (cloud, scan) under row `item` of the frames
    assert bt.failures() == 0


def test_fresh_slices_changes_the_views_between_epochs_and_the_default_does_not(data):
    from hyperpocket_amd import ops
    clouds, ds = data
    fresh = batcher_of(ds, seed=1, fresh_slices=True)
    assert torch.equal(fresh.frames(0), ops.view_frames(160, (1, 0))) and torch.equal(fresh.frames(1), ops.view_frames(160, (1, 1)))
    assert not torch.equal(fresh.frames(0), fresh.frames(1))
    f0, f1 = items_of(epoch_of(fresh), clouds), items_of(epoch_of(fresh), clouds)
    assert sorted(c for c, _ in f0) == sorted(c for c, _ in f1) == sorted(list(range(40)) * 4)
    assert len(set(f0) & set(f1)) <= 8                               # epoch 1: new views
    assert sorted(f0) == sorted(views_by_the_law(clouds, fresh, 0)) and sorted(f1) == sorted(views_by_the_law(clouds, fresh, 1))
    fresh.set_epoch(0)
    assert sorted(items_of(epoch_of(fresh), clouds)) == sorted(f0)   # an epoch's views are a function of (seed, epoch)
    fixed = batcher_of(ds, seed=1)
    fixed.set_epoch(3)
    assert sorted(items_of(epoch_of(fixed), clouds)) == sorted(views_by_the_law(clouds, fixed, 0))


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
    for kw in ({}, {"prefetch": True}):
        other = epoch_of(batcher_of(ds, seed=2, rotate=True, **kw))
        assert len(other) == len(base)
        for x, y in zip(base, other):
            assert all(np.array_equal(p, q) for p, q in zip(x, y)), kw
    another = epoch_of(batcher_of(ds, seed=3, rotate=True))
    assert not all(np.array_equal(x[2], y[2]) for x, y in zip(base, another))
    # a rotation about z of the output rows: z kept, and the split is the unrotated cloud's
    plain = epoch_of(batcher_of(ds, seed=2))
    assert all(np.array_equal(x[2][..., 2], y[2][..., 2]) and np.array_equal(x[0][..., 2], y[0][..., 2]) for x, y in zip(base, plain))
    assert any(not np.array_equal(x[2], y[2]) for x, y in zip(base, plain))


def test_two_epochs_with_prefetch_and_a_ragged_last_batch(data):
    from hyperpocket_amd.datasets.device_dataset import DeviceViewBatcher
    clouds, ds = data
    kw = dict(target=32, num_samples=1, drop_last=False, seed=4, resolution=8)
    a, b = DeviceViewBatcher(ds, 12, **kw), DeviceViewBatcher(ds, 12, prefetch=True, **kw)
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
    from hyperpocket_amd.datasets.device_dataset import DeviceDataset, DeviceViewBatcher
    model = build_model(7)
    return TrainEngine(model), DeviceViewBatcher(DeviceDataset(clouds), 4, target=128, num_samples=1, seed=3, resolution=16, **kw)


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
        # The bar of test_device_training_gpu.py: both sides run the same kernels on bitwise the same batches (the view batcher
        # is bit-reproducible), so what may differ is the order of reductions the device is free to choose and the epoch's mean,
        # taken once on the device there and from three host doubles here: 1e-5 relative = 100 fp32 ulps.
        assert abs(v - want) <= 1e-5 * abs(want), (k, v, want)


def test_val_epoch_runs_on_view_batchers_per_category():
    from hyperpocket_amd.core.training import val_epoch
    from hyperpocket_amd.datasets.device_dataset import DeviceDataset, DeviceViewBatcher
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    clouds = small_clouds(12, 256, 10)
    sets = DeviceDataset(clouds, labels=[0] * 6 + [1] * 6, names=["chair", "table"]).by_label()
    batchers = lambda: {k: DeviceViewBatcher(s, 3, target=128, num_samples=1, seed=5, shuffle=False, resolution=16)
                        for k, s in sets.items()}
    model = build_model(7)
    model.eval()
    got = val_epoch(3, model, batchers())
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

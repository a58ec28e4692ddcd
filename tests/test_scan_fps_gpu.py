"""GPU suite for ScanBatcher(resample="farthest"): the two-stage batch (a pool by tests/scan_law.py, the picks by
tests/fps_law.py) bit for bit at every batch size, the default resampling left alone, and fixed() over such a batcher."""
import copy
import os

import numpy as np
import pytest
import torch

import fps_law
import scan_law

pytestmark = pytest.mark.gpu

CUDA = "cuda"
SEED = 77
TARGET = 64
LENGTHS = [40, 64, 300, 9000]


def _scan(n, seed):
    r = np.random.RandomState(seed)
    return (r.standard_normal((n, 3)) * 0.1 + np.array([0.3, -0.2, 1.0])).astype(np.float32)


@pytest.fixture(scope="module")
def scans():
    return [_scan(n, 10 + n) for n in LENGTHS]


@pytest.fixture(scope="module")
def expected(scans):
    """Per (normalize, pool) and scan: (scan rows (TARGET) int64, the rows' values, the final radius2), computed once."""
    memo = {}

    def get(normalize, pool):
        if (normalize, pool) not in memo:
            rows = []
            for s, scan in enumerate(scans):
                values = scan
                if normalize:
                    center, scale = scan_law.boxes_fp32(scan)
                    values = (scan - center) / scale
                    assert values.dtype == np.float32
                pool_eff = max(TARGET, min(pool, 8192))
                n = len(scan)
                kept = np.arange(n) if n <= pool_eff else scan_law.index_law(SEED, s, n, pool_eff, False)   # stream = item = s
                index, radius2 = fps_law.fps_law(values[kept], TARGET)
                rows.append((kept[index], values[kept[index]], radius2[-1]))
            memo[(normalize, pool)] = rows
        return memo[(normalize, pool)]
    return get


@pytest.mark.parametrize("batch_size", [1, 3, 4])
@pytest.mark.parametrize("normalize,pool", [(True, 8192), (False, 8192), (True, 128), (False, 16)])
def test_farthest_batches_follow_both_laws(scans, expected, normalize, pool, batch_size):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    batcher = ScanBatcher(DeviceScanDataset(scans, device=CUDA), batch_size, target=TARGET, normalize=normalize, seed=SEED,
                          resample="farthest", pool=pool)
    assert batcher.pool == max(TARGET, min(pool, 8192))
    want = expected(normalize, pool)
    item = 0
    for existing, ids, gt in batcher:
        B = existing.size(0)
        assert gt is None and ids.tolist() == list(range(item, item + B))
        assert batcher.last_index.shape == (B, TARGET) and batcher.last_index.dtype == torch.int32
        assert batcher.last_radius2.shape == (B,) and batcher.last_radius2.dtype == torch.float32
        rows, index, radius2 = existing.cpu().numpy(), batcher.last_index.cpu().numpy(), batcher.last_radius2.cpu().numpy()
        for b in range(B):
            want_index, want_rows, want_radius2 = want[item + b]
            n = LENGTHS[item + b]
            assert np.array_equal(index[b], want_index), (item + b, int((index[b] != want_index).sum()))
            assert np.array_equal(rows[b].view(np.uint32), want_rows.view(np.uint32)), item + b
            assert radius2[b].view(np.uint32) == want_radius2.view(np.uint32), item + b
            assert index[b, 0] == (0 if n <= batcher.pool else want_index[0])
            if n <= TARGET:                                        # every row once in pick order, then row 0
                assert sorted(index[b, :n].tolist()) == list(range(n)) and np.all(index[b, n:] == 0)
            else:
                assert len(set(index[b].tolist())) == TARGET
            assert (radius2[b] == 0) == (min(n, batcher.pool) <= TARGET)   # the kept points are the whole pool or not
        item += B
    assert item == len(scans) and batcher.failures() == 0


def test_draws_differ_only_beyond_the_pool(scans):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    batcher = ScanBatcher(DeviceScanDataset(scans, device=CUDA), 8, target=TARGET, seed=SEED, draws=2, resample="farthest")
    existing, ids, _ = next(iter(batcher))
    assert ids.tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    index = batcher.last_index.cpu().numpy()
    for s in range(3):                                             # n <= pool: exact farthest-point sampling, no draw in it
        assert np.array_equal(index[2 * s], index[2 * s + 1])
    assert not np.array_equal(index[6], index[7])                  # 9000 > 8192: another pool, other picks
    for b, stream in ((6, 6), (7, 7)):
        kept = scan_law.index_law(SEED, stream, 9000, 8192, False)
        assert np.array_equal(index[b], kept[fps_law.fps_law(scans[3][kept], TARGET)[0]])


def test_default_resampling_is_left_alone(scans):
    from hyperpocket_amd import ops
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    data = DeviceScanDataset(scans, device=CUDA)
    for normalize in (False, True):
        center, scale = data.boxes() if normalize else (None, None)
        ids = torch.arange(4, dtype=torch.int32, device=CUDA)
        want, want_index, _ = ops.prepare_scans(data.points, data.offsets, ids, ids.long(), TARGET, False, SEED, center, scale)
        for batcher in (ScanBatcher(data, 4, target=TARGET, normalize=normalize, seed=SEED),
                        ScanBatcher(data, 4, target=TARGET, normalize=normalize, seed=SEED, resample="subset", pool=100)):
            existing, _, _ = next(iter(batcher))
            assert torch.equal(existing.view(torch.int32), want.view(torch.int32))
            assert torch.equal(batcher.last_index, want_index) and batcher.last_radius2 is None
            for s in range(4):
                assert np.array_equal(want_index[s].cpu().numpy(), scan_law.index_law(SEED, s, LENGTHS[s], TARGET, False))


def test_fixed_over_a_farthest_batcher(tmp_path, scans):
    from hyperpocket_amd.core.experiments import fixed
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    from hyperpocket_amd.model.full_model import FullModel
    cfg = {"random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "hyper_network": {"use_bias": True, "relu_slope": 0.2},
           "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                              "layer_out_channels": [32, 64, 128, 64]},
           "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}
    torch.manual_seed(2020)
    model = FullModel(copy.deepcopy(cfg))
    model.apply(weights_init)
    model = model.cuda().eval()
    pair = [scans[2], scans[3]]                                    # 300 and 9000 points
    batcher = ScanBatcher(DeviceScanDataset(pair, device=CUDA), 2, target=TARGET, seed=SEED, resample="farthest")
    torch.manual_seed(4)
    existing_list, generated = fixed(model, torch.device(CUDA), {"scan": batcher}, str(tmp_path), 1, noises_per_item=2,
                                     batch_size=2)
    names = sorted(os.listdir(tmp_path / "fixed"))
    assert names == sorted([f"scan_{i}_{j}_reconstruction.npy" for i in range(2) for j in range(2)]
                           + [f"scan_{i}_existing.npy" for i in range(2)])
    assert len(existing_list) == 2 and generated.shape == (2, 2, 2048, 3)
    assert bool(torch.isfinite(generated).all())
    index = batcher.last_index.cpu().numpy()
    for i, scan in enumerate(pair):
        kept = np.load(tmp_path / "fixed" / f"scan_{i}_existing.npy")
        assert kept.shape == (3, TARGET) and kept.dtype == np.float32
        assert np.array_equal(kept.T, scan[index[i]])              # every column is a row of its scan: the picked one
        assert np.array_equal(existing_list[i].cpu().numpy(), kept.T)

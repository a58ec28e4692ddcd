"""GPU suite for the partial-scan pipeline above the kernels: core.experiments.fixed() against the golden-pinned forward(),
FullModel.encode_existing / sample_completions(code=), the written directory through compute_mmd_tmd_uhd against
completion_metrics on the returned tensors, and DeviceScanDataset.from_npy_dir with the way back into the scene."""
import copy
import os

import numpy as np
import pytest
import torch

import scan_law
from conftest import fixture_state_, golden

pytestmark = pytest.mark.gpu

CUDA = "cuda"
TARGET = 64          # points per prepared scan: tiny, the decoder's 2048 is fixed()'s own


def trained_model():
    """The seeded-init model brought to model_trained.npz's operating point (completions of unit scale), in eval mode."""
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    cfg = {"random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "hyper_network": {"use_bias": True, "relu_slope": 0.2},
           "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                              "layer_out_channels": [32, 64, 128, 64]},
           "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}
    gm = golden("model_trained")
    torch.manual_seed(int(gm["seed"]))
    model = FullModel(copy.deepcopy(cfg))
    model.apply(weights_init)
    model = model.cuda()
    fixture_state_(model.state_dict(), gm)
    return model.eval(), gm


def _scan(n, seed, centre=(0.0, 0.0, 0.0)):
    r = np.random.RandomState(seed)
    return (r.standard_normal((n, 3)) * 0.1 + np.asarray(centre)).astype(np.float32)


def _categories():
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset, ScanBatcher
    sets = {"blob": [_scan(n, 20 + n) for n in (50, 64, 300)], "shifted": [_scan(n, 40 + n, (0.1, -0.05, 0.0)) for n in (90, 33)]}
    return {cat: ScanBatcher(DeviceScanDataset(scans, device=CUDA), 2, target=TARGET, seed=5) for cat, scans in sets.items()}


def _record_points(model):
    """Keep every decoder-input draw of the model's sampler, in call order."""
    drawn, draw = [], model._draw_points

    def recording(*a, **kw):
        drawn.append(draw(*a, **kw))
        return drawn[-1]
    model._draw_points = recording
    return drawn


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One fixed() run over two categories (3 and 2 scans, batches of 2, 10 noises each), shared and left unchanged."""
    from hyperpocket_amd.core.experiments import fixed
    results_dir = tmp_path_factory.mktemp("results")
    os.makedirs(results_dir / "fixed" / "stale")                  # must be cleared
    (results_dir / "fixed" / "old_0_0_reconstruction.npy").write_bytes(b"x")
    model, gm = trained_model()
    drawn = _record_points(model)
    torch.manual_seed(31)
    existing_list, generated = fixed(model, torch.device(CUDA), _categories(), str(results_dir), int(gm["epoch"]), std=0.2,
                                     noises_per_item=10, batch_size=2)
    return {"dir": results_dir, "model": model, "epoch": int(gm["epoch"]), "drawn": drawn, "existing": existing_list,
            "generated": generated}


def test_fixed_writes_the_shape_dir_protocol(run):
    from hyperpocket_amd.utils.evaluation.shape_dir import grouped_paths, load_points
    d = str(run["dir"] / "fixed")
    names = sorted(os.listdir(d))
    want = sorted([f"{cat}_{i}_{j}_reconstruction.npy" for cat, n in (("blob", 3), ("shifted", 2)) for i in range(n) for j in range(10)]
                  + [f"{cat}_{i}_existing.npy" for cat, n in (("blob", 3), ("shifted", 2)) for i in range(n)])
    assert names == want                                           # nothing stale, nothing missing
    groups, ex = grouped_paths(d, True)
    assert len(groups) == 5 and len(ex) == 5
    for group, e in zip(groups, ex):
        stem = os.path.basename(e)[:-len("existing.npy")]
        assert all(os.path.basename(p).startswith(stem) for p in group)
        assert np.load(e).shape == (3, TARGET)
        assert all(np.load(p).shape == (3, 2048) and np.load(p).dtype == np.float32 for p in group)
    assert load_points(ex).shape == (5, TARGET, 3)
    assert not run["model"].training
    assert len(run["existing"]) == 5 and run["generated"].shape == (5, 10, 2048, 3)


def test_fixed_equals_forward_bit_for_bit(run):
    """Every file is forward(existing, None, [B,2048,3], epoch, device, noise, points) with fixed()'s own noise (torch's
    global CPU generator, 10 draws of (B, noise_size) per batch, in batch order) and its own decoder points."""
    model, epoch, d = run["model"], run["epoch"], run["dir"] / "fixed"
    fresh, _ = trained_model()                                     # forward() on an identically built model
    torch.manual_seed(31)
    call, item = 0, 0
    with torch.no_grad():
        for cat, batcher in _categories().items():
            for i, (existing, ids, _) in enumerate(batcher):
                B = existing.size(0)
                for k in range(B):
                    on_disk = np.load(d / f"{cat}_{i * 2 + k}_existing.npy")
                    assert np.array_equal(on_disk, existing[k].cpu().numpy().T)
                    assert torch.equal(run["existing"][item + k], existing[k])
                for j in range(10):
                    noise = torch.empty(B, model.get_noise_size()).normal_(mean=0.0, std=0.2).to(CUDA)
                    points = run["drawn"][call]
                    call += 1
                    want = fresh(existing.clone(), None, [B, 2048, 3], epoch, torch.device(CUDA), noise=noise, points=points)
                    assert want.shape == (B, 3, 2048)
                    for k in range(B):
                        got = np.load(d / f"{cat}_{i * 2 + k}_{j}_reconstruction.npy")
                        assert np.array_equal(got.view(np.uint32), want[k].cpu().numpy().view(np.uint32)), (cat, i, k, j)
                        assert torch.equal(run["generated"][item + k, j], want[k].t())
                item += B
    assert call == len(run["drawn"]) == 30 and item == 5           # 3 batches x 10 noises, one decoder call each


def test_fixed_encodes_a_batch_once(tmp_path):
    from hyperpocket_amd.core.experiments import fixed
    model, gm = trained_model()
    calls, encode = [], model.real_encoder.forward
    model.real_encoder.forward = lambda *a, **kw: (calls.append(1), encode(*a, **kw))[1]
    items = [(_scan(TARGET, 60 + i), 0, 0, i) for i in range(3)]   # a map-style dataset of (existing, missing, gt, idx)
    existing_list, generated = fixed(model, torch.device(CUDA), {"plain": items}, str(tmp_path), int(gm["epoch"]),
                                     noises_per_item=10, batch_size=2)
    assert len(calls) == 2                                         # two batches, one encoder pass each
    assert generated.shape == (3, 10, 2048, 3) and len(existing_list) == 3
    for i, it in enumerate(items):
        assert np.array_equal(np.load(tmp_path / "fixed" / f"plain_{i}_existing.npy"), it[0].T)
    assert len(os.listdir(tmp_path / "fixed")) == 33


def test_code_keyword_equals_encoding_inside():
    from hyperpocket_amd import ops
    model, gm = trained_model()
    epoch, K = int(gm["epoch"]), 5
    gen = torch.Generator().manual_seed(3)
    noise = (0.2 * torch.randn(K, model.get_noise_size(), generator=gen)).cuda()
    points = ops.sample_points(K, 256, 1.0, 99, 1, CUDA)
    for rows in (1, K):
        existing = torch.from_numpy(np.stack([_scan(TARGET, 70 + r) for r in range(rows)])).cuda()
        with torch.no_grad():
            code = model.encode_existing(existing)
            assert code.shape == (rows, 128)
            want = model.sample_completions(existing, noise, 256, epoch, points=points)
            got = model.sample_completions(None, noise, 256, epoch, points=points, code=code)     # existing is not read
        assert torch.equal(got, want)
    with pytest.raises(ValueError):
        model.sample_completions(None, noise, 256, epoch, points=points, code=code[:, :64])
    with pytest.raises(ValueError):
        model.sample_completions(None, noise, 256, epoch, points=points, code=code[:3])
    with pytest.raises(ValueError):
        model.encode_existing(existing.transpose(1, 2))


def test_written_directory_and_returned_tensors_give_the_same_metrics(run):
    """The disk and tensor routes of tests/test_completion_metrics_gpu.py meet at rtol 1e-5; so do these."""
    from hyperpocket_amd.core.experiments import compute_mmd_tmd_uhd
    from hyperpocket_amd.utils.evaluation.completion import completion_metrics
    ref = np.stack([_scan(2048, 80 + i) for i in range(4)])
    dataset = [(None, None, ref[i], i) for i in range(len(ref))]
    res = compute_mmd_tmd_uhd(None, torch.device(CUDA), dataset, str(run["dir"]), run["epoch"], 4)
    out = completion_metrics(torch.stack(run["existing"]), run["generated"], torch.from_numpy(ref).to(CUDA), batch_size=4)
    print(res, out)
    np.testing.assert_allclose(res["UHD * 100"], out["UHD"] * 100, rtol=1e-5)
    np.testing.assert_allclose(res["TMD * 100"], out["TMD"] * 100, rtol=1e-5)
    assert out["UHD"] > 0 and out["TMD"] > 0


def test_from_npy_dir_sorts_the_roles_and_restores_into_the_scene(tmp_path):
    from hyperpocket_amd.datasets.scan_dataset import DeviceScanDataset
    obj = _scan(700, 90, (3.0, -2.0, 10.0)) * np.float32(5.0)
    box, scene = _scan(8, 91), _scan(1234, 92) * np.float32(20.0)
    np.save(tmp_path / "object_0.npy", obj.astype(np.float64))     # the reference casts what it loads to float32
    np.save(tmp_path / "object_box_0.npy", box)
    np.save(tmp_path / "scene_0.npy", scene)
    data = DeviceScanDataset.from_npy_dir(str(tmp_path), device=CUDA)
    assert len(data) == 1 and data.names == ["object_0.npy"]
    assert np.array_equal(data.scan(0).cpu().numpy(), obj)
    assert np.array_equal(data.get_obj_box(0).cpu().numpy(), box) and np.array_equal(data.get_scene(0).cpu().numpy(), scene)
    center, scale = data.boxes()
    want_c, want_s = scan_law.boxes_fp32(obj)
    assert np.array_equal(center[0].cpu().numpy(), want_c) and scale[0].item() == want_s
    assert data.boxes()[0] is center                               # computed once
    completion = _scan(2048, 93) * np.float32(3.0)
    _, own = scan_law.boxes_fp32(completion)
    want = scan_law.restore_fp32(completion, own, want_c, want_s)
    got = data.inverse_scale(0, torch.from_numpy(completion).to(CUDA)).cpu().numpy()
    assert np.array_equal(got, want)
    in_scene = data.inverse_scale_to_scene(0, torch.from_numpy(completion).to(CUDA)).cpu().numpy()
    assert in_scene.shape == (1234 + 2048, 3)
    assert np.array_equal(in_scene[:1234], scene) and np.array_equal(in_scene[1234:], want)
    several = data.inverse_scale(0, torch.from_numpy(np.stack([completion, completion * np.float32(0.5)])).to(CUDA)).cpu().numpy()
    assert np.array_equal(several[0], want)
    os.makedirs(tmp_path / "nothing")
    with pytest.raises(ValueError):
        DeviceScanDataset.from_npy_dir(str(tmp_path / "nothing"), device=CUDA)

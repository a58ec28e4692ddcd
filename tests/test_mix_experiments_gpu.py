"""GPU suite for the shape-mixing and re-slicing experiments above the kernels: FullModel.encode_missing, mix_completions
against forward() and against the composition of its parts, and the directories merge_different_categories and
same_model_different_slices write — names, the law's cut of every gt, every completion from its recorded inputs."""
import copy
import os

import numpy as np
import pytest
import torch

import axis_split_law
from conftest import fixture_state_, golden

pytestmark = pytest.mark.gpu

CUDA = "cuda"
N = 64               # points per gt cloud: tiny, the decoder's 2048 is the experiments' own
AMOUNT = 2
SLICES = 2
CATS = ("car", "airplane")

# forward() on one (existing, missing) row at batch 1 and at positions 0 and 3 of a batch of AMOUNT * 2 = 4: the largest
# absolute difference between the three completions (2048 points of magnitude up to 0.32), measured on an MI355X with the
# forward() of the commit before these experiments, which they leave untouched: 0.0, for each of four rows,
# and 0.0 again against two positions of a batch of 16.  A row gathered to another place of a batch could differ from itself
# by as much, so the bound on mix_completions against forward() on the gathered rows is twice that: exact equality.
FORWARD_ACROSS_BATCHES = 0.0


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


def _record_points(model):
    """Keep every decoder-input draw of the model's sampler, in call order."""
    drawn, draw = [], model._draw_points

    def recording(*a, **kw):
        drawn.append(draw(*a, **kw))
        return drawn[-1]
    model._draw_points = recording
    return drawn


def _count_calls(module):
    calls, forward = [], module.forward
    module.forward = lambda *a, **kw: (calls.append(1), forward(*a, **kw))[1]
    return calls


def _gt(seed, stretch):
    r = np.random.RandomState(seed)
    return ((r.rand(N, 3) - 0.5) * np.asarray(stretch)).astype(np.float32)


def _dataset():
    """Two categories of (existing, missing, gt, idx) items; only gt is read."""
    return {"car": [(None, None, _gt(100 + i, (1.0, 0.4, 0.5)), i) for i in range(3)],
            "airplane": [(None, None, _gt(200 + i, (0.6, 0.2, 1.0)), i) for i in range(4)]}


def _halves(rows, seed0):
    """(existing (rows, N/2, 3), missing (rows, N/2, 3)) on the device: the law's cut of `rows` gt clouds."""
    cut = [axis_split_law.split(_gt(seed0 + r, (1.0, 0.5, 0.7)), N // 2, 0) for r in range(rows)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(CUDA)
    return dev(np.stack([c[1] for c in cut])), dev(np.stack([c[0] for c in cut]))


def _compose(model, existing, missing, pairs, points, epoch):
    """The completions of `pairs` in one decoder batch, from the model's own entry points."""
    pairs = torch.as_tensor(pairs, device=CUDA)
    with torch.no_grad():
        code, mean = model.encode_existing(existing), model.encode_missing(missing)
        return model.sample_completions(None, mean[pairs[:, 1]], 2048, epoch, code=code[pairs[:, 0]], points=points)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def test_encode_missing_is_the_vae_encoders_mean():
    from hyperpocket_amd.model.full_model import FullModel
    model, gm = trained_model()
    _, missing = _halves(5, 300)
    kept = missing.clone()
    with torch.no_grad():
        got = model.encode_missing(missing)
        want = model.random_encoder(missing.transpose(1, 2))[1]
    assert got.shape == (5, model.get_noise_size()) and torch.equal(got, want)
    assert missing.shape == kept.shape and torch.equal(missing, kept) and missing.is_contiguous()   # the layout stays
    with pytest.raises(ValueError):
        model.encode_missing(missing.transpose(1, 2))
    model.train()
    with pytest.raises(RuntimeError):
        model.encode_missing(missing)
    cfg = {"random_encoder": {"output_size": 0, "use_bias": True, "relu_slope": 0.2},
           "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
           "hyper_network": {"use_bias": True, "relu_slope": 0.2},
           "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                              "layer_out_channels": [32, 64, 128, 64]},
           "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}
    rec = FullModel(cfg).cuda().eval()
    assert rec.mode.name == "HyperRec"
    with pytest.raises(ValueError):
        rec.encode_missing(missing)


def test_mix_completions_against_forward_and_its_own_parts():
    from hyperpocket_amd import ops
    from hyperpocket_amd.core.experiments import mix_completions
    model, gm = trained_model()
    epoch, dev = int(gm["epoch"]), torch.device(CUDA)
    existing, missing = _halves(4, 400)
    # pairs (i, i): the same batch through the same kernels as forward() -> the same bits
    points = ops.sample_points(4, 2048, 1.0, 77, 1, CUDA)
    diagonal = [(i, i) for i in range(4)]
    got = mix_completions(model, existing, missing, diagonal, 2048, epoch, points=points)
    with torch.no_grad():
        want = model(existing.clone(), missing.clone(), [4, 2048, 3], epoch, dev, points=points)
    assert got.shape == (4, 3, 2048) and torch.equal(got, want)
    # arbitrary pairs, a missing part of its own row count: the composition of the entry points, bit for bit
    _, other = _halves(3, 500)
    pairs = [(i, j) for i in range(4) for j in range(3)] + [(3, 0), (0, 2), (0, 2)]
    points = ops.sample_points(len(pairs), 2048, 1.0, 78, 1, CUDA)
    points[14] = points[13]                                        # the pair (0, 2) twice, under the same decoder input
    got = mix_completions(model, existing, other, torch.tensor(pairs), 2048, epoch, points=points)
    assert got.shape == (15, 3, 2048)
    assert torch.equal(got, _compose(model, existing, other, pairs, points, epoch))
    assert torch.equal(got[13], got[14]) and not torch.equal(got[0], got[1])
    # forward() on the gathered rows: every row at another place of another batch
    rows = torch.tensor(pairs, device=CUDA)
    with torch.no_grad():
        want = model(existing[rows[:, 0]].clone(), other[rows[:, 1]].clone(), [15, 2048, 3], epoch, dev, points=points)
    worst = (got - want).abs().max().item()
    print("mix_completions against forward() on the gathered rows: largest absolute difference", worst,
          "bound", 2 * FORWARD_ACROSS_BATCHES)
    assert worst <= 2 * FORWARD_ACROSS_BATCHES
    # without injected points the model's sampler draws, once per chunk of SAMPLE_CHUNK pairs
    drawn = _record_points(model)
    many = [(i % 4, i % 3) for i in range(70)]
    got = mix_completions(model, existing, other, many, 2048, epoch)
    assert [tuple(d.shape) for d in drawn] == [(64, 2048, 3), (6, 2048, 3)] and got.shape == (70, 3, 2048)
    assert torch.equal(got[:64], _compose(model, existing, other, many[:64], drawn[0], epoch))
    assert torch.equal(got[64:], _compose(model, existing, other, many[64:], drawn[1], epoch))
    with pytest.raises(ValueError):
        mix_completions(model, existing, other, [0, 1], 2048, epoch)
    model.train()
    with pytest.raises(RuntimeError):
        mix_completions(model, existing, other, pairs, 2048, epoch)


# ------------------------------------------------------------------------------------------------
# merge_different_categories
# ------------------------------------------------------------------------------------------------
def _merge(results_dir, as_reference):
    from hyperpocket_amd.core.experiments import merge_different_categories
    model, gm = trained_model()
    drawn = _record_points(model)
    calls = {name: _count_calls(getattr(model, name)) for name in ("real_encoder", "random_encoder")}
    model.train()                                                  # the flag must come back as it was
    np.random.seed(11)
    parts, recs = merge_different_categories(model, torch.device(CUDA), _dataset(), str(results_dir), int(gm["epoch"]),
                                             amount=AMOUNT, first_cat=CATS[0], second_cat=CATS[1], as_reference=as_reference)
    assert model.training
    return {"dir": results_dir / "merge_different_categories", "model": model.eval(), "epoch": int(gm["epoch"]), "drawn": drawn,
            "calls": calls, "parts": parts, "recs": recs}


@pytest.fixture(scope="module")
def merged(tmp_path_factory):
    """One run per value of as_reference, the second into the first one's directory; shared and left unchanged."""
    results_dir = tmp_path_factory.mktemp("results")
    os.makedirs(results_dir / "merge_different_categories" / "stale")          # must be cleared
    slip = _merge(results_dir, True)
    slip["files"] = {name: np.load(slip["dir"] / name) for name in os.listdir(slip["dir"])}
    (results_dir / "merge_different_categories" / "car_9_gt.npy").write_bytes(b"x")
    return {"slip": slip, "ours": _merge(results_dir, False)}


def _pair_rows(as_reference):
    return [(a * AMOUNT + i, (0 if as_reference and a == b == 1 else b) * AMOUNT + j)
            for a in range(2) for b in range(2) for i in range(AMOUNT) for j in range(AMOUNT)]


def test_merge_writes_the_protocols_names_and_the_laws_cuts(merged):
    run = merged["ours"]
    names = sorted(os.listdir(run["dir"]))
    want = sorted([f"{cat}_{i}_{kind}.npy" for cat in CATS for i in range(AMOUNT) for kind in ("existing", "missing", "gt")]
                  + [f"{a}_{i}~{b}_{j}_rec.npy" for a in CATS for b in CATS for i in range(AMOUNT) for j in range(AMOUNT)])
    assert names == want == sorted(merged["slip"]["files"])        # nothing stale after the second run, nothing missing
    np.random.seed(11)
    data = _dataset()
    ids = [np.random.choice(len(data[cat]), AMOUNT, replace=False) for cat in CATS]        # the second from its own length
    for c, cat in enumerate(CATS):
        for i in range(AMOUNT):
            gt = np.load(run["dir"] / f"{cat}_{i}_gt.npy")
            assert gt.dtype == np.float32 and np.array_equal(gt, data[cat][ids[c][i]][2])
            lower, upper, _ = axis_split_law.split(gt, N // 2, 0)
            existing, missing = np.load(run["dir"] / f"{cat}_{i}_existing.npy"), np.load(run["dir"] / f"{cat}_{i}_missing.npy")
            assert existing.shape == missing.shape == (N // 2, 3)
            assert np.array_equal(_bits(existing), _bits(upper)) and np.array_equal(_bits(missing), _bits(lower))
            assert np.array_equal(upper, gt[gt.T[0].argsort()[N // 2:]]) and np.array_equal(lower, gt[gt.T[0].argsort()[:N // 2]])
            for kind, on_disk in (("gt", gt), ("existing", existing), ("missing", missing)):
                assert np.array_equal(_bits(run["parts"][kind][c, i]), _bits(on_disk))
    assert {k: tuple(v.shape) for k, v in run["parts"].items()} == {
        "existing": (2, AMOUNT, N // 2, 3), "missing": (2, AMOUNT, N // 2, 3), "gt": (2, AMOUNT, N, 3)}
    assert all(v.is_cuda for v in run["parts"].values())


def test_merge_runs_each_encoder_once(merged):
    for run in merged.values():
        assert {name: len(c) for name, c in run["calls"].items()} == {"real_encoder": 1, "random_encoder": 1}
        assert len(run["drawn"]) == 1 and tuple(run["drawn"][0].shape) == (4 * AMOUNT ** 2, 2048, 3)     # one decoder batch


def test_merge_completions_are_the_composition_of_their_files(merged):
    fresh, _ = trained_model()
    for key, as_reference in (("ours", False), ("slip", True)):
        run = merged[key]
        load = (lambda name: np.load(run["dir"] / name)) if key == "ours" else (lambda name: run["files"][name])
        stack = lambda kind: torch.from_numpy(np.stack([load(f"{cat}_{i}_{kind}.npy") for cat in CATS for i in range(AMOUNT)])).to(CUDA)
        existing, missing = stack("existing"), stack("missing")
        assert run["recs"].shape == (2, 2, AMOUNT, AMOUNT, 2048, 3) and run["recs"].is_cuda
        want = _compose(fresh, existing, missing, _pair_rows(as_reference), run["drawn"][0], run["epoch"])
        want = want.permute(0, 2, 1).reshape(2, 2, AMOUNT, AMOUNT, 2048, 3)
        assert torch.equal(run["recs"], want)
        for a in range(2):
            for b in range(2):
                for i in range(AMOUNT):
                    for j in range(AMOUNT):
                        rec = load(f"{CATS[a]}_{i}~{CATS[b]}_{j}_rec.npy")
                        assert rec.shape == (2048, 3) and rec.dtype == np.float32
                        assert np.array_equal(_bits(rec), _bits(want[a, b, i, j])), (key, a, b, i, j)
        # second~second under the points it was decoded with: the first category's missing parts with the reference's slip
        # (what second~first holds, up to the decoder's points), the second's own without it
        other = _compose(fresh, existing, missing, _pair_rows(not as_reference), run["drawn"][0], run["epoch"])
        other = other.permute(0, 2, 1).reshape(2, 2, AMOUNT, AMOUNT, 2048, 3)
        assert torch.equal(other[:, 0], want[:, 0]) and torch.equal(other[0, 1], want[0, 1])
        for i in range(AMOUNT):
            for j in range(AMOUNT):
                assert not torch.equal(other[1, 1, i, j], want[1, 1, i, j])
    # the same points for second~first and second~second: equal files with the slip, different ones without it
    points = merged["ours"]["drawn"][0][:AMOUNT ** 2].repeat(4, 1, 1)
    for as_reference in (True, False):
        recs = _compose(fresh, existing, missing, _pair_rows(as_reference), points, merged["ours"]["epoch"])
        recs = recs.view(2, 2, AMOUNT ** 2, 3, 2048)
        assert torch.equal(recs[1, 1], recs[1, 0]) == as_reference


def test_merge_refuses_a_category_that_is_too_small(tmp_path):
    from hyperpocket_amd.core.experiments import merge_different_categories
    model, gm = trained_model()
    with pytest.raises(ValueError):
        merge_different_categories(model, torch.device(CUDA), _dataset(), str(tmp_path), int(gm["epoch"]), amount=4,
                                   first_cat=CATS[0], second_cat=CATS[1])


# ------------------------------------------------------------------------------------------------
# same_model_different_slices
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sliced(tmp_path_factory):
    from hyperpocket_amd.core.experiments import same_model_different_slices
    results_dir = tmp_path_factory.mktemp("results")
    os.makedirs(results_dir / "same_model_different_slices" / "stale")         # must be cleared
    model, gm = trained_model()
    drawn = _record_points(model)
    calls = _count_calls(model.real_encoder)
    np.random.seed(5)
    torch.manual_seed(17)
    recs = same_model_different_slices(model, torch.device(CUDA), _dataset(), str(results_dir), int(gm["epoch"]), amount=AMOUNT,
                                       slices_number=SLICES, std=0.2, seed=9)
    assert not model.training
    return {"dir": results_dir / "same_model_different_slices", "epoch": int(gm["epoch"]), "drawn": drawn, "calls": calls,
            "recs": recs, "noise_size": model.get_noise_size()}


def test_slices_write_the_protocols_names_and_partition_each_gt(sliced):
    from hyperpocket_amd import ops
    d = sliced["dir"]
    want = [f"{cat}_{i}_gt.npy" for cat in CATS for i in range(AMOUNT)]
    want += [f"{cat}_{i}_{j}_{side}_{kind}.npy" for cat in CATS for i in range(AMOUNT) for j in range(SLICES) for side in "fs"
             for kind in ("pcd", "noise", "rec")]
    assert sorted(os.listdir(d)) == sorted(want)
    np.random.seed(5)
    data, item = _dataset(), 0
    for cat in CATS:
        ids = np.random.choice(len(data[cat]), AMOUNT, replace=False)
        for i in range(AMOUNT):
            gt = np.load(d / f"{cat}_{i}_gt.npy")
            assert np.array_equal(gt, data[cat][ids[i]][2])
            cloud = torch.from_numpy(gt).to(CUDA)
            first, second, plane = ops.slice_clouds(cloud.expand(SLICES, -1, -1), N // 2, seed=9 + item)
            plane = plane.cpu().numpy().astype(np.float64)
            assert len({tuple(p) for p in plane.tolist()}) == SLICES           # the cuts of an item differ
            for j in range(SLICES):
                f, s = np.load(d / f"{cat}_{i}_{j}_f_pcd.npy"), np.load(d / f"{cat}_{i}_{j}_s_pcd.npy")
                assert f.shape == s.shape == (N // 2, 3)
                assert np.array_equal(f, first[j].cpu().numpy()) and np.array_equal(s, second[j].cpu().numpy())
                assert sorted(map(tuple, np.concatenate([f, s]).tolist())) == sorted(map(tuple, gt.tolist()))
                side = lambda p: p.astype(np.float64) @ plane[j, :3] + plane[j, 3]
                vf, vs = side(f), side(s)
                vf, vs = vf[np.abs(vf) > 1e-5], vs[np.abs(vs) > 1e-5]          # fp32 classification: points on the plane aside
                assert len(vf) > N // 4 and len(vs) > N // 4
                assert (np.all(vf > 0) and np.all(vs < 0)) or (np.all(vf < 0) and np.all(vs > 0))
            item += 1


def test_slices_noises_and_completions_come_from_their_files(sliced):
    d, epoch = sliced["dir"], sliced["epoch"]
    fresh, _ = trained_model()
    torch.manual_seed(17)
    item = 0
    assert sliced["recs"].shape == (2 * AMOUNT, SLICES, 2, 2048, 3) and sliced["recs"].is_cuda
    for cat in CATS:
        for i in range(AMOUNT):
            order = [(j, side) for j in range(SLICES) for side in "fs"]
            noises = [torch.empty(1, sliced["noise_size"]).normal_(mean=0.0, std=0.2) for _ in order]
            for (j, side), noise in zip(order, noises):
                on_disk = np.load(d / f"{cat}_{i}_{j}_{side}_noise.npy")
                assert on_disk.shape == (1, sliced["noise_size"]) and np.array_equal(on_disk, noise.numpy())
            parts = torch.from_numpy(np.stack([np.load(d / f"{cat}_{i}_{j}_{side}_pcd.npy") for j, side in order])).to(CUDA)
            with torch.no_grad():
                want = fresh.sample_completions(parts, torch.cat(noises).to(CUDA), 2048, epoch, points=sliced["drawn"][item])
            for r, (j, side) in enumerate(order):
                rec = np.load(d / f"{cat}_{i}_{j}_{side}_rec.npy")
                assert rec.shape == (3, 2048) and rec.dtype == np.float32
                assert np.array_equal(_bits(rec), _bits(want[r])), (cat, i, j, side)
                assert torch.equal(sliced["recs"][item, j, "fs".index(side)], want[r].t())
            item += 1
    assert len(sliced["drawn"]) == item == 2 * AMOUNT and len(sliced["calls"]) == item     # per item: one encoding, one decoding

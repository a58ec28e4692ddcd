"""GPU suite for the generativity evaluation: the occupancy-grid kernel (hp_occupancy_grid) and the JSD on it against the
reference-generated fixture (tests/golden/jsd.npz — sklearn's nearest neighbours, the reference's own functions),
FullModel.sample_completions against forward(), and core.experiments.evaluate_generativity against a recomputation from
the public pieces.

Bars: the histograms are integers and must EQUAL the fixture's (the fixture proves it holds no tie between the two
nearest centres); entropy and JSD are fp64 sums of at most R^3 = 21 952 terms over identical integers, worst-case
reordering error n * eps = 2.4e-12 relative, bar 1e-10; completions at the suite's standing bar for a reconstruction of the
trained fixture, 1e-5 absolute (test_model_gpu.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import fixture_state_, golden

pytestmark = pytest.mark.gpu

RESOLUTIONS = (28, 8, 13)
SETS = ("ball45", "ball50", "cube50", "sphere50", "cube60", "one_point", "n1000")


def tag(R, clip):
    return f"R{R}_{'sphere' if clip else 'cube'}"


@pytest.fixture(scope="module")
def g():
    return golden("jsd")


def counts(pclouds, R, clip):
    from hyperpocket_amd.utils.metrics import _occupancy_counts
    c, h = _occupancy_counts(pclouds, R, clip)
    assert c.dtype == np.int32 and h.dtype == np.int32
    return c.copy(), h.copy()


# ---- 1, 2: the fixture ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("R", RESOLUTIONS)
def test_histograms_equal_the_references_exactly(g, R, clip):
    from hyperpocket_amd.utils.metrics import entropy_of_occupancy_grid
    for name in SETS:
        pts = torch.from_numpy(g["set__" + name]).cuda()
        t = tag(R, clip)
        c, h = counts(pts, R, clip)
        want_c, want_h = g[f"counters__{name}__{t}"], g[f"clouds_hit__{name}__{t}"]
        print(name, t, "points placed differently:", int(np.abs(c - want_c).sum()) // 2, "hit differences:", int(np.abs(h - want_h).sum()))
        assert np.array_equal(c, want_c), (name, t)
        assert np.array_equal(h, want_h), (name, t)
        ent, counters = entropy_of_occupancy_grid(pts, R, clip)
        assert counters.dtype == np.float64 and np.array_equal(counters, want_c)
        print(name, t, "entropy", ent, float(g[f"entropy__{name}__{t}"]))
        np.testing.assert_allclose(ent, float(g[f"entropy__{name}__{t}"]), rtol=1e-10, atol=0)


def test_jsd_between_point_cloud_sets_equals_the_references(g):
    from hyperpocket_amd.utils.metrics import jsd_between_point_cloud_sets
    for a, b in zip(SETS[:4], SETS[1:5]):
        got = jsd_between_point_cloud_sets(torch.from_numpy(g["set__" + a]).cuda(), torch.from_numpy(g["set__" + b]).cuda())
        print(a, b, got, float(g[f"jsd__{a}__{b}"]))
        np.testing.assert_allclose(got, float(g[f"jsd__{a}__{b}"]), rtol=1e-10, atol=0)
    got = jsd_between_point_cloud_sets(g["set__n1000"], g["set__cube60"], 13)          # numpy in, other sizes per set
    np.testing.assert_allclose(got, float(g["jsd__n1000__cube60__R13"]), rtol=1e-10, atol=0)


# ---- 3: determinism, batching, the experiment's shape ------------------------------------------------------------------------
@pytest.mark.parametrize("R,clip", [(28, True), (13, True), (8, False)])
def test_batched_call_equals_the_sum_of_per_cloud_calls_and_itself(g, R, clip):
    pts = torch.from_numpy(np.concatenate([g["set__sphere50"], g["set__cube60"]])).cuda()
    c, h = counts(pts, R, clip)
    c2, h2 = counts(pts, R, clip)
    assert np.array_equal(c, c2) and np.array_equal(h, h2)
    assert c.sum() == pts.size(0) * pts.size(1)
    sum_c, sum_h = np.zeros_like(c), np.zeros_like(h)
    for i in range(pts.size(0)):
        ci, hi = counts(pts[i:i + 1], R, clip)
        assert set(np.unique(hi).tolist()) <= {0, 1} and np.array_equal(hi, (ci > 0).astype(np.int32))
        sum_c += ci
        sum_h += hi
    assert np.array_equal(sum_c, c) and np.array_equal(sum_h, h)


def _exhaustive_fp64(pts, grid, chunk=4096):
    """-> (index of the nearest row of `grid` per point by fp64 squared distance, smallest gap to the second nearest)."""
    p, c = pts.reshape(-1, 3).double(), grid.double()
    best, gap = [], float("inf")
    for s in range(0, p.size(0), chunk):
        q = p[s:s + chunk]
        d2 = (q[:, None, 0] - c[None, :, 0]) ** 2 + (q[:, None, 1] - c[None, :, 1]) ** 2 + (q[:, None, 2] - c[None, :, 2]) ** 2
        vals, idx = d2.topk(2, dim=1, largest=False)
        gap = min(gap, (vals[:, 1] - vals[:, 0]).min().item())
        best.append(idx[:, 0])
    return torch.cat(best), gap


def test_experiment_shape_equals_an_exhaustive_fp64_search():
    """S = 300 clouds of 1024 points on the sphere's surface, R = 28 clipped (what evaluate_generativity produces; ~60 % of
    these points need the search): against the arg-min over all 10 144 kept centres in fp64, done in torch on the GPU."""
    from hyperpocket_amd.utils.metrics import unit_cube_grid_point_cloud
    gen = torch.Generator().manual_seed(300)
    v = torch.randn(300, 1024, 3, generator=gen, dtype=torch.float64)
    pts = (0.5 * v / v.norm(dim=2, keepdim=True)).float().cuda()
    grid = torch.from_numpy(unit_cube_grid_point_cloud(28, True)[0]).cuda()
    cell, gap = _exhaustive_fp64(pts, grid)
    assert gap > 0.0, "seeded points hold an exact tie: tie-breaking is not under test"
    want_c = torch.bincount(cell, minlength=grid.size(0)).cpu().numpy()
    per_cloud = cell.view(300, 1024)
    want_h = np.zeros(grid.size(0), np.int64)
    for row in per_cloud:
        want_h[torch.unique(row).cpu().numpy()] += 1
    c, h = counts(pts, 28, True)
    print("points placed differently:", int(np.abs(c - want_c).sum()) // 2, "smallest fp64 gap", gap)
    assert np.array_equal(c, want_c) and np.array_equal(h, want_h)


def test_more_clouds_than_workgroups_and_points_in_several_passes():
    """S above the launch's workgroup cap (clouds loop inside a workgroup) and n above one 1024-point pass, at the cap R = 64."""
    from hyperpocket_amd.utils.metrics import unit_cube_grid_point_cloud
    gen = torch.Generator().manual_seed(5)
    for S, n, R in ((2500, 7, 13), (2, 2500, 64)):
        pts = (torch.rand(S, n, 3, generator=gen) * 1.2 - 0.6).cuda()
        grid = torch.from_numpy(unit_cube_grid_point_cloud(R, True)[0]).cuda()
        cell, gap = _exhaustive_fp64(pts, grid, chunk=512)
        assert gap > 0.0
        c, h = counts(pts, R, True)
        want_h = np.zeros(grid.size(0), np.int64)
        for row in cell.view(S, n):
            want_h[torch.unique(row).cpu().numpy()] += 1
        assert np.array_equal(c, torch.bincount(cell, minlength=grid.size(0)).cpu().numpy())
        assert np.array_equal(h, want_h)


# ---- 4: inputs ---------------------------------------------------------------------------------------------------------------
def test_numpy_and_tensor_inputs_agree_and_bad_inputs_raise(g):
    from hyperpocket_amd.utils.metrics import OCCUPANCY_MAX_RESOLUTION, entropy_of_occupancy_grid
    pts = g["set__cube60"]
    e_np, c_np = entropy_of_occupancy_grid(pts, 28, True)
    dev = torch.from_numpy(pts).cuda()
    before = dev.clone()
    e_t, c_t = entropy_of_occupancy_grid(dev, 28, True)
    assert e_np == e_t and np.array_equal(c_np, c_t) and torch.equal(dev, before)
    e_f64, c_f64 = entropy_of_occupancy_grid(pts.astype(np.float64), 28, True)
    assert e_f64 == e_t and np.array_equal(c_f64, c_t)
    view = torch.from_numpy(np.ascontiguousarray(pts.transpose(0, 2, 1))).cuda().permute(0, 2, 1)     # not contiguous
    assert np.array_equal(entropy_of_occupancy_grid(view, 28, True)[1], c_t)
    for bad in (float("nan"), float("inf"), -float("inf")):
        broken = dev.clone()
        broken[3, 17, 1] = bad
        with pytest.raises(ValueError):
            entropy_of_occupancy_grid(broken, 28, True)
        with pytest.raises(ValueError):
            entropy_of_occupancy_grid(broken.cpu().numpy(), 28, False)
    for R in (1, OCCUPANCY_MAX_RESOLUTION + 1):
        with pytest.raises(ValueError):
            entropy_of_occupancy_grid(dev, R, True)
    with pytest.raises(ValueError):
        entropy_of_occupancy_grid(dev[0], 28, True)          # one cloud without its set dimension
    with pytest.warns(UserWarning):
        entropy_of_occupancy_grid(dev, 28, True, verbose=True)   # cube of side 1.2: outside cube and sphere


# ---- 5: K completions of one partial cloud -----------------------------------------------------------------------------------
def model_config():
    return {"random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
            "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
            "hyper_network": {"use_bias": True, "relu_slope": 0.2},
            "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                               "layer_out_channels": [32, 64, 128, 64]},
            "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}


def trained_model():
    """The model at model_trained.npz's operating point (outputs of unit scale, not the seeded init's O(100))."""
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    gm = golden("model_trained")
    torch.manual_seed(int(gm["seed"]))
    model = FullModel(copy.deepcopy(model_config()))
    model.apply(weights_init)
    model = model.cuda()
    fixture_state_(model.state_dict(), gm)
    return model.eval(), gm


@pytest.mark.parametrize("K", [1, 5, 64, 70])
def test_sample_completions_equals_forward_on_the_repeated_cloud(K):
    from hyperpocket_amd import ops
    model, gm = trained_model()
    epoch, N = int(gm["epoch"]), 2048
    existing = torch.from_numpy(gm["existing"][1:2]).cuda()
    gen = torch.Generator().manual_seed(K)
    noise = (0.2 * torch.randn(K, model.get_noise_size(), generator=gen)).cuda()
    points = ops.sample_points(K, N, 1.0, 99, K, "cuda")
    calls = []
    encode = model.real_encoder.forward
    model.real_encoder.forward = lambda *a, **kw: (calls.append(1), encode(*a, **kw))[1]
    kept, shape, stride = existing.clone(), tuple(existing.shape), existing.stride()
    with torch.no_grad():
        got = model.sample_completions(existing, noise, N, epoch, points=points)
        assert len(calls) == 1
        assert tuple(existing.shape) == shape and existing.stride() == stride and torch.equal(existing, kept)
        want = model(existing.expand(K, -1, -1).clone(), None, [K, N, 3], epoch, torch.device("cuda"), noise=noise, points=points)
        several = model.sample_completions(existing.expand(K, -1, -1).contiguous(), noise, N, epoch, points=points)
    assert got.shape == (K, 3, N) and want.shape == (K, 3, N)
    print("K", K, "max |completion|", want.abs().max().item(), "max error", (got - want).abs().max().item())
    np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(several.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-5)
    if K > 1:           # the K rows are different completions (a spread over one row is undefined)
        assert want.std(dim=0).max().item() > 1e-3
    with torch.no_grad():
        drawn = model.sample_completions(existing, noise, N, epoch)     # the model's own sampler
    assert drawn.shape == (K, 3, N) and torch.isfinite(drawn).all()


def test_sample_completions_hypercloud_takes_the_noise_as_latent():
    from hyperpocket_amd import ops
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    cfg = model_config()
    cfg["real_encoder"]["output_size"] = 0
    torch.manual_seed(3)
    model = FullModel(cfg)
    model.apply(weights_init)
    model = model.cuda().eval()
    gen = torch.Generator().manual_seed(1)
    noise, existing = torch.randn(5, 128, generator=gen).cuda(), (torch.rand(5, 64, 3, generator=gen) - 0.5).cuda()
    points = ops.sample_points(5, 256, 1.0, 99, 1, "cuda")
    with torch.no_grad():
        got = model.sample_completions(None, noise, 256, 1, points=points)
        want = model(existing, None, [5, 256, 3], 1, torch.device("cuda"), noise=noise, points=points)
    assert torch.equal(got, want)
    with pytest.raises(RuntimeError):
        model.train().sample_completions(None, noise, 256, 1, points=points)


# ---- 6: the experiment -------------------------------------------------------------------------------------------------------
def synthetic_datasets():
    r = np.random.RandomState(11)

    def item(i, centre):
        full = (r.standard_normal((2048, 3)) * 0.12 + centre).astype(np.float32)
        order = full[:, 1].argsort()
        return full[order[1024:]][:256].copy(), full[order[:1024]].copy(), full, i     # existing, missing, gt, idx
    return {"blob": [item(i, (0.0, 0.0, 0.0)) for i in range(3)],
            "shifted": [item(i, (0.1, -0.05, 0.0)) for i in range(3)]}


def test_evaluate_generativity_equals_a_recomputation_from_the_public_pieces(tmp_path):
    from hyperpocket_amd.core.experiments import evaluate_generativity, lowest_y_half
    from hyperpocket_amd.utils.metrics import compute_all_metrics, jsd_between_point_cloud_sets
    datasets, device, batch_size, seed = synthetic_datasets(), torch.device("cuda"), 2, 77
    files = []
    for run in ("a", "b"):
        model, gm = trained_model()
        epoch = int(gm["epoch"])
        torch.manual_seed(seed)
        res = evaluate_generativity(model, device, datasets, str(tmp_path / run), epoch, batch_size, 0)
        path = tmp_path / run / "evaluate_generativity" / f"{epoch}eval_gen_by_cat.json"
        assert path.exists()
        files.append(path.read_text())
        assert json.loads(files[-1]) == res
        assert not model.training
    assert files[0] == files[1]
    res = json.loads(files[0])
    keys = {f"{k}-{d}" for k in ("mmd(Fidelity)", "cov(Coverage)", "mmd_smp") for d in ("CD", "EMD")} | {"jsd"}
    assert set(res) == set(datasets) and all(set(v) == keys for v in res.values())

    # a second, identically built and seeded model: the experiment's has advanced its point sampler
    model, gm = trained_model()
    torch.manual_seed(seed)
    with torch.no_grad():
        for cat, items in datasets.items():
            cat_gt = torch.from_numpy(np.stack([it[1] for it in items])).cuda()
            K, want = len(items), {}
            for existing, _, _, _ in items:
                noise = torch.empty(K, model.get_noise_size()).normal_(mean=0.0, std=0.005).cuda()
                rec = model.sample_completions(torch.from_numpy(existing)[None].cuda(), noise, 2048, epoch)
                on_device = lowest_y_half(rec).cpu().numpy()
                picked = []
                for pc, dev_pts in zip(rec.cpu().numpy(), on_device):
                    y = np.sort(pc[1])
                    assert y[1023] < y[1024], "equal y at the cut: the selection is not defined"
                    pts = pc.T[pc[1].argsort(kind="stable")[:1024]]
                    as_set = lambda a: a[np.lexsort(a.T[::-1])]
                    assert np.array_equal(as_set(pts), as_set(dev_pts))
                    picked.append(pts)
                obj_recs = torch.from_numpy(np.stack(picked)).cuda()
                for k, v in compute_all_metrics(obj_recs, cat_gt, batch_size).items():
                    want[k] = want.get(k, 0.0) + v.item()
                want["jsd"] = want.get("jsd", 0.0) + jsd_between_point_cloud_sets(obj_recs, cat_gt)
            print(cat, res[cat], want)
            assert res[cat] == want, cat
            assert 0.0 < want["jsd"] <= K and np.isfinite(list(want.values())).all()

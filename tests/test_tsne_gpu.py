"""GPU suite of the exact t-SNE (csrc/tsne.hip): every kernel against the float64 law of tests/tsne_law.py within the bars
derived there, the bit-level promises (symmetry, zero diagonals, the update, reproducibility, the descent loop against its
own two launches), a whole run on separable clusters, FullModel.latent_and_weights and the make_tsne_reduction experiment."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import axis_split_law
import tsne_law as law
from conftest import fixture_state_, golden

pytestmark = pytest.mark.gpu

CUDA = "cuda"
NS = (2, 63, 64, 65, 130, 257)


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ distances
def _dims():
    tile, kchunk = law.plan(64, 64)
    return tile, kchunk, (1, 3, kchunk - 1, kchunk, kchunk + 1, 2 * kchunk + 1)


def _check_distances(X, D, d, kchunk):
    want = law.sqdist(_host(X))
    got = _host(D).astype(np.float64)
    bar = law.sqdist_bar(d, kchunk)
    worst = (np.abs(got - want) / np.where(want > 0, want, 1.0)).max()
    print(f"sqdist n={X.shape[0]} d={d}: worst relative error {worst / law.U:.2f} u, bar {bar / law.U:.0f} u")
    assert np.all(np.abs(got - want) <= bar * want)                # relative: an exact zero must come out as zero
    assert np.array_equal(_bits(D), _bits(D.t().contiguous())) and not _host(D).diagonal().any()


@pytest.mark.parametrize("n", sorted(set(NS) | {law.plan(64, 64)[0] - 1, law.plan(64, 64)[0] + 1}))
def test_distances_at_every_tile_and_chunk_edge(n):
    from hyperpocket_amd import ops
    tile, kchunk, dims = _dims()
    for d in dims:
        X = law.dev(law.rows(n * 1000 + d, n, d))
        D = ops.pairwise_sqdist(X)
        _check_distances(X, D, d, kchunk)
        if n > 2:
            assert _host(D)[0, 1] > 0 and _host(D)[0, n - 1] > 0   # the rows that differ in their last bits stay apart
    # a row stride above d: the same bits from a view into wider rows
    wide = torch.full((n, 2 * kchunk + 9), float("nan"), device=CUDA)
    wide[:, 4:4 + d] = X
    assert np.array_equal(_bits(ops.pairwise_sqdist(wide[:, 4:4 + d])), _bits(D))


def test_distances_over_decoder_weight_rows():
    from hyperpocket_amd import ops
    _, kchunk, _ = _dims()
    X = law.dev(law.rows(7, 65, 19011))
    D = ops.pairwise_sqdist(X)
    _check_distances(X, D, 19011, kchunk)
    assert np.array_equal(_bits(ops.pairwise_sqdist(X)), _bits(D))
    with pytest.raises(Exception):
        ops.pairwise_sqdist(X.cpu())


# ------------------------------------------------------------------------------------------------ affinities
def _affinity_case(name):
    if name == "identical":
        return law.identical_points(40), 10.0
    if name == "outlier":
        return law.duplicates_and_outlier(), 2.0
    n = int(name)
    X, _ = law.clusters(n, n, 8)
    return law.sqdist(X).astype(np.float32), (1.0 if n == 2 else min(10.0, n / 4.0))


@pytest.mark.parametrize("name", [str(n) for n in NS] + ["identical", "outlier"])
def test_affinities_hold_the_perplexity_and_match_the_law_at_their_own_beta(name):
    from hyperpocket_amd import ops
    D, perplexity = _affinity_case(name)
    n = len(D)
    P, beta, steps = ops.tsne_affinities(law.dev(D), perplexity)
    P2, beta2, steps2 = ops.tsne_affinities(law.dev(D), perplexity)
    assert np.array_equal(_bits(P), _bits(P2)) and np.array_equal(_bits(beta), _bits(beta2))
    assert np.array_equal(_host(steps), _host(steps2))
    Ph, beta, steps = _host(P).astype(np.float64), _host(beta).astype(np.float64), _host(steps)
    assert np.all(np.isfinite(Ph)) and np.all(np.isfinite(beta)) and steps.min() >= 1 and steps.max() <= law.SEARCH_STEPS
    at = law.conditional_at(D, beta)
    # part 1: the kernel's beta holds the perplexity, judged by the law; the target and the tolerance are fp32 in the kernel
    target = math.log(perplexity)
    done = steps < law.SEARCH_STEPS
    miss = np.abs(at["H"] - target)
    slack = law.SEARCH_TOL * (1 + law.U) + law.U * (abs(target) + 1)
    print(f"affinities {name}: steps {steps.min()}..{steps.max()}, worst |H - log perplexity| {miss[done].max() if done.any() else 0:.3g}, "
          f"evaluation bar {at['H_bar'].max():.3g}")
    assert np.all(miss[done] <= slack + at["H_bar"][done])
    if name == "identical":
        assert not done.any() and np.all(law.conditional(D, perplexity)[2] == law.SEARCH_STEPS)
    else:
        assert done.all()
    # part 2: P is the law's joint of the kernel's own beta
    want, bar = law.joint(at["C"]), law.joint_bar(at)
    err = np.abs(Ph - want)
    print(f"   P: worst error over its bar {np.max(err / bar):.3f}")
    assert np.all(err <= bar)
    assert np.array_equal(_bits(P), _bits(P.t().contiguous())) and not Ph.diagonal().any()
    assert abs(Ph.sum() - 1.0) <= n * n * law.U


# ------------------------------------------------------------------------------------------------ gradient
def _synthetic_P(seed, n):
    r = np.random.RandomState(seed)
    P = r.rand(n, n) ** 4
    P = P + P.T
    P[r.rand(n, n) < 0.2] = 0.0
    P = np.maximum(P / P.sum(), law.EPS64)
    np.fill_diagonal(P, 0.0)
    return P.astype(np.float32)


_ROWS, _LANES = law.GRAD_ROWS, law.GRAD_LANES             # rows per workgroup, lanes per row
GRADIENT_CASES = [(n, kind) for n in (2, _ROWS - 1, _ROWS, _ROWS + 1, _LANES - 1, _LANES, _LANES + 1, 130)
                  for kind in ("small", "unit")] + \
                 [(65, "coincident"), (law.GRAD_STAGE + 1, "unit")]


@pytest.mark.parametrize("n,kind", GRADIENT_CASES)
def test_gradient_z_and_kl_within_their_bars(n, kind):
    from hyperpocket_amd.utils.tsne import tsne_gradient
    r = np.random.RandomState(n)
    Y = (r.randn(n, 2) * (1e-4 if kind == "small" else 1.0)).astype(np.float32)
    if kind == "coincident":
        Y[7] = Y[3]
        Y[64] = Y[0]
    P = _synthetic_P(n + 1, n)
    for ex in ((1.0, 12.0) if n <= 256 else (1.0,)):          # the staging seam once: its law is the slow part
        want = law.gradient(P, Y, ex)
        Pd, Yd = law.dev(P), law.dev(Y)
        kept = Yd.clone()
        got = tsne_gradient(Pd, Yd, ex, kl=True)
        assert torch.equal(Yd, kept)
        plain = tsne_gradient(Pd, Yd, ex)
        assert plain.Z is None and plain.kl is None and np.array_equal(_bits(plain.grad), _bits(got.grad))
        g = _host(got.grad).astype(np.float64)
        bar = law.gradient_bar(n) * want["A"] + n * law.TINY
        err = np.abs(g - want["g"])
        print(f"gradient n={n} {kind} ex={ex}: worst error over its bar {np.max(err / bar):.3f}; "
              f"Z {abs(got.Z.item() - want['Z']) / want['Z'] / law.z_bar(n):.3f} of its bar; "
              f"KL {abs(got.kl.item() - want['kl'] * 1.0) / law.kl_bar(want, n):.3f} of its bar")
        assert np.all(err <= bar)
        assert abs(got.Z.item() - want["Z"]) <= law.z_bar(n) * want["Z"]
        if ex == 1.0:
            assert abs(got.kl.item() - want["kl"]) <= law.kl_bar(want, n)


# ------------------------------------------------------------------------------------------------ update
def test_update_is_the_laws_float32_update_bit_for_bit():
    from hyperpocket_amd import ops
    r = np.random.RandomState(3)
    n = 300                                                        # more than one workgroup
    g = (r.randn(n, 2) * 10.0 ** r.uniform(-6, 2, (n, 2))).astype(np.float32)
    upd = (r.randn(n, 2) * 10.0 ** r.uniform(-6, 0, (n, 2))).astype(np.float32)
    gains = r.uniform(0.005, 3.0, (n, 2)).astype(np.float32)
    Y = r.randn(n, 2).astype(np.float32)
    g[:9, 0], upd[5:14, 0], g[20], upd[21] = 0, 0, -0.0, -0.0
    rowacc = np.zeros((n, 8), np.float32)
    rowacc[:, 0:2] = g / np.float32(4)                             # exact, and 4 (a - 0 / Z) gives g back
    rowacc[:, 4] = 1
    for momentum, lr in ((0.5, 200.0), (0.8, 50.0)):
        Yd, ud, gd, grad = law.dev(Y), law.dev(upd), law.dev(gains), torch.empty(n, 2, device=CUDA)
        ops.tsne_update(law.dev(rowacc), Yd, ud, gd, momentum, lr, grad=grad)
        Y1, u1, g1 = law.update(g, upd, gains, Y, momentum, lr)
        assert np.array_equal(_bits(grad)[g != 0], g.view(np.uint32)[g != 0]) and not _host(grad)[g == 0].any()
        assert np.array_equal(_bits(gd), g1.view(np.uint32))
        assert np.array_equal(_bits(ud), u1.view(np.uint32)) and np.array_equal(_bits(Yd), Y1.view(np.uint32))
    with pytest.raises(Exception):
        ops.tsne_update(law.dev(rowacc), Yd, ud, gd[:5], 0.5, 1.0)


# ------------------------------------------------------------------------------------------------ descent
@pytest.fixture(scope="module")
def cluster_run():
    """Shared and left unchanged: three clusters, their law P (fp32) and a start."""
    X, labels = law.clusters(11, 97, 16)
    D = law.sqdist(X).astype(np.float32)
    P = law.joint(law.conditional(D, 10.0)[0]).astype(np.float32)
    Y0 = (np.random.RandomState(12).randn(97, 2) * 1e-4).astype(np.float32)
    return {"X": X, "labels": labels, "P": P, "Y0": Y0}


def test_descend_is_its_two_launches_reproducible_and_near_the_law(cluster_run):
    from hyperpocket_amd import ops
    P, Y0 = cluster_run["P"], cluster_run["Y0"]
    n, iters, explore, ex, lr = len(Y0), 5, 2, 12.0, 200.0
    Pd = law.dev(P)
    runs = []
    for _ in range(2):
        Y = law.dev(Y0)
        upd, gains, rowacc = ops.tsne_state(Y)
        kl = torch.zeros(3, device=CUDA)
        ops.tsne_descend(Pd, Y, upd, gains, rowacc, 0, iters, explore, ex, lr, kl=kl)
        runs.append((Y, upd, gains, kl))
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b))
    Y = law.dev(Y0)
    upd, gains, rowacc = ops.tsne_state(Y)
    for it in range(iters):
        e, momentum = law.schedule(it, explore, ex)
        ops.tsne_gradient_rows(Pd, Y, e, rowacc=rowacc)
        ops.tsne_update(rowacc, Y, upd, gains, momentum, lr)
    for a, b in zip(runs[0][:3], (Y, upd, gains)):
        assert np.array_equal(_bits(a), _bits(b))
    # two halves of the loop continue each other
    Yh = law.dev(Y0)
    uh, gh, rh = ops.tsne_state(Yh)
    ops.tsne_descend(Pd, Yh, uh, gh, rh, 0, 3, explore, ex, lr)
    ops.tsne_descend(Pd, Yh, uh, gh, rh, 3, 2, explore, ex, lr)
    assert np.array_equal(_bits(Yh), _bits(Y))
    # the law: fp64 state, fp32 state, and the kernel's place between them (profiles/tsne_parity.md)
    trace = []
    Y64 = law.descend(P, Y0, iters, explore, ex, lr, trace=trace)
    Y32 = law.descend(P, Y0, iters, explore, ex, lr, dtype=np.float32).astype(np.float64)
    got = _host(Y).astype(np.float64)
    scale = np.abs(Y64).max()
    d32, dk = np.abs(Y32 - Y64).max() / scale, np.abs(got - Y64).max() / scale
    # What one iteration injects into the state.  The fp32-state law: u on Y for the add that moves it, and u each for g's
    # conversion, g gains and lr (g gains): u (max |Y| + 3 lr gains |g|).  The kernels: the same, and their gradient's
    # error lr gains gradient_bar A on top.  First-order errors travel through the same dynamics, so the kernels may
    # stand 1 + the largest ratio of the two injections further from the fp64 trajectory than the fp32-state law does.
    margin = 1 + max(lr * gains * law.gradient_bar(n) * A / (law.U * (ymax + 3 * lr * gains * g)) for ymax, A, gains, g in trace)
    print(f"descent after {iters} iterations, of max |Y|: fp32-state law {d32:.3g}, kernels {dk:.3g}, margin {margin:.1f}")
    assert dk <= margin * d32
    want = law.gradient(P, got)
    assert abs(runs[0][3][0].item() - want["kl"]) <= law.kl_bar(want, n)


@pytest.mark.parametrize("n,init", [(97, "pca"), (193, "random")])
def test_whole_run_separates_three_clusters(n, init):
    from hyperpocket_amd.utils.tsne import initial_embedding, tsne
    from hyperpocket_amd import ops
    X, labels = law.clusters(20 + n, n, 16)
    Xd = law.dev(X)
    out = tsne(Xd, perplexity=10.0, max_iter=500, init=init, seed=4)
    again = tsne(Xd, perplexity=10.0, max_iter=500, init=init, seed=4)
    assert np.array_equal(_bits(out.embedding), _bits(again.embedding)) and np.array_equal(_bits(out.kl), _bits(again.kl))
    Y = _host(out.embedding).astype(np.float64)
    assert np.all(np.isfinite(Y)) and _host(out.steps).max() < law.SEARCH_STEPS
    D = ops.pairwise_sqdist(Xd)
    Y0 = _host(initial_embedding(init, n, D, 4, Xd.device))
    P = law.joint(law.conditional_at(_host(D), _host(out.beta))["C"]).astype(np.float32)
    kl0, kl1 = law.kl_of(P, Y0), law.kl_of(P, Y)
    print(f"whole run n={n} init={init}: law KL {kl0:.4f} -> {kl1:.4f} ({kl1 / kl0:.3f}), kernel's own {out.kl.item():.4f}")
    assert kl1 < 0.5 * kl0
    E = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(E, np.inf)
    assert np.array_equal(labels[E.argmin(1)], labels)


# ------------------------------------------------------------------------------------------------ model and experiment
N = 64
AMOUNT = 3
BACKGROUND = 5


def trained_model():
    """The seeded-init model brought to model_trained.npz's operating point, in eval mode (as test_mix_experiments_gpu)."""
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


def _gt(seed):
    r = np.random.RandomState(seed)
    return ((r.rand(N, 3) - 0.5) * np.asarray((1.0, 0.4, 0.5))).astype(np.float32)


def _items(seed0, count):
    items = []
    for i in range(count):
        gt = _gt(seed0 + i)
        lower, upper, _ = axis_split_law.split(gt, N // 2, 2)
        items.append((np.ascontiguousarray(upper), np.ascontiguousarray(lower), gt, i))
    return items


def test_latent_and_weights_are_forwards_bits():
    model, gm = trained_model()
    items = _items(700, 4)
    existing = law.dev(np.stack([it[0] for it in items]))
    missing = law.dev(np.stack([it[1] for it in items]))
    kept = existing.clone(), missing.clone()
    seen, hyper = [], model.hyper_network.forward
    model.hyper_network.forward = lambda *a, **kw: (seen.append(hyper(*a, **kw)), seen[-1])[1]
    with torch.no_grad():
        latent, weights = model.latent_and_weights(existing, missing)
        model(existing.clone(), missing.clone(), [4, N, 3], int(gm["epoch"]), torch.device(CUDA))
        assert latent.shape == (4, 256) and weights.shape == (4, 19011)
        assert torch.equal(latent, model._last_latent) and torch.equal(weights, seen[1]) and torch.equal(weights, seen[0])
        assert torch.equal(latent, torch.cat([model.encode_missing(missing), model.encode_existing(existing)], 1))
    for t, k in zip((existing, missing), kept):
        assert t.shape == k.shape and t.is_contiguous() and torch.equal(t, k)
    with pytest.raises(ValueError):
        model.latent_and_weights(existing.transpose(1, 2), missing)
    model.train()
    with pytest.raises(RuntimeError):
        model.latent_and_weights(existing, missing)


@pytest.fixture(scope="module")
def reduction(tmp_path_factory):
    from hyperpocket_amd.core import experiments
    results_dir = tmp_path_factory.mktemp("results")
    model, gm = trained_model()
    calls = {name: [] for name in ("real_encoder", "random_encoder")}
    for name, c in calls.items():
        module = getattr(model, name)
        module.forward = (lambda f, c: lambda *a, **kw: (c.append(a[0].shape[0]), f(*a, **kw))[1])(module.forward, c)
    embedded, real_tsne = [], experiments.tsne

    def recording(rows, **kw):
        embedded.append((rows.clone(), kw))
        return real_tsne(rows, **kw)
    experiments.tsne = recording
    data = {"car": _items(800, 5), "chair": _items(900, 2)}
    train = {"car": _items(1000, BACKGROUND)}
    model.train()
    np.random.seed(21)
    try:
        out = experiments.make_tsne_reduction(model, torch.device(CUDA), data, str(results_dir), int(gm["epoch"]),
                                              train_dataset_dict=train, amount=AMOUNT, perplexity=3.0, max_iter=40)
    finally:
        experiments.tsne = real_tsne
    assert model.training
    return {"dir": results_dir / "temp_exp", "out": out, "embedded": embedded, "calls": calls, "data": data, "train": train,
            "model": trained_model()[0]}


def test_reduction_writes_its_files_from_the_rows_it_embeds(reduction):
    d, rows = reduction["dir"], BACKGROUND + 2 * AMOUNT
    want = {"car_latent1.npy": (BACKGROUND, 256), "car_tnw1.npy": (BACKGROUND, 19011), "car_latent_tsne.npy": (rows, 2),
            "car_tnw_tsne.npy": (rows, 2), "car_latent_dist.npy": (AMOUNT,), "car_tnw_dist.npy": (AMOUNT,)}
    assert sorted(os.listdir(d)) == sorted(list(want) + ["gts"])
    assert sorted(os.listdir(d / "gts")) == [f"car_{i}.npy" for i in range(AMOUNT)]
    files = {name: np.load(d / name) for name in want}
    assert {k: v.shape for k, v in files.items()} == want and all(v.dtype == np.float32 for v in files.values())
    np.random.seed(21)
    ids = np.random.choice(5, AMOUNT, replace=False)
    model = reduction["model"]
    existing, missing = [], []
    for i in range(AMOUNT):
        gt = np.load(d / "gts" / f"car_{i}.npy")
        assert np.array_equal(gt, reduction["data"]["car"][ids[i]][2])
        for axis in (0, 1):
            lower, upper, _ = axis_split_law.split(gt, N // 2, axis)
            existing.append(upper)
            missing.append(lower)
    bg = reduction["train"]["car"]
    existing = law.dev(np.stack([it[0] for it in bg] + existing))
    missing = law.dev(np.stack([it[1] for it in bg] + missing))
    with torch.no_grad():
        latent = torch.cat([model.encode_missing(missing), model.encode_existing(existing)], 1)
        weights = model.hyper_network(latent)
    (lat_rows, lat_kw), (tnw_rows, tnw_kw) = reduction["embedded"]
    assert torch.equal(lat_rows, latent) and torch.equal(tnw_rows, weights)
    assert lat_kw["perplexity"] == tnw_kw["perplexity"] == 3.0 and lat_kw["max_iter"] == 40
    assert np.array_equal(files["car_latent1.npy"], _host(latent[:BACKGROUND]))
    assert np.array_equal(files["car_tnw1.npy"], _host(weights[:BACKGROUND]))
    # the test rows in one pass of at most 64, the background in another: each encoder once per batch
    assert reduction["calls"] == {"real_encoder": [2 * AMOUNT, BACKGROUND], "random_encoder": [2 * AMOUNT, BACKGROUND]}
    for name, e, dist in (("latent", reduction["out"][0], reduction["out"][2]), ("tnw", reduction["out"][1], reduction["out"][3])):
        emb = files[f"car_{name}_tsne.npy"]
        assert np.array_equal(emb, _host(e)) and np.all(np.isfinite(emb))
        test = emb[-2 * AMOUNT:].reshape(AMOUNT, 2, 2).astype(np.float64)
        want_dist = np.sqrt(((test[:, 0] - test[:, 1]) ** 2).sum(1))
        assert np.array_equal(files[f"car_{name}_dist.npy"], _host(dist))
        assert np.allclose(files[f"car_{name}_dist.npy"], want_dist, rtol=1e-5, atol=0)


def test_reduction_refuses_too_few_rows(tmp_path):
    from hyperpocket_amd.core.experiments import make_tsne_reduction
    model, gm = trained_model()
    data = {"car": _items(800, 5)}
    with pytest.raises(ValueError):
        make_tsne_reduction(model, torch.device(CUDA), data, str(tmp_path), int(gm["epoch"]), amount=2, perplexity=4.0)
    with pytest.raises(ValueError):
        make_tsne_reduction(model, torch.device(CUDA), data, str(tmp_path), int(gm["epoch"]), amount=6, perplexity=2.0)

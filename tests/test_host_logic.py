"""CPU suite: host-side logic that needs no GPU — module structure / state_dict compatibility with the
reference, the reference-exact point sampler, the flat parameter layout and the 2-rank (gloo)
gradient exchange with the sharded-loss semantics of SURVEY §8e."""
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sys

from conftest import ROOT, golden


def model_config(random_out=128, real_out=128):
    return {
        "random_encoder": {"output_size": random_out, "use_bias": True, "relu_slope": 0.2},
        "real_encoder": {"output_size": real_out, "use_bias": True, "relu_slope": 0.2},
        "hyper_network": {"use_bias": True, "relu_slope": 0.2},
        "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                           "layer_out_channels": [32, 64, 128, 64]},
        "target_network_input": {"constant": False,
                                 "normalization": {"enable": True, "type": "progressive", "epoch": 100}},
    }


@pytest.mark.parametrize("name", ["model_small", "model_hyperrec", "model_hypercloud"])
def test_state_dict_matches_reference_names_shapes_and_seeded_values(name, ref):
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    g = golden(name)
    torch.manual_seed(int(g["seed"]))
    m = FullModel(copy.deepcopy(model_config(int(g["random_out"]), int(g["real_out"]))))
    m.apply(weights_init)
    sd = m.state_dict()
    keys = [k[3:].replace("__", ".") for k in g if k.startswith("w__")]
    assert sorted(sd.keys()) == sorted(keys)            # reference checkpoints load unchanged
    for k, v in sd.items():
        s = g["w__" + k.replace(".", "__")]
        assert abs(v.double().sum().item() - s[0]) <= 1e-9 * max(1.0, abs(s[0])) + 1e-9, k
        assert abs(v.double().norm().item() - s[1]) <= 1e-9 * s[1] + 1e-12, k
    # mode-filtered parameters() (model/full_model.py:82-83) and the helper API
    n = sum(p.numel() for p in m.parameters())
    assert n == {"model_small": 43328515, "model_hyperrec": 42490499}.get(name, n)
    assert m.mode.has_generativity() == (name == "model_small")
    assert m.get_noise_size() == int(g["random_out"])


def test_mode_resolution_errors():
    from hyperpocket_amd.model.full_model import FullModel
    with pytest.raises(ValueError):
        FullModel(copy.deepcopy(model_config(0, 0)))


def test_reference_point_sampler_bit_exact():
    from hyperpocket_amd.utils.points import generate_points, normalization_coef
    g = golden("points")
    cfg = {"target_network_input": model_config()["target_network_input"]}
    for seed, epoch in [(5, 1), (6, 37), (7, 100), (8, 250)]:
        torch.manual_seed(seed)
        assert np.array_equal(generate_points(cfg, epoch, (2048, 3)).numpy(), g[f"seed{seed}_epoch{epoch}"])
    torch.manual_seed(9)
    assert np.array_equal(generate_points(cfg, 1, (512, 3), normalize_points=False).numpy(), g["seed9_nonorm"])
    assert normalization_coef(cfg, 1) == 0.0 and normalization_coef(cfg, 100) == 1.0 and normalization_coef(cfg, 500) == 1.0


def test_flat_parameters_layout():
    from hyperpocket_amd.model.full_model import FullModel
    from hyperpocket_amd.parallel import FlatParameters
    from hyperpocket_amd import ops
    torch.manual_seed(0)
    m = FullModel(copy.deepcopy(model_config()))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    flat = FlatParameters(m)
    assert flat.is_intact()
    # padding: 16-byte alignment per parameter + the heads' matrix padded to a multiple of 8 rows (sharded heads update)
    assert flat.total >= 43328515 and flat.total - 43328515 < 4 * len(flat.params) + 8 * 2048
    h = flat.heads
    assert h["rows"] == 19011 and h["pad_rows"] == 19016 and h["cols"] == 2048 and h["lo"] == 0
    assert all(h["pad_rows"] % w == 0 for w in (1, 2, 4, 8))
    assert flat.flat[h["rows"] * h["cols"]:h["hi"]].abs().sum().item() == 0.0        # pad rows are zero
    names = dict(zip(flat.names, flat.offsets))
    assert names["hyper_network.output.0.bias"] == h["hi"]                             # biases follow the padded matrix
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k])                 # values preserved, now views of one buffer
    # bucket order = the order backward produces gradients: heads, trunk, encoders
    assert flat.names[0].startswith("hyper_network.output") and flat.names[-1].startswith("real_encoder")
    (lo0, hi0), (lo1, hi1), (lo2, hi2) = flat.buckets
    assert lo0 == 0 and hi0 == lo1 and hi1 == lo2 and hi2 == flat.total
    assert hi0 >= 38953539                               # the heads: 90 % of the bytes
    # the registered gradient views alias the flat gradient buffer
    p = dict(m.named_parameters())["hyper_network.output.2.weight"]
    gv = ops._grad_buffer(p)
    gv.fill_(3.0)
    assert flat.grad_of("hyper_network.output.2.weight").eq(3.0).all() and flat.grad.double().sum().item() == 3.0 * p.numel()
    ops.clear_grad_views()


# --------------------------------------------------------------------------------------------- 2-rank gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, out):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "3d-point-clouds-autocomplete_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle import hyperpocket_ref as ref
    from hyperpocket_amd.parallel import FlatParameters, GradientReducer
    from hyperpocket_amd.model.full_model import FullModel
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd import ops
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    torch.manual_seed(11)
    model = FullModel(copy.deepcopy(model_config()))
    model.apply(weights_init)
    flat = FlatParameters(model)
    reducer = GradientReducer(flat)
    # global batch of 4 clouds, 2 per rank; the oracle stands in for the HIP kernels (test only)
    g = torch.Generator().manual_seed(5)
    ex, mi = torch.rand(4, 40, 3, generator=g) - 0.5, torch.rand(4, 40, 3, generator=g) - 0.5
    pts, eps = torch.rand(4, 80, 3, generator=g) * 2 - 1, torch.randn(4, 128, generator=g)
    gt = torch.cat([ex, mi], 1)
    sl = slice(rank * 2, rank * 2 + 2)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    rec, explv, mu, _ = ref.full_forward(P, ex[sl], mi[sl], pts[sl], eps[sl])
    loss = 0.05 * ref.chamfer_loss(gt[sl], rec.permute(0, 2, 1)) \
        + 0.5 * (torch.exp(explv) + torch.square(mu) - 1 - explv).sum() / (2 * world)   # KLD / GLOBAL batch
    loss.backward()
    with torch.no_grad():
        for name in flat.names:
            gr = P[name].grad
            if gr is not None:
                flat.grad_of(name).copy_(gr)
    reducer.launch(0)          # heads first (overlap order), the rest in finish()
    reducer.finish()
    if rank == 0:
        # single-process reference: the whole batch at once, reference loss (KLD / B)
        Pg = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
        loss_all, _, _, _ = ref.step_loss(Pg, ex, mi, gt, pts, eps)
        loss_all.backward()
        worst = 0.0
        for name in flat.names:
            want = Pg[name].grad
            if want is None:
                assert float(flat.grad_of(name).abs().max()) == 0.0
                continue
            err = (flat.grad_of(name) - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
            worst = max(worst, err)
        out.put(worst)
    ops.clear_grad_views()
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gradient_exchange_equals_global_batch_gradient():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    worst = out.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert worst < 2e-3, worst     # fp32 summation-order noise (incl. arg-max near-ties) only


def test_reference_train_epoch_binds_to_this_package_unmodified():
    """with the module aliases installed, the reference's own core/epoch_loops.py (read-only,
    untouched) imports this package's FullModel and drives it; without a GPU the first kernel call refuses to run
    (no CPU fallback) — which is as far as the wiring can be exercised here.  What that file needs of this package is held
    in tests/golden/reference_surface.npz (tests/golden/make_golden_reference_surface.py): every `from module import name`
    it makes, the number of positional arguments of its model calls and the attributes it reads off the model; a fresh
    interpreter with the aliases resolves every import to this package, and the model, called that way, refuses."""
    import subprocess
    import sys
    with np.load(os.path.join(ROOT, "tests", "golden", "reference_surface.npz")) as g:
        imports = [str(x) for x in g["loop_imports"]]
        arity = sorted({int(x) for x in g["loop_forward_arity"]})
        attrs = [str(x) for x in g["loop_model_attrs"]]
    assert "model.full_model:FullModel" in imports and arity == [5] and attrs
    code = r"""
import sys, importlib, copy, operator, torch
sys.dont_write_bytecode = True
sys.path.insert(0, %r); sys.path.insert(0, %r)
aliases = {
        "model.full_model": "hyperpocket_amd.model.full_model", "model.encoder": "hyperpocket_amd.model.encoder",
        "model.hyper_network": "hyperpocket_amd.model.hyper_network", "model.target_network": "hyperpocket_amd.model.target_network",
        "losses.champfer_loss": "hyperpocket_amd.losses.champfer_loss", "utils.points": "hyperpocket_amd.utils.points"}
for ref_name, amd_name in aliases.items():
    sys.modules[ref_name] = importlib.import_module(amd_name)
from hyperpocket_amd.model.full_model import FullModel
from hyperpocket_amd.losses.champfer_loss import ChamferLoss
from hyperpocket_amd import HipExtensionError
bound = {}
for spec in %r:                                   # the reference file's `from module import name` statements
    module, name = spec.split(":")
    bound[name] = getattr(importlib.import_module(module), name)
    if module in aliases:
        assert sys.modules[module].__name__ == aliases[module], module
assert bound["FullModel"] is FullModel
sys.path.insert(0, %r)
from test_host_logic import model_config
m = FullModel(copy.deepcopy(model_config()))
for attr in %r:                                   # what the loop reads off the model
    assert callable(operator.attrgetter(attr)(m)), attr
m.train()
opt, rec_loss = torch.optim.Adam(m.parameters(), lr=1e-4), ChamferLoss()
ex, mi = torch.rand(2, 16, 3), torch.rand(2, 16, 3)
gt, device = torch.cat([ex, mi], 1), torch.device("cpu")
opt.zero_grad()
args = (ex.to(device), mi.to(device), list(gt.shape), 1, device)
assert len(args) == %d                            # the loop's call: model(existing, missing, list(gt.shape), epoch, device)
try:
    m(*args)
except HipExtensionError as e:
    print("REFUSED:", str(e)[:60])
else:
    raise SystemExit("a CPU fallback ran")
""" % (ROOT, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"), imports, os.path.dirname(os.path.abspath(__file__)),
       attrs, arity[0])
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "REFUSED:" in out.stdout


def _bench_launcher(env_extra, *flags):
    import json
    import subprocess
    # gloo on any machine: on a GPU box the ranks would otherwise pick RCCL and want a device each
    env = dict(os.environ, HP_BENCH_BACKEND="gloo", **env_extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], env=env, capture_output=True, text=True,
                       timeout=600)
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    return r.returncode, lines


def test_bench_gpus_n_spawns_n_ranks_and_reports_them():
    """bench.py --gpus N outside torchrun starts N rank processes itself (the driver runs plain
    `python bench.py --gpus 8`).  --rendezvous-only stops after the group's first all-reduce, so this runs without a GPU
    (gloo); tests/test_dp_gpu.py runs the real step through the same launcher."""
    rc, lines = _bench_launcher({}, "--gpus", "2", "--rendezvous-only")
    assert rc == 0 and len(lines) == 1
    assert lines[0]["n_gpus"] == 2 and lines[0]["rccl_ranks"] == 2 and lines[0]["allreduce_sum"] == 3.0
    rc, lines = _bench_launcher({}, "--gpus", "3", "--rendezvous-only")
    assert rc == 0 and lines[0]["n_gpus"] == 3 and lines[0]["allreduce_sum"] == 6.0


def test_bench_launcher_fails_when_a_rank_fails():
    rc, _ = _bench_launcher({"HP_BENCH_FAIL_RANK": "1"}, "--gpus", "2", "--rendezvous-only")
    assert rc != 0


def test_engine_hooks_are_weak_and_move_to_the_latest_engine():
    """The model holds only weak references to its TrainEngine: a second engine on the same model takes the hooks over
    (the first one's state_dict hook is removed), and a dropped engine leaves no-op hooks behind instead of staying
    pinned with its flat buffers."""
    import copy
    import gc
    import bench
    from hyperpocket_amd import ops
    from hyperpocket_amd.core.engine import TrainEngine
    from hyperpocket_amd.model.full_model import FullModel
    try:
        m = FullModel(copy.deepcopy(bench.MODEL_CFG))
        a = TrainEngine(m, fuse_heads_adam=False)
        b = TrainEngine(m, fuse_heads_adam=False)
        assert a._sd_hook is None and m._engine_ref() is b
        a.close()                                   # idempotent, and does not detach the current owner
        assert m._engine_ref() is b
        del a, b
        gc.collect()
        assert m._engine_ref() is None
        m._pre_hypernet_hook()                      # no-ops now
        assert len(m.state_dict()) > 0
    finally:
        ops.clear_grad_views()


def test_bench_counts_gpus_without_touching_hip(monkeypatch):
    import bench
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1,5")
    assert bench.visible_gpus() == 3
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    assert bench.visible_gpus() == 0
    monkeypatch.delenv("HIP_VISIBLE_DEVICES")
    for var in ("ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    assert bench.visible_gpus() in (None, 0) or bench.visible_gpus() >= 0     # sysfs, or unknown: never a HIP call


def _engine_worker(rank, world, port, out):
    """A 3-rank gloo group on CPU: 19016 padded head rows do not divide by 3, so the engine must fall back from the
    row-sharded heads update (HeadsShard) to the flat all-reduce — and that all-reduce must sum over the three ranks."""
    import torch.distributed as dist
    import copy
    from hyperpocket_amd import ops
    from hyperpocket_amd.core.engine import HeadsShard, TrainEngine
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    torch.manual_seed(100 + rank)                     # different weights per rank: the constructor must broadcast rank 0's
    model = FullModel(copy.deepcopy(model_config()))
    model.apply(weights_init)
    eng = TrainEngine(model)
    ok = eng.exchange and eng.shard is None and eng.fused is None and not HeadsShard.usable(eng.flat, world)
    first = eng.flat.flat[:1000].clone()
    gathered = [torch.empty_like(first) for _ in range(world)]
    dist.all_gather(gathered, first)
    ok = ok and all(torch.equal(gathered[0], t) for t in gathered)
    eng.flat.grad.fill_(float(rank + 1))
    eng.reducer.launch_all()
    eng.reducer.finish()
    ok = ok and bool((eng.flat.grad == float(sum(range(1, world + 1)))).all())
    if rank == 0:
        out.put(ok)
    ops.clear_grad_views()
    dist.barrier()
    dist.destroy_process_group()


def test_world_sizes_that_do_not_divide_the_heads_rows_fall_back_to_all_reduce():
    import copy
    from hyperpocket_amd import ops
    from hyperpocket_amd.core.engine import HeadsShard
    from hyperpocket_amd.model.full_model import FullModel
    from hyperpocket_amd.parallel import FlatParameters
    try:
        flat = FlatParameters(FullModel(copy.deepcopy(model_config())))
        assert flat.heads["rows"] == 19011 and flat.heads["pad_rows"] == 19016
        assert [w for w in range(1, 9) if HeadsShard.usable(flat, w)] == [1, 2, 4, 8]
    finally:
        ops.clear_grad_views()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_engine_worker, args=(r, 3, port, out)) for r in range(3)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    assert out.get(timeout=10)


# ------------------------------------------------------------------ deferred hypernetwork updates under DP (world 2 and 4, gloo)
def _cpu_adam(p, g, m, v, lr, b1, b2, eps, step, grad_scale=1.0):
    """torch.optim.Adam's update on flat CPU tensors — TEST SCAFFOLDING standing in for hp_adam_step (the engine's host logic
    under test never looks at the arithmetic; there is no GPU here)."""
    g = g * grad_scale
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p.addcdiv_(m, (v.sqrt() / bc2 ** 0.5).add_(eps), value=-lr / bc1)


def _deferred_worker(rank, world, port, out):
    try:
        _deferred_worker_body(rank, world, port, out)
    except BaseException:
        import traceback
        out.put((rank, traceback.format_exc()[-1500:]))
        raise


def _close_w(a, b):
    """Weights after Adam steps: equal up to rounding, except where a gradient component is of the order of eps — there the update
    is sign-like and two summation orders of the same gradient move single entries by up to ~lr (a handful in 43 M)."""
    d = (a - b).abs()
    return float((d > 1e-7 + 1e-5 * b.abs()).float().mean()) <= 1e-5 and float(d.max()) <= 2.5e-5       # (a stale shard: a quarter of the rows off by ~lr = 1e-4)


def _chk(checks, k, v):
    checks.append((k, bool(v)))
    return bool(v)


def _deferred_worker_body(rank, world, port, out):
    """One rank of a gloo group driving TrainEngine's multi-rank bookkeeping by hand (the kernels replaced by CPU stand-ins):
    after the exchange of a step has been LAUNCHED — sharded heads rows updated and their all-gather in flight, the trunk's
    all-reduce in flight, only the encoders' bucket waited for — a reader of the parameters (`model.state_dict()`) or of the
    optimiser state (`engine.optimizer_state_dict()`) must see the COMPLETED step on every rank: no stale rows of another
    rank's shard, no un-reduced trunk gradient."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "3d-point-clouds-autocomplete_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from hyperpocket_amd import ops
    from hyperpocket_amd.core import engine as engine_mod
    from hyperpocket_amd.core.engine import TrainEngine
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    torch.manual_seed(3)
    model = FullModel(copy.deepcopy(model_config()))
    model.apply(weights_init)
    eng = TrainEngine(model)
    checks = []
    ok = eng.exchange and eng.shard is not None and eng.world == world
    engine_mod.ops.adam_step = _cpu_adam                       # (module attribute the engine calls; restored by process exit)
    flat, sh = eng.flat, eng.shard

    def heads_rows(dth_all, t5_all, r0, rows, lo, hi):         # stand-in for hp_hypernet_heads_dw_adam
        gW = (dth_all[:, r0:r0 + rows].t() @ t5_all).reshape(-1)
        _cpu_adam(flat.flat[lo:hi], gW, eng.exp_avg[lo:hi], eng.exp_avg_sq[lo:hi], eng.lr, eng.betas[0], eng.betas[1], eng.eps,
                  eng._adam_step)
    eng._adam_heads_rows = heads_rows
    sh.adam_rows = heads_rows                                  # (HeadsShard holds the bound method it was built with)
    B = 2
    w0 = flat.flat.clone()
    want_m = torch.zeros_like(flat.flat)
    want_v = torch.zeros_like(flat.flat)
    want_w = w0.clone()
    for step in (1, 2):
        g = torch.Generator().manual_seed(100 * step)          # every rank can rebuild every rank's inputs
        dth = [torch.randn(B, sh.rows, generator=g) * 1e-3 for _ in range(world)]
        t5 = [torch.randn(B, 2048, generator=g) for _ in range(world)]
        rest = [torch.randn(flat.total - sh.hi, generator=g) for _ in range(world)]
        # expected state after this step: Adam on the GLOBAL gradient (sum over ranks)
        gw = sum(d.t() @ t for d, t in zip(dth, t5)).reshape(-1)
        gfull = torch.zeros_like(flat.flat)
        gfull[sh.lo:sh.lo + sh.rows * sh.cols] = gw
        gfull[sh.hi:] = sum(rest)
        _cpu_adam(want_w, gfull, want_m, want_v, eng.lr, eng.betas[0], eng.betas[1], eng.eps, step)
        # what step() does behind the backward in shard mode (core/engine.py), without ever calling finish_pending
        eng._adam_step = step
        flat.grad[sh.hi:] = rest[rank]
        sh.begin(dth[rank], t5[rank])
        eng._after_hypernet_backward()                          # own rows updated, their gather + the trunk's all-reduce in flight
        eng.reducer.launch(2)
        eng.reducer.wait(2)
        eng._adam(2)
        eng._heads_pending = True
        eng.steps = step
        if step == 1:
            sd = model.state_dict()                             # pre-hook: must complete the deferred updates first
            got = torch.cat([sd[n].reshape(-1) for n in flat.names])
            want = torch.cat([want_w[o:o + p.numel()] for p, o in zip(flat.params, flat.offsets)])
            ok = _chk(checks, 1, _close_w(got, want) and not eng._heads_pending) and ok
        else:
            osd = eng.optimizer_state_dict()                    # collective: gathers the row-sharded moments
            params = list(model.parameters())
            off = {id(p): o for p, o in zip(flat.params, flat.offsets)}
            for i, p in enumerate(params):
                o = off[id(p)]
                st = osd["state"][i]
                # (sums over the ranks in gloo's ring order vs python's: compare to the tensor's scale, entries cancel to ~0)
                for key, wantbuf, k in (("exp_avg", want_m, 2), ("exp_avg_sq", want_v, 3)):
                    wv = wantbuf[o:o + p.numel()]
                    d = (st[key].reshape(-1) - wv).abs()
                    ok = _chk(checks, k, bool((d <= 1e-5 * wv.abs() + 1e-6 * wv.abs().max()).all())) and ok
                ok = _chk(checks, 4, float(st["step"]) == 2.0) and ok
            ok = _chk(checks, 5, _close_w(flat.flat[:sh.lo + sh.rows * sh.cols], want_w[:sh.lo + sh.rows * sh.cols])) and ok
            ok = _chk(checks, 6, _close_w(flat.flat[sh.hi:], want_w[sh.hi:])) and ok
    # every rank holds the same parameters
    mine = flat.flat.double().sum().reshape(1)
    alls = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(alls, mine)
    ok = _chk(checks, 7, all(torch.equal(alls[0], t) for t in alls)) and ok
    out.put((rank, True if ok else [c for c in checks if not c[1]]))
    ops.clear_grad_views()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_deferred_hypernetwork_updates_never_leak_stale_rows_into_checkpoints(world):
    """VERDICT r3 task 8(b): the heads' row gather and the trunk's all-reduce stay in flight across the step boundary; a
    `state_dict()` or an `optimizer_state_dict()` between steps must flush them (world sizes 2 and 4, gloo on CPU)."""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_deferred_worker, args=(r, world, port, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(out.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res == {r: True for r in range(world)}, res

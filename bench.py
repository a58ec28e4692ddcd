#!/usr/bin/env python3
"""bench.py — HyperPocket training-step throughput on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--no-emd] [--full [--no-extras] [--no-cpu-baseline]]
    python bench.py --workload chamfer-stress [--gpus N] [--full]   # BASELINE.json configs[4]: B=64/GPU, N=8192 Chamfer fwd+bwd

`--gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself (one process per GPU through
`python -m torch.distributed.run`, before this process has touched the GPU); under torchrun it is a rank.

A "step" is one full training step of the hot path on one batch of synthetic clouds resident in
HBM: forward (2 encoders -> hypernetwork -> batched target networks on freshly sampled points)
-> 0.05*Chamfer + KLD/B + 0.05*EMD/N -> backward -> [SUM all-reduce of the flat gradient over
RCCL when N>1] -> Adam.  Workload = the configuration the metric is quoted on: HyperPocket 128+128,
B=64 clouds per GPU, existing/missing (B,1024,3), gt (B,2048,3), fp32 ("Chamfer+EMD").
value = clouds/s over all ranks (weak scaling: B per GPU fixed).

One JSON line on rank 0.  A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the contract
keys.  With --full the line also carries (--no-extras drops all but cpu_baseline, --no-cpu-baseline drops that one)
  roofline        the DOMINANT kernel family of the step — the EMD sweeps (emd_rows1 / emd_rows2 / emd_grad2: about half of the
                  step's kernel time), bound by the quarter-rate v_exp_f32: achieved = the algorithm's 27 exponentials per point
                  pair / the call's duration measured live with HIP events, peak = the chip's exponential rate
  roofline_mfma   the widest matrix kernel (conv5 + max-pool of the encoder stack: f16 pipe, both operands stored as f16
                  piece pairs), timed live with HIP events against the f16 matrix peak / 3 products
  reference_loop  the same model driven the way the reference's untouched core/epoch_loops.py drives it (Chamfer-only loss,
                  pinned host inputs, 3 x .item(), the caller's optimiser): clouds/s, and how the gap to the engine splits
  cpu_baseline    the oracle's torch-CPU restatement of the reference step timed on this box's cores (16 threads and all)
  breakdown       extra figures (Chamfer-only step, the step with every kernel on its IEEE-fp32 form, one-rank RCCL) — informational
"""
import argparse
import copy
import gc
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODEL_CFG = {
    "random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
    "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
    "hyper_network": {"use_bias": True, "relu_slope": 0.2},
    "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                       "layer_out_channels": [32, 64, 128, 64]},
    "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}},
}
PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: dense fp32 matrix peak (v_mfma_f32_32x32x2_f32)
PEAK_F16_MFMA_TFLOPS = 2516.6    # MI355X_MICROARCH.md: dense f16/bf16 matrix peak (16 x the fp32 matrix rate)
PEAK_F32_VALU_TFLOPS = 157.3     # MI355X_MICROARCH.md: fp32 vector peak (64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz)
PEAK_HBM_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E spec peak
PEAK_VALU_ISSUE_TCYC = 1024 * 2.4e9 / 1e12   # SIMD issue cycles per second: 256 CUs x 4 SIMDs x 2.4 GHz (same guide)
EXP_ISSUE_CYCLES = 8.0                       # v_exp_f32: quarter-rate transcendental, 8 issue cycles per 64-lane wave-instruction
PEAK_TEXP_PER_S = PEAK_VALU_ISSUE_TCYC / EXP_ISSUE_CYCLES * 64.0   # 19.66 T exponentials/s if the chip issued nothing else


def synth_batch(b, n_half, device, seed):
    """existing, missing ~ U(-0.5,0.5)^(B,1024,3), gt = cat(existing, missing)."""
    g = torch.Generator(device=device).manual_seed(seed)
    ex = torch.rand(b, n_half, 3, device=device, generator=g) - 0.5
    mi = torch.rand(b, n_half, 3, device=device, generator=g) - 0.5
    return ex, mi, torch.cat([ex, mi], 1)


DUMP_BYTES_MAX = 64 << 20          # --dump-outputs: everything written, at most
DUMP_SAMPLE = 1 << 18              # ... elements kept per array (a fixed, seeded sample of larger ones): the total stays under
                                   # the cap whatever --batch / --points (train step: 54 tensors; chamfer-stress: 7 arrays)


def sampled(t, rng):
    """A device tensor flattened, as float64 numpy when its values are integers (indices), else float32; above DUMP_SAMPLE
    elements only the elements at DUMP_SAMPLE sorted positions drawn from `rng` (seeded, the same for every run and build)."""
    import numpy as np
    flat = t.detach().reshape(-1)
    if flat.numel() > DUMP_SAMPLE:
        idx = np.sort(rng.choice(flat.numel(), DUMP_SAMPLE, replace=False))
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    return flat.cpu().numpy().astype(np.float32 if flat.is_floating_point() else np.float64)


def dump_outputs(dirname, arrays):
    """--dump-outputs: write name -> array as DIR/<name>.npy (float32 / float64 only) so that two builds' runs with the
    same arguments (same seeded inputs) can be compared output for output."""
    import numpy as np
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    for k, v in arrays.items():
        assert v.dtype in (np.float32, np.float64), (k, v.dtype)
    total = sum(v.nbytes for v in arrays.values())
    assert total <= DUMP_BYTES_MAX, f"--dump-outputs would write {total} bytes"
    os.makedirs(dirname, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), v)


def train_step_outputs(out, model):
    """What a caller of the timed TrainEngine.step holds after the last timed step: the loss terms it returned and the
    model's parameters it updated in place (flattened; tensors above DUMP_SAMPLE elements: see `sampled`)."""
    import numpy as np
    arrays = {k: v.detach().float().reshape(1).cpu().numpy() for k, v in sorted(out.items())}
    rng = np.random.default_rng(0)
    for name, p in model.named_parameters():
        arrays["param." + name] = sampled(p.float(), rng)
    return arrays


def latest_profile(suffix):
    """profiles/rNN_<suffix> of the latest round that has it (name, path) — the committed rocprofv3 summaries."""
    import glob
    hits = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + suffix)))
    return (os.path.basename(hits[-1]), hits[-1]) if hits else (None, None)


def event_time_ms(fn, iters, warm=2):
    """Average duration of fn() measured with HIP events on the stream fn launches on (torch's current stream).
    The events bracket back-to-back launches, so a host-side pause longer than the queued work would be counted as
    kernel time: Python's cyclic collector (a 30 ms gen-2 pass was observed here) is held off for the region.  The
    start event is recorded straight behind the warm-up launches, with no synchronisation in between: an idle gap there
    makes the chip re-ramp its clock inside the timed region (measured: 102 vs 113-118 TFLOP/s on the same launches at
    20 warm-up launches)."""
    gc.collect()
    gc.disable()
    try:
        for _ in range(warm):
            fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
    finally:
        gc.enable()
    return s.elapsed_time(e) / iters


def roofline_widest_matrix_kernel(batch, n_half, minimal=False):
    """The widest MATRIX kernel of the step (5 % of its kernel time; the dominant family is the EMD sweeps, roofline_emd):
    layer 5 of the encoders' conv stack with its fused max-pool,
    max over points of A(M x 512) W(512 x 512)^T + b, M = B*1024 points of one encoder (the step batches both encoders into one
    launch of twice the tiles: `paired_launch` times that shape too).  Round 3 moved the layer from the fp32 matrix pipe
    (gemm_kernel<128,128,4,2,16,4>, v_mfma_f32_32x32x2_f32, 0.79 of 157.3 TFLOP/s) to the f16 pipe with every fp32 operand as two
    f16 pieces — three f16 MFMA products per fp32-equivalent product, fp32 accumulation (csrc/conv_split.hip, 0.30 of f16 / 3);
    round 4 stores the activations already split (csrc/conv_pp.hip), so BOTH operands are DMA-staged into 256 x 256 tiles of a
    persistent 8-wave workgroup per CU.  Algorithmic flops = 2*M*512*512; `achieved` is algorithmic TFLOP/s.  The
    roofline that bounds the kernel is the f16 matrix peak divided by the three products it executes per algorithmic one —
    `peak`; `frac` = achieved / peak = executed f16 flops / f16 peak.  `vs_f32_mfma_peak` prices the same number against the fp32
    matrix peak rounds 1-2 were bound by; `round3_kernel` and `f32_mfma_kernel` are the previous kernels timed here on the same
    operands.  `traffic` (HBM bytes per launch) comes from the PMC passes recorded under profiles/ (FETCH_SIZE x2 correction +
    WRITE_SIZE), measured at B=64."""
    from hyperpocket_amd import ops
    m = batch * n_half
    a = torch.randn(m, 512, device="cuda").abs_()
    w = torch.randn(512, 512, device="cuda") * 0.05
    b = torch.zeros(512, device="cuda")
    c = torch.empty(m, 512, device="cuda")
    # 200 warm-up launches: the chip needs >20 ms of continuous load to reach the clock it then sustains — the state every
    # kernel of a training run executes in (tools/roof_sweep.py)
    pp = ops.GemmPP(a, w, b, relu=False, xcb=256, group_rows=n_half)
    ms = event_time_ms(lambda: pp.run(1), iters=100, warm=200)
    if minimal:      # (the rocprofv3 passes of tools/final_measure.sh: only the kernel itself in the trace)
        flops = 2.0 * m * 512 * 512
        return {"kernel": "conv_pp_kernel<1, 2, 2>", "avg_launch_ms": round(ms, 4), "achieved": round(flops / (ms * 1e-3) / 1e12, 2)}
    a2 = torch.cat([a, a.flip(0)])
    pp2 = ops.GemmPP(a2, w, b, relu=False, xcb=256, group_rows=n_half)
    ms_pair = event_time_ms(lambda: pp2.run(1), iters=60, warm=100)
    del pp2, a2
    g = ops.GemmF16x2(a, w, b, relu=False, out=c)
    ms_r3 = event_time_ms(g.run, iters=60, warm=100)
    ms32 = event_time_ms(lambda: ops.gemm(a, w, bias=b, out=c), iters=50, warm=100)
    flops = 2.0 * m * 512 * 512
    achieved = flops / (ms * 1e-3) / 1e12
    peak = PEAK_F16_MFMA_TFLOPS / 3.0
    traffic = None
    pmc_name, pmc = latest_profile("pmc_gemm_conv5.json")
    if pmc and batch == 64 and n_half == 1024:
        rec = json.load(open(pmc))
        if "conv_pp" in rec.get("kernel", ""):
            traffic = rec["hbm_bytes_per_launch"]
    return {"bound": "mfma", "kernel": "conv_pp_kernel<1, 2, 2> (encoder conv5 + fused max-pool: M=B*1024, N=K=512; both operands stored as "
                                       "2 f16 pieces and DMA-staged, 3 x v_mfma_f32_32x32x16_f16 per 32x32x16 block of products, fp32 "
                                       "accumulate)",
            "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4),
            "peak_is": f"f16 dense MFMA peak {PEAK_F16_MFMA_TFLOPS} TFLOP/s / 3 products per fp32-equivalent product",
            "executed_f16_tflops": round(3 * achieved, 1),
            "paired_launch": {"what": "the step's launch: both encoders = twice the tiles (4 per persistent workgroup instead of 2)",
                              "avg_launch_ms": round(ms_pair, 4), "achieved": round(2 * flops / (ms_pair * 1e-3) / 1e12, 2),
                              "frac": round(2 * flops / (ms_pair * 1e-3) / 1e12 / peak, 4)},
            "vs_f32_mfma_peak": round(achieved / PEAK_F32_MFMA_TFLOPS, 3),
            "round3_kernel": {"kernel": "conv_split_kernel<false> (fp32 activations split in the consumer, 128x128 tiles; stores C)",
                              "avg_launch_ms": round(ms_r3, 4), "achieved": round(flops / (ms_r3 * 1e-3) / 1e12, 2),
                              "frac": round(flops / (ms_r3 * 1e-3) / 1e12 / peak, 4)},
            "f32_mfma_kernel": {"kernel": "gemm_kernel<128,128,4,2,16,4> (v_mfma_f32_32x32x2_f32)", "avg_launch_ms": round(ms32, 4),
                                "achieved": round(flops / (ms32 * 1e-3) / 1e12, 2), "peak": PEAK_F32_MFMA_TFLOPS,
                                "frac": round(flops / (ms32 * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)},
            "traffic": traffic,
            "traffic_source": f"profiles/{pmc_name} (rocprofv3 --pmc passes of this launch; not measured in this run)"
            if traffic is not None else None,
            "avg_launch_ms": round(ms, 4), "flops_per_launch": flops,
            "algorithmic_bytes_per_launch": (m * 512 + 512 * 512 + 512 + 2 * (m // 128) * 512) * 4}


def cpu_baseline(n_half, emd_coef, sample_b=4, timed_steps=2, full_b=64):
    """The oracle (oracle/hyperpocket_ref.py: torch-CPU restatement of the reference step + the C restatement of the
    EMD kernels, kind "port") on bounded samples of the SAME workload (B = 4 and B = 64): `sample_b` clouds of
    the same per-cloud shape and loss terms, 1 warm-up + `timed_steps` timed steps — the headline `value` — and, when the
    host is fast enough for it to stay within ~60 s, one warm-up + one timed step at the metric's own batch `full_b`."""
    from oracle import hyperpocket_ref as ref
    # torch's CPU kernels stop scaling (and thrash across NUMA domains) far below a 256-core host: the headline leg runs on 16
    # threads; the same sample is timed once more on every core the host has (SURVEY 8d asked for os.cpu_count()) and reported
    # beside it
    host_cores = os.cpu_count() or 1
    threads = min(16, host_cores)

    def use(n_threads):
        torch.set_num_threads(n_threads)
        os.environ["OMP_NUM_THREADS"] = str(n_threads)      # the C EMD oracle parallelises over clouds
    use(threads)

    def leg(b, steps):
        P = ref.init_params(2020)
        opt = ref.Adam(P)
        g = torch.Generator().manual_seed(2020)
        ex = torch.rand(b, n_half, 3, generator=g) - 0.5
        mi = torch.rand(b, n_half, 3, generator=g) - 0.5
        gt = torch.cat([ex, mi], 1)

        def one():
            pts = torch.stack([ref.generate_points(1, 2 * n_half) for _ in range(b)])   # CPU draws, as the reference
            eps = torch.randn(b, 128)
            ref.train_step(P, opt, ex, mi, gt, pts, eps, emd_coef=emd_coef)
        one()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        return (time.perf_counter() - t0) / steps

    dt = leg(sample_b, timed_steps)
    what = f"0.05*Chamfer + KLD/B{' + 0.05*EMD/N' if emd_coef else ''}, Adam"
    out = {"value": round(sample_b / dt, 3), "unit": "clouds/s", "cores": threads, "host_cores": host_cores, "kind": "port",
           "sample": f"{timed_steps} timed steps (after 1 warm-up) of the oracle train step ({what}) at B={sample_b}, "
                     f"existing/missing ({sample_b},{n_half},3), gt ({sample_b},{2 * n_half},3); {dt:.2f} s/step; "
                     f"{threads} threads of the host's {host_cores} cores"}
    est = dt * full_b / sample_b * 2                   # 1 warm-up + 1 timed step, if a step scaled linearly with B
    if full_b and full_b != sample_b and est <= 60.0:
        dt_full = leg(full_b, 1)
        out["at_metric_batch"] = {"value": round(full_b / dt_full, 3), "unit": "clouds/s", "batch": full_b,
                                  "sample": f"1 timed step (after 1 warm-up) at B={full_b}; {dt_full:.2f} s/step"}
    elif full_b and full_b != sample_b:
        out["at_metric_batch"] = {"value": None, "batch": full_b,
                                  "sample": f"skipped: ~{est:.0f} s estimated from the B={sample_b} leg (bound: 60 s)"}
    if host_cores > threads:
        # more threads: 64 first; every core only if that was not already slower (at 256 threads one B=4 step took 73 s on the
        # round-5 box — torch's CPU kernels and OpenMP thrash across the NUMA domains — recorded in profiles/r05_cpu_baseline_threads.json;
        # the default run must stay within minutes)
        out["more_threads"] = []
        best = dt
        for n_thr in sorted({min(64, host_cores), host_cores}):
            if n_thr <= threads:
                continue
            if out["more_threads"] and out["more_threads"][-1]["s_per_step"] >= dt and not os.environ.get("HP_BENCH_ALL_CORES"):
                out["more_threads"].append({"cores": n_thr, "value": None,
                                            "sample": f"skipped: {out['more_threads'][-1]['cores']} threads were already no faster than {threads} "
                                                      "(HP_BENCH_ALL_CORES=1 forces it; measured in round 5: 70.7 s/step = 0.057 clouds/s at "
                                                      "256 threads, profiles/r05_cpu_baseline_threads.json)"})
                continue
            use(n_thr)
            dt_n = leg(sample_b, 1)
            out["more_threads"].append({"cores": n_thr, "value": round(sample_b / dt_n, 3), "unit": "clouds/s", "s_per_step": round(dt_n, 2),
                                        "sample": f"1 timed step (after 1 warm-up) at B={sample_b} with {n_thr} threads"})
            best = min(best, dt_n)
        use(threads)
    return out


def dropin_route(batch, n_half, device, steps, optimizer="torch"):
    """The route the reference's own loop takes with the drop-in modules — /root/reference/core/epoch_loops.py:15-39 as
    that file drives it, not the engine: per iteration `optimizer.zero_grad()`, the three inputs moved from pinned host
    memory (the reference's DataLoaders are built with pin_memory=True, core/main.py:91) with `.to(device)`,
    `full_model(existing, missing, list(gt.shape), epoch, device)`, `0.05 * ChamferLoss()(gt, rec.permute(0, 2, 1))`, the
    KLD term in torch, three `.item()` host syncs, `loss.backward()`, `optimizer.step()`.  Chamfer-only: the
    reference's training loss.  optimizer = "torch": torch.optim.Adam(full_model.parameters(), lr=1e-4) exactly as
    core/main.py:62-66 builds it; "flat": hyperpocket_amd.optim.FlatAdam(full_model, lr=1e-4), the documented one-line
    replacement.  Returns ms per iteration: the median of three blocks of `steps` iterations (host clock, device
    idle before and after each block)."""
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.losses.champfer_loss import ChamferLoss
    from hyperpocket_amd.model.full_model import FullModel
    from hyperpocket_amd.optim import FlatAdam
    torch.manual_seed(2020)
    model = FullModel(copy.deepcopy(MODEL_CFG))
    model.apply(weights_init)
    model = model.to(device)
    loss_fn = ChamferLoss().to(device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4) if optimizer == "torch" else FlatAdam(model, lr=1e-4)
    ex, mi, gt = (t.cpu().pin_memory() for t in synth_batch(batch, n_half, device, 2020))
    model.train()
    sums = [0.0, 0.0, 0.0]

    def iteration():
        opt.zero_grad()
        e, m, g = ex.to(device), mi.to(device), gt.to(device)
        rec, logvar, mu = model(e, m, list(g.shape), 1, device)
        loss_r = torch.mean(0.05 * loss_fn(g, rec.permute(0, 2, 1)))
        kld = torch.div(0.5 * (torch.exp(logvar) + torch.square(mu) - 1 - logvar).sum(), e.shape[0])
        total = loss_r + kld
        sums[0] += kld.item()
        sums[1] += loss_r.item()
        sums[2] += total.item()
        total.backward()
        opt.step()

    for _ in range(5):
        iteration()
    # three timed blocks of `steps` iterations, the median reported: the loop is host-bound (three .item() syncs, blocking copies),
    # so one scheduling hiccup of the box's CPU inside a single block of 20 moved the figure by 50 % (2.1 -> 3.6 ms, seen once)
    import gc
    blocks = []
    gc_was = gc.isenabled()
    gc.disable()
    try:
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                iteration()
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t0) / steps * 1e3)
    finally:
        if gc_was:
            gc.enable()
    ms = sorted(blocks)[1]
    assert sums[2] == sums[2], "NaN loss on the drop-in route"
    from hyperpocket_amd import ops
    if optimizer != "torch":
        model.hyper_network._heads_exchange = None
        model._after_encoder_tails = None
    del opt, model
    ops.clear_grad_views()
    return ms


class c_stdout_to_stderr:
    """RCCL prints a version banner to the C-level stdout when a communicator is created; with C buffering it lands
    BEHIND the JSON line at exit.  The contract is one JSON line on stdout: send fd 1 to stderr around group creation and
    flush the C buffer before restoring it."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


def visible_gpus():
    """Number of GPUs the ranks will see, WITHOUT initialising HIP in this process (torch.cuda.device_count() may fall
    back to hipGetDeviceCount, which opens /dev/kfd; the ranks are then children of a GPU-initialised process — the
    pattern to stay away from on this pool).  *_VISIBLE_DEVICES if set, else the KFD topology's nodes with SIMDs; None if
    neither can be read (the ranks then fail by themselves with a clear message)."""
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(",") if x.strip() != ""])
    base = "/sys/class/kfd/kfd/topology/nodes"
    try:
        n = 0
        for node in os.listdir(base):
            with open(os.path.join(base, node, "properties")) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            n += int(props.get("simd_count", "0")) > 0
        return n
    except OSError:
        return None


def spawn_ranks(n):
    """`python bench.py --gpus N` outside torchrun: start N fresh ranks (one process per GPU) and relay their output.
    Nothing in this process has initialised HIP yet (importing torch does not), and it never does — the device count
    comes from the environment / sysfs (visible_gpus) — : the children are separate Python processes started through
    torch.distributed.run, no exec of a GPU-holding process."""
    if not os.environ.get("HP_BENCH_ONE_DEVICE") and os.environ.get("HP_BENCH_BACKEND", "nccl") == "nccl" \
            and "--rendezvous-only" not in sys.argv:
        have = visible_gpus()                     # from the environment / sysfs: this launcher never touches HIP
        if have is not None and have < n:
            print(f"bench.py: --gpus {n} but only {have} GPU(s) visible", file=sys.stderr)
            return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def rendezvous_only(args, world, rank):
    """Launcher self-test (`--rendezvous-only`, used by the CPU suite): the ranks form the group, run one all-reduce and a
    barrier, rank 0 prints a line with the contract's rank bookkeeping.  gloo when no GPU is present."""
    backend = os.environ.get("HP_BENCH_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend, rank=rank, world_size=world)
        dev = "cuda" if backend == "nccl" else "cpu"
        if backend == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        t = torch.ones(4, device=dev) * (rank + 1)
        dist.all_reduce(t)
        dist.barrier()
        total, ranks = float(t[0]), dist.get_world_size()
        dist.destroy_process_group()
    else:
        total, ranks = 1.0, 1
    if rank == 0:
        print(json.dumps({"rendezvous_only": True, "n_gpus": world, "rccl_ranks": ranks, "gpus_arg": args.gpus,
                          "backend": backend if world > 1 else None, "allreduce_sum": total}), flush=True)
    if os.environ.get("HP_BENCH_FAIL_RANK") == str(rank):      # test hook: a failing child must fail the launcher
        sys.exit(3)


def _pmc_profile(suffix):
    """(name, contents) of the latest round's profiles/rNN_<suffix>, or (None, None)."""
    name, path = latest_profile(suffix)
    return (name, json.load(open(path))) if path else (None, None)


def emd_regime_noisy_copy(batch, n, device="cuda"):
    """The regime the EMD legs are timed in: gt ~ U(-0.5,0.5)^3, rec = a permuted copy of gt + N(0, sigma^2) noise, sigma cycling
    over 0.002 / 0.01 / 0.02 / 0.05 — late-training geometry, the "noisy copy" regime of
    tests/test_structural_losses_gpu.py::test_emd_cost_error_distribution_at_full_size (every cost carries mass)."""
    g = torch.Generator(device=device).manual_seed(7)
    f32 = dict(dtype=torch.float32, device=device)
    gt = torch.rand(batch, n, 3, generator=g, **f32) - 0.5
    perm = torch.stack([torch.randperm(n, generator=g, device=device) for _ in range(batch)])
    sig = torch.tensor([0.002, 0.01, 0.02, 0.05], **f32)[torch.arange(batch, device=device) % 4].view(batch, 1, 1)
    rec = torch.gather(gt, 1, perm.unsqueeze(-1).expand(-1, -1, 3)) + sig * torch.randn(batch, n, 3, generator=g, **f32)
    return gt.contiguous(), rec.contiguous()


def emd_culled_share(ws, batch, n, levels):
    """Share of the (64-row tile, 8-candidate block) units the culling sweeps skip at each of the first `levels` annealing levels,
    recomputed on the host side from the bounding boxes emd_order_kernel left in the workspace (emd.hip ws_layout; the same test
    as box_gap2: squared gap of the two boxes > 152 / (|level| log2 e)).  Mean over both directions (rows = set1 and rows = set2)."""
    from hyperpocket_amd._lib import load_library
    per = load_library().hp_approxmatch_workspace_floats(1, n, n)
    w = ws.view(batch, per)
    P = (n + 63) // 64 * 64
    off = 2 * (P + 8) * 4 + (P + 8) + 2 * (P + 8) * 16 + 2 * P
    nb, nt = P // 8, P // 64
    blkL = w[:, off:off + 6 * nb].view(batch, 6, nb)
    blkR = w[:, off + 6 * nb:off + 12 * nb].view(batch, 6, nb)
    tileL = w[:, off + 12 * nb:off + 12 * nb + 6 * nt].view(batch, 6, nt)
    tileR = w[:, off + 12 * nb + 6 * nt:off + 12 * nb + 12 * nt].view(batch, 6, nt)

    def gap2(t, c):
        g = torch.clamp(torch.maximum(c[:, :3, None, :] - t[:, 3:, :, None], t[:, :3, :, None] - c[:, 3:, None, :]), min=0)
        return (g * g).sum(1)
    gl, gr = gap2(tileL, blkR), gap2(tileR, blkL)
    out = []
    for lev in range(levels):
        thr = 152.0 / (4.0 ** (7 - lev) * 1.4426950408889634)
        out.append(round(0.5 * ((gl > thr).float().mean().item() + (gr > thr).float().mean().item()), 4))
    return out


def roofline_emd(batch, n):
    """The DOMINANT kernel family of the Chamfer+EMD step: the EMD sweeps of one hp_emd_forward call (emd_rows1 x9, emd_rows2 x9 — per
    chain of half the clouds since round 5 —, emd_grad2: about half of the step's kernel time in profiles/).  Neither HBM- nor MFMA-bound: the match-free design
    removed the 20.4 GB/call of `match` traffic SURVEY 8(d) prices (measured: ~1 GB/call), and there is no matrix work; what
    bounds it is the quarter-rate v_exp_f32.  SURVEY 8(d) fixes the ALGORITHMIC work at 27 exponentials per point pair (three
    phases x nine levels, approxmatch.cu:86,131,185), so
        achieved = 27 * B * n * m exponentials / the call's duration (HIP events, measured live here)
        peak     = 1024 SIMDs x 2.4 GHz / 8 issue cycles per v_exp_f32 wave-instruction x 64 lanes = 19.66 T exp/s
        frac     = achieved / peak      (the floor VERDICT r4 recomputed: 369 us at B=64, n=2048)
    Round 6: the sweeps of the first levels skip the units whose exponentials are exactly zero, so the call's duration depends
    on the data; the inputs are the late-training regime (emd_regime_noisy_copy), and `executed` prices what the call really
    issues: per pair 27 minus the culled share of the first levels' three exponentials each (recomputed from the boxes in the
    workspace) plus the final sweep's 5 hardware exponentials (9 without the derivation).  `uncull` = the same call with
    hp_emd_set_cull(0) (rounds 1-5's sweeps) on the same inputs.  `issue_stream` is the builder's finer model of the un-culled
    instruction stream (profiles/rNN_emd_issue_model.json).  `traffic`: HBM bytes per call from the PMC passes under profiles/."""
    from hyperpocket_amd._lib import call, current_stream, load_library
    import ctypes
    model_name, model = _pmc_profile("emd_issue_model.json")
    lib = load_library()
    lib.hp_emd_partials_floats.restype = ctypes.c_long
    f32 = dict(dtype=torch.float32, device="cuda")
    a, c = emd_regime_noisy_copy(batch, n)
    temp = torch.empty((batch, 4 * n), **f32)
    ws = torch.empty((lib.hp_approxmatch_workspace_floats(batch, n, n),), **f32)
    part = torch.empty((lib.hp_emd_partials_floats(batch, n, n),), **f32)
    cost = torch.empty((batch,), **f32)
    g2 = torch.empty((batch, n, 3), **f32)
    st = current_stream(a.device)
    fn = lambda: call("hp_emd_forward", batch, n, n, a, c, temp, ws, part, cost, None, g2, st)
    ms = event_time_ms(fn, iters=20, warm=10)
    cull = lib.hp_emd_set_cull(0)
    try:      # (HP_BENCH_EMD_NO_UNCULL=1: the PMC passes of tools/final_measure.sh profile the shipped call only)
        ms0 = event_time_ms(fn, iters=20, warm=10) if cull and not os.environ.get("HP_BENCH_EMD_NO_UNCULL") else ms
    finally:
        lib.hp_emd_set_cull(cull)
    fn()
    torch.cuda.synchronize()
    share = emd_culled_share(ws, batch, n, cull) if cull else []
    derive = lib.hp_emd_set_final_derive(1)
    lib.hp_emd_set_final_derive(derive)
    final_exp = 5 if derive else 9
    pairs = float(batch) * n * n
    achieved = 27.0 * pairs / (ms * 1e-3) / 1e12
    executed = 27.0 - 3.0 * sum(share) + final_exp
    out = {"bound": "valu-exp",
           "kernel": "hp_emd_forward = emd_order_kernel (Hilbert order of both sets) + 9 x (emd_rows1 + emd_rows2) level sweeps — the first "
                     f"{cull} levels on the culling instances —, as two chains of half the clouds on two streams, + one emd_grad2_kernel over all "
                     f"clouds (B={batch}, n=m={n}, cost + d cost/d xyz2)",
           "inputs": "late-training regime: gt U(-0.5,0.5)^3, rec = permuted gt + N(0, sigma^2), sigma in {0.002, 0.01, 0.02, 0.05} "
                     "(the noisy-copy regime of test_emd_cost_error_distribution_at_full_size)",
           "achieved": round(achieved, 3), "peak": round(PEAK_TEXP_PER_S, 2), "unit": "Texp/s",
           "frac": round(achieved / PEAK_TEXP_PER_S, 4),
           "avg_call_ms": round(ms, 4), "exp_per_pair": 27, "exp_per_call": 27.0 * pairs,
           "floor_ms": round(27.0 * pairs / PEAK_TEXP_PER_S / 1e12 * 1e3, 4),
           "peak_is": "1024 SIMDs x 2.4 GHz / 8 issue cycles per v_exp_f32 wave-instruction x 64 lanes (MI355X_MICROARCH.md issue costs)",
           "culled_share_per_level": share,
           "uncull": {"avg_call_ms": round(ms0, 4), "frac": round(27.0 * pairs / (ms0 * 1e-3) / 1e12 / PEAK_TEXP_PER_S, 4),
                      "what": "the same call, same inputs, hp_emd_set_cull(0): caller's point order, every unit evaluated (rounds 1-5)"},
           "executed": {"exp_per_pair": round(executed, 3), "frac": round(executed / 27.0 * achieved / PEAK_TEXP_PER_S, 4),
                        "what": f"27 - 3 x the culled share of each culling level + {final_exp} (the match-free final sweep rebuilds the match "
                                "entries: 5 hardware exponentials per pair with the derived form, 9 without)"}}
    if model and model.get("batch") == batch and model.get("n") == n:
        cyc = model["issue_cycles_per_call"]
        out["issue_stream"] = {"frac_uncull": round(cyc / (ms0 * 1e-3) / 1e12 / PEAK_VALU_ISSUE_TCYC, 4), "issue_cycles_per_call": cyc,
                               "peak_T_issue_cycles_per_s": round(PEAK_VALU_ISSUE_TCYC, 4), "model": f"profiles/{model_name}",
                               "what": "all VALU instructions of the compiled UN-CULLED sweep loops at their issue cost / the un-culled call's time / "
                                       "(1024 SIMDs x 2.4 GHz): a model of the instruction stream, not the algorithmic roofline"}
        out["traffic"] = model.get("hbm_bytes_per_call")
        out["traffic_source"] = f"profiles/{model_name} (rocprofv3 --pmc passes; not measured in this run)"
    else:
        out["traffic"] = None
    return out


def chamfer_stress(args, world, rank, local_rank, grouped, device):
    """BASELINE.json configs[4]: synthetic random clouds, B=64 per GPU, N=8192, fp32 — the O(N^2) Chamfer forward
    (both directed nearest-neighbour passes + the batch sum) and backward (gradients of both sets), nothing else.
    A "step" = one forward + backward over the resident batch; value = point-pair distance evaluations per second
    (2 directions x B x N x N per step) over all ranks.  The kernel is fp32-VALU-bound (820 FLOP per HBM byte):
    `roofline` prices it against the vector peak with the 8 FLOP per pair of SURVEY §8d, and reports the HBM side next
    to it (algorithmic bytes / time, and the PMC-measured bytes when profiles/ holds them for this shape)."""
    import ctypes
    from hyperpocket_amd._lib import call, current_stream, load_library
    lib = load_library()
    B, N = args.batch, args.points
    f32 = dict(dtype=torch.float32, device=device)
    g = torch.Generator(device=device).manual_seed(2020 + rank)
    x = torch.rand(B, N, 3, generator=g, **f32) - 0.5
    y = torch.rand(B, N, 3, generator=g, **f32) - 0.5
    d1, d2 = torch.empty((B, N), **f32), torch.empty((B, N), **f32)
    i1 = torch.empty((B, N), dtype=torch.int32, device=device)
    i2 = torch.empty((B, N), dtype=torch.int32, device=device)
    part = torch.empty((lib.hp_chamfer_workspace_floats(B, N, N),), **f32)
    loss = torch.empty((), **f32)
    one = torch.ones((), **f32)
    gx, gy = torch.empty_like(x), torch.empty_like(y)
    st = current_stream(device)

    def fwd():
        call("hp_chamfer_forward", B, N, x, N, y, d1, i1, d2, i2, part, loss, st)

    def bwd():
        call("hp_chamfer_backward", B, N, x, N, y, i1, i2, one, gx, gy, st)

    def sync():
        if grouped:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        fwd(); bwd()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        fwd(); bwd()
    sync()
    dt = time.perf_counter() - t0
    if grouped:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    ms_per_step = dt / args.steps * 1e3
    pairs = 2.0 * B * N * N
    if rank != 0:
        return
    if args.dump_outputs:
        import numpy as np
        rng = np.random.default_rng(0)      # flattened; above DUMP_SAMPLE elements a fixed, seeded sample (`sampled`)
        dump_outputs(args.dump_outputs, {"loss": loss.reshape(1).cpu().numpy(),
                                         **{k: sampled(t, rng) for k, t in (("dist1", d1), ("dist2", d2), ("idx1", i1),
                                                                           ("idx2", i2), ("grad_xyz1", gx), ("grad_xyz2", gy))}})
    line = {"metric": f"chamfer-stress point-pair evaluations/sec at B={B}/GPU, N={N} (Chamfer forward + backward)",
            "value": round(pairs * world / (ms_per_step * 1e-3), 1), "unit": "pairs/s", "n_gpus": world,
            "rccl_ranks": dist.get_world_size() if grouped else 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"BASELINE.json configs[4] per-GPU shape: Chamfer forward+backward on two U(-0.5,0.5) "
                                   f"sets of ({B},{N},3), fp32; no model, no collective (clouds shard over ranks)",
                       "global_batch": B * world, "points": N, "parallelism": f"dp{world}"},
            "final_loss": loss.item()}
    if args.full and not args.no_extras:
        ms_f = event_time_ms(fwd, iters=10, warm=3)
        ms_b = event_time_ms(bwd, iters=10, warm=3)
        flops = 8.0 * pairs                               # 3 sub, 3 mul, 2 add per pair; compares excluded
        alg_bytes = B * (2 * N * 12 + 2 * N * 8)          # (n+m)*12 B read + (n+m)*8 B written per cloud
        tf = flops / (ms_f * 1e-3) / 1e12
        _, pmc = _pmc_profile("pmc_chamfer_n8192.json")
        traffic = pmc["hbm_bytes_per_launch"] if pmc and pmc.get("batch") == B and pmc.get("n") == N else None
        line["roofline"] = {"bound": "valu", "kernel": "nn_distance_kernel (both directed passes of the Chamfer forward, one launch)",
                            "achieved": round(tf, 2), "peak": PEAK_F32_VALU_TFLOPS, "unit": "TFLOP/s",
                            "frac": round(tf / PEAK_F32_VALU_TFLOPS, 4), "traffic": traffic,
                            "avg_launch_ms": round(ms_f, 4), "flops_per_launch": flops,
                            "algorithmic_bytes_per_launch": alg_bytes,
                            "hbm_GBps_algorithmic": round(alg_bytes / (ms_f * 1e-3) / 1e9, 2),
                            "hbm_frac_of_peak": round(alg_bytes / (ms_f * 1e-3) / 1e9 / PEAK_HBM_GBS, 5),
                            "backward_avg_ms": round(ms_b, 4)}
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="clouds per GPU")
    ap.add_argument("--points", type=int, default=None, help="points per cloud (default 2048; chamfer-stress: 8192)")
    ap.add_argument("--workload", choices=["train-step", "chamfer-stress"], default="train-step")
    ap.add_argument("--rendezvous-only", action="store_true", help="launcher self-test: form the group, one all-reduce, exit")
    ap.add_argument("--no-emd", action="store_true", help="reference-faithful Chamfer-only loss as the headline step")
    ap.add_argument("--precondition", type=int, default=400,
                    help="untimed training steps (after scaling the hypernetwork heads by 2^-6) that bring the model to the state the "
                         "step is timed at: rec at gt's scale; 0 = time the step at the seeded init")
    ap.add_argument("--full", action="store_true",
                    help="after the headline figure, also run the side measurements: rooflines, breakdown, reference loop, the "
                         "one-rank exchange probe and the CPU baseline (chamfer-stress: its roofline)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip roofline/breakdown side measurements")
    ap.add_argument("--roofline-minimal", action="store_true", help="the roofline kernel alone (200 warm-up + 100 timed launches): the command of the rocprofv3 passes")
    ap.add_argument("--roofline-emd-only", action="store_true",
                    help="the dominant family alone: the hp_emd_forward calls `roofline` times (10 warm-up + 20 timed) — the command of its rocprofv3 pass")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (loss terms and the updated parameters, "
                         "a seeded sample of the large tensors; chamfer-stress: distances, indices, gradients) as DIR/<name>.npy")
    ap.add_argument("--roofline-only", action="store_true",
                    help="run only the roofline leg (the dominant kernel at the step's shape) and print its object: the "
                         "command profiles/ pairs with `rocprofv3 --kernel-trace --stats`")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.points is None:
        args.points = 8192 if args.workload == "chamfer-stress" else 2048
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))       # before anything here touches the GPU
    if args.rendezvous_only:
        rendezvous_only(args, int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")))
        return
    if args.roofline_minimal:
        print(json.dumps({"roofline": roofline_widest_matrix_kernel(args.batch, args.points // 2, minimal=True)}), flush=True)
        return
    if args.roofline_emd_only:
        torch.cuda.set_device(0)
        print(json.dumps({"roofline": roofline_emd(args.batch, args.points)}), flush=True)
        return
    if args.roofline_only:
        torch.cuda.set_device(0)
        print(json.dumps({"roofline": roofline_emd(args.batch, args.points),
                          "roofline_mfma": roofline_widest_matrix_kernel(args.batch, args.points // 2)}), flush=True)
        return

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # Test hook (not used by the driver): HP_BENCH_BACKEND=gloo HP_BENCH_ONE_DEVICE=1 exercises the multi-rank code
    # path with every rank on cuda:0, so that it can be checked on a 1-GPU box.
    backend = os.environ.get("HP_BENCH_BACKEND", "nccl")
    if os.environ.get("HP_BENCH_ONE_DEVICE"):
        local_rank = 0
    # Test hook (not used by the driver): HP_BENCH_FORCE_EXCHANGE=1 at WORLD_SIZE=1 forms a one-rank RCCL group and runs
    # every collective of the multi-rank step in it (broadcast, bucketed async all-reduce, deferred waits, barrier).
    force_exchange = bool(os.environ.get("HP_BENCH_FORCE_EXCHANGE")) and world == 1
    if force_exchange:
        os.environ.setdefault("MASTER_PORT", "29533")
    if world > 1 or force_exchange:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            # RCCL's stream from the high-priority pool: its own hardware queue (never folded onto the compute stream's),
            # and the few workgroups of a collective are dispatched ahead of the wide GEMMs' instead of queueing behind
            opts = None
            try:
                opts = dist.ProcessGroupNCCL.Options(is_high_priority_stream=True)
            except Exception:      # older binding: default stream priority
                pass
            with c_stdout_to_stderr():
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank),
                                        pg_options=opts)
                # the communicator (and RCCL's stdout banner) comes with the first collective: do it here, under the guard
                dist.barrier()
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    if args.gpus != world and rank == 0:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}: reporting n_gpus={world}", file=sys.stderr)
    device = torch.device("cuda", local_rank if world > 1 else 0)
    grouped = world > 1 or force_exchange
    if args.workload == "chamfer-stress":
        chamfer_stress(args, world, rank, local_rank, grouped, device)
        if grouped:
            dist.barrier()
            dist.destroy_process_group()
        return

    from hyperpocket_amd.core.engine import TrainEngine
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel

    n_half = args.points // 2
    torch.manual_seed(2020)                     # settings/config.json.sample:107
    model = FullModel(copy.deepcopy(MODEL_CFG))
    model.apply(weights_init)
    model = model.to(device)
    torch.manual_seed(2020 + rank)              # per-rank streams for eps / decoder points
    emd_coef = 0.0 if args.no_emd else 0.05
    # Operating point (round 6).  At the seeded xavier-sqrt2 init the decoder's output sits at O(1e2) against clouds in the +-0.5
    # cube: every exponential of the EMD underflows, every nearest neighbour is the same corner point — a state training leaves
    # within its first steps, and one in which the round-6 EMD sweeps (which skip exactly-zero work) would be timed on next to
    # nothing.  The step is therefore timed where training spends its time: the tests' operating-point recipe
    # (tests/golden/make_golden.py train_to_operating_point) — the hypernetwork heads' weights x 2^-6 (exact), then
    # `--precondition` UNTIMED steps of this same engine on the bench batch — leaves rec at gt's scale (per-cloud std 0.29 against
    # 0.29; EMD costs carry mass, arg-mins are spread).  --precondition 0: the seeded init (rounds 1-5).
    if args.precondition > 0:
        with torch.no_grad():
            for head in model.hyper_network.output:
                head.weight.mul_(2.0 ** -6)
    engine = TrainEngine(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, loss_coef=0.05, emd_coef=emd_coef,
                         force_exchange=force_exchange)
    ex, mi, gt = synth_batch(args.batch, n_half, device, 2020 + rank)
    for _ in range(args.precondition):
        engine.step(ex, mi, gt, epoch=1)
    engine.finish_pending()
    torch.cuda.synchronize()

    def sync():
        engine.finish_pending()     # the heads' all-reduce + Adam of the last step (deferred across the step boundary)
        if grouped:
            dist.barrier()
        torch.cuda.synchronize()

    def run(steps, eng=engine):
        for _ in range(steps):
            out = eng.step(ex, mi, gt, epoch=1)
        return out

    # (Python's cyclic collector is held off over the warm-up and the timed steps: a generation-2 pass — 30 ms were observed in
    #  round 3 — inside a 60 ms timed region is a 50 % error that has nothing to do with the step)
    gc.collect()
    gc.disable()
    try:
        run(args.warmup)
        sync()
        t0 = time.perf_counter()
        out = run(args.steps)
        sync()
        dt = time.perf_counter() - t0
    finally:
        gc.enable()
    if grouped:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    loss = out["loss_all"].item()
    assert loss == loss, "NaN loss"
    if args.dump_outputs and rank == 0:
        # (before the side measurements below, which run more steps of this engine)
        dump_outputs(args.dump_outputs, train_step_outputs(out, model))
    ms_per_step = dt / args.steps * 1e3
    value = args.batch * world / (ms_per_step * 1e-3)

    if rank == 0:
        line = {
            "metric": f"train-step point-clouds/sec at B={args.batch}, N={args.points} (Chamfer+EMD)" if not args.no_emd
            else f"train-step point-clouds/sec at B={args.batch}, N={args.points} (Chamfer only)",
            "value": round(value, 2), "unit": "clouds/s", "n_gpus": world,
            "rccl_ranks": dist.get_world_size() if grouped else 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 storage / accumulation / results; matrix products formed from f16 x2 (bf16 x3) pieces of the fp32 operands — "
                     "NOT IEEE-fp32 products: the all-fp32-kernel step is `value_strict_fp32`",
            "data": "synthetic clouds U(-0.5,0.5)^3; model = seeded xavier init" + (
                f", hypernetwork heads x 2^-6, then {args.precondition} untimed steps of this engine on the bench batch (rec at gt's scale)"
                if args.precondition > 0 else " (rec at O(1e2): every EMD exponential underflows)"),
            "config": {"workload": f"HyperPocket 128+128 train step, B={args.batch}/GPU, existing/missing (B,{n_half},3), "
                                   f"gt (B,{args.points},3), loss 0.05*Chamfer + KLD/B" + ("" if args.no_emd else " + 0.05*EMD/N")
                                   + ", Adam lr 1e-4; timed at " + (f"the operating point {args.precondition} untimed training steps reach from the "
                                                                    "2^-6-scaled heads (rec fills gt's cube: the EMD carries mass and its culling sweeps see "
                                                                    "training-regime geometry); " if args.precondition > 0 else "the seeded init; ") + ("BASELINE.json configs[1] shape at the metric's B=64" if args.batch == 64
                                                           else f"BASELINE.json configs[1] (3D-EPN chair, Chamfer+EMD) at B={args.batch}"
                                                           if args.batch == 32 else f"the metric's shape at B={args.batch}"),
                       "global_batch": args.batch * world, "points": args.points, "parallelism": f"dp{world}",
                       "params": 43328515,
                       "arithmetic": "fp32 weights, fp32 accumulation, fp32 results throughout; the encoders' conv GEMMs form their "
                                     "products on the f16 matrix pipe from two f16 pieces per fp32 operand (three products), and since "
                                     "round 4 the hidden activations h1..h4 are STORED as such piece pairs with block exponents (22-23 "
                                     "significant bits, same bytes as fp32; error vs fp64 within 2.5x rms / 3x max of the fp32 fma chain's, "
                                     "pooled features within 2e-6: tests/test_model_gpu.py; HP_CONV_PRESPLIT=0 restores fp32 "
                                     "activations, HP_CONV_SPLIT=0 the fp32 MFMA GEMMs); the same split-f16 products carry the fused decoder's "
                                     "forward, the delta chain and the dW launch of the encoders' backward (HP_EB_CHAIN16=0: fp32 MFMA), and "
                                     "the hypernetwork heads' forward uses exact three-piece bf16 splits with six products (HP_HEADS_FWD=0: "
                                     "fp32 GEMM) - each with its own error-vs-fp64 test against the fp32 kernel it replaces"},
            "final_loss": loss,
        }
        if args.full and not args.no_extras:
            if emd_coef:
                line["roofline"] = roofline_emd(args.batch, args.points)
                line["roofline_mfma"] = roofline_widest_matrix_kernel(args.batch, n_half)
            else:       # Chamfer-only step: no EMD launches; the widest matrix kernel is the roofline object
                line["roofline"] = roofline_widest_matrix_kernel(args.batch, n_half)
            if world == 1:
                # informational: the reference-faithful Chamfer-only step on the same inputs
                from hyperpocket_amd import ops
                if emd_coef:
                    engine.emd_coef = 0.0
                    run(3)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    run(args.steps)
                    torch.cuda.synchronize()
                    ms2 = (time.perf_counter() - t1) / args.steps * 1e3
                    engine.emd_coef = emd_coef
                    line["breakdown"] = {"chamfer_only_ms_per_step": round(ms2, 4),
                                         "chamfer_only_clouds_per_s": round(args.batch / (ms2 * 1e-3), 2)}
                    # the same Chamfer+EMD step with EVERY kernel on its IEEE-fp32 form (fp32 MFMA / VALU fma; no f16 or bf16
                    # pieces): the number behind the line's dtype "f32" read strictly
                    with ops.strict_fp32():
                        run(3)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        run(args.steps)
                        sync()
                        ms32 = (time.perf_counter() - t1) / args.steps * 1e3
                    run(2)      # (back on the default kernels before anything else is timed)
                    torch.cuda.synchronize()
                    # top level: the figure to credit against an fp32 reference next to `value` (split-piece products)
                    line["value_strict_fp32"] = round(args.batch / (ms32 * 1e-3), 2)
                    line["ms_per_step_strict_fp32"] = round(ms32, 4)
                    line["breakdown"]["strict_fp32_ms_per_step"] = round(ms32, 4)
                    line["breakdown"]["strict_fp32_clouds_per_s"] = round(args.batch / (ms32 * 1e-3), 2)
                    line["breakdown"]["strict_fp32_what"] = ("the timed step with ops.strict_fp32(): conv stack, decoder forward, encoder "
                                                             "backward chain + dW and the heads' forward on their fp32 kernels")
                    # ... and the Chamfer-only iteration on the route the reference's untouched core/epoch_loops.py takes with the
                    # drop-in modules (host-pinned inputs, torch KLD, 3 x .item(), torch.optim.Adam), then with the documented
                    # one-line optimiser replacement
                    ms_t = dropin_route(args.batch, n_half, device, args.steps, "torch")
                    ms_f = dropin_route(args.batch, n_half, device, args.steps, "flat")
                    line["reference_loop"] = {
                        "what": "core/epoch_loops.py:15-39 as the reference drives it, with FullModel + ChamferLoss dropped in: Chamfer-only "
                                "loss (the reference's training loss), inputs .to(device) from pinned host memory, KLD in torch, 3 x .item() "
                                "per iteration, the caller's optimiser; median of three blocks of the timed iterations",
                        "clouds_per_s": round(args.batch / (ms_t * 1e-3), 2), "ms_per_step": round(ms_t, 4),
                        "optimizer": "torch.optim.Adam(full_model.parameters(), lr=1e-4) as core/main.py:62-66 builds it",
                        "with_flat_adam": {"clouds_per_s": round(args.batch / (ms_f * 1e-3), 2), "ms_per_step": round(ms_f, 4),
                                           "optimizer": "hyperpocket_amd.optim.FlatAdam(full_model, lr=1e-4): the one-line replacement of INTEGRATION.md"},
                        "engine_same_loss": {"clouds_per_s": round(args.batch / (ms2 * 1e-3), 2), "ms_per_step": round(ms2, 4),
                                             "what": "TrainEngine.step, Chamfer-only, batch resident in HBM, no host sync"},
                        "engine_over_reference_loop": round(ms_t / ms2, 3),
                        "gap_ms": {"optimizer (torch Adam - FlatAdam)": round(ms_t - ms_f, 4),
                                   "loop (FlatAdam route - engine: H2D copies, torch KLD, .item() syncs)": round(ms_f - ms2, 4)}}
            if world == 1 and not force_exchange and os.environ.get("HP_BENCH_NO_EXCHANGE_PROBE") is None:
                # what the multi-rank step's bookkeeping costs before a byte crosses a link: the same step in a ONE-rank RCCL group
                # in which every collective really runs (broadcast, factor gathers, in-place weight gather, both all-reduces, the
                # deferred waits) minus the plain step above.  N > 1 runs cannot separate it from the wire.  It runs as a CHILD
                # process (HP_BENCH_FORCE_EXCHANGE=1: the group is formed first, then the engine — the order of a real rank):
                # which hardware queue a HIP stream lands on depends on the order streams are created in, and a group formed late
                # inside this process (rounds 3-4) measured that accident, not the exchange (0.09 ... 2.4 ms with the same binary).
                try:
                    torch.cuda.synchronize()
                    def free_port():
                        with socket.socket() as sk:
                            sk.bind(("127.0.0.1", 0))
                            return str(sk.getsockname()[1])
                    env = dict(os.environ, HP_BENCH_FORCE_EXCHANGE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=free_port(),
                               HSA_ENABLE_IPC_MODE_LEGACY="0")
                    cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch),
                           "--points", str(args.points), "--precondition", str(args.precondition), "--no-extras", "--no-cpu-baseline"] + (["--no-emd"] if args.no_emd else [])
                    legs = []
                    for _ in range(2):      # (two children, the faster one: the first pays the box's cold caches)
                        env["MASTER_PORT"] = free_port()
                        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300)
                        rec = [json.loads(ln) for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
                        legs.append(rec[-1]["ms_per_step"])
                    # ... against the plain step measured the same way (a child, same steps), so that both sides share the cold start
                    env0 = {k: v for k, v in env.items() if k != "HP_BENCH_FORCE_EXCHANGE"}
                    plain = []
                    for _ in range(2):
                        p = subprocess.run(cmd, env=env0, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300)
                        rec = [json.loads(ln) for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
                        plain.append(rec[-1]["ms_per_step"])
                    ms_x, ms_0 = min(legs), min(plain)
                    line.setdefault("breakdown", {})["one_rank_rccl_exchange"] = {
                        "ms_per_step": round(ms_x, 4), "plain_ms_per_step": round(ms_0, 4), "exposed_comm_ms": round(ms_x - ms_0, 4),
                        "what": "the multi-rank step (sharded heads update + bucketed all-reduces over RCCL) in a one-rank group minus the plain "
                                "one-GPU step, each as a child process of this run (the group formed before the engine, as in a real rank): "
                                "bookkeeping of the exchange, no wire time"}
                except Exception as exc:      # (informational leg: never fail the line over it)
                    line.setdefault("breakdown", {})["one_rank_rccl_exchange"] = {"error": repr(exc)[:200]}
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(n_half, emd_coef, full_b=args.batch)
        print(json.dumps(line), flush=True)
    if grouped:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

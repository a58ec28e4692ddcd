#!/usr/bin/env python3
"""Point-cloud previews on the GPU (GPU box only): what one picture costs, and where the time goes.  A record, not a gate.

    python tools/bench_render.py [--out profiles/render.json] [--repeats 20] [--no-trace]

1. The kernel, at B = 64 clouds of 2048 points plus an overlay layer of 1024, one view, 500 x 500: per tile side (32, 64, 128)
   and for the default radii (radius2 2 and 9) and for radius2 64 on both layers,
     - kernel time from a `rocprofv3 --kernel-trace --stats` run of its own (a child process that does nothing but these
       launches in a fixed order; the dispatches of render_points_kernel are cut into the configurations by count), and
     - device-event time of one call, the configurations alternated, warmed up.
   Both are reported per call and per image (/ 64).  The images of all tile sides are compared bit for bit first.
2. End to end through core/experiments.py fixed(): 16 scans x 10 noises in batches of 8, with and without save_plots, the
   difference over the 176 PNGs written; and the same pictures step by step — render (device events), device -> host copy and
   write_png at zlib levels 1 and 6 (host clock), with the PNG sizes and the share of pixels that are not background.
   The model is the seeded init with the hypernetwork heads scaled by the power of two (exact) that brings the spread of
   its completions closest to 0.25, the scale of the cube; the numbers do not depend on what the clouds show beyond how
   well the pictures compress, so the last three steps are also timed on the pictures of part 1's shells.
3. matplotlib's 3-D scatter + savefig of one 2048-point cloud on this host, if matplotlib imports; otherwise the figure
   measured on the CPU-only development machine is quoted and labelled as such.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd"))

B, N_POINTS, N_OVERLAY, SIZE = 64, 2048, 1024, (500, 500)
TILES = (32, 64, 128)
WARMUP = 3
MODEL_CFG = {"random_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
             "real_encoder": {"output_size": 128, "use_bias": True, "relu_slope": 0.2},
             "hyper_network": {"use_bias": True, "relu_slope": 0.2},
             "target_network": {"use_bias": True, "relu_slope": 0.2, "freeze_layers_learning": False,
                                "layer_out_channels": [32, 64, 128, 64]},
             "target_network_input": {"constant": False, "normalization": {"enable": True, "type": "progressive", "epoch": 100}}}


def radii():
    from hyperpocket_amd.utils import render as R
    return {"default": [R.DEFAULT_RADIUS2, R.DEFAULT_OVERLAY_RADIUS2], "radius2_64": [64, 64]}


def configurations():
    return [(side, name) for side in TILES for name in radii()]


def shapes():
    """B shells of 2048 points (radius 0.25 .. 0.45, squeezed along one axis) and 1024 overlay points in the cube."""
    r = np.random.RandomState(5)
    d = r.standard_normal((B, N_POINTS, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    shell = d * r.uniform(0.25, 0.45, (B, 1, 1)) * np.array([1.0, 0.6, 0.8])
    over = (r.rand(B, N_OVERLAY, 3) - 0.5) * 0.8
    return torch.from_numpy(np.concatenate([shell, over], 1).astype(np.float32)).cuda()


def launcher(points):
    from hyperpocket_amd import ops
    from hyperpocket_amd.utils import render as R
    views = torch.from_numpy(R.DEFAULT_VIEW[None].copy()).cuda()
    image = torch.empty((B, 1, SIZE[1], SIZE[0], 3), dtype=torch.uint8, device="cuda")
    ends, lib = [N_POINTS, N_POINTS + N_OVERLAY], ops.load_library()

    def run(side, name):
        lib.hp_render_points_set_tile(side)
        try:
            return ops.render_points(points, ends, R.DEFAULT_PALETTE, radii()[name], views, SIZE, fog=R.DEFAULT_FOG, out=image)
        finally:
            lib.hp_render_points_set_tile(0)
    return run


def trace_child(repeats):
    run = launcher(shapes())
    for side, name in configurations():
        for _ in range(WARMUP + repeats):
            run(side, name)
    torch.cuda.synchronize()


def kernel_trace(repeats):
    """Median kernel microseconds per configuration from a rocprofv3 run of the child, or {"error": ...}."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="render_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
               "--trace-child", "--repeats", str(repeats)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if done.returncode != 0 or not files:
            return {"error": f"rocprofv3 exit {done.returncode}, {len(files)} trace files", "tail": done.stdout.decode(errors="replace")[-400:]}
        rows = [r for f in files for r in csv.DictReader(open(f)) if "render_points_kernel" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        per = WARMUP + repeats
        if len(rows) != per * len(configurations()):
            return {"error": f"{len(rows)} dispatches traced, {per * len(configurations())} expected"}
        res = {}
        for c, (side, name) in enumerate(configurations()):
            us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[c * per + WARMUP:(c + 1) * per])
            res[f"tile{side}_{name}"] = {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
                                        "per_image_us": round(us[len(us) // 2] / B, 3), "dispatches": len(us)}
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def median(v):
    return sorted(v)[len(v) // 2]


def kernel_events(repeats):
    from hyperpocket_amd import ops
    run = launcher(shapes())
    first, same = {}, True
    for side, name in configurations():
        image = run(side, name).clone()
        same = same and torch.equal(first.setdefault(name, image), image)
    ms = {c: [] for c in configurations()}
    for _ in range(WARMUP + repeats):
        for c in configurations():
            ms[c].append(event_ms(lambda: run(*c)))
    res = {"same_bits_under_every_tile": bool(same)}
    for (side, name), v in ms.items():
        v = v[WARMUP:]
        lib = ops.load_library()
        lib.hp_render_points_set_tile(side)
        plan = ops.render_points_plan(B, 1, SIZE)
        lib.hp_render_points_set_tile(0)
        res[f"tile{side}_{name}"] = {"median_ms": round(median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                                    "per_image_us": round(median(v) * 1e3 / B, 3), "calls": len(v),
                                    "plan": {"tiles": plan.tiles, "threads": plan.threads, "lds_bytes": plan.lds_bytes,
                                             "workgroups": plan.workgroups}}
    res["default_tile"] = ops.render_points_plan(B, 1, SIZE).tile_w
    return res


def through_fixed():
    import copy
    from hyperpocket_amd.core.experiments import fixed
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel
    from hyperpocket_amd.utils import render as R
    torch.manual_seed(2020)
    model = FullModel(copy.deepcopy(MODEL_CFG))
    model.apply(weights_init)
    model = model.cuda().eval()
    r = np.random.RandomState(9)
    items = [((r.rand(1024, 3).astype(np.float32) - 0.5) * np.array([1.0, 0.5, 0.7], np.float32), 0, 0, i) for i in range(16)]
    with torch.no_grad():
        heads = [head.weight for head in model.hyper_network.output]
        base = [w.clone() for w in heads]
        probe = torch.from_numpy(np.stack([it[0] for it in items[:8]])).cuda()
        noise = torch.empty(8, model.get_noise_size()).normal_(mean=0.0, std=0.015).cuda()
        spread = {}
        for e in range(8, -13, -1):
            for w, b in zip(heads, base):
                w.copy_(b * 2.0 ** e)
            spread[e] = float(model.sample_completions(probe, noise, 2048, 1).std())
        log2_scale = min(spread, key=lambda e: abs(np.log(max(spread[e], 1e-30) / 0.25)))
        for w, b in zip(heads, base):
            w.copy_(b * 2.0 ** log2_scale)
    out = tempfile.mkdtemp(prefix="render_fixed_")
    try:
        wall = {}
        for plots in (False, True, False, True):                   # the first pair warms up
            torch.manual_seed(1)
            wall[plots], (_, generated) = host_ms(lambda: fixed(model, torch.device("cuda"), {"bench": items}, out, 1,
                                                                noises_per_item=10, batch_size=8, save_plots=plots))
        pngs = len([f for f in os.listdir(os.path.join(out, "fixed")) if f.endswith(".png")])
        clouds = generated[:8].flatten(0, 1).contiguous()          # one batch's completions: 80 clouds
        K = clouds.size(0)
        R.render_clouds(clouds)
        render = median([event_ms(lambda: R.render_clouds(clouds)) for _ in range(10)])
        images = R.render_clouds(clouds)[:, 0]
        copy_ms = median([host_ms(lambda: images.cpu())[0] for _ in range(5)])
        host = images.cpu().numpy()
        res = {"heads_scale_log2": log2_scale, "pngs": pngs, "fixed_ms_without_plots": round(wall[False], 2), "fixed_ms_with_plots": round(wall[True], 2),
               "ms_per_png_end_to_end": round((wall[True] - wall[False]) / pngs, 3),
               "clouds_in_the_split": K, "foreground_share": round(float((host != 255).any(3).mean()), 4),
               "completion_spread": round(float(clouds.std()), 4),
               "render_ms_per_png": round(render / K, 4), "copy_ms_per_png": round(copy_ms / K, 4)}
        res.update(write_png_ms(host, out))
        res["write_png_level_in_use"] = R.PNG_LEVEL
        return res, host[0]
    finally:
        shutil.rmtree(out, ignore_errors=True)


def write_png_ms(host, out):
    """write_png of the pictures host (K,H,W,3) at zlib levels 1 and 6: milliseconds and bytes per PNG."""
    from hyperpocket_amd.utils import render as R
    res, K = {}, len(host)
    for level in (1, 6):
        t = time.perf_counter()
        for k in range(K):
            R.write_png(os.path.join(out, f"{k}.png"), host[k], level=level)
        res[f"write_png_level{level}_ms_per_png"] = round((time.perf_counter() - t) * 1e3 / K, 3)
        res[f"png_level{level}_bytes"] = int(np.mean([os.path.getsize(os.path.join(out, f"{k}.png")) for k in range(K)]))
    return res


def shell_pictures():
    """The copy and write_png steps on the pictures of part 1's shells under the default radii."""
    images = launcher(shapes())(0, "default")[:, 0]
    copy_ms = median([host_ms(lambda: images.cpu())[0] for _ in range(5)])
    host = images.cpu().numpy()
    out = tempfile.mkdtemp(prefix="render_shells_")
    try:
        res = {"pictures": len(host), "foreground_share": round(float((host != 255).any(3).mean()), 4),
               "copy_ms_per_png": round(copy_ms / len(host), 4)}
        res.update(write_png_ms(host, out))
        return res, host[0]
    finally:
        shutil.rmtree(out, ignore_errors=True)


def matplotlib_ms():
    quoted = {"seconds_per_plot": [0.14, 0.16], "where": "quoted: measured on the CPU-only development machine, not on this host"}
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return quoted
    p = np.random.RandomState(0).rand(3, 2048) - 0.5
    out = tempfile.mkdtemp(prefix="render_mpl_")
    try:
        times = []
        for k in range(6):
            t = time.perf_counter()
            fig = plt.figure(figsize=(5, 5))
            ax = fig.add_subplot(111, projection="3d")
            ax.scatter(p[0], p[1], p[2], marker=".", s=8, alpha=0.8)
            ax.view_init(elev=10, azim=240)
            for set_lim in (ax.set_xlim3d, ax.set_ylim3d, ax.set_zlim3d):
                set_lim(-0.5, 0.5)
            plt.tight_layout()
            fig.savefig(os.path.join(out, f"{k}.png"))
            plt.close(fig)
            times.append(time.perf_counter() - t)
        return {"seconds_per_plot": round(median(times[1:]), 4), "where": "measured on this host", "plots": len(times) - 1}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child run")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--sample", default=None, help="also write one picture of fixed() and one of the shells into this directory")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.repeats)
    result = {"shape": {"B": B, "points": N_POINTS, "overlay": N_OVERLAY, "size": list(SIZE), "views": 1}}
    if not args.no_trace:                                          # before this process opens the GPU
        result["kernel_trace"] = kernel_trace(args.repeats)
        print("kernel_trace", json.dumps(result["kernel_trace"]), flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py measures on the GPU: none here")
    result["device"] = torch.cuda.get_device_name(0)
    result["kernel_events"] = kernel_events(args.repeats)
    print("kernel_events", json.dumps(result["kernel_events"]), flush=True)
    result["through_fixed"], sample = through_fixed()
    print("through_fixed", json.dumps(result["through_fixed"]), flush=True)
    result["shell_pictures"], shell = shell_pictures()
    print("shell_pictures", json.dumps(result["shell_pictures"]), flush=True)
    result["matplotlib"] = matplotlib_ms()
    if args.sample:
        from hyperpocket_amd.utils.render import write_png
        os.makedirs(args.sample, exist_ok=True)
        write_png(os.path.join(args.sample, "fixed.png"), sample)
        write_png(os.path.join(args.sample, "shells.png"), shell)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()

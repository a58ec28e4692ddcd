#!/usr/bin/env python3
"""How many set2 points does each EMD annealing level still sweep?  GPU box.

A set2 point whose remainR has been clamped to exactly +0 (approxmatch.cu:141, `a >= 1`: the point is oversubscribed) stays at 0
for every later level: its own phase-2 row gives ratioR = 0, and as a candidate it adds exact zeros to phases 1 and 3.  This tool
rebuilds bench.py's operating point (hypernetwork heads x 2^-6, then `--precondition` engine steps on the bench batch), runs one
more step with the EMD call's workspace kept, and reports per level the share of set2 points with ratioR_lev != 0 (read from the
final records, emd.hip ws_layout), plus the share of the plain level launches' pair work that is not an exact zero (the
phase-1/3 launch of levels 2..7 weighted 38 cycles per row-candidate, the phase-2 launch of levels 3..8 weighted 24: DESIGN §4).

    python tools/emd_alive_share.py [--precondition 400] [OUT.json]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402

LEVELS = [-16384, -4096, -1024, -256, -64, -16, -4, -1, -0.25]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--precondition", type=int, default=400)
    ap.add_argument("out", nargs="?")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    from hyperpocket_amd._lib import load_library
    from hyperpocket_amd.core import engine as engine_mod
    from hyperpocket_amd.core.setup import weights_init
    from hyperpocket_amd.model.full_model import FullModel

    torch.manual_seed(2020)                     # bench.py main(): the same model, batch and operating point
    model = FullModel(copy.deepcopy(bench.MODEL_CFG))
    model.apply(weights_init)
    model = model.to(device)
    torch.manual_seed(2020)
    with torch.no_grad():
        for head in model.hyper_network.output:
            head.weight.mul_(2.0 ** -6)
    engine = engine_mod.TrainEngine(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, loss_coef=0.05, emd_coef=0.05)
    ex, mi, gt = bench.synth_batch(args.batch, args.points // 2, device, 2020)
    for _ in range(args.precondition):
        engine.step(ex, mi, gt, epoch=1)
    engine.finish_pending()

    kept = {}
    plain_call = engine_mod.call

    def call(name, *a):       # keep the EMD call's workspace (the engine allocates it per step)
        if name == "hp_emd_forward_acc":
            kept["ws"] = a[6]
        return plain_call(name, *a)
    engine_mod.call = call
    try:
        engine.step(ex, mi, gt, epoch=1)
        engine.finish_pending()
    finally:
        engine_mod.call = plain_call
    torch.cuda.synchronize()

    B, N = args.batch, args.points
    per = load_library().hp_approxmatch_workspace_floats(1, N, N)
    P = (N + 63) // 64 * 64
    frp = 2 * (P + 8) * 4 + (P + 8) + (P + 8) * 16          # plp, prp, rr, flp: emd.hip ws_layout (n == m)
    rec = kept["ws"].view(B, per)[:, frp:frp + (P + 8) * 16].reshape(B, (P + 8) // 2, 32)[:, :N // 2]
    share = []
    for lev in range(len(LEVELS)):
        r = rec[:, :, 6 + 2 * lev:8 + 2 * lev]
        share.append(round((r != 0).float().mean().item(), 4))
    rows1 = sum(38 * share[j] for j in range(2, 8)) / (38 * 6)
    rows2 = sum(24 * share[j] for j in range(3, 9)) / (24 * 6)
    work = (sum(38 * share[j] for j in range(2, 8)) + sum(24 * share[j] for j in range(3, 9))) / (6 * 38 + 6 * 24)
    out = {"what": "share of set2 (rec) points with ratioR_lev != 0 at each level, bench.py operating point "
                   f"(B={B}, N={N}, heads x 2^-6, {args.precondition} engine steps, then one step read back)",
           "levels": LEVELS, "alive_share": share,
           "plain_launch_nonzero_work": {"rows1_levels_2_7": round(rows1, 4), "rows2_levels_3_8": round(rows2, 4),
                                         "weighted": round(work, 4)}}
    print(json.dumps(out), flush=True)
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()

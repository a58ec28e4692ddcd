#!/usr/bin/env python3
"""The hardware reciprocal, logarithm and exponential as the exact t-SNE kernels use them (GPU box only): each measured
once through a kernel of csrc/tsne.hip against float64.  The figures are RCP_MEASURED, LOG_MEASURED and EXP_MEASURED of
tests/tsne_law.py and are recorded in profiles/tsne_parity.md.  A record, not a gate.

    python tools/tsne_accuracy_probe.py

Reciprocal and logarithm: hp_tsne_gradient at n = 2 with P_01 = P_10 = 1, y_0 = 0.  Row 0's z is its only term w_01 =
rcp(1 + |y_1|^2), whose argument is reproduced here in fp32, and its KL row is 1 * (log 1 - log w_01) = -log w_01.
Exponential: hp_tsne_affinities at n = 3 on a line; the workspace holds C, and C_02 / C_01 = exp(-beta e_02) for the beta
the call returns — beside the roundings of the product with log2(e) and of the two divisions, which the figure includes.
Last, one calibration at the largest n the library takes, its whole row in LDS.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3d-point-clouds-autocomplete_amd")]
from hyperpocket_amd import ops
U = 2.0 ** -24
print("device", torch.cuda.get_device_name(0), "LDS per block", torch.cuda.get_device_properties(0).shared_memory_per_block, flush=True)
r = np.random.RandomState(0)
K = 3000
# rcp and log
mag = 10.0 ** r.uniform(-3, 3, K)
ang = r.uniform(0, 2 * math.pi, K)
pts = np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1).astype(np.float32)
P = torch.tensor([[0.0, 1.0], [1.0, 0.0]], device="cuda")
rows = []
kl = torch.zeros(3, device="cuda")
for k in range(K):
    Y = torch.tensor([[0.0, 0.0], [float(pts[k, 0]), float(pts[k, 1])]], device="cuda")
    rows.append(ops.tsne_gradient_rows(P, Y, 1.0, kl=kl)[0].clone())
rows = torch.stack(rows).cpu().numpy()
dx, dy = np.float32(0) - pts[:, 0], np.float32(0) - pts[:, 1]
arg = (np.float32(1) + (dx * dx + dy * dy)).astype(np.float32)
w = rows[:, 4]
want = 1.0 / arg.astype(np.float64)
rel = np.abs(w.astype(np.float64) - want) / want
i = rel.argmax()
print(f"RCP: max rel err {rel.max():.4e} = {rel.max() / U:.3f} u at argument {arg[i]!r}; arguments in [{arg.min()}, {arg.max()}]", flush=True)
lw = np.log(w.astype(np.float64))
ok = (w < 1) & (w >= 2.0 ** -20)
err = np.abs(-rows[:, 5].astype(np.float64) - lw) / np.maximum(1.0, np.abs(lw))
i = np.where(ok, err, 0).argmax()
print(f"LOG: max |err| / max(1, |log w|) {err[ok].max():.4e} = {err[ok].max() / U:.3f} u at w = {w[i]!r}; {ok.sum()} samples, w in [{w[ok].min()}, {w[ok].max()}]", flush=True)
print("LOG at w == 1:", np.abs(rows[:, 5][w == 1]).max() if (w == 1).any() else "none")
# exp
worst, at = 0.0, None
ts = []
for k in range(600):
    a, b = 10.0 ** r.uniform(-2, 2), 10.0 ** r.uniform(-2, 2)
    x = np.array([[0.0], [a], [a + b + a]], np.float32)       # row 0: nearest 1, then 2
    D = ((x - x.T) ** 2).astype(np.float32)
    Dd = torch.from_numpy(D).cuda()
    ws = torch.zeros(3 * 3 + 4, device="cuda")
    Pj, beta, steps = ops.tsne_affinities(Dd, 1.0 + r.uniform(0.05, 0.95), ws=ws)
    C = ws[:9].view(3, 3).cpu().numpy().astype(np.float64)
    bk = float(beta[0].item())
    e = float(np.float32(D[0, 2] - D[0, 1]))
    t = float(np.float32(e * np.float32(bk)))                   # the product as the kernel rounds it
    if C[0, 2] < 1e-30:
        continue
    got = C[0, 2] / C[0, 1]
    rel = abs(got - math.exp(-t)) / math.exp(-t)
    ts.append(t)
    if rel > worst:
        worst, at = rel, (t, bk, e)
print(f"EXP: max rel err of C02/C01 against exp(-fl(beta e)) {worst:.4e} = {worst / U:.3f} u at (t, beta, e) = {at}; t in [{min(ts):.3g}, {max(ts):.3g}], {len(ts)} samples", flush=True)
# the largest n: one calibration launch with the whole row in LDS
n = 16384
X = torch.randn(n, 8, device="cuda")
D = ops.pairwise_sqdist(X)
Pj, beta, steps = ops.tsne_affinities(D, 30.0)
torch.cuda.synchronize()
print("n = 16384: steps", int(steps.min()), int(steps.max()), "sum P", float(Pj.double().sum()), "symmetric", bool(torch.equal(Pj, Pj.t())), flush=True)

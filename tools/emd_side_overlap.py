#!/usr/bin/env python3
"""How much of the EMD call runs beside the loss side stream's kernels, from a `rocprofv3 --kernel-trace --output-format csv` trace
of the bench command (`bench.py --gpus 1 --steps 5 --warmup 2`).

For each of the last 7 steps in the trace it takes every kernel hp_emd_forward_acc launched (from the first emd_order_kernel to the
emd_cost_finish_kernel behind the emd_grad2_kernel) and the side-stream kernels of the same step (nn_distance_kernel,
nn_grad_side_kernel, kld*, sample_points_kernel, torch's normal draw), and reports, in µs:

  * per step: the EMD call's span, the side section's span (first start to last end of those kernels), how long the side section
    runs past the start of the call, the summed duration of the EMD kernels and the part of it spent beside a side-stream kernel,
    and the gap in front of the final sweep (emd_grad2_kernel's start minus the last end of anything it waits for: the level
    launches of both chains and the side section);
  * with -v, every EMD kernel of those steps: start relative to the call, duration, overlapped share;
  * per kernel name: launches and median duration, split into "overlapped" (a side-stream kernel ran during at least 10 % of
    the launch) and "not overlapped";
  * the side-stream kernels: median / min / max duration per name.

    python tools/emd_side_overlap.py TRACE.csv [-v]
"""
import csv
import re
import statistics as st
import sys

SIDE = ("nn_distance_kernel", "nn_grad_side_kernel", "kld", "sample_points_kernel")
SHARE = 0.10      # a launch counts as overlapped from this share of its duration on


def is_side(name):
    return any(k in name for k in SIDE) or ("at::native" in name and "normal" in name.lower())


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):      # cut the argument list, keep the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def covered(s, e, spans):
    """length of [s, e) covered by the union of `spans` (sorted, possibly overlapping)"""
    tot, cur = 0, s
    for a, b in spans:
        a, b = max(a, cur), min(b, e)
        if b > a:
            tot += b - a
            cur = b
    return tot


def main(path, verbose):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    t = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "emd_order_kernel" in r["Kernel_Name"]][::2]
    per_name, side_dur, steps = {}, {}, []
    for i0 in starts[-7:]:
        j = i0
        while "emd_cost_finish_kernel" not in rows[j]["Kernel_Name"]:
            j += 1
        emd = [r for r in rows[i0:j + 1] if "emd_" in r["Kernel_Name"]]
        t0, t1 = t(emd[0])[0], t(emd[-1])[1]
        # the side section of this step: enqueued in front of the call, so it may start up to a few launches before the order kernel
        side = [r for r in rows if is_side(r["Kernel_Name"]) and t(r)[1] > t0 - 300_000 and t(r)[0] < t1]
        spans = sorted(t(r) for r in side)
        for r in side:
            side_dur.setdefault(short(r["Kernel_Name"]), []).append((t(r)[1] - t(r)[0]) / 1e3)
        g2 = next(r for r in emd if "emd_grad2_kernel" in r["Kernel_Name"])
        before = [t(r)[1] for r in emd if t(r)[0] < t(g2)[0] and r is not g2] + [e for _, e in spans]
        tot = ov = 0
        for r in emd:
            s, e = t(r)
            c = covered(s, e, spans)
            tot += e - s
            ov += c
            share = c / max(1, e - s)
            per_name.setdefault(short(r["Kernel_Name"]), {True: [], False: []})[share >= SHARE].append((e - s) / 1e3)
            if verbose:
                print(f"step {len(steps)}  +{(s - t0) / 1e3:8.1f}  {(e - s) / 1e3:7.1f} us  {100 * share:5.1f} %  q{r['Queue_Id']:>3}  {short(r['Kernel_Name'])}")
        steps.append({"emd_span": (t1 - t0) / 1e3,
                      "side_span": (max(e for _, e in spans) - min(s for s, _ in spans)) / 1e3 if spans else 0.0,
                      "side_past_emd_start": (max(e for _, e in spans) - t0) / 1e3 if spans else 0.0,
                      "emd_kernel_sum": tot / 1e3, "of_it_beside_side": ov / 1e3,
                      "gap_before_grad2": (t(g2)[0] - max(before)) / 1e3})
    for k in steps[0]:
        v = [s[k] for s in steps]
        print(f"{k:21s} median {st.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
    print()
    print("| kernel | overlapped: launches | median µs | not overlapped: launches | median µs |")
    print("|---|---:|---:|---:|---:|")
    med = lambda v: f"{st.median(v):.1f}" if v else "-"
    for name, d in per_name.items():
        print(f"| `{name}` | {len(d[True])} | {med(d[True])} | {len(d[False])} | {med(d[False])} |")
    print()
    print("| side-stream kernel | launches | median µs | min | max |")
    print("|---|---:|---:|---:|---:|")
    for name, v in side_dur.items():
        print(f"| `{name[:72]}` | {len(v)} | {st.median(v):.1f} | {min(v):.1f} | {max(v):.1f} |")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], "-v" in sys.argv[2:])

#!/usr/bin/env python3
"""Per-level durations of the plain EMD level launches, from a ONE-chain kernel trace of the bench command
(`HP_EMD_CHAINS=1 rocprofv3 --kernel-trace --output-format csv -- python bench.py --gpus 1 --steps 5 --warmup 2`).

With one chain no two level launches overlap and every step holds one emd_order_kernel launch, so the i-th launch of a kernel
inside a step is that kernel's i-th level: for the list-driven phase-2 sweep (`emd_rows2_kernel<R, 2>`) levels 3..8, for the
compacted phase-1/3 sweep (`emd_rows1_kernel<true, true, R, true>`) the merged launches (2,3)..(7,8).  Prints, per kernel and
position, the median / min / max duration in µs over the last `--last` steps, as a markdown table; with --alive a JSON of
tools/emd_alive_share.py supplies the share of set2 points alive on entry to the level next to the phase-2 rows.

    python tools/emd_level_durations.py TRACE.csv [--alive ALIVE.json] [--last 7]
"""
import argparse
import csv
import json
import re
import statistics as st

KERNELS = (("phase 2", re.compile(r"emd_rows2_kernel<\d, [12](, [01])?>"), 3),
           ("phase 3 + 1", re.compile(r"emd_rows1_kernel<true, true, \d, true>"), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--alive")
    ap.add_argument("--last", type=int, default=7)
    args = ap.parse_args()
    rows = sorted(csv.DictReader(open(args.trace)), key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "emd_order_kernel" in r["Kernel_Name"]]
    steps = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])][-args.last:]
    alive = json.load(open(args.alive))["alive_share"] if args.alive else None
    print("| launch | kernel | level | alive on entry | median µs | min µs | max µs |\n|---|---|---:|---:|---:|---:|---:|")
    for what, pat, first in KERNELS:
        per = {}
        names = set()
        for s in steps:
            hits = [r for r in s if pat.search(r["Kernel_Name"])]
            for i, r in enumerate(hits):
                per.setdefault(i, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                names.add(pat.search(r["Kernel_Name"]).group(0))
        for i in sorted(per):
            v = per[i]
            lev = first + i
            share = f"{alive[lev]:.2f}" if alive and what == "phase 2" and lev < len(alive) else ""
            label = str(lev) if what == "phase 2" else f"{lev}, {lev + 1}"
            print(f"| {what} | `{'/'.join(sorted(names))}` | {label} | {share} | {st.median(v):.1f} | {min(v):.1f} | {max(v):.1f} |")


if __name__ == "__main__":
    main()

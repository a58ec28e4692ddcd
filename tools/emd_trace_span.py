#!/usr/bin/env python3
"""Where the EMD call's time goes, from a `rocprofv3 --kernel-trace --output-format csv` trace of the bench command.

For each of the last 7 steps in the trace (one hp_emd_forward_acc call each: two chains, from the first emd_order_kernel to the
emd_grad2_kernel), in µs: the call's span; the span of the order kernels, of the culling launches, and of the plain level launches
with the compaction launches between them (first start to last end over both chains); the final sweep; the summed duration of the
compaction launches; and the host-bound gaps — the idle time between consecutive level launches on one stream (max and sum).
Prints the median, min and max over those steps.

    python tools/emd_trace_span.py TRACE.csv
"""
import csv
import statistics as st
import sys


def main(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "emd_order_kernel" in r["Kernel_Name"]][::2]
    t = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
    span = lambda v: (max(e for _, e in v) - min(s for s, _ in v)) / 1e3 if v else 0.0
    res = []
    for i0 in starts[-7:]:
        j = i0
        while "emd_grad2_kernel" not in rows[j]["Kernel_Name"]:
            j += 1
        emd = [r for r in rows[i0:j + 1] if "emd_" in r["Kernel_Name"]]
        name = lambda r: r["Kernel_Name"]
        plain = [t(r) for r in emd if any(k in name(r) for k in ("emd_rows1_kernel", "emd_rows2_kernel", "emd_compact_kernel"))]
        comp = [t(r) for r in emd if "emd_compact_kernel" in name(r)]
        by = {}
        for r in emd[:-1]:
            by.setdefault(r["Queue_Id"], []).append(t(r))
        gaps = []
        for v in by.values():
            v.sort()
            gaps += [max(0, b[0] - a[1]) for a, b in zip(v, v[1:])]
        res.append({"span": (t(emd[-1])[1] - t(emd[0])[0]) / 1e3,
                    "order": span([t(r) for r in emd if "emd_order_kernel" in name(r)]),
                    "culling": span([t(r) for r in emd if "cull_kernel" in name(r)]),
                    "plain+compact": span(plain), "final_sweep": span([t(emd[-1])]),
                    "compact_sum": sum(e - s for s, e in comp) / 1e3, "compact_launches": len(comp),
                    "gap_max": max(gaps) / 1e3, "gap_sum_per_stream": sum(gaps) / 1e3 / len(by)})
    for k in res[0]:
        v = [r[k] for r in res]
        print(f"{k:19s} median {st.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")


if __name__ == "__main__":
    main(sys.argv[1])

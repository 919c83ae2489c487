#!/usr/bin/env python3
"""Per-iteration launch table of an NMF HALS loop from a `rocprofv3 --kernel-trace` csv (t_kernel_trace.csv).

    python tools/trace_step_table.py <kernel_trace.csv> [--last N] [--json OUT]

An iteration runs from one launch of the U-side sweep kernel (`--anchor`, default nnf_hals_kernel) to the next.  For the last N
iterations (default 15: the steady state, past the long solves of a cold start) it prints, per iteration and as medians:
the launches on the main stream (the stream of the anchor) and on every other stream, the summed kernel time of the main
stream, the step time, and the step time that belongs to no main-stream kernel (step - sum).  Kernel names are cut at the
first '(' or '<'."""
import argparse
import csv
import json
import statistics
from collections import Counter


def short(name):
    name = name.replace("void ", "")
    for ch in "(<":
        if ch in name:
            name = name[:name.index(ch)]
    return name.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--last", type=int, default=15)
    ap.add_argument("--anchor", default="nnf_hals_kernel")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    with open(a.trace, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r["Stream_Id"]))
    rows.sort()
    anchors = [i for i, r in enumerate(rows) if r[2] == a.anchor]
    if len(anchors) < 3:
        raise SystemExit(f"fewer than three launches of {a.anchor} in {a.trace}")
    main_stream = rows[anchors[-1]][3]
    spans = list(zip(anchors[:-1], anchors[1:]))[-a.last:]
    per_iter, names_main, names_side = [], Counter(), Counter()
    for i0, i1 in spans:
        it = rows[i0:i1]
        on_main = [r for r in it if r[3] == main_stream]
        side = [r for r in it if r[3] != main_stream]
        step = (rows[i1][0] - rows[i0][0]) / 1e3
        busy = sum(r[1] - r[0] for r in on_main) / 1e3
        per_iter.append({"main_launches": len(on_main), "side_launches": len(side), "main_kernel_us": busy, "step_us": step,
                         "unaccounted_us": step - busy})
        names_main.update(r[2] for r in on_main)
        names_side.update(r[2] for r in side)
    med = {k: statistics.median(p[k] for p in per_iter) for k in per_iter[0]}
    n = len(per_iter)
    out = {"iterations": n, "median": med,
           "main_stream_kernels_per_iteration": {k: v / n for k, v in names_main.most_common()},
           "side_stream_kernels_per_iteration": {k: v / n for k, v in names_side.most_common()}}
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(out, per_iteration=per_iter), f, indent=1)


if __name__ == "__main__":
    main()

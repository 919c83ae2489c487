#!/usr/bin/env python3
"""Times of the weighted mode update on the tensor's own layout (nnf_mu_mode_w_f32 + nothing else: the raw sums) next to the
unweighted one (nnf_mu_mode_f32, whose call also finishes the update) and to the unfolded weighted route (nnf_mu_right_w_f32 on
materialised unfoldings of the tensor and of the weights, made before the clock starts), at the NTF bench shape.

    python tools/probes/mu_mode_w_probe.py [--shape 500 500 500] [--rank 30] [--betas 0.5 1] [--modes 0 1] [--calls 100]
                                           [--reps 9] [--warmup 2] [--out FILE.json]

One sample is `--calls` back-to-back calls of one entry between two device events, over the calls; the three entries alternate
sample by sample; median, min and max over `--reps` samples after `--warmup` samples each.  Bytes the algorithm needs per call,
from the shapes: the tensor once (+ the weights once) + the Khatri-Rao operand once per row block of 64 rows of the mode (the
on-layout kernels; once for the unfolded route) + the factor and the outputs; achieved bytes/s = those bytes over the median.
spread_unfold = (max - min) / median of the unfolded route's own samples: the yardstick the on-layout weighted update is held to.
Needs a MI355X (no CPU fallback).

    python tools/probes/mu_mode_w_probe.py --table OUT.json PROBE.json NEW.jsonl PARENT.jsonl
        no GPU: puts the lines of `python tools/time_ntf_mu.py --routes native` on this tree (NEW) and on a built tree of the parent
        commit (PARENT; --root), taken alternately in the same session, next to the probe's cases in one file
        (profiles/mu_mode_w.json): the unweighted NTF MU iteration of both commits, median of each run's medians, and the spread
        (max - min) / median over all of a commit's calls."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def table(out_path, probe_path, new_path, parent_path):
    doc = json.load(open(probe_path))
    load = lambda p: [json.loads(l) for l in open(p) if l.strip()]
    rows = []
    for beta in sorted({r["beta"] for r in load(new_path)}):
        row = {"beta": beta}
        for label, path in (("new", new_path), ("parent", parent_path)):
            runs = [r for r in load(path) if r["beta"] == beta]
            med = statistics.median(r["ms_per_iter"] for r in runs)
            lo, hi = min(r["min_ms_per_iter"] for r in runs), max(r["max_ms_per_iter"] for r in runs)
            row.update(shape=runs[0]["shape"], rank=runs[0]["rank"], iters=runs[0]["iters"])
            row[label] = {"ms_per_iter": med, "min": lo, "max": hi, "spread": round((hi - lo) / med, 3),
                          "runs": [r["ms_per_iter"] for r in runs]}
        row["new_over_parent"] = round(row["new"]["ms_per_iter"] / row["parent"]["ms_per_iter"], 3)
        rows.append(row)
    doc["ntf_mu_iteration_unweighted"] = {
        "what": "compute_ntf(update_rule='mu'), weights=None, whole call over its iterations (tools/time_ntf_mu.py --routes native), "
                "this tree and a built tree of the parent commit alternating in one session", "cases": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in rows:
        print(json.dumps(r))


def main():
    if len(sys.argv) == 6 and sys.argv[1] == "--table":
        return table(*sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[500, 500, 500])
    ap.add_argument("--rank", type=int, default=30)
    ap.add_argument("--betas", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--modes", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("mu_mode_w_probe: needs a GPU (a CPU time says nothing about the device)")
    from nn_fac_amd.engine import get_engine
    from nn_fac_amd._tensor_state import mode_view
    from nn_fac_amd.ntf import _krao_t
    eng = get_engine("cuda:0")
    shape, R = tuple(args.shape), args.rank
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + R)
    gen = [torch.rand(s, R, device="cuda", generator=g) for s in shape]
    T = (torch.einsum("ir,jr,kr->ijk", *gen) + 0.05).contiguous()
    del gen
    Wg = torch.rand(shape, device="cuda", generator=g) * 2
    Wg[torch.rand(shape, device="cuda", generator=g) < 0.1] = 0
    Ft = [torch.rand(R, s, device="cuda", generator=g) + 0.05 for s in shape]
    rows = []
    for mode in args.modes:
        T3, W3, V = mode_view(T, mode), mode_view(Wg, mode), _krao_t(Ft, mode)
        L, I, K = T3.shape
        Xu = torch.movedim(T, mode, -1).reshape(-1, I).contiguous()
        Wu = torch.movedim(Wg, mode, -1).reshape(-1, I).contiguous()
        out, num, den = (torch.empty(R, I, device="cuda") for _ in range(3))
        nrb = math.ceil(I / 64)
        small = 4 * R * I
        need = {"mode_w": 8 * T.numel() + 4 * R * L * K * nrb + 3 * small,
                "mode": 4 * T.numel() + 4 * R * L * K * nrb + 2 * small,
                "unfold_w": 8 * T.numel() + 4 * R * L * K + 3 * small}
        for beta in args.betas:
            entries = {"mode_w": lambda: eng.mu_mode_w(T3, W3, Ft[mode], V, beta, out_num=num, out_den=den),
                       "mode": lambda: eng.mu_mode(T3, Ft[mode], V, beta, out=out),
                       "unfold_w": lambda: eng.mu_right_w(Xu, Wu, V, Ft[mode], beta, out_num=num, out_den=den)}
            times = {k: [] for k in entries}
            for it in range(args.warmup + args.reps):
                for name, call in entries.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.calls):
                        call()
                    b.record()
                    b.synchronize()
                    if it >= args.warmup:
                        times[name].append(a.elapsed_time(b) / args.calls * 1e3)
            row = {"shape": list(shape), "rank": R, "tensor_mode": mode, "beta": beta, "calls": args.calls, "reps": args.reps}
            for name, ts in times.items():
                med = statistics.median(ts)
                row[name] = {"us": round(med, 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1), "bytes": need[name],
                             "TB_per_s": round(need[name] / med / 1e6, 3)}
            row["mode_w_over_mode"] = round(row["mode_w"]["us"] / row["mode"]["us"], 3)
            row["mode_w_over_unfold_w"] = round(row["mode_w"]["us"] / row["unfold_w"]["us"], 3)
            row["spread_unfold"] = round((row["unfold_w"]["max_us"] - row["unfold_w"]["min_us"]) / row["unfold_w"]["us"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
        del Xu, Wu
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": __doc__.split("\n\n")[0], "cases": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

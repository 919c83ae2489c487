#!/usr/bin/env python3
"""Per-iteration time and peak device memory of compute_ntf(update_rule="mu"): the MU factor updates on the tensor's own layout
(nnf_mu_mode_f32, the default up to rank 64) against the route through materialised unfoldings (NNF_MU_UNFOLD=1).

    python tools/time_ntf_mu.py [--shape 500 500 500] [--rank 30] [--betas 1 0.5] [--iters 300] [--reps 7] [--warmup 1]
                                [--routes native unfold] [--root DIR] [--label NAME] [--out FILE]

What is timed: a whole compute_ntf call of `--iters` iterations (tol = 0) on a device tensor with device factors, host clock
around the call between device synchronisations, divided by the iterations -- so the first-use cost of the unfolding route (the
transposed copies of the tensor, made once per run) is spread over the run, as a user pays it.  The routes alternate call by
call in one process; medians over `--reps` calls after `--warmup` calls per route.  Peak memory: the rise of
torch.cuda.max_memory_allocated() over the level before the call (tensor and start factors already on the device), in bytes
and in copies of the tensor.

--root DIR imports nn_fac_amd from another checkout (a built tree of the parent commit: it has no NNF_MU_UNFOLD, every MU run
there takes the unfoldings -- time it with --routes unfold --label parent).

    python tools/time_ntf_mu.py --table OUT.json NEW.jsonl [PARENT.jsonl ...]
        no GPU: merges the lines of the runs (same box, same session) into profiles/r06_ntf_mu_native.json -- medians with min / max,
        peak memory, and the routes' last costs with their relative difference (the routes must compute the same thing).

One JSON line per (beta, route).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(out_path, new_path, *parent_paths):
    load = lambda p: [json.loads(l) for l in open(p) if l.strip()]
    keep = lambda r: {k: r[k] for k in ("ms_per_iter", "min_ms_per_iter", "max_ms_per_iter", "peak_copies", "last_cost")}
    parents = [{r["beta"]: r for r in load(p)} for p in parent_paths]
    rows = []
    for beta in sorted({r["beta"] for r in load(new_path)}):
        new = {r["route"]: r for r in load(new_path) if r["beta"] == beta}
        nat, unf = new["native"], new["unfold"]
        row = {k: nat[k] for k in ("shape", "rank", "beta", "iters", "reps")}
        row.update(native=keep(nat), unfold=keep(unf), parent_unfold=[keep(p[beta]) for p in parents if beta in p],
                   native_over_unfold=round(nat["ms_per_iter"] / unf["ms_per_iter"], 3),
                   # the two routes compute the same iterates: their last costs differ by the rounding of two kernels only
                   last_cost_rel_diff_native_unfold=abs(nat["last_cost"] - unf["last_cost"]) / abs(unf["last_cost"]))
        if row["parent_unfold"]:
            row["native_over_parent"] = round(nat["ms_per_iter"] / row["parent_unfold"][0]["ms_per_iter"], 3)
            row["last_cost_rel_diff_unfold_parent"] = (abs(unf["last_cost"] - row["parent_unfold"][0]["last_cost"])
                                                       / abs(unf["last_cost"]))
        rows.append(row)
    doc = {"what": "compute_ntf(update_rule='mu'), whole call of `iters` iterations on a device tensor (host clock between device "
                   "synchronisations) over the iterations: median, min and max of `reps` calls after a warm-up call, routes "
                   "alternating call by call; native: nnf_mu_mode_f32 on the tensor's own layout; unfold: NNF_MU_UNFOLD=1 in this "
                   "tree; parent_unfold: the parent commit (unfoldings only), one entry per run (before / after this tree's); "
                   "peak_copies: rise of torch.cuda.max_memory_allocated() during the call in copies of the tensor; last_cost: "
                   "the cost after the last iteration, last_cost_rel_diff_*: relative difference between two routes' last costs",
           "command": "python tools/time_ntf_mu.py (this tree), --root <parent tree> --routes unfold --label parent, one box, one session",
           "cases": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in rows:
        print(json.dumps(r))


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--table":
        return table(*sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs="+", default=[500, 500, 500])
    ap.add_argument("--rank", type=int, default=30)
    ap.add_argument("--betas", type=float, nargs="+", default=[1.0, 0.5])
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--routes", nargs="+", choices=["native", "unfold"], default=["native", "unfold"])
    ap.add_argument("--root", default=ROOT, help="checkout to import nn_fac_amd from")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))

    import torch
    if not torch.cuda.is_available():
        sys.exit("time_ntf_mu: needs a GPU (no CPU fallback: a CPU time says nothing about the device)")
    from nn_fac_amd.engine import get_engine
    from nn_fac_amd.ntf import compute_ntf
    get_engine("cuda:0")                                  # the context and its workspace are not part of a run's memory
    shape, R, N = tuple(args.shape), args.rank, len(args.shape)
    g = torch.Generator(device="cuda").manual_seed(sum(shape) + R)
    letters = "ijklmn"[:N]
    gen = [torch.rand(s, R, device="cuda", generator=g) for s in shape]
    T = (torch.einsum(",".join(c + "r" for c in letters) + "->" + letters, *gen) + 0.05).contiguous()
    F0 = [torch.rand(s, R, device="cuda", generator=g) + 0.05 for s in shape]
    del gen
    tensor_bytes = 4 * T.numel()
    lines = []
    for beta in args.betas:
        kw = dict(n_iter_max=args.iters, tol=0, update_rule="mu", beta=beta, return_costs=True, alpha=math.inf,
                  sparsity_coefficients=[None] * N, normalize=[False] * N)
        times, peaks, costs = {r: [] for r in args.routes}, {r: 0 for r in args.routes}, {}
        for it in range(args.warmup + args.reps):
            for route in args.routes:                     # alternating: native, unfold, native, ...
                if route == "unfold":
                    os.environ["NNF_MU_UNFOLD"] = "1"
                else:
                    os.environ.pop("NNF_MU_UNFOLD", None)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                out = compute_ntf(T, R, F0, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                peaks[route] = max(peaks[route], torch.cuda.max_memory_allocated() - before)
                costs[route] = [float(c) for c in out[1]]
                del out
                if it >= args.warmup:
                    times[route].append(dt / args.iters * 1e3)
        os.environ.pop("NNF_MU_UNFOLD", None)
        for route in args.routes:
            rec = {"label": args.label, "shape": list(shape), "rank": R, "beta": beta, "route": route, "iters": args.iters,
                   "reps": args.reps, "ms_per_iter": round(statistics.median(times[route]), 3),
                   "min_ms_per_iter": round(min(times[route]), 3), "max_ms_per_iter": round(max(times[route]), 3),
                   "peak_bytes": int(peaks[route]), "peak_copies": round(peaks[route] / tensor_bytes, 3),
                   "last_cost": costs[route][-1]}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

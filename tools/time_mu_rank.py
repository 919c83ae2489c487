#!/usr/bin/env python3
"""Times one beta-divergence MU update at ranks 65 .. 128: the fused kernels against the composed large-rank route.

    python tools/time_mu_rank.py [--route old|new|both] [--reps 20] [--warmup 3] [--cases all|rank100] [--out FILE]

Routes
  old   Engine._mu_large_rank + Engine.mu_apply: nnf_mu_ratio_f32 writes X .* (UV)^(beta-2) [and (UV)^(beta-1)] as m x n
        operands, plain X H^T / W^T X contractions read them back (the only route for 64 < r <= 128 before the fused
        kernels took these ranks; still the route above 128).  Runs on any checkout that has those two methods.
  new   Engine.mu_left / Engine.mu_right (nnf_mu_left_f32 / nnf_mu_right_f32).
  both  the two interleaved call by call in one process (the same kernel moves by up to 15 % with the state of the chip:
        only interleaved medians compare).

What is timed: the WHOLE update on the stream, HIP events around the call -- every kernel of a route and, for the old one,
the allocation of its m x n operands through the caching allocator (warm after the first call) -- because the old route is
three to five kernels and the library's in-kernel probe brackets one.  For the new route the probe time of the fused kernel
alone (Engine.time_kernel) is reported next to it as `new_kernel_us`.

    python tools/time_mu_rank.py --table PARENT.jsonl NEW.jsonl OUT.json
        no GPU: merges the `--route old` lines of a run on the parent commit with the `--route both` lines of this tree (same
        box, same session) into the table of profiles/r05_mu_rank128.json and says per case whether new <= parent old.

One JSON line per case: medians in microseconds, and the fraction of the fp32 MFMA peak on the 4 r m n algorithmic flops of
an update (P = U V and the contraction with it; bench.py's convention for its MU legs).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32_PEAK_TFLOPS = 157.3     # bench.py: MI355X peak fp32 (matrix)
CASES = [(100000, 2000, 65), (100000, 2000, 100), (100000, 2000, 128), (125000, 4000, 100)]   # last: config E's per-rank block


def table(parent_path, new_path, out_path):
    load = lambda p: [json.loads(l) for l in open(p) if l.strip()]
    rows = []
    for p, n in zip(load(parent_path), load(new_path)):
        key = {k: n[k] for k in ("m", "n", "r", "beta", "side")}
        assert all(p[k] == v for k, v in key.items()), (p, n)
        rows.append(dict(key, parent_old_us=p["old_us"], new_tree_old_us=n["old_us"], new_fused_us=n["new_us"],
                         new_fused_kernel_us=n["new_kernel_us"], parent_old_frac_mfma_peak=p["old_frac_mfma_peak"],
                         new_fused_frac_mfma_peak=n["new_frac_mfma_peak"],
                         parent_old_over_new_fused=round(p["old_us"] / n["new_us"], 3),
                         new_not_slower_than_parent_old=bool(n["new_us"] <= p["old_us"])))
    doc = {"what": "one MU update, whole call on the stream (HIP events), medians of 20 after 3 warm-up calls, microseconds; "
                   "parent_old: Engine._mu_large_rank + mu_apply on the parent commit; new_tree_old: the same route in this "
                   "tree, interleaved call by call with new_fused (Engine.mu_left / mu_right); new_fused_kernel: the fused "
                   "kernel alone (library probe); frac_mfma_peak: 4 r m n flops over the time against %.1f TFLOP/s"
                   % MFMA_F32_PEAK_TFLOPS,
           "command": "python tools/time_mu_rank.py --route old (parent), --route both (this tree), one box, one session",
           "cases": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for r in rows:
        print(r["m"], r["n"], r["r"], r["beta"], r["side"], r["parent_old_us"], r["new_tree_old_us"], r["new_fused_us"],
              r["parent_old_over_new_fused"], "ok" if r["new_not_slower_than_parent_old"] else "SLOWER")


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--table":
        return table(*sys.argv[2:5])
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["old", "new", "both"], default="both")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", choices=["all", "rank100"], default="all")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    import torch
    from nn_fac_amd.engine import get_engine
    eng = get_engine("cuda:0")
    stream = torch.cuda.current_stream()

    def old_call(side, X, Ut, V, beta, out):
        num, den, dvec = eng._mu_large_rank(X, Ut, V, beta, side)
        return eng.mu_apply(Ut if side == "left" else V, num, den, dvec, beta, out=out)

    def new_call(side, X, Ut, V, beta, out):
        return (eng.mu_left if side == "left" else eng.mu_right)(X, Ut, V, beta, out=out)

    routes = {"old": old_call, "new": new_call}
    names = ["old", "new"] if args.route == "both" else [args.route]
    lines = []
    for m, n, r in CASES:
        if args.cases == "rank100" and r != 100:
            continue
        g = torch.Generator(device="cuda").manual_seed(m + n + r)
        Ut = torch.rand(r, m, device="cuda", generator=g) + 0.05
        V = torch.rand(r, n, device="cuda", generator=g) + 0.05
        X = torch.rand(m, n, device="cuda", generator=g) + 0.05
        for beta in (1.0, 0.5):
            for side in ("left", "right"):
                out = torch.empty_like(Ut if side == "left" else V)
                times = {nm: [] for nm in names}
                for it in range(args.warmup + args.reps):
                    for nm in names:                     # interleaved: old, new, old, new, ...
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        routes[nm](side, X, Ut, V, beta, out)
                        b.record(stream)
                        b.synchronize()
                        if it >= args.warmup:
                            times[nm].append(a.elapsed_time(b) * 1e3)
                flops = 4.0 * r * m * n
                rec = {"m": m, "n": n, "r": r, "beta": beta, "side": side, "reps": args.reps, "routes": names}
                for nm in names:
                    med = statistics.median(times[nm])
                    rec[nm + "_us"] = round(med, 1)
                    rec[nm + "_min_us"] = round(min(times[nm]), 1)
                    rec[nm + "_frac_mfma_peak"] = round(flops / (med * 1e-6) / (MFMA_F32_PEAK_TFLOPS * 1e12), 4)
                if "new" in names:
                    kt = eng.time_kernel("mu_left" if side == "left" else "mu_right",
                                         lambda: new_call(side, X, Ut, V, beta, out), reps=args.reps)
                    rec["new_kernel_us"] = round(kt.median * 1e3, 1)
                if len(names) == 2:
                    rec["old_over_new"] = round(rec["old_us"] / rec["new_us"], 3)
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
        del X, Ut, V
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the simplex projection of simplex-constrained KL-NMF next to the MU pass it follows, and the driver next to plain MU.

    python tools/time_simplex.py [--reps 20] [--warmup 3] [--iters 30] [--out FILE]

Per case (100000 x 2000 rank 50: H is 50 x 2000; 200 x 100000 rank 20), on operands of a few iterations into a run:
  accum_us      nnf_mu_right_accum_f32 at beta = 1 (C and D of mu.py:165-166: the pass over X), whole call on the stream
  newton_us     nnf_simplex_proj_kl_f32 (zeroing of the slots + the two launches), whole call on the stream, with the Newton
                iterations the call ran and the lanes per column the plan took (NNF_SIMPLEX_FORCE unset)
  newton_forced_us   the same under each G the rank allows
  simplex_its_per_s / mu_its_per_s   compute_simplex_beta_nmf against compute_nmf(update_rule="mu", beta=1) on the same data
                and starts, `--iters` iterations, tol = 0, device tensors in and out, wall clock around the call
HIP events around the calls, medians of `--reps` after `--warmup`, the two kernels interleaved call by call.  One JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(100000, 2000, 50), (200, 100000, 20)]
GROUPS = (1, 4, 16, 64)


def allowed(r):
    return [G for G in GROUPS if -(-r // G) <= 8 and (G == 1 or r > G // 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from nn_fac_amd import engine
    from nn_fac_amd.nmf import compute_nmf
    from nn_fac_amd.simplex_nmf import compute_simplex_beta_nmf, simplex_right
    dev = torch.device("cuda:0")
    eng = engine.get_engine(dev)
    stream = torch.cuda.current_stream(dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    rows = []
    for m, n, r in CASES:
        g = torch.Generator(device="cpu").manual_seed(m + n + r)
        Ht = torch.rand((r, n), generator=g)
        X = (torch.rand((m, r), generator=g) @ (Ht / Ht.sum(dim=0)) + 0.01 * torch.rand((m, n), generator=g)).to(dev)
        W0, H0 = torch.rand((m, r), generator=g).to(dev), torch.rand((r, n), generator=g).to(dev)
        Ut, V = W0.t().contiguous(), H0
        words = torch.zeros(2, dtype=torch.float64, device=dev)
        for _ in range(5):      # a few iterations in: the operands of a run, not of its random start
            Ut = eng.mu_left(X, Ut, V, 1)
            V = simplex_right(eng, X, Ut, V, 1e-6, words)
        Ut = eng.mu_left(X, Ut, V, 1)
        num, den, dvec = eng.mu_right_accum(X, Ut, V, 1)
        out = torch.empty_like(V)
        os.environ.pop("NNF_SIMPLEX_FORCE", None)
        t_acc, t_new = [], []
        for i in range(args.warmup + args.reps):
            ta = timed(lambda: eng.mu_right_accum(X, Ut, V, 1))
            tn = timed(lambda: eng.simplex_proj(V, num, den, dvec, tol=1e-6, max_iter=100, out=out, status=words))
            if i >= args.warmup:
                t_acc.append(ta)
                t_new.append(tn)
        count, last = words.cpu().tolist()
        forced = {}
        for G in allowed(r):
            os.environ["NNF_SIMPLEX_FORCE"] = str(G)
            ts = [timed(lambda: eng.simplex_proj(V, num, den, dvec, tol=1e-6, max_iter=100, out=out, status=words))
                  for _ in range(args.warmup + args.reps)][args.warmup:]
            forced[str(G)] = round(statistics.median(ts), 1)
        os.environ.pop("NNF_SIMPLEX_FORCE", None)
        its = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for name, run in (("simplex", lambda: compute_simplex_beta_nmf(X, W0, H0, r, 1, n_iter_max=args.iters, tol=0)),
                              ("mu", lambda: compute_nmf(X, r, W0, H0, n_iter_max=args.iters, tol=0, update_rule="mu", beta=1,
                                                         return_costs=True))):
                run()
                torch.cuda.synchronize()
                best = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    res = run()
                    torch.cuda.synchronize()
                    best.append(time.perf_counter() - t0)
                    assert len(res[2]) == args.iters
                its[name] = round(args.iters / statistics.median(best), 1)
        row = dict(m=m, n=n, r=r, accum_us=round(statistics.median(t_acc), 1), newton_us=round(statistics.median(t_new), 1),
                   newton_min_us=round(min(t_new), 1), newton_max_us=round(max(t_new), 1), newton_iterations=int(count),
                   newton_last_step=last, newton_forced_us=forced, simplex_its_per_s=its["simplex"], mu_its_per_s=its["mu"])
        row["newton_over_accum"] = round(row["newton_us"] / row["accum_us"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
    doc = {"what": "simplex projection (Newton solve + update, nnf_simplex_proj_kl_f32) next to nnf_mu_right_accum_f32 at beta = 1 "
                   "on the same operands, whole calls on the stream, HIP events, medians of %d after %d warm-up calls, "
                   "microseconds, interleaved; compute_simplex_beta_nmf against compute_nmf(mu, beta=1), %d iterations, "
                   "iterations per second (median of 3 runs)" % (args.reps, args.warmup, args.iters),
           "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "command": "python tools/time_simplex.py", "cases": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

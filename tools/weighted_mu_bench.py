#!/usr/bin/env python
"""Times of the weighted MU updates next to the unweighted ones and next to the observed-entries (CSR) route (DESIGN.md section 7;
bench.py is the dense flagship and stays as it is).  One JSON line per measurement on stdout and, with --out, appended to a file
(profiles/weighted_mu.jsonl).

    python tools/weighted_mu_bench.py --part A     100000 x 2000 at ranks 50 and 100, beta = 1, 0.5, 2: the weighted left and right
                                                   sums (+ mu_apply) against the unweighted update of the same beta -- at beta = 0.5
                                                   the same arithmetic minus the weight stream, at beta = 1 and 2 what the shortcuts
                                                   (rowsum(V), the Gram form) buy -- and the weighted cost against the unweighted one
    python tools/weighted_mu_bench.py --part B     the same matrix with 50 / 90 / 99 % of its entries observed: one weighted
                                                   iteration (weighted_nmf._one_step_w) against one iteration through
                                                   observed_entries + unstored="missing" (sparse_nmf._one_step_obs), beta = 1

Kernel times are device events around one engine call, the median of `--reps` calls after two warm-up calls; the two versions of
a comparison alternate inside one process.  Bytes: the streams an update has to read once (X, and the weights), 4 m n each.
ms_per_step: `--steps` steps after 2 warm-up steps, a host clock around work that ends in a device synchronise.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nn_fac_amd import engine as _engine, sparse_nmf, weighted_nmf  # noqa: E402
from nn_fac_amd._convert import observed_entries  # noqa: E402

OUT = None


def timed(fn, reps):
    for _ in range(2):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2], ts[0], ts[-1]


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def part_a(eng, m, n, ranks, betas, reps):
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.rand(m, n, device=dev, generator=g) + 0.1
    Wg = torch.rand(m, n, device=dev, generator=g) * 2
    cost = torch.zeros(1, dtype=torch.float64, device=dev)
    for r in ranks:
        Ut, V = torch.rand(r, m, device=dev, generator=g) + 0.05, torch.rand(r, n, device=dev, generator=g) + 0.05
        bufs = {"left": [torch.empty(r, m, device=dev) for _ in range(3)], "right": [torch.empty(r, n, device=dev) for _ in range(3)]}
        for beta in betas:
            for side, F in (("left", Ut), ("right", V)):
                num, den, out = bufs[side]
                plain = (lambda: eng.mu_left(X, Ut, V, beta, out=out)) if side == "left" else (lambda: eng.mu_right(X, Ut, V, beta, out=out))
                sums = (lambda: eng.mu_left_w(X, Wg, Ut, V, beta, out_num=num, out_den=den)) if side == "left" else \
                    (lambda: eng.mu_right_w(X, Wg, Ut, V, beta, out_num=num, out_den=den))

                def weighted():
                    sums()
                    eng.mu_apply(F, num, den, None, beta, out=out)
                res = {}
                for rnd in range(2):      # the two versions alternate
                    for name, fn in (("unweighted", plain), ("weighted", weighted), ("weighted_sums", sums)):
                        res.setdefault(name, []).append(timed(fn, reps))
                best = {k: min(v) for k, v in res.items()}
                emit(kind="update", side=side, m=m, n=n, r=r, beta=beta, reps=reps,
                     unweighted_ms=best["unweighted"][0], weighted_ms=best["weighted"][0], weighted_sums_ms=best["weighted_sums"][0],
                     ratio=best["weighted"][0] / best["unweighted"][0], spread={k: [list(t) for t in v] for k, v in res.items()},
                     weighted_gbytes_per_s=8.0 * m * n / best["weighted_sums"][0] / 1e6)
            a = timed(lambda: eng.betadiv(X, Ut, V, beta, out=cost), reps)
            b = timed(lambda: eng.betadiv_w(X, Wg, Ut, V, beta, out=cost), reps)
            emit(kind="cost", m=m, n=n, r=r, beta=beta, unweighted_ms=a[0], weighted_ms=b[0], ratio=b[0] / a[0],
                 weighted_gbytes_per_s=8.0 * m * n / b[0] / 1e6)


def part_b(eng, m, n, r, beta, fractions, nsteps):
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.rand(m, n, device=dev, generator=g) + 0.1

    def run(step):
        Ut, V = torch.rand(r, m, device=dev) + 0.05, torch.rand(r, n, device=dev) + 0.05
        for _ in range(2):
            Ut, V = step(Ut, V)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(nsteps):
            Ut, V = step(Ut, V)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / nsteps

    for frac in fractions:
        mask = torch.rand(m, n, device=dev, generator=g) < frac
        Wg = mask.to(torch.float32)
        wws = weighted_nmf._Buffers(dev, 0)
        S = sparse_nmf.SparseData(eng, observed_entries(X, mask), dev)
        sws = sparse_nmf._Buffers(r, dev, 0)
        empty = S.empty_slices()
        tw, ts = [], []
        for rnd in range(2):
            tw.append(run(lambda Ut, V: weighted_nmf._one_step_w(eng, X, Wg, wws, Ut, V, beta, [])[:2]))
            ts.append(run(lambda Ut, V: sparse_nmf._one_step_obs(eng, S, sws, Ut, V, beta, [], empty)[:2]))
        emit(kind="step", m=m, n=n, r=r, beta=beta, observed=frac, nnz=S.X.nnz, steps=nsteps, weighted_ms_per_step=min(tw),
             csr_missing_ms_per_step=min(ts), weighted_over_csr=min(tw) / min(ts), spread=dict(weighted=tw, csr=ts))
        del S, mask, Wg
        torch.cuda.empty_cache()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["A", "B"], required=True)
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--ranks", default="50,100")
    ap.add_argument("--betas", default="1,0.5,2")
    ap.add_argument("--fractions", default="0.5,0.9,0.99")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("weighted_mu_bench: no ROCm device (there is nothing to time without one)")
    OUT = a.out
    eng = _engine.get_engine(torch.device("cuda:0"))
    ranks = [int(x) for x in a.ranks.split(",")]
    betas = [float(x) for x in a.betas.split(",")]
    if a.part == "A":
        part_a(eng, a.m, a.n, ranks, betas, a.reps)
    else:
        for r in ranks:
            part_b(eng, a.m, a.n, r, betas[0], [float(x) for x in a.fractions.split(",")], a.steps)


if __name__ == "__main__":
    main()

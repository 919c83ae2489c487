#!/usr/bin/env python
"""Times of the CSR kernels and of one sparse NMF step on generated matrices (bench.py is the dense flagship
and stays as it is).  One JSON line per measurement on stdout.

    python tools/sparse_bench.py --set small            100000 x 2000, rank 50, 0.1 / 1 / 5 % stored, uniform and power-law columns;
                                                        with --dense also the dense driver's step on the densified matrix
    python tools/sparse_bench.py --set large            10^6 x 4000, ranks 50 and 100, 0.1 / 1 / 5 %
    python tools/sparse_bench.py --chunks 128,256,...   the V-side product (rows of X^T: the skewed side) of one case per chunk size
    python tools/sparse_bench.py --set small --observed  the observed-entries leg instead (unstored="missing"): csr_obs (numerator and
                                                        denominator in one pass) at beta = 1, 2 and 0.5 next to csr_xf and csr_kl
                                                        (numerator only) on the same entries, with `fused_over_two_passes` =
                                                        t(csr_obs) / (t(csr_kl) + t(csr_xf)) -- what two separate passes would cost --
                                                        and the ms/step of a missing-entries MU run next to the stored-zero KL step
    python tools/sparse_bench.py --memory               nmf(scipy_csr, 50, ...) for HALS and MU beta = 1 on 10^6 x 4000 at 1 %: the peak of
                                                        torch's allocator against the 16 GB of a dense copy

Kernel times are device events around one engine call (gather kernel + the sum-and-transpose pass), the median of `--reps`
calls after two warm-up calls; bytes are (8 + 4 ldn) per stored entry + the r x nrows output.  ms_per_step: `--steps` steps of
sparse_nmf._one_step_dev after 2 warm-up steps, HALS with bench.py's fixed inner work (10 sweeps, delta = 0).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nn_fac_amd import engine as _engine, nmf as _nmf, sparse_nmf  # noqa: E402


def generate(m, n, density, pattern, seed, dev):
    """Device CSR tensor with about density * m * n stored entries in (0.1, 1.1): uniform positions, or columns drawn from a power
    law (column j with weight (j + 1)^-0.9: the few heaviest columns of 10^6 rows are almost full, the median one holds tens)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    nnz = int(density * m * n)
    rows = torch.randint(0, m, (nnz,), device=dev, generator=g)
    if pattern == "uniform":
        cols = torch.randint(0, n, (nnz,), device=dev, generator=g)
    else:
        cdf = torch.cumsum(torch.arange(1, n + 1, device=dev, dtype=torch.float64) ** -0.9, 0)
        cols = torch.searchsorted(cdf / cdf[-1], torch.rand(nnz, device=dev, dtype=torch.float64, generator=g)).clamp_(max=n - 1)
    keys = torch.unique(rows * n + cols)          # sorted row-major, duplicates dropped
    rows, cols = keys // n, keys % n
    rowptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(rows, minlength=m), 0, out=rowptr[1:])
    vals = torch.rand(keys.numel(), device=dev, generator=g) + 0.1
    return torch.sparse_csr_tensor(rowptr, cols, vals, size=(m, n))


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
    print(json.dumps(kw), flush=True)


def row_stats(A):
    lens = (A.rowptr[1:] - A.rowptr[:-1]).double()
    return dict(max_row=int(lens.max()), median_row=float(lens.median()), nchunks=A.nchunks, ch=A.ch)


def kernels(eng, S, r, reps, case):
    dev = S.X.device
    m, n = S.shape
    Ut, V = torch.rand(r, m, device=dev) + 0.05, torch.rand(r, n, device=dev) + 0.05
    Un, Vn = _engine.node_major(Ut), _engine.node_major(V)
    ldn = Un.stride(0)
    cost = torch.zeros(1, dtype=torch.float64, device=dev)
    for name, A, own, F in (("u_side", S.X, Un, Vn), ("v_side", S.Xt, Vn, Un)):
        nbytes = (8 + 4 * ldn) * A.nnz + 4 * r * A.nrows
        for kern, fn, extra in (("csr_xf", lambda: eng.csr_xf(A, F), 0),
                                ("csr_kl", lambda: eng.csr_kl(A, own, F, cost_out=cost), 4 * ldn * A.nrows)):
            med, lo, hi = timed(fn, reps)
            emit(kind="kernel", kernel=kern, side=name, ms_median=med, ms_min=lo, ms_max=hi, bytes=nbytes + extra,
                 gbytes_per_s=(nbytes + extra) / med / 1e6, **row_stats(A), **case)


def observed(eng, S, r, reps, nsteps, case):
    """The observed-entries leg: csr_obs (sums form) against the two passes it fuses, then the steps."""
    dev = S.X.device
    m, n = S.shape
    Ut, V = torch.rand(r, m, device=dev) + 0.05, torch.rand(r, n, device=dev) + 0.05
    Un, Vn = _engine.node_major(Ut), _engine.node_major(V)
    ldn = Un.stride(0)
    for name, A, own, F in (("u_side", S.X, Un, Vn), ("v_side", S.Xt, Vn, Un)):
        base = {}
        for kern, fn in (("csr_xf", lambda: eng.csr_xf(A, F)), ("csr_kl_num", lambda: eng.csr_kl(A, own, F))):
            base[kern], lo, hi = timed(fn, reps)
            emit(kind="observed", kernel=kern, side=name, ms_median=base[kern], ms_min=lo, ms_max=hi, **row_stats(A), **case)
        nbytes = (8 + 4 * ldn) * A.nnz + (2 * 4 * r + 4 * ldn) * A.nrows
        for beta in (1, 2, 0.5):
            med, lo, hi = timed(lambda: eng.csr_obs(A, own, F, beta), reps)
            emit(kind="observed", kernel="csr_obs", side=name, beta=beta, ms_median=med, ms_min=lo, ms_max=hi, bytes=nbytes,
                 gbytes_per_s=nbytes / med / 1e6, two_passes_ms=base["csr_kl_num"] + base["csr_xf"],
                 fused_over_two_passes=med / (base["csr_kl_num"] + base["csr_xf"]), **row_stats(A), **case)
    ws = sparse_nmf._Buffers(r, dev, 0)
    empty = S.empty_slices()

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
    ms = run(lambda Ut, V: sparse_nmf._one_step_dev(eng, S, ws, Ut, V, "mu", 1, [None, None], [], [False, False], True)[:2])
    emit(kind="step", driver="sparse", unstored="zero", rule="mu", beta=1, ms_per_step=ms, steps=nsteps, **case)
    for beta in (1, 2, 0.5):
        ms = run(lambda Ut, V: sparse_nmf._one_step_obs(eng, S, ws, Ut, V, beta, [], empty)[:2])
        emit(kind="step", driver="sparse", unstored="missing", rule="mu", beta=beta, ms_per_step=ms, steps=nsteps, **case)


def steps(eng, S, r, nsteps, case, dense=None):
    dev = S.X.device
    m, n = S.shape
    inner = dict(_nmf.HALS_INNER)
    _nmf.HALS_INNER.update(maxiter=10, delta=0.0)
    try:
        for rule, beta in (("hals", 2), ("mu", 1)):
            def run(step, k):
                Ut, V = torch.rand(r, m, device=dev) + 0.05, torch.rand(r, n, device=dev) + 0.05
                for _ in range(2):
                    Ut, V = step(Ut, V)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(k):
                    Ut, V = step(Ut, V)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / k
            ws = sparse_nmf._Buffers(r, dev, 0)
            ms = run(lambda Ut, V: sparse_nmf._one_step_dev(eng, S, ws, Ut, V, rule, beta, [None, None], [], [False, False], True)[:2],
                     nsteps)
            emit(kind="step", driver="sparse", rule=rule, beta=beta, ms_per_step=ms, steps=nsteps, **case)
            if dense is not None:
                dws = _nmf._StepBuffers(dense, r)
                ms = run(lambda Ut, V: _nmf._one_nmf_step_dev(eng, dws, dense, r, Ut, V, rule, beta, [None, None], [], [False, False],
                                                              True)[:2], nsteps)
                emit(kind="step", driver="dense", rule=rule, beta=beta, ms_per_step=ms, steps=nsteps, **case)
    finally:
        _nmf.HALS_INNER.update(inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=["small", "large"], default=None)
    ap.add_argument("--densities", default="0.001,0.01,0.05")
    ap.add_argument("--patterns", default="uniform,powerlaw")
    ap.add_argument("--ranks", default=None)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--chunks", default=None)
    ap.add_argument("--memory", action="store_true")
    ap.add_argument("--observed", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sparse_bench: no ROCm device (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    eng = _engine.get_engine(dev)
    dens = [float(x) for x in a.densities.split(",")]
    pats = a.patterns.split(",")

    if a.set:
        m, n = (100000, 2000) if a.set == "small" else (1000000, 4000)
        ranks = [int(x) for x in a.ranks.split(",")] if a.ranks else ([50] if a.set == "small" else [50, 100])
        for d in dens:
            for pat in pats:
                T = generate(m, n, d, pat, 0, dev)
                S = sparse_nmf.SparseData(eng, T, dev)
                dense = T.to_dense() if (a.dense and a.set == "small") else None
                for r in ranks:
                    case = dict(m=m, n=n, r=r, density=d, pattern=pat, nnz=S.X.nnz)
                    if a.observed:
                        observed(eng, S, r, a.reps, a.steps, case)
                        continue
                    kernels(eng, S, r, a.reps, case)
                    steps(eng, S, r, a.steps, case, dense=dense)
                del S, T, dense
                torch.cuda.empty_cache()

    if a.chunks:
        m, n, r, d = 1000000, 4000, 50, 0.01
        for pat in pats:
            T = generate(m, n, d, pat, 0, dev)
            rowptr, colidx, vals, shape = sparse_nmf.to_dev_csr(T, dev, transpose=True)
            Un = _engine.node_major(torch.rand(r, m, device=dev) + 0.05)
            for ch in [int(x) for x in a.chunks.split(",")]:
                A = eng.csr_matrix(rowptr, colidx, vals, shape, ch=ch)
                med, lo, hi = timed(lambda: eng.csr_xf(A, Un), a.reps)
                emit(kind="chunks", kernel="csr_xf", side="v_side", ms_median=med, ms_min=lo, ms_max=hi, m=m, n=n, r=r, density=d,
                     pattern=pat, nnz=A.nnz, library_ch=eng.csr_chunk_entries(A.nnz), **row_stats(A))
            del T, A, rowptr, colidx, vals
            torch.cuda.empty_cache()

    if a.memory:
        import scipy.sparse as sp
        m, n, r, d = 1000000, 4000, 50, 0.01
        T = generate(m, n, d, "uniform", 0, dev)
        X = sp.csr_matrix((T.values().cpu().numpy(), T.col_indices().cpu().numpy().astype(np.int32), T.crow_indices().cpu().numpy()),
                          shape=(m, n))
        del T
        torch.cuda.empty_cache()
        for rule, beta in (("hals", 2), ("mu", 1)):
            torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            U, V, costs, _ = _nmf.nmf(X, r, n_iter_max=3, tol=0, update_rule=rule, beta=beta, return_costs=True, deterministic=True)
            peak = torch.cuda.max_memory_allocated(dev)
            emit(kind="memory", rule=rule, beta=beta, m=m, n=n, r=r, nnz=int(X.nnz), peak_allocated_bytes=peak, dense_copy_bytes=4 * m * n,
                 workspace_bytes=int(eng.lib.nnf_ctx_workspace_bytes(eng.ctx)), seconds=time.perf_counter() - t0, costs=list(costs),
                 finite=bool(np.isfinite(U).all() and np.isfinite(V).all()))
            assert peak < m * n, "something of the size of the dense matrix was allocated"


if __name__ == "__main__":
    main()

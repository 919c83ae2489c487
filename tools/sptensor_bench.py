#!/usr/bin/env python
"""Times of the sparse-tensor kernels on generated tensors, with the CSR product at the same nnz and rank as the yardstick
(bench.py is the dense flagship and stays as it is).  One JSON line per measurement on stdout.

    python tools/sptensor_bench.py                      order 3 (100000 x 20000 x 2000) and order 4 (20000 x 5000 x 2000 x 500),
                                                        ranks 16, 50 and 100, 10^7 stored entries, uniform and power-law indices
    python tools/sptensor_bench.py --nnz 1000000 --orders 3 --ranks 50 --patterns uniform      a smaller run

    python tools/sptensor_bench.py --observed ...       also sptensor_obs (numerator and denominator in one pass, unstored="missing")
                                                        at beta = 1, 2 and 0.5, with `fused_over_two_passes` = its time over
                                                        t(sptensor_kl, numerator only) + t(sptensor_mttkrp) of the same mode

Per tensor and rank: sptensor_mttkrp and sptensor_kl (numerator and cost) of every mode, and csr_xf on the matrix of the first two
extents with the same number of stored entries drawn the same way.  Kernel times are device events around one engine call (gather
kernel + the sum-and-transpose pass), the median of `--reps` calls after two warm-up calls.  Bytes: (4 N + ng 4 ldn) per stored
entry of a tensor of order N (its ng = N - 1 indices and its value, one gathered row per other mode) + the r x extent output, against
csr_xf's (8 + 4 ldn) per entry; `ratio_to_csr_xf` is the measured time over the yardstick's, `byte_ratio` what the bytes alone give.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nn_fac_amd import engine as _engine  # noqa: E402

SHAPES = {3: (100000, 20000, 2000), 4: (20000, 5000, 2000, 500)}


def draw(n, count, pattern, g, dev):
    """`count` indices below n: uniform, or from a power law (index j with weight (j + 1)^-0.9: the few heaviest slices hold a
    large share of the entries, the median one a few)."""
    if pattern == "uniform":
        return torch.randint(0, n, (count,), device=dev, generator=g)
    cdf = torch.cumsum(torch.arange(1, n + 1, device=dev, dtype=torch.float64) ** -0.9, 0)
    return torch.searchsorted(cdf / cdf[-1], torch.rand(count, device=dev, dtype=torch.float64, generator=g)).clamp_(max=n - 1)


def generate(shape, nnz, pattern, seed, dev):
    """Canonical coordinate list (indices int64 [N, <= nnz], values in (0.1, 1.1)): duplicates dropped through a linear key (the
    extents of this tool multiply to less than 2^63)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    key = torch.zeros(nnz, dtype=torch.int64, device=dev)
    for n in shape:
        key = key * n + draw(n, nnz, pattern, g, dev)
    key = torch.unique(key)
    ind = []
    for n in reversed(shape):
        ind.append(key % n)
        key = key // n
    return torch.stack(ind[::-1]).contiguous(), torch.rand(ind[0].numel(), device=dev, generator=g) + 0.1


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


def slice_stats(ptr, nchunks, ch):
    lens = (ptr[1:] - ptr[:-1]).double()
    return dict(max_slice=int(lens.max()), median_slice=float(lens.median()), nchunks=nchunks, ch=ch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nnz", type=int, default=10 ** 7)
    ap.add_argument("--orders", default="3,4")
    ap.add_argument("--ranks", default="16,50,100")
    ap.add_argument("--patterns", default="uniform,powerlaw")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--observed", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sptensor_bench: no ROCm device (there is nothing to time without one)")
    dev = torch.device("cuda:0")
    eng = _engine.get_engine(dev)
    ranks = [int(x) for x in a.ranks.split(",")]
    for order in [int(x) for x in a.orders.split(",")]:
        shape = SHAPES[order]
        for pat in a.patterns.split(","):
            # the yardstick: a CSR matrix of the first two extents, as many entries, drawn the same way
            ind, vals = generate(shape[:2], a.nnz, pat, 1, dev)
            rowptr = torch.zeros(shape[0] + 1, dtype=torch.int64, device=dev)
            torch.cumsum(torch.bincount(ind[0], minlength=shape[0]), 0, out=rowptr[1:])
            A = eng.csr_matrix(rowptr, ind[1].to(torch.int32).contiguous(), vals, shape[:2])
            ind, vals = generate(shape, a.nnz, pat, 0, dev)
            S = eng.sparse_tensor(ind, vals, shape)
            del ind, vals
            cost = torch.zeros(1, dtype=torch.float64, device=dev)
            for r in ranks:
                F = [_engine.node_major(torch.rand(r, n, device=dev) + 0.05) for n in shape]
                ldn = F[0].stride(0)
                case = dict(order=order, shape=list(shape), r=r, ldn=ldn, pattern=pat)
                xf_bytes = (8 + 4 * ldn) * A.nnz + 4 * r * A.nrows
                xf, lo, hi = timed(lambda: eng.csr_xf(A, F[1]), a.reps)
                emit(kind="kernel", kernel="csr_xf", ms_median=xf, ms_min=lo, ms_max=hi, nnz=A.nnz, bytes=xf_bytes,
                     gbytes_per_s=xf_bytes / xf / 1e6, **slice_stats(A.rowptr, A.nchunks, A.ch), **case)
                xf_per_entry = xf / A.nnz
                for mode, M in enumerate(S.modes):
                    others = [f for m, f in enumerate(F) if m != mode]
                    entry = 4 * order + (order - 1) * 4 * ldn
                    if a.observed:
                        mt, _, _ = timed(lambda: eng.sptensor_mttkrp(S, mode, others), a.reps)
                        kl, _, _ = timed(lambda: eng.sptensor_kl(S, mode, F[mode], others), a.reps)
                        emit(kind="observed", kernel="sptensor_mttkrp", mode=mode, ms_median=mt, nnz=M.nnz, **case)
                        emit(kind="observed", kernel="sptensor_kl_num", mode=mode, ms_median=kl, nnz=M.nnz, **case)
                        for beta in (1, 2, 0.5):
                            med, lo, hi = timed(lambda: eng.sptensor_obs(S, mode, F[mode], others, beta), a.reps)
                            emit(kind="observed", kernel="sptensor_obs", mode=mode, beta=beta, ms_median=med, ms_min=lo, ms_max=hi,
                                 nnz=M.nnz, two_passes_ms=kl + mt, fused_over_two_passes=med / (kl + mt),
                                 **slice_stats(M.ptr, M.nchunks, M.ch), **case)
                        continue
                    for kern, fn, extra in (("sptensor_mttkrp", lambda: eng.sptensor_mttkrp(S, mode, others), 0),
                                            ("sptensor_kl", lambda: eng.sptensor_kl(S, mode, F[mode], others, cost_out=cost),
                                             4 * ldn * M.extent)):
                        nbytes = entry * M.nnz + 4 * r * M.extent + extra
                        med, lo, hi = timed(fn, a.reps)
                        emit(kind="kernel", kernel=kern, mode=mode, ms_median=med, ms_min=lo, ms_max=hi, nnz=M.nnz, bytes=nbytes,
                             gbytes_per_s=nbytes / med / 1e6, ratio_to_csr_xf=(med / M.nnz) / xf_per_entry,
                             byte_ratio=entry / (8 + 4 * ldn), **slice_stats(M.ptr, M.nchunks, M.ch), **case)
            del S, A
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

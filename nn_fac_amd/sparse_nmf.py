"""NMF of SPARSE data on the MI355X engine: the steps of nmf.py over the stored entries of a CSR matrix only.

`nmf`, `compute_nmf` and `one_nmf_step` of nn_fac_amd.nmf come here when `data` is a scipy.sparse matrix (any format) or a torch
sparse-CSR tensor (host or device).  There is no dense copy: neither the data nor anything else of size m x n is ever formed, on
the host or on the device.  What an iteration needs from X are the two cross products, and they are sums over stored entries:

    V X^T  (r x m)   nnf_csr_xf_f32 on the CSR of X   with V^T (n x r, node-major) gathered by column index
    U^T X  (r x n)   nnf_csr_xf_f32 on the CSR of X^T with U   (m x r, node-major) gathered by row index

    update_rule="hals" (beta = 2)   node-major copy of the fixed factor -> csr_xf -> gram -> nmf._hals_call (the dense driver's
                                    solve: sparsity_coefficients, normalize, fixed_modes and deterministic / the timed sweep budget
                                    behave as there)
    update_rule="mu", beta = 2      numerator csr_xf, denominator (V V^T) U^T / (U^T U) V through gram + small_gemm, mu_apply
    update_rule="mu", beta = 1      nnf_csr_kl_f32: with P = U V only at the stored entries, the numerator sum_j (x_ij / p_ij) V[k,j]
                                    vanishes wherever x_ij = 0; the denominator is rowsum(V) / colsum(U) (fp64); mu_apply

Cost.  beta = 2: ||X||^2 - 2 <U^T X, V> + <U^T U, V V^T> (HALS: + the sparsity terms of nmf.py:452; MU: halved, as
beta_divergence(., ., 2) of nmf.py:455 is), with ||X||^2 = sum vals^2 in
fp64 once per run, the inner product in fp64 (Engine.dot) and both Grams before their rounding to fp32 (gram(..., out64=)).
There is no pass over the data to fall back to, unlike the dense driver's switch between the identity and the streaming
kernel: that switch exists for fits whose residual is 1e-6 of ||X||^2, and a low-rank fit of a sparse matrix sits far from that
regime (its zeros alone keep the residual at the scale of ||X||^2); a caller with an exactly low-rank sparse matrix should
expect the cost to bottom out near 1e-7 ||X||^2.  beta = 1: sum_stored (x log(x / p) - x) from nnf_csr_kl_f32 (cost only)
after both updates, plus sum(P) = colsum(U) . rowsum(V); a stored zero adds nothing (0 log 0 := 0).

Any other beta raises NotImplementedError before the device is touched: the MU denominator then needs P^(beta - 1) at every
entry, stored or not.  Also refused, before anything is launched: `group=` (sharded runs), init="nndsvd" (it needs an SVD of the
data) and ranks above 128.

All of the above reads an unstored entry as a ZERO (`unstored="zero"`, the default).  `unstored="missing"` reads it as UNKNOWN:
the factorization fits the stored entries only (a stored 0 is an observed zero) and predicts the rest.  Then numerator,
denominator and cost of mu_betadivmin (mu.py:82-97) are all sums over stored entries, for every beta >= 0:

    update_rule="mu", any beta >= 0   per factor: node-major copies -> nnf_csr_obs_f32 (num = sum x p^(beta-2) h, den = sum
                                      p^(beta-1) h from one p per entry) -> mu_apply(F, num, den, None, beta); a row or column
                                      without a stored entry keeps its start value through the run (nothing is known about it;
                                      num / den = 0 / 0 there): the list of those is taken once per run from the row pointers.
                                      Cost: sum_stored d_beta(x | p) from nnf_csr_obs_f32 (cost only) after both updates.

No Grams, no small_gemm, nothing of the data's dense size.  update_rule="hals" with missing entries needs one Gram per row -- a
different algorithm -- and raises NotImplementedError.  `observed_entries(array, mask)` builds the sparse input from a dense
array and a boolean mask, zeros included (scipy.sparse.csr_matrix(dense) would drop them, turning observed zeros into missing
ones).

Setup, once per run (SparseData): the CSR of X and of X^T (host-side `X.T.tocsr()` for SciPy input, a stable sort by column on
the device for a torch tensor), the chunk tables of both (Engine.csr_matrix) and ||X||^2.  The outer loop, its stopping test,
`return_costs`, `toc` and `sweep_log` are those of compute_nmf, on `_outer_loop.Pipeline`.
"""
import math
import numbers

import numpy as np
import torch

from . import _outer_loop as _loop
from . import dist as _dist
from . import engine as _engine
from ._convert import device_of, to_dev, to_dev_t, to_dev_csr, like_input, observed_entries      # noqa: F401 (observed_entries: public here)
from ._status import NMF_COST, NMF_WORDS
from .update_rules.nnls import tic, toc
from .utils import errors as err

PIPELINE_DEPTH = 1   # outer iterations enqueued ahead of the one whose cost the host is looking at


UNSTORED = ("zero", "missing")


def check_unstored(unstored, sparse, what="NMF"):
    """The `unstored` keyword of the drivers: "zero" or "missing", the latter with sparse data only."""
    if unstored not in UNSTORED:
        raise err.InvalidArgumentValue(f'Invalid value for unstored: {unstored!r} (it is "zero" or "missing")')
    if unstored == "missing" and not sparse:
        raise err.InvalidArgumentValue(f'unstored="missing" needs sparse data: a dense array has no unstored entries ({what}; '
                                       f'observed_entries(array, mask) makes the sparse input of a dense array and a mask)')


def check_request(rank, update_rule, beta, group=None, init=None, unstored="zero"):
    """Everything the sparse path refuses, said before anything is uploaded or launched."""
    check_unstored(unstored, True)
    if update_rule not in ["hals", "mu"]:
        raise err.InvalidArgumentValue(f"Invalid update rule: {update_rule}")
    if unstored == "missing":
        if update_rule == "hals":
            raise NotImplementedError('NMF with missing entries (unstored="missing") is built for the multiplicative update: hals '
                                      'then needs one Gram matrix per row, a different algorithm; use update_rule="mu"')
        if not (isinstance(beta, numbers.Real) and 0 <= beta < math.inf):
            raise err.InvalidArgumentValue(f"Invalid value for beta: {beta!r} (a finite beta >= 0 is needed).")
    elif update_rule == "hals" and beta != 2:
        raise err.InvalidArgumentValue(f"The hals is only valid for the frobenius norm, corresponding to the beta divergence with "
                                       f"beta = 2. Here, beta was set to {beta}.")
    elif update_rule == "mu" and beta not in (1, 2):
        raise NotImplementedError(
            f"NMF of sparse data is built for beta = 1 and beta = 2: for any other beta the multiplicative update's denominator "
            f"needs (U V)^(beta - 1) at every entry, stored or not (got beta = {beta!r}); densify the data to use it, or fit the "
            f'stored entries only with unstored="missing"')
    if group is not None:
        raise NotImplementedError("NMF of sparse data does not run row-sharded: group= is refused")
    if init is not None and init.lower() == "nndsvd":
        raise NotImplementedError('init="nndsvd" needs a singular value decomposition of the data and is refused for sparse data: '
                                  'use init="random" or init="custom"')
    if int(rank) > _engine.MAX_RANK:
        raise err.EngineError(f"NMF of sparse data: rank {int(rank)} is above the {_engine.MAX_RANK} the CSR kernels are built for")


class SparseData:
    """The once-per-run setup: CSR of X and of X^T on the device with their chunk tables, ||X||^2 in fp64."""

    def __init__(self, eng, data, dev):
        self.X = eng.csr_matrix(*to_dev_csr(data, dev))
        self.Xt = eng.csr_matrix(*to_dev_csr(data, dev, transpose=True))
        self.shape = self.X.shape
        self.normx2 = self.X.vals.double().pow(2).sum().reshape(1)

    def empty_slices(self):
        """(rows, columns) without a stored entry as boolean masks [1, m] and [1, n], None where there is none: from the row
        pointers, once per run (unstored="missing": such a slice keeps its start value)."""
        out = []
        for A in (self.X, self.Xt):
            empty = A.rowptr[1:] == A.rowptr[:-1]
            out.append(empty[None, :] if bool(empty.any()) else None)
        return out


class _Buffers(_loop.StatusRing):
    """Device scratch reused across iterations: the two fp64 Grams of the cost, the ring of status blocks."""

    def __init__(self, r, dev, depth):
        self.G64u = torch.empty((r, r), dtype=torch.float64, device=dev)
        self.G64v = torch.empty((r, r), dtype=torch.float64, device=dev)
        self.init_ring(depth + 2, NMF_WORDS, dev)
        # (a factor with more columns than the resident sweep kernel holds is solved in blind chunks: nmf._hals_call)
        self.guess_u, self.guess_v = _dist.SweepGuess(), _dist.SweepGuess()


def _frob_cost(eng, S, ws, Ut, V, UtM, have_g64u, sparsity_coefficients, out):
    """out[0] = ||X||^2 - 2 <U^T X, V> + <U^T U, V V^T> + the sparsity terms.  `UtM`: U^T X of THIS Ut, or None (it is formed);
    `have_g64u`: ws.G64u already holds the fp64 Gram of this Ut."""
    from .nmf import _add_sparsity_terms
    if UtM is None:
        UtM = eng.csr_xf(S.Xt, _engine.node_major(Ut))
    if not have_g64u:
        eng.gram(Ut, out64=ws.G64u)
    eng.gram(V, out64=ws.G64v)
    out.copy_(S.normx2 - 2.0 * eng.dot(UtM, V) + (ws.G64u * ws.G64v).sum())
    _add_sparsity_terms(Ut, V, sparsity_coefficients, out)


def _kl_cost(eng, S, Ut, V, out):
    """out[0] = sum_stored (x log(x / p) - x) + colsum(U) . rowsum(V)."""
    eng.csr_kl(S.X, _engine.node_major(Ut), _engine.node_major(V), num=False, cost_out=out)
    out.add_((Ut.sum(dim=1, dtype=torch.float64) * V.sum(dim=1, dtype=torch.float64)).sum())


def _one_step_dev(eng, S, ws, Ut_in, V_in, update_rule, beta, sparsity_coefficients, fixed_modes, normalize, deterministic):
    """One pass of updates on U then V, then the cost, on the device (Ut: r x m, V: r x n; the inputs are not modified).
    Returns (Ut, V, number of HALS solves); the cost and the solves' status words are left in ws.block."""
    from .nmf import _hals_call
    Ut, V = Ut_in, V_in
    nstat = 0
    alpha = math.inf if deterministic else 0.5
    dev = Ut.device
    hals, kl = update_rule == "hals", float(beta) == 1.0
    UtM, have_g64u = None, False

    if 0 not in fixed_modes:
        Vn = _engine.node_major(V)
        if hals:
            t0 = tic(dev, alpha)
            VMt = eng.csr_xf(S.X, Vn)                                   # V X^T (nmf.py:408)
            G = eng.gram(V)                                             # V V^T (nmf.py:407)
            timer = toc(dev, t0)
            Ut = _hals_call(eng, VMt, G, Ut_in, sparsity_coefficients[0], normalize[0], deterministic, timer,
                            ws.solve_words(nstat), guess=ws.guess_u)
            nstat += 1
        elif kl:
            num = eng.csr_kl(S.X, _engine.node_major(Ut_in), Vn)
            Ut = eng.mu_apply(Ut_in, num, None, V.sum(dim=1, dtype=torch.float64), 1)      # mu.py:86-87: the row sums of V
        else:
            num = eng.csr_xf(S.X, Vn)
            Ut = eng.mu_apply(Ut_in, num, eng.small_gemm(eng.gram(V), Ut_in), None, 2)     # (U V) V^T = ((V V^T) U^T)^T

    if 1 not in fixed_modes:
        Un = _engine.node_major(Ut)
        if hals:
            t0 = tic(dev, alpha)
            UtM = eng.csr_xf(S.Xt, Un)                                  # U^T X (nmf.py:433)
            G2 = eng.gram(Ut, out64=ws.G64u)                            # U^T U (nmf.py:432), and its sums before rounding
            have_g64u = True
            timer = toc(dev, t0)
            V = _hals_call(eng, UtM, G2, V_in, sparsity_coefficients[1], normalize[1], deterministic, timer,
                           ws.solve_words(nstat), guess=ws.guess_v)
            nstat += 1
        elif kl:
            num = eng.csr_kl(S.Xt, _engine.node_major(V_in), Un)
            V = eng.mu_apply(V_in, num, None, Ut.sum(dim=1, dtype=torch.float64), 1)
        else:
            UtM = eng.csr_xf(S.Xt, Un)
            G2 = eng.gram(Ut, out64=ws.G64u)
            have_g64u = True
            V = eng.mu_apply(V_in, UtM, eng.small_gemm(G2, V_in), None, 2)

    cost = ws.block[NMF_COST:NMF_COST + 1]
    if hals:
        _frob_cost(eng, S, ws, Ut, V, UtM, have_g64u, sparsity_coefficients, cost)      # nmf.py:452
    elif kl:
        _kl_cost(eng, S, Ut, V, cost)                                                   # nmf.py:455
    else:
        _frob_cost(eng, S, ws, Ut, V, UtM, have_g64u, [None, None], cost)
        cost.mul_(0.5)                                # beta_divergence(., ., 2) = ||.||^2 / 2 (nmf.py:455)
    return Ut, V, nstat


def _one_step_obs(eng, S, ws, Ut_in, V_in, beta, fixed_modes, empty):
    """One pass of MU updates on U then V over the stored entries only (unstored="missing"), then the cost, on the device.
    `empty`: S.empty_slices().  Returns (Ut, V, 0); the cost is left in ws.block."""
    Ut, V = Ut_in, V_in
    if 0 not in fixed_modes:
        num, den = eng.csr_obs(S.X, _engine.node_major(Ut_in), _engine.node_major(V), beta)
        Ut = eng.mu_apply(Ut_in, num, den, None, beta)
        if empty[0] is not None:
            Ut = torch.where(empty[0], Ut_in, Ut)
    if 1 not in fixed_modes:
        num, den = eng.csr_obs(S.Xt, _engine.node_major(V_in), _engine.node_major(Ut), beta)
        V = eng.mu_apply(V_in, num, den, None, beta)
        if empty[1] is not None:
            V = torch.where(empty[1], V_in, V)
    eng.csr_obs(S.X, _engine.node_major(Ut), _engine.node_major(V), beta, sums=False, cost_out=ws.block[NMF_COST:NMF_COST + 1])
    return Ut, V, 0


def _lists(sparsity_coefficients, fixed_modes, normalize):
    if sparsity_coefficients is None:
        sparsity_coefficients = [None, None]
    if fixed_modes is None:
        fixed_modes = []
    if normalize is None or normalize is False:
        normalize = [False, False]
    if len(sparsity_coefficients) != 2:
        raise ValueError("NMF needs 2 sparsity coefficients to be performed")
    return sparsity_coefficients, fixed_modes, normalize


def compute_sparse_nmf(data, rank, U_in, V_in, n_iter_max=100, tol=1e-8, update_rule="hals", beta=2,
                       sparsity_coefficients=[None, None], fixed_modes=[], normalize=[False, False], verbose=False,
                       return_costs=False, deterministic=False, sweep_log=None, group=None, unstored="zero"):
    """compute_nmf (nmf.py:284-329) for sparse `data`.  Factors come back in the kind of U_in / V_in."""
    check_request(np.shape(U_in)[1], update_rule, beta, group=group, unstored=unstored)
    missing = unstored == "missing"
    sparsity_coefficients, fixed_modes, normalize = _lists(sparsity_coefficients, fixed_modes, normalize)
    dev = device_of(data, U_in, V_in)
    eng = _engine.get_engine(dev)
    S = SparseData(eng, data, dev)
    Ut = to_dev_t(U_in, dev).clone()
    V = to_dev(V_in, dev).clone()
    ws = _Buffers(Ut.shape[0], dev, PIPELINE_DEPTH)
    retired = _loop.Retired(tol, verbose=verbose, sweep_log=sweep_log)
    main = torch.cuda.current_stream(dev)
    empty = S.empty_slices() if missing else None

    def enqueue(iteration, factors):
        ws.select(iteration % ws.blocks.shape[0])
        if missing:
            Ut, V, nstat = _one_step_obs(eng, S, ws, factors[0], factors[1], beta, fixed_modes, empty)
        else:
            Ut, V, nstat = _one_step_dev(eng, S, ws, factors[0], factors[1], update_rule, beta, sparsity_coefficients, fixed_modes,
                                         normalize, deterministic)
        step = _loop.Step(iteration, ws.slot, (Ut, V), nstat)
        ws.host[ws.slot].copy_(ws.block, non_blocking=True)
        step.event = main.record_event()
        return step

    def settle(step):
        host = ws.host[step.slot]
        _loop.check_status(host, step.nstat)
        return float(host[NMF_COST]), _loop.sweep_counts(host, step.nstat)

    # (the wall-clock sweep budget synchronises inside a step: nothing is gained by running ahead then)
    loop = _loop.Pipeline(enqueue, settle, retired, [main], depth=PIPELINE_DEPTH if deterministic or missing else 0)
    Ut, V = loop.run(n_iter_max, (Ut, V))
    U_out, V_out = like_input(Ut.t(), U_in), like_input(V, V_in)
    if return_costs:
        return U_out, V_out, retired.cost_fct_vals, retired.toc
    return U_out, V_out


def one_sparse_nmf_step(data, rank, U_in, V_in, norm_data, update_rule, beta, sparsity_coefficients, fixed_modes, normalize,
                        deterministic, unstored="zero"):
    """one_nmf_step (nmf.py:387-458) for sparse `data`.  Returns (U, V, cost).  The setup (transpose, chunk tables) is redone at
    every call: a loop belongs in compute_nmf."""
    check_request(np.shape(U_in)[1], update_rule, beta, unstored=unstored)
    sparsity_coefficients, fixed_modes, normalize = _lists(sparsity_coefficients, fixed_modes, normalize)
    dev = device_of(data, U_in, V_in)
    eng = _engine.get_engine(dev)
    S = SparseData(eng, data, dev)
    Ut, V = to_dev_t(U_in, dev), to_dev(V_in, dev)
    ws = _Buffers(Ut.shape[0], dev, 0)
    if unstored == "missing":
        Ut2, V2, nstat = _one_step_obs(eng, S, ws, Ut, V, beta, fixed_modes, S.empty_slices())
    else:
        Ut2, V2, nstat = _one_step_dev(eng, S, ws, Ut, V, update_rule, beta, sparsity_coefficients, fixed_modes, normalize,
                                       deterministic)
    host = ws.block.cpu()
    _loop.check_status(host, nstat)
    return like_input(Ut2.t(), U_in), like_input(V2, V_in), float(host[NMF_COST])

"""NTF (nonnegative CP) of SPARSE tensors on the MI355X engine: the steps of ntf.py over the stored entries of a coordinate list.

`ntf`, `compute_ntf` and `one_ntf_step` of nn_fac_amd.ntf come here when the tensor is a torch sparse-COO tensor (host or device,
coalesced or not) or a `SparseCOO(indices, values, shape)` (N x nnz integer indices, nnz float values; unsorted entries and
duplicates are allowed and summed), of order 3, 4 or 5; `one_ntf_step` takes the sparse object where the reference takes the list
of unfoldings.  There is no dense copy: neither the tensor, an unfolding nor a Khatri-Rao product is ever formed, on the host or
on the device.  What an iteration needs from the tensor are sums over its stored entries:

    the MTTKRP of mode n   rhs[k, i] = sum_{p in slice i} x_p prod_{m != n} F_m[i_m(p), k]      nnf_sptensor_mttkrp_f32 on the copy
                           of the list sorted by mode n (Engine.sparse_tensor keeps one per mode), the other factors gathered
                           node-major

    update_rule="hals" (beta = 2)   rhs, the other factors' Grams (once per value of a factor) -> alpha = inf: hals_solve_cross
                                    (the Hadamard product of the Grams is formed by the solve); alpha finite: hadamard, the
                                    tic / toc bracket and timed_budget, hals_solve -- the unsharded lines of ntf._one_ntf_step_dev;
                                    sparsity_coefficients, normalize and fixed_modes behave as there
    update_rule="mu", beta = 2      numerator rhs, denominator (Hadamard of the other Grams) F_n through small_gemm, mu_apply
    update_rule="mu", beta = 1      nnf_sptensor_kl_f32: with the model p only at the stored entries, the numerator
                                    sum (x / p) prod_{m != n} F_m[i_m, :] vanishes wherever x = 0; the denominator is the Hadamard
                                    product of the other factors' column sums (a vector of length r, fp64); mu_apply

Cost, divided by ||T||^2 = sum vals^2 (fp64, once per run) as ntf.py:475 does.  beta = 2: the reference's own line (ntf.py:470)
on the last updated mode n, ||T||^2 - 2 <F_n, rhs> + <F_n^T F_n, Hadamard of the other Grams>, with the inner product in fp64
(Engine.dot) and every Gram before its rounding to fp32 (gram(..., out64=)); HALS adds the sparsity terms of ntf.py:463-466, MU
halves the value (beta_divergence(., ., 2) = ||.||^2 / 2).  There is no pass over the data to fall back to, unlike the dense
driver's switch between the identity and the pass over T: that switch exists for fits whose residual is 1e-6 of ||T||^2, and a
low-rank fit of a sparse tensor sits far from that regime (its zeros alone keep the residual at the scale of ||T||^2: 0.9 ||T||^2
on the tensors of the tests); a caller with an exactly low-rank sparse tensor should expect the cost to bottom out near
1e-7 ||T||^2.  beta = 1: sum_stored (x log(x / p) - x) from nnf_sptensor_kl_f32 (cost only) after the updates, plus
sum(P) = sum_k prod_m colsum(F_m)[k]; a stored zero adds nothing (0 log 0 := 0).

Refused with a clear error before anything is uploaded or launched: MU with any other beta (NotImplementedError: the denominator
then needs P^(beta - 1) at every entry, stored or not), orders above 5 (NotImplementedError) and order 2 (a matrix is nmf's
business: it takes scipy.sparse and torch sparse-CSR data), init="nndsvd" (an SVD of every unfolding), `group=` (sharded runs)
and ranks above 128 (EngineError).

All of the above reads an unstored entry as a ZERO (`unstored="zero"`, the default).  `unstored="missing"` reads it as UNKNOWN:
the factorization fits the stored entries only (a stored 0 is an observed zero) and predicts the rest; numerator, denominator
and cost of mu_betadivmin are then all sums over stored entries, for every beta >= 0:

    update_rule="mu", any beta >= 0   per mode: node-major copies -> nnf_sptensor_obs_f32 (num = sum x p^(beta-2) h, den = sum
                                      p^(beta-1) h from one p per entry) -> mu_apply(F, num, den, None, beta); a slice without
                                      a stored entry keeps its start value through the run (num / den = 0 / 0 there): the list
                                      of those is taken once per run from the modes' pointers.  Cost: sum_stored d_beta(x | p)
                                      from nnf_sptensor_obs_f32 (cost only) after the last mode, divided by ||T||^2 as above.

No Grams, no small_gemm, nothing of the tensor's dense size.  update_rule="hals" with missing entries needs one Gram per slice
-- a different algorithm -- and raises NotImplementedError.  `observed_entries(array, mask)` builds the SparseCOO of a dense
array and a boolean mask, zeros included.

Setup, once per run (SparseTensorData): the canonical coordinate list (_convert.to_dev_coo), its N sorted copies with their chunk
tables (Engine.sparse_tensor) and ||T||^2.  The outer loop, its stopping test, `return_costs`, `verbose` and `sweep_log` are those
of compute_ntf, on `_outer_loop.Pipeline`.
"""
import math
import numbers

import numpy as np
import torch

from . import _outer_loop as _loop
from . import engine as _engine
from ._convert import SparseCOO, device_of, is_sparse_tensor, observed_entries, to_dev_coo, to_dev_t, like_input      # noqa: F401 (SparseCOO, observed_entries: public here)
from .update_rules.nnls import tic, toc, timed_budget
from .utils import errors as err

PIPELINE_DEPTH = 1   # outer iterations enqueued ahead of the one whose cost the host is looking at
MIN_ORDER, MAX_ORDER = _engine.SparseTensor.MIN_ORDER, _engine.SparseTensor.MAX_ORDER


def check_request(rank, update_rule, beta, order, group=None, init=None, unstored="zero"):
    """Everything the sparse path refuses, said before anything is uploaded or launched."""
    from .sparse_nmf import check_unstored
    check_unstored(unstored, True, "NTF")
    if update_rule not in ["hals", "mu"]:
        raise err.InvalidArgumentValue(f"Invalid update rule: {update_rule}")
    if unstored == "missing":
        if update_rule == "hals":
            raise NotImplementedError('NTF with missing entries (unstored="missing") is built for the multiplicative update: hals '
                                      'then needs one Gram matrix per slice, a different algorithm; use update_rule="mu"')
        if not (isinstance(beta, numbers.Real) and 0 <= beta < math.inf):
            raise err.InvalidArgumentValue(f"Invalid value for beta: {beta!r} (a finite beta >= 0 is needed).")
    elif update_rule == "hals" and beta != 2:
        raise err.InvalidArgumentValue(f"The hals is only valid for the frobenius norm, corresponding to the beta divergence with "
                                       f"beta = 2. Here, beta was set to {beta}.")
    elif update_rule == "mu" and beta not in (1, 2):
        raise NotImplementedError(
            f"NTF of sparse data is built for beta = 1 and beta = 2: for any other beta the multiplicative update's denominator "
            f"needs the model to the power beta - 1 at every entry, stored or not (got beta = {beta!r}); densify the data to use it, "
            f'or fit the stored entries only with unstored="missing"')
    if order < MIN_ORDER:
        raise NotImplementedError(f"NTF needs a tensor of order >= 3, got order {order}: a sparse matrix is nmf's business (it takes "
                                  f"scipy.sparse matrices and torch sparse-CSR tensors)")
    if order > MAX_ORDER:
        raise NotImplementedError(f"NTF of sparse data is built for tensors of order 3 to {MAX_ORDER}, got order {order}")
    if group is not None:
        raise NotImplementedError("NTF of sparse data does not run sharded: group= is refused")
    if init is not None and init.lower() == "nndsvd":
        raise NotImplementedError('init="nndsvd" needs a singular value decomposition of every unfolding and is refused for sparse '
                                  'data: use init="random" or init="custom"')
    if int(rank) > _engine.MAX_RANK:
        raise err.EngineError(f"NTF of sparse data: rank {int(rank)} is above the {_engine.MAX_RANK} the sparse-tensor kernels are "
                              f"built for")


def _device_of(tensor, factors):
    parts = (tensor.indices, tensor.values) if isinstance(tensor, SparseCOO) else (tensor,)
    return device_of(*parts, *factors)


class SparseTensorData:
    """The once-per-run setup: the N sorted copies of the tensor on the device with their chunk tables, ||T||^2 in fp64."""

    def __init__(self, eng, tensor, dev):
        indices, values, shape = to_dev_coo(tensor, dev)
        self.S = eng.sparse_tensor(indices, values, shape)
        self.shape, self.nway = self.S.shape, self.S.order
        self.normx2 = values.double().pow(2).sum().reshape(1)

    def empty_slices(self):
        """Per mode, the slices without a stored entry as a boolean mask [1, extent], None where there is none: from the modes'
        pointers, once per run (unstored="missing": such a slice keeps its start value)."""
        out = []
        for M in self.S.modes:
            empty = M.ptr[1:] == M.ptr[:-1]
            out.append(empty[None, :] if bool(empty.any()) else None)
        return out


class _Buffers(_loop.StatusRing):
    """Device state reused across iterations: the Grams of the factors (fp32 and before rounding, once per value of a factor) and
    the ring of status blocks -- one HALS status block per mode, then the cost at [8 N]."""

    def __init__(self, eng, nway, dev, depth):
        self.eng = eng
        self.cost_at = _engine.ST_WORDS * nway
        self.init_ring(depth + 2, self.cost_at + 8, dev)
        self._grams = {}

    def gram_of(self, i, F):
        """(F F^T in fp32, the same sums in fp64) of factor i, computed once per value of the factor (_NtfState.gram_of)."""
        hit = self._grams.get(i)
        if hit is not None and hit[0] is F:
            return hit[1], hit[2]
        G64 = torch.empty((F.shape[0], F.shape[0]), dtype=torch.float64, device=F.device)
        G = self.eng.gram(F, out64=G64)
        self._grams[i] = (F, G, G64)
        return G, G64


def _others(Ft, mode):
    return [f for i, f in enumerate(Ft) if i != mode]


def _colsum_product(Ft, skip=None):
    """The Hadamard product of the factors' column sums (the row sums of the transposed factors) in fp64, all but `skip`."""
    out = None
    for i, f in enumerate(Ft):
        if i != skip:
            s = f.sum(dim=1, dtype=torch.float64)
            out = s if out is None else out * s
    return out


def _one_step_dev(eng, D, ws, Ft_in, update_rule, beta, sparsity_coefficients, fixed_modes, normalize, alpha, delta):
    """One pass over the modes, then the cost, on the device (factors transposed, r x dim; the inputs are not modified).
    Returns (factors, number of HALS solves); the cost and the solves' status words are left in ws.block."""
    for fixed_value in fixed_modes:
        sparsity_coefficients[fixed_value] = None
    Ft = list(Ft_in)
    S, N = D.S, D.nway
    dev = Ft[0].device
    hals, kl = update_rule == "hals", float(beta) == 1.0
    deterministic = math.isinf(alpha)
    nstat = 0
    last = None            # (mode, rhs) of the last updated mode: what the reference's cost line is made of (ntf.py:462-470)

    for mode in [m for m in range(N) if m not in fixed_modes]:
        gathered = [_engine.node_major(f) for f in _others(Ft, mode)]
        if hals:
            t0 = tic(dev, alpha)
            grams = [ws.gram_of(i, f)[0] for i, f in enumerate(Ft) if i != mode]      # (ntf.py:442-445)
            Ga = grams[0]
            for g in grams[1:-1]:                   # order > 3: all but the last factor of the product folded here
                Ga = eng.hadamard(Ga, g)
            Gb = grams[-1]
            rhs = eng.sptensor_mttkrp(S, mode, gathered)                              # (ntf.py:448-449)
            new = torch.empty_like(Ft[mode])
            if deterministic:
                eng.hals_solve_cross(rhs, Ga, Gb, Ft[mode], new, 100, delta=delta, sparsity=sparsity_coefficients[mode],
                                     normalize=normalize[mode], status=ws.solve_words(nstat))
            else:
                cross = eng.hadamard(Ga, Gb)
                timer = toc(dev, t0)
                new.copy_(Ft[mode])
                probe = new.clone()
                budget, _ = timed_budget(100, alpha, timer, lambda: eng.hals_sweeps(
                    rhs, cross, probe, 1, sparsity=sparsity_coefficients[mode], normalize=normalize[mode]), dev)
                eng.hals_solve(rhs, cross, new, budget, delta=delta, sparsity=sparsity_coefficients[mode],
                               normalize=normalize[mode], status=ws.solve_words(nstat))
            nstat += 1
            Ft[mode] = new
            last = (mode, rhs)
        elif kl:
            num = eng.sptensor_kl(S, mode, _engine.node_major(Ft[mode]), gathered)
            Ft[mode] = eng.mu_apply(Ft[mode], num, None, _colsum_product(Ft, skip=mode), 1)      # mu.py:86-87
        else:
            rhs = eng.sptensor_mttkrp(S, mode, gathered)
            cross = None
            for i, f in enumerate(Ft):
                if i != mode:
                    g = ws.gram_of(i, f)[0]
                    cross = g if cross is None else eng.hadamard(cross, g)
            Ft[mode] = eng.mu_apply(Ft[mode], rhs, eng.small_gemm(cross, Ft[mode]), None, 2)
            last = (mode, rhs)

    cost = ws.block[ws.cost_at:ws.cost_at + 1]
    if kl and not hals:
        mode = N - 1
        eng.sptensor_kl(S, mode, _engine.node_major(Ft[mode]), [_engine.node_major(f) for f in _others(Ft, mode)], num=False,
                        cost_out=cost)
        cost.add_(_colsum_product(Ft).sum())
    else:
        if last is None:       # nothing was updated: the line on the last mode
            mode = N - 1
            last = (mode, eng.sptensor_mttkrp(S, mode, [_engine.node_major(f) for f in _others(Ft, mode)]))
        mode, rhs = last
        cross64 = None
        for i, f in enumerate(Ft):
            g64 = ws.gram_of(i, f)[1]
            if i != mode:
                cross64 = g64 if cross64 is None else cross64 * g64
        cost.copy_(D.normx2 - 2.0 * eng.dot(Ft[mode], rhs) + (ws.gram_of(mode, Ft[mode])[1] * cross64).sum())
        if hals:
            for index, sparse in enumerate(sparsity_coefficients):
                if sparse:
                    # np.linalg.norm(factor, ord=1): max column abs-sum of the dim x R factor = max row abs-sum of Ft
                    cost.add_(2 * sparse * Ft[index].abs().sum(dim=1).double().max())
        else:
            cost.mul_(0.5)                                # beta_divergence(., ., 2) = ||.||^2 / 2 (ntf.py:473)
    cost.div_(D.normx2)                                   # (ntf.py:475)
    return Ft, nstat


def _one_step_obs(eng, D, ws, Ft_in, beta, fixed_modes, empty):
    """One pass of MU updates over the modes on the stored entries only (unstored="missing"), then the cost, on the device.
    `empty`: D.empty_slices().  Returns (factors, 0); the cost is left in ws.block."""
    Ft = list(Ft_in)
    S, N = D.S, D.nway
    for mode in [m for m in range(N) if m not in fixed_modes]:
        gathered = [_engine.node_major(f) for f in _others(Ft, mode)]
        num, den = eng.sptensor_obs(S, mode, _engine.node_major(Ft[mode]), gathered, beta)
        new = eng.mu_apply(Ft[mode], num, den, None, beta)
        Ft[mode] = new if empty[mode] is None else torch.where(empty[mode], Ft[mode], new)
    cost = ws.block[ws.cost_at:ws.cost_at + 1]
    mode = N - 1
    eng.sptensor_obs(S, mode, _engine.node_major(Ft[mode]), [_engine.node_major(f) for f in _others(Ft, mode)], beta, sums=False,
                     cost_out=cost)
    cost.div_(D.normx2)                                   # (ntf.py:475)
    return Ft, 0


def _lists(nb_modes, sparsity_coefficients, fixed_modes, normalize):
    """The defaults of compute_ntf (ntf.py:292-301)."""
    if sparsity_coefficients is None or len(sparsity_coefficients) != nb_modes:
        print("Irrelevant number of sparsity coefficient (different from the number of modes), they have been set to None.")
        sparsity_coefficients = [None for i in range(nb_modes)]
    if fixed_modes is None:
        fixed_modes = []
    if normalize is None or len(normalize) != nb_modes:
        print("Irrelevant number of normalization booleans (different from the number of modes), they have been set to False.")
        normalize = [False for i in range(nb_modes)]
    return list(sparsity_coefficients), fixed_modes, normalize


def _check_factors(shape, factors):
    if len(factors) != len(shape) or any(tuple(np.shape(f)) != (shape[i], np.shape(factors[0])[1]) for i, f in enumerate(factors)):
        raise err.ArgumentException(f"NTF of a sparse tensor of shape {tuple(shape)} needs one factor of shape (extent, rank) per mode, "
                                    f"got {[tuple(np.shape(f)) for f in factors]}")


def compute_sparse_ntf(tensor_in, rank, factors_in, n_iter_max=100, tol=1e-8, update_rule="hals", beta=2,
                       sparsity_coefficients=[], fixed_modes=[], normalize=[], verbose=False, return_costs=False, alpha=0.5,
                       delta=0.01, sweep_log=None, group=None, unstored="zero"):
    """compute_ntf (ntf.py:288-344) for a sparse `tensor_in`.  Factors come back in the kind of `factors_in`."""
    shape = tuple(int(s) for s in tensor_in.shape)
    check_request(np.shape(factors_in[0])[1] if len(factors_in) else rank, update_rule, beta, len(shape), group=group,
                  unstored=unstored)
    missing = unstored == "missing"
    _check_factors(shape, factors_in)
    sparsity_coefficients, fixed_modes, normalize = _lists(len(shape), sparsity_coefficients, fixed_modes, normalize)
    dev = _device_of(tensor_in, factors_in)
    eng = _engine.get_engine(dev)
    D = SparseTensorData(eng, tensor_in, dev)
    Ft = [to_dev_t(f, dev).clone() for f in factors_in]
    deterministic = math.isinf(alpha)
    ws = _Buffers(eng, D.nway, dev, PIPELINE_DEPTH)
    retired = _loop.Retired(tol, verbose=verbose, sweep_log=sweep_log)
    main = torch.cuda.current_stream(dev)
    empty = D.empty_slices() if missing else None

    def enqueue(iteration, factors):
        ws.select(iteration % ws.blocks.shape[0])
        if missing:
            Ft, nstat = _one_step_obs(eng, D, ws, factors, beta, fixed_modes, empty)
        else:
            Ft, nstat = _one_step_dev(eng, D, ws, factors, update_rule, beta, sparsity_coefficients, fixed_modes, normalize, alpha,
                                      delta)
        step = _loop.Step(iteration, ws.slot, Ft, nstat)
        ws.host[ws.slot].copy_(ws.block, non_blocking=True)
        step.event = main.record_event()
        return step

    def settle(step):
        host = ws.host[step.slot]
        _loop.check_status(host, step.nstat)
        return float(host[ws.cost_at]), _loop.sweep_counts(host, step.nstat)

    # (the wall-clock sweep budget synchronises inside a step: nothing is gained by running ahead then)
    loop = _loop.Pipeline(enqueue, settle, retired, [main], depth=PIPELINE_DEPTH if deterministic or missing else 0)
    Ft = loop.run(n_iter_max, Ft)
    factors = [like_input(f.t(), factors_in[i]) for i, f in enumerate(Ft)]
    if return_costs:
        return factors, retired.cost_fct_vals, retired.toc
    return factors


def one_sparse_ntf_step(tensor_in, rank, in_factors, norm_tensor, update_rule, beta, sparsity_coefficients, fixed_modes, normalize,
                        alpha=0.5, delta=0.01, unstored="zero"):
    """one_ntf_step (ntf.py:422-477) for a sparse tensor, passed where the reference takes the unfoldings.  Returns (factors,
    cost).  The setup (sorted copies, chunk tables) is redone at every call: a loop belongs in compute_ntf."""
    shape = tuple(int(s) for s in tensor_in.shape)
    check_request(np.shape(in_factors[0])[1] if len(in_factors) else rank, update_rule, beta, len(shape), unstored=unstored)
    _check_factors(shape, in_factors)
    dev = _device_of(tensor_in, in_factors)
    eng = _engine.get_engine(dev)
    D = SparseTensorData(eng, tensor_in, dev)
    Ft = [to_dev_t(f, dev) for f in in_factors]
    ws = _Buffers(eng, D.nway, dev, 0)
    if unstored == "missing":
        Ft, nstat = _one_step_obs(eng, D, ws, Ft, beta, fixed_modes or [], D.empty_slices())
    else:
        Ft, nstat = _one_step_dev(eng, D, ws, Ft, update_rule, beta, list(sparsity_coefficients), fixed_modes, normalize, alpha, delta)
    host = ws.block.cpu()
    _loop.check_status(host, nstat)
    return [like_input(f.t(), in_factors[i]) for i, f in enumerate(Ft)], float(host[ws.cost_at])

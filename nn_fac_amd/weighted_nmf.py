"""Weighted NMF of DENSE data on the MI355X engine: a weight per entry next to the data, multiplicative updates of any beta >= 0.

`nmf`, `compute_nmf` and `one_nmf_step` of nn_fac_amd.nmf come here when `weights=` is given.  The fit minimises

    sum_ij Wg[i, j] d_beta(X[i, j] | (U V)[i, j])

with `Wg` an array of the data's shape: finite floats >= 0 (a known per-entry precision: Wg = 1 / variance), or booleans (a mask:
True = observed; converted once per run to 0.0 / 1.0 on the device).  An entry of weight zero is MISSING: it adds nothing to either
update or to the cost whatever the data holds there -- NaN and Inf included, so `weights=~np.isnan(X)` works on the array as it is.
Under a positive weight a zero of the data is an observed zero and a NaN or Inf propagates as in the unweighted drivers.  All-ones
weights are plain mu_betadivmin (mu.py:82-97).  One iteration, with P = U V never written:

    U:  nnf_mu_left_w_f32   num[k, i] = sum_j Wg X P^(beta-2) V[k, j],  den[k, i] = sum_j Wg P^(beta-1) V[k, j]
        nnf_mu_apply_f32    U <- max(U (num / den)^gamma(beta), 1e-12); a row of U whose weights are all zero (den = 0 down its
                            whole column of the r x m sums) keeps its value bit for bit, as an empty slice does under unstored="missing"
    V:  nnf_mu_right_w_f32, nnf_mu_apply_f32, the same on the columns
    cost: nnf_betadiv_w_f32 after both updates (not normalised, as nmf.py:455)

beta = 1 and beta = 2 lose the shortcuts of the unweighted path (rowsum(V), the Gram form): under weights every beta needs the
per-entry denominator, so every beta runs the two-accumulator kernels.  This is the dense counterpart of
`observed_entries(array, mask)` + `unstored="missing"` (sparse_nmf.py): that route gathers twelve bytes per observed entry and is
the tool for data that is mostly missing; this one streams the weights next to the data and is the tool for data that is mostly
there -- and the only one for weights other than 0 and 1.

Refused before the device is touched, each with what to use instead: update_rule="hals" (one Gram per row, a different algorithm),
sparse data (that is unstored="missing"), `group=` (sharded runs), init="nndsvd" (an SVD of data with holes in it), ranks above
128, a weight array of another shape or dtype, beta < 0.  Negative or non-finite weights are refused after the upload, by one
device reduction.  Not built: weights on ntd, PARAFAC2, the simplex, deep and multilayer drivers; one-byte masks in the
kernels; a cost that rides in the left update.  (Weights on ntf: weighted_ntf.py.)

The outer loop, its stopping test, `return_costs`, `toc` and `sweep_log` are those of compute_nmf, on `_outer_loop.Pipeline`.
"""
import math
import numbers

import numpy as np
import torch

from . import _outer_loop as _loop
from . import engine as _engine
from ._convert import device_of, to_dev, to_dev_t, like_input, is_sparse
from ._status import NMF_COST, NMF_WORDS
from .utils import errors as err

PIPELINE_DEPTH = 1   # outer iterations enqueued ahead of the one whose cost the host is looking at


def _kind(weights):
    """'bool' or 'float' of a weight array or tensor, None for anything else."""
    dt = weights.dtype if isinstance(weights, torch.Tensor) else np.asarray(weights).dtype
    if dt in (torch.bool, np.dtype(bool)):
        return "bool"
    floating = dt.is_floating_point if isinstance(dt, torch.dtype) else np.issubdtype(dt, np.floating)
    return "float" if floating else None


def check_request(data, weights, rank, update_rule, beta, group=None, init=None):
    """Everything the weighted path refuses that can be said without the device, before anything is uploaded or launched."""
    if is_sparse(data):
        raise err.InvalidArgumentValue('weights= is for dense data: sparse data says which entries count by storing them -- pass '
                                       'unstored="missing" to fit the stored entries only (observed_entries(array, mask) builds '
                                       'that input from a dense array and a mask)')
    if update_rule not in ["hals", "mu"]:
        raise err.InvalidArgumentValue(f"Invalid update rule: {update_rule}")
    if update_rule == "hals":
        raise NotImplementedError('weighted NMF (weights=) is built for the multiplicative update: hals then needs one Gram matrix '
                                  'per row, a different algorithm; use update_rule="mu" (beta = 2 for the Frobenius fit)')
    if not (isinstance(beta, numbers.Real) and 0 <= beta < math.inf):
        raise err.InvalidArgumentValue(f"Invalid value for beta: {beta!r} (a finite beta >= 0 is needed).")
    if group is not None:
        raise NotImplementedError("weighted NMF does not run row-sharded: group= is refused; run it on one device")
    if init is not None and init.lower() == "nndsvd":
        raise NotImplementedError('init="nndsvd" needs a singular value decomposition of the data, which entries of weight zero '
                                  'leave undefined: use init="random" or init="custom" with weights=')
    if int(rank) > _engine.MAX_RANK:
        raise err.EngineError(f"weighted NMF: rank {int(rank)} is above the {_engine.MAX_RANK} the weighted kernels are built for; "
                              f"use a rank <= {_engine.MAX_RANK}, or the unweighted drivers, which take any rank")
    if tuple(np.shape(weights)) != tuple(data.shape):
        raise err.InvalidArgumentValue(f"weights must have the shape of the data, {tuple(data.shape)}; got {tuple(np.shape(weights))}")
    if _kind(weights) is None:
        raise err.InvalidArgumentValue("weights must be floating point (finite, >= 0) or boolean (a mask: True = observed); "
                                       "convert integer weights with .astype(float)")


def weights_to_dev(weights, dev):
    """The weights as a float32 device matrix (a mask: 0.0 / 1.0), checked finite and >= 0 by one device reduction."""
    Wg = to_dev(weights, dev)
    if _kind(weights) == "float" and not bool((torch.isfinite(Wg) & (Wg >= 0)).all()):
        raise err.InvalidArgumentValue("weights must be finite and >= 0 (a missing entry is a weight of zero, or False in a "
                                       "boolean mask: ~np.isnan(data))")
    return Wg


class _Buffers(_loop.StatusRing):
    """The ring of status blocks (the cost word of every iteration in flight)."""

    def __init__(self, dev, depth):
        self.init_ring(depth + 2, NMF_WORDS, dev)


def _keep_unweighted(F_in, F, den):
    """A slice whose weights are all zero has den = 0 in every rank row (and num = 0: the update would be 0 / 0): it keeps its
    start value, as a slice without stored entries does under unstored="missing"."""
    return torch.where((den == 0).all(dim=0, keepdim=True), F_in, F)


def _one_step_w(eng, X, Wg, ws, Ut_in, V_in, beta, fixed_modes):
    """One pass of weighted MU updates on U then V, then the weighted cost, on the device (the inputs are not modified).
    Returns (Ut, V, 0); the cost is left in ws.block."""
    Ut, V = Ut_in, V_in
    if 0 not in fixed_modes:
        num, den = eng.mu_left_w(X, Wg, Ut_in, V, beta)
        Ut = _keep_unweighted(Ut_in, eng.mu_apply(Ut_in, num, den, None, beta), den)
    if 1 not in fixed_modes:
        num, den = eng.mu_right_w(X, Wg, Ut, V_in, beta)
        V = _keep_unweighted(V_in, eng.mu_apply(V_in, num, den, None, beta), den)
    eng.betadiv_w(X, Wg, Ut, V, beta, out=ws.block[NMF_COST:NMF_COST + 1])
    return Ut, V, 0


def compute_weighted_nmf(data, rank, U_in, V_in, weights, n_iter_max=100, tol=1e-8, update_rule="mu", beta=2, fixed_modes=[],
                         verbose=False, return_costs=False, sweep_log=None, group=None):
    """compute_nmf (nmf.py:284-329) with a weight per entry.  Factors come back in the kind of U_in / V_in."""
    check_request(data, weights, np.shape(U_in)[1], update_rule, beta, group=group)
    fixed_modes = [] if fixed_modes is None else fixed_modes
    dev = device_of(data, U_in, V_in)
    eng = _engine.get_engine(dev)
    X = to_dev(data, dev)
    Wg = weights_to_dev(weights, dev)
    Ut = to_dev_t(U_in, dev).clone()
    V = to_dev(V_in, dev).clone()
    ws = _Buffers(dev, PIPELINE_DEPTH)
    retired = _loop.Retired(tol, verbose=verbose, sweep_log=sweep_log)
    main = torch.cuda.current_stream(dev)

    def enqueue(iteration, factors):
        ws.select(iteration % ws.blocks.shape[0])
        Ut, V, nstat = _one_step_w(eng, X, Wg, ws, factors[0], factors[1], beta, fixed_modes)
        step = _loop.Step(iteration, ws.slot, (Ut, V), nstat)
        ws.host[ws.slot].copy_(ws.block, non_blocking=True)
        step.event = main.record_event()
        return step

    def settle(step):
        host = ws.host[step.slot]
        return float(host[NMF_COST]), _loop.sweep_counts(host, step.nstat)

    loop = _loop.Pipeline(enqueue, settle, retired, [main], depth=PIPELINE_DEPTH)
    Ut, V = loop.run(n_iter_max, (Ut, V))
    U_out, V_out = like_input(Ut.t(), U_in), like_input(V, V_in)
    if return_costs:
        return U_out, V_out, retired.cost_fct_vals, retired.toc
    return U_out, V_out


def one_weighted_nmf_step(data, rank, U_in, V_in, weights, update_rule, beta, fixed_modes):
    """one_nmf_step (nmf.py:387-458) with a weight per entry.  Returns (U, V, cost)."""
    check_request(data, weights, np.shape(U_in)[1], update_rule, beta)
    fixed_modes = [] if fixed_modes is None else fixed_modes
    dev = device_of(data, U_in, V_in)
    eng = _engine.get_engine(dev)
    X = to_dev(data, dev)
    Wg = weights_to_dev(weights, dev)
    Ut, V = to_dev_t(U_in, dev), to_dev(V_in, dev)
    ws = _Buffers(dev, 0)
    Ut2, V2, _ = _one_step_w(eng, X, Wg, ws, Ut, V, beta, fixed_modes)
    return like_input(Ut2.t(), U_in), like_input(V2, V_in), float(ws.block.cpu()[NMF_COST])

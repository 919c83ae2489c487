"""Weighted NTF of DENSE tensors on the MI355X engine: a weight per entry next to the tensor, multiplicative updates of any
beta >= 0, tensors of any order >= 3.

`ntf`, `compute_ntf` and `one_ntf_step` of nn_fac_amd.ntf come here when `weights=` is given.  The fit minimises

    sum_e Wg[e] d_beta(T[e] | model[e])

with `Wg` an array of the tensor's shape: finite floats >= 0 (a known per-entry precision: Wg = 1 / variance), or booleans (a mask:
True = observed; converted once per run to 0.0 / 1.0 on the device).  An entry of weight zero is MISSING: it adds nothing to any
update or to the cost whatever the tensor holds there -- NaN and Inf included, so `weights=~np.isnan(T)` works on the array as it
is.  Under a positive weight a zero of the data is an observed zero and a NaN or Inf propagates as in the unweighted drivers.
All-ones weights are plain mu_betadivmin (mu.py:82-97) on every unfolding.  Per mode, in mode order, with V = khatri_rao(others)^T:

    not the last, r <= 64     nnf_mu_mode_w_f32 on the tensor's and the weights' own layout, seen as (before, I_mode, behind)
    not the last, otherwise   nnf_mu_right_w_f32 on unfoldings of the tensor AND of the weights, materialised once per run
                              (r = 65 .. 128, or NNF_MU_UNFOLD=1, read at call time: the A/B switch of the unweighted path)
    the last                  nnf_mu_right_w_f32 on the views T.view(-1, I_last), Wg.view(-1, I_last)
    then                      nnf_mu_apply_f32: F <- max(F (num / den)^gamma(beta), 1e-12); a slice whose weights are all zero
                              (den = 0 in every rank) keeps its value bit for bit, as an empty slice does under unstored="missing"
    cost                      nnf_betadiv_w_f32 on the last-mode view against khatri_rao(others)^T of the FINAL factors, plus the
                              sparsity terms of the unweighted MU path (ntf.py:472-474)

compute_ntf divides the cost by sum Wg T^2 over the entries of positive weight (fp64, once per run, the data under zero weights
read as 0): ||T||^2 at all-ones weights, the stored-entry norm of unstored="missing" at a 0/1 mask.  one_ntf_step divides by the
caller's norm_tensor^2, as the reference line does (ntf.py:475).

This is the dense counterpart of a SparseCOO of the observed entries with unstored="missing" (sparse_ntf.py): that route gathers
4 N + 4 bytes per observed entry and is the tool for tensors that are mostly missing; this one streams the weights next to the
tensor and is the tool for tensors that are mostly there -- and the only one for weights other than 0 and 1.

Refused before anything is uploaded, each with what to use instead: update_rule="hals", a sparse tensor (that is
unstored="missing"), `group=`, init="nndsvd", ranks above 128, weights of another shape or of an integer dtype, beta < 0 or not
finite.  Negative or non-finite weights are refused after the upload, by one device reduction.  Not built: weights on ntd,
PARAFAC2, the simplex, deep and multilayer drivers; HALS; sharded runs; one-byte masks in the kernels.

The outer loop, its stopping test, `return_costs`, `toc` and `sweep_log` are those of compute_ntf, on `_outer_loop.Pipeline`.
"""
import math
import numbers

import numpy as np
import torch

from . import _outer_loop as _loop
from . import engine as _engine
from ._convert import device_of, to_dev, to_dev_t, like_input, is_sparse_tensor
from ._status import NMF_COST
from ._tensor_state import mode_view, mu_on_layout
from .ntf import _krao_t
from .utils import errors as err
from .weighted_nmf import PIPELINE_DEPTH, _Buffers, _keep_unweighted, _kind, weights_to_dev


def check_request(tensor_shape, sparse, weights, rank, update_rule, beta, group=None, init=None):
    """Everything the weighted path refuses that can be said without the device, before anything is uploaded or launched."""
    if update_rule not in ["hals", "mu"]:
        raise err.InvalidArgumentValue(f"Invalid update rule: {update_rule}")
    if update_rule == "hals":
        raise NotImplementedError('weighted NTF (weights=) is built for the multiplicative update: hals then needs one Gram matrix '
                                  'per slice, a different algorithm; use update_rule="mu" (beta = 2 for the Frobenius fit)')
    if sparse:
        raise err.InvalidArgumentValue('weights= is for dense tensors: a sparse tensor says which entries count by storing them -- '
                                       'pass unstored="missing" to fit the stored entries only')
    if group is not None:
        raise NotImplementedError("weighted NTF does not run sharded: group= is refused; run it on one device")
    if init is not None and init.lower() == "nndsvd":
        raise NotImplementedError('init="nndsvd" needs singular value decompositions of the unfoldings, which entries of weight zero '
                                  'leave undefined: use init="random" or init="custom" with weights=')
    if int(rank) > _engine.MAX_RANK:
        raise _engine.EngineError(f"weighted NTF: rank {int(rank)} is above the {_engine.MAX_RANK} the weighted kernels are built "
                                  f"for; use a rank <= {_engine.MAX_RANK}, or the unweighted drivers, which take any rank")
    if len(tensor_shape) < 3:
        raise NotImplementedError("NTF needs a tensor of order >= 3 (a matrix is nmf's business: nmf(..., weights=))")
    shape, wshape = tuple(int(s) for s in tensor_shape), tuple(np.shape(weights))
    if wshape != shape:
        raise err.InvalidArgumentValue(f"weights must have the shape of the tensor, {shape}; got {wshape}")
    if _kind(weights) is None:
        raise err.InvalidArgumentValue("weights must be floating point (finite, >= 0) or boolean (a mask: True = observed); "
                                       "convert integer weights with .astype(float)")
    if not (isinstance(beta, numbers.Real) and 0 <= beta < math.inf):
        raise err.InvalidArgumentValue(f"Invalid value for beta: {beta!r} (a finite beta >= 0 is needed).")


class _State:
    """The contiguous tensor and its weights on the device and, on the unfolded route only, the unfoldings of both."""

    def __init__(self, eng, T, Wg):
        self.eng, self.T, self.Wg = eng, T.contiguous(), Wg.contiguous()
        self.nway = self.T.dim()
        self._unf = {}

    def unfolded(self, mode):
        """(tl.unfold(T, mode)^T, the same of the weights): contiguous prod(other dims) x I_mode matrices, made once per run."""
        if mode not in self._unf:
            self._unf[mode] = tuple(torch.movedim(A, mode, -1).reshape(-1, A.shape[mode]).contiguous() for A in (self.T, self.Wg))
        return self._unf[mode]

    def last_views(self):
        I = self.T.shape[-1]
        return self.T.view(-1, I), self.Wg.view(-1, I)

    def weighted_norm2(self):
        """sum Wg T^2 over the entries of positive weight as a 1-element float64 device tensor: fp64 sums of blocks of the leading
        rows, the data under zero weights read as 0 (a NaN there does not reach it)."""
        X, W = self.last_views()
        total = torch.zeros(1, dtype=torch.float64, device=X.device)
        rows = max(1, (1 << 24) // int(X.shape[1]))
        for a in range(0, int(X.shape[0]), rows):
            w = W[a:a + rows].double()
            x = torch.where(w > 0, X[a:a + rows].double(), torch.zeros((), dtype=torch.float64, device=X.device))
            total += (w * x * x).sum()
        return total


def _one_step_w(st, ws, Ft_in, beta, sparsity_coefficients, fixed_modes, norm2=None):
    """One pass of weighted MU updates over the modes, then the weighted cost, on the device (the inputs are not modified).
    Returns (factors, 0); the cost -- divided by `norm2`, a float64 device scalar, if given -- is left in ws.block."""
    eng, N = st.eng, st.nway
    Ft = list(Ft_in)
    last = N - 1
    Ut_last = None            # khatri_rao(others)^T of the last mode's update: the cost's operand when that mode is updated
    for mode in [m for m in range(N) if m not in fixed_modes]:
        V = _krao_t(Ft, mode)
        if mode == last:
            X, W = st.last_views()
            num, den = eng.mu_right_w(X, W, V, Ft[mode], beta)
            Ut_last = V
        elif mu_on_layout(eng, Ft[mode].shape[0]):
            num, den = eng.mu_mode_w(mode_view(st.T, mode), mode_view(st.Wg, mode), Ft[mode], V, beta)
        else:
            X, W = st.unfolded(mode)
            num, den = eng.mu_right_w(X, W, V, Ft[mode], beta)
        Ft[mode] = _keep_unweighted(Ft[mode], eng.mu_apply(Ft[mode], num, den, None, beta), den)
    if Ut_last is None:       # the last mode is fixed: the other factors have moved since anything was built from them
        Ut_last = _krao_t(Ft, last)
    cost = ws.block[NMF_COST:NMF_COST + 1]
    X, W = st.last_views()
    eng.betadiv_w(X, W, Ut_last, Ft[last], beta, out=cost)
    for index, sparse in enumerate(sparsity_coefficients):
        if sparse and index not in fixed_modes:
            # np.linalg.norm(factor, ord=1): max column abs-sum of the dim x R factor = max row abs-sum of Ft (ntf.py:472-474)
            cost.add_(2 * sparse * Ft[index].abs().sum(dim=1).double().max())
    if norm2 is not None:
        cost.div_(norm2)
    return Ft, 0


def _lists(nb_modes, sparsity_coefficients, fixed_modes):
    """The defaults of compute_ntf (ntf.py:292-301) for the lists the weighted path reads."""
    if sparsity_coefficients is None or len(sparsity_coefficients) != nb_modes:
        print("Irrelevant number of sparsity coefficient (different from the number of modes), they have been set to None.")
        sparsity_coefficients = [None for i in range(nb_modes)]
    return list(sparsity_coefficients), ([] if fixed_modes is None else fixed_modes)


def compute_weighted_ntf(tensor_in, rank, factors_in, weights, n_iter_max=100, tol=1e-8, update_rule="mu", beta=2,
                         sparsity_coefficients=[], fixed_modes=[], verbose=False, return_costs=False, sweep_log=None, group=None):
    """compute_ntf (ntf.py:288-344) with a weight per entry.  Factors come back in the kind of `factors_in`."""
    check_request(tensor_in.shape, is_sparse_tensor(tensor_in), weights, np.shape(factors_in[0])[1] if len(factors_in) else rank,
                  update_rule, beta, group=group)
    sparsity_coefficients, fixed_modes = _lists(len(tensor_in.shape), sparsity_coefficients, fixed_modes)
    dev = device_of(tensor_in, *factors_in)
    eng = _engine.get_engine(dev)
    st = _State(eng, to_dev(tensor_in, dev), weights_to_dev(weights, dev))
    norm2 = st.weighted_norm2()
    Ft = [to_dev_t(f, dev).clone() for f in factors_in]
    ws = _Buffers(dev, PIPELINE_DEPTH)
    retired = _loop.Retired(tol, verbose=verbose, sweep_log=sweep_log)
    main = torch.cuda.current_stream(dev)

    def enqueue(iteration, factors):
        ws.select(iteration % ws.blocks.shape[0])
        Ft, nstat = _one_step_w(st, ws, factors, beta, sparsity_coefficients, fixed_modes, norm2=norm2)
        step = _loop.Step(iteration, ws.slot, Ft, nstat)
        ws.host[ws.slot].copy_(ws.block, non_blocking=True)
        step.event = main.record_event()
        return step

    def settle(step):
        host = ws.host[step.slot]
        return float(host[NMF_COST]), _loop.sweep_counts(host, step.nstat)

    loop = _loop.Pipeline(enqueue, settle, retired, [main], depth=PIPELINE_DEPTH)
    Ft = loop.run(n_iter_max, Ft)
    factors = [like_input(f.t(), factors_in[i]) for i, f in enumerate(Ft)]
    if return_costs:
        return factors, retired.cost_fct_vals, retired.toc
    return factors


def one_weighted_ntf_step(unfolded_tensors, rank, in_factors, norm_tensor, weights, update_rule, beta, sparsity_coefficients,
                          fixed_modes):
    """one_ntf_step (ntf.py:422-477) with a weight per entry: `weights` in the tensor's shape or in that of the mode-0 unfolding.
    Returns (factors, cost), the cost divided by norm_tensor^2."""
    sparse = is_sparse_tensor(unfolded_tensors)
    dims = tuple(int(s) for s in unfolded_tensors.shape) if sparse else tuple(int(u.shape[0]) for u in unfolded_tensors)
    if not sparse and len(dims) >= 2 and tuple(np.shape(weights)) == tuple(int(s) for s in unfolded_tensors[0].shape):
        weights = weights.reshape(dims)
    check_request(dims, sparse, weights, np.shape(in_factors[0])[1] if len(in_factors) else rank, update_rule, beta)
    sparsity_coefficients, fixed_modes = _lists(len(dims), sparsity_coefficients, fixed_modes)
    dev = device_of(*unfolded_tensors, *in_factors)
    eng = _engine.get_engine(dev)
    st = _State(eng, to_dev(unfolded_tensors[0], dev).reshape(dims), weights_to_dev(weights, dev))
    Ft = [to_dev_t(f, dev) for f in in_factors]
    ws = _Buffers(dev, 0)
    Ft, _ = _one_step_w(st, ws, Ft, beta, sparsity_coefficients, fixed_modes)
    cost = float(ws.block.cpu()[NMF_COST]) / norm_tensor ** 2
    return [like_input(f.t(), in_factors[i]) for i, f in enumerate(Ft)], cost

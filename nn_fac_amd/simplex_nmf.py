"""Simplex-constrained KL-NMF on the MI355X engine -- drop-in for nn_fac/simplex_nmf.py:16-71 at beta = 1.

NMF with the columns of H on the unit simplex (abundances, topic models): Leplat, Gillis, Idier, "Multiplicative updates for NMF
with beta-divergences under disjoint equality constraints", SIMAX 42(2), 2021.  One outer iteration is

    W <- mu_betadivmin(W, H, data, 1)                      nnf_mu_left_f32 (r <= 64: nnf_mu_left_kl_cost_f32, see below)
    C, D of mu.py:165-166                                  nnf_mu_right_accum_f32 (beta = 1: D is r doubles)
    Newton solve for the multipliers + update of H         nnf_simplex_proj_kl_f32
    cost = beta_divergence(data, W H, 1)                   rides on the W update of the NEXT iteration up to rank 64, as in the
                                                           MU beta = 1 loop of nmf.run_steps; nnf_betadiv_f32 above rank 64 and
                                                           after the last iteration

on `_outer_loop.Pipeline`: the host looks at status blocks one or two iterations behind the device; a block carries the cost
and the two Newton words (iterations run, last max |dlambda|), from which the host raises the reference's warning, once per
iteration that ran all 100 Newton iterations without reaching the tolerance.

beta != 1 is refused (NotImplementedError) before the device is touched: the reference's rule does not put the columns of H on
the simplex there (beta = 2: column sums between 5e-12 and 36; beta in {0, 0.5, 1.5, 3}: NaN in the first step, a fractional
power of a negative start value), so there is nothing to be faithful to.
"""
import warnings

import numpy as np
import torch

from . import _outer_loop as _loop
from . import engine as _engine
from ._convert import device_of, to_dev, to_dev_t, like_input
from .utils import errors as err
from .utils import initialize_factors as init_factors

eps = 1e-12   # simplex_nmf.py:14

NEWTON_MAX_ITER = 100     # mu.py:170
NEWTON_WARNING = 'Maximum of iterations reached in the update of the Lagrangian multipliers.'      # normalize_wh.py:56
PIPELINE_DEPTH = 1        # outer iterations enqueued ahead of the one whose cost the host is looking at
# words of an iteration's status block
SX_COST, SX_NEWTON_COUNT, SX_NEWTON_LAST, SX_WORDS = 0, 1, 2, 8


def check_beta(beta, where):
    """Every beta but 1 is refused, with the reason, before anything is uploaded or launched."""
    if beta != 1:
        raise NotImplementedError(
            f"{where}: simplex-constrained NMF is built for beta = 1 only.  The reference's update does not reach the simplex for "
            f"any other beta (beta = 2 leaves column sums between 5e-12 and 36 and never converges; beta in (0, 0.5, 1.5, 3) turns "
            f"NaN in the first step), so there is no result to reproduce (got beta = {beta!r})")


def check_rank(r, where):
    if int(r) > _engine.MAX_RANK:
        raise err.EngineError(f"{where}: rank {int(r)} is above the {_engine.MAX_RANK} the simplex projection kernel is built for")


def newton_warning(count, last, tol, max_iter=NEWTON_MAX_ITER):
    """normalize_wh.py:52-56: the warning fires when the last of `max_iter` iterations did not meet `<= tol`."""
    if int(count) >= int(max_iter) and not float(last) <= float(tol):
        warnings.warn(NEWTON_WARNING)


def simplex_beta_nmf(data, rank, beta, n_iter_max=100, tol=1e-8, tol_update_lagrangian=1e-6, init="random", W_0=None, H_0=None,
                     verbose=False, deterministic=False, seed=0):
    """simplex_nmf.py:16-30."""
    check_beta(beta, "simplex_beta_nmf")
    if deterministic:
        np.random.seed(seed)

    if init.lower() == "custom":
        if W_0 is None or H_0 is None:
            raise err.CustomNotValidFactors("Custom initialization, but (at least) one factor is set to 'None'")
        W, H = W_0, H_0
    else:
        W, H = init_factors.nmf_initialization(data, rank, init, deterministic=deterministic, seed=seed)

    return compute_simplex_beta_nmf(data=data, W_0=W, H_0=H, rank=rank, beta=beta, n_iter_max=n_iter_max, tol=tol,
                                    tol_update_lagrangian=tol_update_lagrangian, verbose=verbose)


def compute_simplex_beta_nmf(data, W_0, H_0, rank, beta, n_iter_max=100, tol=1e-8, tol_update_lagrangian=1e-6, verbose=False):
    """simplex_nmf.py:32-65.  Returns (W, H, cost_fct_vals, toc); the inputs are not modified."""
    check_beta(beta, "compute_simplex_beta_nmf")
    if W_0 is None or H_0 is None:
        raise err.CustomNotValidFactors("Custom initialization, but (at least) one factor is set to 'None'")
    check_rank(W_0.shape[1], "compute_simplex_beta_nmf")
    dev = device_of(data, W_0, H_0)
    eng = _engine.get_engine(dev)
    X = to_dev(data, dev)
    Ut = to_dev_t(W_0, dev)
    V = to_dev(H_0, dev)
    retired = _loop.Retired(tol, verbose=verbose)
    Ut, V = run_steps(eng, X, Ut, V, n_iter_max, tol_update_lagrangian, retired)
    return like_input(Ut.t(), W_0), like_input(V, H_0), retired.cost_fct_vals, retired.toc


def one_step_simplex_beta_nmf(data, W, H, rank, beta, tol_update_lagrangian):
    """simplex_nmf.py:67-71.  Returns (W, H, cost)."""
    check_beta(beta, "one_step_simplex_beta_nmf")
    check_rank(W.shape[1], "one_step_simplex_beta_nmf")
    dev = device_of(data, W, H)
    eng = _engine.get_engine(dev)
    X = to_dev(data, dev)
    block = torch.zeros(SX_WORDS, dtype=torch.float64, device=dev)
    Ut = eng.mu_left(X, to_dev_t(W, dev), to_dev(H, dev), 1)
    V = simplex_right(eng, X, Ut, to_dev(H, dev), tol_update_lagrangian, block[SX_NEWTON_COUNT:SX_NEWTON_LAST + 1])
    eng.betadiv(X, Ut, V, 1, out=block[SX_COST:SX_COST + 1])
    host = block.cpu()
    newton_warning(host[SX_NEWTON_COUNT], host[SX_NEWTON_LAST], tol_update_lagrangian)
    return like_input(Ut.t(), W), like_input(V, H), float(host[SX_COST])


def simplex_right(eng, X, Ut, V, tol_update_lagrangian, newton_words):
    """mu.py:161-175 on the device layout (Ut: r x m, V: r x n): a fresh V with its columns on the simplex; the two Newton words
    go to `newton_words` (2 float64 on the device)."""
    num, den, den_vec = eng.mu_right_accum(X, Ut, V, 1)
    out, _ = eng.simplex_proj(V, num, den, den_vec, tol=tol_update_lagrangian, max_iter=NEWTON_MAX_ITER, status=newton_words)
    return out


def run_steps(eng, X, Ut, V, n_iter, tol_update_lagrangian, retired):
    """The `for iteration` loop of simplex_nmf.py:40-63 with the device running ahead of the host.  Every step writes fresh factor
    tensors (the caller's are never touched, dropped speculative steps cost nothing) and one status block; the only readback
    per iteration is that block.  Up to rank 64 the KL cost of iteration i is a by-product of the W update of iteration i + 1
    (nnf_mu_left_kl_cost_f32), and of one more such update, its output dropped, after the last iteration: every cost of a run
    comes from the same kernel.  Above rank 64 the cost is a pass of its own at the end of the step (nnf_betadiv_f32)."""
    cuda = X.is_cuda
    fused = cuda and isinstance(eng, _engine.Engine) and Ut.shape[0] <= eng.MU_FUSED_MAX_RANK
    depth = PIPELINE_DEPTH + (1 if fused else 0)
    ring = _loop.StatusRing()
    ring.init_ring(depth + 2, SX_WORDS, X.device)
    main = torch.cuda.current_stream(X.device) if cuda else None
    owed = None           # fused: the step whose cost has not been launched yet

    def cost_word(slot):
        return ring.blocks[slot][SX_COST:SX_COST + 1]

    def send(step):
        """The copy of the step's block to the host, behind everything that writes it."""
        if cuda:
            ring.host[step.slot].copy_(ring.blocks[step.slot], non_blocking=True)
            step.event = main.record_event()
        else:
            ring.host[step.slot].copy_(ring.blocks[step.slot])

    def enqueue(iteration, factors):
        nonlocal owed
        Ut, V = factors
        ring.select(iteration % ring.blocks.shape[0])
        if fused and owed is not None:
            Ut = eng.mu_left(X, Ut, V, 1, cost_out=cost_word(owed.slot))      # + the cost of the previous step
        else:
            Ut = eng.mu_left(X, Ut, V, 1)
        V = simplex_right(eng, X, Ut, V, tol_update_lagrangian, ring.block[SX_NEWTON_COUNT:SX_NEWTON_LAST + 1])
        step = _loop.Step(iteration, ring.slot, (Ut, V), 0)
        if fused:
            if owed is not None:
                send(owed)
            owed = step
        else:
            eng.betadiv(X, Ut, V, 1, out=cost_word(ring.slot))
            send(step)
        return step

    def cost_of_the_last_step():
        if fused and owed is not None and owed.event is None:
            eng.mu_left(X, owed.result[0], owed.result[1], 1, cost_out=cost_word(owed.slot))      # (the update itself is dropped)
            send(owed)

    def settle(step):
        host = ring.host[step.slot]
        newton_warning(host[SX_NEWTON_COUNT], host[SX_NEWTON_LAST], tol_update_lagrangian)
        return float(host[SX_COST]), []

    loop = _loop.Pipeline(enqueue, settle, retired, [main] if cuda else [], depth=depth, before_flush=cost_of_the_last_step)
    return loop.run(n_iter, (Ut, V))

"""fp64 NumPy restatement of the reference's simplex-constrained KL-NMF (beta = 1 only): nn_fac/simplex_nmf.py:32-71,
update_rules/mu.py:161-175, utils/normalize_wh.py:24-58 -- written from the statements of those lines, pinned to the reference's
own results by tests/golden/g12_simplex.npz (tests/test_simplex_golden.py; the fixture is written by tools/gen_golden_simplex.py,
which asserts this file equal to the real reference first).  Test infrastructure: what the device kernels are compared with.

Extensions over the reference, all off by default:
  info=           a dict that receives the Newton iteration count, every max|dlambda| and whether the warning fired
  reverse_k=      the two sums over k of the Newton step run over the rows in reversed order (the floor that the summation
                  order alone sets, for the tolerances of tests/test_gpu_simplex.py)
  round32=        the driver rounds W, H, C and D to float32 after every update (what the device's fp32 operands hold)
"""
import warnings

import numpy as np

EPS_MU = 1e-12        # mu.py:18
EPS_NEWTON = 1e-8     # normalize_wh.py:4
WARNING = 'Maximum of iterations reached in the update of the Lagrangian multipliers.'


def _colsum(M, reverse_k):
    # (a copy: NumPy may walk a negatively strided view in memory order)
    return np.sum(np.ascontiguousarray(M[::-1]), axis=0) if reverse_k else np.sum(M, axis=0)


def update_lagragian_multipliers_simplex_projection(C, D, H, beta, lagrangian_multipliers_0, tol=1e-6, n_iter_max=100,
                                                    info=None, reverse_k=False):
    """normalize_wh.py:24-58 at beta = 1.  C, D, H: k x n (D may be k x 1: the same denominator in every column);
    lagrangian_multipliers_0: n x 1.  Returns the n x 1 multipliers."""
    if beta != 1:
        raise NotImplementedError("restated for beta = 1 only")
    k, n = H.shape
    lam = np.array(lagrangian_multipliers_0, dtype=np.float64).reshape(n).copy()
    deltas, warned = [], False
    for it in range(n_iter_max):
        prev = lam.copy()
        den = D - lam[None, :]
        with np.errstate(all="ignore"):
            Mat = H * (C / (den + EPS_NEWTON))           # :35
            Matp = H * (C / (den ** 2))                  # :36  (no eps in this denominator)
            xi = _colsum(Mat, reverse_k) - 1.0           # :46-47
            xip = _colsum(Matp, reverse_k)               # :48
            lam = lam - xi / (xip + EPS_NEWTON)          # :50
            deltas.append(np.max(np.abs(lam - prev)))    # :52  (np.max: a NaN anywhere makes it NaN, which fails <= tol)
        if deltas[-1] <= tol:
            break
        if it == n_iter_max - 1:
            warned = True
            warnings.warn(WARNING)
    if info is not None:
        info.update(count=len(deltas), deltas=np.array(deltas), warned=warned)
    return lam.reshape(n, 1)


def simplex_update(C, D, H, lam):
    """mu.py:172-173 at beta = 1 (gamma = 1): H <- max(H * (C / ((D - lambda) + 1e-12)), 1e-12)."""
    with np.errstate(all="ignore"):
        return np.maximum(H * (C / ((D - np.asarray(lam).reshape(1, -1)) + EPS_MU)), EPS_MU)


def lambda_start(C, D, H):
    """mu.py:168 at beta = 1: D[0,:] - C[0,:] * H[0,:]."""
    return (np.broadcast_to(D, H.shape)[0, :] - C[0, :] * H[0, :]).reshape(-1, 1)


def simplex_operands(data, W, H):
    """C = W^T(X / (WH)), D = W^T 1   (mu.py:165-166 at beta = 1)."""
    WH = W @ H
    return W.T @ ((WH ** (-1)) * data), W.T @ (WH ** 0)


def simplex_proj_mu(data, W, H, beta, tol_update_lagrangian=1e-6, info=None, reverse_k=False, round32=False):
    if beta != 1:
        raise NotImplementedError("restated for beta = 1 only")
    C, D = simplex_operands(data, W, H)
    if round32:
        C, D = _r32(C), _r32(D)
    lam = update_lagragian_multipliers_simplex_projection(C, D, H, beta, lambda_start(C, D, H), tol=tol_update_lagrangian,
                                                          n_iter_max=100, info=info, reverse_k=reverse_k)
    return simplex_update(C, D, H, lam)


def _r32(A):
    return np.asarray(A, dtype=np.float32).astype(np.float64)


def mu_left_kl(W, H, data):
    """mu_betadivmin(W, H, data, 1): mu.py:84-88."""
    K = W @ H
    return np.maximum(W * (((K ** (-1)) * data) @ H.T / np.sum(H, axis=1)[None, :]), EPS_MU)


def kl_divergence(a, b):
    """beta_divergence(a, b, 1) on positive operands (beta_divergence.py:45-48)."""
    return np.sum(a * np.log(a / b) - a + b)


def one_step_simplex_beta_nmf(data, W, H, rank, beta, tol_update_lagrangian, info=None, round32=False):
    W = mu_left_kl(W, H, data)
    if round32:
        W = _r32(W)
    H = simplex_proj_mu(data, W, H, beta, tol_update_lagrangian, info=info, round32=round32)
    if round32:
        H = _r32(H)
    return W, H, kl_divergence(data, W @ H)


def compute_simplex_beta_nmf(data, W_0, H_0, rank, beta, n_iter_max=100, tol=1e-8, tol_update_lagrangian=1e-6, verbose=False,
                             infos=None, round32=False):
    """simplex_nmf.py:32-65.  Returns (W, H, costs, toc); toc is a list of zeros (no clock here)."""
    W, H = W_0.copy(), H_0.copy()
    costs = []
    for iteration in range(n_iter_max):
        info = {}
        W, H, cost = one_step_simplex_beta_nmf(data, W, H, rank, beta, tol_update_lagrangian, info=info, round32=round32)
        if infos is not None:
            infos.append(info)
        costs.append(cost)
        if iteration > 0 and abs(costs[-2] - costs[-1]) < tol:
            break
    return W, H, costs, [0.0] * len(costs)

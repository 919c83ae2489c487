"""fp64 restatement of NMF and NTF with MISSING entries (unstored="missing": nn_fac_amd/sparse_nmf.py, sparse_ntf.py,
nn_fac_amd/csrc/k_sparse_obs.hip): the multiplicative update of any beta >= 0 with every sum cut down to the STORED entries.

A matrix or tensor is a `sptensor_restatement.Coo` (coordinates, values, shape; a matrix is the order-2 case: `from_csr`); every
function walks that list and forms nothing of the data's dense size.  Factors are the reference's, one dim x r matrix per mode
(a matrix: `nmf_factors(U, V)` = [U, V^T]).  Per stored entry e with value x_e, h_e the Hadamard product of the OTHER modes'
factor rows at e and p_e the model at e,

    num[i, k] = sum_{e in slice i} x_e p_e^(beta - 2) h_e[k]        den[i, k] = sum_{e in slice i} p_e^(beta - 1) h_e[k]
    F <- max(F (num / den)^gamma(beta), 1e-12)                      cost = sum_e d_beta(x_e | p_e)

A stored 0 is an observed zero: nothing to num, its term to den, d_beta(0 | p) to the cost (p at beta = 1, +inf at beta = 0,
p^beta / beta otherwise).  A slice without a stored entry keeps its value (0 / 0 otherwise).
tests/test_observed_restatement.py pins this to oracle/nnfac_oracle.py where every entry is stored, and to a dense formula with a
0/1 weight array elsewhere; the GPU tests compare the device against it.
"""
import numpy as np
import scipy.sparse as sp

import nnfac_oracle as orc
from sptensor_restatement import Coo, hadamard_rows, model_at_stored      # noqa: F401


def from_csr(X):
    """The Coo of a scipy.sparse matrix, stored zeros included."""
    X = sp.csr_matrix(X)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    return Coo(np.column_stack([rows, X.indices.astype(np.int64)]), X.data.astype(np.float64), X.shape)


def from_dense(D, mask):
    """The Coo that stores exactly the entries of D where `mask` is set, zeros included."""
    mask = np.asarray(mask, dtype=bool)
    return Coo(np.argwhere(mask), np.asarray(D, dtype=np.float64)[mask], D.shape)


def nmf_factors(U, V):
    return [np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64).T]


def weights(beta, x, p):
    """(x p^(beta - 2), p^(beta - 1)) per stored entry; the first is 0 at a stored 0 whatever p is."""
    with np.errstate(divide="ignore", invalid="ignore"):
        wn = x * p ** (beta - 2.0)
    wn = np.where(x == 0, 0.0, wn)
    return wn, p ** (beta - 1.0)


def sums(X, factors, mode, beta):
    """(num, den) of `mode`, dim x r each; a slice without stored entries has 0 in both."""
    x, p = X.vals, model_at_stored(X, factors)
    h = hadamard_rows(X, factors, skip=mode)
    wn, wd = weights(beta, x, p)
    num = np.zeros((X.shape[mode], factors[0].shape[1]))
    den = np.zeros_like(num)
    np.add.at(num, X.coords[:, mode], wn[:, None] * h)
    np.add.at(den, X.coords[:, mode], wd[:, None] * h)
    return num, den


def terms(beta, x, p):
    """d_beta(x | p) per stored entry (beta_divergence.py:45-52 entry by entry)."""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if beta == 1:
            q = np.where(x == 0, 1.0, x / p)
            return x * np.log(q) - x + p
        if beta == 0:
            q = x / p
            return q - np.log(q) - 1.0      # (x = 0: +inf)
        return (x ** beta + (beta - 1.0) * p ** beta - beta * x * p ** (beta - 1.0)) / (beta * (beta - 1.0))


def cost(X, factors, beta):
    return float(np.sum(terms(beta, X.vals, model_at_stored(X, factors))))


def update_mode(X, factors, mode, beta):
    """mu_betadivmin (mu.py:82-97) of `mode` over the stored entries; slices without one keep their value exactly."""
    num, den = sums(X, factors, mode, beta)
    seen = np.bincount(X.coords[:, mode], minlength=X.shape[mode]) > 0
    F = factors[mode].copy()
    F[seen] = np.maximum(F[seen] * (num[seen] / den[seen]) ** orc.gamma_beta(beta), orc.EPS_MU)
    return F


def one_step(X, in_factors, beta, fixed_modes=(), normalized=None):
    """Every mode not fixed in turn, then the cost -- divided by sum x^2 for tensors (`normalized`, default: order >= 3), as the
    NTF driver does (ntf.py:475)."""
    factors = [np.array(F, dtype=np.float64) for F in in_factors]
    for mode in [m for m in range(len(factors)) if m not in fixed_modes]:
        factors[mode] = update_mode(X, factors, mode, beta)
    c = cost(X, factors, beta)
    if len(factors) >= 3 if normalized is None else normalized:
        c /= float(X.vals @ X.vals)
    return factors, c


def run(X, factors0, n_iter, beta, fixed_modes=(), tol=0.0, normalized=None):
    """compute_nmf / compute_ntf with unstored="missing": (factors, costs)."""
    factors, costs = [np.array(F, dtype=np.float64) for F in factors0], []
    for it in range(n_iter):
        factors, c = one_step(X, factors, beta, fixed_modes, normalized)
        costs.append(c)
        if it > 0 and abs(costs[-2] - costs[-1]) < tol:
            break
    return factors, costs


def heldout_error(D, mask, factors):
    """||(D - model) off the mask|| / ||D off the mask||: what a missing-data fit is for."""
    letters = "abcdefgh"[:len(factors)]
    P = np.einsum(",".join(l + "z" for l in letters) + "->" + letters, *factors)
    off = ~np.asarray(mask, dtype=bool)
    return float(np.linalg.norm((D - P)[off]) / np.linalg.norm(D[off]))

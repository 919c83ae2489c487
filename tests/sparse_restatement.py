"""fp64 restatement of NMF on sparse data over the STORED entries only (nn_fac_amd/sparse_nmf.py, nn_fac_amd/csrc/k_sparse.hip).

Every function takes a scipy.sparse CSR matrix and walks its (row, column, value) triples; none forms anything of size m x n.
tests/test_sparse_restatement.py pins each of them to oracle/nnfac_oracle.py on the densified matrix; the GPU tests
(test_gpu_sparse_kernels.py, test_gpu_sparse_nmf.py) compare the device against them.  Factors are the reference's: U m x r,
V r x n.  The HALS solve and the MU clip never look at the data and are the oracle's own (hals_nnls_acc, EPS_MU).
"""
import math

import numpy as np
import scipy.sparse as sp

import nnfac_oracle as orc


def triples(X):
    """(rows, cols, vals) of every stored entry, row-major; stored zeros included."""
    X = sp.csr_matrix(X)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    return rows, X.indices.astype(np.int64), X.data.astype(np.float64)


def sample(m, n, density, seed, empty_row=None, empty_col=None, stored_zeros=0):
    """m x n CSR with about `density` of its entries stored, values in (0.1, 1.1); one row / column emptied on request and
    `stored_zeros` of the stored values set to an explicit 0."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    if empty_row is not None:
        mask[empty_row, :] = False
    if empty_col is not None:
        mask[:, empty_col] = False
    rows, cols = np.nonzero(mask)
    vals = rng.random(rows.size) + 0.1
    if stored_zeros:
        vals[rng.choice(rows.size, size=stored_zeros, replace=False)] = 0.0
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, n))


def from_row_lengths(lens, n, seed, stored_zeros=0):
    """A CSR matrix whose row i stores lens[i] entries at sorted random columns of n."""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lens] + [np.zeros(0, np.int64)])
    vals = rng.random(indices.size) + 0.1
    if stored_zeros:
        vals[rng.choice(indices.size, size=stored_zeros, replace=False)] = 0.0
    return sp.csr_matrix((vals, indices.astype(np.int32), indptr), shape=(len(lens), n))


# ---- the sums over stored entries ------------------------------------------------------------------------------------------
def cross_vxt(X, V):
    """V X^T (r x m): out[k, i] = sum_{(i, j) stored} x_ij V[k, j]."""
    rows, cols, vals = triples(X)
    out = np.zeros((X.shape[0], V.shape[0]))
    np.add.at(out, rows, vals[:, None] * V.T[cols])
    return out.T


def cross_utx(X, U):
    """U^T X (r x n): out[k, j] = sum_{(i, j) stored} x_ij U[i, k]."""
    rows, cols, vals = triples(X)
    out = np.zeros((X.shape[1], U.shape[1]))
    np.add.at(out, cols, vals[:, None] * U[rows])
    return out.T


def model_at_stored(X, U, V):
    rows, cols, _ = triples(X)
    return np.einsum("pk,pk->p", U[rows], V.T[cols])


def _ratio(vals, p):
    """x / p per stored entry; a stored 0 gives 0 (it adds nothing to the KL sums, whatever p is)."""
    q = np.zeros_like(vals)
    nz = vals != 0
    q[nz] = vals[nz] / p[nz]
    return q


def kl_num_u(X, U, V):
    """The beta = 1 numerator of the U update, ((X ./ (U V)) V^T)^T as r x m, over the stored entries."""
    rows, cols, vals = triples(X)
    q = _ratio(vals, model_at_stored(X, U, V))
    out = np.zeros((X.shape[0], V.shape[0]))
    np.add.at(out, rows, q[:, None] * V.T[cols])
    return out.T


def kl_num_v(X, U, V):
    """The beta = 1 numerator of the V update, U^T (X ./ (U V)) (r x n), over the stored entries."""
    rows, cols, vals = triples(X)
    q = _ratio(vals, model_at_stored(X, U, V))
    out = np.zeros((X.shape[1], U.shape[1]))
    np.add.at(out, cols, q[:, None] * U[rows])
    return out.T


def kl_stored_sum(X, U, V):
    """sum over stored x != 0 of x log(x / p) - x  (what nnf_csr_kl_f32 returns as its cost)."""
    _, _, vals = triples(X)
    p = model_at_stored(X, U, V)
    nz = vals != 0
    return float(np.sum(vals[nz] * np.log(vals[nz] / p[nz]) - vals[nz]))


def kl_cost(X, U, V):
    """beta_divergence(X, U V, 1) with 0 log 0 = 0: the stored sum + sum(U V) = colsum(U) . rowsum(V)."""
    return kl_stored_sum(X, U, V) + float(U.sum(axis=0) @ V.sum(axis=1))


def frob_cost(X, U, V, sparsity_coefficients=(None, None)):
    """||X - U V||_F^2 through ||X||^2 - 2 <U^T X, V> + <U^T U, V V^T>, + the sparsity terms of nmf.py:452."""
    _, _, vals = triples(X)
    s = [0 if c is None else c for c in sparsity_coefficients]
    return float(vals @ vals - 2.0 * np.sum(cross_utx(X, U) * V) + np.sum((U.T @ U) * (V @ V.T))
                 + 2 * (s[0] * np.linalg.norm(U, ord=1) + s[1] * np.linalg.norm(V, ord=1)))


# ---- one step and the loop (nmf.py:387-458, :284-329) ------------------------------------------------------------------------
def one_step(X, U_in, V_in, update_rule, beta, sparsity_coefficients=(None, None), fixed_modes=(), normalize=(False, False),
             sweeps=None):
    """Deterministic step (alpha = inf): U then V, then the cost."""
    U, V = U_in.copy(), V_in.copy()
    if 0 not in fixed_modes:
        if update_rule == "hals":
            out = orc.hals_nnls_acc(cross_vxt(X, V), V @ V.T, U_in.T.copy(), maxiter=100, atime=None, alpha=math.inf, delta=0.01,
                                    sparsity_coefficient=sparsity_coefficients[0], normalize=normalize[0], nonzero=False)
            U = out[0].T
            if sweeps is not None:
                sweeps.append(out[2] - 1)
        elif beta == 1:
            U = np.maximum(U * (kl_num_u(X, U, V).T / V.sum(axis=1)[None, :]), orc.EPS_MU)
        else:
            U = np.maximum(U * (cross_vxt(X, V).T / (U @ (V @ V.T))), orc.EPS_MU)
    if 1 not in fixed_modes:
        if update_rule == "hals":
            out = orc.hals_nnls_acc(cross_utx(X, U), U.T @ U, V_in, maxiter=100, atime=None, alpha=math.inf, delta=0.01,
                                    sparsity_coefficient=sparsity_coefficients[1], normalize=normalize[1], nonzero=False)
            V = out[0]
            if sweeps is not None:
                sweeps.append(out[2] - 1)
        elif beta == 1:
            V = np.maximum(V * (kl_num_v(X, U, V) / U.sum(axis=0)[:, None]), orc.EPS_MU)
        else:
            V = np.maximum(V * (cross_utx(X, U) / ((U.T @ U) @ V)), orc.EPS_MU)
    if update_rule == "mu" and beta == 1:
        cost = kl_cost(X, U, V)
    elif update_rule == "mu":
        cost = 0.5 * frob_cost(X, U, V)      # beta_divergence(., ., 2) = ||.||^2 / 2 (nmf.py:455)
    else:
        cost = frob_cost(X, U, V, sparsity_coefficients)
    return U, V, cost


def run(X, U0, V0, n_iter, update_rule, beta=2, sparsity_coefficients=(None, None), fixed_modes=(), normalize=(False, False),
        tol=0.0, sweeps=None):
    """compute_nmf: (U, V, costs)."""
    U, V, costs = np.array(U0, dtype=np.float64), np.array(V0, dtype=np.float64), []
    for it in range(n_iter):
        U, V, c = one_step(X, U, V, update_rule, beta, sparsity_coefficients, fixed_modes, normalize, sweeps=sweeps)
        costs.append(c)
        if it > 0 and abs(costs[-2] - costs[-1]) < tol:
            break
    return U, V, costs

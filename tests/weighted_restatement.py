"""fp64 restatement of weighted NMF (nn_fac_amd/weighted_nmf.py, the weighted forms of nn_fac_amd/csrc/k_mu.hip and k_cost.hip):
the multiplicative update of any beta >= 0 on dense data with a weight per entry.

With Wg an m x n array of finite weights >= 0, P = U V and gamma(beta) as in mu_betadivmin (mu.py:82-97),

    left :  num[i, k] = sum_j Wg[i, j] X[i, j] P[i, j]^(beta - 2) V[k, j]     den[i, k] = sum_j Wg[i, j] P[i, j]^(beta - 1) V[k, j]
    right:  num[k, j] = sum_i Wg[i, j] X[i, j] P[i, j]^(beta - 2) U[i, k]     den[k, j] = sum_i Wg[i, j] P[i, j]^(beta - 1) U[i, k]
    F <- max(F (num / den)^gamma(beta), 1e-12)                                 cost = sum_ij Wg[i, j] d_beta(X[i, j] | P[i, j])

Where Wg[i, j] == 0 the entry adds exactly 0 to num, den and the cost WHATEVER X[i, j] holds (NaN, +-Inf): a select, not a
product.  Under a positive weight x = 0 is an observed zero: nothing to num, its term to den, d_beta(0 | p) to the cost (p at
beta = 1, +inf at beta = 0, p^beta / beta otherwise).  A row of U (a column of V) whose weights are all zero keeps its value.
Factors are the reference's: U is m x r, V is r x n.  tests/test_weighted_restatement.py pins this to oracle/nnfac_oracle.py at
all-ones weights and to tests/observed_restatement.py at 0/1 weights; the GPU tests compare the device against it.
"""
import numpy as np

import nnfac_oracle as orc


def _parts(X, Wg, U, V, beta):
    """(Wg x P^(beta - 2), Wg P^(beta - 1)) entry by entry, exactly 0 where Wg == 0; the first is 0 at an observed zero too."""
    X, Wg = np.asarray(X, np.float64), np.asarray(Wg, np.float64)
    on = Wg != 0
    P = np.asarray(U, np.float64) @ np.asarray(V, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = np.where(on & (X != 0), Wg * X * P ** (beta - 2.0), 0.0)
        b = np.where(on, Wg * P ** (beta - 1.0), 0.0)
    return a, b


def sums(X, Wg, U, V, beta, side):
    """(num, den) of the 'left' (m x r) or the 'right' (r x n) update."""
    a, b = _parts(X, Wg, U, V, beta)
    if side == "left":
        Vt = np.asarray(V, np.float64).T
        return a @ Vt, b @ Vt
    Ut = np.asarray(U, np.float64).T
    return Ut @ a, Ut @ b


def update(X, Wg, U, V, beta, side):
    """The updated U ('left') or V ('right'); a slice whose weights are all zero keeps its value exactly."""
    num, den = sums(X, Wg, U, V, beta, side)
    on = np.asarray(Wg) != 0
    if side == "left":
        F, seen = np.array(U, dtype=np.float64), on.any(axis=1)
        F[seen] = np.maximum(F[seen] * (num[seen] / den[seen]) ** orc.gamma_beta(beta), orc.EPS_MU)
    else:
        F, seen = np.array(V, dtype=np.float64), on.any(axis=0)
        F[:, seen] = np.maximum(F[:, seen] * (num[:, seen] / den[:, seen]) ** orc.gamma_beta(beta), orc.EPS_MU)
    return F


def terms(beta, x, p):
    """d_beta(x | p) entry by entry (beta_divergence.py:45-52), 1/2 (x - p)^2 at beta = 2."""
    x, p = np.asarray(x, np.float64), np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if beta == 1:
            q = np.where(x == 0, 1.0, x / p)
            return x * np.log(q) - x + p
        if beta == 0:
            q = x / p
            return q - np.log(q) - 1.0      # (x = 0: +inf)
        return (x ** beta + (beta - 1.0) * p ** beta - beta * x * p ** (beta - 1.0)) / (beta * (beta - 1.0))


def cost(X, Wg, U, V, beta):
    Wg = np.asarray(Wg, np.float64)
    P = np.asarray(U, np.float64) @ np.asarray(V, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.where(Wg != 0, Wg * terms(beta, X, P), 0.0)
    return float(t.sum())


def one_step(X, Wg, U, V, beta, fixed_modes=()):
    """U, then V, then the cost: (U, V, cost)."""
    U, V = np.array(U, dtype=np.float64), np.array(V, dtype=np.float64)
    if 0 not in fixed_modes:
        U = update(X, Wg, U, V, beta, "left")
    if 1 not in fixed_modes:
        V = update(X, Wg, U, V, beta, "right")
    return U, V, cost(X, Wg, U, V, beta)


def run(X, Wg, U0, V0, n_iter, beta, fixed_modes=(), tol=0.0):
    """compute_nmf with weights: (U, V, costs)."""
    U, V, costs = np.array(U0, dtype=np.float64), np.array(V0, dtype=np.float64), []
    for it in range(n_iter):
        U, V, c = one_step(X, Wg, U, V, beta, fixed_modes)
        costs.append(c)
        if it > 0 and abs(costs[-2] - costs[-1]) < tol:
            break
    return U, V, costs


def recovery_case(beta):
    """The recovery recipe: a rank-3 truth T, noise of two very different levels, weights = 1 / variance (scaled to a maximum of
    one): (T, X, Wg, U0, V0).  The generator is restarted per beta, the draws come in this order."""
    rng = np.random.default_rng(0)
    A = rng.random((60, 3)) + 0.1
    B = rng.random((3, 50)) + 0.1
    T = A @ B
    sig = np.where(rng.random((60, 50)) < 0.5, 0.5, 0.01)
    if beta == 2:
        X = np.abs(T + sig * rng.standard_normal((60, 50)))
    else:
        X = T * np.exp(sig * rng.standard_normal((60, 50)))
    Wg = sig ** -2 / (sig ** -2).max()
    U0 = rng.random((60, 3))
    V0 = rng.random((3, 50))
    return T, X, Wg, U0, V0


def recovery_error(T, U, V):
    return float(np.linalg.norm(np.asarray(U, np.float64) @ np.asarray(V, np.float64) - T) / np.linalg.norm(T))

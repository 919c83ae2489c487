"""fp64 restatement of weighted NTF (nn_fac_amd/weighted_ntf.py, nnf_mu_mode_w_f32 in nn_fac_amd/csrc/k_mu_mode.hip): the
multiplicative update of any beta >= 0 on a dense tensor of any order with a weight per entry.  TEST INFRASTRUCTURE: NumPy only.

With Wg an array of the tensor's shape holding finite weights >= 0, P the CP model of the factors (one dim x r matrix per mode),
h_e the Hadamard product of the OTHER modes' factor rows at entry e and gamma(beta) as in mu_betadivmin (mu.py:82-97),

    num[i, k] = sum_{e in slice i} Wg[e] T[e] P[e]^(beta - 2) h_e[k]      den[i, k] = sum_{e in slice i} Wg[e] P[e]^(beta - 1) h_e[k]
    F <- max(F (num / den)^gamma(beta), 1e-12)                            cost = sum_e Wg[e] d_beta(T[e] | P[e])

Where Wg[e] == 0 the entry adds exactly 0 to num, den and the cost WHATEVER T[e] holds (NaN, +-Inf): a select, not a product.
Under a positive weight t = 0 is an observed zero: nothing to num, its term to den, d_beta(0 | p) to the cost.  A slice whose
weights are all zero keeps its value.  `run` (compute_ntf) divides the cost by sum Wg T^2 over the entries of positive weight,
`one_step` by the caller's norm_tensor^2 (ntf.py:475).  tests/test_weighted_ntf_restatement.py pins this to
oracle/nnfac_oracle.py at all-ones weights, to tests/observed_restatement.py at 0/1 weights and to tests/weighted_restatement.py
at order 3 with one extent 1; the GPU tests compare the device against it.
"""
import numpy as np

import nnfac_oracle as orc
from weighted_restatement import terms

_LETTERS = "abcdefgh"


def model(factors):
    """The CP model of the factors as a dense tensor."""
    letters = _LETTERS[:len(factors)]
    return np.einsum(",".join(c + "z" for c in letters) + "->" + letters, *[np.asarray(F, np.float64) for F in factors])


def _parts(T, Wg, factors, beta):
    """(Wg T P^(beta - 2), Wg P^(beta - 1)) entry by entry, exactly 0 where Wg == 0; the first is 0 at an observed zero too."""
    T, Wg = np.asarray(T, np.float64), np.asarray(Wg, np.float64)
    on, P = Wg != 0, model(factors)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = np.where(on & (T != 0), Wg * T * P ** (beta - 2.0), 0.0)
        b = np.where(on, Wg * P ** (beta - 1.0), 0.0)
    return a, b


def sums(T, Wg, factors, mode, beta):
    """(num, den) of `mode`, dim x r each; a slice whose weights are all zero has 0 in both."""
    a, b = _parts(T, Wg, factors, beta)
    letters = _LETTERS[:len(factors)]
    spec = letters + "," + ",".join(c + "z" for i, c in enumerate(letters) if i != mode) + "->" + letters[mode] + "z"
    others = [np.asarray(F, np.float64) for i, F in enumerate(factors) if i != mode]
    return np.einsum(spec, a, *others), np.einsum(spec, b, *others)


def update_mode(T, Wg, factors, mode, beta):
    """mu_betadivmin (mu.py:82-97) of `mode` under the weights; slices whose weights are all zero keep their value exactly."""
    num, den = sums(T, Wg, factors, mode, beta)
    seen = np.moveaxis(np.asarray(Wg) != 0, mode, 0).reshape(num.shape[0], -1).any(axis=1)
    F = np.array(factors[mode], dtype=np.float64)
    F[seen] = np.maximum(F[seen] * (num[seen] / den[seen]) ** orc.gamma_beta(beta), orc.EPS_MU)
    return F


def cost(T, Wg, factors, beta):
    """sum Wg d_beta(T | model), not normalised."""
    Wg = np.asarray(Wg, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.where(Wg != 0, Wg * terms(beta, T, model(factors)), 0.0)
    return float(t.sum())


def weighted_norm2(T, Wg):
    """sum Wg T^2 over the entries of positive weight (the data under zero weights read as 0)."""
    Wg = np.asarray(Wg, np.float64)
    return float(np.sum(Wg * np.where(Wg > 0, np.asarray(T, np.float64), 0.0) ** 2))


def one_step(T, Wg, in_factors, beta, norm_tensor, fixed_modes=(), sparsity_coefficients=None):
    """Every mode not fixed in turn, then (cost + sparsity terms) / norm_tensor^2 (ntf.py:472-475): (factors, cost)."""
    factors = [np.array(F, dtype=np.float64) for F in in_factors]
    for mode in [m for m in range(len(factors)) if m not in fixed_modes]:
        factors[mode] = update_mode(T, Wg, factors, mode, beta)
    c = cost(T, Wg, factors, beta)
    for idx, s in enumerate(sparsity_coefficients or []):
        if s and idx not in fixed_modes:
            c += 2 * s * np.linalg.norm(factors[idx], ord=1)
    return factors, c / norm_tensor ** 2


def run(T, Wg, factors0, n_iter, beta, fixed_modes=(), tol=0.0, sparsity_coefficients=None):
    """compute_ntf with weights: (factors, costs), the costs divided by sum Wg T^2."""
    factors, costs = [np.array(F, dtype=np.float64) for F in factors0], []
    norm = np.sqrt(weighted_norm2(T, Wg))
    for it in range(n_iter):
        factors, c = one_step(T, Wg, factors, beta, norm, fixed_modes, sparsity_coefficients)
        costs.append(c)
        if it > 0 and abs(costs[-2] - costs[-1]) < tol:
            break
    return factors, costs


def recovery_case():
    """The recovery recipe: an exactly rank-3 20 x 25 x 30 truth, noise of sigma = 0.5 or 0.01 at random per entry, weights =
    sigma^-2: (truth, T, Wg, factors0).  The draws come in this order."""
    rng = np.random.default_rng(0)
    gen = [rng.random((s, 3)) + 0.1 for s in (20, 25, 30)]
    truth = model(gen)
    sig = np.where(rng.random(truth.shape) < 0.5, 0.5, 0.01)
    T = np.abs(truth + sig * rng.standard_normal(truth.shape))
    F0 = [rng.random((s, 3)) for s in (20, 25, 30)]
    return truth, T, sig ** -2, F0


def recovery_error(truth, factors):
    return float(np.linalg.norm(model(factors) - truth) / np.linalg.norm(truth))

"""tests/sparse_restatement.py (the sums of NMF over the stored entries of a CSR matrix) against oracle/nnfac_oracle.py on the
densified matrix, at the 1e-12 of tests/test_oracle_golden.py.

The matrix: 300 x 200, rank 10, seed 0, about 16 % stored, row 7 and column 11 empty.  One caution on the KL COST: the oracle's
beta_divergence evaluates `np.log(q, where=(q != 0))` without an `out=`, i.e. it reads uninitialised memory wherever the data is
0.  It is therefore pinned to the oracle only on a matrix whose entries are all stored and positive; with zeros in the data it is
pinned to the dense formula written out below with 0 log 0 = 0."""
import numpy as np
import pytest

import nnfac_oracle as orc
import sparse_restatement as rs

RTOL = 1e-12
M, N, R = 300, 200, 10


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def case():
    X = rs.sample(M, N, 0.16, seed=0, empty_row=7, empty_col=11, stored_zeros=5)
    rng = np.random.default_rng(1)
    U, V = rng.random((M, R)) + 0.05, rng.random((R, N)) + 0.05
    D = X.toarray()
    assert not D[7].any() and not D[:, 11].any() and 0.14 < X.nnz / (M * N) < 0.18
    return X, D, U, V


def dense_kl(D, P):
    """beta_divergence(D, P, 1) with 0 log 0 = 0, entry by entry."""
    t = np.zeros_like(D)
    nz = D != 0
    t[nz] = D[nz] * np.log(D[nz] / P[nz])
    return float(np.sum(t - D + P))


def test_cross_products(case):
    X, D, U, V = case
    assert close(rs.cross_vxt(X, V), V @ D.T)
    assert close(rs.cross_utx(X, U), U.T @ D)


def test_kl_numerators(case):
    X, D, U, V = case
    P = U @ V
    assert close(rs.kl_num_u(X, U, V), ((D / P) @ V.T).T)
    assert close(rs.kl_num_v(X, U, V), U.T @ (D / P))
    # and through the oracle's own update
    assert close(np.maximum(U * (rs.kl_num_u(X, U, V).T / V.sum(axis=1)[None, :]), orc.EPS_MU), orc.mu_betadivmin(U, V, D, 1))


def test_kl_cost_with_zeros_against_the_dense_formula(case):
    X, D, U, V = case
    want = dense_kl(D, U @ V)
    assert abs(rs.kl_cost(X, U, V) - want) <= RTOL * abs(want)


def test_kl_cost_against_the_oracle_where_every_entry_is_stored():
    rng = np.random.default_rng(2)
    D = rng.random((40, 30)) + 0.1
    U, V = rng.random((40, 5)) + 0.05, rng.random((5, 30)) + 0.05
    import scipy.sparse as sp
    want = orc.beta_divergence(D, U @ V, 1)
    assert abs(rs.kl_cost(sp.csr_matrix(D), U, V) - want) <= RTOL * abs(want)


def test_frobenius_identity_cost(case):
    X, D, U, V = case
    want = np.linalg.norm(D - U @ V, ord="fro") ** 2
    assert abs(rs.frob_cost(X, U, V) - want) <= RTOL * want
    sp_c = (0.3, 0.2)
    want += 2 * (0.3 * np.linalg.norm(U, ord=1) + 0.2 * np.linalg.norm(V, ord=1))
    assert abs(rs.frob_cost(X, U, V, sp_c) - want) <= RTOL * want


@pytest.mark.parametrize("rule,beta", [("hals", 2), ("mu", 1), ("mu", 2)])
def test_one_step_against_the_oracle(case, rule, beta):
    X, D, U, V = case
    U1, V1, c1 = rs.one_step(X, U, V, rule, beta)
    Uo, Vo, co = orc.one_nmf_step(D, R, U, V, np.linalg.norm(D), rule, beta, [None, None], [], [False, False], True)
    assert close(U1, Uo) and close(V1, Vo)
    if (rule, beta) == ("mu", 1):
        co = dense_kl(D, Uo @ Vo)       # (zeros in the data: see the head of this file)
    assert abs(c1 - co) <= RTOL * abs(co)


@pytest.mark.parametrize("rule,beta", [("hals", 2), ("mu", 1)])
def test_six_iterations_against_the_oracle(case, rule, beta):
    X, D, _, _ = case
    _, U0, V0 = orc.synth_nmf(M, N, R, seed=0, dtype=np.float64)
    sw, swo = [], []
    U1, V1, costs = rs.run(X, U0, V0, 6, rule, beta, sweeps=sw)
    Uo, Vo, co, _ = orc.nmf(D, R, init="custom", U_0=U0, V_0=V0, n_iter_max=6, tol=0, update_rule=rule, beta=beta,
                            return_costs=True, deterministic=True, sweeps=swo)
    assert sw == swo and len(costs) == 6
    assert np.isfinite(Uo).all() and np.isfinite(Vo).all()
    assert close(U1, Uo) and close(V1, Vo)
    if rule == "hals":
        assert np.allclose(costs, co, rtol=RTOL, atol=0)
    else:
        assert abs(costs[-1] - dense_kl(D, Uo @ Vo)) <= RTOL * abs(costs[-1])


@pytest.mark.parametrize("kw", [dict(sparsity_coefficients=(0.05, 0.02)), dict(normalize=(True, False)), dict(fixed_modes=(0,))],
                         ids=["sparsity", "normalize", "fixed0"])
def test_hals_options_against_the_oracle(case, kw):
    X, D, U, V = case
    U1, V1, c1 = rs.one_step(X, U, V, "hals", 2, **kw)
    Uo, Vo, co = orc.one_nmf_step(D, R, U, V, np.linalg.norm(D), "hals", 2, list(kw.get("sparsity_coefficients", (None, None))),
                                  list(kw.get("fixed_modes", ())), list(kw.get("normalize", (False, False))), True)
    assert close(U1, Uo) and close(V1, Vo) and abs(c1 - co) <= RTOL * abs(co)

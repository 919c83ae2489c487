"""tests/sptensor_restatement.py (the sums of NTF over the stored entries of a sparse tensor) against oracle/nnfac_oracle.py on the
densified tensor, at the 1e-12 of tests/test_oracle_golden.py.

Tensors: 40 x 33 x 27 at rank 6, 12 x 9 x 10 x 8 at rank 5 and 7 x 6 x 5 x 4 x 3 at rank 3, about 10 % stored, one empty slice in
each of the first three modes.  The KL COST with zeros in the data is pinned to the dense formula with 0 log 0 = 0 (the oracle's
beta_divergence reads uninitialised memory there: the head of tests/test_sparse_restatement.py) and to the oracle itself on a small
tensor with every entry stored."""
import math

import numpy as np
import pytest

import nnfac_oracle as orc
import sptensor_restatement as rs

RTOL = 1e-12
CASES = {"40x33x27": ((40, 33, 27), 6), "12x9x10x8": ((12, 9, 10, 8), 5), "7x6x5x4x3": ((7, 6, 5, 4, 3), 3)}
EMPTY = [(0, 3), (1, 2), (2, 1)]


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(b), 1e-300)


_cases = {}


def case(name):
    if name not in _cases:
        shape, r = CASES[name]
        X = rs.sample(shape, 0.1, seed=len(shape), empty=EMPTY, stored_zeros=3)
        rng = np.random.default_rng(1)
        factors = [rng.random((d, r)) + 0.05 for d in shape]
        D = X.dense()
        for mode, index in EMPTY:
            assert not np.take(D, index, axis=mode).any()
        assert 0.05 < X.nnz / D.size < 0.13      # (the emptied slices of the small tensor take a third of its entries)
        _cases[name] = (X, D, factors, r)
    return _cases[name]


def dense_kl(D, P):
    """beta_divergence(D, P, 1) with 0 log 0 = 0, entry by entry."""
    t = np.zeros_like(D)
    nz = D != 0
    t[nz] = D[nz] * np.log(D[nz] / P[nz])
    return float(np.sum(t - D + P))


def model(factors):
    return orc.fold(factors[0] @ orc.khatri_rao(factors, skip_matrix=0).T, 0, [F.shape[0] for F in factors])


def unfoldings(D):
    return [orc.unfold(D, m) for m in range(D.ndim)]


@pytest.mark.parametrize("name", list(CASES))
def test_mttkrp_and_the_model_at_the_stored_entries(name):
    X, D, factors, r = case(name)
    for mode in range(D.ndim):
        assert close(rs.mttkrp(X, factors, mode), orc.unfold(D, mode) @ orc.khatri_rao(factors, skip_matrix=mode)), mode
        assert list(X.slice_lengths(mode)) == list((orc.unfold(D, mode) != 0).sum(axis=1) +
                                                   np.bincount(X.coords[X.vals == 0][:, mode], minlength=X.shape[mode])), mode
    assert close(rs.model_at_stored(X, factors), model(factors)[tuple(X.coords.T)])


@pytest.mark.parametrize("name", list(CASES))
def test_kl_numerator_and_cost_with_zeros_against_the_dense_formula(name):
    X, D, factors, r = case(name)
    P = model(factors)
    for mode in range(D.ndim):
        krao = orc.khatri_rao(factors, skip_matrix=mode)
        assert close(rs.kl_num(X, factors, mode), (orc.unfold(D, mode) / orc.unfold(P, mode)) @ krao), mode
        # and through the oracle's own update
        den = np.prod([F.sum(axis=0) for m, F in enumerate(factors) if m != mode], axis=0)
        assert close(np.maximum(factors[mode] * (rs.kl_num(X, factors, mode) / den[None, :]), orc.EPS_MU),
                     orc.mu_betadivmin(factors[mode], krao.T, orc.unfold(D, mode), 1)), mode
    want = dense_kl(D, P)
    assert abs(rs.kl_cost(X, factors) - want) <= RTOL * abs(want)


def test_kl_cost_against_the_oracle_where_every_entry_is_stored():
    rng = np.random.default_rng(2)
    D = rng.random((6, 5, 4)) + 0.1
    factors = [rng.random((d, 3)) + 0.05 for d in D.shape]
    X = rs.Coo(np.argwhere(np.ones_like(D, dtype=bool)), D.reshape(-1), D.shape)
    want = orc.beta_divergence(orc.unfold(D, 2), factors[2] @ orc.khatri_rao(factors, skip_matrix=2).T, 1)
    assert abs(rs.kl_cost(X, factors) - want) <= RTOL * abs(want)


@pytest.mark.parametrize("name", list(CASES))
def test_frobenius_identity_cost(name):
    X, D, factors, r = case(name)
    want = np.sum((D - model(factors)) ** 2)
    for mode in range(D.ndim):
        assert abs(rs.frob_cost(X, factors, mode) - want) <= RTOL * want, mode


def oracle_step(D, r, factors, rule, beta, sparsity=None, fixed=(), normalize=None, sweeps=None):
    N = D.ndim
    return orc.one_ntf_step(unfoldings(D), r, [F.copy() for F in factors], np.linalg.norm(D), rule, beta,
                            [None] * N if sparsity is None else list(sparsity), list(fixed),
                            [False] * N if normalize is None else list(normalize), alpha=math.inf, sweeps=sweeps)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("rule,beta", [("hals", 2), ("mu", 2), ("mu", 1)])
def test_one_step_against_the_oracle(name, rule, beta):
    X, D, factors, r = case(name)
    sw, swo = [], []
    got, c = rs.one_step(X, factors, rule, beta, sweeps=sw)
    want, co = oracle_step(D, r, factors, rule, beta, sweeps=swo)
    assert sw == swo
    for a, b in zip(got, want):
        assert close(a, b)
    if (rule, beta) == ("mu", 1):
        co = dense_kl(D, model(want)) / np.sum(D ** 2)       # (zeros in the data: see the head of this file)
    assert abs(c - co) <= RTOL * abs(co)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("rule,beta", [("hals", 2), ("mu", 2), ("mu", 1)])
def test_five_iterations_against_the_oracle(name, rule, beta):
    X, D, _, r = case(name)
    rng = np.random.default_rng(7)
    start = [rng.random((d, r)) for d in D.shape]
    sw, swo = [], []
    got, costs = rs.run(X, start, 5, rule, beta, sweeps=sw)
    want, co, _ = orc.compute_ntf(D, r, [F.copy() for F in start], n_iter_max=5, tol=0, update_rule=rule, beta=beta,
                                  return_costs=True, alpha=math.inf, sweeps=swo)
    assert sw == swo and len(costs) == 5 and (rule != "hals" or len(sw) == 5 * D.ndim)
    assert all(np.isfinite(F).all() for F in want)
    for a, b in zip(got, want):
        assert close(a, b)
    if (rule, beta) == ("mu", 1):
        assert abs(costs[-1] - dense_kl(D, model(want)) / np.sum(D ** 2)) <= RTOL * abs(costs[-1])
    else:
        assert np.allclose(costs, co, rtol=RTOL, atol=0)
    if rule == "hals":
        assert 0.5 < costs[-1] < 1.0      # far from the cancellation regime of the identity


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kw", [dict(sparsity=(0.05, 0.02, 0.01)), dict(normalize=(True, False, False)), dict(fixed=(0,)),
                                dict(fixed=(2,), sparsity=(0.05, 0.02, 0.01))],
                         ids=["sparsity", "normalize", "fixed0", "fixed-last-with-sparsity"])
def test_hals_options_against_the_oracle(name, kw):
    X, D, factors, r = case(name)
    N = D.ndim
    sparsity = list(kw["sparsity"]) + [None] * (N - 3) if "sparsity" in kw else None
    normalize = list(kw["normalize"]) + [False] * (N - 3) if "normalize" in kw else None
    fixed = kw.get("fixed", ())
    got, c = rs.one_step(X, factors, "hals", 2, sparsity_coefficients=sparsity, fixed_modes=fixed, normalize=normalize)
    want, co = oracle_step(D, r, factors, "hals", 2, sparsity=sparsity, fixed=fixed, normalize=normalize)
    for a, b in zip(got, want):
        assert close(a, b)
    assert abs(c - co) <= RTOL * abs(co)
    for f in fixed:
        assert np.array_equal(got[f], factors[f])


def test_generators():
    X = rs.from_slice_lengths([0, 1, 63, 64, 65, 197, 0], (50, 50), seed=3, stored_zeros=4)
    assert list(X.slice_lengths(0)) == [0, 1, 63, 64, 65, 197, 0] and X.shape == (7, 50, 50) and (X.vals == 0).sum() == 4
    coords, vals = X.sorted_by(2)
    assert (np.diff(coords[:, 2]) >= 0).all() and sorted(vals) == sorted(X.vals)
    same = coords[1:, 2] == coords[:-1, 2]      # inside a slice: lexicographic order of the other modes
    assert ((coords[1:, 0] > coords[:-1, 0]) | ((coords[1:, 0] == coords[:-1, 0]) & (coords[1:, 1] > coords[:-1, 1])))[same].all()
    Y = rs.Coo(X.coords[::-1], X.vals[::-1], X.shape)      # any input order gives the canonical list
    assert np.array_equal(Y.coords, X.coords) and np.array_equal(Y.vals, X.vals)

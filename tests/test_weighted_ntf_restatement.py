"""tests/weighted_ntf_restatement.py (weighted MU of any beta >= 0 on a dense tensor of any order) pinned three ways at the 1e-12 of
tests/test_oracle_golden.py, the refusals of the `weights=` keyword of ntf / compute_ntf / one_ntf_step (raised with no library and
no GPU present), and the recovery recipe the GPU test repeats on the device.

All ones: oracle/nnfac_oracle.py (one_ntf_step and compute_ntf with "mu"), orders 3 and 4.  0/1 weights:
tests/observed_restatement.py on from_dense(T, mask), NaN under the zeros, an empty slice in two modes.  Order 3 with one extent 1:
tests/weighted_restatement.py, each rank-one column of the 1-extent factor folded into the other two factors."""
import numpy as np
import pytest

import nnfac_oracle as orc
import observed_restatement as ob
import weighted_ntf_restatement as wn
import weighted_restatement as wr

RTOL = 1e-12
BETAS = (0, 0.5, 1, 2, 3)


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(b), 1e-300)


def case(shape, r, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random(shape) + 0.1, [rng.random((s, r)) + 0.05 for s in shape], rng


# ---- all ones: the oracle ----
@pytest.mark.parametrize("shape,r", [((7, 6, 5), 3), ((4, 5, 3, 6), 2)])
@pytest.mark.parametrize("beta", BETAS)
def test_all_ones_is_the_oracle(shape, r, beta):
    T, F, _ = case(shape, r)
    N, ones = len(shape), np.ones(shape)
    unf = [orc.unfold(T, m) for m in range(N)]
    for mode in range(N):
        got = wn.update_mode(T, ones, F, mode, beta)
        assert close(got, orc.mu_betadivmin(F[mode], orc.khatri_rao(F, skip_matrix=mode).T, unf[mode], beta))
    norm = np.linalg.norm(T)
    assert abs(wn.weighted_norm2(T, ones) - norm ** 2) <= RTOL * norm ** 2
    for fixed, sparsity in (([], [None] * N), ([1], [None] * N), ([N - 1], [0.3] + [None] * (N - 1))):
        F1, c = wn.one_step(T, ones, F, beta, norm, fixed, sparsity)
        Fo, co = orc.one_ntf_step(unf, r, [f.copy() for f in F], norm, "mu", beta, list(sparsity), fixed, [False] * N)
        assert all(close(a, b) for a, b in zip(F1, Fo)) and abs(c - co) <= RTOL * abs(co), (fixed, c, co)
    F5, costs = wn.run(T, ones, F, 5, beta)
    Fo, co, _ = orc.compute_ntf(T, r, [f.copy() for f in F], n_iter_max=5, tol=0, update_rule="mu", beta=beta, return_costs=True)
    assert all(close(a, b) for a, b in zip(F5, Fo)) and np.allclose(costs, co, rtol=RTOL, atol=0)


# ---- 0/1 weights: the observed-entries restatement, NaN under the zeros ----
def masked_case(shape, r):
    T, F, rng = case(shape, r, 1)
    mask = rng.random(shape) < 0.6
    mask[2] = False               # an empty slice of mode 0
    mask[..., 1] = False          # and of the last mode
    for at in ((0,) * len(shape), (1, 2, 2) + (0,) * (len(shape) - 3)):      # observed zeros
        mask[at], T[at] = True, 0.0
    return T, F, mask


@pytest.mark.parametrize("shape,r", [((7, 6, 5), 3), ((4, 5, 3, 6), 2)])
@pytest.mark.parametrize("beta", BETAS)
def test_zero_one_weights_are_the_observed_entries(shape, r, beta):
    T, F, mask = masked_case(shape, r)
    Wg = mask.astype(np.float64)
    Tn = np.where(mask, T, np.nan)
    S = ob.from_dense(T, mask)
    for mode in range(len(shape)):
        num, den = wn.sums(Tn, Wg, F, mode, beta)
        no, do = ob.sums(S, F, mode, beta)
        assert close(num, no) and close(den, do)
    Tf = np.where(T == 0, 1.0, T) if beta == 0 else T      # (beta = 0: an observed zero costs +inf in both; compare the finite part)
    Tfn, Sf = np.where(mask, Tf, np.nan), ob.from_dense(Tf, mask)
    assert abs(wn.weighted_norm2(Tfn, Wg) - Sf.vals @ Sf.vals) <= RTOL * (Sf.vals @ Sf.vals)
    if beta == 0:
        assert wn.cost(Tn, Wg, F, beta) == np.inf == ob.cost(S, F, beta)
    F5, costs = wn.run(Tfn, Wg, F, 5, beta)
    Fo, co = ob.run(Sf, F, 5, beta)
    assert all(close(a, b) for a, b in zip(F5, Fo)) and np.allclose(costs, co, rtol=RTOL, atol=0)
    assert np.isfinite(costs).all() and all(np.isfinite(f).all() for f in F5)
    assert np.array_equal(F5[0][2], F[0][2]) and np.array_equal(F5[-1][1], F[-1][1])      # the empty slices keep their values
    assert not np.array_equal(F5[0][1], F[0][1]) and not np.array_equal(F5[-1][0], F[-1][0])
    F1, c1 = wn.one_step(Tfn, Wg, F, beta, 3.0, fixed_modes=[0])
    Fo, co = ob.one_step(Sf, F, beta, fixed_modes=[0], normalized=False)
    assert all(close(a, b) for a, b in zip(F1, Fo)) and abs(c1 * 9.0 - co) <= RTOL * abs(co)


# ---- order 3 with one extent 1: the weighted matrix restatement ----
@pytest.mark.parametrize("beta", BETAS)
def test_an_extent_of_one_is_the_weighted_matrix_case(beta):
    (m, n, r) = (9, 8, 3)
    T, (A, b, C), rng = case((m, 1, n), r, 2)
    Wg = rng.random(T.shape) * 2
    Wg[rng.random(T.shape) < 0.25] = 0
    Wg[4] = 0                          # a slice of mode 0 without weight
    T = np.where(Wg == 0, np.nan, T)
    X, W2 = T[:, 0, :], Wg[:, 0, :]
    U, V = A * b, C.T                  # each rank-one column of the 1-extent factor folded into the first factor
    F = [A, b, C]
    assert close(wn.update_mode(T, Wg, F, 0, beta) * b, wr.update(X, W2, U, V, beta, "left"))
    assert close(wn.update_mode(T, Wg, F, 2, beta).T, wr.update(X, W2, U, V, beta, "right"))
    kr = orc.khatri_rao([A, C])        # (m n) x r, the first factor slowest: the row-major order of X
    assert close(wn.update_mode(T, Wg, F, 1, beta), wr.update(X.reshape(1, -1), W2.reshape(1, -1), b, kr.T, beta, "left"))
    c, cm = wn.cost(T, Wg, F, beta), wr.cost(X, W2, U, V, beta)
    assert abs(c - cm) <= RTOL * abs(cm)
    # a whole step with the 1-extent mode fixed is the matrix step on the folded factors
    F1, c1 = wn.one_step(T, Wg, F, beta, 1.0, fixed_modes=[1])
    U1, V1, cm1 = wr.one_step(X, W2, U, V, beta)
    assert close(F1[0] * b, U1) and close(F1[2].T, V1) and abs(c1 - cm1) <= RTOL * abs(cm1)
    assert np.array_equal(F1[0][4], A[4])


# ---- NaN and Inf under zero weight, scaling ----
@pytest.mark.parametrize("beta", BETAS)
def test_nan_under_zero_weight_changes_nothing_and_scaling_scales_the_cost_away(beta):
    T, F, rng = case((6, 5, 7), 3, 4)
    Wg = rng.random(T.shape) * 2
    off = rng.random(T.shape) < 0.3
    Wg[off] = 0
    Tbad = T.copy()
    Tbad[off] = rng.choice([np.nan, np.inf, -np.inf], size=int(off.sum()))
    a, b = wn.run(T * ~off, Wg, F, 3, beta), wn.run(Tbad, Wg, F, 3, beta)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1] and np.isfinite(b[1]).all()
    c = wn.run(Tbad, 7.5 * Wg, F, 3, beta)      # the normalisation scales with the weights: the same costs
    assert all(close(x, y) for x, y in zip(b[0], c[0])) and np.allclose(b[1], c[1], rtol=RTOL, atol=0)


# ---- the recovery recipe (the GPU test repeats it on the device) ----
RECOVERY = (0.00324, 0.0678)      # a stand-alone fp64 run of the formulas, beta = 2, 300 iterations: with weights, without


def test_recovery_recipe():
    truth, T, Wg, F0 = wn.recovery_case()
    Fw, _ = wn.run(T, Wg, F0, 300, 2)
    Fn, _ = wn.run(T, np.ones_like(T), F0, 300, 2)
    ew, en = wn.recovery_error(truth, Fw), wn.recovery_error(truth, Fn)
    print("with weights", ew, "without", en)
    assert ew <= 0.02 and en >= 0.05 and en >= 4 * ew
    assert abs(ew - RECOVERY[0]) <= 0.06 * RECOVERY[0] and abs(en - RECOVERY[1]) <= 0.06 * RECOVERY[1]


# ---- the keyword's refusals: before the device is touched ----
def _calls(T, F0, **kw):
    """The three public functions on one request (ntf with custom start values)."""
    from nn_fac_amd import ntf as drv
    r, N = F0[0].shape[1], len(F0)
    rule, beta, init = kw.pop("update_rule", "mu"), kw.pop("beta", 1), kw.pop("init", "custom")
    out = [lambda: drv.ntf(T, r, init=init, factors_0=F0, n_iter_max=2, update_rule=rule, beta=beta, **kw)]
    if init == "custom":
        out.append(lambda: drv.compute_ntf(T, r, F0, n_iter_max=2, update_rule=rule, beta=beta, **kw))
        unf = T if not isinstance(T, np.ndarray) else [orc.unfold(T, m) for m in range(N)]
        out.append(lambda: drv.one_ntf_step(unf, r, F0, 1.0, rule, beta, [None] * N, [], [False] * N, **kw))
    return out


def test_weight_keyword_refusals(monkeypatch):
    import torch
    from nn_fac_amd import engine, _lib, weighted_ntf
    from nn_fac_amd._convert import SparseCOO
    from nn_fac_amd.utils import errors as err

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(engine, "get_engine", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    T, F0, rng = case((6, 5, 7), 3, 5)
    Wg = rng.random(T.shape)
    table = [
        (dict(weights=Wg, update_rule="hals", beta=2), NotImplementedError, 'update_rule="mu"'),
        (dict(weights=Wg, init="nndsvd"), NotImplementedError, 'init="random"'),
        (dict(weights=Wg[:, :, :-1]), err.InvalidArgumentValue, "shape of the tensor"),
        (dict(weights=Wg.transpose(2, 1, 0)), err.InvalidArgumentValue, "shape of the tensor"),
        (dict(weights=(Wg * 3).astype(np.int64)), err.InvalidArgumentValue, "astype"),
        (dict(weights=Wg, beta=-1), err.InvalidArgumentValue, "beta"),
        (dict(weights=Wg, beta=float("nan")), err.InvalidArgumentValue, "beta"),
        (dict(weights=Wg, beta=float("inf")), err.InvalidArgumentValue, "beta"),
    ]
    for kw, exc, says in table:
        calls = _calls(T, F0, **dict(kw))
        assert calls
        for call in calls:
            with pytest.raises(exc, match=says):
                call()
    with pytest.raises(NotImplementedError, match="group="):
        weighted_ntf.compute_weighted_ntf(T, 3, F0, Wg, n_iter_max=2, beta=1, group=object())
    S = SparseCOO(np.argwhere(T > 0.5).T, T[T > 0.5].astype(np.float32), T.shape)
    for call in _calls(S, F0, weights=Wg):
        with pytest.raises(err.InvalidArgumentValue, match='unstored="missing"'):
            call()
    big = [np.ones((s, 129)) for s in (130, 5, 6)]      # rank above 128
    for call in _calls(np.ones((130, 5, 6)), big, weights=np.ones((130, 5, 6))):
        with pytest.raises(err.EngineError, match="rank 129"):
            call()
    # one_ntf_step takes the weights in the shape of the mode-0 unfolding too: the same refusal, not one of the shape
    unf = [orc.unfold(T, m) for m in range(3)]
    from nn_fac_amd import ntf as drv
    with pytest.raises(NotImplementedError, match='update_rule="mu"'):
        drv.one_ntf_step(unf, 3, F0, 1.0, "hals", 2, [None] * 3, [], [False] * 3, weights=Wg.reshape(6, -1))
    with pytest.raises(err.InvalidArgumentValue, match="shape of the tensor"):
        drv.one_ntf_step(unf, 3, F0, 1.0, "mu", 2, [None] * 3, [], [False] * 3, weights=Wg.reshape(-1, 7))

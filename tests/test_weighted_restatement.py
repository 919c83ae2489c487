"""tests/weighted_restatement.py (weighted MU of any beta >= 0 on dense data) pinned four ways at the 1e-12 of
tests/test_oracle_golden.py, the refusals of the `weights=` keyword of nmf / compute_nmf / one_nmf_step (raised with no library and
no GPU present), the recovery recipe the GPU test repeats on the device, and the plan lines of the weighted MU forms
(tools/nnf_plan.cpp, `ldw=`): the general-beta plans at every MU shape of tests/test_gpu_launch_plans.py, and a shape where the
pitch of the weights alone moves the 32-bit offset bound.

All ones: oracle/nnfac_oracle.py (mu_betadivmin, one_nmf_step with "mu", beta_divergence).  0/1 weights:
tests/observed_restatement.py on from_dense(X, mask), an empty row and an empty column included.  Integer weights: a column of
weight k is that column written k times with weight 1.  Scaling: c Wg gives the same factors and c times the cost.  NaN and Inf
under zero weight change nothing."""
import numpy as np
import pytest

import nnfac_oracle as orc
import observed_restatement as ob
import weighted_restatement as wr
from test_gpu_launch_plans import plan_cases
from test_mu_plan_table import CUS, WS_DEFAULT, ask

RTOL = 1e-12
BETAS = (0, 0.5, 1, 2, 3)


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(b), 1e-300)


def case(seed=0, m=23, n=17, r=4):
    rng = np.random.default_rng(seed)
    return rng.random((m, n)) + 0.1, rng.random((m, r)) + 0.05, rng.random((r, n)) + 0.05, rng


# ---- all ones: the oracle ----
@pytest.mark.parametrize("beta", BETAS)
def test_all_ones_is_the_oracle(beta):
    X, U, V, _ = case()
    ones = np.ones_like(X)
    assert close(wr.update(X, ones, U, V, beta, "left"), orc.mu_betadivmin(U, V, X, beta))
    assert close(wr.update(X, ones, U, V, beta, "right"), orc.mu_betadivmin(V.T, U.T, X.T, beta).T)
    co = orc.beta_divergence(X, U @ V, beta)
    assert abs(wr.cost(X, ones, U, V, beta) - co) <= RTOL * abs(co)
    U1, V1, c = wr.one_step(X, ones, U, V, beta)
    Uo, Vo, co = orc.one_nmf_step(X, 4, U.copy(), V.copy(), np.linalg.norm(X), "mu", beta, [None, None], [], [False, False], True)
    assert close(U1, Uo) and close(V1, Vo) and abs(c - co) <= RTOL * abs(co)
    U5, V5, costs = wr.run(X, ones, U, V, 5, beta)
    Uo, Vo, co, _ = orc.compute_nmf(X, 4, U.copy(), V.copy(), n_iter_max=5, tol=0, update_rule="mu", beta=beta, return_costs=True,
                                    deterministic=True)
    assert close(U5, Uo) and close(V5, Vo) and np.allclose(costs, co, rtol=RTOL, atol=0)


# ---- 0/1 weights: the observed-entries restatement ----
def masked_case():
    X, U, V, rng = case(1)
    mask = rng.random(X.shape) < 0.6
    mask[5, :] = False       # an empty row
    mask[:, 11] = False      # an empty column
    mask[0, 0] = mask[7, 3] = True
    X[0, 0] = X[7, 3] = 0.0      # observed zeros
    return X, U, V, mask


@pytest.mark.parametrize("beta", BETAS)
def test_zero_one_weights_are_the_observed_entries(beta):
    X, U, V, mask = masked_case()
    Wg = mask.astype(np.float64)
    S, F = ob.from_dense(X, mask), ob.nmf_factors(U, V)
    for side, mode in (("left", 0), ("right", 1)):
        num, den = wr.sums(X, Wg, U, V, beta, side)
        no, do = ob.sums(S, F, mode, beta)
        assert close(num if mode == 0 else num.T, no) and close(den if mode == 0 else den.T, do)
    Xf = np.where(X == 0, 1.0, X) if beta == 0 else X      # (beta = 0: an observed zero costs +inf in both; compare the finite part)
    c, co = wr.cost(Xf, Wg, U, V, beta), ob.cost(ob.from_dense(Xf, mask), F, beta)
    assert abs(c - co) <= RTOL * abs(co)
    if beta == 0:
        assert wr.cost(X, Wg, U, V, beta) == np.inf == ob.cost(S, F, beta)
    U5, V5, costs = wr.run(Xf, Wg, U, V, 5, beta)
    (Uo, Vto), co = ob.run(ob.from_dense(Xf, mask), F, 5, beta, normalized=False)
    assert close(U5, Uo) and close(V5, Vto.T) and np.allclose(costs, co, rtol=RTOL, atol=0)
    assert np.array_equal(U5[5], U[5]) and np.array_equal(V5[:, 11], V[:, 11])      # the empty slices keep their values
    assert not np.array_equal(U5[4], U[4]) and not np.array_equal(V5[:, 10], V[:, 10])


# ---- integer weights: a column written k times ----
@pytest.mark.parametrize("beta", BETAS)
def test_integer_weight_is_the_column_written_k_times(beta):
    X, U, V, rng = case(2)
    k, j = 3, 6
    Wg = np.ones_like(X)
    Wg[:, j] = k
    cols = list(range(X.shape[1])) + [j] * (k - 1)
    X2, V2, ones = X[:, cols], V[:, cols], np.ones((X.shape[0], len(cols)))
    assert close(wr.update(X, Wg, U, V, beta, "left"), wr.update(X2, ones, U, V2, beta, "left"))
    c, c2 = wr.cost(X, Wg, U, V, beta), wr.cost(X2, ones, U, V2, beta)
    assert abs(c - c2) <= RTOL * abs(c2)
    Vn, Vn2 = wr.update(X, Wg, U, V, beta, "right"), wr.update(X2, ones, U, V2, beta, "right")
    assert close(Vn, Vn2[:, :X.shape[1]])
    for extra in range(k - 1):
        assert close(Vn2[:, X.shape[1] + extra], Vn2[:, j])


# ---- scaling ----
@pytest.mark.parametrize("beta", BETAS)
def test_scaled_weights_give_the_same_factors(beta):
    X, U, V, rng = case(3)
    Wg = rng.random(X.shape) * 2
    Wg[rng.random(X.shape) < 0.2] = 0
    U1, V1, c1 = wr.run(X, Wg, U, V, 5, beta)
    U2, V2, c2 = wr.run(X, 7.5 * Wg, U, V, 5, beta)
    assert close(U1, U2) and close(V1, V2) and np.allclose(np.asarray(c1) * 7.5, c2, rtol=RTOL, atol=0)


# ---- NaN and Inf under zero weight ----
@pytest.mark.parametrize("beta", BETAS)
def test_nan_and_inf_under_zero_weight_change_nothing(beta):
    X, U, V, rng = case(4)
    Wg = rng.random(X.shape) * 2
    off = rng.random(X.shape) < 0.3
    Wg[off] = 0
    Xbad = X.copy()
    Xbad[off] = rng.choice([np.nan, np.inf, -np.inf], size=int(off.sum()))
    a, b = wr.run(X, Wg, U, V, 3, beta), wr.run(Xbad, Wg, U, V, 3, beta)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.isfinite(b[0]).all() and np.isfinite(b[1]).all() and np.isfinite(b[2]).all()
    for side in ("left", "right"):
        for x, y in zip(wr.sums(X, Wg, U, V, beta, side), wr.sums(Xbad, Wg, U, V, beta, side)):
            assert np.array_equal(x, y)


# ---- the recovery recipe (the GPU test repeats it on the device) ----
RECOVERY = {2: (0.0067, 0.094), 1: (0.0062, 0.19)}      # a stand-alone fp64 run of the formulas: with weights, without


@pytest.mark.parametrize("beta", (2, 1))
def test_recovery_recipe(beta):
    T, X, Wg, U0, V0 = wr.recovery_case(beta)
    Uw, Vw, _ = wr.run(X, Wg, U0, V0, 300, beta)
    Un, Vn, _ = wr.run(X, np.ones_like(X), U0, V0, 300, beta)
    ew, en = wr.recovery_error(T, Uw, Vw), wr.recovery_error(T, Un, Vn)
    print("beta", beta, "with weights", ew, "without", en)
    assert ew <= 0.02 and en >= 0.05
    assert abs(ew - RECOVERY[beta][0]) <= 0.06 * RECOVERY[beta][0] and abs(en - RECOVERY[beta][1]) <= 0.06 * RECOVERY[beta][1]


# ---- the keyword's refusals: before the device is touched ----
def _calls(X, U0, V0, **kw):
    """The three public functions on one request (nmf with custom start values)."""
    from nn_fac_amd import nmf as drv
    r = U0.shape[1]
    rule, beta = kw.pop("update_rule", "mu"), kw.pop("beta", 1)
    group, init = kw.pop("group", None), kw.pop("init", "custom")
    out = [lambda: drv.nmf(X, r, init=init, U_0=U0, V_0=V0, n_iter_max=2, update_rule=rule, beta=beta, **kw)]
    if init == "custom":
        out.append(lambda: drv.compute_nmf(X, r, U0, V0, n_iter_max=2, update_rule=rule, beta=beta, group=group, **kw))
        if group is None:
            out.append(lambda: drv.one_nmf_step(X, r, U0, V0, 1.0, rule, beta, [None, None], [], [False, False], True, **kw))
    return out[1:2] if group is not None else out


def test_weight_keyword_refusals(monkeypatch):
    import scipy.sparse as sp
    import torch
    from nn_fac_amd import engine, _lib
    from nn_fac_amd.utils import errors as err

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(engine, "get_engine", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    X, U0, V0, rng = case(5, 20, 15, 3)
    V0 = V0.copy()
    Wg = rng.random(X.shape)
    table = [
        (dict(weights=Wg, update_rule="hals", beta=2), NotImplementedError, 'update_rule="mu"'),
        (dict(weights=Wg, group=object()), NotImplementedError, "group="),
        (dict(weights=Wg, init="nndsvd"), NotImplementedError, 'init="random"'),
        (dict(weights=Wg[:, :-1]), err.InvalidArgumentValue, "shape of the data"),
        (dict(weights=Wg.T), err.InvalidArgumentValue, "shape of the data"),
        (dict(weights=(Wg * 3).astype(np.int64)), err.InvalidArgumentValue, "astype"),
        (dict(weights=Wg, beta=-1), err.InvalidArgumentValue, "beta"),
        (dict(weights=Wg, beta=float("nan")), err.InvalidArgumentValue, "beta"),
    ]
    for kw, exc, says in table:
        calls = _calls(X, U0, V0, **dict(kw))
        assert calls
        for call in calls:
            with pytest.raises(exc, match=says):
                call()
    for call in _calls(sp.csr_matrix(X), U0, V0, weights=Wg):
        with pytest.raises(err.InvalidArgumentValue, match='unstored="missing"'):
            call()
    big = np.ones((140, 129))      # rank above 128
    for call in _calls(np.ones((140, 150)), big, np.ones((129, 150)), weights=np.ones((140, 150))):
        with pytest.raises(err.EngineError, match="rank 129"):
            call()


def test_weight_values_are_checked_by_the_weighted_module():
    """Negative and non-finite weights are refused by one reduction on the uploaded weights (weights_to_dev): here on the CPU."""
    import torch
    from nn_fac_amd import weighted_nmf
    from nn_fac_amd.utils import errors as err
    good = np.array([[0.0, 1.5], [2.0, 0.0]])
    assert weighted_nmf.weights_to_dev(good, torch.device("cpu")).dtype == torch.float32
    mask = weighted_nmf.weights_to_dev(good > 0, torch.device("cpu"))
    assert mask.dtype == torch.float32 and mask.tolist() == [[0.0, 1.0], [1.0, 0.0]]
    for bad in (-1e-3, np.nan, np.inf):
        w = good.copy()
        w[1, 0] = bad
        with pytest.raises(err.InvalidArgumentValue, match="finite and >= 0"):
            weighted_nmf.weights_to_dev(w, torch.device("cpu"))


# ---- plan lines of the weighted forms ----
def _mu_lines(C):
    """(general-beta line, weighted line) of every MU shape of the launch-plan table; the weights at the pitch of X."""
    out = []
    for name, c in plan_cases(C).items():
        if c.kernel not in ("mu_left", "mu_right", "mu_accum"):
            continue
        launcher = "mu_left" if c.kernel == "mu_left" else "mu_right"
        head = "%s %d %d %d %d %d" % (launcher, C, c.m, c.n, c.r, c.ld or c.n)
        ws = WS_DEFAULT if c.ws is None else c.ws
        for beta in sorted({c.beta, 1.0, 2.0}):      # the weighted form takes the general-beta plan at EVERY beta
            out.append((name, "%s 0.5 %d" % (head, ws), "%s %r %d ldw=%d" % (head, beta, ws, c.ld or c.n)))
    return out


@pytest.mark.parametrize("C", CUS)
def test_weighted_plans_are_the_general_beta_plans(C):
    lines = _mu_lines(C)
    gen, wgt = ask([l[1] for l in lines]), ask([l[2] for l in lines])
    assert len(lines) > 100
    for (name, _, wl), g, w in zip(lines, gen, wgt):
        if "status" in g:      # (a workspace sized for the ONE set of slabs of a KL case)
            assert w == g, (name, wl, g, w)
            continue
        assert g["bm"] == "GEN" and w["bm"] == "WGEN" and w["rem"] == 0, (name, g, w)
        assert {k: v for k, v in g.items() if k != "bm"} == {k: v for k, v in w.items() if k != "bm"}, (name, wl, g, w)


@pytest.mark.parametrize("C", CUS)
def test_the_pitch_of_the_weights_alone_moves_the_offset_bound(C):
    END = 0x7fff0000
    # right: more 128-column blocks than CUs -> one split of rup(200, 64) = 256 rows; the weights' pitch puts 256 + 128 rows
    # outside 32-bit offsets, 128 + 128 rows inside
    n = 128 * C + 200
    ldw = 4 * (-(-END // (4 * 384 * 4)) + 1)
    assert 384 * n * 4 < END <= 384 * ldw * 4 and 256 * ldw * 4 < END
    head = "mu_right %d 200 %d 128 %d 0.5 %d" % (C, n, n, WS_DEFAULT)
    same, wide = ask([head + " ldw=%d" % n, head + " ldw=%d" % ldw])
    assert (same["bound"], same["nsplit"], same["rps"]) == ("occupancy", 1, 256)
    assert (wide["bound"], wide["nsplit"], wide["rps"], wide["bm"], wide["vec"]) == ("offset32", 2, 128, "WGEN", 1)
    # left: 64 rows of X and of the weights inside 32-bit offsets -- refused once the weights' pitch takes them outside
    ld_in, ld_out = (END - 4 * (72 + 128)) // 256 - 1, (END - 4 * (72 + 128)) // 256 + 4
    head = "mu_left %d 300 72 50 72 0.5 %d" % (C, WS_DEFAULT)
    ok, refused, unaligned = ask([head + " ldw=%d" % ld_in, head + " ldw=%d" % ld_out, head + " ldw=75"])
    assert ok["bm"] == "WGEN" and ok["form"] == "small" and refused == {"status": -3}
    assert unaligned["vec"] == 0      # 16-byte loads need X AND the weights aligned
    assert ask([head + " ldw=72 walign=1"])[0]["vec"] == 0 and ask([head + " ldw=72"])[0]["vec"] == 1
    assert ask([head + " ldw=71"]) == [{"status": -1}]      # a pitch below the row length

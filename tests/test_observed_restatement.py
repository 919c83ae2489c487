"""tests/observed_restatement.py (MU over the stored entries only, any beta >= 0) against oracle/nnfac_oracle.py and against an
independently written dense formula, at the 1e-12 of tests/test_oracle_golden.py.

With EVERY entry stored the observed-only update is the reference's own: one step and five steps equal mu_betadivmin / the NTF MU
step of the oracle on the dense array (a 23 x 17 matrix at rank 4; 9 x 8 x 7, 6 x 5 x 4 x 5 and 4 x 3 x 4 x 3 x 3 tensors at ranks
4, 3, 3).  With a partial pattern -- stored zeros, an empty row and an empty column (an empty slice per mode) included -- the step
equals the dense formula with a 0/1 weight array W,  (W o X o P^(beta - 2)) K / (W o P^(beta - 1)) K  on the unfolding, and the
empty slices keep their start values exactly.  Also here: the plan line of the observed-entries kernels (tools/nnf_plan.cpp `obs`)
and observed_entries (nn_fac_amd/_convert.py), which must keep masked zeros through to_dev_csr / to_dev_coo."""
import numpy as np
import pytest
import torch

import nnfac_oracle as orc
import observed_restatement as ob
from test_mu_plan_table import ask
from test_sparse_plan import edge_lengths, rup

RTOL = 1e-12
BETAS = (0, 0.5, 1, 1.5, 2, 3)
SHAPES = {"23x17": ((23, 17), 4), "9x8x7": ((9, 8, 7), 4), "6x5x4x5": ((6, 5, 4, 5), 3), "4x3x4x3x3": ((4, 3, 4, 3, 3), 3)}


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) <= rtol * max(np.linalg.norm(b), 1e-300)


def full_case(name, seed=0):
    shape, r = SHAPES[name]
    rng = np.random.default_rng(seed)
    D = rng.random(shape) + 0.1
    factors = [rng.random((d, r)) + 0.05 for d in shape]
    return D, ob.from_dense(D, np.ones(shape, bool)), factors, r


def oracle_step(D, r, factors, beta):
    """The oracle's MU step: (factors, cost) -- the cost as the oracle's driver of that order states it."""
    if D.ndim == 2:
        U, V, c = orc.one_nmf_step(D, r, factors[0].copy(), factors[1].T.copy(), np.linalg.norm(D), "mu", beta, [None, None], [],
                                   [False, False], True)
        return [U, V.T], c
    return orc.one_ntf_step([orc.unfold(D, m) for m in range(D.ndim)], r, [F.copy() for F in factors], np.linalg.norm(D), "mu", beta,
                            [None] * D.ndim, [], [False] * D.ndim)


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("beta", BETAS)
def test_every_entry_stored_one_step_is_the_oracles(name, beta):
    D, X, factors, r = full_case(name)
    got, c = ob.one_step(X, factors, beta)
    want, co = oracle_step(D, r, factors, beta)
    for a, b in zip(got, want):
        assert close(a, b)
    assert abs(c - co) <= RTOL * abs(co)
    for mode in range(D.ndim):      # and the update of one mode alone is mu_betadivmin on that unfolding
        krao = orc.khatri_rao(factors, skip_matrix=mode)
        assert close(ob.update_mode(X, factors, mode, beta), orc.mu_betadivmin(factors[mode], krao.T, orc.unfold(D, mode), beta)), mode


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("beta", BETAS)
def test_every_entry_stored_five_steps_are_the_oracles(name, beta):
    D, X, _, r = full_case(name)
    rng = np.random.default_rng(7)
    start = [rng.random((d, r)) + 0.01 for d in D.shape]
    got, costs = ob.run(X, start, 5, beta)
    if D.ndim == 2:
        U, V, co, _ = orc.compute_nmf(D, r, start[0].copy(), start[1].T.copy(), n_iter_max=5, tol=0, update_rule="mu", beta=beta,
                                      return_costs=True, deterministic=True)
        want = [U, V.T]
    else:
        want, co, _ = orc.compute_ntf(D, r, [F.copy() for F in start], n_iter_max=5, tol=0, update_rule="mu", beta=beta,
                                      return_costs=True)
    assert len(costs) == 5
    for a, b in zip(got, want):
        assert close(a, b)
    assert np.allclose(costs, co, rtol=RTOL, atol=0)


def partial_case(name):
    """About 40 % stored, four stored zeros, slice 1 of every one of the first three modes (both modes of a matrix) empty."""
    shape, r = SHAPES[name]
    rng = np.random.default_rng(3)
    D = rng.random(shape) + 0.1
    W = rng.random(shape) < 0.4
    for mode in range(min(len(shape), 3)):
        W[(slice(None),) * mode + (1,)] = False
    where = np.argwhere(W)
    for at in where[rng.choice(len(where), size=4, replace=False)]:
        D[tuple(at)] = 0.0
    factors = [rng.random((d, r)) + 0.05 for d in shape]
    return D, W, ob.from_dense(D, W), factors


def dense_update(D, W, factors, mode, beta):
    """The weighted dense formula on the unfolding of `mode`, written without the restatement: rows with no weight are left."""
    K = orc.khatri_rao(factors, skip_matrix=mode)
    Xm, Wm = orc.unfold(D, mode), orc.unfold(W.astype(np.float64), mode)
    P = factors[mode] @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        R1 = np.where(Xm == 0, 0.0, Wm * Xm * P ** (beta - 2.0))
    num, den = R1 @ K, (Wm * P ** (beta - 1.0)) @ K
    F = factors[mode].copy()
    seen = Wm.sum(axis=1) > 0
    gamma = 1 / (2 - beta) if beta < 1 else 1 / (beta - 1) if beta > 2 else 1
    F[seen] = np.maximum(F[seen] * (num[seen] / den[seen]) ** gamma, 1e-12)
    return F


def dense_cost(D, W, factors, beta):
    letters = "abcde"[:D.ndim]
    P = np.einsum(",".join(l + "z" for l in letters) + "->" + letters, *factors)
    x, p = D[W], P[W]
    if beta == 1:
        return float(np.sum(np.where(x == 0, 0.0, x * np.log(np.where(x == 0, 1.0, x) / p)) - x + p))
    if beta == 0:
        with np.errstate(divide="ignore"):
            return float(np.sum(x / p - np.log(x / p) - 1))
    return float(np.sum((x ** beta + (beta - 1) * p ** beta - beta * x * p ** (beta - 1)) / (beta * (beta - 1))))


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("beta", BETAS)
def test_partial_pattern_against_the_weighted_dense_formula(name, beta):
    D, W, X, factors = partial_case(name)
    assert (X.vals == 0).sum() == 4 and 0.1 < X.nnz / D.size < 0.45      # (the emptied slices of a small tensor take a share)
    cur = [F.copy() for F in factors]
    for mode in range(D.ndim):
        num, den = ob.sums(X, cur, mode, beta)
        got = ob.update_mode(X, cur, mode, beta)
        assert close(got, dense_update(D, W, cur, mode, beta)), mode
        if mode < 3:
            assert X.slice_lengths(mode)[1] == 0
            assert np.array_equal(got[1], cur[mode][1]) and not num[1].any() and not den[1].any(), mode
        cur[mode] = got
    stepped, c = ob.one_step(X, factors, beta, normalized=False)
    for a, b in zip(stepped, cur):
        assert np.array_equal(a, b)
    want = dense_cost(D, W, cur, beta)
    assert (np.isinf(c) and np.isinf(want)) if beta == 0 else abs(c - want) <= RTOL * abs(want)      # (beta = 0: d(0 | p) = +inf)
    # five steps: the empty slices still hold their start values, everything else moved
    five, costs = ob.run(X, factors, 5, beta)
    for mode in range(min(D.ndim, 3)):
        assert np.array_equal(five[mode][1], factors[mode][1])
        assert not np.array_equal(five[mode][0], factors[mode][0])
    if beta != 0:
        assert all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:])), costs      # MU with the Fevotte-Idier exponent descends


def test_fixed_modes_and_the_normalised_cost():
    D, W, X, factors = partial_case("9x8x7")
    got, c = ob.one_step(X, factors, 1, fixed_modes=(1,))
    assert np.array_equal(got[1], factors[1]) and not np.array_equal(got[0], factors[0])
    _, raw = ob.one_step(X, factors, 1, fixed_modes=(1,), normalized=False)
    assert abs(c - raw / np.sum(D[W] ** 2)) <= RTOL * c


@pytest.mark.parametrize("beta", [2, 1])
def test_recovery_recipes_in_fp64(beta):
    """The figures the recovery test of the GPU suite leans on: the held-out error of the observed-only fit after 200 iterations."""
    rng = np.random.default_rng(0)
    A, B = rng.random((60, 3)) + 0.1, rng.random((3, 50)) + 0.1
    X, M = A @ B, rng.random((60, 50)) < 0.4
    U0, V0 = rng.random((60, 3)), rng.random((3, 50))
    factors, _ = ob.run(ob.from_dense(X, M), ob.nmf_factors(U0, V0), 200, beta)
    assert ob.heldout_error(X, M, factors) < 0.012
    rng = np.random.default_rng(0)
    true = [rng.random((d, 3)) + 0.1 for d in (30, 25, 20)]
    T = np.einsum("az,bz,cz->abc", *true)
    M = rng.random(T.shape) < 0.3
    start = [rng.random((d, 3)) for d in (30, 25, 20)]
    factors, _ = ob.run(ob.from_dense(T, M), start, 200, beta)
    assert ob.heldout_error(T, M, factors) < 0.02


# ---- the plan line of the observed-entries kernels --------------------------------------------------------------------------------
def obs_line(C, r, ng, lens, **kw):
    return "obs %d r=%d ng=%d lens=%s" % (C, r, ng, ",".join(str(k) for k in lens)) + "".join(" %s=%d" % kv for kv in kw.items())


@pytest.mark.parametrize("C", (256, 304))
@pytest.mark.parametrize("ng", (1, 2, 3, 4))
def test_plan_line_workspace_and_the_kl_plans_lanes(C, ng):
    lens = edge_lengths(64) + [17] * 9
    nchunks = sum(-(-k // 64) for k in lens)
    txt = ",".join(str(k) for k in lens)
    for r in (1, 10, 50, 64, 65, 100, 128):
        for out, cost in ((1, 0), (1, 1), (0, 1)):
            plan, = ask([obs_line(C, r, ng, lens, ch=64, out=out, cost=cost)])
            tag = (C, r, ng, out, cost, plan)
            assert "status" not in plan and plan["ng"] == ng, tag
            one = nchunks * rup(r, 4) * 4
            assert plan["part_bytes"] == (2 * one if out else 0), tag
            assert plan["cost_bytes"] == (8 * -(-nchunks // 4) if cost else 0), tag
            want = 0      # as the cursor carves them: numerator rows, denominator rows, cost partials, each from a 256-byte boundary
            for piece in ([one, one] if out else []) + ([plan["cost_bytes"]] if cost else []):
                want = rup(want, 256) + piece
            assert plan["ws_bytes"] == plan["carved"] == want, tag
            assert ask([obs_line(C, r, ng, lens, ch=64, out=out, cost=cost, ws=want - 1)])[0] == {"status": -4}, tag
            assert "status" not in ask([obs_line(C, r, ng, lens, ch=64, out=out, cost=cost, ws=want)])[0], tag
            # lanes, entries in flight and everything else: the KL plan of the same (r, ng)
            kl, = ask([("sparse %d r=%d" % (C, r) if ng == 1 else "sptensor %d r=%d ng=%d" % (C, r, ng))
                       + " lens=%s ch=64 out=%d cost=%d" % (txt, out, cost)])
            for key in ("L", "U", "G", "rp", "grid", "tgrid", "lds_bytes", "cost_bytes", "nchunks", "chunks"):
                assert plan[key] == kl[key], (key, tag)
            assert plan["part_bytes"] == 2 * kl["part_bytes"], tag


def test_plan_line_refusals_and_names():
    got = ask([obs_line(256, 129, 1, [5]), obs_line(256, 129, 3, [5]), obs_line(256, 128, 1, [5]), obs_line(256, 5, 5, [5]),
               obs_line(256, 5, 0, [5]), obs_line(256, 5, 2, [5], out=0, cost=0), obs_line(256, 5, 2, [0, 0], ws=0)])
    assert [g.get("status", 0) for g in got] == [-3, -3, 0, -1, -1, -1, 0], got
    assert (got[6]["nchunks"], got[6]["ws_bytes"], got[6]["tgrid"]) == (0, 0, 1)
    import subprocess
    from test_mu_plan_table import plan_tool
    text = subprocess.run([plan_tool()], input=obs_line(256, 5, 1, [5]) + "\n" + obs_line(256, 5, 2, [5]) + "\n", capture_output=True,
                          text=True, check=True).stdout.splitlines()
    assert text[0].startswith("[nnf plan] csr_obs ") and text[1].startswith("[nnf plan] sptensor_obs "), text


# ---- observed_entries -------------------------------------------------------------------------------------------------------------
def test_observed_entries_keeps_masked_zeros_through_the_conversions():
    from nn_fac_amd._convert import SparseCOO, observed_entries, to_dev_coo, to_dev_csr
    from nn_fac_amd import sparse_nmf, sparse_ntf
    assert sparse_nmf.observed_entries is observed_entries and sparse_ntf.observed_entries is observed_entries
    cpu = torch.device("cpu")
    rng = np.random.default_rng(5)
    A = rng.random((7, 9))
    M = rng.random((7, 9)) < 0.5
    M[3, :] = False
    zeros = np.argwhere(M)[::4]
    A[tuple(zeros.T)] = 0.0
    for arr, mask in ((A, M), (torch.from_numpy(A), torch.from_numpy(M)), (A.astype(np.float32), M)):
        S = observed_entries(arr, mask)
        assert S.layout == torch.sparse_csr and tuple(S.shape) == (7, 9) and S.values().numel() == M.sum()
        rowptr, colidx, vals, shape = to_dev_csr(S, cpu)
        assert shape == (7, 9) and rowptr.tolist() == [0] + list(np.cumsum(M.sum(axis=1)))
        assert np.array_equal(np.column_stack([np.repeat(np.arange(7), np.diff(rowptr.numpy())), colidx.numpy()]), np.argwhere(M))
        assert np.array_equal(vals.numpy(), A[M].astype(np.float32)) and (vals == 0).sum() == len(zeros) > 0
        rowptr, colidx, vals, shape = to_dev_csr(S, cpu, transpose=True)
        assert shape == (9, 7) and np.array_equal(vals.numpy(), A.T[M.T].astype(np.float32))
        assert np.array_equal(colidx.numpy(), np.argwhere(M.T)[:, 1])
    # scipy input with explicit zeros: kept as well (csr_matrix(dense) would have dropped them before it got here)
    import scipy.sparse as sp
    r, c = np.nonzero(M)
    for X in (sp.csr_matrix((A[M], (r, c)), shape=A.shape), sp.coo_matrix((A[M], (r, c)), shape=A.shape),
              sp.csc_matrix((A[M], (r, c)), shape=A.shape)):
        for tr in (False, True):
            vals = to_dev_csr(X, cpu, transpose=tr)[2]
            assert vals.numel() == M.sum() and (vals == 0).sum() == len(zeros), (type(X).__name__, tr)
        assert X.nnz == M.sum()      # (the caller's matrix is not touched)
    T = rng.random((4, 5, 3, 2))
    MT = rng.random(T.shape) < 0.4
    zt = np.argwhere(MT)[::5]
    T[tuple(zt.T)] = 0.0
    for arr, mask in ((T, MT), (torch.from_numpy(T), torch.from_numpy(MT))):
        S = observed_entries(arr, mask)
        assert isinstance(S, SparseCOO) and S.shape == T.shape
        ind, val, shape = to_dev_coo(S, cpu)
        assert np.array_equal(ind.numpy().T, np.argwhere(MT)) and np.array_equal(val.numpy(), T[MT].astype(np.float32))
        assert (val == 0).sum() == len(zt) > 0
        coo = torch.sparse_coo_tensor(S.indices, S.values, S.shape)      # an uncoalesced torch tensor keeps them too
        assert (to_dev_coo(coo, cpu)[1] == 0).sum() == len(zt)
    with pytest.raises(ValueError):
        observed_entries(A, M[:, :5])
    with pytest.raises(ValueError):
        observed_entries(A, M.astype(np.float64))


def test_refusals_that_need_no_device():
    """The keyword's own refusals are said before a device is looked for."""
    from nn_fac_amd import nmf as nmf_mod, ntf as ntf_mod, sparse_nmf, sparse_ntf
    from nn_fac_amd.utils import errors as err
    A = np.random.default_rng(0).random((6, 5))
    with pytest.raises(err.InvalidArgumentValue, match="dense"):
        nmf_mod.compute_nmf(A, 2, A[:, :2], A[:2, :], unstored="missing", update_rule="mu")
    with pytest.raises(err.InvalidArgumentValue, match="unstored"):
        nmf_mod.compute_nmf(A, 2, A[:, :2], A[:2, :], unstored="nan")
    with pytest.raises(err.InvalidArgumentValue, match="dense"):
        ntf_mod.compute_ntf(np.ones((3, 3, 3)), 2, [np.ones((3, 2))] * 3, unstored="missing", update_rule="mu")
    with pytest.raises(NotImplementedError, match="hals.*mu"):
        sparse_nmf.check_request(3, "hals", 2, unstored="missing")
    with pytest.raises(NotImplementedError, match="hals.*mu"):
        sparse_ntf.check_request(3, "hals", 2, 3, unstored="missing")
    for bad in (-1, -0.5, float("nan"), float("inf")):
        with pytest.raises(err.InvalidArgumentValue, match="beta"):
            sparse_nmf.check_request(3, "mu", bad, unstored="missing")
        with pytest.raises(err.InvalidArgumentValue, match="beta"):
            sparse_ntf.check_request(3, "mu", bad, 3, unstored="missing")
    for beta in (0, 0.5, 1, 1.5, 2, 3, 7.25):
        sparse_nmf.check_request(128, "mu", beta, unstored="missing")
        sparse_ntf.check_request(128, "mu", beta, 5, unstored="missing")
    with pytest.raises(NotImplementedError, match="beta"):      # the stored-zero reading keeps its refusal
        sparse_nmf.check_request(3, "mu", 0.5)

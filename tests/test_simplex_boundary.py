"""The Python boundary of simplex NMF without a GPU: refusals fire before the engine is reached, the signatures are the
reference's, the inputs are never modified, and the outer loop (nn_fac_amd.simplex_nmf.run_steps) gives the restatement's
factors, costs, iteration count and warnings when it runs on the engine double (tests/engine_double.py) on the CPU."""
import inspect
import warnings

import numpy as np
import pytest
import torch

import simplex_restatement as rs
from engine_double import OracleEngine


class SimplexDouble(OracleEngine):
    """The engine double + the simplex projection, from the restatement (fp64 on the CPU)."""

    def simplex_proj(self, H, num, den, den_vec, tol=1e-6, max_iter=100, lambda0=None, out=None, lambda_out=None, status=None,
                     update=True):
        C, Hn = num.numpy().astype(np.float64), H.numpy().astype(np.float64)
        D = den.numpy().astype(np.float64) if den is not None else den_vec.numpy().reshape(-1, 1) * np.ones_like(Hn)
        lam0 = lambda0.numpy().reshape(-1, 1) if lambda0 is not None else rs.lambda_start(C, D, Hn)
        info = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lam = rs.update_lagragian_multipliers_simplex_projection(C, D, Hn, 1, lam0, tol=tol, n_iter_max=max_iter, info=info)
        st = status if status is not None else torch.zeros(2, dtype=torch.float64)
        st[0], st[1] = float(info["count"]), float(info["deltas"][-1])
        if lambda_out is not None:
            lambda_out.copy_(torch.from_numpy(lam.ravel()))
        O = None
        if update:
            O = torch.from_numpy(rs.simplex_update(C, D, Hn, lam))
            if out is not None:
                O = out.copy_(O)
        return O, st


def the_engine_must_not_be_reached(monkeypatch):
    from nn_fac_amd import engine

    def boom(*a, **k):
        raise AssertionError("the engine was reached")
    monkeypatch.setattr(engine, "get_engine", boom)
    from nn_fac_amd import _convert
    monkeypatch.setattr(_convert, "device_of", boom)


@pytest.mark.parametrize("beta", (2, 0, 0.5, 1.5, 3, 1.0000001))
def test_every_beta_but_one_is_refused_before_the_engine(monkeypatch, beta):
    from nn_fac_amd import simplex_nmf as sx
    from nn_fac_amd.update_rules.mu import simplex_proj_mu
    from nn_fac_amd.utils.normalize_wh import update_lagragian_multipliers_simplex_projection
    the_engine_must_not_be_reached(monkeypatch)
    monkeypatch.setattr(sx, "device_of", lambda *a: pytest.fail("the device was asked for"))
    r = np.random.RandomState(0)
    X, W, H = r.rand(6, 7), r.rand(6, 2), r.rand(2, 7)
    calls = [lambda: sx.simplex_beta_nmf(X, 2, beta, n_iter_max=2),
             lambda: sx.simplex_beta_nmf(X, 2, beta, init="custom", W_0=W, H_0=H),
             lambda: sx.compute_simplex_beta_nmf(X, W, H, 2, beta),
             lambda: sx.one_step_simplex_beta_nmf(X, W, H, 2, beta, 1e-6),
             lambda: simplex_proj_mu(X, W, H, beta),
             lambda: update_lagragian_multipliers_simplex_projection(H, H, H, beta, np.zeros((7, 1)))]
    for f in calls:
        with pytest.raises(NotImplementedError, match="beta = 1 only"):
            f()


def test_custom_start_and_rank_checks_fire_before_the_engine(monkeypatch):
    from nn_fac_amd import simplex_nmf as sx
    from nn_fac_amd.utils import errors as err
    the_engine_must_not_be_reached(monkeypatch)
    monkeypatch.setattr(sx, "device_of", lambda *a: pytest.fail("the device was asked for"))
    r = np.random.RandomState(0)
    X, W, H = r.rand(6, 7), r.rand(6, 2), r.rand(2, 7)
    for kw in (dict(W_0=None, H_0=H), dict(W_0=W, H_0=None), dict()):
        with pytest.raises(err.CustomNotValidFactors):
            sx.simplex_beta_nmf(X, 2, 1, init="custom", **kw)
        with pytest.raises(err.CustomNotValidFactors):
            sx.simplex_beta_nmf(X, 2, 1, init="CUSTOM", **kw)
    with pytest.raises(err.InvalidInitializationType):
        sx.simplex_beta_nmf(X, 2, 1, init="invalid_init")
    with pytest.raises(err.EngineError, match="rank 129 is above the 128"):
        sx.compute_simplex_beta_nmf(r.rand(130, 131), r.rand(130, 129), r.rand(129, 131), 129, 1)
    with pytest.raises(err.EngineError, match="rank 129 is above the 128"):
        sx.one_step_simplex_beta_nmf(r.rand(130, 131), r.rand(130, 129), r.rand(129, 131), 129, 1, 1e-6)
    assert (X, W, H) is not None


def test_signatures_are_the_reference_s():
    from nn_fac_amd import simplex_nmf as sx
    from nn_fac_amd.update_rules.mu import simplex_proj_mu
    from nn_fac_amd.utils.normalize_wh import update_lagragian_multipliers_simplex_projection

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(sx.simplex_beta_nmf) == [("data", E), ("rank", E), ("beta", E), ("n_iter_max", 100), ("tol", 1e-8),
                                        ("tol_update_lagrangian", 1e-6), ("init", "random"), ("W_0", None), ("H_0", None),
                                        ("verbose", False), ("deterministic", False), ("seed", 0)]
    assert sig(sx.compute_simplex_beta_nmf) == [("data", E), ("W_0", E), ("H_0", E), ("rank", E), ("beta", E), ("n_iter_max", 100),
                                                ("tol", 1e-8), ("tol_update_lagrangian", 1e-6), ("verbose", False)]
    assert sig(sx.one_step_simplex_beta_nmf) == [("data", E), ("W", E), ("H", E), ("rank", E), ("beta", E),
                                                 ("tol_update_lagrangian", E)]
    assert sig(simplex_proj_mu) == [("data", E), ("W", E), ("H", E), ("beta", E), ("tol_update_lagrangian", 1e-6)]
    assert sig(update_lagragian_multipliers_simplex_projection) == [("C", E), ("D", E), ("H", E), ("beta", E),
                                                                    ("lagrangian_multipliers_0", E), ("tol", 1e-6), ("n_iter_max", 100)]
    assert sx.eps == 1e-12 and sx.NEWTON_WARNING == rs.WARNING


def test_engine_simplex_proj_signature_matches_the_double():
    from nn_fac_amd.engine import Engine
    want = [(p.name, p.kind, p.default) for p in inspect.signature(Engine.simplex_proj).parameters.values()]
    got = [(p.name, p.kind, p.default) for p in inspect.signature(SimplexDouble.simplex_proj).parameters.values()]
    assert got == want


@pytest.mark.parametrize("tol,n_costs", ((0, 8), (400.0, 5)))
def test_outer_loop_on_the_engine_double(golden, tol, n_costs):
    """run_steps on the CPU double: the reference's factors, costs, iteration count (the steps enqueued behind the one that
    stops the loop are dropped) and one warning per iteration whose Newton solve ran out of iterations; inputs untouched."""
    from nn_fac_amd import simplex_nmf as sx
    from nn_fac_amd import _outer_loop as loop
    g = golden("g12_simplex.npz")
    X, W0, H0 = (torch.from_numpy(g["a_" + k].astype(np.float64)) for k in ("X", "W0", "H0"))
    Ut0 = W0.t().contiguous()
    keep = (X.clone(), Ut0.clone(), H0.clone())
    retired = loop.Retired(tol)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        Ut, V = sx.run_steps(SimplexDouble(), X, Ut0, H0, 8, 1e-6, retired)
    assert all(torch.equal(a, b) for a, b in zip(keep, (X, Ut0, H0)))
    assert len(retired.cost_fct_vals) == len(retired.toc) == n_costs
    assert np.allclose(retired.cost_fct_vals, g["a_costs"][:n_costs], rtol=1e-10, atol=0)
    last = n_costs - 1
    assert np.allclose(Ut.numpy().T, g[f"a_W_it{last}"], rtol=1e-9, atol=0) and np.allclose(V.numpy(), g[f"a_H_it{last}"], rtol=1e-9, atol=0)
    assert [str(x.message) for x in w] == [rs.WARNING] * int(g["a_warned"][:n_costs].sum()) and len(w) == 1

"""nn_fac_amd.parafac2 on the device against the real reference's outputs (tests/golden/g11_parafac2.npz).  Needs a MI355X,
except the last test (exceptions are raised before the device is touched).

Bounds.  One step: factors, P_k, W* and mu at 2e-4, cost at 1e-4, sweep counts and increasing_mu equal.  Eight iterations:
per quantity max(2e-4, 10 s), s = the reference's own fp32-vs-fp64 sensitivity stored with the run (the factor 10 covers a
different fp32 summation order compounding over 8 alternations)."""
import math

import numpy as np
import pytest
import torch

from test_parafac2_golden import diags, load_problem, rel, stack

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def p2(built_lib):
    from nn_fac_amd import parafac2
    assert torch.cuda.is_available()
    return parafac2


def one_step(p2, pb, withP, **kw):
    return p2.one_step_parafac2(pb["slices"], pb["r"], pb["W0"], pb["H0"], pb["D0"], pb["mu0"], pb["norm_slices"], pb["prev"],
                                increasing_mu=True, init_with_P=withP, P_list_in=pb["P0"] if withP else None,
                                W_star_in=None if withP else pb["Ws0"], alpha=math.inf, **kw)


@gpu
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("withP", [True, False])
def test_one_step_against_the_reference(golden, p2, name, withP):
    g = golden("g11_parafac2.npz")
    pb = load_problem(g, name)
    p = f"{name}_{'P' if withP else 'S'}_"
    out = one_step(p2, pb, withP)
    info = dict(p2.LAST_STEP_INFO)
    want_P = g[p + "step_P"] if not withP else stack(pb["P0"])
    figs = dict(W=rel(stack(out[0]), g[p + "step_W"]), H=rel(out[1], g[p + "step_H"]), D=rel(diags(out[2]), g[p + "step_D"]),
                Ws=rel(out[3], g[p + "step_Ws"]), P=rel(stack(out[4]), want_P), mu=rel(out[5], g[p + "step_mu"]),
                ce=rel(out[7], g[p + "step_ce"]), cost=abs(out[6] - float(g[p + "step_cost"])) / float(g[p + "step_cost"]))
    print(p, figs, info)
    assert all(isinstance(w, np.ndarray) and w.dtype == np.float64 for w in out[0]) and out[2][0].shape == (pb["r"], pb["r"])
    assert max(figs[k] for k in ("W", "H", "D", "Ws", "P", "mu", "ce")) <= 2e-4, figs
    assert figs["cost"] <= 1e-4, figs
    assert np.array_equal(info["cnt_W"], g[p + "step_cntW"]) and np.array_equal(info["cnt_D"], g[p + "step_cntD"])
    assert info["cnt_H"] == int(g[p + "step_cntH"]) and bool(out[8]) == bool(g[p + "step_inc"])


@gpu
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("withP", [True, False])
def test_eight_iterations_against_the_reference(golden, p2, name, withP):
    g = golden("g11_parafac2.npz")
    pb = load_problem(g, name)
    p = f"{name}_{'P' if withP else 'S'}_"
    W, H, D, costs, toc = p2.compute_parafac_2(pb["slices"], pb["r"], pb["W0"], pb["H0"], pb["D0"], withP,
                                               W_star_in=None if withP else pb["Ws0"], P_list_in=pb["P0"] if withP else None,
                                               n_iter_max=8, tol=0, return_costs=True, alpha=math.inf)
    s = g[p + "run_s"]
    want_c = g[p + "run_costs"]
    figs = np.array([rel(stack(W), g[p + "run_W"]), rel(H, g[p + "run_H"]), rel(diags(D), g[p + "run_D"]),
                     abs(costs[-1] - want_c[-1]) / want_c[-1]])
    bound = np.maximum(2e-4, 10 * s)
    print(p, "achieved (W, H, D, cost):", figs, "bound:", bound, "s:", s)
    assert len(costs) == 8 and len(toc) == 8
    assert (figs <= bound).all(), (figs, bound)


@gpu
def test_random_start_against_the_reference(golden, p2):
    g = golden("g11_parafac2.npz")
    K, m, n, r, seed = (int(v) for v in g["r_shape"])
    X = g["r_X"].astype(np.float64)
    slices = [X[k * m:(k + 1) * m] for k in range(K)]
    W, H, D, costs, _ = p2.parafac_2(slices, r, True, init="random", n_iter_max=8, tol=0, return_costs=True, deterministic=True,
                                     seed=seed)
    s = g["r_run_s"]
    figs = np.array([rel(stack(W), g["r_run_W"]), rel(H, g["r_run_H"]), rel(diags(D), g["r_run_D"]),
                     abs(costs[-1] - g["r_run_costs"][-1]) / g["r_run_costs"][-1]])
    print("random start, achieved (W, H, D, cost):", figs, "s:", s)
    assert isinstance(D, np.ndarray) and D.shape == (K, r, r)        # (the random start hands D_list over as one array)
    assert (figs <= np.maximum(2e-4, 10 * s)).all(), figs


@gpu
@pytest.mark.parametrize("withP", [True, False])
def test_grouped_and_per_slice_routes_agree(golden, p2, withP, monkeypatch):
    pb = load_problem(golden("g11_parafac2.npz"), "b")
    grouped = one_step(p2, pb, withP)
    cg = dict(p2.LAST_STEP_INFO)
    monkeypatch.setenv("NNF_PARAFAC2_PER_SLICE", "1")
    single = one_step(p2, pb, withP)
    cs = dict(p2.LAST_STEP_INFO)
    figs = [rel(stack(grouped[i]), stack(single[i])) for i in (0, 4)] + [rel(grouped[i], single[i]) for i in (1, 3, 5, 7)] + \
        [rel(diags(grouped[2]), diags(single[2])), abs(grouped[6] - single[6]) / single[6]]
    print("grouped vs per-slice:", figs)
    assert max(figs) <= 2e-4, figs
    assert np.array_equal(cg["cnt_W"], cs["cnt_W"]) and np.array_equal(cg["cnt_D"], cs["cnt_D"]) and cg["cnt_H"] == cs["cnt_H"]


@gpu
def test_random_start_without_P_is_well_formed(p2):
    """init_with_P=False from the random start: W* is m x r, so A_k = W_k W*^T is rank-deficient and the reference's P_k depends
    on LAPACK's basis of the null space -- parity is not defined; the properties are."""
    rng = np.random.RandomState(5)
    K, m, n, r = 4, 12, 20, 3
    slices = [rng.rand(m, r) @ rng.rand(r, n) for _ in range(K)]
    W, H, D = p2.parafac_2(slices, r, False, init="random", n_iter_max=3, tol=0, deterministic=True, seed=1)
    assert len(W) == K and all(w.shape == (m, r) for w in W) and H.shape == (r, n) and np.asarray(D).shape == (K, r, r)
    for a in list(W) + [H, np.asarray(D)]:
        assert np.isfinite(a).all() and (a >= 0).all()
    from nn_fac_amd.utils.initialize_factors import parafac2_initialization
    W0, _, _, _, Ws = parafac2_initialization(slices, r, "random", False, deterministic=True, seed=1)
    for P in p2.compute_P_k(W0, Ws, K):
        assert P.shape == (m, m) and np.isfinite(P).all()
        assert np.abs(P.T @ P - np.eye(m)).max() <= 1e-5


@gpu
def test_device_tensors_in_device_tensors_out(golden, p2):
    pb = load_problem(golden("g11_parafac2.npz"), "a")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()   # noqa: E731
    W, H, D = p2.compute_parafac_2([d(x) for x in pb["slices"]], pb["r"], [d(w) for w in pb["W0"]], d(pb["H0"]),
                                   [d(x) for x in pb["D0"]], True, P_list_in=[d(x) for x in pb["P0"]], n_iter_max=2, tol=0,
                                   alpha=math.inf)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in list(W) + [H] + list(D))
    assert [tuple(w.shape) for w in W] == [(m, pb["r"]) for m in pb["rows"]] and tuple(D[0].shape) == (pb["r"], pb["r"])
    assert torch.count_nonzero(D[0] - torch.diag(torch.diagonal(D[0]))) == 0


@gpu
def test_options_are_wired(golden, p2):
    """sparsity, the normalisations and fixed modes against the fp64 restatement after one step (alpha = inf)."""
    import parafac2_restatement as rs
    pb = load_problem(golden("g11_parafac2.npz"), "a")
    D0 = np.array(pb["D0"])
    for kw in (dict(sparsity_coefficient=0.3), dict(normalize=[False, True, True, False, False]), dict(fixed_modes=[0]),
               dict(fixed_modes=[1, 2]), dict(fixed_modes=[4]), dict(normalize=[True, False, False, False, False])):
        args = (pb["slices"], pb["r"], pb["W0"], pb["H0"], D0, pb["mu0"], pb["norm_slices"], pb["prev"])
        com = dict(increasing_mu=True, init_with_P=True, P_list_in=pb["P0"], alpha=math.inf, **kw)
        want = rs.one_step_parafac2(*args, **com)
        got = p2.one_step_parafac2(*args, **com)
        figs = [rel(stack(got[i]), stack(want[i])) for i in (0, 4)] + [rel(got[i], want[i]) for i in (1, 3, 5, 7)] + \
            [rel(diags(got[2]), diags(want[2])), abs(got[6] - want[6]) / want[6]]
        print(kw, figs)
        assert max(figs) <= 2e-4, (kw, figs)


@gpu
def test_slices_longer_than_the_grouped_cap(p2):
    """Slices above Engine.hals_group_max_columns go through the single solve, the others through the grouped one, in one step."""
    import parafac2_restatement as rs
    rng = np.random.RandomState(9)
    rows, n, r = [9000, 40, 8200, 130], 10, 3
    Ht, Wst = rng.rand(r, n), rng.rand(r, r)
    slices, W0, D0 = [], [], []
    for m in rows:
        Q, _ = np.linalg.qr(rng.randn(m, r))
        slices.append((np.abs(Q @ Wst) @ np.diag(0.5 + rng.rand(r)) @ Ht + 0.01 * rng.rand(m, n)).astype(np.float32).astype(np.float64))
        W0.append(rng.rand(m, r).astype(np.float32).astype(np.float64))
        D0.append(np.diag(0.5 + rng.rand(r)).astype(np.float32).astype(np.float64))
    H0, Ws0 = rng.rand(r, n).astype(np.float32).astype(np.float64), rng.rand(r, r).astype(np.float32).astype(np.float64)
    norms = [np.linalg.norm(x) for x in slices]
    mu0 = [np.linalg.norm(slices[k] - W0[k] @ D0[k] @ H0) ** 2 / (10 * np.linalg.norm(W0[k]) ** 2) for k in range(len(rows))]
    com = dict(increasing_mu=True, init_with_P=False, W_star_in=Ws0, alpha=math.inf)
    want = rs.one_step_parafac2(slices, r, W0, H0, D0, mu0, norms, 1e9, **com)
    got = p2.one_step_parafac2(slices, r, W0, H0, D0, mu0, norms, 1e9, **com)
    figs = [rel(stack(got[i]), stack(want[i])) for i in (0, 4)] + [rel(got[i], want[i]) for i in (1, 3, 5, 7)] + \
        [rel(diags(got[2]), diags(want[2])), abs(got[6] - want[6]) / want[6]]
    print("long slices:", figs)
    assert max(figs) <= 2e-4, figs


@gpu
def test_wall_clock_rule_runs(golden, p2):
    """Finite alpha (the reference's 0.5): one probe sweep per launch sets one budget for all its groups.  The counts then depend
    on the clock, so only properties are asserted."""
    pb = load_problem(golden("g11_parafac2.npz"), "b")
    W, H, D, costs, _ = p2.compute_parafac_2(pb["slices"], pb["r"], pb["W0"], pb["H0"], pb["D0"], True, P_list_in=pb["P0"],
                                             n_iter_max=3, tol=0, return_costs=True)
    for a in list(W) + [H] + list(D):
        assert np.isfinite(a).all() and (a >= 0).all()
    assert len(costs) == 3 and np.isfinite(costs).all()
    assert (p2.LAST_STEP_INFO["cnt_W"] >= 2).all() and (p2.LAST_STEP_INFO["cnt_D"] >= 2).all()


def test_exceptions_are_raised_before_the_device_is_touched():
    """No GPU needed: every refusal below comes from the arguments alone."""
    from nn_fac_amd import parafac2 as p2
    from nn_fac_amd.utils import errors as err
    rng = np.random.RandomState(0)
    slices = [rng.rand(9, 7), rng.rand(5, 7)]
    W, D, H = [rng.rand(9, 3), rng.rand(5, 3)], [np.eye(3), np.eye(3)], rng.rand(3, 7)
    P = [np.eye(9)[:, :3], np.eye(5)[:, :3]]
    with pytest.raises(err.CustomNotValidFactors):
        p2.parafac_2(slices, 3, True, init="custom", W_list_in=W, H=None, D_list_in=D)
    with pytest.raises(err.CustomNotValidFactors):
        p2.compute_parafac_2(slices, 3, W, H, D, True)
    with pytest.raises(ValueError):
        p2.one_step_parafac2(slices, 3, W, H, D, [1.0, 1.0], [1.0, 1.0], None, init_with_P=True, W_star_in=rng.rand(3, 3))
    with pytest.raises(ValueError):
        p2.one_step_parafac2(slices, 3, W, H, D, [1.0, 1.0], [1.0, 1.0], None, init_with_P=False, P_list_in=P)
    with pytest.raises(ValueError):
        p2.one_step_parafac2(slices, 3, W, H, D, [1.0, 1.0], [1.0, 1.0], None)
    with pytest.raises(NotImplementedError, match="139-156"):
        p2.parafac_2(slices, 3, True, init="nndsvd")
    with pytest.raises(err.EngineError, match="rank 129"):
        p2.compute_parafac_2([rng.rand(200, 7)], 129, [rng.rand(200, 129)], rng.rand(129, 7), [np.eye(129)], True,
                             P_list_in=[np.eye(200)[:, :129]])
    with pytest.raises(err.InvalidArgumentValue):          # a slice shorter than W* has rows
        p2.compute_parafac_2(slices, 3, W, H, D, False, W_star_in=rng.rand(6, 3))
    with pytest.raises(err.ArgumentException):
        p2.compute_parafac_2(slices, 3, W, rng.rand(3, 8), D, True, P_list_in=P)

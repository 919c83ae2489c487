"""tests/parafac2_restatement.py (the fp64 ground truth of the PARAFAC2 driver) against the real reference's outputs stored in
tests/golden/g11_parafac2.npz (tools/gen_golden_parafac2.py), at 1e-10.  No GPU."""
import math

import numpy as np
import pytest

import parafac2_restatement as rs

TOL = 1e-10


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def load_problem(g, name):
    """The custom-start problem `name` of the fixture as the reference's lists (float64)."""
    rows = [int(v) for v in g[f"{name}_rows"]]
    off = np.concatenate([[0], np.cumsum(rows)])
    cut = lambda a: [np.asarray(a[off[k]:off[k + 1]], dtype=np.float64) for k in range(len(rows))]   # noqa: E731
    return dict(rows=rows, off=off, r=int(g[f"{name}_rank"]), slices=cut(g[f"{name}_X"]), W0=cut(g[f"{name}_W0"]),
                P0=cut(g[f"{name}_P0"]), D0=[np.diag(d.astype(np.float64)) for d in g[f"{name}_D0"]],
                H0=g[f"{name}_H0"].astype(np.float64), Ws0=g[f"{name}_Ws0"].astype(np.float64), mu0=g[f"{name}_mu0"],
                prev=float(g[f"{name}_prev"]), norm_slices=[np.linalg.norm(x, ord='fro') for x in cut(g[f"{name}_X"])])


def stack(lst):
    return np.concatenate([np.asarray(x) for x in lst], axis=0)


def diags(D_list):
    return np.array([np.diagonal(np.asarray(D)) for D in D_list])


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("withP", [True, False])
def test_one_step_matches_the_reference(golden, name, withP):
    g = golden("g11_parafac2.npz")
    pb = load_problem(g, name)
    p = f"{name}_{'P' if withP else 'S'}_"
    info = {}
    out = rs.one_step_parafac2(pb["slices"], pb["r"], pb["W0"], pb["H0"], pb["D0"], pb["mu0"], pb["norm_slices"], pb["prev"],
                               increasing_mu=True, init_with_P=withP, P_list_in=pb["P0"] if withP else None,
                               W_star_in=None if withP else pb["Ws0"], alpha=math.inf, info=info)
    assert rel(stack(out[0]), g[p + "step_W"]) < TOL and rel(out[1], g[p + "step_H"]) < TOL
    assert rel(diags(out[2]), g[p + "step_D"]) < TOL and rel(out[3], g[p + "step_Ws"]) < TOL
    assert rel(stack(out[4]), g[p + "step_P"] if not withP else stack(pb["P0"])) < TOL
    assert rel(out[5], g[p + "step_mu"]) < TOL and rel(out[6], g[p + "step_cost"]) < TOL and rel(out[7], g[p + "step_ce"]) < TOL
    assert bool(out[8]) == bool(g[p + "step_inc"])
    assert np.array_equal(info["cnt_W"], g[p + "step_cntW"]) and np.array_equal(info["cnt_D"], g[p + "step_cntD"])
    assert info["cnt_H"] == int(g[p + "step_cntH"])


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("withP", [True, False])
def test_eight_iterations_match_the_reference(golden, name, withP):
    g = golden("g11_parafac2.npz")
    pb = load_problem(g, name)
    p = f"{name}_{'P' if withP else 'S'}_"
    out = rs.compute_parafac_2(pb["slices"], pb["r"], pb["W0"], pb["H0"], pb["D0"], withP, W_star_in=None if withP else pb["Ws0"],
                               P_list_in=pb["P0"] if withP else None, n_iter_max=8, tol=0, return_costs=True, alpha=math.inf)
    assert rel(stack(out[0]), g[p + "run_W"]) < TOL and rel(out[1], g[p + "run_H"]) < TOL
    assert rel(diags(out[2]), g[p + "run_D"]) < TOL and rel(out[3], g[p + "run_costs"]) < TOL
    assert g[p + "run_s"].shape == (4,) and (g[p + "run_s"] < 1e-3).all()      # the reference's own fp32 sensitivity is tame here


def test_random_start_matches_the_reference(golden):
    g = golden("g11_parafac2.npz")
    K, m, n, r, seed = (int(v) for v in g["r_shape"])
    X = g["r_X"].astype(np.float64)
    slices = [X[k * m:(k + 1) * m] for k in range(K)]
    W, H, D, P, Ws = rs.parafac2_initialization(slices, r, "random", True, deterministic=True, seed=seed)
    out = rs.compute_parafac_2(slices, r, W, H, D, True, W_star_in=Ws, P_list_in=P, n_iter_max=8, tol=0, return_costs=True,
                               alpha=math.inf)
    assert rel(stack(out[0]), g["r_run_W"]) < TOL and rel(out[1], g["r_run_H"]) < TOL
    assert rel(diags(out[2]), g["r_run_D"]) < TOL and rel(out[3], g["r_run_costs"]) < TOL


def test_fixture_is_small(golden):
    import os
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "g11_parafac2.npz")) < 500_000

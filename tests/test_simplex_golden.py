"""tests/simplex_restatement.py -- what the device kernels of simplex NMF are compared with -- pinned to the real reference's own
results (tests/golden/g12_simplex.npz, written by tools/gen_golden_simplex.py) at 1e-12, without a GPU."""
import warnings

import numpy as np
import pytest

import simplex_restatement as rs

RUNS = ("a", "b", "c", "d")
SHAPES = {"a": (100, 200, 5), "b": (70, 67, 19), "c": (130, 97, 50), "d": (90, 130, 100)}
N_ITER = 8


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def caught(fn, *a, **k):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = fn(*a, **k)
    return out, [str(x.message) for x in w]


@pytest.fixture(scope="module")
def g12(golden):
    return golden("g12_simplex.npz")


def f64(g, key):
    return g[key].astype(np.float64)


@pytest.mark.parametrize("name", ("p0", "p1", "p2"))
def test_simplex_proj_mu_calls(g12, name):
    info = {}
    out, msgs = caught(rs.simplex_proj_mu, f64(g12, name + "_X"), f64(g12, name + "_W"), f64(g12, name + "_H"), 1, info=info)
    assert relmax(out, g12[name + "_out"]) < 1e-12
    assert info["count"] == int(g12[name + "_count"]) and info["warned"] == bool(g12[name + "_warned"])
    assert msgs == ([rs.WARNING] if info["warned"] else [])


@pytest.mark.parametrize("name,count", (("m", None), ("n", 100)))
def test_multiplier_calls(g12, name, count):
    """The multiplier function alone, from given start values: a call that converges and one that runs all 100 iterations."""
    info = {}
    lam, msgs = caught(rs.update_lagragian_multipliers_simplex_projection, f64(g12, name + "_C"), f64(g12, name + "_D"),
                       f64(g12, name + "_H"), 1, g12[name + "_lam0"].reshape(-1, 1), info=info)
    assert lam.shape == (g12[name + "_H"].shape[1], 1) and relmax(lam.ravel(), g12[name + "_lam"]) < 1e-12
    assert info["count"] == int(g12[name + "_count"])
    if count is not None:
        assert info["count"] == count and info["warned"] and msgs == [rs.WARNING]
        assert info["deltas"][-1] == float(g12["n_last"]) > 1e-6
    else:
        assert not info["warned"] and not msgs and info["count"] < 100
    # the start values are mu.py:168 on the same operands
    assert relmax(rs.lambda_start(f64(g12, name + "_C"), f64(g12, name + "_D"), f64(g12, name + "_H")).ravel(), g12[name + "_lam0"]) < 1e-12


@pytest.mark.parametrize("name", RUNS)
def test_runs(g12, name):
    m, n, r = SHAPES[name]
    X, W0, H0 = f64(g12, name + "_X"), f64(g12, name + "_W0"), f64(g12, name + "_H0")
    assert X.shape == (m, n) and W0.shape == (m, r) and H0.shape == (r, n) and int(g12[name + "_rank"]) == r
    keep = (X.copy(), W0.copy(), H0.copy())
    infos = []
    (W, H, costs, toc), msgs = caught(rs.compute_simplex_beta_nmf, X, W0, H0, r, 1, n_iter_max=N_ITER, tol=0, infos=infos)
    assert all((a == b).all() for a, b in zip(keep, (X, W0, H0)))
    assert len(costs) == len(toc) == N_ITER
    assert relmax(W, g12[name + "_W"]) < 1e-12 and relmax(H, g12[name + "_H"]) < 1e-12 and relmax(costs, g12[name + "_costs"]) < 1e-12
    assert [i["count"] for i in infos] == g12[name + "_counts"].tolist()
    assert [i["warned"] for i in infos] == g12[name + "_warned"].tolist() and len(msgs) == int(g12[name + "_warned"].sum())
    # what the device tests lean on: the second step runs all 100 Newton iterations, and the columns of H are on the simplex
    assert infos[1]["count"] == 100 and infos[1]["warned"]
    assert np.max(np.abs(H.sum(axis=0) - 1)) < 1e-6


def test_run_a_iterates_and_early_stop(g12):
    X, W0, H0 = f64(g12, "a_X"), f64(g12, "a_W0"), f64(g12, "a_H0")
    W, H = W0, H0
    for t in range(N_ITER):
        (W, H, cost), _ = caught(rs.one_step_simplex_beta_nmf, X, W, H, 5, 1, 1e-6)
        assert relmax(W, g12[f"a_W_it{t}"]) < 1e-12 and relmax(H, g12[f"a_H_it{t}"]) < 1e-12
        assert abs(cost - g12["a_costs"][t]) <= 1e-12 * abs(cost)
    (W, H, costs, _), _ = caught(rs.compute_simplex_beta_nmf, X, W0, H0, 5, 1, n_iter_max=N_ITER, tol=400.0)
    assert len(costs) == 5 and relmax(W, g12["a_W_it4"]) < 1e-12 and relmax(H, g12["a_H_it4"]) < 1e-12


def test_other_betas_are_not_restated():
    with pytest.raises(NotImplementedError):
        rs.simplex_proj_mu(np.ones((3, 4)), np.ones((3, 2)), np.ones((2, 4)), 2)

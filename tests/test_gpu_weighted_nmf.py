"""nmf / compute_nmf / one_nmf_step with `weights=` (nn_fac_amd/weighted_nmf.py: multiplicative updates of any beta >= 0 with a weight
per entry of dense data) against the fp64 restatement of tests/weighted_restatement.py, at the project's MU tolerances
(tests/test_gpu_observed_drivers.py): rel_fro <= 5e-5 on every factor, cost rtol 1e-4.  Five iterations, tol = 0, beta in 0, 0.5, 1,
2, 3, on 300 x 200 at rank 7 (weights uniform in (0, 2) with 25 % zeros, a zero row, a zero column, NaN under the zeros) and
2000 x 300 at rank 70 (start values scaled so that U V is of the size of the data).  Needs a MI355X.

Then the agreement with the paths that exist: a boolean mask against observed_entries(X, mask) + unstored="missing" (two device paths
for one formula: 2 TOL_F), all-ones weights against weights=None (TOL_F), and weights=None itself bit for bit against arrays saved
from the commit before the keyword existed (tests/golden/weighted_nmf_parent.npz).  Then the behaviour of the keyword (fixed_modes,
the caller's arrays, device tensors, slices without weight, NaN against 0 under a mask) and the recovery recipe of
tests/test_weighted_restatement.py on the device."""
import os

import numpy as np
import pytest
import torch

import weighted_restatement as wr

pytestmark = pytest.mark.gpu

TOL_F, TOL_C = 5e-5, 1e-4
N_ITER = 5
BETAS = (0, 0.5, 1, 2, 3)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weighted_nmf_parent.npz")


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def problem(name):
    """(X, Wg, r, U0, V0), every value exactly representable in fp32; X holds NaN where the weight is zero."""
    (m, n), r = ((300, 200), 7) if name == "300x200" else ((2000, 300), 70)
    rng = np.random.default_rng(11 if name == "300x200" else 12)
    X = f32(rng.random((m, n)) + 0.1)
    Wg = f32(rng.random((m, n)) * 2)
    Wg[rng.random((m, n)) < 0.25] = 0
    Wg[7, :] = 0
    Wg[:, 11] = 0
    X[Wg == 0] = np.nan
    s = 2 * np.sqrt(0.6 / r)
    return X, Wg, r, f32(rng.random((m, r)) * s + 0.01), f32(rng.random((r, n)) * s + 0.01)


_references = {}


def reference(name, beta, fixed=()):
    key = (name, beta, tuple(fixed))
    if key not in _references:
        X, Wg, r, U0, V0 = problem(name)
        _references[key] = wr.run(X, Wg, U0, V0, N_ITER, beta, fixed_modes=fixed)
    return _references[key]


def check(tag, got, want):
    U, V, costs = got[:3]
    Ur, Vr, cr = want
    print(tag, "rel", rel(U, Ur), rel(V, Vr), "cost", costs[-1], cr[-1])
    assert len(costs) == N_ITER and U.shape == Ur.shape and V.shape == Vr.shape
    assert rel(U, Ur) <= TOL_F and rel(V, Vr) <= TOL_F, tag
    assert np.allclose(costs, cr, rtol=TOL_C, atol=0), (tag, costs, cr)


@pytest.mark.parametrize("name", ["300x200", "2000x300"])
@pytest.mark.parametrize("beta", BETAS)
def test_five_iterations_against_the_restatement(built_lib, name, beta):
    from nn_fac_amd.nmf import nmf, compute_nmf, one_nmf_step
    X, Wg, r, U0, V0 = problem(name)
    keep = [a.copy() for a in (X, Wg, U0, V0)]
    got = compute_nmf(X, r, U0, V0, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True, weights=Wg)
    assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray) and len(got[3]) == N_ITER
    for a, b in zip((X, Wg, U0, V0), keep):      # the caller's arrays are not modified
        assert np.array_equal(a, b, equal_nan=True)
    check((name, beta), got, reference(name, beta))
    # a slice without weight holds its start value exactly; its neighbour does not
    assert np.array_equal(got[0][7], U0[7]) and np.array_equal(got[1][:, 11], V0[:, 11])
    assert not np.array_equal(got[0][8], U0[8]) and not np.array_equal(got[1][:, 12], V0[:, 12])
    # nmf() with custom start values is the same run; one_nmf_step is its first iteration
    again = nmf(X, r, init="custom", U_0=U0, V_0=V0, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True,
                weights=Wg)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and list(again[2]) == list(got[2])
    U1, V1, c1 = one_nmf_step(X, r, U0, V0, None, "mu", beta, [None, None], [], [False, False], True, weights=Wg)
    assert c1 == got[2][0]
    first = compute_nmf(X, r, U0, V0, n_iter_max=1, tol=0, update_rule="mu", beta=beta, weights=Wg)
    assert np.array_equal(U1, first[0]) and np.array_equal(V1, first[1])


@pytest.mark.parametrize("beta", (0.5, 1, 2))
def test_boolean_mask_agrees_with_the_observed_entries_path(built_lib, beta):
    from nn_fac_amd.sparse_nmf import observed_entries
    from nn_fac_amd.nmf import compute_nmf
    X, Wg, r, U0, V0 = problem("300x200")
    mask = Wg != 0
    kw = dict(n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True)
    got = compute_nmf(X, r, U0, V0, weights=mask, **kw)
    want = compute_nmf(observed_entries(np.nan_to_num(X), mask), r, U0, V0, unstored="missing", **kw)
    print("mask vs observed entries", beta, rel(got[0], want[0]), rel(got[1], want[1]))
    assert rel(got[0], want[0]) <= 2 * TOL_F and rel(got[1], want[1]) <= 2 * TOL_F
    assert np.allclose(got[2], want[2], rtol=2 * TOL_C, atol=0)
    # X[~mask] = nan gives what X[~mask] = 0 gives, bit for bit; a float 0/1 array is the mask
    zero = compute_nmf(np.nan_to_num(X), r, U0, V0, weights=mask, **kw)
    assert np.array_equal(zero[0], got[0]) and np.array_equal(zero[1], got[1]) and list(zero[2]) == list(got[2])
    same = compute_nmf(X, r, U0, V0, weights=mask.astype(np.float32), **kw)
    assert np.array_equal(same[0], got[0]) and np.array_equal(same[1], got[1])


def golden_problem():
    rng = np.random.default_rng(21)
    return f32(rng.random((300, 200)) + 0.1), 7, f32(rng.random((300, 7)) + 0.05), f32(rng.random((7, 200)) + 0.05)


GOLDEN_RUNS = {"mu_b1": dict(update_rule="mu", beta=1), "mu_b05": dict(update_rule="mu", beta=0.5), "mu_b2": dict(update_rule="mu", beta=2)}


def golden_run(tag, **kw):
    """One run of the golden problem: (U, V, costs) as float32 / float64 arrays (tests/golden/weighted_nmf_parent.npz holds these
    from the commit before the keyword existed)."""
    from nn_fac_amd.nmf import compute_nmf
    X, r, U0, V0 = golden_problem()
    U, V, costs, _ = compute_nmf(X, r, U0, V0, n_iter_max=N_ITER, tol=0, return_costs=True, deterministic=True, **GOLDEN_RUNS[tag], **kw)
    return U.astype(np.float32), V.astype(np.float32), np.asarray(costs, np.float64)


@pytest.mark.parametrize("tag", list(GOLDEN_RUNS))
def test_weights_none_is_bitwise_the_parent(built_lib, tag):
    saved = np.load(GOLDEN, allow_pickle=False)
    U, V, costs = golden_run(tag, weights=None)
    assert np.array_equal(U, saved[tag + "_U"]) and np.array_equal(V, saved[tag + "_V"])
    assert np.array_equal(costs, saved[tag + "_costs"])


@pytest.mark.parametrize("beta", BETAS)
def test_all_ones_agree_with_no_weights(built_lib, beta):
    from nn_fac_amd.nmf import compute_nmf
    X, r, U0, V0 = golden_problem()
    kw = dict(n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True)
    a = compute_nmf(X, r, U0, V0, **kw)
    b = compute_nmf(X, r, U0, V0, weights=np.ones_like(X), **kw)
    print("all ones vs None", beta, rel(b[0], a[0]), rel(b[1], a[1]))
    assert rel(b[0], a[0]) <= TOL_F and rel(b[1], a[1]) <= TOL_F and np.allclose(b[2], a[2], rtol=TOL_C, atol=0)


@pytest.mark.parametrize("fixed", ([0], [1]))
def test_fixed_modes_are_honoured(built_lib, fixed):
    from nn_fac_amd.nmf import compute_nmf
    X, Wg, r, U0, V0 = problem("300x200")
    got = compute_nmf(X, r, U0, V0, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=1, return_costs=True, weights=Wg, fixed_modes=fixed)
    check(("fixed", fixed), got, reference("300x200", 1, fixed))
    assert np.array_equal(got[fixed[0]], (U0, V0)[fixed[0]])


def test_device_tensors_in_device_tensors_out_same_bits(built_lib):
    from nn_fac_amd.nmf import compute_nmf, one_nmf_step
    X, Wg, r, U0, V0 = problem("300x200")
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(a).to(dev, torch.float32) for a in (X, U0, V0, Wg)]
    keep = [a.clone() for a in t]
    kw = dict(n_iter_max=3, tol=0, update_rule="mu", beta=0.5, return_costs=True)
    want = compute_nmf(X, r, U0, V0, weights=Wg, **kw)
    got = compute_nmf(t[0], r, t[1], t[2], weights=t[3], **kw)
    assert all(isinstance(a, torch.Tensor) and a.device == dev and a.dtype == torch.float32 for a in got[:2])
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]) and list(got[2]) == list(want[2])
    for a, b in zip(t, keep):
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    # a boolean device mask, and a host mask next to device data
    m1 = compute_nmf(t[0], r, t[1], t[2], weights=t[3] != 0, **kw)
    m2 = compute_nmf(t[0], r, t[1], t[2], weights=Wg != 0, **kw)
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])
    U1, V1, c1 = one_nmf_step(t[0], r, t[1], t[2], None, "mu", 0.5, [None, None], [], [False, False], True, weights=t[3])
    assert isinstance(U1, torch.Tensor) and U1.device == dev and c1 == want[2][0]


def test_bad_weight_values_are_refused_after_the_upload(built_lib):
    from nn_fac_amd.nmf import compute_nmf
    from nn_fac_amd.utils import errors as err
    X, Wg, r, U0, V0 = problem("300x200")
    for bad in (-0.5, np.nan, np.inf):
        w = Wg.copy()
        w[3, 4] = bad
        with pytest.raises(err.InvalidArgumentValue, match="finite and >= 0"):
            compute_nmf(X, r, U0, V0, n_iter_max=2, update_rule="mu", beta=1, weights=w)


@pytest.mark.parametrize("beta", (2, 1))
def test_recovery_on_the_device(built_lib, beta):
    """Weights = 1 / variance recover the truth that the unweighted fit misses: <= 0.02 against >= 0.05."""
    from nn_fac_amd.nmf import compute_nmf
    T, X, Wg, U0, V0 = wr.recovery_case(beta)
    kw = dict(n_iter_max=300, tol=0, update_rule="mu", beta=beta)
    Uw, Vw = compute_nmf(X, 3, U0, V0, weights=Wg, **kw)
    Un, Vn = compute_nmf(X, 3, U0, V0, **kw)
    ew, en = wr.recovery_error(T, Uw, Vw), wr.recovery_error(T, Un, Vn)
    print("recovery beta", beta, "with weights", ew, "without", en)
    assert ew <= 0.02 and en >= 0.05

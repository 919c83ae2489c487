"""ntf / compute_ntf / one_ntf_step with `weights=` (nn_fac_amd/weighted_ntf.py: multiplicative updates of any beta >= 0 with a weight
per entry of a dense tensor) against the fp64 restatement of tests/weighted_ntf_restatement.py, at the tolerances of
tests/test_gpu_weighted_nmf.py: rel_fro <= 5e-5 on every factor, cost rtol 1e-4.  Five iterations, tol = 0, beta in 0, 0.5, 1, 2, 3,
on 30 x 41 x 52 at rank 7 (order 3), 9 x 10 x 11 x 12 at rank 5 (order 4) and 40 x 30 x 70 at rank 70 (above the rank of the
on-layout kernel: the unfolded route); weights uniform in (0, 2) with 25 % zeros, a zero slice in each of two modes, NaN under the
zeros.  Needs a MI355X.

Then the agreement with the paths that exist: NNF_MU_UNFOLD=1 in a child process against the on-layout route and a boolean mask
against a SparseCOO of the masked entries with unstored="missing" (two device paths for one formula: 2 TOL_F), all-ones weights
against weights=None (TOL_F), and weights=None itself bit for bit against arrays saved from the commit before the keyword existed
(tests/golden/weighted_ntf_parent.npz, tools/gen_golden_weighted_ntf_parent.py).  Then the behaviour of the keyword (fixed_modes,
the caller's arrays, device tensors, slices without weight, NaN against 0 under a mask) and the recovery recipe of
tests/test_weighted_ntf_restatement.py on the device."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import weighted_ntf_restatement as wn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_F, TOL_C = 5e-5, 1e-4
N_ITER = 5
BETAS = (0, 0.5, 1, 2, 3)
GOLDEN = os.path.join(ROOT, "tests", "golden", "weighted_ntf_parent.npz")
PROBLEMS = {"order3": ((30, 41, 52), 7, 11), "order4": ((9, 10, 11, 12), 5, 12), "rank70": ((40, 30, 70), 70, 13)}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


_problems, _references = {}, {}


def problem(name):
    """(T, Wg, r, factors0), every value exactly representable in fp32; T holds NaN where the weight is zero.  Start values scaled
    so that the model is of the size of the data."""
    if name not in _problems:
        shape, r, seed = PROBLEMS[name]
        rng = np.random.default_rng(seed)
        T = f32(rng.random(shape) + 0.1)
        Wg = f32(rng.random(shape) * 2)
        Wg[rng.random(shape) < 0.25] = 0
        Wg[3] = 0                 # a slice of mode 0 without weight
        Wg[..., 5] = 0            # and one of the last mode
        T[Wg == 0] = np.nan
        s = (0.6 / r) ** (1.0 / len(shape)) * 2
        _problems[name] = T, Wg, r, [f32(rng.random((d, r)) * s + 0.01) for d in shape]
    return _problems[name]


def reference(name, beta, fixed=()):
    key = (name, beta, tuple(fixed))
    if key not in _references:
        T, Wg, r, F0 = problem(name)
        _references[key] = wn.run(T, Wg, F0, N_ITER, beta, fixed_modes=fixed)
    return _references[key]


def check(tag, got, want, tol_f=TOL_F, tol_c=TOL_C):
    F, costs = got[:2]
    Fr, cr = want[:2]
    print(tag, "rel", [rel(a, b) for a, b in zip(F, Fr)], "cost", costs[-1], cr[-1])
    assert len(costs) == len(cr) and all(a.shape == b.shape for a, b in zip(F, Fr))
    for i, (a, b) in enumerate(zip(F, Fr)):
        assert rel(a, b) <= tol_f, (tag, i, rel(a, b))
    assert np.allclose(costs, cr, rtol=tol_c, atol=0), (tag, costs, cr)


def run(name, beta, **kw):
    from nn_fac_amd.ntf import compute_ntf
    T, Wg, r, F0 = problem(name)
    kw.setdefault("weights", Wg)
    return compute_ntf(T, r, F0, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True, **kw)


@pytest.mark.parametrize("name", list(PROBLEMS))
@pytest.mark.parametrize("beta", BETAS)
def test_five_iterations_against_the_restatement(built_lib, monkeypatch, name, beta):
    from nn_fac_amd.ntf import ntf, compute_ntf, one_ntf_step
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    T, Wg, r, F0 = problem(name)
    N = T.ndim
    keep = [a.copy() for a in (T, Wg, *F0)]
    got = run(name, beta)
    assert all(isinstance(f, np.ndarray) for f in got[0]) and len(got[2]) == N_ITER
    for a, b in zip((T, Wg, *F0), keep):      # the caller's arrays are not modified
        assert np.array_equal(a, b, equal_nan=True)
    check((name, beta), got, reference(name, beta))
    # a slice without weight holds its start value exactly; its neighbour does not
    assert np.array_equal(got[0][0][3], F0[0][3]) and np.array_equal(got[0][-1][5], F0[-1][5])
    assert not np.array_equal(got[0][0][4], F0[0][4]) and not np.array_equal(got[0][-1][6], F0[-1][6])
    # ntf() with custom start values is the same run; one_ntf_step is its first iteration, normalised by the caller's norm
    again = ntf(T, r, init="custom", factors_0=F0, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True, weights=Wg)
    assert all(np.array_equal(a, b) for a, b in zip(again[0], got[0])) and list(again[1]) == list(got[1])
    norm = np.sqrt(wn.weighted_norm2(T, Wg))
    unf = [np.moveaxis(T, m, 0).reshape(T.shape[m], -1) for m in range(N)]
    F1, c1 = one_ntf_step(unf, r, F0, norm, "mu", beta, [None] * N, [], [False] * N, weights=Wg)
    assert np.isclose(c1, got[1][0], rtol=1e-6, atol=0)
    first = compute_ntf(T, r, F0, n_iter_max=1, tol=0, update_rule="mu", beta=beta, weights=Wg)
    assert all(np.array_equal(a, b) for a, b in zip(F1, first))
    F1u, c1u = one_ntf_step(unf, r, F0, norm, "mu", beta, [None] * N, [], [False] * N, weights=Wg.reshape(T.shape[0], -1))
    assert all(np.array_equal(a, b) for a, b in zip(F1u, F1)) and c1u == c1


_UNFOLD_CHILD = r"""
import sys, os, numpy as np
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
sys.path.insert(0, os.path.join(os.getcwd(), "oracle"))
import test_gpu_weighted_ntf as t
res = {}
for name in ("order3", "order4"):
    for beta in (0.5, 1, 2):
        F, costs, _ = t.run(name, beta)
        for i, f in enumerate(F):
            res["%s %r F%d" % (name, beta, i)] = f
        res["%s %r costs" % (name, beta)] = np.asarray(costs)
np.savez(sys.argv[1], **res)
print("done")
"""


def test_the_unfolded_route_agrees_with_the_on_layout_route(built_lib, monkeypatch, tmp_path):
    """NNF_MU_UNFOLD=1 in a child process: unfoldings of the tensor and of the weights through nnf_mu_right_w_f32."""
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    dst = str(tmp_path / "unfold.npz")
    p = subprocess.run([sys.executable, "-c", _UNFOLD_CHILD, dst], env=dict(os.environ, NNF_MU_UNFOLD="1"), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    saved = np.load(dst)
    for name in ("order3", "order4"):
        for beta in (0.5, 1, 2):
            got = run(name, beta)
            want = ([saved["%s %r F%d" % (name, beta, i)] for i in range(len(got[0]))], saved["%s %r costs" % (name, beta)])
            check(("unfold", name, beta), got, want, 2 * TOL_F, 2 * TOL_C)
            check(("unfold against fp64", name, beta), want, reference(name, beta))


def test_the_unfolded_route_unfolds_the_weights_too(built_lib, monkeypatch):
    """Rank 70: modes 0 and 1 through unfoldings of T AND Wg, made once per run; rank 7: none."""
    from nn_fac_amd import weighted_ntf
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    calls, orig = [], weighted_ntf._State.unfolded

    def spy(self, mode):
        calls.append((mode, mode in self._unf))
        X, W = orig(self, mode)
        assert X.shape == W.shape == (self.T.numel() // self.T.shape[mode], self.T.shape[mode]) and X.is_contiguous() and W.is_contiguous()
        return X, W
    monkeypatch.setattr(weighted_ntf._State, "unfolded", spy)
    run("order3", 1)
    assert calls == []
    run("rank70", 1)
    assert [c for c in calls if not c[1]] == [(0, False), (1, False)] and len(calls) >= 2 * N_ITER, calls


@pytest.mark.parametrize("beta", (0.5, 1, 2))
def test_boolean_mask_agrees_with_the_missing_entries_path(built_lib, monkeypatch, beta):
    from nn_fac_amd._convert import SparseCOO
    from nn_fac_amd.ntf import compute_ntf
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    T, Wg, r, F0 = problem("order3")
    mask = Wg != 0
    kw = dict(n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True)
    got = compute_ntf(T, r, F0, weights=mask, **kw)
    S = SparseCOO(np.argwhere(mask).T.copy(), T[mask].astype(np.float32), T.shape)
    want = compute_ntf(S, r, F0, unstored="missing", **kw)
    check(("mask vs stored entries", beta), got, want, 2 * TOL_F, 2 * TOL_C)
    # T[~mask] = nan gives what T[~mask] = 0 gives, bit for bit; a float 0/1 array is the mask
    zero = compute_ntf(np.nan_to_num(T), r, F0, weights=mask, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(zero[0], got[0])) and list(zero[1]) == list(got[1])
    same = compute_ntf(T, r, F0, weights=mask.astype(np.float32), **kw)
    assert all(np.array_equal(a, b) for a, b in zip(same[0], got[0])) and list(same[1]) == list(got[1])


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_weighted_ntf_parent",
                                                  os.path.join(ROOT, "tools", "gen_golden_weighted_ntf_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("tag", ["mu_b1", "mu_b05"])
def test_weights_none_is_bitwise_the_parent(built_lib, monkeypatch, tag):
    from nn_fac_amd.ntf import ntf
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    saved = np.load(GOLDEN, allow_pickle=False)
    F, costs = _gen().golden_run(tag, ntf, weights=None)
    for i, f in enumerate(F):
        assert np.array_equal(f, saved["%s_F%d" % (tag, i)]), (tag, i)
    assert np.array_equal(costs, saved[tag + "_costs"])


@pytest.mark.parametrize("beta", BETAS)
def test_all_ones_agree_with_no_weights(built_lib, monkeypatch, beta):
    from nn_fac_amd.ntf import compute_ntf
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    T, r, F0 = _gen().golden_problem()
    kw = dict(n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True)
    got = compute_ntf(T, r, F0, weights=np.ones_like(T), **kw)
    want = compute_ntf(T, r, F0, sparsity_coefficients=[None] * 3, fixed_modes=[], normalize=[False] * 3, **kw)
    check(("ones", beta), got, want)
    ones = compute_ntf(T, r, F0, weights=np.ones(T.shape, dtype=bool), **kw)
    assert all(np.array_equal(a, b) for a, b in zip(ones[0], got[0]))


@pytest.mark.parametrize("fixed", ([0], [1], [2], [0, 2]))
def test_fixed_modes_are_honoured(built_lib, monkeypatch, fixed):
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    T, Wg, r, F0 = problem("order3")
    got = run("order3", 1, fixed_modes=fixed)
    for m in fixed:
        assert np.array_equal(got[0][m], F0[m].astype(np.float32))
    check(("fixed", fixed), got, reference("order3", 1, fixed))


def test_device_tensors_in_device_tensors_out_same_bits(built_lib, monkeypatch):
    from nn_fac_amd.ntf import compute_ntf
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    T, Wg, r, F0 = problem("order3")
    host = run("order3", 0.5)
    Td, Wd = torch.from_numpy(T.astype(np.float32)).cuda(), torch.from_numpy(Wg.astype(np.float32)).cuda()
    Fd = [torch.from_numpy(f.astype(np.float32)).cuda() for f in F0]
    keep = [t.clone() for t in (Td, Wd, *Fd)]
    got = compute_ntf(Td, r, Fd, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=0.5, return_costs=True, weights=Wd)
    assert all(isinstance(f, torch.Tensor) and f.is_cuda for f in got[0])
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got[0], host[0])) and list(got[1]) == list(host[1])
    for a, b in zip((Td, Wd, *Fd), keep):
        assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_bad_weight_values_are_refused_after_the_upload(built_lib):
    from nn_fac_amd.ntf import compute_ntf
    from nn_fac_amd.utils import errors as err
    T, Wg, r, F0 = problem("order3")
    for bad in (-1e-3, np.nan, np.inf):
        w = Wg.copy()
        w[1, 2, 3] = bad
        with pytest.raises(err.InvalidArgumentValue, match="finite and >= 0"):
            compute_ntf(T, r, F0, n_iter_max=1, update_rule="mu", beta=1, weights=w)


def test_recovery_on_the_device(built_lib, monkeypatch):
    """The recipe of test_weighted_ntf_restatement.test_recovery_recipe: weights = sigma^-2 recover the rank-3 truth better than the
    unweighted fit, and the device lands within 10 % of the restatement's error."""
    from nn_fac_amd.ntf import compute_ntf
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    truth, T, Wg, F0 = wn.recovery_case()
    kw = dict(n_iter_max=300, tol=0, update_rule="mu", beta=2)
    ew = wn.recovery_error(truth, compute_ntf(T, 3, F0, weights=Wg, **kw))
    en = wn.recovery_error(truth, compute_ntf(T, 3, F0, sparsity_coefficients=[None] * 3, fixed_modes=[], normalize=[False] * 3, **kw))
    want = wn.recovery_error(truth, wn.run(T, Wg, F0, 300, 2)[0])      # the restatement's own error, computed here
    print("device: with weights", ew, "without", en, "restatement", want)
    assert ew < en and abs(ew - want) <= 0.1 * want

"""ntf / compute_ntf / one_ntf_step on sparse tensors (nn_fac_amd/sparse_ntf.py) against the fp64 restatement of
tests/sptensor_restatement.py, at the project's fp32 tolerances for sparse NMF (tests/test_gpu_sparse_nmf.py): HALS rel_fro <= 5e-4
on every factor and cost rtol 1e-3; MU rel_fro <= 5e-5 and cost rtol 1e-4.  Five iterations, tol = 0, alpha = inf.

Tensors: 40 x 33 x 27 at rank 6 (about 10 % stored, an empty slice in every mode, stored zeros), 300 x 200 x 50 at rank 50 (about
2 % stored) and 12 x 9 x 10 x 8 at rank 5.  The restatement runs on the fp32-rounded data and start values.  A HALS case compares the
inner sweep counts with the restatement's first: were one inner stopping decision to flip between fp32 and fp64, the factors would
differ by a whole sweep and the case would have to move to another seed -- the tolerances stay.

Start values of the 300 x 200 x 50 case: three rand(dim, 50) factors are a model of 50 / 8 = 6.25 per entry for data whose mean is
0.012, so the first HALS sweeps would compute rhs - cross F as differences of fp32 numbers hundreds of times their result (the head
of tests/test_gpu_sparse_nmf.py measures what that costs, whatever forms the cross products).  The case therefore starts from the
same random factors scaled to the data's mean (the start model has the mean of T).  The small cases keep the unscaled start."""
import gc
import math

import numpy as np
import pytest
import torch

import sptensor_restatement as rs

pytestmark = pytest.mark.gpu

TOL = {"hals": (5e-4, 1e-3), "mu": (5e-5, 1e-4)}
N_ITER = 5
RULES = [("hals", 2), ("mu", 1), ("mu", 2)]


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


_problems = {}


def problem(name):
    """(Coo, rank, start factors), fp32-representable."""
    if name not in _problems:
        if name == "40x33x27":
            X, r = rs.sample((40, 33, 27), 0.1, seed=0, empty=[(0, 7), (1, 11), (2, 3)], stored_zeros=5), 6
        elif name == "300x200x50":
            X, r = rs.sample((300, 200, 50), 0.02, seed=1), 50
        else:
            X, r = rs.sample((12, 9, 10, 8), 0.1, seed=2, empty=[(0, 3)], stored_zeros=2), 5
        X.vals = f32(X.vals)
        rng = np.random.default_rng(5)
        N = len(X.shape)
        mean = X.vals.sum() / np.prod(X.shape)
        scale = float((mean / (r * 0.5 ** N)) ** (1.0 / N)) if name == "300x200x50" else 1.0      # (the head of this file)
        _problems[name] = (X, r, [f32(scale * rng.random((d, r))) for d in X.shape])
    return _problems[name]


def coo(X, device=None):
    """The SparseCOO of a restatement tensor (NumPy lists, or tensors on `device`)."""
    from nn_fac_amd.sparse_ntf import SparseCOO
    ind, val = np.ascontiguousarray(X.coords.T), X.vals.astype(np.float32)
    if device is not None:
        ind, val = torch.from_numpy(ind).to(device), torch.from_numpy(val).to(device)
    return SparseCOO(ind, val, X.shape)


_references = {}


def reference(name, rule, beta, **kw):
    """The restatement's run, once per case."""
    key = (name, rule, beta, tuple(sorted((k, tuple(v)) for k, v in kw.items())))
    if key not in _references:
        X, r, F0 = problem(name)
        sweeps = []
        _references[key] = rs.run(X, F0, N_ITER, rule, beta, sweeps=sweeps, **kw) + (sweeps,)
    return _references[key]


def check(name, rule, beta, got, sweep_log=None, **kw):
    factors, costs = got[:2]
    Fr, cr, sweeps = reference(name, rule, beta, **kw)
    if sweep_log is not None:
        assert list(sweep_log) == list(sweeps), "an inner stopping decision flipped between fp32 and fp64: change the seed"
    tol_f, tol_c = TOL[rule]
    print(name, rule, beta, kw, "rel", [rel(a, b) for a, b in zip(factors, Fr)], "cost", costs[-1], cr[-1])
    assert len(costs) == N_ITER and len(factors) == len(Fr)
    for a, b in zip(factors, Fr):
        assert a.shape == b.shape and rel(a, b) <= tol_f
    assert np.allclose(costs, cr, rtol=tol_c, atol=0), (costs, cr)


@pytest.mark.parametrize("name", ["40x33x27", "300x200x50", "12x9x10x8"])
@pytest.mark.parametrize("rule,beta", RULES)
def test_five_iterations_against_the_restatement(built_lib, name, rule, beta):
    from nn_fac_amd.ntf import ntf, compute_ntf, one_ntf_step
    X, r, F0 = problem(name)
    N = len(X.shape)
    log = []
    got = compute_ntf(coo(X), r, F0, n_iter_max=N_ITER, tol=0, update_rule=rule, beta=beta, sparsity_coefficients=[None] * N,
                      normalize=[False] * N, return_costs=True, alpha=math.inf, sweep_log=log)
    assert all(isinstance(F, np.ndarray) and F.shape == F0[i].shape for i, F in enumerate(got[0])) and len(got[2]) == N_ITER
    check(name, rule, beta, got, sweep_log=log if rule == "hals" else None)
    # one_ntf_step, the sparse object where the unfoldings are, is the first iteration
    F1, c1 = one_ntf_step(coo(X), r, F0, None, rule, beta, [None] * N, [], [False] * N, alpha=math.inf)
    assert all(np.array_equal(a, b) for a, b in zip(F1, compute_ntf(coo(X), r, F0, n_iter_max=1, tol=0, update_rule=rule, beta=beta,
                                                                   sparsity_coefficients=[None] * N, normalize=[False] * N,
                                                                   alpha=math.inf)))
    assert abs(c1 - got[1][0]) <= 1e-12 * abs(c1)
    if rule == "mu":      # ntf() has no alpha: its HALS sweeps follow the wall clock (the last test of this file); MU is the same run
        again = ntf(coo(X), r, init="custom", factors_0=F0, n_iter_max=N_ITER, tol=0, update_rule=rule, beta=beta,
                    sparsity_coefficients=[None] * N, normalize=[False] * N, return_costs=True)
        assert all(np.array_equal(a, b) for a, b in zip(again[0], got[0])) and list(again[1]) == list(got[1])


@pytest.mark.parametrize("kw", [dict(sparsity_coefficients=[0.05, 0.02, 0.01]), dict(normalize=[True, False, False]), dict(fixed_modes=[0]),
                                dict(fixed_modes=[2])], ids=["sparsity", "normalize", "fixed0", "fixed-last"])
def test_hals_options_match_the_restatement(built_lib, kw):
    from nn_fac_amd.ntf import compute_ntf
    X, r, F0 = problem("40x33x27")
    log = []
    args = dict(sparsity_coefficients=[None] * 3, normalize=[False] * 3)
    args.update({k: list(v) for k, v in kw.items()})
    got = compute_ntf(coo(X), r, F0, n_iter_max=N_ITER, tol=0, update_rule="hals", return_costs=True, alpha=math.inf, sweep_log=log,
                      **args)
    check("40x33x27", "hals", 2, got, sweep_log=log, **kw)
    for f in kw.get("fixed_modes", ()):
        assert np.array_equal(got[0][f], F0[f])


def test_unsorted_entries_stored_twice_give_the_same_bits(built_lib):
    from nn_fac_amd.ntf import compute_ntf
    from nn_fac_amd.sparse_ntf import SparseCOO
    X, r, F0 = problem("40x33x27")
    kw = dict(n_iter_max=2, tol=0, sparsity_coefficients=[None] * 3, normalize=[False] * 3, return_costs=True, alpha=math.inf)
    rng = np.random.default_rng(0)
    order = rng.permutation(2 * X.nnz)      # every entry twice at half its value (x / 2 + x / 2 = x exactly), in any order
    ind = np.concatenate([X.coords, X.coords]).T[:, order]
    val = (np.concatenate([X.vals, X.vals]) / 2).astype(np.float32)[order]
    for rule, beta in RULES:
        want = compute_ntf(coo(X), r, F0, update_rule=rule, beta=beta, **kw)
        got = compute_ntf(SparseCOO(ind, val, X.shape), r, F0, update_rule=rule, beta=beta, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0])) and list(got[1]) == list(want[1]), (rule, beta)


def test_torch_coo_on_host_and_device_gives_the_same_bits_and_device_factors(built_lib):
    from nn_fac_amd.ntf import compute_ntf, one_ntf_step
    X, r, F0 = problem("40x33x27")
    T = torch.sparse_coo_tensor(torch.from_numpy(np.ascontiguousarray(X.coords.T)), torch.from_numpy(X.vals.astype(np.float32)), size=X.shape)
    Fd = [torch.from_numpy(F).float().cuda() for F in F0]
    kw = dict(n_iter_max=3, tol=0, sparsity_coefficients=[None] * 3, normalize=[False] * 3, return_costs=True, alpha=math.inf)
    for rule, beta in (("hals", 2), ("mu", 1)):
        want = compute_ntf(coo(X), r, F0, update_rule=rule, beta=beta, **kw)
        for src in (T.cuda(), T, T.coalesce(), coo(X, "cuda")):
            factors, costs, _ = compute_ntf(src, r, Fd, update_rule=rule, beta=beta, **kw)
            assert all(F.is_cuda and F.shape == Fd[i].shape for i, F in enumerate(factors))
            assert all(np.array_equal(F.cpu().numpy(), W.astype(np.float32)) for F, W in zip(factors, want[0]))
            assert list(costs) == list(want[1])
        F1, c1 = one_ntf_step(T.cuda(), r, Fd, None, rule, beta, [None] * 3, [], [False] * 3, alpha=math.inf)
        assert F1[0].is_cuda and abs(c1 - want[1][0]) <= 1e-12 * abs(c1)
    assert all(torch.equal(Fd[i].cpu(), torch.from_numpy(F0[i]).float()) for i in range(3))      # the caller's factors are not modified


@pytest.mark.parametrize("rule,beta", RULES)
def test_every_entry_stored_gives_the_dense_drivers_factors(built_lib, rule, beta):
    from nn_fac_amd.ntf import compute_ntf
    rng = np.random.default_rng(3)
    D = f32(rng.random((13, 11, 7)) + 0.1)
    F0 = [f32(rng.random((d, 4))) for d in D.shape]
    X = rs.Coo(np.argwhere(np.ones(D.shape, dtype=bool)), D.reshape(-1), D.shape)
    kw = dict(n_iter_max=N_ITER, tol=0, update_rule=rule, beta=beta, sparsity_coefficients=[None] * 3, normalize=[False] * 3,
              return_costs=True, alpha=math.inf)
    ls, ld = [], []
    Fs, cs, _ = compute_ntf(coo(X), 4, F0, sweep_log=ls, **kw)
    Fd, cd, _ = compute_ntf(D, 4, F0, sweep_log=ld, **kw)
    assert ls == ld
    tol_f, tol_c = TOL[rule]
    print(rule, beta, "rel", [rel(a, b) for a, b in zip(Fs, Fd)])
    assert all(rel(a, b) <= tol_f for a, b in zip(Fs, Fd)) and np.allclose(cs, cd, rtol=tol_c, atol=0)


def test_no_dense_copy_of_a_tensor_that_would_not_fit(built_lib):
    """20000^3 with 5000 stored entries: 3.2e13 bytes dense.  Two iterations of each rule stay below 64 MB of device memory:
    the peak of torch's allocator over the runs, less what was live before them (inside the whole suite other modules' fixtures
    hold some 240 MB at this point, which says nothing about this driver; run alone, nothing is live and the figure is the peak)."""
    from nn_fac_amd.ntf import compute_ntf
    n, nnz, r = 20000, 5000, 8
    rng = np.random.default_rng(11)
    coords = np.unique(rng.integers(0, n, size=(nnz, 3)), axis=0)
    X = rs.Coo(coords, f32(rng.random(len(coords)) + 0.1), (n, n, n))
    F0 = [f32(rng.random((n, r))) for _ in range(3)]
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    for rule, beta in RULES:
        factors, costs, _ = compute_ntf(coo(X), r, F0, n_iter_max=2, tol=0, update_rule=rule, beta=beta, sparsity_coefficients=[None] * 3,
                                        normalize=[False] * 3, return_costs=True, alpha=math.inf)
        assert len(costs) == 2 and np.isfinite(costs).all()
        assert all(F.shape == (n, r) and np.isfinite(F).all() for F in factors)
    peak = torch.cuda.max_memory_allocated() - live
    print("peak device memory of the runs:", peak, "live before them:", live)
    assert peak < 64 * 2 ** 20


def test_a_default_ntf_call_runs_timed_sweeps_from_a_random_start(built_lib):
    from nn_fac_amd.ntf import ntf
    X, r, _ = problem("40x33x27")
    factors, costs, toc = ntf(coo(X), r, n_iter_max=20, return_costs=True)
    assert len(factors) == 3 and all(F.shape == (d, r) and np.isfinite(F).all() for F, d in zip(factors, X.shape))
    assert np.isfinite(costs).all() and costs[-1] < costs[0] and len(toc) == len(costs)


class RefusingLib:
    """Stands in for eng.lib while a refusal is expected: an entry that is reached is recorded and not run."""

    def __init__(self, lib):
        self._lib, self.reached = lib, []

    def __getattr__(self, name):
        if not name.startswith("nnf_") or name == "nnf_status_string":
            return getattr(self._lib, name)

        def refused(*args):
            self.reached.append(name)
            return 0
        return refused


def test_what_the_sparse_path_refuses_is_said_before_any_launch(built_lib):
    from nn_fac_amd.engine import get_engine, EngineError
    from nn_fac_amd.ntf import ntf, compute_ntf, one_ntf_step
    from nn_fac_amd.sparse_ntf import SparseCOO, compute_sparse_ntf
    X, r, F0 = problem("40x33x27")
    S = coo(X)
    rng = np.random.default_rng(0)
    eng = get_engine("cuda:0")
    real = eng.lib
    eng.lib = proxy = RefusingLib(real)
    try:
        for beta in (0, 0.5, 1.5, 3):
            with pytest.raises(NotImplementedError, match="beta"):
                ntf(S, r, update_rule="mu", beta=beta, n_iter_max=2)
            with pytest.raises(NotImplementedError, match="beta"):
                compute_ntf(S, r, F0, update_rule="mu", beta=beta, n_iter_max=2)
            with pytest.raises(NotImplementedError, match="beta"):
                one_ntf_step(S, r, F0, None, "mu", beta, [None] * 3, [], [False] * 3)
        six = SparseCOO(np.zeros((6, 4), dtype=np.int64), np.ones(4), (2,) * 6)
        with pytest.raises(NotImplementedError, match="order 6"):
            ntf(six, 2, n_iter_max=2)
        with pytest.raises(NotImplementedError, match="order 6"):
            compute_ntf(six, 2, [rng.random((2, 2)) for _ in range(6)], n_iter_max=2)
        two = SparseCOO(np.zeros((2, 4), dtype=np.int64), np.ones(4), (5, 4))
        with pytest.raises(NotImplementedError, match="nmf"):
            ntf(two, 2, n_iter_max=2)
        with pytest.raises(NotImplementedError, match="nmf"):
            one_ntf_step(two, 2, [rng.random((5, 2)), rng.random((4, 2))], None, "hals", 2, [None] * 2, [], [False] * 2)
        with pytest.raises(NotImplementedError, match="nndsvd"):
            ntf(S, r, init="nndsvd", n_iter_max=2)
        with pytest.raises(NotImplementedError, match="group"):
            compute_sparse_ntf(S, r, F0, n_iter_max=2, group=object())
        big = [rng.random((d, 130)) for d in X.shape]
        with pytest.raises(EngineError, match="rank 130"):
            ntf(S, 130, init="custom", factors_0=big, n_iter_max=2)
        with pytest.raises(EngineError, match="rank 130"):
            compute_ntf(S, 130, big, n_iter_max=2, update_rule="mu", beta=1)
        with pytest.raises(EngineError, match="rank 130"):
            one_ntf_step(S, 130, big, None, "hals", 2, [None] * 3, [], [False] * 3)
        assert not proxy.reached, proxy.reached
    finally:
        eng.lib = real

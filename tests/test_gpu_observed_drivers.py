"""nmf / compute_nmf / one_nmf_step and ntf / compute_ntf / one_ntf_step with unstored="missing" (nn_fac_amd/sparse_nmf.py,
sparse_ntf.py: the multiplicative update over the stored entries only) against the fp64 restatement of
tests/observed_restatement.py, at the project's MU tolerances (tests/test_gpu_nmf.py, test_gpu_sparse_nmf.py): rel_fro <= 5e-5 on
every factor, cost rtol 1e-4.  Five iterations, tol = 0, beta in 0, 0.5, 1, 2, 3.

Matrices: the two problems of tests/test_gpu_sparse_nmf.py -- 300 x 200 at rank 10 (16 % stored, an empty row, an empty column,
stored zeros) and 2000 x 300 at rank 50 (5 % stored, the scaled start of that file).  Tensors: the three problems of
tests/test_gpu_sparse_ntf.py (40 x 33 x 27 at rank 6 with an empty slice per mode and stored zeros, 300 x 200 x 50 at rank 50 with its
scaled start, 12 x 9 x 10 x 8 at rank 5) and, that file having no tensor of order 5, 7 x 6 x 5 x 4 x 3 at rank 3 (10 % stored, an
empty slice in the first mode, stored zeros).  At beta = 0 a stored zero makes the cost +inf from the first iteration (d_0(0 | p));
the factors are compared all the same, the costs as equal infinities, and the finite cost of beta = 0 is compared on the problems
without stored zeros.

Then: every entry stored equals the dense driver (the golden-pinned path) at every beta; recovery of the unstored entries of an
exactly low-rank matrix and tensor, where the stored-zero reading of the same sparse object fails; the refusals, said before any
launch; and the peak device memory of a run on data whose dense size would not fit."""
import gc
import math

import numpy as np
import pytest
import torch

import observed_restatement as ob
import sptensor_restatement as ts
import test_gpu_sparse_nmf as mx
import test_gpu_sparse_ntf as tx

pytestmark = pytest.mark.gpu

TOL_F, TOL_C = 5e-5, 1e-4
N_ITER = 5
BETAS = (0, 0.5, 1, 2, 3)
TENSORS = ["40x33x27", "300x200x50", "12x9x10x8", "7x6x5x4x3"]

f32, rel = mx.f32, mx.rel


def tensor_problem(name):
    if name != "7x6x5x4x3":
        return tx.problem(name)
    X = ts.sample((7, 6, 5, 4, 3), 0.1, seed=6, empty=[(0, 3)], stored_zeros=2)
    X.vals = f32(X.vals)
    rng = np.random.default_rng(5)
    return X, 3, [f32(rng.random((d, 3))) for d in X.shape]


_references = {}


def reference(kind, name, beta):
    """The restatement's five iterations, once per case: (factors, costs)."""
    key = (kind, name, beta)
    if key not in _references:
        if kind == "nmf":
            X, r, U0, V0 = mx.problem(name)
            _references[key] = ob.run(ob.from_csr(X), ob.nmf_factors(U0, V0), N_ITER, beta)
        else:
            X, r, F0 = tensor_problem(name)
            _references[key] = ob.run(X, F0, N_ITER, beta)
    return _references[key]


def check(tag, factors, costs, want, want_costs):
    print(tag, "rel", [rel(a, b) for a, b in zip(factors, want)], "cost", costs[-1], want_costs[-1])
    assert len(costs) == N_ITER
    for a, b in zip(factors, want):
        assert a.shape == b.shape and rel(a, b) <= TOL_F, tag
    if np.isinf(want_costs).any():
        assert list(costs) == list(want_costs), tag
    else:
        assert np.allclose(costs, want_costs, rtol=TOL_C, atol=0), (tag, costs, want_costs)


@pytest.mark.parametrize("name", ["300x200", "2000x300"])
@pytest.mark.parametrize("beta", BETAS)
def test_nmf_five_iterations_against_the_restatement(built_lib, name, beta):
    from nn_fac_amd.nmf import nmf, compute_nmf, one_nmf_step
    X, r, U0, V0 = mx.problem(name)
    U0c, V0c = U0.copy(), V0.copy()
    got = compute_nmf(X, r, U0, V0, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True, unstored="missing")
    assert isinstance(got[0], np.ndarray) and got[0].shape == U0.shape and got[1].shape == V0.shape and len(got[3]) == N_ITER
    assert np.array_equal(U0, U0c) and np.array_equal(V0, V0c)      # the caller's factors are not modified
    (Ur, Vtr), cr = reference("nmf", name, beta)
    check(("nmf", name, beta), [got[0], got[1].T], got[2], [Ur, Vtr], cr)
    assert np.isfinite(cr).all() == (beta != 0 or name == "2000x300")      # (stored zeros in the small problem only)
    if name == "300x200":      # the empty row and column hold their start values exactly
        assert np.array_equal(got[0][7], U0[7].astype(np.float32)) and np.array_equal(got[1][:, 11], V0[:, 11].astype(np.float32))
        assert not np.array_equal(got[0][8], U0[8].astype(np.float32))
    # nmf() with custom start values is the same run; one_nmf_step is its first iteration
    again = nmf(X, r, init="custom", U_0=U0, V_0=V0, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True,
                unstored="missing")
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1]) and list(again[2]) == list(got[2])
    U1, V1, c1 = one_nmf_step(X, r, U0, V0, None, "mu", beta, [None, None], [], [False, False], True, unstored="missing")
    assert c1 == got[2][0] or abs(c1 - got[2][0]) <= 1e-12 * abs(c1)
    first = compute_nmf(X, r, U0, V0, n_iter_max=1, tol=0, update_rule="mu", beta=beta, unstored="missing")
    assert np.array_equal(U1, first[0]) and np.array_equal(V1, first[1])


@pytest.mark.parametrize("name", TENSORS)
@pytest.mark.parametrize("beta", BETAS)
def test_ntf_five_iterations_against_the_restatement(built_lib, name, beta):
    from nn_fac_amd.ntf import ntf, compute_ntf, one_ntf_step
    X, r, F0 = tensor_problem(name)
    N = len(X.shape)
    F0c = [F.copy() for F in F0]
    kw = dict(tol=0, update_rule="mu", beta=beta, sparsity_coefficients=[None] * N, normalize=[False] * N, unstored="missing")
    got = compute_ntf(tx.coo(X), r, F0, n_iter_max=N_ITER, return_costs=True, **kw)
    assert all(isinstance(F, np.ndarray) and F.shape == F0[i].shape for i, F in enumerate(got[0])) and len(got[2]) == N_ITER
    assert all(np.array_equal(a, b) for a, b in zip(F0, F0c))
    Fr, cr = reference("ntf", name, beta)
    check(("ntf", name, beta), got[0], got[1], Fr, cr)
    if name == "40x33x27":      # the empty slice of every mode holds its start values exactly
        for mode, index in ((0, 7), (1, 11), (2, 3)):
            assert np.array_equal(got[0][mode][index], F0[mode][index].astype(np.float32)), mode
            assert not np.array_equal(got[0][mode][index + 1], F0[mode][index + 1].astype(np.float32)), mode
    again = ntf(tx.coo(X), r, init="custom", factors_0=F0, n_iter_max=N_ITER, return_costs=True, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(again[0], got[0])) and list(again[1]) == list(got[1])
    F1, c1 = one_ntf_step(tx.coo(X), r, F0, None, "mu", beta, [None] * N, [], [False] * N, unstored="missing")
    assert c1 == got[1][0] or abs(c1 - got[1][0]) <= 1e-12 * abs(c1)
    assert all(np.array_equal(a, b) for a, b in zip(F1, compute_ntf(tx.coo(X), r, F0, n_iter_max=1, **kw)))


def test_fixed_modes_are_honoured(built_lib):
    from nn_fac_amd.nmf import compute_nmf
    from nn_fac_amd.ntf import compute_ntf
    X, r, U0, V0 = mx.problem("300x200")
    U, V = compute_nmf(X, r, U0, V0, n_iter_max=2, tol=0, update_rule="mu", beta=1, fixed_modes=[0], unstored="missing")
    (Ur, Vtr), _ = ob.run(ob.from_csr(X), ob.nmf_factors(U0, V0), 2, 1, fixed_modes=(0,))
    assert np.array_equal(U, U0) and rel(V.T, Vtr) <= TOL_F
    T, rt, F0 = tensor_problem("40x33x27")
    got = compute_ntf(tx.coo(T), rt, F0, n_iter_max=2, tol=0, update_rule="mu", beta=0.5, fixed_modes=[1], sparsity_coefficients=[None] * 3,
                      normalize=[False] * 3, unstored="missing")
    Fr, _ = ob.run(T, F0, 2, 0.5, fixed_modes=(1,))
    assert np.array_equal(got[1], F0[1]) and all(rel(a, b) <= TOL_F for a, b in zip(got, Fr))


def test_device_tensors_in_give_device_tensors_out_with_the_same_bits(built_lib):
    from nn_fac_amd.nmf import compute_nmf, one_nmf_step
    from nn_fac_amd.ntf import compute_ntf, one_ntf_step
    X, r, U0, V0 = mx.problem("300x200")
    T = torch.sparse_csr_tensor(torch.from_numpy(X.indptr.astype(np.int64)), torch.from_numpy(X.indices.astype(np.int64)),
                                torch.from_numpy(X.data.astype(np.float32)), size=X.shape)
    Ud, Vd = torch.from_numpy(U0).float().cuda(), torch.from_numpy(V0).float().cuda()
    for beta in (0.5, 2):
        want = compute_nmf(X, r, U0, V0, n_iter_max=3, tol=0, update_rule="mu", beta=beta, return_costs=True, unstored="missing")
        for src in (T.cuda(), T):
            U, V, costs, _ = compute_nmf(src, r, Ud, Vd, n_iter_max=3, tol=0, update_rule="mu", beta=beta, return_costs=True,
                                         unstored="missing")
            assert U.is_cuda and V.is_cuda and U.shape == Ud.shape and V.shape == Vd.shape
            assert np.array_equal(U.cpu().numpy(), want[0].astype(np.float32)) and np.array_equal(V.cpu().numpy(), want[1].astype(np.float32))
            assert list(costs) == list(want[2])
        U1, V1, c1 = one_nmf_step(T.cuda(), r, Ud, Vd, None, "mu", beta, [None, None], [], [False, False], True, unstored="missing")
        assert U1.is_cuda and abs(c1 - want[2][0]) <= 1e-12 * abs(c1)
    assert torch.equal(Ud.cpu(), torch.from_numpy(U0).float()) and torch.equal(Vd.cpu(), torch.from_numpy(V0).float())
    Xt, rt, F0 = tensor_problem("40x33x27")
    Fd = [torch.from_numpy(F).float().cuda() for F in F0]
    kw = dict(tol=0, update_rule="mu", beta=1, sparsity_coefficients=[None] * 3, normalize=[False] * 3, unstored="missing")
    want = compute_ntf(tx.coo(Xt), rt, F0, n_iter_max=3, return_costs=True, **kw)
    torch_coo = torch.sparse_coo_tensor(torch.from_numpy(np.ascontiguousarray(Xt.coords.T)), torch.from_numpy(Xt.vals.astype(np.float32)),
                                        Xt.shape)
    for src in (tx.coo(Xt, "cuda"), torch_coo.cuda(), torch_coo):
        factors, costs, _ = compute_ntf(src, rt, Fd, n_iter_max=3, return_costs=True, **kw)
        assert all(F.is_cuda and np.array_equal(F.cpu().numpy(), w.astype(np.float32)) for F, w in zip(factors, want[0]))
        assert list(costs) == list(want[1])
    F1, c1 = one_ntf_step(tx.coo(Xt, "cuda"), rt, Fd, None, "mu", 1, [None] * 3, [], [False] * 3, unstored="missing")
    assert all(F.is_cuda for F in F1) and abs(c1 - want[1][0]) <= 1e-12 * abs(c1)
    assert all(torch.equal(a.cpu(), torch.from_numpy(b).float()) for a, b in zip(Fd, F0))


@pytest.mark.parametrize("beta", BETAS)
def test_every_entry_stored_gives_the_dense_drivers_factors(built_lib, beta):
    from nn_fac_amd.nmf import compute_nmf
    from nn_fac_amd.ntf import compute_ntf
    from nn_fac_amd.sparse_nmf import observed_entries
    rng = np.random.default_rng(3)
    D = f32(rng.random((130, 70)) + 0.1)
    U0, V0 = f32(rng.random((130, 8))), f32(rng.random((8, 70)))
    kw = dict(n_iter_max=N_ITER, tol=0, update_rule="mu", beta=beta, return_costs=True)
    Us, Vs, cs, _ = compute_nmf(observed_entries(D, np.ones(D.shape, bool)), 8, U0, V0, unstored="missing", **kw)
    Ud, Vd, cd, _ = compute_nmf(D, 8, U0, V0, **kw)
    print("nmf", beta, "rel U", rel(Us, Ud), "rel V", rel(Vs, Vd), "cost", cs[-1], cd[-1])
    assert rel(Us, Ud) <= TOL_F and rel(Vs, Vd) <= TOL_F and np.allclose(cs, cd, rtol=TOL_C, atol=0)
    T = f32(rng.random((20, 15, 12)) + 0.1)
    F0 = [f32(rng.random((d, 4))) for d in T.shape]
    kw.update(sparsity_coefficients=[None] * 3, normalize=[False] * 3)
    Fs, cs, _ = compute_ntf(observed_entries(T, np.ones(T.shape, bool)), 4, F0, unstored="missing", **kw)
    Fd, cd, _ = compute_ntf(T, 4, F0, **kw)
    print("ntf", beta, "rel", [rel(a, b) for a, b in zip(Fs, Fd)], "cost", cs[-1], cd[-1])
    assert all(rel(a, b) <= TOL_F for a, b in zip(Fs, Fd)) and np.allclose(cs, cd, rtol=TOL_C, atol=0)


@pytest.mark.parametrize("beta", [2, 1])
def test_recovery_of_the_unstored_entries(built_lib, beta):
    """An exactly rank-3 matrix (60 x 50, 40 % stored) and tensor (30 x 25 x 20, 30 % stored): after 200 MU iterations the relative
    error on the UNSTORED entries is <= 0.05 (matrix; fp64: 0.009 at beta = 2, 0.0074 at beta = 1) and <= 0.07 (tensor; fp64: 0.014
    and 0.005) with unstored="missing", and >= 0.5 with the stored-zero reading of the same sparse object (fp64: 0.69, 0.70, 0.73,
    0.72)."""
    from nn_fac_amd.nmf import compute_nmf
    from nn_fac_amd.ntf import compute_ntf
    from nn_fac_amd.sparse_nmf import observed_entries
    rng = np.random.default_rng(0)
    A = rng.random((60, 3)) + 0.1
    B = rng.random((3, 50)) + 0.1
    X = A @ B
    M = rng.random((60, 50)) < 0.4
    U0 = rng.random((60, 3))
    V0 = rng.random((3, 50))
    S = observed_entries(X, M)
    kw = dict(n_iter_max=200, tol=0, update_rule="mu", beta=beta)
    U, V = compute_nmf(S, 3, U0, V0, unstored="missing", **kw)
    Uz, Vz = compute_nmf(S, 3, U0, V0, unstored="zero", **kw)
    miss, zero = ob.heldout_error(X, M, [U, V.T]), ob.heldout_error(X, M, [Uz, Vz.T])
    print("matrix beta", beta, "missing", miss, "zero", zero)
    assert miss <= 0.05 and zero >= 0.5
    rng = np.random.default_rng(0)
    true = [rng.random((d, 3)) + 0.1 for d in (30, 25, 20)]
    T = np.einsum("az,bz,cz->abc", *true)
    MT = rng.random(T.shape) < 0.3
    start = [rng.random((d, 3)) for d in (30, 25, 20)]
    ST = observed_entries(T, MT)
    kw.update(sparsity_coefficients=[None] * 3, normalize=[False] * 3)
    F = compute_ntf(ST, 3, start, unstored="missing", **kw)
    Fz = compute_ntf(ST, 3, start, unstored="zero", **kw)
    miss, zero = ob.heldout_error(T, MT, F), ob.heldout_error(T, MT, Fz)
    print("tensor beta", beta, "missing", miss, "zero", zero)
    assert miss <= 0.07 and zero >= 0.5


def test_what_is_refused_is_said_before_any_launch(built_lib):
    from nn_fac_amd.engine import get_engine, EngineError
    from nn_fac_amd.nmf import nmf, compute_nmf, one_nmf_step
    from nn_fac_amd.ntf import ntf, compute_ntf, one_ntf_step
    from nn_fac_amd.sparse_ntf import SparseCOO, compute_sparse_ntf
    from nn_fac_amd.utils.errors import InvalidArgumentValue
    X, r, U0, V0 = mx.problem("300x200")
    T, rt, F0 = tensor_problem("40x33x27")
    Tc = tx.coo(T)
    rng = np.random.default_rng(0)
    dense, dense3 = X.toarray(), T.dense()
    step2 = (None, "mu", 2, [None, None], [], [False, False], True)
    step3 = (None, "mu", 2, [None] * 3, [], [False] * 3)
    eng = get_engine("cuda:0")
    real = eng.lib
    eng.lib = proxy = mx.RefusingLib(real)
    try:
        # hals with missing entries
        with pytest.raises(NotImplementedError, match=r'hals.*update_rule="mu"'):
            nmf(X, r, n_iter_max=2, unstored="missing")
        with pytest.raises(NotImplementedError, match=r'hals.*update_rule="mu"'):
            compute_nmf(X, r, U0, V0, n_iter_max=2, update_rule="hals", unstored="missing")
        with pytest.raises(NotImplementedError, match=r'hals.*update_rule="mu"'):
            one_nmf_step(X, r, U0, V0, None, "hals", 2, [None, None], [], [False, False], True, unstored="missing")
        with pytest.raises(NotImplementedError, match=r'hals.*update_rule="mu"'):
            ntf(Tc, rt, n_iter_max=2, unstored="missing")
        with pytest.raises(NotImplementedError, match=r'hals.*update_rule="mu"'):
            compute_ntf(Tc, rt, F0, n_iter_max=2, unstored="missing")
        with pytest.raises(NotImplementedError, match=r'hals.*update_rule="mu"'):
            one_ntf_step(Tc, rt, F0, None, "hals", 2, [None] * 3, [], [False] * 3, unstored="missing")
        # dense data has no unstored entries
        with pytest.raises(InvalidArgumentValue, match="dense"):
            nmf(dense, r, update_rule="mu", n_iter_max=2, unstored="missing")
        with pytest.raises(InvalidArgumentValue, match="dense"):
            compute_nmf(dense, r, U0, V0, update_rule="mu", n_iter_max=2, unstored="missing")
        with pytest.raises(InvalidArgumentValue, match="dense"):
            one_nmf_step(dense, r, U0, V0, *step2, unstored="missing")
        with pytest.raises(InvalidArgumentValue, match="dense"):
            ntf(dense3, rt, update_rule="mu", n_iter_max=2, unstored="missing")
        with pytest.raises(InvalidArgumentValue, match="dense"):
            compute_ntf(dense3, rt, F0, update_rule="mu", n_iter_max=2, unstored="missing")
        with pytest.raises(InvalidArgumentValue, match="dense"):
            one_ntf_step([dense3.reshape(40, -1)] * 3, rt, F0, *step3, unstored="missing")
        # another value of the keyword, on sparse and on dense data
        for data in (X, dense):
            with pytest.raises(InvalidArgumentValue, match="unstored"):
                nmf(data, r, update_rule="mu", n_iter_max=2, unstored="nan")
            with pytest.raises(InvalidArgumentValue, match="unstored"):
                compute_nmf(data, r, U0, V0, update_rule="mu", n_iter_max=2, unstored=None)
            with pytest.raises(InvalidArgumentValue, match="unstored"):
                one_nmf_step(data, r, U0, V0, *step2, unstored="Missing")
        for data in (Tc, dense3):
            with pytest.raises(InvalidArgumentValue, match="unstored"):
                ntf(data, rt, update_rule="mu", n_iter_max=2, unstored="nan")
            with pytest.raises(InvalidArgumentValue, match="unstored"):
                compute_ntf(data, rt, F0, update_rule="mu", n_iter_max=2, unstored=0)
        with pytest.raises(InvalidArgumentValue, match="unstored"):
            one_ntf_step(Tc, rt, F0, *step3, unstored="observed")
        # beta < 0
        for beta in (-1, -0.25):
            with pytest.raises(InvalidArgumentValue, match="beta"):
                nmf(X, r, update_rule="mu", beta=beta, n_iter_max=2, unstored="missing")
            with pytest.raises(InvalidArgumentValue, match="beta"):
                compute_nmf(X, r, U0, V0, update_rule="mu", beta=beta, n_iter_max=2, unstored="missing")
            with pytest.raises(InvalidArgumentValue, match="beta"):
                one_nmf_step(X, r, U0, V0, None, "mu", beta, [None, None], [], [False, False], True, unstored="missing")
            with pytest.raises(InvalidArgumentValue, match="beta"):
                ntf(Tc, rt, update_rule="mu", beta=beta, n_iter_max=2, unstored="missing")
            with pytest.raises(InvalidArgumentValue, match="beta"):
                compute_ntf(Tc, rt, F0, update_rule="mu", beta=beta, n_iter_max=2, unstored="missing")
            with pytest.raises(InvalidArgumentValue, match="beta"):
                one_ntf_step(Tc, rt, F0, None, "mu", beta, [None] * 3, [], [False] * 3, unstored="missing")
        # group=, nndsvd, rank 130, orders 6 and 2: as with the stored-zero reading
        with pytest.raises(NotImplementedError, match="group"):
            compute_nmf(X, r, U0, V0, n_iter_max=2, update_rule="mu", group=object(), unstored="missing")
        with pytest.raises(NotImplementedError, match="group"):
            compute_sparse_ntf(Tc, rt, F0, n_iter_max=2, update_rule="mu", group=object(), unstored="missing")
        with pytest.raises(NotImplementedError, match="nndsvd"):
            nmf(X, r, init="nndsvd", update_rule="mu", n_iter_max=2, unstored="missing")
        with pytest.raises(NotImplementedError, match="nndsvd"):
            ntf(Tc, rt, init="nndsvd", update_rule="mu", n_iter_max=2, unstored="missing")
        with pytest.raises(EngineError, match="rank 130"):
            nmf(X, 130, init="custom", U_0=rng.random((300, 130)), V_0=rng.random((130, 200)), update_rule="mu", n_iter_max=2,
                unstored="missing")
        with pytest.raises(EngineError, match="rank 130"):
            compute_nmf(X, 130, rng.random((300, 130)), rng.random((130, 200)), n_iter_max=2, update_rule="mu", beta=0.5,
                        unstored="missing")
        with pytest.raises(EngineError, match="rank 130"):
            compute_ntf(Tc, 130, [rng.random((d, 130)) for d in T.shape], n_iter_max=2, update_rule="mu", unstored="missing")
        six = SparseCOO(np.zeros((6, 1), np.int64), np.ones(1), (3,) * 6)
        with pytest.raises(NotImplementedError, match="order 6"):
            compute_ntf(six, 2, [rng.random((3, 2)) for _ in range(6)], n_iter_max=2, update_rule="mu", unstored="missing")
        with pytest.raises(NotImplementedError, match="order 6"):
            ntf(six, 2, update_rule="mu", n_iter_max=2, unstored="missing")
        two = SparseCOO(np.zeros((2, 1), np.int64), np.ones(1), (3, 3))
        with pytest.raises(NotImplementedError, match="nmf"):
            compute_ntf(two, 2, [rng.random((3, 2)) for _ in range(2)], n_iter_max=2, update_rule="mu", unstored="missing")
        with pytest.raises(NotImplementedError, match="nmf"):
            ntf(two, 2, update_rule="mu", n_iter_max=2, unstored="missing")
        assert not proxy.reached, proxy.reached
    finally:
        eng.lib = real


def _peak_of(run):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - live, live


def test_no_dense_copy_of_data_that_would_not_fit(built_lib):
    """A 20000^3 tensor with 5000 stored entries (3.2e13 bytes dense: the shape of tests/test_gpu_sparse_ntf.py) and a
    200000 x 200000 matrix with 5000 (1.6e11 bytes): two iterations at beta = 1 and at beta = 0.5 stay below 64 MB of device memory
    for the tensor, and for the matrix below 20 buffers of a factor's size (4 m r bytes each, 128 MB in all: start values, two
    iterations in flight, node-major copies, numerators and denominators) -- a thousandth of the dense size.  The peak of torch's
    allocator over the runs, less what was live before them."""
    from nn_fac_amd.nmf import compute_nmf
    from nn_fac_amd.ntf import compute_ntf
    import scipy.sparse as sp
    n, nnz, r = 20000, 5000, 8
    rng = np.random.default_rng(11)
    coords = np.unique(rng.integers(0, n, size=(nnz, 3)), axis=0)
    X = ts.Coo(coords, f32(rng.random(len(coords)) + 0.1), (n, n, n))
    F0 = [f32(rng.random((n, r))) for _ in range(3)]

    def tensor_runs():
        for beta in (1, 0.5):
            factors, costs, _ = compute_ntf(tx.coo(X), r, F0, n_iter_max=2, tol=0, update_rule="mu", beta=beta,
                                            sparsity_coefficients=[None] * 3, normalize=[False] * 3, return_costs=True, unstored="missing")
            assert len(costs) == 2 and np.isfinite(costs).all() and all(F.shape == (n, r) and np.isfinite(F).all() for F in factors)
    peak, live = _peak_of(tensor_runs)
    print("tensor: peak device memory of the runs:", peak, "live before them:", live)
    assert peak < 64 * 2 ** 20
    m = 200000
    at = np.unique(rng.integers(0, m, size=(nnz, 2)), axis=0)
    A = sp.csr_matrix((f32(rng.random(len(at)) + 0.1), (at[:, 0], at[:, 1])), shape=(m, m))
    U0, V0 = f32(rng.random((m, r))), f32(rng.random((r, m)))

    def matrix_runs():
        for beta in (1, 0.5):
            U, V, costs, _ = compute_nmf(A, r, U0, V0, n_iter_max=2, tol=0, update_rule="mu", beta=beta, return_costs=True,
                                         unstored="missing")
            assert len(costs) == 2 and np.isfinite(costs).all() and np.isfinite(U).all() and np.isfinite(V).all()
    peak, live = _peak_of(matrix_runs)
    print("matrix: peak device memory of the runs:", peak, "live before them:", live)
    assert peak < 20 * 4 * m * r

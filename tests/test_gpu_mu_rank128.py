"""The fused beta-divergence updates at ranks 65 .. 128 (MT = 5 .. 8 rank tiles): nnf_mu_left_f32, nnf_mu_right_f32 and
nnf_mu_right_accum_f32 form U V tile by tile inside the kernel for every beta != 2 -- no m x n operand is written anywhere.
Tolerances are the ones the fused kernels already carry below rank 65 (test_gpu_kernels.py: rel_fro < 2e-5, no entry off by
1e-3 relative; drivers 5e-5 / NTD 1e-4).  Needs a MI355X."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import nnfac_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = [65, 80, 81, 96, 97, 100, 112, 113, 127, 128]      # both edges of every 16-rank tile from the fifth to the eighth
BETAS = [0, 0.5, 1, 1.5, 3, 4]
# (m, n, floats of NaN padding behind every row): aligned rows / n % 4 != 0 behind a 5-float padding / fewer than 16 rows /
# fewer than 16 columns behind an aligned padding
SHAPES = [(260, 132, 0), (150, 71, 5), (11, 203, 0), (203, 9, 7)]


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    assert torch.cuda.is_available()
    return get_engine("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def padded(a, pad):
    """Device copy of `a` as a row-strided view whose padding holds NaN."""
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
    t[:, :a.shape[1]] = torch.tensor(np.asarray(a), dtype=torch.float32)
    return t[:, :a.shape[1]]


def nan_like(rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float32, device="cuda")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), what
    r, worst = rel(got, want), float(np.max(np.abs(got - want) / np.abs(want)))
    assert r < 2e-5 and worst < 1e-3, (what, r, worst)


def problem(m, n, r, seed):
    rng = np.random.RandomState(seed)
    U = rng.rand(m, r) + 0.05
    V = rng.rand(r, n) + 0.05
    X = rng.rand(m, r) @ rng.rand(r, n) + 0.05
    return tuple(a.astype(np.float32).astype(np.float64) for a in (X, U, V))


def abi_calls(eng, Xd, Utd, Vd, r, beta):
    """The three entry points through ctypes on NaN-filled outputs: (status codes, Ut_out, V_out, num, den, den_vec)."""
    from nn_fac_amd.engine import _ptr, _ld
    m, n = Xd.shape
    Uo, Vo, num = nan_like(r, m), nan_like(r, n), nan_like(r, n)
    den = nan_like(r, n)
    dvec = torch.full((r,), float("nan"), dtype=torch.float64, device="cuda")
    st = eng._stream()
    args = (eng.ctx, _ptr(Xd), m, n, _ld(Xd), _ptr(Utd), _ld(Utd), _ptr(Vd), _ld(Vd), r, float(beta))
    rc = [eng.lib.nnf_mu_left_f32(*args, _ptr(Uo), _ld(Uo), st),
          eng.lib.nnf_mu_right_f32(*args, _ptr(Vo), _ld(Vo), st),
          eng.lib.nnf_mu_right_accum_f32(*args, _ptr(num), _ld(num), _ptr(den), _ld(den), _ptr(dvec), st)]
    torch.cuda.synchronize()
    return rc, Uo, Vo, num, den, dvec


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("beta", BETAS)
def test_abi_takes_ranks_65_to_128(eng, r, beta):
    """Every entry point returns NNF_OK and matches an fp64 evaluation of mu.py:84-97 (outputs pre-filled with NaN; ragged
    shapes, unaligned rows, NaN in the padding between rows)."""
    for m, n, pad in SHAPES:
        X, U, V = problem(m, n, r, 1000 * r + m + n)
        Xd, Utd, Vd = padded(X, pad), padded(U.T.copy(), pad), padded(V, pad)
        rc, Uo, Vo, num, den, dvec = abi_calls(eng, Xd, Utd, Vd, r, beta)
        assert rc == [0, 0, 0], (rc, m, n, pad)
        tag = (m, n, pad)
        close(Uo.cpu().numpy().T, orc.mu_betadivmin(U, V, X, beta), ("left", tag))
        close(Vo.cpu().numpy(), orc.switch_alternate_mu(X, U, V, beta, "V"), ("right", tag))
        K = U @ V
        close(num.cpu().numpy(), U.T @ (K ** (beta - 2.0) * X), ("accum num", tag))
        if beta == 1:
            np.testing.assert_allclose(dvec.cpu().numpy(), U.sum(axis=0), rtol=1e-12)
            assert torch.isnan(den).all()           # (beta = 1: `den` is not used)
        else:
            close(den.cpu().numpy(), U.T @ K ** (beta - 1.0), ("accum den", tag))
            assert torch.isnan(dvec).all()


@pytest.mark.parametrize("beta", [1, 0.5])
def test_rank_129_is_still_refused(eng, beta):
    X, U, V = problem(150, 140, 129, 5)
    rc, Uo, Vo, num, den, dvec = abi_calls(eng, dev(X), dev(U.T), dev(V), 129, beta)
    assert rc == [-3, -3, -3]
    for t in (Uo, Vo, num, den, dvec):
        assert torch.isnan(t).all()


@pytest.mark.parametrize("beta", [1, 0.5])
def test_no_data_sized_temporary(eng, beta):
    """Device memory taken during an update stays far below one copy of X (the results are 0.055 of it)."""
    m, n, r = 20000, 2000, 100
    g = torch.Generator(device="cuda").manual_seed(1)
    Ut = torch.rand(r, m, device="cuda", generator=g) + 0.05
    V = torch.rand(r, n, device="cuda", generator=g) + 0.05
    X = torch.rand(m, n, device="cuda", generator=g) + 0.05
    for name in ("mu_left", "mu_right", "mu_right_accum"):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = getattr(eng, name)(X, Ut, V, beta)
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - before
        del out
        assert extra < 0.25 * 4 * m * n, (name, extra, 4 * m * n)


_ROUTE_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
from nn_fac_amd.engine import get_engine
eng = get_engine("cuda:0")
g = torch.Generator(device="cuda").manual_seed(0)
m, n, r = 1000, 600, 100
Ut = torch.rand(r, m, device="cuda", generator=g) + 0.05
V = torch.rand(r, n, device="cuda", generator=g) + 0.05
X = torch.rand(m, n, device="cuda", generator=g) + 0.05
for beta in (1.0, 0.5):
    eng.mu_left(X, Ut, V, beta)
    eng.mu_right(X, Ut, V, beta)
    eng.mu_right_accum(X, Ut, V, beta)
torch.cuda.synchronize()
print("done")
"""


def test_rank_100_takes_the_fused_kernels(built_lib):
    """NNF_PLAN_DEBUG (read once per process: a child): a rank-100 update is one mu_left / mu_right plan with seven rank tiles
    (or six and four leftover ranks) and no plain X H^T / W^T X contraction."""
    p = subprocess.run([sys.executable, "-c", _ROUTE_CHILD], env=dict(os.environ, NNF_PLAN_DEBUG="1"), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    plans = re.findall(r"^\[nnf plan\] (\w+) (.*)$", p.stderr, flags=re.M)
    names = [nm for nm, _ in plans]
    assert names.count("mu_left") == 2 and names.count("mu_right") == 4, names
    assert "xht" not in names and "xty" not in names, names
    for nm, rest in plans:
        if nm in ("mu_left", "mu_right"):
            kv = dict(t.split("=", 1) for t in rest.split())
            assert kv["r"] == "100" and (kv["mt"], kv["rem"]) in (("7", "0"), ("6", "4")), (nm, rest)
    assert {dict(t.split("=", 1) for t in rest.split())["bm"] for nm, rest in plans if nm.startswith("mu_")} == {"KL", "GEN"}


def _device_problem(m, n, r, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Ut = torch.rand(r, m, device="cuda", generator=g) + 0.05
    V = torch.rand(r, n, device="cuda", generator=g) + 0.05
    X = (torch.rand(m, r, device="cuda", generator=g) @ torch.rand(r, n, device="cuda", generator=g)) + 0.05
    return X, Ut, V


def _close_dev(got, want, what):
    r, worst = float((got - want).norm() / want.norm()), float(((got - want).abs() / want).max())
    assert r < 2e-5 and worst < 1e-3, (what, r, worst)     # (worst: no row / column block missed or doubled)


@pytest.mark.parametrize("r", [100, 128])
@pytest.mark.parametrize("m", [98304, 100000, 131100])
@pytest.mark.parametrize("beta", [1, 0.5])
def test_left_update_at_full_height(eng, r, m, beta):
    """test_mu_left_row_tilings' recipe at ranks 100 and 128: an fp64 evaluation of mu.py:84-97 on the device."""
    n = 70
    X, Ut, V = _device_problem(m, n, r, m + r)
    U64, V64, X64 = Ut.double().t(), V.double(), X.double()
    K = U64 @ V64
    if beta == 1:
        want = torch.clamp(U64 * ((X64 / K) @ V64.t() / V64.sum(dim=1)), min=1e-12)
    else:
        want = torch.clamp(U64 * ((K ** (beta - 2) * X64) @ V64.t() / (K ** (beta - 1) @ V64.t())) ** orc.gamma_beta(beta),
                           min=1e-12)
    _close_dev(eng.mu_left(X, Ut, V, beta).double().t(), want, (r, m, beta))


@pytest.mark.parametrize("r", [100, 128])
@pytest.mark.parametrize("n", [2000, 2001])
@pytest.mark.parametrize("beta", [1, 0.5])
def test_right_update_at_full_height(eng, r, n, beta):
    m = 100000
    X, Ut, V = _device_problem(m, n, r, n + r)
    want_num = torch.zeros(r, n, dtype=torch.float64, device="cuda")
    want_den = torch.zeros(r, n, dtype=torch.float64, device="cuda")
    for i0 in range(0, m, 10000):                        # fp64 in row blocks (an fp64 copy of X at once is 1.6 GB)
        U64, X64 = Ut[:, i0:i0 + 10000].double(), X[i0:i0 + 10000].double()
        K = U64.t() @ V.double()
        want_num += U64 @ (K ** (beta - 2) * X64)
        want_den += U64 @ K ** (beta - 1)
    want = torch.clamp(V.double() * (want_num / want_den) ** orc.gamma_beta(beta), min=1e-12)
    _close_dev(eng.mu_right(X, Ut, V, beta).double(), want, (r, n, beta))


@pytest.mark.parametrize("beta", [1, 0.5, 3])
def test_nmf_mu_rank_100_against_the_oracle(built_lib, beta):
    from nn_fac_amd.nmf import compute_nmf
    X, U0, V0 = orc.synth_nmf(3000, 800, 100, seed=3, dtype=np.float32)
    U, V, costs, _ = compute_nmf(X, 100, U0, V0, n_iter_max=3, tol=0, update_rule="mu", beta=beta, return_costs=True,
                                 deterministic=True)
    Uo, Vo, co, _ = orc.compute_nmf(X.astype(np.float64), 100, U0.astype(np.float64), V0.astype(np.float64), n_iter_max=3,
                                    tol=0, update_rule="mu", beta=beta, return_costs=True, deterministic=True)
    assert rel(U, Uo) < 5e-5 and rel(V, Vo) < 5e-5, (rel(U, Uo), rel(V, Vo))
    np.testing.assert_allclose(costs, co, rtol=5e-5)


def test_ntf_mu_with_a_rank_above_64(built_lib):
    """NTF-MU (beta = 1) at rank 72: every mode's update is mu_right on an unfolding."""
    from nn_fac_amd.ntf import compute_ntf
    shape, R = (80, 75, 90), 72
    rng = np.random.RandomState(11)
    gen = [rng.rand(s, R) for s in shape]
    T = (np.einsum("ir,jr,kr->ijk", *gen) + 1e-2 * rng.rand(*shape)).astype(np.float32)
    F0 = [rng.rand(s, R).astype(np.float32) + 0.01 for s in shape]
    kw = dict(n_iter_max=3, tol=0, update_rule="mu", beta=1, return_costs=True, alpha=math.inf,
              sparsity_coefficients=[None] * 3, normalize=[False] * 3)
    F, costs, _ = compute_ntf(T, R, F0, **kw)
    Fo, co, _ = orc.compute_ntf(T.astype(np.float64), R, [f.astype(np.float64) for f in F0], **kw)
    for i in range(3):
        assert rel(F[i], Fo[i]) < 5e-5, (i, rel(F[i], Fo[i]))
    np.testing.assert_allclose(costs, co, rtol=5e-5)


def test_ntd_mu_with_a_rank_above_64(built_lib):
    """NTD-MU (beta = 1) with a first-mode rank of 70: the factor update of that mode is mu_right at rank 70."""
    from nn_fac_amd.ntd import compute_ntd
    shape, ranks = (90, 30, 28), [70, 5, 4]
    rng = np.random.RandomState(12)
    core0 = rng.rand(*ranks).astype(np.float32) + 0.01
    F0 = [rng.rand(s, q).astype(np.float32) + 0.01 for s, q in zip(shape, ranks)]
    gc = rng.rand(*ranks)
    gf = [rng.rand(s, q) for s, q in zip(shape, ranks)]
    T = (np.einsum("abc,ia,jb,kc->ijk", gc, *gf) + 1e-2 * rng.rand(*shape)).astype(np.float32)
    kw = dict(n_iter_max=3, tol=0, update_rule="mu", beta=1, sparsity_coefficients=[None] * 4, normalize=[False] * 4,
              return_costs=True, deterministic=True)
    core, facs, costs, _ = compute_ntd(T, list(ranks), core0, F0, fixed_modes=[], **kw)
    wc, wf, wcosts, _ = orc.compute_ntd(T.astype(np.float64), list(ranks), core0.astype(np.float64),
                                        [f.astype(np.float64) for f in F0], **kw)
    assert rel(core, wc) < 1e-4, rel(core, wc)
    for i in range(3):
        assert rel(facs[i], wf[i]) < 1e-4, (i, rel(facs[i], wf[i]))
    np.testing.assert_allclose(costs, wcosts, rtol=1e-4)


@pytest.mark.parametrize("beta", [1, 0.5])
def test_two_calls_are_bitwise_equal(eng, beta):
    X, Ut, V = _device_problem(30000, 1000, 100, 9)
    for name in ("mu_left", "mu_right"):
        a = getattr(eng, name)(X, Ut, V, beta).clone()
        b = getattr(eng, name)(X, Ut, V, beta)
        assert torch.equal(a, b), name
    a, b = eng.mu_right_accum(X, Ut, V, beta), eng.mu_right_accum(X, Ut, V, beta)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)

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
# both edges of every 16-rank tile from the fifth to the eighth; both sides of the last tile's 2-or-4-step flag (r % 16 == 8 / 9:
# 72 / 73, 88 / 89, 104 / 105, 120 / 121) and ranks that are no multiple of 4 (70, 126)
RANKS = [65, 70, 72, 73, 80, 81, 88, 89, 96, 97, 100, 104, 105, 112, 113, 120, 121, 126, 127, 128]
EDGE_RANKS = (65, 100, 128)
BETAS = [0, 0.5, 1, 1.5, 3, 4]
# (m, n, floats of NaN padding behind every row): aligned rows / n % 4 != 0 behind a 5-float padding / fewer than 16 rows /
# fewer than 16 columns behind an aligned padding
SHAPES = [(260, 132, 0), (150, 71, 5), (11, 203, 0), (203, 9, 7)]
# at EDGE_RANKS: the 128-column workgroups and 32-column waves of the right kernel and the 64-column chunks of the left one, at
# one, two and one-and-a-half 128-row workgroups; rows as they come (m = 70), padded to aligned rows (129), behind 7 floats (193)
EDGE_SHAPES = [(m, n, {70: 0, 129: -n % 4, 193: 7}[m]) for m in (70, 129, 193) for n in (1, 31, 32, 33, 127, 128, 129)]


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
    for m, n, pad in SHAPES + (EDGE_SHAPES if r in EDGE_RANKS else []):
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


@pytest.mark.parametrize("r", [65, 100, 121])
@pytest.mark.parametrize("beta", [1, 0.5])
def test_factor_rows_beyond_the_rank_are_not_read(eng, r, beta):
    """Ut and V as the first r rows of buffers with 16 ceil(r / 16) + 8 rows whose other rows hold NaN: the rank tiles are padded
    with zeros, never with the rows that follow in memory.  All three entry points, bit for bit what exact-size factors give."""
    for m, n, pad in [(260, 132, 0), (150, 71, 0)]:          # (aligned X: rank 100 as six tiles + four ranks; unaligned: seven tiles)
        X, U, V = problem(m, n, r, 7 * r + m)
        Xd = padded(X, pad)
        exact = abi_calls(eng, Xd, dev(U.T), dev(V), r, beta)
        rows = 16 * math.ceil(r / 16) + 8
        Ub, Vb = nan_like(rows, m), nan_like(rows, n)
        Ub[:r], Vb[:r] = dev(U.T), dev(V)
        view = abi_calls(eng, Xd, Ub[:r], Vb[:r], r, beta)
        assert exact[0] == view[0] == [0, 0, 0]
        for a, b, what in zip(exact[1:4], view[1:4], ("left", "right", "accum num")):
            assert torch.isfinite(b).all() and torch.equal(a, b), (what, m, n)
        a, b = (exact[5], view[5]) if beta == 1 else (exact[4], view[4])
        assert torch.isfinite(b).all() and torch.equal(a, b), ("accum den", m, n)


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


# ---- 32-bit offsets: the strides the launchers refuse, and the last ones they take ----
LIM = 0x7fff0000


def _last_stride(mt, length):
    """(ok, bad): the largest row stride of the staged factor with 16 (MT + 1) ld 4 + 4 (length + 128) < LIM -- the chunk images
    address MT + 1 tiles of 16 rows from one 32-bit offset -- and the next multiple of 4 above it."""
    ok = (LIM - 4 * (length + 128) - 1) // (64 * (mt + 1))
    assert 64 * (mt + 1) * ok + 4 * (length + 128) < LIM <= 64 * (mt + 1) * (ok + 1) + 4 * (length + 128)
    return ok, 4 * (ok // 4 + 1)


def _strided(buf, rows, cols, ld, values):
    """`values` as a rows x cols view of row stride ld into the NaN-filled flat buffer."""
    buf.fill_(float("nan"))
    view = buf.as_strided((rows, cols), (ld, 1))
    view.copy_(values)
    return view


def _wrappers_refuse(eng, names, X, Ut, V, beta):
    from nn_fac_amd.engine import EngineError
    for name in names:
        with pytest.raises(EngineError, match=r"status -3 "):       # NNF_ERR_UNSUPPORTED: no composed route behind it
            getattr(eng, name)(X, Ut, V, beta)


@pytest.mark.parametrize("r", [64, 65, 128])
@pytest.mark.parametrize("beta", [1, 0.5])
def test_right_update_factor_stride_limit(eng, r, beta):
    """nnf_mu_right_f32 and nnf_mu_right_accum_f32 stage Ut through LDS: the largest stride they take (and the largest that
    keeps 16-byte loads) against fp64, the next multiple of 4 refused with NNF_ERR_UNSUPPORTED and nothing written.  The
    wrappers raise: a stride of millions of floats under a factor a few hundred wide is no layout the drivers produce, and
    the composed route (m x n scratch, two more passes) behind a refusal would hide it.  Device memory: the factor's buffer, 2.15 GB at
    every rank (16 (MT + 1) rows of the limit stride, by its size; not read from the allocator's peak)."""
    import test_gpu_launch_plans as plans
    m, n, mt = 300, 72, -(-r // 16)
    ok, bad = _last_stride(mt, m)
    X, Ut0, V = _device_problem(m, n, r, 3 * r)
    buf = torch.empty(16 * (mt + 1) * bad, device="cuda")       # (every row a chunk image could address: NaN, not foreign memory)
    want_num, want_den = plans.mu_right_terms_fp64(X, Ut0, V, beta)
    want = plans.mu_right_fp64(X, Ut0, V, beta)
    for ld in sorted({ok, ok - ok % 4}):
        Ut = _strided(buf, r, m, ld, Ut0)
        rc, _, Vo, num, den, dvec = abi_calls(eng, X, Ut, V, r, beta)
        assert rc == [0, 0, 0], (ld, rc)
        plans.assert_close(Vo, want, 2e-5, 1e-3, ("right", ld))
        plans.assert_close(num, want_num, 2e-5, 1e-3, ("accum num", ld))
        if beta == 1:
            assert float(((dvec - want_den).abs() / want_den).max()) <= 1e-12
        else:
            plans.assert_close(den, want_den, 2e-5, 1e-3, ("accum den", ld))
    Ut = _strided(buf, r, m, bad, Ut0)
    rc, Uo, Vo, num, den, dvec = abi_calls(eng, X, Ut, V, r, beta)
    assert rc == [0, -3, -3], rc                       # (the left update reads Ut directly: no limit on ldu)
    plans.assert_close(Uo, plans.mu_left_fp64(X, Ut0, V, beta), 2e-5, 1e-3, ("left", bad))
    for t in (Vo, num, den, dvec):
        assert torch.isnan(t).all()
    _wrappers_refuse(eng, ("mu_right", "mu_right_accum"), X, Ut, V, beta)


@pytest.mark.parametrize("r", [64, 65, 128])
@pytest.mark.parametrize("beta", [1, 0.5])
def test_left_update_factor_stride_limit(eng, r, beta):
    """The same for nnf_mu_left_f32 and the stride of V.  Device memory as above."""
    import test_gpu_launch_plans as plans
    m, n, mt = 300, 72, -(-r // 16)
    ok, bad = _last_stride(mt, n)
    X, Ut, V0 = _device_problem(m, n, r, 5 * r)
    buf = torch.empty(16 * (mt + 1) * bad, device="cuda")
    want = plans.mu_left_fp64(X, Ut, V0, beta)
    for ld in sorted({ok, ok - ok % 4}):
        V = _strided(buf, r, n, ld, V0)
        rc, Uo, _, _, _, _ = abi_calls(eng, X, Ut, V, r, beta)
        assert rc == [0, 0, 0], (ld, rc)
        plans.assert_close(Uo, want, 2e-5, 1e-3, ("left", ld))
    V = _strided(buf, r, n, bad, V0)
    rc, Uo, Vo, _, _, _ = abi_calls(eng, X, Ut, V, r, beta)
    assert rc == [-3, 0, 0], rc                        # (the right update reads V directly: no limit on ldv)
    assert torch.isnan(Uo).all()
    plans.assert_close(Vo, plans.mu_right_fp64(X, Ut, V0, beta), 2e-5, 1e-3, ("right", bad))
    _wrappers_refuse(eng, ("mu_left",), X, Ut, V, beta)


@pytest.mark.parametrize("r,beta", [(64, 1), (65, 1), (100, 1), (128, 1), (128, 0.5)])
def test_left_update_x_stride_limit(eng, r, beta):
    """The left kernel addresses 64 rows of X from one 32-bit offset: 64 ldx 4 + 4 (n + 128) < LIM.  200 rows of a NaN-filled
    buffer at the last stride taken (a multiple of 4: 16-byte loads) and the one below it against fp64, the next one refused.
    Device memory: the buffer under X, 8.6 GB by its size."""
    import test_gpu_launch_plans as plans
    m, n = 200, 72
    ok = (LIM - 4 * (n + 128) - 1) // 256
    assert ok % 4 == 0 and 256 * ok + 4 * (n + 128) < LIM <= 256 * (ok + 1) + 4 * (n + 128)
    X0, Ut, V = _device_problem(m, n, r, 7 * r)
    buf = torch.empty(256 * (ok + 1), device="cuda")            # (whole 128-row workgroups)
    want = plans.mu_left_fp64(X0, Ut, V, beta)
    for ld in (ok - 1, ok):
        X = _strided(buf, m, n, ld, X0)
        rc = abi_calls(eng, X, Ut, V, r, beta)
        assert rc[0][0] == 0, (ld, rc[0])
        plans.assert_close(rc[1], want, 2e-5, 1e-3, ("left", ld))
    X = _strided(buf, m, n, ok + 1, X0)
    rc = abi_calls(eng, X, Ut, V, r, beta)
    assert rc[0][0] == -3 and torch.isnan(rc[1]).all(), rc[0]
    _wrappers_refuse(eng, ("mu_left",), X, Ut, V, beta)

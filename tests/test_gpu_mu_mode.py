"""nnf_mu_mode_f32: the beta-divergence MU update of one mode's factor on the tensor's own layout, T seen as (L, I, K), and the
NTF / NTD MU drivers on top of it (no unfolding of T is made up to rank 64).  Kernel tolerances are the ones the fused MU kernels
carry (test_gpu_mu_rank128.close: rel_fro < 2e-5, no entry off by 1e-3 relative, against fp64); drivers 5e-5 (NTF) and 1e-4 (NTD)
against the oracle.  Needs a MI355X.

The edges of the implementation (nn_fac_amd/csrc/k_mu_plan.h, k_mu_mode.hip), each run from both sides:
  rows of I     64 per workgroup (MU_MODE_ROWS), 16 per wave                    I in 15 .. 17, 63 .. 65, 127 .. 129
  k per unit    16 (one MFMA tile; a unit never straddles two l), 4 units per staged chunk: 64 k when K % 16 == 0
                                                                                K in 15 .. 17, 63 .. 65, 127 .. 129
  splits        whole chunks of 4 units each, the last one ragged; a split may start and end in the middle of an l
                (L = 2 and 3 with K = 127 .. 129: 16 / 18 units per l)
  16-byte loads K % 4 == 0 and a pitch of V that is a multiple of 4 (else scalar loads)   pads 0 / 4 / 5 below
  ranks         tiles of 16 (16 | 17, 32 | 33, 48 | 49, 64 | 65 refused), rank steps of 4 inside a tile (3, 20, 50)
  chain         at most 256 units per split unless the workspace holds fewer slabs: 256 | 260 units per split (64 | 65 chunks per
                workgroup, the prefetch hand-off between chunks and the carry of (l, k) across l) on a context whose workspace
                holds two splits, and an occupancy-bound shape of several chunks per workgroup on the default context -- both
                with 16-byte and with scalar loads at every rank-tile count (test_mu_mode_plan.MANY_CHUNKS, BY_OCCUPANCY, whose
                plans tests/test_mu_mode_plan.py pins at 256 and 304 CUs)
Measured on a MI355X over the 1566 cases of test_kernel_against_fp64: rel_fro <= 3.5e-7 and no entry off by more than 4.1e-7 relative."""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import nnfac_oracle as orc
from test_gpu_mu_rank128 import close, dev, nan_like, padded, rel
from test_mu_mode_plan import BY_OCCUPANCY, MANY_CHUNKS, MANY_CHUNKS_RANKS, carved

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKS = [1, 3, 16, 17, 20, 32, 33, 48, 49, 50, 64]
EDGE_RANKS = (1, 20, 64)
BETAS = [0, 0.5, 1, 1.5, 2, 3]
SHAPES = [(1, 70, 203), (5, 33, 71), (7, 16, 64), (3, 130, 129), (40, 9, 5), (6, 1, 50), (9, 50, 1), (1, 1, 1), (2, 260, 260)]
EDGE_SHAPES = ([(2, I, K) for I in (15, 16, 17, 63, 64, 65) for K in (15, 16, 17, 63, 64, 65)] +
               [(L, I, K) for L in (2, 3) for I in (127, 128, 129) for K in (127, 128, 129)])


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    assert torch.cuda.is_available()
    return get_engine("cuda:0")


@functools.lru_cache(maxsize=None)
def problem(L, I, K, r):
    """Strictly positive, rounded to fp32: T (L, I, K) whose mode-1 unfolding is a low-rank product + 0.05, F (I x r), V (r x L K)."""
    rng = np.random.RandomState(1000 * r + 31 * L + 7 * I + K)
    F = rng.rand(I, r) + 0.05
    V = rng.rand(r, L * K) + 0.05
    M = rng.rand(I, r) @ rng.rand(r, L * K) + 0.05
    T = np.ascontiguousarray(M.reshape(I, L, K).transpose(1, 0, 2))
    return tuple(a.astype(np.float32).astype(np.float64) for a in (T, F, V))


@functools.lru_cache(maxsize=None)
def want(L, I, K, r, beta):
    T, F, V = problem(L, I, K, r)
    return orc.mu_betadivmin(F, V, np.moveaxis(T, 1, 0).reshape(I, L * K), beta)


def pad_of(L, I, K):
    """NaN floats behind every row of Ft and V: none, an aligned pitch, an unaligned pitch -- by the shape."""
    return (0, 4 + (-(L * K)) % 4, 5)[(L + I + K) % 3]


def abi_call(eng, Td, Ftd, Vd, r, beta, out=None, shape=None):
    from nn_fac_amd.engine import _ptr, _ld
    L, I, K = shape or Td.shape
    out = nan_like(r, I) if out is None else out
    rc = eng.lib.nnf_mu_mode_f32(eng.ctx, _ptr(Td), L, I, K, _ptr(Ftd), _ld(Ftd), _ptr(Vd), _ld(Vd), r, float(beta), _ptr(out),
                                 _ld(out), eng._stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("beta", BETAS)
def test_kernel_against_fp64(eng, r, beta):
    """Through ctypes on a NaN-filled output, Ft and V as row-strided views whose padding holds NaN."""
    for L, I, K in SHAPES + (EDGE_SHAPES if r in EDGE_RANKS else []):
        T, F, V = problem(L, I, K, r)
        pad = pad_of(L, I, K)
        rc, out = abi_call(eng, dev(T), padded(F.T.copy(), pad), padded(V, pad), r, beta)
        assert rc == 0, (rc, L, I, K)
        close(out.cpu().numpy().T, want(L, I, K, r, beta), (L, I, K, r, beta, pad))


@pytest.mark.parametrize("r", MANY_CHUNKS_RANKS)
@pytest.mark.parametrize("beta", [1, 0.5, 2])
def test_many_chunks_per_workgroup(eng, r, beta):
    """A workgroup walks 64 | 65 chunks (256 | 260 units, two whole l) where a two-split workspace bounds the plan, and 2 .. 5 where
    the default context splits by occupancy: every chunk after the first comes through the prefetch registers."""
    from nn_fac_amd.engine import Engine
    for L, I, K in MANY_CHUNKS:
        small = Engine(torch.device("cuda:0"), workspace_bytes=carved(r, I, 1, 2, beta == 1))
        T, F, V = problem(L, I, K, r)
        rc, out = abi_call(small, dev(T), dev(F.T.copy()), dev(V), r, beta)
        assert rc == 0, (rc, L, I, K)
        close(out.cpu().numpy().T, want(L, I, K, r, beta), (L, I, K, r, beta))
        del small
    L, I, K = BY_OCCUPANCY
    T, F, V = problem(L, I, K, r)
    rc, out = abi_call(eng, dev(T), dev(F.T.copy()), dev(V), r, beta)
    assert rc == 0
    close(out.cpu().numpy().T, want(L, I, K, r, beta), (L, I, K, r, beta))


_SPLIT_CHILD = r"""
import sys, os, numpy as np, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from nn_fac_amd.engine import Engine, get_engine
d = np.load(sys.argv[1])
T, Ft, V = (torch.from_numpy(d[k]).cuda() for k in ("T", "Ft", "V"))
small = Engine(torch.device("cuda:0"), workspace_bytes=int(sys.argv[3]))
res = {}
for name, e in (("default", get_engine("cuda:0")), ("small", small)):
    for beta in (1.0, 0.5):
        sys.stderr.write("[case] %s %r\n" % (name, beta))
        sys.stderr.flush()
        res["%s %r" % (name, beta)] = e.mu_mode(T, Ft, V, beta).cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[2], **res)
print("done")
"""


def test_column_splits_and_row_blocks(built_lib, tmp_path):
    """NNF_PLAN_DEBUG (read once per process: a child): (3, 130, 129) at rank 20 runs as 3 row blocks x 7 column splits on the
    default context; a context whose workspace holds two splits' slabs (of the general-beta form: two sets; four of beta = 1)
    runs it in that many -- split by the workspace alone.  Both against fp64."""
    from test_gpu_launch_plans import parse_plans
    L, I, K, r = 3, 130, 129, 20
    T, F, V = problem(L, I, K, r)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, T=T.astype(np.float32), Ft=np.ascontiguousarray(F.T, dtype=np.float32), V=V.astype(np.float32))
    ws = carved(r, I, 0, 2, False)
    p = subprocess.run([sys.executable, "-c", _SPLIT_CHILD, src, dst, str(ws)], env=dict(os.environ, NNF_PLAN_DEBUG="1"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    plans, got = parse_plans(p.stderr), np.load(dst)
    for beta in (1.0, 0.5):
        for name in ("default", "small"):
            key = "%s %r" % (name, beta)
            lines = [kv for nm, kv in plans[key] if nm == "mu_mode"]
            assert len(lines) == 1, plans[key]
            kv = lines[0]
            assert (kv["L"], kv["I"], kv["K"], kv["r"], kv["nrb"]) == ("3", "130", "129", "20", "3"), kv
            if name == "default":
                assert int(kv["nsplit"]) == 7 and kv["bound"] == "min_cols", kv
            else:
                assert 2 <= int(kv["nsplit"]) <= (4 if beta == 1.0 else 2) and kv["bound"] == "workspace", kv
            close(got[key].T, want(L, I, K, r, beta), (key, kv))


@pytest.mark.parametrize("beta", [1, 0.5, 2])
@pytest.mark.parametrize("I,K,r", [(70, 203, 20), (130, 1000, 33), (33, 64, 64)])
def test_first_mode_against_mu_left(eng, I, K, r, beta):
    """L = 1: the tensor is the I x K matrix of nnf_mu_left_f32.  Same operands, same tolerance."""
    T, F, V = problem(1, I, K, r)
    Td, Ftd, Vd = dev(T), dev(F.T.copy()), dev(V)
    got = eng.mu_mode(Td, Ftd, Vd, beta)
    ref = eng.mu_left(Td[0], Ftd, Vd, beta)
    close(got.cpu().numpy(), ref.cpu().numpy(), (I, K, r, beta))
    close(got.cpu().numpy().T, want(1, I, K, r, beta), (I, K, r, beta, "fp64"))


@pytest.mark.parametrize("r", [3, 20, 50])
@pytest.mark.parametrize("beta", [1, 0.5])
def test_factor_rows_beyond_the_rank_are_not_read(eng, r, beta):
    """Ft and V as the first r rows of buffers with 16 ceil(r / 16) + 8 rows whose other rows hold NaN: bit for bit what
    exact-size factors give."""
    for L, I, K in [(2, 260, 260), (5, 33, 71)]:
        T, F, V = problem(L, I, K, r)
        Td = dev(T)
        rc0, exact = abi_call(eng, Td, dev(F.T.copy()), dev(V), r, beta)
        rows = 16 * math.ceil(r / 16) + 8
        Fb, Vb = nan_like(rows, I), nan_like(rows, L * K)
        Fb[:r], Vb[:r] = dev(F.T.copy()), dev(V)
        rc1, view = abi_call(eng, Td, Fb[:r], Vb[:r], r, beta)
        assert rc0 == rc1 == 0
        assert torch.isfinite(view).all() and torch.equal(exact, view), (L, I, K)


@pytest.mark.parametrize("beta", [1, 0.5])
def test_two_calls_are_bitwise_equal(eng, beta):
    """(12, 200, 400) at rank 30: 4 row blocks x 75 column splits of 4 units."""
    T, F, V = problem(12, 200, 400, 30)
    Td, Ftd, Vd = dev(T), dev(F.T.copy()), dev(V)
    a = eng.mu_mode(Td, Ftd, Vd, beta).clone()
    b = eng.mu_mode(Td, Ftd, Vd, beta)
    assert torch.equal(a, b)
    close(a.cpu().numpy().T, want(12, 200, 400, 30, beta), beta)


def test_refusals(eng):
    L, I, K = 5, 33, 71
    T, F, V = problem(L, I, K, 64)
    Td, Vd = dev(T), dev(V)
    Ftd = dev(F.T.copy())
    F65, V65 = torch.rand(65, I, device="cuda") + 0.05, torch.rand(65, L * K, device="cuda") + 0.05
    rc, out = abi_call(eng, Td, F65, V65, 65, 1)
    assert rc == -3 and torch.isnan(out).all()
    rc, out = abi_call(eng, Td, Ftd, Vd, 64, 1)
    assert rc == 0
    close(out.cpu().numpy().T, want(L, I, K, 64, 1), "rank 64")
    from nn_fac_amd.engine import _ptr
    out = nan_like(64, I)
    st = eng._stream()

    def call(T_=Td, F_=Ftd, V_=Vd, O_=out, ldf=I, ldv=L * K, ldo=I, ctx=None, dims=(L, I, K), beta=1.0):
        p = [None if t is None else _ptr(t) for t in (T_, F_, V_, O_)]
        rc = eng.lib.nnf_mu_mode_f32(eng.ctx if ctx is None else ctx, p[0], *dims, p[1], ldf, p[2], ldv, 64, beta, p[3], ldo, st)
        torch.cuda.synchronize()
        return rc
    assert call() == 0
    out.fill_(float("nan"))
    assert call(T_=None) == call(F_=None) == call(V_=None) == call(O_=None) == -1
    assert call(ldf=I - 1) == call(ldv=L * K - 1) == call(ldo=I - 1) == -1
    assert call(dims=(0, I, K)) == call(dims=(L, 0, K)) == call(dims=(L, I, 0)) == call(beta=-0.5) == call(beta=float("nan")) == -1
    assert torch.isnan(out).all()
    from nn_fac_amd.engine import EngineError
    with pytest.raises(EngineError):
        eng.mu_mode(Td, F65, V65, 1)
    with pytest.raises(EngineError):
        eng.mu_mode(Td[:, :, :-1], Ftd, Vd, 1)          # not contiguous


@pytest.mark.parametrize("beta", [1, 0.5])
def test_workspace_limit(built_lib, beta):
    """The launcher's size limit is the workspace: one byte short of one split's slabs (one set for beta = 1, two otherwise;
    behind the r doubles of the row sums) is refused with NNF_ERR_WORKSPACE and nothing is written; exactly that many bytes run
    the whole update as one split, against fp64."""
    from nn_fac_amd.engine import Engine
    L, I, K, r = 5, 33, 71, 20
    T, F, V = problem(L, I, K, r)
    Td, Ftd, Vd = dev(T), dev(F.T.copy()), dev(V)
    ws = carved(r, I, 1, 1, beta == 1)
    short, enough = (Engine(torch.device("cuda:0"), workspace_bytes=b) for b in (ws - 1, ws))
    rc, out = abi_call(short, Td, Ftd, Vd, r, beta)
    assert rc == -4 and torch.isnan(out).all()
    rc, out = abi_call(enough, Td, Ftd, Vd, r, beta)
    assert rc == 0
    close(out.cpu().numpy().T, want(L, I, K, r, beta), (ws, beta))


# ---- drivers ----
def cp_problem(shape, R, seed):
    rng = np.random.RandomState(seed)
    letters = "ijkl"[:len(shape)]
    gen = [rng.rand(s, R) for s in shape]
    T = (np.einsum(",".join(c + "r" for c in letters) + "->" + letters, *gen) + 0.05).astype(np.float32)
    F0 = [(rng.rand(s, R) + 0.05).astype(np.float32) for s in shape]
    return T, F0


def tucker_problem(shape, ranks, seed):
    rng = np.random.RandomState(seed)
    N = len(shape)
    a, b = "abcd"[:N], "ijkl"[:N]
    spec = a + "," + ",".join(y + x for x, y in zip(a, b)) + "->" + b
    T = (np.einsum(spec, rng.rand(*ranks), *[rng.rand(s, q) for s, q in zip(shape, ranks)]) + 0.05).astype(np.float32)
    core0 = (rng.rand(*ranks) + 0.05).astype(np.float32)
    F0 = [(rng.rand(s, q) + 0.05).astype(np.float32) for s, q in zip(shape, ranks)]
    return T, core0, F0


NTF_CASES = [((33, 17, 21), 5, 1), ((33, 17, 21), 5, 0.5), ((33, 17, 21), 5, 2), ((9, 7, 8, 6), 3, 1)]
NTD_CASES = [((30, 26, 22), (5, 4, 3), 1), ((30, 26, 22), (5, 4, 3), 0.5), ((9, 7, 8, 6), (3, 2, 3, 2), 1)]


@functools.lru_cache(maxsize=None)
def ntf_oracle(shape, R, beta):
    T, F0 = cp_problem(shape, R, sum(shape) + R)
    kw = ntf_kw(len(shape), beta)
    return orc.compute_ntf(T.astype(np.float64), R, [f.astype(np.float64) for f in F0], **kw)


def ntf_kw(N, beta, iters=4):
    return dict(n_iter_max=iters, tol=0, update_rule="mu", beta=beta, return_costs=True, alpha=math.inf,
                sparsity_coefficients=[None] * N, normalize=[False] * N)


def ntd_kw(N, beta, iters=4):
    return dict(n_iter_max=iters, tol=0, update_rule="mu", beta=beta, sparsity_coefficients=[None] * (N + 1),
                normalize=[False] * (N + 1), return_costs=True, deterministic=True)


@functools.lru_cache(maxsize=None)
def ntd_oracle(shape, ranks, beta):
    T, core0, F0 = tucker_problem(shape, ranks, sum(shape) + sum(ranks))
    return orc.compute_ntd(T.astype(np.float64), list(ranks), core0.astype(np.float64), [f.astype(np.float64) for f in F0],
                           **ntd_kw(len(shape), beta))


@pytest.mark.parametrize("unfold", [False, True])
@pytest.mark.parametrize("shape,R,beta", NTF_CASES)
def test_ntf_mu_against_the_oracle(built_lib, monkeypatch, shape, R, beta, unfold):
    from nn_fac_amd.ntf import compute_ntf
    if unfold:
        monkeypatch.setenv("NNF_MU_UNFOLD", "1")
    else:
        monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    T, F0 = cp_problem(shape, R, sum(shape) + R)
    F, costs, _ = compute_ntf(T, R, F0, **ntf_kw(len(shape), beta))
    Fo, co, _ = ntf_oracle(shape, R, beta)
    for i in range(len(shape)):
        assert rel(F[i], Fo[i]) < 5e-5, (i, rel(F[i], Fo[i]))
    np.testing.assert_allclose(costs, co, rtol=5e-5)


@pytest.mark.parametrize("unfold", [False, True])
@pytest.mark.parametrize("shape,ranks,beta", NTD_CASES)
def test_ntd_mu_against_the_oracle(built_lib, monkeypatch, shape, ranks, beta, unfold):
    from nn_fac_amd.ntd import compute_ntd
    if unfold:
        monkeypatch.setenv("NNF_MU_UNFOLD", "1")
    else:
        monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    T, core0, F0 = tucker_problem(shape, ranks, sum(shape) + sum(ranks))
    core, facs, costs, _ = compute_ntd(T, list(ranks), core0, F0, fixed_modes=[], **ntd_kw(len(shape), beta))
    wc, wf, wcosts, _ = ntd_oracle(shape, ranks, beta)
    assert rel(core, wc) < 1e-4, rel(core, wc)
    for i in range(len(shape)):
        assert rel(facs[i], wf[i]) < 1e-4, (i, rel(facs[i], wf[i]))
    np.testing.assert_allclose(costs, wcosts, rtol=1e-4)


@pytest.mark.parametrize("shape,R", [((7, 1, 5), 3), ((17, 5, 1), 1), ((6, 5, 4), 1), ((1, 33, 2), 4)])
@pytest.mark.parametrize("beta", [1, 2, 0.5])
def test_ntf_degenerate_dimensions_on_the_native_route(built_lib, monkeypatch, shape, R, beta):
    """The shapes of test_gpu_ntf.test_ntf_degenerate_dimensions (extents and ranks of 1): finite, non-negative factors, and
    no unfolding was made."""
    from nn_fac_amd import ntf
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    calls = spy_on(monkeypatch, ntf._NtfState)
    T, F0 = orc.synth_ntf(shape, R, seed=sum(shape) + R, dtype=np.float32)
    F, costs, _ = ntf.compute_ntf(T, R, F0, **ntf_kw(3, beta, iters=3))
    assert calls == []
    for f, f0 in zip(F, F0):
        assert f.shape == f0.shape and np.isfinite(f).all() and (f >= 0).all()
    assert np.isfinite(costs).all()


# ---- no unfolding, no tensor-sized allocation ----
def spy_on(monkeypatch, cls):
    calls, orig = [], cls.unfolded_t

    def spy(self, mode):
        calls.append(mode)
        return orig(self, mode)
    monkeypatch.setattr(cls, "unfolded_t", spy)
    return calls


def test_ntf_mu_makes_no_unfolding(built_lib, monkeypatch):
    from nn_fac_amd import ntf
    calls = spy_on(monkeypatch, ntf._NtfState)
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    for shape, R in (((33, 17, 21), 5), ((9, 7, 8, 6), 3), ((20, 70, 18), 64)):
        T, F0 = cp_problem(shape, R, 1)
        ntf.compute_ntf(T, R, F0, **ntf_kw(len(shape), 1, iters=2))
        assert calls == [], (shape, R, calls)
    monkeypatch.setenv("NNF_MU_UNFOLD", "1")                       # the unfolding route: every mode but the last (a view)
    for shape, R in (((33, 17, 21), 5), ((9, 7, 8, 6), 3)):
        del calls[:]
        T, F0 = cp_problem(shape, R, 1)
        ntf.compute_ntf(T, R, F0, **ntf_kw(len(shape), 1, iters=2))
        assert set(calls) == set(range(len(shape) - 1)), (shape, calls)
    monkeypatch.delenv("NNF_MU_UNFOLD")
    del calls[:]
    shape, R = (80, 75, 90), 72                                    # test_ntf_mu_with_a_rank_above_64: unchanged
    T, F0 = cp_problem(shape, R, 11)
    ntf.compute_ntf(T, R, F0, **ntf_kw(3, 1, iters=1))
    assert set(calls) == {0, 1}, calls


def test_ntd_mu_makes_no_unfolding(built_lib, monkeypatch):
    from nn_fac_amd import ntd
    calls = spy_on(monkeypatch, ntd._NtdState)
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    cases = (((30, 26, 22), (5, 4, 3)), ((9, 7, 8, 6), (3, 2, 3, 2)))
    for shape, ranks in cases:
        T, core0, F0 = tucker_problem(shape, ranks, 2)
        ntd.compute_ntd(T, list(ranks), core0, F0, fixed_modes=[], **ntd_kw(len(shape), 1, iters=2))
        assert calls == [], (shape, calls)
    monkeypatch.setenv("NNF_MU_UNFOLD", "1")
    for shape, ranks in cases:
        del calls[:]
        T, core0, F0 = tucker_problem(shape, ranks, 2)
        ntd.compute_ntd(T, list(ranks), core0, F0, fixed_modes=[], **ntd_kw(len(shape), 1, iters=2))
        assert set(calls) == set(range(len(shape) - 1)), (shape, calls)
    monkeypatch.delenv("NNF_MU_UNFOLD")
    del calls[:]
    shape, ranks = (90, 30, 28), (70, 5, 4)                         # test_ntd_mu_with_a_rank_above_64: mode 0 above rank 64
    T, core0, F0 = tucker_problem(shape, ranks, 12)
    ntd.compute_ntd(T, list(ranks), core0, F0, fixed_modes=[], **ntd_kw(3, 1, iters=1))
    assert set(calls) == {0}, calls


def _device_cp(shape, R, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    letters = "ijkl"[:len(shape)]
    gen = [torch.rand(s, R, device="cuda", generator=g) for s in shape]
    T = torch.einsum(",".join(c + "r" for c in letters) + "->" + letters, *gen) + 0.05
    return T.contiguous(), [torch.rand(s, R, device="cuda", generator=g) + 0.05 for s in shape]


def _peak_rise(run):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = run()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


@pytest.mark.parametrize("shape,R", [((128, 96, 160), 4), ((32, 24, 40, 20), 2)])
def test_ntf_mu_allocates_less_than_one_copy_of_the_tensor(eng, monkeypatch, shape, R):
    """A device tensor in, two MU iterations: the peak of the allocator rises by less than one copy of the tensor (what is left are
    the Khatri-Rao operands, sum r / I_n of a copy, and rank-sized intermediates).  With the unfoldings it was N - 1 copies."""
    from nn_fac_amd.ntf import compute_ntf
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    T, F0 = _device_cp(shape, R, 3)
    rise = _peak_rise(lambda: compute_ntf(T, R, F0, **ntf_kw(len(shape), 1, iters=2)))
    assert rise < 4 * T.numel(), (rise, 4 * T.numel())


def test_ntd_mu_allocates_less_than_one_copy_of_the_tensor(eng, monkeypatch):
    from nn_fac_amd.ntd import compute_ntd
    monkeypatch.delenv("NNF_MU_UNFOLD", raising=False)
    shape, ranks = (128, 96, 160), (4, 4, 4)
    T, _ = _device_cp(shape, 4, 5)
    g = torch.Generator(device="cuda").manual_seed(6)
    core0 = torch.rand(*ranks, device="cuda", generator=g) + 0.05
    F0 = [torch.rand(s, q, device="cuda", generator=g) + 0.05 for s, q in zip(shape, ranks)]
    rise = _peak_rise(lambda: compute_ntd(T, list(ranks), core0, F0, fixed_modes=[], **ntd_kw(3, 1, iters=2)))
    assert rise < 4 * T.numel(), (rise, 4 * T.numel())

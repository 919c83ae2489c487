"""nnf_mu_mode_w_f32: the sums of the beta-divergence MU update of one mode's factor under a weight per entry, on the tensor's own
layout (T and Wg seen as (L, I, K)), through ctypes on NaN-filled outputs.  Needs a MI355X.

Reference: fp64 on the device from the fp32 operands, the zero-weight entries of T replaced by 1 first
(test_gpu_weighted_kernels.sums_fp64 on the transposed unfolding, which this call never forms).  Bounds: the project's own for the
weighted sums (test_gpu_weighted_kernels.check_sums: 2e-5 relative Frobenius, 1e-3 per entry, exact zeros in a slice without
weight, nothing non-finite).

The edges, each from both sides, are those of tests/test_gpu_mu_mode.py (rows of I per workgroup and wave, k per unit, units per
chunk, splits that start inside an l, rank tiles and rank steps, many chunks per workgroup on a two-split workspace and by
occupancy) and, new here:
  weights       uniform in (0, 2) with 10 % zeros, one whole i slice zero (num = den = 0 exactly), one whole l slab zero, NaN and
                +-Inf in T under the zeros
  alignment     T alone, Wg alone in a buffer offset by one float (scalar loads), both aligned with K % 4 == 0 (16-byte loads)
  every beta    0, 0.5, 1, 2, 3 through ONE instantiation per rank-tile count and load width
  one slab      a split count of one still goes through the fixed-order slab reduction"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_mu_mode import EDGE_RANKS, EDGE_SHAPES, RANKS, SHAPES, pad_of
from test_gpu_mu_rank128 import nan_like
from test_gpu_weighted_kernels import check_sums, sums_fp64
from test_mu_mode_plan import BY_OCCUPANCY, MANY_CHUNKS, MANY_CHUNKS_RANKS
from test_mu_mode_w_plan import carved_w

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = [0, 0.5, 1, 2, 3]


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    assert torch.cuda.is_available()
    return get_engine("cuda:0")


def offset_copy(t, off):
    """A contiguous copy of `t` that starts `off` floats behind a 16-byte boundary (NaN in front of it)."""
    buf = torch.full((t.numel() + 4,), float("nan"), dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def padded_dev(a, pad):
    """A row-strided view of a copy of the device matrix `a` whose padding holds NaN."""
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=a.device)
    t[:, :a.shape[1]] = a
    return t[:, :a.shape[1]]


@functools.lru_cache(maxsize=None)
def problem(L, I, K, r):
    """On the device, strictly positive where the weight is: T (L, I, K) = a low-rank product + 0.05 with NaN / +-Inf under the
    zero weights, Wg uniform in (0, 2) with 10 % zeros, a whole i slice and a whole l slab of zeros, Ft (r x I), V (r x L K)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * r + 31 * L + 7 * I + K)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)   # noqa: E731
    Ft, V = rnd(r, I) + 0.05, rnd(r, L * K) + 0.05
    T = (torch.einsum("ri,rlk->lik", rnd(r, I), rnd(r, L, K)) + 0.05).contiguous()
    Wg = rnd(L, I, K) * 2 + 1e-3
    Wg[rnd(L, I, K) < 0.1] = 0
    empty = torch.zeros(I, dtype=torch.bool, device="cuda")
    if I > 1:
        empty[I // 2] = True
        Wg[:, I // 2, :] = 0
    if L > 1:
        Wg[L - 1] = 0
    if L == 1 and I == 1:
        Wg[0, 0, 0] = 1.0              # (at least one entry counts)
    empty |= (Wg == 0).all(dim=2).all(dim=0)
    bad = torch.tensor([float("nan"), float("inf"), -float("inf")], device="cuda")
    T = torch.where(Wg == 0, bad[torch.randint(0, 3, T.shape, device="cuda", generator=g)], T)
    return T, Wg, Ft, V, empty


@functools.lru_cache(maxsize=None)
def want(L, I, K, r, beta):
    T, Wg, Ft, V, _ = problem(L, I, K, r)
    unf = lambda A: A.permute(0, 2, 1).reshape(L * K, I)   # noqa: E731  (tl.unfold(., mode)^T of the (L, I, K) view)
    return sums_fp64(unf(T), unf(Wg), V, Ft, beta, "right")


def abi_call(eng, T, Wg, Ft, V, r, beta, num=None, den=None, shape=None):
    from nn_fac_amd.engine import _ptr, _ld
    L, I, K = shape or T.shape
    num = nan_like(r, I) if num is None else num
    den = nan_like(r, I) if den is None else den
    rc = eng.lib.nnf_mu_mode_w_f32(eng.ctx, _ptr(T), _ptr(Wg), L, I, K, _ptr(Ft), _ld(Ft), _ptr(V), _ld(V), r, float(beta),
                                   _ptr(num), _ld(num), _ptr(den), _ld(den), eng._stream())
    torch.cuda.synchronize()
    return rc, num, den


def check(eng, L, I, K, r, beta, align=0, pad=0, what=None):
    """One call against fp64.  align: 0 both aligned, 1 T alone offset by one float, 2 Wg alone."""
    T, Wg, Ft, V, empty = problem(L, I, K, r)
    Td = offset_copy(T, 1) if align == 1 else T
    Wd = offset_copy(Wg, 1) if align == 2 else Wg
    assert (Td.data_ptr() % 16 == 0) == (align != 1) and (Wd.data_ptr() % 16 == 0) == (align != 2)
    rc, num, den = abi_call(eng, Td, Wd, padded_dev(Ft, pad) if pad else Ft, padded_dev(V, pad) if pad else V, r, beta)
    assert rc == 0, (rc, L, I, K, r, beta)
    wn, wd = want(L, I, K, r, beta)
    tag = what or f"L={L} I={I} K={K} r={r} beta={beta} align={align} pad={pad}"
    check_sums(num, wn, empty, tag + " num")
    check_sums(den, wd, empty, tag + " den")
    return num, den


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("beta", BETAS)
def test_kernel_against_fp64(eng, r, beta):
    """Ft and V as row-strided views whose padding holds NaN; T and Wg aligned or one of them offset, by the shape."""
    for L, I, K in SHAPES + (EDGE_SHAPES if r in EDGE_RANKS else []):
        check(eng, L, I, K, r, beta, align=(L + I + K + r) % 3, pad=pad_of(L, I, K))


@pytest.mark.parametrize("r", [1, 20, 33, 64])
@pytest.mark.parametrize("beta", BETAS)
def test_alignment_of_the_tensor_and_of_the_weights(eng, r, beta):
    """K % 4 == 0 (16-byte loads when both are aligned) and K % 4 != 0, each with T alone and Wg alone offset by one float."""
    for L, I, K in [(2, 260, 260), (3, 130, 128), (5, 33, 71)]:
        for align in (0, 1, 2):
            check(eng, L, I, K, r, beta, align=align)


@pytest.mark.parametrize("r", MANY_CHUNKS_RANKS)
@pytest.mark.parametrize("beta", [1, 0.5, 2])
def test_many_chunks_per_workgroup(eng, r, beta):
    """A workgroup walks 64 | 65 chunks (256 | 260 units, two whole l) where a two-split workspace bounds the plan, and several
    where the default context splits by occupancy: every chunk after the first comes through the prefetch registers, the weights
    next to the tensor."""
    from nn_fac_amd.engine import Engine
    for L, I, K in MANY_CHUNKS:
        small = Engine(torch.device("cuda:0"), workspace_bytes=carved_w(r, I, 2))
        check(small, L, I, K, r, beta)
        del small
    check(eng, *BY_OCCUPANCY, r, beta)


_CHILD = r"""
import sys, os, numpy as np, torch
sys.path.insert(0, os.getcwd())
from nn_fac_amd.engine import Engine, get_engine
d = np.load(sys.argv[1])
T, Wg, Ft, V = (torch.from_numpy(d[k]).cuda() for k in ("T", "Wg", "Ft", "V"))
engines = [("default", get_engine("cuda:0"))] + [(n, Engine(torch.device("cuda:0"), workspace_bytes=int(b)))
                                                  for n, b in (("two", sys.argv[3]), ("one", sys.argv[4]))]
res = {}
for name, e in engines:
    for beta in (1.0, 0.5):
        sys.stderr.write("[case] %s %r\n" % (name, beta))
        sys.stderr.flush()
        num, den = e.mu_mode_w(T, Wg, Ft, V, beta)
        res["%s %r num" % (name, beta)], res["%s %r den" % (name, beta)] = num.cpu().numpy(), den.cpu().numpy()
torch.cuda.synchronize()
np.savez(sys.argv[2], **res)
print("done")
"""


def test_the_reported_plan(eng, tmp_path):
    """NNF_PLAN_DEBUG (read once per process: a child): (3, 130, 129) at rank 20 runs as 3 row blocks x 7 column splits on the
    default context (bm=WGEN at beta = 1 too); contexts whose workspace holds two splits' slabs, and one split's, run it in that
    many -- the single slab still through the slab reduction.  All against fp64."""
    from test_gpu_launch_plans import parse_plans
    L, I, K, r = 3, 130, 129, 20
    T, Wg, Ft, V, empty = problem(L, I, K, r)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **{k: v.cpu().numpy() for k, v in (("T", T), ("Wg", Wg), ("Ft", Ft), ("V", V))})
    p = subprocess.run([sys.executable, "-c", _CHILD, src, dst, str(carved_w(r, I, 2)), str(carved_w(r, I, 1))],
                       env=dict(os.environ, NNF_PLAN_DEBUG="1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    plans, got = parse_plans(p.stderr), np.load(dst)
    for beta in (1.0, 0.5):
        wn, wd = want(L, I, K, r, beta)
        for name in ("default", "two", "one"):
            key = "%s %r" % (name, beta)
            lines = [kv for nm, kv in plans[key] if nm == "mu_mode_w"]
            assert len(lines) == 1 and not [nm for nm, _ in plans[key] if nm == "mu_mode"], plans[key]
            kv = lines[0]
            assert (kv["L"], kv["I"], kv["K"], kv["r"], kv["nrb"], kv["bm"], kv["vec"]) == ("3", "130", "129", "20", "3", "WGEN", "0"), kv
            if name == "default":
                assert int(kv["nsplit"]) == 7 and kv["bound"] == "min_cols", kv
            else:
                assert int(kv["nsplit"]) == (2 if name == "two" else 1) and kv["bound"] == "workspace", kv
            check_sums(torch.from_numpy(got[key + " num"]).cuda(), wn, empty, key + " num")
            check_sums(torch.from_numpy(got[key + " den"]).cuda(), wd, empty, key + " den")


@pytest.mark.parametrize("beta", BETAS)
def test_all_ones_agree_with_the_unweighted_update(eng, beta):
    """All-ones weights: mu_apply of the two sums is nnf_mu_mode_f32's update, to the kernels' tolerance."""
    from test_gpu_mu_rank128 import close
    for (L, I, K), r in (((5, 33, 71), 20), ((2, 260, 260), 33)):
        g = torch.Generator(device="cuda").manual_seed(5)
        Ft, V = torch.rand(r, I, device="cuda", generator=g) + 0.05, torch.rand(r, L * K, device="cuda", generator=g) + 0.05
        T = torch.rand(L, I, K, device="cuda", generator=g) + 0.05
        num, den = eng.mu_mode_w(T, torch.ones_like(T), Ft, V, beta)
        close(eng.mu_apply(Ft, num, den, None, beta).cpu().numpy(), eng.mu_mode(T, Ft, V, beta).cpu().numpy(), (L, I, K, r, beta))


@pytest.mark.parametrize("beta", [1, 0.5])
def test_two_calls_are_bitwise_equal_and_nan_is_zero_under_zero_weight(eng, beta):
    L, I, K, r = 12, 200, 400, 30
    T, Wg, Ft, V, _ = problem(L, I, K, r)
    a = [t.clone() for t in eng.mu_mode_w(T, Wg, Ft, V, beta)]
    b = eng.mu_mode_w(T, Wg, Ft, V, beta)
    c = eng.mu_mode_w(torch.where(Wg == 0, torch.zeros_like(T), T), Wg, Ft, V, beta)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_refusals(eng):
    from nn_fac_amd.engine import EngineError, _ptr
    L, I, K = 5, 33, 71
    T, Wg, Ft, V, _ = problem(L, I, K, 64)
    F65, V65 = torch.rand(65, I, device="cuda") + 0.05, torch.rand(65, L * K, device="cuda") + 0.05
    rc, num, den = abi_call(eng, T, Wg, F65, V65, 65, 1)
    assert rc == -3 and torch.isnan(num).all() and torch.isnan(den).all()
    check(eng, L, I, K, 64, 1)
    num, den = nan_like(64, I), nan_like(64, I)
    st = eng._stream()

    def call(T_=T, W_=Wg, F_=Ft, V_=V, N_=num, D_=den, ldf=I, ldv=L * K, ldn=I, ldd=I, dims=(L, I, K), beta=1.0):
        p = [None if t is None else _ptr(t) for t in (T_, W_, F_, V_, N_, D_)]
        rc = eng.lib.nnf_mu_mode_w_f32(eng.ctx, p[0], p[1], *dims, p[2], ldf, p[3], ldv, 64, beta, p[4], ldn, p[5], ldd, st)
        torch.cuda.synchronize()
        return rc
    assert call() == 0
    num.fill_(float("nan")), den.fill_(float("nan"))
    assert call(T_=None) == call(W_=None) == call(F_=None) == call(V_=None) == call(N_=None) == call(D_=None) == -1
    assert call(ldf=I - 1) == call(ldv=L * K - 1) == call(ldn=I - 1) == call(ldd=I - 1) == -1
    assert call(dims=(0, I, K)) == call(dims=(L, 0, K)) == call(dims=(L, I, 0)) == call(beta=-0.5) == call(beta=float("nan")) == -1
    assert torch.isnan(num).all() and torch.isnan(den).all()
    for bad in (lambda: eng.mu_mode_w(T, Wg, F65, V65, 1),                          # rank above 64
                lambda: eng.mu_mode_w(T[:, :, :-1], Wg[:, :, :-1], Ft, V, 1),       # not contiguous
                lambda: eng.mu_mode_w(T, Wg[:, :, :-1], Ft, V, 1),
                lambda: eng.mu_mode_w(T, Wg[:, :-1].contiguous(), Ft, V, 1),        # another shape
                lambda: eng.mu_mode_w(T, Wg.cpu(), Ft, V, 1),                       # another device
                lambda: eng.mu_mode_w(T, Wg, Ft, V, -1), lambda: eng.mu_mode_w(T, Wg, Ft, V, float("inf"))):
        with pytest.raises(EngineError):
            bad()


def test_workspace_limit(built_lib):
    """One byte short of one split's two slabs is refused with NNF_ERR_WORKSPACE and nothing is written; exactly that many bytes
    run the whole update as one split -- through the slab reduction -- against fp64."""
    from nn_fac_amd.engine import Engine
    L, I, K, r, beta = 5, 33, 71, 20, 0.5
    T, Wg, Ft, V, _ = problem(L, I, K, r)
    ws = carved_w(r, I, 1)
    short, enough = (Engine(torch.device("cuda:0"), workspace_bytes=b) for b in (ws - 1, ws))
    rc, num, den = abi_call(short, T, Wg, Ft, V, r, beta)
    assert rc == -4 and torch.isnan(num).all() and torch.isnan(den).all()
    check(enough, L, I, K, r, beta)

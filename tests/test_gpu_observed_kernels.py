"""The observed-entries kernels (nnf_csr_obs_f32, nnf_sptensor_obs_f32; nn_fac_amd/csrc/k_sparse_obs.hip) against the fp64
restatement of tests/observed_restatement.py on the fp32-rounded operands, per output entry.

Matrices: the four families of tests/test_gpu_sparse_kernels.py (67 x 130 and 513 x 40 in chunks of 16, the edge row lengths at
the library's own CH, 8 x 1024 with 16 .. 125 chunks per row in chunks of 8).  Tensors: the families of
tests/test_gpu_sptensor_kernels.py at orders 3, 4 and 5, every mode.  Ranks 1, 10, 50, 64, 65, 100, 128; beta 0, 0.5, 1, 2, 3.
Operands are views of wider NaN-filled buffers, outputs views of wider NaN-filled buffers.

Bounds (u = 2^-24; sums of nonnegative terms, so relative and per entry, built as in those two files), with
C = min(len, CH) + nchunks + 2 + (ng - 1) the chain of the product form:

    beta     num                                den
    2        C                                  C + r + 4
    1        C + r + 4                          C
    0        C + 2 r + 6                        C + r + 4
    3        C + r + 4                          C + 2 r + 6
    other    C + ceil|beta - 2| r + K + 4       C + ceil|beta - 1| r + K + 4

(p is an fp32 dot product of r terms, r u, and enters the weights to the power beta - 2 resp. beta - 1.)  K = 89 is the error of
the single-precision power sparse_obs_pow in ulps: tools/probes/obs_pow_probe.hip -- that function alone against fp64 pow, 10^6
values of p log-uniform in [1e-6, 1e3] -- sees at most 44.211 ulp at the exponent -1.5 and 11.343 at -0.5, the two these tests
use (beta = 0.5); twice the larger, rounded up (profiles/obs_pow_probe.jsonl).  The error of exp2(e log2 p) grows with
|e log2 p| (30 at p = 1e-6, e = -1.5); at the p of these tests, of order 1 .. 30, it is a few ulps.

Cost: fp64 terms on the fp32 p, so |dcost| <= sum_e |d d_beta / d p|(x_e, p_e) (r + 4) u p_e + 1e-12 sum |terms|, with
d d_beta / d p = p^(beta - 2) (p - x): (p - x) at beta = 2, 1 - x / p at beta = 1, (p - x) / p^2 at beta = 0.  At beta = 0 a stored
zero makes the cost +inf (d_0(0 | p)); the finite part is checked on a copy of the data whose zeros are replaced by 0.5."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import observed_restatement as ob
import test_gpu_sparse_kernels as mk
import test_gpu_sptensor_kernels as tk

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
RANKS = (1, 10, 50, 64, 65, 100, 128)
BETAS = (0, 0.5, 1, 2, 3)
POW_K = 89     # ulps of sparse_obs_pow: twice the largest error of tools/probes/obs_pow_probe.hip, rounded up (the head of this file)
MATRICES = ["67x130", "513x40", "edge-lengths", "long-rows"]
TENSORS = tk.ORDER3 + tk.HIGHER


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


@pytest.fixture(scope="module")
def mats(eng):
    return mk.matrices(eng)


@pytest.fixture(scope="module")
def tens(eng):
    return tk.tensors(eng)


def extra_terms(beta, r):
    """(num, den): what the table at the head of this file adds to C."""
    if beta == 2:
        return 0, r + 4
    if beta == 1:
        return r + 4, 0
    if beta == 0:
        return 2 * r + 6, r + 4
    if beta == 3:
        return r + 4, 2 * r + 6
    return math.ceil(abs(beta - 2)) * r + POW_K + 4, math.ceil(abs(beta - 1)) * r + POW_K + 4


def cost_bound(beta, x, p, r):
    dp = np.abs(p ** (beta - 2.0) * (p - x))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ob.terms(beta, x, p)
    return float(np.sum(dp * (r + 4) * U32 * p) + 1e-12 * np.sum(np.abs(t))), float(np.sum(t))


def check_cost(tag, beta, got, x, p, r, rerun):
    """`rerun(vals)`: the cost of the same call on other values (beta = 0: the data with its zeros replaced)."""
    if beta == 0 and (x == 0).any():
        assert got == math.inf, (tag, got)
        x = np.where(x == 0, 0.5, x)
        got = rerun(x)
    bound, want = cost_bound(beta, x, p, r)
    print(tag, "cost err / bound:", abs(got - want) / bound)
    assert abs(got - want) <= bound, (tag, got, want, bound)


@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("r", RANKS)
def test_csr_obs_against_fp64(eng, mats, name, r):
    X, ch = mats[name]
    A = mk.upload(eng, X, ch)
    Own, F = mk.factors(X, r, seed=200 + r)
    Cx = ob.from_csr(X)
    facs = [Own, F]
    p = ob.model_at_stored(Cx, facs)
    chain = mk.chain_terms(X, A.ch)
    empty = np.diff(X.indptr) == 0
    assert empty.any() and (X.data == 0).any()
    On, Fn = mk.padded(Own, extra=8), mk.padded(F)
    m = X.shape[0]
    for beta in BETAS:
        cost = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        on, od = tk.nan_out(r, m), tk.nan_out(r, m)
        num, den = eng.csr_obs(A, On, Fn, beta, cost_out=cost, out_num=on, out_den=od)
        torch.cuda.synchronize()
        assert num.data_ptr() == on.data_ptr() and den.data_ptr() == od.data_ptr()
        wn, wd = ob.sums(Cx, facs, 0, beta)
        en, ed = extra_terms(beta, r)
        mk.assert_rel(num.double().cpu().numpy(), wn.T, chain + en, ("csr_obs num", name, r, beta))
        mk.assert_rel(den.double().cpu().numpy(), wd.T, chain + ed, ("csr_obs den", name, r, beta))
        assert not num.cpu().numpy()[:, empty].any() and not den.cpu().numpy()[:, empty].any()

        def rerun(vals):
            Xz = X.copy()
            Xz.data = vals
            c = torch.zeros(1, dtype=torch.float64, device="cuda")
            assert eng.csr_obs(mk.upload(eng, Xz, ch), On, Fn, beta, sums=False, cost_out=c) is None
            return float(c)
        check_cost(("csr_obs", name, r, beta), beta, float(cost), Cx.vals, p, r, rerun)


def check_sptensor(eng, tens, name, r):
    X, ch = tens[name]
    S = tk.upload(eng, X, ch)
    F = tk.factors(X, r, seed=300 + r)
    ng = len(X.shape) - 1
    p = ob.model_at_stored(X, F)
    for mode in range(len(X.shape)):
        chain = tk.chain_terms(X, mode, S.ch)
        empty = X.slice_lengths(mode) == 0
        On, G = tk.padded(F[mode], extra=8), tk.gathered(F, mode)
        for beta in BETAS:
            cost = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
            num, den = eng.sptensor_obs(S, mode, On, G, beta, cost_out=cost, out_num=tk.nan_out(r, X.shape[mode]),
                                        out_den=tk.nan_out(r, X.shape[mode]))
            torch.cuda.synchronize()
            wn, wd = ob.sums(X, F, mode, beta)
            en, ed = extra_terms(beta, r)
            tk.assert_rel(num.double().cpu().numpy(), wn.T, chain + en, ("sptensor_obs num", name, r, mode, beta))
            tk.assert_rel(den.double().cpu().numpy(), wd.T, chain + ed, ("sptensor_obs den", name, r, mode, beta))
            assert not num.cpu().numpy()[:, empty].any() and not den.cpu().numpy()[:, empty].any()

            def rerun(vals):
                c = torch.zeros(1, dtype=torch.float64, device="cuda")
                assert eng.sptensor_obs(tk.upload(eng, X, ch, vals=vals), mode, On, G, beta, sums=False, cost_out=c) is None
                return float(c)
            check_cost(("sptensor_obs", name, r, mode, beta), beta, float(cost), X.vals, p, r, rerun)
    assert (X.slice_lengths(0) == 0).any() and (X.vals == 0).any() and ng in (2, 3, 4)


@pytest.mark.parametrize("name", TENSORS)
@pytest.mark.parametrize("r", RANKS)
def test_sptensor_obs_against_fp64(eng, tens, name, r):
    check_sptensor(eng, tens, name, r)


def forms(call):
    """(num, den, cost) of the three forms of a call and of a second run of the first."""
    out = []
    for sums, want_cost in ((True, True), (True, True), (True, False), (False, True)):
        c = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda") if want_cost else None
        res = call(sums, c)
        torch.cuda.synchronize()
        assert (res is None) == (not sums)
        out.append((None if res is None else res[0].clone(), None if res is None else res[1].clone(), None if c is None else float(c)))
    return out


def same_bits(a, b):      # (NaN included: bit for bit)
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("r", (10, 100))
def test_two_runs_and_the_three_forms_are_bitwise_equal(eng, mats, tens, r):
    for beta in BETAS:
        for name, (X, ch) in mats.items():
            A = mk.upload(eng, X, ch)
            Own, F = mk.factors(X, r, seed=7)
            On, Fn = mk.padded(Own), mk.padded(F)
            both, again, only_sums, only_cost = forms(lambda sums, c: eng.csr_obs(A, On, Fn, beta, sums=sums, cost_out=c))
            assert same_bits(both[0], again[0]) and same_bits(both[1], again[1]) and both[2] == again[2], (name, beta)
            assert same_bits(both[0], only_sums[0]) and same_bits(both[1], only_sums[1]) and both[2] == only_cost[2], (name, beta)
            assert np.isfinite(both[2]) or beta == 0, (name, beta)
        for name in ("67x130x9", "12x9x10x8", "7x6x5x4x3"):
            X, ch = tens[name]
            S = tk.upload(eng, X, ch)
            F = tk.factors(X, r, seed=7)
            for mode in (0, len(X.shape) - 1):
                On, G = tk.padded(F[mode]), tk.gathered(F, mode)
                both, again, only_sums, only_cost = forms(
                    lambda sums, c: eng.sptensor_obs(S, mode, On, G, beta, sums=sums, cost_out=c))
                assert same_bits(both[0], again[0]) and same_bits(both[1], again[1]) and both[2] == again[2], (name, mode, beta)
                assert same_bits(both[0], only_sums[0]) and same_bits(both[1], only_sums[1]) and both[2] == only_cost[2], (name, mode, beta)


@pytest.mark.parametrize("r", (10, 100))
def test_a_nan_value_reaches_exactly_the_outputs_of_its_row(eng, mats, tens, r):
    for beta in BETAS:
        for name, (X, ch) in mats.items():
            lens = np.diff(X.indptr)
            row = int(np.argmax(lens))                      # the longest row: split into chunks; the NaN sits in its last one
            Xn = X.copy()
            Xn.data[X.indptr[row + 1] - 1] = np.nan
            Own, F = mk.factors(X, r, seed=9)
            cost = torch.zeros(1, dtype=torch.float64, device="cuda")
            num, den = eng.csr_obs(mk.upload(eng, Xn, ch), mk.padded(Own), mk.padded(F), beta, cost_out=cost)
            bad = np.isnan(num.cpu().numpy())
            assert bad[:, row].all() and not np.delete(bad, row, axis=1).any(), (name, beta)
            assert not np.isnan(den.cpu().numpy()).any(), (name, beta)      # (the denominator does not read the value)
            assert np.isnan(float(cost)), (name, beta)
        # a NaN in the own factor's row reaches num and den of that row, and only them; one in the gathered factor the rows that
        # store its column
        X, ch = mats["67x130"]
        A = mk.upload(eng, X, ch)
        Own, F = mk.factors(X, r, seed=9)
        Ob = Own.copy()
        Ob[20, 0] = np.nan
        num, den = (np.isnan(t.cpu().numpy()) for t in eng.csr_obs(A, mk.padded(Ob), mk.padded(F), beta))
        # (the weights that do not read the model: x itself in the numerator at beta = 2, 1 in the denominator at beta = 1)
        for got, free in ((num, 2), (den, 1)):
            assert not got.any() if beta == free else got[:, 20].all() and not np.delete(got, 20, axis=1).any(), beta
        Fb = F.copy()
        Fb[17, 0] = np.nan
        rows, cols, _ = mk.rs.triples(X)
        touched = np.isin(np.arange(X.shape[0]), rows[cols == 17])
        bad = np.isnan(eng.csr_obs(A, mk.padded(Own), mk.padded(Fb), beta)[1].cpu().numpy())
        assert touched.any() and (bad[0] == touched).all(), beta
        assert not bad[1:].any() if beta == 1 else (bad[1:] == touched[None, :]).all(), beta
        # tensors: a NaN value in the last entry of the longest slice of mode 0
        X, ch = tens["long-slices"]
        slice_ = int(np.argmax(X.slice_lengths(0)))
        vals = X.vals.copy()
        vals[np.nonzero(X.coords[:, 0] == slice_)[0][-1]] = np.nan
        F = tk.factors(X, r, seed=9)
        cost = torch.zeros(1, dtype=torch.float64, device="cuda")
        num, den = eng.sptensor_obs(tk.upload(eng, X, ch, vals=vals), 0, tk.padded(F[0]), tk.gathered(F, 0), beta, cost_out=cost)
        bad = np.isnan(num.cpu().numpy())
        assert bad[:, slice_].all() and not np.delete(bad, slice_, axis=1).any() and np.isnan(float(cost)), beta
        assert not np.isnan(den.cpu().numpy()).any(), beta


def test_a_stored_zero_is_an_observed_zero(eng):
    """One row, three entries, the middle one a stored 0: nothing to num, its term to den, d_beta(0 | p) to the cost."""
    import scipy.sparse as sp
    X = sp.csr_matrix((np.array([0.5, 0.0, 2.0]), np.array([0, 2, 3], dtype=np.int32), np.array([0, 3, 3])), shape=(2, 5))
    A = mk.upload(eng, X)
    Own, F = mk.factors(X, 3, seed=1)
    p = Own[0] @ F[[0, 2, 3]].T
    for beta in BETAS:
        cost = torch.zeros(1, dtype=torch.float64, device="cuda")
        num, den = eng.csr_obs(A, mk.padded(Own), mk.padded(F), beta, cost_out=cost)
        wn = 0.5 * p[0] ** (beta - 2) * F[0] + 2.0 * p[2] ** (beta - 2) * F[3]
        wd = sum(p[i] ** (beta - 1) * F[j] for i, j in enumerate((0, 2, 3)))
        assert np.allclose(num.cpu().numpy()[:, 0], wn, rtol=1e-5) and np.allclose(den.cpu().numpy()[:, 0], wd, rtol=1e-5), beta
        assert not num.cpu().numpy()[:, 1].any() and not den.cpu().numpy()[:, 1].any()
        zero_term = {0: math.inf, 1: p[1]}.get(beta, p[1] ** beta / beta if beta else math.inf)
        want = sum(float(ob.terms(beta, np.array([x]), np.array([q]))[0]) for x, q in ((0.5, p[0]), (2.0, p[2]))) + zero_term
        assert float(cost) == want == math.inf if beta == 0 else abs(float(cost) - want) <= 1e-5 * abs(want), (beta, float(cost), want)


# ---- refusals: one operand spoilt at a time, nothing launched (tests/test_gpu_sparse_kernels.py) --------------------------------------
def test_operands_are_refused_before_anything_is_launched(eng, mats, tens):
    refused = mk.refused
    X, ch = mats["67x130"]
    m, n = X.shape
    r = 10
    A = mk.upload(eng, X, ch)
    Own, F = mk.factors(X, r, seed=1)
    On, Fn = mk.padded(Own), mk.padded(F)
    assert len(eng.csr_obs(A, On, Fn, 0.5)) == 2          # the valid call is accepted
    odd = torch.rand(n, r + 1, device="cuda")[:, :r]
    off = torch.rand(n * 12 + 1, device="cuda")[1:].view(n, 12)[:, :r]
    for bad in (Fn.double(), Fn.cpu(), mk.padded(F[:-1]), mk.padded(np.vstack([F, F[:1]])), odd, off,
                torch.rand(n, 2 * r, device="cuda")[:, ::2], mk.padded(mk.f32(np.ones((n, 129))))):
        refused(eng, lambda: eng.csr_obs(A, On, bad, 1))
    for bad in (On.double(), On.cpu(), mk.padded(Own[:-1]), mk.padded(Own[:, :-1]), torch.rand(m, r + 1, device="cuda")[:, :r]):
        refused(eng, lambda: eng.csr_obs(A, bad, Fn, 1))
    for bad in (torch.empty(r, m + 1, device="cuda"), torch.empty(r + 1, m, device="cuda"), torch.empty(r, m, device="cuda").double(),
                torch.empty(r, m), torch.empty(r, 2 * m, device="cuda")[:, ::2]):
        refused(eng, lambda: eng.csr_obs(A, On, Fn, 1, out_num=bad))
        refused(eng, lambda: eng.csr_obs(A, On, Fn, 1, out_den=bad))
    for bad in (torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.float64), torch.zeros(0, dtype=torch.float64, device="cuda")):
        refused(eng, lambda: eng.csr_obs(A, On, Fn, 1, cost_out=bad))
    for bad in (-1, -1e-9, float("nan"), float("inf"), None, "kl"):
        refused(eng, lambda: eng.csr_obs(A, On, Fn, bad))
    refused(eng, lambda: eng.csr_obs(A, On, Fn, 1, sums=False))               # nothing asked for
    refused(eng, lambda: eng.csr_obs((A.rowptr, A.colidx, A.vals), On, Fn, 1))   # not a checked matrix
    # the tensor entry
    T, tch = tens["67x130x9"]
    S = tk.upload(eng, T, tch)
    Ft = tk.factors(T, r, seed=1)
    Ot, G = tk.padded(Ft[0]), tk.gathered(Ft, 0)
    assert len(eng.sptensor_obs(S, 0, Ot, G, 0.5)) == 2
    e0 = T.shape[0]
    for bad in ([G[0]], [G[1], G[0]], [G[0], G[1].cpu()], [G[0], G[1].double()], [G[0], tk.padded(Ft[2][:, :-1])],
                [G[0], tk.padded(Ft[2], extra=8)], [G[0], None]):
        refused(eng, lambda: eng.sptensor_obs(S, 0, Ot, bad, 1))
    for bad in (Ot.double(), Ot.cpu(), tk.padded(Ft[0][:-1]), tk.padded(Ft[0][:, :-1]), None):
        refused(eng, lambda: eng.sptensor_obs(S, 0, bad, G, 1))
    for mode in (3, -1, 1.0):
        refused(eng, lambda: eng.sptensor_obs(S, mode, Ot, G, 1))
    for bad in (torch.empty(r, e0 + 1, device="cuda"), torch.empty(r, e0, device="cuda").double(), torch.empty(r, e0)):
        refused(eng, lambda: eng.sptensor_obs(S, 0, Ot, G, 1, out_num=bad))
        refused(eng, lambda: eng.sptensor_obs(S, 0, Ot, G, 1, out_den=bad))
    for bad in (-1, float("nan"), float("inf")):
        refused(eng, lambda: eng.sptensor_obs(S, 0, Ot, G, bad))
    refused(eng, lambda: eng.sptensor_obs(S, 0, Ot, G, 1, sums=False))
    refused(eng, lambda: eng.sptensor_obs(S, 0, Ot, G, 1, cost_out=torch.zeros(1, device="cuda")))
    refused(eng, lambda: eng.sptensor_obs(A, 0, Ot, G, 1))


def test_the_library_refuses_what_the_engine_would(eng, mats, tens):
    """The C entries' own argument checks: status codes, nothing written."""
    X, ch = mats["67x130"]
    A = mk.upload(eng, X, ch)
    r = 10
    Own, F = mk.factors(X, r, seed=1)
    On, Fn = mk.padded(Own), mk.padded(F)
    num = torch.full((r, X.shape[0]), -1.0, device="cuda")
    den = torch.full((r, X.shape[0]), -1.0, device="cuda")
    cost = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    st = eng._stream()
    ptrs = ("rowptr", "colidx", "vals", "rowchunk", "chunk_row", "Own", "Fn", "num", "den", "cost")

    def obs(**kw):
        a = dict(rowptr=A.rowptr.data_ptr(), colidx=A.colidx.data_ptr(), vals=A.vals.data_ptr(), nrows=A.nrows, ncols=A.ncols, nnz=A.nnz,
                 rowchunk=A.rowchunk.data_ptr(), chunk_row=A.chunk_row.data_ptr(), nchunks=A.nchunks, ch=A.ch, Own=On.data_ptr(),
                 ldo=On.stride(0), Fn=Fn.data_ptr(), ldn=Fn.stride(0), r=r, beta=1.0, num=num.data_ptr(), ldnum=num.stride(0),
                 den=den.data_ptr(), ldden=den.stride(0), cost=cost.data_ptr())
        a.update(kw)
        return eng.lib.nnf_csr_obs_f32(eng.ctx, *[C.c_void_p(v) if k in ptrs else v for k, v in a.items()], st)
    assert obs() == 0
    torch.cuda.synchronize()
    good = (num.clone(), den.clone(), cost.clone())
    for t in (num, den, cost):
        t.fill_(-1.0)
    assert obs(r=129, ldn=132, ldo=132) == -3
    assert [obs(beta=-1.0), obs(beta=float("nan")), obs(beta=float("inf")), obs(num=None), obs(den=None), obs(num=None, den=None, cost=None),
            obs(ldnum=A.nrows - 1), obs(ldden=A.nrows - 1), obs(ldn=r), obs(ldn=r + 1), obs(Fn=Fn.data_ptr() + 4), obs(Own=None),
            obs(ldo=r), obs(Own=On.data_ptr() + 4), obs(rowptr=None), obs(ch=0), obs(nchunks=A.nnz + 1), obs(nrows=0), obs(r=0)] == [-1] * 19
    torch.cuda.synchronize()
    assert all(bool((t == -1.0).all()) for t in (num, den, cost))
    assert obs() == 0 and obs(num=None, den=None) == 0 and obs(cost=None) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((num, den, cost), good))
    # the tensor entry: ng outside 2 .. 4, one of num / den alone, a bad beta
    T, tch = tens["67x130x9"]
    S = tk.upload(eng, T, tch)
    M = S.modes[0]
    Ft = tk.factors(T, r, seed=1)
    Ot, G = tk.padded(Ft[0]), tk.gathered(Ft, 0)
    tn = torch.full((r, M.extent), -1.0, device="cuda")
    td = torch.full((r, M.extent), -1.0, device="cuda")
    gp = (C.c_void_p * 2)(*[g.data_ptr() for g in G])
    ex = (C.c_int64 * 2)(*M.extents)

    def tobs(ng=2, beta=1.0, num=tn.data_ptr(), den=td.data_ptr(), cost=None):
        return eng.lib.nnf_sptensor_obs_f32(eng.ctx, *M.args(), ng, gp, ex, G[0].stride(0), C.c_void_p(Ot.data_ptr()), Ot.stride(0), r, beta,
                                            C.c_void_p(num), tn.stride(0), C.c_void_p(den), td.stride(0), C.c_void_p(cost), st)
    assert [tobs(ng=1), tobs(ng=5), tobs(beta=-0.5), tobs(num=None), tobs(den=None), tobs(num=None, den=None)] == [-1] * 6
    torch.cuda.synchronize()
    assert bool((tn == -1.0).all()) and bool((td == -1.0).all())
    assert tobs() == 0
    torch.cuda.synchronize()
    assert bool((tn >= 0).all()) and bool((td >= 0).all())

"""The CSR kernels (nnf_csr_xf_f32, nnf_csr_kl_f32; nn_fac_amd/csrc/k_sparse.hip) against the fp64 restatement of
tests/sparse_restatement.py, on the fp32-rounded operands.

Matrices: 67 x 130 and 513 x 40 (ragged on both sides of every tile: 64-row tiles of the second kernel, 4 chunks per workgroup),
about 30 % stored, one empty row, one empty column, explicit stored zeros, cut into chunks of 16 so that most rows are split;
7 x 200 with the row lengths 0, 1, CH - 1, CH, CH + 1, 3 CH + 5, 0 at the library's own CH for a matrix of that size; and
8 x 1024 with rows of up to 1000 entries in chunks of 8 -- 16, 17, 18, 38 and 125 chunks per row, on both sides of the count above
which the second kernel sums a row with the whole workgroup.
Node-major operands are views of wider buffers (pitch > r) whose padding holds NaN: a kernel that lets it through shows it.

Bounds (u = 2^-24; the inputs are nonnegative, so every sum is a sum of nonnegative terms and the bounds are relative, per
output entry).  csr_xf: a lane adds at most min(len, CH) FMAs in a chain (one rounding each), the tree over the groups and the
rounding of the fp64 sum of the nchunks partials add one each -- (min(len, CH) + nchunks + 2) u, the issue's figure.  csr_kl: the
same chain on q f with q = x / p: p is an fp32 dot product of r terms (<= r u), the division one more -- + r + 4.  The cost is
accumulated in fp64 on the fp32 p: d(x log(x / p)) = -x dp / p, so |dcost| <= (r + 4) u sum(x) (+ 1e-12 of the terms' absolute
sum for the fp64 part)."""
import numpy as np
import pytest
import torch

import sparse_restatement as rs

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
RANKS = (1, 10, 50, 64, 65, 100, 128)


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def matrices(eng):
    """name -> (scipy CSR with fp32-representable values, chunk size)."""
    out = {}
    for name, (m, n) in (("67x130", (67, 130)), ("513x40", (513, 40))):
        X = rs.sample(m, n, 0.3, seed=m, empty_row=5, empty_col=3, stored_zeros=9)
        X.data = f32(X.data)
        out[name] = (X, 16)
    ch = eng.csr_chunk_entries(7 * 64)
    assert ch == 64
    X = rs.from_row_lengths([0, 1, ch - 1, ch, ch + 1, 3 * ch + 5, 0], 3 * ch + 8, seed=3, stored_zeros=4)
    X.data = f32(X.data)
    out["edge-lengths"] = (X, None)
    # rows of 16 chunks (the last a thread of the second kernel sums alone), 17, 18, 38 and 125 chunks (summed by the whole
    # workgroup in 8 .. 256 segments, ragged ones included), in chunks of 8
    X = rs.from_row_lengths([139, 0, 1, 300, 128, 129, 1000, 7], 1024, seed=4, stored_zeros=6)
    X.data = f32(X.data)
    out["long-rows"] = (X, 8)
    return out


@pytest.fixture(scope="module")
def mats(eng):
    return matrices(eng)


def upload(eng, X, ch=None):
    return eng.csr_matrix(torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices.astype(np.int32)).cuda(),
                          torch.from_numpy(X.data.astype(np.float32)).cuda(), X.shape, ch=ch)


def padded(a, extra=4):
    """nodes x r as a view of a buffer with `extra` more columns (pitch a multiple of 4, > r) full of NaN."""
    nodes, r = a.shape
    buf = torch.full((nodes, (r + 3) // 4 * 4 + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :r] = torch.from_numpy(a.astype(np.float32)).cuda()
    return buf[:, :r]


def factors(X, r, seed):
    rng = np.random.default_rng(seed)
    return f32(rng.random((X.shape[0], r)) + 0.05), f32(rng.random((X.shape[1], r)) + 0.05)


def chain_terms(X, ch):
    """Per row: min(len, CH) + nchunks + 2."""
    lens = np.diff(X.indptr)
    return np.minimum(lens, ch) + -(-lens // ch) + 2


def assert_rel(got, want, terms, tag):
    """|got - want| <= terms u want, entry by entry (r x nrows; terms per row); rows without entries are exactly 0."""
    bound = terms[None, :] * U32 * np.abs(want)
    err = np.abs(got - want)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(tag, "max err / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound), (tag, worst, got[worst], want[worst], bound[worst])


@pytest.mark.parametrize("name", ["67x130", "513x40", "edge-lengths", "long-rows"])
@pytest.mark.parametrize("r", RANKS)
def test_csr_xf_against_fp64(eng, mats, name, r):
    X, ch = mats[name]
    A = upload(eng, X, ch)
    _, F = factors(X, r, seed=r)
    out = torch.full((r, X.shape[0] + 3), float("nan"), device="cuda")[:, :X.shape[0]]
    got = eng.csr_xf(A, padded(F), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    want = rs.cross_vxt(X, F.T)
    assert_rel(got.double().cpu().numpy(), want, chain_terms(X, A.ch), ("csr_xf", name, r))
    empty = np.diff(X.indptr) == 0
    assert empty.any() and not got.cpu().numpy()[:, empty].any()


@pytest.mark.parametrize("name", ["67x130", "513x40", "edge-lengths", "long-rows"])
@pytest.mark.parametrize("r", RANKS)
def test_csr_kl_against_fp64(eng, mats, name, r):
    X, ch = mats[name]
    A = upload(eng, X, ch)
    Own, F = factors(X, r, seed=100 + r)
    cost = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    num = eng.csr_kl(A, padded(Own), padded(F, extra=8), cost_out=cost)
    torch.cuda.synchronize()
    want = rs.kl_num_u(X, Own, F.T)
    assert_rel(num.double().cpu().numpy(), want, chain_terms(X, A.ch) + r + 4, ("csr_kl num", name, r))
    _, _, vals = rs.triples(X)
    p = rs.model_at_stored(X, Own, F.T)
    nz = vals != 0
    terms = vals[nz] * np.log(vals[nz] / p[nz]) - vals[nz]
    bound = (r + 4) * U32 * vals.sum() + 1e-12 * np.abs(terms).sum()
    print("csr_kl cost", name, r, "err / bound:", abs(float(cost[0]) - terms.sum()) / bound)
    assert abs(float(cost[0]) - terms.sum()) <= bound, (name, r, float(cost[0]), terms.sum(), bound)


@pytest.mark.parametrize("r", (10, 100))
def test_two_runs_and_the_three_forms_of_csr_kl_are_bitwise_equal(eng, mats, r):
    for name, (X, ch) in mats.items():
        A = upload(eng, X, ch)
        Own, F = factors(X, r, seed=7)
        On, Fn = padded(Own), padded(F)
        a, b = eng.csr_xf(A, Fn).clone(), eng.csr_xf(A, Fn).clone()
        assert torch.equal(a, b), name
        c1, c2, c3 = (torch.zeros(1, dtype=torch.float64, device="cuda") for _ in range(3))
        both = eng.csr_kl(A, On, Fn, cost_out=c1).clone()
        again = eng.csr_kl(A, On, Fn, cost_out=c2).clone()
        only_num = eng.csr_kl(A, On, Fn).clone()
        assert eng.csr_kl(A, On, Fn, num=False, cost_out=c3) is None
        torch.cuda.synchronize()
        assert torch.equal(both, again) and torch.equal(both, only_num), name
        assert float(c1) == float(c2) == float(c3) and np.isfinite(float(c1)), name


def test_a_nan_value_reaches_exactly_the_outputs_of_its_row(eng, mats):
    r = 10
    for name, (X, ch) in mats.items():
        lens = np.diff(X.indptr)
        row = int(np.argmax(lens))                      # the longest row: split into chunks; the NaN sits in its last one
        Xn = X.copy()
        Xn.data[X.indptr[row + 1] - 1] = np.nan
        A = upload(eng, Xn, ch)
        Own, F = factors(X, r, seed=9)
        xf = eng.csr_xf(A, padded(F)).cpu().numpy()
        cost = torch.zeros(1, dtype=torch.float64, device="cuda")
        kl = eng.csr_kl(A, padded(Own), padded(F), cost_out=cost).cpu().numpy()
        for got in (xf, kl):
            bad = np.isnan(got)
            assert bad[:, row].all() and not np.delete(bad, row, axis=1).any(), name
        assert np.isnan(float(cost)), name
    # and a NaN in the gathered factor reaches the rows that store its column, and only them
    X, ch = mats["67x130"]
    Own, F = factors(X, r, seed=9)
    F[17, 2] = np.nan
    got = np.isnan(eng.csr_xf(upload(eng, X, ch), padded(F)).cpu().numpy())
    rows, cols, _ = rs.triples(X)
    touched = np.isin(np.arange(X.shape[0]), rows[cols == 17])        # (a stored zero in that column too: 0 * NaN)
    assert touched.any() and (got[2] == touched).all() and not np.delete(got, 2, axis=0).any()


def test_the_device_transpose_of_a_torch_csr_is_scipys(mats):
    """_convert.to_dev_csr: the CSR of X^T by a stable sort on the device (torch input) against X.T.tocsr() on the host."""
    from nn_fac_amd._convert import to_dev_csr, is_sparse
    for name, (X, _) in mats.items():
        T = torch.sparse_csr_tensor(torch.from_numpy(X.indptr.astype(np.int64)), torch.from_numpy(X.indices.astype(np.int64)),
                                    torch.from_numpy(X.data.astype(np.float32)), size=X.shape)
        assert is_sparse(T) and is_sparse(X) and is_sparse(X.tocoo()) and not is_sparse(X.toarray()) and not is_sparse(T.to_dense())
        for src in (T, T.cuda()):
            for transpose in (False, True):
                a = to_dev_csr(src, torch.device("cuda:0"), transpose=transpose)
                b = to_dev_csr(X, torch.device("cuda:0"), transpose=transpose)
                assert a[3] == b[3] and all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a[:3], b[:3])), (name, transpose)
        want = X.T.tocsr()
        want.sort_indices()
        assert np.array_equal(b[0].cpu().numpy(), want.indptr) and np.array_equal(b[1].cpu().numpy(), want.indices)


# ---- refusals: one operand spoilt at a time, nothing launched (as tests/test_gpu_engine_args.py does for Engine's own methods) ---
class RefusingLib:
    """Stands in for eng.lib while a refusal is expected: a compute entry that is reached is recorded and not run."""

    def __init__(self, lib):
        self._lib, self.reached = lib, []

    def __getattr__(self, name):
        if not name.startswith("nnf_") or name in ("nnf_status_string", "nnf_csr_chunk_entries"):
            return getattr(self._lib, name)

        def refused(*args):
            self.reached.append(name)
            return 0
        return refused


def refused(eng, call, exc=None):
    from nn_fac_amd.engine import EngineError
    real = eng.lib
    eng.lib = proxy = RefusingLib(real)
    try:
        with pytest.raises(exc or EngineError):
            call()
        assert not proxy.reached, proxy.reached
    finally:
        eng.lib = real


def test_operands_are_refused_before_anything_is_launched(eng, mats):
    X, ch = mats["67x130"]
    m, n = X.shape
    r = 10
    A = upload(eng, X, ch)
    Own, F = factors(X, r, seed=1)
    On, Fn = padded(Own), padded(F)
    eng.csr_xf(A, Fn), eng.csr_kl(A, On, Fn)          # the valid calls are accepted
    c64 = torch.zeros(1, dtype=torch.float64, device="cuda")
    odd = torch.rand(n, r + 1, device="cuda")[:, :r]                     # pitch 11: not a multiple of 4 floats
    off = torch.rand(n * 12 + 1, device="cuda")[1:].view(n, 12)[:, :r]   # base 4 bytes off a 16-byte boundary
    spoilt_F = [Fn.double(), Fn.cpu(), padded(F[:-1]), padded(np.vstack([F, F[:1]])), odd, off,
                torch.rand(n, 2 * r, device="cuda")[:, ::2], padded(f32(np.ones((n, 129))))]
    for bad in spoilt_F:
        refused(eng, lambda: eng.csr_xf(A, bad))
        refused(eng, lambda: eng.csr_kl(A, On, bad))
    for bad in (On.double(), On.cpu(), padded(Own[:-1]), padded(Own[:, :-1]), torch.rand(m, r + 1, device="cuda")[:, :r]):
        refused(eng, lambda: eng.csr_kl(A, bad, Fn))
    for bad in (torch.empty(r, m + 1, device="cuda"), torch.empty(r + 1, m, device="cuda"), torch.empty(r, m, device="cuda").double(),
                torch.empty(r, m), torch.empty(r, 2 * m, device="cuda")[:, ::2]):
        refused(eng, lambda: eng.csr_xf(A, Fn, out=bad))
        refused(eng, lambda: eng.csr_kl(A, On, Fn, out=bad))
    for bad in (torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.float64), torch.zeros(0, dtype=torch.float64, device="cuda")):
        refused(eng, lambda: eng.csr_kl(A, On, Fn, cost_out=bad))
    refused(eng, lambda: eng.csr_kl(A, On, Fn, num=False))               # nothing asked for
    refused(eng, lambda: eng.csr_xf((A.rowptr, A.colidx, A.vals), Fn))   # not a checked matrix
    assert float(c64) == 0.0
    # the CSR triple, at construction
    rp, ci, va = A.rowptr, A.colidx, A.vals
    shifted = rp.clone()
    shifted[0] = 1
    beyond = ci.clone()
    beyond[3] = n
    falling = rp.clone()
    falling[5] = falling[4] - 1
    for args in ((rp.int(), ci, va), (rp, ci.long(), va), (rp, ci, va.double()), (rp.cpu(), ci, va), (rp, ci.cpu(), va), (rp, ci, va.cpu()),
                 (rp[:-1], ci, va), (rp, ci[:-1], va), (rp, ci, va[:-1]), (shifted, ci, va), (falling, ci, va), (rp, beyond, va),
                 (rp, ci, torch.rand(2 * va.numel(), device="cuda")[::2])):
        refused(eng, lambda: eng.csr_matrix(*args, (m, n)))
    refused(eng, lambda: eng.csr_matrix(rp, ci, va, (m, n), ch=0))
    refused(eng, lambda: eng.csr_matrix(rp, ci, va, (m + 1, n)))


def test_the_library_refuses_what_the_engine_would(eng, mats):
    """The C entries' own argument checks (a C-ABI consumer has no engine in front of them): status codes, nothing written."""
    import ctypes as C
    X, ch = mats["67x130"]
    A = upload(eng, X, ch)
    r = 10
    _, F = factors(X, r, seed=1)
    Fn = padded(F)
    out = torch.full((r, X.shape[0]), -1.0, device="cuda")
    st = eng._stream()

    def xf(**kw):
        a = dict(rowptr=A.rowptr.data_ptr(), colidx=A.colidx.data_ptr(), vals=A.vals.data_ptr(), nrows=A.nrows, ncols=A.ncols, nnz=A.nnz,
                 rowchunk=A.rowchunk.data_ptr(), chunk_row=A.chunk_row.data_ptr(), nchunks=A.nchunks, ch=A.ch, Fn=Fn.data_ptr(),
                 ldn=Fn.stride(0), r=r, out=out.data_ptr(), ldo=out.stride(0))
        a.update(kw)
        return eng.lib.nnf_csr_xf_f32(eng.ctx, *[C.c_void_p(v) if k in ("rowptr", "colidx", "vals", "rowchunk", "chunk_row", "Fn", "out")
                                                 else v for k, v in a.items()], st)
    assert xf() == 0
    torch.cuda.synchronize()
    good = out.clone()
    out.fill_(-1.0)
    assert xf(r=129, ldn=132) == -3
    assert [xf(ldn=r), xf(ldn=r + 1), xf(Fn=Fn.data_ptr() + 4), xf(ldo=A.nrows - 1), xf(out=None), xf(rowptr=None), xf(ch=0),
            xf(nchunks=A.nnz + 1), xf(nchunks=(A.nnz - 1) // A.ch), xf(nrows=0), xf(r=0)] == [-1] * 11
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    assert xf() == 0 and torch.equal(out, good)

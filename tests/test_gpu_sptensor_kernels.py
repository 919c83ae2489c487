"""The sparse-tensor kernels (nnf_sptensor_mttkrp_f32, nnf_sptensor_kl_f32; nn_fac_amd/csrc/k_sptensor.hip) against the fp64
restatement of tests/sptensor_restatement.py, on the fp32-rounded operands, every mode of every tensor.

Tensors: 67 x 130 x 9 and 513 x 7 x 40 (ragged on both sides of every tile: 64-slice tiles of the second kernel, 4 chunks per
workgroup), about 5 % stored, one empty slice per mode, explicit stored zeros, cut into chunks of 16 so that most slices are split;
7 x 50 x 50 with the mode-0 slice lengths 0, 1, CH - 1, CH, CH + 1, 3 CH + 5, 0 at the library's own CH for a tensor of that size;
8 x 64 x 64 with slices of up to 1000 entries in chunks of 8 -- 16, 17, 18, 38 and 125 chunks per slice, on both sides of the count
above which the second kernel sums a slice with the whole workgroup; 12 x 9 x 10 x 8 and 7 x 6 x 5 x 4 x 3 for three and four
gathered factors.  Node-major operands are views of wider buffers (pitch > r) whose padding holds NaN, outputs views of wider
NaN-filled buffers: a kernel that lets the padding through, or writes beside its output, shows it.

Bounds (u = 2^-24; the inputs are nonnegative, so every sum is a sum of nonnegative terms and the bounds are relative, per output
entry).  MTTKRP: h is a product of ng fp32 factors (ng - 1 roundings), a lane adds at most min(len, CH) FMAs in a chain (one
rounding each), the tree over the groups and the rounding of the fp64 sum of the nchunks partials add one each --
(min(len, CH) + nchunks + 2 + (ng - 1)) u.  KL numerator: the same chain on q h with q = x / p: p is an fp32 dot product of r terms
of Own .* h (<= r u, and h's error once more: ng - 1), the division one more -- + r + 4 + (ng - 1).  The cost is accumulated in fp64
on the fp32 p: d(x log(x / p)) = -x dp / p, so |dcost| <= (r + 4 + ng - 1) u sum(x) (+ 1e-12 of the terms' absolute sum for the
fp64 part)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sptensor_restatement as rs

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
RANKS = (1, 10, 50, 64, 65, 100, 128)
ORDER3 = ["67x130x9", "513x7x40", "edge-lengths", "long-slices"]
HIGHER = ["12x9x10x8", "7x6x5x4x3"]


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def tensors(eng):
    """name -> (Coo with fp32-representable values, chunk size)."""
    out = {}
    for name, shape in (("67x130x9", (67, 130, 9)), ("513x7x40", (513, 7, 40))):
        X = rs.sample(shape, 0.05, seed=shape[0], empty=[(0, 5), (1, 3), (2, 2)], stored_zeros=9)
        out[name] = (X, 16)
    ch = eng.csr_chunk_entries(6 * 64 + 6)
    assert ch == 64
    out["edge-lengths"] = (rs.from_slice_lengths([0, 1, ch - 1, ch, ch + 1, 3 * ch + 5, 0], (50, 50), seed=3, stored_zeros=4), None)
    # slices of 16 chunks (the last a thread of the second kernel sums alone), 17, 18, 38 and 125 chunks (summed by the whole
    # workgroup in 8 .. 256 segments, ragged ones included), in chunks of 8
    out["long-slices"] = (rs.from_slice_lengths([139, 0, 1, 300, 128, 129, 1000, 7], (64, 64), seed=4, stored_zeros=6), 8)
    out["12x9x10x8"] = (rs.sample((12, 9, 10, 8), 0.1, seed=4, empty=[(0, 3), (1, 2), (2, 1)], stored_zeros=3), 16)
    out["7x6x5x4x3"] = (rs.sample((7, 6, 5, 4, 3), 0.1, seed=5, empty=[(0, 3), (1, 2), (2, 1)], stored_zeros=3), 16)
    for X, _ in out.values():
        X.vals = f32(X.vals)
    return out


@pytest.fixture(scope="module")
def tens(eng):
    return tensors(eng)


def upload(eng, X, ch=None, vals=None):
    return eng.sparse_tensor(torch.from_numpy(np.ascontiguousarray(X.coords.T)).cuda(),
                             torch.from_numpy((X.vals if vals is None else vals).astype(np.float32)).cuda(), X.shape, ch=ch)


def padded(a, extra=4):
    """nodes x r as a view of a buffer with `extra` more columns (pitch a multiple of 4, > r) full of NaN."""
    nodes, r = a.shape
    buf = torch.full((nodes, (r + 3) // 4 * 4 + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :r] = torch.from_numpy(a.astype(np.float32)).cuda()
    return buf[:, :r]


def factors(X, r, seed):
    rng = np.random.default_rng(seed)
    return [f32(rng.random((d, r)) + 0.05) for d in X.shape]


def gathered(F, mode, extra=4):
    return [padded(f, extra) for m, f in enumerate(F) if m != mode]


def nan_out(r, n):
    return torch.full((r, n + 3), float("nan"), device="cuda")[:, :n]


def chain_terms(X, mode, ch):
    """Per slice: min(len, CH) + nchunks + 2 + (ng - 1)."""
    lens = X.slice_lengths(mode)
    return np.minimum(lens, ch) + -(-lens // ch) + 2 + (len(X.shape) - 2)


def assert_rel(got, want, terms, tag):
    """|got - want| <= terms u want, entry by entry (r x extent; terms per slice); slices without entries are exactly 0."""
    bound = terms[None, :] * U32 * np.abs(want)
    err = np.abs(got - want)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(tag, "max err / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound), (tag, worst, got[worst], want[worst], bound[worst])


def check_mttkrp(eng, tens, name, r):
    X, ch = tens[name]
    S = upload(eng, X, ch)
    F = factors(X, r, seed=r)
    for mode in range(len(X.shape)):
        out = nan_out(r, X.shape[mode])
        got = eng.sptensor_mttkrp(S, mode, gathered(F, mode), out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        want = rs.mttkrp(X, F, mode).T
        assert_rel(got.double().cpu().numpy(), want, chain_terms(X, mode, S.ch), ("sptensor_mttkrp", name, r, mode))
        empty = X.slice_lengths(mode) == 0
        assert not got.cpu().numpy()[:, empty].any()
    assert (X.slice_lengths(0) == 0).any()


def check_kl(eng, tens, name, r):
    X, ch = tens[name]
    S = upload(eng, X, ch)
    F = factors(X, r, seed=100 + r)
    ng = len(X.shape) - 1
    p = rs.model_at_stored(X, F)
    terms = rs.kl_terms(X, F)
    bound = (r + 4 + ng - 1) * U32 * X.vals.sum() + 1e-12 * np.abs(terms).sum()
    for mode in range(len(X.shape)):
        cost = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        num = eng.sptensor_kl(S, mode, padded(F[mode], extra=8), gathered(F, mode), cost_out=cost, out=nan_out(r, X.shape[mode]))
        torch.cuda.synchronize()
        want = rs.kl_num(X, F, mode).T
        assert_rel(num.double().cpu().numpy(), want, chain_terms(X, mode, S.ch) + r + 4 + (ng - 1), ("sptensor_kl num", name, r, mode))
        print("sptensor_kl cost", name, r, mode, "err / bound:", abs(float(cost[0]) - terms.sum()) / bound)
        assert abs(float(cost[0]) - terms.sum()) <= bound, (name, r, mode, float(cost[0]), terms.sum(), bound)
    assert p.min() > 0


@pytest.mark.parametrize("name", ORDER3)
@pytest.mark.parametrize("r", RANKS)
def test_mttkrp_against_fp64(eng, tens, name, r):
    check_mttkrp(eng, tens, name, r)


@pytest.mark.parametrize("name", HIGHER)
@pytest.mark.parametrize("r", (10, 100))
def test_mttkrp_of_order_4_and_5_against_fp64(eng, tens, name, r):
    check_mttkrp(eng, tens, name, r)


@pytest.mark.parametrize("name", ORDER3)
@pytest.mark.parametrize("r", RANKS)
def test_kl_against_fp64(eng, tens, name, r):
    check_kl(eng, tens, name, r)


@pytest.mark.parametrize("name", HIGHER)
@pytest.mark.parametrize("r", (10, 100))
def test_kl_of_order_4_and_5_against_fp64(eng, tens, name, r):
    check_kl(eng, tens, name, r)


def test_the_mode_copies_are_stable_sorts_of_the_canonical_list(eng, tens):
    for name, (X, ch) in tens.items():
        S = upload(eng, X, ch)
        assert S.order == len(X.shape) and S.nnz == X.nnz and len(S.modes) == S.order
        for mode, M in enumerate(S.modes):
            coords, vals = X.sorted_by(mode)
            others = [m for m in range(S.order) if m != mode]
            assert M.others == others and M.ptr.dtype == torch.int64 and M.idx.dtype == torch.int32 and M.vals.dtype == torch.float32
            assert np.array_equal(M.ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(X.slice_lengths(mode))])), (name, mode)
            assert np.array_equal(M.idx.cpu().numpy(), coords[:, others].T) and np.array_equal(M.vals.cpu().numpy(), vals.astype(np.float32))
            assert M.nchunks == int((-(-X.slice_lengths(mode) // S.ch)).sum())


@pytest.mark.parametrize("r", (10, 100))
def test_two_runs_and_the_three_forms_of_kl_are_bitwise_equal(eng, tens, r):
    for name, (X, ch) in tens.items():
        S = upload(eng, X, ch)
        F = factors(X, r, seed=7)
        for mode in range(len(X.shape)):
            On, Fn = padded(F[mode]), gathered(F, mode)
            a, b = eng.sptensor_mttkrp(S, mode, Fn).clone(), eng.sptensor_mttkrp(S, mode, Fn).clone()
            assert torch.equal(a, b), (name, mode)
            c1, c2, c3 = (torch.zeros(1, dtype=torch.float64, device="cuda") for _ in range(3))
            both = eng.sptensor_kl(S, mode, On, Fn, cost_out=c1).clone()
            again = eng.sptensor_kl(S, mode, On, Fn, cost_out=c2).clone()
            only_num = eng.sptensor_kl(S, mode, On, Fn).clone()
            assert eng.sptensor_kl(S, mode, On, Fn, num=False, cost_out=c3) is None
            torch.cuda.synchronize()
            assert torch.equal(both, again) and torch.equal(both, only_num), (name, mode)
            assert float(c1) == float(c2) == float(c3) and np.isfinite(float(c1)), (name, mode)


def test_a_nan_value_reaches_exactly_the_outputs_of_its_slices(eng, tens):
    r = 10
    for name, (X, ch) in tens.items():
        row = int(np.argmax(X.slice_lengths(0)))             # the longest slice of mode 0: split into chunks; the NaN is its last entry
        e = int(np.nonzero(X.coords[:, 0] == row)[0][-1])
        vals = X.vals.copy()
        vals[e] = np.nan
        S = upload(eng, X, ch, vals=vals)
        F = factors(X, r, seed=9)
        for mode in range(len(X.shape)):
            hit = int(X.coords[e, mode])
            got = eng.sptensor_mttkrp(S, mode, gathered(F, mode)).cpu().numpy()
            cost = torch.zeros(1, dtype=torch.float64, device="cuda")
            kl = eng.sptensor_kl(S, mode, padded(F[mode]), gathered(F, mode), cost_out=cost).cpu().numpy()
            for out in (got, kl):
                bad = np.isnan(out)
                assert bad[:, hit].all() and not np.delete(bad, hit, axis=1).any(), (name, mode)
            assert np.isnan(float(cost)), (name, mode)
    # and a NaN in a gathered factor reaches the slices that store its index, and only them
    X, ch = tens["67x130x9"]
    F = factors(X, r, seed=9)
    F[1][17, 2] = np.nan
    got = np.isnan(eng.sptensor_mttkrp(upload(eng, X, ch), 0, gathered(F, 0)).cpu().numpy())
    touched = np.isin(np.arange(X.shape[0]), X.coords[X.coords[:, 1] == 17][:, 0])        # (a stored zero at that index too: 0 * NaN)
    assert touched.any() and (got[2] == touched).all() and not np.delete(got, 2, axis=0).any()


# ---- refusals: one operand spoilt at a time, nothing launched (as tests/test_gpu_sparse_kernels.py does for the CSR entries) ----
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


def test_operands_are_refused_before_anything_is_launched(eng, tens):
    X, ch = tens["67x130x9"]
    I, J, K = X.shape
    r = 10
    S = upload(eng, X, ch)
    F = factors(X, r, seed=1)
    On, (Fj, Fk) = padded(F[0]), gathered(F, 0)
    eng.sptensor_mttkrp(S, 0, [Fj, Fk]), eng.sptensor_kl(S, 0, On, [Fj, Fk])          # the valid calls are accepted
    odd = torch.rand(J, r + 1, device="cuda")[:, :r]                     # pitch 11: not a multiple of 4 floats
    off = torch.rand(J * 16 + 1, device="cuda")[1:].view(J, 16)[:, :r]   # base 4 bytes off a 16-byte boundary
    spoilt = [Fj.double(), Fj.cpu(), padded(F[1][:-1]), padded(np.vstack([F[1], F[1][:1]])), odd, off,
              torch.rand(J, 2 * r, device="cuda")[:, ::2], padded(F[1][:, :-1]),          # a rank that is not the other factor's
              padded(F[1], extra=8),                                                      # a pitch that is not the other factor's
              (F[1],)]                                                                    # not a tensor
    for bad in spoilt:
        refused(eng, lambda: eng.sptensor_mttkrp(S, 0, [bad, Fk]))
        refused(eng, lambda: eng.sptensor_kl(S, 0, On, [bad, Fk]))
    big = [padded(f32(np.ones((d, 129)))) for d in X.shape]                               # rank above 128
    refused(eng, lambda: eng.sptensor_mttkrp(S, 0, big[1:]))
    refused(eng, lambda: eng.sptensor_kl(S, 0, big[0], big[1:]))
    for bad_list in ([Fj], [Fj, Fk, Fk], [Fk, Fj], []):                                   # the number and the order of the factors
        refused(eng, lambda: eng.sptensor_mttkrp(S, 0, bad_list))
    for bad_mode in (-1, 3, 1.0, None):
        refused(eng, lambda: eng.sptensor_mttkrp(S, bad_mode, [Fj, Fk]))
    for bad in (On.double(), On.cpu(), padded(F[0][:-1]), padded(F[0][:, :-1]), torch.rand(I, r + 1, device="cuda")[:, :r]):
        refused(eng, lambda: eng.sptensor_kl(S, 0, bad, [Fj, Fk]))
    for bad in (torch.empty(r, I + 1, device="cuda"), torch.empty(r + 1, I, device="cuda"), torch.empty(r, I, device="cuda").double(),
                torch.empty(r, I), torch.empty(r, 2 * I, device="cuda")[:, ::2]):
        refused(eng, lambda: eng.sptensor_mttkrp(S, 0, [Fj, Fk], out=bad))
        refused(eng, lambda: eng.sptensor_kl(S, 0, On, [Fj, Fk], out=bad))
    for bad in (torch.zeros(1, device="cuda"), torch.zeros(1, dtype=torch.float64), torch.zeros(0, dtype=torch.float64, device="cuda")):
        refused(eng, lambda: eng.sptensor_kl(S, 0, On, [Fj, Fk], cost_out=bad))
    refused(eng, lambda: eng.sptensor_kl(S, 0, On, [Fj, Fk], num=False))               # nothing asked for
    refused(eng, lambda: eng.sptensor_mttkrp(S.modes[0], 0, [Fj, Fk]))                 # not a checked tensor
    # the coordinate list, at construction
    ind = torch.from_numpy(np.ascontiguousarray(X.coords.T)).cuda()
    va = torch.from_numpy(X.vals.astype(np.float32)).cuda()
    beyond, below = ind.clone(), ind.clone()
    beyond[1, 3] = J
    below[2, 0] = -1
    for args in ((ind.int(), va, X.shape), (ind, va.double(), X.shape), (ind.cpu(), va, X.shape), (ind, va.cpu(), X.shape),
                 (ind[:, :-1], va, X.shape), (ind, va[:-1], X.shape), (ind[:2], va, X.shape), (beyond, va, X.shape),
                 (below, va, X.shape), (ind, va, (I, J)), (ind, va, (I, J, K, 1)), (ind, va, (I, J, 0)), (ind, va, (I, J - 1, K)),
                 (ind[:2], va, (I, J)),                                            # order 2
                 (torch.zeros((6, 4), dtype=torch.int64, device="cuda"), va[:4], (2,) * 6)):      # order 6
        refused(eng, lambda: eng.sparse_tensor(*args))
    refused(eng, lambda: eng.sparse_tensor(ind, va, X.shape, ch=0))


def test_the_library_refuses_what_the_engine_would(eng, tens):
    """The C entries' own argument checks (a C-ABI consumer has no engine in front of them): status codes, nothing written."""
    X, ch = tens["67x130x9"]
    S = upload(eng, X, ch)
    M = S.modes[0]
    r = 10
    F = factors(X, r, seed=1)
    On, Fn = padded(F[0]), gathered(F, 0)
    out = torch.full((r, M.extent), -1.0, device="cuda")
    cost = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    st = eng._stream()
    ptrs = ("ptr", "idx", "vals", "rowchunk", "chunk_row", "Own", "out", "cost")

    def call(kl, **kw):
        a = dict(ptr=M.ptr.data_ptr(), idx=M.idx.data_ptr(), vals=M.vals.data_ptr(), extent=M.extent, nnz=M.nnz,
                 rowchunk=M.rowchunk.data_ptr(), chunk_row=M.chunk_row.data_ptr(), nchunks=M.nchunks, ch=M.ch, ng=2,
                 Fn=[f.data_ptr() for f in Fn], extents=list(M.extents), ldn=Fn[0].stride(0))
        if kl:
            a.update(Own=On.data_ptr(), ldo_n=On.stride(0))
        a.update(r=r, out=out.data_ptr(), ldo=out.stride(0))
        if kl:
            a.update(cost=cost.data_ptr())
        a.update(kw)
        a["Fn"] = None if a["Fn"] is None else (C.c_void_p * len(a["Fn"]))(*a["Fn"])
        a["extents"] = None if a["extents"] is None else (C.c_int64 * len(a["extents"]))(*a["extents"])
        fn = eng.lib.nnf_sptensor_kl_f32 if kl else eng.lib.nnf_sptensor_mttkrp_f32
        return fn(eng.ctx, *[C.c_void_p(v) if k in ptrs else v for k, v in a.items()], st)

    for kl in (False, True):
        assert call(kl) == 0
        torch.cuda.synchronize()
        good = out.clone()
        out.fill_(-1.0)
        cost.fill_(-1.0)
        assert call(kl, r=129, ldn=132) == -3
        assert call(kl, nnz=2 ** 31) == -3 and call(kl, extent=2 ** 31, ldo=2 ** 31) == -3 and call(kl, extents=[2 ** 31, 9]) == -3
        two = [Fn[0].data_ptr(), Fn[1].data_ptr()]
        got = [call(kl, ldn=r), call(kl, ldn=r + 1), call(kl, Fn=[two[0] + 4, two[1]]), call(kl, Fn=[two[0], two[1] + 4]),
               call(kl, Fn=[two[0], None]), call(kl, Fn=None), call(kl, extents=None), call(kl, extents=[130, 0]),
               call(kl, ng=1), call(kl, ng=5), call(kl, ldo=M.extent - 1), call(kl, ptr=None), call(kl, idx=None), call(kl, vals=None),
               call(kl, rowchunk=None), call(kl, chunk_row=None), call(kl, ch=0), call(kl, nchunks=M.nnz + 1),
               call(kl, nchunks=(M.nnz - 1) // M.ch), call(kl, extent=0), call(kl, r=0)]
        assert got == [-1] * len(got), got
        if kl:
            got = [call(kl, Own=None), call(kl, Own=On.data_ptr() + 4), call(kl, ldo_n=r), call(kl, ldo_n=r + 1), call(kl, out=None, cost=None)]
            assert got == [-1] * len(got), got
        else:
            assert call(kl, out=None) == -1
        torch.cuda.synchronize()
        assert bool((out == -1.0).all()) and float(cost) == -1.0
        assert call(kl) == 0 and torch.equal(out, good)


def test_a_chunk_table_of_another_chunking_gives_an_error_or_wrong_sums_never_a_fault(eng, tens):
    """The host cannot see the device tables: the kernels hold every index they read from them (chunk -> slice, slice -> first
    chunk, ptr) against the extent, nnz and nchunks they are told.  Tables of the right LENGTHS (extent + 1 and nchunks: the two
    the kernels cannot check) but built for another chunk size, and for another tensor's slice lengths, are handed in."""
    from nn_fac_amd.engine import EngineError, csr_chunk_table
    X, ch = tens["67x130x9"]
    r = 10
    F = factors(X, r, seed=2)
    good = upload(eng, X, ch)
    want = [eng.sptensor_mttkrp(good, mode, gathered(F, mode)).clone() for mode in range(3)]
    for other_ch in (4, 64):
        S = upload(eng, X, ch)
        for mode, M in enumerate(S.modes):
            M.rowchunk, M.chunk_row = csr_chunk_table(M.ptr, other_ch)      # ... while the kernel is told `ch`
            M.nchunks = M.chunk_row.numel()
            try:
                got = eng.sptensor_mttkrp(S, mode, gathered(F, mode))
                cost = torch.zeros(1, dtype=torch.float64, device="cuda")
                eng.sptensor_kl(S, mode, padded(F[mode]), gathered(F, mode), cost_out=cost)
            except EngineError as e:      # (fewer chunks than nnz / ch: no table of ch-chunks has that few)
                assert other_ch > ch and "status -1" in str(e), e
                continue
            torch.cuda.synchronize()
            assert other_ch < ch and bool(torch.isfinite(got).all()) and np.isfinite(float(cost))
    # the table of the tensor with its mode-0 slices in reverse order: the right lengths, every chunk in a wrong place
    S = upload(eng, X, ch)
    M = S.modes[0]
    lens = (M.ptr[1:] - M.ptr[:-1]).flip(0)
    other = torch.zeros_like(M.ptr)
    torch.cumsum(lens, 0, out=other[1:])
    M.rowchunk, M.chunk_row = csr_chunk_table(other, ch)
    assert M.chunk_row.numel() == M.nchunks
    got = eng.sptensor_mttkrp(S, 0, gathered(F, 0))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, want[0])
    # and the untouched tensor still gives its sums
    for mode in range(3):
        assert torch.equal(eng.sptensor_mttkrp(good, mode, gathered(F, mode)), want[mode])

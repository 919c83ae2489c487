"""Thin tensor-level wrapper over the C ABI: torch tensors in, raw device pointers out.

PyTorch is plumbing here (device memory, streams); every arithmetic statement of the hot path runs in
libnnfac_hip.so.  Factors are kept "transposed" on the device (Ut: r x m, V: r x n), the layout hals_nnls_acc works on.
"""
import ctypes as C
import os
import threading

import torch

from . import _lib
from ._status import write_status
from .utils import errors as err
from .utils.errors import EngineError

HALS_SPARSITY, HALS_NORMALIZE, HALS_NONZERO = 1, 2, 4
ST_EPS, ST_CNT, ST_EPS0, ST_ERR, ST_WORDS = 0, 1, 2, 3, 8

_engines = {}
_lock = threading.Lock()

MAX_RANK = 128      # NNF_MAX_RANK of include/nnfac_hip.h: up to here one launch per product / cost pass and the register- or
#                     LDS-resident sweep kernels; above, matrix factorisations go on in rank chunks (see check_rank)


def check_rank(r, where):
    """The reference accepts any rank up to min(shape) (nn_fac/nmf.py:175-178; nnls.py:156-170 loops `range(r)`).  The matrix
    path (nmf, hals_nnls_acc, mu_betadivmin) and NTF (ntf, compute_ntf, one_ntf_step) follow it: above 128 the contractions,
    MTTKRPs and cost passes walk the rank in chunks of 128 and the sweeps run in the generic kernel ("Ranks
    above 128") -- callers on those paths do not call this.  The TUCKER kernels (core contractions along the middle axis, the
    projected-gradient core update) are built for ranks <= 128: said at the boundary, before anything is uploaded or launched,
    instead of an NNF_ERR_UNSUPPORTED status from deep inside an iteration."""
    r = int(r)
    if r > MAX_RANK:
        raise EngineError(f"{where}: rank {r} is above the {MAX_RANK} the Tucker kernels (core contractions, core update) of "
                          f"nn_fac_amd are built for; nmf, ntf, hals_nnls_acc and mu_betadivmin take any rank")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _ld(t):
    """Leading dimension (elements) of a 2-D tensor for the C ABI.  PyTorch leaves the stride of a size-1 dimension
    arbitrary (a 1 x m factor -- rank 1 -- can report stride(0) == 1); with a single row it is never used to address
    anything, so any value >= the row length is valid."""
    return t.stride(0) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def _chk2d(t, name):
    # (the stride of a size-1 dimension is arbitrary in PyTorch: a k x 1 tensor need not report stride(1) == 1)
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1):
        raise EngineError(f"{name}: expected a 2-D float32 device tensor with unit inner stride, got "
                          f"{tuple(t.shape)} {t.dtype} {t.device} strides {t.stride()}")
    return t


# ---- marshalling: the recurring shapes of argument ----------------------------------------------------------------------------
def _mat(t):
    """A matrix: (pointer, leading dimension)."""
    return _ptr(t), _ld(t)


def _opt(t):
    """An optional tensor: pointer or NULL."""
    return None if t is None else _ptr(t)


def _optmat(t):
    """An optional matrix: (pointer or NULL, leading dimension or 0)."""
    return (None, 0) if t is None else (_ptr(t), _ld(t))


def _optblocks(t):
    """An optional contiguous stack of blocks: (pointer or NULL, block stride or 0)."""
    return (None, 0) if t is None else (_ptr(t), t.stride(0))


def _triple(X, Ut, V):
    """The argument run of every entry that takes X (m x n), Ut (r x m), V (r x n)."""
    return _ptr(X), X.shape[0], X.shape[1], _ld(X), _ptr(Ut), _ld(Ut), _ptr(V), _ld(V), Ut.shape[0]


def _solve_args(UtM, UtU, V):
    """The argument run of the sweep entries: right-hand side, Gram, factor, r, ncols."""
    return _ptr(UtM), _ld(UtM), _ptr(UtU), _ld(UtU), _ptr(V), _ld(V), V.shape[0], V.shape[1]


def _cp3_args(T, Ft):
    """The argument run of the 3-way CP entries: T, its extents, the three transposed factors, R."""
    return (_ptr(T), *T.shape, *_mat(Ft[0]), *_mat(Ft[1]), *_mat(Ft[2]), Ft[0].shape[0])


# ---- operand checks: each rule is written once, here; every message names the method and the operand --------------------------
def _shaped(t, shape, name):
    """_chk2d and the extents."""
    if _chk2d(t, name).shape != shape:
        raise EngineError(f"{name}: shape mismatch, expected {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _xf(X, F, axis, what, fname):
    """X (m x n) and one transposed factor whose columns run along `axis` of X (Ut: 0, V: 1) -> (m, n, r)."""
    _chk2d(X, what + " X"), _chk2d(F, f"{what} {fname}")
    if F.shape[1] != X.shape[axis]:
        raise EngineError(f"{what}: shape mismatch, X is {tuple(X.shape)}, {fname} {tuple(F.shape)}")
    return X.shape[0], X.shape[1], F.shape[0]


def _xuv(X, Ut, V, what):
    """X (m x n), Ut (r x m), V (r x n) -> (m, n, r)."""
    _chk2d(X, what + " X"), _chk2d(Ut, what + " Ut"), _chk2d(V, what + " V")
    (m, n), r = X.shape, Ut.shape[0]
    if Ut.shape[1] != m or V.shape != (r, n):
        raise EngineError(f"{what}: shape mismatch, X is {m} x {n}, Ut {tuple(Ut.shape)}, V {tuple(V.shape)}")
    return m, n, r


def _solve_ops(UtM, UtU, V, what):
    """Right-hand side of V's shape and a Gram of at least r x r (it may be larger: a view is not needed) -> (r, ncols)."""
    _chk2d(UtM, what + " UtM"), _chk2d(UtU, what + " UtU"), _chk2d(V, what + " V")
    r, ncols = V.shape
    if UtM.shape != (r, ncols) or UtU.shape[0] < r or UtU.shape[1] < r:
        raise EngineError(f"{what}: shape mismatch, V is {r} x {ncols}, UtM {tuple(UtM.shape)}, UtU {tuple(UtU.shape)}")
    return r, ncols


def _gram_pair(G, Gb, name):
    """The second Gram of a Hadamard pair (or None): the entries read one leading dimension for both."""
    if Gb is not None and (_shaped(Gb, G.shape, name).device != G.device or _ld(Gb) != _ld(G)):
        raise EngineError(f"{name}: the two Grams of a Hadamard pair must share device and leading dimension")


def _t3(T, what, exc=EngineError):
    """Contiguous 3-way float32 device tensor."""
    if T.dim() != 3 or T.dtype != torch.float32 or not T.is_cuda or not T.is_contiguous():
        raise exc(f"{what} must be a contiguous 3-way float32 device tensor, got {tuple(T.shape)} {T.dtype} {T.device}")
    return T


def _f32(t, shape, what, contiguous=False):
    """float32 device tensor of `shape`, any layout unless `contiguous`."""
    if t.dtype != torch.float32 or not t.is_cuda or t.shape != shape or (contiguous and not t.is_contiguous()):
        raise EngineError(f"{what} must be a {'contiguous ' if contiguous else ''}float32 device tensor of shape {tuple(shape)}, "
                          f"got {tuple(t.shape)} {t.dtype} {t.device}")
    return t


def _core_ops(core, MtX, grams, status, what):
    """The operands of the Tucker core update: a contiguous float32 device core, an MtX of its shape, one float32 d x d Gram per
    mode of extent d (MtX and the Grams in any layout: they are copied to contiguous buffers), 6 status doubles.  Returns
    (contiguous MtX, contiguous Grams, status)."""
    if not core.is_contiguous() or core.dtype != torch.float32 or not core.is_cuda:
        raise err.ArgumentException(f"{what} updates a contiguous float32 device core in place")
    if len(grams) != core.dim() or tuple(MtX.shape) != tuple(core.shape):
        raise err.ArgumentException(f"{what} needs one Gram per core mode and an MtX of the core's shape")
    for g, d in zip(grams, core.shape):
        if tuple(g.shape) != (d, d) or g.dtype != torch.float32 or g.device != core.device:
            raise err.ArgumentException(f"{what}: the Gram of a mode of extent d is a float32 d x d matrix on the core's device")
    if MtX.dtype != torch.float32 or MtX.device != core.device:
        raise err.ArgumentException(f"{what}: MtX must be float32 on the core's device")
    return MtX.contiguous(), [g.contiguous() for g in grams], _out64(status, 6, core.device, what + " status")


def _cp3(T, Ft, what):
    """T (I x J x K) and its three transposed factors (R x I, R x J, R x K) -> R."""
    _t3(T, what + ": T")
    R = _chk2d(Ft[0], what + " factor 0").shape[0]
    for i in range(3):
        _shaped(Ft[i], (R, T.shape[i]), f"{what} factor {i}")
    return R


def _f64(t, count, dev, what, exact=False):
    """Contiguous float64 tensor on `dev` of at least (exact: exactly) `count` elements."""
    if not torch.is_tensor(t) or t.dtype != torch.float64 or not t.is_contiguous() or t.device != dev \
            or (t.numel() != count if exact else t.numel() < count):
        raise EngineError(f"{what} must be a contiguous float64 tensor on {dev} of {'exactly' if exact else 'at least'} "
                          f"{count} elements")
    return t


def _snap(S, blocks, r, ncols, what):
    """Snapshot window: contiguous float32 device tensor [>= blocks, r, ncols]."""
    if (S.dtype != torch.float32 or not S.is_cuda or not S.is_contiguous() or S.dim() != 3 or S.shape[0] < blocks
            or tuple(S.shape[1:]) != (r, ncols)):
        raise EngineError(f"{what} must be a contiguous float32 device tensor [>= {blocks}, {r}, {ncols}]")
    return S


def _off(off, what):
    """Segment table of the grouped kernels -> ngroups."""
    if off.dtype != torch.int64 or not off.is_cuda or off.dim() != 1 or not off.is_contiguous() or off.numel() < 2:
        raise EngineError(f"{what}: the segment table must be a contiguous int64 device vector of ngroups + 1 entries")
    return off.numel() - 1


def _stack(M, what):
    if M.dim() != 3 or M.dtype != torch.float32 or not M.is_cuda or (M.shape[2] > 1 and M.stride(2) != 1):
        raise EngineError(f"{what}: expected a float32 device stack [groups, rows, cols] with unit inner stride")
    return M


def _out(out, shape, like, what):
    """The caller's `out` (a 2-D float32 matrix of `shape` on like's device), or a fresh one."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if _shaped(out, shape, what).device != like.device:
        raise EngineError(f"{what} must be on {like.device}, got {out.device}")
    return out


def _out64(out, count, dev, what):
    """The caller's float64 result words (_f64), or fresh ones."""
    return torch.empty(count, dtype=torch.float64, device=dev) if out is None else _f64(out, count, dev, what)


def _csr_triple(rowptr, colidx, vals, shape, what):
    """A canonical CSR triple on one device -- rowptr int64 [nrows + 1] from 0 to nnz and non-decreasing, colidx int32 [nnz]
    inside [0, ncols), vals float32 [nnz], all contiguous, nnz < 2^31 -> (nrows, ncols, nnz).  Reads four words back from the
    device: called once per matrix (CsrMatrix), not per launch."""
    nrows, ncols = int(shape[0]), int(shape[1])
    for t, dt, nm in ((rowptr, torch.int64, "rowptr"), (colidx, torch.int32, "colidx"), (vals, torch.float32, "vals")):
        if not torch.is_tensor(t) or t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or not t.is_cuda \
                or t.device != rowptr.device:
            raise EngineError(f"{what} {nm}: expected a contiguous 1-D {dt} tensor on the device of rowptr")
    nnz = vals.numel()
    if nrows < 1 or ncols < 1 or ncols >= 2 ** 31 or nnz >= 2 ** 31:
        raise EngineError(f"{what}: a {nrows} x {ncols} matrix with {nnz} stored entries is outside 1 <= extents, ncols and nnz < 2^31")
    if rowptr.numel() != nrows + 1 or colidx.numel() != nnz:
        raise EngineError(f"{what}: lengths do not fit, {nrows} rows, rowptr {rowptr.numel()}, colidx {colidx.numel()}, vals {nnz}")
    ends = torch.stack([rowptr[0], rowptr[-1], (rowptr[1:] - rowptr[:-1]).min()]).tolist()
    if ends[0] != 0 or ends[1] != nnz or ends[2] < 0:
        raise EngineError(f"{what} rowptr: must rise from rowptr[0] == 0 to rowptr[-1] == nnz ({nnz}); got {ends[0]} .. {ends[1]}")
    if nnz and not bool(((colidx >= 0) & (colidx < ncols)).all()):
        raise EngineError(f"{what} colidx: an index outside [0, {ncols})")
    return nrows, ncols, nnz


def csr_chunk_table(rowptr, ch):
    """The chunk table of include/nnfac_hip.h for chunks of at most `ch` stored entries: (rowchunk int64 [nrows + 1], chunk_row
    int32 [nchunks]); plain index arithmetic on rowptr's device (host tensors too: tests/test_sparse_plan.py)."""
    counts = (rowptr[1:] - rowptr[:-1] + (int(ch) - 1)) // int(ch)
    rowchunk = torch.zeros(rowptr.numel(), dtype=torch.int64, device=rowptr.device)
    torch.cumsum(counts, 0, out=rowchunk[1:])
    rows = torch.arange(counts.numel(), dtype=torch.int32, device=rowptr.device)
    return rowchunk, torch.repeat_interleave(rows, counts).contiguous()


class CsrMatrix:
    """A device CSR matrix with the chunk table the CSR kernels walk (Engine.csr_matrix): checked and cut into chunks once."""

    def __init__(self, eng, rowptr, colidx, vals, shape, ch=None):
        self.nrows, self.ncols, self.nnz = _csr_triple(rowptr, colidx, vals, shape, "csr_matrix")
        self.shape = (self.nrows, self.ncols)
        self.rowptr, self.colidx, self.vals, self.device = rowptr, colidx, vals, rowptr.device
        self.ch = int(ch) if ch is not None else eng.csr_chunk_entries(self.nnz)
        if not 1 <= self.ch <= 1 << 20:
            raise EngineError(f"csr_matrix: a chunk size of {self.ch} is outside 1 .. 2^20")
        self.rowchunk, self.chunk_row = csr_chunk_table(rowptr, self.ch)
        self.nchunks = self.chunk_row.numel()

    def args(self):
        """The argument run of the CSR entries."""
        return (_ptr(self.rowptr), _ptr(self.colidx), _ptr(self.vals), self.nrows, self.ncols, self.nnz, _ptr(self.rowchunk),
                _ptr(self.chunk_row), self.nchunks, self.ch)


def _node_major(F, nodes, what):
    """A gathered operand: nodes x r float32 on the device, unit inner stride, pitch a multiple of 4 floats, base 16-byte aligned
    -> r."""
    if _chk2d(F, what).shape[0] != nodes:
        raise EngineError(f"{what}: a node-major operand of {nodes} rows expected, got {tuple(F.shape)}")
    if _ld(F) % 4 != 0 or F.data_ptr() % 16 != 0:
        raise EngineError(f"{what}: a node-major operand needs a pitch that is a multiple of 4 floats and a 16-byte aligned base "
                          f"(node_major() makes one), got pitch {_ld(F)}")
    return F.shape[1]


def _obs_beta(beta, what):
    """beta of the observed-entries sums as a float: finite and >= 0."""
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise EngineError(f"{what}: beta must be a number, got {beta!r}") from None
    if not (0.0 <= b < float("inf")):
        raise EngineError(f"{what}: beta must be finite and >= 0, got {beta!r}")
    return b


def node_major(Ft):
    """The node-major copy (nodes x r, pitch r rounded up to 4 floats) of a component-major factor Ft (r x nodes): data movement."""
    r, nodes = Ft.shape
    buf = torch.zeros((nodes, (r + 3) // 4 * 4), dtype=torch.float32, device=Ft.device)
    view = buf[:, :r]
    view.copy_(Ft.t())
    return view


class KernelTime(float):
    """Mean launch duration in ms (the float) + the spread of the samples it came from."""

    @classmethod
    def of(cls, samples):
        ts = sorted(float(t) for t in samples)
        k = cls(sum(ts) / len(ts))
        k.n, k.median, k.min, k.max = len(ts), ts[len(ts) // 2], ts[0], ts[-1]
        return k

    def stats(self):
        return {"samples": self.n, "mean_ms": float(self), "median_ms": self.median, "min_ms": self.min, "max_ms": self.max}


class CsrOps:
    """The CSR entries of the engine (Engine inherits them): NMF on sparse data, over the stored entries only.  Their operand
    refusals are tested in tests/test_gpu_sparse_kernels.py, one spoilt operand at a time, as tests/test_gpu_engine_args.py does
    for the methods Engine defines itself."""

    def csr_chunk_entries(self, nnz):
        """Stored entries per chunk the library cuts a matrix of `nnz` stored entries into (nnf_csr_chunk_entries)."""
        return self._query("nnf_csr_chunk_entries", int(nnz))

    def csr_matrix(self, rowptr, colidx, vals, shape, ch=None):
        """A checked device CSR matrix with its chunk table (once per matrix; `ch`: another chunk size than the library's)."""
        return CsrMatrix(self, rowptr, colidx, vals, shape, ch=ch)

    @staticmethod
    def _csr_rank(A, Fn, what):
        if not isinstance(A, CsrMatrix):
            raise EngineError(f"{what}: the matrix must be a CsrMatrix (Engine.csr_matrix)")
        r = _node_major(Fn, A.ncols, what + " Fn")
        if Fn.device != A.device:
            raise EngineError(f"{what} Fn must be on {A.device}, got {Fn.device}")
        if r > MAX_RANK:
            raise EngineError(f"{what}: rank {r} is above the {MAX_RANK} the CSR kernels are built for")
        return r

    def csr_xf(self, A, Fn, out=None):
        """A (CsrMatrix, nrows x ncols), Fn (ncols x r, node-major) -> out[k, i] = sum_{p in row i} vals[p] Fn[colidx[p], k]
        (r x nrows): V X^T from the CSR of X and V^T, U^T X from the CSR of X^T and U (nnf_csr_xf_f32)."""
        r = self._csr_rank(A, Fn, "csr_xf")
        O = _out(out, (r, A.nrows), Fn, "csr_xf out")
        self._call("nnf_csr_xf_f32", *A.args(), *_mat(Fn), r, *_mat(O))
        return O

    def csr_kl(self, A, Own_n, Fn, num=True, cost_out=None, out=None):
        """The beta = 1 sums over the stored entries of A (nnf_csr_kl_f32): with p = <Own_n[i, :], Fn[j, :]> and q = x / p per
        stored x at (i, j), the numerator num[k, i] = sum q Fn[j, k] (r x nrows; `num=False`: not asked for) and, into the
        1-element float64 `cost_out`, sum (x log(x / p) - x).  Returns the numerator or None."""
        r = self._csr_rank(A, Fn, "csr_kl")
        if _node_major(Own_n, A.nrows, "csr_kl Own_n") != r or Own_n.device != A.device:
            raise EngineError(f"csr_kl Own_n: {A.nrows} x {r} on {A.device} expected, got {tuple(Own_n.shape)} on {Own_n.device}")
        if not num and cost_out is None:
            raise EngineError("csr_kl: nothing asked for")
        if cost_out is not None:
            _f64(cost_out, 1, A.device, "csr_kl cost_out")
        O = _out(out, (r, A.nrows), Fn, "csr_kl out") if num else None
        self._call("nnf_csr_kl_f32", *A.args(), *_mat(Own_n), *_mat(Fn), r, *_optmat(O), _opt(cost_out))
        return O

    def csr_obs(self, A, Own_n, Fn, beta, sums=True, cost_out=None, out_num=None, out_den=None):
        """The MU sums of any beta >= 0 over the stored entries of A, read as the OBSERVED ones (nnf_csr_obs_f32): with
        p = <Own_n[i, :], Fn[j, :]> per stored x at (i, j), num[k, i] = sum x p^(beta - 2) Fn[j, k] and den[k, i] = sum
        p^(beta - 1) Fn[j, k] (both r x nrows; `sums=False`: not asked for) and, into the 1-element float64 `cost_out`, sum
        d_beta(x | p).  A stored 0 is an observed zero; a row without stored entries gets num = den = 0.  Returns (num, den) or
        None.  Refusals: tests/test_gpu_observed_kernels.py, one spoilt operand at a time."""
        r = self._csr_rank(A, Fn, "csr_obs")
        if _node_major(Own_n, A.nrows, "csr_obs Own_n") != r or Own_n.device != A.device:
            raise EngineError(f"csr_obs Own_n: {A.nrows} x {r} on {A.device} expected, got {tuple(Own_n.shape)} on {Own_n.device}")
        beta = _obs_beta(beta, "csr_obs")
        if not sums and cost_out is None:
            raise EngineError("csr_obs: nothing asked for")
        if cost_out is not None:
            _f64(cost_out, 1, A.device, "csr_obs cost_out")
        N = _out(out_num, (r, A.nrows), Fn, "csr_obs out_num") if sums else None
        D = _out(out_den, (r, A.nrows), Fn, "csr_obs out_den") if sums else None
        self._call("nnf_csr_obs_f32", *A.args(), *_mat(Own_n), *_mat(Fn), r, beta, *_optmat(N), *_optmat(D), _opt(cost_out))
        return (N, D) if sums else None


class SparseMode:
    """One mode's sorted copy of a sparse tensor (include/nnfac_hip.h): `ptr` int64 [extent + 1] with the role of rowptr, `idx`
    int32 [N - 1, nnz] planar with the other modes (`others`, increasing) one per plane, `vals` float32 [nnz], and the chunk
    table of csr_chunk_table.  Checked once, as _csr_triple checks a CSR matrix."""

    def __init__(self, mode, ptr, idx, vals, shape, ch, what="sparse_tensor"):
        self.mode, self.extent, self.nnz = int(mode), int(shape[mode]), vals.numel()
        self.others = [m for m in range(len(shape)) if m != mode]
        self.extents = [int(shape[m]) for m in self.others]
        what = f"{what} mode {mode}"
        for t, dt, nd, nm in ((ptr, torch.int64, 1, "ptr"), (idx, torch.int32, 2, "idx"), (vals, torch.float32, 1, "vals")):
            if not torch.is_tensor(t) or t.dtype != dt or t.dim() != nd or not t.is_contiguous() or not t.is_cuda \
                    or t.device != ptr.device:
                raise EngineError(f"{what} {nm}: expected a contiguous {nd}-D {dt} tensor on the device of ptr")
        if ptr.numel() != self.extent + 1 or tuple(idx.shape) != (len(self.others), self.nnz):
            raise EngineError(f"{what}: lengths do not fit, extent {self.extent}, ptr {ptr.numel()}, idx {tuple(idx.shape)}, "
                              f"vals {self.nnz}")
        ends = torch.stack([ptr[0], ptr[-1], (ptr[1:] - ptr[:-1]).min()]).tolist()
        if ends[0] != 0 or ends[1] != self.nnz or ends[2] < 0:
            raise EngineError(f"{what} ptr: must rise from ptr[0] == 0 to ptr[-1] == nnz ({self.nnz}); got {ends[0]} .. {ends[1]}")
        if self.nnz:
            top = torch.tensor(self.extents, dtype=torch.int32, device=idx.device)[:, None]
            if not bool(((idx >= 0) & (idx < top)).all()):
                raise EngineError(f"{what} idx: an index outside its mode's extent {self.extents}")
        self.ptr, self.idx, self.vals, self.ch = ptr, idx, vals, int(ch)
        self.rowchunk, self.chunk_row = csr_chunk_table(ptr, self.ch)
        self.nchunks = self.chunk_row.numel()

    def args(self):
        """The argument run of the sparse-tensor entries up to the gathered factors."""
        return (_ptr(self.ptr), _ptr(self.idx), _ptr(self.vals), self.extent, self.nnz, _ptr(self.rowchunk), _ptr(self.chunk_row),
                self.nchunks, self.ch)


class SparseTensor:
    """A device sparse tensor of order 3 .. 5 as the sparse-tensor kernels walk it (Engine.sparse_tensor): one sorted copy per
    mode (SparseMode), each 4 N bytes per stored entry.  `indices` int64 [N, nnz] and `values` float32 [nnz] on one device,
    every index inside its extent; a coordinate stored twice is the caller's business (_convert.to_dev_coo sums duplicates).
    A copy is a stable sort of the list handed in by its mode's index: from the canonical (lexicographic) list every slice keeps
    its entries in lexicographic order of the other modes."""

    MIN_ORDER, MAX_ORDER = 3, 5

    def __init__(self, eng, indices, values, shape, ch=None):
        shape = tuple(int(s) for s in shape)
        N = len(shape)
        if not self.MIN_ORDER <= N <= self.MAX_ORDER:
            raise EngineError(f"sparse_tensor: order {N} is outside the {self.MIN_ORDER} .. {self.MAX_ORDER} the kernels are built for")
        for t, dt, nd, nm in ((indices, torch.int64, 2, "indices"), (values, torch.float32, 1, "values")):
            if not torch.is_tensor(t) or t.dtype != dt or t.dim() != nd or not t.is_cuda or t.device != indices.device:
                raise EngineError(f"sparse_tensor {nm}: expected a {nd}-D {dt} device tensor on the device of indices")
        nnz = values.numel()
        if tuple(indices.shape) != (N, nnz):
            raise EngineError(f"sparse_tensor: indices of shape {(N, nnz)} expected, got {tuple(indices.shape)}")
        if min(shape) < 1 or max(shape) >= 2 ** 31 or nnz >= 2 ** 31:
            raise EngineError(f"sparse_tensor: a tensor of shape {shape} with {nnz} stored entries is outside 1 <= extents and "
                              f"nnz < 2^31")
        top = torch.tensor(shape, dtype=torch.int64, device=indices.device)[:, None]
        if nnz and not bool(((indices >= 0) & (indices < top)).all()):
            raise EngineError(f"sparse_tensor indices: an index outside the shape {shape}")
        self.shape, self.order, self.nnz, self.device = shape, N, nnz, indices.device
        self.ch = int(ch) if ch is not None else eng.csr_chunk_entries(nnz)
        if not 1 <= self.ch <= 1 << 20:
            raise EngineError(f"sparse_tensor: a chunk size of {self.ch} is outside 1 .. 2^20")
        self.modes = []
        for n in range(N):
            order = torch.argsort(indices[n], stable=True)
            ptr = torch.zeros(shape[n] + 1, dtype=torch.int64, device=indices.device)
            torch.cumsum(torch.bincount(indices[n], minlength=shape[n]), 0, out=ptr[1:])
            others = [m for m in range(N) if m != n]
            idx = indices[others][:, order].to(torch.int32).contiguous()
            self.modes.append(SparseMode(n, ptr, idx, values[order].contiguous(), shape, self.ch))


class SparseTensorOps:
    """The sparse-tensor entries of the engine (Engine inherits them): NTF on sparse data, over the stored entries only.  Their
    operand refusals are tested in tests/test_gpu_sptensor_kernels.py, one spoilt operand at a time."""

    def sparse_tensor(self, indices, values, shape, ch=None):
        """A checked device sparse tensor with its N mode copies and their chunk tables (once per tensor; `ch`: another chunk
        size than the library's)."""
        return SparseTensor(self, indices, values, shape, ch=ch)

    @staticmethod
    def _sptensor_ops(S, mode, factors, what):
        """The copy of `mode` and its N - 1 gathered node-major factors (the other modes in increasing order, one common pitch)
        -> (copy, r, host array of device pointers, host array of extents, pitch)."""
        if not isinstance(S, SparseTensor):
            raise EngineError(f"{what}: the tensor must be a SparseTensor (Engine.sparse_tensor)")
        if not isinstance(mode, int) or not 0 <= mode < S.order:
            raise EngineError(f"{what}: mode {mode!r} is not a mode of a tensor of order {S.order}")
        M = S.modes[mode]
        factors = list(factors)
        if len(factors) != S.order - 1:
            raise EngineError(f"{what}: {S.order - 1} gathered factors (the modes {M.others}) expected, got {len(factors)}")
        r = None
        for m, F, ext in zip(M.others, factors, M.extents):
            if not torch.is_tensor(F):
                raise EngineError(f"{what} factor of mode {m}: a node-major device tensor expected, got {type(F).__name__}")
            rm = _node_major(F, ext, f"{what} factor of mode {m}")
            if F.device != S.device:
                raise EngineError(f"{what} factor of mode {m} must be on {S.device}, got {F.device}")
            if r is not None and rm != r:
                raise EngineError(f"{what}: the gathered factors differ in rank ({r} and {rm})")
            r = rm
        if r > MAX_RANK:
            raise EngineError(f"{what}: rank {r} is above the {MAX_RANK} the sparse-tensor kernels are built for")
        pitches = {_ld(F) for F in factors if F.shape[0] > 1}      # (the pitch of a single row addresses nothing)
        if len(pitches) > 1:
            raise EngineError(f"{what}: the gathered factors must share one pitch (node_major() gives it), got {sorted(pitches)}")
        ldn = pitches.pop() if pitches else (r + 3) // 4 * 4
        ptrs = (C.c_void_p * len(factors))(*[F.data_ptr() for F in factors])
        exts = (C.c_int64 * len(factors))(*M.extents)
        return M, r, ptrs, exts, ldn

    def sptensor_mttkrp(self, S, mode, factors_node_major, out=None):
        """The MTTKRP of `mode` over the stored entries of S (nnf_sptensor_mttkrp_f32): out[k, i] = sum_{p in slice i} x_p
        prod_{m != mode} F_m[i_m(p), k]  (r x extent).  `factors_node_major`: the N - 1 other factors, node-major (node_major()),
        in increasing mode order."""
        M, r, ptrs, exts, ldn = self._sptensor_ops(S, mode, factors_node_major, "sptensor_mttkrp")
        O = _out(out, (r, M.extent), M.vals, "sptensor_mttkrp out")
        self._call("nnf_sptensor_mttkrp_f32", *M.args(), len(exts), ptrs, exts, ldn, r, *_mat(O))
        return O

    def sptensor_kl(self, S, mode, Own_n, factors_node_major, num=True, cost_out=None, out=None):
        """The beta = 1 sums of `mode` over the stored entries of S (nnf_sptensor_kl_f32): with h = prod_{m != mode} F_m[i_m, :],
        p = <Own_n[i, :], h> and q = x / p per stored x, the numerator num[k, i] = sum q h[k] (r x extent; `num=False`: not asked
        for) and, into the 1-element float64 `cost_out`, sum (x log(x / p) - x).  Returns the numerator or None."""
        M, r, ptrs, exts, ldn = self._sptensor_ops(S, mode, factors_node_major, "sptensor_kl")
        if not torch.is_tensor(Own_n) or _node_major(Own_n, M.extent, "sptensor_kl Own_n") != r or Own_n.device != S.device:
            raise EngineError(f"sptensor_kl Own_n: {M.extent} x {r} on {S.device} expected, got {tuple(getattr(Own_n, 'shape', ()))} on "
                              f"{getattr(Own_n, 'device', None)}")
        if not num and cost_out is None:
            raise EngineError("sptensor_kl: nothing asked for")
        if cost_out is not None:
            _f64(cost_out, 1, S.device, "sptensor_kl cost_out")
        O = _out(out, (r, M.extent), M.vals, "sptensor_kl out") if num else None
        self._call("nnf_sptensor_kl_f32", *M.args(), len(exts), ptrs, exts, ldn, *_mat(Own_n), r, *_optmat(O), _opt(cost_out))
        return O

    def sptensor_obs(self, S, mode, Own_n, factors_node_major, beta, sums=True, cost_out=None, out_num=None, out_den=None):
        """The MU sums of `mode` at any beta >= 0 over the stored entries of S, read as the OBSERVED ones
        (nnf_sptensor_obs_f32): with h = prod_{m != mode} F_m[i_m, :] and p = <Own_n[i, :], h> per stored x, num[k, i] = sum
        x p^(beta - 2) h[k] and den[k, i] = sum p^(beta - 1) h[k] (both r x extent; `sums=False`: not asked for) and, into the
        1-element float64 `cost_out`, sum d_beta(x | p).  Returns (num, den) or None.  Refusals:
        tests/test_gpu_observed_kernels.py, one spoilt operand at a time."""
        M, r, ptrs, exts, ldn = self._sptensor_ops(S, mode, factors_node_major, "sptensor_obs")
        if not torch.is_tensor(Own_n) or _node_major(Own_n, M.extent, "sptensor_obs Own_n") != r or Own_n.device != S.device:
            raise EngineError(f"sptensor_obs Own_n: {M.extent} x {r} on {S.device} expected, got "
                              f"{tuple(getattr(Own_n, 'shape', ()))} on {getattr(Own_n, 'device', None)}")
        beta = _obs_beta(beta, "sptensor_obs")
        if not sums and cost_out is None:
            raise EngineError("sptensor_obs: nothing asked for")
        if cost_out is not None:
            _f64(cost_out, 1, S.device, "sptensor_obs cost_out")
        N = _out(out_num, (r, M.extent), M.vals, "sptensor_obs out_num") if sums else None
        D = _out(out_den, (r, M.extent), M.vals, "sptensor_obs out_den") if sums else None
        self._call("nnf_sptensor_obs_f32", *M.args(), len(exts), ptrs, exts, ldn, *_mat(Own_n), r, beta, *_optmat(N), *_optmat(D),
                   _opt(cost_out))
        return (N, D) if sums else None


class WeightedOps:
    """The weighted entries of the engine (Engine inherits them): the MU sums and the beta-divergence of dense data with a weight
    per entry (nn_fac_amd/weighted_nmf.py).  Their operand refusals are tested in tests/test_gpu_weighted_kernels.py, one spoilt
    operand at a time, as tests/test_gpu_engine_args.py does for the methods Engine defines itself."""

    @staticmethod
    def _xwuv(X, Wg, Ut, V, beta, what):
        """X, Wg (m x n, pitches of their own), Ut (r x m), V (r x n), beta >= 0 -> (m, n, r, beta)."""
        m, n, r = _xuv(X, Ut, V, what)
        if _shaped(Wg, (m, n), what + " Wg").device != X.device:
            raise EngineError(f"{what} Wg must be on {X.device}, got {Wg.device}")
        if r > MAX_RANK:
            raise EngineError(f"{what}: rank {r} is above the {MAX_RANK} the weighted kernels are built for")
        return m, n, r, _obs_beta(beta, what)

    def mu_left_w(self, X, Wg, Ut, V, beta, out_num=None, out_den=None):
        """num[k, i] = sum_j Wg X P^(beta-2) V[k, j], den[k, i] = sum_j Wg P^(beta-1) V[k, j] with P = Ut^T V (both r x m; nnf_mu_left_w_f32).
        An entry of weight 0 is out of both sums whatever X holds there.  Returns (num, den); mu_apply(Ut, num, den, None, beta) is
        the update."""
        m, n, r, beta = self._xwuv(X, Wg, Ut, V, beta, "mu_left_w")
        N = _out(out_num, (r, m), Ut, "mu_left_w out_num")
        D = _out(out_den, (r, m), Ut, "mu_left_w out_den")
        self._call("nnf_mu_left_w_f32", _ptr(X), m, n, _ld(X), *_mat(Wg), *_mat(Ut), *_mat(V), r, beta, *_mat(N), *_mat(D))
        return N, D

    def mu_right_w(self, X, Wg, Ut, V, beta, out_num=None, out_den=None):
        """num[k, j] = sum_i Wg X P^(beta-2) Ut[k, i], den[k, j] = sum_i Wg P^(beta-1) Ut[k, i] (both r x n; nnf_mu_right_w_f32)."""
        m, n, r, beta = self._xwuv(X, Wg, Ut, V, beta, "mu_right_w")
        N = _out(out_num, (r, n), V, "mu_right_w out_num")
        D = _out(out_den, (r, n), V, "mu_right_w out_den")
        self._call("nnf_mu_right_w_f32", _ptr(X), m, n, _ld(X), *_mat(Wg), *_mat(Ut), *_mat(V), r, beta, *_mat(N), *_mat(D))
        return N, D

    def mu_mode_w(self, T3, W3, Ft, V, beta, out_num=None, out_den=None):
        """The sums of mu_mode under a weight per entry (nnf_mu_mode_w_f32): `T3` the contiguous tensor seen as (L, I_n, K), `W3`
        its weights in the same shape, `Ft` (r x I_n), `V` (r x L*K).  num[k, i] = sum_{l,j} W3 T3 P^(beta-2) V[k, l*K+j],
        den[k, i] = sum_{l,j} W3 P^(beta-1) V[k, l*K+j] (both r x I_n); r <= 64.  Returns (num, den); mu_apply finishes."""
        L, I, K = _t3(T3, "mu_mode_w: T3, seen as (L, I, K),").shape
        _t3(W3, "mu_mode_w: W3, the weights of T3,")
        if W3.shape != T3.shape or W3.device != T3.device:
            raise EngineError(f"mu_mode_w W3: {tuple(T3.shape)} on {T3.device} expected, got {tuple(W3.shape)} on {W3.device}")
        r = _chk2d(Ft, "mu_mode_w Ft").shape[0]
        if Ft.shape[1] != I:
            raise EngineError(f"mu_mode_w Ft: shape mismatch, T3 is {tuple(T3.shape)}, Ft {tuple(Ft.shape)}")
        _shaped(V, (r, L * K), "mu_mode_w V")
        if r > self.MU_MODE_MAX_RANK:
            raise EngineError("mu_mode_w Ft: built for r <= 64")
        beta = _obs_beta(beta, "mu_mode_w")
        N = _out(out_num, (r, I), Ft, "mu_mode_w out_num")
        D = _out(out_den, (r, I), Ft, "mu_mode_w out_den")
        self._call("nnf_mu_mode_w_f32", _ptr(T3), _ptr(W3), L, I, K, *_mat(Ft), *_mat(V), r, beta, *_mat(N), *_mat(D))
        return N, D

    def betadiv_w(self, X, Wg, Ut, V, beta, out=None):
        """sum_ij Wg[i, j] d_beta(X[i, j] | (Ut^T V)[i, j]) into a 1-element float64 device tensor (nnf_betadiv_w_f32)."""
        m, n, r, beta = self._xwuv(X, Wg, Ut, V, beta, "betadiv_w")
        o = _out64(out, 1, X.device, "betadiv_w out")
        self._call("nnf_betadiv_w_f32", _ptr(X), m, n, _ld(X), *_mat(Wg), *_mat(Ut), *_mat(V), r, beta, _ptr(o))
        return o


class Engine(CsrOps, SparseTensorOps, WeightedOps):
    """One context (workspace + device properties) per device."""

    def __init__(self, device, workspace_bytes=0):
        if not torch.cuda.is_available():
            raise EngineError("no ROCm device available: the nn_fac_amd engine is GPU-only (no CPU fallback)")
        self.device = torch.device(device)
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.call(self.lib, "nnf_ctx_create", C.byref(h), self.device.index or 0, workspace_bytes)
        self.ctx = h
        self._resident_cols = {}

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.nnf_ctx_destroy(self.ctx)
        except Exception:  # interpreter shutdown
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        """The one way into a compute entry: `name`(ctx, *args, current stream), found on self.lib by name (a proxy put there
        sees every call); a non-zero status raises EngineError under that name."""
        _lib.call(self.lib, name, self.ctx, *args, self._stream())

    def _query(self, name, *args):
        """An int64 property of the context: `name`(ctx, *args, &value)."""
        out = C.c_int64(0)
        _lib.call(self.lib, name, self.ctx, *args, C.byref(out))
        return int(out.value)

    # ---- contractions -------------------------------------------------------------------------------
    def gram(self, A, out=None, out64=None):
        """A (r x K) -> A A^T (r x r).  out64 (optional, contiguous r x r float64 device tensor): also receives the sums before
        they are rounded to fp32 (nnf_gram_f64_f32), for gram_cost(..., UtU64=...)."""
        r, K = _chk2d(A, "gram A").shape
        if out64 is not None:
            _f64(out64, r * r, A.device, "gram out64")
        G = _out(out, (r, r), A, "gram out")
        if out64 is None:
            self._call("nnf_gram_f32", _ptr(A), r, K, _ld(A), *_mat(G))
        else:
            self._call("nnf_gram_f64_f32", _ptr(A), r, K, _ld(A), *_mat(G), _ptr(out64))
        return G

    def xht(self, X, V, out=None):
        """V (r x n), X (m x n) -> V X^T (r x m)."""
        m, n, r = _xf(X, V, 1, "xht", "V")
        O = _out(out, (r, m), X, "xht out")
        self._call("nnf_xht_f32", _ptr(X), m, n, _ld(X), _ptr(V), r, _ld(V), *_mat(O))
        return O

    def xty(self, X, Ut, out=None):
        """Ut (r x m), X (m x n) -> Ut X (r x n)."""
        m, n, r = _xf(X, Ut, 0, "xty", "Ut")
        O = _out(out, (r, n), X, "xty out")
        self._call("nnf_xty_f32", _ptr(X), m, n, _ld(X), _ptr(Ut), r, _ld(Ut), *_mat(O))
        return O

    def xty_gram(self, X, Ut, out=None, G=None, G64=None):
        """xty(X, Ut, out) and gram(Ut, G, G64) in one main launch and one slab reduction (nnf_xty_gram_f32): the same bits as
        the two calls.  Returns (Ut X, Ut Ut^T)."""
        m, n, r = _xf(X, Ut, 0, "xty_gram", "Ut")
        if G64 is not None:
            _f64(G64, r * r, X.device, "xty_gram G64")
        O, G = _out(out, (r, n), X, "xty_gram out"), _out(G, (r, r), X, "xty_gram G")
        self._call("nnf_xty_gram_f32", _ptr(X), m, n, _ld(X), _ptr(Ut), r, _ld(Ut), *_mat(O), *_mat(G), _opt(G64))
        return O, G

    def xht_gram(self, X, V, out=None, G=None):
        """xht(X, V, out) and gram(V, G) in one main launch and one slab reduction (nnf_xht_gram_f32): the same bits as the two
        calls.  Returns (V X^T, V V^T)."""
        m, n, r = _xf(X, V, 1, "xht_gram", "V")
        O, G = _out(out, (r, m), X, "xht_gram out"), _out(G, (r, r), X, "xht_gram G")
        self._call("nnf_xht_gram_f32", _ptr(X), m, n, _ld(X), _ptr(V), r, _ld(V), *_mat(O), *_mat(G))
        return O, G

    def frob_resid(self, X, Ut, V, out=None):
        """sum (X - Ut^T V)^2 as a 1-element float64 device tensor."""
        m, n, r = _xuv(X, Ut, V, "frob_resid")
        o = _out64(out, 1, X.device, "frob_resid out")
        self._model_scratch(m, n, r)
        self._call("nnf_frob_resid_f32", *_triple(X, Ut, V), _ptr(o))
        return o

    def _model_scratch(self, m, n, r):
        """Ranks above 128: the cost passes build the model U V over rank chunks in an m x n float32 buffer (nnf_ctx_set_scratch);
        kept between calls, grown when a larger one is asked for."""
        if r <= MAX_RANK:
            return
        need = int(m) * ((int(n) + 3) // 4 * 4) * 4
        cur = getattr(self, "_scratch", None)
        if cur is None or cur.numel() < need:
            torch.cuda.current_stream(self.device).synchronize()      # (earlier calls may still read the old buffer)
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
            _lib.call(self.lib, "nnf_ctx_set_scratch", self.ctx, _ptr(self._scratch), need)

    def gram_cost(self, V, UtM, UtU, normx2, out, UtU_b=None, rounding=None, UtU64=None):
        """||X - U V||^2 through the Gram identity (nnf_nmf_gram_cost_cal_f32): `normx2` a 1-element float64 device tensor holding
        ||X||^2, `out` >= 3 float64 on the device: {cost, 1 if the fp32 operands do not carry it to 5e-4, error estimate}.
        rounding = (relative rms, |relative mean|) of the rounding error of a UtM entry (default: 6e-8, 0)."""
        r, n = _solve_ops(UtM, UtU, V, "gram_cost")
        _f64(normx2, 1, V.device, "gram_cost normx2"), _f64(out, 3, V.device, "gram_cost out")
        _gram_pair(UtU, UtU_b, "gram_cost UtU_b")
        sa, ba = (6e-8, 0.0) if rounding is None else (float(rounding[0]), float(rounding[1]))
        if UtU64 is None:
            self._call("nnf_nmf_gram_cost_cal_f32", *_mat(V), *_mat(UtM), _ptr(UtU), _opt(UtU_b), _ld(UtU), r, n, _ptr(normx2),
                       sa, ba, _ptr(out))
            return out
        # (the kernel reads r x r doubles with row stride r, whatever UtU's leading dimension is)
        if UtU_b is not None:
            raise EngineError("gram_cost: UtU64 cannot be combined with a Hadamard pair (UtU_b)")
        _f64(UtU64, r * r, V.device, "gram_cost UtU64", exact=True)
        # the quadratic form on the Gram before its rounding to fp32; rounding[2] = relative rms error of a UtU64 entry
        sg = float(rounding[2]) if rounding is not None and len(rounding) > 2 else 1e-8
        self._call("nnf_nmf_gram_cost_g64_f32", *_mat(V), *_mat(UtM), _ptr(UtU), _ptr(UtU64), _ld(UtU), r, n, _ptr(normx2),
                   sa, ba, sg, _ptr(out))
        return out

    def cross_rounding(self, X, Ut, blocks=16):
        """(relative rms, |relative mean|) of the rounding error the W^T X kernel leaves in an entry of U^T X at THIS shape: the
        product summed in one piece (row splits of the launch plan, fp32 accumulators per workgroup) against the same product
        summed over `blocks` row blocks in float64 -- whose fp32 chains are `blocks` times shorter, so that the difference is
        the long chains' error to ~1/sqrt(blocks).  Two passes over X, once per run (nmf.run_steps)."""
        m = int(X.shape[0])
        full = self.xty(X, Ut).double()
        acc = torch.zeros_like(full)
        step = -(-m // int(blocks))
        step = -(-step // 256) * 256
        for lo in range(0, m, step):
            hi = min(m, lo + step)
            acc += self.xty(X[lo:hi], Ut[:, lo:hi]).double()
        rel = (full - acc) / acc.clamp_min(1e-300)
        rel = torch.where(acc > 0, rel, torch.zeros_like(rel))
        return float(rel.pow(2).mean().sqrt()), abs(float(rel.mean()))

    def gram_rounding(self, Ut, blocks=16):
        """Relative rms error of an entry of the fp64 Gram of nnf_gram_f64_f32 at THIS shape (the fp32 accumulation inside a
        split of the Gram kernel): the Gram in one piece against the sum of the Grams of `blocks` column blocks, whose chains
        are `blocks` times shorter.  r x r work, once per run."""
        r, m = Ut.shape
        full = torch.empty((r, r), dtype=torch.float64, device=Ut.device)
        self.gram(Ut, out64=full)
        acc, part = torch.zeros_like(full), torch.empty_like(full)
        step = -(-m // int(blocks))
        step = -(-step // 256) * 256
        for lo in range(0, m, step):
            self.gram(Ut[:, lo:min(m, lo + step)], out64=part)
            acc += part
        rel = (full - acc) / acc.abs().clamp_min(1e-300)
        rel = torch.where(acc != 0, rel, torch.zeros_like(rel))
        return float(rel.pow(2).mean().sqrt())

    def dot(self, A, B):
        _shaped(B, _chk2d(A, "dot A").shape, "dot B")
        o = torch.empty(1, dtype=torch.float64, device=A.device)
        self._call("nnf_dot_f32", *_mat(A), *_mat(B), A.shape[0], A.shape[1], _ptr(o))
        return o

    def hadamard(self, A, B, out=None):
        """out = A .* B, element by element.  A and B may be views (they are copied to contiguous buffers first: a non-contiguous
        A or B is therefore not refused); a caller's `out` is written as it lies and must be contiguous."""
        _f32(A, A.shape, "hadamard A"), _f32(B, A.shape, "hadamard B")
        if out is not None:
            _f32(out, A.shape, "hadamard out", contiguous=True)
        A, B = A.contiguous(), B.contiguous()
        Cc = torch.empty_like(A) if out is None else out
        self._call("nnf_hadamard_f32", _ptr(A), _ptr(B), _ptr(Cc), A.numel())
        return Cc

    # ---- HALS ---------------------------------------------------------------------------------------
    @staticmethod
    def _hals_flags(sparsity, normalize, nonzero):
        f = 0
        if sparsity is not None:
            f |= HALS_SPARSITY
        if normalize:
            f |= HALS_NORMALIZE
        if nonzero:
            f |= HALS_NONZERO
        return f

    ROWSYNC_MAX_COLUMNS = 131072          # normalize / nonzero: one column per resident thread (k_hals.hip generic path)

    def _check_rowsync_columns(self, rowsync, ncols):
        """normalize=True / nonzero=True need a grid-wide reduction per ROW update, which the generic kernel does with every
        column resident (one per thread, 4 x 128-thread workgroups per CU): say so here instead of a bare status code.
        (persistent solves go on beyond that limit, row by row from the host: _hals_solve_rowwalk; fixed-count sweeps do not.)"""
        if rowsync and ncols > self.ROWSYNC_MAX_COLUMNS:
            raise EngineError(f"fixed-count sweeps with normalize=True / nonzero=True are built for at most "
                              f"{self.ROWSYNC_MAX_COLUMNS} columns (got {ncols}): every row update needs all columns "
                              f"resident on the device at once; normalise the shorter factor, or split the columns and "
                              f"normalise on the host between outer iterations")

    def _hals_solve_rowwalk(self, UtM, UtU, V, max_sweeps, delta, sparsity, st, normalize=True, nonzero=False):
        """hals_nnls_acc(..., normalize=True) on more columns than the generic kernel keeps resident: the rows are walked from
        the host -- row update over all columns (nnf_hals_row_update_f32), row norm, scaling (nnf_hals_row_scale_f32), r x 2
        launches per sweep and one host round trip per sweep for the stopping rule of nnls.py:156 -- the one-device form of the
        row-sharded protocol (dist.sharded_hals_solve_rownorm, which this calls without a group).  Correct and slow (a sweep of a
        rank-50 factor is 100 launches): the option is on no BASELINE configuration."""
        from . import dist as _dist
        eps, cnt, eps0 = _dist.sharded_hals_solve_rownorm(self, UtM, UtU, V, None, budget=int(max_sweeps), delta=float(delta),
                                                          sparsity=sparsity, normalize=normalize, nonzero=nonzero)
        write_status(st, eps, float(cnt), eps0)
        return st

    HALS_MAX_SWEEPS_PER_LAUNCH = 1000     # NNF_HALS_MAX_SWEEPS (exchange tags hold the sweep index in 10 bits)

    def hals_solve(self, UtM, UtU, V, max_sweeps, delta=0.01, sparsity=None, normalize=False, nonzero=False,
                   status=None):
        """In-place accelerated HALS on V (r x ncols); returns the 8-double status tensor (device, not synced)."""
        r, ncols = _solve_ops(UtM, UtU, V, "hals_solve")
        st = _out64(status, ST_WORDS, V.device, "hals_solve status")
        if (normalize or nonzero or r > MAX_RANK) and ncols > self.ROWSYNC_MAX_COLUMNS and int(max_sweeps) > 0:
            # (ranks above 128 run in the generic kernel too: one column per resident thread for a persistent solve)
            return self._hals_solve_rowwalk(UtM, UtU, V, max_sweeps, delta, sparsity, st, normalize=normalize, nonzero=nonzero)
        self._check_rowsync_columns(normalize or nonzero, ncols)
        ops = _solve_args(UtM, UtU, V)
        rule = (float(delta), float(sparsity or 0.0), self._hals_flags(sparsity, normalize, nonzero), _ptr(st))
        total, first = int(max_sweeps), min(int(max_sweeps), self.HALS_MAX_SWEEPS_PER_LAUNCH)
        self._call("nnf_hals_solve_f32", *ops, first, *rule)
        done = first
        while done < total:      # maxiter beyond one launch's tag range: chained launches, no host round trip in between
            step = min(total - done, self.HALS_MAX_SWEEPS_PER_LAUNCH)
            self._call("nnf_hals_solve_continue_f32", *ops, done, step, *rule)
            done += step
        return st

    def hals_solve_cross(self, UtM, Ga, Gb, V_in, V_out, max_sweeps, delta=0.01, sparsity=None, normalize=False, status=None):
        """hals_solve with the Gram Ga .* Gb (Gb may be None), start values V_in and the result in V_out (ntf.py:442-456)."""
        r, ncols = _chk2d(V_out, "hals_solve_cross V_out").shape
        _shaped(UtM, (r, ncols), "hals_solve_cross UtM"), _shaped(V_in, (r, ncols), "hals_solve_cross V_in")
        if _chk2d(Ga, "hals_solve_cross Ga").shape[0] < r or Ga.shape[1] < r:
            raise EngineError(f"hals_solve_cross Ga: a Gram of at least {r} x {r} expected, got {tuple(Ga.shape)}")
        _gram_pair(Ga, Gb, "hals_solve_cross Gb")
        st = _out64(status, ST_WORDS, V_out.device, "hals_solve_cross status")
        if normalize and ncols > self.ROWSYNC_MAX_COLUMNS and int(max_sweeps) > 0:
            if V_out.data_ptr() != V_in.data_ptr():
                V_out.copy_(V_in)
            return self._hals_solve_rowwalk(UtM, Ga if Gb is None else self.hadamard(Ga[:r, :r], Gb[:r, :r]), V_out, max_sweeps,
                                            delta, sparsity, st)
        self._check_rowsync_columns(normalize, ncols)
        self._call("nnf_hals_solve_cross_f32", *_mat(UtM), _ptr(Ga), _opt(Gb), _ld(Ga), *_mat(V_in), *_mat(V_out), r, ncols,
                   int(max_sweeps), float(delta), float(sparsity or 0.0), self._hals_flags(sparsity, normalize, False), _ptr(st))
        return st

    def hals_sweeps(self, UtM, UtU, V, nsweeps, sparsity=None, normalize=False, nonzero=False, snapshots=None, snap_first=0,
                    sweeps_done=0, resid_in=None, resid_out=None):
        """Exactly `nsweeps` in-place sweeps; returns the per-sweep LOCAL sum of squared steps (float64, device).
        snapshots (optional, contiguous float32 [>= nsweeps - snap_first, r, ncols]): block j receives V after sweep
        snap_first + j + 1.  sweeps_done / resid_in / resid_out: this call continues a solve of which `sweeps_done` sweeps have
        run (nnf_hals_sweeps_ex_f32): with the residual state handed on (float32 tensors of hals_resid_floats() elements) the
        chunks of a solve are bit for bit one launch of all its sweeps."""
        r, ncols = _solve_ops(UtM, UtU, V, "hals_sweeps")
        if snapshots is not None:
            _snap(snapshots, nsweeps - int(snap_first), r, ncols, "hals_sweeps snapshots")
        need = self.hals_resid_floats(r, ncols) if (resid_in is not None or resid_out is not None) else 0
        for t in (resid_in, resid_out):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < need or t.device != V.device):
                raise EngineError("hals_sweeps: a residual-state buffer (resid_in, resid_out) must be a contiguous float32 "
                                  "tensor of hals_resid_floats() elements")
        if (normalize or nonzero) and ncols > self.ROWSYNC_MAX_COLUMNS and snapshots is None and int(nsweeps) > 0:
            # more columns than the generic kernel keeps resident: the rows are walked from the host, one sweep per call of the
            # row-walk (the wall-clock rule's one-sweep probe of nmf() / hals_nnls_acc(deterministic=False) lands here)
            from . import dist as _dist
            vals = [_dist.sharded_hals_solve_rownorm(self, UtM, UtU, V, None, budget=1, delta=0.0, sparsity=sparsity,
                                                     normalize=normalize, nonzero=nonzero)[0] for _ in range(int(nsweeps))]
            return torch.tensor(vals, dtype=torch.float64, device=V.device)
        self._check_rowsync_columns(normalize or nonzero, ncols)
        nd = torch.zeros(max(int(nsweeps), 1), dtype=torch.float64, device=V.device)
        keep = need > 0           # (the other kernel layouts carry no state and take NULL)
        self._call("nnf_hals_sweeps_ex_f32", *_solve_args(UtM, UtU, V), int(nsweeps), int(sweeps_done), float(sparsity or 0.0),
                   self._hals_flags(sparsity, normalize, nonzero), _ptr(nd), *_optblocks(snapshots), int(snap_first),
                   _opt(resid_in if keep else None), _opt(resid_out if keep else None))
        return nd[:int(nsweeps)]

    def hals_resid_floats(self, r, ncols):
        """Elements of one residual-state buffer for blind chunks on an r x ncols factor (0: the layout that runs keeps no state)."""
        return self._query("nnf_hals_resid_floats", int(r), int(ncols))

    def hals_row_update(self, UtM, UtU, V, k, sparsity=None, out=None):
        """Row k of V (this rank's columns) gets the update of nnls.py:162-170, in place; returns a 2-element float64 device
        tensor {sum of squared steps, sum of squares of the updated row} (row-sharded solves with normalize, dist.py)."""
        _solve_ops(UtM, UtU, V, "hals_row_update")
        o = _out64(out, 2, V.device, "hals_row_update out")
        self._call("nnf_hals_row_update_f32", *_solve_args(UtM, UtU, V), int(k), float(sparsity or 0.0),
                   self._hals_flags(sparsity, False, False), _ptr(o))
        return o

    def hals_row_scale(self, V, k, normsq, ncols_total):
        """Row k of V /= sqrt(normsq[0]) (a float64 device scalar), or := 1 / sqrt(ncols_total) when it is 0 (nnls.py:181-185)."""
        _chk2d(V, "hals_row_scale V"), _f64(normsq, 1, V.device, "hals_row_scale normsq")
        self._call("nnf_hals_row_scale_f32", *_mat(V), V.shape[1], int(k), _ptr(normsq), int(ncols_total))
        return V

    def hals_resident_columns(self, r):
        """Columns the register-resident sweep kernel of rank r holds on this device (blind chunks with snapshots, and fast
        sweeps at all, need column blocks of at most this size: dist.sharded_hals_solve)."""
        hit = self._resident_cols.get(int(r))
        if hit is None:
            hit = self._resident_cols[int(r)] = self._query("nnf_hals_resident_columns", int(r))
        return hit

    # ---- grouped kernels (PARAFAC2: K per-slice problems per launch) ------------------------------------
    def hals_group_max_columns(self, r):
        """Longest group hals_solve_group takes (nnf_hals_group_max_columns); longer ones go through hals_solve."""
        return self._query("nnf_hals_group_max_columns", int(r))

    def hals_solve_group(self, UtM, UtU, V, off, max_group_cols, max_sweeps, delta=0.01, status=None):
        """One accelerated-HALS solve per group in ONE launch, in place on V (r x total): group g owns the columns
        [off[g], off[g+1]), its Gram is UtU[g] (a [groups, r, r] stack).  `max_group_cols`: the caller's bound on the group
        lengths (the table lives on the device).  Returns the [groups, 8] float64 status tensor (device, not synced)."""
        r, total = _chk2d(V, "hals_solve_group V").shape
        _shaped(UtM, (r, total), "hals_solve_group UtM"), _stack(UtU, "hals_solve_group UtU")
        ng = _off(off, "hals_solve_group off")
        if UtU.shape[0] != ng or UtU.shape[1] < r or UtU.shape[2] < r:
            raise EngineError(f"hals_solve_group UtU: expected [{ng}, >= {r}, >= {r}], got {tuple(UtU.shape)}")
        st = torch.zeros((ng, ST_WORDS), dtype=torch.float64, device=V.device) if status is None else \
            _f64(status, ng * ST_WORDS, V.device, "hals_solve_group status")
        self._call("nnf_hals_solve_group_f32", *_mat(UtM), _ptr(UtU), UtU.stride(1), UtU.stride(0), *_mat(V), r, _ptr(off), ng,
                   int(max_group_cols), total, int(max_sweeps), float(delta), _ptr(st))
        return st

    def group_gram(self, A, off, B=None, T=None, gram=True, out64=None):
        """Per group of columns of A (r x total), one pass: (G [groups, r, r] float32 = A_g A_g^T or None, dots [groups, r] float64
        = sum_i A[q,i] B[q,i] or None, err [groups] float64 = ||A_g - T_g||_F^2 or None).  out64 (optional, contiguous
        [groups, r, r] float64 device tensor): also receives the Gram sums before they are rounded to fp32."""
        r, total = _chk2d(A, "group_gram A").shape
        ng = _off(off, "group_gram off")
        for t, nm in ((B, "B"), (T, "T")):
            if t is not None:
                _shaped(t, A.shape, "group_gram " + nm)
        if not gram and B is None and T is None:
            raise EngineError("group_gram: nothing asked for")
        if out64 is not None:
            if not gram:
                raise EngineError("group_gram out64: the fp64 Gram sums come with gram=True only")
            _f64(out64, ng * r * r, A.device, "group_gram out64")
        G = torch.empty((ng, r, r), dtype=torch.float32, device=A.device) if gram else None
        dots = torch.empty((ng, r), dtype=torch.float64, device=A.device) if B is not None else None
        errs = torch.empty(ng, dtype=torch.float64, device=A.device) if T is not None else None
        self._call("nnf_group_gram_f32", *_mat(A), r, _ptr(off), ng, total, _opt(G), r, r * r, _opt(out64), *_optmat(B), _opt(dots),
                   *_optmat(T), _opt(errs))
        return G, dots, errs

    def group_gemm(self, M, A, off, max_group_cols, out=None):
        """out[:, seg g] = M[g] @ A[:, seg g] for a [groups, p, q] stack M (p, q <= 128) and A (q x total)."""
        q, total = _chk2d(A, "group_gemm A").shape
        ng, p = _off(off, "group_gemm off"), _stack(M, "group_gemm M").shape[1]
        if M.shape[0] != ng or M.shape[2] != q:
            raise EngineError(f"group_gemm M: expected [{ng}, p, {q}], got {tuple(M.shape)}")
        O = _out(out, (p, total), A, "group_gemm out")
        if O.data_ptr() == A.data_ptr():
            raise EngineError("group_gemm out must not alias A")
        self._call("nnf_group_gemm_f32", _ptr(M), M.stride(1), M.stride(0), p, q, *_mat(A), _ptr(off), ng, int(max_group_cols),
                   total, *_mat(O))
        return O

    def frob_resid_rows(self, X, Ut, V, out=None):
        """Per-row ||x_i - (Ut^T V)_i||^2 as m float64 on the device (one streaming pass, nnf_frob_resid_rows_f32)."""
        m, n, r = _xuv(X, Ut, V, "frob_resid_rows")
        o = _out64(out, m, X.device, "frob_resid_rows out")
        self._call("nnf_frob_resid_rows_f32", *_triple(X, Ut, V), _ptr(o))
        return o

    def hals_stop_restore(self, sums, head, budget, delta, V, snapshots, status):
        """Device-side replay of the stopping rule over the all-reduced per-sweep sums of a blind chunk (dist.py): `snapshots`
        (or None) holds V after each of the last sums.numel() - head sweeps.  One block per sweep of the window is asked for, as
        hals_sweeps writes them; that is one more than the replay can ever restore from (a stop at the last sweep restores
        nothing), so the rule is stricter than the library needs.  `sums` sets the number of sweeps: it has no wrong length.
        `status` takes the first four words of a solve's status block (eps, cnt, eps0, err)."""
        r, ncols = _chk2d(V, "hals_stop_restore V").shape
        n = _f64(sums, 1, V.device, "hals_stop_restore sums").numel()
        _f64(status, ST_ERR + 1, V.device, "hals_stop_restore status")
        if snapshots is not None:
            _snap(snapshots, n - int(head), r, ncols, "hals_stop_restore snapshots")
        self._call("nnf_hals_stop_restore_f32", _ptr(sums), n, int(head), int(budget), float(delta), *_mat(V), r, ncols,
                   *_optblocks(snapshots), _ptr(status))
        return status

    # ---- MU / beta-divergence -----------------------------------------------------------------------
    MU_FUSED_MAX_RANK = 64   # the fused COST forms (mu_left(cost_out=...), mu_left_num) are built for r <= 64
    MU_FUSED_UPDATE_MAX_RANK = 128   # the fused two-MFMA updates: r <= 128 for every beta (beta = 2 has no limit: Gram form)

    def _mu_large_rank(self, X, Ut, V, beta, side, checked=False):
        """r > 128 (any beta; the model then builds up over rank chunks inside R1; callable at any rank, which is how
        tools/time_mu_rank.py times it against the fused kernels): one pass writes the element-wise operands R1 = X.*(UV)^(beta-2), R2 = (UV)^(beta-1)
        (m x n device scratch each), then the numerator / denominator are plain X H^T ('left') or W^T X ('right') products.
        Returns (num, den or None, den_vec or None) like mu_right_accum.  `checked`: the caller has run _xuv on the triple."""
        (m, n) = X.shape if checked else _xuv(X, Ut, V, "_mu_large_rank")[:2]
        kl = float(beta) == 1.0
        R1 = torch.empty((m, n), dtype=torch.float32, device=X.device)
        R2 = None if kl else torch.empty((m, n), dtype=torch.float32, device=X.device)
        self._call("nnf_mu_ratio_f32", *_triple(X, Ut, V), float(beta), _ptr(R1), _opt(R2), _ld(R1))
        if side == "left":
            num = self.xht(R1, V)
            den = None if kl else self.xht(R2, V)
            dvec = V.sum(dim=1, dtype=torch.float64) if kl else None          # mu.py:86-87
        else:
            num = self.xty(R1, Ut)
            den = None if kl else self.xty(R2, Ut)
            dvec = Ut.sum(dim=1, dtype=torch.float64) if kl else None
        return num, den, dvec

    def _mu_composed(self, r, beta):
        """Whether an update of rank r goes through _mu_large_rank + mu_apply (no fused kernel there)."""
        return (r > self.MU_FUSED_UPDATE_MAX_RANK and float(beta) != 2.0) or r > MAX_RANK

    def mu_left(self, X, Ut, V, beta, out=None, cost_out=None):
        """`cost_out` (1-element float64 device tensor; beta = 1, r <= 64 only): also receives beta_divergence(X, U V, 1) of
        the INPUT factors (nnf_mu_left_kl_cost_f32)."""
        m, n, r = _xuv(X, Ut, V, "mu_left")
        if cost_out is not None:
            if float(beta) != 1.0 or r > self.MU_FUSED_MAX_RANK:
                raise EngineError("mu_left cost_out: the fused cost is built for beta = 1 and r <= 64")
            _f64(cost_out, 1, X.device, "mu_left cost_out")
        O = _out(out, (r, m), Ut, "mu_left out")
        if cost_out is not None:
            self._call("nnf_mu_left_kl_cost_f32", *_triple(X, Ut, V), *_mat(O), _ptr(cost_out))
        elif self._mu_composed(r, beta):
            self.mu_apply(Ut, *self._mu_large_rank(X, Ut, V, beta, "left", checked=True), beta, out=O)
        else:
            self._call("nnf_mu_left_f32", *_triple(X, Ut, V), float(beta), *_mat(O))
        return O

    MU_MODE_MAX_RANK = 64   # the mode update on the tensor's own layout (mu_mode)

    def mu_mode(self, T3, Ft, V, beta, out=None):
        """mu_betadivmin of one mode's factor against tl.unfold(T, n) without forming it: `T3` is the contiguous tensor seen
        as (L, I_n, K), `Ft` the mode's transposed factor (r x I_n), `V` the other operand (r x L*K, column l*K + k for the
        entries T3[l, :, k]).  r <= 64 (nnf_mu_mode_f32)."""
        L, I, K = _t3(T3, "mu_mode: T3, seen as (L, I, K),").shape
        r = _chk2d(Ft, "mu_mode Ft").shape[0]
        if Ft.shape[1] != I:
            raise EngineError(f"mu_mode Ft: shape mismatch, T3 is {tuple(T3.shape)}, Ft {tuple(Ft.shape)}")
        _shaped(V, (r, L * K), "mu_mode V")
        if r > self.MU_MODE_MAX_RANK:
            raise EngineError("mu_mode Ft: built for r <= 64")
        O = _out(out, (r, I), Ft, "mu_mode out")
        self._call("nnf_mu_mode_f32", _ptr(T3), L, I, K, *_mat(Ft), *_mat(V), r, float(beta), *_mat(O))
        return O

    def mu_right(self, X, Ut, V, beta, out=None):
        m, n, r = _xuv(X, Ut, V, "mu_right")
        O = _out(out, (r, n), V, "mu_right out")
        if self._mu_composed(r, beta):
            self.mu_apply(V, *self._mu_large_rank(X, Ut, V, beta, "right", checked=True), beta, out=O)
        else:
            self._call("nnf_mu_right_f32", *_triple(X, Ut, V), float(beta), *_mat(O))
        return O

    def mu_right_accum(self, X, Ut, V, beta):
        """This row block's numerator / denominator of the right update (row-sharded runs): returns (num r x n,
        den r x n or None, den_vec r doubles or None); all three are sums over the rows and all-reduce additively."""
        m, n, r = _xuv(X, Ut, V, "mu_right_accum")
        if self._mu_composed(r, beta):
            return self._mu_large_rank(X, Ut, V, beta, "right", checked=True)
        num = torch.empty((r, n), dtype=torch.float32, device=X.device)
        den = torch.empty((r, n), dtype=torch.float32, device=X.device) if float(beta) != 1.0 else None
        dvec = torch.empty(r, dtype=torch.float64, device=X.device) if float(beta) == 1.0 else None
        self._call("nnf_mu_right_accum_f32", *_triple(X, Ut, V), float(beta), *_mat(num), *_optmat(den), _opt(dvec))
        return num, den, dvec

    def mu_apply(self, F, num, den, den_vec, beta, out=None):
        """out = max(F * (num/den)^gamma(beta), 1e-12) (mu.py:84-97) from already reduced numerator / denominator."""
        r, cols = _chk2d(F, "mu_apply F").shape
        _shaped(num, (r, cols), "mu_apply num")
        if den is not None:
            _shaped(den, (r, cols), "mu_apply den")
        if den_vec is not None:
            _f64(den_vec, r, F.device, "mu_apply den_vec")
        O = _out(out, (r, cols), F, "mu_apply out")
        self._call("nnf_mu_apply_f32", *_mat(F), r, cols, *_mat(num), *_optmat(den), _opt(den_vec), float(beta), *_mat(O))
        return O

    SIMPLEX_MAX_ITER = 1024   # Newton iterations one nnf_simplex_proj_kl_f32 call takes (one stopping slot each)

    def simplex_proj(self, H, num, den, den_vec, tol=1e-6, max_iter=100, lambda0=None, out=None, lambda_out=None, status=None,
                     update=True):
        """simplex_proj_mu at beta = 1 from reduced operands (mu.py:161-175; normalize_wh.py:24-58): the Newton solve for the
        per-column multipliers -- from `lambda0` (cols float64) or the reference's start -- and, with `update`, the update of H
        that puts its columns on the unit simplex.  `num`, and exactly one of `den` (r x cols) and `den_vec` (r float64), are
        what mu_right_accum(..., 1) returns.  Returns (H_out or None, status): status = 2 float64 on the device, {iterations run,
        max |dlambda| of the last one}; `lambda_out` (cols float64) receives the multipliers.  `out` may be H itself."""
        r, cols = _chk2d(H, "simplex_proj H").shape
        _shaped(num, (r, cols), "simplex_proj num")
        if (den is None) == (den_vec is None):
            raise EngineError("simplex_proj: exactly one of den / den_vec is given")
        if den is not None:
            _shaped(den, (r, cols), "simplex_proj den")
        for name, t, count in (("den_vec", den_vec, r), ("lambda0", lambda0, cols), ("lambda_out", lambda_out, cols)):
            if t is not None:
                _f64(t, count, H.device, "simplex_proj " + name)
        if r > MAX_RANK or not 1 <= int(max_iter) <= self.SIMPLEX_MAX_ITER:
            raise EngineError(f"simplex_proj: built for r <= {MAX_RANK} and 1 <= max_iter <= {self.SIMPLEX_MAX_ITER}")
        st = _out64(status, 2, H.device, "simplex_proj status")
        O = _out(out, (r, cols), H, "simplex_proj out") if update else None
        self._call("nnf_simplex_proj_kl_f32", *_mat(H), r, cols, *_mat(num), *_optmat(den), _opt(den_vec), _opt(lambda0),
                   float(tol), int(max_iter), *_optmat(O), _opt(lambda_out), _ptr(st))
        return O, st

    # ---- deep KL-NMF (deep_mu.py:8-14) -------------------------------------------------------------
    def mu_left_num(self, X, Ut, V, out=None):
        """Raw KL numerator of the left update: num[k,i] = sum_j (X[i,j] / (UV)[i,j]) V[k,j]  (r x m)."""
        m, n, r = _xuv(X, Ut, V, "mu_left_num")
        O = _out(out, (r, m), X, "mu_left_num out")
        self._call("nnf_mu_left_num_f32", *_triple(X, Ut, V), *_mat(O))
        return O

    def small_gemm(self, A, B, out=None):
        """A (p x q, q <= 2048) @ B (q x cols) -> p x cols: a rank-sized left operand against a wide matrix."""
        (p, q), cols = _chk2d(A, "small_gemm A").shape, _chk2d(B, "small_gemm B").shape[1]
        if B.shape[0] != q:
            raise EngineError(f"small_gemm B: shape mismatch, A is {p} x {q}, B {tuple(B.shape)}")
        O = _out(out, (p, cols), A, "small_gemm out")
        self._call("nnf_small_gemm_f32", *_mat(A), p, q, *_mat(B), cols, *_mat(O))
        return O

    def deep_kl_apply(self, Ft, num, hsum, WHnext_t, lam, out=None):
        """max(1e-12, (b/lam) / (W0(b exp(a/lam)/lam) + 1e-12)) with b = Ft .* num, a = hsum[k] - lam log(WHnext_t)."""
        r, cols = _chk2d(Ft, "deep_kl_apply Ft").shape
        _shaped(num, (r, cols), "deep_kl_apply num"), _shaped(WHnext_t, (r, cols), "deep_kl_apply WHnext_t")
        _f64(hsum, r, Ft.device, "deep_kl_apply hsum", exact=True)
        O = _out(out, (r, cols), Ft, "deep_kl_apply out")
        self._call("nnf_deep_kl_apply_f32", *_mat(Ft), r, cols, *_mat(num), _ptr(hsum), *_mat(WHnext_t), float(lam), *_mat(O))
        return O

    PROBE_KERNELS = {"xty": 0, "xht": 1, "cost": 2, "hals": 3, "mu_left": 4, "mu_right": 5, "mttkrp": 6}

    def set_probe(self, ev_begin=None, ev_end=None, kernel="xty"):
        """Measurement hook (bench.py): two torch.cuda.Event(enable_timing=True) that the library records on the launch
        stream right before and right after the main kernel named by `kernel` (NNF_PROBE_* of include/nnfac_hip.h); call
        with no arguments to remove them.  The events must have been recorded once already (torch creates the underlying
        hipEvent_t lazily)."""
        b = C.c_void_p(ev_begin.cuda_event) if ev_begin is not None else None
        e = C.c_void_p(ev_end.cuda_event) if ev_end is not None else None
        _lib.call(self.lib, "nnf_ctx_set_probe_kernel", self.ctx, self.PROBE_KERNELS[kernel])
        _lib.call(self.lib, "nnf_ctx_set_probe", self.ctx, b, e)

    def set_probe_ring(self, pairs=None, kernel="xty"):
        """Measurement hook for a whole timed region (bench.py): `pairs` = [(begin, end), ...] of already recorded
        torch.cuda.Event(enable_timing=True); the i-th launch of `kernel` from now on records pair i on its launch stream
        (launches beyond the list record nothing).  None removes the ring (nnf_ctx_set_probe_ring)."""
        _lib.call(self.lib, "nnf_ctx_set_probe_kernel", self.ctx, self.PROBE_KERNELS[kernel])
        if not pairs:
            _lib.call(self.lib, "nnf_ctx_set_probe_ring", self.ctx, None, 0)
            return
        arr = (C.c_void_p * (2 * len(pairs)))(*[C.c_void_p(e.cuda_event) for pr in pairs for e in pr])
        _lib.call(self.lib, "nnf_ctx_set_probe_ring", self.ctx, arr, len(pairs))

    def probe_ring_count(self):
        """Pairs of the current ring recorded so far."""
        return int(self.lib.nnf_ctx_probe_ring_count(self.ctx))

    @staticmethod
    def probe_pairs(n, stream):
        """n (begin, end) pairs of timing events, each recorded once on `stream` (torch creates the hipEvent_t lazily)."""
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in evs:
            a.record(stream)
            b.record(stream)
        return evs

    def time_kernel(self, kernel, fn, reps=20):
        """Duration (ms) of the main kernel `kernel` over `reps` calls of `fn` (which must launch it exactly once on the
        current stream), measured with HIP events recorded by the library immediately around that kernel.  Returns a
        `KernelTime`: the plain MEAN over all samples as a float (nothing is dropped), with .median / .min / .max / .n."""
        stream = torch.cuda.current_stream(self.device)
        evs = self.probe_pairs(reps, stream)
        fn()
        stream.synchronize()
        try:
            self.set_probe_ring(evs, kernel)
            for _ in range(reps):
                fn()
        finally:
            self.set_probe_ring(None, kernel)
        stream.synchronize()
        return KernelTime.of([a.elapsed_time(b) for a, b in evs])

    # ---- NTD -----------------------------------------------------------------------------------------
    def mttkrp3_from_partial(self, Y, Ft, axis, out=None):
        """Y (R x A x B, contiguous) contracted with the rows of Ft over `axis` (1: A, 2: B) -> R x (the other extent)."""
        R, A, B = _t3(Y, "mttkrp3_from_partial: Y").shape
        _shaped(Ft, (R, A if axis == 1 else B), "mttkrp3_from_partial Ft")
        O = _out(out, (R, B if axis == 1 else A), Y, "mttkrp3_from_partial out")
        self._call("nnf_mttkrp3_from_partial_f32", _ptr(Y), A, B, *_mat(Ft), R, int(axis), *_mat(O))
        return O

    def ttm3(self, T, Ft, mode, out=None):
        """T x_mode F^T for a contiguous 3-way tensor and a transposed factor Ft (r x I_mode).
        Result layout: mode 0 -> (r, J, K); mode 1 -> (I, r, K); mode 2 -> (r, I, J)  (include/nnfac_hip.h)."""
        I, J, K = _t3(T, "ttm3: T", err.ArgumentException).shape
        r = _chk2d(Ft, "ttm3 Ft").shape[0]
        if mode not in (0, 1, 2) or Ft.shape[1] != T.shape[mode]:
            raise EngineError(f"ttm3 Ft: r x {tuple(T.shape)}[mode] with mode in 0..2 expected, got {tuple(Ft.shape)}, mode {mode}")
        shape = (r, J, K) if mode == 0 else ((I, r, K) if mode == 1 else (r, I, J))
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=T.device)
        elif _t3(out, "ttm3: out").shape != shape or out.device != T.device:
            raise EngineError(f"ttm3: out must have shape {shape} on {T.device}, got {tuple(out.shape)} on {out.device}")
        self._call("nnf_ttm3_f32", _ptr(T), I, J, K, *_mat(Ft), r, int(mode), _ptr(out))
        return out

    def ntd_core_pg(self, core, MtX, grams, sparse, delta, max_iter, norm_sq, status=None):
        """Projected-gradient core update (ntd.py:588-619), in place on `core`; returns the 6-double status block
        {iterations, last update, first update, step, reconstruction error, 0} (device tensor, no sync)."""
        if core.dim() != 3:
            raise err.ArgumentException("ntd_core_pg updates a contiguous float32 3-way core in place")
        MtX, M, st = _core_ops(core, MtX, grams, status, "ntd_core_pg")
        self._call("nnf_ntd_core_pg_f32", _ptr(core), _ptr(MtX), _ptr(M[0]), _ptr(M[1]), _ptr(M[2]), *core.shape, float(sparse),
                   float(delta), int(max_iter), float(norm_sq), _ptr(st))
        return st

    def ntd_core_pgn(self, core, MtX, grams, sparse, delta, max_iter, norm_sq, status=None):
        """ntd_core_pg for a core of any order 3..8 (nnf_ntd_core_pgn_f32: the mode products run mode by mode, no merged
        trailing mode); in place on `core`, returns the same 6-double status block."""
        MtX, M, st = _core_ops(core, MtX, grams, status, "ntd_core_pgn")
        n = core.dim()
        ptrs = (C.c_void_p * n)(*[g.data_ptr() for g in M])
        dims = (C.c_int * n)(*[int(d) for d in core.shape])
        self._call("nnf_ntd_core_pgn_f32", _ptr(core), _ptr(MtX), ptrs, n, dims, float(sparse), float(delta), int(max_iter),
                   float(norm_sq), _ptr(st))
        return st

    def betadiv(self, X, Ut, V, beta, out=None):
        m, n, r = _xuv(X, Ut, V, "betadiv")
        o = _out64(out, 1, X.device, "betadiv out")
        self._model_scratch(m, n, r)
        self._call("nnf_betadiv_f32", *_triple(X, Ut, V), float(beta), _ptr(o))
        return o

    def mttkrp3(self, T, Ft, mode, out=None):
        """T (I x J x K, contiguous), Ft = [F0^T, F1^T, F2^T] (each R x dim) -> R x dim_mode."""
        R = _cp3(T, Ft, "mttkrp3")
        O = _out(out, (R, T.shape[mode]), T, "mttkrp3 out")
        self._call("nnf_mttkrp3_f32", *_cp3_args(T, Ft), int(mode), *_mat(O))
        return O

    CP3_FUSED_MAX_RANK = 64

    def cp3_partial_cost(self, T, Ft, Y, cost):
        """One pass over T: cost[0] = ||T - [[F0,F1,F2]]||^2 (float64 device scalar) and Y[r][i][j] = sum_k T[i,j,k] F2[k,r]."""
        R = _cp3(T, Ft, "cp3_partial_cost")
        if _t3(Y, "cp3_partial_cost: Y").shape != (R, *T.shape[:2]) or Y.device != T.device:
            raise EngineError(f"cp3_partial_cost: Y must be R x I x J on {T.device}, got {tuple(Y.shape)} on {Y.device}")
        _f64(cost, 1, T.device, "cp3_partial_cost cost")
        self._call("nnf_cp3_partial_cost_f32", *_cp3_args(T, Ft), _ptr(Y), _ptr(cost))
        return Y

    def cp3_betadiv(self, T, Ft, beta, out=None):
        """beta-divergence between T (I x J x K) and the CP model of Ft = [F0^T, F1^T, F2^T]; float64 device scalar."""
        R = _cp3(T, Ft, "cp3_betadiv")
        o = _out64(out, 1, T.device, "cp3_betadiv out")
        self._model_scratch(T.shape[0] * T.shape[1], T.shape[2], R)
        self._call("nnf_cp3_betadiv_f32", *_cp3_args(T, Ft), float(beta), _ptr(o))
        return o


class Comm:
    """RCCL communicator of the C ABI (nnf_comm_*): what a C-ABI consumer uses for the row-sharded exchanges.  The Python
    drivers go through torch.distributed (the same RCCL underneath); this wrapper exists for the ABI tests and for hosts
    that do not initialise torch.distributed."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _lib.call(_lib.load(), "nnf_comm_unique_id", buf)
        return buf.raw

    def __init__(self, engine, nranks, rank, unique_id):
        self.engine = engine
        h = C.c_void_p()
        _lib.call(engine.lib, "nnf_comm_create", C.byref(h), engine.ctx, int(nranks), int(rank),
                  C.create_string_buffer(unique_id, 128))
        self.h = h

    def size(self):
        return self.engine.lib.nnf_comm_size(self.h)

    def rank(self):
        return self.engine.lib.nnf_comm_rank(self.h)

    def allreduce_(self, t):
        if not t.is_cuda or not t.is_contiguous() or t.dtype not in (torch.float32, torch.float64):
            raise EngineError("Comm.allreduce_: contiguous float32 / float64 device tensor expected")
        _lib.call(self.engine.lib, "nnf_allreduce_f32" if t.dtype == torch.float32 else "nnf_allreduce_f64", self.h, _ptr(t),
                  t.numel(), self.engine._stream())
        return t

    def close(self):
        if getattr(self, "h", None):
            self.engine.lib.nnf_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def get_engine(device=None):
    """Process-wide engine for `device` (default: current device)."""
    if not torch.cuda.is_available():
        raise EngineError("no ROCm device available: the nn_fac_amd engine is GPU-only (no CPU fallback)")
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    if dev.index is None:
        dev = torch.device(f"cuda:{torch.cuda.current_device()}")
    with _lock:
        e = _engines.get(dev.index)
        if e is None:
            # 1 GiB of scratch for the main context (NNF_WORKSPACE_MB overrides): the split-K slabs of W^T X at 10^6 x 4000 rank
            # 100 are 780 MB when a workgroup sums at most 2048 rows in fp32 (k_xty.hip: launch_xty) -- with the C default of
            # 256 MiB the plan falls back to longer chains.  Side contexts keep the default.
            mb = int(os.environ.get("NNF_WORKSPACE_MB", "1024"))
            e = Engine(dev, workspace_bytes=mb << 20)
            _engines[dev.index] = e
        return e


_side = {}


def get_side_engine(device, role="gram"):
    """Process-wide extra context + stream of `device` per role, for work that overlaps with a launch on the main stream (a
    context's workspace serves one stream at a time).  Created once: context creation allocates and clears its workspace."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with _lock:
        e = _side.get((idx, role))
        if e is None:
            e = (Engine(torch.device(f"cuda:{idx}"), workspace_bytes=64 << 20), torch.cuda.Stream(device=idx))
            _side[(idx, role)] = e
        return e

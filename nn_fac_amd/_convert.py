"""Boundary conversions: the drop-in functions accept NumPy arrays or torch tensors and answer in kind."""
import numpy as np
import torch

from .utils.errors import EngineError


def device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise EngineError("no ROCm device available: the nn_fac_amd engine is GPU-only (no CPU fallback)")
    return torch.device(f"cuda:{torch.cuda.current_device()}")


def to_dev(x, device):
    """float32, device-resident, unit inner stride.  NumPy (any float dtype) and CPU tensors are uploaded;
    a conforming device tensor is returned as is (no copy)."""
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=torch.float32)
    else:
        a = np.asarray(x)
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    if t.dim() >= 1 and t.stride(-1) != 1:
        t = t.contiguous()
    return t


def to_dev_t(x, device):
    """Device float32 copy/view of x^T with unit inner stride (x: m x r -> r x m).  No copy if x is already a
    transposed view of such a tensor."""
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=torch.float32).t()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x).T, dtype=np.float32)).to(device)
    if t.stride(-1) != 1:
        t = t.contiguous()
    return t


def _is_scipy_sparse(x):
    return type(x).__module__.startswith("scipy.sparse") and hasattr(x, "tocsr")


def is_sparse(x):
    """A scipy.sparse matrix or array of any format, or a torch sparse-CSR tensor (the inputs of nn_fac_amd.sparse_nmf)."""
    if isinstance(x, torch.Tensor):
        return x.layout == torch.sparse_csr
    return _is_scipy_sparse(x)


def to_dev_csr(x, device, transpose=False):
    """Canonical CSR of a sparse input (of its transpose: `transpose`) on the device: (rowptr int64, colidx int32, vals float32,
    shape) with sorted indices and no duplicates; stored zeros stay.  Never through a dense copy: a SciPy input is converted
    on the host (`.tocsr()`, `sum_duplicates()`, `sort_indices()`; the transpose by `.T.tocsr()`), a torch CSR tensor -- host or
    device, taken as canonical -- on the device (the transpose by a stable sort of the entries by column)."""
    if isinstance(x, torch.Tensor):
        m, n = x.shape
        rowptr = x.crow_indices().to(device=device, dtype=torch.int64)
        colidx = x.col_indices().to(device=device, dtype=torch.int64)
        vals = x.values().to(device=device, dtype=torch.float32)
        if transpose:
            rows = torch.repeat_interleave(torch.arange(m, dtype=torch.int64, device=device), rowptr[1:] - rowptr[:-1])
            order = torch.argsort(colidx, stable=True)      # row-major in, so every new row keeps its entries sorted
            counts = torch.bincount(colidx, minlength=n)
            rowptr = torch.zeros(n + 1, dtype=torch.int64, device=device)
            torch.cumsum(counts, 0, out=rowptr[1:])
            colidx, vals, (m, n) = rows[order], vals[order], (n, m)
        return rowptr.contiguous(), colidx.to(torch.int32).contiguous(), vals.contiguous(), (int(m), int(n))
    a = (x.T if transpose else x).tocsr(copy=True)      # (a copy: the caller's matrix is not canonicalised in place)
    a.sum_duplicates()
    a.sort_indices()
    return (torch.from_numpy(a.indptr.astype(np.int64)).to(device), torch.from_numpy(a.indices.astype(np.int32)).to(device),
            torch.from_numpy(a.data.astype(np.float32)).to(device), (int(a.shape[0]), int(a.shape[1])))


class SparseCOO:
    """A sparse tensor as coordinate lists (the input of nn_fac_amd.sparse_ntf next to a torch sparse-COO tensor): `indices` an
    N x nnz integer array or tensor, `values` a float array or tensor of nnz entries, `shape` the N extents.  Entries may be
    unsorted and a coordinate may be stored more than once (the values are summed)."""

    def __init__(self, indices, values, shape):
        self.indices, self.values, self.shape = indices, values, tuple(int(s) for s in shape)
        if len(np.shape(indices)) != 2 or len(np.shape(values)) != 1 or tuple(np.shape(indices)) != (len(self.shape), np.shape(values)[0]):
            raise ValueError(f"SparseCOO: indices of shape {(len(self.shape), 'nnz')} and values of shape ('nnz',) expected, got "
                             f"{tuple(np.shape(indices))} and {tuple(np.shape(values))}")

    @property
    def ndim(self):
        return len(self.shape)


def is_sparse_tensor(x):
    """A torch sparse-COO tensor or a SparseCOO (the inputs of nn_fac_amd.sparse_ntf)."""
    if isinstance(x, torch.Tensor):
        return x.layout == torch.sparse_coo
    return isinstance(x, SparseCOO)


def to_dev_coo(x, device):
    """The canonical coordinate list of a sparse tensor input on the device: (indices int64 [N, nnz], values float32 [nnz], shape)
    with the entries in lexicographic order of their coordinates and no coordinate twice -- duplicates are summed in fp32, in
    input order inside a coordinate, after a stable sort; stored zeros stay.  Never through a dense copy, and never through a
    linear index (the product of five extents below 2^31 does not fit 64 bits): one stable sort per mode, last mode first."""
    if isinstance(x, torch.Tensor):
        if x.dense_dim() != 0:
            raise EngineError("a sparse tensor with dense dimensions is not a coordinate list of scalars")
        ind, val, shape = x._indices(), x._values(), tuple(int(s) for s in x.shape)      # (as stored: coalesced or not)
    else:
        ind, val, shape = x.indices, x.values, x.shape
    if not isinstance(ind, torch.Tensor):
        ind = torch.from_numpy(np.ascontiguousarray(np.asarray(ind), dtype=np.int64))
    if not isinstance(val, torch.Tensor):
        val = torch.from_numpy(np.ascontiguousarray(np.asarray(val), dtype=np.float32))
    ind, val = ind.to(device=device, dtype=torch.int64), val.to(device=device, dtype=torch.float32)
    nnz = val.numel()
    order = torch.arange(nnz, dtype=torch.int64, device=device)
    for m in reversed(range(len(shape))):
        order = order[torch.argsort(ind[m][order], stable=True)]
    ind, val = ind[:, order], val[order]
    if nnz > 1:
        first = torch.ones(nnz, dtype=torch.bool, device=device)      # the first entry of every coordinate
        first[1:] = (ind[:, 1:] != ind[:, :-1]).any(dim=0)
        if not bool(first.all()):
            seg = torch.cumsum(first, 0) - 1
            starts = torch.nonzero(first).flatten()
            nth = torch.arange(nnz, dtype=torch.int64, device=device) - starts[seg]
            out = val[starts].clone()
            for k in range(1, int(nth.max()) + 1):      # the k-th duplicate of every coordinate that has one: distinct targets
                sel = nth == k
                out[seg[sel]] += val[sel]
            ind, val = ind[:, starts], out
    return ind.contiguous(), val.contiguous(), shape


def observed_entries(array, mask):
    """The sparse input that holds exactly the entries of the dense `array` (NumPy or torch, order >= 2) where the boolean `mask`
    (same shape) is set, ZEROS INCLUDED, in row-major order: a torch sparse-CSR tensor for a matrix, a SparseCOO for order >= 3,
    on the device of a torch `array`.  The input of unstored="missing" runs (sparse_nmf.py, sparse_ntf.py), where a stored zero
    is an observed zero: scipy.sparse.csr_matrix(dense) drops zeros and would turn them into missing entries."""
    a = array if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(array)))
    if isinstance(mask, torch.Tensor):
        w = mask.to(a.device)
    else:
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(mask))).to(a.device)
    if w.dtype != torch.bool or tuple(w.shape) != tuple(a.shape) or a.dim() < 2:
        raise ValueError(f"observed_entries: a boolean mask of the array's shape {tuple(a.shape)} (order >= 2) expected, got "
                         f"{w.dtype} {tuple(w.shape)}")
    indices = torch.nonzero(w).t().contiguous()      # N x nnz, lexicographic
    values = a[w]
    if a.dim() > 2:
        return SparseCOO(indices, values, a.shape)
    crow = torch.zeros(a.shape[0] + 1, dtype=torch.int64, device=a.device)
    torch.cumsum(w.sum(dim=1), 0, out=crow[1:])
    return torch.sparse_csr_tensor(crow, indices[1], values, size=tuple(a.shape))


def like_input(t, proto):
    """Return device tensor `t` in the type/dtype of the caller's `proto` (ndarray -> ndarray of its dtype)."""
    if isinstance(proto, torch.Tensor):
        return t if proto.is_cuda else t.to(proto.device, proto.dtype)
    dt = np.asarray(proto).dtype if proto is not None else np.float64
    if not np.issubdtype(dt, np.floating):
        dt = np.float64
    return t.detach().cpu().numpy().astype(dt, copy=False)

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


def like_input(t, proto):
    """Return device tensor `t` in the type/dtype of the caller's `proto` (ndarray -> ndarray of its dtype)."""
    if isinstance(proto, torch.Tensor):
        return t if proto.is_cuda else t.to(proto.device, proto.dtype)
    dt = np.asarray(proto).dtype if proto is not None else np.float64
    if not np.issubdtype(dt, np.floating):
        dt = np.float64
    return t.detach().cpu().numpy().astype(dt, copy=False)

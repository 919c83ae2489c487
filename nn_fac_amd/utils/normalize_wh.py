"""normalize_WH and the multiplier solve of simplex NMF (nn_fac/utils/normalize_wh.py:6-58).

normalize_WH is the scaling multilayer NMF applies between its layers (multilayer_nmf.py:47-51): the product W H is unchanged,
one factor is divided by the sums of the chosen factor, the other multiplied by them.  Host arithmetic on the caller's arrays.

update_lagragian_multipliers_simplex_projection (:24-58, the reference's spelling) is the per-column Newton solve behind
simplex_proj_mu (mu.py:161-175), on the device at beta = 1 (nnf_simplex_proj_kl_f32; every other beta is refused,
nn_fac_amd/simplex_nmf.py says why).  The experiments of the same file the reference itself marks as not working (:61-162) are
not restated.
NumPy in -> NumPy out; torch tensors (host or device) in -> tensors out.
"""
import numpy as np
import torch

eps = 1e-8   # normalize_wh.py:4


def normalize_WH(W, H, matrix):
    if matrix not in ("W", "H"):
        raise ValueError(f"Matrix must be either 'W' or 'H', but it is {matrix}")
    is_t = isinstance(W, torch.Tensor) or isinstance(H, torch.Tensor)
    if matrix == "H":                       # rows of H sum to one (normalize_wh.py:8-10)
        scale = H.sum(dim=1) if is_t else np.sum(H, axis=1)
        return W * scale[None, :], H / scale[:, None]
    scale = W.sum(dim=0) if is_t else np.sum(W, axis=0)      # columns of W sum to one (:13-15)
    return W / scale[None, :], H * scale[:, None]


def update_lagragian_multipliers_simplex_projection(C, D, H, beta, lagrangian_multipliers_0, tol=1e-6, n_iter_max=100):
    """normalize_wh.py:24-58 at beta = 1: C, D, H are k x n, lagrangian_multipliers_0 is n x 1; returns the n x 1 multipliers
    after at most n_iter_max (<= 1024) Newton iterations, all columns stopped together.  The operands go to the device as
    float32, the start values and the iteration in float64."""
    from .. import engine as _engine
    from .. import simplex_nmf as _sx
    from .._convert import device_of, to_dev, like_input
    _sx.check_beta(beta, "update_lagragian_multipliers_simplex_projection")
    _sx.check_rank(H.shape[0], "update_lagragian_multipliers_simplex_projection")
    if not 1 <= int(n_iter_max) <= _engine.Engine.SIMPLEX_MAX_ITER:
        raise _engine.EngineError(f"update_lagragian_multipliers_simplex_projection: n_iter_max must lie in 1 .. "
                                  f"{_engine.Engine.SIMPLEX_MAX_ITER} (got {n_iter_max})")
    n = H.shape[1]
    dev = device_of(C, D, H, lagrangian_multipliers_0)
    eng = _engine.get_engine(dev)
    if isinstance(lagrangian_multipliers_0, torch.Tensor):
        lam0 = lagrangian_multipliers_0.to(device=dev, dtype=torch.float64).reshape(n).contiguous()
    else:
        lam0 = torch.from_numpy(np.ascontiguousarray(np.asarray(lagrangian_multipliers_0, dtype=np.float64).reshape(n))).to(dev)
    lam = torch.empty(n, dtype=torch.float64, device=dev)
    _, status = eng.simplex_proj(to_dev(H, dev), to_dev(C, dev), to_dev(D, dev), None, tol=tol, max_iter=n_iter_max, lambda0=lam0,
                                 lambda_out=lam, update=False)
    count, last = status.cpu().tolist()
    _sx.newton_warning(count, last, tol, n_iter_max)
    return like_input(lam.reshape(n, 1), lagrangian_multipliers_0)

"""What the NTF and NTD drivers keep of their tensor on the device, and the MU update of one of its modes."""
import math
import os

import torch

from . import dist as _dist
from ._outer_loop import StatusRing


class TensorState(StatusRing):
    """Device-resident contiguous tensor, its squared norm (`group`: T is this rank's block of the leading mode -- summed
    over the ranks) and, MU only, the materialised unfoldings; the driver adds its status ring."""

    def __init__(self, eng, T, group=None):
        self.eng, self.group = eng, group
        self.T = T.contiguous()
        self.nway = self.T.dim()
        self.t0 = self.T.view(self.T.shape[0], -1)
        self.norm2 = eng.dot(self.t0, self.t0)          # float64 device scalar, ||T||^2
        if _dist.is_sharded(group):
            _dist.allreduce_(self.norm2, group)
        self._unf = {}

    def unfolded_t(self, mode):
        """tl.unfold(T, mode)^T = moveaxis(mode -> last).reshape(-1, dim) as a contiguous (prod(other dims)) x I_mode matrix
        (MU path).  The last mode is a view of T; the others are materialised once per run -- only above rank 64 or under
        NNF_MU_UNFOLD=1 (mu_on_layout)."""
        if mode not in self._unf:
            self._unf[mode] = torch.movedim(self.T, mode, -1).reshape(-1, self.T.shape[mode]).contiguous()
        return self._unf[mode]


def mode_view(T, mode):
    """The contiguous tensor as (prod of the extents before `mode`, I_mode, prod of those behind): a view."""
    shape = [int(d) for d in T.shape]
    return T.view(math.prod(shape[:mode]), shape[mode], math.prod(shape[mode + 1:]))


def mu_on_layout(eng, r):
    """Whether the MU update of a mode other than the last (whose unfolding is a view) runs on the tensor's own layout
    (Engine.mu_mode) instead of a materialised unfolding: up to the kernel's rank, unless NNF_MU_UNFOLD=1 (read at call time)."""
    return r <= eng.MU_MODE_MAX_RANK and os.environ.get("NNF_MU_UNFOLD") != "1"


def mu_mode_update(st, mode, Ft_mode, V, beta):
    """mu_betadivmin(F, V, unfold(T, mode)) (ntf.py:459-460, ntd.py:672) on the TRANSPOSED problem unfold^T ~ V^T F^T, V = the
    r_mode x prod(other dims) operand of the driver (NTF: the Khatri-Rao product, NTD: the expanded core); returns the new
    transposed factor.  The unfolding is short and fat (I_mode rows), its transpose gives the streaming kernel prod(other
    dims) rows to split over, and the last mode's is a view of T.  Every other mode is updated on the tensor's own layout,
    seen as (extents before) x I_mode x (extents behind), against the same V (nnf_mu_mode_f32, r_mode <= 64): no transposed
    copy of T.  NNF_MU_UNFOLD=1 (read at call time) takes the unfolding for every mode, for A/B runs."""
    eng = st.eng
    if mode == st.nway - 1:
        return eng.mu_right(st.T.view(-1, st.T.shape[mode]), V, Ft_mode, beta)
    if mu_on_layout(eng, Ft_mode.shape[0]):
        return eng.mu_mode(mode_view(st.T, mode), Ft_mode, V, beta)
    return eng.mu_right(st.unfolded_t(mode), V, Ft_mode, beta)

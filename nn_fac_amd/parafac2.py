"""Nonnegative PARAFAC2 with flexible coupling on the MI355X engine -- drop-in for nn_fac/parafac2.py (cited as p2:line).

``parafac_2``, ``compute_parafac_2``, ``one_step_parafac2``, ``compute_P_k`` and ``compute_W_star`` keep the reference's
signatures, return shapes and exceptions (NumPy in -> NumPy out, device tensors in -> device tensors out; the returned D_k
are r x r diagonal matrices).  One extension: the trailing keyword ``alpha`` of compute_parafac_2 / one_step_parafac2, the
wall-clock factor of the sweep rule (nnls.py:156,314) that the reference fixes at 0.5; ``parafac_2(deterministic=True)``
passes math.inf, as nmf and ntd do.

The K slices X_k (m_k x n) are stacked once per run as Xs (sum m_k x n) with a device table of row offsets; the factors live
transposed on the device (Wt: r x sum m_k, Pt: r' x sum m_k, Dt: r x K with d_k in column k).  One step (p2:402-602):
  * the data-sized passes run once on the stacked slices with the tuned streaming kernels: P = H Xs^T (one xht; it serves
    both VMt_k = d_k o P[:, seg k] of the W_k updates and UtM_k[q] = sum_i Wt[q,i] P[q,i] of the D_k updates), the H update's
    UtM = (Wt o d) Xs (one xty) and the per-row residuals (nnf_frob_resid_rows_f32), whose segment sums are the slices' costs;
  * the K rank-sized problems per statement run in ONE launch each (k_group.hip): all W_k solves
    (nnf_hals_solve_group_f32 on the shifted operands UtM + mu_k target, UtU + mu_k I of update_rules/nnls.py), all D_k solves
    (K one-column groups), the Grams W_k^T W_k with the dots and the coupling errors (nnf_group_gram_f32), and
    P_k = A_k S_k^{-1/2} (nnf_group_gemm_f32) -- the polar factor of A_k = W_k W*^T that the reference takes from an SVD per
    slice (p2:605-612), here from one batched fp64 eigh of the r' x r' Grams S_k = A_k^T A_k; a slice whose S_k is singular to
    1e-12 (the random start with init_with_P=False) takes its P_k from torch.linalg.svd in fp64;
  * groups longer than Engine.hals_group_max_columns go through the existing hals_solve one at a time, as do all W_k solves
    with normalize[0] (the row normalisation is per slice).
The mu rule (p2:590-600) runs on the HOST: one device-to-host copy of 3K + 3 doubles per iteration (slice residuals,
coupling errors, sweep counts, the 1-norm of H).

NNF_PARAFAC2_PER_SLICE=1 composes the same step slice by slice from the entry points that existed before the grouped
kernels (hals_solve, gram, frob_resid, torch SVD per slice): the comparison route of the tests and of tools/time_parafac2.py.
``LAST_STEP_INFO`` holds the sweep counts of the last step (cnt_W, cnt_D per slice, cnt_H)."""
import math
import os
import time

import numpy as np
import torch

from . import engine as _engine
from ._convert import device_of
from .update_rules import nnls as _nnls
from .utils import errors as err
from .utils import initialize_factors as init_factors

LAST_STEP_INFO = {}
MAX_COUPLING_ROWS = 128     # rows of W* (columns of the P_k): the grouped product takes p, q <= 128


def _per_slice():
    return os.environ.get("NNF_PARAFAC2_PER_SLICE", "0") not in ("", "0")


# ---- boundary -----------------------------------------------------------------------------------------------
def _is_t(x):
    return isinstance(x, torch.Tensor)


def _shape(x):
    return tuple(int(d) for d in x.shape)


def _check_problem(slices, rank, W_list, H, D_list, W_star, P_list, init_with_P):
    """Everything that can be refused from shapes alone, before the device is touched."""
    rank = int(rank)
    if rank > _engine.MAX_RANK:
        raise err.EngineError(f"parafac2: rank {rank} is above the {_engine.MAX_RANK} the grouped PARAFAC2 kernels of nn_fac_amd "
                              f"are built for")
    K = len(slices)
    if K < 1 or len(W_list) != K or len(D_list) != K:
        raise err.ArgumentException("PARAFAC2 needs one W_k and one D_k per slice.")
    n = _shape(slices[0])[1]
    rows = []
    for k in range(K):
        m, nk = _shape(slices[k])
        if nk != n or _shape(W_list[k]) != (m, rank):
            raise err.ArgumentException(f"Slice {k}: shapes {_shape(slices[k])} / W_k {_shape(W_list[k])} do not fit rank {rank}.")
        rows.append(m)
    if _shape(H) != (rank, n):
        raise err.ArgumentException(f"H is {_shape(H)}, expected {(rank, n)}.")
    rp = None
    if init_with_P and P_list is not None:
        rp = _shape(P_list[0])[1]
        if len(P_list) != K or any(_shape(P_list[k]) != (rows[k], rp) for k in range(K)):
            raise err.ArgumentException("PARAFAC2 needs one P_k of m_k rows per slice, all with the same number of columns.")
    elif not init_with_P and W_star is not None:
        rp = _shape(W_star)[0]
        if _shape(W_star)[1] != rank:
            raise err.ArgumentException(f"W* is {_shape(W_star)}, expected {rank} columns.")
    if rp is not None:
        if rp > MAX_COUPLING_ROWS:
            raise err.EngineError(f"parafac2: W* with {rp} rows is above the {MAX_COUPLING_ROWS} the grouped product is built for")
        if min(rows) < rp:
            raise err.InvalidArgumentValue(f"Every slice needs at least as many rows as W* ({rp}): the P_k have orthonormal "
                                           f"columns (shortest slice: {min(rows)} rows).")
    return rows, n


class _State:
    """The stacked problem on the device."""

    def __init__(self, slices, rank, W_list, H, D_list, W_star, P_list, rows, n):
        self.dev = dev = device_of(*slices, H)
        self.eng = _engine.get_engine(dev)
        self.r, self.K, self.n, self.rows = int(rank), len(slices), n, rows
        self.total = sum(rows)
        self.off_host = [0]
        for m in rows:
            self.off_host.append(self.off_host[-1] + m)
        self.off = torch.tensor(self.off_host, dtype=torch.int64, device=dev)
        self.offK = torch.arange(self.K + 1, dtype=torch.int64, device=dev)
        self.segid = torch.repeat_interleave(torch.arange(self.K, device=dev), torch.tensor(rows, device=dev))
        self.cap = self.eng.hals_group_max_columns(self.r)
        self.maxlen = max(rows)
        self.tensors = _is_t(H)
        self.np_dtype = np.asarray(H).dtype if not _is_t(H) and np.issubdtype(np.asarray(H).dtype, np.floating) else np.float64
        up = self._up
        self.Xs = torch.cat([up(x) for x in slices], dim=0).contiguous()
        self.Wt = torch.cat([up(w) for w in W_list], dim=0).t().contiguous()
        self.H = up(H).clone().contiguous()
        self.Dt = torch.stack([self._diag(D) for D in D_list], dim=1).contiguous()          # r x K
        self.Ws = up(W_star).clone().contiguous() if W_star is not None else None
        self.Pt = torch.cat([up(p) for p in P_list], dim=0).t().contiguous() if P_list is not None else None

    def _up(self, x):
        if _is_t(x):
            return x.to(device=self.dev, dtype=torch.float32)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32)).to(self.dev)

    def _diag(self, D):
        D = self._up(D)
        return torch.diagonal(D).clone() if D.dim() == 2 and D.shape[0] == D.shape[1] else D.reshape(-1).clone()

    def seg(self, k):
        return slice(self.off_host[k], self.off_host[k + 1])

    def mu_cols(self, mu):
        return torch.as_tensor(np.asarray(mu, dtype=np.float32), device=self.dev)[self.segid]

    # ---- results in the caller's kind -------------------------------------------------------------
    def _out(self, t):
        return t if self.tensors else t.detach().cpu().numpy().astype(self.np_dtype, copy=False)

    def rows_list(self, Mt):
        """Mt (c x total) -> the list of its segments transposed back (m_k x c)."""
        full = Mt.t().contiguous()
        if not self.tensors:
            full = self._out(full)
            return [full[self.seg(k)].copy() for k in range(self.K)]
        return [full[self.seg(k)].clone() for k in range(self.K)]

    def W_list(self):
        return self.rows_list(self.Wt)

    def P_list(self):
        return self.rows_list(self.Pt)

    def D_list(self, as_array):
        D = torch.diag_embed(self.Dt.t().contiguous())                                        # K x r x r
        if not self.tensors:
            D = self._out(D)
            return D if as_array else [D[k].copy() for k in range(self.K)]
        return D if as_array else [D[k].clone() for k in range(self.K)]

    def H_out(self):
        return self._out(self.H.clone())

    def Ws_out(self):
        return self._out(self.Ws.clone())


# ---- the pieces of one step -------------------------------------------------------------------------------
def _w_star(st, mu, normalize):
    """p2:614-630: W* = sum_k mu_k P_k^T W_k / sum mu, optionally with unit columns; one product over the stacked rows."""
    Pmu = st.Pt * st.mu_cols(mu)[None, :]
    if _per_slice():
        acc = torch.zeros((st.Pt.shape[0], st.r), dtype=torch.float64, device=st.dev)
        for k in range(st.K):
            acc += st.eng.xht(st.Wt[:, st.seg(k)], Pmu[:, st.seg(k)]).double()
    else:
        acc = st.eng.xht(st.Wt, Pmu).double()                  # (Pt o mu) Wt^T : r' x r
    Ws = acc / float(np.sum(mu))
    if normalize:
        nrm = Ws.norm(dim=0)
        Ws = Ws / torch.where(nrm != 0, nrm, torch.ones_like(nrm))
    return Ws.float().contiguous()


def _polar_svd(A64):
    U, _, Vh = torch.linalg.svd(A64, full_matrices=False)
    return U @ Vh


def _p_k(st):
    """p2:605-612: P_k = U[:, :r'] Vt[:r', :] of svd(W_k W*^T), the polar factor of A_k = W_k W*^T."""
    eng = st.eng
    At = eng.small_gemm(st.Ws, st.Wt)                           # W* Wt : r' x total
    rp = At.shape[0]
    if _per_slice():
        Pt = torch.empty_like(At)
        for k in range(st.K):
            Pt[:, st.seg(k)] = _polar_svd(At[:, st.seg(k)].double().t()).t().float()
        return Pt
    S64 = torch.empty((st.K, rp, rp), dtype=torch.float64, device=st.dev)
    eng.group_gram(At, st.off, out64=S64)
    lam, Q = torch.linalg.eigh(S64)
    bad = ~(lam[:, 0] >= 1e-12 * lam[:, -1]) | ~(lam[:, -1] > 0)
    isq = torch.where(lam > 0, lam, torch.ones_like(lam)).rsqrt()
    Sih = (Q * isq[:, None, :]) @ Q.transpose(1, 2)              # S_k^{-1/2}, symmetric
    Pt = eng.group_gemm(Sih.float().contiguous(), At, st.off, st.maxlen)
    for k in torch.nonzero(bad).flatten().tolist():              # singular S_k: that slice alone, from an SVD in fp64
        Pt[:, st.seg(k)] = _polar_svd(At[:, st.seg(k)].double().t()).t().float()
    return Pt


def _runs(st, lens_ok):
    """Maximal runs [g0, g1) of consecutive groups the grouped solve takes."""
    runs, g = [], 0
    while g < st.K:
        if lens_ok[g]:
            g1 = g
            while g1 < st.K and lens_ok[g1]:
                g1 += 1
            runs.append((g, g1))
            g = g1
        else:
            g += 1
    return runs


def _timed(st, alpha, atime, probe):
    """Sweeps allowed by cnt <= 1 + alpha*rho (nnls.py:156): rho = wall time of the products / wall time of one probe sweep."""
    return _nnls.timed_budget(100, alpha, atime, probe, st.dev)[0]


def _update_W(st, mu, P, Tt, HH64, normalize0, alpha, t0):
    """p2:510-524 for every slice: coupled solves on the shifted operands (update_rules/nnls.py:111-175)."""
    eng, r, K = st.eng, st.r, st.K
    dcol = st.Dt[:, st.segid]
    Ms = torch.addcmul(P * dcol, Tt, st.mu_cols(mu)[None, :].expand_as(Tt))       # d_k o P + mu_k target
    d64 = st.Dt.t().double()                                                       # K x r
    G64 = d64[:, :, None] * d64[:, None, :] * HH64[None]
    diag = torch.diagonal(G64, dim1=1, dim2=2)
    frozen = diag == 0
    diag += torch.as_tensor(np.asarray(mu, dtype=np.float64), device=st.dev)[:, None]
    diag[frozen] = 0.0                                                             # rows the reference skips (nnls.py:316)
    Gs = G64.float().contiguous()
    atime = _nnls.toc(st.dev, t0)
    status = torch.zeros((K, _engine.ST_WORDS), dtype=torch.float64, device=st.dev)
    grouped = [(not _per_slice()) and (not normalize0) and st.rows[k] <= st.cap for k in range(K)]
    runs = _runs(st, grouped)

    def launch(V, sweeps, stt):
        for g0, g1 in runs:
            eng.hals_solve_group(Ms, Gs[g0:g1], V, st.off[g0:g1 + 1], min(st.maxlen, st.cap), sweeps, delta=0.01,
                                 status=stt[g0:g1])
    if runs:
        budget = _timed(st, alpha, atime, lambda: launch(st.Wt.clone(), 1, torch.empty_like(status)))
        launch(st.Wt, budget, status)
    for k in range(K):
        if grouped[k]:
            continue
        sg = st.seg(k)
        Mk, Vk = Ms[:, sg], st.Wt[:, sg]
        budget = _timed(st, alpha, atime, lambda: eng.hals_sweeps(Mk, Gs[k], Vk.clone(), 1, normalize=normalize0))
        eng.hals_solve(Mk, Gs[k], Vk, budget, delta=0.01, normalize=normalize0, status=status[k])
    return status


def _grams(st, P, Tt):
    """Per slice: G_k = W_k^T W_k (fp64 sums), c_k[q] = sum_i Wt[q,i] P[q,i], e_k = ||W_k - P_k W*||_F^2."""
    eng, K, r = st.eng, st.K, st.r
    G64 = torch.empty((K, r, r), dtype=torch.float64, device=st.dev)
    if not _per_slice():
        _, c, e = eng.group_gram(st.Wt, st.off, B=P, T=Tt, out64=G64)
        return G64, c, e
    c = torch.empty((K, r), dtype=torch.float64, device=st.dev) if P is not None else None
    e = torch.empty(K, dtype=torch.float64, device=st.dev)
    for k in range(K):
        sg = st.seg(k)
        eng.gram(st.Wt[:, sg], out64=G64[k])
        if P is not None:
            c[k] = (st.Wt[:, sg].double() * P[:, sg].double()).sum(dim=1)
        e[k] = (st.Wt[:, sg].double() - Tt[:, sg].double()).pow(2).sum()
    return G64, c, e


def _update_D(st, G64, c, HH64, alpha, t0):
    """p2:526-556 for every slice: K one-column solves, UtU_k = (W_k^T W_k) o (H H^T), UtM_k = c_k."""
    eng, K = st.eng, st.K
    UtU = (G64 * HH64[None]).float().contiguous()
    UtM = c.t().float().contiguous()                                               # r x K
    atime = _nnls.toc(st.dev, t0)
    status = torch.zeros((K, _engine.ST_WORDS), dtype=torch.float64, device=st.dev)
    if not _per_slice():
        budget = _timed(st, alpha, atime, lambda: eng.hals_solve_group(UtM, UtU, st.Dt.clone(), st.offK, 1, 1))
        eng.hals_solve_group(UtM, UtU, st.Dt, st.offK, 1, budget, delta=0.01, status=status)
        return status
    for k in range(K):
        Mk, Vk = UtM[:, k:k + 1], st.Dt[:, k:k + 1]
        budget = _timed(st, alpha, atime, lambda: eng.hals_sweeps(Mk, UtU[k], Vk.clone(), 1))
        eng.hals_solve(Mk, UtU[k], Vk, budget, delta=0.01, status=status[k])
    return status


def _slice_sums(st, rows64):
    cs = torch.cumsum(rows64, dim=0)
    cs = torch.cat([torch.zeros(1, dtype=torch.float64, device=st.dev), cs])
    return cs[st.off[1:]] - cs[st.off[:-1]]


def _slice_resid(st, Us):
    """||X_k - W_k D_k H||_F^2 for every slice (K doubles on the device); Us = Wt o d."""
    if not _per_slice():
        return _slice_sums(st, st.eng.frob_resid_rows(st.Xs, Us, st.H))
    out = torch.empty(st.K, dtype=torch.float64, device=st.dev)
    for k in range(st.K):
        st.eng.frob_resid(st.Xs[st.seg(k)], Us[:, st.seg(k)], st.H, out=out[k:k + 1])
    return out


def _scaled_W(st):
    return (st.Wt * st.Dt[:, st.segid]).contiguous()


def _step(st, mu_in, norm_slices, prev_cost, increasing_mu, tol_mu, step_mu, init_with_P, sparsity, fixed_modes, normalize, alpha):
    """One pass of p2:402-602 on the device state; returns (mu, cost, couple_error, increasing_mu, slice residuals)."""
    eng, K, r = st.eng, st.K, st.r
    mu = np.array(mu_in, dtype=np.float64).copy()
    normalize = list(normalize) + [False] * (5 - len(normalize))
    if init_with_P:                                                                # p2:495-507 (the reference's conditions)
        st.Ws = _w_star(st, mu, True)
        if 4 in fixed_modes:
            st.Pt = _p_k(st)
    else:
        st.Pt = _p_k(st)
        if 3 in fixed_modes:
            st.Ws = _w_star(st, mu, normalize[3])
    if st.Ws.shape[1] != r or st.Pt.shape != (st.Ws.shape[0], st.total):
        raise err.ArgumentException(f"W* {tuple(st.Ws.shape)} and the P_k ({st.Pt.shape[0]} columns) do not fit rank {r}.")

    Tt = eng.small_gemm(st.Ws.t().contiguous(), st.Pt)                             # targets (P_k W*)^T : r x total
    HH64 = torch.empty((r, r), dtype=torch.float64, device=st.dev)
    need_P = (0 not in fixed_modes) or (2 not in fixed_modes)
    t0 = _nnls.tic(st.dev, alpha)
    P = eng.xht(st.Xs, st.H) if need_P else None                                   # H Xs^T : r x total
    eng.gram(st.H, out64=HH64)
    stW = stD = stH = None
    if 0 not in fixed_modes:
        stW = _update_W(st, mu, P, Tt, HH64, normalize[0], alpha, t0)
    t0 = _nnls.tic(st.dev, alpha)
    G64, c, e = _grams(st, P if 2 not in fixed_modes else None, Tt)
    if 2 not in fixed_modes:
        stD = _update_D(st, G64, c, HH64, alpha, t0)
    if normalize[2]:                                                               # p2:558-564
        nrm = st.Dt.double().norm(dim=1)
        st.Dt = torch.where(nrm[:, None] == 0, torch.full_like(st.Dt, 1.0 / K ** 2),
                            (st.Dt.double() / torch.where(nrm == 0, torch.ones_like(nrm), nrm)[:, None]).float()).contiguous()
    if 1 not in fixed_modes:                                                       # p2:566-582
        t0 = _nnls.tic(st.dev, alpha)
        Us = _scaled_W(st)
        UtM = eng.xty(st.Xs, Us)
        d64 = st.Dt.t().double()
        UtU = (d64[:, :, None] * d64[:, None, :] * G64).sum(dim=0).float().contiguous()
        atime = _nnls.toc(st.dev, t0)
        budget = _timed(st, alpha, atime,
                         lambda: eng.hals_sweeps(UtM, UtU, st.H.clone(), 1, sparsity=sparsity, normalize=normalize[1]))
        stH = eng.hals_solve(UtM, UtU, st.H, budget, delta=0.01, sparsity=sparsity, normalize=normalize[1])
    else:
        Us = _scaled_W(st)
    resid = _slice_resid(st, Us)

    # ---- the one device-to-host copy of the iteration -------------------------------------------------------
    zK = torch.ones(K, dtype=torch.float64, device=st.dev)
    h1 = st.H.double().abs().sum(dim=0).max().reshape(1)                           # np.linalg.norm(H, ord=1), p2:588
    pack = torch.cat([resid, e,
                      stW[:, _engine.ST_CNT] if stW is not None else zK, stW[:, _engine.ST_ERR] if stW is not None else 0 * zK,
                      stD[:, _engine.ST_CNT] if stD is not None else zK, stD[:, _engine.ST_ERR] if stD is not None else 0 * zK,
                      stH[[_engine.ST_CNT, _engine.ST_ERR]] if stH is not None else torch.tensor([1.0, 0.0], dtype=torch.float64,
                                                                                                 device=st.dev), h1]).cpu().numpy()
    resid_h, e_h = pack[:K], pack[K:2 * K]
    if pack[3 * K:4 * K].any() or pack[5 * K:6 * K].any() or pack[6 * K + 1] != 0:
        raise err.EngineError("parafac2: a HALS solve reported an error status; result invalid")
    LAST_STEP_INFO.clear()
    LAST_STEP_INFO.update(cnt_W=pack[2 * K:3 * K].astype(np.int64), cnt_D=pack[4 * K:5 * K].astype(np.int64),
                          cnt_H=int(pack[6 * K]))
    cost = 0
    if sparsity != None:  # noqa: E711
        cost = sparsity * float(pack[6 * K + 2])
    couple_error = []
    for k in range(K):                                                             # p2:590-600 (cost = the RUNNING sum)
        couple_error.append(math.sqrt(e_h[k]))
        cost += resid_h[k] + (mu[k] * couple_error[k] ** 2) / norm_slices[k]
        if prev_cost != None:  # noqa: E711
            if mu[k] < tol_mu and (prev_cost - cost) > 0 and increasing_mu:
                mu[k] *= step_mu
            elif increasing_mu:
                increasing_mu = False
    return mu, float(cost), couple_error, increasing_mu, resid_h


def _check_init(init_with_P, P_list_in, W_star_in):
    if P_list_in is None and W_star_in is None:
        raise ValueError('The list of P_k and W^* are both to None: one has to be set for the operation.')
    elif init_with_P == True and P_list_in is None:  # noqa: E712
        raise ValueError('PARAFAC2 is set with the init of P_k, but they are set to None.')
    elif init_with_P == False and W_star_in is None:  # noqa: E712
        raise ValueError('PARAFAC2 is set with the init of W^*, but it is set to None.')


# ---- the reference's entry points ---------------------------------------------------------------------------
def parafac_2(tensor_slices, rank, init_with_P, init="random", W_list_in=None, H=None, D_list_in=None, W_star=None, P_list=None,
              tol_mu=1e6, step_mu=1.02, n_iter_max=100, tol=1e-6, sparsity_coefficient=None, fixed_modes=[],
              normalize=[False, False, False, False, False], verbose=False, return_costs=False, deterministic=False, seed=0):
    """Nonnegative PARAFAC2 (p2:18-198; see the reference docstring for the model and the options).  As in the reference,
    this entry hands compute_parafac_2 the default tol_mu / step_mu and no normalisation (p2:196-198)."""
    if deterministic:
        np.random.seed(seed)
    if init.lower() == "custom":
        if W_list_in is None or H is None or D_list_in is None:
            raise err.CustomNotValidFactors("Custom initialization, but (at least) one factor is set to 'None'")
        W_list, D_list = list(W_list_in), D_list_in
    else:
        W_list, H, D_list, P_list, W_star = init_factors.parafac2_initialization(tensor_slices, rank, init, init_with_P,
                                                                                 deterministic=deterministic, seed=seed)
        if _is_t(tensor_slices[0]):                               # device tensors in -> device tensors out
            dev = tensor_slices[0].device
            cv = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)   # noqa: E731
            W_list, H, D_list = [cv(w) for w in W_list], cv(H), cv(D_list)
            P_list = [cv(p) for p in P_list] if P_list is not None else None
            W_star = cv(W_star) if W_star is not None else None
    return compute_parafac_2(tensor_slices, rank, W_list_in=W_list, H_0=H, D_list_in=D_list, init_with_P=init_with_P,
                             W_star_in=W_star, P_list_in=P_list, n_iter_max=n_iter_max, tol=tol,
                             sparsity_coefficient=sparsity_coefficient, fixed_modes=fixed_modes,
                             normalize=[False, False, False, False], verbose=verbose, return_costs=return_costs,
                             alpha=math.inf if deterministic else 0.5)


def compute_parafac_2(tensor_slices, rank, W_list_in, H_0, D_list_in, init_with_P, W_star_in=None, P_list_in=None, tol_mu=1e6,
                      step_mu=1.02, n_iter_max=100, tol=1e-8, sparsity_coefficient=None, fixed_modes=[],
                      normalize=[False, False, False, False, False], verbose=False, return_costs=False, alpha=0.5):
    """p2:202-400 on the device.  Returns (W_list, H, D_list[, cost_fct_vals, toc])."""
    if W_star_in is None and P_list_in is None:
        # (the reference names a class its errors module does not have, p2:322)
        raise err.CustomNotValidFactors("Initialization not valid: W^* and P_list cannot be both None.")
    _check_init(init_with_P, P_list_in, W_star_in)
    rows, n = _check_problem(tensor_slices, rank, W_list_in, H_0, D_list_in, W_star_in, P_list_in, init_with_P)
    st = _State(tensor_slices, rank, W_list_in, H_0, D_list_in, W_star_in, P_list_in, rows, n)
    K = st.K
    cost_fct_vals, toc, couple_error, increasing_mu = [], [], [], True
    tic = time.time()
    # p2:336-340: mu_k = ||X_k - W_k D_k H||^2 / (10 ||W_k||^2), and the slice norms
    resid = _slice_resid(st, _scaled_W(st)).cpu().numpy()
    norm_slices = np.sqrt(_slice_resid(st, torch.zeros_like(st.Wt)).cpu().numpy())
    w2 = _slice_sums(st, st.Wt.double().pow(2).sum(dim=0)).cpu().numpy()
    mu_list = resid / (10 * w2)
    for iteration in range(n_iter_max):
        prev = None if iteration == 0 else cost_fct_vals[-1]
        if iteration == 1:                                                         # p2:350-352: the residuals of the factors
            for k in range(K):                                                     # the last step left (its cost pass)
                mu_list[k] = 0.2 * math.sqrt(resid[k]) / couple_error[k]
        if iteration == 2:
            increasing_mu = True
        mu_list, cost, couple_error, increasing_mu, resid = _step(st, mu_list, norm_slices, prev, increasing_mu, tol_mu, step_mu,
                                                                  init_with_P, sparsity_coefficient, fixed_modes, normalize, alpha)
        toc.append(time.time() - tic)
        cost_fct_vals.append(cost)
        if verbose:
            if iteration == 0:
                print('Normalized cost function value={}'.format(cost))
            else:
                print('Normalized cost function value={}, variation={}.'.format(cost, cost_fct_vals[-2] - cost_fct_vals[-1]))
            for k in range(K):
                print('Couple_error for channel {} = {}'.format(k, couple_error[k]))
        if iteration > 0 and abs(cost_fct_vals[-2] - cost_fct_vals[-1]) < tol:
            if verbose:
                print('Converged in {} iterations.'.format(iteration))
            break
    as_array = isinstance(D_list_in, np.ndarray) or (_is_t(D_list_in) and D_list_in.dim() == 3)
    if return_costs:
        return st.W_list(), st.H_out(), st.D_list(as_array), cost_fct_vals, toc
    return st.W_list(), st.H_out(), st.D_list(as_array)


def one_step_parafac2(slices, rank, W_list_in, H_in, D_list_in, mu_list_in, norm_slices, previous_cost_fct_val, increasing_mu=True,
                      tol_mu=1e6, step_mu=1.02, init_with_P=True, W_star_in=None, P_list_in=None, sparsity_coefficient=None,
                      fixed_modes=[], normalize=[False, False, False, False, False], alpha=0.5):
    """p2:402-602: one pass over all factors.  Returns (W_list, H, D_list, W_star, P_list, mu_list, cost, couple_error,
    increasing_mu)."""
    _check_init(init_with_P, P_list_in, W_star_in)
    rows, n = _check_problem(slices, rank, W_list_in, H_in, D_list_in, W_star_in, P_list_in, init_with_P)
    st = _State(slices, rank, W_list_in, H_in, D_list_in, None if init_with_P else W_star_in,
                P_list_in if init_with_P else None, rows, n)
    ns = np.array([float(v) for v in norm_slices], dtype=np.float64)
    mu_in = np.array([float(v) for v in mu_list_in], dtype=np.float64)
    mu, cost, ce, inc, _ = _step(st, mu_in, ns, previous_cost_fct_val, increasing_mu, tol_mu, step_mu, init_with_P,
                                 sparsity_coefficient, fixed_modes, normalize, alpha)
    as_array = isinstance(D_list_in, np.ndarray) or (_is_t(D_list_in) and D_list_in.dim() == 3)
    return st.W_list(), st.H_out(), st.D_list(as_array), st.Ws_out(), st.P_list(), mu, cost, ce, inc


def compute_P_k(W_list, W_star, nb_channel):
    """p2:605-612: the list of P_k = U[:, :r'] Vt[:r', :] of svd(W_k W*^T)."""
    W_list = list(W_list)[:nb_channel]
    rank = _shape(W_list[0])[1]
    rp = _shape(W_star)[0]
    if rank > _engine.MAX_RANK or rp > MAX_COUPLING_ROWS:
        raise err.EngineError(f"compute_P_k: rank {rank} / {rp} rows of W* are above the 128 the grouped kernels are built for")
    if min(_shape(w)[0] for w in W_list) < rp:
        raise err.InvalidArgumentValue(f"Every W_k needs at least as many rows as W* ({rp}).")
    st = _factor_state(W_list, W_star, None)
    st.Pt = _p_k(st)
    return st.P_list()


def compute_W_star(P_list, W_list, mu_list, nb_channel, normalize=False):
    """p2:614-630: W* = sum_k mu_k P_k^T W_k / sum_k mu_k, optionally with unit columns."""
    W_list, P_list = list(W_list)[:nb_channel], list(P_list)[:nb_channel]
    if _shape(W_list[0])[1] > _engine.MAX_RANK:
        raise err.EngineError("compute_W_star: rank above the 128 the grouped kernels are built for")
    st = _factor_state(W_list, None, P_list)
    mu = np.array([float(v) for v in list(mu_list)[:nb_channel]], dtype=np.float64)
    st.Ws = _w_star(st, mu, normalize)
    return st.Ws_out()


def _factor_state(W_list, W_star, P_list):
    """A state that carries factors only (no data): for the two stand-alone helpers."""
    rank = _shape(W_list[0])[1]
    rows = [_shape(w)[0] for w in W_list]
    proto = W_list[0]
    if _is_t(proto):
        mk = lambda s: torch.zeros(s, dtype=torch.float32, device=proto.device)   # noqa: E731
    else:
        mk = lambda s: np.zeros(s, dtype=np.asarray(proto).dtype)                 # noqa: E731
    slices = [mk((m, 1)) for m in rows]
    return _State(slices, rank, W_list, mk((rank, 1)), [mk((rank, rank)) for _ in rows], W_star, P_list, rows, 1)

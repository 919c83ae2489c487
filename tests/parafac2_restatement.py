"""NumPy fp64 restatement of the reference's nonnegative PARAFAC2 (nn_fac/parafac2.py:202-630, cited as p2:line) and of its
random initialisation (nn_fac/utils/initialize_factors.py:111-137).  TEST INFRASTRUCTURE: the ground truth the device driver
(nn_fac_amd/parafac2.py) is compared with; tools/gen_golden_parafac2.py asserts it equal to the real reference at 1e-10 when
it writes tests/golden/g11_parafac2.npz, tests/test_parafac2_golden.py re-checks it against that fixture.

One addition to the reference's signatures: ``alpha`` (the wall-clock budget factor of the two NNLS solvers, which the
reference fixes at 0.5; math.inf removes the wall clock from the sweep rule) and ``info`` (a dict that receives the sweep
counts of every solve of the step)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import nnfac_oracle as orc  # noqa: E402


def compute_P_k(W_list, W_star, nb_channel):
    """p2:605-612"""
    out = []
    rp = W_star.shape[0]
    for k in range(nb_channel):
        U, _, Vt = np.linalg.svd(W_list[k] @ W_star.T)
        out.append(U[:, 0:rp] @ Vt[0:rp, :])
    return out


def compute_W_star(P_list, W_list, mu_list, nb_channel, normalize=False):
    """p2:614-630"""
    acc = np.zeros((P_list[0].shape[1], W_list[0].shape[1]))
    for k in range(nb_channel):
        acc += mu_list[k] * P_list[k].T @ W_list[k]
    W_star = acc / np.sum(mu_list)
    if normalize:
        for q in range(W_star.shape[1]):
            nrm = np.linalg.norm(W_star[:, q], ord=2)
            if nrm != 0:
                W_star[:, q] /= nrm
    return W_star


def one_step_parafac2(slices, rank, W_list_in, H_in, D_list_in, mu_list_in, norm_slices, previous_cost_fct_val,
                      increasing_mu=True, tol_mu=1e6, step_mu=1.02, init_with_P=True, W_star_in=None, P_list_in=None,
                      sparsity_coefficient=None, fixed_modes=[], normalize=[False, False, False, False, False], alpha=0.5,
                      info=None):
    """p2:402-602"""
    W_list = list(W_list_in)
    D_list = np.array(D_list_in).copy() if isinstance(D_list_in, np.ndarray) else list(D_list_in)
    H = H_in.copy()
    mu_list = np.array(mu_list_in, dtype=np.float64).copy()
    cost = 0
    K = len(W_list)
    if P_list_in is None and W_star_in is None:
        raise ValueError('The list of P_k and W^* are both to None: one has to be set for the operation.')
    elif init_with_P == True and P_list_in is None:  # noqa: E712
        raise ValueError('PARAFAC2 is set with the init of P_k, but they are set to None.')
    elif init_with_P == False and W_star_in is None:  # noqa: E712
        raise ValueError('PARAFAC2 is set with the init of W^*, but it is set to None.')
    if init_with_P:                                                                     # p2:495-507
        P_list = list(P_list_in)
        W_star = compute_W_star(P_list, W_list, mu_list, K, normalize=True)
        if 4 in fixed_modes:
            P_list = compute_P_k(W_list, W_star, K)
    else:
        W_star = W_star_in
        P_list = compute_P_k(W_list, W_star, K)
        if 3 in fixed_modes:
            W_star = compute_W_star(P_list, W_list, mu_list, K, normalize=normalize[3])
    cnt_W, cnt_D, cnt_H = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64), 0
    for k in range(K):
        if 0 not in fixed_modes:                                                        # p2:510-524
            DkH = D_list[k] @ H
            VVt = DkH @ DkH.T
            VMt = DkH @ slices[k].T
            Wt, _, cnt_W[k], _ = orc.hals_coupling_nnls_acc(VMt, VVt, W_list[k].T, (P_list[k] @ W_star).T, mu_list[k], maxiter=100,
                                                            atime=None, alpha=alpha, delta=0.01, normalize=normalize[0],
                                                            nonzero=False)
            W_list[k] = Wt.T
        if 2 not in fixed_modes:                                                        # p2:526-556
            Wk = W_list[k]
            UtU = (Wk.T @ Wk) * (H @ H.T)
            UtM = np.sum((Wk.T @ slices[k]) * H, axis=1).reshape(-1, 1)
            d = np.diagonal(D_list[k]).reshape(-1, 1)
            dn, _, cnt_D[k], _ = orc.hals_nnls_acc(UtM, UtU, d, maxiter=100, atime=None, alpha=alpha, delta=0.01,
                                                   sparsity_coefficient=None, normalize=False, nonzero=False)
            D_list[k] = np.diag(dn.flatten())
    if normalize[2]:                                                                    # p2:558-564 (D_list a 3-way array)
        D_list = np.array(D_list)
        for q in range(rank):
            nrm = np.linalg.norm(D_list[:, q], ord='fro')
            if nrm == 0:
                D_list[:, q, q] = [1 / (K ** 2) for _ in range(K)]
            else:
                D_list[:, q] /= nrm
    if 1 not in fixed_modes:                                                            # p2:566-582
        UtU = np.zeros((rank, rank))
        UtM = np.zeros((rank, slices[0].shape[1]))
        for k in range(K):
            WkDk = W_list[k] @ D_list[k]
            UtU += WkDk.T @ WkDk
            UtM += WkDk.T @ slices[k]
        H, _, cnt_H, _ = orc.hals_nnls_acc(UtM, UtU, H, maxiter=100, atime=None, alpha=alpha, delta=0.01,
                                           sparsity_coefficient=sparsity_coefficient, normalize=normalize[1], nonzero=False)
    couple_error = []
    if sparsity_coefficient != None:  # noqa: E711                                      # p2:587-588
        cost = sparsity_coefficient * np.linalg.norm(H, ord=1)
    for k in range(K):                                                                  # p2:590-600
        couple_error.append(np.linalg.norm(W_list[k] - P_list[k] @ W_star, ord='fro'))
        cost += np.linalg.norm(slices[k] - W_list[k] @ D_list[k] @ H) ** 2 + (mu_list[k] * couple_error[k] ** 2) / norm_slices[k]
        if previous_cost_fct_val != None:  # noqa: E711
            if mu_list[k] < tol_mu and (previous_cost_fct_val - cost) > 0 and increasing_mu:
                mu_list[k] *= step_mu
            elif increasing_mu:
                increasing_mu = False
    if info is not None:
        info.update(cnt_W=cnt_W, cnt_D=cnt_D, cnt_H=int(cnt_H))
    return W_list, H, D_list, W_star, P_list, mu_list, cost, couple_error, increasing_mu


def compute_parafac_2(tensor_slices, rank, W_list_in, H_0, D_list_in, init_with_P, W_star_in=None, P_list_in=None, tol_mu=1e6,
                      step_mu=1.02, n_iter_max=100, tol=1e-8, sparsity_coefficient=None, fixed_modes=[],
                      normalize=[False, False, False, False, False], verbose=False, return_costs=False, alpha=0.5, trace=None):
    """p2:202-400.  ``trace`` (a list) receives, per iteration, a dict with the step's mu, couple errors, flag and counts."""
    K = len(tensor_slices)
    W_list, H, D_list = list(W_list_in), H_0.copy(), D_list_in.copy()
    W_star = None if W_star_in is None else W_star_in.copy()
    P_list = None if P_list_in is None else list(P_list_in)
    if W_star is None and P_list is None:
        raise orc.ArgumentException("Initialization not valid: W^* and P_list cannot be both None.")
    costs, norm_slices, couple_error, increasing_mu = [], [], [], True
    mu_list = np.zeros(K)
    for k in range(K):                                                                  # p2:336-340
        mu_list[k] = (np.linalg.norm(tensor_slices[k] - (W_list[k] @ D_list[k] @ H), ord='fro') ** 2) / \
            (10 * np.linalg.norm(W_list[k], ord='fro') ** 2)
        norm_slices.append(np.linalg.norm(tensor_slices[k], ord='fro'))
    for it in range(n_iter_max):
        prev = None if it == 0 else costs[-1]
        if it == 1:                                                                     # p2:350-352
            for k in range(K):
                mu_list[k] = 0.2 * np.linalg.norm(tensor_slices[k] - W_list[k] @ D_list[k] @ H, ord='fro') / couple_error[k]
        if it == 2:
            increasing_mu = True
        info = {}
        W_list, H, D_list, W_star, P_list, mu_list, cost, couple_error, increasing_mu = one_step_parafac2(
            tensor_slices, rank, W_list, H, D_list, mu_list, norm_slices, prev, increasing_mu=increasing_mu, tol_mu=tol_mu,
            step_mu=step_mu, init_with_P=init_with_P, P_list_in=P_list, W_star_in=W_star, sparsity_coefficient=sparsity_coefficient,
            fixed_modes=fixed_modes, normalize=normalize, alpha=alpha, info=info)
        costs.append(cost)
        if trace is not None:
            info.update(mu=np.array(mu_list), couple_error=np.array(couple_error), increasing_mu=bool(increasing_mu))
            trace.append(info)
        if it > 0 and abs(costs[-2] - costs[-1]) < tol:
            break
    if return_costs:
        return W_list, np.array(H), D_list, costs, W_star, P_list
    return W_list, np.array(H), D_list


def parafac2_initialization(tensor_slices, rank, init_type, init_with_P, deterministic=False, seed=0):
    """initialize_factors.py:111-137 ('random' only; the reference's 'nndsvd' branch returns nothing)."""
    K = len(tensor_slices)
    r, n = tensor_slices[0].shape
    if deterministic:
        np.random.seed(seed)
    if init_type.lower() != "random":
        raise NotImplementedError(init_type)
    H = np.random.rand(rank, n)
    W_list, D_list = [], []
    for k in range(K):
        W_list.append(np.random.rand(tensor_slices[k].shape[0], rank))
        D_list.append(np.diag(np.random.rand(rank)))
    D_list = np.array(D_list)
    if init_with_P:
        P_list = [np.identity(tensor_slices[k].shape[0])[:, 0:rank] for k in range(K)]
        W_star = None
    else:
        W_star = np.random.rand(r, rank)
        P_list = None
    return W_list, H, D_list, P_list, W_star

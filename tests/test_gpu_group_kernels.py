"""The grouped kernels (k_group.hip: nnf_hals_solve_group_f32, nnf_group_gram_f32, nnf_group_gemm_f32,
nnf_frob_resid_rows_f32) against fp64 NumPy per group.  Needs a MI355X.

Solve tolerance: the one the single solves carry against g1 / g8 (test_gpu_kernels.py): factor rel <= 2e-4, eps within 2e-3
relative, sweep count EQUAL.  The inputs are chosen (and asserted, on the fp64 restatement alone) so that eps/(delta*eps0) is
at least 1e-3 away from 1 at the stopping sweep and at the one before it: no case is excused from the count comparison."""
import math

import numpy as np
import pytest
import torch

import nnfac_oracle as orc

pytestmark = pytest.mark.gpu

RANKS = [1, 3, 16, 17, 32, 33, 50, 64, 65, 128]
CAP = 8192          # NNF_HALS_GROUP_MAX_COLUMNS (asserted against the query entry below)


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    assert torch.cuda.is_available()
    return get_engine("cuda:0")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def odd(a, pad=5):
    """The same matrix at a pitch padded by `pad` floats in a buffer that starts 7 floats off an allocation (NaN around it)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    r, c = a.shape
    ld = c + pad
    buf = torch.full((r * ld + 7,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[7:7 + r * ld].view(r, ld)[:, :c]
    view.copy_(torch.from_numpy(a))
    return view


def odd_stack(G, pad=3):
    G = np.ascontiguousarray(G, dtype=np.float32)
    K, r, c = G.shape
    buf = torch.full((K, r + 2, c + pad), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[:, :r, :c]
    view.copy_(torch.from_numpy(G))
    return view


def offsets(lens):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, torch.from_numpy(off).cuda()


def group_problem(r, n, seed, zero_diag=None, zero_cross=False, fast=False):
    """One group: the Gram of 3r + 5 uniform rows (ill-conditioned: many sweeps) or, `fast`, of 8r centred rows (few sweeps: the
    groups of cap columns at the large ranks), and the matching cross matrix; float32 values (what the device sees)."""
    rng = np.random.RandomState(seed)
    U = rng.randn(8 * r, r) if fast else rng.rand(3 * r + 5, r)
    W = np.maximum(rng.rand(r, n) - 0.3, 0.0) if fast else rng.rand(r, n)
    G = (U.T @ U).astype(np.float32)
    M = (U.T @ (U @ W + 0.05 * rng.rand(U.shape[0], n))).astype(np.float32)
    V = rng.rand(r, n).astype(np.float32)
    if zero_diag is not None:
        G[zero_diag % r, zero_diag % r] = 0.0
    if zero_cross:
        M[:], V[:] = 0.0, 0.0
    return G, M, V


def group_reference(G, M, V, budget, delta=0.01):
    """fp64 restatement of one group; None when its stopping rule comes within 1e-3 of a flip at one of its last two sweeps."""
    log = []
    Vg, e, c, _ = orc.hals_nnls_acc(M.astype(np.float64), G.astype(np.float64), V.astype(np.float64), maxiter=budget,
                                    alpha=math.inf, delta=delta, sweep_log=log)
    for s in log[-2:]:
        if delta * log[0] > 0 and abs(s / (delta * log[0]) - 1.0) < 1e-3:       # (delta = 0 never stops: no flip)
            return None
    return Vg, e, c


_REF = {}


def solve_case(key, r, lens, seed, budget, delta=0.01, **kw):
    """Inputs and their fp64 answers, once per key.  Group g is drawn from the first of the seeds 1000 seed + g, + 500000, ...
    whose restatement keeps the margin (decided by the restatement alone, never by the device's result)."""
    if key not in _REF:
        total = int(np.sum(lens))
        G = np.empty((len(lens), r, r), dtype=np.float32)
        M, V, want = np.empty((r, total), dtype=np.float32), np.empty((r, total), dtype=np.float32), np.empty((r, total))
        eps, cnt, c0 = [], [], 0
        for g, n in enumerate(lens):
            for s in range(1000 * seed + g, 1000 * seed + g + 20 * 500000, 500000):
                Gg, Mg, Vg = group_problem(r, n, s, **kw)
                ref = group_reference(Gg, Mg, Vg, budget, delta)
                if ref is not None:
                    break
            else:
                raise AssertionError(("no seed with a margin", key, g))
            G[g], M[:, c0:c0 + n], V[:, c0:c0 + n], want[:, c0:c0 + n] = Gg, Mg, Vg, ref[0]
            eps.append(ref[1]), cnt.append(ref[2])
            c0 += n
        _REF[key] = (G, M, V, want, np.array(eps, dtype=np.float64), np.array(cnt))
    return _REF[key]


def check_solve(eng, key, r, lens, seed, budget, frozen_row=None, **kw):
    off, offd = offsets(lens)
    G, M, V, want, eps, cnt = solve_case(key, r, lens, seed, budget, **kw)
    Vd, Md, Gd = odd(V), odd(M, pad=9), odd_stack(G)
    st = eng.hals_solve_group(Md, Gd, Vd, offd, int(max(lens)), budget).cpu().numpy()
    got = Vd.cpu().numpy()
    bad = []
    for g, n in enumerate(lens):
        sl = slice(off[g], off[g + 1])
        e = rel(got[:, sl], want[:, sl]) if np.linalg.norm(want[:, sl]) > 0 else float(np.abs(got[:, sl]).max(initial=0.0))
        print(f"group {g} len {n}: rel {e:.2e} cnt {int(st[g, 1])}/{cnt[g]} eps {st[g, 0]:.6e}/{float(eps[g]):.6e}")
        # eps is a sum of r*n squared fp32 steps, each rounded at half an ulp of an entry of V or more: below that floor
        # (a sweep that only moves last bits -- rank 1 after its first sweep) it is rounding, not a figure to compare
        floor = 1e-12 + r * n * (2.0 ** -23 * max(1.0, float(np.abs(want[:, sl]).max(initial=0.0)))) ** 2
        if int(st[g, 1]) != cnt[g] or e > 2e-4 or abs(st[g, 0] - eps[g]) > 2e-3 * abs(eps[g]) + floor or st[g, 3] != 0:
            bad.append((g, n, int(st[g, 1]), int(cnt[g]), e, st[g, 0], float(eps[g]), st[g, 3]))
    assert not bad, bad
    if frozen_row is not None:
        assert np.array_equal(got[frozen_row], V[frozen_row])
    return got, st


def mixed_lens():
    return [1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, CAP - 1, CAP]


def test_cap_query(eng):
    assert eng.hals_group_max_columns(1) == CAP and eng.hals_group_max_columns(128) == CAP


@pytest.mark.parametrize("r", RANKS)
def test_grouped_solve_mixed_lengths(eng, r):
    """Every tile path (one column, below / at / above one tile, many tiles, cap - 1 and cap) in one launch."""
    check_solve(eng, ("mixed", r), r, mixed_lens(), 100 + r, 100, fast=r >= 64)


@pytest.mark.parametrize("r", [3, 17, 128])
def test_grouped_solve_is_deterministic(eng, r):
    lens = [1, 65, 257, 700]
    G, M, V = solve_case(("det", r), r, lens, 200 + r, 100)[:3]
    _, offd = offsets(lens)
    outs = []
    for _ in range(2):
        Vd = dev(V)
        st = eng.hals_solve_group(dev(M), dev(G), Vd, offd, max(lens), 100)
        outs.append((Vd.cpu().numpy(), st.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1][:, :4], outs[1][1][:, :4])


@pytest.mark.parametrize("r", [3, 16, 50])
def test_grouped_solve_300_groups(eng, r):
    """More groups than compute units, ragged, with one-column groups among them."""
    lens = list(np.random.RandomState(r).randint(1, 41, size=300))
    check_solve(eng, ("many", r), r, lens, 300 + r, 100)


@pytest.mark.parametrize("r", [1, 17, 128])
def test_grouped_solve_one_column_groups(eng, r):
    """K one-column problems in one launch (the D_k updates of PARAFAC2)."""
    lens = [1] * (300 if r < 128 else 60)
    check_solve(eng, ("ones", r), r, lens, 400 + r, 100)


def test_grouped_solve_single_group(eng):
    lens = [130]
    check_solve(eng, ("single", 17), 17, lens, 501, 100)


@pytest.mark.parametrize("budget", [1, 2])
def test_grouped_solve_budgets(eng, budget):
    lens = [1, 64, 129, 300]
    _, st = check_solve(eng, ("budget", budget), 16, lens, 600, budget)
    assert (st[:, 1] == budget + 1).all()


def test_grouped_solve_zero_diagonal_row_stays_untouched(eng):
    lens = [1, 65, 300]
    check_solve(eng, ("zerodiag", 17), 17, lens, 700, 100, frozen_row=4, zero_diag=4)


def test_grouped_solve_all_zero_cross_runs_to_the_budget(eng):
    lens = [1, 65, 300]
    _, st = check_solve(eng, ("zerocross", 16), 16, lens, 800, 7, zero_cross=True)
    assert (st[:, 1] == 8).all() and (st[:, 0] == 0).all()


def test_grouped_solve_refusals_leave_the_outputs_untouched(eng):
    from nn_fac_amd.utils.errors import EngineError
    lens = [5, 9]
    _, offd = offsets(lens)
    for r, maxlen in ((4, CAP + 1), (129, 9)):
        G, M, V = solve_case(("refuse", r), r, lens, 900 + r, 10)[:3]
        Vd = dev(V)
        st = torch.full((2, 8), -7.0, dtype=torch.float64, device="cuda")
        with pytest.raises(EngineError):
            eng.hals_solve_group(dev(M), dev(G), Vd, offd, maxlen, 10, status=st)
        assert np.array_equal(Vd.cpu().numpy(), V) and (st.cpu().numpy() == -7.0).all()
    # a group longer than the caller declared: that group is skipped whole and says so, the others are solved
    G, M, V = solve_case(("short", 4), 4, lens, 950, 10)[:3]
    Vd = dev(V)
    st = eng.hals_solve_group(dev(M), dev(G), Vd, offd, 5, 10).cpu().numpy()
    got = Vd.cpu().numpy()
    assert st[0, 3] == 0 and st[1, 3] == 5 and np.array_equal(got[:, 5:], V[:, 5:]) and not np.array_equal(got[:, :5], V[:, :5])


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("shape", ["mixed", "many", "single"])
def test_group_gram_dots_error(eng, r, shape):
    rng = np.random.RandomState(1000 + r)
    lens = {"mixed": mixed_lens(), "many": list(rng.randint(1, 41, size=300)), "single": [77]}[shape]
    off, offd = offsets(lens)
    total = int(off[-1])
    A, B, T = (rng.rand(r, total).astype(np.float32) for _ in range(3))
    T = (A + 0.1 * T).astype(np.float32)
    G64 = torch.empty((len(lens), r, r), dtype=torch.float64, device="cuda")
    G, c, e = eng.group_gram(odd(A), offd, B=odd(B, pad=2), T=odd(T, pad=11), out64=G64)
    G2, c2, e2 = eng.group_gram(dev(A), offd, B=dev(B), T=dev(T))
    assert torch.equal(G, G2) and torch.equal(c, c2) and torch.equal(e, e2)          # pitch-independent and deterministic
    G, c, e, G64 = G.cpu().numpy(), c.cpu().numpy(), e.cpu().numpy(), G64.cpu().numpy()
    assert np.array_equal(G64.astype(np.float32), G)
    A64, B64, T64 = A.astype(np.float64), B.astype(np.float64), T.astype(np.float64)
    for g in range(len(lens)):
        sl = slice(off[g], off[g + 1])
        assert rel(G[g], A64[:, sl] @ A64[:, sl].T) < 1e-5
        assert rel(G64[g], A64[:, sl] @ A64[:, sl].T) < 1e-12
        assert rel(c[g], np.sum(A64[:, sl] * B64[:, sl], axis=1)) < 1e-12
        want = np.sum((A64[:, sl] - T64[:, sl]) ** 2)
        assert abs(e[g] - want) <= 1e-12 * want
    # dots / error alone (no Gram)
    _, c3, e3 = eng.group_gram(dev(A), offd, B=dev(B), T=dev(T), gram=False)
    assert np.array_equal(c3.cpu().numpy(), c) and np.array_equal(e3.cpu().numpy(), e)


@pytest.mark.parametrize("p,q", [(1, 1), (5, 17), (17, 6), (50, 50), (64, 65), (128, 128)])
@pytest.mark.parametrize("shape", ["mixed", "many", "single"])
def test_group_gemm(eng, p, q, shape):
    rng = np.random.RandomState(2000 + p + q)
    lens = {"mixed": mixed_lens(), "many": list(rng.randint(1, 41, size=300)), "single": [77]}[shape]
    off, offd = offsets(lens)
    total = int(off[-1])
    M = (rng.rand(len(lens), p, q) - 0.3).astype(np.float32)
    A = rng.rand(q, total).astype(np.float32)
    out = odd(np.zeros((p, total)), pad=6)
    eng.group_gemm(odd_stack(M), odd(A), offd, max(lens), out=out)
    again = eng.group_gemm(dev(M), dev(A), offd, 1)              # (the bound sizes the launch only)
    assert torch.equal(out, again)
    got = out.cpu().numpy()
    for g in range(len(lens)):
        sl = slice(off[g], off[g + 1])
        assert rel(got[:, sl], M[g].astype(np.float64) @ A[:, sl].astype(np.float64)) < 1e-5


def test_group_gemm_and_gram_refuse_rank_129(eng):
    from nn_fac_amd.utils.errors import EngineError
    _, offd = offsets([4, 4])
    A = torch.rand((129, 8), device="cuda")
    out = torch.full((3, 8), -7.0, device="cuda")
    with pytest.raises(EngineError):
        eng.group_gemm(torch.rand((2, 3, 129), device="cuda"), A, offd, 4, out=out)
    assert (out == -7.0).all()
    with pytest.raises(EngineError):
        eng.group_gram(A, offd)
    with pytest.raises(EngineError):
        eng.frob_resid_rows(torch.rand((8, 5), device="cuda"), A, torch.rand((129, 5), device="cuda"))


@pytest.mark.parametrize("m,n,r", [(1, 1, 1), (17, 15, 3), (300, 70, 6), (294, 33, 17), (1000, 260, 50), (513, 130, 64),
                                   (130, 257, 65), (777, 100, 128)])
def test_frob_resid_rows(eng, m, n, r):
    rng = np.random.RandomState(m + 3 * n + 7 * r)
    Ut, V = rng.rand(r, m).astype(np.float32), rng.rand(r, n).astype(np.float32)
    X = (Ut.T.astype(np.float64) @ V * (1 + 0.1 * rng.randn(m, n))).astype(np.float32)
    rows = eng.frob_resid_rows(odd(X), odd(Ut, pad=3), odd(V, pad=1))
    assert torch.equal(rows, eng.frob_resid_rows(dev(X), dev(Ut), dev(V)))
    rows = rows.cpu().numpy()
    want = np.sum((X.astype(np.float64) - Ut.T.astype(np.float64) @ V.astype(np.float64)) ** 2, axis=1)
    lens = [m] if m < 8 else [1, m // 3, m - 1 - m // 3]
    off, _ = offsets(lens)
    for g in range(len(lens)):
        sl = slice(off[g], off[g + 1])
        assert abs(rows[sl].sum() - want[sl].sum()) <= 1e-5 * want[sl].sum()
    total = float(eng.frob_resid(dev(X), dev(Ut), dev(V)))
    assert abs(rows.sum() - total) <= 1e-5 * total

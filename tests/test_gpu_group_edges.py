"""The grouped kernels (k_group.hip) at the edges test_gpu_group_kernels.py leaves out, against fp64 NumPy on the fp32-rounded
inputs.  Needs a MI355X.

1. nnf_frob_resid_rows_f32 row by row.  With u = 2^-24, rho the fp64 residual and e_ij = (r + 2) u ((|Ut|^T |V|)_ij + |X_ij|)
   (an fp32 FMA chain of length r plus the subtraction), every row must satisfy
   |rows[i] - want[i]| <= sum_j (2 |rho_ij| e_ij + e_ij^2).  The bound is derived, not tuned; each case prints the worst
   achieved fraction of it.  Worst over all cases, measured on an MI355X: 0.157 of the bound (m 31, n 1, r 2, noisy data: one
   entry per row, nothing averages); at r = 127 / 128 on the fit exact to rounding it is below 0.001.
2. Segment tables the kernels must not trust, 3. empty groups, 4. the length boundary of the resident tile, 5. the call shape of
   the PARAFAC2 driver (sub-runs of a table, full-width operands) and the independence of the groups, 6. the stopping rule at
   other deltas and at max_sweeps = 0, 7. every refusal the four entries name, through the C ABI.

Bitwise comparisons go through the integer image of the buffers (NaN margins and sentinels included)."""
import math

import numpy as np
import pytest
import torch

import nnfac_oracle as orc
from test_gpu_group_kernels import (check_solve, group_problem, group_reference, odd, odd_stack, offsets,  # noqa: F401
                                    rel, solve_case)

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = -1, -3          # NNF_ERR_ARG, NNF_ERR_UNSUPPORTED (include/nnfac_hip.h)
CAP = 8192
MARGIN = 16                        # floats around every row of a framed operand
SENT = -7.0


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    assert torch.cuda.is_available()
    return get_engine("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def bits(t):
    """The integer image of a tensor (host): NaNs and signed zeros compare as what they are."""
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(a, b)


def framed(a, fill=float("nan")):
    """`a` as a view into a larger allocation: MARGIN floats of `fill` before the first and after the last column of EVERY
    row.  Returns (allocation, view)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.shape[0], a.shape[1] + 2 * MARGIN), fill, dtype=torch.float32, device="cuda")
    view = buf[:, MARGIN:MARGIN + a.shape[1]]
    view.copy_(torch.from_numpy(a))
    return buf, view


def ld(t):
    from nn_fac_amd.engine import _ld
    return int(_ld(t))


def table(off):
    off = np.asarray(off, dtype=np.int64)
    return off, torch.from_numpy(off).cuda()


def cols(off, g):
    """Columns of group g inside a framed allocation."""
    return slice(MARGIN + int(off[g]), MARGIN + int(off[g + 1]))


# ------------------------------------------------------------------------------------------------------------------
# launches that own every output buffer (sentinel -7 where nothing may be written), through the C entries
# ------------------------------------------------------------------------------------------------------------------
def solve_problem(r, lens, seed):
    total = int(np.sum(lens))
    G = np.empty((len(lens), r, r), dtype=np.float32)
    M, V = np.empty((r, total), dtype=np.float32), np.empty((r, total), dtype=np.float32)
    c0 = 0
    for g, n in enumerate(lens):
        G[g], M[:, c0:c0 + n], V[:, c0:c0 + n] = group_problem(r, int(n), seed + g)
        c0 += n
    return G, M, V


def run_solve(eng, prob, off, maxlen, budget, delta=0.01):
    """One launch on framed operands with an untrusted table.  Returns the integer images of V's whole allocation before and
    after, and the status blocks (pre-filled with -7)."""
    G, M, V = prob
    r, total = V.shape
    off, offd = table(off)
    ng = len(off) - 1
    _, Mv = framed(M)
    Vb, Vv = framed(V)
    Gv = odd_stack(G[:ng]) if ng <= G.shape[0] else None
    before = bits(Vb)
    st = torch.full((ng, 8), SENT, dtype=torch.float64, device="cuda")
    code = eng.lib.nnf_hals_solve_group_f32(eng.ctx, Mv.data_ptr(), ld(Mv), Gv.data_ptr(), Gv.stride(1), Gv.stride(0),
                                            Vv.data_ptr(), ld(Vv), r, offd.data_ptr(), ng, int(maxlen), total, int(budget),
                                            float(delta), st.data_ptr(), eng._stream())
    assert code == 0, code
    return {"V0": before, "V": bits(Vb), "st": st.cpu().numpy()}


def gram_problem(r, total, seed):
    rng = np.random.RandomState(seed)
    A, B, T = (rng.rand(r, total).astype(np.float32) for _ in range(3))
    return A, B, (A + 0.1 * T).astype(np.float32)


def run_gram(eng, prob, off, ldg=None, gstride=None):
    """G, G64, dots and err of one launch, all requested, all pre-filled with -7 (G: NaN when the caller's pitch is wider than
    r, returned as the whole allocation)."""
    A, B, T = prob
    r, total = A.shape
    off, offd = table(off)
    ng = len(off) - 1
    views = [framed(x)[1] for x in (A, B, T)]
    Av, Bv, Tv = views
    packed = ldg is None
    ldg, gstride = (r, r * r) if packed else (ldg, gstride)
    G = torch.full((ng * gstride + 8,), SENT if packed else float("nan"), dtype=torch.float32, device="cuda")
    G64 = torch.full((ng, r, r), SENT, dtype=torch.float64, device="cuda")
    dots = torch.full((ng, r), SENT, dtype=torch.float64, device="cuda")
    err = torch.full((ng,), SENT, dtype=torch.float64, device="cuda")
    code = eng.lib.nnf_group_gram_f32(eng.ctx, Av.data_ptr(), ld(Av), r, offd.data_ptr(), ng, total, G.data_ptr(), ldg, gstride,
                                      G64.data_ptr(), Bv.data_ptr(), ld(Bv), dots.data_ptr(), Tv.data_ptr(), ld(Tv),
                                      err.data_ptr(), eng._stream())
    assert code == 0, code
    out = {"G64": bits(G64), "dots": bits(dots), "err": bits(err), "Graw": bits(G)}
    if packed:
        assert (out["Graw"][ng * r * r:] == SENT32).all()
        out["G"] = out["Graw"][:ng * r * r].reshape(ng, r, r)
    return out


def gemm_problem(p, q, ng, total, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(ng, p, q) - 0.3).astype(np.float32), rng.rand(q, total).astype(np.float32)


def run_gemm(eng, prob, off, maxlen):
    """The whole allocation of `out` (pre-filled with -7, NaN margins) after one launch."""
    M, A = prob
    ng_all, p, q = M.shape
    total = A.shape[1]
    off, offd = table(off)
    ng = len(off) - 1
    _, Av = framed(A)
    Ob, Ov = framed(np.full((p, total), SENT))
    Mv = odd_stack(M[:ng])
    code = eng.lib.nnf_group_gemm_f32(eng.ctx, Mv.data_ptr(), Mv.stride(1), Mv.stride(0), p, q, Av.data_ptr(), ld(Av),
                                      offd.data_ptr(), ng, int(maxlen), total, Ov.data_ptr(), ld(Ov), eng._stream())
    assert code == 0, code
    return {"out": bits(Ob)}


SENT32, SENT64 = np.float32(SENT).view(np.uint32), np.float64(SENT).view(np.uint64)       # the images of the sentinel
NAN32 = np.uint32(0x7FC00000)                                                          # ... and of torch's NaN fill


# ------------------------------------------------------------------------------------------------------------------
# 1. per-row residuals, row by row
# ------------------------------------------------------------------------------------------------------------------
RES_M = [1, 15, 16, 17, 31, 33, 100]
RES_N = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 130]
RES_R = [1, 2, 3, 4, 5, 7, 8, 17, 127, 128]


def resid_shapes():
    """A pruned product: the three axes walked at their own periods (every value of each axis appears), and the cases where
    the 16-row, 16-column and rank-4 edges meet."""
    met = [(16, 16, 4), (15, 15, 3), (17, 17, 5), (16, 64, 8), (17, 65, 7), (31, 63, 127), (33, 49, 128), (100, 130, 128),
           (100, 130, 127), (1, 1, 1)]
    walk = [(RES_M[i % 7], RES_N[i % 11], RES_R[i % 10]) for i in range(33)]
    out = []
    for s in met + walk:
        if s not in out:
            out.append(s)
    return out


def test_resid_shapes_cover_every_axis_value():
    sh = resid_shapes()
    assert {s[0] for s in sh} == set(RES_M) and {s[1] for s in sh} == set(RES_N) and {s[2] for s in sh} == set(RES_R)
    assert 38 <= len(sh) <= 45


@pytest.mark.parametrize("m,n,r", resid_shapes())
def test_frob_resid_rows_row_by_row(eng, m, n, r):
    """Every row against fp64 within the derived fp32 bound (module docstring), on noisy data and on a fit exact to rounding
    (where a lost or misplaced rank step is hundreds of bounds away); nothing written past row m; two calls and two pitches
    bitwise equal."""
    rng = np.random.RandomState(m + 131 * n + 17 * r)
    u = 2.0 ** -24
    Ut = (rng.rand(r, m) * np.sqrt(1.0 + np.arange(m))).astype(np.float32)       # row i of the factor scaled by sqrt(1 + i)
    V = rng.rand(r, n).astype(np.float32)
    P = Ut.T.astype(np.float64) @ V.astype(np.float64)
    worst = 0.0
    for form in ("noisy", "exact"):
        X = (P * (1.0 + 0.1 * rng.randn(m, n))).astype(np.float32) if form == "noisy" else P.astype(np.float32)
        rho = X.astype(np.float64) - P
        want = np.sum(rho ** 2, axis=1)
        e = (r + 2) * u * (np.abs(Ut).T.astype(np.float64) @ np.abs(V).astype(np.float64) + np.abs(X).astype(np.float64))
        bound = np.sum(2.0 * np.abs(rho) * e + e * e, axis=1)
        outs = []
        for Xd, Ud, Vd in ((dev(X), dev(Ut), dev(V)), (odd(X), odd(Ut, pad=3), odd(V, pad=1)), (dev(X), dev(Ut), dev(V))):
            out = torch.full((m + 16,), SENT, dtype=torch.float64, device="cuda")
            eng.frob_resid_rows(Xd, Ud, Vd, out=out)
            outs.append(out.cpu().numpy())
        assert same(outs[0].view(np.uint64), outs[2].view(np.uint64)), "two calls differ"
        assert same(outs[0].view(np.uint64), outs[1].view(np.uint64)), "padded and contiguous operands differ"
        assert (outs[0][m:] == SENT).all()
        ratio = np.abs(outs[0][:m] - want) / bound
        print(f"resid rows m {m} n {n} r {r} {form}: worst ratio {ratio.max():.3e} (row {int(ratio.argmax())})")
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (form, int(ratio.argmax()), float(ratio.max()))
    print(f"RESID_WORST {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------
# 2. segment tables the kernels must not trust
# ------------------------------------------------------------------------------------------------------------------
BAD_LENS = [20, 130, 10, 40, 25]                       # clean table 0, 20, 150, 160, 200, 225
# name -> (entry changed, its value, the bad group); exactly one group is bad and no good group overlaps another
BAD_TABLES = {"lo<0": (0, -8, 0), "hi<lo first": (0, 28, 0), "hi<lo last": (5, 192, 4), "hi>total": (5, 233, 4)}


def bad_table(defect):
    clean = np.concatenate([[0], np.cumsum(BAD_LENS)]).astype(np.int64)
    bad = clean.copy()
    at, val, g = BAD_TABLES[defect]
    bad[at] = val
    return clean, bad, g


@pytest.mark.parametrize("defect", list(BAD_TABLES) + ["longer than declared"])
@pytest.mark.parametrize("r", [3, 17])
def test_solve_skips_a_group_with_a_bad_range(eng, r, defect):
    """A group whose range is negative, decreasing, beyond total_cols or longer than declared is skipped whole: V untouched,
    status {1, 1, 0, 5}; the other four groups as with a clean table, bit for bit; the margins untouched.
    Safety: every operand is a view with 16 floats of margin before its first and after its last column in every row,
    total_cols is the view's width and a bad range strays by at most 8 columns, so no address a kernel WITHOUT the guard would
    form leaves an allocation -- a failed guard is a wrong value here, never a fault."""
    prob = solve_problem(r, BAD_LENS, 5000 + r)
    if defect == "longer than declared":
        clean = bad_table("lo<0")[0]
        bad, g, maxlen = clean, 1, 64                    # (the table is sound; group 1 has 130 columns)
    else:
        clean, bad, g = bad_table(defect)
        maxlen = 130
    ref = run_solve(eng, prob, clean, 130, 12)
    got = run_solve(eng, prob, bad, maxlen, 12)
    want = ref["V"].copy()
    want[:, cols(clean, g)] = ref["V0"][:, cols(clean, g)]
    assert not same(ref["V"][:, cols(clean, g)], ref["V0"][:, cols(clean, g)])            # (the clean launch does solve it)
    assert same(got["V"], want)
    assert list(got["st"][g, :4]) == [1.0, 1.0, 0.0, 5.0] and (got["st"][g, 4:] == SENT).all()
    for k in range(5):
        if k != g:
            assert same(got["st"][k, :4].view(np.uint64), ref["st"][k, :4].view(np.uint64)) and got["st"][k, 3] == 0


@pytest.mark.parametrize("defect", list(BAD_TABLES))
@pytest.mark.parametrize("r", [3, 17, 33])
def test_gram_skips_a_group_with_a_bad_range(eng, r, defect):
    """G, G64, dots and err of the bad group keep their sentinel, the others are those of a clean table (same safety condition
    as test_solve_skips_a_group_with_a_bad_range: framed operands, a stray of at most 8 columns)."""
    clean, bad, g = bad_table(defect)
    prob = gram_problem(r, int(clean[-1]), 5100 + r)
    ref, got = run_gram(eng, prob, clean), run_gram(eng, prob, bad)
    for name in ("G", "G64", "dots", "err"):
        for k in range(5):
            if k == g:
                assert (got[name][k] == (SENT32 if name == "G" else SENT64)).all(), name
                assert not same(ref[name][k], got[name][k])
            else:
                assert same(got[name][k], ref[name][k]), (name, k)


@pytest.mark.parametrize("defect", list(BAD_TABLES))
@pytest.mark.parametrize("p,q", [(3, 5), (17, 17), (33, 6)])
def test_gemm_skips_a_group_with_a_bad_range(eng, p, q, defect):
    """The bad group's columns of `out` keep their sentinel, the rest of the allocation (margins included) is that of a clean
    table (same safety condition: framed operands, a stray of at most 8 columns)."""
    clean, bad, g = bad_table(defect)
    prob = gemm_problem(p, q, 5, int(clean[-1]), 5200 + p)
    ref, got = run_gemm(eng, prob, clean, 130), run_gemm(eng, prob, bad, 130)
    want = ref["out"].copy()
    want[:, cols(clean, g)] = SENT32
    assert not same(ref["out"], want)
    assert same(got["out"], want)
    assert (got["out"][:, :MARGIN] == NAN32).all() and (got["out"][:, -MARGIN:] == NAN32).all()


# ------------------------------------------------------------------------------------------------------------------
# 3. empty groups
# ------------------------------------------------------------------------------------------------------------------
EMPTY_TABLES = {"first": [0, 5, 70, 130], "middle twice": [5, 70, 0, 0, 130], "last": [5, 70, 130, 0]}


def with_and_without_empties(lens):
    full = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    keep = [g for g, n in enumerate(lens) if n > 0]
    dense = np.concatenate([[0], np.cumsum([lens[g] for g in keep])]).astype(np.int64)
    return full, dense, keep


def test_fp64_restatement_of_a_zero_column_problem():
    """What the reference's loop gives for no columns: every sweep sums to 0, 0 >= delta * 0 holds, it runs to the budget."""
    G = group_problem(3, 1, 1)[0].astype(np.float64)
    log = []
    with np.errstate(all="ignore"):
        _, eps, cnt, _ = orc.hals_nnls_acc(np.zeros((3, 0)), G, np.zeros((3, 0)), maxiter=9, alpha=math.inf, delta=0.01,
                                           sweep_log=log)
    assert eps == 0 and cnt == 10 and log[0] == 0


@pytest.mark.parametrize("where", list(EMPTY_TABLES))
@pytest.mark.parametrize("r", [3, 17])
def test_solve_empty_groups(eng, r, where):
    """An empty group changes no column and reports {eps 0, cnt budget + 1, eps0 0, err 0} (the restatement's answer); its
    neighbours are those of a launch without it, bit for bit."""
    lens = EMPTY_TABLES[where]
    full, dense, keep = with_and_without_empties(lens)
    G, M, V = solve_problem(r, lens, 5300 + r)
    got = run_solve(eng, (G, M, V), full, 130, 9)
    ref = run_solve(eng, (G[keep], M, V), dense, 130, 9)
    assert same(got["V"], ref["V"]) and not same(got["V"], got["V0"])
    for g, n in enumerate(lens):
        if n == 0:
            assert list(got["st"][g, :4]) == [0.0, 10.0, 0.0, 0.0]
    assert same(got["st"][keep, :4].view(np.uint64), ref["st"][:, :4].view(np.uint64))


@pytest.mark.parametrize("where", list(EMPTY_TABLES))
@pytest.mark.parametrize("r", [3, 17])
def test_gram_empty_groups(eng, r, where):
    """An empty group's G, G64, dots and err are written, and are exactly 0; its neighbours are unaffected."""
    lens = EMPTY_TABLES[where]
    full, dense, keep = with_and_without_empties(lens)
    prob = gram_problem(r, int(full[-1]), 5400 + r)
    got, ref = run_gram(eng, prob, full), run_gram(eng, prob, dense)
    for name in ("G", "G64", "dots", "err"):
        for g, n in enumerate(lens):
            if n == 0:
                assert (got[name][g] == 0).all(), (name, g)                      # (the image of +0.0)
        assert same(got[name][keep], ref[name]), name


@pytest.mark.parametrize("where", list(EMPTY_TABLES))
@pytest.mark.parametrize("p,q", [(3, 3), (17, 17)])
def test_gemm_empty_groups(eng, p, q, where):
    """An empty group writes nothing: the whole allocation of `out` is that of a launch without it."""
    lens = EMPTY_TABLES[where]
    full, dense, keep = with_and_without_empties(lens)
    M, A = gemm_problem(p, q, len(lens), int(full[-1]), 5500 + p)
    got, ref = run_gemm(eng, (M, A), full, 130), run_gemm(eng, (M[keep], A), dense, 130)
    assert same(got["out"], ref["out"])
    assert not (got["out"][:, MARGIN:-MARGIN] == SENT32).any()


# ------------------------------------------------------------------------------------------------------------------
# 4. the boundary between the LDS-resident tile and the tile walk
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [3, 17, 32, 33])
def test_grouped_solve_at_the_resident_tile_boundary(eng, r):
    """Lengths 127, 128 (the last resident one) and 129 (the first that walks two tiles), tolerances of check_solve."""
    check_solve(eng, ("edge128", r), r, [127, 128, 129], 1100 + r, 100)


# ------------------------------------------------------------------------------------------------------------------
# 5. the driver's call shape, and the independence of the groups
# ------------------------------------------------------------------------------------------------------------------
RUN_LENS = [5, 130, 64, 1, 33, 128, 70]
SUB_RUNS = [(0, 2), (2, 3), (3, 7)]


@pytest.mark.parametrize("r", [3, 17])
def test_solve_sub_runs_equal_the_full_launch(eng, r):
    """parafac2._update_W: off[g0:g1+1], Gs[g0:g1], status[g0:g1] with off[g0] > 0 and the operands at their full width."""
    off, offd = offsets(RUN_LENS)
    G, M, V = solve_problem(r, RUN_LENS, 5600 + r)
    Md, Gd = odd(M, pad=9), odd_stack(G)
    Vfull = odd(V)
    stfull = eng.hals_solve_group(Md, Gd, Vfull, offd, max(RUN_LENS), 15)
    Vsub = odd(V)
    st = torch.full((len(RUN_LENS), 8), SENT, dtype=torch.float64, device="cuda")
    for g0, g1 in SUB_RUNS:
        before, stb = bits(Vsub), st.cpu().numpy().copy()
        eng.hals_solve_group(Md, Gd[g0:g1], Vsub, offd[g0:g1 + 1], max(RUN_LENS), 15, status=st[g0:g1])
        after, sta = bits(Vsub), st.cpu().numpy()
        lo, hi = int(off[g0]), int(off[g1])
        assert same(after[:, :lo], before[:, :lo]) and same(after[:, hi:], before[:, hi:])
        assert not same(after[:, lo:hi], before[:, lo:hi])
        assert same(sta[:g0], stb[:g0]) and same(sta[g1:], stb[g1:])
    assert same(bits(Vsub), bits(Vfull))
    assert same(bits(st[:, :4]), bits(stfull[:, :4]))


@pytest.mark.parametrize("p,q", [(3, 5), (17, 17)])
def test_gemm_sub_runs_equal_the_full_launch(eng, p, q):
    off, offd = offsets(RUN_LENS)
    M, A = gemm_problem(p, q, len(RUN_LENS), int(off[-1]), 5700 + p)
    Md, Ad = odd_stack(M), odd(A)
    full = odd(np.full((p, int(off[-1])), SENT), pad=6)
    eng.group_gemm(Md, Ad, offd, max(RUN_LENS), out=full)
    sub = odd(np.full((p, int(off[-1])), SENT), pad=6)
    for g0, g1 in SUB_RUNS:
        before = bits(sub)
        eng.group_gemm(Md[g0:g1], Ad, offd[g0:g1 + 1], max(RUN_LENS), out=sub)
        after = bits(sub)
        lo, hi = int(off[g0]), int(off[g1])
        assert same(after[:, :lo], before[:, :lo]) and same(after[:, hi:], before[:, hi:])
        assert not (after[:, lo:hi] == SENT32).any()
    assert same(bits(sub), bits(full))


@pytest.mark.parametrize("r", [3, 17])
def test_gram_sub_runs_equal_the_full_launch(eng, r):
    """The same with the outputs sliced: a sub-run writes its own blocks of G, G64, dots and err and no other."""
    off, offd = offsets(RUN_LENS)
    total, ng = int(off[-1]), len(RUN_LENS)
    A, B, T = gram_problem(r, total, 5800 + r)
    ref = run_gram(eng, (A, B, T), off)
    Av, Bv, Tv = odd(A), odd(B, pad=2), odd(T, pad=11)
    G = torch.full((ng, r, r), SENT, dtype=torch.float32, device="cuda")
    G64 = torch.full((ng, r, r), SENT, dtype=torch.float64, device="cuda")
    dots = torch.full((ng, r), SENT, dtype=torch.float64, device="cuda")
    err = torch.full((ng,), SENT, dtype=torch.float64, device="cuda")
    outs = {"G": G, "G64": G64, "dots": dots, "err": err}
    for g0, g1 in SUB_RUNS:
        before = {k: bits(v) for k, v in outs.items()}
        sub = offd[g0:g1 + 1]
        code = eng.lib.nnf_group_gram_f32(eng.ctx, Av.data_ptr(), ld(Av), r, sub.data_ptr(), g1 - g0, total, G[g0:].data_ptr(), r,
                                          r * r, G64[g0:].data_ptr(), Bv.data_ptr(), ld(Bv), dots[g0:].data_ptr(), Tv.data_ptr(),
                                          ld(Tv), err[g0:].data_ptr(), eng._stream())
        assert code == 0
        for k, v in outs.items():
            after = bits(v)
            assert same(after[:g0], before[k][:g0]) and same(after[g1:], before[k][g1:]), k
    for k, v in outs.items():
        assert same(bits(v), ref[k]), k


@pytest.mark.parametrize("r,long_group", [(3, False), (17, False), (17, True)])
def test_solve_of_a_group_does_not_depend_on_its_position(eng, r, long_group):
    """Group 150 of 300 solved alone (ngroups = 1, its columns at offset 0): the same V and status words 0 .. 3, bit for bit."""
    lens = [int(x) for x in np.random.RandomState(r).randint(1, 41, size=300)]
    if long_group:
        lens[150] = 200                                  # (the tile walk; the others keep their tile in LDS)
    off, offd = offsets(lens)
    G, M, V = solve_problem(r, lens, 5900 + r)
    Vd = dev(V)
    st = eng.hals_solve_group(dev(M), dev(G), Vd, offd, max(lens), 40)
    sl = slice(int(off[150]), int(off[151]))
    Va = dev(V[:, sl])
    _, off1 = offsets([lens[150]])
    st1 = eng.hals_solve_group(dev(M[:, sl]), dev(G[150:151]), Va, off1, lens[150], 40)
    assert same(bits(Va), bits(Vd[:, sl]))
    assert same(bits(st1[0, :4]), bits(st[150, :4])) and float(st1[0, 3]) == 0


LEAK_LENS = [20, 130, 64, 1, 40]


def poisoned(a, off, g, value):
    a = a.copy()
    a[:, int(off[g]):int(off[g + 1])] = value
    return a


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("g", [1, 2], ids=["walked", "resident"])
@pytest.mark.parametrize("r", [3, 17])
def test_solve_does_not_leak_a_poisoned_group(eng, r, g, value):
    """NaN (or +Inf, which is NaN by the second row of the first sweep: Inf - Inf) in one group's UtM: every other group, the
    margins and their status are those of the clean run.  The poisoned group ends after its first sweep, as the reference does:
    np.maximum hands the NaN on, the sum of squared steps is NaN and !(NaN >= delta * eps0) leaves the loop -- cnt == 2."""
    off, _ = offsets(LEAK_LENS)
    G, M, V = solve_problem(r, LEAK_LENS, 6000 + r)
    ref = run_solve(eng, (G, M, V), off, 130, 25)
    got = run_solve(eng, (G, poisoned(M, off, g, value), V), off, 130, 25)
    mask = np.ones(ref["V"].shape[1], dtype=bool)
    mask[cols(off, g)] = False
    assert same(got["V"][:, mask], ref["V"][:, mask])
    keep = [k for k in range(len(LEAK_LENS)) if k != g]
    assert same(got["st"][keep].view(np.uint64), ref["st"][keep].view(np.uint64))
    print(f"poisoned group status {got['st'][g, :4]}")
    assert got["st"][g, 1] == 2 and got["st"][g, 3] == 0 and math.isnan(got["st"][g, 0])


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("r", [3, 17])
def test_gram_and_gemm_do_not_leak_a_poisoned_group(eng, r, g, value):
    off, _ = offsets(LEAK_LENS)
    total, ng = int(off[-1]), len(LEAK_LENS)
    keep = [k for k in range(ng) if k != g]
    A, B, T = gram_problem(r, total, 6100 + r)
    ref, got = run_gram(eng, (A, B, T), off), run_gram(eng, (poisoned(A, off, g, value), B, T), off)
    for name in ("G", "G64", "dots", "err"):
        assert same(got[name][keep], ref[name][keep]), name
    M, A = gemm_problem(r, r + 2, ng, total, 6200 + r)
    ref, got = run_gemm(eng, (M, A), off, 130), run_gemm(eng, (M, poisoned(A, off, g, value)), off, 130)
    mask = np.ones(ref["out"].shape[1], dtype=bool)
    mask[cols(off, g)] = False
    assert same(got["out"][:, mask], ref["out"][:, mask])


@pytest.mark.parametrize("r", [3, 17, 33])
def test_gram_into_a_caller_owned_pitch(eng, r):
    """ldg = r + 3, gstride = r (r + 3) + 5 in a NaN-filled buffer: the values of the packed call, the padding still NaN."""
    off, _ = offsets(RUN_LENS)
    ng, ldg, gstride = len(RUN_LENS), r + 3, r * (r + 3) + 5
    prob = gram_problem(r, int(off[-1]), 6300 + r)
    ref, got = run_gram(eng, prob, off), run_gram(eng, prob, off, ldg=ldg, gstride=gstride)
    raw = got["Graw"]
    written = np.zeros(raw.shape, dtype=bool)
    for g in range(ng):
        blk = raw[g * gstride:g * gstride + r * ldg].reshape(r, ldg)
        assert same(blk[:, :r], ref["G"][g]), g
        written[g * gstride:g * gstride + r * ldg].reshape(r, ldg)[:, :r] = True
    assert (raw[~written] == NAN32).all() and not (raw[written] == NAN32).any()
    for name in ("G64", "dots", "err"):
        assert same(got[name], ref[name]), name


# ------------------------------------------------------------------------------------------------------------------
# 6. the stopping rule
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("r", [3, 17])
def test_grouped_solve_other_deltas(eng, r, delta):
    """Count, eps, eps0 and the factor against the restatement at other deltas (tolerances and margin rule of check_solve);
    delta = 0 never stops before the budget."""
    lens, budget = [1, 65, 129, 300], (20 if delta == 0.0 else 100)
    off, offd = offsets(lens)
    G, M, V, want, eps, cnt = solve_case(("delta", r, delta), r, lens, 1200 + r, budget, delta=delta)
    Vd = odd(V)
    st = eng.hals_solve_group(odd(M, pad=9), odd_stack(G), Vd, offd, max(lens), budget, delta=delta).cpu().numpy()
    got = Vd.cpu().numpy()
    bad = []
    for g, n in enumerate(lens):
        sl = slice(off[g], off[g + 1])
        eps0 = orc.hals_nnls_acc(M[:, sl].astype(np.float64), G[g].astype(np.float64), V[:, sl].astype(np.float64), maxiter=1,
                                 alpha=math.inf, delta=delta)[1]
        e = rel(got[:, sl], want[:, sl])
        floor = 1e-12 + r * n * (2.0 ** -23 * max(1.0, float(np.abs(want[:, sl]).max(initial=0.0)))) ** 2
        print(f"delta {delta} r {r} len {n}: rel {e:.2e} cnt {int(st[g, 1])}/{cnt[g]} eps {st[g, 0]:.6e}/{float(eps[g]):.6e} "
              f"({abs(st[g, 0] - eps[g]) / max(abs(eps[g]), 1e-300):.2e}) eps0 {st[g, 2]:.6e}/{float(eps0):.6e} "
              f"({abs(st[g, 2] - eps0) / max(abs(eps0), 1e-300):.2e})")
        if (int(st[g, 1]) != cnt[g] or e > 2e-4 or abs(st[g, 0] - eps[g]) > 2e-3 * abs(eps[g]) + floor
                or abs(st[g, 2] - eps0) > 2e-3 * abs(eps0) + floor or st[g, 3] != 0):
            bad.append((g, n, int(st[g, 1]), int(cnt[g]), e, st[g, 0], float(eps[g]), st[g, 2], float(eps0), st[g, 3]))
    assert not bad, bad
    if delta == 0.0:
        assert (st[:, 1] == budget + 1).all()


@pytest.mark.parametrize("r", [3, 17])
def test_grouped_solve_no_sweeps(eng, r):
    """max_sweeps = 0: V bitwise unchanged (resident and walked groups alike), status {1, 1, 0, 0}."""
    off, _ = offsets(LEAK_LENS)
    got = run_solve(eng, solve_problem(r, LEAK_LENS, 6400 + r), off, 130, 0)
    assert same(got["V"], got["V0"])
    assert (got["st"][:, :4] == np.array([1.0, 1.0, 0.0, 0.0])).all() and (got["st"][:, 4:] == SENT).all()


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals through the C ABI: the status the argument check names, and no output touched
# ------------------------------------------------------------------------------------------------------------------
def refuse(fn, order, base, cases, outputs):
    """Every case changes some arguments of a valid call; `outputs`: name -> (tensor, its image before)."""
    bad = []
    for what, change, want in cases:
        args = dict(base)
        args.update(change)
        code = fn(*[args[k] for k in order])
        torch.cuda.synchronize()
        touched = [k for k, (t, b) in outputs.items() if not same(bits(t), b)]
        print(f"{what}: status {code}")
        if code != want or touched:
            bad.append((what, code, want, touched))
    assert not bad, bad
    assert len({c[0] for c in cases}) == len(cases)


def test_solve_refusals(eng):
    r, total = 4, 14
    _, offd = offsets([5, 9])
    G, M, V = solve_problem(r, [5, 9], 7000)
    Gd, Md, Vd = dev(G), dev(M), dev(V)
    G129 = torch.zeros((2, 129, 129), dtype=torch.float32, device="cuda")
    st = torch.full((2, 8), SENT, dtype=torch.float64, device="cuda")
    order = ["ctx", "UtM", "ldm", "UtU", "ldg", "gstride", "V", "ldv", "r", "off", "ngroups", "maxcols", "total", "sweeps",
             "delta", "status", "stream"]
    base = dict(ctx=eng.ctx, UtM=Md.data_ptr(), ldm=total, UtU=Gd.data_ptr(), ldg=r, gstride=r * r, V=Vd.data_ptr(), ldv=total,
                r=r, off=offd.data_ptr(), ngroups=2, maxcols=9, total=total, sweeps=10, delta=0.01, status=st.data_ptr(),
                stream=eng._stream())
    cases = [(f"null {k}", {k: None}, ARG) for k in ("ctx", "UtM", "UtU", "V", "off", "status")]
    cases += [("ldm < total_cols", {"ldm": total - 1}, ARG), ("ldv < total_cols", {"ldv": total - 1}, ARG),
              ("ldg < r", {"ldg": r - 1}, ARG), ("gstride < 1 with two groups", {"gstride": 0}, ARG),
              ("r < 1", {"r": 0}, ARG), ("ngroups < 1", {"ngroups": 0}, ARG), ("ngroups < 0", {"ngroups": -1}, ARG),
              ("max_group_cols < 0", {"maxcols": -1}, ARG), ("total_cols < 0", {"total": -1}, ARG),
              ("max_sweeps < 0", {"sweeps": -1}, ARG),
              ("r = 129", {"r": 129, "ldg": 129, "gstride": 129 * 129, "UtU": G129.data_ptr()}, UNSUPPORTED),
              ("max_group_cols = cap + 1", {"maxcols": CAP + 1}, UNSUPPORTED)]
    refuse(eng.lib.nnf_hals_solve_group_f32, order, base, cases, {"V": (Vd, bits(Vd)), "status": (st, bits(st))})


def test_gram_refusals(eng):
    r, total = 4, 14
    _, offd = offsets([5, 9])
    A, B, T = (dev(x) for x in gram_problem(r, total, 7100))
    G = torch.full((2, 129, 129), SENT, dtype=torch.float32, device="cuda")
    G64 = torch.full((2, 129, 129), SENT, dtype=torch.float64, device="cuda")
    dots = torch.full((2, 129), SENT, dtype=torch.float64, device="cuda")
    err = torch.full((2,), SENT, dtype=torch.float64, device="cuda")
    order = ["ctx", "A", "lda", "r", "off", "ngroups", "total", "G", "ldg", "gstride", "G64", "B", "ldb", "dots", "T", "ldt", "err",
             "stream"]
    base = dict(ctx=eng.ctx, A=A.data_ptr(), lda=total, r=r, off=offd.data_ptr(), ngroups=2, total=total, G=G.data_ptr(), ldg=r,
                gstride=r * r, G64=G64.data_ptr(), B=B.data_ptr(), ldb=total, dots=dots.data_ptr(), T=T.data_ptr(), ldt=total,
                err=err.data_ptr(), stream=eng._stream())
    cases = [(f"null {k}", {k: None}, ARG) for k in ("ctx", "A", "off")]
    cases += [("r < 1", {"r": 0}, ARG), ("ngroups < 1", {"ngroups": 0}, ARG), ("ngroups < 0", {"ngroups": -2}, ARG),
              ("total_cols < 0", {"total": -1}, ARG), ("lda < total_cols", {"lda": total - 1}, ARG),
              ("nothing asked for", {"G": None, "G64": None, "dots": None, "err": None}, ARG),
              ("ldg < r", {"ldg": r - 1}, ARG), ("gstride < 1 with two groups", {"gstride": 0}, ARG),
              ("G64 without G", {"G": None}, ARG), ("dots without B", {"B": None}, ARG),
              ("ldb < total_cols", {"ldb": total - 1}, ARG), ("err without T", {"T": None}, ARG),
              ("ldt < total_cols", {"ldt": total - 1}, ARG),
              ("r = 129", {"r": 129, "ldg": 129, "gstride": 129 * 129}, UNSUPPORTED)]
    refuse(eng.lib.nnf_group_gram_f32, order, base, cases,
           {"G": (G, bits(G)), "G64": (G64, bits(G64)), "dots": (dots, bits(dots)), "err": (err, bits(err))})


def test_gemm_refusals(eng):
    p, q, total = 3, 4, 14
    _, offd = offsets([5, 9])
    M, A = (dev(x) for x in gemm_problem(p, q, 2, total, 7200))
    M129 = torch.zeros((2, 129, 129), dtype=torch.float32, device="cuda")
    A129 = torch.zeros((129, total), dtype=torch.float32, device="cuda")
    out = torch.full((129, total), SENT, dtype=torch.float32, device="cuda")
    order = ["ctx", "M", "ldm", "mstride", "p", "q", "A", "lda", "off", "ngroups", "maxcols", "total", "out", "ldo", "stream"]
    base = dict(ctx=eng.ctx, M=M.data_ptr(), ldm=q, mstride=p * q, p=p, q=q, A=A.data_ptr(), lda=total, off=offd.data_ptr(),
                ngroups=2, maxcols=9, total=total, out=out.data_ptr(), ldo=total, stream=eng._stream())
    big = {"M": M129.data_ptr(), "ldm": 129, "mstride": 129 * 129, "A": A129.data_ptr()}
    cases = [(f"null {k}", {k: None}, ARG) for k in ("ctx", "M", "A", "off", "out")]
    cases += [("p < 1", {"p": 0}, ARG), ("q < 1", {"q": 0}, ARG), ("ngroups < 1", {"ngroups": 0}, ARG),
              ("ngroups < 0", {"ngroups": -1}, ARG), ("max_group_cols < 0", {"maxcols": -1}, ARG),
              ("total_cols < 0", {"total": -1}, ARG), ("ldm < q", {"ldm": q - 1}, ARG),
              ("mstride < 1 with two groups", {"mstride": 0}, ARG), ("lda < total_cols", {"lda": total - 1}, ARG),
              ("ldo < total_cols", {"ldo": total - 1}, ARG), ("out == A", {"out": A.data_ptr()}, ARG),
              ("p = 129", dict(big, p=129), UNSUPPORTED), ("q = 129", dict(big, q=129), UNSUPPORTED)]
    refuse(eng.lib.nnf_group_gemm_f32, order, base, cases, {"out": (out, bits(out)), "A": (A, bits(A))})


def test_resid_rows_refusals(eng):
    m, n, r = 6, 5, 3
    rng = np.random.RandomState(7300)
    X, Ut, V = dev(rng.rand(m, n)), dev(rng.rand(r, m)), dev(rng.rand(r, n))
    Ut129, V129 = (torch.zeros((129, k), dtype=torch.float32, device="cuda") for k in (m, n))
    rows = torch.full((m + 16,), SENT, dtype=torch.float64, device="cuda")
    order = ["ctx", "X", "m", "n", "ldx", "Ut", "ldu", "V", "ldv", "r", "rows", "stream"]
    base = dict(ctx=eng.ctx, X=X.data_ptr(), m=m, n=n, ldx=n, Ut=Ut.data_ptr(), ldu=m, V=V.data_ptr(), ldv=n, r=r,
                rows=rows.data_ptr(), stream=eng._stream())
    cases = [(f"null {k}", {k: None}, ARG) for k in ("ctx", "X", "Ut", "V", "rows")]
    cases += [("m < 1", {"m": 0}, ARG), ("n < 1", {"n": 0}, ARG), ("r < 1", {"r": 0}, ARG), ("m < 0", {"m": -1}, ARG),
              ("ldx < n", {"ldx": n - 1}, ARG), ("ldu < m", {"ldu": m - 1}, ARG), ("ldv < n", {"ldv": n - 1}, ARG),
              ("r = 129", {"r": 129, "Ut": Ut129.data_ptr(), "V": V129.data_ptr()}, UNSUPPORTED)]
    refuse(eng.lib.nnf_frob_resid_rows_f32, order, base, cases, {"rows": (rows, bits(rows))})

"""GPU: the kernels off the headline loop that the NTD chains and deep KL-NMF call directly -- the small GEMM
(nnf_small_gemm_f32), the raw KL numerator (nnf_mu_left_num_f32) and the deep-KL element-wise tail (nnf_deep_kl_apply_f32) --
against fp64 evaluations of the same expressions on the same fp32-rounded inputs.

Bounds (u = 2^-24):
  - small_gemm: one fp32 FMA chain of length q per entry, |C - AB| <= (q + 1) u (|A| |B|) entrywise; and the relative Frobenius
    bound 1e-5 of the suite's other products (random positive data: the chain error grows like sqrt(q) u, < 3e-6 at q = 2048);
  - mu_left_num: the MU bounds of tests/test_gpu_kernels.py::test_mu_left_row_tilings (rel 2e-5, no entry off by 1e-3);
  - deep_kl_apply: every stage is fp64 and only the output is rounded to fp32, so each entry is within two fp32 ulps of the
    reference expression (deep_mu.py:8-14, scipy's lambertw) -- or equals the reference's 1e-12 floor where its exp overflows.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


# ---- small GEMM -----------------------------------------------------------------------------------------------------------
def _guarded(a, extra_rows, extra_cols, row_fill):
    """a as the top-left block of a larger fp32 device buffer: NaN in the padding columns, `row_fill` in the guard rows."""
    r, c = a.shape
    buf = torch.full((r + extra_rows, c + extra_cols), float("nan"), dtype=torch.float32, device="cuda")
    buf[r:, :c] = row_fill
    buf[:r, :c] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return buf, buf[:r, :c]


@pytest.mark.parametrize("q", [1, 8, 9, 1536, 1537, 2048])      # 1537 and up: more than 48 KiB of A rows in LDS
@pytest.mark.parametrize("p", [1, 7, 8, 9, 129])                # partial and whole chunks of eight output rows
def test_small_gemm_against_fp64(eng, p, q):
    rng = np.random.RandomState(p * 4099 + q)
    for cols in (1, 255, 257):
        A = rng.rand(p, q).astype(np.float32)
        B = rng.rand(q, cols).astype(np.float32)
        # A's guard rows hold finite values: a kernel that ran a whole chunk of eight rows past p would write them into out's
        # guard rows (NaN) -- in bounds of the buffers, and visible
        bufA, Ad = _guarded(A, 8, 3, 1.0)
        bufB, Bd = _guarded(B, 0, 5, 1.0)
        bufO, Od = _guarded(np.zeros((p, cols), np.float32), 8, 5, float("nan"))
        eng.small_gemm(Ad, Bd, out=Od)
        got = Od.double().cpu().numpy()
        A64, B64 = A.astype(np.float64), B.astype(np.float64)
        want = A64 @ B64
        assert np.isfinite(got).all(), (p, q, cols)
        assert (np.abs(got - want) <= (q + 1) * U32 * (np.abs(A64) @ np.abs(B64))).all(), (p, q, cols)
        assert np.linalg.norm(got - want) <= 1e-5 * np.linalg.norm(want), (p, q, cols)
        assert torch.isnan(bufO[p:]).all() and torch.isnan(bufO[:, cols:]).all(), "wrote outside out"
        assert torch.equal(bufA[:p, :q].cpu(), torch.from_numpy(A)) and torch.isnan(bufA[:, q:]).all()


def test_small_gemm_refuses_q_above_2048(eng):
    from nn_fac_amd.utils.errors import EngineError
    A = torch.rand(3, 2049, device="cuda")
    B = torch.rand(2049, 10, device="cuda")
    out = torch.full((3, 10), 7.0, device="cuda")
    with pytest.raises(EngineError):
        eng.small_gemm(A, B, out=out)
    assert (out == 7.0).all()


# ---- raw KL numerator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [98304, 100000, 131072, 131100])  # the row tilings of test_mu_left_row_tilings
@pytest.mark.parametrize("r", [1, 16, 17, 33, 64])
def test_mu_left_num_against_fp64(eng, m, r):
    n = 70
    g = torch.Generator(device="cuda").manual_seed(m + r)
    Ut = torch.rand(r, m, device="cuda", generator=g) + 0.05
    V = torch.rand(r, n, device="cuda", generator=g) + 0.05
    X = (torch.rand(m, r, device="cuda", generator=g) @ torch.rand(r, n, device="cuda", generator=g)) + 0.05
    U64, V64, X64 = Ut.double().t(), V.double(), X.double()
    want = ((X64 / (U64 @ V64)) @ V64.t()).t()          # r x m: num[k, i] = sum_j X[i,j] / (UV)[i,j] V[k,j]
    got = eng.mu_left_num(X, Ut, V).double()
    assert got.shape == (r, m)
    assert float((got - want).norm() / want.norm()) < 2e-5
    assert float(((got - want).abs() / want).max()) < 1e-3       # no row block missed or doubled


def test_mu_left_num_refuses_rank_65(eng):
    from nn_fac_amd.utils.errors import EngineError
    m, n, r = 300, 40, 65
    out = torch.full((r, m), 7.0, device="cuda")
    with pytest.raises(EngineError):
        eng.mu_left_num(torch.rand(m, n, device="cuda"), torch.rand(r, m, device="cuda"), torch.rand(r, n, device="cuda"), out=out)
    assert (out == 7.0).all()


# ---- deep-KL tail: Lambert W in log space -------------------------------------------------------------------------------------
LMAX = math.log(np.finfo(np.float64).max)
H_OVER_LAM = [0.0, 30.0, 300.0, 705.0, 709.3, 720.0]                    # hsum[k] / lambda, one per row
B_VALUES = [0.0, 1e-20, 1e-8, 0.01, 1.0, 2.718, 100.0, 1e8, 1e20]
WH_VALUES = [0.0, 1e-20, 1e-3, 1.0, 1e3, 1e15]


def _deep_kl_reference(b, a, lam):
    """deep_mu.py:10-12 on b, a (fp64): max(eps, (b/lam) / (W0(b exp(a/lam) / lam) + eps))."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        from scipy.special import lambertw
        lam_arg = b * np.exp(a / lam) / lam
        w = lambertw(lam_arg, k=0).real
        return np.maximum(1e-12, (1 / lam * b) / (w + 1e-12))


@pytest.mark.parametrize("lam", [0.3, 1.0, 2.0, 7.0])
def test_deep_kl_apply_every_branch(eng, lam):
    import mpmath
    r, cols = len(H_OVER_LAM), len(B_VALUES) * len(WH_VALUES)
    b_row = np.array([bv for bv in B_VALUES for _ in WH_VALUES], dtype=np.float32)
    wh_row = np.array([wv for _ in B_VALUES for wv in WH_VALUES], dtype=np.float32)
    F = np.where(b_row > 0, 1.0, 0.0).astype(np.float32)[None, :].repeat(r, 0)      # b = F * num: F = 0 gives b = 0
    num = np.where(b_row > 0, b_row, 1.0).astype(np.float32)[None, :].repeat(r, 0)
    WH = wh_row[None, :].repeat(r, 0)
    hsum = np.array(H_OVER_LAM) * lam
    got = eng.deep_kl_apply(torch.from_numpy(F).cuda(), torch.from_numpy(num).cuda(), torch.from_numpy(hsum).cuda(),
                            torch.from_numpy(WH).cuda(), lam).double().cpu().numpy()
    b = F.astype(np.float64) * num.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = hsum[:, None] - lam * np.log(WH.astype(np.float64))
        L = np.log(b) + a / lam - math.log(lam)                              # log of the Lambert W argument
        Lb = np.log(b) + a / lam
    want = _deep_kl_reference(b, a, lam)
    # b = 0 where exp(a / lambda) overflows (WHn = 0 among them): the reference's 0 * inf is NaN, the kernel keeps the 1e-12 floor
    # of every other b = 0 entry (a NaN would poison the whole layer)
    zero_inf = (b == 0) & (a / lam > LMAX)
    assert np.array_equal(np.isnan(want), zero_inf) and (got[zero_inf] == np.float32(1e-12)).all()
    ok = ~zero_inf
    floor = ok & ((b == 0) | ~np.isfinite(a) | (a / lam > LMAX) | (Lb > LMAX) | (L > LMAX))
    branch = {"b = 0": (b == 0) & ok, "WHn = 0": (WH == 0) & (b > 0), "L < -36": ok & ~floor & (L < -36),
              "-36 <= L <= 1": ok & ~floor & (L >= -36) & (L <= 1), "1 < L < 700": ok & ~floor & (L > 1) & (L < 700),
              "overflow floor": floor & (b > 0), "product overflows, quotient would not": ok & (a / lam <= LMAX) & (Lb > LMAX) & (L <= LMAX)}
    for name, sel in branch.items():
        if name == "product overflows, quotient would not" and lam <= 1:
            continue
        assert sel.any(), f"no entry in branch {name}"
    assert (want[floor] == 1e-12).all()
    want32 = want.astype(np.float32).astype(np.float64)
    assert np.array_equal(got[floor], want32[floor]), "the reference's overflow floor"
    live = ok & ~floor
    err = np.abs(got - want)
    assert (err[live] <= 2 * 2 * U32 * want[live]).all(), float((err[live] / want[live]).max())    # two fp32 ulps
    # large finite L: against mpmath from the log-argument (w + log w = L), not through exp
    mpmath.mp.dps = 40
    for k, i in zip(*np.nonzero(live & (L > 1))):
        w = mpmath.lambertw(mpmath.exp(mpmath.mpf(float(L[k, i]))))
        ref = max(1e-12, float((mpmath.mpf(b[k, i]) / lam) / (w + mpmath.mpf("1e-12"))))
        assert abs(got[k, i] - ref) <= 4 * U32 * ref, (k, i, float(L[k, i]), got[k, i], ref)

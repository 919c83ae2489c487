"""The weighted forms of the fused MU kernels and of the cost kernel (nnf_mu_left_w_f32, nnf_mu_right_w_f32, nnf_betadiv_w_f32;
k_mu.hip parts 7 .. 10, k_cost.hip) against fp64, on every launch plan they take.  Needs a MI355X.

The model is tests/test_gpu_launch_plans.py: the shapes are written from the CU count so that each case sits on the side of a plan
threshold it names, the plan is read back from NNF_PLAN_DEBUG (a child process: the library reads the variable once), and every
measured call writes NaN-filled outputs right after a call on other data.  The weighted forms take the general-beta plans (bm=WGEN):
the small / mid / hi row mixes of the left update up to rank 64, 128-row workgroups above; the occupancy, min_rows, workspace and
one-split bounds of the right update at ranks 34, 65 and 128, and one offset32 case in which only the pitch of the WEIGHTS crosses
the 32-bit offset line.  Then every beta of 0, 0.5, 1, 2, 3 at ranks 1, 16, 50, 64, 65, 100, 128 on one small shape whose weights
hold every pattern at once (below), with X and the weights aligned, and each of the two alone in an unaligned buffer.

Reference: fp64 on the device from the fp32 operands, the zero-weight entries of X replaced by 1 before it is formed.  Bounds: the
project's own for these kernels -- num and den as the mu_accum rows of test_gpu_launch_plans (2e-5 global, 1e-3 per entry), the cost
within 1e-5 relative as its cost rows; zero rows and columns give exact zeros.
"""
import collections
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_launch_plans import ROOT, WS_ERR, _cdiv, _cus, _m_of, mu_right_prologue, mu_right_terms_fp64, mu_accum_into, parse_plans

pytestmark = pytest.mark.gpu

GLOB, ENT, COST = 2e-5, 1e-3, 1e-5
BETAS = (0, 0.5, 1, 2, 3)
RANKS = (1, 16, 50, 64, 65, 100, 128)
END32 = 0x7fff0000

WCase = collections.namedtuple("WCase", "side m n r beta ldx ldw ws expect")


def weighted_cases(C):
    """{name: WCase}: `ldx` / `ldw` the pitches of X and of the weights (None: n), `ws` the context workspace (None: the
    process engine's), `expect` the fields the library must report."""
    cases = {}

    def add(name, side, m, n, r, beta, expect, ldx=None, ldw=None, ws=None):
        assert name not in cases
        cases[name] = WCase(side, m, n, r, beta, ldx, ldw, ws, dict(expect, bm="WGEN", rem=0, mt=_cdiv(r, 16)))

    # ---- left: one workgroup per CU.  T <= 8 C row tiles: 128-row workgroups; up to rank 64 then 192 + 128 rows (mid) and, past
    # 12 C, 256 + 192 (hi); above rank 64 128-row workgroups whatever the height ----
    for form, T in [("small", 8 * C), ("mid", 8 * C + 1), ("hi", 12 * C + 1)]:
        add(f"left_r50_{form}", "left", _m_of(T), 72, 50, 0.5, dict(form=form, vec=1))
    for r in (65, 128):
        add(f"left_r{r}_small", "left", _m_of(8 * C), 72, r, 0.5, dict(form="small", vec=1, grid=_cdiv(_m_of(8 * C), 128)))
        add(f"left_r{r}_rows128", "left", _m_of(8 * C + 1), 72, r, 1 if r == 65 else 2,
            dict(form="rows128", vec=1, grid=_cdiv(_m_of(8 * C + 1), 128), n_hi=0, n_mid=0))
    add("left_r128_unaligned", "left", _m_of(8 * C + 1), 70, 128, 0.5, dict(form="rows128", vec=0), ldx=71, ldw=71)

    # ---- right: nsplit = C / column blocks (256 columns up to rank 64, 128 above), cut to m / 64 and to the pairs of slabs the
    # workspace holds; rows per split halved until they stay inside 32-bit offsets at the LARGER of the two pitches ----
    def right(name, m, n, r, beta, bound, nsplit, rps=None, **kw):
        rps = 64 * _cdiv(_cdiv(m, nsplit), 64) if rps is None else rps
        add(name, "right", m, n, r, beta, dict(bound=bound, nsplit=_cdiv(m, rps), rps=rps, vec=kw.pop("vec", 1)), **kw)

    for r, beta in [(34, 0.5), (65, 1), (128, 2)]:
        ncb = _cdiv(2000, 256 if r <= 64 else 128)
        right(f"right_r{r}_occupancy", 20000, 2000, r, beta, "occupancy", C // ncb)
        right(f"right_r{r}_min_rows", 1000, 1000, r, beta, "min_rows", _cdiv(1000, 64))
        slabs = 10 * r * 2000 * 4      # ten PAIRS of slabs, the second set behind the cursor's 256-byte alignment
        right(f"right_r{r}_workspace", 20000, 2000, r, beta, "workspace", 10,
              ws=mu_right_prologue(r, 20000, 0.5) + 256 * _cdiv(slabs, 256) + slabs)
        n_one = (256 if r <= 64 else 128) * C + 200      # more column blocks than CUs: one split
        right(f"right_r{r}_one_split", 300, n_one, r, beta, "occupancy", 1)
    # only the weights' pitch crosses the line: one split of 256 rows at the pitch of X, halved at the pitch of the weights
    n_one = 128 * C + 200
    ldw = 4 * (_cdiv(END32, 4 * 384 * 4) + 1)
    assert 384 * n_one * 4 < END32 <= 384 * ldw * 4 and 256 * ldw * 4 < END32
    right("right_r128_offset32_ldw_only", 200, n_one, 128, 0.5, "offset32", None, rps=128, ldw=ldw)
    return cases


CASE_NAMES = list(weighted_cases(256))


def strided(m, n, ld, dev="cuda"):
    """An m x n view of pitch ld (None: contiguous); a narrow padding holds NaN (a wide one is left as it is: gigabytes)."""
    if ld is None or ld == n:
        return torch.empty(m, n, device=dev)
    buf = torch.empty(m * ld, device=dev).view(m, ld)
    if ld - n <= 64:
        buf[:, n:] = float("nan")
    return buf[:, :n]


def make_inputs(case, seed, dev="cuda"):
    g = torch.Generator(device=dev).manual_seed(seed)
    m, n, r = case.m, case.n, case.r
    X, Wg = strided(m, n, case.ldx), strided(m, n, case.ldw)
    X.copy_(torch.rand(m, n, device=dev, generator=g) + 0.05)
    Wg.copy_(torch.rand(m, n, device=dev, generator=g) * 2)
    Wg[torch.rand(m, n, device=dev, generator=g) < 0.1] = 0
    Wg[m // 3, :] = 0      # a row and a column without weight
    Wg[:, n // 2] = 0
    Ut = torch.rand(r, m, device=dev, generator=g) + 0.05
    V = torch.rand(r, n, device=dev, generator=g) + 0.05
    return {"X": X, "Wg": Wg, "Ut": Ut, "V": V}


def sums_fp64(X, Wg, Ut, V, beta, side):
    """(num, den) in fp64 from the fp32 operands, the zero-weight entries of X replaced by 1 first; row blocks of at most 2^24
    entries."""
    U64, V64 = Ut.double(), V.double()
    num = torch.zeros((Ut.shape[0], X.shape[0] if side == "left" else X.shape[1]), dtype=torch.float64, device=X.device)
    den = torch.zeros_like(num)
    step = max(64, (1 << 24) // X.shape[1])
    for i0 in range(0, X.shape[0], step):
        W = Wg[i0:i0 + step].double()
        Xb = torch.where(W == 0, torch.ones_like(W), X[i0:i0 + step].double())
        P = U64[:, i0:i0 + step].t() @ V64
        a = torch.where(Xb == 0, torch.zeros_like(W), W * Xb * P ** (beta - 2))
        b = W * P ** (beta - 1)
        if side == "left":
            num[:, i0:i0 + step] = V64 @ a.t()
            den[:, i0:i0 + step] = V64 @ b.t()
        else:
            num += U64[:, i0:i0 + step] @ a
            den += U64[:, i0:i0 + step] @ b
    return num, den


def cost_fp64(X, Wg, Ut, V, beta):
    W = Wg.double()
    x = torch.where(W == 0, torch.ones_like(W), X.double())
    P = Ut.double().t() @ V.double()
    if beta == 1:
        t = torch.where(x == 0, P, x * torch.log(torch.where(x == 0, torch.ones_like(x), x) / P) - x + P)
    elif beta == 0:
        t = x / P - torch.log(x / P) - 1
    elif beta == 2:
        t = 0.5 * (x - P) ** 2
    else:
        t = (x ** beta + (beta - 1) * P ** beta - beta * x * P ** (beta - 1)) / (beta * (beta - 1))
    return float((W * t).sum())


def check_sums(got, want, empty, what):
    """Finite; exact zeros where the slice has no weight; elsewhere global relative error <= GLOB and entrywise <= ENT.
    Returns the two figures."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries (a tile never written, or a NaN let through)"
    assert bool((got[:, empty] == 0).all()), f"{what}: a slice without weight must be exactly 0"
    g, w = got[:, ~empty], want[:, ~empty]
    d = (g - w).abs()
    fg = float(d.norm() / w.norm())
    fe = float((d / w.abs()).max()) if bool((w > 0).all()) else float("inf")
    print(f"{what}: global {fg:.3e} entrywise {fe:.3e}")
    assert fg <= GLOB and fe <= ENT, f"{what}: global {fg:.3e} (<= {GLOB}), entrywise {fe:.3e} (<= {ENT})"
    return fg, fe


_ENGINES = {}


def engine_for(ws):
    from nn_fac_amd.engine import Engine, get_engine
    if ws is None:
        return get_engine("cuda:0")
    if ws not in _ENGINES:
        _ENGINES[ws] = Engine(torch.device("cuda:0"), workspace_bytes=ws)
    return _ENGINES[ws]


def run_case(eng, case, inp, num=None, den=None):
    fn = eng.mu_left_w if case.side == "left" else eng.mu_right_w
    return fn(inp["X"], inp["Wg"], inp["Ut"], inp["V"], case.beta, out_num=num, out_den=den)


def other_data(inp):
    return dict(inp, Ut=inp["Ut"] * 2 + 0.5, V=inp["V"] * 3 + 1)


# ---- the plan table, as the library reports it ----
_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_weighted_kernels as P
for name, case in P.weighted_cases(P._cus()).items():
    sys.stderr.write("[case] %s\n" % name)
    sys.stderr.flush()
    inp = P.make_inputs(case, 1)
    P.run_case(P.engine_for(case.ws), case, inp)
    torch.cuda.synchronize()
    del inp
    torch.cuda.empty_cache()
print("done")
"""


def test_weighted_plan_table(built_lib):
    """Every case takes the plan it is listed with: one report line of its launcher per call, bm=WGEN."""
    p = subprocess.run([sys.executable, "-c", _CHILD], env=dict(os.environ, NNF_PLAN_DEBUG="1"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    reported = parse_plans(p.stderr)
    cases = weighted_cases(_cus())
    assert sorted(reported) == sorted(cases)
    bad, seen = [], collections.defaultdict(set)
    for name, case in cases.items():
        lines = [kv for (l, kv) in reported[name] if l == "mu_" + case.side]
        if len(lines) != 1:
            bad.append((name, "report lines", reported[name]))
            continue
        kv = lines[0]
        assert int(kv["m"]) == case.m and int(kv["r"]) == case.r, (name, kv)
        for key, want in case.expect.items():
            if kv.get(key) != str(want):
                bad.append((name, key, kv.get(key), want))
        seen[case.side].add(kv.get("form") or kv.get("bound"))
    assert not bad, "\n".join(map(str, bad))
    assert seen["left"] == {"small", "mid", "hi", "rows128"} and seen["right"] == {"occupancy", "min_rows", "workspace", "offset32"}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_weighted_plan_values(name, built_lib):
    """Each case against fp64, entry by entry, in NaN-filled outputs right after a call on other data (same engine)."""
    case = weighted_cases(_cus())[name]
    eng = engine_for(case.ws)
    inp = make_inputs(case, 7)
    want_num, want_den = sums_fp64(inp["X"], inp["Wg"], inp["Ut"], inp["V"], case.beta, case.side)
    cols = case.m if case.side == "left" else case.n
    num, den = (torch.empty(case.r, cols, device="cuda") for _ in range(2))
    run_case(eng, case, other_data(inp), num, den)
    num.fill_(float("nan"))
    den.fill_(float("nan"))
    got = run_case(eng, case, inp, num, den)
    assert got[0].data_ptr() == num.data_ptr() and got[1].data_ptr() == den.data_ptr()
    empty = torch.zeros(cols, dtype=torch.bool, device="cuda")
    empty[case.m // 3 if case.side == "left" else case.n // 2] = True
    check_sums(num, want_num, empty, name + " num")
    check_sums(den, want_den, empty, name + " den")


# ---- every beta at one small shape, every weight pattern in one matrix ----
M, N = 200, 136


def pattern_inputs(r, layout, dev="cuda"):
    """X and the weights of the small shape: `layout` 'aligned' (both contiguous), 'x_unaligned' (X in a 203 x 139 buffer),
    'w_unaligned' (the weights in a 200 x 137 buffer).  Weights uniform in (0, 2) with a zero row, a zero column, a zero 64 x 64
    block on the tile grid and one across it, 30 % scattered zeros -- NaN, +Inf and -Inf in X under all of them -- and a few
    zeros of X under positive weights."""
    g = torch.Generator(device=dev).manual_seed(100 + r)
    X = torch.empty(203, 139, device=dev).fill_(float("nan"))[:M, :N] if layout == "x_unaligned" else torch.empty(M, N, device=dev)
    Wg = torch.empty(M, 137, device=dev).fill_(float("nan"))[:, :N] if layout == "w_unaligned" else torch.empty(M, N, device=dev)
    X.copy_(torch.rand(M, N, device=dev, generator=g) + 0.05)
    Wg.copy_(torch.rand(M, N, device=dev, generator=g) * 2 + 1e-3)
    Wg[17, :] = 0
    Wg[:, 5] = 0
    Wg[64:128, 64:128] = 0
    Wg[100:164, 30:94] = 0
    Wg[torch.rand(M, N, device=dev, generator=g) < 0.3] = 0
    off = Wg == 0
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")], device=dev)
    X[off] = bad[torch.randint(0, 3, (int(off.sum()),), device=dev, generator=g)]
    zeros = [(3, 7), (40, 9), (150, 120), (199, 135), (64, 0)]
    for i, j in zeros:
        Wg[i, j] = 0.7
        X[i, j] = 0.0
    Ut = torch.rand(r, M, device=dev, generator=g) + 0.05
    V = torch.rand(r, N, device=dev, generator=g) + 0.05
    return {"X": X, "Wg": Wg, "Ut": Ut, "V": V}


@pytest.mark.parametrize("r", RANKS)
def test_every_beta_and_pattern(r, built_lib):
    eng = engine_for(None)
    erow = torch.zeros(M, dtype=torch.bool, device="cuda")
    ecol = torch.zeros(N, dtype=torch.bool, device="cuda")
    erow[17] = ecol[5] = True
    worst = {}
    for layout in ("aligned", "x_unaligned", "w_unaligned"):
        inp = pattern_inputs(r, layout)
        X, Wg, Ut, V = inp["X"], inp["Wg"], inp["Ut"], inp["V"]
        assert bool(torch.isnan(X).any()) and bool(torch.isinf(X).any())
        for beta in BETAS:
            for side, cols, empty in (("left", M, erow), ("right", N, ecol)):
                want = sums_fp64(X, Wg, Ut, V, beta, side)
                num, den = (torch.full((r, cols), float("nan"), device="cuda") for _ in range(2))
                fn = eng.mu_left_w if side == "left" else eng.mu_right_w
                fn(X, Wg, Ut, V, beta, out_num=num, out_den=den)
                for nm, got, w in (("num", num, want[0]), ("den", den, want[1])):
                    f = check_sums(got, w, empty, f"r={r} {layout} beta={beta} {side} {nm}")
                    worst[beta] = max(worst.get(beta, (0, 0)), f)
                num2, den2 = (torch.full((r, cols), float("nan"), device="cuda") for _ in range(2))
                fn(X, Wg, Ut, V, beta, out_num=num2, out_den=den2)
                assert torch.equal(num, num2) and torch.equal(den, den2), "two calls must be bitwise equal"
            # the cost: +inf at beta = 0 with an observed zero; the finite part on a copy with those zeros replaced
            out = torch.full((1,), 1e300, dtype=torch.float64, device="cuda")
            got = float(eng.betadiv_w(X, Wg, Ut, V, beta, out=out))
            if beta == 0:
                assert got == float("inf")
                Xf = X.clone()
                Xf[(X == 0) & (Wg != 0)] = 0.5
                got, want_c = float(eng.betadiv_w(Xf, Wg, Ut, V, beta)), cost_fp64(Xf, Wg, Ut, V, beta)
            else:
                want_c = cost_fp64(X, Wg, Ut, V, beta)
            print(f"r={r} {layout} beta={beta} cost: relative {abs(got - want_c) / abs(want_c):.3e}")
            assert abs(got - want_c) <= COST * abs(want_c), (r, layout, beta, got, want_c)
    print("worst (global, entrywise) per beta:", worst)


@pytest.mark.parametrize("r", (34, 100))
def test_all_ones_agree_with_the_unweighted_accumulate(r, built_lib):
    """Wg == 1 against nnf_mu_right_accum_f32 at a general beta, within the sum of the two bounds (not bitwise: the weighted
    form multiplies by 1.0 after the power pair)."""
    eng = engine_for(None)
    g = torch.Generator(device="cuda").manual_seed(r)
    m, n = 3000, 520
    inp = {"X": torch.rand(m, n, device="cuda", generator=g) + 0.05, "Ut": torch.rand(r, m, device="cuda", generator=g) + 0.05,
           "V": torch.rand(r, n, device="cuda", generator=g) + 0.05}
    ones = torch.ones(m, n, device="cuda")
    for beta in (0.5, 3):
        num, den = eng.mu_right_w(inp["X"], ones, inp["Ut"], inp["V"], beta)
        n0, d0 = (torch.empty(r, n, device="cuda") for _ in range(2))
        dvec = torch.empty(r, dtype=torch.float64, device="cuda")
        mu_accum_into(eng, inp, beta, n0, d0, dvec)
        for a, b in ((num, n0), (den, d0)):
            d = (a.double() - b.double()).abs()
            assert float(d.norm() / b.double().norm()) <= 2 * GLOB and float((d / b.double().abs()).max()) <= 2 * ENT


# ---- refusals: nothing launched, the outputs untouched ----
def _raw(eng, name, X, Wg, Ut, V, beta, num, den, r=None, ldw=None, null_w=False):
    from nn_fac_amd.engine import _ld, _ptr
    fn = getattr(eng.lib, name)
    args = [eng.ctx, _ptr(X), X.shape[0], X.shape[1], _ld(X), None if null_w else _ptr(Wg), _ld(Wg) if ldw is None else ldw,
            _ptr(Ut), _ld(Ut), _ptr(V), _ld(V), Ut.shape[0] if r is None else r, float(beta)]
    if name == "nnf_betadiv_w_f32":
        return fn(*args, _ptr(num), eng._stream())
    return fn(*args, _ptr(num), _ld(num), _ptr(den), _ld(den), eng._stream())


def test_c_abi_refusals(built_lib):
    eng = engine_for(None)
    m, n, r = 300, 136, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    X, Wg = torch.rand(m, n, device="cuda", generator=g), torch.rand(m, n, device="cuda", generator=g)
    Ut, V = torch.rand(r + 1, m, device="cuda", generator=g), torch.rand(r + 1, n, device="cuda", generator=g)
    spoilt = [(dict(r=129), -3), (dict(ldw=n - 1), -1), (dict(null_w=True), -1), (dict(beta=-1.0), -1), (dict(beta=float("nan")), -1)]
    for name, cols in (("nnf_mu_left_w_f32", m), ("nnf_mu_right_w_f32", n), ("nnf_betadiv_w_f32", 1)):
        for kw, status in spoilt:
            kw = dict(kw)
            beta = kw.pop("beta", 0.5)
            rr = kw.get("r", r)
            if name == "nnf_betadiv_w_f32":
                num = den = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
            else:
                num, den = (torch.full((r + 1, cols), float("nan"), device="cuda") for _ in range(2))
            st = _raw(eng, name, X, Wg, Ut[:rr] if rr <= r else Ut, V[:rr] if rr <= r else V, beta, num, den, **kw)
            torch.cuda.synchronize()
            assert st == status, (name, kw, beta, st)
            assert bool(torch.isnan(num).all()) and bool(torch.isnan(den).all()), (name, kw)
        ok = _raw(eng, name, X, Wg, Ut[:r], V[:r], 0.5, *(torch.empty((1,), dtype=torch.float64, device="cuda"),) * 2) \
            if name == "nnf_betadiv_w_f32" else _raw(eng, name, X, Wg, Ut[:r], V[:r], 0.5, *(torch.empty(r, cols, device="cuda") for _ in range(2)))
        assert ok == 0


def test_workspace_one_byte_short_of_a_slab_pair(built_lib):
    from nn_fac_amd.engine import Engine
    from nn_fac_amd.utils.errors import EngineError
    m, n, r = 1000, 520, 50
    slab = r * n * 4
    need = mu_right_prologue(r, m, 0.5) + 256 * _cdiv(slab, 256) + slab
    g = torch.Generator(device="cuda").manual_seed(4)
    X, Wg = torch.rand(m, n, device="cuda", generator=g) + 0.05, torch.rand(m, n, device="cuda", generator=g)
    Ut, V = torch.rand(r, m, device="cuda", generator=g) + 0.05, torch.rand(r, n, device="cuda", generator=g) + 0.05
    num, den = (torch.full((r, n), float("nan"), device="cuda") for _ in range(2))
    with pytest.raises(EngineError, match=WS_ERR):
        Engine(torch.device("cuda:0"), workspace_bytes=need - 1).mu_right_w(X, Wg, Ut, V, 0.5, out_num=num, out_den=den)
    torch.cuda.synchronize()
    assert bool(torch.isnan(num).all()) and bool(torch.isnan(den).all())
    Engine(torch.device("cuda:0"), workspace_bytes=need).mu_right_w(X, Wg, Ut, V, 0.5, out_num=num, out_den=den)
    want = sums_fp64(X, Wg, Ut, V, 0.5, "right")
    none = torch.zeros(n, dtype=torch.bool, device="cuda")
    check_sums(num, want[0], none, "one pair of slabs num")
    check_sums(den, want[1], none, "one pair of slabs den")


# ---- the operand refusals of the three Engine methods (WeightedOps), one spoilt operand at a time ----
def test_engine_method_refusals(built_lib):
    from nn_fac_amd.utils.errors import EngineError
    eng = engine_for(None)
    m, n, r = 64, 40, 5
    ok = dict(X=torch.rand(m, n, device="cuda"), Wg=torch.rand(m, n, device="cuda"), Ut=torch.rand(r, m, device="cuda"),
              V=torch.rand(r, n, device="cuda"), beta=1.5)
    spoilt = {
        "Wg": [torch.rand(m, n + 1, device="cuda"), torch.rand(m, n), torch.rand(m, n, device="cuda").double(),
               torch.rand(n, m, device="cuda").t()],
        "X": [torch.rand(m + 1, n, device="cuda"), torch.rand(m, n, device="cuda").double()],
        "Ut": [torch.rand(r, m + 1, device="cuda"), torch.rand(129, m, device="cuda")],
        "V": [torch.rand(r + 1, n, device="cuda")],
        "beta": [-0.5, float("nan"), float("inf"), "two"],
    }
    for method, cols in (("mu_left_w", m), ("mu_right_w", n), ("betadiv_w", None)):
        fn = getattr(eng, method)
        for key, values in spoilt.items():
            for v in values:
                kw = dict(ok, **{key: v})
                if key == "Ut" and v.shape[0] == 129:
                    kw["V"] = torch.rand(129, n, device="cuda")
                with pytest.raises(EngineError, match=method):
                    fn(kw["X"], kw["Wg"], kw["Ut"], kw["V"], kw["beta"])
        if cols is None:
            for bad in (torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.float64)):
                with pytest.raises(EngineError, match="betadiv_w out"):
                    fn(ok["X"], ok["Wg"], ok["Ut"], ok["V"], ok["beta"], out=bad)
            assert fn(ok["X"], ok["Wg"], ok["Ut"], ok["V"], ok["beta"]).shape == (1,)
        else:
            for which in ("out_num", "out_den"):
                for bad in (torch.empty(r, cols + 1, device="cuda"), torch.empty(r, cols), torch.empty(r, cols, device="cuda").double()):
                    with pytest.raises(EngineError, match=f"{method} {which}"):
                        fn(ok["X"], ok["Wg"], ok["Ut"], ok["V"], ok["beta"], **{which: bad})
            num, den = fn(ok["X"], ok["Wg"], ok["Ut"], ok["V"], ok["beta"])
            assert num.shape == den.shape == (r, cols)

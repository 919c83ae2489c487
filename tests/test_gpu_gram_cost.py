"""nnf_gram_cost_kernel (the Gram-identity cost of the HALS loops of nmf and ntf), its three entry points, the calibration that
feeds it (Engine.cross_rounding / gram_rounding) and nnf_dot_f32 (its ||X||^2) against extended-precision restatements on the
SAME fp32 operands (tests/gram_cost_restatement.py).  The kernel sums in fp64 throughout, so the bounds are the a-priori error of
an fp64 sum of that many products, doubled -- about 1e-11 relative, where a dropped element, a wrong stride or the wrong Gram
shows.  Needs a MI355X."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import gram_cost_restatement as gcr

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5
NNF_OK, NNF_ERR_ARG = 0, -1
PAD_V, PAD_M, PAD_G = 5, 12, 3
# (sigma_a, bias_a): the default, what a 1e6-row run calibrates to, NTF's
ROUNDINGS = [(6e-8, 0.0), (9.5e-7, 2.2e-7), (6e-8, 1e-9)]
SIGMA_G64 = [5e-9, 0.0]
FORMS = ["fp32", "had", "g64"]


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    assert torch.cuda.is_available()
    return get_engine("cuda:0")


def bits(t):
    """The bytes of a tensor, as integers (NaN == NaN)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).clone()


class Operand:
    """An r x c fp32 operand on the device: contiguous, or the view [:, :c] of a buffer whose padding holds NaN."""

    def __init__(self, a, pad=0):
        a = np.ascontiguousarray(a, dtype=np.float32)
        buf = np.full((a.shape[0], a.shape[1] + pad), np.nan, dtype=np.float32)
        buf[:, :a.shape[1]] = a
        self.host = a
        self.buf = torch.from_numpy(buf).cuda()
        self.t = self.buf[:, :a.shape[1]]
        self.before = bits(self.buf)

    def untouched(self):
        return torch.equal(bits(self.buf), self.before)


class Case:
    """The operands of one (r, n) in every form, and their sums."""
    _data = {}

    @classmethod
    def data(cls, r, n):
        """Host arrays and V V^T of (r, n), shared by the forms and layouts."""
        if (r, n) not in cls._data:
            rng = np.random.RandomState(r * 10007 + n)
            V = rng.rand(r, n).astype(np.float32)
            V[rng.rand(r, n) < 0.2] = 0.0                      # exact zeros, as a projected factor has
            V[r // 2, n // 2] = 0.625                          # (never all of it: r = n = 1)
            UtM = (rng.rand(r, n) - 0.25).astype(np.float32)
            G = (rng.rand(r, r) - 0.25).astype(np.float32)     # NOT symmetric: a transposed read shows
            G2 = (rng.rand(r, r) - 0.25).astype(np.float32)
            G64 = G.astype(np.float64) + 1e-9 * rng.rand(r, r)  # reading G in its place is 1e-9 away
            cls._data[(r, n)] = (V, UtM, G, G2, G64, gcr.column_gram(V))
        return cls._data[(r, n)]

    def __init__(self, r, n, padded=False, V=None):
        Vh, UtM, G, G2, G64, W = self.data(r, n)
        if V is not None:
            Vh, W = V, gcr.column_gram(V)
        self.r, self.n = r, n
        self.V = Operand(Vh, PAD_V if padded else 0)
        self.UtM = Operand(UtM, PAD_M if padded else 0)
        self.G = Operand(G, PAD_G if padded else 0)
        self.G2 = Operand(G2, PAD_G if padded else 0)
        self.G64h = G64
        self.G64 = torch.from_numpy(G64).cuda()
        self.sums = {"fp32": gcr.sums(Vh, UtM, G, W=W), "had": gcr.sums(Vh, UtM, G, G2=G2, W=W),
                     "g64": gcr.sums(Vh, UtM, G, G64=G64, W=W)}
        self.nx2 = torch.zeros(1, dtype=torch.float64, device="cuda")

    def set_cost(self, form, target):
        """normx2 such that the cost of `form` is about `target`; returns the double the kernel will read."""
        s = self.sums[form]
        nx = float(2 * s.A - s.B + gcr.LD(target))
        self.nx2.fill_(nx)
        return nx

    def untouched(self):
        return self.V.untouched() and self.UtM.untouched() and self.G.untouched() and self.G2.untouched() \
            and torch.equal(bits(self.G64), bits(torch.from_numpy(self.G64h)))

    def call(self, eng, form, block, sa=6e-8, ba=0.0, sg=5e-9):
        out = block[19:22]
        if form == "g64":
            eng.gram_cost(self.V.t, self.UtM.t, self.G.t, self.nx2, out, rounding=(sa, ba, sg), UtU64=self.G64)
        else:
            eng.gram_cost(self.V.t, self.UtM.t, self.G.t, self.nx2, out, rounding=(sa, ba),
                          UtU_b=self.G2.t if form == "had" else None)

    def call_default_entry(self, eng, form, block):
        """nnf_nmf_gram_cost_f32 (6e-8 / 0 built in): no engine method, through the library."""
        from nn_fac_amd.engine import _ld, _ptr
        out = block[19:22]
        st = eng.lib.nnf_nmf_gram_cost_f32(eng.ctx, _ptr(self.V.t), _ld(self.V.t), _ptr(self.UtM.t), _ld(self.UtM.t), _ptr(self.G.t),
                                           _ptr(self.G2.t) if form == "had" else None, _ld(self.G.t), self.r, self.n,
                                           _ptr(self.nx2), _ptr(out), eng._stream())
        assert st == NNF_OK


def new_block():
    return torch.full((32,), SENTINEL, dtype=torch.float64, device="cuda")


def read_block(block):
    """(cost, flag, est) of a status block whose other words must still hold the sentinel."""
    h = block.cpu().numpy()
    rest = np.delete(h, [19, 20, 21])
    assert (rest == SENTINEL).all(), "words outside [19:22] of the status block were written"
    return h[19:22].copy()


worst = {"cost": 0.0, "est": 0.0}


def check_against_restatement(eng, case, form, target):
    """Part A for one (case, form): every rounding figure and entry point of the form."""
    nx = case.set_cost(form, target)
    figures = [(sa, ba, sg) for sa, ba in ROUNDINGS for sg in (SIGMA_G64 if form == "g64" else [gcr.SIGMA_G_FP32])]
    for sa, ba, sg in figures:
        ref = gcr.verdict(case.sums[form], nx, sa, ba, sg)
        block = new_block()
        case.call(eng, form, block, sa, ba, sg)
        cost, flag, est = read_block(block)
        dc, de = abs(cost - ref.cost) / ref.tol_cost, abs(est - ref.est) / ref.tol_est
        worst["cost"], worst["est"] = max(worst["cost"], dc), max(worst["est"], de)
        print(f"A {form} r={case.r} n={case.n} ld={case.V.t.stride(0)} sigma=({sa:g},{ba:g},{sg:g}) cost {cost:.17g} "
              f"|cost-ref|/tol_cost {dc:.3g} |est-ref|/tol_est {de:.3g} tol_cost/|terms| "
              f"{ref.tol_cost / (abs(nx) + 2 * ref.abs_a + ref.abs_b):.2g} flag {flag:g}/{ref.flag} "
              f"worst so far {worst['cost']:.3g} {worst['est']:.3g}")
        assert ref.est / (5e-4 * ref.cost) < 0.5 or ref.est / (5e-4 * ref.cost) > 2      # (the data's choice, not the kernel's)
        assert abs(cost - ref.cost) <= ref.tol_cost
        assert abs(est - ref.est) <= ref.tol_est
        assert flag == ref.flag
        again = new_block()
        case.call(eng, form, again, sa, ba, sg)
        assert torch.equal(bits(again), bits(block)), "a second call gave other bits"
        if form != "g64" and (sa, ba) == (6e-8, 0.0):
            dflt = new_block()
            case.call_default_entry(eng, form, dflt)
            assert torch.equal(bits(dflt), bits(block)), "nnf_nmf_gram_cost_f32 differs from _cal at (6e-8, 0)"
    assert case.untouched(), "an operand or its padding was written"


def cost_target(case, form, reliable):
    """A cost 8x to either side of the flag's threshold at the LARGEST / smallest estimate the form's figures give, so that
    the verdict of every figure is determined: `reliable` -> flag 0 everywhere, else flag 1 everywhere."""
    ests = [gcr.verdict(case.sums[form], 0.0, sa, ba, sg).est for sa, ba in ROUNDINGS
            for sg in (SIGMA_G64 if form == "g64" else [gcr.SIGMA_G_FP32])]
    return 8 * max(ests) / 5e-4 if reliable else min(ests) / 5e-4 / 8


# ---- A: the kernel against the restatement on the same operands ----------------------------------------------------------------
RANKS_LDS = [1, 15, 16, 17, 33, 64, 100, 128]            # Gram staged in LDS; 128 in fp64 needs 139264 bytes of it
COLS_LDS = [1, 15, 16, 17, 130, 4117]                    # 4117 columns: 258 workgroups, the last one's loop over partials wraps
RANKS_GLOBAL = [129, 160, 200]                           # Gram read where it lies: stride ldg (fp32) / r (fp64)
COLS_GLOBAL = [1, 17, 130]


@pytest.mark.parametrize("n", COLS_LDS)
@pytest.mark.parametrize("r", RANKS_LDS)
@pytest.mark.parametrize("form", FORMS)
def test_kernel_matches_restatement_contiguous(eng, form, r, n):
    case = Case(r, n)
    check_against_restatement(eng, case, form, cost_target(case, form, reliable=(r + n) % 2 == 0))


@pytest.mark.parametrize("n", [17, 4117])
@pytest.mark.parametrize("r", RANKS_LDS)
@pytest.mark.parametrize("form", FORMS)
def test_kernel_matches_restatement_padded(eng, form, r, n):
    case = Case(r, n, padded=True)
    check_against_restatement(eng, case, form, cost_target(case, form, reliable=(r + n) % 2 == 1))


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n", COLS_GLOBAL)
@pytest.mark.parametrize("r", RANKS_GLOBAL)
@pytest.mark.parametrize("form", FORMS)
def test_kernel_matches_restatement_above_rank_128(eng, form, r, n, padded):
    """The Gram read in place: the fp32 form with row stride ldg, the fp64 form with row stride r while UtU is padded, the
    Hadamard product formed per element -- in fp32, rounded once, as below rank 128."""
    case = Case(r, n, padded=padded)
    check_against_restatement(eng, case, form, cost_target(case, form, reliable=(r + n + padded) % 2 == 0))


# ---- B: the verdict ------------------------------------------------------------------------------------------------------------
def run_verdict(eng, case, form, nx):
    case.nx2.fill_(nx)
    ref = gcr.verdict(case.sums[form], nx, 6e-8, 0.0, 5e-9 if form == "g64" else gcr.SIGMA_G_FP32)
    block = new_block()
    case.call(eng, form, block)
    return ref, read_block(block)


@pytest.mark.parametrize("form", FORMS)
def test_verdict(eng, form):
    case = Case(33, 130, padded=True)
    s = case.sums[form]
    terms = float(2 * s.abs_a + s.abs_b)
    # a cost far above the estimate: reliable
    ref, (cost, flag, est) = run_verdict(eng, case, form, float(2 * s.A - s.B) + 1e3 * terms)
    assert ref.est / (5e-4 * ref.cost) < 0.5
    assert flag == 0.0 and ref.flag == 0 and abs(cost - ref.cost) <= ref.tol_cost
    # a cost of 1e-9 of the terms: the fp32 operands do not carry it
    ref, (cost, flag, est) = run_verdict(eng, case, form, float(2 * s.A - s.B) + 1e-9 * terms)
    assert ref.cost > 0 and ref.est / (5e-4 * ref.cost) > 2
    assert flag == 1.0 and ref.flag == 1 and abs(cost - ref.cost) <= ref.tol_cost
    # a negative cost: flagged, and reported as it is
    ref, (cost, flag, est) = run_verdict(eng, case, form, float(2 * s.A - s.B) - terms)
    assert ref.cost < 0 and ref.est / (5e-4 * ref.cost) < 0.5
    assert flag == 1.0 and ref.flag == 1 and cost < 0 and abs(cost - ref.cost) <= ref.tol_cost
    assert abs(est - ref.est) <= ref.tol_est


@pytest.mark.parametrize("form", FORMS)
def test_nan_operand_is_flagged_and_the_ticket_returns(eng, form):
    clean = Case(33, 130, padded=True)
    clean.set_cost(form, cost_target(clean, form, reliable=True))
    first = new_block()
    clean.call(eng, form, first)
    assert read_block(first)[1] == 0.0
    Vn = clean.V.host.copy()
    Vn[20, 77] = np.nan
    bad = Case(33, 130, padded=True, V=Vn)
    bad.nx2.copy_(clean.nx2)
    block = new_block()
    bad.call(eng, form, block)
    cost, flag, est = read_block(block)
    assert math.isnan(cost) and flag == 1.0
    after = new_block()
    clean.call(eng, form, after)
    assert torch.equal(bits(after), bits(first))


# ---- C: the ticket across launches ---------------------------------------------------------------------------------------------
def test_back_to_back_calls_of_different_grids(eng):
    """One counter per context, returned to zero by the kernel: calls of 258, 1, 2, 9 and 258 workgroups in the three forms queued
    on one stream without a synchronisation, a cross product (which takes its partials from the same workspace) in between."""
    r = 33
    plan = [(4117, "fp32"), (1, "had"), (17, "g64"), (130, "fp32"), (4117, "had")]
    cases = []
    for n, form in plan:
        case = Case(r, n, padded=(n != 130))
        case.set_cost(form, cost_target(case, form, reliable=True))
        cases.append(case)
    rng = np.random.RandomState(11)
    X, Ut = torch.from_numpy(rng.rand(3000, 70).astype(np.float32)).cuda(), torch.from_numpy(rng.rand(20, 3000).astype(np.float32)).cuda()
    alone = []
    for case, (n, form) in zip(cases, plan):
        block = new_block()
        case.call(eng, form, block)
        torch.cuda.synchronize()
        alone.append(bits(block))
    xty_alone = bits(eng.xty(X, Ut))
    torch.cuda.synchronize()
    blocks = [new_block() for _ in plan]
    prod = None
    for i, (case, (n, form)) in enumerate(zip(cases, plan)):
        case.call(eng, form, blocks[i])
        if i == 2:
            prod = eng.xty(X, Ut)
    torch.cuda.synchronize()
    for i, block in enumerate(blocks):
        read_block(block)
        assert torch.equal(bits(block), alone[i]), f"call {i} {plan[i]} differs from the same call alone"
    assert torch.equal(bits(prod), xty_alone)


# ---- D: refusals through the C ABI ---------------------------------------------------------------------------------------------
def test_refusals(eng):
    from nn_fac_amd.engine import _ptr
    r, n = 17, 130
    case = Case(r, n, padded=True)
    case.set_cost("fp32", 1.0)
    V, M, G, G2 = case.V.t, case.UtM.t, case.G.t, case.G2.t
    ldv, ldm, ldg = V.stride(0), M.stride(0), G.stride(0)
    block = new_block()
    out, nx, st, lib, ctx = _ptr(block[19:22]), _ptr(case.nx2), eng._stream(), eng.lib, eng.ctx
    nan = float("nan")

    def f32(ldv=ldv, ldm=ldm, ldg=ldg, r=r, n=n, b=None):
        return lib.nnf_nmf_gram_cost_f32(ctx, _ptr(V), ldv, _ptr(M), ldm, _ptr(G), b, ldg, r, n, nx, out, st)

    def cal(sa=6e-8, ba=0.0, ldv=ldv, ldm=ldm, ldg=ldg, r=r, n=n, b=None):
        return lib.nnf_nmf_gram_cost_cal_f32(ctx, _ptr(V), ldv, _ptr(M), ldm, _ptr(G), b, ldg, r, n, nx, sa, ba, out, st)

    def g64(sa=6e-8, ba=0.0, sg=5e-9, ldv=ldv, ldm=ldm, ldg=ldg, r=r, n=n, g=_ptr(case.G64)):
        return lib.nnf_nmf_gram_cost_g64_f32(ctx, _ptr(V), ldv, _ptr(M), ldm, _ptr(G), g, ldg, r, n, nx, sa, ba, sg, out, st)

    refused = {
        "sigma_a = -1": [cal(sa=-1.0), g64(sa=-1.0)],
        "sigma_a = NaN": [cal(sa=nan), g64(sa=nan)],
        "bias_a = -1": [cal(ba=-1.0), g64(ba=-1.0)],
        "bias_a = NaN": [cal(ba=nan)],
        "sigma_g = NaN": [g64(sg=nan)],
        "sigma_g = -1": [g64(sg=-1.0)],
        "ldv < n": [f32(ldv=n - 1), cal(ldv=n - 1), g64(ldv=n - 1)],
        "ldm < n": [f32(ldm=n - 1), cal(ldm=n - 1), g64(ldm=n - 1)],
        "ldg < r": [f32(ldg=r - 1), cal(ldg=r - 1), g64(ldg=r - 1), f32(ldg=r - 1, b=_ptr(G2))],
        "n = 0": [f32(n=0), cal(n=0), g64(n=0)],
        "r = 0": [f32(r=0), cal(r=0), g64(r=0)],
        "g64 without UtU64": [g64(g=None)],
    }
    torch.cuda.synchronize()
    for what, statuses in refused.items():
        assert all(s == NNF_ERR_ARG for s in statuses), (what, statuses)
    assert (block.cpu().numpy() == SENTINEL).all(), "a refused call wrote its output"
    # (and the same arguments, unspoilt, are accepted)
    assert f32() == NNF_OK and cal() == NNF_OK and g64() == NNF_OK and f32(b=_ptr(G2)) == NNF_OK
    assert np.isfinite(read_block(block)).all()


def test_engine_refuses_a_malformed_fp64_gram(eng):
    """Engine.gram_cost hands UtU64 to a kernel that reads r x r doubles with row stride r."""
    from nn_fac_amd.utils.errors import EngineError
    r, n = 17, 33
    case = Case(r, n)
    case.set_cost("g64", 1.0)
    block = new_block()
    out = block[19:22]
    big = torch.zeros((r + 1, r + 1), dtype=torch.float64, device="cuda")
    malformed = {
        "float32": case.G64.float(),
        "a view with a row stride": big[:r, :r],
        "more than r*r elements": big[:, :r].contiguous(),
        "fewer than r*r elements": case.G64[:r - 1].contiguous(),
        "on the host": case.G64.cpu(),
    }
    for what, g in malformed.items():
        with pytest.raises(EngineError):
            eng.gram_cost(case.V.t, case.UtM.t, case.G.t, case.nx2, out, rounding=(6e-8, 0.0, 5e-9), UtU64=g)
    with pytest.raises(EngineError):           # the C refusal no ABI entry can reach: a Hadamard pair and UtU64 together
        eng.gram_cost(case.V.t, case.UtM.t, case.G.t, case.nx2, out, UtU_b=case.G2.t, UtU64=case.G64)
    torch.cuda.synchronize()
    assert (block.cpu().numpy() == SENTINEL).all()
    eng.gram_cost(case.V.t, case.UtM.t, case.G.t, case.nx2, out, rounding=(6e-8, 0.0, 5e-9), UtU64=case.G64.view(-1))
    assert abs(read_block(block)[0] - 1.0) < 1e-6


# ---- E: the identity against the true residual, operands made by the device kernels ---------------------------------------------
worst_e = {"ratio": 0.0}


@pytest.mark.parametrize("noise", gcr.IDENTITY_NOISE)
@pytest.mark.parametrize("m,n,r", gcr.IDENTITY_SHAPES)
def test_identity_on_device_made_operands(eng, m, n, r, noise):
    """U^T X from nnf_xty_f32, U^T U and its fp64 sums from nnf_gram_f64_f32, ||X||^2 from nnf_dot_f32: the cost is inside its own
    estimate of the fp64 residual; at 3 % noise it is reliable and within 5e-4, at an (almost) exact fit it says it is not."""
    U, V, X, want = gcr.identity_case(m, n, r, noise)
    Xd = torch.from_numpy(X).cuda()
    Utd = torch.from_numpy(np.ascontiguousarray(U.T)).cuda()
    Vd = torch.from_numpy(V).cuda()
    UtM = eng.xty(Xd, Utd)
    G64 = torch.empty((r, r), dtype=torch.float64, device="cuda")
    UtU = eng.gram(Utd, out64=G64)
    nx2 = eng.dot(Xd, Xd)
    for form, rounding, g in (("fp32", (6e-8, 0.0), None), ("g64", (6e-8, 0.0, 5e-9), G64)):
        block = new_block()
        eng.gram_cost(Vd, UtM, UtU, nx2, block[19:22], rounding=rounding, UtU64=g)
        cost, flag, est = read_block(block)
        ratio = abs(cost - want) / est
        worst_e["ratio"] = max(worst_e["ratio"], ratio)
        print(f"E {form} m={m} n={n} r={r} noise={noise:g} cost {cost:.9e} want {want:.9e} |cost-want|/est {ratio:.4g} "
              f"est/(5e-4 want) {est / (5e-4 * want):.4g} flag {flag:g} worst so far {worst_e['ratio']:.4g}")
        assert abs(cost - want) <= est          # the kernel's own claim, whatever it says of the cost's use
        if noise == 3e-2:
            assert flag == 0.0
            assert abs(cost - want) <= 5e-4 * want
        else:
            assert flag == 1.0


# ---- F: cross_rounding and gram_rounding ---------------------------------------------------------------------------------------
def block_bounds(m, blocks):
    step = (m + blocks - 1) // blocks
    step = (step + 255) // 256 * 256
    return [(lo, min(m, lo + step)) for lo in range(0, m, step)]


def restated_cross_rounding(eng, X, Ut, blocks):
    full = eng.xty(X, Ut).double().cpu().numpy()
    acc = np.zeros_like(full)
    for lo, hi in block_bounds(X.shape[0], blocks):
        acc += eng.xty(X[lo:hi], Ut[:, lo:hi]).double().cpu().numpy()
    rel = np.zeros_like(full)
    np.divide(full - acc, acc, out=rel, where=acc > 0)
    return math.sqrt(float(np.mean(rel * rel))), abs(float(np.mean(rel))), int((acc <= 0).sum())


def restated_gram_rounding(eng, Ut, blocks):
    r, m = Ut.shape
    full, part = torch.empty((r, r), dtype=torch.float64, device="cuda"), torch.empty((r, r), dtype=torch.float64, device="cuda")
    eng.gram(Ut, out64=full)
    full, acc = full.cpu().numpy(), np.zeros((r, r))
    for lo, hi in block_bounds(m, blocks):
        eng.gram(Ut[:, lo:hi], out64=part)
        acc += part.cpu().numpy()
    rel = np.zeros_like(full)
    np.divide(full - acc, np.abs(acc), out=rel, where=acc != 0)
    return math.sqrt(float(np.mean(rel * rel))), int((acc == 0).sum())


def rounding_operands(m, n=67, r=33):
    rng = np.random.RandomState(m + n + r)
    return torch.from_numpy(rng.rand(m, n).astype(np.float32)).cuda(), torch.from_numpy(rng.rand(r, m).astype(np.float32)).cuda()


def test_block_bounds():
    """The step is a sixteenth of the rows rounded up to 256: ragged last blocks of one row, and a single block."""
    assert block_bounds(256, 16) == [(0, 256)] and block_bounds(5000, 1) == [(0, 5000)]
    assert block_bounds(257, 16) == [(0, 256), (256, 257)]
    assert len(block_bounds(4096, 16)) == 16 and block_bounds(4096, 16)[-1] == (3840, 4096)
    assert len(block_bounds(4097, 16)) == 9 and block_bounds(4097, 16)[-1] == (4096, 4097)
    assert len(block_bounds(5000, 16)) == 10 and block_bounds(5000, 16)[-1] == (4608, 5000)


@pytest.mark.parametrize("m,blocks", [(1, 16), (100, 16), (256, 16), (5000, 1), (257, 1)])
def test_one_block_measures_exactly_zero(eng, m, blocks):
    """One block is the whole product, and the kernels give the same bits on the same operands."""
    X, Ut = rounding_operands(m)
    assert eng.cross_rounding(X, Ut, blocks=blocks) == (0.0, 0.0)
    assert eng.gram_rounding(Ut, blocks=blocks) == 0.0


@pytest.mark.parametrize("m", [257, 4096, 4097, 5000])
def test_rounding_figures_against_host_block_sums(eng, m):
    X, Ut = rounding_operands(m)
    sa, ba = eng.cross_rounding(X, Ut, blocks=16)
    wsa, wba, _ = restated_cross_rounding(eng, X, Ut, 16)
    sg = eng.gram_rounding(Ut, blocks=16)
    wsg, _ = restated_gram_rounding(eng, Ut, 16)
    print(f"F m={m}: cross_rounding ({sa:.6e}, {ba:.6e}) restated ({wsa:.6e}, {wba:.6e}); gram_rounding {sg:.6e} restated {wsg:.6e}")
    assert abs(sa - wsa) <= 1e-12 * wsa and abs(sg - wsg) <= 1e-12 * wsg
    # the mean is a sum of signed terms: 1e-12 of what it is a mean OF (the rms bounds the mean absolute term)
    assert abs(ba - wba) <= 1e-12 * max(wba, wsa)


def test_rounding_figures_with_entries_whose_sum_is_zero(eng):
    """A zero column of X leaves zeros in U^T X, a zero row of U^T zeros in the Gram: counted as 0 error, the figures finite."""
    X, Ut = rounding_operands(5000)
    X[:, 7] = 0.0
    Ut[3, :] = 0.0
    sa, ba = eng.cross_rounding(X, Ut, blocks=16)
    wsa, wba, zeros = restated_cross_rounding(eng, X, Ut, 16)
    assert zeros >= Ut.shape[0]
    sg = eng.gram_rounding(Ut, blocks=16)
    wsg, gzeros = restated_gram_rounding(eng, Ut, 16)
    assert gzeros == 2 * Ut.shape[0] - 1
    assert math.isfinite(sa) and math.isfinite(ba) and math.isfinite(sg) and sa > 0 and sg > 0
    assert abs(sa - wsa) <= 1e-12 * wsa and abs(sg - wsg) <= 1e-12 * wsg and abs(ba - wba) <= 1e-12 * max(wba, wsa)


@pytest.mark.parametrize("m,n,r", [(40000, 64, 16), (70001, 70, 50)])
def test_calibration_covers_the_true_rounding(eng, m, n, r):
    """The figure the NMF driver hands the kernel, max(1.5 sigma_a, 6e-8), is not below the true relative rms error of the
    cross product at this shape (against an fp64 product on the device)."""
    g = torch.Generator(device="cuda").manual_seed(m + n + r)
    X = torch.rand(m, n, device="cuda", generator=g)
    Ut = torch.rand(r, m, device="cuda", generator=g)
    sa, ba = eng.cross_rounding(X, Ut)
    want = Ut.double() @ X.double()
    true_rms = float((((eng.xty(X, Ut).double() - want) / want) ** 2).mean().sqrt())
    print(f"F calibration m={m} n={n} r={r}: cross_rounding sigma_a {sa:.4e} bias_a {ba:.4e}; handed to the kernel "
          f"{max(1.5 * sa, 6e-8):.4e}; true relative rms {true_rms:.4e}")
    assert max(1.5 * sa, 6e-8) >= true_rms


# ---- G: nnf_dot_f32 ------------------------------------------------------------------------------------------------------------
def dot_operand(rng, rows, cols, pad, signed=False):
    a = rng.rand(rows, cols).astype(np.float32) - (0.5 if signed else 0.0)
    return Operand(a, pad)


def check_dot(eng, A, B):
    want, absum = gcr.exact_dot(A.host, B.host)
    got = eng.dot(A.t, B.t)
    again = eng.dot(A.t, B.t)
    tol = 2 * A.host.size * 2.0 ** -53 * absum
    g = float(got)
    print(f"G {A.host.shape} ld {A.t.stride(0)}/{B.t.stride(0)}: got {g:.17g} want {want:.17g} |diff|/tol {abs(g - want) / tol:.3g}")
    assert abs(g - want) <= tol
    assert torch.equal(bits(got), bits(again))
    assert A.untouched() and B.untouched()


@pytest.mark.parametrize("rows,cols,pad_a,pad_b", [(1, 1, 0, 0), (9, 257, 3, 7), (3, 700001, 0, 0), (2049, 1025, 7, 2),
                                                   (3, 700001, 1, 0)])
def test_dot(eng, rows, cols, pad_a, pad_b):
    """One element; padded rows with NaN in the padding; above 2^21 elements (the grid capped at 1024 workgroups, every thread
    striding), contiguous and padded."""
    rng = np.random.RandomState(rows * 31 + cols)
    check_dot(eng, dot_operand(rng, rows, cols, pad_a, signed=True), dot_operand(rng, rows, cols, pad_b))


def test_dot_with_itself(eng):
    A = dot_operand(np.random.RandomState(2), 2049, 1025, 5)
    check_dot(eng, A, A)


def test_dot_with_heavy_cancellation(eng):
    """<[a, a], [b, -b]> = 0 exactly: the bound is on the sum of absolute products, not on the result."""
    rng = np.random.RandomState(4)
    a, b = rng.rand(37, 5000).astype(np.float32) - 0.5, rng.rand(37, 5000).astype(np.float32)
    A, B = Operand(np.hstack([a, a]), 3), Operand(np.hstack([b, -b]), 0)
    assert gcr.exact_dot(A.host, B.host)[0] == 0.0
    check_dot(eng, A, B)

"""Simplex-constrained KL-NMF on the device: the Newton / update kernel through the C ABI (nnf_simplex_proj_kl_f32) against
tests/simplex_restatement.py fed the same fp32 operands, and the drivers against tests/golden/g12_simplex.npz (the real
reference's results).

Tolerances.
  Kernel.  The restatement against itself with the two sums over k of the Newton step in reversed order, on the operands of
  this file (every rank x column count of SHAPES, the planted and the fixture calls, the oscillating columns among them): H
  differs by at most 1.2e-13 relative per entry, lambda by at most 6.2e-14 of max(|lambda|, 1).  That is the floor the order of
  summation sets; the kernel's butterfly order differs from both, so it gets ten times the floor: 1.2e-12 and 6.2e-13.  H_out is
  float32: half an ulp, 2^-24, on top.  Iteration counts are compared exactly.
  Driver.  The restatement run with W, H, C and D rounded to float32 after every update against the fixture, 8 iterations:
  W 2.0e-6 / 2.5e-7 / 3.0e-6 / 8.0e-7, H 4.4e-7 / 3.2e-7 / 3.3e-6 / 1.7e-6 relative Frobenius, cost 6.7e-7 / 1.5e-7 / 6.0e-6 /
  1.5e-6 relative (runs a / b / c / d; the fixture's *_floor).  Ten times the largest, for the fp32 sums inside the fused kernels:
  3.0e-5, 3.4e-5 and 6.1e-5 -- within the MU class of the project (5e-5) times 1.2.
Every entry of every column is compared."""
import ctypes as C
import os
import subprocess
import sys
import warnings
from functools import lru_cache

import numpy as np
import pytest
import torch

import simplex_restatement as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_H = 1.2e-12 + 2.0 ** -24          # relative, per entry (see the head of this file)
TOL_LAMBDA = 6.2e-13                  # of max(|lambda|, 1)
TOL_RUN_W, TOL_RUN_H, TOL_RUN_COST = 3.0e-5, 3.4e-5, 6.1e-5
RANKS = (1, 2, 3, 5, 16, 17, 50, 64, 65, 100, 128)
COLS = (1, 63, 64, 65, 257, 2000)
GROUPS = (1, 4, 16, 64)
NAN = float("nan")


def allowed(r):
    """The lanes per column a rank allows (k_simplex_plan.h; tests/test_simplex_plan.py pins the rule)."""
    return [G for G in GROUPS if -(-r // G) <= 8 and (G == 1 or r > G // 4)]


def r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@lru_cache(maxsize=None)
def operands(r, cols, seed, m=24):
    """(H, C, den_vec) of a KL step, rounded to float32: H on the simplex, C = W^T(X / WH), D = W^T 1."""
    rng = np.random.RandomState(seed)
    W = rng.rand(m, r) + 0.05
    Ht = rng.rand(r, cols)
    Ht /= Ht.sum(axis=0)
    X = W @ Ht + 0.01 * rng.rand(m, cols)
    H = rng.rand(r, cols) + 0.05
    H /= H.sum(axis=0)
    Cm, D = rs.simplex_operands(X, W, H)
    return r32(H), r32(Cm), r32(D[:, 0])


def restated(H, Cm, D, lam0=None, tol=1e-6, max_iter=100):
    """(H_out, lambda, count, last step) of the restatement on these operands."""
    info = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lam = rs.update_lagragian_multipliers_simplex_projection(Cm, D, H, 1, rs.lambda_start(Cm, D, H) if lam0 is None else
                                                                 np.asarray(lam0).reshape(-1, 1), tol=tol, n_iter_max=max_iter, info=info)
    return rs.simplex_update(Cm, D, H, lam), lam.ravel(), info["count"], info["deltas"][-1], info


@lru_cache(maxsize=None)
def reference(r, cols, seed):
    H, Cm, dv = operands(r, cols, seed)
    return restated(H, Cm, dv[:, None] * np.ones_like(H))


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd import engine
    return engine.get_engine(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def g12(golden):
    return golden("g12_simplex.npz")


def padded(a, pad):
    """A device float32 r x cols view of a NaN-filled r x (cols + pad) buffer."""
    r, cols = a.shape
    buf = torch.full((r, cols + pad), NAN, dtype=torch.float32, device="cuda")
    buf[:, :cols] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return buf


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Call:
    """One call of nnf_simplex_proj_kl_f32 on padded, NaN-framed buffers; the outputs are NaN-filled beforehand."""

    def __init__(self, eng, H, Cm, den=None, den_vec=None, lam0=None, tol=1e-6, max_iter=100, pad=3, alias=False, want_H=True,
                 want_lam=True, r_arg=None, ldh=None):
        r, cols = H.shape
        self.r, self.cols = r, cols
        self.Hb, self.Cb = padded(H, pad), padded(Cm, pad)
        self.Db = padded(den, pad) if den is not None else None
        self.dv = torch.from_numpy(np.ascontiguousarray(den_vec, dtype=np.float64)).cuda() if den_vec is not None else None
        self.l0 = torch.from_numpy(np.ascontiguousarray(lam0, dtype=np.float64).reshape(-1)).cuda() if lam0 is not None else None
        self.Ob = self.Hb if alias else (torch.full((r, cols + pad + 2), NAN, dtype=torch.float32, device="cuda") if want_H else None)
        self.lam = torch.full((cols,), NAN, dtype=torch.float64, device="cuda") if want_lam else None
        self.st = torch.full((2,), NAN, dtype=torch.float64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.rc = eng.lib.nnf_simplex_proj_kl_f32(
            eng.ctx, ptr(self.Hb), self.Hb.stride(0) if ldh is None else ldh, r if r_arg is None else r_arg, cols, ptr(self.Cb),
            self.Cb.stride(0), ptr(self.Db), self.Db.stride(0) if self.Db is not None else 0, ptr(self.dv), ptr(self.l0), float(tol),
            int(max_iter), ptr(self.Ob), self.Ob.stride(0) if self.Ob is not None else 0, ptr(self.lam), ptr(self.st), st)
        torch.cuda.synchronize()

    def H_out(self):
        out = self.Ob.cpu().numpy()
        assert np.isnan(out[:, self.cols:]).all(), "H_out: the padding was written"
        if self.Ob is not self.Hb:
            assert np.isnan(self.Hb.cpu().numpy()[:, self.cols:]).all()
        return out[:, :self.cols]

    def lam_out(self):
        return self.lam.cpu().numpy()

    def status(self):
        return self.st.cpu().numpy()


def check_H(got, want, tag):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(want).all(), tag
    err = np.abs(got - want) / np.abs(want)
    assert np.isfinite(got).all() and err.max() <= TOL_H, (tag, float(err.max()), np.unravel_index(np.argmax(err), err.shape))


def check_lam(got, want, tag):
    err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
    assert np.isfinite(got).all() and err.max() <= TOL_LAMBDA, (tag, float(err.max()), int(np.argmax(err)))


def check_last(got, want, lam, tag):
    """The last step is a difference of two multipliers, each within TOL_LAMBDA of the restatement's."""
    assert abs(got - want) <= 2 * TOL_LAMBDA * max(1.0, float(np.max(np.abs(lam)))), (tag, got, want)


def forces(r):
    return [None] + allowed(r)


def set_force(monkeypatch, G):
    if G is None:
        monkeypatch.delenv("NNF_SIMPLEX_FORCE", raising=False)
    else:
        monkeypatch.setenv("NNF_SIMPLEX_FORCE", str(G))


# ---- shapes and plans -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RANKS)
def test_every_shape_under_every_plan(eng, monkeypatch, r):
    """Every rank x column count, unforced and under every G the rank allows, den_vec and den matrix forms (bitwise equal: the
    per-row denominator is representable in float32), against the restatement on the same fp32 operands."""
    for cols in COLS:
        H, Cm, dv = operands(r, cols, 1000 * r + cols)
        want_H, want_lam, want_count, want_last, _ = reference(r, cols, 1000 * r + cols)
        D = dv[:, None] * np.ones_like(H)
        for G in forces(r):
            set_force(monkeypatch, G)
            tag = (r, cols, G)
            vec = Call(eng, H, Cm, den_vec=dv)
            mat = Call(eng, H, Cm, den=D, pad=5)
            assert vec.rc == 0 and mat.rc == 0, tag
            for c in (vec, mat):
                st = c.status()
                assert st[0] == want_count, (tag, st, want_count)
                check_last(st[1], want_last, want_lam, tag)
                check_lam(c.lam_out(), want_lam, tag)
                check_H(c.H_out(), want_H, tag)
            assert np.array_equal(vec.H_out(), mat.H_out()) and np.array_equal(vec.lam_out(), mat.lam_out()), tag
            assert np.array_equal(vec.status(), mat.status()), tag


def test_more_workgroups_than_one_resident_round(eng, monkeypatch):
    """5 x 70001: under G = 16 that is 4376 workgroups of 16 columns."""
    r, cols = 5, 70001
    H, Cm, dv = operands(r, cols, 99)
    want_H, want_lam, want_count, _, _ = reference(r, cols, 99)
    for G in forces(r):
        set_force(monkeypatch, G)
        c = Call(eng, H, Cm, den_vec=dv)
        assert c.rc == 0 and c.status()[0] == want_count, (G, c.status(), want_count)
        check_lam(c.lam_out(), want_lam, G)
        check_H(c.H_out(), want_H, G)


def test_plan_line_under_plan_debug(built_lib):
    """NNF_PLAN_DEBUG: one "[nnf plan] simplex" line per call, naming the plan tools/nnf_plan.cpp gives for this device."""
    from test_mu_plan_table import ask
    child = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_simplex as t\n"
             "from nn_fac_amd import engine; e = engine.get_engine(torch.device('cuda:0'))\n"
             "print('cus', torch.cuda.get_device_properties(0).multi_processor_count)\n"
             "for r, cols in ((50, 2000), (5, 70001), (17, 257)):\n"
             "    H, Cm, dv = t.operands(r, cols, 5)\n"
             "    assert t.Call(e, H, Cm, den_vec=dv).rc == 0\n"
             "print('done')\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, NNF_PLAN_DEBUG="1")
    env.pop("NNF_SIMPLEX_FORCE", None)
    p = subprocess.run([sys.executable, "-c", child], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    cus = int(p.stdout.split("cus")[1].split()[0])
    lines = [ln for ln in p.stderr.splitlines() if ln.startswith("[nnf plan] simplex ")]
    assert len(lines) == 3, p.stderr[-3000:]
    want = ask(["simplex %d r=%d cols=%d" % (cus, r, cols) for r, cols in ((50, 2000), (5, 70001), (17, 257))])
    for ln, w in zip(lines, want):
        got = dict(kv.split("=", 1) for kv in ln.split()[3:])
        assert {k: str(v) for k, v in w.items()} == got, (ln, w)


# ---- buffer hygiene ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,cols", ((5, 257), (50, 65), (128, 63)))
def test_buffer_hygiene(eng, monkeypatch, r, cols):
    H, Cm, dv = operands(r, cols, 1000 * r + cols)
    for G in forces(r):
        set_force(monkeypatch, G)
        a, b = Call(eng, H, Cm, den_vec=dv), Call(eng, H, Cm, den_vec=dv, pad=8)
        assert a.rc == 0 and b.rc == 0
        # two calls are bitwise equal, whatever the pitches
        assert np.array_equal(a.H_out(), b.H_out()) and np.array_equal(a.lam_out(), b.lam_out()) and np.array_equal(a.status(), b.status())
        # H_out aliasing H gives the same bits as a separate H_out
        al = Call(eng, H, Cm, den_vec=dv, alias=True)
        assert al.rc == 0 and np.array_equal(al.H_out(), a.H_out()) and np.array_equal(al.lam_out(), a.lam_out())
        # H_out = NULL with lambda_out gives the same multipliers; lambda_out = NULL gives the same H
        only_lam = Call(eng, H, Cm, den_vec=dv, want_H=False)
        only_H = Call(eng, H, Cm, den_vec=dv, want_lam=False)
        assert only_lam.rc == 0 and np.array_equal(only_lam.lam_out(), a.lam_out()) and np.array_equal(only_lam.status(), a.status())
        assert only_H.rc == 0 and np.array_equal(only_H.H_out(), a.H_out())
        # the inputs are not written
        assert np.array_equal(a.Hb.cpu().numpy()[:, :cols], H.astype(np.float32)) and np.array_equal(a.Cb.cpu().numpy()[:, :cols], Cm.astype(np.float32))


def test_lambda0_given_reproduces_the_multiplier_fixture(eng, monkeypatch, g12):
    """The matrix form with start values given -- what utils.normalize_wh.update_lagragian_multipliers_simplex_projection calls --
    on the fixture's converging call: the reference's multipliers and its iteration count."""
    Cm, D, H = (g12["m_" + k].astype(np.float64) for k in "CDH")
    for G in forces(H.shape[0]):
        set_force(monkeypatch, G)
        c = Call(eng, H, Cm, den=D, lam0=g12["m_lam0"], want_H=False)
        assert c.rc == 0 and c.status()[0] == int(g12["m_count"]) and c.status()[1] <= 1e-6
        check_lam(c.lam_out(), g12["m_lam"], G)
    from nn_fac_amd.utils.normalize_wh import update_lagragian_multipliers_simplex_projection
    monkeypatch.delenv("NNF_SIMPLEX_FORCE", raising=False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        lam = update_lagragian_multipliers_simplex_projection(Cm, D, H, 1, g12["m_lam0"].reshape(-1, 1))
    assert not w and isinstance(lam, np.ndarray) and lam.shape == (H.shape[1], 1) and lam.dtype == np.float64
    check_lam(lam.ravel(), g12["m_lam"], "python")


# ---- the global stop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,cols,seed,gap,tol", ((5, 300, 7, 1e-5, 1e-6), (5, 300, 7, 1e-5, 5e-3), (50, 130, 8, 1e-4, 1e-6)))
def test_one_slow_column_sets_the_count_for_all(eng, monkeypatch, r, cols, seed, gap, tol):
    """One planted column starts just below its first pole and needs many more iterations than the rest; all columns stop
    together: the count is the restatement's exactly, and the fast columns hold their values after that many iterations."""
    H, Cm, dv = operands(r, cols, seed)
    D = dv[:, None] * np.ones_like(H)
    lam0 = rs.lambda_start(Cm, D, H).ravel()
    _, _, plain_count, _, _ = restated(H, Cm, D, lam0, tol=tol)
    j = cols // 2
    lam0[j] = D[:, j].min() - gap
    want_H, want_lam, T, _, info = restated(H, Cm, D, lam0, tol=tol)
    # the comparison of counts is honest only if the stopping iteration is clear of the tolerance on both sides
    assert T >= plain_count + 4 and info["deltas"][T - 2] >= 10 * tol and info["deltas"][T - 1] <= tol / 10, (T, info["deltas"][-3:])
    for G in forces(r):
        set_force(monkeypatch, G)
        for kw in (dict(den_vec=dv), dict(den=D)):
            c = Call(eng, H, Cm, lam0=lam0, tol=tol, **kw)
            assert c.rc == 0 and c.status()[0] == T, (G, c.status(), T)
            check_lam(c.lam_out(), want_lam, G)
            check_H(c.H_out(), want_H, G)
    if tol > 1e-4:
        # with a loose tolerance a column stopped at its own convergence would sit measurably elsewhere
        own = np.array([restated(H[:, [i]], Cm[:, [i]], D[:, [i]], lam0[[i]], tol=tol)[1][0] for i in range(0, cols, 7) if i != j])
        glob = np.array([want_lam[i] for i in range(0, cols, 7) if i != j])
        assert np.max(np.abs(own - glob) / np.maximum(np.abs(glob), 1.0)) > 1e3 * TOL_LAMBDA


# ---- non-convergence --------------------------------------------------------------------------------------------------
def test_the_call_that_never_converges(eng, monkeypatch, g12):
    """The fixture's 100-iteration call (the second step of run a: a few columns oscillate by 1e8)."""
    Cm, D, H = (g12["n_" + k].astype(np.float64) for k in "CDH")
    lam0 = g12["n_lam0"]
    assert int(g12["n_count"]) == 100 and float(g12["n_last"]) > 1e-6
    for G in forces(H.shape[0]):
        set_force(monkeypatch, G)
        for max_iter in (100, 7, 1):
            want_H, want_lam, count, last, _ = restated(H, Cm, D, lam0, max_iter=max_iter)
            assert count == max_iter and last > 1e-6
            c = Call(eng, H, Cm, den=D, lam0=lam0, max_iter=max_iter)
            st = c.status()
            assert c.rc == 0 and st[0] == max_iter and st[1] > 1e-6, (G, max_iter, st, last)
            check_last(st[1], last, want_lam, (G, max_iter))
            check_lam(c.lam_out(), want_lam, (G, max_iter))
            check_H(c.H_out(), want_H, (G, max_iter))
            if max_iter == 100:
                check_lam(c.lam_out(), g12["n_lam"], (G, "fixture"))
                # the reference's start values are the default ones
                d = Call(eng, H, Cm, den=D)
                assert np.array_equal(d.lam_out(), c.lam_out()) and np.array_equal(d.H_out(), c.H_out())


def test_exactly_one_warning_through_python(eng, monkeypatch, g12):
    from nn_fac_amd.utils.normalize_wh import update_lagragian_multipliers_simplex_projection
    from nn_fac_amd.update_rules.mu import simplex_proj_mu
    monkeypatch.delenv("NNF_SIMPLEX_FORCE", raising=False)
    Cm, D, H = (g12["n_" + k].astype(np.float64) for k in "CDH")
    keep = (Cm.copy(), D.copy(), H.copy())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        lam = update_lagragian_multipliers_simplex_projection(Cm, D, H, 1, g12["n_lam0"].reshape(-1, 1))
    assert [str(x.message) for x in w] == [rs.WARNING]
    check_lam(lam.ravel(), g12["n_lam"], "python")
    assert all(np.array_equal(a, b) for a, b in zip(keep, (Cm, D, H)))
    # simplex_proj_mu: p0 runs out of iterations in the reference (one warning), p1 and p2 converge (none)
    for name in ("p0", "p1", "p2"):
        X, W, Hp = (g12[f"{name}_{k}"].astype(np.float64) for k in "XWH")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = simplex_proj_mu(X, W, Hp, 1)
        assert [str(x.message) for x in w] == ([rs.WARNING] if bool(g12[name + "_warned"]) else []), name
        assert isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == Hp.shape
        want = g12[name + "_out"]
        assert np.linalg.norm(out - want) <= TOL_RUN_H * np.linalg.norm(want), (name, np.linalg.norm(out - want) / np.linalg.norm(want))


# ---- NaN ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,cols", ((5, 257), (50, 130)))
def test_nan_is_kept(eng, monkeypatch, r, cols):
    """One NaN in num: that column is NaN, the call runs all max_iter iterations (np.max of a NaN fails <= tol), and every other
    column is what the restatement gives after max_iter iterations."""
    H, Cm, dv = operands(r, cols, 1000 * r + cols)
    D = dv[:, None] * np.ones_like(H)
    j, k = cols // 3, r // 2
    bad = Cm.copy()
    bad[k, j] = NAN
    for max_iter in (100, 9):
        want_H, want_lam, count, _, _ = restated(H, Cm, D, tol=-1.0, max_iter=max_iter)      # (tol < 0: all max_iter iterations)
        assert count == max_iter
        for G in forces(r):
            set_force(monkeypatch, G)
            c = Call(eng, H, bad, den_vec=dv, max_iter=max_iter)
            st, got_H, got_lam = c.status(), c.H_out(), c.lam_out()
            assert c.rc == 0 and st[0] == max_iter and np.isnan(st[1]), (G, st)
            assert np.isnan(got_H[:, j]).all() and np.isnan(got_lam[j]), G
            others = np.arange(cols) != j
            check_lam(got_lam[others], want_lam[others], G)
            check_H(got_H[:, others], want_H[:, others], G)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(eng, monkeypatch):
    monkeypatch.delenv("NNF_SIMPLEX_FORCE", raising=False)
    H, Cm, dv = operands(5, 65, 5065)
    D = dv[:, None] * np.ones_like(H)
    H129 = np.ones((129, 4))

    def untouched(c):
        return np.isnan(c.Ob.cpu().numpy()).all() and np.isnan(c.lam.cpu().numpy()).all() and np.isnan(c.status()).all()
    cases = [(-3, Call(eng, H129, H129, den_vec=np.ones(129))),               # rank above 128
             (-3, Call(eng, H, Cm, den_vec=dv, max_iter=0)), (-3, Call(eng, H, Cm, den_vec=dv, max_iter=1025)),
             (-1, Call(eng, H, Cm, den_vec=dv, den=D)), (-1, Call(eng, H, Cm)),    # both, neither
             (-1, Call(eng, H, Cm, den_vec=dv, r_arg=0)), (-1, Call(eng, H, Cm, den_vec=dv, ldh=64))]
    for want, c in cases:
        assert c.rc == want and untouched(c), (want, c.rc)
    monkeypatch.setenv("NNF_SIMPLEX_FORCE", "64")      # a group the rank does not allow; a value that is none of the four
    c = Call(eng, H, Cm, den_vec=dv)
    assert c.rc == -3 and untouched(c)
    monkeypatch.setenv("NNF_SIMPLEX_FORCE", "3")
    c = Call(eng, H, Cm, den_vec=dv)
    assert c.rc == -1 and untouched(c)
    monkeypatch.delenv("NNF_SIMPLEX_FORCE")
    # a context whose workspace cannot hold the slots
    from nn_fac_amd import engine
    small = engine.Engine(torch.device("cuda:0"), workspace_bytes=512)
    if small.lib.nnf_ctx_workspace_bytes(small.ctx) < 808:
        c = Call(small, H, Cm, den_vec=dv)
        assert c.rc == -4 and untouched(c)
    ok = Call(eng, H, Cm, den_vec=dv, max_iter=1024)
    assert ok.rc == 0 and ok.status()[0] == reference(5, 65, 5065)[2]
    from nn_fac_amd.utils.errors import EngineError
    with pytest.raises(EngineError):
        eng.simplex_proj(torch.ones((5, 8), device="cuda"), torch.ones((5, 8), device="cuda"), None, None)


# ---- the drivers --------------------------------------------------------------------------------------------------------
def rel_fro(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name,as_tensor", (("a", False), ("a", True), ("c", False), ("d", False), ("d", True)))
def test_driver_against_the_fixture(eng, monkeypatch, g12, name, as_tensor):
    """compute_simplex_beta_nmf from the fixture's starts, 8 iterations: 100 x 200 r5 and 130 x 97 r50 (the cost rides on the next
    W update), 90 x 130 r100 (the cost is a pass of its own).  Factors, every cost, the iteration count and the warnings."""
    from nn_fac_amd.simplex_nmf import compute_simplex_beta_nmf
    monkeypatch.delenv("NNF_SIMPLEX_FORCE", raising=False)
    X, W0, H0 = (g12[f"{name}_{k}"].astype(np.float64) for k in ("X", "W0", "H0"))
    r = int(g12[name + "_rank"])
    if as_tensor:
        args = [torch.from_numpy(a.astype(np.float32)).cuda() for a in (X, W0, H0)]
        keep = [a.clone() for a in args]
    else:
        args = [X, W0, H0]
        keep = [a.copy() for a in args]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        W, H, costs, toc = compute_simplex_beta_nmf(args[0], args[1], args[2], r, 1, n_iter_max=8, tol=0)
    assert all((torch.equal(a, b) if as_tensor else np.array_equal(a, b)) for a, b in zip(keep, args))
    if as_tensor:
        assert W.is_cuda and H.is_cuda and W.dtype == torch.float32
        W, H = W.cpu().numpy(), H.cpu().numpy()
    else:
        assert isinstance(W, np.ndarray) and W.dtype == np.float64 and H.dtype == np.float64
    assert W.shape == W0.shape and H.shape == H0.shape and len(costs) == len(toc) == 8
    got = (rel_fro(W, g12[name + "_W"]), rel_fro(H, g12[name + "_H"]), float(np.max(np.abs(np.array(costs) - g12[name + "_costs"]) / g12[name + "_costs"])))
    print(name, "rel_fro(W), rel_fro(H), max rel cost:", got)
    assert got[0] <= TOL_RUN_W and got[1] <= TOL_RUN_H and got[2] <= TOL_RUN_COST, got
    assert [str(x.message) for x in w] == [rs.WARNING] * int(g12[name + "_warned"].sum())
    assert np.max(np.abs(H.sum(axis=0) - 1)) <= 1e-5


def test_column_sums_from_iteration_3_on(eng, monkeypatch, g12):
    """From iteration 3 on (the reference's 0-based loop variable) the columns of H sum to 1 within 1e-5, on the three runs."""
    from nn_fac_amd.simplex_nmf import one_step_simplex_beta_nmf
    monkeypatch.delenv("NNF_SIMPLEX_FORCE", raising=False)
    for name in ("a", "c", "d"):
        X, W, H = (g12[f"{name}_{k}"].astype(np.float64) for k in ("X", "W0", "H0"))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for it in range(8):
                W, H, cost = one_step_simplex_beta_nmf(X, W, H, int(g12[name + "_rank"]), 1, 1e-6)
                assert abs(cost - g12[name + "_costs"][it]) <= TOL_RUN_COST * g12[name + "_costs"][it], (name, it)
                if it >= 3:
                    assert np.max(np.abs(H.sum(axis=0) - 1)) <= 1e-5, (name, it)


def test_early_stop_and_the_reference_s_example(eng, monkeypatch, g12):
    """tol = 400 lies a factor 10 below |cost 2 - cost 3| (3992) and 12 above |cost 3 - cost 4| (33) of run a: the loop stops
    at iteration 4 with five costs and that iteration's factors; the iterations enqueued behind it are dropped."""
    from nn_fac_amd.simplex_nmf import compute_simplex_beta_nmf, simplex_beta_nmf
    monkeypatch.delenv("NNF_SIMPLEX_FORCE", raising=False)
    d = np.abs(np.diff(g12["a_costs"]))
    assert (d[:3] > 4000 * 0.99).all() and d[3] < 40
    X, W0, H0 = (g12[f"a_{k}"].astype(np.float64) for k in ("X", "W0", "H0"))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        W, H, costs, toc = simplex_beta_nmf(X, 5, 1, n_iter_max=8, tol=400.0, init="custom", W_0=W0, H_0=H0)
    assert len(costs) == len(toc) == 5 and len(w) == int(g12["a_warned"][:5].sum())
    assert np.max(np.abs(np.array(costs) - g12["a_costs"][:5]) / g12["a_costs"][:5]) <= TOL_RUN_COST
    assert rel_fro(W, g12["a_W_it4"]) <= TOL_RUN_W and rel_fro(H, g12["a_H_it4"]) <= TOL_RUN_H
    # simplex_nmf.py:73-79, the reference's own example
    np.random.seed(42)
    m, n, rank = 100, 200, 5
    W_0, H_0 = np.random.rand(m, rank), np.random.rand(rank, n)
    data = W_0 @ H_0 + 1e-2 * np.random.rand(m, n)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        W, H, lossfun, t = simplex_beta_nmf(data, rank, beta=1, n_iter_max=100, deterministic=True, seed=42)
    assert W.shape == (m, rank) and H.shape == (rank, n) and 2 <= len(lossfun) == len(t) <= 100
    assert np.isfinite(lossfun).all() and lossfun[-1] < lossfun[0] and np.max(np.abs(H.sum(axis=0) - 1)) <= 1e-5

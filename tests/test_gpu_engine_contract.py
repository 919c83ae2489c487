"""GPU contract: the engine double (tests/engine_double.OracleEngine, fp64 on the CPU) against the HIP engine it stands in for.

The gloo world-size-2 suite and bench.py's multi-rank launch test run the row-sharded protocol on the double, so they are only as
good as its agreement with nn_fac_amd.engine.Engine.  Every public method of the double has at least one case in CONTRACT below
(tests/test_abi_and_host.py checks that on the CPU): both engines are called on the same fp32-rounded inputs -- the double on
fp64 copies -- and the test compares the returned values, the in-place effects and WHICH arguments the call changes.

Bounds (u = 2^-24, the fp32 unit roundoff):
  - exact: status words and control flow (hals_stop_restore); the Hadamard product and the fill value 1/sqrt(ncols_total) of
    hals_row_scale equal the fp32 rounding of the double's fp64 value;
  - hals_row_update: per entry |dV| <= 2 ((r+3) u (|UtU[k]| |V| + |UtM[k]| + sp) / UtU[k,k] + 2u |V_new[k]|)  (an fp32 FMA chain of
    length r, the subtraction, the reciprocal and the add); the two sums get the Cauchy-Schwarz image of that bound;
  - hals_row_scale: one fp32 rounding of an fp64 quotient, |dv| <= 2u |v|;
  - everything else: the existing suite's relative Frobenius bounds for that kernel (1e-5 for products / costs, 2e-5 MU
    updates, 1e-4 on V and 5e-3 on the sweep sums for HALS sweeps and solves).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from engine_double import OracleEngine  # noqa: E402

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24


class Pad:
    """An fp32 matrix passed as a view [:, :cols] of a wider buffer whose padding columns hold NaN."""

    def __init__(self, a, pad=5):
        self.a, self.pad = np.asarray(a, dtype=np.float32), pad


def _to(x, device):
    """numpy float32 -> fp32 on the GPU / fp64 on the CPU; numpy float64 stays fp64 on both; lists recurse."""
    if isinstance(x, list):
        return [_to(v, device) for v in x]
    if isinstance(x, Pad):
        r, c = x.a.shape
        dt = torch.float32 if device == "cuda" else torch.float64
        buf = torch.full((r, c + x.pad), float("nan"), dtype=dt, device=device)
        buf[:, :c] = torch.from_numpy(x.a.astype(np.float64)).to(dt)
        v = buf[:, :c]
        v._pad_buffer = buf
        return v
    if isinstance(x, np.ndarray):
        if x.dtype == np.float64:
            return torch.from_numpy(x.copy()).to(device)
        t = torch.from_numpy(x.astype(np.float64))
        return t.to(device=device, dtype=torch.float32).contiguous() if device == "cuda" else t.contiguous()
    return x


def _tensors(args):
    out = []
    for i, a in enumerate(args):
        if isinstance(a, list):
            out += [((i, j), t) for j, t in enumerate(a) if torch.is_tensor(t)]
        elif torch.is_tensor(a):
            out.append(((i,), a))
    return out


def _snap(t):
    return t.detach().to("cpu", torch.float64).clone()


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(torch.nan_to_num(a, nan=-7.25e300), torch.nan_to_num(b, nan=-7.25e300)))


def _np(x):
    if x is None:
        return None
    if isinstance(x, (tuple, list)):
        return [_np(v) for v in x]
    return x.detach().to("cpu", torch.float64).numpy()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def call_both(eng, method, args, kwargs=None):
    """Calls `method` on the HIP engine and on the double with the same inputs.  Returns, per engine, (returned value, the
    tensor arguments after the call, the positions of the arguments the call changed, the device-side args)."""
    kwargs = kwargs or {}
    res = []
    for e, device in ((eng, "cuda"), (OracleEngine(), "cpu")):
        a = [_to(x, device) for x in args]
        kw = {k: _to(v, device) for k, v in kwargs.items()}
        before = {pos: _snap(t) for pos, t in _tensors(a)}
        ret = getattr(e, method)(*a, **kw)
        if device == "cuda":
            torch.cuda.synchronize()
        after = {pos: _snap(t) for pos, t in _tensors(a)}
        changed = sorted(pos for pos in before if not _same(before[pos], after[pos]))
        res.append((_np(ret), {p: v.numpy() for p, v in after.items()}, changed, a))
    (gr, ga, gc, gargs), (wr, wa, wc, _) = res
    assert gc == wc, f"{method}: the HIP engine changes arguments {gc}, the double {wc}"
    for _, t in _tensors(gargs):                     # padded views: nothing written outside the view
        buf = getattr(t, "_pad_buffer", None)
        if buf is not None:
            assert torch.isnan(buf[:, t.shape[1]:]).all(), f"{method}: wrote into the padding of a view"
    return gr, wr, ga, wa, gc


def check_rel(got, want, tol, what):
    if isinstance(want, list):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            check_rel(g, w, tol, f"{what}[{i}]")
        return
    if want is None:
        assert got is None, what
        return
    got, want = np.asarray(got, np.float64).reshape(np.shape(want)), np.asarray(want, np.float64)
    assert np.isfinite(got).all(), what
    if tol == "round32":                              # one fp32 rounding of an exact fp64 value
        assert np.array_equal(got, want.astype(np.float32).astype(np.float64)), what
        return
    assert _rel(got, want) <= tol, (what, _rel(got, want))


def plain(method, tol, build):
    """A case whose returned value and changed arguments agree to the relative Frobenius bound `tol`."""
    def run(eng):
        args, kwargs = build(np.random.RandomState(len(method) + 7))
        gr, wr, ga, wa, changed = call_both(eng, method, args, kwargs)
        check_rel(gr, wr, tol, f"{method} result")
        for pos in changed:
            check_rel(ga[pos], wa[pos], tol, f"{method} argument {pos}")
    return run


def f32(*shape, rng, lo=0.05):
    return (rng.rand(*shape) + lo).astype(np.float32)


# ---- hals_row_update / hals_row_scale / hals_stop_restore: the device half of the row-sharded protocol (dist.py) -------------
def row_update_case(r, ncols, k, sparsity="none", zero_diag=False, pad=False, seed=0):
    def run(eng):
        rng = np.random.RandomState(seed + 31 * r + k)
        A = rng.rand(3 * r + 5, r)
        UtU = (A.T @ A).astype(np.float32)
        if zero_diag:
            UtU[k, :] = 0.0
            UtU[:, k] = 0.0
        UtM = (UtU.astype(np.float64) @ rng.rand(r, ncols) * 1.1).astype(np.float32)
        V = f32(r, ncols, rng=rng, lo=0.0)
        kwargs = {} if sparsity == "none" else {"sparsity": sparsity}
        gr, wr, ga, wa, changed = call_both(eng, "hals_row_update", [UtM, UtU, Pad(V) if pad else V, k], kwargs)
        sp = 0.0 if sparsity in ("none", None) else float(sparsity)
        d = float(UtU[k, k])
        Vn = wa[(2,)]
        if zero_diag:
            assert changed == [], changed                  # nnls.py:160: the row is left alone ...
            assert gr[0] == 0.0 and abs(gr[1] - wr[1]) <= 4 * U32 * wr[1]      # ... but its sum of squares is still reported
            return
        assert changed == [(2,)]
        V64 = V.astype(np.float64)
        bound = 2 * ((r + 3) * U32 * (np.abs(UtU[k].astype(np.float64)) @ V64 + np.abs(UtM[k]) + sp) / d + 2 * U32 * np.abs(Vn[k]))
        err = np.abs(ga[(2,)] - Vn)
        assert (err[k] <= bound).all(), float((err[k] / bound).max())
        assert (err[np.arange(r) != k] == 0).all()         # the other rows are not touched
        e2 = float(np.linalg.norm(bound))                  # | ||a||^2 - ||b||^2 | <= (2 ||b|| + ||a - b||) ||a - b||
        assert abs(gr[0] - wr[0]) <= 2 * math.sqrt(wr[0]) * e2 + e2 * e2
        assert abs(gr[1] - wr[1]) <= 2 * math.sqrt(wr[1]) * e2 + e2 * e2 + 4 * U32 * wr[1]
    return run


def row_scale_case(r, ncols, k, normsq, ncols_total, pad=False):
    def run(eng):
        rng = np.random.RandomState(ncols + k)
        V = f32(r, ncols, rng=rng)
        gr, wr, ga, wa, changed = call_both(eng, "hals_row_scale", [Pad(V) if pad else V, k, np.array([normsq]), ncols_total])
        assert changed == [(0,)]
        got, want = ga[(0,)], wa[(0,)]
        assert (got[np.arange(r) != k] == V[np.arange(r) != k]).all()
        if normsq == 0.0:
            assert (got[k] == np.float32(1.0 / math.sqrt(ncols_total))).all()      # exactly the rounded fill value
            assert (want[k] == 1.0 / math.sqrt(ncols_total)).all()
        else:
            assert (np.abs(got[k] - want[k]) <= 2 * U32 * np.abs(want[k])).all()
    return run


def stop_restore_case(sums, head, budget, delta=0.01, snapshots=True, r=3, ncols=257, pad=False):
    """sums: the all-reduced per-sweep sums of a blind chunk; snapshots: blocks for sweeps head .. nsweeps-1."""
    def run(eng):
        rng = np.random.RandomState(len(sums) * 10 + head)
        V = f32(r, ncols, rng=rng)
        n = len(sums)
        snaps = rng.rand(n - head, r, ncols).astype(np.float32) if snapshots else None
        status = np.full(8, -5.0)
        gr, wr, ga, wa, changed = call_both(eng, "hals_stop_restore",
                                            [np.asarray(sums, dtype=np.float64), head, budget, delta, Pad(V) if pad else V,
                                             snaps, status])
        assert np.array_equal(ga[(6,)][:4], wa[(6,)][:4], equal_nan=True), (ga[(6,)], wa[(6,)])   # status words: exact
        assert np.array_equal(ga[(4,)], wa[(4,)])                                                 # V: exact
        assert (0,) not in changed and (5,) not in changed
    return run


NSW = [1.0, 0.5, 0.2, 0.05, 0.004, 0.001]        # delta = 0.01: the rule stops at sweep 4 (0.004 < 0.01 * 1.0)

CONTRACT = {
    "hals_row_update": {
        "plain_k0": row_update_case(8, 300, 0),
        "last_row": row_update_case(8, 300, 7),
        "zero_diagonal": row_update_case(6, 300, 2, zero_diag=True),
        "sparsity_none": row_update_case(5, 257, 1, sparsity=None),
        "sparsity_zero": row_update_case(5, 257, 1, sparsity=0.0),
        "sparsity": row_update_case(5, 257, 3, sparsity=0.3),
        "ncols1": row_update_case(4, 1, 1),
        "ncols255": row_update_case(4, 255, 3),
        "ncols256": row_update_case(4, 256, 0),
        "ncols257": row_update_case(17, 257, 16),
        "grid_stride_wraps": row_update_case(3, 2048 * 256 + 1000, 1),
        "view_nan_padding": row_update_case(9, 300, 4, pad=True),
        "rank1": row_update_case(1, 300, 0),
    },
    "hals_row_scale": {
        "normsq": row_scale_case(4, 300, 2, 37.5, 300),
        "normsq_zero_shard": row_scale_case(4, 300, 1, 0.0, 1000),
        "one_column": row_scale_case(3, 1, 2, 2.25, 1),
        "one_column_zero": row_scale_case(3, 1, 0, 0.0, 7),
        "view_nan_padding": row_scale_case(5, 260, 4, 3.0, 260, pad=True),
    },
    "hals_stop_restore": {
        "stop_at_sweep0": stop_restore_case([1.0, 0.9, 0.8], 0, 100, delta=2.0),
        "stop_inside_window": stop_restore_case(NSW, 2, 100),
        "stop_at_last_sweep_run": stop_restore_case(NSW[:5], 2, 100),
        "stop_before_head": stop_restore_case(NSW, 5, 100),
        "no_stop": stop_restore_case(NSW[:4], 1, 100),
        "budget1": stop_restore_case(NSW, 0, 1),
        "budget_inside_window": stop_restore_case(NSW, 1, 3),
        "one_sweep_no_snapshots": stop_restore_case([0.7], 0, 100, snapshots=False),
        "nan_in_sums": stop_restore_case([1.0, 0.5, float("nan"), 0.2, 0.1], 1, 100),
        "nan_first_sum": stop_restore_case([float("nan"), 0.5, 0.2], 0, 100),
        "view_nan_padding": stop_restore_case(NSW, 2, 100, pad=True),
    },
    # ---- the rest: one small ragged case each (their deep coverage lives in test_gpu_kernels / _ntf / _ntd) -------------
    "gram": {"ragged": plain("gram", 1e-5, lambda g: ([f32(7, 301, rng=g)], {}))},
    "xht": {"ragged": plain("xht", 1e-5, lambda g: ([f32(133, 71, rng=g), f32(9, 71, rng=g)], {}))},
    "xty": {"ragged": plain("xty", 1e-5, lambda g: ([f32(133, 71, rng=g), f32(9, 133, rng=g)], {}))},
    "frob_resid": {"ragged": plain("frob_resid", 1e-5, lambda g: ([f32(133, 71, rng=g), f32(9, 133, rng=g), f32(9, 71, rng=g)], {}))},
    "dot": {"ragged": plain("dot", 1e-5, lambda g: ([f32(9, 257, rng=g), f32(9, 257, rng=g)], {}))},
    "hadamard": {"ragged": plain("hadamard", "round32", lambda g: ([f32(9, 257, rng=g), f32(9, 257, rng=g)], {}))},
    "mu_left": {f"beta{b}": plain("mu_left", 2e-5, lambda g, b=b: ([f32(133, 71, rng=g), f32(9, 133, rng=g), f32(9, 71, rng=g), b], {}))
                for b in (0.5, 1, 2)},
    "mu_right_accum": {f"beta{b}": plain("mu_right_accum", 1e-5,
                                         lambda g, b=b: ([f32(133, 71, rng=g), f32(9, 133, rng=g), f32(9, 71, rng=g), b], {}))
                       for b in (1, 2, 3)},
    "mu_apply": {"den": plain("mu_apply", 2e-5, lambda g: ([f32(9, 71, rng=g), f32(9, 71, rng=g), f32(9, 71, rng=g), None, 1.5], {})),
                 "den_vec": plain("mu_apply", 2e-5, lambda g: ([f32(9, 71, rng=g), f32(9, 71, rng=g), None,
                                                                 g.rand(9) + 0.5, 1], {}))},
    "betadiv": {f"beta{b}": plain("betadiv", 1e-5, lambda g, b=b: ([f32(133, 71, rng=g), f32(9, 133, rng=g), f32(9, 71, rng=g), b], {}))
                for b in (0, 0.5, 1, 2, 3)},
    "mttkrp3": {f"mode{m}": plain("mttkrp3", 1e-5, lambda g, m=m: ([f32(13, 11, 17, rng=g), [f32(5, 13, rng=g), f32(5, 11, rng=g),
                                                                                           f32(5, 17, rng=g)], m], {}))
                for m in range(3)},
    "cp3_betadiv": {f"beta{b}": plain("cp3_betadiv", 1e-5, lambda g, b=b: ([f32(13, 11, 17, rng=g),
                                                                             [f32(5, 13, rng=g), f32(5, 11, rng=g), f32(5, 17, rng=g)], b], {}))
                    for b in (1, 2)},
    "cp3_partial_cost": {"ragged": plain("cp3_partial_cost", 1e-5, lambda g: ([f32(13, 11, 17, rng=g),
                                                                               [f32(5, 13, rng=g), f32(5, 11, rng=g), f32(5, 17, rng=g)],
                                                                               np.zeros((5, 13, 11), np.float32), np.zeros(1)], {}))},
    "ttm3": {f"mode{m}": plain("ttm3", 1e-5, lambda g, m=m: ([f32(13, 11, 17, rng=g), f32(6, (13, 11, 17)[m], rng=g), m], {}))
             for m in range(3)},
    "mttkrp3_from_partial": {f"axis{a}": plain("mttkrp3_from_partial", 1e-5,
                                               lambda g, a=a: ([f32(5, 13, 11, rng=g), f32(5, 13 if a == 1 else 11, rng=g), a], {}))
                             for a in (1, 2)},
}


def _hals_case(method, sparsity):
    def run(eng):
        rng = np.random.RandomState(11)
        r, n = 7, 301
        A = rng.rand(40, r)
        UtU = (A.T @ A).astype(np.float32)
        UtM = (A.T @ (A @ rng.rand(r, n))).astype(np.float32)
        V = f32(r, n, rng=rng)
        if method == "hals_sweeps":
            gr, wr, ga, wa, changed = call_both(eng, method, [UtM, UtU, V, 5], {"sparsity": sparsity})
            assert changed == [(2,)]
            check_rel(ga[(2,)], wa[(2,)], 1e-4, "V")
            np.testing.assert_allclose(gr, wr, rtol=5e-3)
        else:
            st = np.zeros(8)
            gr, wr, ga, wa, changed = call_both(eng, method, [UtM, UtU, V, 50], {"delta": 0.01, "sparsity": sparsity,
                                                                                 "status": st})
            assert "status" not in changed and changed == [(2,)]
            check_rel(ga[(2,)], wa[(2,)], 2e-4, "V")
            assert gr[1] == wr[1] and gr[3] == wr[3] == 0.0, (gr[:4], wr[:4])          # sweep count and error word: exact
            np.testing.assert_allclose(gr[[0, 2]], wr[[0, 2]], rtol=5e-3)              # eps, eps0
    return run


CONTRACT["hals_sweeps"] = {"plain": _hals_case("hals_sweeps", None), "sparsity": _hals_case("hals_sweeps", 0.1)}
CONTRACT["hals_solve"] = {"plain": _hals_case("hals_solve", None), "sparsity": _hals_case("hals_solve", 0.1)}

CASES = [(m, c) for m in sorted(CONTRACT) for c in CONTRACT[m]]


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


@pytest.mark.parametrize("method,case", CASES, ids=[f"{m}-{c}" for m, c in CASES])
def test_engine_matches_its_double(eng, method, case):
    CONTRACT[method][case](eng)

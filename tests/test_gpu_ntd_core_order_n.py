"""GPU parity of the order-N projected-gradient core update (nnf_ntd_core_pgn_f32, Engine.ntd_core_pgn) and of the NTD-HALS
driver on tensors of order 4 and 5 whose merged trailing core extent exceeds 128.

The yardstick is the fp64 loop of test_gpu_ntd.py::_pg_reference restated for N modes, on inputs built like
test_gpu_ntd.py::_check_core_pg (seed sum(dims), data shape 5 d + 3 per mode, factors scale * rand, Grams, MtX and start core
rounded through fp32 on both sides).  Bounds are that file's for the fp64 forms: iteration count equal, |step - ref| <= 1e-12,
core rel < 1e-5, |error - ref| <= 1e-6 ||T||^2 (lds32: count within 3 when delta > 0, core rel < 1e-4).
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import nnfac_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda").contiguous()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def pgn_form(dims, num_cus=256):
    """The launcher's rule (pg_launch in k_ntd.hip), restated: images are the transposed Grams with rows padded to a multiple of
    four floats.  `multi` (S >= 2048, 4 <= d0 <= CUs, 400 doubles + the images of modes 1.. + four slab-sized fp64 arrays within
    150 KiB), else one workgroup: `lds64` / `lds32` (272 doubles + all images + four core-sized arrays within 160 KiB), else
    `ws`, which keeps the images in LDS only within 64 KiB and otherwise reads them from the workspace (`ws_gram`)."""
    S = int(np.prod(dims))
    img = [d * ((d + 3) & ~3) for d in dims]
    fixed = 272 * 8 + 4 * sum(img)
    if S >= 2048 and 4 <= dims[0] <= num_cus and 400 * 8 + 4 * (sum(img[1:]) + 2) + 4 * (S // dims[0]) * 8 <= 150 * 1024:
        return "multi"
    if fixed + 4 * S * 8 <= 160 * 1024:
        return "lds64"
    if fixed + 4 * S * 4 <= 160 * 1024:
        return "lds32"
    return "ws_gram" if fixed > 64 * 1024 else "ws"


# the dims of section A and the form each must take (the literal entries pin the rule above, not the other way round)
PGN_FORMS = {(3, 2, 3, 2): "lds64", (2, 2, 2, 3, 2): "lds64", (1, 5, 1, 4): "lds64", (4, 3, 5, 2): "lds64",
             (8, 8, 12, 12): "multi", (4, 3, 20, 20): "multi", (6, 5, 13, 11): "multi", (5, 4, 3, 6, 7): "multi",
             (128, 2, 3, 3): "multi", (3, 40, 9, 9): "ws", (2, 2, 64, 64): "ws", (2, 100, 100, 3): "ws_gram"}


def test_form_table_follows_the_rule():
    assert {d: pgn_form(d) for d in PGN_FORMS} == PGN_FORMS


@pytest.fixture(scope="module")
def pgn_forms(built_lib):
    """{dims: form} as the library reports it (NNF_NTD_DEBUG) for every core of PGN_FORMS, from one subprocess."""
    code = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
from nn_fac_amd.engine import get_engine
eng = get_engine("cuda:0")
for d in %r:
    c = torch.ones(d, device="cuda")
    eng.ntd_core_pgn(c, torch.ones(d, device="cuda"), [torch.eye(n, device="cuda") for n in d], 0.0, 0.01, 0, 1.0)
    torch.cuda.synchronize()
print("done")
""" % (sorted(PGN_FORMS),)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NNF_NTD_DEBUG="1"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-2000:]
    got = {}
    for m in re.finditer(r"\[nnf ntd\] pgn d=\(([\d,]+)\) S=(\d+) form=(\w+)", p.stderr):
        d = tuple(int(x) for x in m.group(1).split(","))
        assert int(m.group(2)) == int(np.prod(d))
        got[d] = m.group(3)
    return got


def test_core_update_forms(pgn_forms):
    """B: every core of section A takes the form the rule gives it; the grid form, both LDS-free placements and the plain
    one-workgroup form are all reached."""
    assert pgn_forms == PGN_FORMS
    assert {"multi", "lds64", "ws", "ws_gram"} <= set(pgn_forms.values())
    for d in [(8, 8, 12, 12), (4, 3, 20, 20), (6, 5, 13, 11), (5, 4, 3, 6, 7), (128, 2, 3, 3)]:
        assert pgn_forms[d] == "multi"
    assert pgn_forms[(2, 2, 64, 64)] == "ws"


# ----------------------------------------------------------------------------------------------------------------------
# the fp64 yardstick
# ----------------------------------------------------------------------------------------------------------------------
def pg_reference(core0, MtX, M, sparse, delta, max_iter, ratios=None):
    """ntd.py:592-619 in fp64 for any number of modes: returns (core, iterations, step)."""
    step = 1.0
    for m_ in M:
        step *= 1 / np.linalg.svd(m_, compute_uv=False)[0]
    step = round(step, 6)
    core, cnt, upd0, upd = core0.copy(), 1, 0, 1
    while cnt <= max_iter and upd >= delta * upd0:
        grad = -MtX + orc.multi_mode_dot(core, M) + sparse * np.ones(core.shape)
        dc = np.minimum(step * grad, core)
        core = core - dc
        upd = np.sqrt(np.sum(dc ** 2))
        if cnt == 1:
            upd0 = upd
        if ratios is not None:
            ratios.append(upd / upd0 if upd0 else np.inf)
        cnt += 1
    return core, cnt - 1, step


@functools.lru_cache(maxsize=None)
def pg_inputs(dims, scale):
    """(MtX, Grams, start core, ||T||^2), fp32-rounded fp64 arrays; built once per (dims, scale) and never modified."""
    rng = np.random.RandomState(sum(dims))
    n = len(dims)
    shape = tuple(5 * d + 3 for d in dims)
    F = [scale * rng.rand(shape[i], dims[i]) for i in range(n)]   # scale keeps the 6-decimal step away from 0
    core_true = rng.rand(*dims)
    T = orc.multi_mode_dot(core_true, F)
    T += 0.01 * rng.rand(*shape)
    MtX = orc.multi_mode_dot(T, F, transpose=True).astype(np.float32).astype(np.float64)
    M = tuple((f.T @ f).astype(np.float32).astype(np.float64) for f in F)
    core0 = rng.rand(*dims).astype(np.float32).astype(np.float64)
    nrm2 = float(np.sum(T ** 2))
    for a in (MtX, core0) + M:
        a.setflags(write=False)
    return MtX, M, core0, nrm2


@functools.lru_cache(maxsize=None)
def pg_case(dims, sparse, scale, max_iter, delta):
    MtX, M, core0, nrm2 = pg_inputs(dims, scale)
    if sparse == "median":
        sparse = float(np.float32(np.median(MtX)))
    core, iters, step = pg_reference(core0, MtX, list(M), sparse, delta, max_iter)
    want_err = nrm2 - 2 * np.sum(MtX * core) + np.sum(orc.multi_mode_dot(core, list(M)) * core)
    core.setflags(write=False)
    return sparse, core, iters, step, want_err


def check_core_pgn(eng, pgn_forms, dims, sparse, scale, max_iter, delta, iters_want=None, zeros_want=None):
    MtX, M, core0, nrm2 = pg_inputs(dims, scale)
    zeroing = sparse == "median"
    sparse, core, iters, step, want_err = pg_case(dims, sparse, scale, max_iter, delta)
    if iters_want is not None:
        assert iters == iters_want                  # the yardstick itself: the counts the cases were chosen for
    cd = dev(core0)
    st = eng.ntd_core_pgn(cd, dev(MtX), [dev(m_) for m_ in M], sparse, delta, max_iter, nrm2).cpu().numpy()
    assert pgn_forms[dims] == PGN_FORMS[dims]
    fp32_store = pgn_forms[dims] == "lds32"         # (rounds the core to fp32 after every step)
    got = cd.cpu().numpy()
    print(dims, sparse, max_iter, delta, "iters", int(st[0]), iters, "step", st[3], step, "rel", rel(got, core),
          "err", st[4], want_err, "bound", 1e-6 * nrm2)
    assert st[5] == 0.0
    assert abs(int(st[0]) - iters) <= (3 if fp32_store and delta > 0 else 0)
    assert abs(st[3] - step) <= 1e-12
    assert rel(got, core) < (1e-4 if fp32_store else 1e-5)
    assert abs(st[4] - want_err) <= 1e-6 * nrm2
    if zeroing:
        zeros = int(np.sum(core == 0))
        if zeros_want is not None:
            assert zeros == zeros_want
        assert zeros >= core.size // 10 and abs(int(np.sum(got == 0)) - zeros) <= core.size // 100, (zeros, int(np.sum(got == 0)))


# dims, sparse, scale, max_iter, delta, steps of the fp64 loop, entries it zeroes
A_CASES = [
    ((3, 2, 3, 2), 0.0, 1.0, 300, 0.01, 84, None),
    ((2, 2, 2, 3, 2), 0.05, 1.0, 300, 0.01, 250, None),
    ((1, 5, 1, 4), 0.0, 1.0, 300, 0.01, 141, None),
    ((4, 3, 5, 2), "median", 1.0, 300, 0.01, 24, 102),
    ((8, 8, 12, 12), 0.0, 0.3, 300, 0.01, 300, None),
    ((4, 3, 20, 20), 0.0, 0.3, 300, 0.01, 300, None),
    ((6, 5, 13, 11), 0.0, 0.3, 300, 0.01, 300, None),
    ((6, 5, 13, 11), "median", 0.3, 300, 0.01, 82, 4074),
    ((5, 4, 3, 6, 7), 0.0, 0.5, 300, 0.01, 300, None),
    ((128, 2, 3, 3), 0.0, 0.3, 300, 0.01, 300, None),
    ((3, 40, 9, 9), 0.0, 0.3, 25, 0.01, 25, None),
    ((2, 2, 64, 64), 0.0, 0.1, 12, 0.0, 12, None),
    ((2, 2, 64, 64), 0.0, 0.1, 300, 0.01, 2, None),
    ((2, 100, 100, 3), 0.0, 0.1, 6, 0.0, 6, None),
]


@pytest.mark.parametrize("dims,sparse,scale,max_iter,delta,iters,zeros", A_CASES)
def test_core_pgn_against_fp64_loop(eng, pgn_forms, dims, sparse, scale, max_iter, delta, iters, zeros):
    """A: every form, orders 4 and 5, extents of 1, a slab count of 128, a sparsity that zeroes entries, a loop that stops
    after 2 steps and loops that run all 300."""
    check_core_pgn(eng, pgn_forms, dims, sparse, scale, max_iter, delta, iters, zeros)


@pytest.mark.parametrize("dims,sparse,scale,max_iter,delta", [
    ((3, 2, 3, 2), 0.0, 1.0, 0, 0.01), ((3, 2, 3, 2), 0.0, 1.0, 1, 0.01),
    ((8, 8, 12, 12), 0.0, 0.3, 0, 0.01), ((8, 8, 12, 12), 0.0, 0.3, 1, 0.01),
    ((4, 3, 20, 20), 0.0, 0.3, 40, 0.0)])
def test_core_pgn_edges(eng, pgn_forms, dims, sparse, scale, max_iter, delta):
    """max_iter 0 and 1 on the one-workgroup and the grid form; delta = 0 (every step runs)."""
    check_core_pgn(eng, pgn_forms, dims, sparse, scale, max_iter, delta)


# ----------------------------------------------------------------------------------------------------------------------
# C: agreement with the three-mode entry
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,scale,max_iter", [((9, 9, 3), 1.0, 300), ((16, 12, 20), 0.1, 300), ((3, 40, 50), 0.1, 300),
                                                 ((2, 64, 64), 0.1, 25)])
def test_three_modes_through_the_new_entry_are_bit_identical(eng, dims, scale, max_iter):
    """ndim = 3: lds64, multi, lds32 and ws cores give the same core and the same six status doubles, bit for bit, through
    both entries (one device implementation, same form selection, same summation order)."""
    MtX, M, core0, nrm2 = pg_inputs(dims, scale)
    a, b = dev(core0), dev(core0)
    grams = [dev(m_) for m_ in M]
    sa = eng.ntd_core_pg(a, dev(MtX), grams, 0.0, 0.01, max_iter, nrm2).cpu().numpy()
    sb = eng.ntd_core_pgn(b, dev(MtX), grams, 0.0, 0.01, max_iter, nrm2).cpu().numpy()
    assert sa[5] == 0.0 and int(sa[0]) >= 2
    assert sa.tobytes() == sb.tobytes(), (sa, sb)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dims,scale", [((4, 3, 5, 2), 1.0), ((8, 8, 8, 8), 0.3)])
def test_native_against_kronecker_merged(eng, dims, scale):
    """The native entry on the 4-way core against the three-mode entry on the core with its two trailing modes merged and the
    Kronecker product of their Grams.  Both are fp64 and differ in the order of the products only -- provided they are given
    the same problem: the product of two fp32 Gram entries has 48 significant bits, so the trailing Grams are first rounded
    to 11 bits (through fp16), which makes their Kronecker product exact in fp32.  Equal counts and rounded step, cores
    within 1e-6, errors within 1e-9 (relative)."""
    MtX, M, core0, nrm2 = pg_inputs(dims, scale)
    M = [M[0], M[1]] + [m_.astype(np.float16).astype(np.float64) for m_ in M[2:]]
    Mk = np.kron(M[2], M[3])
    assert np.array_equal(Mk, Mk.astype(np.float32).astype(np.float64))
    d3 = (dims[0], dims[1], dims[2] * dims[3])
    a, b = dev(core0), dev(core0.reshape(d3))
    sa = eng.ntd_core_pgn(a, dev(MtX), [dev(m_) for m_ in M], 0.0, 0.01, 300, nrm2).cpu().numpy()
    sb = eng.ntd_core_pg(b, dev(MtX.reshape(d3)), [dev(M[0]), dev(M[1]), dev(Mk)], 0.0, 0.01, 300, nrm2).cpu().numpy()
    print(dims, sa, sb)
    assert sa[5] == 0.0 and sb[5] == 0.0
    assert int(sa[0]) == int(sb[0]) and int(sa[0]) >= 2
    assert sa[3] == sb[3]
    assert rel(a.cpu().numpy().reshape(d3), b.cpu().numpy()) < 1e-6
    assert abs(sa[4] - sb[4]) <= 1e-9 * abs(sb[4])


# ----------------------------------------------------------------------------------------------------------------------
# D: the driver
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ranks", [((9, 8, 14, 13), (3, 2, 12, 11)), ((12, 11, 18, 17), (8, 8, 12, 12)),
                                         ((5, 4, 70, 66), (2, 2, 64, 64)), ((7, 6, 7, 6, 8), (3, 2, 5, 5, 6)),
                                         ((8, 5, 8, 7, 7), (4, 2, 6, 6, 6))])
def test_ntd_hals_order_n_any_core(built_lib, shape, ranks):
    """NTD-HALS on tensors of order 4 and 5 whose merged trailing core extent is 132 ... 4096 (> 128: the native core update),
    three iterations against the oracle, data recipe and seed rule of test_gpu_ntd.py::test_ntd_order_n."""
    from nn_fac_amd.ntd import compute_ntd
    rng = np.random.RandomState(sum(shape) + sum(ranks))
    N = len(shape)
    G = rng.rand(*ranks)
    Fs = [rng.rand(s, q) for s, q in zip(shape, ranks)]
    T = orc.multi_mode_dot(G, Fs) + 1e-2 * rng.rand(*shape)
    T = T.astype(np.float32)
    C0 = (rng.rand(*ranks) + 0.05).astype(np.float32)
    F0 = [(rng.rand(s, q) + 0.05).astype(np.float32) for s, q in zip(shape, ranks)]
    kw = dict(n_iter_max=3, tol=0, update_rule="hals", return_costs=True, deterministic=True,
              sparsity_coefficients=[None] * (N + 1), normalize=[False] * (N + 1))
    sw, pg, swo, pgo = [], [], [], []
    core, F, costs, _ = compute_ntd(T, list(ranks), C0, F0, sweep_log=sw, pg_log=pg, **kw)
    co, Fo, cso, _ = orc.compute_ntd(T.astype(np.float64), list(ranks), C0.astype(np.float64), [f.astype(np.float64) for f in F0],
                                     sweeps=swo, pg_iters=pgo, **kw)
    print(shape, ranks, "core", rel(core, co), "factors", [rel(F[i], Fo[i]) for i in range(N)], costs, cso, sw, swo, pg, pgo)
    assert core.shape == co.shape and rel(core, co) < 5e-3, rel(core, co)
    for i in range(N):
        assert rel(F[i], Fo[i]) < 5e-3, (i, rel(F[i], Fo[i]))
    np.testing.assert_allclose(costs, cso, rtol=5e-3)
    assert sw == swo and pg == pgo, (sw, swo, pg, pgo)


def test_ntd_end_to_end_with_a_large_tail(built_lib):
    from nn_fac_amd.ntd import ntd
    shape, ranks = (9, 8, 14, 13), [3, 2, 12, 11]
    T = np.random.RandomState(7).rand(*shape)
    core, facs = ntd(T, list(ranks), init="random", n_iter_max=2, deterministic=True)
    assert core.shape == tuple(ranks) and np.all(core >= 0)
    assert [f.shape for f in facs] == [(shape[i], ranks[i]) for i in range(4)] and all(np.all(f >= 0) for f in facs)


# ----------------------------------------------------------------------------------------------------------------------
# E: refusals
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(4, 3), (2,) * 9, (2, 129, 2, 2), (128, 128, 128, 4)])
def test_refusals_leave_core_and_status_untouched(eng, dims):
    """ndim 2 and 9, an extent of 129 and S = 2^23 are refused before anything is launched or written.  (The Grams of the
    S > 2^22 case are 1 x 1 stand-ins: the refusal comes before they are looked at, and the engine's own shape check is
    what this test is not about, so the C entry is called directly.)"""
    import ctypes as C
    from nn_fac_amd import _lib
    n = len(dims)
    S = int(np.prod(dims))
    core = torch.full((S,), 7.0, dtype=torch.float32, device="cuda")
    mtx = torch.ones((S,), dtype=torch.float32, device="cuda")
    status = torch.full((6,), 7.0, dtype=torch.float64, device="cuda")
    gram = torch.eye(129, dtype=torch.float32, device="cuda")
    ptrs = (C.c_void_p * n)(*[gram.data_ptr()] * n)
    dd = (C.c_int * n)(*dims)
    rc = eng.lib.nnf_ntd_core_pgn_f32(eng.ctx, C.c_void_p(core.data_ptr()), C.c_void_p(mtx.data_ptr()), ptrs, n, dd, 0.0, 0.01, 5,
                                      1.0, C.c_void_p(status.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc in (-1, -3), rc                     # NNF_ERR_ARG / NNF_ERR_UNSUPPORTED
    assert bool((core == 7.0).all()) and bool((status == 7.0).all())


def test_engine_refuses_mismatched_arguments(eng):
    from nn_fac_amd.utils.errors import ArgumentException, EngineError
    core = torch.full((3, 2, 3, 2), 7.0, device="cuda")
    grams = [torch.eye(d, device="cuda") for d in (3, 2, 3, 2)]
    with pytest.raises(ArgumentException):
        eng.ntd_core_pgn(core, torch.ones((3, 2, 3, 2), device="cuda"), grams[:3], 0.0, 0.01, 5, 1.0)
    with pytest.raises(ArgumentException):
        eng.ntd_core_pgn(core, torch.ones((3, 2, 6), device="cuda"), grams, 0.0, 0.01, 5, 1.0)
    c2 = torch.full((4, 3), 7.0, device="cuda")
    with pytest.raises(EngineError):
        eng.ntd_core_pgn(c2, torch.ones((4, 3), device="cuda"), [torch.eye(4, device="cuda"), torch.eye(3, device="cuda")], 0.0,
                         0.01, 5, 1.0)
    assert bool((core == 7.0).all()) and bool((c2 == 7.0).all())

"""The MU route above rank 128 (beta != 2) and its ratio pass, against fp64.  Needs a MI355X (the case table does not: tests/
test_mu_plan_table.py checks its plans against the library's plan arithmetic at 256 and 304 compute units).

Engine._mu_composed sends mu_left, mu_right and mu_right_accum through nnf_mu_ratio_f32, then nnf_xht_f32 / nnf_xty_f32 on the
m x n operands it wrote, then nnf_mu_apply_f32.  The ratio pass is nnf_cost_kernel (k_cost.hip) in its NNF_RATIO_KL, NNF_RATIO_GEN
and NNF_PROD forms; above rank 128 the model U V builds up over rank chunks of 128 in R1 itself: chunk 0 writes its product
(prod), every later chunk reads the model back (pin=1) and the last one turns it into the ratios.  The cost passes run the same
kernel and show its product through one sum only; the ratio outputs show it element by element.

  1. test_ratio_values: nnf_mu_ratio_f32 through the C entry, R1 = X .* P^(beta-2), R2 = P^(beta-1) with P = Ut^T V in fp64 from
     the fp32 operands, at the k-step, load-group, V-buffer, rank-chunk, row-tile, column-block, column-split and load-width
     edges (RATIO_CASES names each case by what it reaches).  Ut, V uniform in [0.5, 1.5]: every rank row contributes at least
     1 / (9 r) of every entry of P (asserted) -- 2.9e-4 at r = 385, nearly three times the entrywise tolerance, so a rank row
     left out or added twice fails wherever it is missing.  X uniform in [0.05, 1.05] with exact zeros at tile corners, where
     R1 must be +0.  R1 / R2 are NaN before every call (R1 is the model buffer: a chunk that reads before it writes shows), the
     measured call follows one on other data, the padding of a pitched R1 / R2 keeps its bits, two calls give the same bits.
     Tolerances: the pair of test_gpu_launch_plans.assert_close for plain products, 1e-5 global and 1e-4 entrywise (fp32 worst
     case of an r-term nonnegative dot product: r 2^-24 = 2.3e-5 at r = 385; reciprocal, log and exp2 add about 2e-6).
  2. test_ratio_plans: a child process under NNF_PLAN_DEBUG runs the case list once; a rank-r call reports ceil(r / 128)
     passes in chunk order, each with the load width, load group, V buffers and column splits its case names, and the list
     reaches what REQUIRED_RATIO and REQUIRED_COMBOS name.
  3. test_composed_updates: Engine.mu_left / mu_right / mu_right_accum at ranks 129, 200, 257 against mu_left_fp64,
     mu_right_fp64, mu_right_terms_fp64 (test_gpu_launch_plans), contiguous and as NaN-padded views; tolerances from that
     file: 2e-5 global, 1e-3 entrywise, 1e-12 for the fp64 den_vec.  test_rank128_fused_and_composed_agree: the two routes
     at the rank where both exist.
  4. test_composed_nonfinite: a NaN and a +Inf in X and a NaN in the factor make exactly the entries of mu_left / mu_right
     non-finite (NaN as NaN, Inf as Inf) that the fp64 NumPy statement of the update (oracle/nnfac_oracle.py) makes so.

Measured on a MI355X (maxima over all cases of the part; global / entrywise as assert_close defines them):
  part                                         against      beta:  0         0.5       1         1.5       2         3
  1  ratio R1, R2                              1e-5 / 1e-4  global 4.2e-7    2.6e-7    1.8e-7    2.0e-7    3.9e-7    7.7e-7
                                                            entry  1.6e-6    1.1e-6    7.5e-7    6.1e-7    1.1e-6    2.1e-6
  3  mu_left                                   2e-5 / 1e-3  global 2.6e-7    3.7e-7    3.7e-7    5.2e-7    --        2.7e-7
                                                            entry  1.2e-6    1.5e-6    1.6e-6    2.3e-6    --        1.2e-6
  3  mu_right                                  2e-5 / 1e-3  global 8.2e-8    1.6e-7    1.0e-7    1.3e-7    --        8.2e-8
                                                            entry  3.4e-7    5.9e-7    4.5e-7    6.5e-7    --        3.5e-7
  3  mu_right_accum num, den                   2e-5 / 1e-3  global 2.7e-7    1.6e-7    9.4e-8    1.5e-7    --        5.3e-7
                                                            entry  7.1e-7    5.7e-7    4.5e-7    5.5e-7    --        1.1e-6
  3  mu_right_accum den_vec (beta = 1)         1e-12        entry  0 (the same fp64 sum)
  3  rank 128, fused and composed against fp64 2e-5 / 1e-3  global 2.7e-7    3.4e-7    3.7e-7    4.9e-7    --        2.6e-7
                                                            entry  1.1e-6    1.4e-6    1.7e-6    2.0e-6    --        1.1e-6
  3  rank 128, composed against fused          2e-5 / 1e-3  global 4.5e-8    4.3e-8    5.7e-8    5.7e-8    --        4.6e-8
                                                            entry  2.3e-7    2.4e-7    2.3e-7    2.3e-7    --        2.3e-7
  4  finite entries, left / right              2e-5 / 1e-3  global --        2.6e-7    2.4e-7    --        --        --
                                                            entry  --        1.3e-6    1.2e-6    --        --        --
Each of these deliberate faults, tried on a copy of the tree, fails here: the Pin add dropped from nnf_cost_kernel (every r > 128
case of test_ratio_values, test_composed_updates, test_composed_nonfinite), the ratio stores masked by cc <= jrem (the padding
check of the d_ldr_* cases), the last rank chunk skipped in launch_cost_any_rank (the same tests as the first, and
test_ratio_plans, test_ratio_refusals), gamma = 1 at beta = 3 in the fp64 reference (test_composed_updates,
test_rank128_fused_and_composed_agree).
"""
import collections
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_launch_plans import ROOT, mu_left_fp64, mu_right_fp64, mu_right_terms_fp64, parse_plans

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.25                      # the padding of a pitched R1 / R2, and an R2 that must not be touched
GLOB, ENT = 1e-5, 1e-4                # part 1: plain products (assert_close in test_gpu_launch_plans)
MU_GLOB, MU_ENT, DVEC_REL = 2e-5, 1e-3, 1e-12      # parts 3, 4: the MU pair of that file
FULL = (1, 0, 0.5, 1.5, 2, 3)
TWO = (1, 0.5)
ERR_ARG = -1
MAX_M, MAX_N, MAX_R = 257, 2200, 385
assert 1 / (9 * MAX_R) > 2.5 * ENT    # a rank row's least share of P against the entrywise tolerance

# layout fields, in floats: x_pitch / ut_pitch / v_pitch / ldr (None: contiguous), x_off / ut_off (the operand starts that many
# floats behind a 16-byte aligned allocation).  expect: csplit / NN / vdb of the LAST pass of a call (None: not named).
Case = collections.namedtuple("Case", "m n r betas x_pitch x_off ut_pitch ut_off v_pitch ldr expect")


def _cdiv(a, b):
    return -(-a // b)


def ratio_cases():
    """{name: Case}.  The names say what a case reaches; not a cross product."""
    cases = {}

    def add(name, m, n, r, betas=TWO, x_pitch=None, x_off=0, ut_pitch=None, ut_off=0, v_pitch=None, ldr=None, expect=None):
        assert name not in cases and m <= MAX_M and n <= MAX_N and r <= MAX_R
        cases[name] = Case(m, n, r, betas, x_pitch, x_off, ut_pitch, ut_off, v_pitch, ldr, expect)

    # ---- ranks, 130 x 68 (two row tiles, the second of two rows; two column blocks, the second of four columns), everything on
    # vector loads.  Ut at pitch 132: the full waves of the first workgroup take the vector staging (with its zeroed rank rows
    # when r % 4 != 0), the ragged wave of the second the element-wise one.  1, 4, 5, 9: 1, 1, 2, 3 k-steps (no trip of the
    # pipelined loop, an odd tail, an exact trip); NN / vdb: rank rows per load group, two V buffers -- of the last pass
    for r, nn, vdb, what in [(1, 4, 1, "one_kstep"), (4, 4, 1, "one_full_kstep"), (5, 4, 1, "two_ksteps"), (9, 4, 1, "three_ksteps"),
                             (50, 4, 1, "nn4_two_v"), (64, 4, 0, "nn4_one_v"), (100, 8, 0, "nn8_one_v"), (120, 8, 1, "nn8_two_v"),
                             (128, 8, 1, "full_chunk"), (129, 8, 1, "last_chunk_of_1"), (131, 8, 1, "last_chunk_of_3"),
                             (200, 8, 1, "last_chunk_of_72"), (256, 8, 1, "two_full_chunks"), (257, 8, 1, "three_chunks_mid_prod_pin"),
                             (385, 8, 1, "four_chunks")]:
        add(f"rank{r}_{what}", 130, 68, r, betas=FULL if r == 129 else TWO, ut_pitch=132, expect=dict(csplit=1, NN=nn, vdb=vdb))
    # ---- rows, n = 65 (dword loads).  33: waves 2 and 3 of the workgroup have no rows; 32 and 128: every wave full and Ut
    # aligned (vector staging); every other m: a ragged wave or an unaligned Ut (element-wise staging)
    for m in (1, 31, 32, 33, 127, 128, 129, 130, 257):
        for r in (50, 129):
            add(f"rows{m}_r{r}", m, 65, r)
    add("rows257_r257_ut_vector_staging", 257, 68, 257, ut_pitch=260)
    # ---- columns, m = 33.  4 and 64: vector loads; 63 / 64 / 65: the block edge; 257: five blocks, one live column in the last
    for n in (1, 3, 4, 63, 64, 65, 257):
        for r in (9, 131):
            add(f"cols{n}_r{r}", 33, n, r)
    # 577: ten blocks, two column splits, one live column in the last block; 2200: 35 blocks in 8 splits of 5, the last empty
    add("cols577_two_splits_r100", 33, 577, 100, expect=dict(csplit=2, NN=8, vdb=0))
    add("cols577_two_splits_r257", 130, 577, 257, betas=FULL, expect=dict(csplit=2, NN=8, vdb=1))
    add("cols2200_empty_split_r50", 129, 2200, 50, expect=dict(csplit=8, NN=4, vdb=1))
    add("cols2200_empty_split_r385", 257, 2200, 385, betas=FULL, expect=dict(csplit=8, NN=8, vdb=1))
    add("betas_r100", 33, 65, 100, betas=FULL)
    # ---- layouts, 130 rows, at a rank below 128, at 129 and at 257
    for r in (100, 129, 257):
        add(f"a_contiguous_vec_r{r}", 130, 68, r)                       # VEC=1; above 128: VEC=1 with pin=1
        add(f"b_x_pitched_r1_odd_r{r}", 130, 65, r, x_pitch=68)         # X on vector loads alone; with the model read back: dwords
        add(f"c_x_one_float_in_r{r}", 130, 68, r, x_off=1)              # VEC=0 with R1 / R2 aligned
        add(f"d_ldr_n_plus_3_r{r}", 130, 68, r, ldr=71)
        add(f"d_ldr_multiple_of_4_r{r}", 130, 65, r, x_pitch=68, ldr=68)   # vector loads whose last piece straddles n
        add(f"e_ut_one_float_in_r{r}", 128, 68, r, ut_off=1)
        add(f"e_ut_pitch_odd_r{r}", 128, 68, r, ut_pitch=129)
        add(f"f_v_pitched_r{r}", 130, 68, r, v_pitch=73)
    return cases


RATIO_CASES = ratio_cases()
# what the case list must reach as a whole (test_ratio_plans on the device, test_mu_plan_table without one)
REQUIRED_RATIO = {"op": {"ratio_kl", "ratio_gen", "prod"}, "pin": {"0", "1"}, "VEC": {"0", "1"}, "NN": {"4", "8"}, "vdb": {"0", "1"},
                  "csplit": {"1", ">1"}}
REQUIRED_COMBOS = [dict(op="prod", pin="1"), dict(op="ratio_kl", pin="1", VEC="1"), dict(op="ratio_gen", pin="1", VEC="0"),
                   dict(op="ratio_kl", pin="0", NN="8", vdb="0"), dict(op="ratio_gen", pin="0", NN="8", vdb="0")]


def expected_passes(case, beta):
    """What a call of the case reports, pass by pass: the chunk's rank, the form, whether it reads the model back, the load width
    (X and, with pin, the model buffer R1 share one: both must be 16-byte aligned with a pitch that is a multiple of 4)."""
    x_vec = case.x_off % 4 == 0 and (case.x_pitch or case.n) % 4 == 0
    r_vec = (case.ldr or case.n) % 4 == 0
    chunks = [min(128, case.r - k0) for k0 in range(0, case.r, 128)]
    assert len(chunks) == _cdiv(case.r, 128)
    return [dict(m=case.m, n=case.n, r=rc, op="prod" if c + 1 < len(chunks) else ("ratio_kl" if beta == 1 else "ratio_gen"),
                 pin=int(c > 0), VEC=int(x_vec and (c == 0 or r_vec)), grid=_cdiv(case.m, 128)) for c, rc in enumerate(chunks)]


def check_passes(name, beta, lines, bad, seen, combos):
    """One call's report lines against expected_passes and the case's `expect`; notes what they reach."""
    case = RATIO_CASES[name]
    want = expected_passes(case, beta)
    if len(lines) != len(want):
        bad.append((name, beta, "passes", len(lines), len(want)))
        return
    for c, (kv, w) in enumerate(zip(lines, want)):
        kv = {k: str(v) for k, v in kv.items()}
        for key, val in w.items():
            if kv.get(key) != str(val):
                bad.append((name, beta, f"pass {c}", key, kv.get(key), val))
        if kv["op"] == "prod" and kv["NN"] != "8":
            bad.append((name, beta, f"pass {c}", "a model pass loads 8 rank rows per group", kv["NN"]))
        for key in ("op", "pin", "VEC", "NN", "vdb"):
            seen[key].add(kv[key])
        seen["csplit"].add("1" if kv["csplit"] == "1" else ">1")
        for n, combo in enumerate(REQUIRED_COMBOS):
            if all(kv[k] == v for k, v in combo.items()):
                combos.add(n)
    for key, val in (case.expect or {}).items():
        if str(lines[-1].get(key)) != str(val):
            bad.append((name, beta, "last pass", key, lines[-1].get(key), val))


def check_reach(seen, combos):
    for key, want in REQUIRED_RATIO.items():
        assert want <= seen[key], (key, want - seen[key])
    assert combos == set(range(len(REQUIRED_COMBOS))), [REQUIRED_COMBOS[n] for n in set(range(len(REQUIRED_COMBOS))) - combos]


# ---- data ----
def make_pool():
    """One seeded pool (left unchanged): X, Ut, V of every shape are leading blocks of it."""
    g = torch.Generator(device="cpu").manual_seed(20128)
    return {"X": (torch.rand(MAX_M, MAX_N, generator=g) + 0.05).cuda(), "Ut": (torch.rand(MAX_R, MAX_M, generator=g) + 0.5).cuda(),
            "V": (torch.rand(MAX_R, MAX_N, generator=g) + 0.5).cuda()}


def place(src, pitch=None, off=0):
    """A device copy of `src` as a view with row pitch `pitch` that starts `off` floats into a fresh allocation; every float around
    it holds NaN."""
    rows, cols = src.shape
    pitch = pitch or cols
    assert pitch >= cols
    buf = torch.full((off + rows * pitch,), NAN, dtype=torch.float32, device="cuda")
    view = torch.as_strided(buf, (rows, cols), (pitch, 1), off)
    view.copy_(src)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + 4 * off
    return view


def zero_corners(X):
    """Exact zeros at the tile corners that exist: first / last row and column, rows 31 / 32, columns 63 / 64."""
    m, n = X.shape
    for i, j in [(0, 0), (0, n - 1), (m - 1, 0), (m - 1, n - 1), (31, 63), (31, 64), (32, 63), (32, 64)]:
        if i < m and j < n:
            X[i, j] = 0.0
    return X


def ratio_operands(pool, case):
    """(X, Ut, V) of the case in its layout, and the same shapes and layouts with other values."""
    m, n, r = case.m, case.n, case.r
    X, Ut, V = zero_corners(pool["X"][:m, :n].clone()), pool["Ut"][:r, :m], pool["V"][:r, :n]
    lay = lambda x, u, v: (place(x, case.x_pitch, case.x_off), place(u, case.ut_pitch, case.ut_off), place(v, case.v_pitch))
    return lay(X, Ut, V), lay(X * 0.5 + 0.25, Ut * 2 + 0.5, V * 3 + 1)


def ratio_outputs(case, beta, with_r2=None):
    """(R1, R2) as m x ldr buffers: NaN where the pass writes, SENTINEL in the padding; R2 None at beta = 1 unless asked for
    (then all SENTINEL: it must not be written)."""
    ldr = case.ldr or case.n
    R1 = torch.full((case.m, ldr), SENTINEL, device="cuda")
    R1[:, :case.n] = NAN
    if beta == 1:
        return R1, (torch.full((case.m, ldr), SENTINEL, device="cuda") if with_r2 else None)
    return R1, R1.clone()


def mu_ratio(eng, X, Ut, V, beta, R1, R2, ldr=None):
    """nnf_mu_ratio_f32 on caller-owned outputs (whole m x ldr buffers; `ldr` overrides their pitch); returns the status."""
    from nn_fac_amd.engine import _ld, _opt, _ptr
    return eng.lib.nnf_mu_ratio_f32(eng.ctx, _ptr(X), X.shape[0], X.shape[1], _ld(X), _ptr(Ut), _ld(Ut), _ptr(V), _ld(V), Ut.shape[0],
                                    float(beta), _opt(R1), _opt(R2), R1.shape[1] if ldr is None else ldr, eng._stream())


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


MEASURED = collections.defaultdict(lambda: [0.0, 0.0])


def close(got, want, glob, ent, what, part, beta, where=None):
    """assert_close of test_gpu_launch_plans (finite; global and entrywise relative error), the entrywise part over `where`
    (default: everywhere); prints the two figures before it asserts and keeps the maxima per (part, beta)."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries (a tile never written, or a model read before it was)"
    d = (got - want).abs()
    norm = float(want.norm())
    g = float(d.norm()) / norm if norm > 0 else float(d.norm())
    rel = d / want.abs() if where is None else (d / want.abs())[where]
    e = float(rel.max()) if rel.numel() else 0.0
    print(f"[measured] part={part} beta={beta} global={g:.3e} entrywise={e:.3e} {what}")
    rec = MEASURED[(part, beta)]
    rec[0], rec[1] = max(rec[0], g), max(rec[1], e)
    assert g <= glob and e <= ent, f"{what}: global {g:.3e} (<= {glob}), entrywise {e:.3e} (<= {ent})"


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """Every case here is ordinary data and every refusal an argument check: nothing can make a kernel fault.  Should the device
    report an error all the same, nothing more is started on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error: {e}", returncode=3)


@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


@pytest.fixture(scope="module")
def pool(built_lib):
    return make_pool()


# ---- 1. the ratio pass, element by element ----
@pytest.mark.parametrize("name", list(RATIO_CASES))
def test_ratio_values(name, eng, pool):
    case = RATIO_CASES[name]
    m, n, r = case.m, case.n, case.r
    (X, Ut, V), (X2, Ut2, V2) = ratio_operands(pool, case)
    U64, V64, X64 = Ut.double(), V.double(), X.double()
    P = U64.t() @ V64
    share = float(U64.min() * V64.min() / P.max())
    assert share >= (1 - 1e-12) / (9 * r), (name, share)      # every rank row's share of every entry of the model
    nz = X != 0
    assert int((~nz).sum()) >= 1 and bool((X64[~nz] == 0).all())
    for beta in case.betas:
        what = f"{name} beta={beta}"
        R1, R2 = ratio_outputs(case, beta)
        assert mu_ratio(eng, X2, Ut2, V2, beta, R1, R2) == 0, what        # other data first: its values and workspace stay behind
        R1[:, :n] = NAN
        if R2 is not None:
            R2[:, :n] = NAN
        assert mu_ratio(eng, X, Ut, V, beta, R1, R2) == 0, what            # (beta = 1: R2 == NULL)
        close(R1[:, :n], X64 * P ** (beta - 2), GLOB, ENT, what + " R1", "ratio", beta, where=nz)
        assert bool((bits(R1[:, :n])[~nz] == 0).all()), f"{what}: R1 is not +0 where X is 0"
        if beta != 1:
            close(R2[:, :n], P ** (beta - 1), GLOB, ENT, what + " R2", "ratio", beta)
        for R in (R1, R2):
            if R is not None:
                assert bool((bits(R[:, n:]) == bits(torch.full_like(R[:, n:], SENTINEL))).all()), f"{what}: padding written"
        S1, S2 = ratio_outputs(case, beta, with_r2=True)
        assert mu_ratio(eng, X, Ut, V, beta, S1, S2) == 0, what            # again: the same bits (beta = 1: R2 given, not written)
        assert torch.equal(bits(S1), bits(R1)), f"{what}: two calls differ in R1"
        if beta == 1:
            assert bool((bits(S2) == bits(torch.full_like(S2, SENTINEL))).all()), f"{what}: R2 written at beta = 1"
        else:
            assert torch.equal(bits(S2), bits(R2)), f"{what}: two calls differ in R2"


def test_ratio_refusals(eng, pool):
    """ldr < n, R2 == NULL with beta != 1, beta < 0 or NaN, R1 == NULL: NNF_ERR_ARG from the argument checks, nothing launched,
    R1 / R2 untouched."""
    for name in ("rank100_nn8_one_v", "rank257_three_chunks_mid_prod_pin"):
        case = RATIO_CASES[name]
        (X, Ut, V), _ = ratio_operands(pool, case)
        R1 = torch.full((case.m, case.n), NAN, device="cuda")
        R2 = R1.clone()
        for what, beta, r1, r2, ldr in [("ldr < n", 0.5, R1, R2, case.n - 1), ("ldr < n at beta = 1", 1, R1, None, case.n - 1),
                                        ("no R2 at beta = 0.5", 0.5, R1, None, case.n), ("no R2 at beta = 2", 2, R1, None, case.n),
                                        ("beta < 0", -0.5, R1, R2, case.n), ("beta NaN", NAN, R1, R2, case.n),
                                        ("no R1", 1, None, R2, case.n), ("no R1 at beta = 0.5", 0.5, None, R2, case.n)]:
            assert mu_ratio(eng, X, Ut, V, beta, r1, r2, ldr=ldr) == ERR_ARG, (name, what)
        torch.cuda.synchronize()
        assert bool(torch.isnan(R1).all()) and bool(torch.isnan(R2).all()), name
        assert mu_ratio(eng, X, Ut, V, 0.5, R1, R2) == 0 and bool(torch.isfinite(R1).all()) and bool(torch.isfinite(R2).all())


# ---- 2. which instances ran ----
_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_mu_above_128 as A
from nn_fac_amd.engine import get_engine
eng, pool = get_engine("cuda:0"), A.make_pool()
for name, case in A.RATIO_CASES.items():
    (X, Ut, V), _ = A.ratio_operands(pool, case)
    for beta in case.betas:
        sys.stderr.write("[case] %s|%r\n" % (name, beta))
        sys.stderr.flush()
        R1, R2 = A.ratio_outputs(case, beta)
        assert A.mu_ratio(eng, X, Ut, V, beta, R1, R2) == 0
        torch.cuda.synchronize()
print("done")
"""


def test_ratio_plans(built_lib):
    """The passes every (case, beta) of part 1 reports under NNF_PLAN_DEBUG: ceil(r / 128) of them with the chunk ranks in order,
    all but the last writing the model, all but the first reading it back, each at the load width its layout gives; the last
    with the splits, load group and V buffers its case names; and the list reaches REQUIRED_RATIO and REQUIRED_COMBOS."""
    p = subprocess.run([sys.executable, "-c", _CHILD], env=dict(os.environ, NNF_PLAN_DEBUG="1"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    reported = parse_plans(p.stderr)
    want = [f"{name}|{beta!r}" for name, case in RATIO_CASES.items() for beta in case.betas]
    assert sorted(reported) == sorted(want)
    bad, seen, combos = [], collections.defaultdict(set), set()
    for key in want:
        name, beta = key.split("|")
        assert all(l == "cost" for l, _ in reported[key]), (key, reported[key])
        check_passes(name, float(beta), [kv for _, kv in reported[key]], bad, seen, combos)
    assert not bad, "\n".join(map(str, bad))
    check_reach(seen, combos)
    print("reached:", {k: sorted(v) for k, v in sorted(seen.items())})


# ---- 3. the composed updates ----
COMPOSED_SHAPES = [(130, 577), (257, 65), (33, 260)]
COMPOSED_BETAS = (1, 0, 0.5, 1.5, 3)


def composed_operands(pool, m, n, r, pitched, other=False):
    """Contiguous operands, or views whose padding holds NaN (pitches n + 5, m + 5, n + 7); `other`: the same layout, other values."""
    X, Ut, V = pool["X"][:m, :n], pool["Ut"][:r, :m], pool["V"][:r, :n]
    if other:
        X, Ut, V = X * 0.5 + 0.25, Ut * 2 + 0.5, V * 3 + 1
    return (place(X, n + 5), place(Ut, m + 5), place(V, n + 7)) if pitched else (place(X), place(Ut), place(V))


def nan_out(rows, cols, pitched):
    return place(torch.full((rows, cols), NAN, device="cuda"), cols + 3 if pitched else None)


@pytest.mark.parametrize("m,n", COMPOSED_SHAPES)
@pytest.mark.parametrize("r", [129, 200, 257])
def test_composed_updates(r, m, n, eng, pool):
    assert all(eng._mu_composed(r, b) for b in COMPOSED_BETAS)
    for beta in COMPOSED_BETAS:
        ref = composed_operands(pool, m, n, r, False)
        want_l, want_r = mu_left_fp64(*ref, beta), mu_right_fp64(*ref, beta)
        want_num, want_den = mu_right_terms_fp64(*ref, beta)
        for pitched in (False, True):
            X, Ut, V = composed_operands(pool, m, n, r, pitched)
            other = composed_operands(pool, m, n, r, pitched, other=True)
            what = f"r={r} {m}x{n} beta={beta} {'pitched' if pitched else 'contiguous'}"
            for side, call, want in (("left", eng.mu_left, want_l), ("right", eng.mu_right, want_r)):
                out = nan_out(*want.shape, pitched)
                call(*other, beta, out=out)
                out.fill_(NAN)
                got = call(X, Ut, V, beta, out=out)
                assert got.data_ptr() == out.data_ptr()
                close(got, want, MU_GLOB, MU_ENT, f"mu_{side} {what}", f"mu_{side}", beta)
            eng.mu_right_accum(*other, beta)
            num, den, dvec = eng.mu_right_accum(X, Ut, V, beta)
            close(num, want_num, MU_GLOB, MU_ENT, f"accum num {what}", "accum", beta)
            if beta == 1:
                assert den is None and dvec.dtype == torch.float64
                dv = float(((dvec - want_den).abs() / want_den).max())
                print(f"[measured] part=accum_den_vec beta={beta} entrywise={dv:.3e} {what}")
                assert dv <= DVEC_REL, (what, dv)
            else:
                assert dvec is None
                close(den, want_den, MU_GLOB, MU_ENT, f"accum den {what}", "accum", beta)


@pytest.mark.parametrize("m,n", COMPOSED_SHAPES)
def test_rank128_fused_and_composed_agree(m, n, eng, pool):
    """Rank 128, where both routes exist (the comparison tools/time_mu_rank.py makes): the fused kernels and
    _mu_large_rank + mu_apply against fp64 and against each other."""
    r = 128
    assert not any(eng._mu_composed(r, b) for b in COMPOSED_BETAS)
    X, Ut, V = composed_operands(pool, m, n, r, False)
    other = composed_operands(pool, m, n, r, False, other=True)
    for beta in COMPOSED_BETAS:
        for side, fused_call, F, ref in (("left", eng.mu_left, Ut, mu_left_fp64), ("right", eng.mu_right, V, mu_right_fp64)):
            what = f"rank 128 {side} {m}x{n} beta={beta}"
            want = ref(X, Ut, V, beta)
            fused = fused_call(X, Ut, V, beta)
            out = nan_out(*want.shape, False)
            eng.mu_apply(other[1] if side == "left" else other[2], *eng._mu_large_rank(*other, beta, side), beta, out=out)
            out.fill_(NAN)
            composed = eng.mu_apply(F, *eng._mu_large_rank(X, Ut, V, beta, side), beta, out=out)
            assert composed.data_ptr() == out.data_ptr()
            close(fused, want, MU_GLOB, MU_ENT, what + " fused", "rank128_fused", beta)
            close(composed, want, MU_GLOB, MU_ENT, what + " composed", "rank128_composed", beta)
            close(composed, fused.double(), MU_GLOB, MU_ENT, what + " composed against fused", "rank128_between", beta)


# ---- 4. NaN and Inf on the composed route ----
def check_nonfinite(what, got, want, part, beta):
    """The NaN set and the +Inf / -Inf sets equal the reference's; the finite entries within the MU pair."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape
    assert np.isnan(want).any() and np.isinf(want).any(), f"{what}: the reference is finite -- the case checks nothing"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN at {np.argwhere(np.isnan(got) != np.isnan(want))[:8].tolist()}"
    for s in (1, -1):
        a, b = np.isinf(got) & (np.sign(got) == s), np.isinf(want) & (np.sign(want) == s)
        assert np.array_equal(a, b), f"{what}: Inf at {np.argwhere(a != b)[:8].tolist()}"
    f = np.isfinite(want)
    d = np.abs(got[f] - want[f])
    g, e = float(np.linalg.norm(d) / np.linalg.norm(want[f])), float((d / np.abs(want[f])).max())
    print(f"[measured] part={part} beta={beta} global={g:.3e} entrywise={e:.3e} {what}")
    rec = MEASURED[(part, beta)]
    rec[0], rec[1] = max(rec[0], g), max(rec[1], e)
    assert g <= MU_GLOB and e <= MU_ENT, f"{what}: global {g:.3e} (<= {MU_GLOB}), entrywise {e:.3e} (<= {MU_ENT})"


@pytest.mark.parametrize("beta", TWO)
def test_composed_nonfinite(beta, eng, pool):
    """Rank 129 on 130 x 257: a NaN at X[17, 200], +Inf at X[100, 64] and a NaN in the last rank row of Ut (left update) or of V
    (right update, the rank row the last chunk holds alone).  As np.maximum keeps them: row 17 and the factor's row of the left
    update NaN, row 100 +Inf; column 200 and the factor's column of the right update NaN, column 64 +Inf; nothing else."""
    import nnfac_oracle as orc
    m, n, r = 130, 257, 129
    assert eng._mu_composed(r, beta)
    X = pool["X"][:m, :n].cpu().double().numpy().copy()
    U = pool["Ut"][:r, :m].cpu().double().numpy().T.copy()
    V = pool["V"][:r, :n].cpu().double().numpy().copy()
    X[17, 200], X[100, 64] = NAN, float("inf")
    Un, Vn = U.copy(), V.copy()
    Un[40, r - 1] = NAN
    Vn[r - 1, 129] = NAN
    with np.errstate(all="ignore"):
        want_l = orc.mu_betadivmin(Un, V, X, beta).T                        # r x m
        want_r = orc.switch_alternate_mu(X, U, Vn, beta, "V")               # r x n
    dev = lambda a, pad: place(torch.tensor(a, dtype=torch.float32), a.shape[1] + pad)
    for pad in (0, 5):
        Xd, Ud, Und, Vd, Vnd = dev(X, pad), dev(U.T, pad), dev(Un.T, pad), dev(V, pad), dev(Vn, pad)
        out = nan_out(r, m, pad > 0)
        got = eng.mu_left(Xd, Und, Vd, beta, out=out)
        assert got.data_ptr() == out.data_ptr()
        check_nonfinite(f"left beta={beta} pad={pad}", got.cpu().numpy(), want_l, "nonfinite_left", beta)
        out = nan_out(r, n, pad > 0)
        got = eng.mu_right(Xd, Ud, Vnd, beta, out=out)
        check_nonfinite(f"right beta={beta} pad={pad}", got.cpu().numpy(), want_r, "nonfinite_right", beta)
        num, den, dvec = eng.mu_right_accum(Xd, Ud, Vnd, beta)
        check_nonfinite(f"accum + apply beta={beta} pad={pad}", eng.mu_apply(Vnd, num, den, dvec, beta).cpu().numpy(), want_r,
                        "nonfinite_right", beta)
    assert math.isnan(want_l[0, 17]) and math.isinf(want_l[0, 100]) and math.isnan(want_r[0, 200]) and math.isinf(want_r[0, 64])

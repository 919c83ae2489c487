"""Every launch plan of the tensor side (k_mttkrp.hip, the CP cost of k_cost.hip), against fp64.  Needs a MI355X, except for
test_tensor_cases_reach_required.

launch_seg (MTTKRP modes 0 and 1), launch_rows (mode 2), nnf_mttkrp3_from_partial_f32 (dimension tree) and the cost pass with
Khatri-Rao rows (nnf_cp3_betadiv_f32) pick a plan from the shape, the rank, the alignment and strides of the operands, the CU
count and the free workspace.  tensor_cases(C) names the plan every case must take, with its shape written from the CU count so
that each case sits on the side of a threshold it says it does.  test_tensor_cases_reach_required checks the table against a
Python restatement of the four plan formulas (no GPU; tests/test_mu_plan_table.py checks every row, and the restatement of it,
against the library's own plan arithmetic through tools/nnf_plan.cpp, without a GPU either), test_tensor_plan_table against the
library's own report (NNF_PLAN_DEBUG), test_tensor_values / test_cp3_cost check every case against a plain fp64 evaluation on the
device.

Bounds, and where each comes from:
  * exact inputs (small integers of both signs, sum |T| |Fa| |Fb| < 2^24 for every output, asserted on the fp64 reference of
    the absolute values): every product, every fp32 partial sum in any order, every fp64 slab sum and the final rounding are
    exact, so the kernel must equal the fp64 evaluation bit for bit (torch.equal) whatever the plan.  No tolerance.
  * realistic inputs (positive uniform data, reductions up to the 250000 of bench config D): global 1e-5 and entrywise 1e-4, the
    bounds test_gpu_launch_plans.test_plan_values uses for products, and for every entry the order-free bound
    |got - want| <= (n + 2) * 2^-24 * sum |terms| (n terms rounded once each as products -- here exact or one rounding of the
    Khatri-Rao entry -- and at most n - 1 fp32 additions, each relative 2^-24, plus the final rounding).
  * CP cost: realistic data within 1e-5 of the fp64 beta-divergence of the same fp32 inputs (test_plan_values' bound for
    `cost`); planted residuals 2^p on an integer model give 0.5 * sum 4^p exactly.

Branches no case can reach:
  * partial_mid bound=grid: nchunk > 65535 needs 4 * CUs / (cb * R) > 65535, i.e. more than 16383 CUs.
  * launch_rows NNF_ERR_UNSUPPORTED (rps <= 64 inside the halving): 192 * n * 4 >= 0x7fff0000 is a tensor row of 11 MB, and
    a T of 64 such rows with its fp64 reference is beyond the free-memory guard.
  * "rps % nb != 0" for nb in {1, 2, 4, 64}: rows per split are a multiple of 64, so these nb always start a split at j = 0;
    the cases with nb in {3, 5, 63, 65, 500} start splits inside an i.
  * launch_seg's second refusal (16 * MT * lds * 4 >= 0x7fff0000) needs a 2 GB factor on the segment side; the rows kernel's
    krf=0 case holds the same stride and covers the arithmetic, mode 0/1 would only return the status.
"""
import collections
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_launch_plans import _cdiv, _cus, _halved, _splits, assert_close, engine_for, parse_plans

gpu = pytest.mark.gpu        # per test: test_tensor_cases_reach_required runs without a device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = 0x7fff0000
WS_DEFAULT = 1024 << 20                 # get_engine's context
ERR_UNSUPPORTED, ERR_WORKSPACE = -3, -4
BIG_FREE = 16 << 30                     # the large-memory cases need this much free device memory

# kernel: "mttkrp" (shape I, J, K; mode 0..2), "partial" (shape A, B; mode = axis 1 or 2), "cp3" (shape I, J, K; mode None).
# ld: extra floats of row stride {"f0", "f1", "f2", "out"} (the padding holds NaN; "partial" has one factor, "f1"); align: offset in floats of the base of
# {"T", "f0", "f1", "f2"} from an aligned allocation; ws: context workspace in bytes (None: the process engine's);
# expect: the fields the library must report, or {"status": s} for a refusal.
Case = collections.namedtuple("Case", "kernel shape R mode ld align ws beta expect")


def _rup(a, b):
    return _cdiv(a, b) * b


# ---------------------------------------------------------------------------------------------------------------------------
# the four plan formulas, restated
# ---------------------------------------------------------------------------------------------------------------------------
def seg_plan(C, nrows, ldrow, nseg, segstride, klen, R, ws, t_off, fs_ld, fk_ld, fk_off):
    mt = _cdiv(R, 16)
    if (64 * ldrow + klen + 256) * 4 >= LIM or 16 * mt * fs_ld * 4 >= LIM:
        return {"status": ERR_UNSUPPORTED}
    nrb = _cdiv(nrows, 256)
    nsplit, bound = 2 * C // nrb, "occupancy"
    if nsplit < 1:
        nsplit, bound = 1, "one"
    if nsplit > nseg:
        nsplit, bound = nseg, "segments"
    ws_max = (ws // 4) // (R * _rup(nrows, 4))
    if ws_max < 1:
        return {"status": ERR_WORKSPACE}
    if nsplit > ws_max:
        nsplit, bound = ws_max, "workspace"
    sps = _cdiv(nseg, nsplit)
    nsplit = _cdiv(nseg, sps)
    return dict(nrows=nrows, nseg=nseg, klen=klen, r=R, mt=mt, VEC=int(t_off % 4 == 0 and ldrow % 4 == 0 and segstride % 4 == 0),
                fkvec=int(fk_off % 4 == 0 and fk_ld % 4 == 0), pp=int(mt <= 2), nsplit=nsplit, sps=sps, bound=bound)


def rows_plan(C, m, n, nb, R, ws, t_off, lda, ldb):
    mt = _cdiv(R, 16)
    ncb = _cdiv(n, 256)
    nsplit, bound = max(1, 2 * C // ncb), "occupancy"
    if nsplit > _cdiv(m, 64):
        nsplit, bound = _cdiv(m, 64), "rows"
    ws_max = (ws // 4) // (R * _rup(n, 4))
    if ws_max < 1:
        return {"status": ERR_WORKSPACE}
    if nsplit > ws_max:
        nsplit, bound = ws_max, "workspace"
    rps = _rup(_cdiv(m, nsplit), 64)
    while (rps + 128) * n * 4 >= LIM:
        if rps <= 64:
            return {"status": ERR_UNSUPPORTED}
        rps, bound = _rup(rps // 2, 64), "offset32"
    nsplit = _cdiv(m, rps)
    if nsplit > ws_max:
        return {"status": ERR_WORKSPACE}
    krf = nb >= 4 and 16 * mt * lda * 4 < LIM and 16 * mt * ldb * 4 < LIM
    return dict(m=m, n=n, nb=nb, r=R, mt=mt, VEC=int(t_off % 4 == 0 and n % 4 == 0), krf=int(krf),
                krdiv="slow" if not krf else ("carry" if nb >= 64 else "redivide"), nsplit=nsplit, rps=rps, bound=bound)


def partial_plan(C, A, B, R, axis, ws):
    """One pass (R <= 128)."""
    if axis == 2:
        grid = min(_cdiv(R * A, 4), 8192)
        return dict(A=A, B=B, r=R, grid=grid, strided=int(R * A > 4 * grid))
    cb = _cdiv(B, 256)
    nchunk, bound = max(1, _cdiv(4 * C, cb * R)), "occupancy"
    if nchunk > _cdiv(A, 16):
        nchunk, bound = _cdiv(A, 16), "rows16"
    if nchunk > 65535:
        nchunk, bound = 65535, "grid"
    a_per = _cdiv(A, nchunk)
    nchunk = _cdiv(A, a_per)
    if nchunk * R * _rup(B, 4) * 4 > ws:
        return {"status": ERR_WORKSPACE}
    if cb > 65535:
        return {"status": ERR_UNSUPPORTED}
    return dict(A=A, B=B, r=R, nchunk=nchunk, a_per=a_per, bound=bound)


def cp3_plan(C, I, J, K, R, t_off):
    """The last (or only) rank pass of the CP cost: T as an (I J) x K matrix, Khatri-Rao rows on the left (no column-split cap)."""
    r = R - 128 * ((R - 1) // 128)
    grid, nblk = _cdiv(I * J, 128), _cdiv(K, 64)
    csplit = max(1, min(_cdiv(16 * C, grid), nblk // 4))
    KS = _cdiv(r, 4)
    wg = lambda b: min(3, (160 * 1024) // b)
    shm2 = 4 * 2 * KS * 64 * 4 + 2 * KS * 64 * 16 + 64
    vdb = 0 if wg(shm2 - KS * 64 * 16) > wg(shm2) else 1
    pin = int(R > 128)
    return dict(m=I * J, n=K, r=r, grid=grid, csplit=csplit, NN=8 if (pin or KS > 16) else 4, vdb=vdb,
                VEC=int(t_off % 4 == 0 and K % 4 == 0), pin=pin, kr=J)


def plan_of(C, case):
    """What the restated formulas give for a case (of its first rank pass; the CP cost: of its last)."""
    ld, al = case.ld or {}, case.align or {}
    ws = WS_DEFAULT if case.ws is None else case.ws
    R = min(case.R, 128)
    if case.kernel == "mttkrp":
        I, J, K = case.shape
        l0, l1, l2 = I + ld.get("f0", 0), J + ld.get("f1", 0), K + ld.get("f2", 0)
        if case.mode == 0:
            return seg_plan(C, I, J * K, J, K, K, R, ws, al.get("T", 0), l1, l2, al.get("f2", 0))
        if case.mode == 1:
            return seg_plan(C, J, K, I, J * K, K, R, ws, al.get("T", 0), l0, l2, al.get("f2", 0))
        return rows_plan(C, I * J, K, J, R, ws, al.get("T", 0), l0, l1)
    if case.kernel == "partial":
        return partial_plan(C, case.shape[0], case.shape[1], R, case.mode, ws)
    return cp3_plan(C, *case.shape, case.R, al.get("T", 0))


def launcher_of(case):
    if case.kernel == "mttkrp":
        return "mttkrp_rows" if case.mode == 2 else "mttkrp_seg"
    if case.kernel == "partial":
        return "partial_last" if case.mode == 2 else "partial_mid"
    return "cost"


# ---------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------
MT_RANKS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 81, 95, 96, 97, 112, 113, 127, 128]
PAD = {"f0": 3, "f1": 5, "f2": 4, "out": 7}


def tensor_cases(C):
    """{name: Case} for a device with C compute units."""
    cases = {}

    def add(name, kernel, shape, R, mode, expect, ld=None, align=None, ws=None, beta=None):
        assert name not in cases, name
        cases[name] = Case(kernel, tuple(shape), R, mode, ld, align, ws, beta, expect)

    def seg(name, mode, nrows, nseg, klen, R, expect, **kw):
        """Mode 0: rows i, segments j.  Mode 1: rows j, segments i (ldrow and segstride change places)."""
        add(f"seg{mode}_{name}", "mttkrp", (nrows, nseg, klen) if mode == 0 else (nseg, nrows, klen), R, mode, expect, **kw)

    for mode in (0, 1):
        # ---- rank tiles: MT 1..8, the two-register-set pipeline up to rank 32, one workgroup per SIMD pair above rank 64 ----
        for R in MT_RANKS:
            seg(f"r{R}", mode, 70, 9, 37, R, dict(mt=_cdiv(R, 16), pp=int(R <= 32), bound="segments", nsplit=9, sps=1, VEC=0))
        seg("r200", mode, 70, 9, 37, 200, dict(r=128, mt=8, pp=0))       # two rank passes, one report line each
        # ---- splits ----
        nseg = C + C // 2 + 1          # two row blocks: C splits asked for, two segments each -> re-rounded, the last one short
        seg("occupancy_rerounded", mode, 300, nseg, 8, 20, dict(bound="occupancy", sps=2, nsplit=_cdiv(nseg, 2)))
        seg("occupancy_r100", mode, 300, nseg, 129, 100, dict(mt=7, bound="occupancy", sps=2, nsplit=_cdiv(nseg, 2)))
        seg("segments", mode, 300, C - 1, 8, 20, dict(bound="segments", sps=1, nsplit=C - 1))
        seg("one_segment", mode, 300, 1, 40, 20, dict(bound="segments", sps=1, nsplit=1))
        slab = 20 * 100 * 4
        seg("workspace_two_slabs", mode, 100, 11, 24, 20, dict(bound="workspace", nsplit=2, sps=6), ws=2 * slab)   # last split: 5
        seg("workspace_one_slab", mode, 100, 11, 24, 20, dict(bound="workspace", nsplit=1, sps=11), ws=slab)
        seg("workspace_short", mode, 100, 11, 24, 20, dict(status=ERR_WORKSPACE), ws=slab - 4)
        # ---- rows: waves without rows, partial waves, a second row block ----
        for nrows in (1, 63, 64, 65, 255, 256, 257):
            seg(f"rows{nrows}", mode, nrows, 5, 40, 18, dict(nrows=nrows, VEC=1, fkvec=1, bound="segments"))
            seg(f"rows{nrows}_r70", mode, nrows, 5, 40, 70, dict(nrows=nrows, mt=5, pp=0, bound="segments"))
        # ---- the segment length: ragged tail (krem < 4) and the 64-column chunk edge, both load widths ----
        for klen in (1, 3, 4, 63, 64, 65, 127, 128, 129):
            seg(f"klen{klen}", mode, 70, 6, klen, 18, dict(klen=klen, VEC=int(klen % 4 == 0)))
            seg(f"klen{klen}_r40", mode, 70, 6, klen, 40, dict(klen=klen, pp=0, VEC=int(klen % 4 == 0)))     # one register set
            if klen % 4 == 0:
                seg(f"klen{klen}_offset_T", mode, 70, 6, klen, 18, dict(klen=klen, VEC=0), align={"T": 1})
        # (mode 0: J K is a multiple of 4, the segment stride K is not; mode 1 the other way round)
        seg("klen6_even_nseg", mode, 70, 6, 6, 18, dict(klen=6, VEC=0))
        # ---- the inner factor ----
        seg("fk_odd_ld", mode, 70, 6, 64, 18, dict(VEC=1, fkvec=0), ld={"f2": 1})
        seg("fk_offset", mode, 70, 6, 64, 18, dict(VEC=1, fkvec=0), align={"f2": 1})
        seg("padded", mode, 70, 6, 64, 40, dict(VEC=1, fkvec=1), ld=PAD)
    # more row blocks than twice the CUs: one split
    add("seg1_one_split", "mttkrp", (3, 512 * C + 1, 8), 5, 1, dict(bound="one", nsplit=1, sps=3))
    # the 31-bit offset of a wave's 64 rows: the last J K that fits (K = 4: J K is then the largest multiple of 4), and the next
    jk = ((LIM // 4 - 1 - 4 - 256) // 64) // 4 * 4
    assert (64 * jk + 4 + 256) * 4 < LIM <= (64 * (jk + 4) + 4 + 256) * 4
    add("big_seg0_offset_limit", "mttkrp", (65, jk // 4, 4), 17, 0, dict(mt=2, VEC=1, bound="occupancy", nsplit=2 * C))
    add("seg0_offset_refused", "mttkrp", (2, jk // 4 + 1, 4), 17, 0, dict(status=ERR_UNSUPPORTED))

    # ---- the rows kernel (mode 2): T as an (I J) x K matrix, nb = J ----
    def rows(name, I, J, K, R, expect, **kw):
        add(f"rows_{name}", "mttkrp", (I, J, K), R, 2, expect, **kw)

    for R in MT_RANKS:      # 63 rows: a single partial chunk
        rows(f"r{R}", 7, 9, 40 if R % 2 else 37, R, dict(mt=_cdiv(R, 16), VEC=R % 2, krf=1, krdiv="redivide", nsplit=1, bound="rows"))
    rows("offset_T", 7, 9, 40, 18, dict(VEC=0), align={"T": 1})
    rows("r200", 7, 9, 40, 200, dict(r=128, mt=8, krf=1))
    # nb: the slow form below 4, the (i, j) pair divided again every chunk below 64, carried from 64; 64-row splits
    for J, I, div in [(1, 200, "slow"), (2, 100, "slow"), (3, 67, "slow"), (4, 50, "redivide"), (5, 13, "redivide"),
                      (63, 5, "redivide"), (64, 3, "carry"), (65, 3, "carry"), (500, 2, "carry"), (9, 7, "redivide")]:
        m = I * J
        rows(f"nb{J}", I, J, 44, 21, dict(nb=J, krf=int(J >= 4), krdiv=div, bound="rows", rps=64, nsplit=_cdiv(m, 64)))
        rows(f"nb{J}_r70", I, J, 41, 70, dict(nb=J, mt=5, VEC=0, krdiv=div, bound="rows", rps=64, nsplit=_cdiv(m, 64)))
    m_occ = 65 * (_cdiv(128 * C, 65) + 1)           # more 64-row chunks than two workgroups per CU
    rows("occupancy", m_occ // 65, 65, 40, 21, dict(bound="occupancy", nsplit=_splits(m_occ, 2 * C)))
    rows("workspace", 40, 65, 40, 21, dict(bound="workspace", nsplit=_splits(2600, 3)), ws=3 * 21 * 40 * 4)
    rows("workspace_short", 40, 65, 40, 21, dict(status=ERR_WORKSPACE), ws=21 * 40 * 4 - 4)
    rows("padded", 6, 70, 64, 40, dict(VEC=1, krdiv="carry"), ld=PAD)
    # rows of a megabyte: one split (1024 column blocks), halved until (rps + 128) rows stay inside 31 bits
    Kw = 256 * 1024
    rps = _halved(2100, Kw)
    assert rps == 1088
    add("big_rows_offset32", "mttkrp", (21, 100, Kw), 4, 2, dict(bound="offset32", rps=rps, nsplit=_cdiv(2100, rps), krdiv="carry"))
    add("big_rows_offset32_one_slab", "mttkrp", (21, 100, Kw), 4, 2, dict(status=ERR_WORKSPACE), ws=4 * Kw * 4)
    # a factor whose padded rank rows leave 31-bit offsets: the slow Khatri-Rao form at nb >= 4
    L = _cdiv(LIM, 16 * 8 * 4)
    add("big_rows_krf0_stride", "mttkrp", (6, 70, 64), 113, 2, dict(krf=0, krdiv="slow", mt=8), ld={"f0": L - 6})

    # ---- dimension tree: axis 2 (rows of B entries, one wave each), axis 1 (columns, a-chunks into slabs) ----
    def part(name, axis, A, B, R, expect, **kw):
        add(f"part{axis}_{name}", "partial", (A, B), R, axis, expect, **kw)

    for B in (1, 63, 64, 65, 511, 512, 513, 1025):
        part(f"B{B}", 2, 7, B, 5, dict(B=B, strided=0))
    part("r1", 2, 1, 1, 1, dict(grid=1, strided=0))
    part("edge_lo", 2, 256, 65, 128, dict(grid=8192, strided=0))
    part("edge_hi", 2, 257, 65, 128, dict(grid=8192, strided=1))
    part("r129", 2, 300, 63, 129, dict(r=128, grid=8192, strided=1))
    part("r200", 2, 3, 513, 200, dict(r=128, strided=0), ld=PAD)
    part("padded", 2, 40, 70, 9, dict(strided=0), ld=PAD)
    A_occ = 16 * C + 40
    part("occupancy", 1, A_occ, 256, 4, dict(bound="occupancy", a_per=_cdiv(A_occ, C), nchunk=_cdiv(A_occ, _cdiv(A_occ, C))))
    assert _cdiv(A_occ, C) % 8 != 0
    for A in (1, 15, 16, 17):
        part(f"A{A}", 1, A, 100, 3, dict(bound="rows16", nchunk=_cdiv(A, 16), a_per=_cdiv(A, _cdiv(A, 16))))
    for B in (1, 255, 256, 257):
        part(f"B{B}", 1, 50, B, 6, dict(B=B, bound="rows16", nchunk=4, a_per=13))
    part("r129", 1, 50, 70, 129, dict(r=128, bound="rows16", nchunk=4, a_per=13))
    part("r200", 1, 20, 33, 200, dict(r=128), ld=PAD)
    part("padded", 1, 40, 70, 9, dict(bound="rows16"), ld=PAD)
    part("workspace_short", 1, 64, 1000, 8, dict(status=ERR_WORKSPACE), ws=4096)
    part("grid_refused", 1, 1, 256 * 65535 + 1, 1, dict(status=ERR_UNSUPPORTED))

    # ---- CP cost: the cost kernel with Khatri-Rao rows, 128-row tiles over (i, j) ----
    def cp3(name, I, J, K, R, beta, expect, **kw):
        add(f"cp3_{name}", "cp3", (I, J, K), R, None, dict(kr=J, **expect), beta=beta, **kw)

    betas = (2, 1, 0, 1.5)
    for n, (J, I) in enumerate([(1, 129), (2, 64), (127, 1), (128, 2), (129, 1), (300, 3), (17, 15)]):      # I J % 128: 1, 0, 127, 0, 1, 4, 127
        cp3(f"J{J}", I, J, 100, 20, betas[n % 4], dict(csplit=1, NN=4, VEC=1))
    for n, (R, nn, vdb) in enumerate([(1, 4, 1), (16, 4, 1), (17, 4, 1), (64, 4, 0), (65, 8, 0), (104, 8, 0), (128, 8, 1)]):
        cp3(f"r{R}", 9, 31, 100, R, betas[n % 4], dict(csplit=1, NN=nn, vdb=vdb))
    cp3("r129", 9, 31, 100, 129, 2, dict(r=1, pin=1, NN=8))
    cp3("r200", 9, 31, 70, 200, 1, dict(r=72, pin=1, NN=8, VEC=0))
    cp3("csplit_quarter", 9, 31, 1300, 20, 1.5, dict(csplit=5))
    Ic = _cdiv(1024 * C, 100)                        # 8 C row tiles: two column splits of the 13 blocks (13 / 4 = 3 allowed)
    cp3("csplit_occupancy", Ic, 100, 770, 20, 2, dict(csplit=2, grid=_cdiv(Ic * 100, 128), VEC=0))
    cp3("offset_T", 9, 31, 100, 20, 1, dict(VEC=0), align={"T": 1})
    cp3("odd_K", 9, 31, 99, 20, 0, dict(VEC=0))
    cp3("padded", 9, 31, 100, 20, 2, dict(VEC=1), ld=PAD)
    return cases


CASE_NAMES = list(tensor_cases(256))
REQUIRED = {("mttkrp_seg", "mt"): set("12345678"), ("mttkrp_seg", "VEC"): {"0", "1"}, ("mttkrp_seg", "fkvec"): {"0", "1"},
            ("mttkrp_seg", "pp"): {"0", "1"}, ("mttkrp_seg", "bound"): {"occupancy", "segments", "workspace", "one"},
            ("mttkrp_rows", "mt"): set("12345678"), ("mttkrp_rows", "VEC"): {"0", "1"}, ("mttkrp_rows", "krf"): {"0", "1"},
            ("mttkrp_rows", "krdiv"): {"carry", "redivide", "slow"},
            ("mttkrp_rows", "bound"): {"occupancy", "rows", "workspace", "offset32"},
            ("partial_last", "strided"): {"0", "1"}, ("partial_mid", "bound"): {"occupancy", "rows16"},
            ("cost", "NN"): {"4", "8"}, ("cost", "vdb"): {"0", "1"}, ("cost", "VEC"): {"0", "1"}, ("cost", "pin"): {"0", "1"},
            ("cost", "csplit"): {"1", "quarter", "occupancy"}}
REQUIRED_REFUSALS = {("mttkrp_seg", ERR_WORKSPACE), ("mttkrp_seg", ERR_UNSUPPORTED), ("mttkrp_rows", ERR_WORKSPACE),
                     ("partial_mid", ERR_WORKSPACE), ("partial_mid", ERR_UNSUPPORTED)}
TAG_KEYS = ("mt", "VEC", "fkvec", "pp", "krf", "krdiv", "bound", "strided", "NN", "vdb", "pin")


def _note(seen, launcher, kv):
    for key in TAG_KEYS:
        if key in kv:
            seen[(launcher, key)].add(str(kv[key]))
    if launcher == "cost" and int(kv["kr"]) > 0:
        cs, nblk = int(kv["csplit"]), _cdiv(int(kv["n"]), 64)
        seen[("cost", "csplit")].add("1" if cs == 1 else ("quarter" if cs == nblk // 4 else "occupancy"))


def _is_big(name):
    return name.startswith("big_")


def test_tensor_cases_reach_required():
    """The table as written reaches every tag and refusal REQUIRED names, and every field a case lists is what the restated
    plan formulas give, at 256 CUs and at 304 (no GPU)."""
    for C in (256, 304):
        cases = tensor_cases(C)
        seen, refused, bad = collections.defaultdict(set), set(), []
        for name, case in cases.items():
            plan = plan_of(C, case)
            if "status" in plan or "status" in case.expect:
                if plan != case.expect:
                    bad.append((name, plan, case.expect))
                refused.add((launcher_of(case), plan.get("status")))
                continue
            for key, want in case.expect.items():
                if str(plan.get(key)) != str(want):
                    bad.append((name, key, plan.get(key), want))
            _note(seen, launcher_of(case), plan)
        assert not bad, "\n".join(map(str, bad))
        for key, want in REQUIRED.items():
            assert want <= seen[key], (C, key, want - seen[key])
        assert REQUIRED_REFUSALS <= refused, REQUIRED_REFUSALS - refused
        # what the issue asks of single cases
        c = cases["seg0_occupancy_rerounded"]
        nseg = c.shape[1]
        assert C < nseg < 2 * C and c.expect["nsplit"] != C and nseg % c.expect["sps"] != 0          # re-rounded, last split short
        assert cases["seg1_one_split"].shape[1] > 512 * C
        assert any(c.kernel == "mttkrp" and c.mode == 2 and c.shape[0] * c.shape[1] < 64 for c in cases.values())
        assert {(c.shape[0] * c.shape[1]) % 64 for c in cases.values() if c.kernel == "mttkrp" and c.mode == 2} >= {1, 63}
        assert {(c.shape[0] * c.shape[1]) % 128 for c in cases.values() if c.kernel == "cp3"} >= {0, 1, 127}
        assert {c.beta for c in cases.values() if c.kernel == "cp3"} == {2, 1, 0, 1.5}
        nb_inside = {c.shape[1] for c in cases.values() if c.kernel == "mttkrp" and c.mode == 2 and "rps" in c.expect
                     and c.expect.get("nsplit", 1) > 1 and c.expect["rps"] % c.shape[1] != 0}
        assert nb_inside >= {3, 5, 63, 65, 500, 100}, nb_inside
        assert sum(_is_big(n) for n in cases) == 4      # three large tensors, one of them also on a one-slab engine


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _based(numel, off, dev):
    """A flat float32 buffer of `numel` entries starting `off` floats after an aligned allocation."""
    return torch.empty(numel + off, device=dev)[off:]


def _fill(dst, kind, lo, hi, g):
    """dst <- integers in [lo, hi] (kind "exact") or uniform (0.05, 1.05) (kind "real"), in pieces (no second full-size buffer)."""
    flat = dst.view(-1) if dst.is_contiguous() else None
    if flat is None:
        src = (torch.randint(lo, hi + 1, dst.shape, device=dst.device, generator=g).float() if kind == "exact"
               else torch.rand(dst.shape, device=dst.device, generator=g) + 0.05)
        dst.copy_(src)
        return
    step = 1 << 26
    for a in range(0, flat.numel(), step):
        piece = flat[a:a + step]
        if kind == "exact":
            piece.copy_(torch.randint(lo, hi + 1, piece.shape, device=dst.device, generator=g))
        else:
            piece.copy_(torch.rand(piece.shape, device=dst.device, generator=g) + 0.05)


def _factor(R, dim, pad, off, kind, lo, hi, g, dev):
    ld = dim + pad
    buf = _based(R * ld, off, dev).view(R, ld)
    if pad:
        buf.fill_(float("nan"))
    F = buf[:, :dim]
    _fill(F, kind, lo, hi, g)
    return F


def make_inputs(case, seed, kind, dev="cuda"):
    """{"T" | "Y", "Ft"}: integers of both signs ("exact": T in [-2, 2], factors in [-1, 2]; {-1, 0, 1} when a reduction of that
    range could pass 2^24) or positive uniform data ("real").  Every factor has its own stream of values, so that exchanged
    factors, a transposed index or a wrong i = row / nb change the result."""
    g = torch.Generator(device=dev).manual_seed(seed)
    ld, al = case.ld or {}, case.align or {}
    R = case.R
    if case.kernel == "partial":
        A, B = case.shape
        n = A if case.mode == 1 else B
        Y = torch.empty(R, A, B, device=dev)
        _fill(Y, kind, -2, 2, g)
        return {"Y": Y, "Ft": _factor(R, n, ld.get("f1", 0), al.get("f1", 0), kind, -1, 2, g, dev)}
    I, J, K = case.shape
    red = I * J * K // case.shape[case.mode] if case.kernel == "mttkrp" else R
    small = 8 * red >= 2 ** 24
    T = _based(I * J * K, al.get("T", 0), dev).view(I, J, K)
    _fill(T, kind, -1 if small else -2, 1 if small else 2, g)
    Ft = [_factor(R, d, ld.get(f"f{i}", 0), al.get(f"f{i}", 0), kind, -1, 1 if small else 2, g, dev) for i, d in enumerate(case.shape)]
    return {"T": T, "Ft": Ft}


def other_data(inp):
    """The same tensor with other factors of the same strides (for the call before the measured one)."""
    out = dict(inp)
    fs = inp["Ft"] if isinstance(inp["Ft"], list) else [inp["Ft"]]
    new = []
    for f in fs:
        buf = torch.full((f.shape[0], f.stride(0) if f.shape[0] > 1 else f.shape[1]), float("nan"), device=f.device)
        o = buf[:, :f.shape[1]]
        o.copy_(f * 3 + 1)
        new.append(o)
    out["Ft"] = new if isinstance(inp["Ft"], list) else new[0]
    return out


def out_buffer(case):
    """(buffer filled with NaN, the view the kernel writes)."""
    dim = case.shape[case.mode] if case.kernel == "mttkrp" else case.shape[2 - case.mode]
    buf = torch.full((case.R, dim + (case.ld or {}).get("out", 0)), float("nan"), device="cuda")
    return buf, buf[:, :dim]


def run_case(eng, case, inp, out=None):
    if case.kernel == "mttkrp":
        return eng.mttkrp3(inp["T"], inp["Ft"], case.mode, out=out)
    if case.kernel == "partial":
        return eng.mttkrp3_from_partial(inp["Y"], inp["Ft"], case.mode, out=out)
    return eng.cp3_betadiv(inp["T"], inp["Ft"], case.beta, out=out)


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references (plain torch)
# ---------------------------------------------------------------------------------------------------------------------------
def khatri_rao_t(Fa, Fb):
    """(R x a), (R x b) -> R x (a b), first index slowest."""
    return (Fa[:, :, None] * Fb[:, None, :]).reshape(Fa.shape[0], -1)


def mttkrp_fp64(T64, F, mode):
    """out[r][x] of the mode, fp64: the unfolding times the Khatri-Rao product of the two other factors."""
    I, J, K = T64.shape
    if mode == 0:
        return (T64.reshape(I, J * K) @ khatri_rao_t(F[1], F[2]).t()).t()
    if mode == 1:
        return torch.einsum("ijk,rik->rj", T64, F[0][:, :, None] * F[2][:, None, :])
    return (T64.reshape(I * J, K).t() @ khatri_rao_t(F[0], F[1]).t()).t()


def partial_fp64(Y64, F, axis):
    return torch.einsum("rab,ra->rb", Y64, F) if axis == 1 else torch.einsum("rab,rb->ra", Y64, F)


def reference(case, inp, absolute=False):
    f = (lambda t: t.abs().double()) if absolute else (lambda t: t.double())
    if case.kernel == "mttkrp":
        return mttkrp_fp64(f(inp["T"]), [f(x) for x in inp["Ft"]], case.mode)
    return partial_fp64(f(inp["Y"]), f(inp["Ft"]), case.mode)


def reduction_length(case):
    if case.kernel == "partial":
        return case.shape[0] if case.mode == 1 else case.shape[1]
    I, J, K = case.shape
    return I * J * K // case.shape[case.mode]


def betadiv_fp64(T, P, beta):
    if beta == 1:
        return float((T * torch.log(T / P) - T + P).sum())
    if beta == 2:
        return float(0.5 * ((T - P) ** 2).sum())
    if beta == 0:
        return float((T / P - torch.log(T / P) - 1).sum())
    return float(((T ** beta + (beta - 1) * P ** beta - beta * T * P ** (beta - 1)) / (beta * (beta - 1))).sum())


def cp_model_fp64(Ft):
    F = [f.double() for f in Ft]
    return torch.einsum("ri,rj,rk->ijk", *F)


def big_guard(name):
    if _is_big(name):
        free = torch.cuda.mem_get_info()[0]
        if free < BIG_FREE:
            pytest.skip(f"{name}: {free >> 30} GiB of device memory free, needs 16 GiB")


# ---------------------------------------------------------------------------------------------------------------------------
# the plan table, as the library reports it
# ---------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_tensor_plans as P
from nn_fac_amd.engine import EngineError
cases = P.tensor_cases(P._cus())
for name, case in cases.items():
    if P._is_big(name) and torch.cuda.mem_get_info()[0] < P.BIG_FREE:
        sys.stderr.write("[skipped] %s\n" % name)
        continue
    sys.stderr.write("[case] %s\n" % name)
    sys.stderr.flush()
    inp = P.make_inputs(case, 1, "real")
    eng = P.engine_for(case)
    try:
        P.run_case(eng, case, inp)
    except EngineError as e:
        sys.stderr.write("[nnf plan] refused status=%s\n" % str(e).split("status ")[1].split()[0])
    torch.cuda.synchronize()
    del inp
    torch.cuda.empty_cache()
print("done")
"""


@pytest.fixture(scope="module")
def reported(built_lib):
    p = subprocess.run([sys.executable, "-c", _CHILD], env=dict(os.environ, NNF_PLAN_DEBUG="1"), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    skipped = [l[10:].strip() for l in p.stderr.splitlines() if l.startswith("[skipped] ")]
    return parse_plans(p.stderr), skipped


@gpu
def test_tensor_plan_table(reported):
    """Every case takes the plan it is listed with (one report line of its launcher per rank pass, a refusal reports nothing),
    and the table as a whole reaches every tag and refusal of REQUIRED."""
    plans, skipped = reported
    cases = tensor_cases(_cus())
    assert all(_is_big(n) for n in skipped), skipped
    assert sorted(plans) == sorted(set(cases) - set(skipped))
    seen, refused, bad = collections.defaultdict(set), set(), []
    for name, case in cases.items():
        if name in skipped:
            continue
        lines = [kv for (l, kv) in plans[name] if l == launcher_of(case)]
        status = [int(kv["status"]) for (l, kv) in plans[name] if l == "refused"]
        if "status" in case.expect:
            if status != [case.expect["status"]] or lines:
                bad.append((name, "refusal", plans[name]))
            refused.add((launcher_of(case), status[0] if status else None))
            continue
        if status or len(lines) != _cdiv(case.R, 128):
            bad.append((name, "report lines", plans[name]))
            continue
        kv = lines[-1] if case.kernel == "cp3" else lines[0]
        for key, want in case.expect.items():
            if kv.get(key) != str(want):
                bad.append((name, key, kv.get(key), want))
        for key, want in plan_of(_cus(), case).items():          # and the whole line is what the restated formulas give
            if kv.get(key) != str(want):
                bad.append((name, "restated", key, kv.get(key), want))
        for l in lines:
            _note(seen, launcher_of(case), l)
    assert not bad, "\n".join(map(str, bad))
    print("reached:", {f"{l}.{k}": sorted(v) for (l, k), v in sorted(seen.items())}, "refusals:", sorted(refused),
          "skipped:", skipped)
    for key, want in REQUIRED.items():          # (offset32 is reached by a large-memory case only)
        assert want - ({"offset32"} if skipped else set()) <= seen[key], (key, want - seen[key])
    assert REQUIRED_REFUSALS <= refused, REQUIRED_REFUSALS - refused


# ---------------------------------------------------------------------------------------------------------------------------
# values: MTTKRP and dimension tree
# ---------------------------------------------------------------------------------------------------------------------------
def measured_call(eng, case, inp, what):
    """The case on `inp`, into a NaN-filled output right after a call on other data with the same engine: a tile or split left
    out shows as NaN or as the other call's value.  Returns the result (the padding of the output checked bit for bit)."""
    buf, out = out_buffer(case)
    run_case(eng, case, other_data(inp), out=out)
    buf.fill_(float("nan"))
    before = buf.view(torch.int32).clone()
    got = run_case(eng, case, inp, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr(), what
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries (a tile never written, or padding read)"
    assert torch.equal(buf.view(torch.int32)[:, out.shape[1]:], before[:, out.shape[1]:]), f"{what}: output padding written"
    return got


def assert_exact(got, want, what):
    if not torch.equal(got.double(), want):
        d = (got.double() - want)
        idx = torch.nonzero(d)
        r, x = (int(v) for v in idx[0])
        raise AssertionError(f"{what}: {idx.shape[0]} of {d.numel()} entries differ from the exact result; first at "
                             f"[{r}, {x}]: got {float(got[r, x])}, want {float(want[r, x])}")


VALUE_CASES = [n for n in CASE_NAMES if tensor_cases(256)[n].kernel != "cp3"]


@gpu
@pytest.mark.parametrize("name", VALUE_CASES)
def test_tensor_values(name, built_lib):
    """Exact inputs: the kernel equals the fp64 evaluation bit for bit.  Realistic inputs (reductions up to 250000): global 1e-5,
    entrywise 1e-4 and the order-free bound (n + 2) 2^-24 sum |terms| for every entry.  A refusal leaves `out` untouched."""
    from nn_fac_amd.engine import EngineError
    big_guard(name)
    case = tensor_cases(_cus())[name]
    eng = engine_for(case)
    torch.cuda.reset_peak_memory_stats()
    inp = make_inputs(case, 7, "exact")
    if "status" in case.expect:
        buf, out = out_buffer(case)
        with pytest.raises(EngineError, match=rf"status {case.expect['status']} "):
            run_case(eng, case, inp, out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all()), f"{name}: a refused call wrote its output"
        return
    got = measured_call(eng, case, inp, name)
    want = reference(case, inp)
    bound = float(reference(case, inp, absolute=True).max())
    assert bound < 2 ** 24, f"{name}: the exact inputs are not exact ({bound} >= 2^24)"       # an error of the test, not a skip
    assert_exact(got, want, name + " (exact inputs)")
    del inp, want, got
    n = reduction_length(case)
    if n <= 250000:
        inp = make_inputs(case, 11, "real")
        got = measured_call(eng, case, inp, name)
        want = reference(case, inp)
        assert_close(got, want, 1e-5, 1e-4, name + " (realistic inputs)")
        d = (got.double() - want).abs() - (n + 2) * 2.0 ** -24 * want          # positive data: sum |terms| = want
        assert float(d.max()) <= 0, f"{name}: entry {int(d.argmax())} is outside (n + 2) 2^-24 sum|terms| by {float(d.max()):.3e}"
    if _is_big(name):
        print(f"peak device memory {name}: {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ---------------------------------------------------------------------------------------------------------------------------
# values: CP cost
# ---------------------------------------------------------------------------------------------------------------------------
CP3_CASES = [n for n in CASE_NAMES if tensor_cases(256)[n].kernel == "cp3"]


def plant_positions(case, csplit):
    """Up to 12 (row, column) entries of the (I J) x K matrix where indexing goes wrong: first and last row of a 128-row tile,
    the rows where i wraps inside a tile, the last row (of a ragged tile); first and last column of every column split, the
    last column (of a ragged 64-block)."""
    I, J, K = case.shape
    m = I * J
    rows = [0, 127, 128, J - 1, J, 2 * J - 1, 128 + J - 128 % J, m - 1 - (m - 1) % 128, m - 1]
    per = _cdiv(_cdiv(K, 64), csplit)
    cols = [0, K - 1]
    for s in range(csplit):
        cols += [s * per * 64, min((s + 1) * per * 64, K) - 1]
    cols += [63, 64]
    rows = [r for n, r in enumerate(rows) if 0 <= r < m and r not in rows[:n]]
    cols = [c for n, c in enumerate(cols) if 0 <= c < K and c not in cols[:n]]
    pos = []
    for n in range(12 * len(rows) * len(cols)):
        p = (rows[n % len(rows)], cols[(n + n // len(rows)) % len(cols)])
        if p not in pos:
            pos.append(p)
        if len(pos) == 12:
            break
    return pos


def planted_cost(pos):
    """0.5 * sum 4^p: the beta = 2 cost of a tensor that is its model but for differences 2^p at the planted entries."""
    return 0.5 * sum(4.0 ** p for p in range(len(pos)))


def plant(T, model, pos):
    """T <- model, plus 2^p at plant p."""
    T.copy_(model)
    flat = T.view(-1, T.shape[2])
    for p, (row, col) in enumerate(pos):
        flat[row, col] += 2.0 ** p
    return T


def _call_cost(eng, case, inp, beta):
    out = torch.empty(1, dtype=torch.float64, device="cuda")
    eng.cp3_betadiv(inp["T"], other_data(inp)["Ft"], beta, out=out)
    out.fill_(1e300)
    return float(eng.cp3_betadiv(inp["T"], inp["Ft"], beta, out=out))


@gpu
@pytest.mark.parametrize("name", CP3_CASES)
def test_cp3_cost(name, built_lib):
    """(a) realistic data against the fp64 beta-divergence, 1e-5; (b) planted residuals on an integer model give 0.5 sum 4^p
    exactly; (c) rank <= 64: cp3_partial_cost gives twice that, bit for bit, and Y is the exact mode-2 product."""
    case = tensor_cases(_cus())[name]
    eng = engine_for(case)
    plan = plan_of(_cus(), case)
    # (a)
    inp = make_inputs(case, 13, "real")
    model = cp_model_fp64(inp["Ft"])
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.rand(model.shape, device="cuda", generator=g) * 2 - 1
    inp["T"].copy_((model * (1 + 0.05 * noise)).clamp_(min=1e-3))
    del noise
    want = betadiv_fp64(inp["T"].double(), model, case.beta)
    got = _call_cost(eng, case, inp, case.beta)
    print(f"{name}: beta {case.beta} got {got!r} want {want!r} rel {abs(got - want) / abs(want):.3e}")
    assert abs(got - want) <= 1e-5 * abs(want), (name, got, want)
    del inp, model
    # (b)
    inp = make_inputs(case, 17, "exact")
    model = cp_model_fp64(inp["Ft"])
    assert float(cp_model_fp64([f.abs() for f in inp["Ft"]]).max()) + 2 ** 12 < 2 ** 24
    pos = plant_positions(case, plan["csplit"])
    plant(inp["T"], model, pos)
    want = planted_cost(pos)
    assert betadiv_fp64(inp["T"].double(), model, 2) == want
    got = _call_cost(eng, case, inp, 2)
    if got != want:
        diff = int(round(2 * (got - want)))
        bits = [p for p in range(len(pos)) if (abs(diff) >> (2 * p)) & 3]
        raise AssertionError(f"{name}: cost {got} != {want}; 2 * difference {diff}: plants {[(p, pos[p]) for p in bits]} "
                             f"({'doubled or misplaced' if diff > 0 else 'missed'})")
    # (c)
    if case.R <= 64:
        I, J, K = case.shape
        cost = torch.empty(1, dtype=torch.float64, device="cuda")
        Y = torch.empty(case.R, I, J, device="cuda")
        eng.cp3_partial_cost(inp["T"], other_data(inp)["Ft"], Y, cost)
        Y.fill_(float("nan"))
        cost.fill_(1e300)
        eng.cp3_partial_cost(inp["T"], inp["Ft"], Y, cost)
        assert float(cost) == 2 * want, (name, float(cost), 2 * want)
        assert torch.equal(Y.double(), torch.einsum("ijk,rk->rij", inp["T"].double(), inp["Ft"][2].double())), name


# ---------------------------------------------------------------------------------------------------------------------------
# the same problem on two plans
# ---------------------------------------------------------------------------------------------------------------------------
def _same_problem(case, inp, **changes):
    """The case's exact inputs copied into the layout of `changes` (another alignment / stride / workspace)."""
    other = case._replace(**changes)
    new = make_inputs(other, 7, "exact")
    key = "T" if "T" in inp else "Y"
    new[key].copy_(inp[key])
    if isinstance(inp["Ft"], list):
        for a, b in zip(new["Ft"], inp["Ft"]):
            a.copy_(b)
    else:
        new["Ft"].copy_(inp["Ft"])
    return other, new


@gpu
@pytest.mark.parametrize("name,changes", [
    ("seg0_workspace_two_slabs", dict(ws=None)), ("seg1_workspace_one_slab", dict(ws=None)), ("rows_workspace", dict(ws=None)),
    ("seg0_klen64", dict(align={"T": 1})), ("seg1_klen128", dict(align={"T": 1})), ("rows_r17", dict(align={"T": 1})),
    ("rows_nb65", dict(align={"T": 1})), ("big_rows_krf0_stride", dict(ld=None))])
def test_bit_identity_between_plans(name, changes, built_lib):
    """On exact inputs fewer splits (small workspace), the scalar load path (T at an offset base) and the slow Khatri-Rao form
    give the very same bits as the default plan."""
    big_guard(name)
    case = tensor_cases(_cus())[name]
    inp = make_inputs(case, 7, "exact")
    a = run_case(engine_for(case), case, inp)
    other, inp2 = _same_problem(case, inp, **changes)
    assert plan_of(_cus(), other) != plan_of(_cus(), case), name
    b = run_case(engine_for(other), other, inp2)
    assert torch.equal(a, b), name
    assert_exact(a, reference(case, inp), name)


# ---------------------------------------------------------------------------------------------------------------------------
# the plan edges through the driver
# ---------------------------------------------------------------------------------------------------------------------------
_DRIVER_CHILD = r"""
import sys, os, math, numpy as np
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "oracle"))
import nnfac_oracle as orc
from nn_fac_amd.ntf import compute_ntf
rule, beta, shape, R = sys.argv[1], int(sys.argv[2]), tuple(int(v) for v in sys.argv[3].split("x")), int(sys.argv[4])
T, F0 = orc.synth_ntf(shape, R, seed=3, dtype=np.float32)
F, costs, _ = compute_ntf(T, R, F0, n_iter_max=3, tol=0, update_rule=rule, beta=beta, return_costs=True, alpha=math.inf,
                          sparsity_coefficients=[None] * 3, normalize=[False] * 3)
Fo, co, _ = orc.compute_ntf(T.astype(np.float64), R, [f.astype(np.float64) for f in F0], n_iter_max=3, tol=0,
                            update_rule=rule, beta=beta, return_costs=True, alpha=math.inf)
rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
print("result", max(rel(F[i], Fo[i]) for i in range(3)), float(np.max(np.abs(np.asarray(costs) - co) / np.abs(co))))
"""


@gpu
@pytest.mark.parametrize("route,rule,beta,env,launchers", [
    ("tree", "hals", 2, {}, ["mttkrp_rows m=4095 n=129 nb=65 r=33 mt=3", "partial_last A=63 B=65 r=33", "partial_mid A=63 B=65 r=33"]),
    ("direct", "hals", 2, {"NNF_COST": "direct"}, ["mttkrp_rows m=4095 n=129 nb=65 r=33 mt=3", "mu_left m=4095 n=129 r=33", "bm=FROB"]),
    ("mu_kl", "mu", 1, {}, ["mu_right m=", "cost m=4095 n=129 r=33 op=kl", "kr=65"])])
def test_driver_reaches_plan_edges(route, rule, beta, env, launchers, built_lib):
    """One ntf() run per route at a shape on the plan edges above (63 x 65 x 129: a partial wave, nb = 65, a ragged chunk after
    two full ones; rank 33: three rank tiles, no second register set) against the fp64 oracle, with test_gpu_ntf.py's
    tolerances (HALS 2e-3, MU 5e-5); the route's launches appear in the report (the pass over T that NNF_COST=direct asks for is
    the fused cost-and-partial-product kernel up to rank 64, the MU cost is the cost kernel with Khatri-Rao rows)."""
    p = subprocess.run([sys.executable, "-c", _DRIVER_CHILD, rule, str(beta), "63x65x129", "33"],
                       env=dict(os.environ, NNF_PLAN_DEBUG="1", **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    relF, relC = (float(v) for v in [l for l in p.stdout.splitlines() if l.startswith("result")][0].split()[1:])
    tol = 2e-3 if rule == "hals" else 5e-5
    print(route, relF, relC)
    assert relF < tol and relC <= tol, (route, relF, relC)
    report = [l for l in p.stderr.splitlines() if l.startswith("[nnf plan] ")]
    for want in launchers:
        assert any(want in l for l in report), (route, want, sorted(set(report)))

"""Every HALS sweep plan (k_hals_plan.h: hals_make_plan) and kernel instance against fp64.  Needs a MI355X, except
test_hals_cases_reach_required; test_hals_plan_table.py checks the same table against the plan header without one.

hals_make_plan picks one of eight layouts from the shape of a call and the CU count: wave (k_hals_wave.hip, one wave per column,
CPW columns per compute wave), quad (k_hals_quad.hip, CH rows per lane), mfma (k_hals_mfma.hip, padded rank RP), the lane
kernel resident or streaming (k_hals_fast.hip, RP), and the generic kernel with the column in LDS, in LDS four lanes per column
(LDS-big, ranks above 128) or in global memory (GCOL).  hals_cases(C) names the plan every case must take, with shapes written
from the CU count and the pinned per-CU figures PER_CU so that each case sits exactly on the side of a threshold it says it
does; test_hals_plan_table checks that against the library's report (NNF_HALS_DEBUG), and test_hals_plan_values runs every
case against oracle/nnfac_oracle.py's hals_nnls_acc in fp64 on the fp32-rounded inputs.

PER_CU holds the workgroups per CU the plan relied on, as the MI355X reported them (256 CUs): an occupancy change moves cases
to other layouts, and the table test then fails by name.  One threshold has no case: wave's `need <= 384` never binds there,
since a 12-wave workgroup holds one workgroup per CU (PER_CU wave nw=12) and 256 <= 384.

Values (fixed sweep count: mode 0 with delta = 0, or mode 1).  The Gram is "sharp": G = S (I + E) S with E symmetric, zero on
the diagonal, |E| row sums <= 0.4, S = diag(0.8 .. 1.25), so that rho = max_k sum_{i != k} |G_ki| / G_kk < 1.  UtM = G W with W
of mixed sign (entries get projected to zero) and a few start values below zero.  A row update is
    v_k <- max(v_k + (UtM_k - sp - G_k . v) / G_kk, 0) = max((UtM_k - sp - sum_{i != k} G_ki v_i) / G_kk, 0),
a 1-Lipschitz function of the other entries.  Its fp32 evaluation (an FMA chain of length r, the subtraction, the reciprocal,
the add; or a residual pushed up to REFRESH = 8 sweeps between re-formations) is off by at most
    l_k = KAPPA (r + 3) u (|G_k| |v| + |UtM_k| + sp) / G_kk + 2 u |v_k'|,     u = 2^-24,  KAPPA = 2 min(s, REFRESH)
per entry, with |v| the larger of the entries before and after the sweep.  An error e in the other entries moves v_k by at most
sum_i |G_ki| / G_kk e_i, so the errors after sweep s obey  e_s <= (I - |L'|)^-1 (|U'| e_{s-1} + l_s)  (L', U' the strictly lower /
upper parts of D^-1 |G|), evaluated along the oracle's trajectory.  Every entry of V must be within e_s; the per-sweep sums
within the Cauchy-Schwarz image  | ||a||^2 - ||b||^2 | <= (2 ||b|| + ||a - b||) ||a - b||  of the step errors.  Rows with a zero
Gram diagonal are skipped (nnls.py:160): bit for bit their start values.

Every call writes into NaN-filled outputs (V_out of a cross solve, the snapshots) right after a call on other data in the same
plan (same engine: the workspace holds that call's Gram image, barrier words and slots).  Inputs stay bit-identical, padding
columns of V keep their sentinel bits, NaN in the padding of UtM, UtU and V_in does not leak.  Many columns: one block of columns
the oracle solves, tiled (columns are independent when delta = 0).

Stop rule (test_hals_stop_rule): NMF-like positive Grams; delta sits at the geometric mean of the oracle's ratios after sweeps
c - 1 and c (>= 2 % from each), so the oracle stops at sweep c.  Sweep counts equal, V within the suite's solve tolerance of the
oracle's V after sweep c and clear of the V after sweeps c - 1 and c + 1.
"""
import collections
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import nnfac_oracle as orc  # noqa: E402

U32 = 2.0 ** -24
REFRESH = 8               # WAVE_REFRESH / MFMA_NREF_V: sweeps between re-formations of a pushed residual
UNSUP = -3                # NNF_ERR_UNSUPPORTED
SP = 0.05                 # sparsity coefficient of the "sp" cases
BLOCK = 2048              # columns the oracle solves for a tiled case

# workgroups per CU the plan relies on, as reported on the MI355X (NNF_HALS_DEBUG, 256 CUs)
PER_CU = {}
for _ru in range(8, 129, 8):
    PER_CU[("wave", _ru, 1, 1)] = 4 if _ru <= 64 else 3 if _ru == 72 else 2
    PER_CU[("wave", _ru, 1, 2)] = 3 if _ru <= 72 else 2
    PER_CU[("wave", _ru, 1, 12)] = 1
    PER_CU[("wave", _ru, 2, 12)] = 1
for _ch in range(1, 33):
    PER_CU[("quad", _ch)] = 8 if _ch <= 15 else 7 if _ch == 16 else 6 if _ch <= 18 else 5 if _ch <= 20 else 4 if _ch == 21 \
        else 3 if _ch <= 24 else 2
RPS = (8, 16, 24, 32, 40, 48, 50, 52, 56, 64, 80, 96, 100, 104, 112, 128)
MFMA_RPS = (48, 50, 52, 64, 80, 96, 100)
for _rp in RPS:
    PER_CU[("lane-resident", _rp)] = 3 if _rp <= 16 else 2
    PER_CU[("lane-streaming", _rp)] = 3 if _rp <= 32 else 2
for _rp in MFMA_RPS:
    PER_CU[("mfma", _rp)] = 2
PER_CU.update({("generic-lds", 8): 4, ("generic-lds", 20): 4, ("generic-lds", 100): 2, ("generic-lds", 128): 2,
               ("generic-lds-big", 129): 8, ("generic-lds-big", 200): 5, ("generic-lds-big", 600): 2, ("generic-gcol", 0): 4})


def _cdiv(a, b):
    return -(-a // b)


def pick_rp(r):
    for o in RPS:
        if r <= o:
            return o
    return (r + 7) & ~7


def wave_nw(n):
    return min(max(_cdiv(n, 256), 1), 12)


Case = collections.namedtuple("Case", "entry r n ld flags force gram2 budget opts expect")


def hals_cases(C):
    """{name: Case} for a device with C compute units.
    entry: solve | cross (V_in -> V_out, optional second Gram) | sweeps (mode 1) | snap (mode 1 with snapshots) | cont (a solve
    chained by nnf_hals_solve_continue_f32) | chunks (mode 1 in two calls handing the residual state on) | csolve (the C entry
    point itself, normalize=True); ld: padding columns {ldm, ldv, ldvs, ldg} (or a stride, "ldv_abs" ...); flags: "", "sp",
    "norm", "nz"; expect: the report's fields (the last report line of the case)."""
    cases = {}

    def add(name, entry, r, n, expect, ld=None, flags="", force=None, gram2=False, budget=4, **opts):
        assert name not in cases, name
        cases[name] = Case(entry, r, n, ld or {}, flags, force, gram2, budget, opts, expect)

    def wave(r, n, cpw, **kw):
        nw = wave_nw(n)
        pc = PER_CU[("wave", (r + 7) & ~7, cpw, nw if nw in (1, 2) else 12)] if nw in (1, 2, 12) else None
        e = dict(layout="wave", cpw=cpw, nw=nw, grid=_cdiv(n, nw * cpw), err=0, **kw)
        if pc is not None:
            e["per_cu"] = pc
        return e

    def quad(r, n, **kw):
        ch = (r + 3) // 4
        return dict(layout="quad", ch=ch, grid=_cdiv(n, 16), per_cu=PER_CU[("quad", ch)], err=0, **kw)

    def lane(r, n, res=True, **kw):
        rp = pick_rp(r)
        lay = "lane-resident" if res else "lane-streaming"
        pc = PER_CU[(lay, rp)]
        return dict(layout=lay, RP=rp, gs=int(32 < rp <= 52), per_cu=pc,
                    grid=_cdiv(n, 256) if res else min(pc * C, 2048), err=0, **kw)

    def mfma(r, n, **kw):
        rp = pick_rp(r)
        return dict(layout="mfma", RP=rp, gs=int(32 < rp <= 52), per_cu=PER_CU[("mfma", rp)], grid=_cdiv(n, 256), err=0, **kw)

    def generic(form, r, n, key=None, **kw):
        per = 32 if form == "generic-lds-big" else 128
        return dict(layout=form, RP=pick_rp(r), gs=0, per_cu=PER_CU[(form, r if key is None else key)], grid=_cdiv(n, per), err=0,
                    **kw)

    w12 = 12 * min(384, PER_CU[("wave", 8, 1, 12)] * C)         # the most columns a 1-column-per-wave solve holds
    w24 = 24 * min(384, PER_CU[("wave", 8, 2, 12)] * C)         # ... 2 columns per wave
    # ---- wave: every (RU, CPW); CPW 1 at its limit, CPW 2 one past it; padding of every operand on half of them ----
    for ru in range(8, 129, 8):
        r = ru - (ru // 8) % 3                                  # ranks 8k, 8k - 1 and 8k - 2 (padding rows of the image)
        pad = dict(ldm=3, ldv=5, ldg=2) if ru % 16 else {}
        add(f"wave_ru{ru}_cpw1_limit", "solve", r, w12, wave(r, w12, 1, prep=0, copy=0), ld=pad)
        add(f"wave_ru{ru}_cpw2", "solve", r, w12 + 1, wave(r, w12 + 1, 2, prep=0, copy=0), ld=pad, budget=3)
    add("wave_cpw2_limit", "solve", 30, w24, wave(30, w24, 2))
    add("wave_cpw2_over_quad", "solve", 30, w24 + 1, quad(30, w24 + 1))
    add("wave_forced_over_refused", "solve", 30, w24 + 1, dict(err=UNSUP), force="wave")
    # ncols edges (nw 1 / 2, ragged last compute wave)
    for n in (1, 15, 16, 17, 255, 256, 257):
        add(f"wave_n{n}", "solve", 13, n, wave(13, n, 1), ld=dict(ldv=3, ldm=1))
    # features: second Gram, separate start values, sparsity, zero diagonal, no sweep
    add("wave_cross_gram2", "cross", 40, 700, wave(40, 700, 1, hadamard=0, copy=0, prep=0), gram2=True, ld=dict(ldv=2, ldvs=7, ldg=3))
    add("wave_cross_sp", "cross", 20, 500, wave(20, 500, 1, copy=0), flags="sp", ld=dict(ldvs=1))
    add("wave_zero_diag", "solve", 50, 900, wave(50, 900, 1), zero_diag=(0, 17, 49))
    add("wave_no_sweep", "cross", 24, 600, wave(24, 600, 1, prep=1, copy=1), budget=0, ld=dict(ldvs=4, ldv=1))

    # ---- quad: every CH (mode 1: no wave); the 32768-column and the per-CU caps ----
    for ch in range(1, 33):
        r = 4 * ch - (ch % 4)                                   # rows per lane ch, the last lane partly padding
        r = max(r, 1)
        add(f"quad_ch{ch}", "sweeps", r, 700, quad(r, 700), ld=dict(ldm=2, ldv=1, ldg=1) if ch % 2 else {}, budget=3)
    add("quad_n32768", "sweeps", 20, 32768, quad(20, 32768), budget=3)
    add("quad_n32769_lane", "sweeps", 20, 32769, lane(20, 32769), budget=3)
    nq = 16 * PER_CU[("quad", 25)] * C                          # CH 25: 2 per CU
    add("quad_ch25_cap", "solve", 100, nq, quad(100, nq), budget=3)
    add("quad_ch25_cap_over_lane", "solve", 100, nq + 1, lane(100, nq + 1), budget=3)
    for n in (1, 15, 16, 17, 255, 256, 257):
        add(f"quad_n{n}", "sweeps", 37, n, quad(37, n), ld=dict(ldv=2))
    add("quad_cross_gram2", "cross", 30, w24 + 100, quad(30, w24 + 100, hadamard=0, copy=0), gram2=True, ld=dict(ldvs=3, ldg=2))
    add("quad_cross_sp_zero_diag", "cross", 61, 8000, quad(61, 8000, copy=0), flags="sp", zero_diag=(3, 60), ld=dict(ldvs=9))
    add("quad_forced_cross", "cross", 12, 900, quad(12, 900, copy=0), force="quad", ld=dict(ldvs=5))
    add("quad_cont", "cont", 44, 5000, quad(44, 5000), budget=3)
    add("quad_snap", "snap", 28, 3000, quad(28, 3000), budget=4)
    add("quad_no_sweep", "cross", 24, 20000, quad(24, 20000, copy=1, prep=1), budget=0, ld=dict(ldvs=2))
    add("lane_no_sweep", "cross", 24, 40000, dict(layout="lane-resident", copy=1, prep=1, err=0), budget=0, ld=dict(ldvs=2))
    # start values with a stride past quad's 32-bit offsets (rows up to r + 15): copied into V first; at the limit: read
    lim = (0x7fff0000 - 1) // (4 * (2 + 16))
    add("quad_ldvs_limit", "cross", 2, 1000, quad(2, 1000, copy=0), force="quad", ld=dict(ldvs_abs=lim))
    add("quad_ldvs_over_copy", "cross", 2, 1000, quad(2, 1000, copy=1), force="quad", ld=dict(ldvs_abs=lim + 1))

    # ---- lane: every RP resident and streaming (forced where mfma would take it) ----
    for rp in RPS:
        r = rp if rp % 8 else rp - 3
        r = max(r, rp - 7 if rp > 8 else 5)
        force = "lane" if rp in MFMA_RPS and rp >= 64 else None
        res_cap = 256 * PER_CU[("lane-resident", rp)] * C
        pad = dict(ldm=1, ldv=2, ldg=1) if rp % 16 else {}
        add(f"lane_rp{rp}_res_limit", "sweeps", r, res_cap, lane(r, res_cap), force=force, ld=pad, budget=3)
        add(f"lane_rp{rp}_stream", "sweeps", r, res_cap + 1, lane(r, res_cap + 1, res=False), force=force, ld=pad, budget=3)
    # pick_rp and gs boundaries (48 / 49, 52 / 53, 100 / 101; RP 32 / 40 for gs)
    add("lane_r32_no_gs", "sweeps", 32, 40000, lane(32, 40000), budget=3)
    add("lane_r33_gs", "sweeps", 33, 40000, lane(33, 40000), budget=3)
    add("lane_r48", "sweeps", 48, 40000, lane(48, 40000), budget=3)
    add("lane_r49", "sweeps", 49, 40000, lane(49, 40000), budget=3)
    add("lane_r52_gs", "sweeps", 52, 40000, lane(52, 40000), budget=3)
    add("lane_r53_no_gs", "sweeps", 53, 40000, lane(53, 40000), budget=3)
    add("lane_r101", "sweeps", 101, 40000, lane(101, 40000), budget=3)
    # features: resident lane reads V_in itself, streaming copies; Hadamard launch; sparsity; zero diagonal; ncols; snapshots
    add("lane_res_cross_gram2", "cross", 20, 40000, lane(20, 40000, hadamard=1, copy=0), gram2=True, ld=dict(ldvs=3, ldv=1, ldg=2))
    ns = 256 * PER_CU[("lane-resident", 24)] * C + 1            # RP 24: one column more than stays resident
    add("lane_stream_cross_gram2", "cross", 20, ns, lane(20, ns, res=False, hadamard=1, copy=1), gram2=True, ld=dict(ldvs=3))
    add("lane_res_sp_zero_diag", "solve", 45, 40000, lane(45, 40000), flags="sp", zero_diag=(0, 44))
    add("lane_stream_sp_zero_diag", "sweeps", 30, 200000, lane(30, 200000, res=False), flags="sp", zero_diag=(29,), budget=3)
    for n in (1, 255, 257):
        add(f"lane_n{n}", "sweeps", 57, n, lane(57, n), force="lane", ld=dict(ldv=1))
    add("lane_snap", "snap", 24, 40000, lane(24, 40000), budget=4)
    add("lane_stream_snap_refused", "snap", 24, ns, dict(err=UNSUP), budget=3)
    add("lane_cont", "cont", 20, 40000, lane(20, 40000), budget=3)
    # the 32-bit buffer offsets of the lane (and mfma) kernel, whose loads and stores cover all RP padded rows of a column:
    # ((RP - 1) ld + n) 4 < 0x7fff0000.  The rest of these buffers holds NaN (sentinels in V): a padded row whose offset wrapped
    # back into the operand would read it.  At rank 2 (RP 8) the bound on the r real rows alone let such strides through.
    lim32 = (0x7fff0000 - 4 - 40000 * 4) // (4 * 7)
    add("lane_ldm_32bit_limit", "sweeps", 2, 40000, lane(2, 40000), ld=dict(ldm_abs=lim32), budget=3)
    add("lane_ldm_32bit_refused", "sweeps", 2, 40000, dict(err=UNSUP), ld=dict(ldm_abs=lim32 + 1), budget=3)
    add("lane_ldm_32bit_padded_rows_refused", "sweeps", 2, 40000, dict(err=UNSUP), ld=dict(ldm_abs=(0x7fff0000 - 4 - 40000 * 4) // 4),
        budget=3)
    add("lane_ldv_32bit_limit", "solve", 2, 40000, lane(2, 40000), ld=dict(ldv_abs=lim32), budget=3)
    add("lane_ldvs_32bit_limit", "cross", 2, 40000, lane(2, 40000, copy=0), ld=dict(ldvs_abs=lim32), budget=3)
    add("lane_ldvs_32bit_over_copy", "cross", 2, 40000, lane(2, 40000, copy=1), ld=dict(ldvs_abs=lim32 + 1), budget=3)

    # ---- mfma: every RP (forced below 64); the 32768-column switch and the per-CU cap at rank 64 ----
    for rp in MFMA_RPS:
        r = rp if rp in (50, 52, 100) else rp - 1
        force = "mfma" if rp < 64 else None
        add(f"mfma_rp{rp}", "sweeps", r, 40000, mfma(r, 40000), force=force, ld=dict(ldm=1, ldv=3, ldg=1) if rp % 16 else {}, budget=3)
    # 32768 columns, not one more: not mfma, and lane where quad does not hold them -- the first mfma rank whose quad instance
    # keeps fewer than 32768 columns resident (rank 64 at 256 CUs: CH 16 holds 7 x 16 columns per CU)
    rq = next(rp for rp in MFMA_RPS if rp >= 64 and 16 * PER_CU[("quad", rp // 4)] * C < 32768)
    add("mfma_r64_n32768_lane", "sweeps", rq, 32768, lane(rq, 32768), budget=3)
    add("mfma_r64_n32769", "sweeps", 64, 32769, mfma(64, 32769), budget=3)
    nm = 256 * PER_CU[("mfma", 64)] * C
    add("mfma_r64_cap", "sweeps", 64, nm, mfma(64, nm), budget=3)
    add("mfma_r64_cap_over_stream", "sweeps", 64, nm + 1, lane(64, nm + 1, res=False), budget=3)
    add("mfma_r100", "solve", 100, 40000, mfma(100, 40000))
    add("mfma_r101_lane", "solve", 101, 40000, lane(101, 40000))
    add("mfma_cross_gram2", "cross", 80, 40000, mfma(80, 40000, hadamard=1, copy=0), gram2=True, ld=dict(ldvs=2, ldg=1))
    add("mfma_sp_zero_diag", "solve", 50, 40000, mfma(50, 40000), force="mfma", flags="sp", zero_diag=(0, 49))
    add("mfma_snap", "snap", 96, 40000, mfma(96, 40000), budget=4)
    add("mfma_chunks", "chunks", 64, 40000, mfma(64, 40000), budget=5)
    add("mfma_cont", "cont", 96, 40000, mfma(96, 40000), budget=3)

    # ---- generic: LDS / LDS-big / GCOL x mode 0 / 1; the exchanging grid's cap at the C entry point ----
    add("generic_lds_norm_m0", "solve", 20, 1000, generic("generic-lds", 20, 1000, copy=0), flags="norm", ld=dict(ldm=1, ldv=2, ldg=1))
    add("generic_lds_nz_m1", "sweeps", 8, 700, generic("generic-lds", 8, 700), flags="nz", budget=3)
    add("generic_lds_cross", "cross", 20, 900, generic("generic-lds", 20, 900, copy=1, hadamard=1), flags="norm", gram2=True,
        ld=dict(ldvs=3))
    add("generic_lds_no_sweep", "cross", 20, 300, dict(layout="generic-lds", copy=1, prep=1, err=0), flags="norm", budget=0,
        ld=dict(ldvs=3))
    add("generic_big_m0", "solve", 200, 600, generic("generic-lds-big", 200, 600))
    add("generic_big_m1", "sweeps", 129, 500, generic("generic-lds-big", 129, 500), flags="sp", budget=3)
    ng = 32 * PER_CU[("generic-lds-big", 600)] * C              # rank 600: the most columns LDS-big keeps resident
    add("generic_big_r600_cap", "solve", 600, ng, generic("generic-lds-big", 600, ng), budget=2)
    add("generic_gcol_r600_over", "solve", 600, ng + 1, generic("generic-gcol", 600, ng + 1, key=0), budget=2)
    add("generic_big_r600_m1_no_cap", "sweeps", 600, ng + 1, generic("generic-lds-big", 600, ng + 1), budget=2)
    add("generic_gcol_m1", "sweeps", 1200, 300, generic("generic-gcol", 1200, 300, key=0), budget=2)
    add("generic_gcol_m0_zero_diag", "solve", 1200, 300, generic("generic-gcol", 1200, 300, key=0), budget=2, zero_diag=(7,))
    ncap = 128 * PER_CU[("generic-lds", 8)] * C
    add("generic_csolve_cap", "csolve", 8, ncap, generic("generic-lds", 8, ncap), flags="norm", budget=2)
    add("generic_csolve_cap_over_refused", "csolve", 8, ncap + 1, dict(layout="generic-lds", err=UNSUP), flags="norm", budget=2)
    ncap100 = 128 * PER_CU[("generic-lds", 100)] * C
    add("generic_csolve_r100_cap", "csolve", 100, ncap100, generic("generic-lds", 100, ncap100), flags="norm", budget=2)
    add("generic_csolve_r100_over_refused", "csolve", 100, ncap100 + 1, dict(layout="generic-lds", err=UNSUP), flags="norm",
        budget=2)
    return cases


CASE_NAMES = list(hals_cases(256))


def reached(cases):
    """The tags the table reaches, from its expectations."""
    seen = set()
    for name, c in cases.items():
        e = c.expect
        lay = e.get("layout")
        if e.get("err", 0) != 0:
            if c.force == "wave":
                seen.add(("refuse", "wave_forced"))
            elif c.entry == "snap":
                seen.add(("refuse", "snap_stream"))
            elif "ldm_abs" in c.ld:
                seen.add(("refuse", "32bit"))
            elif c.entry == "csolve":
                seen.add(("refuse", "generic_cap"))
            continue
        if c.budget == 0:
            seen.add(("no_sweep", lay))
            continue
        if lay == "wave":
            seen.add(("wave", (c.r + 7) & ~7, e["cpw"]))
        elif lay == "quad":
            seen.add(("quad", e["ch"]))
        elif lay.startswith("lane"):
            seen.add((lay, e["RP"]))
        elif lay == "mfma":
            seen.add(("mfma", e["RP"]))
        else:
            seen.add((lay, 1 if c.entry in ("sweeps", "snap") else 0))
        if "gs" in e:
            seen.add(("gs", e["gs"]))
        if c.entry == "cross":
            seen.add(("copy", lay, e.get("copy")))
            if c.gram2:
                seen.add(("hadamard", lay, e.get("hadamard")))
        if c.entry == "cross" and not c.gram2 and lay not in ("wave", "quad"):
            seen.add(("hadamard", lay, 0))
        if c.opts.get("zero_diag"):
            seen.add(("zero_diag", lay))
        if c.flags == "sp":
            seen.add(("sp", lay))
    return seen


REQUIRED = ({("wave", ru, cpw) for ru in range(8, 129, 8) for cpw in (1, 2)} | {("quad", ch) for ch in range(1, 33)}
            | {(lay, rp) for rp in RPS for lay in ("lane-resident", "lane-streaming")} | {("mfma", rp) for rp in MFMA_RPS}
            | {(g, m) for g in ("generic-lds", "generic-lds-big", "generic-gcol") for m in (0, 1)}
            | {("gs", 0), ("gs", 1)}
            | {("copy", "wave", 0), ("copy", "quad", 0), ("copy", "quad", 1), ("copy", "lane-resident", 0),
               ("copy", "lane-streaming", 1), ("copy", "mfma", 0), ("copy", "generic-lds", 1)}
            | {("hadamard", "wave", 0), ("hadamard", "quad", 0), ("hadamard", "lane-resident", 1), ("hadamard", "lane-streaming", 1),
               ("hadamard", "mfma", 1), ("hadamard", "generic-lds", 1)}
            | {("no_sweep", "wave"), ("no_sweep", "lane-resident"), ("no_sweep", "generic-lds")}
            | {("zero_diag", lay) for lay in ("wave", "quad", "lane-resident", "lane-streaming", "mfma", "generic-gcol")}
            | {("sp", lay) for lay in ("wave", "quad", "lane-resident", "lane-streaming", "mfma", "generic-lds-big")}
            | {("refuse", k) for k in ("wave_forced", "snap_stream", "32bit", "generic_cap")})


def test_hals_cases_reach_required():
    """The table as written (256 CUs) reaches every instance, layout, feature route and refusal REQUIRED names (no GPU)."""
    seen = reached(hals_cases(256))
    assert not (REQUIRED - seen), sorted(REQUIRED - seen, key=str)
    # the quad ldvs pair and a stride on every operand
    cases = hals_cases(256)
    assert cases["quad_ldvs_over_copy"].expect["copy"] == 1 and cases["quad_ldvs_limit"].expect["copy"] == 0
    for key in ("ldm", "ldv", "ldvs", "ldg"):
        assert any(key in c.ld for c in cases.values()), key


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def sharp_gram(r, rng):
    B = rng.uniform(-1.0, 1.0, (r, r))
    E = np.triu(B, 1)
    E = E + E.T
    rs = np.abs(E).sum(axis=1).max()
    if rs > 0:
        E *= 0.4 / rs
    s = rng.uniform(0.8, 1.25, r)
    return ((np.eye(r) + E) * s[:, None] * s[None, :]).astype(np.float32)


def case_data(case, seed):
    """fp32 numpy inputs of a case: UtM (r x n), UtU, UtU2 (or None), V0 (start values).  Wide cases are one block of columns
    tiled; `ncol_block` is the block the oracle solves."""
    rng = np.random.RandomState(seed)
    r, n = case.r, case.n
    G = sharp_gram(r, rng)
    G2 = None
    if case.gram2:
        G2 = rng.uniform(0.7, 1.3, (r, r)).astype(np.float32)
        G2 = ((G2 + G2.T) / 2).astype(np.float32)
        Gh = G.astype(np.float32) * G2                                 # the fp32 Hadamard product the kernels form
    else:
        Gh = G
    for k in case.opts.get("zero_diag", ()):
        G[k, k] = 0.0
        if G2 is not None:
            G2[k, k] = 0.0
        Gh[k, k] = 0.0
    nb = n if case.flags == "norm" else min(n, BLOCK)      # the row norms couple the columns: no tiling
    W = rng.standard_normal((r, nb))
    UtM = (Gh.astype(np.float64) @ W).astype(np.float32)
    V0 = rng.uniform(0.0, 1.0, (r, nb)).astype(np.float32)
    neg = rng.uniform(size=(r, nb)) < 0.03
    V0[neg] = -rng.uniform(0.0, 0.5, int(neg.sum())).astype(np.float32)
    for k in case.opts.get("zero_diag", ()):
        V0[k, : max(1, nb // 3)] = -0.25                               # a skipped row keeps even negative values
    return dict(UtM=UtM, G=G, G2=G2, Gh=Gh, V0=V0, nb=nb)


def oracle_run(d, budget, flags, ncols=None):
    """fp64 trajectory of hals_nnls_acc on the fp32 inputs of one block (first `ncols` columns): [V_0 .. V_budget], [nodelta]."""
    nb = d["nb"] if ncols is None else ncols
    UtM, G, V = (d["UtM"][:, :nb].astype(np.float64), d["Gh"].astype(np.float64), d["V0"][:, :nb].astype(np.float64))
    kw = dict(alpha=math.inf, delta=0.0)
    if flags == "sp":
        kw["sparsity_coefficient"] = SP
    kw["normalize"] = flags == "norm"
    kw["nonzero"] = flags == "nz"
    traj, log = [V], []
    for _ in range(budget):
        V, _, _, _ = orc.hals_nnls_acc(UtM, G, V, maxiter=1, sweep_log=log, **kw)
        traj.append(V)
    return traj, log


def error_bound(d, traj, flags, r):
    """Per-entry bound after every sweep (module docstring); rows with a zero diagonal: 0 (bit for bit)."""
    G = d["Gh"].astype(np.float64)
    diag = np.diag(G).copy()
    live = diag != 0
    Dinv = np.where(live, 1.0 / np.where(live, diag, 1.0), 0.0)
    A = np.abs(G) * Dinv[:, None]
    np.fill_diagonal(A, 0.0)
    Lr, Ur = np.tril(A, -1), np.triu(A, 1)
    Minv = np.linalg.inv(np.eye(r) - Lr)
    UtM = np.abs(d["UtM"][:, : traj[0].shape[1]].astype(np.float64))
    sp = SP if flags == "sp" else 0.0
    e = np.zeros_like(traj[0])
    out = []
    for s in range(1, len(traj)):
        vabs = np.maximum(np.abs(traj[s - 1]), np.abs(traj[s]))
        kappa = 2 * min(s, REFRESH)
        loc = kappa * (r + 3) * U32 * (np.abs(G) @ vabs + UtM + sp) * Dinv[:, None] + 2 * U32 * np.abs(traj[s])
        loc[~live] = 0.0
        e = Minv @ (Ur @ e + loc)
        out.append(e)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = np.array([0x7fc0beef], dtype=np.uint32).view(np.float32)[0]     # a NaN with a payload: padding of V


def _padded(torch, a, cols, pad, fill, n_abs=None):
    """Device fp32 view [:, :cols] of a buffer with `pad` extra columns holding `fill` (or a row stride n_abs)."""
    rows = a.shape[0]
    ld = n_abs if n_abs is not None else cols + pad
    if n_abs is not None:                     # (everything but the view holds `fill` too)
        buf = torch.full(((rows - 1) * ld + cols,), float(fill), device="cuda", dtype=torch.float32)
        v = buf.as_strided((rows, cols), (ld, 1))
    else:
        buf = torch.full((rows, ld), float(fill), device="cuda", dtype=torch.float32)
        v = buf[:, :cols]
    if isinstance(fill, np.floating) and np.isnan(fill):
        buf.view(torch.int32)[:] = int(np.array([fill], dtype=np.float32).view(np.int32)[0])
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    v._buf = buf
    return v


def device_inputs(case, d):
    import torch
    n = case.n
    reps = _cdiv(n, d["nb"])
    tile = lambda a: np.tile(a, (1, reps))[:, :n]   # noqa: E731
    ld = case.ld
    UtM = _padded(torch, tile(d["UtM"]), n, ld.get("ldm", 0), float("nan"), ld.get("ldm_abs"))
    G = _padded(torch, d["G"], case.r, ld.get("ldg", 0), float("nan"))
    G2 = _padded(torch, d["G2"], case.r, ld.get("ldg", 0), float("nan")) if d["G2"] is not None else None
    V0 = tile(d["V0"])
    if case.entry == "cross":
        Vin = _padded(torch, V0, n, ld.get("ldvs", 0), float("nan"), ld.get("ldvs_abs"))
        V = _padded(torch, np.full_like(V0, np.nan), n, ld.get("ldv", 0), SENTINEL)
    else:
        Vin = None
        V = _padded(torch, V0, n, ld.get("ldv", 0), SENTINEL, ld.get("ldv_abs"))
    return dict(UtM=UtM, G=G, G2=G2, Vin=Vin, V=V)


def run_call(eng, case, t, snaps=None, resid=None):
    """The case's call(s).  Returns (status or None, per-sweep sums or None)."""
    import torch
    from nn_fac_amd import _lib
    sp = SP if case.flags == "sp" else None
    norm, nz = case.flags == "norm", case.flags == "nz"
    e, b = case.entry, case.budget
    if e == "solve":
        return eng.hals_solve(t["UtM"], t["G"], t["V"], b, delta=0.0, sparsity=sp, normalize=norm, nonzero=nz), None
    if e == "cross":
        return eng.hals_solve_cross(t["UtM"], t["G"], t["G2"], t["Vin"], t["V"], b, delta=0.0, sparsity=sp, normalize=norm), None
    if e == "sweeps":
        return None, eng.hals_sweeps(t["UtM"], t["G"], t["V"], b, sparsity=sp, normalize=norm, nonzero=nz)
    if e == "snap":
        return None, eng.hals_sweeps(t["UtM"], t["G"], t["V"], b, sparsity=sp, snapshots=snaps, snap_first=1)
    if e == "chunks":
        nf = eng.hals_resid_floats(case.r, case.n)
        ra = torch.empty(nf, device="cuda")
        n1 = eng.hals_sweeps(t["UtM"], t["G"], t["V"], 2, sparsity=sp, resid_out=ra)
        n2 = eng.hals_sweeps(t["UtM"], t["G"], t["V"], b - 2, sparsity=sp, sweeps_done=2, resid_in=ra)
        return None, torch.cat([n1, n2])
    if e == "cont":
        st = eng.hals_solve(t["UtM"], t["G"], t["V"], 2, delta=0.0, sparsity=sp)
        V = t["V"]
        _lib.check(eng.lib.nnf_hals_solve_continue_f32(eng.ctx, t["UtM"].data_ptr(), t["UtM"].stride(0),
                                                       t["G"].data_ptr(), t["G"].stride(0), V.data_ptr(), V.stride(0), case.r,
                                                       case.n, 2, b - 2, 0.0, float(sp or 0.0), 1 if sp else 0, st.data_ptr(),
                                                       eng._stream()), "nnf_hals_solve_continue_f32")
        return st, None
    if e == "csolve":
        V = t["V"]
        st = torch.empty(8, dtype=torch.float64, device="cuda")
        _lib.check(eng.lib.nnf_hals_solve_f32(eng.ctx, t["UtM"].data_ptr(), t["UtM"].stride(0), t["G"].data_ptr(), t["G"].stride(0),
                                              V.data_ptr(), V.stride(0), case.r, case.n, b, 0.0, 0.0, 2, st.data_ptr(),
                                              eng._stream()), "nnf_hals_solve_f32")
        return st, None
    raise AssertionError(e)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- the plan table, as the library reports it ----
_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_hals_plans as P
from nn_fac_amd.engine import get_engine, EngineError
eng = get_engine("cuda:0")
cases = P.hals_cases(P._cus())
for name, case in cases.items():
    sys.stderr.write("[case] %s\n" % name)
    sys.stderr.flush()
    if case.force:
        os.environ["NNF_HALS_FORCE"] = case.force
    else:
        os.environ.pop("NNF_HALS_FORCE", None)
    d = P.case_data(case, 1)
    t = P.device_inputs(case, d)
    snaps = torch.empty(max(case.budget - 1, 1), case.r, case.n, device="cuda") if case.entry == "snap" else None
    try:
        P.run_call(eng, case, t, snaps=snaps)
    except EngineError as e:
        sys.stderr.write("[refused] %s\n" % e)
    torch.cuda.synchronize()
    del t, snaps
    torch.cuda.empty_cache()
print("done")
"""


def parse_report(line):
    """{key: value} of one "[nnf hals] ..." report line (values as strings; "layout": the name after the arrow)."""
    head, tail = line[11:].split(" -> ")
    f = tail.split()
    kv = dict(kv.split("=", 1) for kv in head.split() + f[1:])
    kv["layout"] = f[0]
    return kv


def parse_plans(stderr):
    """{case name: [{key: value}]} (one dict per report line) from the child's stderr."""
    plans, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("[case] "):
            cur = line[7:].strip()
            plans[cur] = []
        elif line.startswith("[nnf hals] ") and cur is not None:
            plans[cur].append(parse_report(line))
    return plans


# ---- the same table without a device: the library's plan header through tools/nnf_plan.cpp ----
FLAG_BITS = {"": 0, "sp": 1, "norm": 2, "nz": 4}      # NNF_HALS_SPARSITY, NNF_HALS_NORMALIZE, NNF_HALS_NONZERO


def hals_line(C, case, wave_pc=None):
    """The `hals` line of tools/nnf_plan.cpp for the call of run_call() that writes the case's LAST report line, with every
    per-CU figure PER_CU pins for the kernel instances of its shape (the tool fails when the plan asks for one that is not
    there).  wave_pc: the figure of a wave instance with 3 .. 11 compute waves, which PER_CU does not pin; default: the
    pinned figure of 12 compute waves -- more waves per workgroup cannot raise it, so the case has to hold with it."""
    e, r, n, b, ld = case.entry, case.r, case.n, case.budget, case.ld
    mode = 1 if e in ("sweeps", "snap", "chunks") else 0
    nsweeps, sweep0 = (b - 2, 2) if e in ("cont", "chunks") else (b, 0)       # the second call of the two
    flags = 2 if e == "csolve" else FLAG_BITS[case.flags]
    kv = dict(mode=mode, r=r, ncols=n, nsweeps=nsweeps, sweep0=sweep0, flags=flags,
              ldm=ld.get("ldm_abs", n + ld.get("ldm", 0)), ldv=ld.get("ldv_abs", n + ld.get("ldv", 0)))
    if e == "cross":
        kv.update(own_start=1, gram2=int(case.gram2), ldvs=ld.get("ldvs_abs", n + ld.get("ldvs", 0)))
    if e == "snap":
        kv["snapshots"] = 1
    if case.force:
        kv["force"] = case.force[0]
    rp = pick_rp(r)
    if r <= 128:
        ru, nw = (r + 7) & ~7, wave_nw(n)
        kv["pc_wave1"] = PER_CU.get(("wave", ru, 1, nw), wave_pc or PER_CU[("wave", ru, 1, 12)])
        if ("wave", ru, 2, nw) in PER_CU:
            kv["pc_wave2"] = PER_CU[("wave", ru, 2, nw)]
        kv["pc_quad"] = PER_CU[("quad", (r + 3) // 4)]
        kv["pc_lane_res"], kv["pc_lane_stream"] = PER_CU[("lane-resident", rp)], PER_CU[("lane-streaming", rp)]
    else:
        kv["pc_generic_gcol"] = PER_CU[("generic-gcol", 0)]
    for key, form in (("pc_mfma", "mfma"), ("pc_generic_lds", "generic-lds"), ("pc_generic_big", "generic-lds-big")):
        if (form, rp if form == "mfma" else r) in PER_CU:
            kv[key] = PER_CU[(form, rp if form == "mfma" else r)]
    return "hals %d " % C + " ".join("%s=%s" % item for item in kv.items())


def ask_plan_tool(lines):
    """The answer of tools/nnf_plan.cpp to each line (built by test_mu_plan_table.plan_tool)."""
    from test_mu_plan_table import plan_tool
    p = subprocess.run([plan_tool()], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    answers = p.stdout.splitlines()
    assert len(answers) == len(lines), p.stdout[-2000:]
    return answers


def hals_tool_plans(C, cases, wave_pc=None):
    """{case name: {key: value}}: the report line the library's plan header gives for each case on C compute units."""
    names = list(cases)
    answers = ask_plan_tool([hals_line(C, cases[nm], (wave_pc or {}).get(nm)) for nm in names])
    return {nm: parse_report(text) for nm, text in zip(names, answers)}


@pytest.fixture(scope="module")
def reported(built_lib):
    env = dict(os.environ, NNF_HALS_DEBUG="1")
    env.pop("NNF_HALS_FORCE", None)
    p = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    return parse_plans(p.stderr)


@pytest.mark.gpu
def test_hals_plan_table(reported):
    """Every case takes the plan it is listed with (its last report line), and the reported per-CU figures are PER_CU's.  The
    plan header, asked through tools/nnf_plan.cpp for the request hals_line() makes of the case, answers that same line field by
    field: the CPU table test (test_hals_plan_table.py) asks about the calls the library was really given."""
    cases = hals_cases(_cus())
    assert sorted(reported) == sorted(cases)
    bad = []
    for name, case in cases.items():
        if not reported[name]:
            bad.append((name, "no report line"))
            continue
        kv = reported[name][-1]
        if int(kv["r"]) != case.r or int(kv["ncols"]) != case.n:
            bad.append((name, "shape", kv["r"], kv["ncols"]))
        for key, want in case.expect.items():
            if kv.get(key) != str(want):
                bad.append((name, key, kv.get(key), want))
    assert not bad, "\n".join(map(str, bad))
    # (a wave instance PER_CU does not pin: the figure the library reported)
    wave_pc = {name: int(lines[-1]["per_cu"]) for name, lines in reported.items() if lines[-1]["layout"] == "wave"}
    for name, kv in hals_tool_plans(_cus(), cases, wave_pc).items():
        for key, got in reported[name][-1].items():
            if kv[key] != got:
                bad.append((name, "tool", key, kv[key], got))
    assert not bad, "\n".join(map(str, bad))


# ---- values ----
def _check_block(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    ok = np.isfinite(got) & (err <= bound)
    if not ok.all():
        k, j = np.unravel_index(int(np.argmin(ok)), ok.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} entries off, first at ({k}, {j}): got {got[k, j]!r} want {want[k, j]!r} "
                             f"bound {bound[k, j]:.3e}")
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hals_plan_values(name, built_lib, monkeypatch):
    """Each case against the fp64 oracle, entry by entry (module docstring), after a call on other data in the same plan."""
    import torch
    from nn_fac_amd.engine import EngineError, get_engine
    case = hals_cases(_cus())[name]
    if case.force:
        monkeypatch.setenv("NNF_HALS_FORCE", case.force)
    else:
        monkeypatch.delenv("NNF_HALS_FORCE", raising=False)
    eng = get_engine("cuda:0")
    r, n, b = case.r, case.n, case.budget
    nsnap = max(b - 1, 1)
    snaps = torch.empty(nsnap, r, n, device="cuda") if case.entry == "snap" else None
    if case.expect.get("err", 0) != 0:
        d = case_data(case, 5)
        t = device_inputs(case, d)
        keep = t["V"].clone()
        with pytest.raises(EngineError, match="status -3"):
            run_call(eng, case, t, snaps=snaps)
        torch.cuda.synchronize()
        assert torch.equal(t["V"].view(torch.int32), keep.view(torch.int32)), name      # refused before anything ran
        return
    # a call on other data in the same plan first: its workspace (Gram image, barrier words, slots, residual) stays behind
    other = case_data(case, 99)
    other["UtM"] = other["UtM"] * 3 + 1
    run_call(eng, case, device_inputs(case, other), snaps=snaps)
    d = case_data(case, 5)
    t = device_inputs(case, d)
    keep = {k: t[k]._buf.clone() for k in ("UtM", "G", "G2", "Vin") if t.get(k) is not None}
    if snaps is not None:
        snaps.fill_(float("nan"))
    st, nd = run_call(eng, case, t, snaps=snaps)
    torch.cuda.synchronize()
    for k, v in keep.items():                                   # inputs bit-identical, padding included
        assert torch.equal(t[k]._buf.view(torch.int32), v.view(torch.int32)), f"{name}: input {k} modified"
    Vb = t["V"]._buf
    sbits = int(np.array([SENTINEL]).view(np.int32)[0])
    if "ldv_abs" in case.ld:                                     # everything outside the r x n view keeps its sentinel bits
        assert int((Vb.view(torch.int32) == sbits).sum()) == Vb.numel() - r * n, f"{name}: V written outside its rows"
    elif Vb.shape[1] > n:                                        # the padding columns of V keep their sentinel bits
        pad = Vb[:, n:].contiguous().view(torch.int32).cpu().numpy()
        assert (pad == sbits).all(), f"{name}: padding of V written"
    got = t["V"].cpu().numpy()
    # the fp64 reference: one block; full columns per block, then the remainder's own sums
    nb = d["nb"]
    traj, log = oracle_run(d, b, case.flags)
    bounds = error_bound(d, traj, case.flags, r) if b > 0 else []
    reps, rem = divmod(n, nb)
    logs = [reps * x for x in log]
    if rem:
        _, lr = oracle_run(d, b, case.flags, ncols=rem)
        logs = [x + y for x, y in zip(logs, lr)]
    want = traj[-1]
    worst = 0.0
    if case.flags == "norm":                  # the row norms couple the columns: the suite's solve tolerance on the whole
        assert nb == n
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert rel < 2e-4, (name, rel)
    else:
        bnd = bounds[-1] if b > 0 else np.zeros_like(want)
        for j0 in range(0, n, nb):
            w = min(nb, n - j0)
            worst = max(worst, _check_block(got[:, j0:j0 + w], want[:, :w], bnd[:, :w], f"{name} cols {j0}.."))
    for k in case.opts.get("zero_diag", ()):
        assert np.array_equal(got[k], np.tile(d["V0"][k], reps + 1)[:n]), f"{name}: row {k} with a zero diagonal moved"
    if st is not None:
        s = st.cpu().numpy()
        assert s[3] == 0.0 and int(s[1]) == b + 1, (name, s[:4])
        if b == 0:
            assert s[0] == 1.0 and s[2] == 0.0, (name, s[:4])
        else:
            assert abs(s[0] - logs[-1]) <= 5e-3 * logs[-1] and abs(s[2] - logs[0]) <= 5e-3 * logs[0], (name, s[:4], logs[0], logs[-1])
    if nd is not None:
        ndv = nd.cpu().numpy()
        assert len(ndv) == b
        for s_ in range(b):
            if case.flags == "norm":
                assert abs(ndv[s_] - logs[s_]) <= 5e-3 * logs[s_], (name, s_, ndv[s_], logs[s_])
                continue
            eb = bounds[s_] + (bounds[s_ - 1] if s_ > 0 else 0.0)        # step error <= e_s + e_{s-1}
            e2 = math.sqrt(reps + 1) * float(np.linalg.norm(eb))
            assert abs(ndv[s_] - logs[s_]) <= 2 * math.sqrt(logs[s_]) * e2 + e2 * e2 + 1e-12 * logs[s_], (name, s_, ndv[s_], logs[s_])
    if snaps is not None:                     # block j: V after sweep j + 2 (snap_first = 1)
        sn = snaps.cpu().numpy()
        for j in range(b - 1):
            for j0 in range(0, n, nb):
                w = min(nb, n - j0)
                _check_block(sn[j][:, j0:j0 + w], traj[j + 2][:, :w], bounds[j + 1][:, :w], f"{name} snapshot {j}")
    print(f"{name}: worst err / bound {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------------------
# the stop rule
# ---------------------------------------------------------------------------------------------------------------------------
StopCase = collections.namedtuple("StopCase", "layout r n nb c budget flags apart seed delta")


def _nmf_like(r, nb, seed):
    rng = np.random.RandomState(seed)
    A = rng.rand(4 * r, r)
    G = (A.T @ A).astype(np.float32)
    UtM = (A.T @ (A @ rng.rand(r, nb) + 0.05 * rng.rand(4 * r, nb))).astype(np.float32)
    V0 = rng.rand(r, nb).astype(np.float32)
    return dict(UtM=UtM, G=G, Gh=G, G2=None, V0=V0, nb=nb)


def _place_delta(log, c, budget):
    """delta with the oracle stopping after sweep c (budget: None), or None where the margins are under 2 %."""
    if c == budget:
        return 0.0
    ratio = [x / log[0] for x in log]
    lo, hi = ratio[c - 1], ratio[c - 2]                          # stops after c: ratio_c < delta <= ratio_{c-1}, all before >= delta
    if not (hi >= lo * 1.02 ** 2) or min(ratio[:c - 1]) < hi:
        return None
    return math.sqrt(lo * hi)


def stop_cases():
    """(name, StopCase); the seed of each is the first whose oracle log allows the 2 % margins (chosen here, on the CPU)."""
    out = []
    spec = [("wave_cpw1", 20, 1000, 1000, None)] + [("wave_cpw2", 20, 3073, 3073, None)] \
        + [("quad", 20, 8000, 2000, None), ("mfma", 64, 40000, 2000, None), ("lane_res", 20, 40000, 2000, None),
           ("lane_stream", 20, 133120, 2048, None), ("generic_lds", 20, 1000, 1000, "nz"), ("generic_gcol", 1200, 256, 256, None)]
    for lay, r, n, nb, flags in spec:
        cs = [2, 7, 8, 9, 15, 16, 17, 18, 33, "budget"] if lay == "wave_cpw1" else [3, 17] if lay == "wave_cpw2" else \
            [2, 6] if lay == "generic_gcol" else [3, 9]
        for c in cs:
            budget = 40 if c != "budget" else 12
            cc = budget if c == "budget" else c
            out.append((f"{lay}_c{c}", lay, r, n, nb, cc, budget if c == "budget" else cc + 3, flags))
    return out


_SEEDS = {}


def _stop_case(name):
    for nm, lay, r, n, nb, c, budget, flags in stop_cases():
        if nm != name:
            continue
        if name not in _SEEDS:
            for seed in range(100, 140):
                d = _nmf_like(r, nb, seed)
                traj, log = oracle_run(d, c + 1, "" if flags is None else flags)
                delta = _place_delta(log, c, budget)
                if delta is None:
                    continue
                # V after sweep c must differ from V after c - 1 and c + 1 by more than 10x the tolerance
                vc = traj[c]
                apart = min(np.linalg.norm(traj[c - 1] - vc), np.linalg.norm(traj[c + 1] - vc)) >= 2e-3 * np.linalg.norm(vc)
                if name not in _SEEDS or (apart and not _SEEDS[name][4]):
                    _SEEDS[name] = (seed, delta, d, traj, apart)
                if apart:
                    break
        seed, delta, d, traj, apart = _SEEDS[name]
        return StopCase(lay, r, n, nb, c, budget, flags, apart, seed, delta), d, traj
    raise KeyError(name)


STOP_LAYOUT = {"wave_cpw1": "wave", "wave_cpw2": "wave", "quad": "quad", "mfma": "mfma", "lane_res": "lane-resident",
               "lane_stream": "lane-streaming", "generic_lds": "generic-lds", "generic_gcol": "generic-gcol"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in stop_cases()])
def test_hals_stop_rule(name, built_lib, monkeypatch, capfd):
    """delta placed so that the oracle stops after sweep c: same sweep count, V = the oracle's V after sweep c."""
    import torch
    from nn_fac_amd.engine import get_engine
    monkeypatch.delenv("NNF_HALS_FORCE", raising=False)
    monkeypatch.setenv("NNF_HALS_DEBUG", "1")
    sc, d, traj = _stop_case(name)
    eng = get_engine("cuda:0")
    reps = sc.n // sc.nb
    assert reps * sc.nb == sc.n
    UtM = torch.from_numpy(np.tile(d["UtM"], (1, reps))).cuda()
    V = torch.from_numpy(np.tile(d["V0"], (1, reps))).cuda()
    G = torch.from_numpy(d["G"]).cuda()
    capfd.readouterr()
    st = eng.hals_solve(UtM, G, V, sc.budget, delta=sc.delta, nonzero=sc.flags == "nz").cpu().numpy()
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith("[nnf hals]")]
    assert lines and f"-> {STOP_LAYOUT[sc.layout]} " in lines[-1], lines
    if sc.layout.startswith("wave"):
        assert f" cpw={sc.layout[-1]} " in lines[-1], lines[-1]
    assert st[3] == 0.0 and int(st[1]) == sc.c + 1, (name, st[:4], sc.c)
    got = V.cpu().numpy()
    vc = traj[sc.c]
    tol = 2e-4 * np.linalg.norm(vc)
    for j0 in range(0, sc.n, sc.nb):
        g = got[:, j0:j0 + sc.nb]
        e = np.linalg.norm(g - vc)
        assert e < tol, (name, j0, e / np.linalg.norm(vc))
        if sc.apart:              # (the oracle's V after sweeps c - 1 and c + 1 lie >= 10 tolerances away)
            assert e < 0.1 * np.linalg.norm(g - traj[sc.c - 1]) and e < 0.1 * np.linalg.norm(g - traj[sc.c + 1]), name

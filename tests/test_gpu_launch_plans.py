"""Every launch plan of the streaming (k_xty.hip, k_xht.hip, k_gram.hip, k_cost.hip, k_xht_lds.hip) and MU (k_mu.hip) launchers, against fp64.  Needs a MI355X.

The launchers pick a plan from m, n, r, the alignment of X, the CU count and the free workspace: the X H^T row tilings and
their k-split tail, the split counts of W^T X, of the right MU update and of the Gram, the row mixes of the left MU update,
the column splits and load widths of the cost pass.  PLAN_CASES names the plan every case must take, with its shape written
from the CU count so that each case sits exactly on the side of a threshold it says it does; test_plan_table checks that
against the library's own report (NNF_PLAN_DEBUG), and test_plan_values checks every case against a plain fp64 evaluation
on the device, entry by entry, with the output pre-filled with NaN and the workspace slabs left over from a call on other
data.

The MU rows run up to rank 128: the kernels of five to eight rank tiles have launch forms of their own (128-row workgroups only,
or a 192 / 128-row mix over rounds of at most 12 tiles; 128-column workgroups in the right update), and REQUIRED_BIG names what
the rows with mt >= 5 must reach without the help of the rows below.  `mu_accum` is the accumulate-only form of the right update
(nnf_mu_right_accum_f32): the same plans, the slabs reduced into num / den.  tests/test_mu_plan_table.py checks the X H^T, W^T X
and MU rows without a device, against the library's own plan arithmetic (csrc/k_stream_plan.h, k_mu_plan.h through
tools/nnf_plan.cpp) at 256 and 304 compute units.

One branch is not reachable and has no case: nnf_plan_xht refuses the tail when 8 * extra > T, but a tail of four or more
shares already needs extra <= 4 * (slots / parts) <= slots, and a one-round T is more than 8 * slots.
"""
import collections
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS_ERR = r"status -4 \(context workspace too small\)"       # NNF_ERR_WORKSPACE

Case = collections.namedtuple("Case", "kernel m n r ld ws beta expect")


def _cdiv(a, b):
    return -(-a // b)


def _splits(rows, nsplit):
    """The split count after the launchers round the rows per split up to 64: cdiv(rows, rup(cdiv(rows, nsplit), 64))."""
    return _cdiv(rows, 64 * _cdiv(_cdiv(rows, nsplit), 64))


def _halved(rows, ld):
    """Rows per split of a one-split plan after the halving that keeps (rows + 128) * ld * 4 inside 32-bit offsets."""
    rps = 64 * _cdiv(rows, 64)
    while (rps + 128) * ld * 4 >= 0x7fff0000:
        rps = 64 * _cdiv(rps // 2, 64)
    return rps


def _m_of(T, ragged=5):
    """A row count with cdiv(m, 16) == T and a ragged last tile."""
    return 16 * T - ragged


def mu_right_prologue(r, m, beta):
    """Workspace bytes launch_mu_right takes before its slabs: r doubles, for beta = 1 the r x np partials of the row sums of
    Ut when m has np = min(m / 8192, 64) > 1 pieces, every block on the cursor's 256-byte alignment."""
    off = r * 8
    pieces = min(m // 8192, 64)
    if beta == 1.0 and pieces > 1:
        off = 256 * _cdiv(off, 256) + r * pieces * 8
    return 256 * _cdiv(off, 256)


def plan_cases(C):
    """{name: Case} for a device with C compute units.  `ld` is the row stride of X (None: n), `ws` the context workspace
    in bytes (None: the process engine's), `expect` the fields the library must report for the case's launch."""
    cases = {}

    def add(name, kernel, m, n, r, expect, ld=None, ws=None, beta=None):
        assert name not in cases
        cases[name] = Case(kernel, m, n, r, ld, ws, beta, expect)

    # ---- X H^T (launch_xht; ranks <= 32 with aligned X: launch_xht_lds) ----
    # slots = resident workgroups: 2 per CU up to four rank tiles (MT + (REM > 0) <= 4), 1 above; waves = 4 slots, T = row tiles.
    s4, s8 = 2 * C, C
    w4, w8 = 4 * s4, 4 * s8

    def tail(parts, tiles, cpp):
        return dict(tail_parts=parts, tail_tiles=tiles, tail_cpp=cpp)

    no_tail = tail(0, 0, 0)
    # rank 50 = three MFMA tiles + two VALU ranks (four tiles' worth, s4).  n = 200: 4 column chunks, 188: 3, 260: 5, 2100: 33.
    add("xht_small_edge", "xht", _m_of(2 * w4), 200, 50, dict(form="small", mt=3, rem=2, **no_tail))
    add("xht_round32_extra1", "xht", _m_of(2 * w4 + 1), 200, 50, dict(form="round32", nth=3, n_hi=0, **tail(4, 1, 1)))
    add("xht_round32_3chunks", "xht", _m_of(2 * w4 + 1), 188, 50, dict(form="round32", nth=3, n_hi=1, **no_tail))
    add("xht_round32_5chunks", "xht", _m_of(2 * w4 + 5), 260, 50, dict(form="round32", **tail(4, 5, 2)))     # share 3 empty
    add("xht_round32_parts8", "xht", _m_of(2 * w4 + 4 * (s4 // 16) + 1), 2100, 50, dict(form="round32", **tail(8, 4 * (s4 // 16) + 1, 5)))
    add("xht_round32_parts4_limit", "xht", _m_of(2 * w4 + s4), 2100, 50, dict(form="round32", **tail(4, s4, 9)))
    add("xht_round32_parts4_over", "xht", _m_of(2 * w4 + s4 + 1), 2100, 50,
        dict(form="round32", nth=3, n_hi=_cdiv(s4 + 1, 4), **no_tail))
    add("xht_round32_edge_hi", "xht", _m_of(3 * w4), 200, 50, dict(form="round32", nth=3, n_hi=s4, **no_tail))
    add("xht_round43_extra1", "xht", _m_of(3 * w4 + 1), 200, 50, dict(form="round43", nth=4, n_hi=0, **tail(4, 1, 1)))
    add("xht_round43_parts32", "xht", _m_of(3 * w4 + 4 * (s4 // 32)), 2100, 50,
        dict(form="round43", **tail(32, 4 * (s4 // 32), 2)))                     # 17 shares hold the 33 chunks, 15 are empty
    add("xht_round43_parts16", "xht", _m_of(3 * w4 + 4 * (s4 // 32) + 1), 2100, 50,
        dict(form="round43", **tail(16, 4 * (s4 // 32) + 1, 3)))
    add("xht_round43_edge_hi", "xht", _m_of(4 * w4), 200, 50, dict(form="round43", nth=4, n_hi=s4, **no_tail))
    add("xht_rounds_edge", "xht", _m_of(4 * w4 + 1), 200, 50, dict(form="rounds", nth=4, grid=_cdiv(_m_of(4 * w4 + 1), 256),
                                                                     **no_tail))
    # the tail's rank condition: two tiles (unaligned rank 32: MT 2, no leftover ranks) against three (rank 33: 2 + VALU)
    add("xht_rank32_unaligned_no_tail", "xht", _m_of(2 * w4 + 1), 200, 32, dict(form="round32", mt=2, rem=0, vec=0, **no_tail),
        ld=201)
    add("xht_rank33_tail", "xht", _m_of(2 * w4 + 1), 200, 33, dict(form="round32", mt=2, rem=2, vec=1, **tail(4, 1, 1)))
    add("xht_rank33_unaligned_tail", "xht", _m_of(2 * w4 + 3), 200, 33, dict(form="round32", mt=3, rem=0, vec=0, **tail(4, 3, 1)),
        ld=203)
    # ranks 51, 52: three tiles + four leftover ranks are padded to four tiles
    add("xht_rank51_padded", "xht", _m_of(3 * w4 + 1), 200, 51, dict(form="round43", mt=4, rem=0, **tail(4, 1, 1)))
    add("xht_rank52_padded", "xht", _m_of(2 * w4 + 2), 200, 52, dict(form="round32", mt=4, rem=0, **tail(4, 2, 1)))
    # the tail's slabs do not fit the workspace: the (nth, nth - 1) mix instead (32 shares x 50 x 1024 rows > 1 MiB)
    add("xht_tail_no_workspace", "xht", _m_of(3 * w4 + 4 * (s4 // 32)), 2100, 50,
        dict(form="round43", nth=4, n_hi=_cdiv(4 * (s4 // 32), 4), **no_tail), ws=1 << 20)
    # one resident workgroup per CU (rank 100 = 6 tiles + 4 VALU ranks): one round with a tail, and the two-tile form
    add("xht_rank100_round43_tail", "xht", _m_of(3 * w8 + 10), 2100, 100, dict(form="round43", mt=6, rem=4, **tail(32, 10, 2)))
    add("xht_rank100_round32", "xht", _m_of(2 * w8 + 1), 200, 100, dict(form="round32", **tail(4, 1, 1)))
    add("xht_two_tiles_edge_lo", "xht", _m_of(14 * w8), 200, 96, dict(form="rounds", mt=6, rem=0, **no_tail))
    add("xht_two_tiles", "xht", _m_of(14 * w8 + 1), 200, 96, dict(form="two_tiles", nth=2, grid=_cdiv(_m_of(14 * w8 + 1), 128),
                                                                   **no_tail))
    add("xht_two_tiles_rank81", "xht", _m_of(14 * w8 + 3), 136, 81, dict(form="two_tiles", mt=5, rem=2, **no_tail))
    add("xht_rank80_five_tiles", "xht", _m_of(14 * w8 + 1), 200, 80, dict(form="rounds", mt=5, rem=0, **no_tail))
    add("xht_unaligned_rounds", "xht", _m_of(4 * w4 + 1), 200, 50, dict(form="rounds", mt=4, rem=0, vec=0, **no_tail), ld=201)
    # ranks <= 32, aligned X: X staged through LDS
    add("xht_lds_rounds", "xht", _m_of(4 * w4 + 1), 256, 32, dict(form="lds", tiling="rounds", mt=2, rem=0))
    add("xht_lds_round43", "xht", _m_of(3 * w4 + 1), 208, 20, dict(form="lds", tiling="round43", mt=1, rem=4))
    add("xht_lds_shared_lines", "xht", _m_of(2 * w4 + 1), 200, 18, dict(form="lds", tiling="shared_lines", mt=1, rem=2))

    # ---- W^T X (launch_xty): nsplit = resident workgroups / column blocks, raised to m / 2048, cut to m / 64, the workspace,
    # then rows per split halved until a split's rows stay inside 32-bit offsets.  Rank 50: 3 workgroups per CU, rank 100: 1.
    t50 = 3 * C // _cdiv(2000, 256)
    add("xty_occupancy", "xty", 1024 * t50 + 7, 2000, 50, dict(bound="occupancy", nsplit=_splits(1024 * t50 + 7, t50)))
    add("xty_min_rows", "xty", 3000, 2000, 50, dict(bound="min_rows"))
    t100 = C // _cdiv(2000, 256)
    m_cap = 2048 * (t100 + 1) + 100
    add("xty_rows_cap", "xty", m_cap, 2000, 100, dict(bound="rows_cap", nsplit=_cdiv(m_cap, 2048)))
    slab100 = 100 * 2000 * 4
    add("xty_workspace", "xty", m_cap, 2000, 100, dict(bound="workspace", nsplit=_splits(m_cap, (t100 + 1) // 2)),
        ws=slab100 * ((t100 + 1) // 2) + 4096)
    n_wide = max(250000, 256 * (3 * C + 1))      # more column blocks than resident workgroups: one split, then halved
    add("xty_offset32", "xty", 2000, n_wide, 50, dict(bound="offset32", nsplit=_cdiv(2000, _halved(2000, n_wide)),
                                                     rows_per_split=_halved(2000, n_wide)))
    add("xty_unaligned", "xty", 1024 * t50 + 7, 2000, 50, dict(bound="occupancy", mt=4, rem=0, vec=0), ld=2001)

    # ---- the right MU update (launch_mu_right): KL 2 workgroups per CU, general beta 1; no rows cap ----
    add("mu_right_kl_occupancy", "mu_right", 20000, 2000, 50, dict(bm="KL", bound="occupancy", nsplit=_splits(20000, 2 * C // 8)), beta=1.0)
    add("mu_right_gen_occupancy", "mu_right", 20000, 2000, 34, dict(bm="GEN", bound="occupancy", nsplit=_splits(20000, C // 8)), beta=0.5)
    add("mu_right_min_rows", "mu_right", 1000, 2000, 50, dict(bm="KL", bound="min_rows", nsplit=_cdiv(1000, 64)), beta=1.0)
    # (the KL form first takes r doubles and the rowsum's r x 2 partials: 1536 bytes with the alignment)
    add("mu_right_workspace", "mu_right", 20000, 2000, 50, dict(bm="KL", bound="workspace", nsplit=_splits(20000, 10)), beta=1.0,
        ws=10 * 50 * 2000 * 4 + 1536)
    n_one = max(70000, 256 * C + 4464)      # more column blocks than CUs: one split in both forms (KL: 2 C / ncb = 1)
    add("mu_right_one_split", "mu_right", 3000, n_one, 50, dict(bm="KL", bound="occupancy", nsplit=1), beta=1.0)
    rps = _halved(8000, n_one)
    add("mu_right_offset32_kl", "mu_right", 8000, n_one, 50, dict(bm="KL", bound="offset32", nsplit=_cdiv(8000, rps), rps=rps), beta=1.0)
    add("mu_right_offset32_gen", "mu_right", 8000, n_one, 20, dict(bm="GEN", bound="offset32", nsplit=_cdiv(8000, rps), rps=rps), beta=1.5)

    # ---- the left MU update (launch_mu_left): T row tiles over slots = 2 workgroups per CU (KL, KLC) or 1 (general beta):
    # T <= 8 slots: 128-row workgroups; else W = whole rounds, T > 12 W: 256-row (n_hi) + 192-row; else 192 + 128-row ----
    for r, mt, rem in [(16, 1, 0), (18, 1, 2), (20, 1, 4), (32, 2, 0), (34, 2, 2), (48, 3, 0), (50, 3, 2), (64, 4, 0)]:
        s = 2 * C
        for form, T in [("small", 8 * s), ("mid", 8 * s + 1), ("hi", 12 * s + 1)]:
            add(f"mu_left_r{r}_{form}", "mu_left", _m_of(T), 72, r, dict(bm="KL", form=form, mt=mt, rem=rem, vec=1), beta=1.0)
    add("mu_left_hi_full_round", "mu_left", _m_of(16 * 2 * C), 72, 50, dict(bm="KL", form="hi", grid=2 * C), beta=1.0)
    add("mu_left_two_rounds", "mu_left", _m_of(16 * 2 * C + 1), 72, 50, dict(bm="KL", form="mid", grid=4 * C, n_hi=0), beta=1.0)
    for form, T in [("small", 8 * 2 * C), ("mid", 8 * 2 * C + 1), ("hi", 12 * 2 * C + 1)]:
        add(f"mu_left_unaligned_{form}", "mu_left", _m_of(T), 70, 50, dict(bm="KL", form=form, mt=4, rem=0, vec=0), beta=1.0, ld=71)
    for form, T in [("small", 8 * C), ("mid", 8 * C + 1), ("hi", 12 * C + 1)]:
        add(f"mu_left_gen_{form}", "mu_left", _m_of(T), 72, 50, dict(bm="GEN", form=form, mt=4, rem=0), beta=0.5)
    add("mu_left_frob_cp3", "cp3_partial_cost", 300 * 40, 70, 20, dict(bm="FROB"))

    # ---- ranks 65 .. 128 (MT = 5 .. 8 rank tiles), left update.  KL at MT >= 6: one workgroup per CU, no 256-row workgroups;
    # T <= 8 slots: 128-row workgroups; else W3 = whole rounds of at most 12 tiles: T <= 8 W3: 128-row workgroups again
    # (rows128), else W3 workgroups of which cdiv(T - 8 W3, 4) take 192 rows.  Ranks 97 .. 100 on aligned X: six tiles + four
    # leftover ranks ----
    def left(name, T, n, r, form, mt, rem, vec, beta, grid=None, n_mid=0, ld=None):
        m = _m_of(T)
        add(name, "mu_left", m, n, r, dict(bm="KL" if beta == 1.0 else "GEN", form=form, mt=mt, rem=rem, vec=vec,
                                           grid=_cdiv(m, 128) if grid is None else grid, n_hi=0, n_mid=n_mid), beta=beta, ld=ld)

    s = C

    def left_edges(tag, r, mt, rem, vec, full):
        n, ld = (72, None) if vec else (70, 71)
        if full:
            left(f"mu_left_{tag}_small", 8 * s, n, r, "small", mt, rem, vec, 1.0, ld=ld)
        left(f"mu_left_{tag}_mid_one", 8 * s + 1, n, r, "mid", mt, rem, vec, 1.0, grid=s, n_mid=1, ld=ld)
        if full:
            left(f"mu_left_{tag}_mid_one_full", 8 * s + 4, n, r, "mid", mt, rem, vec, 1.0, grid=s, n_mid=1, ld=ld)   # no spare tile
        left(f"mu_left_{tag}_mid_all", 12 * s, n, r, "mid", mt, rem, vec, 1.0, grid=s, n_mid=s, ld=ld)   # no 128-row workgroup
        left(f"mu_left_{tag}_rows128_lo", 12 * s + 1, n, r, "rows128", mt, rem, vec, 1.0, ld=ld)
        left(f"mu_left_{tag}_rows128_hi", 16 * s, n, r, "rows128", mt, rem, vec, 1.0, ld=ld)
        left(f"mu_left_{tag}_two_rounds", 16 * s + 1, n, r, "mid", mt, rem, vec, 1.0, grid=2 * s, n_mid=1, ld=ld)
        if full:
            left(f"mu_left_{tag}_three_rounds", 24 * s + 1, n, r, "mid", mt, rem, vec, 1.0, grid=3 * s, n_mid=1, ld=ld)

    for r, mt, rem in [(96, 6, 0), (100, 6, 4), (112, 7, 0), (128, 8, 0)]:
        left_edges(f"r{r}", r, mt, rem, 1, True)
    left_edges("r100_unaligned", 100, 7, 0, 0, False)
    left_edges("r128_unaligned", 128, 8, 0, 0, False)
    # the six-tiles-and-four form holds for ranks 97 .. 100 only (rank 96 above: mt=6 rem=0)
    left("mu_left_r97_mid_one", 8 * s + 1, 72, 97, "mid", 6, 4, 1, 1.0, grid=s, n_mid=1)
    left("mu_left_r101_mid_one", 8 * s + 1, 72, 101, "mid", 7, 0, 1, 1.0, grid=s, n_mid=1)
    left("mu_left_r101_rows128_lo", 12 * s + 1, 72, 101, "rows128", 7, 0, 1, 1.0)
    # KL at MT = 5: two workgroups per CU, 128 rows each whatever the height
    for r in (65, 80):
        left(f"mu_left_r{r}_small", 8 * 2 * C, 72, r, "small", 5, 0, 1, 1.0)
        left(f"mu_left_r{r}_rows128", 8 * 2 * C + 1, 72, r, "rows128", 5, 0, 1, 1.0)
    # general beta: one workgroup per CU, 128 rows each
    for r, mt in [(65, 5), (128, 8)]:
        left(f"mu_left_r{r}_gen_small", 8 * C, 72, r, "small", mt, 0, 1, 0.5)
        left(f"mu_left_r{r}_gen_rows128", 8 * C + 1, 72, r, "rows128", mt, 0, 1, 0.5)
    left("mu_left_r128_gen_unaligned", 8 * C + 1, 70, 128, "rows128", 8, 0, 0, 0.5, ld=71)

    # ---- ranks 65 .. 128, right update and its accumulate-only form: 128 columns per workgroup, one workgroup per CU in both
    # beta forms: nsplit = C / cdiv(n, 128) ----
    def right(name, m, n, r, beta, bound, nsplit, rps=None, kernel="mu_right", vec=1, rem=0, **kw):
        rps = 64 * _cdiv(_cdiv(m, nsplit), 64) if rps is None else rps
        add(name, kernel, m, n, r, dict(bm="KL" if beta == 1.0 else "GEN", bound=bound, nsplit=_cdiv(m, rps), rps=rps,
                                        mt=(r + (0 if rem else 15)) // 16, rem=rem, vec=vec), beta=beta, **kw)

    n_big = 128 * C + 200                   # more 128-column blocks than CUs: one split
    # the fewest rows (in 64s) with (rows + 128) rows of X outside 32-bit offsets: halved once; 64 fewer: one split as it is
    rows_off = 64 * _cdiv(_cdiv(0x7fff0000, 4 * n_big) - 128, 64)
    m_off = rows_off - 37
    assert _halved(m_off, n_big) == 64 * _cdiv(rows_off // 2, 64) and _halved(m_off - 64, n_big) == rows_off - 64
    for r in (65, 128):
        for beta in (1.0, 0.5 if r == 65 else 1.5):
            tag = f"mu_right_r{r}_{'kl' if beta == 1.0 else 'gen'}"
            nacc = 1 if beta == 1.0 else 2
            right(f"{tag}_occupancy", 20000, 2000, r, beta, "occupancy", C // 16)
            right(f"{tag}_min_rows", 1000, 1000, r, beta, "min_rows", _cdiv(1000, 64))            # C / 8 > 16 splits of 64 rows
            # room for ten slabs (general beta: ten pairs, the second set behind the cursor's 256-byte alignment)
            slabs = 10 * r * 2000 * 4
            right(f"{tag}_workspace", 20000, 2000, r, beta, "workspace", 10,
                  ws=mu_right_prologue(r, 20000, beta) + (nacc - 1) * 256 * _cdiv(slabs, 256) + slabs)
            right(f"{tag}_one_split", 3000, n_big, r, beta, "occupancy", 1)
            right(f"{tag}_offset32", m_off, n_big, r, beta, "offset32", None, rps=_halved(m_off, n_big))
    right("mu_right_r128_kl_one_split_last", m_off - 64, n_big, 128, 1.0, "occupancy", 1)
    # as many 64-row chunks as splits: still the occupancy bound
    right("mu_right_r128_kl_occupancy_edge", 64 * (C // 16) - 10, 2000, 128, 1.0, "occupancy", C // 16, rps=64)
    # four bytes short of ten slabs behind the row sums' partials: nine
    right("mu_right_r128_kl_workspace_short", 20000, 2000, 128, 1.0, "workspace", 9,
          ws=mu_right_prologue(128, 20000, 1.0) + 10 * 128 * 2000 * 4 - 4)
    # ten pairs of rank-65 slabs to the byte: the second set starts 128 bytes further, nine pairs fit
    assert (10 * 65 * 2000 * 4) % 256 == 128
    right("mu_right_r65_gen_workspace_tight", 20000, 2000, 65, 0.5, "workspace", 9, ws=mu_right_prologue(65, 20000, 0.5) + 2 * 10 * 65 * 2000 * 4)
    right("mu_right_r96_kl_occupancy", 20000, 2000, 96, 1.0, "occupancy", C // 16)            # six and seven rank tiles
    right("mu_right_r112_gen_occupancy", 20000, 2000, 112, 0.5, "occupancy", C // 16)
    right("mu_right_r128_kl_unaligned", 20000, 2000, 128, 1.0, "occupancy", C // 16, vec=0, ld=2001)
    right("mu_right_r65_gen_unaligned", 20000, 2000, 65, 0.5, "occupancy", C // 16, vec=0, ld=2001)
    # nnf_mu_right_accum_f32: the same plans, the slabs reduced into num / den instead of the finished update
    right("mu_accum_r50_kl", 20000, 2000, 50, 1.0, "occupancy", 2 * C // 8, kernel="mu_accum", rem=2)
    right("mu_accum_r50_gen", 20000, 2000, 50, 0.5, "occupancy", C // 8, kernel="mu_accum")
    right("mu_accum_r100_kl", 20000, 2000, 100, 1.0, "occupancy", C // 16, kernel="mu_accum")
    right("mu_accum_r100_gen", 20000, 2000, 100, 1.5, "occupancy", C // 16, kernel="mu_accum")
    right("mu_accum_r100_gen_workspace", 20000, 2000, 100, 0.5, "workspace", 10, kernel="mu_accum",
          ws=mu_right_prologue(100, 20000, 0.5) + 2 * 10 * 100 * 2000 * 4)

    # ---- Gram (launch_gram, launch_gram_blocks) ----
    add("gram_small", "gram", 1000, None, 50, dict(form="small"))
    add("gram_single_rank100", "gram", 1000, None, 100, dict(form="single", bound="short"))
    add("gram_single_ragged", "gram", 1001, None, 50, dict(form="single", bound="short"))
    add("gram_slabs_min_cols", "gram", 5000, None, 50, dict(form="slabs", bound="min_cols", nsplit=_cdiv(5000, 64)))
    add("gram_slabs_occupancy", "gram", 100000, None, 50, dict(form="slabs", bound="occupancy"))
    K512 = 512 * (2 * C + 1) + 100
    add("gram_slabs_chain512", "gram", K512, None, 50, dict(form="slabs", bound="chain512", nsplit=_cdiv(K512, 512)))
    add("gram_slabs_workspace", "gram", K512, None, 128, dict(form="slabs", bound="workspace", nsplit=_splits(K512, 128)),
        ws=128 * 128 * 128 * 4 + 4096)
    add("gram_blocks", "gram", 30000, None, 200, dict(form="blocks", bound="chain512", nsplit=_splits(30000, _cdiv(30000, 512))))
    add("gram_blocks_workspace", "gram", 30000, None, 200, dict(form="blocks", bound="workspace", nsplit=_splits(30000, 20)),
        ws=20 * 200 * 200 * 4 + 4096)

    # ---- the cost pass (launch_cost): column splits, loads of 4 or 8 rank rows, one or two V buffers, vector X loads ----
    add("cost_csplit_kl", "cost", 1000, 4000, 50, dict(op="kl", csplit=15, NN=4, vdb=1, VEC=1), beta=1.0)
    add("cost_one_split_frob", "cost", 100000, 200, 50, dict(op="frob", csplit=1, NN=4, vdb=1, VEC=1), beta=2.0)
    add("cost_nn8_gen", "cost", 3000, 1000, 100, dict(op="gen", NN=8, vdb=0, VEC=1), beta=0.5)
    add("cost_vdb0_kl", "cost", 3000, 1000, 64, dict(op="kl", NN=4, vdb=0, VEC=1), beta=1.0)
    add("cost_nn8_vdb1", "cost", 3000, 1000, 120, dict(op="kl", NN=8, vdb=1, VEC=1), beta=1.0)
    add("cost_unaligned", "cost", 3000, 1000, 50, dict(op="kl", NN=4, VEC=0), beta=1.0, ld=1001)
    return cases


CASE_NAMES = list(plan_cases(256))
# what test_plan_table requires the table as a whole to reach
REQUIRED = {("xht", "form"): {"lds", "small", "round32", "round43", "rounds", "two_tiles"},
            ("xty", "bound"): {"occupancy", "rows_cap", "workspace", "offset32"},
            ("gram", "form"): {"small", "single", "slabs", "blocks"},
            ("gram", "bound"): {"workspace"},
            ("mu_left", "bm"): {"KL", "KLC", "GEN", "FROB"},
            ("mu_left", "form"): {"small", "mid", "hi"},
            ("mu_right", "bound"): {"occupancy", "workspace", "offset32"},
            ("mu_right", "bm"): {"KL", "GEN"},
            ("cost", "NN"): {"4", "8"}, ("cost", "vdb"): {"0", "1"}, ("cost", "VEC"): {"0", "1"}}
# what the cases at ranks 65 .. 128 (report lines with mt >= 5) must reach on their own
REQUIRED_BIG = {("mu_left", "mt"): set("5678"), ("mu_right", "mt"): set("5678"),
                ("mu_left", "form"): {"small", "mid", "rows128"}, ("mu_left", "rem"): {"0", "4"},
                ("mu_left", "bm"): {"KL", "GEN"}, ("mu_right", "bm"): {"KL", "GEN"},
                ("mu_left", "vec"): {"0", "1"}, ("mu_right", "vec"): {"0", "1"},
                ("mu_right", "bound"): {"occupancy", "min_rows", "workspace", "offset32"}}
TAG_KEYS = ("form", "bound", "bm", "NN", "vdb", "VEC", "tiling", "mt", "rem", "vec")


def note_plan(seen, seen_big, launcher, kv):
    """Adds the tags of one report line to `seen`, and to `seen_big` when the line is a MU plan of five or more rank tiles."""
    for key in TAG_KEYS:
        if key in kv:
            seen[(launcher, key)].add(str(kv[key]))
            if launcher in ("mu_left", "mu_right") and int(kv["mt"]) >= 5:
                seen_big[(launcher, key)].add(str(kv[key]))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- data: nonnegative, X as a view of a wider buffer when ld > n (the padding holds NaN) ----
def make_inputs(case, seed, dev="cuda"):
    g = torch.Generator(device=dev).manual_seed(seed)
    m, n, r = case.m, case.n, case.r
    if case.kernel == "gram":
        return {"A": torch.rand(r, m, device=dev, generator=g)}
    if case.kernel == "cp3_partial_cost":
        I, J, K = 300, m // 300, n
        return {"T": torch.rand(I, J, K, device=dev, generator=g),
                "Ft": [torch.rand(r, d, device=dev, generator=g) + 0.05 for d in (I, J, K)]}
    ld = case.ld or n
    buf = torch.empty(m, ld, device=dev)
    if ld > n:
        buf[:, n:] = float("nan")
    X = buf[:, :n]
    X.copy_(torch.rand(m, n, device=dev, generator=g) + 0.05)
    Ut = torch.rand(r, m, device=dev, generator=g) + 0.05
    V = torch.rand(r, n, device=dev, generator=g) + 0.05
    return {"X": X, "Ut": Ut, "V": V}


def mu_right_terms_fp64(X, Ut, V, beta):
    """(num, den) of the right update in fp64, U^T (K^(beta-2) .* X) and U^T K^(beta-1) (beta = 1: den[k] = sum_i U[i, k], a
    vector), summed over row blocks of at most 2^25 entries of X (an fp64 copy of the widest X at once is 4 GB)."""
    V64 = V.double()
    num = torch.zeros(V.shape, dtype=torch.float64, device=V.device)
    den = torch.zeros(V.shape, dtype=torch.float64, device=V.device)
    step = max(64, (1 << 25) // X.shape[1])
    for i0 in range(0, X.shape[0], step):
        U64, X64 = Ut[:, i0:i0 + step].double(), X[i0:i0 + step].double()
        K = U64.t() @ V64
        num += U64 @ (K ** (beta - 2) * X64)
        if beta != 1:
            den += U64 @ K ** (beta - 1)
    return num, (Ut.double().sum(dim=1) if beta == 1 else den)


def mu_accum_into(eng, inp, beta, num, den, dvec):
    """nnf_mu_right_accum_f32 on caller-owned outputs (Engine.mu_right_accum allocates its own)."""
    from nn_fac_amd.engine import _ld, _ptr
    X, Ut, V = inp["X"], inp["Ut"], inp["V"]
    st = eng.lib.nnf_mu_right_accum_f32(eng.ctx, _ptr(X), X.shape[0], X.shape[1], _ld(X), _ptr(Ut), _ld(Ut), _ptr(V), _ld(V),
                                        Ut.shape[0], float(beta), _ptr(num), _ld(num), _ptr(den), _ld(den), _ptr(dvec),
                                        eng._stream())
    assert st == 0, st


def gamma_beta(beta):
    return 1 / (2 - beta) if beta < 1 else (1 / (beta - 1) if beta > 2 else 1.0)


def mu_left_fp64(X, Ut, V, beta):
    U, V, X = Ut.double().t(), V.double(), X.double()
    K = U @ V
    if beta == 1:
        return torch.clamp(U * ((X / K) @ V.t() / V.sum(dim=1)), min=1e-12).t()
    return torch.clamp(U * ((K ** (beta - 2) * X) @ V.t() / (K ** (beta - 1) @ V.t())) ** gamma_beta(beta), min=1e-12).t()


def mu_right_fp64(X, Ut, V, beta):
    U, V, X = Ut.double(), V.double(), X.double()
    K = U.t() @ V
    if beta == 1:
        return torch.clamp(V * ((U @ (X / K)) / U.sum(dim=1, keepdim=True)), min=1e-12)
    return torch.clamp(V * ((U @ (K ** (beta - 2) * X)) / (U @ K ** (beta - 1))) ** gamma_beta(beta), min=1e-12)


def betadiv_fp64(X, Ut, V, beta):
    X, P = X.double(), Ut.double().t() @ V.double()
    if beta == 1:
        return float((X * torch.log(X / P) - X + P).sum())
    if beta == 2:
        return float(0.5 * ((X - P) ** 2).sum())
    return float(((X ** beta + (beta - 1) * P ** beta - beta * X * P ** (beta - 1)) / (beta * (beta - 1))).sum())


def assert_close(got, want, glob, ent, what):
    """Finite, global relative error <= glob, entrywise relative error <= ent (every entry of want is positive)."""
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite entries (a tile never written)"
    d = (got - want).abs()
    g = float(d.norm() / want.norm())
    e = float((d / want.abs()).max())
    assert g <= glob and e <= ent, f"{what}: global {g:.3e} (<= {glob}), entrywise {e:.3e} (<= {ent}) at {int((d / want.abs()).argmax())}"


_ENGINES = {}


def engine_for(case):
    from nn_fac_amd.engine import Engine, get_engine
    if case.ws is None:
        return get_engine("cuda:0")
    if case.ws not in _ENGINES:
        _ENGINES[case.ws] = Engine(torch.device("cuda:0"), workspace_bytes=case.ws)
    return _ENGINES[case.ws]


def run_case(eng, case, inp, out=None, cost_out=None):
    """The launch the case is about, on `eng`.  Returns the output tensor (or the cost scalar tensor)."""
    k = case.kernel
    if k == "xht":
        return eng.xht(inp["X"], inp["V"], out=out)
    if k == "xty":
        return eng.xty(inp["X"], inp["Ut"], out=out)
    if k == "gram":
        return eng.gram(inp["A"], out=out)
    if k == "mu_left":
        return eng.mu_left(inp["X"], inp["Ut"], inp["V"], case.beta, out=out, cost_out=cost_out)
    if k == "mu_right":
        return eng.mu_right(inp["X"], inp["Ut"], inp["V"], case.beta, out=out)
    if k == "mu_accum":
        return eng.mu_right_accum(inp["X"], inp["Ut"], inp["V"], case.beta)
    if k == "cost":
        return eng.betadiv(inp["X"], inp["Ut"], inp["V"], case.beta, out=out)
    if k == "cp3_partial_cost":
        T, Ft = inp["T"], inp["Ft"]
        Y = out if out is not None else torch.empty(case.r, T.shape[0], T.shape[1], device=T.device)
        eng.cp3_partial_cost(T, Ft, Y, cost_out)
        return Y
    raise AssertionError(k)


def other_data(case, inp):
    """Inputs of the same shape with different values (for the call before the measured one)."""
    out = dict(inp)
    if "V" in inp:
        out["V"] = inp["V"] * 3 + 1
    if "Ut" in inp:
        out["Ut"] = inp["Ut"] * 2 + 0.5
    if "A" in inp:
        out["A"] = inp["A"] * 3 + 1
    if "Ft" in inp:
        out["Ft"] = [f * 2 + 1 for f in inp["Ft"]]
    return out


# ---- the plan table, as the library reports it ----
_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_launch_plans as P
C = P._cus()
cases = P.plan_cases(C)
for name, case in cases.items():
    sys.stderr.write("[case] %s\n" % name)
    sys.stderr.flush()
    inp = P.make_inputs(case, 1)
    eng = P.engine_for(case)
    cost = torch.empty(1, dtype=torch.float64, device="cuda")
    P.run_case(eng, case, inp, cost_out=cost if case.kernel == "cp3_partial_cost" else None)
    if P.has_fused_cost(case):
        P.run_case(eng, case, inp, cost_out=cost)
    torch.cuda.synchronize()
    del inp
    torch.cuda.empty_cache()
print("done")
"""


def parse_plans(stderr):
    """{case name: [(launcher, {key: value})]} from the child's stderr."""
    plans, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("[case] "):
            cur = line[7:].strip()
            plans[cur] = []
        elif line.startswith("[nnf plan] ") and cur is not None:
            f = line[11:].split()
            plans[cur].append((f[0], dict(kv.split("=", 1) for kv in f[1:])))
    return plans


@pytest.fixture(scope="module")
def reported(built_lib):
    p = subprocess.run([sys.executable, "-c", _CHILD], env=dict(os.environ, NNF_PLAN_DEBUG="1"), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    return parse_plans(p.stderr)


def _launcher_of(case):
    return {"cost": "cost", "cp3_partial_cost": "mu_left", "mu_accum": "mu_right"}.get(case.kernel, case.kernel)


def has_fused_cost(case):
    """The KL left update has a second form that carries the cost, up to rank 64 (test_fused_kl_cost_rank_limit)."""
    return case.kernel == "mu_left" and case.beta == 1.0 and case.r <= 64


def test_plan_table(reported):
    """Every case of PLAN_CASES takes the plan it is listed with (one report line of its launcher per call), and the table as
    a whole reaches every form and bound tag of the launchers."""
    cases = plan_cases(_cus())
    assert sorted(reported) == sorted(cases)
    seen, seen_big = collections.defaultdict(set), collections.defaultdict(set)
    bad = []
    for name, case in cases.items():
        lines = [kv for (l, kv) in reported[name] if l == _launcher_of(case)]
        calls = 2 if has_fused_cost(case) else 1
        if len(lines) != calls:
            bad.append((name, "report lines", reported[name]))
            continue
        kv = lines[0]
        assert int(kv["K" if case.kernel == "gram" else "m"]) == case.m and int(kv["r"]) == case.r, (name, kv)
        for key, want in case.expect.items():
            if kv.get(key) != str(want):
                bad.append((name, key, kv.get(key), want))
        if calls == 2:      # the fused-cost form keeps the KL update's plan
            klc = lines[1]
            if klc.get("bm") != "KLC" or {k: v for k, v in klc.items() if k != "bm"} != {k: v for k, v in kv.items() if k != "bm"}:
                bad.append((name, "KLC plan", klc, kv))
        for l, kvs in reported[name]:
            note_plan(seen, seen_big, l, kvs)
        if case.kernel == "xht" and int(kv["tail_parts"]) > 0:
            seen[("xht", "tail_parts")].add(kv["tail_parts"])
        if case.kernel == "cost":
            seen[("cost", "csplit")].add("1" if kv["csplit"] == "1" else ">1")
    assert not bad, "\n".join(map(str, bad))
    for key, want in REQUIRED.items():
        assert want <= seen[key], (key, want - seen[key])
    for key, want in REQUIRED_BIG.items():
        assert want <= seen_big[key], ("mt >= 5", key, want - seen_big[key])
    assert {"4", "8", "16", "32"} <= seen[("xht", "tail_parts")]
    assert seen[("cost", "csplit")] == {"1", ">1"}
    print("reached:", {f"{l}.{k}": sorted(v) for (l, k), v in sorted(seen.items())})
    print("reached at mt >= 5:", {f"{l}.{k}": sorted(v) for (l, k), v in sorted(seen_big.items())})


# ---- values ----
@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_values(name, built_lib):
    """Each case against fp64 on the device, entry by entry.  The measured call writes into a NaN-filled output right after a
    call on the same shape with other data (same engine): a tile, share or split left out shows as NaN or as the other call's
    value, never as the right one."""
    case = plan_cases(_cus())[name]
    eng = engine_for(case)
    inp = make_inputs(case, 7)
    k = case.kernel
    if k == "cost":
        out = torch.empty(1, dtype=torch.float64, device="cuda")
        run_case(eng, case, other_data(case, inp), out=out)
        out.fill_(1e300)
        got = float(run_case(eng, case, inp, out=out))
        want = betadiv_fp64(inp["X"], inp["Ut"], inp["V"], case.beta)
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
        return
    if k == "cp3_partial_cost":
        T, Ft = inp["T"], inp["Ft"]
        cost = torch.empty(1, dtype=torch.float64, device="cuda")
        Y = torch.empty(case.r, T.shape[0], T.shape[1], device="cuda")
        run_case(eng, case, other_data(case, inp), out=Y, cost_out=cost)
        Y.fill_(float("nan"))
        cost.fill_(1e300)
        run_case(eng, case, inp, out=Y, cost_out=cost)
        T64, F = T.double(), [f.double() for f in Ft]
        assert_close(Y, torch.einsum("ijk,rk->rij", T64, F[2]), 1e-5, 1e-4, name)
        want = float(((T64 - torch.einsum("ri,rj,rk->ijk", *F)) ** 2).sum())
        assert abs(float(cost) - want) <= 1e-5 * want, (float(cost), want)
        return
    if k == "mu_accum":
        want_num, want_den = mu_right_terms_fp64(inp["X"], inp["Ut"], inp["V"], case.beta)
        run_case(eng, case, other_data(case, inp))
        num, den = (torch.full((case.r, case.n), float("nan"), device="cuda") for _ in range(2))
        dvec = torch.full((case.r,), float("nan"), dtype=torch.float64, device="cuda")
        mu_accum_into(eng, inp, case.beta, num, den, dvec)
        assert_close(num, want_num, 2e-5, 1e-3, name + " num")
        if case.beta == 1:      # den[k] in fp64 from fp32 entries: only the order of the m additions differs
            assert float(((dvec - want_den).abs() / want_den).max()) <= 1e-12 and bool(torch.isnan(den).all())
        else:
            assert_close(den, want_den, 2e-5, 1e-3, name + " den")
            assert bool(torch.isnan(dvec).all())
        return
    if k == "xht":
        want = inp["V"].double() @ inp["X"].double().t()
    elif k == "xty":
        want = inp["Ut"].double() @ inp["X"].double()
    elif k == "gram":
        want = inp["A"].double() @ inp["A"].double().t()
    elif k == "mu_left":
        want = mu_left_fp64(inp["X"], inp["Ut"], inp["V"], case.beta)
    elif case.r > 64:       # (the widest X: fp64 in row blocks)
        num, den = mu_right_terms_fp64(inp["X"], inp["Ut"], inp["V"], case.beta)
        ratio = num / (den[:, None] if case.beta == 1 else den)
        want = torch.clamp(inp["V"].double() * ratio ** gamma_beta(case.beta), min=1e-12)
        del num, den, ratio
    else:
        want = mu_right_fp64(inp["X"], inp["Ut"], inp["V"], case.beta)
    out = torch.empty(want.shape, dtype=torch.float32, device="cuda")
    run_case(eng, case, other_data(case, inp), out=out)
    out.fill_(float("nan"))
    got = run_case(eng, case, inp, out=out)
    assert got.data_ptr() == out.data_ptr()
    mu = k in ("mu_left", "mu_right")
    assert_close(got, want, 2e-5 if mu else 1e-5, 1e-3 if mu else 1e-4, name)


# ---- the fused KL cost of the left update (nnf_mu_left_kl_cost_f32) ----
KL_CASES = [nm for nm in CASE_NAMES if has_fused_cost(plan_cases(256)[nm])]


@pytest.mark.parametrize("name", KL_CASES)
def test_fused_kl_cost(name, built_lib):
    """cost_out = beta_divergence(X, U V, 1) of the input factors in fp64 (overwritten, not accumulated), and the update is
    nnf_mu_left_f32's bit for bit."""
    case = plan_cases(_cus())[name]
    eng = engine_for(case)
    inp = make_inputs(case, 11)
    cost = torch.full((1,), 1e300, dtype=torch.float64, device="cuda")
    out = torch.empty(case.r, case.m, device="cuda")
    run_case(eng, case, other_data(case, inp), out=out, cost_out=cost)
    out.fill_(float("nan"))
    cost.fill_(1e300)
    fused = run_case(eng, case, inp, out=out, cost_out=cost).clone()
    want = betadiv_fp64(inp["X"], inp["Ut"], inp["V"], 1.0)
    assert abs(float(cost) - want) <= 1e-5 * want, (float(cost), want)
    plain = run_case(eng, case, inp)
    assert torch.equal(fused, plain)


def test_fused_kl_cost_rank_limit(built_lib):
    """The fused cost stops at rank 64: r = 65 with cost_out is refused by the wrapper and by the C entry point."""
    from nn_fac_amd.engine import EngineError, get_engine
    eng = get_engine("cuda:0")
    X = torch.rand(300, 70, device="cuda") + 0.05
    for r, ok in ((64, True), (65, False)):
        Ut, V = torch.rand(r, 300, device="cuda") + 0.05, torch.rand(r, 70, device="cuda") + 0.05
        cost = torch.empty(1, dtype=torch.float64, device="cuda")
        if ok:
            eng.mu_left(X, Ut, V, 1.0, cost_out=cost)
            continue
        with pytest.raises(EngineError, match="beta = 1 and r <= 64"):
            eng.mu_left(X, Ut, V, 1.0, cost_out=cost)
        O = torch.empty_like(Ut)
        st = eng.lib.nnf_mu_left_kl_cost_f32(eng.ctx, X.data_ptr(), 300, 70, 70, Ut.data_ptr(), 300, V.data_ptr(), 70, r,
                                             O.data_ptr(), 300, cost.data_ptr(), eng._stream())
        assert st == -3      # NNF_ERR_UNSUPPORTED


# ---- the X H^T switches, read once per process ----
_SWITCH_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_launch_plans as P
cases = P.plan_cases(P._cus())
eng = P.engine_for(cases["xht_round32_parts8"])
res = {}
for name in ("xht_round32_parts8", "xht_two_tiles"):
    case = cases[name]
    sys.stderr.write("[case] %s\n" % name)
    sys.stderr.flush()
    inp = P.make_inputs(case, 3)
    out = torch.empty(case.r, case.m, device="cuda")
    P.run_case(eng, case, P.other_data(case, inp), out=out)
    out.fill_(float("nan"))
    P.run_case(eng, case, inp, out=out)
    res[name] = out.cpu()
torch.save(res, sys.argv[1])
print("done")
"""


def _switch_run(tmp_path, tag, env):
    path = str(tmp_path / f"{tag}.pt")
    p = subprocess.run([sys.executable, "-c", _SWITCH_CHILD, path], env=dict(os.environ, NNF_PLAN_DEBUG="1", **env),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    plans = parse_plans(p.stderr)
    return torch.load(path), {nm: [kv for l, kv in v if l == "xht"][-1] for nm, v in plans.items()}


def test_xht_tail_and_two_tile_switches(tmp_path, built_lib):
    """NNF_XHT_TAIL=0 and NNF_XHT_NT2=0 / 1 (read once per process, so one child each way): both forms of a tail case and of
    a two-tile case against fp64, and the rows the forms contract in the same k order come out bit for bit the same."""
    on, plan_on = _switch_run(tmp_path, "on", {"NNF_XHT_TAIL": "1", "NNF_XHT_NT2": "1"})
    off, plan_off = _switch_run(tmp_path, "off", {"NNF_XHT_TAIL": "0", "NNF_XHT_NT2": "0"})
    tail_case = plan_on["xht_round32_parts8"]
    assert int(tail_case["tail_parts"]) == 8 and int(plan_off["xht_round32_parts8"]["tail_parts"]) == 0
    assert plan_on["xht_two_tiles"]["form"] == "two_tiles" and plan_off["xht_two_tiles"]["form"] == "rounds"
    cases = plan_cases(_cus())
    for name in ("xht_round32_parts8", "xht_two_tiles"):
        inp = make_inputs(cases[name], 3)
        want = inp["V"].double() @ inp["X"].double().t()
        for res in (on, off):
            assert_close(res[name].cuda(), want, 1e-5, 1e-4, name)
    # rows below the tail's first row: every form sums a row's 64-column chunks in the same order
    row0 = 64 * (int(tail_case["nth"]) - 1) * int(tail_case["grid"])
    a, b = on["xht_round32_parts8"], off["xht_round32_parts8"]
    assert torch.equal(a[:, :row0], b[:, :row0])
    assert torch.equal(on["xht_two_tiles"], off["xht_two_tiles"])


# ---- a workspace too small for one slab ----
def test_workspace_too_small_for_one_slab(built_lib):
    """xty, mu_right and the Gram refuse with NNF_ERR_WORKSPACE when not even one split-K slab fits, and write nothing."""
    from nn_fac_amd.engine import Engine, EngineError
    eng = Engine(torch.device("cuda:0"), workspace_bytes=4096)
    m, n, r = 5000, 2000, 50
    X = torch.rand(m, n, device="cuda") + 0.05
    Ut, V = torch.rand(r, m, device="cuda") + 0.05, torch.rand(r, n, device="cuda") + 0.05
    for call in (lambda o: eng.xty(X, Ut, out=o), lambda o: eng.mu_right(X, Ut, V, 1.0, out=o),
                 lambda o: eng.mu_right(X, Ut, V, 0.5, out=o)):
        out = torch.full((r, n), float("nan"), device="cuda")
        with pytest.raises(EngineError, match=WS_ERR):
            call(out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
    A = torch.rand(200, 30000, device="cuda")               # blocks: rank above 128
    G = torch.full((200, 200), float("nan"), device="cuda")
    with pytest.raises(EngineError, match=WS_ERR):
        eng.gram(A, out=G)
    A = torch.rand(50, 30000, device="cuda")                # slabs into a strided output (no unsplit form)
    Gw = torch.full((50, 64), float("nan"), device="cuda")
    with pytest.raises(EngineError, match=WS_ERR):
        eng.gram(A, out=Gw[:, :50])
    # K > 512 splits: the fp32 chains must be split (one chain over all of K missed the single-call bound, 1.5e-5)
    A = torch.rand(128, 512 * (2 * _cus() + 1) + 100, device="cuda")
    Gs = torch.full((128, 128), float("nan"), device="cuda")
    with pytest.raises(EngineError, match=WS_ERR):
        eng.gram(A, out=Gs)
    torch.cuda.synchronize()
    assert bool(torch.isnan(G).all()) and bool(torch.isnan(Gw).all()) and bool(torch.isnan(Gs).all())

"""The launch plan of the WEIGHTED mode update on the tensor's own layout (nnf_mu_mode_w_f32; mu_plan_mode with its weighted flag in
nn_fac_amd/csrc/k_mu_plan.h) at 256 and at 304 compute units, without a GPU: the `mu_mode_w` line of tools/nnf_plan.cpp.

What differs from the unweighted plan (tests/test_mu_mode_plan.py): every beta takes two sets of slabs and nothing in front of them
(no r doubles, no row-sum pieces), the form is reported as bm=WGEN, 16-byte loads need the weights aligned too (walign=), and the
resident workgroups per CU are those of the weighted instantiations' registers: four at MT = 1 (128 VGPRs), three at MT = 2 (148 |
156), two at MT = 3 and 4 (180 .. 212).  The unweighted lines of the same shapes must stay what test_mu_mode_plan.py expects."""
import pytest

from test_mu_plan_table import ask
import test_mu_mode_plan as base
from test_mu_mode_plan import BY_OCCUPANCY, CHUNK, CUS, MANY_CHUNKS, MANY_CHUNKS_RANKS, ROWS, SHAPES, UNIT, UNITS_CAP, WS_DEFAULT, cdiv, rup

RANKS = (1, 20, 33, 64)
BETAS = (1.0, 0.5, 2.0)


def line(C, L, I, K, r, beta, ws=WS_DEFAULT, extra=""):
    return "mu_mode_w %d %d %d %d %d %r %d%s" % (C, L, I, r, K, beta, ws, extra)


def carved_w(r, I, nsplit):
    """What the launcher takes from a 256-byte aligned bump allocator: two sets of nsplit slabs of r x rup(I, 4) floats, no prologue."""
    off = 0
    for b in [4 * nsplit * r * rup(I, 4)] * 2:
        off = rup(off, 256) + b
    return off


def wgpc_w(r):
    return {1: 4, 2: 3, 3: 2, 4: 2}[cdiv(r, 16)]


@pytest.mark.parametrize("C", CUS)
def test_row_blocks_and_splits_cover_the_tensor(C):
    cases = [(L, I, K, r, beta) for (L, I, K) in SHAPES for r in RANKS for beta in BETAS]
    for (L, I, K, r, beta), plan in zip(cases, ask([line(C, *c) for c in cases])):
        tag = (C, L, I, K, r, beta, plan)
        assert "status" not in plan, tag
        assert plan["mt"] == cdiv(r, 16) and plan["bm"] == "WGEN" and plan["vec"] == int(K % 4 == 0), tag
        assert plan["kt"] == cdiv(K, UNIT) and plan["units"] == L * cdiv(K, UNIT), tag
        assert plan["wgpc"] == wgpc_w(r), tag
        # the row blocks cover I, the last one starts inside it
        assert plan["nrb"] * ROWS >= I > (plan["nrb"] - 1) * ROWS, tag
        # every unit is covered once: the splits cover the units, the last one starts inside them, whole chunks each
        assert plan["ups"] % CHUNK == 0 and plan["nsplit"] >= 1, tag
        assert plan["nsplit"] * plan["ups"] >= plan["units"] > (plan["nsplit"] - 1) * plan["ups"], tag
        # the fp32 chain of a workgroup: at most 256 units (the workspace is ample here)
        assert plan["bound"] in ("occupancy", "chain", "min_cols") and plan["ups"] <= UNITS_CAP, tag
        if plan["bound"] == "occupancy":
            want = max(1, plan["wgpc"] * C // plan["nrb"])
            assert plan["nsplit"] == cdiv(plan["units"], rup(cdiv(plan["units"], want), CHUNK)), tag
        # two slab sets and no prologue, at every beta
        assert plan["pieces"] == 0 and plan["ldp"] == rup(I, 4), tag
        assert plan["ws_bytes"] == carved_w(r, I, plan["nsplit"]) <= WS_DEFAULT, tag


@pytest.mark.parametrize("C", CUS)
def test_the_plan_does_not_depend_on_beta(C):
    for (L, I, K) in SHAPES:
        for r in RANKS:
            a, b, c = ask([line(C, L, I, K, r, beta) for beta in BETAS])
            assert a == b == c, (L, I, K, r, a, b, c)


@pytest.mark.parametrize("C", CUS)
def test_the_weights_alignment_decides_the_load_width(C):
    got = ask([line(C, 2, 260, 260, 20, 0.5), line(C, 2, 260, 260, 20, 0.5, extra=" walign=1"),
               line(C, 2, 260, 260, 20, 0.5, extra=" align=1"), line(C, 2, 260, 260, 20, 0.5, extra=" ldv=521"),
               line(C, 2, 260, 261, 20, 0.5)])
    assert [g["vec"] for g in got] == [1, 0, 0, 0, 0], got


@pytest.mark.parametrize("C", CUS)
def test_a_small_workspace_bounds_the_splits(C):
    cases, lines = [], []
    for (L, I, K) in [(2, 260, 260), (5, 33, 71), (1, 70, 203), (500, 500, 500)]:
        for r in (1, 20, 64):
            for beta in BETAS:
                for s in (1, 2, 3):
                    cases.append((L, I, K, r, beta, s, carved_w(r, I, s)))
                    lines.append(line(C, L, I, K, r, beta, ws=cases[-1][-1]))
                cases.append((L, I, K, r, beta, 0, carved_w(r, I, 1) - 1))
                lines.append(line(C, L, I, K, r, beta, ws=cases[-1][-1]))
    for (L, I, K, r, beta, s, ws), plan in zip(cases, ask(lines)):
        tag = (C, L, I, K, r, beta, s, ws, plan)
        if s == 0:
            assert plan == {"status": -4}, tag
            continue
        assert "status" not in plan and plan["ws_max"] == s and plan["nsplit"] <= s, tag
        assert plan["nsplit"] * plan["ups"] >= plan["units"] > (plan["nsplit"] - 1) * plan["ups"], tag
        assert plan["ws_bytes"] <= ws, tag
        units = L * cdiv(K, UNIT)
        if cdiv(units, CHUNK) > s:
            assert plan["bound"] == "workspace" and plan["nsplit"] == cdiv(units, rup(cdiv(units, s), CHUNK)), tag


@pytest.mark.parametrize("C", CUS)
def test_refusals(C):
    got = ask([line(C, 2, 260, 260, 65, 1.0),              # rank above 64: NNF_ERR_UNSUPPORTED
               line(C, 2, 260, 260, 64, 1.0),              # (the last rank taken)
               line(C, 0, 260, 260, 20, 1.0),              # empty extents, a negative beta, a short pitch of V: NNF_ERR_ARG
               line(C, 2, 0, 260, 20, 1.0),
               line(C, 2, 260, 0, 20, 1.0),
               line(C, 2, 260, 260, 20, -1.0),
               line(C, 2, 260, 260, 20, 1.0, extra=" ldv=519"),
               line(C, 2, 260, 260, 20, 1.0, ws=0)])       # no workspace: NNF_ERR_WORKSPACE
    assert [g.get("status", 0) for g in got] == [-3, 0, -1, -1, -1, -1, -1, -4], got


@pytest.mark.parametrize("C", CUS)
def test_the_many_chunk_cases_are_what_they_say(C):
    """What tests/test_gpu_mu_mode_w.py runs against fp64: two splits of 256 | 260 units on a two-split workspace, and the
    occupancy-bound shape with several chunks per workgroup at every rank."""
    cases = [(s, r, b) for s in MANY_CHUNKS for r in MANY_CHUNKS_RANKS for b in BETAS]
    lines = [line(C, *s, r, b, ws=carved_w(r, s[1], 2)) for s, r, b in cases]
    for ((L, I, K), r, beta), plan in zip(cases, ask(lines)):
        units = L * cdiv(K, UNIT)
        assert units in (512, 520) and plan["bound"] == "workspace" and plan["nsplit"] == 2 and plan["nrb"] == 2, plan
        assert plan["ups"] == units // 2 and plan["vec"] == int(K % 4 == 0), plan
    for plan in ask([line(C, *BY_OCCUPANCY, r, b) for r in MANY_CHUNKS_RANKS for b in BETAS]):
        assert plan["bound"] == "occupancy" and plan["vec"] == 1 and plan["nrb"] == 3 and 8 <= plan["ups"] <= 40, plan


@pytest.mark.parametrize("C", CUS)
def test_the_flagship_shape_fills_the_device(C):
    """500^3 at rank 30 (MT = 2: three workgroups per CU): 8 row blocks, between two and three workgroups per CU."""
    for plan in ask([line(C, 500, 500, 500, 30, b) for b in BETAS]):
        assert plan["nrb"] == 8 and plan["wgpc"] == 3 and 2 * C <= plan["nrb"] * plan["nsplit"] <= 3 * C, plan


@pytest.mark.parametrize("C", CUS)
def test_the_unweighted_lines_are_unchanged(C):
    """The mu_mode lines of the same shapes: what tests/test_mu_mode_plan.py expects of them, field by field."""
    cases = [(L, I, K, r, beta) for (L, I, K) in SHAPES for r in RANKS for beta in base.BETAS]
    for (L, I, K, r, beta), plan in zip(cases, ask([base.line(C, *c) for c in cases])):
        tag = (C, L, I, K, r, beta, plan)
        kl = beta == 1.0
        assert plan["bm"] == ("KL" if kl else "GEN") and plan["wgpc"] == base.wgpc_of(r, kl, K % 4 == 0), tag
        assert plan["pieces"] == (base.pieces_of(L * K) if kl else 0), tag
        assert plan["ws_bytes"] == base.carved(r, I, plan["pieces"], plan["nsplit"], kl), tag
        if plan["bound"] == "occupancy":
            want = max(1, plan["wgpc"] * C // plan["nrb"])
            assert plan["nsplit"] == cdiv(plan["units"], rup(cdiv(plan["units"], want), CHUNK)), tag

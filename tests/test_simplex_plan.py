"""The launch plan of the simplex projection (nnf_simplex_proj_kl_f32; simplex_make_plan in nn_fac_amd/csrc/k_simplex_plan.h) at
256 and at 304 compute units, without a GPU: tools/nnf_plan.cpp prints it from the header the launcher takes it from.

The plan's edges: G in {1, 4, 16, 64} lanes per column; a lane holds at most 8 rows (G >= r / 8) and a group is never wider
than four times the rank (G = 1, or r > G / 4); among those the largest G with cols * G <= 1024 lanes per CU, else the smallest;
256 / G columns per workgroup."""
import pytest

from test_mu_plan_table import ask

CUS = (256, 304)
GROUPS = (1, 4, 16, 64)
ROWS_PER_LANE, LANES_PER_CU, BLOCK = 8, 1024, 256
RANKS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 50, 64, 65, 100, 128)


def cdiv(a, b):
    return -(-a // b)


def allowed(r):
    return [G for G in GROUPS if cdiv(r, G) <= ROWS_PER_LANE and (G == 1 or r > G // 4)]


def line(C, r, cols, **kw):
    return "simplex %d r=%d cols=%d" % (C, r, cols) + "".join(" %s=%d" % kv for kv in kw.items())


def test_the_groups_a_rank_allows():
    """One rank on each side of every threshold of the rule."""
    assert [allowed(r) for r in RANKS] == [[1], [1, 4], [1, 4], [1, 4], [1, 4, 16], [1, 4, 16], [4, 16], [4, 16], [4, 16, 64],
                                           [4, 16, 64], [16, 64], [16, 64], [16, 64], [16, 64], [16, 64], [16, 64]]


def check_cover(plan, r, cols, tag):
    G = plan["G"]
    assert G in allowed(r), tag
    # the kernel instance holds the lane's rows; the workgroups cover every column exactly once: column j belongs to workgroup
    # j // cpb, the last workgroup starts inside the columns
    assert plan["rpl"] in (1, 2, 4, 8) and plan["rpl"] >= cdiv(r, G) and (plan["rpl"] == 1 or plan["rpl"] // 2 < cdiv(r, G)), tag
    assert plan["cpb"] == BLOCK // G and plan["grid"] * plan["cpb"] >= cols > (plan["grid"] - 1) * plan["cpb"], tag


@pytest.mark.parametrize("C", CUS)
def test_group_choice_on_each_side_of_every_threshold(C):
    cases = []
    for r in RANKS:
        al = allowed(r)
        for G in al:      # the last column count at which G still fits 1024 lanes per CU, and the first at which it does not
            edge = C * LANES_PER_CU // G
            cases += [(r, edge), (r, edge + 1)]
        cases += [(r, 1), (r, 63), (r, 2000), (r, 70001), (r, 10 ** 6)]
    for (r, cols), plan in zip(cases, ask([line(C, r, cols) for r, cols in cases])):
        tag = (C, r, cols, plan)
        assert "status" not in plan and plan["forced"] == 0 and plan["max_iter"] == 100 and plan["ws_bytes"] == 808, tag
        check_cover(plan, r, cols, tag)
        fits = [G for G in allowed(r) if cols * G <= C * LANES_PER_CU]
        assert plan["G"] == (max(fits) if fits else min(allowed(r))), tag


@pytest.mark.parametrize("C", CUS)
def test_the_shapes_the_plan_was_made_for(C):
    """Config B's 50 x 2000 H spreads over the chip with 64 lanes per column; 10^5 and more columns take one or four."""
    b, wide20, wide5 = ask([line(C, 50, 2000), line(C, 20, 100000), line(C, 5, 100000)])
    assert b["G"] == 64 and b["grid"] == 500
    assert wide20["G"] == 4 and wide5["G"] == 1


@pytest.mark.parametrize("C", CUS)
def test_forced_groups(C):
    cases = [(r, cols, G) for r in RANKS for cols in (1, 257, 70001) for G in GROUPS]
    for (r, cols, G), plan in zip(cases, ask([line(C, r, cols, force=G) for r, cols, G in cases])):
        tag = (C, r, cols, G, plan)
        if G in allowed(r):
            assert plan.get("G") == G and plan["forced"] == 1, tag
            check_cover(plan, r, cols, tag)
        else:
            assert plan == {"status": -3}, tag


@pytest.mark.parametrize("C", CUS)
def test_refusals(C):
    """Each refusal is decided before the launcher touches the workspace or launches anything (k_simplex.hip returns the plan's
    status, or the argument check's, first)."""
    got = ask([line(C, 129, 10),                       # rank above 128: NNF_ERR_UNSUPPORTED
               line(C, 128, 10),                       # (the last rank taken)
               line(C, 5, 10, max_iter=0),             # max_iter outside 1 .. 1024: NNF_ERR_UNSUPPORTED
               line(C, 5, 10, max_iter=1025),
               line(C, 5, 10, max_iter=1024),
               line(C, 5, 10, max_iter=1),
               line(C, 0, 10), line(C, 5, 0),          # empty extents, a short pitch, both / neither denominator, a force that is
               line(C, 5, 10, pitch=9),                # none of the four: NNF_ERR_ARG
               line(C, 5, 10, both=1), line(C, 5, 10, both=-1),
               line(C, 5, 10, force=2),
               line(C, 5, 10, ws=807),                 # a workspace one byte short of max_iter + 1 words: NNF_ERR_WORKSPACE
               line(C, 5, 10, ws=808),
               line(C, 5, 10, max_iter=1024, ws=8199), line(C, 5, 10, max_iter=1024, ws=8200)])
    assert [g.get("status", 0) for g in got] == [-3, 0, -3, -3, 0, 0, -1, -1, -1, -1, -1, -1, -4, 0, -4, 0], got

"""The launch plan of the mode update on the tensor's own layout (nnf_mu_mode_f32; mu_plan_mode in nn_fac_amd/csrc/k_mu_plan.h)
at 256 and at 304 compute units, without a GPU: tools/nnf_plan.cpp prints it from the header the launcher takes it from, as
tests/test_mu_plan_table.py does for the matrix kernels.

The plan's edges (k_mu_plan.h): 64 rows of I per workgroup (MU_MODE_ROWS), 16 k per unit (MU_MODE_UNIT; a unit never straddles two
l), 4 units per staged chunk (MU_MODE_CHUNK: the units per split are a multiple of it), at most 256 units per split
(MU_MODE_UNITS_CAP: the fp32 chain of one workgroup) unless the workspace holds fewer slabs, rank <= 64."""
import pytest

from test_mu_plan_table import ask

CUS = (256, 304)
WS_DEFAULT = 1024 << 20
ROWS, UNIT, CHUNK, UNITS_CAP = 64, 16, 4, 256
SHAPES = [(1, 70, 203), (5, 33, 71), (7, 16, 64), (3, 130, 129), (40, 9, 5), (6, 1, 50), (9, 50, 1), (1, 1, 1), (2, 260, 260),
          # both sides of the edges: rows per workgroup, k per unit, units per chunk, units per split
          (1, 64, 16), (1, 65, 17), (2, 63, 15), (1, 128, 64), (1, 129, 65), (3, 64, 4096), (3, 64, 4097), (1, 20, 16 * 256 * 2 + 1),
          # (more row blocks than a quarter of the resident workgroups: the chain bound sets the splits)
          (1, 4000, 100000),
          (500, 500, 500), (1, 500, 250000)]
RANKS = (1, 20, 30, 33, 64)
BETAS = (1.0, 0.5)


# Many chunks per workgroup (tests/test_gpu_mu_mode.py runs them against fp64).  (L, I, K): 512 | 520 units over four l, K % 4 == 0 and
# != 0 -- on a context whose workspace holds two splits' slabs that is 256 | 260 units per split, both sides of MU_MODE_UNITS_CAP;
# and one shape the default context splits by occupancy into several chunks per workgroup, as it does the drivers' tensors
MANY_CHUNKS = [(4, 70, 2048), (4, 70, 2080), (4, 70, 2046), (4, 70, 2078)]
MANY_CHUNKS_RANKS = (1, 20, 33, 64)
BY_OCCUPANCY = (16, 130, 4096)


def cdiv(a, b):
    return -(-a // b)


def rup(a, b):
    return cdiv(a, b) * b


def line(C, L, I, K, r, beta, ws=WS_DEFAULT, extra=""):
    return "mu_mode %d %d %d %d %d %r %d%s" % (C, L, I, r, K, beta, ws, extra)


def pieces_of(cols):
    return 64 if cols // 8192 > 64 else cols // 8192 if cols // 8192 > 1 else 1


def carved(r, I, pieces, nsplit, kl):
    """What the launcher takes from a 256-byte aligned bump allocator: r doubles, the row sums' partials (beta = 1, long rows),
    then one (beta = 1) or two sets of nsplit slabs of r x rup(I, 4) floats."""
    off = 0
    takes = [8 * r] + ([8 * r * pieces] if pieces > 1 else []) + [4 * nsplit * r * rup(I, 4)] * (1 if kl else 2)
    for b in takes:
        off = rup(off, 256) + b
    return off


def wgpc_of(r, kl, vec):
    """Resident workgroups per CU the plan aims at: four up to 128 VGPRs of the instantiation, three beyond (k_mu_plan.h)."""
    mt = cdiv(r, 16)
    return 4 if (mt <= 3 or vec if kl else mt <= 2) else 3


def all_cases(C):
    return [(L, I, K, r, beta) for (L, I, K) in SHAPES for r in RANKS for beta in BETAS]


@pytest.mark.parametrize("C", CUS)
def test_row_blocks_and_splits_cover_the_tensor(C):
    cases = all_cases(C)
    for (L, I, K, r, beta), plan in zip(cases, ask([line(C, *c) for c in cases])):
        tag = (C, L, I, K, r, beta, plan)
        assert "status" not in plan, tag
        kl = beta == 1.0
        assert plan["mt"] == cdiv(r, 16) and plan["bm"] == ("KL" if kl else "GEN") and plan["vec"] == int(K % 4 == 0), tag
        assert plan["kt"] == cdiv(K, UNIT) and plan["units"] == L * cdiv(K, UNIT), tag
        assert plan["wgpc"] == wgpc_of(r, kl, K % 4 == 0), tag
        # the row blocks cover I, the last one starts inside it
        assert plan["nrb"] * ROWS >= I > (plan["nrb"] - 1) * ROWS, tag
        # the splits cover the units, the last one starts inside them, whole chunks each
        assert plan["ups"] % CHUNK == 0 and plan["nsplit"] >= 1, tag
        assert plan["nsplit"] * plan["ups"] >= plan["units"] > (plan["nsplit"] - 1) * plan["ups"], tag
        # the fp32 chain of a workgroup: at most 256 units (the workspace is ample here)
        assert plan["bound"] in ("occupancy", "chain", "min_cols") and plan["ups"] <= UNITS_CAP, tag
        if plan["bound"] == "occupancy":
            want = max(1, plan["wgpc"] * C // plan["nrb"])
            assert plan["nsplit"] == cdiv(plan["units"], rup(cdiv(plan["units"], want), CHUNK)), tag
        # the workspace the plan counts is what the launcher carves
        assert plan["pieces"] == (pieces_of(L * K) if kl else 0) and plan["ldp"] == rup(I, 4), tag
        assert plan["ws_bytes"] == carved(r, I, plan["pieces"], plan["nsplit"], kl) <= WS_DEFAULT, tag


@pytest.mark.parametrize("C", CUS)
def test_the_flagship_shapes_fill_the_device(C):
    """500^3 at rank 30 (the benchmark's NTF shape) and its first mode as a matrix: 8 row blocks, at least 3 workgroups per CU."""
    for shape in ((500, 500, 500), (1, 500, 250000)):
        for plan in ask([line(C, *shape, 30, b) for b in BETAS]):
            assert plan["nrb"] == 8 and plan["wgpc"] == 4 and 3 * C <= plan["nrb"] * plan["nsplit"] <= 4 * C, plan


@pytest.mark.parametrize("C", CUS)
def test_a_small_workspace_bounds_the_splits(C):
    """With exactly the bytes of s splits the plan takes s (or fewer, by the rounding of the units per split) and names the
    workspace as the bound; one byte less than one split's worth is refused with NNF_ERR_WORKSPACE."""
    cases, lines = [], []
    for (L, I, K) in [(2, 260, 260), (5, 33, 71), (1, 70, 203), (500, 500, 500)]:
        for r in (1, 20, 64):
            for beta in BETAS:
                kl = beta == 1.0
                p = pieces_of(L * K) if kl else 0
                for s in (1, 2, 3):
                    cases.append((L, I, K, r, beta, s, carved(r, I, p, s, kl)))
                    lines.append(line(C, L, I, K, r, beta, ws=cases[-1][-1]))
                cases.append((L, I, K, r, beta, 0, carved(r, I, p, 1, kl) - 1))
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
               line(C, 2, 260, 260, 65, 0.5),
               line(C, 2, 260, 260, 64, 1.0),              # (the last rank taken)
               line(C, 0, 260, 260, 20, 1.0),              # empty extents, a negative beta, a short pitch of V: NNF_ERR_ARG
               line(C, 2, 0, 260, 20, 1.0),
               line(C, 2, 260, 0, 20, 1.0),
               line(C, 2, 260, 260, 20, -1.0),
               line(C, 2, 260, 260, 20, 1.0, extra=" ldv=519"),
               line(C, 2, 260, 260, 20, 1.0, extra=" ldv=520"),
               line(C, 2, 260, 260, 20, 1.0, ws=0)])       # no workspace: NNF_ERR_WORKSPACE
    assert [g.get("status", 0) for g in got] == [-3, -3, 0, -1, -1, -1, -1, -1, 0, -4], got


@pytest.mark.parametrize("C", CUS)
def test_the_many_chunk_cases_are_what_they_say(C):
    """The workspace-bound cases: two splits of 256 | 260 units = 64 | 65 chunks per workgroup, each split two whole l.  The
    occupancy-bound case: at least two chunks per workgroup at every rank."""
    cases = [(s, r, b) for s in MANY_CHUNKS for r in MANY_CHUNKS_RANKS for b in BETAS]
    lines = [line(C, *s, r, b, ws=carved(r, s[1], 1, 2, b == 1.0)) for s, r, b in cases]
    for ((L, I, K), r, beta), plan in zip(cases, ask(lines)):
        units = L * cdiv(K, UNIT)
        assert units in (512, 520) and plan["bound"] == "workspace" and plan["nsplit"] == 2 and plan["nrb"] == 2, plan
        assert plan["ups"] == units // 2 and plan["vec"] == int(K % 4 == 0), plan
    for plan in ask([line(C, *BY_OCCUPANCY, r, b) for r in MANY_CHUNKS_RANKS for b in BETAS]):
        assert plan["bound"] == "occupancy" and plan["vec"] == 1 and plan["nrb"] == 3 and 8 <= plan["ups"] <= 20, plan

"""The launch plan and the chunk table of the CSR kernels (nnf_csr_xf_f32, nnf_csr_kl_f32; nn_fac_amd/csrc/k_sparse_plan.h)
without a GPU: tools/nnf_plan.cpp prints them from the header the launcher and the kernels take them from.

A matrix is cut into chunks of at most CH consecutive stored entries of one row (one wave each); the rows of the edge cases are
the lengths 0, 1, CH - 1, CH, CH + 1 and 3 CH + 5.  The chunks must cover every stored entry exactly once and in order, the
workspace the plan states must be what the launcher's cursor hands out, and the table nn_fac_amd.engine.csr_chunk_table builds
with torch (what the kernels are handed at run time) must be the tool's."""
import pytest
import torch

from test_mu_plan_table import ask

CUS = (256, 304)
CH_MIN, CH_MAX, WAVES_PER_CU = 64, 1024, 16


def line(C, r, lens, **kw):
    return "sparse %d r=%d lens=%s" % (C, r, ",".join(str(k) for k in lens)) + "".join(" %s=%d" % kv for kv in kw.items())


def chunks_of(plan):
    text = plan["chunks"]
    return [] if text == "-" else [tuple(int(v) for v in c.split(":")) for c in str(text).split(",")]


def edge_lengths(ch):
    return [0, 1, ch - 1, ch, ch + 1, 3 * ch + 5]


def check_cover(plan, lens, ch, tag):
    """Every stored entry in exactly one chunk, chunks in row order and entry order, none longer than ch, none empty."""
    chunks = chunks_of(plan)
    assert plan["CH"] == ch and plan["nchunks"] == len(chunks) == sum(-(-k // ch) for k in lens), tag
    nxt, rows = 0, []
    for row, first, end in chunks:
        assert first == nxt and 0 < end - first <= ch, (tag, row, first, end)
        nxt = end
        rows.append(row)
    assert nxt == sum(lens) == plan["nnz"] and rows == sorted(rows), tag
    begin = 0
    for i, k in enumerate(lens):      # a row's chunks hold exactly its entries; all but its last are full
        mine = [(f, e) for row, f, e in chunks if row == i]
        assert (mine[0][0], mine[-1][1]) == (begin, begin + k) if k else not mine, (tag, i)
        assert all(e - f == ch for f, e in mine[:-1]), (tag, i)
        begin += k


def rup(a, b):
    return -(-a // b) * b


@pytest.mark.parametrize("C", CUS)
@pytest.mark.parametrize("ch", [1, 7, 64, 512])
def test_chunks_cover_every_stored_entry_once_and_in_order(C, ch):
    cases = [edge_lengths(ch), list(reversed(edge_lengths(ch))), [0, 0, 0], [3 * ch + 5], [0], [1], [ch] * 5, [0, ch + 1, 0, 0, 2 * ch]]
    for lens, plan in zip(cases, ask([line(C, 10, lens, ch=ch) for lens in cases])):
        assert "status" not in plan, (lens, plan)
        check_cover(plan, lens, ch, (C, ch, lens))
        assert plan["nrows"] == len(lens) and plan["grid"] == -(-plan["nchunks"] // 4) and plan["tgrid"] == -(-len(lens) // 64)


@pytest.mark.parametrize("C", CUS)
def test_chunk_size_from_sizes_alone(C):
    """A quarter of one wave's share of the stored entries, as a power of two inside [64, 1024] (one long row carries nnz here)."""
    for nnz in (0, 1, 63, 64 * 4 * WAVES_PER_CU * C - 1, 64 * 4 * WAVES_PER_CU * C, 128 * 4 * WAVES_PER_CU * C, 200 * 4 * WAVES_PER_CU * C,
                4 * 10 ** 7, 2 * 10 ** 8, 2 ** 31 - 1):
        plan, = ask([line(C, 50, [nnz])])
        share = nnz // (4 * WAVES_PER_CU * C)
        want = CH_MIN
        while want * 2 <= CH_MAX and want * 2 <= share:
            want *= 2
        assert plan["CH"] == want, (C, nnz, plan["CH"])
    # 10^6 x 4000 at 1 %: 4e7 stored entries over 256 CUs are 2441 per wave in flight -> chunks of 1024
    assert ask([line(256, 50, [4 * 10 ** 7])])[0]["CH"] == 1024


@pytest.mark.parametrize("C", CUS)
def test_lanes_and_workspace_are_what_the_launcher_carves(C):
    lens = edge_lengths(64) + [17] * 9
    nchunks = sum(-(-k // 64) for k in lens)
    for r in (1, 4, 5, 8, 9, 10, 16, 17, 32, 33, 50, 64, 65, 100, 128):
        pieces = -(-r // 4)
        L = next(p for p in (1, 2, 4, 8, 16, 32) if p >= pieces)
        for out, cost in ((1, 0), (1, 1), (0, 1)):
            plan, = ask([line(C, r, lens, ch=64, out=out, cost=cost)])
            tag = (C, r, out, cost, plan)
            assert (plan["L"], plan["G"], plan["rp"]) == (L, 64 // L, rup(r, 4)), tag
            assert plan["U"] == (4 if L >= 16 else 2 if L >= 4 else 1) and plan["G"] * plan["U"] >= 8, tag
            assert plan["part_bytes"] == (nchunks * rup(r, 4) * 4 if out else 0), tag
            assert plan["cost_bytes"] == (8 * -(-nchunks // 4) if cost else 0), tag
            assert plan["lds_bytes"] == 64 * (rup(r, 4) + 1) * 4 <= 64 * 1024, tag
            # each carve starts on a 256-byte boundary of the workspace; the plan's figure is where the cursor ends up
            want = rup(plan["part_bytes"], 256) + plan["cost_bytes"] if cost else plan["part_bytes"]
            assert plan["ws_bytes"] == plan["carved"] == want, tag
            # one byte less than that is refused, exactly that much is taken
            assert ask([line(C, r, lens, ch=64, out=out, cost=cost, ws=want - 1)])[0] == {"status": -4}, tag
            assert "status" not in ask([line(C, r, lens, ch=64, out=out, cost=cost, ws=want)])[0], tag


@pytest.mark.parametrize("C", CUS)
def test_refusals_and_empty_matrices(C):
    got = ask([line(C, 129, [5]),                      # rank above 128: NNF_ERR_UNSUPPORTED
               line(C, 128, [5]),
               line(C, 0, [5]),                        # no rank, no chunk size, nothing asked for: NNF_ERR_ARG
               line(C, 5, [5], ch=0),
               line(C, 5, [5], out=0, cost=0),
               line(C, 5, [0, 0, 0, 0]),               # an all-empty matrix: no chunk, no workspace, the second kernel writes zeros
               line(C, 5, [0, 0, 0, 0], ws=0),
               line(C, 5, [0]),                        # nrows = 1
               line(C, 5, [200])])
    assert [g.get("status", 0) for g in got] == [-3, 0, -1, -1, -1, 0, 0, 0, 0], got
    empty = got[5]
    assert (empty["nchunks"], empty["grid"], empty["tgrid"], empty["ws_bytes"], empty["chunks"]) == (0, 0, 1, 0, "-")
    assert (got[7]["nchunks"], got[7]["tgrid"]) == (0, 1) and chunks_of(got[8]) == [(0, 0, 64), (0, 64, 128), (0, 128, 192), (0, 192, 200)]


@pytest.mark.parametrize("ch", [1, 7, 64])
def test_the_table_torch_builds_is_the_tools(ch):
    """nn_fac_amd.engine.csr_chunk_table (plain index arithmetic, on the device at run time) against the chunks of the tool."""
    from nn_fac_amd.engine import csr_chunk_table
    lens = edge_lengths(ch) + [0, 0, 2 * ch, 1, 0]
    rowptr = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0)
    rowchunk, chunk_row = csr_chunk_table(rowptr, ch)
    chunks = chunks_of(ask([line(256, 10, lens, ch=ch)])[0])
    assert rowchunk.dtype == torch.int64 and chunk_row.dtype == torch.int32
    assert chunk_row.tolist() == [row for row, _, _ in chunks]
    assert rowchunk.tolist() == [sum(1 for row, _, _ in chunks if row < i) for i in range(len(lens) + 1)]
    # all-empty: no chunk
    rowchunk, chunk_row = csr_chunk_table(torch.zeros(4, dtype=torch.int64), ch)
    assert rowchunk.tolist() == [0, 0, 0, 0] and chunk_row.numel() == 0

"""The launch plan of the sparse-tensor kernels (nnf_sptensor_mttkrp_f32, nnf_sptensor_kl_f32; nn_fac_amd/csrc/k_sparse_plan.h)
without a GPU: tools/nnf_plan.cpp prints it from the header the launcher and the kernels take it from.

One mode's sorted copy of a tensor is cut like a CSR matrix whose rows are the slices of the mode (tests/test_sparse_plan.py: the
chunk rule, the cover of the stored entries); what the `sptensor` line adds is ng = N - 1 gathered factors per entry and, with
them, the entries a lane keeps in flight: U(L, ng) = 2 U_csr(L) / ng rounded down to a power of two, at least 1."""
import pytest
import torch

from test_mu_plan_table import ask
from test_sparse_plan import check_cover, chunks_of, edge_lengths, rup

CUS = (256, 304)
RANKS = (1, 10, 50, 64, 65, 100, 128)
NGS = (2, 3, 4)


def line(C, r, ng, lens, **kw):
    return "sptensor %d r=%d ng=%d lens=%s" % (C, r, ng, ",".join(str(k) for k in lens)) + "".join(" %s=%d" % kv for kv in kw.items())


def unroll(L, ng):
    """2 U_csr / ng as a power of two: the table at the head of the plan's section of k_sparse_plan.h, written out."""
    return {2: {1: 1, 2: 1, 4: 2, 8: 2, 16: 4, 32: 4}, 3: {1: 1, 2: 1, 4: 1, 8: 1, 16: 2, 32: 2}, 4: {1: 1, 2: 1, 4: 1, 8: 1, 16: 2, 32: 2}}[ng][L]


@pytest.mark.parametrize("C", CUS)
@pytest.mark.parametrize("ng", NGS)
def test_lanes_entries_in_flight_grids_and_workspace(C, ng):
    lens = edge_lengths(64) + [17] * 9
    nchunks = sum(-(-k // 64) for k in lens)
    for r in RANKS:
        pieces = -(-r // 4)
        L = next(p for p in (1, 2, 4, 8, 16, 32) if p >= pieces)
        for out, cost in ((1, 0), (1, 1), (0, 1)):
            plan, = ask([line(C, r, ng, lens, ch=64, out=out, cost=cost)])
            tag = (C, r, ng, out, cost, plan)
            assert "status" not in plan, tag
            assert (plan["L"], plan["G"], plan["rp"], plan["ng"]) == (L, 64 // L, rup(r, 4), ng), tag
            assert plan["U"] == unroll(L, ng) and plan["U"] * ng <= 8, tag      # at most 8 16-byte pieces in flight per lane
            assert plan["grid"] == -(-nchunks // 4) and plan["tgrid"] == (-(-len(lens) // 64) if out else 0), tag
            assert plan["part_bytes"] == (nchunks * rup(r, 4) * 4 if out else 0), tag
            assert plan["cost_bytes"] == (8 * -(-nchunks // 4) if cost else 0), tag
            assert plan["lds_bytes"] == 64 * (rup(r, 4) + 1) * 4 <= 64 * 1024, tag
            want = rup(plan["part_bytes"], 256) + plan["cost_bytes"] if cost else plan["part_bytes"]
            assert plan["ws_bytes"] == plan["carved"] == want, tag
            # one byte less than that is refused, exactly that much is taken
            assert ask([line(C, r, ng, lens, ch=64, out=out, cost=cost, ws=want - 1)])[0] == {"status": -4}, tag
            assert "status" not in ask([line(C, r, ng, lens, ch=64, out=out, cost=cost, ws=want)])[0], tag
            # everything but U is the CSR plan of the same row lengths
            csr, = ask(["sparse %d r=%d lens=%s ch=64 out=%d cost=%d" % (C, r, ",".join(str(k) for k in lens), out, cost)])
            for key in ("L", "G", "rp", "grid", "tgrid", "lds_bytes", "part_bytes", "cost_bytes", "ws_bytes", "nchunks", "chunks"):
                assert plan[key] == csr[key], (key, tag)


@pytest.mark.parametrize("C", CUS)
def test_refusals_and_empty_tensors(C):
    got = ask([line(C, 129, 2, [5]),                      # rank above 128: NNF_ERR_UNSUPPORTED
               line(C, 128, 2, [5]),
               line(C, 0, 2, [5]),                        # no rank, no chunk size, nothing asked for: NNF_ERR_ARG
               line(C, 5, 2, [5], ch=0),
               line(C, 5, 2, [5], out=0, cost=0),
               line(C, 5, 1, [5]),                        # ng outside 2 .. 4 (a matrix; an order-6 tensor): NNF_ERR_ARG
               line(C, 5, 5, [5]),
               line(C, 5, 0, [5]),
               line(C, 5, 4, [5]),
               line(C, 5, 3, [0, 0, 0, 0]),               # nothing stored: no chunk, no workspace, the second kernel writes zeros
               line(C, 5, 3, [0, 0, 0, 0], ws=0),
               line(C, 5, 2, [200])])
    assert [g.get("status", 0) for g in got] == [-3, 0, -1, -1, -1, -1, -1, -1, 0, 0, 0, 0], got
    empty = got[9]
    assert (empty["nchunks"], empty["grid"], empty["tgrid"], empty["ws_bytes"], empty["chunks"]) == (0, 0, 1, 0, "-")
    assert chunks_of(got[11]) == [(0, 0, 64), (0, 64, 128), (0, 128, 192), (0, 192, 200)]


@pytest.mark.parametrize("C", CUS)
@pytest.mark.parametrize("ch", [1, 7, 64, 512])
def test_chunk_spans_of_the_edge_slice_lengths(C, ch):
    """Slices of 0, 1, CH - 1, CH, CH + 1 and 3 CH + 5 entries: every stored entry in exactly one chunk, in order."""
    lens = edge_lengths(ch)
    for ng in NGS:
        plan, = ask([line(C, 10, ng, lens, ch=ch)])
        assert "status" not in plan, plan
        check_cover(plan, lens, ch, (C, ch, ng))
        want = [(i, b, min(b + ch, e)) for i, (s, e) in enumerate(zip([sum(lens[:i]) for i in range(len(lens))],
                                                                    [sum(lens[:i + 1]) for i in range(len(lens))]))
                for b in range(s, e, ch)]
        assert chunks_of(plan) == want, (C, ch, ng)


def test_the_table_of_a_mode_copy_is_the_tools():
    """What Engine.sparse_tensor hands the kernels for a mode (engine.csr_chunk_table on the copy's ptr) against the tool."""
    from nn_fac_amd.engine import csr_chunk_table
    ch = 64
    lens = edge_lengths(ch) + [0, 2 * ch]
    ptr = torch.tensor([0] + lens, dtype=torch.int64).cumsum(0)
    rowchunk, chunk_row = csr_chunk_table(ptr, ch)
    chunks = chunks_of(ask([line(256, 10, 3, lens, ch=ch)])[0])
    assert chunk_row.tolist() == [row for row, _, _ in chunks]
    assert rowchunk.tolist() == [sum(1 for row, _, _ in chunks if row < i) for i in range(len(lens) + 1)]

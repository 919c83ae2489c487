"""The fused MU kernels of ranks 65 .. 128 stay inside the chip's budget (no GPU needed: reads the ISA `make` keeps)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _budget_tool():
    spec = importlib.util.spec_from_file_location("mu_rank128_budget", os.path.join(ROOT, "tools", "mu_rank128_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rank_65_to_128_mu_kernels_fit_registers_and_lds_without_scratch(built_lib):
    """Every instantiation the dispatcher can select above rank 64 -- MT = 5 .. 8 rank tiles, KL and general beta, aligned and
    unaligned X, both kernels, and the left KL form with four leftover ranks on the VALU pipe: 33 in all -- is in the kept ISA (build/k_mu3.s .. k_mu6.s) with a private segment of 0 bytes
    and no spilled register, at most 512 VGPR + AGPR (one 256-thread workgroup per CU), and static LDS plus the dynamic LDS
    the launcher computes (csrc/k_mu_plan.h, through tools/nnf_plan.cpp) within the 160 KiB of a CU."""
    tool = _budget_tool()
    rows = tool.table()
    assert len(rows) == 33
    missing = [(r["side"], r["mt"], r["rem"], r["form"], r["vec"]) for r in rows if not r["found"]]
    assert not missing, missing
    for r in rows:
        tag = (r["side"], r["mt"], r["rem"], r["form"], r["vec"])
        assert r["scratch"] == 0 and r["spills"] == 0, (tag, r)
        assert r["regs"] <= 512, (tag, r)
        assert r["lds"] <= 160 * 1024, (tag, r)
        assert r["lds"] >= 2 * (2 * r["mt"] + (r["rem"] > 0)) * 256 * 16, (tag, r)      # (both chunk images, double-buffered, are in there)

"""Every row of test_gpu_hals_plans.hals_cases against the library's own HALS sweep plan, at 256 and at 304 compute units.  No GPU:
the plan is decided in a HIP-free header (nn_fac_amd/csrc/k_hals_plan.h) that takes the occupancy answers as plain figures, and
tools/nnf_plan.cpp, a plain host program over that header, prints the plan of a `hals` line as the library reports it under
NNF_HALS_DEBUG.  The per-CU figures are the pinned PER_CU of the table; test_hals_plan_table checks on the device that they are
what the MI355X reports and that the lines asked here are the calls the library is given."""
import subprocess

import pytest

from test_gpu_hals_plans import MFMA_RPS, PER_CU, RPS, ask_plan_tool, hals_cases, hals_line, hals_tool_plans
from test_mu_plan_table import CUS, plan_tool


@pytest.mark.parametrize("C", CUS)
def test_hals_cases_take_the_plans_they_name(C):
    """Every field a case lists, and its shape, is what the library's plan gives for the call that writes its last report."""
    cases = hals_cases(C)
    bad = []
    for name, kv in hals_tool_plans(C, cases).items():
        case = cases[name]
        if int(kv["r"]) != case.r or int(kv["ncols"]) != case.n:
            bad.append((name, "shape", kv["r"], kv["ncols"]))
        for key, want in case.expect.items():
            if kv.get(key) != str(want):
                bad.append((name, key, kv.get(key), want))
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.parametrize("C", CUS)
def test_hals_resident_columns(C):
    """nnf_hals_resident_columns: 256 columns per resident lane workgroup (128 per GCOL workgroup above rank 128), at most 2048."""
    lines = ["hals_resident %d r=%d pc_lane_res=%d" % (C, rp, PER_CU[("lane-resident", rp)]) for rp in RPS]
    want = ["columns=%d" % (256 * min(PER_CU[("lane-resident", rp)] * C, 2048)) for rp in RPS]
    lines.append("hals_resident %d r=200 pc_generic_gcol=%d" % (C, PER_CU[("generic-gcol", 0)]))
    want.append("columns=%d" % (128 * min(PER_CU[("generic-gcol", 0)] * C, 2048)))
    assert ask_plan_tool(lines) == want


def test_a_missing_figure_is_an_error():
    """A figure the plan asks for and the line does not give ends the tool, by name: no case passes on a silent zero."""
    line = hals_line(256, hals_cases(256)["mfma_r64_n32769"])
    assert " pc_mfma=%d" % PER_CU[("mfma", MFMA_RPS[3])] in line
    p = subprocess.run([plan_tool()], input=line.replace(" pc_mfma=", " pc_other=") + "\n", capture_output=True, text=True)
    assert p.returncode != 0 and "pc_mfma" in p.stderr and "[nnf hals]" not in p.stdout, (p.returncode, p.stdout, p.stderr)

"""Where the resident lane solve takes its 576-thread form (hals_plan::comm, k_hals_comm.hip: 8 compute waves + 1 communication
wave, 512 columns per workgroup, one per CU), at 256 and at 304 compute units, without a GPU: the plan header
(nn_fac_amd/csrc/k_hals_plan.h) through tools/nnf_plan.cpp.  The form is for mode-0 solves of the row-split ranks (33 .. 52)
whose 256-thread workgroups outnumber the CUs; everything else keeps the plan it had, and asks for no new occupancy figure."""
import subprocess

import pytest

from test_gpu_hals_plans import PER_CU, ask_plan_tool, parse_report, pick_rp
from test_mu_plan_table import CUS, plan_tool


def _line(C, r, n, mode=0, nsweeps=100, comm_pc=1, **kv):
    rp = pick_rp(r)
    f = dict(mode=mode, r=r, ncols=n, nsweeps=nsweeps, pc_lane_res=PER_CU[("lane-resident", rp)],
             pc_lane_stream=PER_CU[("lane-streaming", rp)])
    if comm_pc is not None:
        f["pc_lane_comm"] = comm_pc
    f.update(kv)
    return "hals %d " % C + " ".join("%s=%s" % item for item in f.items())


def _plan(line):
    return parse_report(ask_plan_tool([line])[0])


def _cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize("C", CUS)
def test_threshold_is_more_workgroups_than_cus(C):
    """cdiv(ncols, 256) == CUs keeps the 256-thread workgroups -- and asks for no figure of the new form --, one more takes it."""
    for r in (33, 50, 52):
        rp = pick_rp(r)
        old = _plan(_line(C, r, 256 * C, comm_pc=None))
        assert (old["layout"], old["comm"], old["grid"], old["per_cu"]) == ("lane-resident", "0", str(C), str(PER_CU[("lane-resident", rp)]))
        n = 256 * C + 1
        new = _plan(_line(C, r, n))
        assert (new["layout"], new["comm"], new["grid"], new["per_cu"]) == ("lane-resident", "1", str(_cdiv(n, 512)), "1")
        # everything else of the report line is what the 256-thread form has
        lane = _plan(_line(C, r, n, force="l"))
        assert lane["comm"] == "0" and lane["grid"] == str(C + 1)
        assert {k: v for k, v in new.items() if k not in ("comm", "grid", "per_cu")} == \
            {k: v for k, v in lane.items() if k not in ("comm", "grid", "per_cu")}


@pytest.mark.parametrize("C", CUS)
def test_a_chained_launch_and_a_cross_solve_take_it_too(C):
    n = 256 * C + 1
    assert _plan(_line(C, 50, n, sweep0=2))["comm"] == "1"
    p = _plan(_line(C, 50, n, own_start=1, ldvs=n + 3, ldv=n + 1, ldm=n + 2))
    assert (p["comm"], p["copy"]) == ("1", "0")              # (the kernel reads its start values itself, as the 256-thread form)


@pytest.mark.parametrize("C", CUS)
def test_other_calls_keep_their_plan(C):
    """Mode 1, ranks 32 and 53, the row-level flags, a form that does not fit, and more granules than the communication wave sums."""
    n = 256 * C + 1
    for line in (_line(C, 50, n, mode=1, nsweeps=3, comm_pc=None), _line(C, 32, n, comm_pc=None), _line(C, 53, n, comm_pc=None)):
        p = _plan(line)
        assert (p["layout"], p["comm"], p["grid"], p["err"]) == ("lane-resident", "0", str(C + 1), "0"), line
    for flags in (2, 4):                                     # NNF_HALS_NORMALIZE, NNF_HALS_NONZERO: the generic kernel
        p = _plan(_line(C, 50, n, flags=flags, comm_pc=None, pc_generic_lds=2))
        assert (p["layout"], p["comm"]) == ("generic-lds", "0")
    p = _plan(_line(C, 50, n, comm_pc=0))
    assert (p["comm"], p["grid"], p["per_cu"]) == ("0", str(C + 1), "2")
    if 2 * C > 512:                                          # resident in 256-thread workgroups, 513 granules
        p = _plan(_line(C, 50, 256 * 513, comm_pc=None))
        assert (p["layout"], p["comm"], p["grid"]) == ("lane-resident", "0", "513")


@pytest.mark.parametrize("C", CUS)
def test_force_letter(C):
    """NNF_HALS_FORCE=c...: the new form at any number of columns for ranks 33 .. 52, the lane kernel as `lane` gives it elsewhere."""
    for r, n in ((33, 513), (50, 700), (52, 1025), (50, 40000)):
        p = _plan(_line(C, r, n, force="c"))
        assert (p["layout"], p["comm"], p["grid"], p["per_cu"]) == ("lane-resident", "1", str(_cdiv(n, 512)), "1")
    for r, mode in ((50, 1), (32, 0), (53, 0), (20, 0)):
        kw = dict(mode=mode, nsweeps=3, comm_pc=None)
        c, l = _plan(_line(C, r, 700, force="c", **kw)), _plan(_line(C, r, 700, force="l", **kw))
        assert c == l and c["layout"] == "lane-resident" and c["comm"] == "0"


@pytest.mark.parametrize("C", CUS)
def test_resident_columns_are_unchanged(C):
    lines = ["hals_resident %d r=%d pc_lane_res=%d" % (C, r, PER_CU[("lane-resident", pick_rp(r))]) for r in (33, 50, 52)]
    assert ask_plan_tool(lines) == ["columns=%d" % (256 * min(2 * C, 2048))] * 3


def test_the_new_figure_is_asked_for_by_name():
    line = _line(256, 50, 256 * 256 + 1, comm_pc=None)
    p = subprocess.run([plan_tool()], input=line + "\n", capture_output=True, text=True)
    assert p.returncode != 0 and "pc_lane_comm" in p.stderr and "[nnf hals]" not in p.stdout, (p.returncode, p.stdout, p.stderr)

"""Every row of test_gpu_launch_plans.plan_cases (MU, X H^T, W^T X, Gram, cost; cp3_partial_cost is a left MU update at a fixed
shape and has its plan checked on the device only) and every row of test_gpu_tensor_plans.tensor_cases (MTTKRP by segments and by
rows, the two dimension-tree contractions, the CP cost) and every pass of test_gpu_mu_above_128.ratio_cases (the ratio pass of the
MU route above rank 128) against the library's own plan arithmetic, at 256 and at 304 compute units.  No GPU: the launchers take their plans from HIP-free
headers (nn_fac_amd/csrc/k_stream_plan.h, k_mu_plan.h), and tools/nnf_plan.cpp, a plain host program over the same headers,
prints the plan of a case as the library reports it under NNF_PLAN_DEBUG.  This is what keeps the tables' shapes on the side of
the thresholds they name on a machine that cannot ask the library (test_plan_table and test_tensor_plan_table do, on the device)."""
import atexit
import collections
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

import test_gpu_mu_above_128 as above
import test_gpu_tensor_plans as tensor
from test_gpu_launch_plans import REQUIRED, REQUIRED_BIG, ROOT, _cdiv, note_plan, parse_plans, plan_cases

WS_DEFAULT = 1024 << 20         # get_engine's context
CUS = (256, 304)
LAUNCHER = {"mu_left": "mu_left", "mu_right": "mu_right", "mu_accum": "mu_right", "xht": "xht", "xty": "xty", "gram": "gram",
            "cost": "cost"}


@functools.lru_cache(maxsize=None)
def plan_tool():
    """tools/nnf_plan.cpp, built once with the host compiler (no ROCm include path)."""
    tmp = tempfile.mkdtemp(prefix="nnf_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    exe = os.path.join(tmp, "nnf_plan")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-I", os.path.join(ROOT, "nn_fac_amd", "csrc"),
                    os.path.join(ROOT, "tools", "nnf_plan.cpp"), "-o", exe], check=True)
    return exe


def ask(lines):
    """The tool's answer to each case line: the fields of the report line (numbers as int), or {"status": code}."""
    p = subprocess.run([plan_tool()], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
    answers = p.stdout.splitlines()
    assert len(answers) == len(lines), p.stdout[-2000:]
    out = []
    for n, text in enumerate(answers):
        reports = parse_plans("[case] %d\n%s\n" % (n, text))[str(n)]
        kv = reports[0][1] if reports else dict([text.split("=", 1)])
        out.append({k: int(v) if v.lstrip("-").isdigit() else v for k, v in kv.items()})
    return out


def case_line(C, case):
    if case.kernel == "gram":       # the factor is r x m, contiguous, and so is G
        return "gram %d %d %d %d %d 0 %d" % (C, case.m, case.m, case.r, case.m, WS_DEFAULT if case.ws is None else case.ws)
    return "%s %d %d %d %d %d %r %d" % (LAUNCHER[case.kernel], C, case.m, case.n, case.r, case.ld or case.n, case.beta or 0.0,
                                        WS_DEFAULT if case.ws is None else case.ws)


@functools.lru_cache(maxsize=None)
def _answers(C):
    lines = [case_line(C, c) for c in plan_cases(C).values() if c.kernel in LAUNCHER]
    return dict(zip(lines, ask(lines)))


def plan_of(C, case):
    return _answers(C)[case_line(C, case)]


def mu_cases(C):
    return {nm: c for nm, c in plan_cases(C).items() if c.kernel in ("mu_left", "mu_right", "mu_accum")}


@pytest.mark.parametrize("C", CUS)
def test_mu_cases_take_the_plans_they_name(C):
    """Every field a MU case lists is what the library's plan gives, and the workgroups of every left plan cover the
    rows with none of them starting beyond the last row."""
    bad = []
    for name, case in mu_cases(C).items():
        plan = plan_of(C, case)
        for key, want in case.expect.items():
            if str(plan.get(key)) != str(want):
                bad.append((name, key, plan.get(key), want))
        if case.kernel == "mu_left" and "status" not in plan:
            sizes = [256] * plan["n_hi"] + [192] * plan["n_mid"] + [128] * (plan["grid"] - plan["n_hi"] - plan["n_mid"])
            assert plan["grid"] >= plan["n_hi"] + plan["n_mid"] and sum(sizes) >= case.m > sum(sizes[:-1]), (name, plan)
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.parametrize("C", CUS)
def test_mu_cases_reach_required(C):
    """The MU rows reach what REQUIRED names for the two launchers, and the rows at ranks 65 .. 128 reach REQUIRED_BIG on
    their own; the thresholds the table says it straddles are straddled."""
    cases = mu_cases(C)
    seen, seen_big = collections.defaultdict(set), collections.defaultdict(set)
    plans = {}
    for name, case in cases.items():
        plans[name] = plan = plan_of(C, case)
        assert "status" not in plan, (name, plan)
        note_plan(seen, seen_big, "mu_left" if case.kernel == "mu_left" else "mu_right", plan)
    for key, want in REQUIRED.items():
        if key[0] in ("mu_left", "mu_right"):
            assert want - {"KLC", "FROB"} <= seen[key], (key, want - seen[key])      # (the cost-carrying forms: second calls)
    for key, want in REQUIRED_BIG.items():
        assert want <= seen_big[key], (key, want - seen_big[key])
    big = {nm: p for nm, p in plans.items() if p["mt"] >= 5}
    # left: both sides of every edge, per (mt, rem) of the KL forms with a 192-row workgroup
    for mt, rem in [(6, 0), (6, 4), (7, 0), (8, 0)]:
        mine = [p for nm, p in big.items() if cases[nm].kernel == "mu_left" and (p["mt"], p["rem"], p["bm"], p["vec"]) == (mt, rem, "KL", 1)]
        T = {_cdiv(p["m"], 16): p for p in mine}
        s = C
        assert all(p["slots"] == s for p in mine)
        for t, form in [(8 * s, "small"), (8 * s + 1, "mid"), (8 * s + 4, "mid"), (12 * s, "mid"), (12 * s + 1, "rows128"),
                        (16 * s, "rows128"), (16 * s + 1, "mid"), (24 * s + 1, "mid")]:
            assert t in T and T[t]["form"] == form, (mt, rem, t, form)
        assert T[12 * s]["n_mid"] == T[12 * s]["grid"] == s and T[8 * s + 1]["n_mid"] == T[8 * s + 4]["n_mid"] == 1
    for nm, p in big.items():
        if cases[nm].kernel == "mu_left" and (p["mt"] == 5 or p["bm"] == "GEN"):
            assert p["n_mid"] == p["n_hi"] == 0 and p["grid"] == _cdiv(p["m"], 128), (nm, p)
            assert p["slots"] == (2 * C if p["mt"] == 5 and p["bm"] == "KL" else C)
    assert {p["r"] for p in big.values() if p.get("rem") == 4} == {97, 100}
    # right: every bound at MT = 5 and 8 in both beta forms, a one-split plan, a multi-split accumulate-only plan per form
    for mt in (5, 8):
        for bm in ("KL", "GEN"):
            got = {p["bound"] for nm, p in big.items() if cases[nm].kernel == "mu_right" and (p["mt"], p["bm"]) == (mt, bm)}
            assert got == {"occupancy", "min_rows", "workspace", "offset32"}, (mt, bm, got)
            assert any(p["nsplit"] == 1 and p["ncb"] > C for nm, p in big.items()
                       if cases[nm].kernel == "mu_right" and (p["mt"], p["bm"]) == (mt, bm))
    for nm, p in plans.items():
        if cases[nm].kernel == "mu_right" and p["bound"] == "workspace":
            assert p["nsplit"] == p["ws_max"], (nm, p)
    acc = {(p["mt"] >= 5, p["bm"], p["bound"]) for nm, p in plans.items() if cases[nm].kernel == "mu_accum" and p["nsplit"] > 1}
    assert acc >= {(False, "KL", "occupancy"), (False, "GEN", "occupancy"), (True, "KL", "occupancy"),
                   (True, "GEN", "occupancy"), (True, "GEN", "workspace")}, acc


def xcases(C):
    return {nm: c for nm, c in plan_cases(C).items() if c.kernel in ("xht", "xty")}


@pytest.mark.parametrize("C", CUS)
def test_xht_xty_cases_take_the_plans_they_name(C):
    """Every field an X H^T or W^T X case lists is what the library's plan gives, the table reaches what REQUIRED names for the two
    launchers, and the workgroups (and tail tiles) of every X H^T plan cover the rows."""
    seen, bad = collections.defaultdict(set), []
    for name, case in xcases(C).items():
        plan = plan_of(C, case)
        assert "status" not in plan, (name, plan)
        for key, want in case.expect.items():
            if str(plan.get(key)) != str(want):
                bad.append((name, key, plan.get(key), want))
        note_plan(seen, collections.defaultdict(set), case.kernel, plan)
        if case.kernel == "xht":
            rows = 64 * (plan["n_hi"] * plan["nth"] + (plan["grid"] - plan["n_hi"]) * (plan["nth"] - 1)) + 16 * plan["tail_tiles"]
            assert plan["grid"] >= plan["n_hi"] and rows >= case.m, (name, plan)
            if plan["tail_parts"]:
                seen[("xht", "tail_parts")].add(str(plan["tail_parts"]))
    assert not bad, "\n".join(map(str, bad))
    for key in (("xht", "form"), ("xty", "bound")):
        assert REQUIRED[key] <= seen[key], (key, REQUIRED[key] - seen[key])
    assert {"4", "8", "16", "32"} <= seen[("xht", "tail_parts")]


def rows_line(C, case):
    """A mode-2 MTTKRP case of tensor_cases as the rows launcher sees it (its first rank pass): T as an (I J) x K matrix."""
    (I, J, K), ld, al = case.shape, case.ld or {}, case.align or {}
    return "mttkrp_rows %d %d %d %d %d 0 %d nb=%d lda=%d ldb=%d align=%d" % (
        C, I * J, K, min(case.R, 128), K, WS_DEFAULT if case.ws is None else case.ws, J, I + ld.get("f0", 0), J + ld.get("f1", 0),
        al.get("T", 0))


@pytest.mark.parametrize("C", CUS)
def test_mttkrp_rows_cases_take_the_plans_they_name(C):
    """Every field (or refusal) a mode-2 MTTKRP case of test_gpu_tensor_plans lists is what the library's plan gives, which is
    also what that file's own formula gives, and the rows reach what its REQUIRED names for the launcher."""
    cases = {nm: c for nm, c in tensor.tensor_cases(C).items() if c.kernel == "mttkrp" and c.mode == 2}
    plans = dict(zip(cases, ask([rows_line(C, c) for c in cases.values()])))
    seen, refused, bad = collections.defaultdict(set), set(), []
    for name, case in cases.items():
        plan = plans[name]
        formula = tensor.plan_of(C, case)
        if {k: str(v) for k, v in formula.items()} != {k: str(plan.get(k)) for k in formula}:
            bad.append((name, "formula", formula, plan))
        if "status" in plan or "status" in case.expect:
            if plan != case.expect:
                bad.append((name, plan, case.expect))
            refused.add(plan.get("status"))
            continue
        for key, want in case.expect.items():
            if str(plan.get(key)) != str(want):
                bad.append((name, key, plan.get(key), want))
        tensor._note(seen, "mttkrp_rows", plan)
        if plan["bound"] == "workspace":
            assert plan["nsplit"] == _cdiv(plan["m"], 64 * _cdiv(_cdiv(plan["m"], plan["ws_max"]), 64)), (name, plan)
    assert not bad, "\n".join(map(str, bad))
    for key, want in tensor.REQUIRED.items():
        if key[0] == "mttkrp_rows":
            assert want <= seen[key], (C, key, want - seen[key])
    assert tensor.ERR_WORKSPACE in refused


def tensor_line(C, case):
    """A mode-0 or mode-1 MTTKRP, dimension-tree or CP-cost case of tensor_cases as its launcher sees it: its first rank pass, for
    the CP cost its last (the pass that reads the model of the earlier ones)."""
    ld, al = case.ld or {}, case.align or {}
    ws = WS_DEFAULT if case.ws is None else case.ws
    if case.kernel == "partial":
        A, B = case.shape
        return "%s %d %d %d %d %d 0 %d" % (tensor.launcher_of(case), C, A, B, min(case.R, 128), B, ws)
    I, J, K = case.shape
    if case.kernel == "cp3":
        return "cost %d %d %d %d %d %r %d kr=%d pin=%d align=%d" % (
            C, I * J, K, case.R - 128 * ((case.R - 1) // 128), K, float(case.beta), ws, J, case.R > 128, al.get("T", 0))
    # mode 0: rows i, segments j (stride K) against factors 1 and 2; mode 1: rows j, segments i (stride J K) against factors 0 and 2
    nrows, ldrow, nseg, segstride, fsld = ((I, J * K, J, K, J + ld.get("f1", 0)) if case.mode == 0
                                           else (J, K, I, J * K, I + ld.get("f0", 0)))
    return "mttkrp_seg %d %d %d %d %d 0 %d nseg=%d segstride=%d fsld=%d fkld=%d fkalign=%d align=%d" % (
        C, nrows, K, min(case.R, 128), ldrow, ws, nseg, segstride, fsld, K + ld.get("f2", 0), al.get("f2", 0), al.get("T", 0))


@pytest.mark.parametrize("C", CUS)
def test_tensor_cases_take_the_plans_they_name(C):
    """Every field (or refusal) a mode-0 / mode-1 MTTKRP, dimension-tree or CP-cost case of test_gpu_tensor_plans lists is what the
    library's plan gives, which is also what that file's own formulas give, field by field; these rows reach what its REQUIRED and
    REQUIRED_REFUSALS name for their four launchers (the large cases need no memory here)."""
    cases = {nm: c for nm, c in tensor.tensor_cases(C).items() if not (c.kernel == "mttkrp" and c.mode == 2)}
    plans = dict(zip(cases, ask([tensor_line(C, c) for c in cases.values()])))
    seen, refused, bad = collections.defaultdict(set), set(), []
    for name, case in cases.items():
        plan, launcher = plans[name], tensor.launcher_of(case)
        formula = tensor.plan_of(C, case)
        if {k: str(v) for k, v in formula.items()} != {k: str(plan.get(k)) for k in formula}:
            bad.append((name, "formula", formula, plan))
        if "status" in plan or "status" in case.expect:
            if plan != case.expect:
                bad.append((name, plan, case.expect))
            refused.add((launcher, plan.get("status")))
            continue
        for key, want in case.expect.items():
            if str(plan.get(key)) != str(want):
                bad.append((name, key, plan.get(key), want))
        tensor._note(seen, launcher, plan)
        if plan.get("bound") == "workspace":
            assert launcher == "mttkrp_seg" and plan["nsplit"] == _cdiv(plan["nseg"], _cdiv(plan["nseg"], plan["ws_max"])), (name, plan)
    assert not bad, "\n".join(map(str, bad))
    assert {tensor.launcher_of(c) for c in cases.values()} == {"mttkrp_seg", "partial_last", "partial_mid", "cost"}
    for key, want in tensor.REQUIRED.items():
        if key[0] != "mttkrp_rows":
            assert want <= seen[key], (C, key, want - seen[key])
    # (the refusal of the rows launcher: test_mttkrp_rows_cases_take_the_plans_they_name)
    want = {(l, st) for (l, st) in tensor.REQUIRED_REFUSALS if l != "mttkrp_rows"}
    assert len(want) == len(tensor.REQUIRED_REFUSALS) - 1 and want <= refused, want - refused
    assert {nm for nm in cases if tensor._is_big(nm)} == {"big_seg0_offset_limit"} and "status" not in plans["big_seg0_offset_limit"]
    assert plans["part1_grid_refused"] == {"status": tensor.ERR_UNSUPPORTED}       # enough workspace, too many column blocks


@pytest.mark.parametrize("C", CUS)
def test_gram_and_cost_cases_take_the_plans_they_name(C):
    """Every field a Gram or cost case lists is what the library's plan gives; the rows reach what REQUIRED names for the two
    launchers and column splits of one and of more; a Gram plan bound by the workspace has the splits that workspace holds, and no
    plan carves more than there is."""
    cases = {nm: c for nm, c in plan_cases(C).items() if c.kernel in ("gram", "cost")}
    seen, bad = collections.defaultdict(set), []
    for name, case in cases.items():
        plan = plan_of(C, case)
        assert "status" not in plan, (name, plan)
        assert plan["K" if case.kernel == "gram" else "m"] == case.m and plan["r"] == case.r, (name, plan)
        for key, want in case.expect.items():
            if str(plan.get(key)) != str(want):
                bad.append((name, key, plan.get(key), want))
        note_plan(seen, collections.defaultdict(set), case.kernel, plan)
        ws = WS_DEFAULT if case.ws is None else case.ws
        if case.kernel == "cost":
            seen[("cost", "csplit")].add("1" if plan["csplit"] == 1 else ">1")
            assert plan["partial_bytes"] == 8 * plan["grid"] * plan["csplit"] and plan["vf_bytes"] == 1024 * _cdiv(case.n, 64) * plan["KS"]
            assert 256 * _cdiv(plan["partial_bytes"], 256) + plan["vf_bytes"] <= ws, (name, plan)
        else:
            assert plan["ws_bytes"] == (4 * case.r ** 2 * plan["nsplit"] if plan["form"] in ("slabs", "blocks") else 0) <= ws, (name, plan)
            assert plan["nsplit"] == _cdiv(case.m, plan["kps"]) and plan["kps"] % 64 == 0 or plan["form"] == "small", (name, plan)
            if plan["bound"] == "workspace":
                assert plan["ws_max"] == ws // (4 * case.r ** 2), (name, plan)
                assert plan["nsplit"] == _cdiv(case.m, 64 * _cdiv(_cdiv(case.m, plan["ws_max"]), 64)), (name, plan)
    assert not bad, "\n".join(map(str, bad))
    for key in (("gram", "form"), ("gram", "bound"), ("cost", "NN"), ("cost", "vdb"), ("cost", "VEC")):
        assert REQUIRED[key] <= seen[key], (key, REQUIRED[key] - seen[key])
    assert seen[("cost", "csplit")] == {"1", ">1"}


def ratio_lines(C, case, beta):
    """The passes of one nnf_mu_ratio_f32 call of test_gpu_mu_above_128.ratio_cases as launch_cost_any_rank makes them: rank
    chunks of 128, all but the last writing the model (prod), all but the first reading it back from R1 (pin, at R1's pitch)."""
    return ["cost %d %d %d %d %d %r %d align=%d op=%s pin=%d ldr=%d" % (
        C, case.m, case.n, p["r"], case.x_pitch or case.n, float(beta), WS_DEFAULT, case.x_off, p["op"], p["pin"], case.ldr or case.n)
        for p in above.expected_passes(case, beta)]


@pytest.mark.parametrize("C", CUS)
def test_ratio_cases_take_the_plans_they_name(C):
    """Every pass of every (case, beta) of test_gpu_mu_above_128.ratio_cases -- the rank edges, n = 577 and n = 2200, the layouts --
    takes the load width its layout gives and, in its last pass, the column splits, load group and V buffers the case names; the
    list reaches REQUIRED_RATIO and REQUIRED_COMBOS; the last of the 8 column splits at n = 2200 is empty."""
    calls = [(name, beta) for name, case in above.RATIO_CASES.items() for beta in case.betas]
    lines = [ratio_lines(C, above.RATIO_CASES[name], beta) for name, beta in calls]
    answers = iter(ask([l for ls in lines for l in ls]))
    bad, seen, combos = [], collections.defaultdict(set), set()
    for (name, beta), ls in zip(calls, lines):
        plans = [next(answers) for _ in ls]
        assert all("status" not in p for p in plans), (name, beta, plans)
        above.check_passes(name, beta, plans, bad, seen, combos)
        case = above.RATIO_CASES[name]
        for p in plans:
            assert 1 <= p["csplit"] <= max(1, _cdiv(case.n, 64) // 4) and p["KS"] == _cdiv(p["r"], 4), (name, p)
            assert p["partial_bytes"] == 8 * p["grid"] * p["csplit"] and p["vf_bytes"] == 1024 * _cdiv(case.n, 64) * p["KS"], (name, p)
            assert p["shm"] == 2048 * p["KS"] + (2 if p["vdb"] else 1) * 1024 * p["KS"] + 64 <= 160 * 1024, (name, p)
            if case.n == 2200:      # 35 column blocks in splits of cdiv(35, 8) = 5: seven hold them all
                per = _cdiv(_cdiv(case.n, 64), p["csplit"])
                assert p["csplit"] == 8 and per * (p["csplit"] - 1) >= _cdiv(case.n, 64), (name, p)
            elif p["csplit"] > 1:   # no empty split anywhere else
                assert _cdiv(_cdiv(case.n, 64), p["csplit"]) * (p["csplit"] - 1) < _cdiv(case.n, 64), (name, p)
    assert not bad, "\n".join(map(str, bad))
    above.check_reach(seen, combos)
    named = {nm for nm, c in above.RATIO_CASES.items() if c.expect}
    assert {c.r for nm, c in above.RATIO_CASES.items() if nm in named and c.n == 68} == {1, 4, 5, 9, 50, 64, 100, 120, 128, 129, 131, 200, 256,
                                                                                       257, 385}
    assert {c.n for nm, c in above.RATIO_CASES.items() if nm in named} == {68, 577, 2200}

"""NaN and Inf in the OPERANDS of the kernels, against the fp64 oracle on the same fp32 operands (include/nnfac_hip.h,
"Non-finite operands"; DESIGN.md has the section).  Needs a MI355X, except the three tests at the end of the HALS part (the
case table against the plan header, the expectations against a plain oracle solve, the CPU engine double against the oracle).

Every projection of the reference is np.maximum or np.minimum, and both keep a NaN.  So one NaN in a solve's operands makes that
column of the factor NaN, the sum of squared steps NaN and ends hals_nnls_acc after that sweep (`eps >= delta * eps0` is false);
one NaN in X makes a row of an MU update NaN.  A kernel that takes its maximum with fmaxf / v_max_f32 returns the operand that
is not NaN instead: a clean zero, a finite sum, err = 0.  What is checked, against the oracle evaluated on the poisoned data:
  1. an output column (solve) or row / column (MU) the reference leaves all finite: within the tolerance the kernel's own test
     file derives (test_gpu_hals_plans.error_bound on its sharp Grams, the suite's 2e-4 norm-wise solve tolerance on the
     NMF-like Grams of the stop-rule test; 2e-5 / 1e-3 for MU);
  2. any other column: NaN where the reference is NaN, non-finite where it is non-finite, and an entry the reference leaves
     finite there within tolerance OR NaN -- a kernel may poison a whole column, never return it clean.  The tolerance of such
     an entry is norm-wise, 2e-4 of the larger of the column's finite part and its start values: the entrywise bound of a sharp
     Gram is derived from finite right-hand sides;
  3. status of a solve: cnt the reference's, eps NaN exactly when the reference's is, eps0 within 5e-3 or non-finite of the same
     kind, err 0;   4. blind sweeps: nodelta[s] NaN exactly where the reference's sum is;   5. snapshots: item 2 per block;
  6. costs: NaN when the reference's sum is NaN;   7. products: the set of NaN entries equals the reference's (0 * NaN counts,
     as in numpy), every other entry within tolerance.

HALS.  One case per layout from test_gpu_hals_plans.hals_cases (the smallest the table has), run as a solve with delta = 0.01 and
a budget of 6 on NMF-like data whose clean oracle runs at least 4 sweeps (the seed is searched on the CPU, with 2 % margins
around every stopping decision), and the table's own cross / sweeps / snap / cont / chunks cases on their sharp Grams (delta = 0:
only a NaN ends those early).  Poisons, one at a time: NaN / +Inf / -Inf in one UtM entry, NaN in one start value, NaN in a
symmetric off-diagonal pair of the Gram, NaN on its diagonal, NaN in the second Gram of a cross solve -- at the first and last
row, the first leftover row of an mfma rank, the first and last column, columns 255 and 256 (workgroup and wave edges), and the
last column of a streaming solve (read in a later pass).  Columns are independent once the sweep count is known (no `norm`): the
poisoned column is solved by the oracle on its own, the clean block as in test_gpu_hals_plans; a Gram poison, `norm` or `nz`
couples everything and the oracle solves the whole poisoned block.  Each case first runs the same call unpoisoned on the same engine
(its workspace stays behind) and asserts the reference's clean count -- which differs from the poisoned one for every poison but
-Inf, whose entry the reference clips to 0 like any negative value.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

import nnfac_oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_hals_plans as P  # noqa: E402

NAN, INF = float("nan"), float("inf")
DELTA, BUDGET = 0.01, 6


@pytest.fixture(autouse=True)
def _stop_at_a_device_error(request):
    """Non-finite operands are ordinary data: no test here can make a kernel fault.  Should the device report an error all the
    same, nothing more is started on it."""
    yield
    if "gpu" in request.keywords:
        import torch
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"device error after {request.node.name}: {e}", returncode=3)

# layout key: (case of hals_cases, NNF_HALS_FORCE of the solve, layout the report must name, columns per wave or None)
SOLVE_LAYOUTS = {
    "wave1": ("wave_n257", None, "wave", 1), "wave2": ("wave_ru8_cpw2", None, "wave", 2), "quad": ("quad_n257", "quad", "quad", None),
    "lane": ("lane_n257", "lane", "lane-resident", None), "lane_xy": ("lane_r33_gs", "lane", "lane-resident", None),
    "stream": ("lane_rp8_stream", "lane", "lane-streaming", None), "stream_xy": ("lane_rp40_stream", "lane", "lane-streaming", None),
    "mfma50": ("mfma_rp50", "mfma", "mfma", None), "mfma64": ("mfma_rp64", "mfma", "mfma", None),
    "gen_norm": ("generic_lds_norm_m0", None, "generic-lds", None), "gen_nz": ("generic_lds_nz_m1", None, "generic-lds", None),
    "gen_big_sp": ("generic_big_m1", None, "generic-lds-big", None), "gen_gcol": ("generic_gcol_m1", None, "generic-gcol", None)}
SOLVE_POISONS = ("utm_nan", "utm_nan00", "utm_pinf", "utm_ninf", "vin_nan", "gram_pair", "gram_diag")
# the table's own cases of the other entries (entry, force and layout as listed there) and the poisons each takes
ENTRY_CASES = {
    "wave_cross_gram2": ("utm_nan", "gram2", "vin_nan"), "quad_forced_cross": ("utm_nan", "gram_pair"),
    "quad_cross_gram2": ("gram2", "utm_pinf"), "lane_res_cross_gram2": ("utm_nan", "gram2"), "mfma_cross_gram2": ("utm_nan", "gram2"),
    "generic_lds_cross": ("utm_nan", "gram2"),
    "quad_n257": ("utm_nan", "vin_nan"), "lane_n257": ("utm_nan", "utm_pinf"), "lane_r33_gs": ("utm_nan", "vin_nan", "utm_ninf"),
    "lane_rp8_stream": ("utm_nan", "vin_nan"), "lane_rp40_stream": ("utm_nan", "vin_nan"), "mfma_rp50": ("utm_nan", "vin_nan", "utm_pinf"),
    "mfma_rp64": ("utm_nan", "gram_pair"), "generic_lds_nz_m1": ("utm_nan",), "generic_big_m1": ("utm_nan", "gram_diag"),
    "generic_gcol_m1": ("vin_nan",),
    "quad_snap": ("utm_nan", "utm_pinf"), "lane_snap": ("utm_nan", "utm_pinf"), "mfma_snap": ("utm_nan", "utm_pinf"),
    "quad_cont": ("utm_nan",), "lane_cont": ("utm_nan",), "mfma_cont": ("utm_nan", "vin_nan"),
    "mfma_chunks": ("utm_nan", "utm_pinf", "vin_nan")}
HALS_PARAMS = [(f"solve-{k}-{p}", k, None, p) for k in SOLVE_LAYOUTS for p in SOLVE_POISONS] + \
              [(f"{nm}-{p}", None, nm, p) for nm, ps in ENTRY_CASES.items() for p in ps]

def the_case(C, key, name):
    """(Case, layout, cpw) of a parameter: a layout's case turned into a solve of budget 6, or a case of the table as it is."""
    cases = P.hals_cases(C)
    if key is not None:
        base, force, layout, cpw = SOLVE_LAYOUTS[key]
        c = cases[base]
        return c._replace(entry="solve", budget=BUDGET, force=force, gram2=False), layout, cpw
    c = cases[name]
    return c, c.expect["layout"], c.expect.get("cpw") if c.expect["layout"] == "wave" else None


def poison_of(p, case):
    """(operand, row, column, value).  Rows: the first, the last real one, the first leftover row of mfma's rank 50; columns: the
    first, the last (a later pass of the streaming kernel), 255 and 256."""
    r, n = case.r, case.n
    mid = 48 if (r == 50 and case.force == "mfma") else min(3, r - 1)
    return {"utm_nan": ("UtM", mid, 255, NAN), "utm_nan00": ("UtM", 0, 0, NAN), "utm_pinf": ("UtM", r - 1, 256, INF),
            "utm_ninf": ("UtM", 1, n - 1, -INF), "vin_nan": ("V", r - 1, n - 1, NAN), "gram_pair": ("G", 2, min(6, r - 1), NAN),
            "gram_diag": ("G", r // 2, r // 2, NAN), "gram2": ("G2", 1, 4, NAN)}[p]


# ---------------------------------------------------------------------------------------------------------------------------
# the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def sweeps_of(UtM, G, V0, budget, flags):
    """[V_0 .. V_budget], [nodelta] of hals_nnls_acc in fp64, one sweep at a time."""
    kw = dict(alpha=math.inf, delta=0.0, normalize=flags == "norm", nonzero=flags == "nz")
    if flags == "sp":
        kw["sparsity_coefficient"] = P.SP
    V = V0.astype(np.float64)
    traj, log = [V], []
    with np.errstate(all="ignore"):
        for _ in range(budget):
            V, _, _, _ = orc.hals_nnls_acc(UtM.astype(np.float64), G.astype(np.float64), V, maxiter=1, sweep_log=log, **kw)
            traj.append(V)
    return traj, log


def replay(sums, delta):
    """Sweeps the loop of nnls.py:156 runs when these are the sums of its sweeps (len(sums) = the budget)."""
    for c, s in enumerate(sums, 1):
        if not (s >= delta * sums[0]):
            return c
    return len(sums)


def margins_ok(sums, delta):
    """No stopping decision of a clean solve within 2 % of the threshold (the fp32 sums move a ratio by far less)."""
    c = replay(sums, delta)
    cont = all(s >= 1.02 * delta * sums[0] for s in sums[:c - 1])
    return cont and (c == len(sums) and sums[-1] >= 1.02 * delta * sums[0] or sums[c - 1] <= delta * sums[0] / 1.02)


@functools.lru_cache(maxsize=None)
def clean_problem(key, name):
    """(data, trajectory, sums of the block, per-sweep entrywise bounds or None) of a parameter's unpoisoned problem; a solve's
    data is the first NMF-like seed whose clean oracle runs >= 4 sweeps with margins."""
    case, _, _ = the_case(256, key, name)
    nb = case.n if case.flags in ("norm", "nz") else min(case.n, P.BLOCK)     # (these two couple the columns: no tiling)
    if key is None:
        d = P.case_data(case, 5)
        traj, log = sweeps_of(d["UtM"], d["Gh"], d["V0"], case.budget, case.flags)
        return d, traj, log, (P.error_bound(d, traj, case.flags, case.r) if case.flags != "norm" else None)
    for seed in range(100, 120):
        d = P._nmf_like(case.r, nb, seed)
        traj, log = sweeps_of(d["UtM"], d["Gh"], d["V0"], BUDGET, case.flags)
        if replay(log, DELTA) >= 4 and margins_ok(log, DELTA):
            return d, traj, log, None
    raise AssertionError(f"{key}: no seed whose clean oracle runs 4 sweeps with margins")


def _hadamard(G, G2):
    return G if G2 is None else (G.astype(np.float32) * G2).astype(np.float32)


def expectation(case, d, traj_c, log_c, spec, delta):
    """What the reference makes of the poisoned call: (sweeps run c, sums of all budget sweeps, V after sweep s as a function
    s -> r x n array).  Tiled cases: see the module docstring."""
    what, k, j, val = spec
    r, n, nb, b = case.r, case.n, d["nb"], case.budget
    reps, rem = divmod(n, nb)
    coupled = what in ("G", "G2") or case.flags in ("norm", "nz")   # (nz: the all-zero-row test and np.max(V) see every column)
    if coupled:
        dp = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in d.items()}
        if what in ("G", "G2"):
            dp[what][k, j] = val
            if what == "G" and j != k:
                dp["G"][j, k] = val
            dp["Gh"] = _hadamard(dp["G"], dp["G2"])
        else:
            assert nb == n, "a coupled case is not tiled"
            dp["UtM" if what == "UtM" else "V0"][k, j] = val
        traj, log = sweeps_of(dp["UtM"], dp["Gh"], dp["V0"], b, case.flags)
        sums = [reps * x for x in log]
        if rem:
            _, lr = sweeps_of(dp["UtM"][:, :rem], dp["Gh"], dp["V0"][:, :rem], b, case.flags)
            sums = [x + y for x, y in zip(sums, lr)]
        V_at = lambda s: np.tile(traj[s], (1, reps + 1))[:, :n]   # noqa: E731
    else:
        jb = j % nb
        u, v0 = d["UtM"][:, jb:jb + 1].copy(), d["V0"][:, jb:jb + 1].copy()
        _, log_col_clean = sweeps_of(u, d["Gh"], v0, b, case.flags)
        (u if what == "UtM" else v0)[k, 0] = val
        traj_col, log_col = sweeps_of(u, d["Gh"], v0, b, case.flags)
        sums = [reps * x for x in log_c]
        if rem:
            _, lr = sweeps_of(d["UtM"][:, :rem], d["Gh"], d["V0"][:, :rem], b, case.flags)
            sums = [x + y for x, y in zip(sums, lr)]
        sums = [x - y + z for x, y, z in zip(sums, log_col_clean, log_col)]

        def V_at(s):
            V = np.tile(traj_c[s], (1, reps + 1))[:, :n]
            V[:, j] = traj_col[s][:, 0]
            return V
    c = replay(sums, delta) if case.entry in ("solve", "cross", "cont") else b
    return c, sums, V_at


def clean_sums(case, d, log_c):
    reps, rem = divmod(case.n, d["nb"])
    sums = [reps * x for x in log_c]
    if rem:
        _, lr = sweeps_of(d["UtM"][:, :rem], d["Gh"], d["V0"][:, :rem], case.budget, case.flags)
        sums = [x + y for x, y in zip(sums, lr)]
    return sums


# ---------------------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------------------
def check_columns(what, got, want, bound, scale):
    """Items 1 and 2 on an r x n result.  bound: entrywise (r x n) or None (2e-4 norm-wise over the finite columns);
    scale: per-column magnitude (n) that floors the norm-wise tolerance of a poisoned column."""
    got = got.astype(np.float64)
    fin = np.isfinite(want).all(axis=0)
    g, w = got[:, fin], want[:, fin]
    assert np.isfinite(g).all(), f"{what}: non-finite entries in {int((~np.isfinite(g)).any(axis=0).sum())} columns the reference leaves finite"
    if bound is not None:
        bad = np.abs(g - w) > bound[:, fin]
        assert not bad.any(), f"{what}: {int(bad.sum())} entries of finite columns off their bound, worst {np.abs(g - w).max():.3e}"
    elif w.size:
        e = np.linalg.norm(g - w) / np.linalg.norm(w)
        assert e < 2e-4, f"{what}: finite columns off by {e:.3e}"
    g, w = got[:, ~fin], want[:, ~fin]
    if not w.size:
        return
    isn, nonf = np.isnan(w), ~np.isfinite(w)
    assert np.isnan(g[isn]).all(), f"{what}: {int((~np.isnan(g[isn])).sum())} of {int(isn.sum())} entries are NaN in the reference, not here"
    assert (~np.isfinite(g[nonf])).all(), f"{what}: {int(np.isfinite(g[nonf]).sum())} entries are non-finite in the reference, finite here"
    wf = np.where(nonf, 0.0, w)
    tol = 2e-4 * np.maximum(np.sqrt((wf ** 2).sum(axis=0)), scale[~fin])
    ok = nonf | np.isnan(g) | (np.abs(g - wf) <= tol[None, :])
    assert ok.all(), f"{what}: {int((~ok).sum())} entries the reference leaves finite in a poisoned column are off and not NaN"


def same_kind(a, b):
    """Both NaN, or the same infinity."""
    return (math.isnan(a) and math.isnan(b)) or (math.isinf(a) and a == b)


def check_sum(what, got, want):
    got, want = float(got), float(want)
    if math.isfinite(want):
        assert math.isfinite(got) and abs(got - want) <= 5e-3 * abs(want), (what, got, want)
    else:
        assert same_kind(got, want), (what, got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# the device run
# ---------------------------------------------------------------------------------------------------------------------------
def run(eng, case, t, snaps=None):
    if case.entry == "solve":
        sp = P.SP if case.flags == "sp" else None
        return eng.hals_solve(t["UtM"], t["G"], t["V"], case.budget, delta=DELTA, sparsity=sp, normalize=case.flags == "norm",
                              nonzero=case.flags == "nz"), None
    return P.run_call(eng, case, t, snaps=snaps)


@pytest.mark.gpu
@pytest.mark.parametrize("pid,key,name,poison", HALS_PARAMS, ids=[p[0] for p in HALS_PARAMS])
def test_hals_poisoned(pid, key, name, poison, built_lib, monkeypatch, capfd):
    import torch
    from nn_fac_amd.engine import get_engine
    case, layout, cpw = the_case(P._cus(), key, name)
    if case.force:
        monkeypatch.setenv("NNF_HALS_FORCE", case.force)
    else:
        monkeypatch.delenv("NNF_HALS_FORCE", raising=False)
    monkeypatch.setenv("NNF_HALS_DEBUG", "1")
    eng = get_engine("cuda:0")
    r, n, b = case.r, case.n, case.budget
    delta = DELTA if case.entry == "solve" else 0.0
    d, traj_c, log_c, bounds = clean_problem(key, name)
    spec = poison_of(poison, case)
    c, sums, V_at = expectation(case, d, traj_c, log_c, spec, delta)
    csum = clean_sums(case, d, log_c)
    c_clean = replay(csum, delta) if case.entry in ("solve", "cross", "cont") else b
    snaps = torch.empty(max(b - 1, 1), r, n, device="cuda") if case.entry == "snap" else None
    # ---- the same call unpoisoned, on the same engine, just before ----
    capfd.readouterr()
    st0, nd0 = run(eng, case, P.device_inputs(case, d), snaps=snaps)
    torch.cuda.synchronize()
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[nnf hals]")]
    assert lines and f"-> {layout} " in lines[-1] and (cpw is None or f" cpw={cpw} " in lines[-1]), lines[-1:]
    if st0 is not None:
        s0 = st0.cpu().numpy()
        assert int(s0[1]) == c_clean + 1 and s0[3] == 0.0 and math.isfinite(s0[0]), (pid, s0[:4], c_clean)
    else:
        assert bool(torch.isfinite(nd0).all()), pid
    # ---- poisoned ----
    t = P.device_inputs(case, d)
    what, k, j, val = spec
    target = {"UtM": t["UtM"], "V": t["Vin"] if case.entry == "cross" else t["V"], "G": t["G"], "G2": t["G2"]}[what]
    target[k, j] = val
    if what == "G" and j != k:
        target[j, k] = val
    if snaps is not None:
        snaps.fill_(NAN)
    st, nd = run(eng, case, t, snaps=snaps)
    torch.cuda.synchronize()
    got = t["V"].cpu().numpy()
    reps = -(-n // d["nb"])
    scale = np.tile(np.linalg.norm(d["V0"].astype(np.float64), axis=0), reps)[:n]
    tile = lambda a: np.tile(a, (1, reps))[:, :n]   # noqa: E731
    check_columns(pid, got, V_at(c), tile(bounds[c - 1]) if bounds is not None else None, scale)
    if st is not None:                     # item 3
        s = st.cpu().numpy()
        assert int(s[1]) == c + 1, (pid, "cnt", s[:4], c)
        assert s[3] == 0.0, (pid, "err", s[:4])
        assert math.isnan(s[0]) == math.isnan(sums[c - 1]), (pid, "eps", s[:4], sums[c - 1])
        if math.isfinite(sums[c - 1]):
            check_sum((pid, "eps"), s[0], sums[c - 1])
        check_sum((pid, "eps0"), s[2], sums[0])
        if poison != "utm_ninf":           # (the reference clips a -Inf entry like any negative one: same count as the clean solve)
            assert c != c_clean and int(s[1]) != int(s0[1]), (pid, c, c_clean)
    if nd is not None:                     # item 4
        ndv = nd.cpu().numpy()
        assert len(ndv) == b and (poison == "utm_ninf" or not all(math.isfinite(x) for x in sums)), (pid, sums)
        for s_ in range(b):
            assert math.isnan(ndv[s_]) == math.isnan(sums[s_]), (pid, s_, ndv, sums)
            check_sum((pid, "nodelta", s_), ndv[s_], sums[s_])
    if snaps is not None:                  # item 5: block i holds V after sweep i + 2
        sn = snaps.cpu().numpy()
        for i in range(b - 1):
            check_columns(f"{pid} snapshot {i}", sn[i], V_at(i + 2), tile(bounds[i + 1]), scale)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["utm", "v", "gram_row"])
def test_hals_row_update_poisoned(what, built_lib):
    """The row-sharded piece: NaN in UtM[k], in V and in UtU[k] -- the affected entries of row k are NaN, both sums are NaN."""
    import torch
    from nn_fac_amd.engine import get_engine
    eng = get_engine("cuda:0")
    r, n, k = 20, 700, 7
    d = P._nmf_like(r, n, 3)
    UtM, G, V = (d[x].astype(np.float64) for x in ("UtM", "G", "V0"))
    if what == "utm":
        UtM[k, 256] = NAN
    elif what == "v":
        V[3, 699] = NAN            # another row of the column: reaches row k through the dot product
    else:
        G[k, 5] = NAN              # the whole row
    with np.errstate(all="ignore"):
        step = np.maximum((UtM[k] - G[k] @ V) / G[k, k], -V[k])
    want = V.copy()
    want[k] += step
    dev = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()   # noqa: E731
    Vd = dev(V)
    out2 = eng.hals_row_update(dev(UtM), dev(G), Vd, k).cpu().numpy()
    assert np.isnan(out2).all(), out2
    got = Vd.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (int(np.isnan(got).sum()), int(np.isnan(want).sum()))
    f = np.isfinite(want)
    assert np.abs(got[f] - want[f]).max() <= 2e-4 * np.linalg.norm(want[k][np.isfinite(want[k])])


# ---- no GPU: the table, the expectations, the engine double ----
def test_case_table():
    """Every parameter names a case of hals_cases, the plan header (tools/nnf_plan.cpp) gives each the layout it is listed with,
    the poisoned entries exist, and a solve's clean oracle runs at least 4 of its 6 sweeps and not the poisoned count."""
    cases = {pid: the_case(256, key, name) for pid, key, name, _ in HALS_PARAMS}
    plans = P.hals_tool_plans(256, {pid: c[0] for pid, c in cases.items()})
    for pid, key, name, poison in HALS_PARAMS:
        case, layout, cpw = cases[pid]
        kv = plans[pid]
        assert kv["layout"] == layout and kv["err"] == "0" and (cpw is None or kv["cpw"] == str(cpw)), (pid, kv)
        what, k, j, _ = poison_of(poison, case)
        assert 0 <= k < case.r and 0 <= j < (case.n if what in ("UtM", "V") else case.r), (pid, what, k, j)
        assert what != "G2" or case.gram2, pid
    assert {c[1] for c in cases.values()} == {"wave", "quad", "mfma", "lane-resident", "lane-streaming", "generic-lds",
                                              "generic-lds-big", "generic-gcol"}
    for key in ("wave1", "lane", "gen_nz"):            # (the other layouts' data is made the same way, at the GPU tests' cost)
        _, _, log, _ = clean_problem(key, None)
        assert 4 <= replay(log, DELTA) <= BUDGET and margins_ok(log, DELTA), (key, log)


def _full_solve(UtM, G, V0, budget, delta, flags=""):
    kw = dict(alpha=math.inf, delta=delta, maxiter=budget, normalize=flags == "norm", nonzero=flags == "nz")
    with np.errstate(all="ignore"):
        return orc.hals_nnls_acc(UtM.astype(np.float64), G.astype(np.float64), V0.astype(np.float64), **kw)


ORACLE_POISONS = [("UtM", 3, 5, NAN), ("V", 6, 5, NAN), ("G", 2, 6, NAN), ("UtM", 3, 5, INF), ("UtM", 3, 5, -INF), ("G", 4, 4, NAN)]


@pytest.mark.parametrize("spec", ORACLE_POISONS, ids=lambda s: f"{s[0]}{s[1]}_{s[2]}_{s[3]}")
def test_expectations_are_the_oracle(spec):
    """expectation() -- one column on its own, the clean block, the replayed stopping rule -- against hals_nnls_acc on the whole
    poisoned problem (r = 8, 12 columns tiled to 30, delta = 0.01, budget 20), and the reference's behaviour itself: a NaN ends
    the solve after that sweep (cnt = 2, eps NaN) with NaN from the poisoned row down, a NaN start value takes the whole column,
    a NaN Gram pair every column from row 2 down, +Inf ends it one sweep later, -Inf is clipped to 0 and changes nothing else."""
    r, nb, n, b = 8, 12, 30, 20
    d = P._nmf_like(r, nb, 11)
    case = P.Case("solve", r, n, {}, "", None, False, b, {}, {})
    traj_c, log_c = sweeps_of(d["UtM"], d["Gh"], d["V0"], b, "")
    c, sums, V_at = expectation(case, d, traj_c, log_c, spec, DELTA)
    what, k, j, val = spec
    full = {x: np.tile(d[x], (1, 3))[:, :n].copy() for x in ("UtM", "V0")}
    G = d["G"].copy()
    if what == "G":
        G[k, j] = G[j, k] = val
    else:
        full["UtM" if what == "UtM" else "V0"][k, j] = val
    V, eps, cnt, _ = _full_solve(full["UtM"], G, full["V0"], b, DELTA)
    assert cnt == c + 1 and (math.isnan(eps) == math.isnan(sums[c - 1])), (cnt, c, eps, sums[:c])
    np.testing.assert_array_equal(np.isnan(V), np.isnan(V_at(c)))
    f = np.isfinite(V)
    np.testing.assert_allclose(V_at(c)[f], V[f], rtol=1e-12, atol=1e-300)
    c_clean = replay(clean_sums(case, d, log_c), DELTA)
    assert c_clean >= 4
    if val != -INF:
        assert c == (2 if val == INF else 1) and math.isnan(eps)
    else:
        assert c == c_clean and np.isfinite(V).all() and V[k, j] == 0.0
    if what == "UtM" and math.isnan(val):
        assert np.isnan(V[k:, j]).all() and np.isfinite(V[:k, j]).all() and np.isfinite(np.delete(V, j, axis=1)).all()
        one, _, _, _ = _full_solve(np.delete(full["UtM"], j, axis=1), G, np.delete(full["V0"], j, axis=1), 1, 0.0)
        np.testing.assert_allclose(np.delete(V, j, axis=1), one, rtol=1e-12)   # the other columns: the one-sweep result
    if what == "V":
        assert np.isnan(V[:, j]).all() and np.isfinite(np.delete(V, j, axis=1)).all()
    if what == "G" and k != j:
        assert np.isnan(V[min(k, j):]).all() and np.isfinite(V[:min(k, j)]).all()


@pytest.mark.parametrize("spec", ORACLE_POISONS[:5], ids=lambda s: f"{s[0]}{s[1]}_{s[2]}_{s[3]}")
def test_engine_double_matches_the_oracle(spec):
    """tests/engine_double.py (the engine of test_dist_gloo.py) on the poisoned solves: its persistent solve, its blind sweeps +
    hals_stop_restore (the row-sharded protocol: the stopping rule replayed over the sums) and its row update give what
    hals_nnls_acc gives -- NaN pattern, count and the NaN-ness of eps."""
    import torch
    from engine_double import OracleEngine
    r, n, b = 8, 12, 20
    d = P._nmf_like(r, n, 11)
    what, k, j, val = spec
    UtM, G, V0 = (d[x].astype(np.float64) for x in ("UtM", "G", "V0"))
    if what == "G":
        G[k, j] = G[j, k] = val
    else:
        (UtM if what == "UtM" else V0)[k, j] = val
    want, eps, cnt, _ = _full_solve(UtM, G, V0, b, DELTA)
    eng = OracleEngine()
    tt = lambda a: torch.from_numpy(a.copy())   # noqa: E731
    with np.errstate(all="ignore"):
        V = tt(V0)
        st = eng.hals_solve(tt(UtM), tt(G), V, b, delta=DELTA)
        np.testing.assert_array_equal(V.numpy(), want)
        assert int(st[1]) == cnt and math.isnan(float(st[0])) == math.isnan(eps) and float(st[3]) == 0.0
        # blind sweeps with a snapshot of every sweep, then the replay
        V = tt(V0)
        snaps = torch.full((b, r, n), NAN, dtype=torch.float64)
        sums = eng.hals_sweeps(tt(UtM), tt(G), V, b, snapshots=snaps, snap_first=0)
        st = torch.zeros(8, dtype=torch.float64)
        eng.hals_stop_restore(sums, 0, b, DELTA, V, snaps, st)
        np.testing.assert_array_equal(V.numpy(), want)
        assert int(st[1]) == cnt and math.isnan(float(st[0])) == math.isnan(eps) and float(st[3]) == 0.0
        # one sweep, row by row
        V = tt(V0)
        nd = 0.0
        for row in range(r):
            nd += float(eng.hals_row_update(tt(UtM), tt(G), V, row)[0])
        one, e1, _, _ = _full_solve(UtM, G, V0, 1, 0.0)
    np.testing.assert_array_equal(np.isnan(V.numpy()), np.isnan(one))
    f = np.isfinite(one)
    np.testing.assert_allclose(V.numpy()[f], one[f], rtol=1e-12)
    assert math.isnan(nd) == math.isnan(e1) and (math.isnan(nd) or same_kind(nd, e1) or abs(nd - e1) <= 1e-9 * e1)


# ---------------------------------------------------------------------------------------------------------------------------
# MU: one row of the left update, one column of the right update
# ---------------------------------------------------------------------------------------------------------------------------
MU_RANKS = (20, 50, 100, 130)             # <= 32, 33-64, 65-128 (fused), 130 (the ratio path)
MU_BETAS = (0, 0.5, 1, 2, 3)
MU_POISONS = {"x_nan": ("X", 17, 23, NAN), "v_nan": ("V", 2, 23, NAN), "u_nan": ("U", 5, 2, NAN), "x_inf": ("X", 17, 23, INF)}


def mu_problem(m, n, r, seed):
    rng = np.random.RandomState(seed)
    U, V = rng.rand(m, r) + 0.05, rng.rand(r, n) + 0.05
    X = rng.rand(m, r) @ rng.rand(r, n) + 0.05
    return tuple(a.astype(np.float32).astype(np.float64) for a in (X, U, V))


def check_lines(what, got, want, glob=2e-5, ent=1e-3):
    """Items 1 and 2 on the COLUMNS of got / want (pass transposes for rows); finite lines: the MU files' rel 2e-5, worst 1e-3."""
    got = np.asarray(got, dtype=np.float64)
    fin = np.isfinite(want).all(axis=0)
    g, w = got[:, fin], want[:, fin]
    assert np.isfinite(g).all(), f"{what}: non-finite where the reference is finite"
    if w.size:
        assert np.linalg.norm(g - w) <= glob * np.linalg.norm(w) and (np.abs(g - w) <= ent * np.abs(w)).all(), what
    g, w = got[:, ~fin], want[:, ~fin]
    assert np.isnan(g[np.isnan(w)]).all(), f"{what}: a NaN of the reference is not NaN here"
    assert (~np.isfinite(g[~np.isfinite(w)])).all(), f"{what}: a non-finite entry of the reference is finite here"
    f = np.isfinite(w)
    assert (np.isnan(g[f]) | (np.abs(g[f] - w[f]) <= ent * np.abs(w[f]))).all(), f"{what}: finite entries of a poisoned line off"
    assert (~fin).any(), f"{what}: the reference has no poisoned line -- the case checks nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("poison", list(MU_POISONS))
@pytest.mark.parametrize("beta", MU_BETAS)
@pytest.mark.parametrize("r", MU_RANKS)
def test_mu_updates_poisoned(r, beta, poison, built_lib):
    """mu_left, mu_right, mu_right_accum + mu_apply (and mu_left with cost_out at beta = 1, r <= 64) on a ragged 70 x 90 problem
    behind NaN-padded rows, against mu_betadivmin / switch_alternate_mu on the poisoned operands."""
    import torch
    from nn_fac_amd.engine import get_engine
    from test_gpu_mu_rank128 import padded
    eng = get_engine("cuda:0")
    m, n = 70, 90
    X, U, V = mu_problem(m, n, r, 100 * r + int(10 * beta))
    what, i, j, val = MU_POISONS[poison]
    {"X": X, "U": U, "V": V}[what][i, j] = val
    with np.errstate(all="ignore"):
        want_l = orc.mu_betadivmin(U, V, X, beta)                         # m x r
        want_r = orc.switch_alternate_mu(X, U, V, beta, "V")              # r x n
    Xd, Utd, Vd = padded(X, 5), padded(U.T.copy(), 5), padded(V, 7)
    tag = (r, beta, poison)
    check_lines(("left", tag), eng.mu_left(Xd, Utd, Vd, beta).cpu().numpy(), want_l.T)          # columns of Ut_new = rows of U
    check_lines(("right", tag), eng.mu_right(Xd, Utd, Vd, beta).cpu().numpy(), want_r)
    num, den, dvec = eng.mu_right_accum(Xd, Utd, Vd, beta)
    check_lines(("accum + apply", tag), eng.mu_apply(Vd, num, den, dvec, beta).cpu().numpy(), want_r)
    if beta == 1 and r <= 64:
        cost = torch.zeros(1, dtype=torch.float64, device="cuda")
        out = eng.mu_left(Xd, Utd, Vd, 1, cost_out=cost)
        check_lines(("left + cost", tag), out.cpu().numpy(), want_l.T)
        assert math.isnan(float(cost)), (tag, float(cost))


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["t_nan", "v_nan", "t_inf"])
@pytest.mark.parametrize("beta", MU_BETAS)
@pytest.mark.parametrize("r", (20, 50))
def test_mu_mode_poisoned(r, beta, poison, built_lib):
    """The mode update on the tensor's own layout (r <= 64): one row of the factor for a poisoned tensor entry."""
    import torch
    from nn_fac_amd.engine import get_engine
    from test_gpu_mu_rank128 import dev, padded
    eng = get_engine("cuda:0")
    L, I, K = 5, 23, 18
    rng = np.random.RandomState(r + int(10 * beta))
    F, V = rng.rand(I, r) + 0.05, rng.rand(r, L * K) + 0.05
    M = rng.rand(I, r) @ rng.rand(r, L * K) + 0.05
    T, F, V = (a.astype(np.float32).astype(np.float64) for a in (np.ascontiguousarray(M.reshape(I, L, K).transpose(1, 0, 2)), F, V))
    if poison == "v_nan":
        V[2, 31] = NAN
    else:
        T[3, 17, 11] = NAN if poison == "t_nan" else INF
    with np.errstate(all="ignore"):
        want = orc.mu_betadivmin(F, V, np.moveaxis(T, 1, 0).reshape(I, L * K), beta)      # I x r
    got = eng.mu_mode(dev(T), padded(F.T.copy(), 5), padded(V, 6), beta)
    check_lines(("mu_mode", r, beta, poison), got.cpu().numpy(), want.T)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["num_nan", "f_nan", "num_inf", "wh_nan", "hsum_nan"])
def test_deep_kl_apply_poisoned(poison, built_lib):
    """deep_KL_mu's element-wise tail (deep_mu.py:8-14): NaN where lambertw and np.maximum leave one.  b = F .* num = +Inf gives
    inf / (lambertw(inf) + eps) = NaN in the reference."""
    import torch
    from scipy.special import lambertw
    from nn_fac_amd.engine import get_engine
    from test_gpu_mu_rank128 import padded
    eng = get_engine("cuda:0")
    r, cols, lam = 7, 300, 0.7
    rng = np.random.RandomState(4)
    F, num, WH = (rng.rand(r, cols).astype(np.float32).astype(np.float64) + 0.05 for _ in range(3))
    hsum = rng.rand(r) * 3 + 1
    if poison == "hsum_nan":
        hsum[4] = NAN
    else:
        {"num_nan": num, "f_nan": F, "num_inf": num, "wh_nan": WH}[poison][4, 257] = INF if poison == "num_inf" else NAN
    F, num, WH = (a.astype(np.float32).astype(np.float64) for a in (F, num, WH))
    with np.errstate(all="ignore"):
        b = F * num
        a = hsum[:, None] - lam * np.log(WH)
        want = np.maximum(1e-12, (b / lam) / (lambertw(b * np.exp(a / lam) / lam, k=0).real + 1e-12))
    assert np.isnan(want).any()
    got = eng.deep_kl_apply(padded(F, 3), padded(num, 1), torch.from_numpy(hsum).cuda(), padded(WH, 2), lam).cpu().numpy().astype(np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    f = np.isfinite(want)
    assert np.isfinite(got[f]).all() and (np.abs(got[f] - want[f]) <= 1e-5 * np.abs(want[f])).all()


# ---------------------------------------------------------------------------------------------------------------------------
# NTD core: np.minimum keeps the NaN, the first update norm is NaN, the loop ends after one step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["mtx_nan", "gram_nan"])
@pytest.mark.parametrize("dims,max_iter", [((4, 3, 2), 300), ((2, 64, 64), 25)], ids=["lds64", "ws"])
@pytest.mark.parametrize("entry", ["pg", "pgn"])
def test_ntd_core_poisoned(entry, dims, max_iter, poison, built_lib):
    """ntd.py:588-619 with a NaN in MtX (one entry of the first step, then -- through the mode products -- all of them; the loop
    ends after step 1 because upd is NaN) and in a Gram (np.linalg.svd of a matrix with a NaN does not converge: the reference
    raises; the power iteration here gives a NaN step, and the contract's "never clean" asks for a NaN core and a NaN upd)."""
    import torch
    from nn_fac_amd.engine import get_engine
    from test_gpu_ntd import _pg_reference
    eng = get_engine("cuda:0")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()   # noqa: E731
    rng = np.random.RandomState(sum(dims))
    shape = tuple(5 * d + 3 for d in dims)
    Fs = [0.1 * rng.rand(shape[i], dims[i]) for i in range(3)]
    T = orc.multi_mode_dot(rng.rand(*dims), Fs) + 0.01 * rng.rand(*shape)
    MtX = orc.multi_mode_dot(T, Fs, transpose=True).astype(np.float32).astype(np.float64)
    M = [(f.T @ f).astype(np.float32).astype(np.float64) for f in Fs]
    core0 = rng.rand(*dims).astype(np.float32).astype(np.float64)
    nrm2 = float(np.sum(T ** 2))
    call = eng.ntd_core_pg if entry == "pg" else eng.ntd_core_pgn
    clean = dev(core0)
    st_clean = call(clean, dev(MtX), [dev(m_) for m_ in M], 0.0, 0.01, max_iter, nrm2).cpu().numpy()
    assert int(st_clean[0]) > 1 and math.isfinite(st_clean[1]) and bool(torch.isfinite(clean).all())
    if poison == "mtx_nan":
        MtX[dims[0] - 1, 1, dims[2] - 1] = NAN
        with np.errstate(all="ignore"):
            want, iters, step = _pg_reference(core0, MtX, M, 0.0, 0.01, max_iter)
        assert iters == 1 and np.isnan(want).sum() == 1          # (the reference stops before the NaN spreads)
    else:
        M[1][0, dims[1] - 1] = M[1][dims[1] - 1, 0] = NAN
        want, iters = np.full(dims, NAN), 1       # np.minimum(NaN * gradient, core) in every entry, upd NaN: one step
    cd = dev(core0)
    st = call(cd, dev(MtX), [dev(m_) for m_ in M], 0.0, 0.01, max_iter, nrm2).cpu().numpy()
    got = cd.cpu().numpy().astype(np.float64)
    assert int(st[0]) == iters and math.isnan(st[1]) and st[5] == 0.0, st
    assert np.isnan(got[np.isnan(want)]).all()
    f = np.isfinite(want)
    assert (np.isnan(got[f]) | (np.abs(got[f] - want[f]) <= 1e-5 * np.linalg.norm(want[f]))).all()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))       # mtx_nan: that one entry; gram_nan: the whole core


# ---------------------------------------------------------------------------------------------------------------------------
# costs and products
# ---------------------------------------------------------------------------------------------------------------------------
def _first_of_each_form(kernel):
    """One case of test_gpu_launch_plans.plan_cases per launch plan family (`form`) of a kernel, default workspace, no refusal."""
    import test_gpu_launch_plans as L
    seen, out = set(), []
    for name, c in L.plan_cases(256).items():
        form = c.expect.get("form")
        if c.kernel == kernel and c.ws is None and c.expect.get("err") is None and form not in seen:
            seen.add(form)
            out.append(name)
    return out


PRODUCT_CASES = [(k, nm) for k in ("xht", "xty", "gram") for nm in _first_of_each_form(k)]
PRODUCT_SPOTS = ("interior", "last_col", "last_row", "factor")


def _nan_set(a_rows, b_cols):
    """NaN entries of A @ B for otherwise finite operands: the rows of A and the columns of B that hold a NaN (0 * NaN is NaN)."""
    return a_rows[:, None] | b_cols[None, :]


@pytest.mark.gpu
@pytest.mark.parametrize("spot", PRODUCT_SPOTS)
@pytest.mark.parametrize("kernel,name", PRODUCT_CASES, ids=[c[1] for c in PRODUCT_CASES])
def test_streaming_products_poisoned(kernel, name, spot, built_lib):
    """V X^T, U^T X and A A^T on one shape per launch plan family: the NaN entries are exactly the reference's (a whole output
    column for an entry of X, a whole row for a factor entry; a Gram's row and column), every other entry is the clean product's.
    The fused entries (xht_gram, xty_gram) on the same operands: the same bits in both outputs."""
    import torch
    import test_gpu_launch_plans as L
    case = L.plan_cases(L._cus())[name]
    eng = L.engine_for(case)
    inp = L.make_inputs(case, 7)
    r = case.r
    if kernel == "gram":
        A = inp["A"]
        want = A.double() @ A.double().t()
        k, j = {"interior": (r // 2, case.m // 2), "last_col": (1, case.m - 1), "last_row": (r - 1, 3), "factor": (r - 1, case.m - 1)}[spot]
        A[k, j] = NAN
        rows = torch.zeros(r, dtype=torch.bool, device="cuda")
        rows[k] = True
        nan = rows[:, None] | rows[None, :]
        got = eng.gram(A)
    else:
        X, F = inp["X"], inp["V" if kernel == "xht" else "Ut"]       # xht: F (r x n) X^T (n x m);  xty: F (r x m) X (m x n)
        want = F.double() @ (X.double().t() if kernel == "xht" else X.double())
        m, n = X.shape
        rows = torch.zeros(r, dtype=torch.bool, device="cuda")
        cols = torch.zeros(want.shape[1], dtype=torch.bool, device="cuda")
        if spot == "factor":
            F[r - 1, F.shape[1] - 1] = NAN           # the last real rank row (ranks 33, 50, 96, 100: padded rank tiles)
            rows[r - 1] = True
        else:
            i, j = {"interior": (m // 2, n // 2), "last_col": (m // 3, n - 1), "last_row": (m - 1, 1)}[spot]
            X[i, j] = NAN
            cols[i if kernel == "xht" else j] = True
        nan = _nan_set(rows, cols)
        got = eng.xht(X, F) if kernel == "xht" else eng.xty(X, F)
        fused, G = (eng.xht_gram(X, F) if kernel == "xht" else eng.xty_gram(X, F))
        assert torch.equal(fused.view(torch.int32), got.view(torch.int32)), (name, spot, "fused product")
        Gw = eng.gram(F)
        assert torch.equal(G.view(torch.int32), Gw.view(torch.int32)), (name, spot, "fused Gram")
        assert bool(torch.isnan(G).any()) == (spot == "factor")     # a NaN in the small factor reaches BOTH outputs
    assert torch.equal(torch.isnan(got), nan), (name, spot, int(torch.isnan(got).sum()), int(nan.sum()))
    L.assert_close(got[~nan], want[~nan], 1e-5, 1e-4, (name, spot))


def _small(m, n, r, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(m, n, device="cuda", generator=g) + 0.05, torch.rand(r, m, device="cuda", generator=g) + 0.05,
            torch.rand(r, n, device="cuda", generator=g) + 0.05)


@pytest.mark.gpu
@pytest.mark.parametrize("r", (33, 100))
@pytest.mark.parametrize("spot", PRODUCT_SPOTS)
def test_small_products_poisoned(r, spot, built_lib):
    """small_gemm, mu_left_num, mu_right_accum, ttm3, mttkrp3 and mttkrp3_from_partial at ranks 33 and 100 (padded rank tiles):
    NaN set equal to the reference's, entry for entry."""
    import torch
    from nn_fac_amd.engine import get_engine
    eng = get_engine("cuda:0")
    m, n = 150, 203
    X, Ut, V = _small(m, n, r, r)
    # ---- small_gemm: A (r x m) @ X (m x n)
    A, B = Ut.clone(), X.clone()
    rows, cols = torch.zeros(r, dtype=torch.bool, device="cuda"), torch.zeros(n, dtype=torch.bool, device="cuda")
    if spot == "factor":
        A[r - 1, m - 1] = NAN
        rows[r - 1] = True
    else:
        i, j = {"interior": (m // 2, n // 2), "last_col": (m // 3, n - 1), "last_row": (m - 1, 1)}[spot]
        B[i, j] = NAN
        cols[j] = True
    want = A.double().nan_to_num(0.0) @ B.double().nan_to_num(0.0)
    got = eng.small_gemm(A, B)
    nan = _nan_set(rows, cols)
    assert torch.equal(torch.isnan(got), nan), ("small_gemm", spot)
    assert float(((got.double() - want)[~nan].abs() / want[~nan]).max()) <= 1e-4
    # ---- the KL numerator of the left update and the accumulate-only right update (beta = 1): X / (U V)
    Xp, Utp, Vp = X.clone(), Ut.clone(), V.clone()
    if spot == "factor":
        Vp[r - 1, n - 1] = NAN        # K[:, n-1] is NaN: every row of the left numerator, column n-1 of the right one
        nan_l = torch.ones(r, m, dtype=torch.bool, device="cuda")
        nan_r = _nan_set(torch.zeros(r, dtype=torch.bool, device="cuda"), torch.arange(n, device="cuda") == n - 1)
    else:
        Xp[i, j] = NAN
        nan_l = _nan_set(torch.zeros(r, dtype=torch.bool, device="cuda"), torch.arange(m, device="cuda") == i)
        nan_r = _nan_set(torch.zeros(r, dtype=torch.bool, device="cuda"), torch.arange(n, device="cuda") == j)
    K = Ut.double().t() @ V.double()
    if r <= 64:                                           # (nnf_mu_left_num_f32 is built up to rank 64)
        got = eng.mu_left_num(Xp, Utp, Vp)
        assert torch.equal(torch.isnan(got), nan_l), ("mu_left_num", spot, int(torch.isnan(got).sum()), int(nan_l.sum()))
        want = V.double() @ (X.double() / K).t()
        if (~nan_l).any():
            assert float(((got.double() - want)[~nan_l].abs() / want[~nan_l]).max()) <= 1e-3
    num, _, dvec = eng.mu_right_accum(Xp, Utp, Vp, 1)
    assert torch.equal(torch.isnan(num), nan_r) and bool(torch.isfinite(dvec).all()), ("mu_right_accum", spot)
    want = Ut.double() @ (X.double() / K)
    assert float(((num.double() - want)[~nan_r].abs() / want[~nan_r]).max()) <= 1e-3
    # ---- tensor products: a NaN in T[i0, j0, k0] / in the last real rank row of a factor
    I, J, Kk = 9, 37, 41
    g = torch.Generator(device="cuda").manual_seed(5)
    T = torch.rand(I, J, Kk, device="cuda", generator=g)
    Ft = [torch.rand(r, d_, device="cuda", generator=g) + 0.05 for d_ in (I, J, Kk)]
    pos = {"interior": (4, 18, 20), "last_col": (2, 5, Kk - 1), "last_row": (I - 1, J - 1, 0)}.get(spot)
    if pos:
        T[pos] = NAN
    else:
        Ft[2][r - 1, Kk - 1] = NAN
    T64, F64 = T.double().cpu().numpy(), [f.double().cpu().numpy() for f in Ft]
    ones_r = torch.ones(r, dtype=torch.bool, device="cuda")
    with np.errstate(all="ignore"):
        for mode in range(3):
            a, b_ = [x for x in range(3) if x != mode]
            want = np.einsum("ijk,r%s,r%s->r%s" % ("ijk"[a], "ijk"[b_], "ijk"[mode]), T64, F64[a], F64[b_])
            if pos:                                           # T[pos]: entry pos[mode] of every rank row
                exp = _nan_set(~ones_r, torch.arange(T.shape[mode], device="cuda") == pos[mode])
            elif mode == 2:                                   # Ft[2] is not an operand of mode 2
                exp = torch.zeros(r, T.shape[2], dtype=torch.bool, device="cuda")
            else:                                             # Ft[2][r-1, K-1]: rank row r-1, every entry
                exp = _nan_set(torch.arange(r, device="cuda") == r - 1, torch.zeros(T.shape[mode], dtype=torch.bool, device="cuda"))
            assert np.array_equal(np.isnan(want), exp.cpu().numpy()), ("reference NaN set", mode, spot)
            got = eng.mttkrp3(T, Ft, mode)
            assert torch.equal(torch.isnan(got), exp), ("mttkrp3", mode, spot, int(torch.isnan(got).sum()), int(exp.sum()))
            g, ok = got.double().cpu().numpy(), ~np.isnan(want)
            assert (np.abs(g - want)[ok] <= 1e-4 * np.abs(want[ok])).all(), ("mttkrp3", mode, spot)
            want = np.einsum("ijk,r%s->%s" % ("ijk"[mode], ("rjk", "irk", "rij")[mode]), T64, F64[mode])     # (mode 2: r x I x J)
            got = eng.ttm3(T, Ft[mode], mode).double().cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)), ("ttm3", mode, spot)
            ok = ~np.isnan(want)
            assert (np.abs(got - want)[ok] <= 1e-4 * np.abs(want[ok])).all(), ("ttm3", mode, spot)
        Y = eng.ttm3(T, Ft[2], 2)                                         # R x I x J: the partial MTTKRP's operand
        Y64 = Y.double().cpu().numpy()
        for axis, f in ((1, Ft[0]), (2, Ft[1])):
            want = np.einsum("rab,ra->rb" if axis == 1 else "rab,rb->ra", Y64, f.double().cpu().numpy())
            got = eng.mttkrp3_from_partial(Y, f, axis).double().cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)), ("mttkrp3_from_partial", axis, spot)
            ok = ~np.isnan(want)
            assert (np.abs(got - want)[ok] <= 1e-4 * np.abs(want[ok])).all(), ("mttkrp3_from_partial", axis, spot)


@pytest.mark.gpu
@pytest.mark.parametrize("spot", PRODUCT_SPOTS)
def test_costs_poisoned(spot, built_lib):
    """frob_resid, betadiv (every beta), frob_resid_rows, gram_cost, cp3_betadiv and cp3_partial_cost: NaN when the reference's sum
    is NaN; frob_resid_rows NaN in exactly the affected rows."""
    import torch
    from nn_fac_amd.engine import get_engine
    eng = get_engine("cuda:0")
    for r in (33, 100):
        m, n = 150, 203
        X, Ut, V = _small(m, n, r, 7 * r)
        rows = torch.zeros(m, dtype=torch.bool, device="cuda")
        if spot == "factor":
            Ut[r - 1, m - 1] = NAN
            rows[m - 1] = True
        else:
            i, j = {"interior": (m // 2, n // 2), "last_col": (m // 3, n - 1), "last_row": (m - 1, 1)}[spot]
            X[i, j] = NAN
            rows[i] = True
        assert math.isnan(float(eng.frob_resid(X, Ut, V))), ("frob_resid", r, spot)
        for beta in MU_BETAS:
            assert math.isnan(float(eng.betadiv(X, Ut, V, beta))), ("betadiv", r, beta, spot)
        got = eng.frob_resid_rows(X, Ut, V)
        assert torch.equal(torch.isnan(got), rows), ("frob_resid_rows", r, spot, int(torch.isnan(got).sum()))
        want = ((X.double() - Ut.double().t() @ V.double()) ** 2).sum(dim=1)
        assert float(((got - want)[~rows].abs() / want[~rows]).max()) <= 1e-4
        # the Gram identity: ||X||^2 - 2 <V, UtM> + <V, UtU V>
        UtM, UtU = eng.xty(X, Ut), eng.gram(Ut)
        out = torch.zeros(3, dtype=torch.float64, device="cuda")
        normx2 = (X.double() ** 2).sum().reshape(1)
        eng.gram_cost(V, UtM, UtU, normx2, out)
        o = out.cpu().numpy()
        assert math.isnan(o[0]) and o[1] == 1.0, ("gram_cost", r, spot, o)
    I, J, K, R = 9, 37, 41, 20
    g = torch.Generator(device="cuda").manual_seed(3)
    T = torch.rand(I, J, K, device="cuda", generator=g) + 0.05
    Ft = [torch.rand(R, d_, device="cuda", generator=g) + 0.05 for d_ in (I, J, K)]
    pos = {"interior": (4, 18, 20), "last_col": (2, 5, K - 1), "last_row": (I - 1, J - 1, 0)}.get(spot)
    if pos:
        T[pos] = NAN
    else:
        Ft[1][R - 1, J - 1] = NAN
    for beta in (1, 2, 0.5):
        assert math.isnan(float(eng.cp3_betadiv(T, Ft, beta))), ("cp3_betadiv", beta, spot)
    cost = torch.zeros(1, dtype=torch.float64, device="cuda")
    Y = torch.empty(R, I, J, device="cuda")
    eng.cp3_partial_cost(T, Ft, Y, cost)
    assert math.isnan(float(cost)), ("cp3_partial_cost", spot)
    wantY = torch.einsum("ijk,rk->rij", T.double(), Ft[2].double())
    assert torch.equal(torch.isnan(Y), torch.isnan(wantY)), ("cp3_partial_cost Y", spot)


@pytest.mark.gpu
@pytest.mark.parametrize("spot", PRODUCT_SPOTS)
@pytest.mark.parametrize("name", _first_of_each_form("cost") + _first_of_each_form("cp3_partial_cost"))
def test_cost_plans_poisoned(name, spot, built_lib):
    """The cost pass on the launch-plan table's shapes (column splits, load widths): a NaN at an interior entry, in the last
    valid column of a row, in the last row, and in a factor entry of the last rank row."""
    import torch
    import test_gpu_launch_plans as L
    case = L.plan_cases(L._cus())[name]
    eng = L.engine_for(case)
    inp = L.make_inputs(case, 7)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    if case.kernel == "cost":
        m, n = case.m, case.n
        if spot == "factor":
            inp["Ut"][case.r - 1, m - 1] = NAN
        else:
            inp["X"][{"interior": (m // 2, n // 2), "last_col": (m // 3, n - 1), "last_row": (m - 1, 1)}[spot]] = NAN
        got = float(L.run_case(eng, case, inp, out=out))
    else:
        T = inp["T"]
        I, J, K = T.shape
        if spot == "factor":
            inp["Ft"][1][case.r - 1, J - 1] = NAN
        else:
            T[{"interior": (I // 2, J // 2, K // 2), "last_col": (I // 3, 1, K - 1), "last_row": (I - 1, J - 1, 0)}[spot]] = NAN
        L.run_case(eng, case, inp, cost_out=out)
        got = float(out)
    assert math.isnan(got), (name, spot, got)


# ---------------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rule,beta", [("hals", 2), ("mu", 1), ("mu", 2)])
def test_nmf_with_a_nan_in_x(rule, beta, built_lib):
    """nmf() on 60 x 50, rank 4, X[17, 23] = NaN, three iterations: the reference returns all-NaN factors and NaN costs (after one
    iteration one row of U and all of V, after two everything).  The call returns: no exception, no retry through the error codes
    of the outer loop."""
    from nn_fac_amd.nmf import nmf
    X, U0, V0 = orc.synth_nmf(60, 50, 4, seed=2, dtype=np.float32)
    X[17, 23] = NAN
    kw = dict(init="custom", n_iter_max=3, tol=0, update_rule=rule, beta=beta, return_costs=True, deterministic=True)
    with np.errstate(all="ignore"):
        Uo, Vo, co, _ = orc.nmf(X.astype(np.float64), 4, U_0=U0.astype(np.float64), V_0=V0.astype(np.float64), **kw)
    assert np.isnan(Uo).all() and np.isnan(Vo).all() and np.isnan(co).all()
    U, V, costs, _ = nmf(X, 4, U_0=U0, V_0=V0, **kw)
    assert np.isnan(np.asarray(U)).all() and np.isnan(np.asarray(V)).all(), (np.isnan(U).mean(), np.isnan(V).mean())
    assert len(costs) == len(co) and np.isnan(np.asarray(costs, dtype=np.float64)).all(), costs


@pytest.mark.gpu
def test_ntf_with_a_nan_in_the_tensor(built_lib):
    """ntf (hals) on 8 x 9 x 10, rank 3, one NaN entry, three iterations, against orc.compute_ntf: NaN where it is NaN."""
    from nn_fac_amd.ntf import compute_ntf
    shape, R = (8, 9, 10), 3
    rng = np.random.RandomState(1)
    gen = [rng.rand(s, R) for s in shape]
    T = (np.einsum("ir,jr,kr->ijk", *gen) + 1e-2 * rng.rand(*shape)).astype(np.float32)
    T[3, 4, 5] = NAN
    F0 = [rng.rand(s, R).astype(np.float32) + 0.01 for s in shape]
    kw = dict(n_iter_max=3, tol=0, update_rule="hals", beta=2, return_costs=True, alpha=math.inf,
              sparsity_coefficients=[None] * 3, normalize=[False] * 3)
    with np.errstate(all="ignore"):
        Fo, co, _ = orc.compute_ntf(T.astype(np.float64), R, [f.astype(np.float64) for f in F0], **kw)
    assert all(np.isnan(f).any() for f in Fo) and np.isnan(co).all()
    F, costs, _ = compute_ntf(T, R, F0, **kw)
    for i in range(3):
        got, want = np.asarray(F[i], dtype=np.float64), Fo[i]
        assert np.isnan(got[np.isnan(want)]).all(), (i, int(np.isnan(got).sum()), int(np.isnan(want).sum()))
        f = np.isfinite(want)
        assert (np.isnan(got[f]) | (np.abs(got[f] - want[f]) <= 5e-5 * np.linalg.norm(want[f]))).all(), i
    assert len(costs) == len(co) and np.isnan(np.asarray(costs, dtype=np.float64)).all(), costs

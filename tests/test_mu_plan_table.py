"""The MU rows of test_gpu_launch_plans.plan_cases against a plain restatement of launch_mu_left and launch_mu_right (k_mu.hip,
k_mu_kernels.h), at 256 and at 304 compute units.  No GPU: this is what keeps the table's shapes on the side of the thresholds
they name on a machine that cannot ask the library (test_plan_table does, through NNF_PLAN_DEBUG, on the device)."""
import collections

import pytest

from test_gpu_launch_plans import REQUIRED, REQUIRED_BIG, _cdiv, note_plan, plan_cases

LIM = 0x7fff0000
WS_DEFAULT = 1024 << 20         # get_engine's context
ERR_UNSUPPORTED, ERR_WORKSPACE = -3, -4
CUS = (256, 304)


def _rup(a, b):
    return _cdiv(a, b) * b


class Cursor:
    """nnf_ws_cursor: blocks of the context workspace, each on a 256-byte boundary."""

    def __init__(self, cap):
        self.cap, self.off = cap, 0

    def take(self, nbytes):
        a = _rup(self.off, 256)
        if a + nbytes > self.cap:
            return None
        self.off = a + nbytes
        return a

    def remaining(self):
        return max(self.cap - _rup(self.off, 256), 0)


def split_rank(r, rem_ok):
    """mu_split_rank: (MT, REM).  Leftover ranks on the VALU pipe: up to 4 next to one tile, up to 2 next to two or three."""
    q, rem = divmod(r, 16)
    rem_of = 2 if rem <= 2 else (4 if q == 1 and rem <= 4 else 0)
    if rem_ok and 1 <= q <= 3 and rem >= 1 and rem_of > 0:
        return q, rem_of
    return _cdiv(r, 16), 0


def rowsum_scratch(cur, r, K):
    """nnf_launch_rowsum: r x np partials when a row has np = min(K / 8192, 64) > 1 pieces."""
    pieces = min(K // 8192, 64)
    return pieces <= 1 or cur.take(r * pieces * 8) is not None


def left_plan(C, case):
    m, n, r, ldx = case.m, case.n, case.r, case.ld or case.n
    kl, vec = case.beta == 1.0, (case.ld or case.n) % 4 == 0          # (the test's X starts an allocation: 16-byte aligned)
    ldv = n
    if r > 64:
        mt, rem = (6, 4) if kl and 96 < r <= 100 and vec else (_cdiv(r, 16), 0)
    else:
        mt, rem = split_rank(r, kl and vec)
    if rem:
        vec = True
    if 64 * ldx * 4 + 4 * (n + 128) >= LIM or 16 * (mt + 1) * ldv * 4 + 4 * (n + 128) >= LIM:
        return dict(status=ERR_UNSUPPORTED)
    wgpc = 1 if not kl or mt > 5 else 2                               # MU_LEFT_WGPC (KL, general beta)
    rows128 = mt > 4 and (not kl or mt == 5)                          # MU_LEFT_ROWS128
    slots, T = wgpc * C, _cdiv(m, 16)
    W = _cdiv(T, 16 * slots) * slots
    n_hi, n_mid, grid = 0, 0, W
    if rows128 or T <= 8 * slots:
        grid = _cdiv(m, 128)
    elif mt > 4:
        W3 = _cdiv(T, 12 * slots) * slots
        if T <= 8 * W3:
            grid = _cdiv(m, 128)
        else:
            grid, n_mid = W3, _cdiv(T - 8 * W3, 4)
    elif T > 12 * W:
        n_hi = _cdiv(T - 12 * W, 4)
        n_mid = W - n_hi
    else:
        n_mid = _cdiv(T - 8 * W, 4)
    form = "small" if T <= 8 * slots else "hi" if n_hi > 0 else "mid" if n_mid > 0 else "rows128" if mt > 4 else "mid"
    return dict(m=m, n=n, r=r, mt=mt, rem=rem, vec=int(vec), bm="KL" if kl else "GEN", form=form, grid=grid, n_hi=n_hi,
                n_mid=n_mid, slots=slots)


def right_plan(C, case):
    m, n, r, ldx = case.m, case.n, case.r, case.ld or case.n
    kl, vec = case.beta == 1.0, (case.ld or case.n) % 4 == 0
    ldu = m
    mt, rem = (_cdiv(r, 16), 0) if r > 64 else split_rank(r, kl and vec)
    if rem:
        vec = True
    if 16 * (mt + 1) * ldu * 4 + 4 * (m + 128) >= LIM:
        return dict(status=ERR_UNSUPPORTED)
    ncb = _cdiv(n, 64 * (2 if mt > 4 else 4))                         # MU_RIGHT_NC
    ldp, nacc = _rup(n, 4), 1 if kl else 2
    nsplit = max((2 if kl and mt <= 4 else 1) * C // ncb, 1)
    bound = "occupancy"
    if nsplit > _cdiv(m, 64):
        nsplit, bound = _cdiv(m, 64), "min_rows"
    slab = r * ldp * 4
    cur = Cursor(case.ws if case.ws is not None else WS_DEFAULT)
    if cur.take(r * 8) is None or (kl and not rowsum_scratch(cur, r, m)):
        return dict(status=ERR_WORKSPACE)
    ws_max = cur.remaining() // (slab * nacc)
    while nacc == 2 and ws_max >= 1 and _rup(ws_max * slab, 256) + ws_max * slab > cur.remaining():
        ws_max -= 1                                                   # (the second slab set starts on a 256-byte boundary)
    if ws_max < 1:
        return dict(status=ERR_WORKSPACE)
    if nsplit > ws_max:
        nsplit, bound = ws_max, "workspace"
    rps = _rup(_cdiv(m, nsplit), 64)
    while (rps + 128) * ldx * 4 >= LIM:
        if rps <= 64:
            return dict(status=ERR_UNSUPPORTED)
        rps, bound = _rup(rps // 2, 64), "offset32"
    nsplit = _cdiv(m, rps)
    if nsplit > ws_max or any(cur.take(nsplit * slab) is None for _ in range(nacc)):
        return dict(status=ERR_WORKSPACE)
    return dict(m=m, n=n, r=r, mt=mt, rem=rem, vec=int(vec), bm="KL" if kl else "GEN", nsplit=nsplit, rps=rps, bound=bound,
                ncb=ncb, ws_max=ws_max)


def plan_of(C, case):
    return left_plan(C, case) if case.kernel == "mu_left" else right_plan(C, case)


def mu_cases(C):
    return {nm: c for nm, c in plan_cases(C).items() if c.kernel in ("mu_left", "mu_right", "mu_accum")}


@pytest.mark.parametrize("C", CUS)
def test_mu_cases_take_the_plans_they_name(C):
    """Every field a MU case lists is what the restated launchers give, and the workgroups of every left plan cover the
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

"""Time one outer iteration of nonnegative PARAFAC2 (nn_fac_amd/parafac2.py) on the device: the grouped route (one launch per
statement for all K slices) against the same step composed slice by slice from the entry points that existed before the grouped
kernels (NNF_PARAFAC2_PER_SLICE=1: hals_solve, gram, frob_resid, an SVD per slice).

    python tools/time_parafac2.py --case many  --out profiles/parafac2_many.json      # K = 200 slices of 64..256 rows, n = 512, r = 16
    python tools/time_parafac2.py --case long  --out profiles/parafac2_long.json      # K = 8 slices of 50000 rows, n = 2000, r = 50

What is measured: host clock around `steps` iterations; every iteration ends in the device-to-host copy of its mu rule, so
the window is synchronised.  alpha = inf (the sweep counts do not depend on the wall clock, both routes do the same sweeps).
The two routes alternate, `rounds` times each, after a warm-up of both; the median per iteration and the spread over the
rounds are reported, with the calls into libnnfac_hip.so per iteration (each is one to three kernel launches; the torch glue
between them is not counted) and the agreement of the two routes after their first step.  Needs a GPU: there is no fallback."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nn_fac_amd import parafac2 as p2  # noqa: E402


class CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("nnf_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def problem(case, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    if case == "many":
        rows = [int(v) for v in np.random.RandomState(1).randint(64, 257, size=200)]
        n, r = 512, 16
    else:
        rows, n, r = [50000] * 8, 2000, 50
    rand = lambda *s: torch.rand(*s, generator=g, device=dev, dtype=torch.float32)   # noqa: E731
    H = rand(r, n)
    Ws = rand(r, r)
    slices, W0, D0 = [], [], []
    for m in rows:
        Q, _ = torch.linalg.qr(rand(m, r) - 0.5)
        slices.append(((Q @ Ws).abs() * (0.5 + rand(r))[None, :]) @ H + 0.01 * rand(m, n))
        W0.append(rand(m, r))
        D0.append(torch.diag(0.5 + rand(r)))
    return rows, n, r, slices, W0, D0, rand(r, n), rand(r, r)


def make_state(rows, n, r, slices, W0, D0, H0, Ws0):
    st = p2._State(slices, r, W0, H0, D0, Ws0, None, rows, n)
    resid = p2._slice_resid(st, p2._scaled_W(st)).cpu().numpy()
    norms = np.sqrt(p2._slice_resid(st, torch.zeros_like(st.Wt)).cpu().numpy())
    w2 = p2._slice_sums(st, st.Wt.double().pow(2).sum(dim=0)).cpu().numpy()
    return st, resid / (10 * w2), norms


def iterate(st, mu, norms, steps, prev=None):
    for _ in range(steps):
        mu, cost, _, _, _ = p2._step(st, mu, norms, prev, True, 1e6, 1.02, False, None, [], [False] * 5, math.inf)
        prev = cost
    return mu, prev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["many", "long"], required=True)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_parafac2.py needs a GPU")
    dev = torch.device("cuda:0")
    pb = problem(a.case, dev)
    routes = {"grouped": "0", "per_slice": "1"}
    state, first, calls = {}, {}, {}
    for name, env in routes.items():                       # warm-up: one state per route, the first step counted and kept
        os.environ["NNF_PARAFAC2_PER_SLICE"] = env
        st, mu, norms = make_state(*pb)
        lib = st.eng.lib
        st.eng.lib = CountingLib(lib)
        try:
            mu, prev = iterate(st, mu, norms, 1)
            calls[name] = dict(sorted(st.eng.lib.calls.items()))
        finally:
            st.eng.lib = lib
        first[name] = (st.Wt.clone(), st.H.clone(), st.Dt.clone(), prev)
        mu, prev = iterate(st, mu, norms, 1, prev)
        state[name] = (st, mu, norms, prev)
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())   # noqa: E731
    agree = {"W": rel(first["grouped"][0], first["per_slice"][0]), "H": rel(first["grouped"][1], first["per_slice"][1]),
             "D": rel(first["grouped"][2], first["per_slice"][2]),
             "cost": abs(first["grouped"][3] - first["per_slice"][3]) / abs(first["per_slice"][3])}
    times = {name: [] for name in routes}
    for _ in range(a.rounds):
        for name, env in routes.items():
            os.environ["NNF_PARAFAC2_PER_SLICE"] = env
            st, mu, norms, prev = state[name]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            mu, prev = iterate(st, mu, norms, a.steps, prev)
            torch.cuda.synchronize(dev)
            times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            state[name] = (st, mu, norms, prev)
    res = {"case": a.case, "K": len(pb[0]), "rows": [min(pb[0]), max(pb[0])], "n": pb[1], "r": pb[2], "steps_per_round": a.steps,
           "alpha": "inf", "device": torch.cuda.get_device_name(0),
           "ms_per_iteration": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "rounds": v}
                                for k, v in times.items()},
           "library_calls_per_iteration": {k: {"total": int(sum(v.values())), "by_entry": v} for k, v in calls.items()},
           "agreement_after_one_step": agree}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

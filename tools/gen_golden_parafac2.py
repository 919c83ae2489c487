"""Generate tests/golden/g11_parafac2.npz by running the REAL reference's nonnegative PARAFAC2 (ax-le/nn-fac checked out at
/root/reference: nn_fac/parafac2.py) on seeded inputs, after asserting tests/parafac2_restatement.py equal to it at 1e-10.

TEST INFRASTRUCTURE ONLY, build container only: the reference never travels, the .npz does.  The reference imports tensorly,
which is given the in-memory stand-in of oracle/gen_golden.py.  The wall clock is taken out of the sweep rule
(nnls.py:156,314) by wrapping the reference's two NNLS entries to alpha = inf; the wrappers also record the sweep counts.

Per run the fixture also holds the reference's OWN fp32-vs-fp64 sensitivity `s` per quantity: the same run with every input
cast to float32, compared with the float64 run (relative Frobenius / relative difference).

Usage:  python tools/gen_golden_parafac2.py
"""
import math
import os
import sys

import numpy as np

REF = "/root/reference"
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden", "g11_parafac2.npz")
N_ITER = 8


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def stack(lst):
    return np.concatenate([np.asarray(x) for x in lst], axis=0)


def diags(D_list):
    return np.array([np.diagonal(np.asarray(D)) for D in D_list])


def h(x):
    return np.asarray(x).astype(np.float16).astype(np.float64)


def f16(x):
    y = np.asarray(x).astype(np.float16)
    assert (y.astype(np.float64) == np.asarray(x)).all()
    return y


def problem(rows, n, r, seed):
    rng = np.random.RandomState(seed)
    Ht = rng.rand(r, n)
    Wst = rng.rand(r, r)
    slices, W0, D0, P0 = [], [], [], []
    for m in rows:
        Q, _ = np.linalg.qr(rng.randn(m, r))
        Wk = np.abs(Q @ Wst) + 0.05 * rng.rand(m, r)
        slices.append(Wk @ np.diag(0.5 + rng.rand(r)) @ Ht + 0.01 * rng.rand(m, n))
        W0.append(rng.rand(m, r))
        D0.append(np.diag(0.5 + rng.rand(r)))
        Qp, _ = np.linalg.qr(rng.randn(m, r))
        P0.append(Qp)
    # every input is rounded to float16 once: the fixture stores it in two bytes per entry, exactly, and the float64, the
    # float32 and the device runs all start from the very same numbers
    return dict(slices=[h(x) for x in slices], W0=[h(x) for x in W0], D0=[h(x) for x in D0], P0=[h(x) for x in P0],
                H0=h(rng.rand(r, n)), Ws0=h(rng.rand(r, r)), r=r, rows=list(rows), n=n)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("gen_golden_parafac2.py needs /root/reference (build container only)")
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gen_golden
    gen_golden._install_tensorly_standin()
    sys.path.insert(0, REF)
    import nn_fac.update_rules.nnls as ref_nnls
    import nn_fac.parafac2 as ref
    import parafac2_restatement as rs

    counts = []
    plain, coupled = ref_nnls.hals_nnls_acc, ref_nnls.hals_coupling_nnls_acc

    def w_plain(*a, **k):
        k["alpha"] = math.inf
        out = plain(*a, **k)
        counts.append(("p", a[0].shape[1], int(out[2])))
        return out

    def w_coupled(*a, **k):
        k["alpha"] = math.inf
        out = coupled(*a, **k)
        counts.append(("c", a[0].shape[1], int(out[2])))
        return out
    ref_nnls.hals_nnls_acc, ref_nnls.hals_coupling_nnls_acc = w_plain, w_coupled

    def split_counts(K):
        """the recorded solves of ONE step, in call order: (coupled, plain one-column) per slice, then H"""
        cw = np.array([c for t, _, c in counts if t == "c"], dtype=np.int64)
        pl = [c for t, _, c in counts if t == "p"]
        assert len(cw) == K and len(pl) == K + 1
        return cw, np.array(pl[:K], dtype=np.int64), int(pl[K])

    g = {}
    problems = {"a": problem([7, 256, 33, 64, 65, 18, 12, 42], 70, 6, 1101),
                "b": problem([70, 31, 129, 64], 33, 17, 1102)}
    for name, pb in problems.items():
        K, r = len(pb["rows"]), pb["r"]
        g[f"{name}_rows"], g[f"{name}_rank"] = np.array(pb["rows"], dtype=np.int64), np.int64(r)
        g[f"{name}_X"], g[f"{name}_W0"], g[f"{name}_P0"] = f16(stack(pb["slices"])), f16(stack(pb["W0"])), f16(stack(pb["P0"]))
        g[f"{name}_D0"], g[f"{name}_H0"], g[f"{name}_Ws0"] = f16(diags(pb["D0"])), f16(pb["H0"]), f16(pb["Ws0"])
        norm_slices = [np.linalg.norm(x, ord='fro') for x in pb["slices"]]
        mu0 = np.array([np.linalg.norm(pb["slices"][k] - pb["W0"][k] @ pb["D0"][k] @ pb["H0"], ord='fro') ** 2 /
                        (10 * np.linalg.norm(pb["W0"][k], ord='fro') ** 2) for k in range(K)])
        prev = 10.0 * float(sum(v ** 2 for v in norm_slices))      # above any cost: the mu rule takes its first branch
        g[f"{name}_mu0"], g[f"{name}_prev"] = mu0, np.float64(prev)
        for withP in (True, False):
            p = f"{name}_{'P' if withP else 'S'}_"
            kw = dict(init_with_P=withP, P_list_in=pb["P0"] if withP else None, W_star_in=None if withP else pb["Ws0"])
            # ---- one step ---------------------------------------------------------------------------------
            del counts[:]
            out = ref.one_step_parafac2(pb["slices"], r, pb["W0"], pb["H0"], pb["D0"], mu0, norm_slices, prev, increasing_mu=True,
                                        **kw)
            cw, cd, ch = split_counts(K)
            info = {}
            chk = rs.one_step_parafac2(pb["slices"], r, pb["W0"], pb["H0"], pb["D0"], mu0, norm_slices, prev, increasing_mu=True,
                                       alpha=math.inf, info=info, **kw)
            for i in (0, 2, 4):
                assert rel(stack(chk[i]), stack(out[i])) < 1e-10, (p, i)
            for i in (1, 3, 5, 6, 7):
                assert rel(chk[i], out[i]) < 1e-10, (p, i)
            assert chk[8] == out[8] and (info["cnt_W"] == cw).all() and (info["cnt_D"] == cd).all() and info["cnt_H"] == ch
            g[p + "step_W"], g[p + "step_H"], g[p + "step_D"] = stack(out[0]), out[1], diags(out[2])
            g[p + "step_Ws"], g[p + "step_mu"] = out[3], np.array(out[5])
            if not withP:                       # (init_with_P: the P_k of the step are the inputs)
                g[p + "step_P"] = stack(out[4])
            g[p + "step_cost"], g[p + "step_ce"], g[p + "step_inc"] = np.float64(out[6]), np.array(out[7]), np.bool_(out[8])
            g[p + "step_cntW"], g[p + "step_cntD"], g[p + "step_cntH"] = cw, cd, np.int64(ch)
            # ---- N_ITER iterations, fp64 and with every input cast to fp32 -----------------------------------------
            runs = {}
            for dt in (np.float64, np.float32):
                c = lambda lst: [np.asarray(x, dtype=dt) for x in lst]   # noqa: E731
                del counts[:]
                o = ref.compute_parafac_2(c(pb["slices"]), r, c(pb["W0"]), pb["H0"].astype(dt), c(pb["D0"]), withP,
                                          W_star_in=None if withP else pb["Ws0"].astype(dt), P_list_in=c(pb["P0"]) if withP else None,
                                          n_iter_max=N_ITER, tol=0, return_costs=True)
                runs[dt] = (stack(o[0]), o[1], diags(o[2]), np.array(o[3]), [c_ for _, _, c_ in counts])
            W, H, D, costs, cn = runs[np.float64]
            W32, H32, D32, costs32, cn32 = runs[np.float32]
            assert len(costs) == N_ITER
            o = rs.compute_parafac_2(pb["slices"], r, pb["W0"], pb["H0"], pb["D0"], withP, W_star_in=None if withP else pb["Ws0"],
                                     P_list_in=pb["P0"] if withP else None, n_iter_max=N_ITER, tol=0, return_costs=True,
                                     alpha=math.inf)
            assert rel(stack(o[0]), W) < 1e-10 and rel(o[1], H) < 1e-10 and rel(diags(o[2]), D) < 1e-10 and rel(o[3], costs) < 1e-10
            g[p + "run_W"], g[p + "run_H"], g[p + "run_D"], g[p + "run_costs"] = W, H, D, costs
            g[p + "run_s"] = np.array([rel(W32, W), rel(H32, H), rel(D32, D), abs(costs32[-1] - costs[-1]) / abs(costs[-1])])
            g[p + "run_counts_equal_fp32"] = np.bool_(cn == cn32)
            print(p, "s(W,H,D,cost) =", g[p + "run_s"], "counts equal in fp32:", cn == cn32, "cost", costs[-1])

    # ---- equal slices, init="random", init_with_P=True, deterministic=True ---------------------------------------------
    rng = np.random.RandomState(1103)
    K, m, n, r = 5, 40, 50, 5
    Ht = rng.rand(r, n)
    slices = [h(rng.rand(m, r) @ np.diag(0.5 + rng.rand(r)) @ Ht + 0.01 * rng.rand(m, n)) for _ in range(K)]
    runs = {}
    for dt in (np.float64, np.float32):
        o = ref.parafac_2([x.astype(dt) for x in slices], r, True, init="random", n_iter_max=N_ITER, tol=0, return_costs=True,
                          deterministic=True, seed=7)
        runs[dt] = (stack(o[0]), o[1], diags(o[2]), np.array(o[3]))
    W, H, D, costs = runs[np.float64]
    Wl, Hi, Dl, Pl, Ws = rs.parafac2_initialization(slices, r, "random", True, deterministic=True, seed=7)
    o = rs.compute_parafac_2(slices, r, Wl, Hi, Dl, True, W_star_in=Ws, P_list_in=Pl, n_iter_max=N_ITER, tol=0, return_costs=True,
                             alpha=math.inf)
    assert rel(stack(o[0]), W) < 1e-10 and rel(o[1], H) < 1e-10 and rel(diags(o[2]), D) < 1e-10 and rel(o[3], costs) < 1e-10
    g["r_X"], g["r_shape"] = f16(stack(slices)), np.array([K, m, n, r, 7], dtype=np.int64)
    g["r_run_W"], g["r_run_H"], g["r_run_D"], g["r_run_costs"] = W, H, D, costs
    W32, H32, D32, costs32 = runs[np.float32]
    g["r_run_s"] = np.array([rel(W32, W), rel(H32, H), rel(D32, D), abs(costs32[-1] - costs[-1]) / abs(costs[-1])])
    print("r_ s(W,H,D,cost) =", g["r_run_s"])
    np.savez_compressed(OUT, **g)
    print(f"G11 ok: {os.path.getsize(OUT) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()

"""Generate tests/golden/g12_simplex.npz by running the REAL reference's simplex-constrained NMF (ax-le/nn-fac:
nn_fac/simplex_nmf.py, update_rules/mu.py:161-175, utils/normalize_wh.py:24-58) on seeded inputs, after asserting
tests/simplex_restatement.py equal to it at 1e-12.

TEST INFRASTRUCTURE ONLY: the reference never travels, the .npz does.  The reference's mu.py imports tensorly, which is given
the in-memory stand-in of oracle/gen_golden.py.  The Newton iteration counts are the restatement's (the reference does not
return them); the restatement's multipliers, warnings and factors are asserted equal to the reference's in every call.

The generator also asserts the two facts the beta = 1 restriction of nn_fac_amd.simplex_nmf rests on: at beta = 1 the columns
of H sum to 1 within 1e-6 after every step, at beta = 2 they do not.

Usage:  python tools/gen_golden_simplex.py <checkout of the reference>
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
OUT = os.path.join(ROOT, "tests", "golden", "g12_simplex.npz")
N_ITER = 8
# The seeds were picked among 1 .. 80 for what the tests lean on: the second step of every run takes all 100 Newton iterations
# (and warns), and from iteration 3 on (the reference's 0-based loop variable) the columns of H sum to 1.  Most seeds give the
# first; before iteration 3 the reference's rule leaves sums far from 1 at every seed tried at ranks 50 and 100.
RUNS = {"a": (100, 200, 5, 3), "b": (70, 67, 19, 10), "c": (130, 97, 50, 39), "d": (90, 130, 100, 55)}
PROJ = {"p0": (40, 33, 3, 1211), "p1": (25, 70, 17, 1212), "p2": (30, 9, 1, 1213)}
SIMPLEX_FROM = 3


def h(x):
    """Rounded to float16 once: two bytes per entry in the fixture, and every run starts from the very same numbers."""
    return np.asarray(x).astype(np.float16).astype(np.float64)


def f16(x):
    y = np.asarray(x).astype(np.float16)
    assert (y.astype(np.float64) == np.asarray(x)).all()
    return y


def f32(x):
    y = np.asarray(x).astype(np.float32)
    assert (y.astype(np.float64) == np.asarray(x)).all()
    return y


def r32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def problem(m, n, r, seed):
    """Random starts, X = W H_simplex + 0.01 rand."""
    rng = np.random.RandomState(seed)
    W0, H0 = rng.rand(m, r), rng.rand(r, n)
    Ht = rng.rand(r, n)
    X = rng.rand(m, r) @ (Ht / Ht.sum(axis=0)) + 1e-2 * rng.rand(m, n)
    X, W0, H0 = h(X), h(W0), h(H0)
    assert X.min() > 0 and W0.min() > 0 and H0.min() > 0
    return X, W0, H0


def warned_at_second_step(infos):
    return infos[1]["warned"] and infos[1]["count"] == 100


def caught(fn, *a, **k):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = fn(*a, **k)
    return out, [str(x.message) for x in w]


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "nn_fac")):
        raise SystemExit(__doc__)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gen_golden
    gen_golden._install_tensorly_standin()
    sys.path.insert(0, sys.argv[1])
    import nn_fac.update_rules.mu as ref_mu
    import nn_fac.utils.normalize_wh as ref_nw
    import nn_fac.simplex_nmf as ref
    import simplex_restatement as rs

    g = {}
    # ---- single calls of simplex_proj_mu ------------------------------------------------------------------------------
    for name, (m, n, r, seed) in PROJ.items():
        X, W, H = problem(m, n, r, seed)
        out, msgs = caught(ref_mu.simplex_proj_mu, X, W, H, 1)
        info = {}
        chk, _ = caught(rs.simplex_proj_mu, X, W, H, 1, info=info)
        assert relmax(chk, out) < 1e-12 and info["warned"] == (len(msgs) > 0), name
        assert all(s == rs.WARNING for s in msgs)
        g[f"{name}_X"], g[f"{name}_W"], g[f"{name}_H"] = f16(X), f16(W), f16(H)
        g[f"{name}_out"], g[f"{name}_count"], g[f"{name}_warned"] = out, np.int64(info["count"]), np.bool_(info["warned"])
        print(name, "newton", info["count"], "warned", info["warned"])

    # ---- the runs: N_ITER iterations from custom starts; every multiplier call recorded ---------------------------------
    calls = []
    inner = ref_nw.update_lagragian_multipliers_simplex_projection

    def recording(C, D, H, beta, lam0, tol=1e-6, n_iter_max=100):
        out = inner(C, D, H, beta, lam0, tol=tol, n_iter_max=n_iter_max)
        calls.append((C.copy(), D.copy(), H.copy(), lam0.copy(), out.copy()))
        return out
    ref_nw.update_lagragian_multipliers_simplex_projection = recording
    full = None
    for name, (m, n, r, seed) in RUNS.items():
        X, W0, H0 = problem(m, n, r, seed)
        del calls[:]
        (W, H, costs, _), msgs = caught(ref.compute_simplex_beta_nmf, X, W0, H0, r, 1, n_iter_max=N_ITER, tol=0)
        infos = []
        (Wr, Hr, cr, _), _ = caught(rs.compute_simplex_beta_nmf, X, W0, H0, r, 1, n_iter_max=N_ITER, tol=0, infos=infos)
        assert len(costs) == N_ITER and relmax(Wr, W) < 1e-12 and relmax(Hr, H) < 1e-12 and relmax(cr, costs) < 1e-12, name
        assert sum(i["warned"] for i in infos) == len(msgs) and all(s == rs.WARNING for s in msgs), name
        assert warned_at_second_step(infos), name
        Wi, Hi = W0, H0
        for t in range(N_ITER):      # the fact the beta = 1 restriction rests on: the columns of H end up on the simplex
            (Wi, Hi, _), _ = caught(ref.one_step_simplex_beta_nmf, X, Wi, Hi, r, 1, 1e-6)
            assert t < SIMPLEX_FROM or np.max(np.abs(Hi.sum(axis=0) - 1)) < 1e-6, (name, t)
            if name == "a":          # the iterates of run a (early stops are compared with these)
                g[f"a_W_it{t}"], g[f"a_H_it{t}"] = Wi, Hi
        assert relmax(Wi, W) < 1e-12 and relmax(Hi, H) < 1e-12
        counts = np.array([i["count"] for i in infos], dtype=np.int64)
        warned = np.array([i["warned"] for i in infos])
        g[f"{name}_X"], g[f"{name}_W0"], g[f"{name}_H0"], g[f"{name}_rank"] = f16(X), f16(W0), f16(H0), np.int64(r)
        g[f"{name}_W"], g[f"{name}_H"], g[f"{name}_costs"] = W, H, np.array(costs)
        g[f"{name}_counts"], g[f"{name}_warned"] = counts, warned
        # the driver's own floor: the same run with W, H, C, D rounded to float32 after every update
        (W32, H32, c32, _), _ = caught(rs.compute_simplex_beta_nmf, X, W0, H0, r, 1, n_iter_max=N_ITER, tol=0, round32=True)
        g[f"{name}_floor"] = np.array([np.linalg.norm(W32 - W) / np.linalg.norm(W), np.linalg.norm(H32 - H) / np.linalg.norm(H),
                                       np.max(np.abs(np.array(c32) - costs) / np.abs(costs))])
        print(name, "newton", counts.tolist(), "warned", warned.tolist(), "cost", costs[0], "->", costs[-1], "fp32 floor",
              g[f"{name}_floor"])
        if name == "a":
            # every multiplier call of this run, operands rounded to float32 (what the device kernel is fed) and re-run
            hit = [i for i, w_ in enumerate(warned) if w_]
            assert hit, "no call of run a runs all 100 iterations: pick another seed"
            i = hit[0]
            C, D, Hc, lam0, _ = calls[i]
            C, D, Hc = r32(C), r32(D), r32(Hc)
            lam0 = rs.lambda_start(C, D, Hc)      # (mu.py:168 on the rounded operands, as the device forms it)
            out, msgs = caught(inner, C, D, Hc, 1, lam0, tol=1e-6, n_iter_max=100)
            info = {}
            chk, _ = caught(rs.update_lagragian_multipliers_simplex_projection, C, D, Hc, 1, lam0, info=info)
            assert relmax(chk, out) < 1e-12 and info["count"] == 100 and info["warned"] and len(msgs) == 1
            g["n_C"], g["n_D"], g["n_H"], g["n_lam0"], g["n_lam"] = f32(C), f32(D), f32(Hc), lam0.reshape(-1), out.reshape(-1)
            g["n_count"], g["n_last"], g["n_iteration"] = np.int64(100), np.float64(info["deltas"][-1]), np.int64(i)
            last = g["n_last"]
            # a converging call of the same run, the multiplier function alone (lambda0 given)
            j = next(t for t, w_ in enumerate(warned) if not w_ and t > i)
            C, D, Hc, lam0, _ = calls[j]
            C, D, Hc = r32(C), r32(D), r32(Hc)
            lam0 = rs.lambda_start(C, D, Hc)      # (mu.py:168 on the rounded operands, as the device forms it)
            out, msgs = caught(inner, C, D, Hc, 1, lam0, tol=1e-6, n_iter_max=100)
            info = {}
            chk, _ = caught(rs.update_lagragian_multipliers_simplex_projection, C, D, Hc, 1, lam0, info=info)
            assert relmax(chk, out) < 1e-12 and not msgs and not info["warned"], (relmax(chk, out), msgs, info["count"])
            g["m_C"], g["m_D"], g["m_H"], g["m_lam0"], g["m_lam"] = f32(C), f32(D), f32(Hc), lam0.reshape(-1), out.reshape(-1)
            g["m_count"] = np.int64(info["count"])
            print("multiplier calls: non-converging at iteration", i, "last", last, "; converging at", j, "count",
                  g["m_count"])
            full = (X, W0, H0, r)
    ref_nw.update_lagragian_multipliers_simplex_projection = inner

    # ---- beta = 2: what the reference's rule gives (the reason nn_fac_amd refuses every beta but 1) ------------------------
    X, W0, H0, r = full
    with np.errstate(all="ignore"):
        (_, H2, _, _), _ = caught(ref.compute_simplex_beta_nmf, X, W0, H0, r, 2, n_iter_max=N_ITER, tol=0)
    s2 = H2.sum(axis=0)
    assert not np.max(np.abs(s2 - 1)) < 1e-6, "beta = 2 column sums"
    print(f"beta = 2 column sums after {N_ITER} iterations:", float(np.min(s2)), "...", float(np.max(s2)))
    np.savez_compressed(OUT, **g)
    print(f"G12 ok: {os.path.getsize(OUT) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()

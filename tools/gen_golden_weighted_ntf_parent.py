"""Writes tests/golden/weighted_ntf_parent.npz: the factors and costs of ntf(..., update_rule="mu") at beta = 1 and beta = 0.5, five
iterations with tol = 0, on the 30 x 41 x 52 rank-7 problem of tests/test_gpu_weighted_ntf.py -- to be run on a MI355X FROM THE
COMMIT BEFORE the `weights=` keyword of ntf existed (the script passes no such keyword and needs nothing of that commit's
successors).  tests/test_gpu_weighted_ntf.py::test_weights_none_is_bitwise_the_parent compares weights=None against the file bit
for bit and reads `golden_problem` and `RUNS` from here.

    python tools/gen_golden_weighted_ntf_parent.py [output.npz]

NNF_GOLDEN_TREE: the checkout whose built package runs (default: the one this file lies in).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITER = 5
RUNS = {"mu_b1": 1, "mu_b05": 0.5}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def golden_problem():
    """(T, r, factors0): 30 x 41 x 52 at rank 7, every value exactly representable in fp32."""
    shape, r = (30, 41, 52), 7
    rng = np.random.default_rng(31)
    return f32(rng.random(shape) + 0.1), r, [f32(rng.random((s, r)) + 0.05) for s in shape]


def golden_run(tag, ntf, **kw):
    """One run: (factors as float32 arrays, costs as float64)."""
    T, r, F0 = golden_problem()
    F, costs, _ = ntf(T, r, init="custom", factors_0=F0, n_iter_max=N_ITER, tol=0, update_rule="mu", beta=RUNS[tag],
                      sparsity_coefficients=[None] * 3, fixed_modes=[], normalize=[False] * 3, return_costs=True, **kw)
    return [np.asarray(f, np.float32) for f in F], np.asarray(costs, np.float64)


def main(out):
    sys.path.insert(0, os.environ.get("NNF_GOLDEN_TREE", ROOT))
    from nn_fac_amd.ntf import ntf
    saved = {}
    for tag in RUNS:
        F, costs = golden_run(tag, ntf)
        for i, f in enumerate(F):
            saved["%s_F%d" % (tag, i)] = f
        saved[tag + "_costs"] = costs
        print(tag, costs)
    np.savez(out, **saved)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "weighted_ntf_parent.npz"))

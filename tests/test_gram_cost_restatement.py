"""The restatement of the Gram-identity cost (tests/gram_cost_restatement.py) against the plain residual, on the CPU: the identity
itself on unrounded fp64 operands, and the estimate's claim |cost - residual| <= est on operands rounded to fp32."""
import numpy as np
import pytest

import gram_cost_restatement as gcr


@pytest.mark.parametrize("m,n,r", [(300, 40, 7), (200, 33, 130)])
def test_identity_on_unrounded_operands(m, n, r):
    """U^T X and U^T U formed in fp64 from fp32 U, V, X and NOT rounded: the restated cost is sum((X - U V)^2) to 1e-9 of
    ||X||^2 (the cancellation of three terms of that size in extended precision leaves far less)."""
    rng = np.random.RandomState(m + n + r)
    U, V, X = (rng.rand(m, r).astype(np.float32), rng.rand(r, n).astype(np.float32), rng.rand(m, n).astype(np.float32))
    U64, V64, X64 = U.astype(np.float64), V.astype(np.float64), X.astype(np.float64)
    normx2 = float(np.sum(X64 * X64))
    want = float(np.sum((X64 - U64 @ V64) ** 2))
    got = gcr.restate(V, U64.T @ X64, None, normx2, G64=U64.T @ U64)
    print(m, n, r, "restated", got.cost, "residual", want, "difference / ||X||^2", abs(got.cost - want) / normx2)
    assert abs(got.cost - want) <= 1e-9 * normx2
    # the sums are what they are called
    assert abs(got.V2 - np.sum(V64 * V64)) <= 1e-12 * got.V2
    assert abs(got.A - np.sum(V64 * (U64.T @ X64))) <= 1e-12 * got.abs_a
    assert got.abs_a >= abs(got.A) and got.abs_b >= abs(got.B)


def test_hadamard_gram_is_the_fp32_product_and_g64_replaces_the_gram():
    rng = np.random.RandomState(5)
    r, n = 9, 21
    V = rng.rand(r, n).astype(np.float32)
    UtM = (rng.rand(r, n) - 0.25).astype(np.float32)
    G, G2 = (rng.rand(r, r) - 0.25).astype(np.float32), (rng.rand(r, r) - 0.25).astype(np.float32)
    had = gcr.restate(V, UtM, G, 100.0, G2=G2)
    one = gcr.restate(V, UtM, G * G2, 100.0)
    assert had == one
    V64 = V.astype(np.float64)
    assert abs(had.B - np.einsum("aj,ab,bj->", V64, (G * G2).astype(np.float64), V64)) <= 1e-12 * had.abs_b
    exact_product = G.astype(np.float64) * G2.astype(np.float64)                 # (not what a Hadamard pair means)
    assert gcr.restate(V, UtM, None, 100.0, G64=exact_product).B != had.B
    G64 = G.astype(np.float64) + 1e-9 * rng.rand(r, r)
    g64 = gcr.restate(V, UtM, G, 100.0, sigma_g=5e-9, G64=G64)
    assert abs(g64.B - np.einsum("aj,ab,bj->", V64, G64, V64)) <= 1e-12 * g64.abs_b
    assert g64.gmax == float(np.abs(G64.astype(np.float32)).max())
    with pytest.raises(ValueError):
        gcr.restate(V, UtM, G, 100.0, G2=G2, G64=G64)


def test_verdict_rule():
    V = np.array([[1.0, 2.0]], dtype=np.float32)
    UtM = np.array([[3.0, -1.0]], dtype=np.float32)
    G = np.array([[2.0]], dtype=np.float32)
    s = gcr.sums(V, UtM, G)
    assert (float(s.A), float(s.A2), float(s.B), float(s.V2), float(s.abs_a), float(s.abs_b)) == (1.0, 13.0, 10.0, 5.0, 5.0, 10.0)
    got = gcr.verdict(s, 4.0, sigma_a=0.25, bias_a=0.5, sigma_g=0.125)
    assert got.cost == 12.0
    want_est = 4 * np.sqrt((2 * 0.25) ** 2 * 13.0 + (0.125 * 2.0 * 5.0) ** 2) + 4 * 0.5 * 1.0
    assert abs(got.est - want_est) <= 4e-16 * want_est
    assert got.flag == 1
    assert gcr.verdict(s, 4.0, sigma_a=1e-9, bias_a=0.0, sigma_g=0.0).flag == 0
    assert gcr.verdict(s, -9.0, sigma_a=0.0, bias_a=0.0, sigma_g=0.0).flag == 1          # a negative cost, whatever the estimate
    assert gcr.verdict(s, float("nan")).flag == 1


@pytest.mark.parametrize("noise", gcr.IDENTITY_NOISE)
@pytest.mark.parametrize("m,n,r", gcr.IDENTITY_SHAPES)
def test_estimate_covers_operands_rounded_to_fp32(m, n, r, noise):
    """U^T X and U^T U rounded to fp32 (correctly, once): the error of the restated cost is inside its estimate, in the fp32-Gram
    form at (6e-8, 0) and in the fp64-Gram form at (6e-8, 0, 5e-9)."""
    U, V, X, want = gcr.identity_case(m, n, r, noise)
    U64, X64 = U.astype(np.float64), X.astype(np.float64)
    normx2 = float(np.sum(X64 * X64))
    UtM = (U64.T @ X64).astype(np.float32)
    G64 = U64.T @ U64
    W = gcr.column_gram(V)
    for name, got in (("fp32", gcr.restate(V, UtM, G64.astype(np.float32), normx2, 6e-8, 0.0, W=W)),
                      ("g64", gcr.restate(V, UtM, G64.astype(np.float32), normx2, 6e-8, 0.0, 5e-9, G64=G64, W=W))):
        print(m, n, r, noise, name, "|cost - want| / est =", abs(got.cost - want) / got.est, "est / (5e-4 want) =",
              got.est / (5e-4 * want) if want > 0 else np.inf, "flag", got.flag)
        assert abs(got.cost - want) <= got.est
        assert got.flag == (0 if noise == 3e-2 else 1)

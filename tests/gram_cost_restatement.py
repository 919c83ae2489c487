"""Extended-precision restatement of the Gram-identity cost (nnf_gram_cost_kernel, nn_fac_amd/csrc/nnf_api.hip; the contract is in
include/nnfac_hip.h).  TEST INFRASTRUCTURE: NumPy only, no torch, no GPU -- the ground truth tests/test_gpu_gram_cost.py holds
the kernel to, and itself checked against the plain residual by tests/test_gram_cost_restatement.py.

It restates the kernel's DEFINITIONS, not its code (no 16-thread split, no partials, no ticket):

    A  = sum_aj v_aj utm_aj          A2 = sum_aj (v_aj utm_aj)^2
    B  = sum_j v_j^T G v_j           V2 = sum_aj v_aj^2
    cost = normx2 - 2 A + B
    est  = 4 sqrt((2 sigma_a sqrt(A2))^2 + (sigma_g max|G| V2)^2) + 4 bias_a |A|
    flag = 0 if est <= 5e-4 cost, else 1            (a NaN or a non-positive cost gives 1)

with G the fp32 Gram; for a Hadamard pair the fp32 product G*G2 rounded ONCE (at every rank); with G64 given, the quadratic form
is taken on G64 and max|G| on float32(G64).  Sums run in np.longdouble (64-bit mantissa on x86); where longdouble is a plain
double they run through math.fsum, on products that are exact in fp64 wherever the operands are fp32.

B is evaluated as <G, V V^T>: the same sum of the same r*r*n products, grouped so that W = V V^T -- which does not depend on the
Gram -- can be computed once (`column_gram`) and shared by every form tested on the same V."""
import math
from collections import namedtuple

import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63
U53 = 2.0 ** -53
SIGMA_G_FP32 = 4e-8            # what the two fp32-Gram entry points hand the kernel (fp32 storage of a Gram entry)

Sums = namedtuple("Sums", "A A2 B V2 gmax abs_a abs_b r n")
GramCost = namedtuple("GramCost", "cost flag est A A2 B V2 abs_a abs_b gmax tol_cost tol_est")


def _sum(a):
    """Sum of an array of exactly representable terms: longdouble pairwise, or fsum (exact) where longdouble is a double."""
    a = np.asarray(a)
    if WIDE:
        return LD(a.astype(LD, copy=False).sum())
    return LD(math.fsum(a.astype(np.float64, copy=False).ravel().tolist()))


def _f32(a, name):
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"{name}: float32 expected, got {a.dtype}")
    return a


def column_gram(V):
    """(V V^T, |V| |V|^T) in extended precision; products of two fp32 numbers are exact in fp64."""
    V = _f32(V, "V")
    if WIDE:
        Vl = V.astype(LD)
        W = Vl @ Vl.T
        Wabs = W if not (V < 0).any() else np.abs(Vl) @ np.abs(Vl).T
        return W, Wabs
    r = V.shape[0]
    V64, W, Wabs = V.astype(np.float64), np.zeros((r, r)), np.zeros((r, r))
    for a in range(r):
        for b in range(a + 1):
            p = V64[a] * V64[b]
            W[a, b] = W[b, a] = math.fsum(p.tolist())
            Wabs[a, b] = Wabs[b, a] = math.fsum(np.abs(p).tolist())
    return W, Wabs


def effective_gram(G, G2=None, G64=None):
    """(the Gram the quadratic form is taken on, the fp32 Gram max|G| is taken over)."""
    if G64 is not None:
        if G2 is not None:
            raise ValueError("G64 cannot be combined with a Hadamard pair")
        G64 = np.asarray(G64)
        if G64.dtype != np.float64:
            raise TypeError(f"G64: float64 expected, got {G64.dtype}")
        return G64, G64.astype(np.float32)
    G = _f32(G, "G")
    if G2 is not None:
        G = G * _f32(G2, "G2")             # fp32 product, rounded once
    return G, G


def sums(V, UtM, G, G2=None, G64=None, W=None):
    """The operand sums.  UtM may be fp64 (the CPU test hands over an unrounded U^T X); V and the Grams are typed as above.
    W = column_gram(V), if the caller has it already."""
    V = _f32(V, "V")
    UtM = np.asarray(UtM)
    if UtM.dtype not in (np.float32, np.float64) or UtM.shape != V.shape:
        raise TypeError("UtM: float32 or float64 of V's shape expected")
    r, n = V.shape
    Gq, Gf = effective_gram(G, G2, G64)
    if Gq.shape != (r, r):
        raise ValueError("the Gram must be r x r")
    W, Wabs = column_gram(V) if W is None else W
    if WIDE:
        P = V.astype(LD) * UtM.astype(LD)
        A, A2, abs_a = P.sum(), (P * P).sum(), np.abs(P).sum()
        V2 = np.trace(W)
        Gl = Gq.astype(LD)
        B, abs_b = (Gl * W).sum(), (np.abs(Gl) * Wabs).sum()
    else:
        P = V.astype(np.float64) * UtM.astype(np.float64)
        A, A2, abs_a = _sum(P), _sum(P * P), _sum(np.abs(P))
        V2 = _sum(np.diag(W))
        Gd = Gq.astype(np.float64)
        B, abs_b = _sum(Gd * W), _sum(np.abs(Gd) * Wabs)
    gmax = float(np.abs(Gf).max())         # (NaN if the Gram holds one, as fmaxf would not give -- no test puts one there)
    return Sums(LD(A), LD(A2), LD(B), LD(V2), gmax, LD(abs_a), LD(abs_b), r, n)


def verdict(s, normx2, sigma_a=6e-8, bias_a=0.0, sigma_g=SIGMA_G_FP32):
    """cost, flag, estimate and the a-priori bounds from the sums of `sums`."""
    nx = LD(float(normx2))
    cost = nx - 2 * s.A + s.B
    sa = 2 * LD(sigma_a) * np.sqrt(s.A2)
    sb = LD(sigma_g) * LD(s.gmax) * s.V2
    est = 4 * np.sqrt(sa * sa + sb * sb) + 4 * LD(bias_a) * abs(s.A)
    flag = 0 if est <= LD(5e-4) * cost else 1
    # worst case of an fp64 sum of N products (each product and each addition rounds once: N u of the sum of absolute terms),
    # doubled; N = the longest chain the kernel can form -- n*r column terms, r terms of a Gram row, 8 for the closing arithmetic
    N = s.n * s.r + s.r + 8
    tol_cost = 2 * N * U53 * (abs(float(nx)) + 2 * float(s.abs_a) + float(s.abs_b))
    tol_est = 2 * N * U53 * float(est) + 4 * float(bias_a) * N * U53 * float(s.abs_a)
    return GramCost(float(cost), flag, float(est), float(s.A), float(s.A2), float(s.B), float(s.V2), float(s.abs_a),
                    float(s.abs_b), s.gmax, tol_cost, tol_est)


def restate(V, UtM, G, normx2, sigma_a=6e-8, bias_a=0.0, sigma_g=None, G2=None, G64=None, W=None):
    """The whole statement in one call.  sigma_g None: 4e-8, the fp32-Gram entry points' figure."""
    return verdict(sums(V, UtM, G, G2=G2, G64=G64, W=W), normx2, sigma_a, bias_a, SIGMA_G_FP32 if sigma_g is None else sigma_g)


def exact_dot(A, B):
    """(sum_ij A_ij B_ij, sum_ij |A_ij B_ij|) of fp32 arrays; the products are exact in fp64."""
    P = _f32(A, "A").astype(np.float64) * _f32(B, "B").astype(np.float64)
    return float(_sum(P)), float(_sum(np.abs(P)))


# ---- the identity against the true residual: the data of tests/test_gram_cost_restatement.py and of part E on the device ----
IDENTITY_SHAPES = [(3000, 130, 5), (3000, 130, 33), (3000, 130, 100), (2000, 67, 128), (1500, 50, 160)]    # (m, n, r)
IDENTITY_NOISE = [3e-2, 1e-3, 1e-4, 0.0]


def identity_case(m, n, r, noise):
    """fp32 U (m x r), V (r x n), X = (U V)(1 + noise * randn) and the fp64 residual sum((X - U V)^2) of those fp32 arrays."""
    rng = np.random.RandomState(m + n + r)
    U, V = rng.rand(m, r), rng.rand(r, n)
    X = (U @ V * (1 + noise * rng.randn(m, n))).astype(np.float32)
    U, V = U.astype(np.float32), V.astype(np.float32)
    want = float(np.sum((X.astype(np.float64) - U.astype(np.float64) @ V.astype(np.float64)) ** 2))
    return U, V, X, want

// Simplex-constrained KL update of H (nn_fac/update_rules/mu.py:161-175, utils/normalize_wh.py:24-58 at beta = 1): the
// per-column Newton solve for the Lagrange multipliers and the update that uses them (nnf_simplex_proj_kl_f32).
//
// Layout (k_simplex_plan.h): G lanes per column, lane q of a group owns the rows k = q, q + G, ...; its share of H, C (num) and
// D (den, or the per-row den_vec staged once per workgroup in LDS) sits in registers as fp64 for the whole call, nothing is
// re-read per iteration.  The two sums over k of an iteration are the lane's own rows in row order, then an xor butterfly over
// the group: every lane of a group ends up with the same bits and forms the same multiplier.
//
// The reference stops ALL columns at the first iteration whose largest |lambda - lambda_prev| over the columns is <= tol.
// Columns do not otherwise depend on each other, so the solve is two stream-ordered launches of the same kernel and nothing in
// either waits for another workgroup:
//   phase 0  every column iterates; max_j |dlambda_j| of iteration t is folded into slot t of a max_iter-slot array in the
//            context workspace (zeroed in stream order first): per wave a shuffle maximum, per workgroup an LDS maximum, then
//            one 64-bit unsigned atomic maximum per non-zero slot on the BITS of the non-negative double -- their order is the
//            order of the values, and a NaN's bits lie above infinity's, so that a slot holding NaN fails "<= tol" as np.max
//            does.  A wave leaves early once every one of its columns has a step of exactly 0 (every later step is 0 too) or
//            of NaN (it stays NaN: recorded as "NaN from iteration t on" in one more word, an atomic maximum of max_iter - t).
//   phase 1  every workgroup reads the slots, takes the reference's iteration count (first t with slot[t] <= tol, else
//            max_iter), re-runs exactly that many iterations through the same step function -- the same bits, nothing depends on
//            the other columns -- and applies mu.py:172-173.
// Every loop is bounded by max_iter; a grid that is not fully resident can only be slow.
#include "nnf_internal.h"
#include "k_simplex_plan.h"

// the reference's statements as they stand: products and sums are rounded one by one, as NumPy rounds them
#pragma clang fp contract(off)

NNF_BUILD_FLAGS(k_simplex, "SIMPLEX_BLOCK=" NNF_STR(SIMPLEX_BLOCK) " SIMPLEX_ROWS_PER_LANE=" NNF_STR(SIMPLEX_ROWS_PER_LANE))

namespace {

typedef unsigned long long u64;

template <int G>
__device__ __forceinline__ double simplex_group_sum(double v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// one iteration of normalize_wh.py:33-50 for the column this lane's group owns (beta = 1); `nrows`: rows this lane holds
template <int G, int RPL>
__device__ __forceinline__ double simplex_newton_step(const double (&h)[RPL], const double (&c)[RPL], const double (&d)[RPL], int nrows,
                                                      double lam) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        const double den = d[i] - lam;
        const double mat = h[i] * (c[i] / (den + 1e-8));    // :35
        const double matp = h[i] * (c[i] / (den * den));    // :36  (no eps in this denominator)
        if (i < nrows) {
            s1 += mat;
            s2 += matp;
        }
    }
    s1 = simplex_group_sum<G>(s1);                          // :46, :48
    s2 = simplex_group_sum<G>(s2);
    return lam - (s1 - 1.0) / (s2 + 1e-8);                  // :47, :50
}

template <int G, int RPL, bool MAT>
__global__ __launch_bounds__(SIMPLEX_BLOCK) void nnf_simplex_kernel(int phase, const float* H, int64_t ldh, int r, int64_t cols,
                                                                    const float* num, int64_t ldnum, const float* den, int64_t ldden,
                                                                    const double* den_vec, const double* lambda0, double tol,
                                                                    int max_iter, u64* slots, float* H_out, int64_t ldo,
                                                                    double* lambda_out, double* status) {
    __shared__ double s_dv[NNF_MAX_RANK];
    __shared__ u64 s_max[SIMPLEX_MAX_ITER];
    __shared__ u64 s_nan;
    __shared__ int s_run;
    const int tid = threadIdx.x, lane = tid & 63, q = tid % G;
    const int64_t j = (int64_t)blockIdx.x * (SIMPLEX_BLOCK / G) + tid / G;
    const bool valid = j < cols;
    const int nrows = (valid && q < r) ? (r - q + G - 1) / G : 0;

    if (!MAT)
        for (int k = tid; k < r; k += SIMPLEX_BLOCK) s_dv[k] = den_vec[k];
    if (phase == 0) {
        for (int t = tid; t < max_iter; t += SIMPLEX_BLOCK) s_max[t] = 0;
        if (tid == 0) s_nan = 0;
    } else if (tid == 0) {
        // the reference's count: the first iteration whose largest step is <= tol (a NaN step never is), else all of them
        const int nan_from = max_iter - (int)slots[max_iter];
        int n_run = max_iter;
        for (int t = 0; t < max_iter && t < nan_from; ++t)
            if (__builtin_bit_cast(double, slots[t]) <= tol) {
                n_run = t + 1;
                break;
            }
        s_run = n_run;
        if (blockIdx.x == 0) {
            status[0] = (double)n_run;
            status[1] = n_run - 1 >= nan_from ? __builtin_nan("") : __builtin_bit_cast(double, slots[n_run - 1]);
        }
    }
    __syncthreads();

    double h[RPL], c[RPL], d[RPL];
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        const int k = q + G * i;
        h[i] = c[i] = 0.0;
        d[i] = 1.0;
        if (i < nrows) {
            h[i] = (double)H[(int64_t)k * ldh + j];
            c[i] = (double)num[(int64_t)k * ldnum + j];
            d[i] = MAT ? (double)den[(int64_t)k * ldden + j] : s_dv[k];
        }
    }
    // mu.py:168 at beta = 1: D[0,:] - C[0,:] * H[0,:], formed by the lane that owns row 0
    double lam = lambda0 != nullptr ? (valid ? lambda0[j] : 0.0) : __shfl(d[0] - c[0] * h[0], lane & ~(G - 1), 64);

    if (phase == 0) {
        bool done = !valid, nan_seen = false;
        for (int t = 0; t < max_iter; ++t) {
            const double nl = simplex_newton_step<G, RPL>(h, c, d, nrows, lam);
            const double dl = fabs(nl - lam);
            lam = nl;
            const bool isnan_dl = valid && dl != dl;
            u64 b = valid ? __builtin_bit_cast(u64, dl) : 0;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const u64 o = __shfl_xor(b, m, 64);
                b = o > b ? o : b;
            }
            if (lane == 0 && b != 0) atomicMax(&s_max[t], b);
            if (!nan_seen && __any(isnan_dl)) {
                nan_seen = true;
                if (lane == 0) atomicMax(&s_nan, (u64)(max_iter - t));
            }
            done = done || dl == 0.0 || isnan_dl;
            if (__all(done)) break;
        }
        __syncthreads();
        for (int t = tid; t < max_iter; t += SIMPLEX_BLOCK)
            if (s_max[t] != 0) atomicMax(&slots[t], s_max[t]);
        if (tid == 0 && s_nan != 0) atomicMax(&slots[max_iter], s_nan);
        return;
    }

    const int n_run = s_run;
    for (int t = 0; t < n_run; ++t) lam = simplex_newton_step<G, RPL>(h, c, d, nrows, lam);
    if (lambda_out != nullptr && valid && q == 0) lambda_out[j] = lam;
    if (H_out != nullptr) {
#pragma unroll
        for (int i = 0; i < RPL; ++i) {
            if (i < nrows) {
                const double v = h[i] * (c[i] / ((d[i] - lam) + 1e-12));             // mu.py:172
                H_out[(int64_t)(q + G * i) * ldo + j] = (float)(v < 1e-12 ? 1e-12 : v);   // :173 (a NaN stays a NaN, as np.maximum keeps it)
            }
        }
    }
}

// NNF_SIMPLEX_FORCE=1|4|16|64 pins the lanes per column (tests run every instance on the same operands); read on every call:
// the tests change it inside one process.  -1: a value that is none of the four.
int simplex_force() {
    const char* e = getenv("NNF_SIMPLEX_FORCE");
    if (!e || !*e) return 0;
    const int v = atoi(e);
    return (v == 1 || v == 4 || v == 16 || v == 64) ? v : -1;
}

template <int G, int RPL>
void simplex_launch(int phase, const simplex_plan& p, hipStream_t st, const float* H, int64_t ldh, int r, int64_t cols, const float* num,
                    int64_t ldnum, const float* den, int64_t ldden, const double* den_vec, const double* lambda0, double tol, int max_iter,
                    u64* slots, float* H_out, int64_t ldo, double* lambda_out, double* status) {
    if (den != nullptr)
        hipLaunchKernelGGL((nnf_simplex_kernel<G, RPL, true>), dim3((unsigned)p.grid), dim3(SIMPLEX_BLOCK), 0, st, phase, H, ldh, r, cols, num,
                           ldnum, den, ldden, den_vec, lambda0, tol, max_iter, slots, H_out, ldo, lambda_out, status);
    else
        hipLaunchKernelGGL((nnf_simplex_kernel<G, RPL, false>), dim3((unsigned)p.grid), dim3(SIMPLEX_BLOCK), 0, st, phase, H, ldh, r, cols, num,
                           ldnum, den, ldden, den_vec, lambda0, tol, max_iter, slots, H_out, ldo, lambda_out, status);
}

}   // namespace

extern "C" int nnf_simplex_proj_kl_f32(nnf_ctx* ctx, const float* H, int64_t ldh, int r, int64_t cols, const float* num, int64_t ldnum,
                                       const float* den, int64_t ldden, const double* den_vec_f64, const double* lambda0_f64, double tol,
                                       int max_iter, float* H_out, int64_t ldo, double* lambda_out_f64, double* status_f64, void* stream) {
    if (!ctx || !H || !num || !status_f64 || r < 1 || cols < 1 || ldh < cols || ldnum < cols) return NNF_ERR_ARG;
    if ((den != nullptr) == (den_vec_f64 != nullptr)) return NNF_ERR_ARG;      // exactly one of the two
    if ((den != nullptr && ldden < cols) || (H_out != nullptr && ldo < cols)) return NNF_ERR_ARG;
    const int force = simplex_force();
    if (force < 0) return NNF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    nnf_ws_cursor cur(ctx);
    const simplex_plan p = simplex_make_plan(ctx->num_cus, r, cols, max_iter, force, cur.remaining());
    if (p.status != NNF_OK) return p.status;
    if (nnf_plan_debug()) simplex_report(stderr, r, cols, max_iter, den != nullptr, p);
    u64* slots = (u64*)cur.take(p.ws_bytes);
    if (!slots) return NNF_ERR_WORKSPACE;
    if (hipMemsetAsync(slots, 0, p.ws_bytes, st) != hipSuccess) return NNF_ERR_LAUNCH;
    for (int phase = 0; phase < 2; ++phase) {
#define SIMPLEX_CASE(G_, RPL_)                                                                                                          \
    if (p.G == G_ && p.rpl == RPL_)                                                                                                     \
        simplex_launch<G_, RPL_>(phase, p, st, H, ldh, r, cols, num, ldnum, den, ldden, den_vec_f64, lambda0_f64, tol, max_iter, slots, \
                                 H_out, ldo, lambda_out_f64, status_f64);
        SIMPLEX_CASE(1, 1) SIMPLEX_CASE(1, 2) SIMPLEX_CASE(1, 4) SIMPLEX_CASE(1, 8)
        SIMPLEX_CASE(4, 1) SIMPLEX_CASE(4, 2) SIMPLEX_CASE(4, 4) SIMPLEX_CASE(4, 8)
        SIMPLEX_CASE(16, 1) SIMPLEX_CASE(16, 2) SIMPLEX_CASE(16, 4) SIMPLEX_CASE(16, 8)
        SIMPLEX_CASE(64, 1) SIMPLEX_CASE(64, 2)
#undef SIMPLEX_CASE
        NNF_CHECK_LAUNCH();
    }
    return NNF_OK;
}

// NMF and NTF with MISSING entries: the MU sums of any beta >= 0 over the stored (= observed) entries only (include/nnfac_hip.h:
// nnf_csr_obs_f32, nnf_sptensor_obs_f32).  Decomposition, lanes per entry, entries in flight and workspace: k_sparse_plan.h
// (sparse_obs_make_plan: the CSR / sparse-tensor plan with two workspace arrays).
//
//   nnf_sparse_obs_kernel<L, NG, FORM>   the gather kernels of k_sparse.hip (NG = 1: colidx is index plane 0) and k_sptensor.hip
//                                      (NG = 2 .. 4) in their KL form, with two sums per chunk instead of one.  One wave per chunk
//                                      of at most CH entries of one slice, lane (g, l) takes the entries first + g, first + g + G,
//                                      ... and the components 4 l .. 4 l + 3; per entry it reads the NG indices, then one 16-byte
//                                      piece of each gathered row, U entries in flight.  h = (F_0 .* F_1) .* ... in fp32 in mode
//                                      order; p = <Own_n[i, :], h> as the lane's four products in index order and the fixed xor
//                                      tree over the L lanes -- ONCE per entry; from it the two weights
//                                          wn = x p^(beta - 2)   and   wd = p^(beta - 1)
//                                      and the two FMA chains num = fmaf(wn, h, num), den = fmaf(wd, h, den) in entry order.  The G
//                                      groups are added in the fixed xor tree and the chunk's two rows go to row `chunk` of two
//                                      node-major workspace arrays with plain 16-byte stores.  beta is a wave-uniform run-time
//                                      argument: 0, 1, 2 and 3 are multiplications and divisions, every other beta goes through
//                                      sparse_obs_pow (k_sparse_obs_pow.h).  The cost terms d_beta(x | p) are fp64 in lane l = 0
//                                      from the fp32 p, added over the wave and then over the workgroup's four waves in wave
//                                      order.
//   nnf_csr_rowsum_kernel              (k_sparse.hip, through nnf_csr_rowsum_launch) adds a slice's chunks in chunk order in fp64,
//                                      once per array.  A slice without stored entries owns no chunk: its num and den are 0.
//
// A stored 0 is an OBSERVED zero: it adds nothing to num (also where p^(beta - 2) is infinite), its full term to den (h itself
// at beta = 1) and d_beta(0 | p) to the cost -- p at beta = 1 and +inf at beta = 0, as nnf_betadiv_f32 has it for a zero entry,
// p^beta / beta otherwise.  NaN / Inf in vals or the factors reach the sums of their slice and the cost.
//
// An index outside its factor's extent drops the entry: whatever the tables hold, no load leaves the arrays.  Padding columns
// (r .. ldn) are read and masked.
#include "k_sparse_common.h"
#include "k_sparse_obs_pow.h"

namespace {

enum { OBS_SUMS = 1, OBS_COST = 2, OBS_BOTH = 3 };
enum { OBS_B0 = 0, OBS_B1 = 1, OBS_B2 = 2, OBS_B3 = 3, OBS_BGEN = 4 };      // how the weights are formed: wave-uniform

constexpr int OBS_NG_MAX = SPTENSOR_NG_MAX;
constexpr int obs_unroll(int L, int ng) { return ng == 1 ? sparse_unroll(L) : sptensor_unroll(L, ng); }

struct obs_ops {      // the gathered factors, in increasing mode order (a matrix: the one gathered factor)
    const float* F[OBS_NG_MAX];
    int64_t ext[OBS_NG_MAX];
};

struct obs_copy {      // one mode's sorted copy (a matrix: its CSR) and its chunk table
    const int64_t* ptr;
    const int* idx;
    const float* vals;
    int64_t nrows, nnz;
    const int64_t* rowchunk;
    const int* chunk_row;
    int64_t nchunks;
    int ch;
};

// d_beta(x | p) in fp64 (beta_divergence.py:45-52 per entry); x = 0: p at beta = 1, +inf at beta = 0 (-log 0).  No contraction
// of a product and a sum into an FMA in here: which ones the compiler fuses differs from one kernel instance to the next, and the
// three forms must give the same bits.
__device__ __forceinline__ double obs_cost_term(int bc, double beta, double x, double p) {
#pragma clang fp contract(off)
    if (bc == OBS_B2) {
        const double d = x - p;
        return 0.5 * d * d;
    }
    if (bc == OBS_B1) return x == 0.0 ? p : x * log(x / p) - x + p;
    if (bc == OBS_B0) {
        const double q = x / p;
        return q - log(q) - 1.0;
    }
    if (bc == OBS_B3) return (x * x * x + 2.0 * p * p * p - 3.0 * x * p * p) * (1.0 / 6.0);
    const double pb1 = exp((beta - 1.0) * log(p));                   // p^(beta - 1)
    const double xb = x == 0.0 ? 0.0 : exp(beta * log(x));           // (beta > 0 here: 0^beta = 0)
    return (xb + (beta - 1.0) * pb1 * p - beta * x * pb1) / (beta * (beta - 1.0));
}

template <int L, int NG, int FORM>
__global__ __launch_bounds__(SPARSE_BLOCK, 4) void nnf_sparse_obs_kernel(const obs_copy S, const float* __restrict__ Own, int64_t ldown,
                                                                      const obs_ops ops, int64_t ldn, int r, int bc, double beta,
                                                                      float* __restrict__ part_num, float* __restrict__ part_den, int rp,
                                                                      double* __restrict__ costpart) {
    constexpr int G = 64 / L, U = obs_unroll(L, NG);
    constexpr bool SUMS = (FORM & OBS_SUMS) != 0, COST = (FORM & OBS_COST) != 0;
    __shared__ double red[SPARSE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane % L, g = lane / L;
    const int64_t c = (int64_t)blockIdx.x * SPARSE_WAVES + wave;
    const bool piece = 4 * l < rp;       // this lane owns a 16-byte piece of the row
    const float e2 = (float)beta - 2.f, e1 = (float)beta - 1.f;

    // the chunk's span: every index is checked against the arrays' extents (an inconsistent table costs wrong sums, no fault)
    int64_t row = -1;
    sparse_span sp{0, 0};
    if (c < S.nchunks) {
        row = S.chunk_row[c];
        if (row >= 0 && row < S.nrows) sp = sparse_chunk_span(S.ptr[row], S.ptr[row + 1], c - S.rowchunk[row], S.ch, S.nnz);
        else row = -1;
    }

    f32x4 own = {0.f, 0.f, 0.f, 0.f};
    bool keep[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) keep[t] = 4 * l + t < r;
    if (piece && row >= 0) {
        const f32x4 o = *reinterpret_cast<const f32x4*>(Own + row * ldown + 4 * l);
#pragma unroll
        for (int t = 0; t < 4; ++t) own[t] = keep[t] ? o[t] : 0.f;
    }

    f32x4 num = {0.f, 0.f, 0.f, 0.f}, den = {0.f, 0.f, 0.f, 0.f};
    double cost = 0.0;
    for (int64_t base = sp.first; base < sp.end; base += G * U) {       // (wave-uniform bounds: every lane runs every shuffle)
        bool ok[U];
        float x[U];
        f32x4 f[U][NG];
        float pm[U];      // the model at the trip's entries
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e = base + u * G + g;
            ok[u] = e < sp.end;
            x[u] = 0.f;
            int j[NG];
#pragma unroll
            for (int m = 0; m < NG; ++m) {
                f[u][m] = f32x4{0.f, 0.f, 0.f, 0.f};
                j[m] = 0;
            }
            if (ok[u]) {
                x[u] = S.vals[e];
#pragma unroll
                for (int m = 0; m < NG; ++m) {
                    j[m] = S.idx[(int64_t)m * S.nnz + e];
                    ok[u] = ok[u] && j[m] >= 0 && j[m] < ops.ext[m];
                }
                if (ok[u] && piece) {
#pragma unroll
                    for (int m = 0; m < NG; ++m) f[u][m] = *reinterpret_cast<const f32x4*>(ops.F[m] + (int64_t)j[m] * ldn + 4 * l);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            f32x4 h = f[u][0];
#pragma unroll
            for (int m = 1; m < NG; ++m) {
#pragma unroll
                for (int t = 0; t < 4; ++t) h[t] *= f[u][m][t];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) h[t] = keep[t] ? h[t] : 0.f;
            float p = own[0] * h[0];
            p = fmaf(own[1], h[1], p);
            p = fmaf(own[2], h[2], p);
            p = fmaf(own[3], h[3], p);
#pragma unroll
            for (int s = 1; s < L; s *= 2) p += __shfl_xor(p, s);
            if (ok[u]) {
                if (SUMS) {
                    float wn, wd;
                    if (bc == OBS_B2) {
                        wn = x[u];
                        wd = p;
                    } else if (bc == OBS_B1) {
                        wn = x[u] / p;
                        wd = 1.f;
                    } else if (bc == OBS_B0) {
                        wn = x[u] / (p * p);
                        wd = 1.f / p;
                    } else if (bc == OBS_B3) {
                        wn = x[u] * p;
                        wd = p * p;
                    } else {
                        wn = x[u] * sparse_obs_pow(p, e2);
                        wd = sparse_obs_pow(p, e1);
                    }
                    if (x[u] != 0.f) {      // an observed 0 adds nothing to the numerator; a NaN is not 0
#pragma unroll
                        for (int t = 0; t < 4; ++t) num[t] = fmaf(wn, h[t], num[t]);
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) den[t] = fmaf(wd, h[t], den[t]);
                }
            }
            pm[u] = p;
        }
        if (COST) {
            // the fp64 terms after the trip's sums, when the gathered pieces are dead, and one entry at a time: left alone, the
            // scheduler interleaves the U logarithms and exponentials with the FMA chains (138 registers in the form with both
            // outputs at L >= 16)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                asm volatile("" : "+v"(cost), "+v"(pm[u]));
                if (ok[u] && l == 0) cost += obs_cost_term(bc, beta, (double)x[u], (double)pm[u]);
            }
        }
    }

    if (SUMS) {
#pragma unroll
        for (int s = 32; s >= L; s /= 2) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                num[t] += __shfl_xor(num[t], s);
                den[t] += __shfl_xor(den[t], s);
            }
        }
        if (c < S.nchunks && g == 0 && piece) {
            *reinterpret_cast<f32x4*>(part_num + c * rp + 4 * l) = num;
            *reinterpret_cast<f32x4*>(part_den + c * rp + 4 * l) = den;
        }
    }
    if (COST) {
        cost = nnf_wave_sum_f64(cost);
        if (lane == 0) red[wave] = cost;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int w = 0; w < SPARSE_WAVES; ++w) s += red[w];
            costpart[blockIdx.x] = s;
        }
    }
}

struct obs_launch_args {
    const sparse_plan* p;
    hipStream_t st;
    obs_copy S;
    const float* Own;
    int64_t ldown;
    obs_ops ops;
    int64_t ldn;
    int r, bc;
    double beta;
    float *part_num, *part_den;
    double* costpart;
};

template <int NG, int FORM>
void obs_launch_ng(const obs_launch_args& a) {
#define OBS_CASE(L_)                                                                                                                 \
    case L_:                                                                                                                         \
        hipLaunchKernelGGL((nnf_sparse_obs_kernel<L_, NG, FORM>), dim3((unsigned)a.p->grid), dim3(SPARSE_BLOCK), 0, a.st, a.S, a.Own,    \
                           a.ldown, a.ops, a.ldn, a.r, a.bc, a.beta, a.part_num, a.part_den, a.p->rp, a.costpart);                    \
        break;
    switch (a.p->L) {
        OBS_CASE(1)
        OBS_CASE(2)
        OBS_CASE(4)
        OBS_CASE(8)
        OBS_CASE(16)
        OBS_CASE(32)
    }
#undef OBS_CASE
}

template <int FORM>
void obs_launch(int ng, const obs_launch_args& a) {
    if (ng == 1) obs_launch_ng<1, FORM>(a);
    else if (ng == 2) obs_launch_ng<2, FORM>(a);
    else if (ng == 3) obs_launch_ng<3, FORM>(a);
    else obs_launch_ng<4, FORM>(a);
}

// Both entries from here on: `ng` gathered factors of the copy S, every check of the KL entries made by the caller.
int obs_run(nnf_ctx* ctx, const char* what, const obs_copy& S, int ng, const obs_ops& ops, int64_t ldn, const float* Own_n, int64_t ldo_n,
            int r, double beta, float* num, int64_t ldnum, float* den, int64_t ldden, double* cost_f64, void* stream) {
    if (!Own_n || ldo_n < r || ldo_n % 4 != 0 || !nnf_aligned16(Own_n)) return NNF_ERR_ARG;
    if ((num == nullptr) != (den == nullptr) || (!num && !cost_f64)) return NNF_ERR_ARG;
    if (num && (ldnum < S.nrows || ldden < S.nrows)) return NNF_ERR_ARG;
    if (!(beta >= 0.0) || !(beta <= 1.7976931348623157e308)) return NNF_ERR_ARG;      // negative, NaN or infinite
    hipStream_t st = (hipStream_t)stream;
    nnf_ws_cursor cur(ctx);
    const sparse_plan p = sparse_obs_make_plan(r, ng, S.nrows, S.nchunks, num != nullptr, cost_f64 != nullptr, cur.remaining());
    if (p.status != NNF_OK) return p.status;
    if (nnf_plan_debug())
        sparse_report(stderr, what, r, S.nrows, S.nnz, S.nchunks, S.ch, p, ng == 1 ? " ng=1" : ng == 2 ? " ng=2" : ng == 3 ? " ng=3" : " ng=4");
    obs_launch_args a{&p, st, S, Own_n, ldo_n, ops, ldn, r, 0, beta, nullptr, nullptr, nullptr};
    a.bc = beta == 0.0 ? OBS_B0 : beta == 1.0 ? OBS_B1 : beta == 2.0 ? OBS_B2 : beta == 3.0 ? OBS_B3 : OBS_BGEN;
    if (S.nchunks > 0) {
        if (num && !(a.part_num = (float*)cur.take(p.part_bytes / 2))) return NNF_ERR_WORKSPACE;
        if (num && !(a.part_den = (float*)cur.take(p.part_bytes / 2))) return NNF_ERR_WORKSPACE;
        if (cost_f64 && !(a.costpart = (double*)cur.take(p.cost_bytes))) return NNF_ERR_WORKSPACE;
        if (num && cost_f64) obs_launch<OBS_BOTH>(ng, a);
        else if (num) obs_launch<OBS_SUMS>(ng, a);
        else obs_launch<OBS_COST>(ng, a);
        NNF_CHECK_LAUNCH();
    }
    if (cost_f64) {
        if (S.nchunks > 0) {
            const int rc = nnf_launch_sum_f64(a.costpart, p.grid, 1.0, cost_f64, st);
            if (rc != NNF_OK) return rc;
        } else if (hipMemsetAsync(cost_f64, 0, sizeof(double), st) != hipSuccess) {
            return NNF_ERR_LAUNCH;
        }
    }
    if (!num) return NNF_OK;
    const int rc = nnf_csr_rowsum_launch(p, st, a.part_num, S.rowchunk, S.nrows, S.nchunks, r, num, ldnum);
    if (rc != NNF_OK) return rc;
    return nnf_csr_rowsum_launch(p, st, a.part_den, S.rowchunk, S.nrows, S.nchunks, r, den, ldden);
}

}   // namespace

extern "C" int nnf_csr_obs_f32(nnf_ctx* ctx, const int64_t* rowptr, const int32_t* colidx, const float* vals, int64_t nrows, int64_t ncols,
                               int64_t nnz, const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, const float* Own_n,
                               int64_t ldo_n, const float* Fn, int64_t ldn, int r, double beta, float* num, int64_t ldnum, float* den,
                               int64_t ldden, double* cost_f64, void* stream) {
    const int bad = nnf_csr_args_ok(ctx, rowptr, colidx, vals, nrows, ncols, nnz, rowchunk, chunk_row, nchunks, ch, Fn, ldn, r);
    if (bad != NNF_OK) return bad;
    const obs_copy S{rowptr, colidx, vals, nrows, nnz, rowchunk, chunk_row, nchunks, ch};
    const obs_ops ops{{Fn, nullptr, nullptr, nullptr}, {ncols, 0, 0, 0}};
    return obs_run(ctx, "csr_obs", S, 1, ops, ldn, Own_n, ldo_n, r, beta, num, ldnum, den, ldden, cost_f64, stream);
}

extern "C" int nnf_sptensor_obs_f32(nnf_ctx* ctx, const int64_t* ptr, const int32_t* idx, const float* vals, int64_t extent, int64_t nnz,
                                    const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, int ng,
                                    const float* const* Fn, const int64_t* extents, int64_t ldn, const float* Own_n, int64_t ldo_n, int r,
                                    double beta, float* num, int64_t ldnum, float* den, int64_t ldden, double* cost_f64, void* stream) {
    if (!Fn || !extents || ng < SPTENSOR_NG_MIN || ng > SPTENSOR_NG_MAX) return NNF_ERR_ARG;
    obs_ops ops{{nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0}};
    for (int m = 0; m < ng; ++m) {      // the CSR entries' checks on the mode's copy and every gathered factor
        const int bad = nnf_csr_args_ok(ctx, ptr, idx, vals, extent, extents[m], nnz, rowchunk, chunk_row, nchunks, ch, Fn[m], ldn, r);
        if (bad != NNF_OK) return bad;
        ops.F[m] = Fn[m];
        ops.ext[m] = extents[m];
    }
    if (extent > 2147483647) return NNF_ERR_UNSUPPORTED;
    const obs_copy S{ptr, idx, vals, extent, nnz, rowchunk, chunk_row, nchunks, ch};
    return obs_run(ctx, "sptensor_obs", S, ng, ops, ldn, Own_n, ldo_n, r, beta, num, ldnum, den, ldden, cost_f64, stream);
}

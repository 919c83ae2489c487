// NTF on sparse (COO) tensors: the two sums over the stored entries of one mode's sorted copy (include/nnfac_hip.h:
// nnf_sptensor_mttkrp_f32, nnf_sptensor_kl_f32).  Decomposition, lanes per entry, entries in flight and workspace:
// k_sparse_plan.h (the CSR plan with sptensor_unroll).
//
//   nnf_sptensor_gather_kernel<L, NG, MODE>   the CSR gather kernel (k_sparse.hip) with NG = N - 1 gathered rows per stored entry
//                                      instead of one: one wave per chunk of at most CH entries of one slice, lane (g, l) takes the
//                                      entries first + g, first + g + G, ... and the components 4 l .. 4 l + 3; per entry it reads
//                                      the NG indices idx[m][p] (planar, so that the G groups of a wave read consecutive words of
//                                      every plane), then one 16-byte piece of each row F_m[idx[m][p], :], U entries in flight.
//                                      h = (F_0 .* F_1) .* F_2 ... in fp32 in mode order, then acc = fmaf(x, h, acc) in entry
//                                      order; the G groups are added in the fixed xor tree and the chunk's r sums go to row
//                                      `chunk` of the node-major workspace with plain 16-byte stores.  KL: p = <Own_n[i, :], h> as
//                                      the lane's four products in index order and a fixed xor tree over the L lanes; q = x / p;
//                                      the cost terms are fp64 in lane l = 0, added over the wave and then over the workgroup's
//                                      four waves in wave order.
//   nnf_csr_rowsum_kernel              (k_sparse.hip, through nnf_csr_rowsum_launch) adds a slice's chunks in chunk order in fp64.
//
// An index outside its factor's extent drops the entry (as a column index outside [0, ncols) does in the CSR kernel): whatever
// the tables hold, no load leaves the arrays.  Padding columns (r .. ldn) are read and never used: the KL form masks them, the
// product form only lets them reach workspace columns that the second pass does not read.
#include "k_sparse_common.h"

namespace {

enum { SP_XF = 0, SP_KL_NUM = 1, SP_KL_COST = 2, SP_KL_BOTH = 3 };

struct sptensor_ops {      // the gathered factors, in increasing mode order
    const float* F[SPTENSOR_NG_MAX];
    int64_t ext[SPTENSOR_NG_MAX];
};

template <int L, int NG, int MODE>
__global__ __launch_bounds__(SPARSE_BLOCK) void nnf_sptensor_gather_kernel(
    const int64_t* __restrict__ ptr, const int* __restrict__ idx, const float* __restrict__ vals, int64_t nrows, int64_t nnz,
    const int64_t* __restrict__ rowchunk, const int* __restrict__ chunk_row, int64_t nchunks, int ch, const float* __restrict__ Own,
    int64_t ldown, const sptensor_ops ops, int64_t ldn, int r, float* __restrict__ part, int rp, double* __restrict__ costpart) {
    constexpr int G = 64 / L, U = sptensor_unroll(L, NG);
    constexpr bool KL = MODE != SP_XF, NUM = MODE != SP_KL_COST, COST = (MODE & SP_KL_COST) != 0;
    __shared__ double red[SPARSE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = lane % L, g = lane / L;
    const int64_t c = (int64_t)blockIdx.x * SPARSE_WAVES + wave;
    const bool piece = 4 * l < rp;       // this lane owns a 16-byte piece of the row

    // the chunk's span: every index is checked against the arrays' extents (an inconsistent table costs wrong sums, no fault)
    int64_t row = -1;
    sparse_span sp{0, 0};
    if (c < nchunks) {
        row = chunk_row[c];
        if (row >= 0 && row < nrows) sp = sparse_chunk_span(ptr[row], ptr[row + 1], c - rowchunk[row], ch, nnz);
        else row = -1;
    }

    f32x4 own = {0.f, 0.f, 0.f, 0.f};
    bool keep[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) keep[t] = 4 * l + t < r;
    if (KL && piece && row >= 0) {
        const f32x4 o = *reinterpret_cast<const f32x4*>(Own + row * ldown + 4 * l);
#pragma unroll
        for (int t = 0; t < 4; ++t) own[t] = keep[t] ? o[t] : 0.f;
    }

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    double cost = 0.0;
    for (int64_t base = sp.first; base < sp.end; base += G * U) {       // (wave-uniform bounds: every lane runs every shuffle)
        bool ok[U];
        float x[U];
        f32x4 f[U][NG];
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
                x[u] = vals[e];
#pragma unroll
                for (int m = 0; m < NG; ++m) {
                    j[m] = idx[(int64_t)m * nnz + e];
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
            if (!KL) {
                if (ok[u]) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = fmaf(x[u], h[t], acc[t]);
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) h[t] = keep[t] ? h[t] : 0.f;
                float p = own[0] * h[0];
                p = fmaf(own[1], h[1], p);
                p = fmaf(own[2], h[2], p);
                p = fmaf(own[3], h[3], p);
#pragma unroll
                for (int s = 1; s < L; s *= 2) p += __shfl_xor(p, s);
                if (ok[u] && x[u] != 0.f) {        // a stored 0 adds nothing to either sum (0 log 0 := 0); a NaN is not 0
                    const float q = x[u] / p;
                    if (NUM) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[t] = fmaf(q, h[t], acc[t]);
                    }
                    if (COST && l == 0) cost += (double)x[u] * log((double)x[u] / (double)p) - (double)x[u];
                }
            }
        }
    }

    if (NUM) {
#pragma unroll
        for (int s = 32; s >= L; s /= 2) {
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] += __shfl_xor(acc[t], s);
        }
        if (c < nchunks && g == 0 && piece) *reinterpret_cast<f32x4*>(part + c * rp + 4 * l) = acc;
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

struct sptensor_copy {      // one mode's sorted copy and its chunk table
    const int64_t* ptr;
    const int* idx;
    const float* vals;
    int64_t nrows, nnz;
    const int64_t* rowchunk;
    const int* chunk_row;
    int64_t nchunks;
    int ch;
};

template <int NG, int MODE>
void gather_launch_ng(const sparse_plan& p, hipStream_t st, const sptensor_copy& S, const float* Own, int64_t ldown, const sptensor_ops& ops,
                      int64_t ldn, int r, float* part, double* costpart) {
#define SPTENSOR_CASE(L_)                                                                                                            \
    case L_:                                                                                                                         \
        hipLaunchKernelGGL((nnf_sptensor_gather_kernel<L_, NG, MODE>), dim3((unsigned)p.grid), dim3(SPARSE_BLOCK), 0, st, S.ptr, S.idx, \
                           S.vals, S.nrows, S.nnz, S.rowchunk, S.chunk_row, S.nchunks, S.ch, Own, ldown, ops, ldn, r, part, p.rp,     \
                           costpart);                                                                                                \
        break;
    switch (p.L) {
        SPTENSOR_CASE(1)
        SPTENSOR_CASE(2)
        SPTENSOR_CASE(4)
        SPTENSOR_CASE(8)
        SPTENSOR_CASE(16)
        SPTENSOR_CASE(32)
    }
#undef SPTENSOR_CASE
}

template <int MODE>
void gather_launch(int ng, const sparse_plan& p, hipStream_t st, const sptensor_copy& S, const float* Own, int64_t ldown,
                   const sptensor_ops& ops, int64_t ldn, int r, float* part, double* costpart) {
    if (ng == 2) gather_launch_ng<2, MODE>(p, st, S, Own, ldown, ops, ldn, r, part, costpart);
    else if (ng == 3) gather_launch_ng<3, MODE>(p, st, S, Own, ldown, ops, ldn, r, part, costpart);
    else gather_launch_ng<4, MODE>(p, st, S, Own, ldown, ops, ldn, r, part, costpart);
}

// the checks both entries share: the CSR entries' (nnf_csr_args_ok) on the mode's copy and every gathered factor
int sptensor_args_ok(const nnf_ctx* ctx, const sptensor_copy& S, int ng, const float* const* Fn, const int64_t* extents, int64_t ldn, int r,
                     sptensor_ops& ops) {
    if (!Fn || !extents || ng < SPTENSOR_NG_MIN || ng > SPTENSOR_NG_MAX) return NNF_ERR_ARG;
    for (int m = 0; m < ng; ++m) {
        const int bad = nnf_csr_args_ok(ctx, S.ptr, S.idx, S.vals, S.nrows, extents[m], S.nnz, S.rowchunk, S.chunk_row, S.nchunks, S.ch,
                                        Fn[m], ldn, r);
        if (bad != NNF_OK) return bad;
        ops.F[m] = Fn[m];
        ops.ext[m] = extents[m];
    }
    for (int m = ng; m < SPTENSOR_NG_MAX; ++m) {
        ops.F[m] = nullptr;
        ops.ext[m] = 0;
    }
    if (S.nrows > 2147483647) return NNF_ERR_UNSUPPORTED;
    return NNF_OK;
}

}   // namespace

extern "C" int nnf_sptensor_mttkrp_f32(nnf_ctx* ctx, const int64_t* ptr, const int32_t* idx, const float* vals, int64_t extent, int64_t nnz,
                                       const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, int ng,
                                       const float* const* Fn, const int64_t* extents, int64_t ldn, int r, float* out, int64_t ldo,
                                       void* stream) {
    const sptensor_copy S{ptr, idx, vals, extent, nnz, rowchunk, chunk_row, nchunks, ch};
    sptensor_ops ops;
    const int bad = sptensor_args_ok(ctx, S, ng, Fn, extents, ldn, r, ops);
    if (bad != NNF_OK) return bad;
    if (!out || ldo < extent) return NNF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    nnf_ws_cursor cur(ctx);
    const sparse_plan p = sptensor_make_plan(r, ng, extent, nchunks, true, false, cur.remaining());
    if (p.status != NNF_OK) return p.status;
    if (nnf_plan_debug()) sparse_report(stderr, "sptensor_mttkrp", r, extent, nnz, nchunks, ch, p, ng == 2 ? " ng=2" : ng == 3 ? " ng=3" : " ng=4");
    float* part = nullptr;
    if (nchunks > 0) {
        part = (float*)cur.take(p.part_bytes);
        if (!part) return NNF_ERR_WORKSPACE;
        gather_launch<SP_XF>(ng, p, st, S, nullptr, 0, ops, ldn, r, part, nullptr);
        NNF_CHECK_LAUNCH();
    }
    return nnf_csr_rowsum_launch(p, st, part, rowchunk, extent, nchunks, r, out, ldo);
}

extern "C" int nnf_sptensor_kl_f32(nnf_ctx* ctx, const int64_t* ptr, const int32_t* idx, const float* vals, int64_t extent, int64_t nnz,
                                   const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, int ng,
                                   const float* const* Fn, const int64_t* extents, int64_t ldn, const float* Own_n, int64_t ldo_n, int r,
                                   float* num, int64_t ldnum, double* cost_f64, void* stream) {
    const sptensor_copy S{ptr, idx, vals, extent, nnz, rowchunk, chunk_row, nchunks, ch};
    sptensor_ops ops;
    const int bad = sptensor_args_ok(ctx, S, ng, Fn, extents, ldn, r, ops);
    if (bad != NNF_OK) return bad;
    if (!Own_n || ldo_n < r || ldo_n % 4 != 0 || !nnf_aligned16(Own_n)) return NNF_ERR_ARG;
    if ((!num && !cost_f64) || (num && ldnum < extent)) return NNF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    nnf_ws_cursor cur(ctx);
    const sparse_plan p = sptensor_make_plan(r, ng, extent, nchunks, num != nullptr, cost_f64 != nullptr, cur.remaining());
    if (p.status != NNF_OK) return p.status;
    if (nnf_plan_debug()) sparse_report(stderr, "sptensor_kl", r, extent, nnz, nchunks, ch, p, ng == 2 ? " ng=2" : ng == 3 ? " ng=3" : " ng=4");
    float* part = nullptr;
    double* costpart = nullptr;
    if (nchunks > 0) {
        if (num && !(part = (float*)cur.take(p.part_bytes))) return NNF_ERR_WORKSPACE;
        if (cost_f64 && !(costpart = (double*)cur.take(p.cost_bytes))) return NNF_ERR_WORKSPACE;
        if (num && cost_f64) gather_launch<SP_KL_BOTH>(ng, p, st, S, Own_n, ldo_n, ops, ldn, r, part, costpart);
        else if (num) gather_launch<SP_KL_NUM>(ng, p, st, S, Own_n, ldo_n, ops, ldn, r, part, costpart);
        else gather_launch<SP_KL_COST>(ng, p, st, S, Own_n, ldo_n, ops, ldn, r, part, costpart);
        NNF_CHECK_LAUNCH();
    }
    if (cost_f64) {
        if (nchunks > 0) {
            const int rc = nnf_launch_sum_f64(costpart, p.grid, 1.0, cost_f64, st);
            if (rc != NNF_OK) return rc;
        } else if (hipMemsetAsync(cost_f64, 0, sizeof(double), st) != hipSuccess) {
            return NNF_ERR_LAUNCH;
        }
    }
    return num ? nnf_csr_rowsum_launch(p, st, part, rowchunk, extent, nchunks, r, num, ldnum) : NNF_OK;
}

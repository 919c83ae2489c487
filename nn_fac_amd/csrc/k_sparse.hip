// NMF on CSR data: the two products of a factor with the stored entries only (include/nnfac_hip.h: nnf_csr_xf_f32,
// nnf_csr_kl_f32).  Decomposition, lanes per entry and workspace: k_sparse_plan.h.
//
//   nnf_csr_gather_kernel<L, MODE>     one wave per chunk of at most CH stored entries of one row.  Lane (g, l) of the wave takes the
//                                      entries first + g, first + g + G, ... (G = 64 / L) and the components 4 l .. 4 l + 3 of each
//                                      gathered row Fn[colidx[p], :]: one 16-byte load per lane and entry, U entries in flight per
//                                      lane.  fp32 FMAs per lane in entry order, then the G groups are added in a fixed xor tree,
//                                      and the chunk's r sums go to row `chunk` of the node-major workspace with plain 16-byte
//                                      stores.  KL: p = <Own_n[i, :], Fn[j, :]> is the lane's four products in index order and a
//                                      fixed xor tree over the L lanes; q = x / p; the cost terms are fp64 in lane l = 0, added
//                                      over the wave and then over the workgroup's four waves in wave order.
//   nnf_csr_rowsum_kernel              out[k, i] = the workspace rows of the chunks of row i, added in chunk order in fp64, rounded
//                                      once; 64 matrix rows per workgroup through an LDS tile, so that the workspace is read along
//                                      k and the component-major output written along i.  A row without chunks is 0.  A row of
//                                      more than SPARSE_LONG_ROW chunks is summed by the whole workgroup, segment by segment (one
//                                      thread walking 14823 chunks of the heaviest column of a 10^6 x 4000 power-law matrix took
//                                      20 ms, one dependent load each: DESIGN.md section 7).
//
// Why the node-major workspace and a second pass instead of an LDS-transposed tile in the gather kernel: a workgroup's four
// chunks belong to at most four rows, so a tile transposed there would still leave 4-byte stores r x nrows apart; the second
// pass is needed for split rows in any case, and it moves 8 r bytes per chunk against (8 + 4 ldn) bytes per stored entry.
//
// Padding columns (r .. ldn of a node-major operand) are read and never used: the KL form masks them, the product form only
// lets them reach workspace columns that the second pass does not read.
#include "k_sparse_common.h"

namespace {

enum { SP_XF = 0, SP_KL_NUM = 1, SP_KL_COST = 2, SP_KL_BOTH = 3 };

template <int L, int MODE>
__global__ __launch_bounds__(SPARSE_BLOCK) void nnf_csr_gather_kernel(
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx, const float* __restrict__ vals, int64_t nrows, int64_t ncols,
    int64_t nnz, const int64_t* __restrict__ rowchunk, const int* __restrict__ chunk_row, int64_t nchunks, int ch,
    const float* __restrict__ Own, int64_t ldown, const float* __restrict__ Fn, int64_t ldn, int r, float* __restrict__ part, int rp,
    double* __restrict__ costpart) {
    constexpr int G = 64 / L, U = sparse_unroll(L);
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
        if (row >= 0 && row < nrows) sp = sparse_chunk_span(rowptr[row], rowptr[row + 1], c - rowchunk[row], ch, nnz);
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
        f32x4 f[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t e = base + u * G + g;
            ok[u] = e < sp.end;
            x[u] = 0.f;
            f[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok[u]) {
                const int j = colidx[e];
                x[u] = vals[e];
                ok[u] = j >= 0 && j < ncols;
                if (ok[u] && piece) f[u] = *reinterpret_cast<const f32x4*>(Fn + (int64_t)j * ldn + 4 * l);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!KL) {
                if (ok[u]) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[t] = fmaf(x[u], f[u][t], acc[t]);
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) f[u][t] = keep[t] ? f[u][t] : 0.f;
                float p = own[0] * f[u][0];
                p = fmaf(own[1], f[u][1], p);
                p = fmaf(own[2], f[u][2], p);
                p = fmaf(own[3], f[u][3], p);
#pragma unroll
                for (int s = 1; s < L; s *= 2) p += __shfl_xor(p, s);
                if (ok[u] && x[u] != 0.f) {        // a stored 0 adds nothing to either sum (0 log 0 := 0); a NaN is not 0
                    const float q = x[u] / p;
                    if (NUM) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) acc[t] = fmaf(q, f[u][t], acc[t]);
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

__global__ __launch_bounds__(256) void nnf_csr_rowsum_kernel(const float* __restrict__ part, int rp, const int64_t* __restrict__ rowchunk,
                                                             int64_t nrows, int64_t nchunks, int r, float* __restrict__ out,
                                                             int64_t ldo) {
    extern __shared__ float tile[];      // SPARSE_TILE_ROWS x (rp + 1)
    __shared__ double seg[256 * 4];      // the segment sums of a long row
    const int64_t i0 = (int64_t)blockIdx.x * SPARSE_TILE_ROWS;
    const int pitch = rp + 1;
    // rows of at most SPARSE_LONG_ROW chunks: one thread per (row, k), chunks in order
    for (int idx = threadIdx.x; idx < SPARSE_TILE_ROWS * rp; idx += blockDim.x) {
        const int row = idx / rp, k = idx - row * rp;
        const int64_t i = i0 + row;
        float v = 0.f;
        if (i < nrows) {
            int64_t c0 = rowchunk[i], c1 = rowchunk[i + 1];
            if (c0 < 0) c0 = 0;
            if (c1 > nchunks) c1 = nchunks;
            if (c1 - c0 > SPARSE_LONG_ROW) continue;      // (summed by the whole workgroup below)
            if (c1 - c0 == 1) {
                v = part[c0 * rp + k];
            } else if (c1 > c0) {
                double s = 0.0;
#pragma unroll 4
                for (int64_t c = c0; c < c1; ++c) s += (double)part[c * rp + k];
                v = (float)s;
            }
        }
        tile[row * pitch + k] = v;
    }
    // a long row (the heavy columns of a term-document matrix: thousands of chunks) is summed by the whole workgroup: its chunk
    // list is cut into nseg contiguous segments, thread (s, q) adds the 16-byte piece q of the chunks of segment s in chunk
    // order, then the segments are added in segment order -- a fixed order that follows the chunk order block by block
    const int k4n = rp / 4, nseg = 256 / k4n;
    const int sq = threadIdx.x / k4n, q = threadIdx.x - sq * k4n;
    for (int row = 0; row < SPARSE_TILE_ROWS && i0 + row < nrows; ++row) {      // (block-uniform: the bounds depend on the row only)
        int64_t c0 = rowchunk[i0 + row], c1 = rowchunk[i0 + row + 1];
        if (c0 < 0) c0 = 0;
        if (c1 > nchunks) c1 = nchunks;
        if (c1 - c0 <= SPARSE_LONG_ROW) continue;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        if (sq < nseg) {
            const int64_t per = (c1 - c0 + nseg - 1) / nseg, cb = c0 + sq * per, ce = cb + per < c1 ? cb + per : c1;
#pragma unroll 4
            for (int64_t c = cb; c < ce; ++c) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(part + c * rp + 4 * q);
#pragma unroll
                for (int t = 0; t < 4; ++t) a[t] += (double)v[t];
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) seg[threadIdx.x * 4 + t] = a[t];
        __syncthreads();
        if (threadIdx.x < k4n) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                double s = 0.0;
                for (int g = 0; g < nseg; ++g) s += seg[(g * k4n + threadIdx.x) * 4 + t];
                tile[row * pitch + 4 * threadIdx.x + t] = (float)s;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < SPARSE_TILE_ROWS * r; idx += blockDim.x) {
        const int k = idx / SPARSE_TILE_ROWS, row = idx - k * SPARSE_TILE_ROWS;
        const int64_t i = i0 + row;
        if (i < nrows) out[(int64_t)k * ldo + i] = tile[row * pitch + k];
    }
}

template <int MODE>
void gather_launch(const sparse_plan& p, hipStream_t st, const int64_t* rowptr, const int* colidx, const float* vals, int64_t nrows,
                   int64_t ncols, int64_t nnz, const int64_t* rowchunk, const int* chunk_row, int64_t nchunks, int ch, const float* Own,
                   int64_t ldown, const float* Fn, int64_t ldn, int r, float* part, double* costpart) {
#define SPARSE_CASE(L_)                                                                                                              \
    case L_:                                                                                                                         \
        hipLaunchKernelGGL((nnf_csr_gather_kernel<L_, MODE>), dim3((unsigned)p.grid), dim3(SPARSE_BLOCK), 0, st, rowptr, colidx, vals,  \
                           nrows, ncols, nnz, rowchunk, chunk_row, nchunks, ch, Own, ldown, Fn, ldn, r, part, p.rp, costpart);       \
        break;
    switch (p.L) {
        SPARSE_CASE(1)
        SPARSE_CASE(2)
        SPARSE_CASE(4)
        SPARSE_CASE(8)
        SPARSE_CASE(16)
        SPARSE_CASE(32)
    }
#undef SPARSE_CASE
}

}   // namespace

// the checks both entries share (and those of k_sptensor.hip: k_sparse_common.h); `nnz`, `nchunks` and `ch` are the caller's word
// on the device tables (the kernels hold every index they read from them against these extents)
int nnf_csr_args_ok(const nnf_ctx* ctx, const void* rowptr, const void* colidx, const void* vals, int64_t nrows, int64_t ncols, int64_t nnz,
                    const void* rowchunk, const void* chunk_row, int64_t nchunks, int ch, const float* Fn, int64_t ldn, int r) {
    if (!ctx || !rowptr || !rowchunk || nrows < 1 || ncols < 1 || nnz < 0 || nchunks < 0 || !Fn || r < 1 || !sparse_chunk_ok(ch))
        return NNF_ERR_ARG;
    if (nnz > 0 && (!colidx || !vals)) return NNF_ERR_ARG;
    if (nchunks > 0 && !chunk_row) return NNF_ERR_ARG;
    if (nnz > 2147483647 || ncols > 2147483647) return NNF_ERR_UNSUPPORTED;
    if (r > NNF_MAX_RANK) return NNF_ERR_UNSUPPORTED;
    if (ldn < r || ldn % 4 != 0 || !nnf_aligned16(Fn)) return NNF_ERR_ARG;
    if (nchunks > nnz || nchunks * (int64_t)ch < nnz) return NNF_ERR_ARG;      // (no table of `ch`-chunks of nnz entries has that many)
    return NNF_OK;
}

int nnf_csr_rowsum_launch(const sparse_plan& p, hipStream_t st, const float* part, const int64_t* rowchunk, int64_t nrows, int64_t nchunks,
                          int r, float* out, int64_t ldo) {
    hipLaunchKernelGGL(nnf_csr_rowsum_kernel, dim3((unsigned)p.tgrid), dim3(256), p.lds_bytes, st, part, p.rp, rowchunk, nrows, nchunks, r,
                       out, ldo);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

extern "C" int nnf_csr_chunk_entries(nnf_ctx* ctx, int64_t nnz, int64_t* out) {
    if (!ctx || !out || nnz < 0) return NNF_ERR_ARG;
    static const char* force = getenv("NNF_SPARSE_CH");      // measurements (tools/sparse_bench.py): another chunk size
    const int forced = force ? atoi(force) : 0;
    if (force && !sparse_chunk_ok(forced)) return NNF_ERR_ARG;
    *out = force ? forced : sparse_chunk_entries(ctx->num_cus, nnz);
    return NNF_OK;
}

extern "C" int nnf_csr_xf_f32(nnf_ctx* ctx, const int64_t* rowptr, const int32_t* colidx, const float* vals, int64_t nrows, int64_t ncols,
                              int64_t nnz, const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, const float* Fn,
                              int64_t ldn, int r, float* out, int64_t ldo, void* stream) {
    const int bad = nnf_csr_args_ok(ctx, rowptr, colidx, vals, nrows, ncols, nnz, rowchunk, chunk_row, nchunks, ch, Fn, ldn, r);
    if (bad != NNF_OK) return bad;
    if (!out || ldo < nrows) return NNF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    nnf_ws_cursor cur(ctx);
    const sparse_plan p = sparse_make_plan(r, nrows, nchunks, true, false, cur.remaining());
    if (p.status != NNF_OK) return p.status;
    if (nnf_plan_debug()) sparse_report(stderr, "csr_xf", r, nrows, nnz, nchunks, ch, p);
    float* part = nullptr;
    if (nchunks > 0) {
        part = (float*)cur.take(p.part_bytes);
        if (!part) return NNF_ERR_WORKSPACE;
        gather_launch<SP_XF>(p, st, rowptr, colidx, vals, nrows, ncols, nnz, rowchunk, chunk_row, nchunks, ch, nullptr, 0, Fn, ldn, r, part,
                             nullptr);
        NNF_CHECK_LAUNCH();
    }
    return nnf_csr_rowsum_launch(p, st, part, rowchunk, nrows, nchunks, r, out, ldo);
}

extern "C" int nnf_csr_kl_f32(nnf_ctx* ctx, const int64_t* rowptr, const int32_t* colidx, const float* vals, int64_t nrows, int64_t ncols,
                              int64_t nnz, const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, const float* Own_n,
                              int64_t ldo_n, const float* Fn, int64_t ldn, int r, float* num, int64_t ldnum, double* cost_f64, void* stream) {
    const int bad = nnf_csr_args_ok(ctx, rowptr, colidx, vals, nrows, ncols, nnz, rowchunk, chunk_row, nchunks, ch, Fn, ldn, r);
    if (bad != NNF_OK) return bad;
    if (!Own_n || ldo_n < r || ldo_n % 4 != 0 || !nnf_aligned16(Own_n)) return NNF_ERR_ARG;
    if ((!num && !cost_f64) || (num && ldnum < nrows)) return NNF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    nnf_ws_cursor cur(ctx);
    const sparse_plan p = sparse_make_plan(r, nrows, nchunks, num != nullptr, cost_f64 != nullptr, cur.remaining());
    if (p.status != NNF_OK) return p.status;
    if (nnf_plan_debug()) sparse_report(stderr, "csr_kl", r, nrows, nnz, nchunks, ch, p);
    float* part = nullptr;
    double* costpart = nullptr;
    if (nchunks > 0) {
        if (num && !(part = (float*)cur.take(p.part_bytes))) return NNF_ERR_WORKSPACE;
        if (cost_f64 && !(costpart = (double*)cur.take(p.cost_bytes))) return NNF_ERR_WORKSPACE;
        if (num && cost_f64)
            gather_launch<SP_KL_BOTH>(p, st, rowptr, colidx, vals, nrows, ncols, nnz, rowchunk, chunk_row, nchunks, ch, Own_n, ldo_n, Fn, ldn,
                                      r, part, costpart);
        else if (num)
            gather_launch<SP_KL_NUM>(p, st, rowptr, colidx, vals, nrows, ncols, nnz, rowchunk, chunk_row, nchunks, ch, Own_n, ldo_n, Fn, ldn,
                                     r, part, costpart);
        else
            gather_launch<SP_KL_COST>(p, st, rowptr, colidx, vals, nrows, ncols, nnz, rowchunk, chunk_row, nchunks, ch, Own_n, ldo_n, Fn, ldn,
                                      r, part, costpart);
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
    return num ? nnf_csr_rowsum_launch(p, st, part, rowchunk, nrows, nchunks, r, num, ldnum) : NNF_OK;
}

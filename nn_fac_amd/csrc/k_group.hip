// Grouped kernels (gfx950): many small per-group problems in ONE launch each -- the K slices of nonnegative PARAFAC2
// (nn_fac/parafac2.py:509-600), whose per-slice operands are rank-sized while K runs to hundreds.
//
// A "group" g owns the columns [off[g], off[g+1]) of stacked r x (sum of lengths) operands; `off` is a DEVICE array of
// ngroups + 1 int64.  Nothing here exchanges anything between workgroups: no grid barrier, no flag in memory, no ticket.
//   nnf_hals_solve_group_f32   one workgroup = one group = one accelerated-HALS solve; its stopping rule is a workgroup sum
//   nnf_group_gram_f32         one workgroup = one group: A_g A_g^T, row dots against B, ||A_g - T_g||^2, fp64 sums
//   nnf_group_gemm_f32         out[:, seg g] = M_g A[:, seg g]
//   nnf_frob_resid_rows_f32    per-row ||x_i - u_i V||^2, model tile on the 16x16x4 fp32 MFMA, never stored
// Every sum has a fixed order (two calls are bitwise equal).  A segment table the kernels cannot trust (negative, decreasing,
// beyond `total_cols`, or a group longer than the caller declared) makes the group a no-op: nothing of it is read or written
// (the solve says so in its status block, NNF_HALS_ST_ERR = 5).
#include "k_hals_common.h"   // the stopping rule and the status block of a solve

#define GRP_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// group g's validated column range; false: skip the group
__device__ __forceinline__ bool grp_range(const int64_t* __restrict__ off, int g, int64_t total, int64_t maxlen, int64_t& lo,
                                          int64_t& hi) {
    lo = off[g];
    hi = off[g + 1];
    return lo >= 0 && hi >= lo && hi <= total && (maxlen <= 0 || hi - lo <= maxlen);
}

// ---------------------------------------------------------------------------------------------------------
// Grouped accelerated HALS.  128 threads, one column per thread and tile of 128 columns; the group's Gram image (padded to
// RP = r rounded up to 4, rows read as broadcast float4) and 1/diag live in LDS next to the tile's columns (vl[k][tid]: a
// thread touches its own column only, no synchronisation inside a sweep).  A group of at most 128 columns keeps its tile
// in LDS over all sweeps; a longer one walks its tiles every sweep, V read and written in place (the block of a group within
// the cap, r x NNF_HALS_GROUP_MAX_COLUMNS floats <= 4 MiB, stays in the L2 of the XCD).  Arithmetic of a row update = that of
// the generic kernel of k_hals.hip: fp32 dot in index order, fp32 step, squared steps summed in fp64.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void nnf_hals_group_kernel(const float* __restrict__ UtM, int64_t ldm,
                                                             const float* __restrict__ UtU, int64_t ldg, int64_t gstride,
                                                             float* __restrict__ V, int64_t ldv, int r, int RP,
                                                             const int64_t* __restrict__ off, int64_t maxlen, int64_t total,
                                                             int max_sweeps, double delta, double* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Gl = reinterpret_cast<float*>(smem);        // [RP][RP]
    float* dinv = Gl + (size_t)RP * RP;                 // [RP]
    float* vl = dinv + RP;                              // [RP][128]
    double* red = reinterpret_cast<double*>(vl + (size_t)RP * 128);   // [2]
    const int g = blockIdx.x, tid = threadIdx.x;
    double* st = status + (size_t)g * NNF_HALS_ST_WORDS;
    int64_t lo, hi;
    if (!grp_range(off, g, total, maxlen, lo, hi)) {
        if (tid == 0) hals_status_defaults(st, 5.0);
        return;
    }
    const float* Gg = UtU + (int64_t)g * gstride;
    for (int e = tid; e < RP * RP; e += 128) {
        const int a = e / RP, b = e - a * RP;
        Gl[e] = (a < r && b < r) ? Gg[(int64_t)a * ldg + b] : 0.f;
    }
    for (int k = tid; k < RP; k += 128) {
        const float d = (k < r) ? Gg[(int64_t)k * ldg + k] : 0.f;
        dinv[k] = (d != 0.f) ? (float)(1.0 / (double)d) : 0.f;      // 0: leave the row alone (nnls.py:161)
    }
    for (int k = r; k < RP; ++k) vl[k * 128 + tid] = 0.f;
    __syncthreads();

    const bool resident = (hi - lo) <= 128;
    if (resident) {
        const bool active = lo + tid < hi;
        for (int k = 0; k < r; ++k) vl[k * 128 + tid] = active ? V[(int64_t)k * ldv + lo + tid] : 0.f;
    }
    double eps0 = 0.0, eps = 1.0;
    int done = 0;
    for (int s = 1; s <= max_sweeps; ++s) {
        double nd = 0.0;
        for (int64_t c0 = lo; c0 < hi; c0 += 128) {
            const int64_t col = c0 + tid;
            const bool active = col < hi;
            const int64_t cc = active ? col : lo;
            if (!resident)
                for (int k = 0; k < r; ++k) vl[k * 128 + tid] = active ? V[(int64_t)k * ldv + cc] : 0.f;
            for (int k = 0; k < r; ++k) {
                const float di = dinv[k];
                if (di == 0.f) continue;
                const float4* gk = reinterpret_cast<const float4*>(Gl + (size_t)k * RP);
                float dot = 0.f;
                for (int i4 = 0; i4 < RP / 4; ++i4) {
                    const float4 gq = gk[i4];
                    const float* vv = vl + (size_t)(4 * i4) * 128 + tid;
                    dot = fmaf(gq.x, vv[0], dot);
                    dot = fmaf(gq.y, vv[128], dot);
                    dot = fmaf(gq.z, vv[256], dot);
                    dot = fmaf(gq.w, vv[384], dot);
                }
                const float vk = vl[k * 128 + tid];
                // np.maximum(x, -v), NaN included (nnls.py:167): fmaxf would drop a NaN of x, turn the group's V into clean
                // zeros and go on sweeping; kept, it makes the sum of squared steps NaN and the stopping rule below ends the group
                const float x = (UtM[(int64_t)k * ldm + cc] - dot) * di;
                float step = (x < -vk) ? -vk : x;
                if (!active) step = 0.f;
                vl[k * 128 + tid] = vk + step;
                nd += (double)step * (double)step;
            }
            if (!resident && active)
                for (int k = 0; k < r; ++k) V[(int64_t)k * ldv + col] = vl[k * 128 + tid];
        }
        // the group's sum of squared steps: lanes (fixed DPP tree), then the two waves in index order; every thread gets it
        nd = nnf_wave_sum_f64(nd);
        if ((tid & 63) == 0) red[tid >> 6] = nd;
        __syncthreads();
        const double tot = red[0] + red[1];
        __syncthreads();
        if (!hals_note_sum(tot, s, 0, delta, eps0, eps, done)) break;
    }
    if (resident && lo + tid < hi)
        for (int k = 0; k < r; ++k) V[(int64_t)k * ldv + lo + tid] = vl[k * 128 + tid];
    if (tid == 0) {   // (no prep launch: the defaults first, then the three words of a solve that ran over them)
        hals_status_defaults(st);
        hals_status_finish(st, max_sweeps >= 1, 0, done, eps, eps0, false);
    }
}

static size_t hals_group_lds(int RP) { return ((size_t)RP * RP + RP + (size_t)RP * 128) * 4 + 16; }

extern "C" int nnf_hals_group_max_columns(nnf_ctx* ctx, int r, int64_t* columns_out) {
    if (!ctx || r < 1 || !columns_out) return NNF_ERR_ARG;
    if (r > NNF_MAX_RANK) return NNF_ERR_UNSUPPORTED;
    *columns_out = NNF_HALS_GROUP_MAX_COLUMNS;
    return NNF_OK;
}

extern "C" int nnf_hals_solve_group_f32(nnf_ctx* ctx, const float* UtM, int64_t ldm, const float* UtU, int64_t ldg,
                                        int64_t gstride, float* V, int64_t ldv, int r, const int64_t* off, int ngroups,
                                        int64_t max_group_cols, int64_t total_cols, int max_sweeps, double delta,
                                        double* status_f64, void* stream) {
    if (!ctx || !UtM || !UtU || !V || !off || !status_f64 || r < 1 || ngroups < 1 || max_group_cols < 0 || total_cols < 0 ||
        max_sweeps < 0 || ldg < r || ldm < total_cols || ldv < total_cols || (ngroups > 1 && gstride < 1))
        return NNF_ERR_ARG;
    if (r > NNF_MAX_RANK || max_group_cols > NNF_HALS_GROUP_MAX_COLUMNS) return NNF_ERR_UNSUPPORTED;
    const int RP = (r + 3) & ~3;
    const size_t lds = hals_group_lds(RP);
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&nnf_hals_group_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)hals_group_lds(NNF_MAX_RANK)) != hipSuccess)
            return NNF_ERR_LAUNCH;
        raised = true;
    }
    hipLaunchKernelGGL(nnf_hals_group_kernel, dim3(ngroups), dim3(128), lds, (hipStream_t)stream, UtM, ldm, UtU, ldg, gstride, V,
                       ldv, r, RP, off, max_group_cols, total_cols, max_sweeps, delta, status_f64);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Grouped Gram / row dots / coupling error.  256 threads as a 16 x 16 grid; thread (ty, tx) keeps the NU x NU entries
// (ty + 16u, tx + 16v) of the group's Gram in fp64 over tiles of 32 columns staged in LDS (NU = 1, 2, 4, 8 for r <= 16, 32,
// 64, 128).  The dots are one wave per row (lanes stride the columns, DPP tree), the error one workgroup sum.
// ---------------------------------------------------------------------------------------------------------
template <int NU>
__global__ __launch_bounds__(256) void nnf_group_gram_kernel(const float* __restrict__ A, int64_t lda, int r,
                                                             const int64_t* __restrict__ off, int64_t total, float* __restrict__ G,
                                                             int64_t ldg, int64_t gstride, double* __restrict__ G64,
                                                             const float* __restrict__ B, int64_t ldb, double* __restrict__ dots, const float* __restrict__ T, int64_t ldt,
                                                             double* __restrict__ errs) {
    constexpr int TC = 32, ROWS = 16 * NU;
    __shared__ float tile[ROWS][TC + 1];
    __shared__ double red[4];
    const int g = blockIdx.x, tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    int64_t lo, hi;
    if (!grp_range(off, g, total, 0, lo, hi)) return;
    if (G) {
        double acc[NU][NU];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int v = 0; v < NU; ++v) acc[u][v] = 0.0;
        for (int64_t c0 = lo; c0 < hi; c0 += TC) {
            const int nc = (hi - c0 < TC) ? (int)(hi - c0) : TC;
            for (int e = tid; e < ROWS * TC; e += 256) {
                const int row = e / TC, c = e - row * TC;
                tile[row][c] = (row < r && c < nc) ? A[(int64_t)row * lda + c0 + c] : 0.f;
            }
            __syncthreads();
            for (int c = 0; c < nc; ++c) {
                double av[NU], bv[NU];
#pragma unroll
                for (int u = 0; u < NU; ++u) { av[u] = (double)tile[ty + 16 * u][c]; bv[u] = (double)tile[tx + 16 * u][c]; }
#pragma unroll
                for (int u = 0; u < NU; ++u)
#pragma unroll
                    for (int v = 0; v < NU; ++v) acc[u][v] = fma(av[u], bv[v], acc[u][v]);
            }
            __syncthreads();
        }
        float* Gg = G + (int64_t)g * gstride;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int v = 0; v < NU; ++v) {
                const int a = ty + 16 * u, b = tx + 16 * v;
                if (a < r && b < r) {
                    Gg[(int64_t)a * ldg + b] = (float)acc[u][v];
                    if (G64) G64[((int64_t)g * r + a) * r + b] = acc[u][v];      // the sums before their rounding to fp32
                }
            }
    }
    if (dots) {
        const int w = tid >> 6, lane = tid & 63;
        for (int q = w; q < r; q += 4) {                       // (wave-uniform trip count: every lane reaches the DPP sum)
            double s = 0.0;
            for (int64_t i = lo + lane; i < hi; i += 64)
                s = fma((double)A[(int64_t)q * lda + i], (double)B[(int64_t)q * ldb + i], s);
            s = nnf_wave_sum_f64(s);
            if (lane == 0) dots[(int64_t)g * r + q] = s;
        }
    }
    if (errs) {
        double e = 0.0;
        for (int q = 0; q < r; ++q)
            for (int64_t i = lo + tid; i < hi; i += 256) {
                const double d = (double)A[(int64_t)q * lda + i] - (double)T[(int64_t)q * ldt + i];
                e = fma(d, d, e);
            }
        e = nnf_block_sum_f64(e, red);
        if (tid == 0) errs[g] = e;
    }
}

extern "C" int nnf_group_gram_f32(nnf_ctx* ctx, const float* A, int64_t lda, int r, const int64_t* off, int ngroups,
                                  int64_t total_cols, float* G, int64_t ldg, int64_t gstride, double* G64, const float* B,
                                  int64_t ldb, double* dots_f64, const float* T, int64_t ldt, double* err_f64, void* stream) {
    if (!ctx || !A || !off || r < 1 || ngroups < 1 || total_cols < 0 || lda < total_cols || (!G && !dots_f64 && !err_f64) ||
        (G && (ldg < r || (ngroups > 1 && gstride < 1))) || (G64 && !G) || (dots_f64 && (!B || ldb < total_cols)) ||
        (err_f64 && (!T || ldt < total_cols)))
        return NNF_ERR_ARG;
    if (r > NNF_MAX_RANK) return NNF_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
#define GRP_GRAM(NU)                                                                                                          \
    hipLaunchKernelGGL(nnf_group_gram_kernel<NU>, dim3(ngroups), dim3(256), 0, st, A, lda, r, off, total_cols, G, ldg, gstride, G64, \
                       B, ldb, dots_f64, T, ldt, err_f64)
    if (r <= 16) GRP_GRAM(1);
    else if (r <= 32) GRP_GRAM(2);
    else if (r <= 64) GRP_GRAM(4);
    else GRP_GRAM(8);
#undef GRP_GRAM
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Grouped rank-sized product.  Workgroup (g, y): M_g (p x q) in LDS, tiles of 64 columns of the group (y, y + gridDim.y, ...)
// staged in LDS; wave w forms the output rows w, w + 4, ... of the tile, lane = column.  fp32 FMAs in index order.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nnf_group_gemm_kernel(const float* __restrict__ M, int64_t ldm, int64_t mstride, int p, int q,
                                                             const float* __restrict__ A, int64_t lda,
                                                             const int64_t* __restrict__ off, int64_t total,
                                                             float* __restrict__ out, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Ml = reinterpret_cast<float*>(smem);      // [p][q]
    float* At = Ml + (size_t)p * q;                   // [q][64]
    const int g = blockIdx.x, tid = threadIdx.x, w = tid >> 6, c = tid & 63;
    int64_t lo, hi;
    if (!grp_range(off, g, total, 0, lo, hi)) return;
    if (lo + (int64_t)blockIdx.y * 64 >= hi) return;           // (uniform over the workgroup)
    const float* Mg = M + (int64_t)g * mstride;
    for (int e = tid; e < p * q; e += 256) {
        const int a = e / q, b = e - a * q;
        Ml[e] = Mg[(int64_t)a * ldm + b];
    }
    for (int64_t c0 = lo + (int64_t)blockIdx.y * 64; c0 < hi; c0 += (int64_t)gridDim.y * 64) {
        __syncthreads();
        for (int e = tid; e < q * 64; e += 256) {
            const int b = e >> 6, cc = e & 63;
            At[e] = (c0 + cc < hi) ? A[(int64_t)b * lda + c0 + cc] : 0.f;
        }
        __syncthreads();
        const int64_t col = c0 + c;
        for (int a = w; a < p; a += 4) {
            float acc = 0.f;
            for (int b = 0; b < q; ++b) acc = fmaf(Ml[a * q + b], At[b * 64 + c], acc);
            if (col < hi) out[(int64_t)a * ldo + col] = acc;
        }
    }
}

extern "C" int nnf_group_gemm_f32(nnf_ctx* ctx, const float* M, int64_t ldm, int64_t mstride, int p, int q, const float* A,
                                  int64_t lda, const int64_t* off, int ngroups, int64_t max_group_cols, int64_t total_cols,
                                  float* out, int64_t ldo, void* stream) {
    if (!ctx || !M || !A || !off || !out || p < 1 || q < 1 || ngroups < 1 || max_group_cols < 0 || total_cols < 0 || ldm < q ||
        (ngroups > 1 && mstride < 1) || lda < total_cols || ldo < total_cols || out == A)
        return NNF_ERR_ARG;
    if (p > NNF_MAX_RANK || q > NNF_MAX_RANK) return NNF_ERR_UNSUPPORTED;
    const size_t lds = ((size_t)p * q + (size_t)q * 64) * 4;
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&nnf_group_gemm_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (NNF_MAX_RANK * NNF_MAX_RANK + NNF_MAX_RANK * 64) * 4) != hipSuccess)
            return NNF_ERR_LAUNCH;
        raised = true;
    }
    int64_t gy = nnf_cdiv(max_group_cols > 0 ? max_group_cols : 1, 64);     // (a hint: longer groups stride their tiles)
    if (gy > 64) gy = 64;
    hipLaunchKernelGGL(nnf_group_gemm_kernel, dim3(ngroups, (int)gy), dim3(256), lds, (hipStream_t)stream, M, ldm, mstride, p, q, A,
                       lda, off, total_cols, out, ldo);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Per-row squared residuals.  Workgroup = 16 rows of X, 4 waves; wave w takes the 16-column tiles w, w + 4, ... of those
// rows: the 16 x 16 model tile is r/4 MFMAs (A operand: the rows' factor entries staged once in LDS, B operand: V from
// L2), the lane's four entries (rows 4*(lane/16) + j, column lane%16) are subtracted from X and squared into fp64.  Row sums:
// 16 lanes (xor tree), then the four waves in index order.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nnf_resid_rows_kernel(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                                             const float* __restrict__ Ut, int64_t ldu,
                                                             const float* __restrict__ V, int64_t ldv, int r, int R4,
                                                             double* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ul = reinterpret_cast<float*>(smem);       // [R4][16]
    __shared__ double part[4][16];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, li = l & 15, lk = l >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    for (int e = tid; e < R4 * 16; e += 256) {
        const int k = e >> 4, i = e & 15;
        ul[e] = (k < r && row0 + i < m) ? Ut[(int64_t)k * ldu + row0 + i] : 0.f;
    }
    __syncthreads();
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t ntiles = (n + 15) / 16;
    for (int64_t t = w; t < ntiles; t += 4) {
        const int64_t col = t * 16 + li;
        const bool cok = col < n;
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < R4; k0 += 4) {
            const int kk = k0 + lk;
            const float a = ul[kk * 16 + li];
            const float b = (cok && kk < r) ? V[(int64_t)kk * ldv + col] : 0.f;
            d = GRP_MFMA16(a, b, d);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = row0 + 4 * lk + j;
            if (cok && row < m) {
                const float diff = X[row * ldx + col] - d[j];
                acc[j] = fma((double)diff, (double)diff, acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double v = acc[j];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 8, 64);
        if (li == 0) part[w][4 * lk + j] = v;
    }
    __syncthreads();
    if (tid < 16 && row0 + tid < m) rows[row0 + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

extern "C" int nnf_frob_resid_rows_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut,
                                       int64_t ldu, const float* V, int64_t ldv, int r, double* rows_f64, void* stream) {
    if (!ctx || !X || !Ut || !V || !rows_f64 || m < 1 || n < 1 || r < 1 || ldx < n || ldu < m || ldv < n) return NNF_ERR_ARG;
    if (r > NNF_MAX_RANK) return NNF_ERR_UNSUPPORTED;
    const int R4 = (r + 3) & ~3;
    const int64_t grid = nnf_cdiv(m, 16);
    if (grid > 0x7fffffff) return NNF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nnf_resid_rows_kernel, dim3((unsigned)grid), dim3(256), (size_t)R4 * 16 * 4, (hipStream_t)stream, X, m, n, ldx,
                       Ut, ldu, V, ldv, r, R4, rows_f64);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

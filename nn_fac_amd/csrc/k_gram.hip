// The Gram G[r x r] = A[r x K] * A^T  (nmf.py:407,432; ntf.py:442-445) in four forms: split over K with one LDS image, the same
// in 64 x 64 blocks above rank 128, one workgroup for short factors, and the fp64 copy next to the fp32 result.  The design
// shared with W^T X, X H^T and the cost pass is described at the head of k_stream_common.h.
#include "k_gram_body.h"

// gram: slab[ks] = A[:, split ks] * A[:, split ks]^T -- the body lives in k_gram_body.h (shared with the cross-product riders)
template <int MT>
__global__ __launch_bounds__(256) void nnf_gram_kernel(const float* __restrict__ A, int r, int64_t K, int64_t lda,
                                                       float* __restrict__ slabs, int64_t k_per_split, int a_vec_ok) {
    __shared__ f32x4 ldsA[2][MT * 256];
    nnf_gram_body<MT>(A, r, K, lda, slabs, k_per_split, a_vec_ok, (int)blockIdx.x, ldsA);
}

// Short factors (the I_mode x R factors of NTF / NTD: K <= 1024, r <= 64): one workgroup of eight waves, wave w owns the
// k range [w*kpw, (w+1)*kpw) and reads its operand fragments straight from global memory -- ALL of a wave's loads are in
// flight at once, so the kernel is one memory round trip + <= 128 MFMAs + one LDS reduction in fixed wave order.  (The
// chunked kernel above walks K in 64-wide LDS-staged chunks: eight dependent round trips for K = 500, 9 us of a 0.5 ms NTF
// iteration three times over.)  Both MFMA operands are the same registers: lane (i = l&15, g = l>>4) holds
// A[16*mt + i][k0 + 4g .. +3]; component c of every lane contracts k0 + 4g + c over g, the four components cover 16 k's.
template <int MT, int KS>
__global__ __launch_bounds__(512) void nnf_gram_small_kernel(const float* __restrict__ A, int r, int K, int64_t lda,
                                                             float* __restrict__ G) {
    __shared__ f32x4 red[4][MT * MT][64];   // 64 KB at MT = 4
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ii = lane & 15, g = lane >> 4;
    const int kw = w * (16 * KS);
    f32x4 fr[KS][MT];
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int row = 16 * mt + ii, k = kw + 16 * s + 4 * g;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < r && k < K) {   // K % 4 == 0 (vector path only): a lane's four k's are in or out together
                v = *reinterpret_cast<const f32x4*>(A + (int64_t)row * lda + k);
            }
            fr[s][mt] = v;
        }
    f32x4 acc[MT][MT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int b = 0; b < MT; ++b) acc[a][b] = MFMA16(fr[s][a][c], fr[s][b][c], acc[a][b]);
    // fixed order: wave w + 4 is added to wave w, then the four sums in order 0..3
    if (w >= 4) {
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < MT; ++b) red[w - 4][a * MT + b][lane] = acc[a][b];
    }
    __syncthreads();
    if (w < 4) {
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                const f32x4 x = red[w][a * MT + b][lane];
                f32x4 y = acc[a][b];
                y[0] += x[0]; y[1] += x[1]; y[2] += x[2]; y[3] += x[3];
                red[w][a * MT + b][lane] = y;
            }
    }
    __syncthreads();
    // tile (a, b), lane l, register reg  <->  G[16a + 4(l>>4) + reg][16b + (l&15)]
    for (int e = threadIdx.x; e < MT * MT * 64; e += 512) {
        const int t = e >> 6, l = e & 63;
        f32x4 s = red[0][t][l];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) {
            const f32x4 x = red[ww][t][l];
            s[0] += x[0]; s[1] += x[1]; s[2] += x[2]; s[3] += x[3];
        }
        const int a = t / MT, b = t - a * MT, col = 16 * b + (l & 15);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 16 * a + 4 * (l >> 4) + reg;
            if (row < r && col < r) G[row * r + col] = s[reg];
        }
    }
}

template <int MT>
static int launch_gram_small(const float* A, int r, int64_t K, int64_t lda, float* G, hipStream_t st) {
    // 16-wide k steps per wave (8 waves)
    return nnf_dispatch<8>((int)nnf_cdiv(K, 128), [&](auto ks) -> int {
        hipLaunchKernelGGL((nnf_gram_small_kernel<MT, decltype(ks)::value>), dim3(1), dim3(512), 0, st, A, r, (int)K, lda, G);
        NNF_CHECK_LAUNCH();
        return NNF_OK;
    });
}

// G64[a][b] = (double)G[a][b]: the fp64 copy of a Gram that was formed without slabs (K <= 1024: one workgroup)
__global__ void nnf_gram_widen_kernel(const float* __restrict__ G, int64_t ldg, int r, double* __restrict__ G64) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < r * r) G64[e] = (double)G[(int64_t)(e / r) * ldg + (e % r)];
}
static int launch_gram_widen(const float* G, int64_t ldg, int r, double* G64, hipStream_t st) {
    if (!G64) return NNF_OK;
    hipLaunchKernelGGL(nnf_gram_widen_kernel, dim3((r * r + 255) / 256), dim3(256), 0, st, G, ldg, r, G64);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// plan (nnf_plan_gram, k_stream_plan.h; a refusal launches nothing), report, carve, launch, reduce
template <int MT>
static int launch_gram(nnf_ctx* ctx, nnf_ws_cursor& cur, const float* A, int r, int64_t K, int64_t lda, float* G, int64_t ldg,
                       hipStream_t st, double* G64) {
    const int a_vec_ok = x_vec_ok(A, lda) ? 1 : 0;
    const nnf_gram_plan pl = nnf_plan_gram(ctx->num_cus, r, K, ldg == r, a_vec_ok, cur.remaining());
    if (pl.status != NNF_OK) return pl.status;
    if (nnf_plan_debug()) nnf_report_gram(stderr, r, K, pl);
    if constexpr (MT <= 4) {
        if (pl.form == NNF_GRAM_SMALL) {
            const int rc = launch_gram_small<MT>(A, r, K, lda, G, st);
            return rc != NNF_OK ? rc : launch_gram_widen(G, ldg, r, G64, st);
        }
    }
    if (pl.form == NNF_GRAM_SINGLE) {
        hipLaunchKernelGGL((nnf_gram_kernel<MT>), dim3(1), dim3(256), 0, st, A, r, K, lda, G, pl.kps, a_vec_ok);
        NNF_CHECK_LAUNCH();
        return launch_gram_widen(G, ldg, r, G64, st);
    }
    float* slabs = (float*)cur.take((size_t)pl.nsplit * r * r * 4);
    if (!slabs) return NNF_ERR_WORKSPACE;   // (the plan caps the slabs to the workspace only where it raised their number)
    hipLaunchKernelGGL((nnf_gram_kernel<MT>), dim3((int)pl.nsplit), dim3(256), 0, st, A, r, K, lda, slabs, pl.kps, a_vec_ok);
    NNF_CHECK_LAUNCH();
    return nnf_launch_reduce_slabs(slabs, (int)pl.nsplit, (int64_t)r * r, r, r, r, G, ldg, st, G64);
}

// Ranks above NNF_MAX_RANK: the Gram in 64 x 64 blocks.  Workgroup (split ks, block pair (bi, bj)) multiplies the k range of
// its split of row block bi by the same range of row block bj -- two LDS images instead of one, otherwise the kernel above.
// Block (bj, bi) is computed by its own workgroup from the same products in the same order, so the result is symmetric bit
// for bit, as the single-image kernel's is.  Slabs [split][r x r], reduced in split order by the usual launch.
__global__ __launch_bounds__(256) void nnf_gram_blocks_kernel(const float* __restrict__ A, int r, int64_t K, int64_t lda,
                                                              float* __restrict__ slabs, int64_t k_per_split, int a_vec_ok, int nb) {
    constexpr int MT = 4;
    __shared__ f32x4 ldsA[2][MT * 256], ldsB[2][MT * 256];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jj = lane & 15, g = lane >> 4;
    const int bi = (int)blockIdx.y / nb, bj = (int)blockIdx.y - bi * nb;
    const float* Ai = A + (int64_t)64 * bi * lda;
    const float* Bj = A + (int64_t)64 * bj * lda;
    const int ri = r - 64 * bi < 64 ? r - 64 * bi : 64, rj = r - 64 * bj < 64 ? r - 64 * bj : 64;
    const int64_t k_begin = (int64_t)blockIdx.x * k_per_split;
    const int64_t k_end = (k_begin + k_per_split < K) ? (k_begin + k_per_split) : K;
    const int nchunk = (int)((k_end - k_begin + 63) >> 6);
    f32x4 acc[MT];
#pragma unroll
    for (int b = 0; b < MT; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 areg[MT], breg[MT];
    stageA_load<MT>(Ai, lda, ri, k_end, k_begin, a_vec_ok, areg);
    stageA_load<MT>(Bj, lda, rj, k_end, k_begin, a_vec_ok, breg);
    stageA_store<MT>(ldsA[0], areg);
    stageA_store<MT>(ldsB[0], breg);
    __syncthreads();
    for (int q = 0; q < nchunk; ++q) {
        const f32x4* imgA = ldsA[q & 1];
        const f32x4* imgB = ldsB[q & 1];
        stageA_load<MT>(Ai, lda, ri, k_end, k_begin + 64 * (int64_t)(q + 1), a_vec_ok, areg);
        stageA_load<MT>(Bj, lda, rj, k_end, k_begin + 64 * (int64_t)(q + 1), a_vec_ok, breg);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f32x4 af = imgA[(w * 4 + t) * 64 + lane];       // wave w owns tile row w of the block
            f32x4 bf[MT];
#pragma unroll
            for (int b = 0; b < MT; ++b) bf[b] = imgB[(b * 4 + t) * 64 + lane];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int b = 0; b < MT; ++b) acc[b] = MFMA16(af[c], bf[b][c], acc[b]);
        }
        stageA_store<MT>(const_cast<f32x4*>(ldsA[(q + 1) & 1]), areg);
        stageA_store<MT>(const_cast<f32x4*>(ldsB[(q + 1) & 1]), breg);
        __syncthreads();
    }
    float* sl = slabs + (int64_t)blockIdx.x * r * r;
#pragma unroll
    for (int b = 0; b < MT; ++b)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 64 * bi + 16 * w + 4 * g + reg, col = 64 * bj + 16 * b + jj;
            if (row < r && col < r) sl[(int64_t)row * r + col] = acc[b][reg];
        }
}

static int launch_gram_blocks(nnf_ctx* ctx, nnf_ws_cursor& cur, const float* A, int r, int64_t K, int64_t lda, float* G, int64_t ldg,
                              hipStream_t st, double* G64) {
    const int nb = (r + 63) / 64, a_vec_ok = x_vec_ok(A, lda) ? 1 : 0;
    const nnf_gram_plan pl = nnf_plan_gram(ctx->num_cus, r, K, ldg == r, a_vec_ok, cur.remaining());
    if (pl.status != NNF_OK) return pl.status;
    if (nnf_plan_debug()) nnf_report_gram(stderr, r, K, pl);
    float* slabs = (float*)cur.take((size_t)pl.nsplit * r * r * 4);
    if (!slabs) return NNF_ERR_WORKSPACE;   // (cannot happen: the plan counted them)
    hipLaunchKernelGGL(nnf_gram_blocks_kernel, dim3((int)pl.nsplit, nb * nb), dim3(256), 0, st, A, r, K, lda, slabs, pl.kps, a_vec_ok, nb);
    NNF_CHECK_LAUNCH();
    return nnf_launch_reduce_slabs(slabs, (int)pl.nsplit, (int64_t)r * r, r, r, r, G, ldg, st, G64);
}

int nnf_gram_impl(nnf_ctx* ctx, nnf_ws_cursor& cur, const float* A, int r, int64_t K, int64_t lda, float* G, int64_t ldg,
                  hipStream_t st, double* G64) {
    if (!ctx || !A || !G || r < 1 || K < 1 || lda < K || ldg < r) return NNF_ERR_ARG;
    if (r > NNF_MAX_RANK) return launch_gram_blocks(ctx, cur, A, r, K, lda, G, ldg, st, G64);
    return nnf_dispatch<8>((r + 15) / 16, [&](auto mt) { return launch_gram<decltype(mt)::value>(ctx, cur, A, r, K, lda, G, ldg, st, G64); });
}
extern "C" int nnf_gram_f32(nnf_ctx* ctx, const float* A, int r, int64_t K, int64_t lda, float* G, int64_t ldg,
                            void* stream) {
    if (!ctx) return NNF_ERR_ARG;
    nnf_ws_cursor cur(ctx);
    return nnf_gram_impl(ctx, cur, A, r, K, lda, G, ldg, (hipStream_t)stream, nullptr);
}
// The same Gram, and next to it the sums BEFORE they are rounded to fp32 (G64: r x r doubles, contiguous): the split-K slabs are
// added in fp64 anyway, so the copy costs a second store.  For the Gram-identity cost (nnf_nmf_gram_cost_g64_f32): fp32 storage of
// U^T U alone (relative rms 3.4e-8 per entry) bounds that cost's accuracy at ~1e-4 of a late-run cost at 10^6 x 4000 rank 100.
extern "C" int nnf_gram_f64_f32(nnf_ctx* ctx, const float* A, int r, int64_t K, int64_t lda, float* G, int64_t ldg,
                                double* G64, void* stream) {
    if (!ctx || !G64) return NNF_ERR_ARG;
    nnf_ws_cursor cur(ctx);
    return nnf_gram_impl(ctx, cur, A, r, K, lda, G, ldg, (hipStream_t)stream, G64);
}


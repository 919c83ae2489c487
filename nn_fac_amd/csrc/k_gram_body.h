// The split-K Gram body shared by the stand-alone Gram kernel (k_gram.hip) and by the cross-product launches it rides in
// (nnf_xty_gram_kernel, k_xty.hip; nnf_xht_gram_kernel, k_xht.hip): one body, so a slab is the same bits wherever it is formed.
#pragma once
#include "k_stream_common.h"

// =========================================================================================================
// gram: slab[ks] = A[:, split ks] * A[:, split ks]^T.  Both MFMA operands are the same LDS fragment image
// (B[k][col] = A[col][k] is the A-fragment of tile `col/16`).  Wave w owns tile rows {w, w+4}.
// =========================================================================================================
// `split`: the split of K this workgroup forms (the stand-alone kernel: blockIdx.x; a rider: its index behind the main grid);
// ldsA: the workgroup's two chunk images (a rider uses the LDS of the cross product it rides with -- the same MT tiles).
template <int MT>
__device__ __forceinline__ void nnf_gram_body(const float* __restrict__ A, int r, int64_t K, int64_t lda,
                                              float* __restrict__ slabs, int64_t k_per_split, int a_vec_ok, int split,
                                              f32x4 (*ldsA)[MT * 256]) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jj = lane & 15, g = lane >> 4;
    const int64_t k_begin = (int64_t)split * k_per_split;
    const int64_t k_end = (k_begin + k_per_split < K) ? (k_begin + k_per_split) : K;
    const int nchunk = (int)((k_end - k_begin + 63) >> 6);
    constexpr int NR = (MT + 3) / 4;  // tile rows per wave
    f32x4 acc[NR][MT];
#pragma unroll
    for (int a = 0; a < NR; ++a)
#pragma unroll
        for (int b = 0; b < MT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 areg[MT];
    stageA_load<MT>(A, lda, r, k_end, k_begin, a_vec_ok, areg);
    stageA_store<MT>(ldsA[0], areg);
    __syncthreads();
    for (int q = 0; q < nchunk; ++q) {
        const f32x4* img = ldsA[q & 1];
        stageA_load<MT>(A, lda, r, k_end, k_begin + 64 * (int64_t)(q + 1), a_vec_ok, areg);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 bf[MT];
#pragma unroll
            for (int b = 0; b < MT; ++b) bf[b] = img[(b * 4 + t) * 64 + lane];
#pragma unroll
            for (int a = 0; a < NR; ++a) {
                const int mt = w + 4 * a;
                if (mt < MT) {
                    const f32x4 af = img[(mt * 4 + t) * 64 + lane];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int b = 0; b < MT; ++b) acc[a][b] = MFMA16(af[c], bf[b][c], acc[a][b]);
                }
            }
        }
        stageA_store<MT>(const_cast<f32x4*>(ldsA[(q + 1) & 1]), areg);
        __syncthreads();
    }
    float* sl = slabs + (int64_t)split * r * r;
#pragma unroll
    for (int a = 0; a < NR; ++a) {
        const int mt = w + 4 * a;
        if (mt < MT) {
#pragma unroll
            for (int b = 0; b < MT; ++b)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = 16 * mt + 4 * g + reg, col = 16 * b + jj;
                    if (row < r && col < r) sl[row * r + col] = acc[a][b][reg];
                }
        }
    }
}


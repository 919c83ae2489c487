// The cost / ratio / product pass over X and the model Ut^T V, which is never materialised  (nmf.py:452,455;
// beta_divergence.py:45-52): the beta-divergences, the element-wise operands of the MU update above rank 64, the CP cost.  The
// design shared with W^T X, X H^T and the Gram is described at the head of k_stream_common.h.
#include "k_stream_common.h"

// =========================================================================================================
// frob: sum_ij (X[i][j] - sum_k Ut[k][i] V[k][j])^2
//   workgroup = 128 rows (wave w: rows 32w..32w+31 as two 16-row M tiles), sweeping all columns in 64-wide blocks.
//   P tile: A[i = l&15][k] = Ut[k][i] fragments (whole rank, staged once), B[k][col] = V[k][j0+4jj+c] fragments
//   (restaged per column block, fragment order), D[row = 4g+reg][col = jj] of N tile cc <-> column j0+4jj+cc,
//   which is exactly what a lane's float4 load of X[row][j0+4jj..+3] holds.
//   The rank loop is a run-time loop (both operands come from LDS), so one kernel serves every r <= 128.
// =========================================================================================================
// Right-operand fragments of ALL column blocks, laid out exactly as the cost kernel stages them:
//   Vf[(blk*KS + s)*64 + L] = float4 V[4s + (L>>4)][64 blk + 4(L&15) .. +3]   (zero outside r x n)
// V is tiny (r x n) and identical for every workgroup, so the index arithmetic and the ragged-edge masks are done once here
// instead of once per workgroup and column block.
__global__ __launch_bounds__(256) void nnf_cost_prepv_kernel(const float* __restrict__ V, int64_t ldv, int r, int64_t n, int KS,
                                                             f32x4* __restrict__ Vf, int64_t total) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int L = (int)(e & 63);
        const int64_t q = e >> 6;
        const int s_ = (int)(q % KS);
        const int64_t blk = q / KS;
        const int k = 4 * s_ + (L >> 4);
        const int64_t j = 64 * blk + 4 * (L & 15);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k < r && j < n) {
            const float* p = V + (int64_t)k * ldv + j;
            v[0] = p[0];
            if (j + 1 < n) v[1] = p[1];
            if (j + 2 < n) v[2] = p[2];
            if (j + 3 < n) v[3] = p[3];
        }
        Vf[e] = v;
    }
}

// PIN (ranks above 128, walked in chunks of <= 128): the model of the EARLIER rank chunks, m x n with row stride ldr in Pin, is
// added to this chunk's product before the element-wise part -- read one block ahead like X (Pin may be R1: a lane reads its
// own elements of a block before it writes them).
// WT (nnf_betadiv_w_f32): a weight per entry, streamed like X through a resource and pitch of its own; the term of an entry is
// its weight times the divergence, and exactly 0 where the weight is 0, whatever X holds there (a select: 0 * NaN is NaN).
template <int OP, bool VEC, int NV, bool PIN = false, bool WT = false>   // NV = float4 pieces of a V image per thread: 4 up to r = 64, 8 up to r = 128
__global__ __launch_bounds__(256, PIN || WT ? 2 : 3) void nnf_cost_kernel(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                                          const float* __restrict__ Ut, int64_t ldu,
                                                          const f32x4* __restrict__ Vf, int r,
                                                          float beta, double* __restrict__ partial,
                                                          const float* __restrict__ Ub, int64_t ldub, int64_t nbu,
                                                          float* __restrict__ R1, float* __restrict__ R2, int64_t ldr,
                                                          int u_vec_ok, int vdb, const float* Pin = nullptr,
                                                          const float* __restrict__ Wg = nullptr, int64_t ldw = 0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int KS = (r + 3) >> 2;                               // k-steps of 4
    float* ldsU = reinterpret_cast<float*>(smem);              // [wave 4][rt 2][KS][64]
    // V image: two buffers (vdb = 1: the next block is written while this one is read, one barrier per block) or ONE (vdb = 0:
    // ranks 77..104, where the second buffer is what keeps a second workgroup off the CU -- 100 KB against 75 KB of the
    // 160 KB; with a single wave per SIMD the rank-100 cost pass of config E ran at 0.34 of the MFMA peak)
    f32x4* ldsV = reinterpret_cast<f32x4*>(smem + (size_t)4 * 2 * KS * 64 * 4);  // [vdb ? 2 : 1][KS][64] float4
    double* red = reinterpret_cast<double*>(smem + (size_t)4 * 2 * KS * 64 * 4 + (size_t)(vdb ? 2 : 1) * KS * 64 * 16);
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jj = lane & 15, g = lane >> 4;
    const int64_t i0w = (int64_t)blockIdx.x * 128 + 32 * w;
    int64_t rows = m - i0w;
    if (rows > 32) rows = 32;
    const uint32_t bytes = rows > 0 ? (uint32_t)(((rows - 1) * ldx + n) * 4) : 0u;
    const rsrc_t rs = nnf_make_rsrc(X + (rows > 0 ? i0w : 0) * ldx, bytes);
    const int ldx4 = (int)(ldx * 4);
    const int voff = (int)(((int64_t)4 * g * ldx + 4 * jj) * 4);
    // column blocks [blk0, blk1) of this workgroup: blockIdx.y splits the column range so that the grid has several times
    // more workgroups than resident slots (128-row workgroups alone give 782 for 512 slots at B: a 1.5-round tail)
    const int nblk_all = (int)((n + 63) >> 6);
    const int per = (nblk_all + (int)gridDim.y - 1) / (int)gridDim.y;
    const int blk0 = (int)blockIdx.y * per;
    const int nblk = (blk0 + per < nblk_all) ? (blk0 + per) : nblk_all;

    // U fragments of this wave's 32 rows: ldsU[w][rt][s][lane] = Ut[4s + (lane>>4)][i0w + 16rt + (lane&15)]
    if (Ub == nullptr && u_vec_ok && rows == 32) {
        // four consecutive rows i of one rank row k are four consecutive floats of the image: 16-byte loads straight
        // into 16-byte LDS stores, all of a wave's loads in flight together (the element-wise loop below costs a
        // division and a dependent round trip per element -- a prologue as long as the MFMA work of a short column range)
        const int nq = 8 * r;                      // float4 pieces: (k, j) -> Ut[k][i0w + 4j .. +3], j = 0..7
        float* dstw = ldsU + (size_t)(w * 2) * KS * 64;
        for (int e0 = 0; e0 < nq; e0 += 4 * 64) {
            f32x4 piece[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + 64 * u + lane;
                piece[u] = (e < nq) ? *reinterpret_cast<const f32x4*>(Ut + (int64_t)(e >> 3) * ldu + i0w + 4 * (e & 7))
                                    : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = e0 + 64 * u + lane;
                const int k = e >> 3, j = e & 7;
                if (e < nq)
                    *reinterpret_cast<f32x4*>(dstw + ((j >> 2) * KS + (k >> 2)) * 64 + (k & 3) * 16 + 4 * (j & 3)) = piece[u];
            }
        }
        if (r & 3) {   // rank rows r .. 4KS-1 of the last k-step are zero
            const int k = r + (lane >> 4);
            if (k < 4 * KS) {
                dstw[(0 * KS + (k >> 2)) * 64 + (k & 3) * 16 + (lane & 15)] = 0.f;
                dstw[(1 * KS + (k >> 2)) * 64 + (k & 3) * 16 + (lane & 15)] = 0.f;
            }
        }
    } else {
        // element-wise staging (ragged last workgroup, unaligned U, Khatri-Rao rows of the CP cost): a lane's entries are
        // (rt, s) -> Ut[4s + (lane>>4)][i0w + 16rt + (lane&15)], i.e. only TWO tensor rows per lane (one division each for the
        // Khatri-Rao split), and the loads go out eight at a time from clamped addresses.  (One entry per trip with its
        // loads under the `k < r && i < m` test was 2 KS dependent round trips + divisions in front of the first MFMA --
        // longer than the MFMA work of a CP-cost workgroup: 4 column blocks.)
        const int L = lane;
        int64_t ia0, ib0, ia1, ib1;
        const int64_t i_0 = i0w + (L & 15), i_1 = i_0 + 16;
        const bool ok0 = i_0 < m, ok1 = i_1 < m;
        if (Ub == nullptr) { ia0 = ok0 ? i_0 : 0; ia1 = ok1 ? i_1 : 0; ib0 = ib1 = 0; }
        else {
            const int64_t c0 = ok0 ? i_0 : 0, c1 = ok1 ? i_1 : 0;
            ia0 = c0 / nbu; ib0 = c0 - ia0 * nbu;
            ia1 = c1 / nbu; ib1 = c1 - ia1 * nbu;
        }
        float* dstw = ldsU + (size_t)(w * 2) * KS * 64 + L;
        auto stage = [&](auto kr) {   // kr: with / without the second (Khatri-Rao) factor -- no per-entry branch either way
            constexpr bool KR = decltype(kr)::value;
            for (int j0 = 0; j0 < 2 * KS; j0 += 8) {
                float ua[8], ub[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int j = j0 + u < 2 * KS ? j0 + u : 0;
                    const bool rt = j >= KS;
                    const int k = 4 * (j - (rt ? KS : 0)) + (L >> 4);
                    const bool ok = k < r && (rt ? ok1 : ok0);
                    const int64_t kc = ok ? k : 0;
                    ua[u] = Ut[kc * ldu + (ok ? (rt ? ia1 : ia0) : 0)];
                    if constexpr (KR) ub[u] = Ub[kc * ldub + (ok ? (rt ? ib1 : ib0) : 0)];
                    else ub[u] = 1.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int j = j0 + u;
                    if (j < 2 * KS) {
                        const bool rt = j >= KS;
                        const int k = 4 * (j - (rt ? KS : 0)) + (L >> 4);
                        const bool ok = k < r && (rt ? ok1 : ok0);
                        dstw[j * 64] = ok ? ua[u] * ub[u] : 0.f;
                    }
                }
            }
        };
        if (Ub != nullptr) stage(std::true_type{});
        else stage(std::false_type{});
    }
    // V fragments of one 64-column block: img[s][lane] = float4 V[4s + (lane>>4)][j0 + 4(lane&15) .. +3].
    // Staged in two halves: global loads into registers before the MFMAs of the current block, LDS writes after them.
    f32x4 vreg[NV];
    auto stageV_load = [&](int blk) {   // straight copies of the pre-arranged fragments (nnf_cost_prepv_kernel)
        const f32x4* src = Vf + (size_t)blk * KS * 64;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int e = threadIdx.x + 256 * u;
            vreg[u] = (e < KS * 64 && blk < nblk_all) ? src[e] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto stageV_store = [&](f32x4* img) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int e = threadIdx.x + 256 * u;
            if (e < KS * 64) img[e] = vreg[u];
        }
    };
    stageV_load(blk0);
    stageV_store(ldsV + (size_t)(vdb ? (blk0 & 1) : 0) * KS * 64);
    // X one block ahead.  (A two-block ring was tried: same time, 12 more registers -- and at <= 136 registers three of these
    // waves leave room on a SIMD for a wave of the persistent V-side sweep kernel, which the outer loop overlaps this
    // kernel with.)  The block past the workgroup's column range is "read" through an out-of-range offset: zeros, no
    // memory traffic (the prefetch used to fetch the next rows' data: 1.24 GB instead of 0.82 GB per launch).
    f32x4 xb[2][4];  // [rt][reg]: row i0w + 16rt + 4g + reg, columns j0+4jj..+3
    f32x4 pb[PIN ? 2 : 1][PIN ? 4 : 1];   // the same elements of Pin
    rsrc_t rsp = rs;
    int ldp4 = 0, voffp = 0;
    if constexpr (PIN) {
        rsp = nnf_make_rsrc(Pin + (rows > 0 ? i0w : 0) * ldr, rows > 0 ? (uint32_t)(((rows - 1) * ldr + n) * 4) : 0u);
        ldp4 = (int)(ldr * 4);
        voffp = (int)(((int64_t)4 * g * ldr + 4 * jj) * 4);
    }
    f32x4 wb[WT ? 2 : 1][WT ? 4 : 1];   // the same elements of Wg
    rsrc_t rsw = rs;
    int ldw4 = 0, voffw = 0;
    if constexpr (WT) {
        rsw = nnf_make_rsrc(Wg + (rows > 0 ? i0w : 0) * ldw, rows > 0 ? (uint32_t)(((rows - 1) * ldw + n) * 4) : 0u);
        ldw4 = (int)(ldw * 4);
        voffw = (int)(((int64_t)4 * g * ldw + 4 * jj) * 4);
    }
    auto xload = [&](int blk) {
        const int vo = (blk < nblk) ? voff : (int)0x7ffffff0;
        if constexpr (WT) {
            const int vw = (blk < nblk) ? voffw : (int)0x7ffffff0;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) wb[rt][reg] = nnf_bload4<VEC>(rsw, vw, (16 * rt + reg) * ldw4 + 256 * blk);
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) xb[rt][reg] = nnf_bload4<VEC>(rs, vo, (16 * rt + reg) * ldx4 + 256 * blk);
        if constexpr (PIN) {
            const int vp = (blk < nblk) ? voffp : (int)0x7ffffff0;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) pb[rt][reg] = nnf_bload4<VEC>(rsp, vp, (16 * rt + reg) * ldp4 + 256 * blk);
        }
    };
    xload(blk0);
    __syncthreads();

    double dsum = 0.0;
    const float* uf = ldsU + (size_t)(w * 2) * KS * 64 + lane;
    for (int blk = blk0; blk < nblk; ++blk) {
        const f32x4* img = ldsV + (size_t)(vdb ? (blk & 1) : 0) * KS * 64;
        stageV_load(blk + 1);   // past the last block every entry is masked to zero (j >= n)
        f32x4 acc[2][4];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) acc[rt][cc] = f32x4{0.f, 0.f, 0.f, 0.f};
        // k loop, two steps per trip, software-pipelined by hand: the fragments of the next step are read from LDS (three
        // hand-issued ds_reads) while the MFMAs of the current one run.  The compiler rotates a C++ version of this back
        // into "read, wait, multiply" (tools/ notes: ~30 % of the MFMA time exposed).  Nothing is in flight at the loop
        // back-edge or at any other control-flow merge, which is what makes hand-issued loads safe (k_hals_quad.hip).
        {
            const unsigned bvb = (unsigned)(uintptr_t)img + (unsigned)lane * 16u;        // + 1024 per k-step
            const unsigned a0b = (unsigned)(uintptr_t)uf;                                 // + 256 per k-step
            const unsigned a1b = a0b + (unsigned)KS * 256u;
            f32x4 bvA, bvB;
            float a0A, a1A, a0B, a1B;
            asm volatile("ds_read_b128 %0, %3\n\tds_read_b32 %1, %4\n\tds_read_b32 %2, %5\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(bvA), "=&v"(a0A), "=&v"(a1A) : "v"(bvb), "v"(a0b), "v"(a1b));
            int s = 0;
            for (; s + 1 < KS; s += 2) {
                const int sb = s + 1, sa = (s + 2 < KS) ? s + 2 : KS - 1;   // the clamped extra read is never used
                // (the A set rides through the statement as in/out operands so that its MFMAs cannot be scheduled above it,
                //  and the accumulators ride through the wait so that they cannot sink below it)
                asm volatile("ds_read_b128 %0, %6\n\tds_read_b32 %1, %7\n\tds_read_b32 %2, %8"
                             : "=&v"(bvB), "=&v"(a0B), "=&v"(a1B), "+v"(bvA), "+v"(a0A), "+v"(a1A)
                             : "v"(bvb + (unsigned)sb * 1024u), "v"(a0b + (unsigned)sb * 256u), "v"(a1b + (unsigned)sb * 256u));
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    acc[0][cc] = MFMA16(a0A, bvA[cc], acc[0][cc]);
                    acc[1][cc] = MFMA16(a1A, bvA[cc], acc[1][cc]);
                }
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(bvB), "+v"(a0B), "+v"(a1B), "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]),
                               "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]), "+v"(acc[1][3]));
                asm volatile("ds_read_b128 %0, %6\n\tds_read_b32 %1, %7\n\tds_read_b32 %2, %8"
                             : "=&v"(bvA), "=&v"(a0A), "=&v"(a1A), "+v"(bvB), "+v"(a0B), "+v"(a1B)
                             : "v"(bvb + (unsigned)sa * 1024u), "v"(a0b + (unsigned)sa * 256u), "v"(a1b + (unsigned)sa * 256u));
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    acc[0][cc] = MFMA16(a0B, bvB[cc], acc[0][cc]);
                    acc[1][cc] = MFMA16(a1B, bvB[cc], acc[1][cc]);
                }
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(bvA), "+v"(a0A), "+v"(a1A), "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]),
                               "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]), "+v"(acc[1][3]));
            }
            if (s < KS) {   // odd number of k-steps: the A set holds step KS-1
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    acc[0][cc] = MFMA16(a0A, bvA[cc], acc[0][cc]);
                    acc[1][cc] = MFMA16(a1A, bvA[cc], acc[1][cc]);
                }
            }
        }
        // residual of this 32 x 64 block; columns past n hold the next row's data -> masked out
        const int64_t jrem = n - (64 * (int64_t)blk + 4 * jj);
        float loc = 0.f;
        if constexpr (PIN) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) acc[rt][cc][reg] += pb[rt][reg][cc];
        }
        if constexpr (OP == NNF_RATIO_KL || OP == NNF_RATIO_GEN || OP == NNF_PROD) {
            // large-rank MU (r > 64): the element-wise operands are written out, the two contractions follow as plain
            // X H^T / W^T X launches on them (k_mu.hip).  One float4 per (row piece): columns j0+4jj .. +3.
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int rowl = 16 * rt + 4 * g + reg;
                    if (rowl >= rows) continue;
                    f32x4 o1, o2;
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        const float p = acc[rt][cc][reg], x = xb[rt][reg][cc];
                        if constexpr (OP == NNF_PROD) {
                            o1[cc] = p;
                            o2[cc] = 0.f;
                        } else if constexpr (OP == NNF_RATIO_KL) {
                            o1[cc] = x * __builtin_amdgcn_rcpf(p);
                            o2[cc] = 0.f;
                        } else {
                            const float lp = __builtin_amdgcn_logf(p);
                            o2[cc] = __builtin_amdgcn_exp2f((beta - 1.f) * lp);
                            o1[cc] = o2[cc] * __builtin_amdgcn_rcpf(p) * x;
                        }
                    }
                    const int64_t off = (i0w + rowl) * ldr + 64 * (int64_t)blk + 4 * jj;
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        if (cc < jrem) {
                            R1[off + cc] = o1[cc];
                            if constexpr (OP == NNF_RATIO_GEN) R2[off + cc] = o2[cc];
                        }
                    }
                }
        } else if constexpr (WT) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const bool rowok = 16 * rt + 4 * g + reg < rows;   // rows past the end of the matrix
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        const float wv = wb[rt][reg][cc];
                        const float term = wv * nnf_cost_term<OP>(xb[rt][reg][cc], acc[rt][cc][reg], beta);
                        loc += (rowok && cc < jrem && wv != 0.f) ? term : 0.f;
                    }
                }
        } else
        if (rows == 32 && 64 * (int64_t)(blk + 1) <= n) {   // interior block (wave-uniform): no edge masks
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) loc += nnf_cost_term<OP>(xb[rt][reg][cc], acc[rt][cc][reg], beta);
        } else {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    if (16 * rt + 4 * g + reg >= rows) continue;   // rows past the end of the matrix
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) {
                        if (cc < jrem) loc += nnf_cost_term<OP>(xb[rt][reg][cc], acc[rt][cc][reg], beta);
                    }
                }
        }
        dsum += (double)loc;
        xload(blk + 1);
        if (!vdb) __syncthreads();   // single buffer: every wave is past its last read of this block's image
        stageV_store(ldsV + (size_t)(vdb ? ((blk + 1) & 1) : 0) * KS * 64);
        __syncthreads();
    }
    const double bs = nnf_block_sum_f64(dsum, red);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = bs;
}

// One pass of at most NNF_MAX_RANK rank rows.  Everything from `beta` on is optional (a plain squared residual).
struct cost_request {
    const float* X; int64_t m, n, ldx;
    const float* Ut; int64_t ldu;          // left operand, r x m
    const float* V; int64_t ldv;           // right operand, r x n
    int r;
    float beta = 2.f; double scale = 1.0;
    double* out = nullptr;                 // cost passes: out[0] = scale * sum of the terms
    const float* Ub = nullptr; int64_t ldub = 0, nbu = 1;        // Khatri-Rao rows (CP cost): U[k][i] = Ut[k][i / nbu] * Ub[k][i % nbu]
    float* R1 = nullptr; float* R2 = nullptr; int64_t ldr = 0;   // ratio passes: the outputs, m x n with row stride ldr; NNF_PROD: R1
    const float* Pin = nullptr;            // the model of the earlier rank chunks (row stride ldr), added to this pass's product
    size_t ws_cap = 0;                     // != 0: the workspace ends here (its tail holds that model)
    const float* Wg = nullptr; int64_t ldw = 0;   // weighted cost (r <= NNF_MAX_RANK): m x n weights, streamed next to X
};

template <int OP>
static int launch_cost(nnf_ctx* ctx, const cost_request& q, hipStream_t st) {
    // plan (nnf_plan_cost, k_stream_plan.h; a refusal launches nothing), report, carve, launch, sum
    const float* const X = q.X;
    const int64_t m = q.m, n = q.n, ldx = q.ldx;
    const int r = q.r;
    if (q.Pin != nullptr && q.ldr < n) return NNF_ERR_ARG;
    // tuning knob (tools/cost_probe.py): NNF_COST_CSPLIT overrides the number of column splits
    static const int forced = [] { const char* e = getenv("NNF_COST_CSPLIT"); return e ? atoi(e) : 0; }();
    nnf_ws_cursor cur(ctx);
    if (q.ws_cap) cur.cap = q.ws_cap;
    const nnf_cost_plan pl = nnf_plan_cost(ctx->num_cus, m, n, r, q.Ub != nullptr, forced, q.Pin != nullptr, OP == NNF_PROD, cur.remaining());
    if (pl.status != NNF_OK) return pl.status;
    // (a later rank chunk of a rank above 128, launch_cost_any_rank, reads the model next to X: one load width for both)
    const bool vec = x_vec_ok(X, ldx) && (q.Pin == nullptr || x_vec_ok(q.Pin, q.ldr)) && (q.Wg == nullptr || x_vec_ok(q.Wg, q.ldw));
    if (nnf_plan_debug()) {
        static const char* const ops[] = {"frob", "kl", "is", "gen", "ratio_kl", "ratio_gen", "prod"};
        nnf_report_cost(stderr, m, n, r, ops[OP], vec, q.Pin != nullptr, q.Ub ? q.nbu : 0, pl, q.Wg ? " weighted=1" : "");
    }
    const int grid = pl.grid, csplit = pl.csplit, KS = pl.KS, vdb = pl.vdb, u_vec_ok = x_vec_ok(q.Ut, q.ldu) ? 1 : 0;
    const size_t shm = pl.shm;
    double* partial = (double*)cur.take(pl.partial_bytes);
    f32x4* Vf = (f32x4*)cur.take(pl.vf_bytes);
    if (!partial || !Vf) return NNF_ERR_WORKSPACE;   // (cannot happen: the plan counted them)
    {
        const int64_t vf_total = (int64_t)(pl.vf_bytes / 16);
        int64_t pg = nnf_cdiv(vf_total, 256);
        if (pg > 1024) pg = 1024;
        hipLaunchKernelGGL(nnf_cost_prepv_kernel, dim3((int)pg), dim3(256), 0, st, q.V, q.ldv, r, n, KS, Vf, vf_total);
        NNF_CHECK_LAUNCH();
    }
    const auto launch = [&](auto vv, auto nn, auto pin, auto wt) {
        const auto kernel = nnf_cost_kernel<OP, decltype(vv)::value, decltype(nn)::value, decltype(pin)::value, decltype(wt)::value>;
        if (shm > 48 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        hipLaunchKernelGGL(kernel, dim3(grid, csplit), dim3(256), shm, st, X, m, n, ldx, q.Ut, q.ldu, Vf, r, q.beta, partial, q.Ub, q.ldub,
                           q.nbu, q.R1, q.R2, q.ldr, u_vec_ok, vdb, q.Pin, q.Wg, q.ldw);
    };
    const auto pick = [&](auto vv) {   // per load width: one instance that reads a model back, one that writes it, two for the rest
        if constexpr (OP <= NNF_COST_GEN) {   // the weighted cost: the same two widths of the V image
            if (q.Wg != nullptr) {
                if (pl.NN != 4) launch(vv, nnf_int<8>{}, std::false_type{}, std::true_type{});
                else launch(vv, nnf_int<4>{}, std::false_type{}, std::true_type{});
                return;
            }
        }
        if (q.Pin != nullptr) launch(vv, nnf_int<8>{}, std::true_type{}, std::false_type{});
        else if (OP == NNF_PROD || pl.NN != 4) launch(vv, nnf_int<8>{}, std::false_type{}, std::false_type{});
        else launch(vv, nnf_int<4>{}, std::false_type{}, std::false_type{});
    };
    nnf_probe(ctx, NNF_PROBE_COST, 0, st);
    if (vec) pick(std::true_type{});
    else pick(std::false_type{});
    NNF_CHECK_LAUNCH();
    nnf_probe(ctx, NNF_PROBE_COST, 1, st);
    if (OP == NNF_RATIO_KL || OP == NNF_RATIO_GEN || OP == NNF_PROD) return NNF_OK;   // nothing to sum
    return nnf_launch_sum_f64(partial, (int64_t)grid * csplit, q.scale, q.out, st);
}

// what every entry point checks of a request before it launches (has_out: the result pointer of a cost pass is there)
static int cost_args_ok(nnf_ctx* ctx, const cost_request& q, bool has_out) {
    if (!ctx || !q.X || !q.Ut || !q.V || !has_out || q.m < 1 || q.n < 1 || q.r < 1 || q.ldx < q.n || q.ldu < q.m || q.ldv < q.n)
        return NNF_ERR_ARG;
    return nnf_cost_offsets_ok(q.ldx, q.n) ? NNF_OK : NNF_ERR_UNSUPPORTED;
}

// The cost / ratio pass at any rank.  Up to NNF_MAX_RANK: one launch.  Above: the model U V is built up over rank chunks of
// <= 128 in an m x n buffer P -- chunk 0 writes its product (NNF_PROD), every later chunk adds its own to what it reads
// back, and the LAST chunk does so inside the pass that was asked for (cost terms or ratios on X and the whole model).
// P is the first output of a ratio pass (R1, in place), else the caller's scratch (nnf_ctx_set_scratch) or, if that is
// absent or too small, the tail of the context workspace; NNF_ERR_WORKSPACE when neither holds 4*m*ldp bytes.
// (Not nnf_rank_passes: the chunks are not independent of each other, each reads the model the ones before it left.)
template <int OP>
static int launch_cost_any_rank(nnf_ctx* ctx, const cost_request& q, hipStream_t st) {
    if (q.r <= NNF_MAX_RANK) return launch_cost<OP>(ctx, q, st);
    float* P = q.R1;
    int64_t ldp = q.ldr;
    size_t cap = 0;
    if (!P) {
        ldp = (q.n + 3) & ~(int64_t)3;
        const size_t need = (size_t)q.m * ldp * 4;
        if (ctx->big && ctx->big_bytes >= need) P = (float*)ctx->big;
        else {
            if (need + ((size_t)8 << 20) > ctx->ws_bytes) return NNF_ERR_WORKSPACE;
            cap = (ctx->ws_bytes - need) & ~(size_t)255;
            P = (float*)(ctx->ws + cap);
        }
    }
    if (!nnf_cost_offsets_ok(ldp, q.n)) return NNF_ERR_UNSUPPORTED;
    for (int k0 = 0; k0 < q.r; k0 += NNF_MAX_RANK) {
        cost_request c = q;                 // this chunk: its rank rows of the operands, the model read back and the cap
        c.r = q.r - k0 < NNF_MAX_RANK ? q.r - k0 : NNF_MAX_RANK;
        c.Ut = q.Ut + (int64_t)k0 * q.ldu;
        c.V = q.V + (int64_t)k0 * q.ldv;
        c.Ub = q.Ub ? q.Ub + (int64_t)k0 * q.ldub : nullptr;
        c.ldr = ldp;
        c.Pin = k0 ? P : nullptr;
        c.ws_cap = cap;
        int e;
        if (k0 + c.r < q.r) {               // not the last: the model so far goes (back) to P
            c.out = nullptr;
            c.R1 = P;
            c.R2 = nullptr;
            e = launch_cost<NNF_PROD>(ctx, c, st);
        } else {
            e = launch_cost<OP>(ctx, c, st);
        }
        if (e != NNF_OK) return e;
    }
    return NNF_OK;
}

// the beta-divergence of a request (beta = 2: 1/2 ||X - UV||^2, beta_divergence.py:51-52)
static int launch_betadiv(nnf_ctx* ctx, cost_request q, double beta, hipStream_t st) {
    q.beta = (float)beta;
    q.scale = beta == 2.0 ? 0.5 : 1.0;
    if (beta == 2.0) return launch_cost_any_rank<NNF_COST_FROB>(ctx, q, st);
    if (beta == 1.0) return launch_cost_any_rank<NNF_COST_KL>(ctx, q, st);
    if (beta == 0.0) return launch_cost_any_rank<NNF_COST_IS>(ctx, q, st);
    return launch_cost_any_rank<NNF_COST_GEN>(ctx, q, st);
}

extern "C" int nnf_frob_resid_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut,
                                  int64_t ldu, const float* V, int64_t ldv, int r, double* out_f64, void* stream) {
    const cost_request q = {.X = X, .m = m, .n = n, .ldx = ldx, .Ut = Ut, .ldu = ldu, .V = V, .ldv = ldv, .r = r, .out = out_f64};
    const int rc = cost_args_ok(ctx, q, out_f64 != nullptr);
    if (rc != NNF_OK) return rc;
    return launch_cost_any_rank<NNF_COST_FROB>(ctx, q, (hipStream_t)stream);
}

extern "C" int nnf_betadiv_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut,
                               int64_t ldu, const float* V, int64_t ldv, int r, double beta, double* out_f64,
                               void* stream) {
    const cost_request q = {.X = X, .m = m, .n = n, .ldx = ldx, .Ut = Ut, .ldu = ldu, .V = V, .ldv = ldv, .r = r, .out = out_f64};
    const int rc = cost_args_ok(ctx, q, out_f64 != nullptr);
    if (rc != NNF_OK) return rc;
    if (!(beta >= 0.0)) return NNF_ERR_ARG;
    return launch_betadiv(ctx, q, beta, (hipStream_t)stream);
}

// Element-wise operands of mu_betadivmin (mu.py:84-97) at any rank r >= 1 (the drivers take this route above NNF_MAX_RANK, where
// there is no fused kernel):
//   R1 = X .* (U V)^(beta-2)   and, unless beta == 1,   R2 = (U V)^(beta-1),   both m x n with row stride ldr.
// Above NNF_MAX_RANK R1 is also the model buffer of launch_cost_any_rank: written before it is read, whatever it held.
extern "C" int nnf_mu_ratio_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                                const float* V, int64_t ldv, int r, double beta, float* R1, float* R2, int64_t ldr,
                                void* stream) {
    const cost_request q = {.X = X, .m = m, .n = n, .ldx = ldx, .Ut = Ut, .ldu = ldu, .V = V, .ldv = ldv, .r = r, .beta = (float)beta,
                            .R1 = R1, .R2 = R2, .ldr = ldr};
    const int rc = cost_args_ok(ctx, q, true);
    if (rc != NNF_OK) return rc;
    if (!(beta >= 0.0) || !R1 || ldr < n || (beta != 1.0 && !R2)) return NNF_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (beta == 1.0) return launch_cost_any_rank<NNF_RATIO_KL>(ctx, q, st);
    return launch_cost_any_rank<NNF_RATIO_GEN>(ctx, q, st);
}

// beta-divergence between a dense 3-way tensor and its CP model [[F0, F1, F2]]: the cost kernel on T seen as an (I*J) x K
// matrix.  Row (i,j) of the left operand is F0[i,:].*F1[j,:], generated while it is staged; the right operand is F2^T as is.
// I*J rows give the kernel its parallelism (one workgroup per 128 rows).  Replaces the cost lines of ntf.py:470-473 (the
// reference rebuilds the 500 x 250000 reconstruction explicitly).
// (ranks above 128: the model is built up over rank chunks in a tensor-sized buffer, launch_cost_any_rank)
extern "C" int nnf_cp3_betadiv_f32(nnf_ctx* ctx, const float* T, int64_t I, int64_t J, int64_t K, const float* Ft0,
                                   int64_t ld0, const float* Ft1, int64_t ld1, const float* Ft2, int64_t ld2, int R,
                                   double beta, double* out_f64, void* stream) {
    if (!ctx || !T || !Ft0 || !Ft1 || !Ft2 || !out_f64 || I < 1 || J < 1 || K < 1 || R < 1 || ld0 < I || ld1 < J ||
        ld2 < K || !(beta >= 0.0))
        return NNF_ERR_ARG;
    if (!nnf_cost_offsets_ok(K, K)) return NNF_ERR_UNSUPPORTED;
    const cost_request q = {.X = T, .m = I * J, .n = K, .ldx = K, .Ut = Ft0, .ldu = ld0, .V = Ft2, .ldv = ld2, .r = R, .out = out_f64,
                            .Ub = Ft1, .ldub = ld1, .nbu = J};
    return launch_betadiv(ctx, q, beta, (hipStream_t)stream);
}

// Weighted beta-divergence  sum_ij Wg[i][j] d_beta(X[i][j] | (U V)[i][j])  (not normalised, as nmf.py:455): the cost of weighted
// NMF (nnf_mu_left_w_f32 / nnf_mu_right_w_f32).  An entry of weight zero adds exactly 0 whatever X holds there.  beta = 2 counts
// 1/2 (x - p)^2 per entry like nnf_betadiv_f32.  Same launch plans as the unweighted pass; r <= NNF_MAX_RANK.
extern "C" int nnf_betadiv_w_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Wg, int64_t ldw,
                                 const float* Ut, int64_t ldu, const float* V, int64_t ldv, int r, double beta, double* out_f64,
                                 void* stream) {
    const cost_request q = {.X = X, .m = m, .n = n, .ldx = ldx, .Ut = Ut, .ldu = ldu, .V = V, .ldv = ldv, .r = r, .out = out_f64,
                            .Wg = Wg, .ldw = ldw};
    const int rc = cost_args_ok(ctx, q, out_f64 != nullptr);
    if (rc != NNF_OK && rc != NNF_ERR_UNSUPPORTED) return rc;
    if (!Wg || ldw < n || !(beta >= 0.0)) return NNF_ERR_ARG;
    if (rc != NNF_OK || r > NNF_MAX_RANK || !nnf_cost_offsets_ok(ldw, n)) return NNF_ERR_UNSUPPORTED;
    return launch_betadiv(ctx, q, beta, (hipStream_t)stream);
}

// beta-divergence multiplicative update of ONE mode's factor on the tensor's own layout (mu_betadivmin, mu.py:79-97, against
// tl.unfold(T, n) without forming it).  T is contiguous and seen as (L, I, K); Ft is the mode's transposed factor (r x I), V the
// other operand (r x L*K: khatri_rao(others)^T or the expanded core), column l*K + k of V belongs to the entries T[l, :, k]:
//
//   P[l,i,k] = sum_r Ft[r,i] V[r, l*K+k]
//   num[r,i] = sum_{l,k} T[l,i,k] P^(beta-2) V[r, l*K+k],   den[r,i] = sum_{l,k} P^(beta-1) V[r, l*K+k]   (beta = 1: rowsum(V)[r], fp64)
//   out[r,i] = max(Ft[r,i] (num/den)^gamma(beta), 1e-12)
//
// One pass over T where it lies, 16 bytes per lane along k; nothing of the tensor's size is written.  A workgroup (4 waves) owns
// MU_MODE_ROWS = 64 rows of I -- one 16-row tile per wave -- and a contiguous range of units (k_mu_plan.h: 16 consecutive k of
// one l).  Per unit a wave runs, as the matrix kernels of k_mu_kernels.h do,
//   MFMA #1 : P^T tile (16 k x 16 i) = V-tile^T Ft-tile, contracted over the rank (V from LDS, Ft fragments resident in registers)
//   VALU    : R1 = P^(beta-2) .* T [, R2 = P^(beta-1)] in the accumulator layout, zero outside the tensor (mu_elem: the same
//             conventions for zero entries as nnf_mu_left_f32)
//   MFMA #2 : num (+ den) += V-tile R, contracted over the 16 k: the accumulator of MFMA #1 is the B operand as it stands
// The V chunk (MU_MODE_CHUNK units x 16 MT ranks x 16 k) is staged once per workgroup in LDS, in an order both MFMAs read
// without bank conflicts, and serves the four waves; the next chunk's V and T are in flight in registers meanwhile.
// The partial sums of a split go to its slab; nnf_launch_mu_finish (k_mu.hip) adds the slabs in split order in fp64 and finishes.
//
// Weighted form (WT, nnf_mu_mode_w_f32): a weight Wg[l,i,k] >= 0 per entry, contiguous like T,
//   num[r,i] = sum_{l,k} Wg T P^(beta-2) V[r, l*K+k],   den[r,i] = sum_{l,k} Wg P^(beta-1) V[r, l*K+k]
// for any beta -- beta = 1 has no rowsum(V) shortcut under weights, so every beta carries both accumulators, and one instantiation
// per (rank tiles, load width) serves every beta (mu_elem_w: a wave-uniform switch in front of a unit's element-wise step).  The
// weights of a lane's four k ride next to T through load_t and the prefetch.  An entry of weight zero is out of both sums
// whatever T holds there (a select, not a product: 0 * NaN would be NaN).  The raw sums go out: the slabs of both sets are added
// in split order in fp64 by nnf_launch_reduce_sets (one launch for the two sets, each the bits of nnf_launch_reduce_slabs), a single
// slab included, and nnf_mu_apply_f32 finishes.
#include "k_mu_kernels.h"

NNF_BUILD_FLAGS(k_mu_mode, "MU_MODE_ROWS=" NNF_STR(MU_MODE_ROWS) " MU_MODE_CHUNK=" NNF_STR(MU_MODE_CHUNK))

// r1 = p^(beta-2) x, r2 = p^(beta-1).  beta = 2 is exact (r1 = x, r2 = p) instead of exp2(log2 p) -- and keeps a zero of P a zero.
template <bool KL>
__device__ __forceinline__ void mu_mode_elem(float x, float p, float beta, bool beta2, float& r1, float& r2) {
    if constexpr (KL) {
        mu_elem<BM_KL>(x, p, beta, r1, r2);
    } else {
        mu_elem<BM_GEN>(x, p, beta, r1, r2);
        r1 = beta2 ? x : r1;
        r2 = beta2 ? p : r2;
    }
}

// VEC: T, V (and Wg) 16-byte aligned with K % 4 == 0 and ldv % 4 == 0 -- every group of four k is one 16-byte load, wholly inside or outside
template <int MT, bool KL, bool VEC, bool WT = false>
__global__ __launch_bounds__(256) void nnf_mu_mode_kernel(const float* __restrict__ T, int64_t L, int64_t I, int64_t K,
                                                          const float* __restrict__ Ft, int64_t ldf,
                                                          const float* __restrict__ V, int64_t ldv, int r, float beta,
                                                          float* __restrict__ snum, float* __restrict__ sden, int64_t ldp,
                                                          int64_t nrb, int64_t kt, int64_t units, int64_t ups,
                                                          const float* __restrict__ Wg = nullptr) {
    static_assert(!(WT && KL), "the weighted form carries both accumulators at every beta");
    constexpr int CH = MU_MODE_CHUNK, RP = 16 * MT, WCH = WT ? CH : 1;
    __shared__ __attribute__((aligned(16))) float Vs[CH * RP * 16];   // [unit][rank][16 k]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int64_t rb = (int64_t)blockIdx.x % nrb, sp = (int64_t)blockIdx.x / nrb;
    const int64_t u_begin = sp * ups, u_end = (u_begin + ups < units) ? u_begin + ups : units;
    const int64_t i = rb * MU_MODE_ROWS + 16 * w + c16;   // this lane's row of I
    const bool row_ok = i < I;
    [[maybe_unused]] bool beta2 = false;   // without weights: beta = 2 exact
    [[maybe_unused]] int bsel = 0;         // WT: the element-wise body (mu_elem_w), wave-uniform
    if constexpr (WT) bsel = mu_bsel(beta);
    else beta2 = beta == 2.f;

    // resident Ft fragments of MFMA #1: B[k = rank 4s + g][n = i]
    float ftf[4 * MT];
#pragma unroll
    for (int s = 0; s < 4 * MT; ++s) {
        const int rank = 4 * s + g;
        ftf[s] = (row_ok && rank < r) ? Ft[(int64_t)rank * ldf + i] : 0.f;
    }
    f32x4 num[MT], den[KL ? 1 : MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        num[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (!KL) den[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // staging of V: MT quads (four k of one rank of one unit) per thread, rank slowest so that a rank's 64 k are one run of lanes
    // (l, ku) of unit u = l * kt + ku, stepped without 64-bit divisions: one unit on
    auto step = [&](int64_t& l, int64_t& ku) {
        const bool wrap = ku + 1 >= kt;
        ku = wrap ? 0 : ku + 1;
        l += wrap ? 1 : 0;
    };
    auto load_v = [&](int64_t u0, int64_t l0, int64_t ku0, f32x4 (&vq)[MT]) {
        const int uu = (tid >> 2) % CH, k4 = 4 * (tid & 3);   // (256 quads are a whole number of chunks' worth: the same for every j)
        int64_t l = l0, ku = ku0;
#pragma unroll
        for (int t = 0; t < CH - 1; ++t)
            if (t < uu) step(l, ku);
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int rank = (tid + 256 * j) / (4 * CH);
            const int64_t u = u0 + uu;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (u < u_end && rank < r) {
                const int64_t k = ku * 16 + k4;
                const float* p = V + (int64_t)rank * ldv + l * K + k;
                if constexpr (VEC) {
                    if (k < K) v = *reinterpret_cast<const f32x4*>(p);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k + e < K) v[e] = p[e];
                }
            }
            vq[j] = v;
        }
    };
    auto store_v = [&](const f32x4 (&vq)[MT]) {
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int q = tid + 256 * j, rank = q / (4 * CH), uu = (q >> 2) % CH, k4 = 4 * (q & 3);
            *reinterpret_cast<f32x4*>(&Vs[(uu * RP + rank) * 16 + k4]) = vq[j];
        }
    };
    // this lane's four k (4g .. 4g+3) of row i in each unit of a chunk; krem[uu] = how many of them lie inside the tensor
    // (WT: their weights from the same offset of Wg)
    auto load_t = [&](int64_t u0, int64_t l0, int64_t ku0, f32x4 (&x)[CH], int (&krem)[CH], f32x4 (&wq)[WCH]) {
        int64_t l = l0, ku = ku0;
#pragma unroll
        for (int uu = 0; uu < CH; ++uu) {
            const int64_t u = u0 + uu;
            f32x4 v = {0.f, 0.f, 0.f, 0.f}, wv = {0.f, 0.f, 0.f, 0.f};
            int rem = 0;
            if (uu > 0) step(l, ku);
            if (u < u_end && row_ok) {
                const int64_t k = ku * 16 + 4 * g;
                const int64_t off = (l * I + i) * K + k;
                const float* p = T + off;
                rem = K - k > 4 ? 4 : (K - k > 0 ? (int)(K - k) : 0);
                if constexpr (VEC) {
                    if (rem > 0) v = *reinterpret_cast<const f32x4*>(p);
                    if constexpr (WT)
                        if (rem > 0) wv = *reinterpret_cast<const f32x4*>(Wg + off);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < rem) v[e] = p[e];
                    if constexpr (WT) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (e < rem) wv[e] = Wg[off + e];
                    }
                }
            }
            x[uu] = v;
            if constexpr (WT) wq[uu] = wv;
            krem[uu] = rem;
        }
    };

    f32x4 vq[MT], x[CH], wq[WCH];
    int krem[CH];
    int64_t ln = u_begin / kt, kun = u_begin - ln * kt;   // the chunk in flight starts at unit (ln, kun)
    load_v(u_begin, ln, kun, vq);
    load_t(u_begin, ln, kun, x, krem, wq);
    for (int64_t u0 = u_begin; u0 < u_end; u0 += CH) {
        __syncthreads();   // the previous chunk's reads are done
        store_v(vq);
        __syncthreads();
        f32x4 xc[CH], wc[WCH];
        int kc[CH];
#pragma unroll
        for (int uu = 0; uu < CH; ++uu) { xc[uu] = x[uu]; kc[uu] = krem[uu]; }
        if constexpr (WT) {
#pragma unroll
            for (int uu = 0; uu < CH; ++uu) wc[uu] = wq[uu];
        }
        if (u0 + CH < u_end) {   // the next chunk: in flight during this one's MFMAs
#pragma unroll
            for (int t = 0; t < CH; ++t) step(ln, kun);
            load_v(u0 + CH, ln, kun, vq);
            load_t(u0 + CH, ln, kun, x, krem, wq);
        }
#pragma unroll
        for (int uu = 0; uu < CH; ++uu) {
            // (no test for units beyond the split's end, nor for rank steps beyond r: their V is zero in LDS and their krem is 0,
            //  and a branch per unit or per step pins every LDS read behind a full wait right in front of its MFMA)
            const float* vu = &Vs[uu * RP * 16];
            // MFMA #1: accP[jj] = P[k = 4g + jj][i]
            f32x4 accP = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4 * MT; ++s)
                accP = MFMA16(vu[(4 * s + g) * 16 + c16], ftf[s], accP);
            f32x4 R1, R2;
            if constexpr (WT) {
                // a weight of zero takes the entry out of both sums whatever T holds there (a select: 0 * NaN would be NaN)
                auto body = [&](auto bs) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        float r1, r2;
                        const float wv = wc[uu][jj];
                        mu_elem_w<decltype(bs)::value>(xc[uu][jj], accP[jj], wv, beta, r1, r2);
                        const bool ok = jj < kc[uu] && wv > 0.f;
                        R1[jj] = ok ? r1 : 0.f;
                        R2[jj] = ok ? r2 : 0.f;
                    }
                };
                if (bsel == 1) body(nnf_int<1>{});
                else if (bsel == 2) body(nnf_int<2>{});
                else body(nnf_int<0>{});
            } else {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                float r1, r2;
                mu_mode_elem<KL>(xc[uu][jj], accP[jj], beta, beta2, r1, r2);
                const bool ok = jj < kc[uu];   // (0 for rows beyond I and units beyond the split)
                R1[jj] = ok ? r1 : 0.f;
                R2[jj] = ok ? r2 : 0.f;
            }
            }
            // MFMA #2: A[m = rank 16mt + c16][k slot g] = V[rank][k = 4g + jj], B[k slot g][n = i] = R[jj]
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(&vu[(16 * mt + c16) * 16 + 4 * g]);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    num[mt] = MFMA16(av[jj], R1[jj], num[mt]);
                    if constexpr (!KL) den[mt] = MFMA16(av[jj], R2[jj], den[mt]);
                }
            }
        }
    }
    // num[mt][jj]: rank 16mt + 4g + jj, row i
    if (row_ok) {
        float* on = snum + sp * ((int64_t)r * ldp) + i;
        float* od = KL ? nullptr : sden + sp * ((int64_t)r * ldp) + i;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int rank = 16 * mt + 4 * g + jj;
                if (rank < r) {
                    on[(int64_t)rank * ldp] = num[mt][jj];
                    if constexpr (!KL) od[(int64_t)rank * ldp] = den[mt][jj];
                }
            }
    }
}

template <int MT, bool KL, bool VEC>
static int launch_mu_mode(nnf_ctx* ctx, const float* T, int64_t L, int64_t I, int64_t K, const float* Ft, int64_t ldf,
                          const float* V, int64_t ldv, int r, double beta, float* out, int64_t ldo, hipStream_t st) {
    nnf_ws_cursor cur(ctx);
    const mu_mode_plan pl = mu_plan_mode(cur, ctx->num_cus, L, I, K, r, KL, VEC);
    if (pl.status != NNF_OK) return pl.status;
    if (nnf_plan_debug()) mu_report_mode(stderr, L, I, K, r, MT, VEC, KL, pl);
    const int64_t slab_elems = (int64_t)r * pl.ldp;
    double* dvec = (double*)cur.take((size_t)r * 8);
    double* part = pl.pieces > 1 ? (double*)cur.take((size_t)r * pl.pieces * 8) : nullptr;
    float* snum = (float*)cur.take((size_t)pl.nsplit * slab_elems * 4);
    float* sden = KL ? nullptr : (float*)cur.take((size_t)pl.nsplit * slab_elems * 4);
    if (!dvec || (pl.pieces > 1 && !part) || !snum || (!KL && !sden)) return NNF_ERR_WORKSPACE;   // (cannot happen: the plan took the same)
    if (KL) {   // den[k] = rowsum(V)[k]   (mu.py:86-87)
        const int rc = nnf_launch_rowsum_f64(part, pl.pieces, V, ldv, r, L * K, dvec, st);
        if (rc != NNF_OK) return rc;
    }
    hipLaunchKernelGGL((nnf_mu_mode_kernel<MT, KL, VEC>), dim3((unsigned)(pl.nrb * pl.nsplit)), dim3(256), 0, st, T, L, I, K, Ft, ldf,
                       V, ldv, r, (float)beta, snum, sden, pl.ldp, pl.nrb, pl.kt, pl.units, pl.ups);
    NNF_CHECK_LAUNCH();
    return nnf_launch_mu_finish(Ft, ldf, r, I, snum, sden, (int)pl.nsplit, slab_elems, pl.ldp, KL ? dvec : nullptr, beta, out, ldo, st);
}

template <bool KL, bool VEC, typename... A>
static int mu_mode_by_rank(int r, A... a) {
    switch ((r + 15) / 16) {
        case 1: return launch_mu_mode<1, KL, VEC>(a...);
        case 2: return launch_mu_mode<2, KL, VEC>(a...);
        case 3: return launch_mu_mode<3, KL, VEC>(a...);
        case 4: return launch_mu_mode<4, KL, VEC>(a...);
        default: return NNF_ERR_UNSUPPORTED;
    }
}

extern "C" int nnf_mu_mode_f32(nnf_ctx* ctx, const float* T, int64_t L, int64_t I, int64_t K, const float* Ft, int64_t ldf,
                               const float* V, int64_t ldv, int r, double beta, float* out, int64_t ldo, void* stream) {
    if (!ctx || !T || !Ft || !V || !out || L < 1 || I < 1 || K < 1 || r < 1 || !(beta >= 0.0)) return NNF_ERR_ARG;
    if ((double)L * (double)K >= 4.0e18) return NNF_ERR_UNSUPPORTED;
    if (ldf < I || ldv < L * K || ldo < I) return NNF_ERR_ARG;
    if (r > MU_MODE_MAX_RANK) return NNF_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = x_vec_ok(T, K) && x_vec_ok(V, ldv);
    const bool kl = beta == 1.0;
    if (kl) return vec ? mu_mode_by_rank<true, true>(r, ctx, T, L, I, K, Ft, ldf, V, ldv, r, beta, out, ldo, st)
                       : mu_mode_by_rank<true, false>(r, ctx, T, L, I, K, Ft, ldf, V, ldv, r, beta, out, ldo, st);
    return vec ? mu_mode_by_rank<false, true>(r, ctx, T, L, I, K, Ft, ldf, V, ldv, r, beta, out, ldo, st)
               : mu_mode_by_rank<false, false>(r, ctx, T, L, I, K, Ft, ldf, V, ldv, r, beta, out, ldo, st);
}

// ---- weighted form: the raw numerator and denominator of the mode update under a weight per entry ----
template <int MT, bool VEC>
static int launch_mu_mode_w(nnf_ctx* ctx, const float* T, const float* Wg, int64_t L, int64_t I, int64_t K, const float* Ft,
                            int64_t ldf, const float* V, int64_t ldv, int r, double beta, float* num, int64_t ldn, float* den,
                            int64_t ldd, hipStream_t st) {
    nnf_ws_cursor cur(ctx);
    const mu_mode_plan pl = mu_plan_mode(cur, ctx->num_cus, L, I, K, r, false, VEC, true);
    if (pl.status != NNF_OK) return pl.status;
    if (nnf_plan_debug()) mu_report_mode(stderr, L, I, K, r, MT, VEC, false, pl, "", true);
    const int64_t slab_elems = (int64_t)r * pl.ldp;
    float* snum = (float*)cur.take((size_t)pl.nsplit * slab_elems * 4);
    float* sden = (float*)cur.take((size_t)pl.nsplit * slab_elems * 4);
    if (!snum || !sden) return NNF_ERR_WORKSPACE;   // (cannot happen: the plan took the same)
    hipLaunchKernelGGL((nnf_mu_mode_kernel<MT, false, VEC, true>), dim3((unsigned)(pl.nrb * pl.nsplit)), dim3(256), 0, st, T, L, I, K,
                       Ft, ldf, V, ldv, r, (float)beta, snum, sden, pl.ldp, pl.nrb, pl.kt, pl.units, pl.ups, Wg);
    NNF_CHECK_LAUNCH();
    // the slabs of a split in split order, fp64 (one slab too: the same rounding whatever the split count)
    const nnf_reduce_set sets[2] = {nnf_plan_reduce_set(snum, (int)pl.nsplit, slab_elems, r, I, pl.ldp, num, ldn, nullptr),
                                    nnf_plan_reduce_set(sden, (int)pl.nsplit, slab_elems, r, I, pl.ldp, den, ldd, nullptr)};
    return nnf_launch_reduce_sets(sets, 2, st);   // both sets in one launch, each the bits of a reduction of its own
}

template <bool VEC, typename... A>
static int mu_mode_w_by_rank(int r, A... a) {
    switch ((r + 15) / 16) {
        case 1: return launch_mu_mode_w<1, VEC>(a...);
        case 2: return launch_mu_mode_w<2, VEC>(a...);
        case 3: return launch_mu_mode_w<3, VEC>(a...);
        case 4: return launch_mu_mode_w<4, VEC>(a...);
        default: return NNF_ERR_UNSUPPORTED;
    }
}

extern "C" int nnf_mu_mode_w_f32(nnf_ctx* ctx, const float* T, const float* Wg, int64_t L, int64_t I, int64_t K, const float* Ft,
                                 int64_t ldf, const float* V, int64_t ldv, int r, double beta, float* num, int64_t ldn,
                                 float* den, int64_t ldd, void* stream) {
    if (!ctx || !T || !Wg || !Ft || !V || !num || !den || L < 1 || I < 1 || K < 1 || r < 1 || !(beta >= 0.0)) return NNF_ERR_ARG;
    if ((double)L * (double)K >= 4.0e18) return NNF_ERR_UNSUPPORTED;
    if (ldf < I || ldv < L * K || ldn < I || ldd < I) return NNF_ERR_ARG;
    if (r > MU_MODE_MAX_RANK) return NNF_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = x_vec_ok(T, K) && x_vec_ok(Wg, K) && x_vec_ok(V, ldv);
    return vec ? mu_mode_w_by_rank<true>(r, ctx, T, Wg, L, I, K, Ft, ldf, V, ldv, r, beta, num, ldn, den, ldd, st)
               : mu_mode_w_by_rank<false>(r, ctx, T, Wg, L, I, K, Ft, ldf, V, ldv, r, beta, num, ldn, den, ldd, st);
}

// X H^T: out[r x m] = V[r x n] * X[m x n]^T  (nmf.py:408) with the fragments of X loaded straight into registers; ranks up to
// 32 go to the LDS-staged form of k_xht_lds.hip.  The design shared with W^T X, the Gram and the cost pass is described at the
// head of k_stream_common.h.
#include "k_gram_body.h"
#ifndef XHT_ABL
#define XHT_ABL 0   // timing-only ablations of nnf_xht_kernel (tools/xht_ablate.sh); 0 = the product
#endif
NNF_BUILD_FLAGS(k_xht, "XHT_ABL=" NNF_STR(XHT_ABL))

// =========================================================================================================
// xht: out[rk][i] = sum_j V[rk][j] * X[i][j]
//   workgroup = 256 rows of X (wave w: rows 64w..64w+63 as four 16-row N tiles), k runs over the n columns.
//   B operand lane (ii = l&15, g = l>>4) of tile nt, k-group t: float4 X[i0w+16nt+ii][64q+16t+4g .. +3].
// =========================================================================================================
// One 64-deep chunk of the contraction: the MFMAs of chunk q on its LDS image `img`, the leftover rank rows on the VALU pipe
// between them, X of chunk q + 1 reloaded in place behind the k-group that frees its registers and the image of chunk q + 1
// stored into `img_next` behind the last k-group.  RAGGED: the chunk may reach past column n -- the components at and beyond n
// are masked (never multiply a staged zero by out-of-row data: the allocated row padding may hold NaN).  Only the last chunk of
// a row can be that; the body of the chunk loop is the unmasked form: no compare, select or branch between its MFMAs.
template <int MT, int REM, bool VEC, int NT, bool RAGGED>
__device__ __forceinline__ void nnf_xht_chunk(const f32x4* __restrict__ img, f32x4* __restrict__ img_next, int q, int64_t n,
                                              const float* __restrict__ V, int64_t ldv, int r, int a_vec_ok, rsrc_t rs, int voff,
                                              int ldx4, int lane, int g, f32x4 (&acc)[MT][NT], f32x4 (&xb)[4][NT],
                                              float (&ev)[REM > 0 ? REM : 1][NT], f32x4 (&areg)[MT + (REM > 0 ? 1 : 0)]) {
    constexpr int MTA = MT + (REM > 0 ? 1 : 0);
    stageA_load<MTA>(V, ldv, r, n, 64 * (int64_t)(q + 1), a_vec_ok, areg);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f32x4 af[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = img[(mt * 4 + t) * 64 + lane];
        f32x4 uv[REM > 0 ? REM : 1];   // V[16MT+rr][64q+16t+4g+c], c = 0..3
        if constexpr (REM > 0 && XHT_ABL != 3) {
#pragma unroll
            for (int rr = 0; rr < REM; ++rr) uv[rr] = img[(MT * 4 + t) * 64 + 16 * g + rr];
        }
        f32x4 xs[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) xs[nt] = xb[t][nt];
        if constexpr (RAGGED && XHT_ABL != 5) {
            const int64_t nrem = n - (64 * (int64_t)q + 16 * t + 4 * g);
            if (nrem < 4) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c >= nrem) xs[nt][c] = 0.f;
            }
        }
        // component by component: the rank tiles on MFMA, then the leftover rows' FMAs of the same component (every chain of
        // ev still runs t, then c)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
#if XHT_ABL == 2
                    if (mt == 0) acc[0][nt][c] += af[0][c] * xs[nt][c];
#else
                    acc[mt][nt] = MFMA16(af[mt][c], xs[nt][c], acc[mt][nt]);
#endif
                }
            if constexpr (REM > 0 && XHT_ABL != 3) {
#pragma unroll
                for (int rr = 0; rr < REM; ++rr)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) ev[rr][nt] = fmaf(uv[rr][c], xs[nt][c], ev[rr][nt]);
            }
        }
        // finish the chains HERE: left alone, the scheduler sinks them (and the X registers they read) to the barrier
        if constexpr (REM > 0 && XHT_ABL != 3) {
#pragma unroll
            for (int rr = 0; rr < REM; ++rr)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) asm volatile("" : "+v"(ev[rr][nt]));
        }
#if XHT_ABL != 1
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) xb[t][nt] = nnf_bload4<VEC>(rs, voff, nt * 16 * ldx4 + 256 * (q + 1) + 64 * t);
#endif
        // keep every k-group's reloads and leftover-row FMAs inside the group (as in k_xty.hip; without the fence the four-tile
        // forms without leftover rows come out slower, DESIGN.md section 7 "X H^T chunk loop")
        __builtin_amdgcn_sched_barrier(0);
    }
#if XHT_ABL != 4
    stageA_store<MTA>(img_next, areg);
    __syncthreads();
#endif
}

// NT = 16-row tiles per wave (a workgroup covers 64*NT rows starting at row0).
template <int MT, int REM, bool VEC, int NT>
__device__ __forceinline__ void nnf_xht_body(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                             const float* __restrict__ V, int64_t ldv, int r, float* __restrict__ out,
                                             int64_t ldo, int a_vec_ok, int64_t row0, f32x4 (*ldsA)[(MT + (REM > 0 ? 1 : 0)) * 256],
                                             int q0 = 0, int q1 = -1, int64_t oshift = 0) {
    // [q0, q1): the 64-column chunks this call contracts (default: all of them; a sub-range = a k-split share, see the kernel);
    // row i of the result goes to column i - oshift of `out` (a share's slab starts at the first k-split row)
    constexpr int MTA = MT + (REM > 0 ? 1 : 0);
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ii = lane & 15, g = lane >> 4;
    const int64_t i0w = row0 + 16 * NT * w;
    int64_t rows = m - i0w;
    if (rows > 16 * NT) rows = 16 * NT;
    const uint32_t bytes = rows > 0 ? (uint32_t)(((rows - 1) * ldx + n) * 4) : 0u;
    const rsrc_t rs = nnf_make_rsrc(X + (rows > 0 ? i0w : 0) * ldx, bytes);
    const int voff = (int)(((int64_t)ii * ldx + 4 * g) * 4);
    const int ldx4 = (int)(ldx * 4);
    const int nchunk = q1 >= 0 ? q1 : (int)((n + 63) >> 6);
    // chunks [q0, nwhole) lie wholly inside n; the one behind them, where the range holds it, is the ragged end of the row
    const int nwhole = (n >> 6) < nchunk ? (int)(n >> 6) : nchunk;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 xb[4][NT];  // [k-group t][row tile nt]
    f32x4 areg[MTA];
    float ev[REM > 0 ? REM : 1][NT];   // leftover rank rows x the 16-row tiles: partial over this lane's k
#pragma unroll
    for (int rr = 0; rr < (REM > 0 ? REM : 1); ++rr)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) ev[rr][nt] = 0.f;

    stageA_load<MTA>(V, ldv, r, n, 64 * (int64_t)q0, a_vec_ok, areg);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) xb[t][nt] = nnf_bload4<VEC>(rs, voff, nt * 16 * ldx4 + 256 * q0 + 64 * t);
    stageA_store<MTA>(ldsA[0], areg);
    __syncthreads();

#define NNF_XHT_CHUNK(RAGGED, FROM, TO, Q) \
    nnf_xht_chunk<MT, REM, VEC, NT, RAGGED>(ldsA[FROM], ldsA[TO], Q, n, V, ldv, r, a_vec_ok, rs, voff, ldx4, lane, g, acc, xb, ev, areg)
    // the first chunk of the range sits in image 0
    int q = q0, from = 0;
    if constexpr (NT > 1) {
        // two chunks per trip: each half names its LDS image as a constant
        for (; q + 2 <= nwhole; q += 2) {
            NNF_XHT_CHUNK(false, 0, 1, q);
            NNF_XHT_CHUNK(false, 1, 0, q + 1);
        }
        if (q < nwhole) {   // odd count of whole chunks
            NNF_XHT_CHUNK(false, 0, 1, q);
            ++q;
            from = 1;
        }
    } else {
        // the one-tile body of the k-split shares (a few chunks each, one at config B): one chunk per trip as before -- sixteen
        // MFMAs per rank tile do not cover the loads of a trip whichever way it is unrolled
        for (; q < nwhole; ++q, from ^= 1) NNF_XHT_CHUNK(false, from, from ^ 1, q);
    }
    if (q < nchunk) NNF_XHT_CHUNK(true, from, from ^ 1, q);
#undef NNF_XHT_CHUNK

    // epilogue: tile (mt, nt): out[16mt + 4g + reg][i0w + 16nt + ii]
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int64_t i = i0w + 16 * nt + ii;
        if (i < m) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int rk = 16 * mt + 4 * g + reg;
                    if (rk < r) out[(int64_t)rk * ldo + (i - oshift)] = acc[mt][nt][reg];
                }
        }
    }
    if constexpr (REM > 0) {
#pragma unroll
        for (int rr = 0; rr < REM; ++rr)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float x = ev[rr][nt];
                x += __shfl_xor(x, 16, 64);
                x += __shfl_xor(x, 32, 64);
                const int64_t i = i0w + 16 * nt + ii;
                const int rk = 16 * MT + rr;
                if (g == 0 && rk < r && i < m) out[(int64_t)rk * ldo + (i - oshift)] = x;
            }
    }
}

// A resident wave is the unit the MFMA pipe is shared in, and one round of workgroups covers B's 100000 rows: with
// 64 rows per wave everywhere that is 1563 waves on 1024 SIMDs -- the SIMDs holding two of them decide the time
// (8 row tiles against 6.1 on average).  The first n_hi workgroups take NTH tiles per wave, the others NTH-1, chosen
// on the host so that one full round of resident workgroups covers the matrix (7 tiles on the busiest SIMD).
// b: the workgroup's index in the X H^T grid; ldsA: its two chunk images
template <int MT, int REM, bool VEC, int NTH>
__device__ __forceinline__ void nnf_xht_wg(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                           const float* __restrict__ V, int64_t ldv, int r,
                                           float* __restrict__ out, int64_t ldo, int a_vec_ok, int n_hi,
                                           float* __restrict__ tail_slabs, int64_t tail_row0, int64_t tail_ld,
                                           int tail_tiles, int tail_parts, int tail_cpp, int b,
                                           f32x4 (*ldsA)[(MT + (REM > 0 ? 1 : 0)) * 256]) {
    if (b < n_hi)
        nnf_xht_body<MT, REM, VEC, NTH>(X, m, n, ldx, V, ldv, r, out, ldo, a_vec_ok, (int64_t)b * (64 * NTH), ldsA);
    else
        nnf_xht_body<MT, REM, VEC, NTH - 1>(X, m, n, ldx, V, ldv, r, out, ldo, a_vec_ok,
                                            (int64_t)n_hi * (64 * NTH) + (int64_t)(b - n_hi) * (64 * (NTH - 1)), ldsA);
    // k-split tail (launch_xht): the row tiles that do not fill another whole round -- 106 of config B's 6250 -- are shared by ALL
    // workgroups instead of making 27 of them a third longer: workgroup b takes chunk share p = b % parts of the four tiles
    // 4 (b / parts) + wave, into slab p; the shares are added in share order by the usual slab reduction.
    if (tail_parts > 0) {
        const int p = b % tail_parts, tg = b / tail_parts;
        if (4 * tg < tail_tiles) {
            __syncthreads();
            const int nchunk_all = (int)((n + 63) >> 6);
            const int q0 = p * tail_cpp, q1 = (q0 + tail_cpp < nchunk_all) ? q0 + tail_cpp : nchunk_all;
            nnf_xht_body<MT, REM, VEC, 1>(X, m, n, ldx, V, ldv, r, tail_slabs + (int64_t)p * r * tail_ld, tail_ld, a_vec_ok,
                                          tail_row0 + 64 * (int64_t)tg, ldsA, q0 < q1 ? q0 : q1, q1, tail_row0);
        }
    }
}

#define NNF_XHT_BOUNDS __launch_bounds__(256, (MT + (REM > 0) <= 4 || NTH <= 2 ? 2 : 1))
template <int MT, int REM, bool VEC, int NTH>
__global__ NNF_XHT_BOUNDS void nnf_xht_kernel(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                              const float* __restrict__ V, int64_t ldv, int r,
                                              float* __restrict__ out, int64_t ldo, int a_vec_ok, int n_hi,
                                              float* __restrict__ tail_slabs, int64_t tail_row0, int64_t tail_ld,
                                              int tail_tiles, int tail_parts, int tail_cpp) {
    __shared__ f32x4 ldsA[2][(MT + (REM > 0 ? 1 : 0)) * 256];
    nnf_xht_wg<MT, REM, VEC, NTH>(X, m, n, ldx, V, ldv, r, out, ldo, a_vec_ok, n_hi, tail_slabs, tail_row0, tail_ld, tail_tiles,
                                  tail_parts, tail_cpp, (int)blockIdx.x, ldsA);
}

// X H^T with the Gram of its left factor riding in the same launch (nnf_xht_gram_f32): workgroups [0, main_grid) are the cross
// product's (tail shares included), workgroup main_grid + s forms split s of V V^T (k_gram_body.h) in the same LDS -- the Gram
// stages the same MT + (REM > 0) tiles of V.  Same bodies, same plans: the bits of the two launches of their own.
template <int MT, int REM, bool VEC, int NTH>
__global__ NNF_XHT_BOUNDS void nnf_xht_gram_kernel(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                                   const float* __restrict__ V, int64_t ldv, int r,
                                                   float* __restrict__ out, int64_t ldo, int a_vec_ok, int n_hi,
                                                   float* __restrict__ tail_slabs, int64_t tail_row0, int64_t tail_ld,
                                                   int tail_tiles, int tail_parts, int tail_cpp, int main_grid,
                                                   float* __restrict__ gslabs, int64_t g_kps) {
    constexpr int MTA = MT + (REM > 0 ? 1 : 0);
    __shared__ f32x4 ldsA[2][MTA * 256];
    const int b = (int)blockIdx.x;
    if (b < main_grid)
        nnf_xht_wg<MT, REM, VEC, NTH>(X, m, n, ldx, V, ldv, r, out, ldo, a_vec_ok, n_hi, tail_slabs, tail_row0, tail_ld, tail_tiles,
                                      tail_parts, tail_cpp, b, ldsA);
    else
        nnf_gram_body<MTA>(V, r, n, ldv, gslabs, g_kps, a_vec_ok, b - main_grid, ldsA);
}

template <int MT, int REM, bool VEC>
static int launch_xht(nnf_ctx* ctx, nnf_ws_cursor& cur, const float* X, int64_t m, int64_t n, int64_t ldx, const float* V, int r, int64_t ldv,
                      float* out, int64_t ldo, hipStream_t st, nnf_gram_ride* ride) {
    if (!nnf_xht_offsets_ok(n, ldx)) return NNF_ERR_UNSUPPORTED;
    static const int nt2 = [] { const char* e = getenv("NNF_XHT_NT2"); return e ? atoi(e) : -1; }();
    static const int tail_on = [] { const char* e = getenv("NNF_XHT_TAIL"); return e ? atoi(e) : 1; }();
    const size_t free_bytes = cur.remaining();
    const nnf_xht_plan pl = nnf_plan_xht_direct(ctx->num_cus, m, n, r, nnf_rank_tiles{MT, REM}, nt2, tail_on, free_bytes);
    if (!pl.covers(m)) return NNF_ERR_UNSUPPORTED;   // (cannot happen: the split covers m by construction)
    if (nnf_plan_debug()) nnf_report_xht(stderr, m, n, r, nnf_rank_tiles{MT, REM}, VEC, false, pl);
    const int a_vec_ok = x_vec_ok(V, ldv) ? 1 : 0;
    const size_t tail_bytes = pl.tail_parts > 0 ? (size_t)pl.tail_parts * r * pl.tail_ld * 4 : 0;
    nnf_gram_plan gp{};
    nnf_rider_plan rp{};
    if (ride) {   // the Gram's plan as a call of its own makes it: against the whole free workspace
        gp = nnf_plan_gram(ctx->num_cus, r, n, ride->ldg == r, a_vec_ok, free_bytes);
        rp = nnf_plan_rider(pl.grid, tail_bytes, gp, r, MT + (REM > 0 ? 1 : 0), free_bytes);
        if (nnf_plan_debug()) nnf_report_rider(stderr, "xht_gram", rp);
    }
    const bool rides = ride && rp.rides;
    float* tail_slabs = pl.tail_parts > 0 ? (float*)cur.take(tail_bytes) : nullptr;
    if (pl.tail_parts > 0 && !tail_slabs) return NNF_ERR_WORKSPACE;   // (cannot happen: the plan counted them)
    float* gslabs = rides ? (float*)cur.take(rp.rider_bytes) : nullptr;
    if (rides && !gslabs) return NNF_ERR_WORKSPACE;   // (cannot happen: nnf_plan_rider counted both carves)
    if (rides && nnf_plan_debug()) nnf_report_gram(stderr, r, n, gp);
    nnf_probe(ctx, NNF_PROBE_XHT, 0, st);   // (with its rider, where one comes along)
#define NNF_XHT_GO(NTH)                                                                                                               \
    do {                                                                                                                              \
        if (rides)                                                                                                                    \
            hipLaunchKernelGGL((nnf_xht_gram_kernel<MT, REM, VEC, NTH>), dim3((int)rp.grid), dim3(256), 0, st, X, m, n, ldx, V, ldv, r, \
                               out, ldo, a_vec_ok, (int)pl.n_hi, tail_slabs, pl.tail_row0, pl.tail_ld, pl.tail_tiles, pl.tail_parts,  \
                               pl.tail_cpp, (int)pl.grid, gslabs, gp.kps);                                                           \
        else                                                                                                                          \
            hipLaunchKernelGGL((nnf_xht_kernel<MT, REM, VEC, NTH>), dim3((int)pl.grid), dim3(256), 0, st, X, m, n, ldx, V, ldv, r, out, \
                               ldo, a_vec_ok, (int)pl.n_hi, tail_slabs, pl.tail_row0, pl.tail_ld, pl.tail_tiles, pl.tail_parts,       \
                               pl.tail_cpp);                                                                                          \
    } while (0)
    if (pl.nth == 4) NNF_XHT_GO(4);
    else if (pl.nth == 2) {
        if constexpr (MT + (REM > 0) > 4) NNF_XHT_GO(2);
    } else NNF_XHT_GO(3);
#undef NNF_XHT_GO
    NNF_CHECK_LAUNCH();
    nnf_probe(ctx, NNF_PROBE_XHT, 1, st);
    // the k-split shares of the last rows, added in share order, and the rider's splits: one launch
    nnf_reduce_set sets[2];
    int nsets = 0;
    if (pl.tail_parts > 0)
        sets[nsets++] = nnf_plan_reduce_set(tail_slabs, pl.tail_parts, (int64_t)r * pl.tail_ld, r, m - pl.tail_row0, pl.tail_ld,
                                            out + pl.tail_row0, ldo);
    if (rides) {
        sets[nsets++] = nnf_plan_reduce_set(gslabs, (int)gp.nsplit, (int64_t)r * r, r, r, r, ride->G, ride->ldg, ride->G64);
        ride->rode = true;
    }
    return nsets > 0 ? nnf_launch_reduce_sets(sets, nsets, st) : NNF_OK;
}

int nnf_xht_lds_launch(nnf_ctx* ctx, int MT, int REM, const float* X, int64_t m, int64_t n, int64_t ldx, const float* V, int r,
                       int64_t ldv, float* out, int64_t ldo, hipStream_t st);   // k_xht_lds.hip
int nnf_xht_impl(nnf_ctx* ctx, nnf_ws_cursor& cur, const float* X, int64_t m, int64_t n, int64_t ldx, const float* V,
                 int r, int64_t ldv, float* out, int64_t ldo, hipStream_t st, nnf_gram_ride* ride) {
    if (!ctx || !X || !V || !out || m < 1 || n < 1 || r < 1 || ldx < n || ldv < n || ldo < m) return NNF_ERR_ARG;
    if (r > NNF_MAX_RANK)   // the rows of the result are independent of each other
        return nnf_rank_passes(r, cur, [&](int k0, int rc) {
            return nnf_xht_impl(ctx, cur, X, m, n, ldx, V + (int64_t)k0 * ldv, rc, ldv, out + (int64_t)k0 * ldo, ldo, st);
        });
    const bool vec = x_vec_ok(X, ldx);
    const nnf_rank_tiles t = nnf_xht_tiles(r, vec);
    const char* pick = getenv("NNF_XHT");       // measurement knob: "direct" keeps the register-fragment kernel
    if (nnf_xht_use_lds(t, vec) && !(pick && pick[0] == 'd'))
        return nnf_xht_lds_launch(ctx, t.MT, t.REM, X, m, n, ldx, V, r, ldv, out, ldo, st);
    return nnf_dispatch<8>(t.MT, [&](auto mt) -> int {
        constexpr int MT = decltype(mt)::value;
        const auto go = [&](auto rem, auto v) {
            return launch_xht<MT, decltype(rem)::value, decltype(v)::value>(ctx, cur, X, m, n, ldx, V, r, ldv, out, ldo, st, ride);
        };
        if (!vec) return go(nnf_int<0>{}, std::false_type{});
        if (t.REM == 2) return go(nnf_int<2>{}, std::true_type{});
        if (t.REM == 4) return go(nnf_int<4>{}, std::true_type{});
        return go(nnf_int<0>{}, std::true_type{});
    });
}
extern "C" int nnf_xht_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* V, int r,
                           int64_t ldv, float* out, int64_t ldo, void* stream) {
    if (!ctx) return NNF_ERR_ARG;
    nnf_ws_cursor cur(ctx);
    return nnf_xht_impl(ctx, cur, X, m, n, ldx, V, r, ldv, out, ldo, (hipStream_t)stream);
}
// X H^T and the Gram of its left factor, G = V V^T (pitch ldg), in one main launch and one reduction where nnf_plan_rider lets
// the Gram ride (the register-fragment kernel: ranks above 32), as two calls otherwise: the bits of nnf_xht_f32 + nnf_gram_f32
// either way.
extern "C" int nnf_xht_gram_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* V, int r,
                                int64_t ldv, float* out, int64_t ldo, float* G, int64_t ldg, void* stream) {
    if (!ctx || !V || !G || r < 1 || n < 1 || ldv < n || ldg < r) return NNF_ERR_ARG;
    nnf_gram_ride ride{G, ldg, nullptr, false};
    nnf_ws_cursor cur(ctx);
    const int rc = nnf_xht_impl(ctx, cur, X, m, n, ldx, V, r, ldv, out, ldo, (hipStream_t)stream, &ride);
    if (rc != NNF_OK || ride.rode) return rc;
    nnf_ws_cursor gcur(ctx);   // (same stream: the Gram takes the workspace the cross product has finished with)
    return nnf_gram_impl(ctx, gcur, V, r, n, ldv, G, ldg, (hipStream_t)stream, nullptr);
}

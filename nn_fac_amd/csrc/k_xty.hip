// W^T X: out[r x n] = Ut[r x m] * X[m x n]  (nmf.py:433), split over m, the slabs added by k_reduce.hip.
// The design shared with X H^T, the Gram and the cost pass is described at the head of k_stream_common.h.
#include "k_gram_body.h"
#ifndef XTY_BIG_WG
#define XTY_BIG_WG 2   // resident workgroups per CU the W^T X kernel of five or six rank tiles is compiled for (A/B: tools/abl_build.sh)
#endif
NNF_BUILD_FLAGS(k_xty, "XTY_BIG_WG=" NNF_STR(XTY_BIG_WG))

// =========================================================================================================
// xty: slab[ks][rk][j] = sum_{i in split ks} Ut[rk][i] * X[i][j]
//   grid: 8*ceil(nsplit/8)*ncb workgroups of 256 threads; workgroup = (row split ks, 256-column block cb);
//   wave w owns columns cb*256 + 64w .. +63 (lane: 4*(l&15)+c), all MT row tiles; k runs over the split's rows.
// =========================================================================================================
// REM > 0: rank = 16*MT + (1..REM) -- the MT full 16-row tiles run on MFMA, the REM leftover rows on the VALU pipe, which
// is otherwise idle here (fp32 MFMA and fp32 VALU have the same peak on gfx950, so padding r=50 to 64 would burn 22 % of
// the MFMA time on zeros).  The leftover rows' operand is the (MT+1)-th tile of the same LDS image, read as a broadcast.
// bid: the workgroup's index in the cross-product grid; ldsA: its two chunk images
template <int MT, int REM, bool VEC>
__device__ __forceinline__ void nnf_xty_body(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                             const float* __restrict__ Ut, int64_t ldu, int r,
                                             float* __restrict__ slabs, int64_t ldp, int ncb, int nsplit,
                                             int64_t rows_per_split, int a_vec_ok, int bid,
                                             f32x4 (*ldsA)[(MT + (REM > 0 ? 1 : 0)) * 256]) {
    constexpr int MTA = MT + (REM > 0 ? 1 : 0);   // tiles staged in LDS
    int ks, cb;
    nnf_xcd_map(bid, ncb, ks, cb);
    if (ks >= nsplit) return;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jj = lane & 15, g = lane >> 4;
    const int64_t i_begin = (int64_t)ks * rows_per_split;
    const int64_t i_end = (i_begin + rows_per_split < m) ? (i_begin + rows_per_split) : m;
    const int nchunk = (int)((i_end - i_begin + 63) >> 6);
    const int64_t jl = (int64_t)cb * 256 + w * 64 + 4 * jj;  // lane's first column

    const rsrc_t rs = nnf_make_rsrc(X + i_begin * ldx, (uint32_t)(((i_end - i_begin - 1) * ldx + n) * 4));
    // lanes whose columns lie outside the matrix read nothing (offset beyond num_records -> 0)
    const int voff = (jl < n) ? (int)(((int64_t)4 * g * ldx + jl) * 4) : (int)0x7ffffff0;
    const int ldx4 = (int)(ldx * 4);

    f32x4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) acc[mt][cc] = f32x4{0.f, 0.f, 0.f, 0.f};

    // X prefetch ring: two 16-row groups (8 KB per wave) ahead of the MFMAs; with three workgroups per CU and the
    // per-group scheduling fence below that is enough in flight, and it keeps the kernel under 168 VGPRs without spills
    f32x4 xb[2][4];  // [group parity][k-step c]: row i_begin + 16*gi + 4g + c, columns jl..jl+3
    f32x4 areg[MTA];
    f32x4 ev[REM > 0 ? REM : 1];   // leftover rows: partial sums over this lane's rows, columns jl..jl+3
#pragma unroll
    for (int rr = 0; rr < (REM > 0 ? REM : 1); ++rr) ev[rr] = f32x4{0.f, 0.f, 0.f, 0.f};

    stageA_load<MTA>(Ut, ldu, r, i_end, i_begin, a_vec_ok, areg);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) xb[t][c] = nnf_bload4<VEC>(rs, voff, (16 * t + c) * ldx4);
    stageA_store<MTA>(ldsA[0], areg);
    __syncthreads();

    for (int q = 0; q < nchunk; ++q) {
        const f32x4* img = ldsA[q & 1];
        // next chunk's A tile: global loads now, LDS write after the MFMAs (rows past i_end come back as zeros)
        stageA_load<MTA>(Ut, ldu, r, i_end, i_begin + 64 * (int64_t)(q + 1), a_vec_ok, areg);
        const int soff_q = q * 64 * ldx4;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            f32x4 af[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[mt] = img[(mt * 4 + t) * 64 + lane];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) acc[mt][cc] = MFMA16(af[mt][c], xb[t & 1][c][cc], acc[mt][cc]);
            if constexpr (REM > 0) {
#pragma unroll
                for (int rr = 0; rr < REM; ++rr) {
                    const f32x4 uv = img[(MT * 4 + t) * 64 + 16 * g + rr];   // Ut[16MT+rr][row 16t+4g+c], c = 0..3
#pragma unroll
                    for (int c = 0; c < 4; ++c) ev[rr] = __builtin_elementwise_fma(f32x4{uv[c], uv[c], uv[c], uv[c]}, xb[t & 1][c], ev[rr]);
                }
            }
            // refill the registers just consumed with the rows two groups ahead (past the end: zeros)
#pragma unroll
            for (int c = 0; c < 4; ++c) xb[t & 1][c] = nnf_bload4<VEC>(rs, voff, soff_q + (16 * (t + 2) + c) * ldx4);
            // keep every group's loads and leftover-row FMAs inside the group: without the fence hipcc moves all 16 refill
            // loads and the whole VALU part to the end of the chunk, where nothing is left to hide them behind
            __builtin_amdgcn_sched_barrier(0);
        }
        stageA_store<MTA>(const_cast<f32x4*>(ldsA[(q + 1) & 1]), areg);
        __syncthreads();
    }

    // epilogue: D[row = 4g+reg][col = jj] of tile (mt, cc) is out[16mt+4g+reg][jl+cc] -> one float4 per (mt, reg)
    if (jl < ldp) {
        float* sl = slabs + (int64_t)ks * r * ldp;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int rk = 16 * mt + 4 * g + reg;
                if (rk < r) {
                    f32x4 o = {acc[mt][0][reg], acc[mt][1][reg], acc[mt][2][reg], acc[mt][3][reg]};
                    *reinterpret_cast<f32x4*>(sl + (int64_t)rk * ldp + jl) = o;
                }
            }
    }
    if constexpr (REM > 0) {   // sum the four row groups (lanes l, l^16, l^32, l^48), lanes of group 0 store
        float* sl = slabs + (int64_t)ks * r * ldp;
#pragma unroll
        for (int rr = 0; rr < REM; ++rr) {
            f32x4 e = ev[rr];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float x = e[c];
                x += __shfl_xor(x, 16, 64);
                x += __shfl_xor(x, 32, 64);
                e[c] = x;
            }
            const int rk = 16 * MT + rr;
            if (g == 0 && rk < r && jl < ldp) *reinterpret_cast<f32x4*>(sl + (int64_t)rk * ldp + jl) = e;
        }
    }
}

template <int MT, int REM, bool VEC>
__global__ __launch_bounds__(256, (nnf_xty_wg_per_cu(MT, REM, XTY_BIG_WG))) void nnf_xty_kernel(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                                         const float* __restrict__ Ut, int64_t ldu, int r,
                                                         float* __restrict__ slabs, int64_t ldp, int ncb, int nsplit,
                                                         int64_t rows_per_split, int a_vec_ok) {
    __shared__ f32x4 ldsA[2][(MT + (REM > 0 ? 1 : 0)) * 256];
    nnf_xty_body<MT, REM, VEC>(X, m, n, ldx, Ut, ldu, r, slabs, ldp, ncb, nsplit, rows_per_split, a_vec_ok, (int)blockIdx.x, ldsA);
}

// W^T X with the Gram of its left factor riding in the same launch (nnf_xty_gram_f32): workgroups [0, main_grid) are the cross
// product's, workgroup main_grid + s forms split s of Ut Ut^T (k_gram_body.h) in the same LDS -- the Gram stages the same
// MT + (REM > 0) tiles of Ut.  Same bodies, same plans: every slab is the bits the two launches of their own write.
template <int MT, int REM, bool VEC>
__global__ __launch_bounds__(256, (nnf_xty_wg_per_cu(MT, REM, XTY_BIG_WG))) void nnf_xty_gram_kernel(const float* __restrict__ X, int64_t m, int64_t n, int64_t ldx,
                                                         const float* __restrict__ Ut, int64_t ldu, int r,
                                                         float* __restrict__ slabs, int64_t ldp, int ncb, int nsplit,
                                                         int64_t rows_per_split, int a_vec_ok, int main_grid,
                                                         float* __restrict__ gslabs, int64_t g_kps) {
    constexpr int MTA = MT + (REM > 0 ? 1 : 0);
    __shared__ f32x4 ldsA[2][MTA * 256];
    const int b = (int)blockIdx.x;
    if (b < main_grid)
        nnf_xty_body<MT, REM, VEC>(X, m, n, ldx, Ut, ldu, r, slabs, ldp, ncb, nsplit, rows_per_split, a_vec_ok, b, ldsA);
    else
        nnf_gram_body<MTA>(Ut, r, m, ldu, gslabs, g_kps, a_vec_ok, b - main_grid, ldsA);
}

// plan (k_stream_plan.h; a refusal launches nothing), report, carve, launch, reduce.  ride: the Gram of Ut asked to come along
// (nnf_plan_rider decides; where it does not ride, ride->rode stays false and the caller runs the Gram on its own).
template <int MT, int REM, bool VEC>
static int launch_xty(nnf_ctx* ctx, nnf_ws_cursor& cur, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int r,
                      int64_t ldu, float* out, int64_t ldo, hipStream_t st, nnf_gram_ride* ride) {
    const size_t free_bytes = cur.remaining();
    const nnf_split_plan pl = nnf_plan_xty(ctx->num_cus, m, n, ldx, r, nnf_rank_tiles{MT, REM}, XTY_BIG_WG, free_bytes);
    if (pl.status != NNF_OK) return pl.status;
    if (nnf_plan_debug()) nnf_report_xty(stderr, m, n, r, nnf_rank_tiles{MT, REM}, VEC, pl);
    const int ncb = (int)nnf_cdiv(n, 256), nsplit = (int)pl.nsplit;
    const int64_t ldp = nnf_rup(n, 4), slab_elems = (int64_t)r * ldp;
    const int a_vec_ok = x_vec_ok(Ut, ldu) ? 1 : 0;
    const int main_grid = nnf_split_grid(nsplit, ncb);
    nnf_gram_plan gp{};
    nnf_rider_plan rp{};
    if (ride) {   // the Gram's plan as a call of its own makes it: against the whole free workspace
        gp = nnf_plan_gram(ctx->num_cus, r, m, ride->ldg == r, a_vec_ok, free_bytes);
        rp = nnf_plan_rider(main_grid, (size_t)nsplit * slab_elems * 4, gp, r, MT + (REM > 0 ? 1 : 0), free_bytes);
        if (nnf_plan_debug()) nnf_report_rider(stderr, "xty_gram", rp);
    }
    float* slabs = (float*)cur.take((size_t)nsplit * slab_elems * 4);
    if (!slabs) return NNF_ERR_WORKSPACE;   // (cannot happen: the plan counted them)
    if (ride && rp.rides) {
        if (nnf_plan_debug()) nnf_report_gram(stderr, r, m, gp);
        float* gslabs = (float*)cur.take(rp.rider_bytes);
        if (!gslabs) return NNF_ERR_WORKSPACE;   // (cannot happen: nnf_plan_rider counted both carves)
        nnf_probe(ctx, NNF_PROBE_XTY, 0, st);   // measurement hook: the main kernel, now with its rider (bench.py)
        hipLaunchKernelGGL((nnf_xty_gram_kernel<MT, REM, VEC>), dim3((int)rp.grid), dim3(256), 0, st, X, m, n, ldx, Ut, ldu, r,
                           slabs, ldp, ncb, nsplit, pl.rows_per_split, a_vec_ok, main_grid, gslabs, gp.kps);
        NNF_CHECK_LAUNCH();
        nnf_probe(ctx, NNF_PROBE_XTY, 1, st);
        const nnf_reduce_set sets[2] = {
            nnf_plan_reduce_set(slabs, nsplit, slab_elems, r, n, ldp, out, ldo),
            nnf_plan_reduce_set(gslabs, (int)gp.nsplit, (int64_t)r * r, r, r, r, ride->G, ride->ldg, ride->G64)};
        ride->rode = true;
        return nnf_launch_reduce_sets(sets, 2, st);
    }
    nnf_probe(ctx, NNF_PROBE_XTY, 0, st);   // measurement hook: the main kernel alone (bench.py)
    hipLaunchKernelGGL((nnf_xty_kernel<MT, REM, VEC>), dim3(main_grid), dim3(256), 0, st, X, m, n, ldx, Ut, ldu, r,
                       slabs, ldp, ncb, nsplit, pl.rows_per_split, a_vec_ok);
    NNF_CHECK_LAUNCH();
    nnf_probe(ctx, NNF_PROBE_XTY, 1, st);
    return nnf_launch_reduce_slabs(slabs, nsplit, slab_elems, r, n, ldp, out, ldo, st);
}

int nnf_xty_impl(nnf_ctx* ctx, nnf_ws_cursor& cur, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut,
                 int r, int64_t ldu, float* out, int64_t ldo, hipStream_t st, nnf_gram_ride* ride) {
    if (!ctx || !X || !Ut || !out || m < 1 || n < 1 || r < 1 || ldx < n || ldu < m || ldo < n) return NNF_ERR_ARG;
    if (r > NNF_MAX_RANK)   // the rows of the result are independent of each other (no rider: the Gram runs in blocks there)
        return nnf_rank_passes(r, cur, [&](int k0, int rc) {
            return nnf_xty_impl(ctx, cur, X, m, n, ldx, Ut + (int64_t)k0 * ldu, rc, ldu, out + (int64_t)k0 * ldo, ldo, st);
        });
    const bool vec = x_vec_ok(X, ldx);
    const nnf_rank_tiles t = nnf_xty_tiles(r, vec);
    return nnf_dispatch<8>(t.MT, [&](auto mt) -> int {
        constexpr int MT = decltype(mt)::value;
        const auto go = [&](auto rem, auto v) {
            return launch_xty<MT, decltype(rem)::value, decltype(v)::value>(ctx, cur, X, m, n, ldx, Ut, r, ldu, out, ldo, st, ride);
        };
        if (!vec) return go(nnf_int<0>{}, std::false_type{});
        if (t.REM == 2) return go(nnf_int<2>{}, std::true_type{});
        if (t.REM == 4) return go(nnf_int<4>{}, std::true_type{});
        return go(nnf_int<0>{}, std::true_type{});
    });
}
extern "C" int nnf_xty_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int r,
                           int64_t ldu, float* out, int64_t ldo, void* stream) {
    if (!ctx) return NNF_ERR_ARG;
    nnf_ws_cursor cur(ctx);
    return nnf_xty_impl(ctx, cur, X, m, n, ldx, Ut, r, ldu, out, ldo, (hipStream_t)stream);
}
// W^T X and the Gram of its left factor, G = Ut Ut^T (pitch ldg; G64: its fp64 sums, may be NULL), in one main launch and one
// reduction where nnf_plan_rider lets the Gram ride, as two calls otherwise: the bits of nnf_xty_f32 + nnf_gram_f32 /
// nnf_gram_f64_f32 either way.
extern "C" int nnf_xty_gram_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int r,
                                int64_t ldu, float* out, int64_t ldo, float* G, int64_t ldg, double* G64, void* stream) {
    if (!ctx || !Ut || !G || r < 1 || m < 1 || ldu < m || ldg < r) return NNF_ERR_ARG;
    nnf_gram_ride ride{G, ldg, G64, false};
    nnf_ws_cursor cur(ctx);
    const int rc = nnf_xty_impl(ctx, cur, X, m, n, ldx, Ut, r, ldu, out, ldo, (hipStream_t)stream, &ride);
    if (rc != NNF_OK || ride.rode) return rc;
    nnf_ws_cursor gcur(ctx);   // (same stream: the Gram takes the workspace the cross product has finished with)
    return nnf_gram_impl(ctx, gcur, Ut, r, m, ldu, G, ldg, (hipStream_t)stream, G64);
}

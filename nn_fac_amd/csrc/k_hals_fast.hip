// Fast HALS sweep kernels: one lane = one column of V, column resident in VGPRs, Gram through the scalar cache.
// Compiled once per part, -DHALS_PART=p (k_parts.h; each part instantiates the padded ranks HALS_TABLE gives it), so the parts build
// in parallel.  See k_hals.hip for the algorithm, the grid-exchange protocol and the entry points.
#include "k_hals_common.h"
#include "k_hals_lane_sweep.h"   // the row-split sweep of ranks 33 .. 64 (shared with k_hals_comm.hip)
#include "k_parts.h"

#ifndef HALS_PART
#error "compile with -DHALS_PART=<part>"
#endif
#define NNF_PART HALS_PART

NNF_BUILD_FLAGS(NNF_CAT(k_hals_fast, HALS_PART), "HALS_LATE_ISSUE=" NNF_STR(HALS_LATE_ISSUE) " HALS_MID_AT(R)=" NNF_STR(HALS_MID_AT(R)) " HALS_DBG=" NNF_STR(HALS_DBG))

// Scalar (SMEM) loads issued by hand.  SMEM returns out of order, so the only usable wait is lgkmcnt(0) and hipcc cannot
// software-pipeline such loads itself (it sinks every load to its use: one exposed scalar-cache round trip per 16 values).
// Here a 32-float block of the Gram row is fetched while the previous block is being consumed: wait(current) ->
// issue(next) -> 16 x v_pk_fma_f32 with SGPR-pair operands.  The loads are invisible to hipcc's counters (so it adds no
// waits of its own); the "+s" wait statements carry the data dependence (cdna_hip_programming.md s.5.7 form (ii)).
#define NNF_SLOAD2(d0, d1, base, off) \
    asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dwordx16 %1, %2, %4" : "=&s"(d0), "=&s"(d1) : "s"(base), "i"((off) * 4), "i"((off) * 4 + 64))
#define NNF_SLOAD2D(d0, d1, dd, base, off, doff) \
    asm volatile("s_load_dwordx16 %0, %3, %4\n\ts_load_dwordx16 %1, %3, %5\n\ts_load_dword %2, %3, %6" \
                 : "=&s"(d0), "=&s"(d1), "=&s"(dd) : "s"(base), "i"((off) * 4), "i"((off) * 4 + 64), "i"((doff) * 4))
#define NNF_SWAIT2(d0, d1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(d0), "+s"(d1))
#define NNF_SWAIT3(d0, d1, dd) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(d0), "+s"(d1), "+s"(dd))

// One Gauss-Seidel sweep (nnls.py:158-170) over the column held in v2 = {(v[0],v[1]), (v[2],v[3]), ...}.
//   x     = (UtM[k] - UtU[k,:].v - sp) / UtU[k,k]
//   v[k] <- max(v[k] + x, 0)            (== v[k] + max(x, -v[k]) of the reference, same rounding)
//   step  = x if not clipped else -v[k]
// Gp: padded Gram, row stride RS = 32*ceil(R/32) floats (zeros past r), followed by R pairs (1/diag, nz): (0, 0) = skip row.
template <int R, bool KEEPB, class MID>
__device__ __forceinline__ float hals_sweep_column(f32x2 (&v2)[R / 2], const float (&b)[KEEPB ? R : 1], rsrc_t rb, int voff,
                                                   int ldm4, const float* __restrict__ Gp, float sp, const MID& mid) {
    constexpr int NBLK = (R + 31) / 32, RS = 32 * NBLK, P = R / 2, DOFF = R * RS;
    const uint64_t base = (uint64_t)Gp;
    f32x16 buf[2][2];
    float dv[2];
    float nd = 0.f;
    // UtM column not resident (R > 104): fetch it BPF rows ahead of its use (rows >= r: outside the descriptor -> 0)
    constexpr int BPF = 8;
    float bring[KEEPB ? 1 : BPF];
    if constexpr (!KEEPB) {
#pragma unroll
        for (int i = 0; i < BPF; ++i)
            bring[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, voff, i * ldm4, 0));
    }
    NNF_SLOAD2D(buf[0][0], buf[0][1], dv[0], base, 0, DOFF);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        if (k == HALS_MID_AT(R)) mid();
        f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f}, a2 = {0.f, 0.f}, a3 = {0.f, 0.f};   // four chains: FMA latency > 2 issues
        float di = 0.f;
#pragma unroll
        for (int blk = 0; blk < NBLK; ++blk) {
            const int jb = k * NBLK + blk, cur = jb & 1, nxt = cur ^ 1;
            if (blk == 0) {
                NNF_SWAIT3(buf[cur][0], buf[cur][1], dv[k & 1]);
                di = dv[k & 1];
            } else {
                NNF_SWAIT2(buf[cur][0], buf[cur][1]);
            }
            // next block of the stream (next row's first block also brings that row's 1/diag)
            if (blk + 1 < NBLK) {
                NNF_SLOAD2(buf[nxt][0], buf[nxt][1], base, k * RS + 32 * (blk + 1));
            } else if (k + 1 < R) {
                NNF_SLOAD2D(buf[nxt][0], buf[nxt][1], dv[(k + 1) & 1], base, (k + 1) * RS, DOFF + 2 * (k + 1));
            }
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                if (16 * blk + j < P)
                    a0 = __builtin_elementwise_fma(f32x2{buf[cur][0][2 * j], buf[cur][0][2 * j + 1]}, v2[16 * blk + j], a0);
                if (16 * blk + 8 + j < P)
                    a1 = __builtin_elementwise_fma(f32x2{buf[cur][1][2 * j], buf[cur][1][2 * j + 1]}, v2[16 * blk + 8 + j], a1);
                if (16 * blk + j + 1 < P)
                    a2 = __builtin_elementwise_fma(f32x2{buf[cur][0][2 * j + 2], buf[cur][0][2 * j + 3]}, v2[16 * blk + j + 1], a2);
                if (16 * blk + 8 + j + 1 < P)
                    a3 = __builtin_elementwise_fma(f32x2{buf[cur][1][2 * j + 2], buf[cur][1][2 * j + 3]}, v2[16 * blk + 8 + j + 1], a3);
            }
        }
        const f32x2 a = (a0 + a1) + (a2 + a3);
        const float dot = a[0] + a[1];
        float bk;
        if constexpr (KEEPB) {
            bk = b[k];
        } else {
            bk = bring[k % BPF];
            if (k + BPF < R)
                bring[k % BPF] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, voff, (k + BPF) * ldm4, 0));
        }
        const float vk = v2[k / 2][k & 1];
        // KEEPB: the resident column already holds UtM - sp.  A zero Gram diagonal (or a padded row) has di = 0: then
        // x = 0 and the row must stay untouched whatever its sign (nnls.py:160) -> force "keep" with a scalar-side test.
        // Non-finite values go the way np.maximum sends them (nnfac_hip.h "Non-finite operands"): a NaN t is kept (`t > 0` would
        // clip it to a clean 0), and a row with di = 0 sees a residual of 0 whatever its all-zero Gram row made of an Inf
        // elsewhere in the column (0 * Inf is NaN) -- one select on the scalar-side test; the arithmetic of a live row is untouched.
        const bool skip = __builtin_bit_cast(unsigned, di) == 0u;
        const float res = KEEPB ? (bk - dot) : (bk - dot - sp);
        const float x = (skip ? 0.f : res) * di;
        const float t = vk + x;
        const bool keep = !(t <= 0.f) | skip;
        const float vn = keep ? t : 0.f;
        const float step = keep ? x : -vk;
        v2[k / 2][k & 1] = vn;
        nd = fmaf(step, step, nd);
        asm volatile("" : "+v"(nd));  // finish this row's bookkeeping here (otherwise it is sunk to the end of the sweep)
    }
    return nd;
}

template <int RP, bool RES>
__global__ __launch_bounds__(256, (RP > 104 ? 1 : 2)) void nnf_hals_kernel(hals_args a) {
    constexpr bool KEEPB = (RP <= 104);   // UtM column resident in VGPRs next to the V column (fits 256 registers)
    constexpr bool XY = (RP > 32 && RP <= 52);   // row-split sweep on operands pre-scaled by 1/diag (its 3 buffers need RP+24 SGPRs: beyond 52 the allocator starts spilling in-flight buffers)
    const bool all_live = XY && (a.dinv[2 * RP] != 0.f);   // wave-uniform: no zero on the Gram diagonal (prep kernel)
    __shared__ double red[4 * 3];
    __shared__ double red2[2][2][4];   // [sweep parity][block sum | collect][wave]: see hals_block_sum1
    __shared__ unsigned lds_flag;
    if (threadIdx.x == 0) lds_flag = 1u;   // time-out flag of the collects, armed once (read after a barrier)
    const int nblocks = gridDim.x;
    const int64_t gthreads = (int64_t)nblocks * 256;
    const int64_t gtid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // descriptors over the whole matrices: rows >= r / columns of idle lanes fall outside num_records
    // (loads return 0, stores are dropped by the hardware range check)
    const rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(a.V, 0, (int)(((int64_t)(a.r - 1) * a.ldv + a.ncols) * 4), 0x00020000);
    const rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.UtM), 0,
                                                        (int)(((int64_t)(a.r - 1) * a.ldm + a.ncols) * 4), 0x00020000);
    const int ldv4 = (int)(a.ldv * 4), ldm4 = (int)(a.ldm * 4);
    // start values: a.Vsrc (resident kernel only: the column is read ONCE, before the first sweep, and V is written once, at
    // the end -- so a solve that starts from another matrix, nmf.py:415 `hals_nnls_acc(..., U_in^T)`, needs no copy of it first;
    // the streaming kernel re-reads V every sweep and gets Vsrc == V from the entry point)
    const rsrc_t rvs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.Vsrc), 0,
                                                         (int)(((int64_t)(a.r - 1) * a.ldvs + a.ncols) * 4), 0x00020000);
    const int ldvs4 = (int)(a.ldvs * 4);
    f32x2 v2[RP / 2];
    float b[KEEPB ? RP : 1];
    // XY: the one-instruction row update (no GUARD) drops a NaN, so it runs on finite data only.  The streaming form always
    // runs with GUARD, which keeps NaN and Inf.  The resident form -- config B's U-side solve -- decides once per launch, right
    // after its column is loaded: 0 * x summed over the scaled right-hand side and the start values is 0 unless one of them is
    // Inf or NaN (2 RP FMAs); the prep kernel leaves "this Gram row is finite" in the last float of every row of the scaled
    // Gram (0, or NaN), which rides in the same sum -- one load per lane, in flight with the column's.
    // Finite operands stay finite (fp32 overflow aside), so a wave that finds all of it finite keeps the one-instruction form.
    bool plain = false;   // wave-uniform
    auto sweep = [&](int voff, const auto& mid) -> float {
        if constexpr (XY) {
            return plain ? hals_sweep_column_xy<RP, false>(v2, hals_b_regs<RP>{b}, a.Gs, a.dinv, mid)
                         : hals_sweep_column_xy<RP, true>(v2, hals_b_regs<RP>{b}, a.Gs, a.dinv, mid);
        } else {
            return hals_sweep_column<RP, KEEPB>(v2, b, rb, voff, ldm4, a.Gp, a.sp, mid);
        }
    };
    auto load_col = [&](int voff) {
#pragma unroll
        for (int k = 0; k < RP; ++k) {
            v2[k / 2][k & 1] = RES ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rvs, voff, k * ldvs4, 0))
                                   : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rv, voff, k * ldv4, 0));
            if constexpr (KEEPB) {   // the sparsity constant is folded in once (rows >= r: di = 0, value irrelevant)
                b[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, voff, k * ldm4, 0)) - a.sp;
                if constexpr (XY) b[k] *= a.dinv[2 * k];   // scaled operands (hals_sweep_column_xy)
            }
        }
    };
    auto store_col = [&](int voff) {
#pragma unroll
        for (int k = 0; k < RP; ++k) {
            // NB: __builtin_bit_cast straight from an ext-vector element reads element 0 (hipcc 7.2): go through a scalar
            const float val = v2[k / 2][k & 1];
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), rv, voff, k * ldv4, 0);
        }
    };
    const int voff0 = gtid < a.ncols ? (int)(gtid * 4) : (int)0x7ffffff0;
    if constexpr (RES) load_col(voff0);
    if constexpr (RES && XY) {
        static_assert(!XY || RP < 64, "the scaled Gram's rows have a spare last float");
        float c = a.Gs[(threadIdx.x & 63) < RP ? (threadIdx.x & 63) * 64 + 63 : 63];   // one register, taken in the order of the loads
#pragma unroll
        for (int k = 0; k < RP; ++k) {
            c = fmaf(v2[k / 2][k & 1], 0.f, c);
            c = fmaf(b[k], 0.f, c);
            asm volatile("" : "+v"(c));
        }
        plain = all_live && __ballot(!(c == 0.f)) == 0ull;
    }
    // Sweep loop.  mode 1: fixed count, per-sweep local partials, nothing to decide.
    // mode 0, resident columns, RP <= 64 (240 VGPRs at RP = 64, no spills): lag-one speculation.  After sweep s the workgroup publishes its partial and goes
    // straight on to sweep s+1 in registers; only then does it collect the global sum of sweep s (published by every
    // workgroup a whole sweep ago, its granule loads issued a sweep ago: the wait is normally free).  If that sum says
    // "stop" (nnls.py:156) the registers hold one sweep too many and V is taken from a register copy made before the
    // sweep; V is written to memory once, at the end.  Cost: one wasted sweep at the end instead of a stall per sweep.
    // Larger ranks have no registers for the copy; storing V after every confirmed sweep instead costs more than it saves
    // (125000 x 100: 100 vs 45 us per sweep), so they -- and the strided mode -- wait for the sum of the sweep just done.
    constexpr bool BACKUP = RES && RP <= 64;
    constexpr bool SPEC = BACKUP;
    f32x2 vb[BACKUP ? RP / 2 : 1];

    double eps0 = 0.0, eps = 1.0;
    int done = 0;
    bool ok = true, stopped = false;
    if (a.mode == 0 && a.sweep0 > 0 && !hals_take_over(a.status, a.sweep0, a.delta, eps0, eps)) return;
    hals_prefetch pf;
    pf.s = 0;
    for (int s = 1; s <= a.max_sweeps; ++s) {
        double nd = 0.0;
        if constexpr (BACKUP) {
            if (a.mode == 0) {
#pragma unroll
                for (int k = 0; k < RP / 2; ++k) vb[k] = v2[k];   // V after sweep s-1
            }
        }
        if constexpr (RES) {
            float f;
            if constexpr (SPEC && (RP > 52 || !HALS_LATE_ISSUE)) {   // (RP > 52: 240+ VGPRs already, no room for the four address registers)
                if (a.mode == 0 && s >= 2) hals_collect_issue(a.sy, s - 1, nblocks, pf);   // consumed after this sweep
                f = sweep(voff0, hals_mid_none{});
            } else if constexpr (SPEC) {
                // granules of sweep s-1, consumed after this sweep: their loads go out in the middle of it (hals_mid_issue);
                // nothing to collect (fixed-count mode, first sweep): row 0 of the region is read and ignored (pf.s = 0)
                const bool want = a.mode == 0 && s >= 2;   // (set up here and in k_hals_quad.hip, not by a shared builder: it moved the quad kernel's instruction count)
                const hals_word* row = hals_row(a.sy, want ? s - 1 : 0, nblocks);
                const int b0 = (int)threadIdx.x < nblocks ? (int)threadIdx.x : 0;
                const int b1 = (int)threadIdx.x + 256 < nblocks ? (int)threadIdx.x + 256 : 0;
                pf.s = want ? s - 1 : 0;
                f = sweep(voff0, hals_mid_issue{(unsigned long long)(row + 2 * (size_t)b0), (unsigned long long)(row + 2 * (size_t)b1), pf});
                hals_mid_wait(pf);
            } else {
                f = sweep(voff0, hals_mid_none{});
            }
            nd = gtid < a.ncols ? (double)f : 0.0;
        } else {
            for (int64_t col = gtid; col < a.ncols; col += gthreads) {
                const int voff = (int)(col * 4);
                load_col(voff);
                nd += (double)sweep(voff, hals_mid_none{});
                store_col(voff);
            }
        }
        double bs;
        bool merged = false;    // SPEC: this sweep's block sum and the collect of sweep s-1 share one barrier
        double tot_m = 0.0;
        if constexpr (RES && SPEC) {
            if (a.mode == 0 && s >= 2 && !(HALS_DBG & 14)) {
                ok = hals_sum_collect1<256>(a.sy, nd, bs, s - 1, nblocks, tot_m, red2[s & 1][0], red2[s & 1][1], &lds_flag, pf);
                merged = true;
            }
        }
        if (!merged) {
            if constexpr (RES && (HALS_DBG & 8) != 0) bs = nd;   // timing only: no wave sum, no barrier
            else if constexpr (RES) bs = hals_block_sum1<256>(nd, red2[s & 1][0]);   // valid in every thread; one barrier
            else bs = nnf_block_sum_f64(nd, red);
        }
        if (a.mode == 1) {
            if (threadIdx.x == 0) a.sweep_partials[(size_t)(s - 1) * nblocks + blockIdx.x] = bs;
            if constexpr (RES) {
                if (a.snapshots != nullptr && gtid < a.ncols && s > a.snap_first) {   // V after sweep s (fire-and-forget stores)
                    float* sp_ = a.snapshots + (size_t)(s - 1 - a.snap_first) * a.snap_stride + gtid;
#pragma unroll
                    for (int k = 0; k < RP; ++k)
                        if (k < a.r) sp_[(int64_t)k * a.ncols] = v2[k / 2][k & 1];
                }
            }
            done = s;
            continue;
        }
        if (!(HALS_DBG & 12)) hals_publish(a.sy, s, nblocks, bs);
        const int c = SPEC ? s - 1 : s;         // sweep whose global sum is examined now
        if (c >= 1 && !(HALS_DBG & 14)) {
            double tot;
            if (merged) tot = tot_m;
            else if constexpr (RES) ok = hals_collect1(a.sy, c, nblocks, tot, red2[s & 1][1], &lds_flag, pf);
            else ok = hals_collect(a.sy, c, nblocks, tot, red, &lds_flag, &pf);
            if (!ok) break;
            if (c == 1 && a.sweep0 == 0) eps0 = tot;   // (hals_note_sum written out: through it hipcc allocates the sweep's registers differently)
            eps = tot;
            done = c;
            if (!(eps >= a.delta * eps0) && !HALS_DBG) { stopped = true; break; }   // nnls.py:156: sweep c was the last one (the rule written out: see hals_take_over)
        }
    }
    if constexpr (RES) {
        if (a.mode == 0) {
            if constexpr (BACKUP) {
                if (stopped || !ok) {   // the registers hold one sweep too many: fall back to the copy
#pragma unroll
                    for (int k = 0; k < RP / 2; ++k) v2[k] = vb[k];
                }
            }
            if (a.max_sweeps >= 1) store_col(voff0);
        }
    }
    if (a.mode == 1) {
        if constexpr (RES) store_col(voff0);
    } else if (SPEC && ok && !stopped && a.max_sweeps >= 1 && !HALS_DBG) {
        double tot;                             // ran to the sweep budget: the last sweep's sum is still due
        ok = hals_collect(a.sy, a.max_sweeps, nblocks, tot, red, &lds_flag);
        if (ok) {   // (hals_note_sum written out: through it the rank 32 and 64 kernels spill other scalar registers)
            if (a.max_sweeps == 1 && a.sweep0 == 0) eps0 = tot;
            eps = tot;
            done = a.max_sweeps;
        }
    }
    if (a.mode == 0 && blockIdx.x == 0 && threadIdx.x == 0)
        hals_status_finish(a.status, a.max_sweeps >= 1, a.sweep0, done, eps, eps0, !ok);
}

template <int RP>
static int fast_per_cu(bool res) {
    static int cached[2] = {-1, -1};
    int& c = cached[res ? 1 : 0];
    if (c < 0) {
        int nb = 0;
        const hipError_t e = res ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, nnf_hals_kernel<RP, true>, 256, 0)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, nnf_hals_kernel<RP, false>, 256, 0);
        c = hals_per_cu(e, nb, 3);
    }
    return c;
}

template <int RP>
static int fast_launch(bool res, const hals_args& a, int nblocks, hipStream_t st) {
    if (res) hipLaunchKernelGGL((nnf_hals_kernel<RP, true>), dim3(nblocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((nnf_hals_kernel<RP, false>), dim3(nblocks), dim3(256), 0, st, a);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// X(part, padded rank): every instantiation, once (k_parts.h), cut by measured compile time (ranks 100 and 104: 50 CPU-seconds
// each).  Part 0 also holds the dispatchers.  A kernel's code can depend on what else its unit instantiates (ranks 8 .. 64 in ONE
// unit: other register allocation in all ten resident-column kernels): compare the kept ISA kernel by kernel after moving an entry.
#define HALS_TABLE(X)                                                                                            \
    X(0, 8) X(0, 16) X(0, 24) X(0, 32) X(0, 40) X(0, 48)                                                         \
    X(1, 50) X(1, 52) X(1, 56) X(1, 64)                                                                          \
    X(2, 80) X(2, 96)                                                                                            \
    X(3, 100)                                                                                                    \
    X(4, 104)                                                                                                    \
    X(5, 112) X(5, 128)
NNF_PART_DISPATCHER(fast_mine, HALS_TABLE)

int NNF_CAT(nnf_hals_fast_per_cu_part, HALS_PART)(int RP, bool res) {
    return fast_mine(RP, 0, [&](auto rp) { return fast_per_cu<decltype(rp)::value>(res); });
}
int NNF_CAT(nnf_hals_fast_launch_part, HALS_PART)(int RP, bool res, const hals_args& a, int nblocks, hipStream_t st) {
    return fast_mine(RP, NNF_ERR_UNSUPPORTED, [&](auto rp) { return fast_launch<decltype(rp)::value>(res, a, nblocks, st); });
}

#if HALS_PART == 0
#define HALS_DECLARE(p, v)                                      \
    int NNF_PART_FN(nnf_hals_fast_per_cu_part, p)(int, bool);   \
    int NNF_PART_FN(nnf_hals_fast_launch_part, p)(int, bool, const hals_args&, int, hipStream_t);
#define HALS_PER_CU(p, v) case v: return NNF_PART_FN(nnf_hals_fast_per_cu_part, p)(RP, res);
#define HALS_LAUNCH(p, v) case v: return NNF_PART_FN(nnf_hals_fast_launch_part, p)(RP, res, a, nblocks, st);
HALS_TABLE(HALS_DECLARE)
int nnf_hals_fast_per_cu(int RP, bool res) {
    switch (RP) { HALS_TABLE(HALS_PER_CU) default: return 0; }
}
int nnf_hals_fast_launch(int RP, bool res, const hals_args& a, int nblocks, hipStream_t st) {
    switch (RP) { HALS_TABLE(HALS_LAUNCH) default: return NNF_ERR_UNSUPPORTED; }
}
#endif

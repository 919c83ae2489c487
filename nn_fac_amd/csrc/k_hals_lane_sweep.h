// The row-split Gauss-Seidel sweep of the lane kernels, 32 < R <= 64 (k_hals_fast.hip: 256-thread workgroups, the scaled right-hand
// side in registers; k_hals_comm.hip: 8 compute waves + 1 communication wave, the right-hand side in LDS).
#pragma once
#include "k_hals_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

// ---- scalar-cache operand buffers -------------------------------------------------------------------------
// W floats of a Gram row held in SGPRs as 16/8/4-dword pieces (s_load_dwordx16/x8/x4).  Scalar loads return out of
// order, so the only usable wait is lgkmcnt(0): the schedule below is built so that everything outstanding at a wait
// was issued at least ~half a row of FMAs earlier (tools/smem_probe.hip: ~60 ns for two x16 hits, ~105 ns from L2).
template <int W>
struct sgbuf {
    f32x16 a, b;
    f32x8 q;
    f32x4 r;
};
template <int W, bool TIED>
__device__ __forceinline__ void sg_issue(sgbuf<W>& d, uint64_t base, int off) {
    constexpr int N16 = W / 16, N8 = (W % 16) / 8, N4 = (W % 8) / 4;
    static_assert(W % 4 == 0 && N16 <= 2, "piece decomposition");
    // TIED: the destination registers are the ones that held the previous row's piece (consumed just above)
    if constexpr (TIED) {
        if constexpr (N16 >= 1) asm volatile("s_load_dwordx16 %0, %1, %2" : "+s"(d.a) : "s"(base), "i"(off * 4));
        if constexpr (N16 >= 2) asm volatile("s_load_dwordx16 %0, %1, %2" : "+s"(d.b) : "s"(base), "i"(off * 4 + 64));
        if constexpr (N8 == 1) asm volatile("s_load_dwordx8 %0, %1, %2" : "+s"(d.q) : "s"(base), "i"(off * 4 + 64 * N16));
        if constexpr (N4 == 1) asm volatile("s_load_dwordx4 %0, %1, %2" : "+s"(d.r) : "s"(base), "i"(off * 4 + 64 * N16 + 32 * N8));
    } else {
        if constexpr (N16 >= 1) asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(d.a) : "s"(base), "i"(off * 4));
        if constexpr (N16 >= 2) asm volatile("s_load_dwordx16 %0, %1, %2" : "=s"(d.b) : "s"(base), "i"(off * 4 + 64));
        if constexpr (N8 == 1) asm volatile("s_load_dwordx8 %0, %1, %2" : "=s"(d.q) : "s"(base), "i"(off * 4 + 64 * N16));
        if constexpr (N4 == 1) asm volatile("s_load_dwordx4 %0, %1, %2" : "=s"(d.r) : "s"(base), "i"(off * 4 + 64 * N16 + 32 * N8));
    }
}
// after s_waitcnt: tell the compiler the pieces now hold their loaded values (nothing may be read above this point)
template <int W>
__device__ __forceinline__ void sg_arrived(sgbuf<W>& d) {
    constexpr int N16 = W / 16, N8 = (W % 16) / 8, N4 = (W % 8) / 4;
    if constexpr (N16 >= 1) asm volatile("" : "+s"(d.a));
    if constexpr (N16 >= 2) asm volatile("" : "+s"(d.b));
    if constexpr (N8 == 1) asm volatile("" : "+s"(d.q));
    if constexpr (N4 == 1) asm volatile("" : "+s"(d.r));
}
template <int W>
__device__ __forceinline__ f32x2 sg_pair(const sgbuf<W>& d, int p) {   // floats 2p, 2p+1 of the buffer
    constexpr int N16 = W / 16, N8 = (W % 16) / 8;
    const int j = 2 * p;
    if (N16 >= 1 && j < 16) return f32x2{d.a[j], d.a[j + 1]};
    if (N16 >= 2 && j < 32) return f32x2{d.b[j - 16], d.b[j - 15]};
    const int j2 = j - 16 * N16;
    if (N8 == 1 && j2 < 8) return f32x2{d.q[j2], d.q[j2 + 1]};
    const int j3 = j2 - 8 * N8;
    return f32x2{d.r[j3], d.r[j3 + 1]};
}

// ---- where row k's scaled right-hand side b[k] comes from -------------------------------------------------
// issue(k): called one row ahead, right behind row k - 1's wait (row 0: in front of the loop); get(k): row k's value, called
// behind row k's s_waitcnt lgkmcnt(0).
// In registers (the 256-thread workgroups): nothing to issue.
template <int R>
struct hals_b_regs {
    const float (&b)[R];
    __device__ __forceinline__ void issue(int) {}
    __device__ __forceinline__ float get(int k) { return b[k]; }
};
// In LDS, b_lds[k][thread] with HALS_B_PITCH floats per row (bank = thread: no conflicts): one hand-issued ds_read_b32 per row,
// two destination registers in turn.  LDS returns a wave's reads in order and shares lgkmcnt with the scalar loads, whose
// out-of-order return already forces every wait of the sweep to be lgkmcnt(0): the row's one wait covers the read.  A lane
// reads only what it wrote itself, and a wave's LDS operations complete in order: no barrier.  The 16-bit offset field of
// the instruction reaches 32 rows, so rows 32 .. R - 1 go through a second address register.
constexpr int HALS_B_PITCH = 512;
struct hals_b_lds {
    unsigned a0, a1;   // LDS byte addresses of this thread's entries of rows 0 and 32
    float v[2];
    __device__ __forceinline__ void issue(int k) {
        if (k < 32) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[k & 1]) : "v"(a0), "i"(k * HALS_B_PITCH * 4));
        else asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v[k & 1]) : "v"(a1), "i"((k - 32) * HALS_B_PITCH * 4));
    }
    __device__ __forceinline__ float get(int k) {
        asm volatile("" : "+v"(v[k & 1]));
        return v[k & 1];
    }
};

// One Gauss-Seidel sweep for 32 < R <= 64 with the UtM column resident.  Operands are pre-scaled by 1/diag:
// Gs = diag(1/diag) UtU (rows with a zero diagonal are all zero) and b = (UtM - sp)/diag, so a row update is
//     x = b[k] - Gs[k,:].v ;  d = max(x, -v[k]) ;  v[k] += d ;  nodelta += d*d          (nnls.py:162-170)
// i.e. 6 vector instructions after the R/2 packed FMAs of the dot product.
// A Gram row is split into X = columns [0, XW) and Y = columns [XW, XW+24).  Y is double-buffered and fetched a whole
// row ahead; X is single-buffered and refilled for the next row as soon as its FMAs have issued, i.e. before the Y
// part and the row bookkeeping -- so the single lgkmcnt(0) per row finds both in (or nearly in) the registers.
// GUARD: some Gram diagonal is zero (rare).  Such a row must be left alone whatever it holds (nnls.py:160): d is
// multiplied by the row's nz flag (0/1) fetched with the Y part.  Without GUARD there is no per-row flag at all.
// GUARD is also the variant that keeps non-finite values as np.maximum does (nnfac_hip.h "Non-finite operands"): v_max_f32
// returns the operand that is not NaN, so without GUARD a NaN x writes a clean v[k] = 0; with it d is a compare-and-select
// (two instructions, NaN kept) and the nz flag is applied with v_mul_legacy_f32 (0 * anything = 0: a skipped row stays put next
// to an Inf or NaN elsewhere in the column).  The streaming kernel always runs with GUARD; the resident one where a Gram
// diagonal is zero or an operand is not finite (see nnf_hals_kernel).
template <int R, bool GUARD, class MID, class BSRC>
__device__ __forceinline__ float hals_sweep_column_xy(f32x2 (&v2)[R / 2], BSRC b, const float* __restrict__ Gs,
                                                      const float* __restrict__ nzp, const MID& mid) {
    constexpr int RS = 64, P = R / 2, YW = 24, XW = (R - YW + 3) & ~3, XP = XW / 2;
    static_assert(YW == 24, "the Y issue statement below is written for x16 + x8");
    static_assert(R > 32 && R <= 64 && R % 2 == 0 && XW + YW <= RS && XW >= 8, "row split");
    const uint64_t base = (uint64_t)Gs, nzb = (uint64_t)nzp;
    sgbuf<XW> X;
    sgbuf<YW> Y[2];
    f32x2 dv[2];   // (1/diag, nz) pair of the row (GUARD only)
    float nd = 0.f;
    sg_issue<XW, false>(X, base, 0);
    sg_issue<YW, false>(Y[0], base, XW);
    if constexpr (GUARD) asm volatile("s_load_dwordx2 %0, %1, %2" : "=s"(dv[0]) : "s"(nzb), "i"(0));
    b.issue(0);
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int cur = k & 1, nxt = cur ^ 1;
        if (k == HALS_MID_AT(R)) mid();
        if constexpr (GUARD) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(dv[cur]));
        else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        sg_arrived<XW>(X);
        sg_arrived<YW>(Y[cur]);
        const float bk = b.get(k);
        if (k + 1 < R) {   // one statement, so that all of it is issued here and not wherever the scheduler sinks it
            if constexpr (GUARD)
                asm volatile("s_load_dwordx16 %0, %3, %4\n\ts_load_dwordx8 %1, %3, %5\n\ts_load_dwordx2 %2, %6, %7"
                             : "=&s"(Y[nxt].a), "=&s"(Y[nxt].q), "=&s"(dv[nxt])
                             : "s"(base), "i"(((k + 1) * RS + XW) * 4), "i"(((k + 1) * RS + XW + 16) * 4), "s"(nzb),
                               "i"(8 * (k + 1)));
            else
                asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dwordx8 %1, %2, %4"
                             : "=&s"(Y[nxt].a), "=&s"(Y[nxt].q)
                             : "s"(base), "i"(((k + 1) * RS + XW) * 4), "i"(((k + 1) * RS + XW + 16) * 4));
            b.issue(k + 1);
        }
        f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};   // two chains are enough: the other wave of the SIMD fills the FMA latency
#pragma unroll
        for (int p = 0; p < XP; ++p) {
            const f32x2 g = sg_pair<XW>(X, p);
            if (p & 1) a1 = __builtin_elementwise_fma(g, v2[p], a1);
            else a0 = __builtin_elementwise_fma(g, v2[p], a0);
        }
        asm volatile("" : "+v"(a0), "+v"(a1));   // X is consumed: its registers may be refilled
        if (k + 1 < R) sg_issue<XW, true>(X, base, (k + 1) * RS);
#pragma unroll
        for (int p = XP; p < P; ++p) {
            const f32x2 g = sg_pair<YW>(Y[cur], p - XP);
            if (p & 1) a1 = __builtin_elementwise_fma(g, v2[p], a1);
            else a0 = __builtin_elementwise_fma(g, v2[p], a0);
        }
        const f32x2 a = a0 + a1;
        const float vk = v2[k / 2][k & 1];
        const float x = bk - (a[0] + a[1]);
        float dl;
        if constexpr (GUARD) {
            const float sel = !(x < -vk) ? x : -vk;   // np.maximum(x, -v[k]), NaN included
            asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(dl) : "s"(dv[cur][1]), "v"(sel));
        } else {   // max(x, -v[k]) in one instruction (fmaxf adds a canonicalising max for the negated operand); finite operands only
            asm("v_max_f32 %0, %1, -%2" : "=v"(dl) : "v"(x), "v"(vk));
        }
        v2[k / 2][k & 1] = vk + dl;
        nd = fmaf(dl, dl, nd);
        asm volatile("" : "+v"(nd));  // finish this row's bookkeeping here (otherwise it is sunk to the end of the sweep)
    }
    return nd;
}

// HALS-NNLS solves with FEW columns (the r x n "V side" of NMF at n = 2000, the 500 x R factors of NTF, the replicated
// 100 x 4000 solve of the row-sharded 1e6 x 4000 problem): ONE WAVE PER COLUMN, lane i <-> row i, "push" form of the sweep.
//
// The sweep of nnls.py:158-170 is r SEQUENTIAL row updates; each of the other layouts (k_hals_fast.hip: a lane per column,
// k_hals_quad.hip: four lanes per column) spends a whole dot product G[k,:].v -- r/2 or r/8 packed FMAs plus a cross-lane
// reduction -- on the critical path of every row, so a solve with few columns is a handful of lone waves crawling through
// ~r * 17 dependent instructions per sweep (3.5 us per sweep at 50 x 2000, 125 waves, 95 % of the chip idle).  Here the
// residual of EVERY row is kept up to date instead (one VGPR: lane i holds the scaled residual of row i)
//
//        acc[i] = ( UtM[i] - sp - sum_j UtU[i][j] v[j] ) / UtU[i][i]                      (all v[j] current)
//
// and a row update is      d = max(acc[k], -v[k]) ;  v[k] += d ;  acc[i] -= G'[i][k] * d  for all i      (G' = D^-1 UtU)
// -- the reference's statement with the dot product read off the residual: v_max (all lanes, lane k's value is the step),
// v_readlane (the step to an SGPR), v_fma (every lane pushes the step into its own residual), v_writelane (lane k keeps
// its step): FOUR vector instructions per row, three of them dependent, whatever the rank, and no scalar instruction at all
// (the sweep is unrolled: the lane numbers are immediates).  Column k of G' comes from an LDS image shared by the
// workgroup's waves.  There are n waves instead of n/16: 2000 columns = two waves on every SIMD of 250 CUs.
//
// Rounding: the residual is formed from scratch (b' - G'v, summed in row order like the reference's dot product) when the
// kernel starts and every 8 sweeps, and pushed forward in between; each push rounds once relative to the residual itself
// (which shrinks as the solve converges), not to the dot product, so the carried residual is as accurate as a freshly
// evaluated fp32 one.  Results differ from the other layouts in the last bits, like those differ from
// each other.
//
// Stopping rule (nnls.py:156) on the device.  A sweep takes ~0.5 us here -- a third of the round trip through the memory
// side of the chip that a grid-wide exchange costs (the granules cross XCDs: ~1.6 us measured) -- so the compute waves never
// wait for it:
//   * a compute wave ends a sweep with its fp32 sum of squared steps (DPP) as a tagged fp64 in an LDS slot and a snapshot of
//     its column in a global scratch ring (256 coalesced bytes; 16 sweeps deep), then goes on to the next sweep;
//   * FOUR more waves per workgroup, the COMMUNICATION waves, do the exchange; wave u serves the sweeps c = u + 1 (mod 4):
//     it adds the slots of sweep c in wave order once they are all there, publishes the block sum as two tagged granules
//     (k_hals_common.h), then reads the granules of ALL blocks for sweep c - 4 (published a few sweeps ago: normally one
//     round trip), adds them in block order -- the same double in every workgroup -- and leaves the total and the verdict
//     `total >= delta * eps0` in an LDS ring.  Each of the four takes a round trip per sweep it serves; together they keep up
//     with the sweeps.  (One wave with four requests in flight would do as well -- but in-flight registers across a loop
//     with re-read branches are exactly what hipcc's wait-count insertion turns into "wait for everything".)
//   * a compute wave reads the verdicts IN SWEEP ORDER, one LDS word per sweep, before it starts a sweep: it may run ahead of
//     them by at most the depth of its snapshot ring, and at the first "stop" verdict -- sweep c -- it reloads the snapshot of
//     sweep c and leaves.  Sweeps run ahead of a stop are discarded.
// Nothing in a sweep depends on the exchange; every spin is bounded.  Control words travel through LDS as relaxed
// workgroup-scope atomics (`volatile` makes hipcc drain every outstanding memory operation in front of each access).
// Rows with a zero Gram diagonal (nnls.py:160) and the padding rows hold residual 0 and "-v" = -inf: their step is 0.
#include "k_hals_common.h"

// (WAVE_COMM, WAVE_MAX_NW, WAVE_SNAP, WAVE_NP and the sizes the plan counts with them: k_hals_plan.h)
#ifndef WAVE_REFRESH_V
#define WAVE_REFRESH_V 8             // (A/B builds: 4, 2 -- tools/probes/wave_refresh_probe.sh; accuracy / time table in DESIGN.md section 4)
#endif
constexpr int WAVE_REFRESH = WAVE_REFRESH_V;   // the residual is re-formed from scratch (b' - G'v) every so many sweeps (a power of two)
constexpr unsigned WAVE_ERR = 0xffffffffu;

#ifndef WAVE_DBG
#define WAVE_DBG 0      // timing-only ablations (tools/probes/vside_probe.py): 1 = verdicts without totals (run to the budget), 4 = no row updates
#endif
NNF_BUILD_FLAGS(k_hals_wave, "WAVE_DBG=" NNF_STR(WAVE_DBG) " WAVE_REFRESH_V=" NNF_STR(WAVE_REFRESH_V))

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float wave_dpp_add_f32(float v) {
    const int m = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false);
    return v + __builtin_bit_cast(float, m);
}
// fixed-order fp32 sum over the 64 lanes (same DPP ladder as nnf_wave_sum_f64), wave-uniform result
__device__ __forceinline__ float wave_sum_f32(float v) {
    v = wave_dpp_add_f32<0xB1, 0xf>(v);
    v = wave_dpp_add_f32<0x4E, 0xf>(v);
    v = wave_dpp_add_f32<0x141, 0xf>(v);
    v = wave_dpp_add_f32<0x140, 0xf>(v);
    v = wave_dpp_add_f32<0x142, 0xa>(v);
    v = wave_dpp_add_f32<0x143, 0xc>(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// prep: image of G' by COLUMNS.  img[k][lane] (RL = 1) or img[k][lane] = {row lane, row lane + 64} (RL = 2):
//   G'[i][k] = UtU[i][k] / UtU[i][i]   (0 where the diagonal is 0, outside r x r, in the padding rows k >= r)
// UtU[i][k] as stored -- NOT UtU[k][i]: the reference reads rows of whatever it is handed (nnls.py:167) and its own tests pass
// a random, non-symmetric "Gram" (tests/nnls_tests.py:44-45).  Then 1/diag per row, counter, status.
__global__ void nnf_hals_prep_wave_kernel(const float* __restrict__ UtU, const float* __restrict__ UtU2, int64_t ldg, int r, int RL,
                                          float* __restrict__ img, float* __restrict__ dinv, unsigned* counter, double* status) {
    const int k = blockIdx.x;                   // image row = Gram column
    const int W = 64 * RL;
    auto gram = [&](int a, int b) -> float {
        const float g = UtU[(int64_t)a * ldg + b];
        return UtU2 ? g * UtU2[(int64_t)a * ldg + b] : g;
    };
    for (int c = threadIdx.x; c < W; c += blockDim.x) {
        const int i = (RL == 2) ? ((c >> 1) + 64 * (c & 1)) : c;    // RL = 2: float2 {row lane, row lane + 64}
        float val = 0.f;
        if (k < r && i < r) {
            const float d = gram(i, i);
            if (d != 0.f) val = gram(i, k) * (float)(1.0 / (double)d);
        }
        img[(size_t)k * W + c] = val;
    }
    if (k < r && threadIdx.x == 0) {
        const float d = gram(k, k);
        dinv[k] = (d != 0.f) ? (float)(1.0 / (double)d) : 0.f;
    }
    if (blockIdx.x == 0) {
        for (int i = r + threadIdx.x; i < 128; i += blockDim.x) dinv[i] = 0.f;
        if (threadIdx.x == 0) {
            *counter = 0u;
            if (status) hals_status_defaults(status);
        }
    }
}

// LDS control block behind the image.  Every word that crosses waves carries the sweep number it belongs to.
struct wave_ctl {
    unsigned long long slot[WAVE_SNAP][WAVE_MAX_NW][2];   // tagged halves {sweep, lo32} {sweep, hi32} of a compute wave's fp64 sum
    unsigned long long tot[WAVE_SNAP][2];                 // the same for the global sum of a sweep
    unsigned long long ver[WAVE_SNAP];                    // verdict {sweep : 32 | 1 = stop, 2 = time-out : 32}, written after tot
    unsigned long long eps0[2];                           // tagged halves (tag 1) of the global sum of sweep 1
    unsigned long long fin;                               // {1 : 32 | stopping sweep : 32} once a compute wave has found it
};

// Words of the control block are exchanged between waves of the workgroup with RELAXED workgroup-scope atomics: plain LDS
// reads / writes that the compiler neither caches in registers nor hoists out of a polling loop.  (`volatile` accesses made
// hipcc drain EVERY outstanding memory operation first -- s_waitcnt vmcnt(0) in front of each poll, i.e. the round trip of the
// snapshot store of the sweep before, 0.65 us per sweep.)
__device__ __forceinline__ unsigned long long wave_ld(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void wave_st(unsigned long long* p, unsigned long long x) {
    __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void wave_st_tagged(unsigned long long* p2, unsigned tagv, double x) {
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, x), tag = (unsigned long long)tagv << 32;
    wave_st(p2, tag | (bits & 0xffffffffull));
    wave_st(p2 + 1, tag | (bits >> 32));
}
// false while either half does not carry `tagv` yet
__device__ __forceinline__ bool wave_ld_tagged(const unsigned long long* p2, unsigned tagv, double& x) {
    const unsigned long long h0 = wave_ld(p2), h1 = wave_ld(p2 + 1);
    x = __builtin_bit_cast(double, (h1 << 32) | (h0 & 0xffffffffull));
    return (unsigned)(h0 >> 32) == tagv && (unsigned)(h1 >> 32) == tagv;
}

// row update K (compile-time: every operand position is an immediate) of the CPW columns a wave holds -- the columns'
// chains are independent, so a wave with two columns fills the latency of one chain with the other.
// EXACT: the form for a wave that holds a non-finite value (nnfac_hip.h "Non-finite operands").  v_max_f32 returns the operand
// that is not NaN: a NaN residual would give the step -v[k], a clean v[k] = 0 and a finite sum.  With EXACT the step is a
// compare-and-select that keeps the NaN, as np.maximum does (one more instruction on the chain of every row), and the step of
// a row that is skipped (zero diagonal, padding: dead) is 0 whatever its residual holds -- 0 * Inf pushed into it by
// another row's step is a NaN there, not in the reference.
template <int RL, int CPW, int K, bool EXACT>
__device__ __forceinline__ void wave_row(const float* img, float (&acc)[CPW][RL], const float (&nvd)[CPW][RL], float (&dk)[CPW][RL],
                                         const bool (&dead)[CPW][RL]) {
    constexpr int H = K >> 6, KL = K & 63, W = 64 * RL;
    float g[RL];
#pragma unroll
    for (int h = 0; h < RL; ++h) g[h] = img[K * W + h];
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
        float d;   // lane KL's value is the step of row K
        if constexpr (EXACT) d = dead[c][H] ? 0.f : (!(acc[c][H] < nvd[c][H]) ? acc[c][H] : nvd[c][H]);
        else asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(acc[c][H]), "v"(nvd[c][H]));   // max(acc, -v) in one instruction (fmaxf adds a canonicalising max)
        const float sd = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d), KL));
#pragma unroll
        for (int h = 0; h < RL; ++h) acc[c][h] = fmaf(g[h], -sd, acc[c][h]);
        // lane KL keeps its step (v_writelane: SGPR data, immediate lane select; this clang has no builtin for it)
        asm("v_writelane_b32 %0, %1, %2" : "+v"(dk[c][H]) : "s"(sd), "n"(KL));
    }
}
template <int RL, int CPW, int K, int RU, bool EXACT>
struct wave_rows {
    static __device__ __forceinline__ void run(const float* img, float (&acc)[CPW][RL], const float (&nvd)[CPW][RL], float (&dk)[CPW][RL],
                                               const bool (&dead)[CPW][RL]) {
        wave_row<RL, CPW, K, EXACT>(img, acc, nvd, dk, dead);
        if constexpr (K + 1 < RU) wave_rows<RL, CPW, K + 1, RU, EXACT>::run(img, acc, nvd, dk, dead);
    }
};

// fixed-order fp64 sum of lanes 0 .. 15 of `v` (other lanes must hold 0), wave-uniform
__device__ __forceinline__ double wave_sum16_f64(double v) {
    v = nnf_dpp_add_f64<0xB1, 0xf>(v);
    v = nnf_dpp_add_f64<0x4E, 0xf>(v);
    v = nnf_dpp_add_f64<0x141, 0xf>(v);
    v = nnf_dpp_add_f64<0x140, 0xf>(v);
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, 0);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 0);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | (unsigned long long)lo);
}

// global sum of sweep s: the granules of all blocks, strided over the lanes (late ones are re-read, bounded), added in block
// order per lane, DPP wave sum -- the same double in every workgroup.  false = time-out or `fin` set (wave-uniform).
__device__ __forceinline__ bool wave_total(const hals_sync& sy, const wave_ctl* ctl, int s, int nblocks, int lane, double& total) {
    const unsigned tag = hals_tag(sy, s);
    const hals_word* base = hals_row(sy, s, nblocks);
    unsigned long long g0[WAVE_NP], g1[WAVE_NP];
    // every request of the wave goes out before the first answer is looked at: no load under a branch (lanes past the last
    // block re-read block 0 and ignore it) -- one round trip for the lot, not one per pair
#pragma unroll
    for (int i = 0; i < WAVE_NP; ++i) {
        const int b = lane + 64 * i < nblocks ? lane + 64 * i : 0;
        g0[i] = __hip_atomic_load(base + 2 * (size_t)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        g1[i] = __hip_atomic_load(base + 2 * (size_t)b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    bool fresh = true;
#pragma unroll
    for (int i = 0; i < WAVE_NP; ++i) fresh = fresh && (unsigned)(g0[i] >> 32) == tag && (unsigned)(g1[i] >> 32) == tag;
    bool late = false;
    if (__ballot(!fresh) != 0ull) {                       // somebody's granule is not there yet: re-read (rare, bounded)
#pragma unroll 1
        for (int i = 0; i < WAVE_NP; ++i) {
            const int b = lane + 64 * i < nblocks ? lane + 64 * i : 0;
            unsigned long long a0 = g0[0], a1 = g1[0];
#pragma unroll
            for (int u = 0; u < WAVE_NP; ++u)
                if (u == i) { a0 = g0[u]; a1 = g1[u]; }
            unsigned spins = 0;   // (not hals_granule_wait: this loop sleeps before its first re-read too and looks at `fin`; and through the helper every instantiation spills other scalar registers)
            while (!((unsigned)(a0 >> 32) == tag && (unsigned)(a1 >> 32) == tag)) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > HALS_SPIN_LIMIT || ((spins & 63u) == 0u && wave_ld(&ctl->fin) != 0ull)) { late = true; break; }
                a0 = __hip_atomic_load(base + 2 * (size_t)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a1 = __hip_atomic_load(base + 2 * (size_t)b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int u = 0; u < WAVE_NP; ++u)
                if (u == i) { g0[u] = a0; g1[u] = a1; }
        }
    }
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < WAVE_NP; ++i)
        v += (lane + 64 * i < nblocks) ? hals_granule_value(g0[i], g1[i]) : 0.0;
    total = nnf_wave_sum_f64(v);
    return __ballot(late) == 0ull;
}

// ---- a communication wave: serves the sweeps c = u + 1, u + 1 + WAVE_COMM, ... ---------------------------------------------
// block sum of sweep c: waits (bounded) until every compute wave has left its tagged sum; false: time-out or the solve is over
__device__ __forceinline__ bool wave_block_sum(wave_ctl* ctl, int c, int NW, int lane, double& bs) {
    const int sl = c & (WAVE_SNAP - 1);
    unsigned spins = 0;
    double v = 0.0;
    for (;;) {
        double x = 0.0;
        const bool have = lane >= NW || wave_ld_tagged(&ctl->slot[sl][lane < NW ? lane : 0][0], (unsigned)c, x);
        if (__ballot(!have) == 0ull) {
            v = lane < NW ? x : 0.0;
            break;
        }
        if (wave_ld(&ctl->fin) != 0ull) return false;     // the compute waves have left: the slots of this sweep will never come
        __builtin_amdgcn_s_sleep(2);
        if (++spins > HALS_SPIN_LIMIT) return false;
    }
    bs = wave_sum16_f64(v);
    return true;
}
// total + verdict of sweep cd into the rings (nnls.py:156: the loop goes on while eps >= delta * eps0).  false: give up.
__device__ __forceinline__ bool wave_judge(const hals_args& a, wave_ctl* ctl, int cd, int nblocks, int lane) {
    double tot = 0.0;
    unsigned flag = 0u;
    if (!(WAVE_DBG & 1)) {
        if (!wave_total(a.sy, ctl, cd, nblocks, lane, tot)) {
            if (wave_ld(&ctl->fin) != 0ull) return false;
            flag = 2u;                                    // time-out
        } else {
            double e0 = tot;
            if (cd == 1) {
                if (lane == 0) wave_st_tagged(&ctl->eps0[0], 1u, tot);
            } else {                                      // eps0 comes from the wave that serves sweep 1 (bounded wait)
                unsigned spins = 0;
                while (!wave_ld_tagged(&ctl->eps0[0], 1u, e0)) {
                    __builtin_amdgcn_s_sleep(2);
                    if (++spins > HALS_SPIN_LIMIT || wave_ld(&ctl->fin) != 0ull) return false;
                }
            }
            flag = hals_goes_on(tot, a.delta, e0) ? 0u : 1u;
        }
    }
    if (lane == 0) {
        const int sl = cd & (WAVE_SNAP - 1);
        wave_st_tagged(&ctl->tot[sl][0], (unsigned)cd, tot);
        wave_st(&ctl->ver[sl], ((unsigned long long)(unsigned)cd << 32) | (unsigned long long)flag);   // after tot: LDS keeps a wave's order
    }
    return flag == 0u;
}
__device__ __forceinline__ void wave_comm_loop(const hals_args& a, wave_ctl* ctl, int NW, int u, int lane, int nblocks) {
    const int S = a.max_sweeps;
    int c = u + 1;
    for (; c <= S; c += WAVE_COMM) {
        double bs;
        if (!wave_block_sum(ctl, c, NW, lane, bs)) return;
        hals_publish(a.sy, c, nblocks, bs, lane == 0);
        const int cd = c - WAVE_COMM;                     // published by everybody a few sweeps ago
        if (cd >= 1 && !wave_judge(a, ctl, cd, nblocks, lane)) return;
    }
    // the last sweep this wave served has not been judged yet
    const int cd = c - WAVE_COMM;
    if (cd >= 1 && cd <= S) (void)wave_judge(a, ctl, cd, nblocks, lane);
}

// ---- the kernel ---------------------------------------------------------------------------------------------------------
// a.Gp = UtU (r x r, row stride ldg), a.Gs = the second Gram of a Hadamard pair or NULL: every workgroup builds its own LDS
// image of G' by columns from them (a few Gram entries per thread; a preparation launch of its own was 5-6 us in front of a
// 17 us solve at the NTF shapes).  snap: global scratch [ncols][WAVE_SNAP][64 RL] floats.
// CPW: columns per compute wave (2 when one column per wave would need more workgroups than the chip holds at once).
template <int RL, int RU, int CPW>
__global__ __launch_bounds__(1024) void nnf_hals_wave_kernel(hals_args a, int64_t ldg, float* __restrict__ snap) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    constexpr int W = 64 * RL;
    wave_ctl* ctl = reinterpret_cast<wave_ctl*>(wlds + (size_t)RU * W);
    const int NW = (blockDim.x >> 6) - WAVE_COMM;         // compute waves; waves NW .. NW+3 are the communication waves
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nblocks = gridDim.x;
    auto gram = [&](int i, int k) -> float {              // UtU[i][k] as stored (rows: see the preparation kernel's note)
        const float g = a.Gp[(int64_t)i * ldg + k];
        return a.Gs ? g * a.Gs[(int64_t)i * ldg + k] : g;
    };
    for (int e = threadIdx.x; e < RU * W; e += blockDim.x) {
        const int k = e / W, c = e - k * W;
        const int i = (RL == 2) ? ((c >> 1) + 64 * (c & 1)) : c;
        float val = 0.f;
        if (k < a.r && i < a.r) {
            const float d = gram(i, i);
            if (d != 0.f) val = gram(i, k) * (float)(1.0 / (double)d);
        }
        wlds[e] = val;
    }
    for (int e = threadIdx.x; e < (int)(sizeof(wave_ctl) / 8); e += blockDim.x)
        reinterpret_cast<unsigned long long*>(ctl)[e] = 0ull;
    if (blockIdx.x == 0 && threadIdx.x == 0) hals_status_defaults(a.status);   // (rewritten by this same thread at the end)
    __syncthreads();                                      // the only barrier: image and control block are in LDS
    if (w >= NW) {
        wave_comm_loop(a, ctl, NW, w - NW, lane, nblocks);
        return;
    }
    const int64_t col0 = ((int64_t)blockIdx.x * NW + w) * CPW;
    // this lane's rows: lane (and lane + 64) of each column; start values from a.Vsrc (== a.V for an in-place solve)
    float v[CPW][RL], acc[CPW][RL], nvd[CPW][RL], dk[CPW][RL], bs[CPW][RL];
    bool dead[CPW][RL];
    float* mysnap[CPW];
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
        const int64_t col = col0 + c;
        const bool valid = col < a.ncols;
#pragma unroll
        for (int h = 0; h < RL; ++h) {
            const int row = lane + 64 * h;
            const bool in = valid && row < a.r;
            float di = 0.f;                               // 0: zero diagonal or padding row
            if (row < a.r) {
                const float d = gram(row, row);
                di = (d != 0.f) ? (float)(1.0 / (double)d) : 0.f;
            }
            dead[c][h] = !(in && di != 0.f);
            v[c][h] = in ? a.Vsrc[(int64_t)row * a.ldvs + col] : 0.f;
            const float bm = in ? a.UtM[(int64_t)row * a.ldm + col] : 0.f;
            bs[c][h] = dead[c][h] ? 0.f : (bm - a.sp) * di;
            nvd[c][h] = dead[c][h] ? -__builtin_inff() : -v[c][h];
            acc[c][h] = 0.f;
        }
        mysnap[c] = snap + ((size_t)(valid ? col : 0) * WAVE_SNAP) * W + (RL == 2 ? 2 * lane : lane);
    }
    const bool valid0 = col0 < a.ncols;                   // (a wave whose first column is past the end has nothing to sweep)
    const float* img = wlds + (RL == 2 ? 2 * lane : lane);
    // residual from scratch: acc = b' - G' v   (columns of G' one by one in row order -- the order of the reference's dot
    // product --, v[j] through an SGPR).  At the start, and again every WAVE_REFRESH sweeps: the pushes in between carry it
    // forward exactly up to one rounding each, and the refresh keeps those roundings from adding up over a long solve.
    auto refresh = [&]() {
#pragma unroll
        for (int c = 0; c < CPW; ++c)
#pragma unroll
            for (int h = 0; h < RL; ++h) acc[c][h] = bs[c][h];
#pragma unroll
        for (int j = 0; j < RU; ++j) {
            float g[RL];
#pragma unroll
            for (int h = 0; h < RL; ++h) g[h] = img[j * W + h];
#pragma unroll
            for (int c = 0; c < CPW; ++c) {
                const float vj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[c][j >> 6]), j & 63));
#pragma unroll
                for (int h = 0; h < RL; ++h) acc[c][h] = fmaf(g[h], -vj, acc[c][h]);
            }
        }
    };
    if (valid0) refresh();
    // Which row update this wave runs, decided once: everything that enters a sweep is in the start values, the scaled
    // right-hand side and the first residual (a non-finite Gram entry makes the residual of its row non-finite whatever v
    // holds: 0 * Inf and 0 * NaN are NaN).  All finite: they stay finite (fp32 overflow aside) and the one-instruction form
    // is exact; else the wave runs the form that keeps NaN and Inf as the reference does.
    bool odd = false;
#pragma unroll
    for (int c = 0; c < CPW; ++c)
#pragma unroll
        for (int h = 0; h < RL; ++h)
            odd = odd || (valid0 && !(acc[c][h] * 0.f == 0.f)) || !(v[c][h] * 0.f == 0.f) || !(bs[c][h] * 0.f == 0.f);
    const bool exact = __ballot(odd) != 0ull;             // wave-uniform
    const int S = a.max_sweeps;
    int judged = 0;                                       // verdicts read so far: sweeps 1 .. judged go on
    unsigned stop = 0u;                                   // the stopping sweep once its verdict has been read; WAVE_ERR
    // Verdicts are read IN SWEEP ORDER.  The sweep loop looks at ONE ring word per sweep (verdicts arrive at the rate of the
    // sweeps, a few sweeps late: that keeps pace) and only when it would otherwise overrun the ring does it wait.
    auto take = [&](unsigned long long x) -> bool {       // x: the ring word of sweep judged + 1; true = it was that sweep's verdict
        if ((int)(unsigned)(x >> 32) != judged + 1) return false;
        ++judged;
        const unsigned fl = (unsigned)x;
        if (fl != 0u) stop = (fl == 1u) ? (unsigned)judged : WAVE_ERR;
        return true;
    };
    auto wait_verdicts = [&](int need) {                  // rare path: until sweep `need` is judged (bounded)
        unsigned spins = 0;
        while (stop == 0u && judged < need) {
            if (take(wave_ld(&ctl->ver[(judged + 1) & (WAVE_SNAP - 1)]))) { spins = 0; continue; }
            __builtin_amdgcn_s_sleep(2);
            if (++spins > HALS_SPIN_LIMIT) stop = WAVE_ERR;
        }
    };
    int ran = 0;                                          // sweeps this wave has run
    for (int s = 1; s <= S; ++s) {
        // the slot / snapshot of sweep s reuses those of sweep s - WAVE_SNAP: that sweep must have been judged (and go on)
        (void)take(wave_ld(&ctl->ver[(judged + 1) & (WAVE_SNAP - 1)]));
        if (__builtin_expect(judged < s - WAVE_SNAP + 1, 0)) wait_verdicts(s - WAVE_SNAP + 1);
        if (stop != 0u) break;
#pragma unroll
        for (int c = 0; c < CPW; ++c)
#pragma unroll
            for (int h = 0; h < RL; ++h) dk[c][h] = 0.f;
        if (valid0 && s > 1 && ((s - 1) & (WAVE_REFRESH - 1)) == 0) refresh();
        if (valid0 && !(WAVE_DBG & 4)) {
            if (exact) wave_rows<RL, CPW, 0, RU, true>::run(img, acc, nvd, dk, dead);
            else wave_rows<RL, CPW, 0, RU, false>::run(img, acc, nvd, dk, dead);
        }
        float f = 0.f;
        const int sl = s & (WAVE_SNAP - 1);
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
#pragma unroll
            for (int h = 0; h < RL; ++h) {
                v[c][h] += dk[c][h];
                nvd[c][h] = dead[c][h] ? -__builtin_inff() : -v[c][h];
                f = fmaf(dk[c][h], dk[c][h], f);
            }
            if (col0 + c < a.ncols) {                     // V after sweep s: coalesced, fire and forget (read back by this wave only)
#pragma unroll
                for (int h = 0; h < RL; ++h) mysnap[c][(size_t)sl * W + h] = v[c][h];
            }
        }
        const double wsum = (double)wave_sum_f32(f);
        if (lane == 0) wave_st_tagged(&ctl->slot[sl][w][0], (unsigned)s, wsum);
        ran = s;
    }
    if (stop == 0u && S >= 1) wait_verdicts(S);           // the budget ran out: every sweep must be judged
    const unsigned last = stop != 0u ? stop : (unsigned)S;    // the sweep whose column is the result
    if (w == 0 && lane == 0) wave_st(&ctl->fin, (1ull << 32) | (unsigned long long)last);     // (communication waves may leave)
    // A time-out seen by ANY compute wave is left in the call's workspace word, tagged with the call's epoch: workgroup 0 may
    // still find every granule later (it needs the same late granule, so it ends after this store) and folds the word in.
    const unsigned err_tag = 0xE0000000u | a.sy.epoch;
    if (last == WAVE_ERR && lane == 0) __hip_atomic_store(a.sy.counter, err_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (S >= 1) {
        if (last != WAVE_ERR && (int)last != ran) __builtin_amdgcn_s_waitcnt(0);   // (own snapshot stores have landed before they are read back)
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
            const int64_t col = col0 + c;
            if (col < a.ncols) {
                if (last != WAVE_ERR && (int)last != ran) {   // sweeps run ahead of the stop are dropped
                    const int sl = (int)last & (WAVE_SNAP - 1);
#pragma unroll
                    for (int h = 0; h < RL; ++h) v[c][h] = __builtin_nontemporal_load(&mysnap[c][(size_t)sl * W + h]);
                }
#pragma unroll
                for (int h = 0; h < RL; ++h) {
                    const int row = lane + 64 * h;
                    if (row < a.r) a.V[(int64_t)row * a.ldv + col] = v[c][h];
                }
            }
        }
    }
    if (blockIdx.x == 0 && w == 0 && lane == 0) {
        double eps = 1.0, eps0 = 0.0;
        const bool judged_all = S >= 1 && last != WAVE_ERR;
        if (judged_all) {
            (void)wave_ld_tagged(&ctl->tot[(int)last & (WAVE_SNAP - 1)][0], last, eps);
            (void)wave_ld_tagged(&ctl->eps0[0], 1u, eps0);
            if (last == 1u) eps0 = eps;
            if (WAVE_DBG & 1) { eps = 1.0; eps0 = 0.0; }
        }
        hals_status_finish(a.status, judged_all, 0, (int)last, eps, eps0,   // (no chained launches: sweep0 = 0)
                           last == WAVE_ERR || __hip_atomic_load(a.sy.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == err_tag);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------
static size_t wave_lds(int r) { return (size_t)wave_ru(r) * 64 * wave_rl(r) * 4 + sizeof(wave_ctl) + 16; }

template <int RL, int RU, int CPW>
static int wave_per_cu(int nw) {
    static int cached[WAVE_MAX_NW + 1];               // per instance and nw: workgroups per CU + 1 (0 = not asked yet)
    if (cached[nw] == 0) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&nnf_hals_wave_kernel<RL, RU, CPW>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        int nb = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, nnf_hals_wave_kernel<RL, RU, CPW>, 64 * (nw + WAVE_COMM),
                                                                           wave_lds(RU));
        cached[nw] = hals_per_cu(e, nb, 0) + 1;
    }
    return cached[nw] - 1;
}
template <int RL, int RU, int CPW>
static int wave_launch(int nw, const hals_args& a, int64_t ldg, float* snap, int nblocks, hipStream_t st) {
    hipLaunchKernelGGL((nnf_hals_wave_kernel<RL, RU, CPW>), dim3(nblocks), dim3(64 * (nw + WAVE_COMM)), wave_lds(RU), st, a, ldg, snap);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}
#define WAVE_CASES(FN, ...)                                                                                                  \
    switch (wave_ru(r)) {                                                                                                    \
        WAVE_CASE(8, FN, __VA_ARGS__) WAVE_CASE(16, FN, __VA_ARGS__) WAVE_CASE(24, FN, __VA_ARGS__) WAVE_CASE(32, FN, __VA_ARGS__)     \
        WAVE_CASE(40, FN, __VA_ARGS__) WAVE_CASE(48, FN, __VA_ARGS__) WAVE_CASE(56, FN, __VA_ARGS__) WAVE_CASE(64, FN, __VA_ARGS__)    \
        WAVE_CASE(72, FN, __VA_ARGS__) WAVE_CASE(80, FN, __VA_ARGS__) WAVE_CASE(88, FN, __VA_ARGS__) WAVE_CASE(96, FN, __VA_ARGS__)    \
        WAVE_CASE(104, FN, __VA_ARGS__) WAVE_CASE(112, FN, __VA_ARGS__) WAVE_CASE(120, FN, __VA_ARGS__) WAVE_CASE(128, FN, __VA_ARGS__) \
    }
#define WAVE_CASE(N, FN, ...) \
    case N: return cpw == 1 ? FN<(N <= 64 ? 1 : 2), N, 1>(__VA_ARGS__) : FN<(N <= 64 ? 1 : 2), N, 2>(__VA_ARGS__);

int nnf_hals_wave_per_cu(int r, int cpw, int nw) {
    WAVE_CASES(wave_per_cu, nw)
    return 0;
}
int nnf_hals_wave_launch(int cpw, int nw, const hals_args& a, int64_t ldg, float* snap, int nblocks, hipStream_t st) {
    const int r = a.r;
    WAVE_CASES(wave_launch, nw, a, ldg, snap, nblocks, st)
    return NNF_ERR_UNSUPPORTED;
}

// status defaults and the barrier word (a solve with no sweep to run); the sweep kernel builds its image from the Gram(s)
int nnf_hals_wave_prep(const float* UtU, const float* UtU2, int64_t ldg, int r, float* Gw, unsigned* counter, double* status,
                       hipStream_t st) {
    const int ru = wave_ru(r), rl = wave_rl(r);
    hipLaunchKernelGGL(nnf_hals_prep_wave_kernel, dim3(ru), dim3(64), 0, st, UtU, UtU2, ldg, r, rl, Gw, Gw + (size_t)ru * 64 * rl,
                       counter, status);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// Resident lane solve (mode 0) of the row-split ranks, 32 < RP <= 52, with the stopping exchange on a spare wave: workgroups of
// 8 compute waves + 1 communication wave, one per CU.  The plan (k_hals_plan.h) takes this form where the 256-thread workgroups
// of k_hals_fast.hip already put two waves on some SIMDs (more workgroups than CUs); results are theirs bit for bit.
//
// Room for the ninth wave: the scaled right-hand side b[] lives in LDS (b_lds[k][thread], 2 KB per row) instead of RP registers
// per lane, read back one row ahead by the sweep itself (hals_b_lds, k_hals_lane_sweep.h): the kernel stays under 168 VGPRs, so
// three waves fit the SIMD that hosts the communication wave.
//
// Compute wave, per sweep s: sweep in registers; every lane leaves its fp32 sum of squared steps in nd[s & 1][thread], lane 0
// then writes the wave's tag s; after the sweep the wave reads ONE word, the verdict of sweep s - 1 (lag-one speculation and the
// register copy of V as in the 256-thread form), and only spins (bounded) if it is not there yet.  No barrier, no DPP ladder,
// no granule traffic.
// Communication wave, per sweep c: waits for the 8 tags, forms the block sum of each 256-column half exactly as a 256-thread
// workgroup does ((double)f per lane, the DPP ladder per 64 lanes, the four wave sums in wave order) and publishes it as granule
// 2 * blockIdx + half of the same granule space (one granule per 256 columns, hals_publish's format); then collects all granules
// of sweep c, adds them in the order of hals_sum_collect1 (thread 64k + l takes g[64k + l] + g[256 + 64k + l], ladder per 64, the
// four in order) and leaves the verdict hals_goes_on() in a tagged LDS ring.  The four ladders of a sum run as one (lc_sum4x64).  It sleeps in every poll, every spin is bounded,
// and `fin` lets it leave when a compute wave has given up.  Status block and chained launches: hals_take_over /
// hals_status_finish as everywhere.
#include "k_hals_common.h"
#include "k_hals_lane_sweep.h"

constexpr int LC_CW = 8;                      // compute waves per workgroup
constexpr int LC_COLS = 64 * LC_CW;           // columns per workgroup
constexpr int LC_THREADS = LC_COLS + 64;      // + the communication wave
constexpr int LC_RING = 4;                    // tag / verdict rings (a compute wave runs at most one sweep ahead of the verdicts)
constexpr int LC_NP = 8;                      // granule pairs per lane of the communication wave: at most 512 granules
static_assert(LC_COLS == HALS_B_PITCH, "one row of b_lds holds the workgroup's columns");

// LDS control block behind b_lds and nd: every word that crosses waves carries the sweep it belongs to
struct lane_ctl {
    unsigned tag[LC_RING][LC_CW];             // s once the wave's 64 sums of sweep s are in nd[s & 1]
    unsigned long long ver[LC_RING];          // verdict {sweep : 32 | 0 = go on, 1 = stop, 2 = time-out : 32}
    unsigned fin;                             // a compute wave has given up: the communication wave may leave
};
static inline size_t lc_lds_bytes(int RP) { return ((size_t)RP + 2) * LC_COLS * 4 + sizeof(lane_ctl); }

#define LC_WG __HIP_MEMORY_SCOPE_WORKGROUP

// granule `gi` of sweep s: hals_publish with the granule index given (one lane)
__device__ __forceinline__ void lc_publish(const hals_sync& sy, int s, int ngran, int gi, double mine) {
    const hals_word bits = __builtin_bit_cast(hals_word, mine);
    const hals_word tag = (hals_word)hals_tag(sy, s) << 32;
    hals_word* g = reinterpret_cast<hals_word*>(sy.sslots) + ((size_t)s * ngran + gi) * 2;
    __hip_atomic_store(g, tag | (bits & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, tag | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// until every compute wave has left its sums of sweep c (bounded); false: time-out, or the compute waves have left.
// The communication wave shares its SIMD with two compute waves and every instruction it issues is taken from them: a poll
// is a handful of instructions every ~256 cycles.
__device__ __forceinline__ bool lc_wait_tags(const lane_ctl* ctl, int c, int lane) {
    unsigned spins = 0;
    for (;;) {
        const unsigned t = __hip_atomic_load(&ctl->tag[c & (LC_RING - 1)][lane & (LC_CW - 1)], __ATOMIC_ACQUIRE, LC_WG);
        if (__ballot(t != (unsigned)c) == 0ull) return true;
        if (__hip_atomic_load(&ctl->fin, __ATOMIC_RELAXED, LC_WG) != 0u) return false;
        __builtin_amdgcn_s_sleep(4);
        if (++spins > HALS_SPIN_LIMIT) return false;
    }
}

// Four of nnf_wave_sum_f64's fixed-order 64-value sums in ONE pass.  Row k of the wave (lanes 16k .. 16k + 15) stands for wave k
// of a 256-thread workgroup, lane 16k + m holds that wave's values 4m .. 4m + 3, i.e. lane L holds values 4L .. 4L + 3 of the
// 256.  nnf_wave_sum_f64 is a balanced binary tree over the lanes -- neighbours (xor 1), pairs of neighbours (xor 2), the two
// quads of a half row, the two halves of a row, rows 0 + 1 and 2 + 3, and those two -- and fp64 addition commutes, so the same
// tree is: two levels inside the lane, then xor 1, xor 2, half-row mirror and row mirror across lanes.  Same additions on the
// same operands, a fifth of the instructions.  Every lane of row k returns sum k.
__device__ __forceinline__ double lc_sum4x64(double x0, double x1, double x2, double x3) {
    double v = (x0 + x1) + (x2 + x3);
    v = nnf_dpp_add_f64<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v = nnf_dpp_add_f64<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v = nnf_dpp_add_f64<0x141, 0xf>(v);   // row_half_mirror
    v = nnf_dpp_add_f64<0x140, 0xf>(v);   // row_mirror
    return v;
}
// the four row values of `v` added in row order, as the 256-thread workgroups add their four wave sums (wave-uniform)
__device__ __forceinline__ double lc_rows_in_order(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, 16 * k);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), 16 * k);
        const double w = __builtin_bit_cast(double, ((unsigned long long)hi << 32) | (unsigned long long)lo);
        t = k == 0 ? w : t + w;
    }
    return t;
}

// block sum of one 256-column half, as hals_block_sum1<256> / hals_sum_collect1<256> form it
__device__ __forceinline__ double lc_half_sum(const float* nd_half, int lane) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(nd_half + 4 * lane);
    return lc_rows_in_order(lc_sum4x64((double)x[0], (double)x[1], (double)x[2], (double)x[3]));
}

// global sum of sweep c over the `ngran` granules, in the order of the 256-thread workgroups: thread t = 64k + l of those takes
// g[t] + g[256 + t] -- here lane L takes t = 4L .. 4L + 3 (lc_sum4x64).  Every request of a round goes out before the first answer
// is looked at (a lane's granules past the last one re-read granule 0 and ignore it); the first round waits until the other
// workgroups have had time to publish, and a round with a stale granule is repeated after a sleep (bounded).  false: time-out,
// or `fin` set.
__device__ __forceinline__ bool lc_total(const hals_sync& sy, const lane_ctl* ctl, int c, int ngran, int lane, double& total) {
    const unsigned tag = hals_tag(sy, c);
    const hals_word* base = hals_row(sy, c, ngran);
    hals_word g0[LC_NP], g1[LC_NP];
    unsigned spins = 0;
    __builtin_amdgcn_s_sleep(32);
    for (;;) {
#pragma unroll
        for (int i = 0; i < LC_NP; ++i) {
            const int t = 256 * (i >> 2) + 4 * lane + (i & 3);
            const int b = t < ngran ? t : 0;
            g0[i] = __hip_atomic_load(base + 2 * (size_t)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            g1[i] = __hip_atomic_load(base + 2 * (size_t)b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        bool fresh = true;
#pragma unroll
        for (int i = 0; i < LC_NP; ++i) fresh = fresh && (unsigned)(g0[i] >> 32) == tag && (unsigned)(g1[i] >> 32) == tag;
        if (__ballot(!fresh) == 0ull) break;
        __builtin_amdgcn_s_sleep(16);
        if (++spins > HALS_SPIN_LIMIT || ((spins & 63u) == 0u && __hip_atomic_load(&ctl->fin, __ATOMIC_RELAXED, LC_WG) != 0u)) return false;
    }
    double x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {             // thread t = 4 lane + j of a 256-thread workgroup: its two granule pairs
        double v = 0.0;
        v += (4 * lane + j < ngran) ? hals_granule_value(g0[j], g1[j]) : 0.0;
        v += (256 + 4 * lane + j < ngran) ? hals_granule_value(g0[j + 4], g1[j + 4]) : 0.0;
        x[j] = v;
    }
    total = lc_rows_in_order(lc_sum4x64(x[0], x[1], x[2], x[3]));
    return true;
}

__device__ __forceinline__ void lc_verdict(lane_ctl* ctl, int c, unsigned flag, int lane) {
    if (lane == 0)
        __hip_atomic_store(&ctl->ver[c & (LC_RING - 1)], ((unsigned long long)(unsigned)c << 32) | (unsigned long long)flag,
                           __ATOMIC_RELAXED, LC_WG);
}

// the communication wave: sweeps 1 .. max_sweeps in turn; eps0 / eps come in as hals_take_over left them
__device__ __forceinline__ void lc_comm_loop(const hals_args& a, lane_ctl* ctl, const float* nd, int ngran, int lane, double eps0, double eps) {
    int done = 0;
    bool ok = true;
    for (int c = 1; c <= a.max_sweeps; ++c) {
        if (!lc_wait_tags(ctl, c, lane)) { ok = false; lc_verdict(ctl, c, 2u, lane); break; }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int gi = 2 * (int)blockIdx.x + h;
            if (gi < ngran) {                 // (a ragged last workgroup may hold one half only)
                const double bs = lc_half_sum(nd + (c & 1) * LC_COLS + 256 * h, lane);
                if (lane == 0) lc_publish(a.sy, c, ngran, gi, bs);
            }
        }
        double tot;
        if (!lc_total(a.sy, ctl, c, ngran, lane, tot)) { ok = false; lc_verdict(ctl, c, 2u, lane); break; }
        if (c == 1 && a.sweep0 == 0) eps0 = tot;
        eps = tot;
        done = c;
        const bool on = hals_goes_on(eps, a.delta, eps0);   // nnls.py:156
        lc_verdict(ctl, c, on ? 0u : 1u, lane);
        if (!on) break;
    }
    if (blockIdx.x == 0 && lane == 0) hals_status_finish(a.status, a.max_sweeps >= 1, a.sweep0, done, eps, eps0, !ok);
}

template <int RP>
__global__ __launch_bounds__(LC_THREADS) void nnf_hals_comm_kernel(hals_args a, int ngran) {
    static_assert(RP > 32 && RP <= 52, "the row-split ranks");
    extern __shared__ __attribute__((aligned(16))) float lc_lds[];
    float* b_lds = lc_lds;                                // [RP][LC_COLS]
    float* nd_lds = lc_lds + (size_t)RP * LC_COLS;        // [2][LC_COLS]
    lane_ctl* ctl = reinterpret_cast<lane_ctl*>(nd_lds + 2 * LC_COLS);
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    double eps0 = 0.0, eps = 1.0;
    if (a.sweep0 > 0 && !hals_take_over(a.status, a.sweep0, a.delta, eps0, eps)) return;   // (every thread of the grid alike)
    for (int e = tid; e < (int)(sizeof(lane_ctl) / 4); e += LC_THREADS) reinterpret_cast<unsigned*>(ctl)[e] = 0u;
    __syncthreads();                                      // the only barrier: the control block is in LDS
    if (w == LC_CW) {
        lc_comm_loop(a, ctl, nd_lds, ngran, lane, eps0, eps);
        return;
    }

    const int64_t gtid = (int64_t)blockIdx.x * LC_COLS + tid;
    // descriptors over the whole matrices, as in nnf_hals_kernel: rows >= r / columns of idle lanes fall outside num_records
    const rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(a.V, 0, (int)(((int64_t)(a.r - 1) * a.ldv + a.ncols) * 4), 0x00020000);
    const rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.UtM), 0,
                                                        (int)(((int64_t)(a.r - 1) * a.ldm + a.ncols) * 4), 0x00020000);
    const rsrc_t rvs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.Vsrc), 0,
                                                         (int)(((int64_t)(a.r - 1) * a.ldvs + a.ncols) * 4), 0x00020000);
    const int ldv4 = (int)(a.ldv * 4), ldm4 = (int)(a.ldm * 4), ldvs4 = (int)(a.ldvs * 4);
    const int voff0 = gtid < a.ncols ? (int)(gtid * 4) : (int)0x7ffffff0;
    const bool all_live = a.dinv[2 * RP] != 0.f;          // wave-uniform: no zero on the Gram diagonal (prep kernel)
    f32x2 v2[RP / 2], vb[RP / 2];
    bool plain;
    {
        float b[RP];
#pragma unroll
        for (int k = 0; k < RP; ++k) {
            v2[k / 2][k & 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rvs, voff0, k * ldvs4, 0));
            b[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, voff0, k * ldm4, 0)) - a.sp;
            b[k] *= a.dinv[2 * k];
        }
        // finite operands take the one-instruction row update (see nnf_hals_kernel): the same test, wave-local
        float c = a.Gs[lane < RP ? lane * 64 + 63 : 63];
#pragma unroll
        for (int k = 0; k < RP; ++k) {
            c = fmaf(v2[k / 2][k & 1], 0.f, c);
            c = fmaf(b[k], 0.f, c);
            asm volatile("" : "+v"(c));
            b_lds[k * LC_COLS + tid] = b[k];
        }
        plain = all_live && __ballot(!(c == 0.f)) == 0ull;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // b is in LDS before the first hand-issued read (and not sunk below it)
    const unsigned ba = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float*)(b_lds + tid);
    const hals_b_lds bsrc{ba, ba + 32u * LC_COLS * 4u, {0.f, 0.f}};

    bool ok = true, stopped = false;
    for (int s = 1; s <= a.max_sweeps; ++s) {
#pragma unroll
        for (int k = 0; k < RP / 2; ++k) vb[k] = v2[k];   // V after sweep s-1
        const float f = plain ? hals_sweep_column_xy<RP, false>(v2, bsrc, a.Gs, a.dinv, hals_mid_none{})
                              : hals_sweep_column_xy<RP, true>(v2, bsrc, a.Gs, a.dinv, hals_mid_none{});
        nd_lds[(s & 1) * LC_COLS + tid] = gtid < a.ncols ? f : 0.f;
        if (lane == 0) __hip_atomic_store(&ctl->tag[s & (LC_RING - 1)][w], (unsigned)s, __ATOMIC_RELEASE, LC_WG);
        if (s >= 2) {   // the verdict of sweep s-1, formed while this sweep ran
            const unsigned long long* vp = &ctl->ver[(s - 1) & (LC_RING - 1)];
            unsigned long long x = __hip_atomic_load(vp, __ATOMIC_RELAXED, LC_WG);
            unsigned spins = 0;
            while ((unsigned)(x >> 32) != (unsigned)(s - 1)) {
                if (++spins > HALS_SPIN_LIMIT) { x = 2ull; break; }
                if (spins < 64u) __builtin_amdgcn_s_sleep(1);
                else __builtin_amdgcn_s_sleep(16);
                x = __hip_atomic_load(vp, __ATOMIC_RELAXED, LC_WG);
            }
            const unsigned flag = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)x);
            if (flag == 1u) { stopped = true; break; }    // nnls.py:156: sweep s-1 was the last one
            if (flag != 0u) { ok = false; break; }
        }
    }
    if (!ok && lane == 0) __hip_atomic_store(&ctl->fin, 1u, __ATOMIC_RELAXED, LC_WG);
    if (stopped || !ok) {   // the registers hold one sweep too many: fall back to the copy
#pragma unroll
        for (int k = 0; k < RP / 2; ++k) v2[k] = vb[k];
    }
#pragma unroll
    for (int k = 0; k < RP; ++k) {
        const float val = v2[k / 2][k & 1];
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), rv, voff0, k * ldv4, 0);
    }
    if (!ok && blockIdx.x == 0 && tid == 0) hals_status_finish(a.status, false, 0, 0, 0.0, 0.0, true);
}

// ---- host side --------------------------------------------------------------------------------------------------------
template <int RP>
static int comm_per_cu() {
    static int cached = -1;
    if (cached < 0) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&nnf_hals_comm_kernel<RP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lc_lds_bytes(RP));
        int nb = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, nnf_hals_comm_kernel<RP>, LC_THREADS, lc_lds_bytes(RP));
        cached = hals_per_cu(e, nb, 1);
    }
    return cached;
}
template <int RP>
static int comm_launch(const hals_args& a, int nblocks, hipStream_t st) {
    if (comm_per_cu<RP>() < 1) return NNF_ERR_LAUNCH;     // (also raises the kernel's dynamic LDS limit, once)
    const int ngran = (int)nnf_cdiv(a.ncols, 256);
    if (ngran > 64 * LC_NP || nblocks != (int)nnf_cdiv(a.ncols, LC_COLS) || a.mode != 0) return NNF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((nnf_hals_comm_kernel<RP>), dim3(nblocks), dim3(LC_THREADS), lc_lds_bytes(RP), st, a, ngran);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

#define LC_RANKS(X) X(40) X(48) X(50) X(52)   // pick_rp's padded ranks above 32 and up to 52
int nnf_hals_comm_per_cu(int RP) {
#define LC_PER_CU(v) case v: return comm_per_cu<v>();
    switch (RP) { LC_RANKS(LC_PER_CU) default: return 0; }
}
int nnf_hals_comm_launch(int RP, const hals_args& a, int nblocks, hipStream_t st) {
#define LC_LAUNCH(v) case v: return comm_launch<v>(a, nblocks, st);
    switch (RP) { LC_RANKS(LC_LAUNCH) default: return NNF_ERR_UNSUPPORTED; }
}

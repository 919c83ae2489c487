// The plan of a HALS sweep call (k_hals.hip: hals_entry): which kernel runs it, on which grid and after which preparation, decided
// in ONE place from the shape of the call, the CU count and the workgroups per CU the occupancy API reports -- the launch and the
// capacity queries (nnf_hals_resident_columns, nnf_hals_resid_floats) read the same answer.  It launches nothing and takes no
// workspace.  Also the pure size arithmetic of the layouts (k_hals_wave.hip, k_hals_quad.hip, k_hals_mfma.hip read their constants
// from here) and the NNF_HALS_DEBUG line that reports a plan.  No HIP in here: the occupancy answers come in through five plain
// function pointers (hals_occupancy), so tools/nnf_plan.cpp, a plain host program, prints the same plans for any CU count and
// any set of per-CU figures (tests/test_hals_plan_table.py).
#pragma once
#include "k_stream_plan.h"

#define NNF_HALS_MAX_SWEEPS 1000   // per launch: the exchange tag holds the sweep index in 10 bits (k_hals_common.h)
#define NNF_HALS_MAX_BLOCKS 2048   // workgroups of one persistent solve (3 * 256 CUs fits)

enum hals_layout { HL_WAVE, HL_QUAD, HL_MFMA, HL_LANE_RES, HL_LANE_STREAM, HL_GENERIC_LDS, HL_GENERIC_BIG, HL_GENERIC_GCOL };
static const char* const hals_layout_name[] = {"wave", "quad", "mfma", "lane-resident", "lane-streaming", "generic-lds",
                                               "generic-lds-big", "generic-gcol"};

// What the plan reads of a call: plain values (hals_request, k_hals.hip, keeps the pointers and yields this)
struct hals_shape {
    int mode;                      // 0: solve (stopping rule on the device)  1: fixed sweep count, per-sweep sums
    int r; int64_t ncols;
    int64_t ldm, ldv, ldvs;        // row strides of UtM, V and the start values (ldvs = ldv where V holds them)
    int nsweeps, sweep0;           // sweep0: sweeps already run by earlier launches of the same solve
    unsigned flags;
    bool gram2;                    // a second Gram is present (Hadamard pair)
    bool own_start;                // separate start values are given (Vsrc != V)
    bool snapshots;                // snapshots were asked for
    // NNF_HALS_FORCE pins the layout (tests run every kernel on the same fixtures); its first letter counts (0: not set):
    //   l lane only;  q no wave, no mfma, quad beyond 32768 columns;  w no mfma, a solve wave cannot hold is refused;
    //   m mfma ahead of wave and quad where it covers the padded rank;
    //   c lane only, and the resident solve of ranks 33 .. 52 in its 576-thread form (hals_plan::comm) at any number of columns
    char force;
};

struct hals_plan {
    int err = NNF_OK;              // else: what the call is refused with
    hals_layout layout = HL_LANE_RES;
    int RP = 0, nblocks = 0, per_cu = 0;   // padded rank (lane, mfma, generic); grid; workgroups per CU it relies on
    int cpw = 0, nw = 0, ch = 0;   // wave: columns per compute wave, compute waves per workgroup; quad: rows per lane
    size_t lds = 0;                // generic: dynamic LDS bytes
    bool hadamard = false, copy = false, prep = true;   // launches in front of the sweep
    bool gs = false;               // lane, mfma: the row-scaled Gram next to the padded one
    bool comm = false;             // lane-resident: the 576-thread form (k_hals_comm.hip: 512 columns per workgroup, one per CU)
    size_t gram_floats = 0, mfma_floats = 0, snap_floats = 0;   // workspace
};

// Workgroups per CU a persistent launch of one kernel instance relies on (0: it does not fit at all).  The library answers
// from the occupancy API, cached per instance (k_hals_common.h: hals_per_cu and the layouts' queries).
struct hals_occupancy {
    int (*wave)(int r, int cpw, int nw);
    int (*quad)(int ch);
    int (*lane)(int RP, bool resident);
    int (*mfma)(int RP);
    int (*generic)(int mode, hals_layout layout, int r, size_t lds_bytes, int cap);   // cap: at most so many (0: no cap)
    int (*lane_comm)(int RP);      // the 576-thread form of the resident lane solve
};

static inline int pick_rp(int r) {
    const int opts[] = {8, 16, 24, 32, 40, 48, 50, 52, 56, 64, 80, 96, 100, 104, 112, 128};   // 100: config E's rank
    for (int o : opts)
        if (r <= o) return o;
    return (r + 7) & ~7;      // above NNF_MAX_RANK: the generic kernel only (its padded Gram has one row per 8)
}

// ---- k_hals_wave.hip: one wave per column ----
constexpr int WAVE_COMM = 4;         // communication waves per workgroup
constexpr int WAVE_MAX_NW = 16 - WAVE_COMM;   // compute waves (= columns) per workgroup (1024 threads in all)
constexpr int WAVE_SNAP = 16;        // snapshot / slot / verdict rings (sweeps a compute wave may run ahead of the verdicts, + 1)
constexpr int WAVE_NP = 6;           // granule pairs per lane of a communication wave: nblocks <= 384
static inline int wave_ru(int r) { return (r + 7) & ~7; }
static inline int wave_rl(int r) { return r <= 64 ? 1 : 2; }
static inline size_t nnf_hals_wave_gram_floats(int r) { return (size_t)wave_ru(r) * 64 * wave_rl(r) + 128; }
static inline size_t nnf_hals_wave_snap_floats(int r, int64_t ncols) { return (size_t)ncols * WAVE_SNAP * 64 * wave_rl(r); }
// nw compute waves per workgroup (about one workgroup per CU), workgroups for cpw columns per compute wave; 0: more
// workgroups than the communication waves collect
static inline int nnf_hals_wave_grid(int64_t ncols, int cpw, int* nw_out) {
    int nw = (int)nnf_cdiv(ncols, 256);
    if (nw < 1) nw = 1;
    if (nw > WAVE_MAX_NW) nw = WAVE_MAX_NW;
    *nw_out = nw;
    const int64_t need = nnf_cdiv(ncols, (int64_t)nw * cpw);
    return need > 64 * WAVE_NP ? 0 : (int)need;
}

// ---- k_hals_quad.hip: the row-scaled Gram image, then 1/diag per row ----
static inline size_t nnf_hals_quad_gram_floats(int r) {
    const int ch = (r + 3) / 4, rq = 4 * ch, rs = 4 * ((ch + 3) & ~3);
    return (size_t)rq * rs + rq;
}

// ---- k_hals_mfma.hip: row tiles, leftover rows and k-blocks of a padded rank ----
struct mfma_shape { int rt, rem, nkb; };
static inline bool mfma_shape_of(int RP, mfma_shape& s) {
    switch (RP) {
        case 48: s = {3, 0, 12}; return true;
        case 50: s = {3, 2, 13}; return true;
        case 52: s = {3, 4, 13}; return true;
        case 64: s = {4, 0, 16}; return true;
        case 80: s = {5, 0, 20}; return true;
        case 96: s = {6, 0, 24}; return true;
        case 100: s = {6, 4, 25}; return true;
        default: return false;
    }
}
static inline bool nnf_hals_mfma_supported(int RP) { mfma_shape s; return mfma_shape_of(RP, s); }
static inline size_t nnf_hals_mfma_gram_floats(int RP) {
    mfma_shape s;
    if (!mfma_shape_of(RP, s)) return 0;
    return (size_t)s.nkb * ((s.rt + 3) / 4) * 256 + (size_t)s.nkb * 32 + 64;
}
// floats of residual state a chunked solve of `ncols` columns carries from launch to launch (0: rank not covered)
static inline size_t nnf_hals_mfma_resid_floats(int RP, int64_t ncols) {
    mfma_shape s;
    if (!mfma_shape_of(RP, s) || ncols < 1) return 0;
    return (size_t)nnf_cdiv(ncols, 256) * 4 * (s.rt * 4 + 1) * 256;
}

// ---- k_hals.hip: the generic kernel, three forms (column in LDS; four lanes per column in LDS, above rank 128; GCOL) per mode ----
constexpr size_t HALS_GENERIC_LDS_MAX = (size_t)150 * 1024;   // columns in LDS up to here
constexpr size_t HALS_GENERIC_SHM_FIXED = 16 + 3 * 2 * 8 + 64;

// ---- k_hals_comm.hip: granules (one per 256 columns) its communication wave collects, 8 pairs per lane ----
constexpr int HALS_COMM_MAX_GRANULES = 512;

static inline int64_t hals_cap(int cus, int per_cu) {   // workgroups that stay resident at per_cu per CU
    const int64_t c = (int64_t)per_cu * cus;
    return c < NNF_HALS_MAX_BLOCKS ? c : NNF_HALS_MAX_BLOCKS;
}
// The buffer offsets of rows 0 .. rows-1 of an operand with row stride ld fit 32 bits.  The lane and mfma kernels load (and
// store) all RP padded rows of a column and rely on the rows >= r falling outside the descriptor: checked with rows = RP, so
// that no padded row's offset wraps back into the rows of the operand.
static inline bool hals_32bit(int rows, int64_t ld, int64_t ncols) {
    return (((int64_t)(rows - 1) * ld + ncols) * 4) < (int64_t)0x7fff0000;
}

// the padded Gram (RP x RS, RS = RP rounded up to 32) and the RP (1/diag, nz) pairs + the all-live flag, then (64-byte
// aligned) the row-scaled Gram of the lane kernel
static inline size_t hals_gs_off(int RP) { return ((((size_t)RP * (32 * ((RP + 31) / 32)) + 2 * RP + 1) + 15) & ~(size_t)15); }

static inline hals_plan hals_refuse(hals_plan p, int err) { p.err = err; return p; }

static inline hals_plan hals_make_plan(int cus, const hals_occupancy& occ, const hals_shape& q) {
    hals_plan p;
    const int r = q.r; const int64_t n = q.ncols;
    const bool rowsync = (q.flags & (NNF_HALS_NORMALIZE | NNF_HALS_NONZERO)) != 0;
    const bool generic = r > NNF_MAX_RANK || rowsync;
    const bool sweeps = q.nsweeps > 0;
    const char force = q.force;
    p.RP = pick_rp(r);
    // many columns at ranks 64..100: the push form on the matrix cores; below rank 64 a k-block has too few MFMAs to cover its
    // own gather -> update -> scatter chain (measured: 9.7-10.6 against 9.4-9.6 us per sweep at rank 50)
    const bool mfma = !generic && sweeps && force != 'l' && force != 'c' && force != 'q' && force != 'w' && nnf_hals_mfma_supported(p.RP) &&
                      (force == 'm' || (p.RP >= 64 && n > 32768));
    const bool pin_mfma = force == 'm' && mfma;

    // few columns, a persistent solve from its first sweep: one wave per column, 1 or 2 columns per compute wave
    const bool wave_shape = !generic && q.mode == 0 && q.sweep0 == 0;
    if (wave_shape && force != 'l' && force != 'c' && force != 'q' && !pin_mfma) {
        for (int cpw = 1; cpw <= 2; ++cpw) {
            int nw = 0;
            const int need = nnf_hals_wave_grid(n, cpw, &nw);
            if (need < 1 || need > NNF_HALS_MAX_BLOCKS) continue;
            const int pc = occ.wave(r, cpw, nw);
            if (pc < 1) break;
            if (need <= (int64_t)pc * cus) {
                p.layout = HL_WAVE, p.cpw = cpw, p.nw = nw, p.nblocks = need, p.per_cu = pc;
                p.prep = !sweeps;           // (the sweep kernel builds its Gram image itself)
                p.copy = !sweeps && q.own_start;
                p.gram_floats = nnf_hals_wave_gram_floats(r);
                p.snap_floats = nnf_hals_wave_snap_floats(r, n);
                return p;
            }
        }
    }
    if (force == 'w' && wave_shape) return hals_refuse(p, NNF_ERR_UNSUPPORTED);

    // few columns (<= 32768: at most two waves per SIMD): four lanes per column, 16 columns per workgroup.  Its buffer
    // offsets reach row r + 15 of V, UtM and the start values in 32 bits: start values beyond that are copied into V first.
    auto quad_32bit = [&](int64_t ld) { return (int64_t)(r + 16) * ld * 4 < (int64_t)0x7fff0000; };
    if (!generic && force != 'l' && force != 'c' && !pin_mfma && (n <= 32768 || force == 'q') && quad_32bit(q.ldv > q.ldm ? q.ldv : q.ldm)) {
        const int ch = (r + 3) / 4, pc = occ.quad(ch);
        const int64_t need = nnf_cdiv(n, 16);
        if (pc > 0 && need <= hals_cap(cus, pc)) {
            p.layout = HL_QUAD, p.ch = ch, p.nblocks = (int)need, p.per_cu = pc;
            // (the sweep kernel reads the start values and forms the Hadamard Gram itself)
            p.copy = q.own_start && (!sweeps || !quad_32bit(q.ldvs));
            p.gram_floats = nnf_hals_quad_gram_floats(r);
            return p;
        }
    }

    // the padded Gram, 1/diag and the barrier words (nnf_hals_prep_kernel) in front of the lane, mfma and generic kernels; the
    // Hadamard Gram and separate start values come from two small launches -- except that the resident lane kernel reads its
    // start values itself (once)
    const int RS = 32 * ((p.RP + 31) / 32);
    p.gs = !generic && p.RP > 32 && p.RP <= 52;
    p.gram_floats = hals_gs_off(p.RP) + (p.gs ? (size_t)p.RP * RS : 0);
    p.hadamard = q.gram2;
    const int lane_pc = generic ? 0 : occ.lane(p.RP, true);
    const bool lane_fits = lane_pc > 0 && nnf_cdiv(n, 256) <= hals_cap(cus, lane_pc);
    p.copy = q.own_start && !(!generic && sweeps && lane_fits && hals_32bit(p.RP, q.ldvs, n));
    if (!sweeps) {   // the prep kernel only (the status defaults of a solve with no sweep to run)
        p.layout = generic ? HL_GENERIC_LDS : HL_LANE_RES;
        return p;
    }

    if (generic) {
        // one column per thread; when the workgroups exchange (mode 0, or a row-level reduction per row update) all of them are
        // resident.  The column in LDS (r x 128 floats per workgroup; above rank 128 four lanes per column, r x 32 floats) while
        // that fits and -- when the workgroups exchange -- all of them stay resident with it; else (ranks above ~1200, or more
        // columns than that holds) the column stays in global memory (GCOL).  Measured at rank 200
        // (tools/probes/bigrank_sweep_probe.py): LDS 3-5x faster per sweep.
        const bool exchanges = q.mode == 0 || rowsync;
        if (r > NNF_MAX_RANK) {
            p.layout = HL_GENERIC_BIG;
            p.lds = (size_t)r * 32 * 4 + HALS_GENERIC_SHM_FIXED;
            p.per_cu = p.lds <= HALS_GENERIC_LDS_MAX ? occ.generic(q.mode, HL_GENERIC_BIG, r, p.lds, 0) : 0;
            if (p.per_cu < 1 || (exchanges && nnf_cdiv(n, 32) > hals_cap(cus, p.per_cu))) {
                p.layout = HL_GENERIC_GCOL;
                p.lds = HALS_GENERIC_SHM_FIXED;
                p.per_cu = occ.generic(q.mode, HL_GENERIC_GCOL, r, p.lds, 4);
            }
        } else {
            p.layout = HL_GENERIC_LDS;
            p.lds = (size_t)r * 128 * 4 + HALS_GENERIC_SHM_FIXED;
            p.per_cu = occ.generic(q.mode, HL_GENERIC_LDS, r, p.lds, 4);
        }
        if (p.per_cu < 1) return hals_refuse(p, NNF_ERR_LAUNCH);
        const int64_t grid = nnf_cdiv(n, p.layout == HL_GENERIC_BIG ? 32 : 128);
        // blind sweeps without row-level reductions exchange nothing: no residency needed (any number of columns)
        if (grid > (exchanges ? hals_cap(cus, p.per_cu) : (int64_t)0x7fffffff)) return hals_refuse(p, NNF_ERR_UNSUPPORTED);
        p.nblocks = (int)grid;
        return p;
    }

    if (!hals_32bit(p.RP, q.ldv, n) || !hals_32bit(p.RP, q.ldm, n)) return hals_refuse(p, NNF_ERR_UNSUPPORTED);
    const int64_t need = nnf_cdiv(n, 256);
    if (mfma) {   // when every column stays resident; else the lane kernel
        const int pc = occ.mfma(p.RP);
        if (pc > 0 && need <= hals_cap(cus, pc)) {
            p.layout = HL_MFMA, p.nblocks = (int)need, p.per_cu = pc;
            p.mfma_floats = nnf_hals_mfma_gram_floats(p.RP);
            return p;
        }
    }
    if (lane_pc < 1) return hals_refuse(p, NNF_ERR_LAUNCH);
    if (lane_fits) {
        p.layout = HL_LANE_RES, p.nblocks = (int)need, p.per_cu = lane_pc;
        // A solve of the row-split ranks whose 256-thread workgroups outnumber the CUs has two waves on some SIMDs whatever the
        // layout: 8 compute waves per CU are no slower, and a ninth wave takes the stopping exchange off them (k_hals_comm.hip;
        // its communication wave sums at most HALS_COMM_MAX_GRANULES granules, one per 256 columns as here).
        // NNF_HALS_FORCE: `lane` keeps the 256-thread workgroups, `c` takes the new form at any number of columns.
        if (q.mode == 0 && p.gs && need <= HALS_COMM_MAX_GRANULES && force != 'l' && (force == 'c' || need > cus)) {
            const int pc = occ.lane_comm ? occ.lane_comm(p.RP) : 0;
            const int64_t need2 = nnf_cdiv(n, 512);
            if (pc > 0 && need2 <= hals_cap(cus, pc)) p.comm = true, p.nblocks = (int)need2, p.per_cu = pc;
        }
        return p;
    }
    // more columns than stay resident: the streaming form strides over column sets (no snapshots)
    if (q.snapshots) return hals_refuse(p, NNF_ERR_UNSUPPORTED);
    p.layout = HL_LANE_STREAM, p.per_cu = occ.lane(p.RP, false);
    if (p.per_cu < 1) return hals_refuse(p, NNF_ERR_LAUNCH);
    p.nblocks = (int)hals_cap(cus, p.per_cu);
    return p;
}

// the NNF_HALS_DEBUG line of a call (tests/test_gpu_hals_plans.py keys on it)
static inline void hals_report(FILE* f, const hals_shape& q, const hals_plan& p, const char* more = "") {
    fprintf(f, "[nnf hals] r=%d ncols=%lld mode=%d sweeps=%d sweep0=%d flags=%u -> %s grid=%d per_cu=%d cpw=%d nw=%d ch=%d "
            "RP=%d gs=%d lds=%zu hadamard=%d copy=%d prep=%d err=%d comm=%d%s\n", q.r, (long long)q.ncols, q.mode, q.nsweeps, q.sweep0,
            q.flags, hals_layout_name[p.layout], p.nblocks, p.per_cu, p.cpw, p.nw, p.ch, p.RP, p.gs, p.lds, p.hadamard, p.copy,
            p.prep, p.err, p.comm, more);
}

// Columns a persistent launch keeps resident at rank r (nnf_hals_resident_columns): the resident lane kernel, 256 columns per
// workgroup; above NNF_MAX_RANK the generic kernel with the column per thread in global memory (GCOL), 128 per workgroup.
// 0: that kernel does not fit.
static inline int64_t hals_resident_columns(int cus, const hals_occupancy& occ, int r) {
    if (r > NNF_MAX_RANK) return hals_cap(cus, occ.generic(0, HL_GENERIC_GCOL, r, HALS_GENERIC_SHM_FIXED, 4)) * 128;
    return hals_cap(cus, occ.lane(pick_rp(r), true)) * 256;
}

// Launch plans of the streaming and MTTKRP launchers (k_xty.hip, k_xht.hip, k_gram.hip, k_cost.hip: W^T X, X H^T, the Gram, the cost pass; k_xht_lds.hip;
// k_mttkrp.hip: the segment and rows kernels, the two dimension-tree contractions; k_mu_plan.h builds on them):
// what a call will launch, decided from sizes alone before anything is carved from the workspace or launched, and the
// NNF_PLAN_DEBUG line that reports it (every "[nnf plan]" line of the library is formatted in these two headers).  No HIP in here: tools/nnf_plan.cpp is a plain host program that prints the same plans
// for any CU count (tests/test_mu_plan_table.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nnfac_hip.h"

constexpr int64_t nnf_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr int64_t nnf_rup(int64_t a, int64_t b) { return nnf_cdiv(a, b) * b; }
constexpr int64_t NNF_OFFSET32_END = 0x7fff0000;   // the byte offsets of buffer loads stay below this

// workspace carve helper: 256-byte aligned bump allocator (a plan asks a copy of the caller's cursor what would fit; on a null
// base the same take / remaining sequence runs without a device)
struct nnf_ctx;
struct nnf_ws_cursor {
    char* base;
    size_t cap, off;
    nnf_ws_cursor(char* b, size_t c) : base(b), cap(c), off(0) {}
    nnf_ws_cursor(nnf_ctx* c);   // over ctx->ws (nnf_internal.h)
    bool reserve(size_t bytes) {   // take() without the address: what a plan asks
        const size_t a = (off + 255) & ~size_t(255);
        if (a + bytes > cap) return false;
        off = a + bytes;
        return true;
    }
    void* take(size_t bytes) { return reserve(bytes) ? base + (off - bytes) : nullptr; }
    size_t remaining() const {
        const size_t a = (off + 255) & ~size_t(255);
        return a < cap ? cap - a : 0;
    }
};

// ---- rank -> (MFMA tiles, VALU leftover rows) ----
struct nnf_rank_tiles { int MT, REM; };
// r = 16q + (1..4), q >= 1 keeps q tiles on MFMA and 2 or 4 rows on VALU (aligned X only: the callers pad otherwise)
constexpr nnf_rank_tiles nnf_split_rank(int r) {
    const int q = r / 16, rem = r % 16;
    return (q >= 1 && q <= 7 && rem >= 1 && rem <= 4) ? nnf_rank_tiles{q, rem <= 2 ? 2 : 4} : nnf_rank_tiles{(r + 15) / 16, 0};
}
// W^T X: the leftover rows need 16-byte loads of X
constexpr nnf_rank_tiles nnf_xty_tiles(int r, bool vec) { return vec ? nnf_split_rank(r) : nnf_rank_tiles{(r + 15) / 16, 0}; }
// X H^T.  Ranks 51, 52: three tiles + four leftover ranks next to the 4-row-tile body do not fit 256 registers (84 bytes of
// scratch, drains inside the chunk loop: 292 us against 238 us for the padded four tiles at 100000 x 2000,
// tools/probes/rank_step_probe.py)
constexpr nnf_rank_tiles nnf_xht_tiles(int r, bool vec) {
    const nnf_rank_tiles t = nnf_split_rank(r);
    return !vec ? nnf_rank_tiles{(r + 15) / 16, 0} : (t.MT == 3 && t.REM == 4) ? nnf_rank_tiles{4, 0} : t;
}
// X staged through LDS in 256-byte row pieces (k_xht_lds.hip) where the load path, not the MFMA rate, bounds the product
constexpr bool nnf_xht_use_lds(nnf_rank_tiles t, bool vec) { return vec && t.MT + (t.REM > 0) <= 2; }

// W^T X, workgroups per CU by rank tiles: up to four tiles three (<= 168 registers); five and six tiles (ranks 65 ... 98) `big_wg`
// (the build switch XTY_BIG_WG: two) -- the kernel fits 256 registers there without a spill where the compiler took up to 348 for
// one wave per SIMD.  Six tiles + four leftover ranks (rank 100) and seven / eight tiles stay at one: at 256 registers rank 100
// spills 4 and -- worse -- waits for a staging load inside the chunk loop (a full drain of the X prefetch ring per trip,
// tools/check_loop_drains.py), for 6.54 -> 6.34 ms at 10^6 x 4000 (tools/probes/xty_occ_probe.py): not taken.
constexpr int nnf_xty_wg_per_cu(int MT, int REM, int big_wg) {
    return MT + (REM > 0) <= 4 ? 3 : ((MT <= 6 && !(MT == 6 && REM == 4)) ? big_wg : 1);
}
// resident workgroups per CU of the direct X H^T kernel in its four- and three-tile forms
constexpr int nnf_xht_wg_per_cu(int MT, int REM) { return MT + (REM > 0) <= 4 ? 2 : 1; }
// W^T X: a workgroup sums its rows in fp32 (MFMA accumulators); the slabs are added in fp64.  Cap the rows per workgroup: at
// 1e6 x 4000 rank 100 the occupancy plan is 16 splits of 62500 rows, and an entry of U^T X came out with 9.5e-7 relative rms
// and a -2.2e-7 MEAN error (tools/probes/accum_error_probe.py) -- enough to take the Gram-identity cost of a HALS iteration
// (which multiplies the mean by ||X||^2) to its 5e-4 bound.  The mean falls with the SQUARE of the chain length (62500 ->
// 8192 rows: -2.2e-7 -> -3.7e-9, rms 9.5e-7 -> 1.2e-7), and at 8192 rows it was still what sent a 10^6 x 4000 rank-100 run
// back to the streaming cost kernel after ~20 iterations (tools/probes/identity_terms_probe.py: bias term 3.3e4 of a 5.9e4
// bound, actual error 1.4e4).  2048 rows: 489 slabs of 1.6 MB there (+10 % traffic on an MFMA-bound pass; fewer if the
// context workspace is smaller -- the Python engine creates its main context with 1 GiB).
constexpr int64_t NNF_XTY_ROWS_CAP = 2048;

// ---- the long axis cut into slabs (W^T X, the right MU update, the MTTKRP rows kernel) ----
struct nnf_split_plan {
    int status;                // NNF_OK, or the refusal
    int64_t nsplit, rows_per_split;
    const char* bound;         // which bound set the split count (NNF_PLAN_DEBUG)
    int64_t ws_max;            // slabs (per set) the free workspace holds
};
// rows x pitch floats under col_blocks column blocks: `resident` workgroups (per CU x CUs) shared among the column blocks, raised
// to rows / rows_cap (0: no cap), cut to rows / 64 and to what free_bytes hold of nsets sets of slabs of slab_bytes each; the
// rows per split in 64s, halved until (rows + 128) * pitch * 4 stays inside 32-bit offsets.
inline nnf_split_plan nnf_plan_split(int64_t rows, int64_t pitch, int64_t col_blocks, int64_t resident, int64_t rows_cap,
                                     int64_t slab_bytes, int nsets, size_t free_bytes, const char* min_rows = "min_rows") {
    nnf_split_plan p{NNF_OK, resident / col_blocks, 0, "occupancy", 0};
    if (p.nsplit < 1) p.nsplit = 1;
    if (rows_cap > 0 && p.nsplit < nnf_cdiv(rows, rows_cap)) { p.nsplit = nnf_cdiv(rows, rows_cap); p.bound = "rows_cap"; }
    if (p.nsplit > nnf_cdiv(rows, 64)) { p.nsplit = nnf_cdiv(rows, 64); p.bound = min_rows; }
    const int64_t free = (int64_t)free_bytes;
    p.ws_max = free / (slab_bytes * nsets);
    // (every further set starts on the cursor's 256-byte boundary, which a set of nsplit slabs need not end on)
    while (nsets > 1 && p.ws_max >= 1 && (nsets - 1) * nnf_rup(p.ws_max * slab_bytes, 256) + p.ws_max * slab_bytes > free) --p.ws_max;
    if (p.ws_max < 1) { p.status = NNF_ERR_WORKSPACE; return p; }
    if (p.nsplit > p.ws_max) { p.nsplit = p.ws_max; p.bound = "workspace"; }
    p.rows_per_split = nnf_rup(nnf_cdiv(rows, p.nsplit), 64);
    while ((p.rows_per_split + 128) * pitch * 4 >= NNF_OFFSET32_END) {
        if (p.rows_per_split <= 64) { p.status = NNF_ERR_UNSUPPORTED; return p; }
        p.rows_per_split = nnf_rup(p.rows_per_split / 2, 64);
        p.bound = "offset32";
    }
    p.nsplit = nnf_cdiv(rows, p.rows_per_split);
    if (p.nsplit > p.ws_max) p.status = NNF_ERR_WORKSPACE;
    return p;
}
// workgroups of a split kernel: the splits in eights (nnf_xcd_map) x the column blocks
constexpr int nnf_split_grid(int64_t nsplit, int col_blocks) { return 8 * (int)nnf_cdiv(nsplit, 8) * col_blocks; }

inline nnf_split_plan nnf_plan_xty(int cus, int64_t m, int64_t n, int64_t ldx, int r, nnf_rank_tiles t, int big_wg, size_t free_bytes) {
    return nnf_plan_split(m, ldx, nnf_cdiv(n, 256), nnf_xty_wg_per_cu(t.MT, t.REM, big_wg) * (int64_t)cus, NNF_XTY_ROWS_CAP,
                          (int64_t)r * nnf_rup(n, 4) * 4, 1, free_bytes);
}
inline void nnf_report_xty(FILE* f, int64_t m, int64_t n, int r, nnf_rank_tiles t, bool vec, const nnf_split_plan& p,
                           const char* more = "") {
    fprintf(f, "[nnf plan] xty m=%lld n=%lld r=%d mt=%d rem=%d vec=%d nsplit=%lld rows_per_split=%lld bound=%s grid=%d%s\n",
            (long long)m, (long long)n, r, t.MT, t.REM, (int)vec, (long long)p.nsplit, (long long)p.rows_per_split, p.bound,
            nnf_split_grid(p.nsplit, (int)nnf_cdiv(n, 256)), more);
}

// MTTKRP rows kernel: the tensor as an m x n matrix (no padding), two workgroups per CU, no rows cap
inline nnf_split_plan nnf_plan_rows(int cus, int64_t m, int64_t n, int r, size_t free_bytes) {
    return nnf_plan_split(m, n, nnf_cdiv(n, 256), 2 * (int64_t)cus, 0, (int64_t)r * nnf_rup(n, 4) * 4, 1, free_bytes, "rows");
}
// buffer-addressed Khatri-Rao generation: 31-bit byte offsets into both factors, at most one wrap inside four rows
// (padded rank rows: their offsets must not wrap either)
constexpr bool nnf_rows_kr_fast(int64_t nb, int MT, int64_t lda, int64_t ldb) {
    return nb >= 4 && (int64_t)(16 * MT) * lda * 4 < NNF_OFFSET32_END && (int64_t)(16 * MT) * ldb * 4 < NNF_OFFSET32_END;
}
inline void nnf_report_rows(FILE* f, int64_t m, int64_t n, int64_t nb, int r, int MT, bool vec, bool kr_fast,
                            const nnf_split_plan& p, const char* more = "") {
    fprintf(f, "[nnf plan] mttkrp_rows m=%lld n=%lld nb=%lld r=%d mt=%d VEC=%d krf=%d krdiv=%s nsplit=%lld rps=%lld bound=%s%s\n",
            (long long)m, (long long)n, (long long)nb, r, MT, (int)vec, (int)kr_fast, !kr_fast ? "slow" : nb >= 64 ? "carry" : "redivide",
            (long long)p.nsplit, (long long)p.rows_per_split, p.bound, more);
}

// ---- X H^T: rows of X over workgroups ----
// A workgroup is four waves of `nth` 16-row tiles each; the first n_hi workgroups take nth tiles per wave, the others nth - 1.
struct nnf_xht_plan {
    const char* form;
    int nth;
    int64_t n_hi, grid;
    int tail_parts, tail_tiles, tail_cpp;   // the k-split tail (all 0: none)
    int64_t tail_row0, tail_ld;
    bool covers(int64_t m) const { return n_hi * 64 * nth + (grid - n_hi) * 64 * (nth - 1) + 16 * (int64_t)tail_tiles >= m; }
};
// `slots` resident workgroups, `tiles` rank tiles (leftover ranks count as one).  nt2 / tail_on: NNF_XHT_NT2 (-1: unset) and
// NNF_XHT_TAIL; narrow: the LDS-staged kernel's 32-row waves.  free_bytes: what the tail's slabs may take.
inline nnf_xht_plan nnf_plan_xht(int64_t m, int64_t n, int r, int64_t slots, int tiles, int nt2, int tail_on, size_t free_bytes,
                                 bool narrow = false) {
    const int64_t T = nnf_cdiv(m, 16), waves = 4 * slots;
    nnf_xht_plan p{"small", 3, 0, nnf_cdiv(m, 128), 0, 0, 0, 0, 0};   // small: 128-row workgroups
    // six and more rank tiles (ranks 96 ... 128), many rounds: TWO row tiles per wave keep a wave at 248 registers, so that two
    // workgroups share a CU -- the four-tile form needs 404 (256 + 148 accumulation registers) and runs one wave per SIMD.
    // Measured (tools/probes/xht_nt2_probe.py, four -> two tiles): rank 100, 10^6 x 4000 7.16 -> 6.56 ms (0.71 -> 0.775 of the MFMA
    // peak), 500000 rows 3.58 -> 3.47, 250000 1.79 -> 1.73; rank 96 x 600000 2.17 -> 2.05; ranks 112 / 128 x 10^6 -4 % / -2 %;
    // below ~230000 rows (125000: 0.97 -> 1.00) and at five rank tiles (rank 80: 2.75 -> 2.79) the four-tile form stays ahead.
    // NNF_XHT_NT2=0 / 1 forces either form (A/B on one box).
    const bool two_tiles = tiles > 4 && T > 4 * waves && (nt2 >= 0 ? nt2 != 0 : (tiles >= 6 && T > 14 * waves));
    if (narrow || two_tiles) {
        p.form = narrow ? "shared_lines" : "two_tiles";
        p.nth = 2;
        p.n_hi = p.grid = nnf_cdiv(m, 128);
    } else if (T > 4 * waves) {     // several rounds: 256-row workgroups
        p.form = "rounds";
        p.nth = 4;
        p.n_hi = p.grid = nnf_cdiv(m, 256);
    } else if (T > 2 * waves) {     // one round: (4,3) or (3,2) tiles per wave
        p.nth = T > 3 * waves ? 4 : 3;
        p.form = p.nth == 4 ? "round43" : "round32";
        const int64_t extra = T - 4 * (p.nth - 1) * slots, nchunk_all = nnf_cdiv(n, 64);
        p.n_hi = nnf_cdiv(extra, 4);
        p.grid = slots;
        // few tiles beyond a whole round of nth - 1 per wave (config B: 106 beyond 6144): every workgroup stays at nth - 1 and the
        // extra tiles are contracted in k-split shares by all of them -- 6 + 2 % on every SIMD instead of 7 tiles on the busiest.
        // (Not for ranks <= 32: the LDS-staged form is bit for bit the unsplit kernel there, tests.  NNF_XHT_TAIL=0 switches it off.)
        if (tail_on && tiles >= 3 && extra > 0 && nchunk_all >= 4) {
            int parts = 32;
            while (parts > 1 && (parts > nchunk_all || 4 * (slots / parts) < extra)) parts >>= 1;
            const int64_t row0 = 64 * (int64_t)(p.nth - 1) * slots, ld = nnf_rup(m - row0, 4);
            // (slabs that do not fit the workspace: the (nth, nth - 1) mix above)
            if (parts >= 4 && 4 * (slots / parts) >= extra && 8 * extra <= T && (size_t)parts * r * ld * 4 <= free_bytes) {
                p.n_hi = 0;
                p.tail_parts = parts;
                p.tail_tiles = (int)extra;
                p.tail_cpp = (int)nnf_cdiv(nchunk_all, parts);
                p.tail_row0 = row0;
                p.tail_ld = ld;
            }
        }
    }
    return p;
}
// a workgroup's 64 rows of X and a factor chunk inside 32-bit offsets (else both kernels refuse)
constexpr bool nnf_xht_offsets_ok(int64_t n, int64_t ldx) { return 64 * ldx * 4 + 4 * (n + 128) < NNF_OFFSET32_END; }
// the register-fragment kernel (nnf_xht_kernel)
inline nnf_xht_plan nnf_plan_xht_direct(int cus, int64_t m, int64_t n, int r, nnf_rank_tiles t, int nt2, int tail_on, size_t free_bytes) {
    return nnf_plan_xht(m, n, r, (int64_t)nnf_xht_wg_per_cu(t.MT, t.REM) * cus, t.MT + (t.REM > 0), nt2, tail_on, free_bytes);
}
// lds: the LDS-staged kernel (its tiling is reported as such; always 16-byte loads, never a tail)
inline void nnf_report_xht(FILE* f, int64_t m, int64_t n, int r, nnf_rank_tiles t, bool vec, bool lds, const nnf_xht_plan& p,
                           const char* more = "") {
    fprintf(f, "[nnf plan] xht m=%lld n=%lld r=%d mt=%d rem=%d vec=%d form=%s%s nth=%d n_hi=%lld grid=%lld tail_parts=%d "
               "tail_tiles=%d tail_cpp=%d%s\n", (long long)m, (long long)n, r, t.MT, t.REM, (int)vec, lds ? "lds tiling=" : "", p.form,
            p.nth, (long long)p.n_hi, (long long)p.grid, p.tail_parts, p.tail_tiles, p.tail_cpp, more);
}
// the LDS-staged kernel's wave height.  A row pitch that is not a whole number of 128-byte lines leaves every 256-byte piece
// sharing its first and last line with the neighbouring chunks' pieces of the same row: the wave comes back for them one chunk
// later, after everything the XCD's 64 resident workgroups fetched in between -- 4 MB with 64-row waves, the size of the L2
// (250000 x 500: 660 MB fetched for 500 MB, 127 us).  32-row waves (48 KB of LDS: three workgroups per CU) halve that distance:
// 559 MB, 120 us.  Aligned pitches have no shared lines and keep the 64-row waves (100000 x 2000 rank 32: 157 us against 175).
// (rows start on a line every 128 / gcd(pitch mod 128, 128) rows: the narrow form from every fourth row on -- with every
//  second row aligned, 100000 x 2000, the 64-row waves stay ahead, 159 us against 190).  pin: NNF_XHT_NT (0: unset, 2: narrow)
inline bool nnf_xht_lds_narrow(int64_t ldx, int pin) {
    int64_t off = (ldx * 4) % 128, gcd = 128;
    while (off) { const int64_t t = gcd % off; gcd = off; off = t; }
    return pin ? pin == 2 : (128 / gcd >= 4);
}
// the LDS-staged kernel (nnf_xht_lds_kernel): the same row tiling at two resident workgroups per CU, without the two-tile form and
// the tail
inline nnf_xht_plan nnf_plan_xht_lds(int cus, int64_t m, int64_t n, int r, nnf_rank_tiles t, int64_t ldx, int pin) {
    return nnf_plan_xht(m, n, r, (int64_t)2 * cus, t.MT + (t.REM > 0), 0, 0, 0, nnf_xht_lds_narrow(ldx, pin));
}

// ---- MTTKRP modes 0 and 1: the segments of a row cut into splits (launch_seg) ----
struct nnf_seg_plan {
    int status;                // NNF_OK, or the refusal
    int64_t nsplit, sps;       // splits, segments per split
    const char* bound;
    int64_t ws_max;            // slabs the free workspace holds
};
// nrows rows of nseg segments of klen entries (row pitch ldrow), the segment-side factor at pitch fs_ld: a wave's 64 rows and the
// padded rank rows of that factor inside 31-bit offsets; two workgroups per CU shared among the 256-row blocks, at least one
// split, at most one per segment and what free_bytes hold of slabs (r x rup(nrows, 4) floats), then segments per split re-rounded
inline nnf_seg_plan nnf_plan_seg(int cus, int64_t nrows, int64_t ldrow, int64_t nseg, int64_t klen, int r, int64_t fs_ld,
                                 size_t free_bytes) {
    nnf_seg_plan p{NNF_OK, 2 * (int64_t)cus / nnf_cdiv(nrows, 256), 0, "occupancy", 0};
    if ((64 * ldrow + klen + 256) * 4 >= NNF_OFFSET32_END || (int64_t)(16 * ((r + 15) / 16)) * fs_ld * 4 >= NNF_OFFSET32_END) {
        p.status = NNF_ERR_UNSUPPORTED;
        return p;
    }
    if (p.nsplit < 1) { p.nsplit = 1; p.bound = "one"; }
    if (p.nsplit > nseg) { p.nsplit = nseg; p.bound = "segments"; }
    p.ws_max = (int64_t)(free_bytes / 4) / ((int64_t)r * nnf_rup(nrows, 4));
    if (p.ws_max < 1) { p.status = NNF_ERR_WORKSPACE; return p; }
    if (p.nsplit > p.ws_max) { p.nsplit = p.ws_max; p.bound = "workspace"; }
    p.sps = nnf_cdiv(nseg, p.nsplit);
    p.nsplit = nnf_cdiv(nseg, p.sps);
    return p;
}
// vec / fkvec: 16-byte loads of the tensor / of the inner factor; pp: the two-register-set pipeline (up to two rank tiles)
inline void nnf_report_seg(FILE* f, int64_t nrows, int64_t nseg, int64_t klen, int r, int MT, bool vec, bool fkvec, bool pp,
                           const nnf_seg_plan& p, const char* more = "") {
    fprintf(f, "[nnf plan] mttkrp_seg nrows=%lld nseg=%lld klen=%lld r=%d mt=%d VEC=%d fkvec=%d pp=%d nsplit=%lld sps=%lld bound=%s%s\n",
            (long long)nrows, (long long)nseg, (long long)klen, r, MT, (int)vec, (int)fkvec, (int)pp, (long long)p.nsplit,
            (long long)p.sps, p.bound, more);
}

// ---- MTTKRP from a partial product Y (r x A x B): nnf_mttkrp3_from_partial_f32 ----
// axis 2: one wave per (r, a) row, four to a workgroup, at most 8192 workgroups (beyond that the waves stride the rows)
struct nnf_partial_last_plan { int64_t grid; bool strided; };
inline nnf_partial_last_plan nnf_plan_partial_last(int64_t A, int r) {
    const int64_t rows = (int64_t)r * A, grid = nnf_cdiv(rows, 4) < 8192 ? nnf_cdiv(rows, 4) : 8192;
    return {grid, rows > 4 * grid};
}
inline void nnf_report_partial_last(FILE* f, int64_t A, int64_t B, int r, const nnf_partial_last_plan& p, const char* more = "") {
    fprintf(f, "[nnf plan] partial_last A=%lld B=%lld r=%d grid=%lld strided=%d%s\n", (long long)A, (long long)B, r,
            (long long)p.grid, (int)p.strided, more);
}
// axis 1: enough a-chunks to fill the chip (four workgroups per CU over column blocks x ranks), at least 16 rows each; one slab
// (r x rup(B, 4) floats) per chunk
struct nnf_partial_mid_plan {
    int status;
    int64_t nchunk, a_per;
    const char* bound;
};
inline nnf_partial_mid_plan nnf_plan_partial_mid(int cus, int64_t A, int64_t B, int r, size_t free_bytes) {
    const int64_t cb = nnf_cdiv(B, 256);
    nnf_partial_mid_plan p{NNF_OK, nnf_cdiv((int64_t)4 * cus, cb * r), 0, "occupancy"};
    if (p.nchunk < 1) p.nchunk = 1;
    if (p.nchunk > nnf_cdiv(A, 16)) { p.nchunk = nnf_cdiv(A, 16); p.bound = "rows16"; }
    if (p.nchunk > 65535) { p.nchunk = 65535; p.bound = "grid"; }
    p.a_per = nnf_cdiv(A, p.nchunk);
    p.nchunk = nnf_cdiv(A, p.a_per);
    if ((size_t)p.nchunk * r * nnf_rup(B, 4) * 4 > free_bytes) p.status = NNF_ERR_WORKSPACE;
    else if (cb > 65535) p.status = NNF_ERR_UNSUPPORTED;   // (grid.x)
    return p;
}
inline void nnf_report_partial_mid(FILE* f, int64_t A, int64_t B, int r, const nnf_partial_mid_plan& p, const char* more = "") {
    fprintf(f, "[nnf plan] partial_mid A=%lld B=%lld r=%d nchunk=%lld a_per=%lld bound=%s%s\n", (long long)A, (long long)B, r,
            (long long)p.nchunk, (long long)p.a_per, p.bound, more);
}

// ---- the Gram A A^T of an r x K factor (launch_gram, launch_gram_blocks) ----
enum nnf_gram_form { NNF_GRAM_SMALL, NNF_GRAM_SINGLE, NNF_GRAM_SLABS, NNF_GRAM_BLOCKS };
struct nnf_gram_plan {
    int status;
    nnf_gram_form form;
    int64_t nsplit, kps;       // splits of K (one slab of r x r floats each, but for small and single), columns per split
    const char* bound;
    int64_t ws_max;            // slabs the free workspace holds
};
// small: one 512-thread workgroup, straight into G (at most four rank tiles, K <= 1024 in whole float4s, a contiguous G and
// 16-byte loads of A: vec).  Otherwise splits of K.  Up to NNF_MAX_RANK: one split per two resident workgroups per CU (the slab
// reduction spreads every output element over up to 16 threads, so its cost grows slowly with the split count: 64 splits left a
// 50 x 100000 Gram at 22 us and a 100 x 125000 one at 127 us; a workgroup walks its split in 64-wide LDS-staged chunks, one
// memory round trip each: with one split per CU the Gram of a 50 x 100000 factor was 7 dependent round trips = 15.7 us in front
// of W^T X; two resident workgroups per CU halve the chain and overlap each other's waits); short factors (the I_mode x R factors
// of NTF / NTD, K <= 1024) with a contiguous G: one workgroup, no split, written straight into G -- the whole Gram is a few
// microseconds of work and the slab reduction would be a second launch of the same length (single).  The fp32 chain inside a
// split stays short (<= 512 columns): what the chains leave is all the error the fp64 copy of the sums has (nnf_gram_f64_f32);
// the same plan with and without the copy.  A workspace without room for one slab is refused there rather than run as one chain
// over all of K.  (Only there: with fewer splits asked for than the workspace holds nothing is capped, and the launcher's carve
// is what refuses.)  Ranks above NNF_MAX_RANK (blocks: 64 x 64 blocks of G, a workgroup per split and block pair): about two
// workgroups per CU over all block pairs, 64-column chunks, chains of 512, as many slabs as the workspace holds.
inline nnf_gram_plan nnf_plan_gram(int cus, int r, int64_t K, bool ldg_is_r, bool vec, size_t free_bytes) {
    const int64_t max_split = nnf_cdiv(K, 64), chain = nnf_cdiv(K, 512);
    nnf_gram_plan p{NNF_OK, NNF_GRAM_SMALL, 1, K, "none", (int64_t)(free_bytes / 4) / ((int64_t)r * r)};
    if (r > NNF_MAX_RANK) {
        const int64_t nb = (r + 63) / 64;
        p.form = NNF_GRAM_BLOCKS;
        p.nsplit = nnf_cdiv((int64_t)2 * cus, nb * nb);
        p.bound = "occupancy";
        if (p.nsplit > max_split) { p.nsplit = max_split; p.bound = "min_cols"; }
        if (p.ws_max < 1) { p.status = NNF_ERR_WORKSPACE; return p; }
        if (p.nsplit < chain) { p.nsplit = chain; p.bound = "chain512"; }
        if (p.nsplit > p.ws_max) { p.nsplit = p.ws_max; p.bound = "workspace"; }
        if (p.nsplit < 1) p.nsplit = 1;
    } else {
        if ((r + 15) / 16 <= 4 && K <= 1024 && (K & 3) == 0 && ldg_is_r && vec) return p;
        p.nsplit = cus > 8 ? 2 * (int64_t)cus : 8;
        p.bound = "occupancy";
        if (p.nsplit > max_split) { p.nsplit = max_split; p.bound = "min_cols"; }
        if (p.nsplit < 1) p.nsplit = 1;
        if (K <= 1024 && ldg_is_r) { p.nsplit = 1; p.bound = "short"; }
        if (p.nsplit > 1 && p.nsplit < chain) {
            p.nsplit = chain;
            p.bound = "chain512";
            if (p.ws_max < 1) { p.status = NNF_ERR_WORKSPACE; return p; }
            if (p.nsplit > p.ws_max) { p.nsplit = p.ws_max; p.bound = "workspace"; }
        }
    }
    p.kps = nnf_rup(nnf_cdiv(K, p.nsplit), 64);
    p.nsplit = nnf_cdiv(K, p.kps);
    if (p.form != NNF_GRAM_BLOCKS) p.form = p.nsplit == 1 && ldg_is_r ? NNF_GRAM_SINGLE : NNF_GRAM_SLABS;
    return p;
}
inline void nnf_report_gram(FILE* f, int r, int64_t K, const nnf_gram_plan& p, const char* more = "") {
    static const char* const forms[] = {"small", "single", "slabs", "blocks"};
    fprintf(f, "[nnf plan] gram r=%d K=%lld form=%s nsplit=%lld kps=%lld bound=%s%s\n", r, (long long)K, forms[p.form],
            (long long)p.nsplit, (long long)p.kps, p.bound, more);
}

// ---- a cross product with the Gram of its factor riding in the same launch (nnf_xty_gram_f32, nnf_xht_gram_f32) ----
// The cross product keeps its own plan and its first main_grid workgroups; the Gram keeps the plan a call of its own takes
// (`g`, made against the same free workspace) and rides as workgroups [rider_offset, rider_offset + rider_grid), one per split.
// Both carves come from one cursor: the cross product's slabs first (main_bytes, 0: none), the Gram's behind them on the
// cursor's 256-byte boundary.  Only the slab form rides (small / single write G without slabs, blocks has a grid of its own), and
// only where both carves fit and the Gram stages `tiles` rank tiles, the LDS image of the cross product: otherwise rides = false
// and the two run as the launches of their own, which gives the same bits.
struct nnf_rider_plan {
    bool rides;
    int64_t main_grid, rider_grid, rider_offset, grid;
    size_t main_bytes, rider_bytes, rider_ws_off, ws_bytes;
};
inline nnf_rider_plan nnf_plan_rider(int64_t main_grid, size_t main_bytes, const nnf_gram_plan& g, int r, int tiles,
                                     size_t free_bytes) {
    nnf_rider_plan p{false, main_grid, 0, main_grid, main_grid, main_bytes, 0, 0, main_bytes};
    if (g.status != NNF_OK || g.form != NNF_GRAM_SLABS || (r + 15) / 16 != tiles) return p;
    nnf_ws_cursor cur(nullptr, free_bytes);
    const size_t rider_bytes = (size_t)g.nsplit * r * r * 4;
    if ((main_bytes > 0 && !cur.reserve(main_bytes)) || !cur.reserve(rider_bytes)) return p;
    p.rides = true;
    p.rider_grid = g.nsplit;
    p.grid = main_grid + g.nsplit;
    p.rider_bytes = rider_bytes;
    p.rider_ws_off = cur.off - rider_bytes;
    p.ws_bytes = cur.off;
    return p;
}
inline void nnf_report_rider(FILE* f, const char* what, const nnf_rider_plan& p, const char* more = "") {
    fprintf(f, "[nnf plan] %s rides=%d main_grid=%lld rider_grid=%lld rider_offset=%lld grid=%lld main_bytes=%zu rider_bytes=%zu "
               "rider_ws_off=%zu ws_bytes=%zu%s\n", what, (int)p.rides, (long long)p.main_grid, (long long)p.rider_grid,
            (long long)p.rider_offset, (long long)p.grid, p.main_bytes, p.rider_bytes, p.rider_ws_off, p.ws_bytes, more);
}

// ---- the fixed-order slab reduction behind every split launch (k_reduce.hip) ----
// One set of slabs, where its sums go and the form the reduction takes for it: lg > 0: 2^lg threads per element ("par2" ..
// "par16"); else vec4: four columns per thread; else one element per thread ("plain").  blocks: its workgroups; block0: where
// they start in a launch shared with other sets (nnf_launch_reduce_sets fills it in).
#define NNF_REDUCE_MAX_SETS 3
struct nnf_reduce_set {
    const float* slabs;
    float* out;
    double* out64;
    int64_t slab_stride, cols, lds, ldo;
    int nslab, rows;
    int lg, vec4, blocks, block0;
};
// the form and the workgroups a set takes (the same for a launch of its own and for a share of a fused one); the slab pointer
// is read for its 16-byte alignment only.  The order of the sums each form keeps is restated in tests/reduce_restatement.py.
// (The 4096-workgroup cap of the parts forms never binds: rows * cols < 2^(20 - lg) elements at 2^(8 - lg) per workgroup are at
// most 4096 workgroups, so a workgroup of those forms walks its loop once -- tests/test_reduce_plan.py holds that as a property.)
inline nnf_reduce_set nnf_plan_reduce_set(const float* slabs, int nslab, int64_t slab_stride, int rows, int64_t cols, int64_t lds,
                                          float* out, int64_t ldo, double* out64 = nullptr) {
    nnf_reduce_set q{slabs, out, out64, slab_stride, cols, lds, ldo, nslab, rows, 0, 0, 0, 0};
    const int64_t total = (int64_t)rows * cols;
    // enough threads to fill the chip: 2^lg parts per element when the output is small
    while (q.lg < 4 && (total << q.lg) < ((int64_t)1 << 19) && (2 << q.lg) <= nslab) ++q.lg;
    if (q.lg > 0) {
        const int64_t grid = nnf_cdiv(total, 256 >> q.lg);
        q.blocks = grid > 4096 ? 4096 : (int)grid;
        return q;
    }
    // (four columns per thread only when that still leaves enough threads to fill the chip: 20 vs 16 us at r x n = 1e5)
    if (out64 == nullptr && (lds & 3) == 0 && (slab_stride & 3) == 0 && (((uintptr_t)slabs) & 15) == 0 && total >= ((int64_t)1 << 21)) {
        const int64_t total4 = (int64_t)rows * ((cols + 3) >> 2);
        const int64_t grid4 = (total4 + 255) / 256;
        q.vec4 = 1;
        q.blocks = grid4 > 2048 ? 2048 : (int)grid4;
        return q;
    }
    const int64_t grid = (total + 255) / 256;
    q.blocks = grid > 2048 ? 2048 : grid < 1 ? 1 : (int)grid;
    return q;
}
constexpr const char* nnf_reduce_form_name(int lg, int vec4) {
    return lg == 1 ? "par2" : lg == 2 ? "par4" : lg == 3 ? "par8" : lg >= 4 ? "par16" : vec4 ? "vec4" : "plain";
}
// NNF_REDUCE_DEBUG: one line per set of every reduction launch (set `set` of `nsets`, counted from 0).  A tag of its own:
// the "[nnf plan]" lines of a call are counted by the tests that key on them.
inline void nnf_report_reduce(FILE* f, const nnf_reduce_set& q, int set, int nsets, const char* more = "") {
    fprintf(f, "[nnf reduce] rows=%d cols=%lld nslab=%d lds=%lld ldo=%lld out64=%d form=%s blocks=%d set=%d/%d block0=%d%s\n", q.rows,
            (long long)q.cols, q.nslab, (long long)q.lds, (long long)q.ldo, (int)(q.out64 != nullptr), nnf_reduce_form_name(q.lg, q.vec4),
            q.blocks, set, nsets, q.block0, more);
}

// ---- the cost / ratio pass (launch_cost): 128-row workgroups x column splits ----
// 32 rows of X (or of the model buffer of a rank above 128) at pitch ld and a factor chunk inside 32-bit offsets
constexpr bool nnf_cost_offsets_ok(int64_t ld, int64_t n) { return 32 * ld * 4 + 4 * (n + 128) < NNF_OFFSET32_END; }
struct nnf_cost_plan {
    int status;
    int grid, csplit;          // row tiles, column splits
    int KS, NN, vdb;           // k-steps of 4 rank rows, rank rows per load group, two V buffers
    size_t shm;                // dynamic LDS
    size_t partial_bytes, vf_bytes;   // the two carves: a double per workgroup, the staged right operand
};
// kr: Khatri-Rao rows on the left (the CP cost); forced: NNF_COST_CSPLIT (0: unset); pin: a later rank chunk of a rank above
// 128, which reads the model so far; prod: the pass only writes the model (NNF_PROD)
inline nnf_cost_plan nnf_plan_cost(int cus, int64_t m, int64_t n, int r, bool kr, int forced, bool pin, bool prod,
                                   size_t free_bytes) {
    nnf_cost_plan p{NNF_OK, (int)nnf_cdiv(m, 128), 0, (r + 3) / 4, 0, 0, 0, 0, 0};
    // column splits: aim at ~8 workgroups per resident slot, keep at least 4 column blocks per workgroup
    const int nblk_all = (int)nnf_cdiv(n, 64);
    p.csplit = (int)nnf_cdiv((int64_t)8 * 2 * cus, p.grid);
    if (p.csplit > nblk_all / 4) p.csplit = nblk_all / 4;
    // every column split stages the workgroup's 128 x r tile of U again: keep that re-read below ~5 % of the pass over X
    // (config B: 6 splits moved 1.02 GB for 0.82 GB algorithmic, PMC; the launch time is flat over 2..8 splits, so the
    // splits buy nothing there) -- as long as the grid still fills the resident slots twice over
    int cap = (int)((0.05 * (double)n) / (double)(r > 0 ? r : 1));
    if (cap < 1) cap = 1;
    const int need = (int)nnf_cdiv((int64_t)2 * 3 * cus, p.grid);   // two rounds of 3 workgroups per CU
    if (cap < need) cap = need;
    if (!kr && p.csplit > cap) p.csplit = cap;
    if (forced > 0) p.csplit = forced < nblk_all ? forced : nblk_all;
    if (p.csplit < 1) p.csplit = 1;
    p.NN = (pin || prod || p.KS > 16) ? 8 : 4;
    // two V buffers unless dropping one lets another workgroup onto the CU (ranks 53..64: a third, 77..104: a second; see the kernel)
    const size_t shm2 = (size_t)4 * 2 * p.KS * 64 * 4 + (size_t)2 * p.KS * 64 * 16 + 64, shm1 = shm2 - (size_t)p.KS * 64 * 16;
    const size_t lds_cu = 160 * 1024;
    auto wg_per_cu = [&](size_t b) { const size_t w = lds_cu / b; return w > 3 ? (size_t)3 : w; };   // (launch bound: 3)
    p.vdb = wg_per_cu(shm1) > wg_per_cu(shm2) ? 0 : 1;
    p.shm = p.vdb ? shm2 : shm1;
    p.partial_bytes = (size_t)p.grid * p.csplit * 8;
    p.vf_bytes = (size_t)nblk_all * p.KS * 64 * 16;
    nnf_ws_cursor cur(nullptr, free_bytes);
    if (!cur.reserve(p.partial_bytes) || !cur.reserve(p.vf_bytes)) p.status = NNF_ERR_WORKSPACE;
    return p;
}
// op: the pass (frob, kl, is, gen, ratio_kl, ratio_gen, prod); vec: 16-byte loads of X (and of the model buffer); kr: the
// Khatri-Rao inner length (0: none)
inline void nnf_report_cost(FILE* f, int64_t m, int64_t n, int r, const char* op, bool vec, bool pin, int64_t kr,
                            const nnf_cost_plan& p, const char* more = "") {
    fprintf(f, "[nnf plan] cost m=%lld n=%lld r=%d op=%s grid=%d csplit=%d NN=%d vdb=%d VEC=%d pin=%d kr=%lld%s\n", (long long)m,
            (long long)n, r, op, p.grid, p.csplit, p.NN, p.vdb, (int)vec, (int)pin, (long long)kr, more);
}

// Residency arithmetic and launch plans of the fused MU kernels that the kernels (k_mu_kernels.h), their launchers (k_mu.hip) and
// tools/nnf_plan.cpp share.  No HIP in here: the tool is a plain host program.
#pragma once
#include "k_stream_plan.h"

enum { BM_KL = 1, BM_FROB = 2, BM_KLC = 3, BM_GEN = 9, BM_WGEN = 10 };   // BM_KLC: the KL update + the KL divergence of its INPUT factors   // BM_FROB: R = X (plain X V^T) + the squared residual, see nnf_cp3_partial_cost_f32
// BM_WGEN: per-entry weights next to X, any beta (k_mu.hip, "weighted forms"): numerator AND denominator accumulators like BM_GEN
constexpr const char* mu_bm_name(int BM) {
    return BM == BM_KL ? "KL" : BM == BM_KLC ? "KLC" : BM == BM_FROB ? "FROB" : BM == BM_WGEN ? "WGEN" : "GEN";
}
// the forms that carry a denominator accumulator next to the numerator's: they share every residency figure and launch plan
constexpr bool mu_two_acc(int BM) { return BM == BM_GEN || BM == BM_WGEN; }

// Where the loop-invariant ("resident") factor fragments of MFMA #1 live: in registers for the KL forms, and for every form
// above rank 64 (MT > 4 rank tiles, where the chunk images alone take 16 KiB of LDS per tile); otherwise (general beta,
// r <= 64) in LDS.
constexpr bool mu_frags_in_regs(int MT, bool general_beta) { return !general_beta || MT > 4; }

// dynamic LDS of one workgroup: two double-buffered chunk images (+ the resident fragments unless in registers)
constexpr size_t mu_shm(int MT, int REM, int r, bool regf) {
    return ((regf ? 0 : (size_t)4 * ((r + 3) / 4) * 64) + (size_t)2 * (2 * MT + (REM > 0 ? 1 : 0)) * 256) * 16;
}

// resident workgroups per CU of the left kernel: three for the small Frobenius forms (<= 168 VGPRs), one for general beta
// and for ranks above 80 (MT > 5: 16 KiB of chunk images per rank tile)
constexpr int mu_left_wgpc(int MT, int REM, int BM) {
    return mu_two_acc(BM) || MT > 5 ? 1 : ((MT + (REM > 0) <= 2 && REM <= 2 && BM == BM_FROB) ? 3 : 2);
}
// above rank 64 the left kernel has its 128-row form only for general beta (numerator + denominator + fragments in registers)
// and at MT = 5 (there that form stays within 256 registers and 80 KiB of LDS: two workgroups share a CU, which measured
// faster than the better balanced mix of 192- and 128-row workgroups at one per CU: 719 against 792 us at 100000 x 2000, r = 65)
constexpr bool mu_left_rows128(int MT, int BM) { return MT > 4 && (mu_two_acc(BM) || MT == 5); }
// 16-column tiles per wave of the right kernel: 256 columns per workgroup, 128 at MT > 4 (k_mu_kernels.h)
constexpr int mu_right_nc(int MT) { return MT > 4 ? 2 : 4; }
// resident 4-wave workgroups per CU the right update's split count aims at
constexpr int mu_right_wgpc(int MT, int BM) { return BM == BM_KL && MT <= 4 ? 2 : 1; }

// leftover ranks handled on the VALU pipe: up to 4 next to one MFMA tile (ranks 17..20), up to 2 next to two or three (33, 34,
// 49, 50) -- four leftover ranks at two tiles left scratch reloads inside the right kernel's chunk loop, at three tiles hipcc
// spilled hundreds of registers (256 per wave at two workgroups per CU)
constexpr int mu_rem_of(int q, int rem) { return rem <= 2 ? 2 : (q == 1 && rem <= 4 ? 4 : 0); }
// Rank split of the fused kernels up to rank 64: MT full 16-rank tiles on MFMA, plus -- for 16q+1 .. 16q+4 ranks, aligned X, not
// the general-beta form -- the leftover ranks on the VALU pipe (REM = 2 or 4) instead of a padded tile.
constexpr nnf_rank_tiles mu_split_rank(int r, bool rem_ok) {
    const int q = r / 16, rem = r % 16;
    return (rem_ok && q >= 1 && q <= 3 && rem >= 1 && mu_rem_of(q, rem) > 0) ? nnf_rank_tiles{q, mu_rem_of(q, rem)}
                                                                              : nnf_rank_tiles{(r + 15) / 16, 0};
}
// ranks 97 .. 100 (config E's rank), left KL update, aligned X: six tiles on MFMA and the four leftover ranks on the VALU pipe
// instead of a padded seventh tile -- 6.25 tiles' worth of work instead of 6.5 + 7 in the two MFMAs
constexpr bool mu_left_kl_six_and_four(int r, bool vec) { return r > 96 && r <= 100 && vec; }
// the split an update takes (ranks 65 .. 128: whole tiles but for the form above)
constexpr nnf_rank_tiles mu_tiles_of(bool left, int r, bool kl, bool vec) {
    return r <= 64 ? mu_split_rank(r, kl && vec)
                   : (left && kl && mu_left_kl_six_and_four(r, vec)) ? nnf_rank_tiles{6, 4} : nnf_rank_tiles{(r + 15) / 16, 0};
}

// pieces a row of K entries is summed in (nnf_launch_rowsum): 1 = one workgroup per row, no scratch
constexpr int nnf_rowsum_pieces(int64_t K) { return K / 8192 > 64 ? 64 : K / 8192 > 1 ? (int)(K / 8192) : 1; }

// ---- right update ----
struct mu_right_plan {
    nnf_split_plan split;   // over the rows of X (status: NNF_OK, or the refusal)
    int ncb;                // column blocks
    int pieces;             // of the row sums of Ut (KL; else 0)
};
// `cur`: a copy of the caller's cursor -- the update takes r doubles, the row sums' partials, then one (KL) or two sets of slabs
inline mu_right_plan mu_plan_right(nnf_ws_cursor cur, int cus, int64_t m, int64_t n, int64_t ldx, int64_t ldu, int r, int MT, int BM) {
    mu_right_plan p{{NNF_ERR_UNSUPPORTED, 0, 0, "", 0}, (int)nnf_cdiv(n, 64 * mu_right_nc(MT)), BM == BM_KL ? nnf_rowsum_pieces(m) : 0};
    if ((int64_t)(16 * (MT + 1)) * ldu * 4 + 4 * (m + 128) >= NNF_OFFSET32_END) return p;   // 32-bit image offsets
    p.split.status = NNF_ERR_WORKSPACE;
    if (!cur.reserve((size_t)r * 8) || (p.pieces > 1 && !cur.reserve((size_t)r * p.pieces * 8))) return p;
    p.split = nnf_plan_split(m, ldx, p.ncb, mu_right_wgpc(MT, BM) * (int64_t)cus, 0, (int64_t)r * nnf_rup(n, 4) * 4,
                             mu_two_acc(BM) ? 2 : 1, cur.remaining());
    return p;
}
// weighted form: a second stream with its own pitch runs next to X through the same 32-bit offsets -- the offset bound and the
// row halving of the split hold for the larger of the two pitches
inline mu_right_plan mu_plan_right_w(nnf_ws_cursor cur, int cus, int64_t m, int64_t n, int64_t ldx, int64_t ldw, int64_t ldu, int r, int MT) {
    return mu_plan_right(cur, cus, m, n, ldx > ldw ? ldx : ldw, ldu, r, MT, BM_WGEN);
}
inline void mu_report_right(FILE* f, int64_t m, int64_t n, int r, nnf_rank_tiles t, bool vec, int BM, const mu_right_plan& p,
                            const char* more = "") {
    fprintf(f, "[nnf plan] mu_right m=%lld n=%lld r=%d mt=%d rem=%d vec=%d bm=%s nsplit=%lld rps=%lld bound=%s%s\n", (long long)m,
            (long long)n, r, t.MT, t.REM, (int)vec, mu_bm_name(BM), (long long)p.split.nsplit, (long long)p.split.rows_per_split,
            p.split.bound, more);
}

// ---- left update ----
// Rows per workgroup (4 waves x 4, 3 or 2 tiles of 16 rows): whole ROUNDS of resident workgroups, all of about the same
// length -- R = ceil(T / (16 slots)) rounds of `slots` workgroups, each 8 to 16 tiles, as a mix of two adjacent sizes.
// 256-row workgroups everywhere put 977 workgroups on the 768 slots of the 250000-row pass of config D: a second round
// that is 27 % full and as long as the first.  Less than one round of 128-row workgroups: 128 rows each (most CUs busy).
struct mu_left_plan {
    int status;
    const char* form;
    int64_t grid, n_hi, n_mid;   // the first n_hi workgroups take 256 rows, the next n_mid 192, the others 128
    int64_t slots;               // resident workgroups
    int pieces;                  // of the row sums of V (KL forms; else 0)
    bool covers(int64_t m) const { return n_hi * 256 + n_mid * 192 + (grid - n_hi - n_mid) * 128 >= m; }
};
// `cur`: a copy of the caller's cursor -- the update takes r doubles, the row sums' partials and, in the cost-carrying forms,
// one double per workgroup
inline mu_left_plan mu_plan_left(nnf_ws_cursor cur, int cus, int64_t m, int64_t n, int64_t ldx, int64_t ldv, int r, nnf_rank_tiles t,
                                 int BM) {
    const int MT = t.MT;
    mu_left_plan p{NNF_ERR_UNSUPPORTED, "", 0, 0, 0, (int64_t)mu_left_wgpc(MT, t.REM, BM) * cus,
                   BM == BM_KL || BM == BM_KLC ? nnf_rowsum_pieces(n) : 0};
    if (64 * ldx * 4 + 4 * (n + 128) >= NNF_OFFSET32_END) return p;
    if ((int64_t)(16 * (MT + 1)) * ldv * 4 + 4 * (n + 128) >= NNF_OFFSET32_END) return p;   // 32-bit image offsets
    const int64_t slots = p.slots, T = nnf_cdiv(m, 16);
    const int64_t W = nnf_cdiv(T, 16 * slots) * slots;
    p.grid = W;
    if (mu_left_rows128(MT, BM) || T <= 8 * slots) {
        p.grid = nnf_cdiv(m, 128);
    } else if (MT > 4) {   // ranks 81 .. 128, KL: 192- and 128-row workgroups (rounds of 8 to 12 tiles each; 16 do not fit the registers)
        const int64_t W3 = nnf_cdiv(T, 12 * slots) * slots;
        if (T <= 8 * W3) p.grid = nnf_cdiv(m, 128);
        else { p.grid = W3; p.n_mid = nnf_cdiv(T - 8 * W3, 4); }
    } else if (T > 12 * W) {
        p.n_hi = nnf_cdiv(T - 12 * W, 4);
        p.n_mid = W - p.n_hi;
    } else {
        p.n_mid = nnf_cdiv(T - 8 * W, 4);
    }
    p.form = T <= 8 * slots ? "small" : p.n_hi > 0 ? "hi" : p.n_mid > 0 ? "mid" : MT > 4 ? "rows128" : "mid";
    if (!p.covers(m)) return p;   // (cannot happen)
    const bool fits = cur.reserve((size_t)r * 8) && (p.pieces <= 1 || cur.reserve((size_t)r * p.pieces * 8)) &&
                      ((BM != BM_FROB && BM != BM_KLC) || cur.reserve((size_t)p.grid * 8));
    p.status = fits ? NNF_OK : NNF_ERR_WORKSPACE;
    return p;
}
// weighted form: the offset bound holds for the larger of the two pitches (see mu_plan_right_w)
inline mu_left_plan mu_plan_left_w(nnf_ws_cursor cur, int cus, int64_t m, int64_t n, int64_t ldx, int64_t ldw, int64_t ldv, int r, int MT) {
    return mu_plan_left(cur, cus, m, n, ldx > ldw ? ldx : ldw, ldv, r, nnf_rank_tiles{MT, 0}, BM_WGEN);
}
inline void mu_report_left(FILE* f, int64_t m, int64_t n, int r, nnf_rank_tiles t, bool vec, int BM, const mu_left_plan& p,
                           const char* more = "") {
    fprintf(f, "[nnf plan] mu_left m=%lld n=%lld r=%d mt=%d rem=%d vec=%d bm=%s form=%s grid=%lld n_hi=%lld n_mid=%lld%s\n",
            (long long)m, (long long)n, r, t.MT, t.REM, (int)vec, mu_bm_name(BM), p.form, (long long)p.grid, (long long)p.n_hi,
            (long long)p.n_mid, more);
}

// ---- mode update on the tensor's own layout (k_mu_mode.hip) ----
// T seen as (L, I, K): a workgroup owns MU_MODE_ROWS rows of I and a contiguous range of "units" -- one unit is 16 consecutive k
// of one l (the last unit of an l is ragged when K % 16 != 0), so that no MFMA tile straddles two slabs of T.  A workgroup stages
// MU_MODE_CHUNK units of V at a time in LDS.  The units are cut into `nsplit` ranges whose r x I partial numerators (and
// denominators, beta != 1) go to slabs in the workspace and are added in split order in fp64.
constexpr int MU_MODE_ROWS = 64;            // rows of I per workgroup: 4 waves x one 16-row tile
constexpr int MU_MODE_UNIT = 16;            // k per unit: one MFMA tile
constexpr int MU_MODE_CHUNK = 4;            // units per staged chunk of V
// resident workgroups per CU the split count aims at: what the registers of an instantiation hold (build/k_mu_mode.s) -- four
// 4-wave workgroups up to 128 VGPRs (beta = 1 up to MT = 3, and MT = 4 with 16-byte loads: 128; beta != 1 up to MT = 2: 108),
// three beyond (beta = 1, MT = 4, scalar loads: 132; beta != 1, MT = 3 and 4: 136 .. 152).  LDS (4 KiB per rank tile) never binds.
constexpr int mu_mode_wgpc(int MT, bool kl, bool vec) { return (kl ? (MT <= 3 || vec) : MT <= 2) ? 4 : 3; }
// the weighted form (nnf_mu_mode_w_f32: one instantiation per MT and load width serves every beta; MU_MODE_CHUNK more f32x4 in
// flight for the weights, and their copies of the chunk being worked on, next to both accumulators).  VGPRs of the instantiations
// (build/k_mu_mode.s; none spills, none has scratch), 16-byte | scalar loads: MT = 1: 128 | 128, MT = 2: 148 | 156, MT = 3: 180 |
// 184, MT = 4: 204 | 212 -- four 4-wave workgroups per CU up to 128 VGPRs, three up to 168, two up to 256: the load width never
// changes the figure
constexpr int mu_mode_w_wgpc(int MT, bool /*vec*/) { return MT <= 1 ? 4 : MT == 2 ? 3 : 2; }
// a workgroup sums its columns in fp32 MFMA accumulators: at most 256 units = 4096 columns, a chain of 1024 MFMA steps (the
// W^T X kernel's 2048-row cap is a chain of 512; its notes in k_stream_plan.h say what longer chains cost)
constexpr int64_t MU_MODE_UNITS_CAP = 256;
constexpr int MU_MODE_MAX_RANK = 64;
constexpr size_t mu_mode_shm(int MT) { return (size_t)MU_MODE_CHUNK * 16 * MT * MU_MODE_UNIT * 4; }
struct mu_mode_plan {
    int status;
    int64_t nrb;        // row blocks of MU_MODE_ROWS rows
    int64_t kt;         // units per l: ceil(K / 16)
    int64_t units;      // L * kt
    int64_t nsplit;     // column splits
    int64_t ups;        // units per split (a multiple of MU_MODE_CHUNK)
    const char* bound;  // which bound set the split count
    int64_t ws_max;     // splits the free workspace holds
    int pieces;         // of the row sums of V (beta = 1; else 0)
    int64_t ldp;        // pitch of a slab row
};
// `cur`: a copy of the caller's cursor -- the update takes r doubles, the row sums' partials, then one (beta = 1) or two sets of
// nsplit slabs of r x ldp floats.  `weighted` (nnf_mu_mode_w_f32, any beta): two sets of slabs and nothing in front of them
inline mu_mode_plan mu_plan_mode(nnf_ws_cursor cur, int cus, int64_t L, int64_t I, int64_t K, int r, bool kl, bool vec,
                                 bool weighted = false) {
    mu_mode_plan p{NNF_ERR_UNSUPPORTED, nnf_cdiv(I, MU_MODE_ROWS), nnf_cdiv(K, MU_MODE_UNIT), 0, 0, 0, "occupancy", 0, 0, nnf_rup(I, 4)};
    if (r > MU_MODE_MAX_RANK) return p;
    // element and column indices are 64-bit in the kernel; keep the products well inside them
    if ((double)L * (double)I * (double)K >= 4.0e18 || (double)L * (double)p.kt >= 4.0e18) return p;
    p.units = L * p.kt;
    p.pieces = kl && !weighted ? nnf_rowsum_pieces(L * K) : 0;
    p.status = NNF_ERR_WORKSPACE;
    if (!weighted && (!cur.reserve((size_t)r * 8) || (p.pieces > 1 && !cur.reserve((size_t)r * p.pieces * 8)))) return p;
    const int nsets = kl && !weighted ? 1 : 2;
    const int64_t slab_bytes = (int64_t)r * p.ldp * 4, free = (int64_t)cur.remaining();
    p.ws_max = free / (slab_bytes * nsets);
    while (nsets > 1 && p.ws_max >= 1 && nnf_rup(p.ws_max * slab_bytes, 256) + p.ws_max * slab_bytes > free) --p.ws_max;
    if (p.ws_max < 1) return p;
    p.nsplit = (int64_t)(weighted ? mu_mode_w_wgpc((r + 15) / 16, vec) : mu_mode_wgpc((r + 15) / 16, kl, vec)) * cus / p.nrb;
    if (p.nsplit < 1) p.nsplit = 1;
    if (p.nsplit < nnf_cdiv(p.units, MU_MODE_UNITS_CAP)) { p.nsplit = nnf_cdiv(p.units, MU_MODE_UNITS_CAP); p.bound = "chain"; }
    if (p.nsplit > nnf_cdiv(p.units, MU_MODE_CHUNK)) { p.nsplit = nnf_cdiv(p.units, MU_MODE_CHUNK); p.bound = "min_cols"; }
    if (p.nsplit > p.ws_max) { p.nsplit = p.ws_max; p.bound = "workspace"; }
    p.ups = nnf_rup(nnf_cdiv(p.units, p.nsplit), MU_MODE_CHUNK);
    p.nsplit = nnf_cdiv(p.units, p.ups);
    p.status = NNF_ERR_UNSUPPORTED;
    if ((double)p.nrb * (double)p.nsplit > 2147483647.0) return p;   // one-dimensional grid
    p.status = NNF_OK;
    return p;
}
// bytes the launcher carves for a plan (tools/nnf_plan.cpp prints it; tests/test_mu_mode_plan.py checks it against a cursor)
inline size_t mu_mode_ws_bytes(const mu_mode_plan& p, int r, bool kl, bool weighted = false) {
    nnf_ws_cursor c(nullptr, ~size_t(0) >> 1);
    if (!weighted) c.reserve((size_t)r * 8);
    if (p.pieces > 1) c.reserve((size_t)r * p.pieces * 8);
    for (int s = 0; s < (kl && !weighted ? 1 : 2); ++s) c.reserve((size_t)p.nsplit * r * p.ldp * 4);
    return c.off;
}
inline void mu_report_mode(FILE* f, int64_t L, int64_t I, int64_t K, int r, int MT, bool vec, bool kl, const mu_mode_plan& p,
                           const char* more = "", bool weighted = false) {
    fprintf(f, "[nnf plan] %s L=%lld I=%lld K=%lld r=%d mt=%d vec=%d bm=%s nrb=%lld nsplit=%lld ups=%lld units=%lld bound=%s%s\n",
            weighted ? "mu_mode_w" : "mu_mode", (long long)L, (long long)I, (long long)K, r, MT, (int)vec,
            weighted ? mu_bm_name(BM_WGEN) : kl ? "KL" : "GEN", (long long)p.nrb, (long long)p.nsplit,
            (long long)p.ups, (long long)p.units, p.bound, more);
}

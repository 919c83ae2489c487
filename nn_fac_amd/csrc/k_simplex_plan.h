// Launch plan of the simplex projection's Newton solve (k_simplex.hip; nnf_simplex_proj_kl_f32) that the launcher and
// tools/nnf_plan.cpp share.  No HIP in here: the tool is a plain host program.
//
// G lanes share a column: lane q of a group owns the rows k = q, q + G, q + 2G, ... and keeps them in registers as fp64 for
// the whole call -- at most SIMPLEX_ROWS_PER_LANE of them, which bounds G from below; a group with lanes that own no row at all
// but the first quarter of it is never taken, which bounds G from above.  Among the G a rank allows the plan takes the largest
// one whose cols * G lanes still fit SIMPLEX_LANES_PER_CU lanes per CU (a few thousand columns spread over the chip), and the
// smallest one beyond that (10^5 columns: one or four lanes per column, every lane busy with rows).
#pragma once
#include "k_stream_plan.h"

constexpr int SIMPLEX_BLOCK = 256;            // threads per workgroup: 256 / G columns
constexpr int SIMPLEX_ROWS_PER_LANE = 8;      // rows of a column one lane holds (H, C and D: 48 VGPRs of fp64 at most)
constexpr int SIMPLEX_LANES_PER_CU = 1024;    // lanes per CU up to which a wider group is preferred
constexpr int SIMPLEX_MAX_ITER = 1024;        // Newton iterations of one call: one slot of the stopping array each (8 KiB of LDS)
constexpr int SIMPLEX_GROUPS[4] = {1, 4, 16, 64};

// rows per lane of a rank at G lanes per column
constexpr int simplex_rows_per_lane(int r, int G) { return (r + G - 1) / G; }
// may a column of r rows run on G lanes?
constexpr bool simplex_group_ok(int r, int G) {
    return (G == 1 || G == 4 || G == 16 || G == 64) && simplex_rows_per_lane(r, G) <= SIMPLEX_ROWS_PER_LANE && (G == 1 || r > G / 4);
}
// bytes of the context workspace a call takes: one 64-bit slot per Newton iteration + the "NaN since" word
constexpr size_t simplex_ws_bytes(int max_iter) { return ((size_t)max_iter + 1) * 8; }

struct simplex_plan {
    int status;        // NNF_OK, or the refusal
    int G;             // lanes per column
    int rpl;           // rows per lane, rounded up to a power of two (the kernel instance)
    int cpb;           // columns per workgroup
    int64_t grid;      // workgroups: column j belongs to workgroup j / cpb
    bool forced;       // NNF_SIMPLEX_FORCE set G
    size_t ws_bytes;
};

// `force`: the value of NNF_SIMPLEX_FORCE (0: not set); a value the rank does not allow is refused
inline simplex_plan simplex_make_plan(int cus, int r, int64_t cols, int max_iter, int force, size_t ws_free) {
    simplex_plan p{NNF_ERR_UNSUPPORTED, 0, 0, 0, 0, force != 0, 0};
    if (r > NNF_MAX_RANK || max_iter < 1 || max_iter > SIMPLEX_MAX_ITER) return p;
    if (force != 0) {
        if (!simplex_group_ok(r, force)) return p;
        p.G = force;
    } else {
        for (int G : SIMPLEX_GROUPS) {
            if (!simplex_group_ok(r, G)) continue;
            if (p.G == 0 || (double)cols * G <= (double)cus * SIMPLEX_LANES_PER_CU) p.G = G;
        }
    }
    const int need = simplex_rows_per_lane(r, p.G);
    p.rpl = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
    p.cpb = SIMPLEX_BLOCK / p.G;
    p.grid = nnf_cdiv(cols, p.cpb);
    if (p.grid > 2147483647) return p;   // one-dimensional grid
    p.ws_bytes = simplex_ws_bytes(max_iter);
    p.status = ws_free >= p.ws_bytes ? NNF_OK : NNF_ERR_WORKSPACE;
    return p;
}
inline void simplex_report(FILE* f, int r, int64_t cols, int max_iter, bool matrix, const simplex_plan& p, const char* more = "") {
    fprintf(f, "[nnf plan] simplex r=%d cols=%lld max_iter=%d den=%s G=%d rpl=%d cpb=%d grid=%lld forced=%d ws_bytes=%zu%s\n", r,
            (long long)cols, max_iter, matrix ? "matrix" : "vec", p.G, p.rpl, p.cpb, (long long)p.grid, (int)p.forced, p.ws_bytes, more);
}

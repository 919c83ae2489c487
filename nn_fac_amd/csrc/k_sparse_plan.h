// Launch plan of the CSR kernels (k_sparse.hip; nnf_csr_xf_f32, nnf_csr_kl_f32) that the launcher, the kernels and
// tools/nnf_plan.cpp share.  No HIP in here: the tool is a plain host program.
//
// Work item = one CHUNK: at most CH consecutive stored entries of one row.  Row i of a matrix with row lengths len[i] owns the
// chunks [rowchunk[i], rowchunk[i + 1]), rowchunk = exclusive prefix sum of ceil(len[i] / CH) (an empty row owns none); chunk q
// of a row holds its entries [q CH, min((q + 1) CH, len)).  The table (rowchunk, and chunk -> row) is built once per matrix by
// the caller from CH = sparse_chunk_entries(); the kernels recompute a chunk's span from rowptr with sparse_chunk_span().
// One wave per chunk, whatever the row lengths are: a row of 10^6 entries is 10^6 / CH waves, a row of 10 entries is one.
//
// Inside a wave L lanes share a stored entry: lane l of a group reads the components 4 l .. 4 l + 3 of the gathered node-major
// row as one 16-byte load (L = the power of two that covers ceil(r / 4)), the 64 / L groups take consecutive entries, and every
// lane keeps U entries in flight (its loads are issued before the first of them is used).  Every chunk leaves its r sums as one
// node-major row of the context workspace (slot = chunk index); the second kernel adds the rows of a matrix row's chunks in
// chunk order in fp64 and writes the component-major output through an LDS tile of SPARSE_TILE_ROWS rows (coalesced on both
// sides).  Nothing is added by more than one writer: no atomics, no waiting, bitwise equal from run to run.
#pragma once
#include "k_stream_plan.h"

constexpr int SPARSE_BLOCK = 256;          // threads per workgroup of the gather kernel: 4 waves = 4 chunks
constexpr int SPARSE_WAVES = SPARSE_BLOCK / 64;
constexpr int SPARSE_TILE_ROWS = 64;       // matrix rows per workgroup of the sum-and-transpose kernel
constexpr int SPARSE_LONG_ROW = 16;        // chunks above which the whole workgroup sums a row (in contiguous segments of its chunk list)
constexpr int SPARSE_CH_MIN = 64;          // bounds of the chunk size (a power of two)
constexpr int SPARSE_CH_MAX = 1024;
constexpr int SPARSE_WAVES_PER_CU = 16;    // waves in flight per CU the chunk rule counts with

// floats of one node-major workspace row
constexpr int sparse_row_floats(int r) { return (r + 3) / 4 * 4; }
// lanes that share a stored entry: the power of two covering ceil(r / 4) 16-byte pieces
constexpr int sparse_lanes(int r) {
    const int pieces = (r + 3) / 4;
    return pieces <= 1 ? 1 : pieces <= 2 ? 2 : pieces <= 4 ? 4 : pieces <= 8 ? 8 : pieces <= 16 ? 16 : 32;
}
// stored entries one lane keeps in flight (64 / L * U per wave: 8 at ranks 65 .. 128, 16 at 17 .. 64, 32 .. 64 below)
constexpr int sparse_unroll(int L) { return L >= 16 ? 4 : L >= 4 ? 2 : 1; }

// Chunk size from sizes alone: a quarter of one wave's share of the stored entries (entries / waves in flight), rounded down to
// a power of two, within [SPARSE_CH_MIN, SPARSE_CH_MAX] -- a row longer than that is summed by several waves, so the longest
// wave of a skewed matrix is at most a quarter of the mean wave's work ahead of the others.
constexpr int sparse_chunk_entries(int cus, int64_t nnz) {
    const int64_t share = nnz / ((int64_t)4 * SPARSE_WAVES_PER_CU * (cus < 1 ? 1 : cus));
    int ch = SPARSE_CH_MIN;
    while (ch * 2 <= SPARSE_CH_MAX && ch * 2 <= share) ch *= 2;
    return ch;
}
constexpr bool sparse_chunk_ok(int ch) { return ch >= 1 && ch <= (1 << 20); }

// chunks a row of `len` stored entries owns
constexpr int64_t sparse_chunks_of_row(int64_t len, int ch) { return len <= 0 ? 0 : (len + ch - 1) / ch; }

// Entries [first, end) of chunk q (0-based inside its row) of the row [row_begin, row_end) of a matrix with nnz stored entries.
// Whatever the tables hold, the span lies inside [0, nnz] and is at most ch long (an inconsistent table gives an empty or a
// wrong span, never an index outside the arrays).
struct sparse_span { int64_t first, end; };
constexpr sparse_span sparse_chunk_span(int64_t row_begin, int64_t row_end, int64_t q, int ch, int64_t nnz) {
    if (row_begin < 0) row_begin = 0;
    if (row_end > nnz) row_end = nnz;
    if (q < 0 || row_begin >= row_end || q > (row_end - row_begin) / ch) return sparse_span{0, 0};
    const int64_t first = row_begin + q * ch;
    if (first >= row_end) return sparse_span{0, 0};
    return sparse_span{first, first + ch < row_end ? first + ch : row_end};
}

struct sparse_plan {
    int status;          // NNF_OK, or the refusal
    int L, U, G;         // lanes per stored entry, entries in flight per lane, entries per wave step (64 / L)
    int rp;              // floats of a workspace row
    int64_t grid;        // workgroups of the gather kernel: chunk c belongs to wave c % 4 of workgroup c / 4
    int64_t tgrid;       // workgroups of the sum-and-transpose kernel (0: no component-major output asked for)
    size_t lds_bytes;    // LDS tile of the sum-and-transpose kernel
    size_t part_bytes;   // workspace: nchunks node-major rows (0: no output matrix)
    size_t cost_bytes;   // workspace: one double per workgroup of the gather kernel (0: no cost)
    size_t ws_bytes;     // both, as the cursor carves them (each carve starts on a 256-byte boundary)
};

// `want_out`: a component-major r x nrows result is produced (csr_xf always; csr_kl with num != NULL); `want_cost`: the fp64
// cost partials (csr_kl with cost_f64 != NULL)
inline sparse_plan sparse_make_plan(int r, int64_t nrows, int64_t nchunks, bool want_out, bool want_cost, size_t ws_free) {
    sparse_plan p{NNF_ERR_UNSUPPORTED, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (r < 1 || r > NNF_MAX_RANK) return p;
    p.L = sparse_lanes(r);
    p.U = sparse_unroll(p.L);
    p.G = 64 / p.L;
    p.rp = sparse_row_floats(r);
    p.grid = nnf_cdiv(nchunks, SPARSE_WAVES);
    p.tgrid = want_out ? nnf_cdiv(nrows, SPARSE_TILE_ROWS) : 0;
    if (p.grid > 2147483647 || p.tgrid > 2147483647) return p;   // one-dimensional grids
    p.lds_bytes = (size_t)SPARSE_TILE_ROWS * (p.rp + 1) * 4;
    p.part_bytes = want_out ? (size_t)nchunks * p.rp * 4 : 0;
    p.cost_bytes = want_cost ? (size_t)p.grid * 8 : 0;
    nnf_ws_cursor cur(nullptr, ws_free);
    const bool fits = (p.part_bytes == 0 || cur.reserve(p.part_bytes)) && (p.cost_bytes == 0 || cur.reserve(p.cost_bytes));
    p.ws_bytes = p.cost_bytes != 0 ? ((p.part_bytes + 255) & ~size_t(255)) + p.cost_bytes : p.part_bytes;
    p.status = fits ? NNF_OK : NNF_ERR_WORKSPACE;
    return p;
}
inline void sparse_report(FILE* f, const char* what, int r, int64_t nrows, int64_t nnz, int64_t nchunks, int ch, const sparse_plan& p,
                          const char* more = "") {
    fprintf(f, "[nnf plan] %s r=%d nrows=%lld nnz=%lld nchunks=%lld CH=%d L=%d U=%d G=%d rp=%d grid=%lld tgrid=%lld lds_bytes=%zu "
               "part_bytes=%zu cost_bytes=%zu ws_bytes=%zu%s\n", what, r, (long long)nrows, (long long)nnz, (long long)nchunks, ch, p.L,
            p.U, p.G, p.rp, (long long)p.grid, (long long)p.tgrid, p.lds_bytes, p.part_bytes, p.cost_bytes, p.ws_bytes, more);
}

// ---- sparse TENSORS (k_sptensor.hip; nnf_sptensor_mttkrp_f32, nnf_sptensor_kl_f32) ------------------------------------------------
// One mode's sorted copy of a COO tensor is a CSR matrix whose "row" is a slice of that mode and whose stored entry carries
// ng = N - 1 indices instead of one column: the chunk table, the spans, the lanes per entry, the workspace rows and the second
// pass are the CSR kernels' (everything above).  What differs is what a lane holds in flight: ng 16-byte pieces per entry (one of
// every gathered factor row) instead of one, so the entries in flight per lane are cut to keep the pieces in flight per lane
// (U ng) at about twice the CSR kernel's U: 2 U / ng rounded down to a power of two, at least 1.
//     L        1, 2   4, 8   16, 32          pieces in flight per lane (U ng)
//     ng = 2   1      2      4               2 / 4 / 8
//     ng = 3   1      1      2               3 / 3 / 6
//     ng = 4   1      1      2               4 / 4 / 8
// The registers of every instance (build/k_sptensor.s) stay below the 128 of four waves per SIMD, so the
// chunk rule's SPARSE_WAVES_PER_CU = 16 holds for these kernels too.
constexpr int SPTENSOR_NG_MIN = 2;         // gathered factors per entry: tensors of order 3 ..
constexpr int SPTENSOR_NG_MAX = 4;         // .. 5
constexpr int sptensor_unroll(int L, int ng) {
    const int u = sparse_unroll(L) * 2 / (ng < 1 ? 1 : ng);
    return u >= 4 ? 4 : u >= 2 ? 2 : 1;
}
// the CSR plan of the mode's copy (nrows = the extent of the mode) with the entries in flight of `ng` gathered factors
inline sparse_plan sptensor_make_plan(int r, int ng, int64_t extent, int64_t nchunks, bool want_out, bool want_cost, size_t ws_free) {
    sparse_plan p = sparse_make_plan(r, extent, nchunks, want_out, want_cost, ws_free);
    if (ng < SPTENSOR_NG_MIN || ng > SPTENSOR_NG_MAX) {
        p.status = NNF_ERR_ARG;
        return p;
    }
    if (p.L > 0) p.U = sptensor_unroll(p.L, ng);
    return p;
}

// ---- OBSERVED entries only (k_sparse_obs.hip; nnf_csr_obs_f32, nnf_sptensor_obs_f32) ----------------------------------------------
// The MU sums of a factorization that fits the stored entries and nothing else: numerator AND denominator are sums over a slice's
// stored entries, so one gather kernel leaves two node-major workspace rows per chunk (one array each) and the second pass runs
// once per array.  A CSR matrix is the ng = 1 case of a mode's copy (colidx = index plane 0): chunk table, spans, lanes per entry,
// entries in flight and workspace rows are those of the plans above -- sparse_make_plan at ng = 1, sptensor_make_plan at
// ng = 2 .. 4 -- with part_bytes doubled and carved as two arrays (each starts on the cursor's 256-byte boundary).
constexpr int SPARSE_OBS_NG_MIN = 1;
inline sparse_plan sparse_obs_make_plan(int r, int ng, int64_t nrows, int64_t nchunks, bool want_sums, bool want_cost, size_t ws_free) {
    sparse_plan p = ng == SPARSE_OBS_NG_MIN ? sparse_make_plan(r, nrows, nchunks, want_sums, want_cost, ~size_t(0) >> 1)
                                            : sptensor_make_plan(r, ng, nrows, nchunks, want_sums, want_cost, ~size_t(0) >> 1);
    if (p.status != NNF_OK) return p;
    const size_t one = p.part_bytes;      // one array: nchunks node-major rows
    p.part_bytes = 2 * one;
    nnf_ws_cursor cur(nullptr, ws_free);
    const bool fits = (one == 0 || (cur.reserve(one) && cur.reserve(one))) && (p.cost_bytes == 0 || cur.reserve(p.cost_bytes));
    nnf_ws_cursor all(nullptr, ~size_t(0) >> 1);
    if (one != 0) all.reserve(one), all.reserve(one);
    if (p.cost_bytes != 0) all.reserve(p.cost_bytes);
    p.ws_bytes = all.off;
    p.status = fits ? NNF_OK : NNF_ERR_WORKSPACE;
    return p;
}

// The launch plans of libnnfac_hip.so without a device: the library's own plan functions (nn_fac_amd/csrc/k_stream_plan.h,
// k_mu_plan.h, k_hals_plan.h, k_simplex_plan.h) for any CU count, printed as the library reports them under NNF_PLAN_DEBUG / NNF_HALS_DEBUG.
//
//   nnf_plan < cases     one case per line:  <launcher> <CUs> <m> <n> <r> <row pitch of X> <beta> <workspace bytes> [key=value ...]
//                        launcher: xht | xty | mu_left | mu_right | mu_mode | mu_mode_w | mttkrp_rows | mttkrp_seg | partial_last |
//                        partial_mid | gram | cost; the factors are contiguous (r x m, r x n);
//                        optional keys: align= (offset of X from a 16-byte boundary, in floats; default 0) and, for mttkrp_rows
//                        (m x n = the unfolded tensor, pitch n), nb= lda= ldb= (Khatri-Rao inner length, factor pitches).
//                        Answer, one line per case: the "[nnf plan] ..." line of that launch, followed on the same line by the
//                        fields of the plan the report leaves out (slots, ncb, ws_max), or "status=<code>" for a refusal.
//                        beta = 2 (the Gram form of the MU updates: X H^T / W^T X + a Gram) is not a plan of these launchers.
//                        mu_left / mu_right with ldw= (the pitch of the weights, >= n) and optionally walign= (their offset from a
//                        16-byte boundary, in floats): the weighted forms (nnf_mu_left_w_f32 / nnf_mu_right_w_f32, bm=WGEN) --
//                        any beta, 2 included; the general-beta plans with the offset bounds taken at max(pitch of X, ldw), and
//                        16-byte loads only if X and the weights both qualify.
//                        mu_mode (the mode update on the tensor's own layout, any beta) reads the same eight fields as
//                          mu_mode <CUs> <L> <I> <r> <K> <beta> <workspace bytes> [align=] [ldv=]
//                        and adds kt= wgpc= ws_max= pieces= ldp= ws_bytes= (what the launcher carves for the plan).
//                        mu_mode_w (its weighted form, nnf_mu_mode_w_f32, bm=WGEN) reads the same line plus walign= (the weights'
//                        offset from a 16-byte boundary, in floats): any beta on two sets of slabs with nothing in front of them.
//                        The tensor and Gram launchers read the eight fields as
//                          mttkrp_seg <CUs> <rows> <segment length> <r> <row pitch> 0 <workspace bytes> [align=] [nseg=] [segstride=]
//                                     [fsld=] [fkld=] [fkalign=]     (segments per row, their stride, the pitches of the segment-side
//                                     and the inner factor, the inner factor's offset from a 16-byte boundary; default: one
//                                     segment, contiguous factors); adds ws_max=
//                          partial_last | partial_mid <CUs> <A> <B> <r> <B> 0 <workspace bytes>     (Y is r x A x B); partial_mid
//                                     adds ws_bytes=
//                          gram <CUs> <K> <K> <r> <pitch of A> 0 <workspace bytes> [align=] [ldg=]     (any rank; ldg: the pitch of
//                                     G, default r); adds ws_max= ws_bytes=
//                          xty_gram | xht_gram <CUs> <m> <n> <r> <row pitch of X> 0 <workspace bytes> [align=] [fld=] [falign=] [ldg=]
//                                     the cross product with the Gram of its factor riding in the launch (nnf_plan_rider; fld /
//                                     falign: the factor's pitch and offset from a 16-byte boundary, ldg: the pitch of G):
//                                     "[nnf plan] xty_gram rides= main_grid= rider_grid= rider_offset= grid= main_bytes=
//                                     rider_bytes= rider_ws_off= ws_bytes=", then gram_nsplit= gram_kps= gram_bytes= of the Gram's
//                                     own plan; rides=0: the two run as calls of their own
//                          cost <CUs> <m> <n> <r> <row pitch of X> <beta> <workspace bytes> [align=] [op=] [kr=] [pin=] [ldr=] [ralign=]
//                                     [csplit=]
//                                     op: ratio_kl | ratio_gen | prod (default: the cost of that beta; prod: a pass that only
//                                     writes the model, every rank pass but the last of a rank above 128); kr: the Khatri-Rao inner
//                                     length of the CP cost (T as an (I J) x K matrix: m = I J, n = K, kr = J); pin=1: a later
//                                     rank pass of a rank above 128, which reads the model back (the CP cost of rank R is asked
//                                     for its last pass: pin=1, r = R - 128 ((R - 1) / 128)); ldr, ralign: the pitch of the model
//                                     buffer and its offset from a 16-byte boundary, in floats (default: aligned, as the
//                                     library's own buffer is; the first output of nnf_mu_ratio_f32 is the caller's) -- X and the
//                                     model are loaded at one width; csplit: NNF_COST_CSPLIT; adds KS= shm= partial_bytes=
//                                     vf_bytes=
//                        The HALS sweep plan (k_hals_plan.h) reads key=value fields only:
//                          hals <CUs> mode= r= ncols= nsweeps= [sweep0=] [flags=] [ldm=] [ldv=] [ldvs=] [gram2=] [own_start=]
//                               [snapshots=] [force=] [pc_...=]     the fields of hals_shape: mode 0 a solve, 1 blind sweeps; flags
//                                     the NNF_HALS_* bits; the pitches default to ncols (ldvs: to ldv); gram2 / own_start /
//                                     snapshots = 1: a second Gram, separate start values, snapshots asked for; force: the
//                                     first letter of NNF_HALS_FORCE.  pc_...: the workgroups per CU the device would report
//                                     for the kernel instances of this shape -- pc_wave1= pc_wave2= (1, 2 columns per compute
//                                     wave) pc_quad= pc_lane_res= pc_lane_stream= pc_mfma= pc_generic_lds= pc_generic_big=
//                                     pc_generic_gcol= (the generic kernel's three forms, after their cap).  A figure the plan
//                                     asks for and the line does not give is an error: the tool names it and exits with 3.
//                                     Answer: the "[nnf hals] ..." line of that call (NNF_HALS_DEBUG; a refusal is its err=),
//                                     followed by gram_floats= mfma_floats= snap_floats= (what the launcher carves).
//                          hals_resident <CUs> r= [pc_lane_res=] [pc_generic_gcol=]     nnf_hals_resident_columns: "columns=<n>"
//                        The simplex projection's plan (k_simplex_plan.h) reads key=value fields too:
//                          simplex <CUs> r= cols= [max_iter=] [ws=] [force=] [matrix=] [pitch=] [both=]     max_iter defaults to
//                                     100, ws (free workspace bytes) to 1 GiB; force: NNF_SIMPLEX_FORCE; matrix=1: the
//                                     denominator is the r x cols matrix; pitch: the smallest of the operands' pitches (default
//                                     cols); both=1 / both=-1: den and den_vec both given / both missing.  Answer: the
//                                     "[nnf plan] simplex ..." line of that call, or "status=<code>" for a refusal (the argument
//                                     checks of nnf_simplex_proj_kl_f32 included).
//                        The slab reduction behind every split launch (nnf_plan_reduce_set, k_stream_plan.h), key=value only:
//                          reduce rows= cols= nslab= [lds=] [stride=] [ldo=] [align=] [out64=]     lds / ldo default to cols, stride
//                                     (floats from one slab to the next) to rows * lds; align: the slabs' offset from a 16-byte
//                                     boundary in floats; out64=1: the fp64 sums are asked for.  Answer: the "[nnf reduce] ..."
//                                     line of that launch (NNF_REDUCE_DEBUG), or "status=<code>" (the argument checks of
//                                     nnf_reduce_slabs_f32).
//                        The CSR kernels' plan (k_sparse_plan.h), key=value only:
//                          sparse <CUs> r= lens=<len0,len1,...> [ch=] [out=] [cost=] [ws=]     lens: the stored entries of every row
//                                     (the tool forms rowptr and the chunk table from them with the header's own functions); ch:
//                                     the chunk size (default: sparse_chunk_entries of the CU count and nnz); out / cost (default
//                                     1 / 0): a component-major result / the fp64 cost is asked for (csr_xf: out=1 cost=0; csr_kl:
//                                     any pair but 0 0); ws: free workspace bytes (default 1 GiB).  Answer: the "[nnf plan] csr_..."
//                                     line of that call (csr_xf / csr_kl), then carved= (the bytes a cursor has handed out after the launcher's
//                                     carves) and chunks=<row>:<first>:<end>,... (every chunk in chunk order, spans from
//                                     sparse_chunk_span as the kernel takes them; "-" for none), or "status=<code>".
//                        The sparse-tensor kernels' plan (k_sparse_plan.h: the CSR plan of one mode's sorted copy), key=value only:
//                          sptensor <CUs> r= ng= lens=<len0,len1,...> [ch=] [out=] [cost=] [ws=]     as `sparse`, with lens the stored
//                                     entries of every slice of the mode and ng = N - 1 the gathered factors per entry (2 .. 4).
//                                     Answer: the "[nnf plan] sptensor_..." line of that call (sptensor_mttkrp: out=1 cost=0;
//                                     sptensor_kl otherwise) with U = sptensor_unroll(L, ng), then ng=, carved= and chunks=, or
//                                     "status=<code>" (the argument checks of the entries included).
//                        The observed-entries kernels' plan (k_sparse_plan.h: sparse_obs_make_plan), key=value only:
//                          obs <CUs> r= ng= lens=<len0,len1,...> [ch=] [out=] [cost=] [ws=]     as `sptensor`, with ng = 1 for a CSR
//                                     matrix (1 .. 4) and out: the two sums (numerator and denominator) are asked for.  Answer:
//                                     the "[nnf plan] csr_obs ..." (ng = 1) or "[nnf plan] sptensor_obs ..." line of that call
//                                     (part_bytes: both workspace arrays), then ng=, carved= and chunks=, or "status=<code>".
//   nnf_plan shm         the dynamic LDS the fused MU launchers ask for at ranks 65 .. 128, one line per (MT, form):
//                        "<MT> <REM> <KL|GEN> <bytes>"   (r = 16 MT + REM, the largest rank of the split)
//
// Build: c++ -std=c++17 -I nn_fac_amd/csrc tools/nnf_plan.cpp -o nnf_plan   (tests/test_mu_plan_table.py and
// tools/mu_rank128_budget.py do it)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "k_mu_plan.h"
#include "k_hals_plan.h"
#include "k_simplex_plan.h"
#include "k_sparse_plan.h"
#include <string>
#include <vector>

static long long key_of(const char* rest, const char* key, long long dflt) {
    char pat[32];
    snprintf(pat, sizeof pat, " %s=", key);
    const char* at = strstr(rest, pat);
    return at ? atoll(at + strlen(pat)) : dflt;
}

// the pass of a cost line: op= if given, else the cost of beta
static const char* cost_op(const char* rest, double beta) {
    static const char* const named[] = {"ratio_kl", "ratio_gen", "prod"};
    const char* at = strstr(rest, " op=");
    for (const char* nm : named)
        if (at && strncmp(at + 4, nm, strlen(nm)) == 0 && strchr(" \t\r\n", at[4 + strlen(nm)])) return nm;
    return at ? nullptr : beta == 2.0 ? "frob" : beta == 1.0 ? "kl" : beta == 0.0 ? "is" : "gen";
}

static int print_shm() {
    for (int MT = 5; MT <= 8; ++MT)
        for (int gen = 0; gen < 2; ++gen)
            printf("%d 0 %s %zu\n", MT, gen ? "GEN" : "KL", mu_shm(MT, 0, 16 * MT, mu_frags_in_regs(MT, gen != 0)));
    printf("6 4 KL %zu\n", mu_shm(6, 4, 100, mu_frags_in_regs(6, false)));   // ranks 97 .. 100: leftover ranks on the VALU pipe
    return 0;
}

// ---- hals lines: the occupancy answers of the plan are the pc_ fields of the line being answered ----
static const char* hals_line;
static int hals_figure(const char* key) {
    char pat[32];
    snprintf(pat, sizeof pat, " %s=", key);
    const char* at = strstr(hals_line, pat);
    if (!at) {
        fprintf(stderr, "nnf_plan: the plan asks for %s, which this line does not give: %s", key, hals_line);
        exit(3);
    }
    return atoi(at + strlen(pat));
}
static int pc_wave(int, int cpw, int) { return hals_figure(cpw == 1 ? "pc_wave1" : "pc_wave2"); }
static int pc_quad(int) { return hals_figure("pc_quad"); }
static int pc_lane(int, bool resident) { return hals_figure(resident ? "pc_lane_res" : "pc_lane_stream"); }
static int pc_mfma(int) { return hals_figure("pc_mfma"); }
static int pc_generic(int, hals_layout l, int, size_t, int) {
    return hals_figure(l == HL_GENERIC_LDS ? "pc_generic_lds" : l == HL_GENERIC_BIG ? "pc_generic_big" : "pc_generic_gcol");
}
static int pc_lane_comm(int) { return hals_figure("pc_lane_comm"); }
static const hals_occupancy hals_line_occupancy = {pc_wave, pc_quad, pc_lane, pc_mfma, pc_generic, pc_lane_comm};

static int answer_hals(const char* name, const char* line) {
    int C = 0, used = 0;
    if (sscanf(line, "%*s %d%n", &C, &used) != 1 || C < 1) return 2;
    const char* rest = hals_line = line + used;
    const long long r = key_of(rest, "r", 0);
    if (strcmp(name, "hals_resident") == 0) {
        const long long columns = r < 1 ? 0 : hals_resident_columns(C, hals_line_occupancy, (int)r);
        if (columns > 0) printf("columns=%lld\n", columns);
        else printf("status=%d\n", r < 1 ? NNF_ERR_ARG : NNF_ERR_LAUNCH);
        return 0;
    }
    const long long n = key_of(rest, "ncols", 0), ldm = key_of(rest, "ldm", n), ldv = key_of(rest, "ldv", n);
    const char* fat = strstr(rest, " force=");
    const hals_shape q = {(int)key_of(rest, "mode", -1), (int)r, n, ldm, ldv, key_of(rest, "ldvs", ldv), (int)key_of(rest, "nsweeps", -1),
                          (int)key_of(rest, "sweep0", 0), (unsigned)key_of(rest, "flags", 0), key_of(rest, "gram2", 0) != 0,
                          key_of(rest, "own_start", 0) != 0, key_of(rest, "snapshots", 0) != 0,
                          fat && !strchr(" \t\r\n", fat[7]) ? fat[7] : (char)0};
    // (the argument checks of hals_entry, k_hals.hip)
    if ((q.mode != 0 && q.mode != 1) || r < 1 || n < 1 || ldm < n || ldv < n || q.nsweeps < 0 || q.sweep0 < 0 ||
        (q.flags & ~(NNF_HALS_SPARSITY | NNF_HALS_NORMALIZE | NNF_HALS_NONZERO))) {
        printf("status=%d\n", NNF_ERR_ARG);
    } else if (q.nsweeps > NNF_HALS_MAX_SWEEPS) {
        printf("status=%d\n", NNF_ERR_UNSUPPORTED);
    } else {
        const hals_plan p = hals_make_plan(C, hals_line_occupancy, q);
        char more[96];
        snprintf(more, sizeof more, " gram_floats=%zu mfma_floats=%zu snap_floats=%zu", p.gram_floats, p.mfma_floats, p.snap_floats);
        hals_report(stdout, q, p, more);
    }
    return 0;
}

static int answer_simplex(const char* line) {
    int C = 0, used = 0;
    if (sscanf(line, "%*s %d%n", &C, &used) != 1 || C < 1) return 2;
    const char* rest = line + used;
    const long long r = key_of(rest, "r", 0), cols = key_of(rest, "cols", 0), force = key_of(rest, "force", 0);
    const long long max_iter = key_of(rest, "max_iter", 100), ws = key_of(rest, "ws", 1024ll << 20), both = key_of(rest, "both", 0);
    // (the argument checks of nnf_simplex_proj_kl_f32, k_simplex.hip)
    if (r < 1 || cols < 1 || key_of(rest, "pitch", cols) < cols || both != 0 ||
        (force != 0 && force != 1 && force != 4 && force != 16 && force != 64)) {
        printf("status=%d\n", NNF_ERR_ARG);
        return 0;
    }
    const simplex_plan p = simplex_make_plan(C, (int)(r > 1000000 ? 1000000 : r), cols, (int)max_iter, (int)force, (size_t)ws);
    if (p.status != NNF_OK) printf("status=%d\n", p.status);
    else simplex_report(stdout, (int)r, cols, (int)max_iter, key_of(rest, "matrix", 0) != 0, p);
    return 0;
}

static int answer_sparse(const char* line, bool tensor, bool obs = false) {
    int C = 0, used = 0;
    if (sscanf(line, "%*s %d%n", &C, &used) != 1 || C < 1) return 2;
    const char* rest = line + used;
    const char* at = strstr(rest, " lens=");
    if (!at) return 2;
    std::vector<int64_t> rowptr(1, 0);
    for (const char* q = at + 6; *q && !strchr(" \t\r\n", *q);) {
        char* end = nullptr;
        const long long len = strtoll(q, &end, 10);
        if (end == q || len < 0) return 2;
        rowptr.push_back(rowptr.back() + len);
        q = *end == ',' ? end + 1 : end;
    }
    const int64_t nrows = (int64_t)rowptr.size() - 1, nnz = rowptr.back();
    const long long r = key_of(rest, "r", 0), ws = key_of(rest, "ws", 1024ll << 20);
    const int ch = (int)key_of(rest, "ch", sparse_chunk_entries(C, nnz));
    const bool out = key_of(rest, "out", 1) != 0, cost = key_of(rest, "cost", 0) != 0;
    const int ng = (int)key_of(rest, "ng", 0);
    // (the argument checks of nnf_csr_args_ok, k_sparse.hip, and of sptensor_args_ok, k_sptensor.hip)
    if (nrows < 1 || r < 1 || !sparse_chunk_ok(ch) || (!out && !cost) || (tensor && (ng < SPTENSOR_NG_MIN || ng > SPTENSOR_NG_MAX)) ||
        (obs && (ng < SPARSE_OBS_NG_MIN || ng > SPTENSOR_NG_MAX))) {
        printf("status=%d\n", NNF_ERR_ARG);
        return 0;
    }
    // the chunk table as the caller builds it: rowchunk = exclusive prefix sum of the rows' chunk counts, chunk -> row
    std::vector<int64_t> rowchunk(1, 0);
    std::vector<int> chunk_row;
    for (int64_t i = 0; i < nrows; ++i) {
        const int64_t k = sparse_chunks_of_row(rowptr[i + 1] - rowptr[i], ch);
        rowchunk.push_back(rowchunk.back() + k);
        chunk_row.insert(chunk_row.end(), (size_t)k, (int)i);
    }
    const int64_t nchunks = rowchunk.back();
    const int rr = (int)(r > 1000000 ? 1000000 : r);
    const sparse_plan p = obs      ? sparse_obs_make_plan(rr, ng, nrows, nchunks, out, cost, (size_t)ws)
                          : tensor ? sptensor_make_plan(rr, ng, nrows, nchunks, out, cost, (size_t)ws)
                                   : sparse_make_plan(rr, nrows, nchunks, out, cost, (size_t)ws);
    if (p.status != NNF_OK) {
        printf("status=%d\n", p.status);
        return 0;
    }
    nnf_ws_cursor cur(nullptr, (size_t)ws);      // the launcher's carves, in its order
    if (nchunks > 0 && out && obs) cur.reserve(p.part_bytes / 2), cur.reserve(p.part_bytes / 2);      // (numerator, denominator)
    else if (nchunks > 0 && out) cur.reserve(p.part_bytes);
    if (nchunks > 0 && cost) cur.reserve(p.cost_bytes);
    std::string chunks;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int row = chunk_row[(size_t)c];
        const sparse_span sp = sparse_chunk_span(rowptr[row], rowptr[row + 1], c - rowchunk[row], ch, nnz);
        char one[96];
        snprintf(one, sizeof one, "%s%d:%lld:%lld", c ? "," : "", row, (long long)sp.first, (long long)sp.end);
        chunks += one;
    }
    std::string more = " carved=" + std::to_string(cur.off) + " chunks=" + (nchunks ? chunks : std::string("-"));
    if (tensor || obs) more = " ng=" + std::to_string(ng) + more;
    const char* what = obs ? (ng == 1 ? "csr_obs" : "sptensor_obs") : tensor ? (out && !cost ? "sptensor_mttkrp" : "sptensor_kl") : (out && !cost ? "csr_xf" : "csr_kl");
    sparse_report(stdout, what, (int)r, nrows, nnz, nchunks, ch, p, more.c_str());
    return 0;
}

static int answer_reduce(const char* line) {
    const char* rest = line + strcspn(line, " \t");
    const long long rows = key_of(rest, "rows", 0), cols = key_of(rest, "cols", 0), nslab = key_of(rest, "nslab", 0);
    const long long lds = key_of(rest, "lds", cols), ldo = key_of(rest, "ldo", cols), stride = key_of(rest, "stride", rows * lds);
    // (the argument checks of nnf_reduce_slabs_f32, k_reduce.hip)
    if (nslab < 1 || rows < 1 || cols < 1 || lds < cols || ldo < cols || stride < (rows - 1) * lds + cols) {
        printf("status=%d\n", NNF_ERR_ARG);
        return 0;
    }
    // pointers that only carry what the plan reads of them: the slabs' offset from a 16-byte boundary, whether out64 is given
    static double sums64;
    const nnf_reduce_set q = nnf_plan_reduce_set((const float*)(uintptr_t)(4096 + 4 * (key_of(rest, "align", 0) & 3)), (int)nslab, stride,
                                                 (int)rows, cols, lds, nullptr, ldo, key_of(rest, "out64", 0) != 0 ? &sums64 : nullptr);
    nnf_report_reduce(stdout, q, 0, 1);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "shm") == 0) return print_shm();
    char line[4096], name[32], more[192];
    while (fgets(line, sizeof line, stdin)) {
        long long C, m, n, r, ld, ws;
        double beta;
        int used = 0;
        if (sscanf(line, "%31s", name) == 1 && strcmp(name, "reduce") == 0) {
            answer_reduce(line);
            continue;
        }
        if (sscanf(line, "%31s", name) == 1 && (strcmp(name, "sparse") == 0 || strcmp(name, "sptensor") == 0)) {
            if (answer_sparse(line, name[1] == 'p' && name[2] == 't') != 0) {
                fprintf(stderr, "nnf_plan: bad case line: %s", line);
                return 2;
            }
            continue;
        }
        if (sscanf(line, "%31s", name) == 1 && strcmp(name, "obs") == 0) {
            if (answer_sparse(line, false, true) != 0) {
                fprintf(stderr, "nnf_plan: bad case line: %s", line);
                return 2;
            }
            continue;
        }
        if (sscanf(line, "%31s", name) == 1 && (strncmp(name, "hals", 4) == 0 || strcmp(name, "simplex") == 0)) {
            if ((name[0] == 's' ? answer_simplex(line) : answer_hals(name, line)) != 0) {
                fprintf(stderr, "nnf_plan: bad case line: %s", line);
                return 2;
            }
            continue;
        }
        if (sscanf(line, "%31s %lld %lld %lld %lld %lld %lf %lld%n", name, &C, &m, &n, &r, &ld, &beta, &ws, &used) != 8) {
            if (line[strspn(line, " \t\r\n")] == 0) continue;
            fprintf(stderr, "nnf_plan: bad case line: %s", line);
            return 2;
        }
        const char* rest = line + used;
        const bool vec = key_of(rest, "align", 0) % 4 == 0 && ld % 4 == 0;   // x_vec_ok
        const nnf_ws_cursor cur(nullptr, (size_t)ws);
        const bool left = strcmp(name, "mu_left") == 0;
        int status = NNF_ERR_UNSUPPORTED;   // (ranks above 128 run in passes of 128: ask for one pass)
        more[0] = 0;
        if (strcmp(name, "mu_mode") == 0 || strcmp(name, "mu_mode_w") == 0) {   // m = L, n = I, ld = K
            const long long ldv = key_of(rest, "ldv", m * ld);
            const bool wt = name[7] != 0;   // the weighted form: any beta on the two-accumulator plan, 16-byte loads need Wg aligned too
            const bool kl = beta == 1.0 && !wt;
            const bool mvec = key_of(rest, "align", 0) % 4 == 0 && ld % 4 == 0 && ldv % 4 == 0 && (!wt || key_of(rest, "walign", 0) % 4 == 0);
            const int MT = (int)(r + 15) / 16;
            if (m < 1 || n < 1 || ld < 1 || r < 1 || !(beta >= 0.0) || ldv < m * ld) {
                status = NNF_ERR_ARG;
            } else {
                const mu_mode_plan p = mu_plan_mode(cur, (int)C, m, n, ld, (int)r, kl, mvec, wt);
                snprintf(more, sizeof more, " kt=%lld wgpc=%d ws_max=%lld pieces=%d ldp=%lld ws_bytes=%zu", (long long)p.kt,
                         wt ? mu_mode_w_wgpc(MT, mvec) : mu_mode_wgpc(MT, kl, mvec), (long long)p.ws_max,
                         p.pieces, (long long)p.ldp, p.status == NNF_OK ? mu_mode_ws_bytes(p, (int)r, kl, wt) : (size_t)0);
                if ((status = p.status) == NNF_OK) mu_report_mode(stdout, m, n, ld, (int)r, MT, mvec, kl, p, more, wt);
            }
        } else if (m < 1 || n < 1 || r < 1 || ld < n) {
            status = NNF_ERR_ARG;
        } else if (strcmp(name, "gram") == 0 && key_of(rest, "ldg", r) < r) {
            status = NNF_ERR_ARG;
        } else if (strcmp(name, "gram") == 0) {   // m = n = K, ld = the pitch of A
            const nnf_gram_plan p = nnf_plan_gram((int)C, (int)r, m, key_of(rest, "ldg", r) == r, vec, cur.remaining());
            snprintf(more, sizeof more, " ws_max=%lld ws_bytes=%zu", (long long)p.ws_max,
                     p.status == NNF_OK && p.form >= NNF_GRAM_SLABS ? (size_t)(p.nsplit * r * r * 4) : (size_t)0);
            if ((status = p.status) == NNF_OK) nnf_report_gram(stdout, (int)r, m, p, more);
        } else if (strcmp(name, "xty_gram") == 0 || strcmp(name, "xht_gram") == 0) {
            // the fused launch of a cross product and its factor's Gram (nnf_plan_rider): both plans as their own calls make them,
            // then the grid and the carve of the launch that holds both
            const bool xty = name[1] == 't';
            const long long K = xty ? m : n, fld = key_of(rest, "fld", K), ldg = key_of(rest, "ldg", r);
            const bool fvec = key_of(rest, "falign", 0) % 4 == 0 && fld % 4 == 0;   // x_vec_ok of the factor
            const nnf_rank_tiles t = xty ? nnf_xty_tiles((int)r, vec) : nnf_xht_tiles((int)r, vec);
            const nnf_gram_plan g = nnf_plan_gram((int)C, (int)r, K, ldg == r, fvec, cur.remaining());
            long long main_grid = -1;
            size_t main_bytes = 0;
            bool apart = false;   // forms of the cross product that take no rider: the two run as calls of their own
            if (fld < K || ldg < r) {
                status = NNF_ERR_ARG;
            } else if (r > NNF_MAX_RANK || (!xty && nnf_xht_use_lds(t, vec))) {   // rank passes, the LDS-staged X H^T
                apart = true;
            } else if (xty) {
                const nnf_split_plan p = nnf_plan_xty((int)C, m, n, ld, (int)r, t, 2, cur.remaining());
                if ((status = p.status) == NNF_OK) {
                    main_grid = nnf_split_grid(p.nsplit, (int)nnf_cdiv(n, 256));
                    main_bytes = (size_t)(p.nsplit * r * nnf_rup(n, 4) * 4);
                }
            } else if (nnf_xht_offsets_ok(n, ld)) {
                const nnf_xht_plan p = nnf_plan_xht_direct((int)C, m, n, (int)r, t, -1, 1, cur.remaining());
                if (p.covers(m)) {
                    status = NNF_OK;
                    main_grid = p.grid;
                    main_bytes = p.tail_parts > 0 ? (size_t)p.tail_parts * r * p.tail_ld * 4 : 0;
                }
            }
            if (main_grid >= 0) {
                const nnf_rider_plan rp = nnf_plan_rider(main_grid, main_bytes, g, (int)r, t.MT + (t.REM > 0), cur.remaining());
                snprintf(more, sizeof more, " gram_nsplit=%lld gram_kps=%lld gram_bytes=%zu", (long long)g.nsplit, (long long)g.kps,
                         g.status == NNF_OK && g.form >= NNF_GRAM_SLABS ? (size_t)(g.nsplit * r * r * 4) : (size_t)0);
                nnf_report_rider(stdout, name, rp, more);
            } else if (apart) {
                status = NNF_OK;
                nnf_report_rider(stdout, name, nnf_rider_plan{});
            }
        } else if (r > NNF_MAX_RANK) {
        } else if (strcmp(name, "mttkrp_seg") == 0) {   // m = rows, n = segment length, ld = row pitch
            const long long nseg = key_of(rest, "nseg", 1), segstride = key_of(rest, "segstride", n);
            const int MT = (int)(r + 15) / 16;
            const nnf_seg_plan p = nnf_plan_seg((int)C, m, ld, nseg, n, (int)r, key_of(rest, "fsld", nseg), cur.remaining());
            snprintf(more, sizeof more, " ws_max=%lld", (long long)p.ws_max);
            if ((status = p.status) == NNF_OK)
                nnf_report_seg(stdout, m, nseg, n, (int)r, MT, vec && segstride % 4 == 0,
                               key_of(rest, "fkalign", 0) % 4 == 0 && key_of(rest, "fkld", n) % 4 == 0, MT <= 2, p, more);
        } else if (strcmp(name, "partial_last") == 0) {   // m = A, n = B
            status = NNF_OK;
            nnf_report_partial_last(stdout, m, n, (int)r, nnf_plan_partial_last(m, (int)r));
        } else if (strcmp(name, "partial_mid") == 0) {
            const nnf_partial_mid_plan p = nnf_plan_partial_mid((int)C, m, n, (int)r, cur.remaining());
            snprintf(more, sizeof more, " ws_bytes=%zu", (size_t)(p.nchunk * r * nnf_rup(n, 4) * 4));
            if ((status = p.status) == NNF_OK) nnf_report_partial_mid(stdout, m, n, (int)r, p, more);
        } else if (strcmp(name, "cost") == 0) {
            const char* op = cost_op(rest, beta);
            const bool pin = key_of(rest, "pin", 0) != 0;
            // (launch_cost: a pass that reads the model back loads X and the model at one width)
            const bool cvec = vec && (!pin || (key_of(rest, "ralign", 0) % 4 == 0 && key_of(rest, "ldr", 0) % 4 == 0));
            if (!op || !(beta >= 0.0) || (pin && key_of(rest, "ldr", n) < n)) {
                status = NNF_ERR_ARG;
            } else if (nnf_cost_offsets_ok(ld, n)) {
                const nnf_cost_plan p = nnf_plan_cost((int)C, m, n, (int)r, key_of(rest, "kr", 0) > 0, (int)key_of(rest, "csplit", 0), pin,
                                                      strcmp(op, "prod") == 0, cur.remaining());
                snprintf(more, sizeof more, " KS=%d shm=%zu partial_bytes=%zu vf_bytes=%zu", p.KS, p.shm, p.partial_bytes, p.vf_bytes);
                if ((status = p.status) == NNF_OK) nnf_report_cost(stdout, m, n, (int)r, op, cvec, pin, key_of(rest, "kr", 0), p, more);
            }
        } else if (strcmp(name, "xty") == 0) {
            const nnf_rank_tiles t = nnf_xty_tiles((int)r, vec);
            const nnf_split_plan p = nnf_plan_xty((int)C, m, n, ld, (int)r, t, 2, cur.remaining());   // (XTY_BIG_WG: the product's 2)
            snprintf(more, sizeof more, " ws_max=%lld", (long long)p.ws_max);
            if ((status = p.status) == NNF_OK) nnf_report_xty(stdout, m, n, (int)r, t, vec, p, more);
        } else if (strcmp(name, "xht") == 0) {
            const nnf_rank_tiles t = nnf_xht_tiles((int)r, vec);
            const bool lds = nnf_xht_use_lds(t, vec);
            if (nnf_xht_offsets_ok(n, ld)) {
                const nnf_xht_plan p = lds ? nnf_plan_xht_lds((int)C, m, n, (int)r, t, ld, 0)
                                           : nnf_plan_xht_direct((int)C, m, n, (int)r, t, -1, 1, cur.remaining());
                if (p.covers(m)) {
                    status = NNF_OK;
                    nnf_report_xht(stdout, m, n, (int)r, t, vec, lds, p);
                }
            }
        } else if (strcmp(name, "mttkrp_rows") == 0) {
            const int MT = (int)(r + 15) / 16;
            const nnf_split_plan p = nnf_plan_rows((int)C, m, n, (int)r, cur.remaining());
            snprintf(more, sizeof more, " ws_max=%lld", (long long)p.ws_max);
            if ((status = p.status) == NNF_OK)
                nnf_report_rows(stdout, m, n, key_of(rest, "nb", 1), (int)r, MT, vec,
                                nnf_rows_kr_fast(key_of(rest, "nb", 1), MT, key_of(rest, "lda", 1), key_of(rest, "ldb", 1)), p, more);
        } else if ((left || strcmp(name, "mu_right") == 0) && key_of(rest, "ldw", 0) != 0) {   // the weighted forms
            const long long ldw = key_of(rest, "ldw", 0);
            const bool wvec = vec && key_of(rest, "walign", 0) % 4 == 0 && ldw % 4 == 0;
            const nnf_rank_tiles t{(int)(r + 15) / 16, 0};
            if (ldw < n || !(beta >= 0.0)) {
                status = NNF_ERR_ARG;
            } else if (left) {
                const mu_left_plan p = mu_plan_left_w(cur, (int)C, m, n, ld, ldw, n, (int)r, t.MT);
                snprintf(more, sizeof more, " slots=%lld", (long long)p.slots);
                if ((status = p.status) == NNF_OK) mu_report_left(stdout, m, n, (int)r, t, wvec, BM_WGEN, p, more);
            } else {
                const mu_right_plan p = mu_plan_right_w(cur, (int)C, m, n, ld, ldw, m, (int)r, t.MT);
                snprintf(more, sizeof more, " ncb=%d ws_max=%lld", p.ncb, (long long)p.split.ws_max);
                if ((status = p.split.status) == NNF_OK) mu_report_right(stdout, m, n, (int)r, t, wvec, BM_WGEN, p, more);
            }
        } else if ((left || strcmp(name, "mu_right") == 0) && beta != 2.0) {
            const int BM = beta == 1.0 ? BM_KL : BM_GEN;
            const nnf_rank_tiles t = mu_tiles_of(left, (int)r, BM == BM_KL, vec);
            if (left) {
                const mu_left_plan p = mu_plan_left(cur, (int)C, m, n, ld, n, (int)r, t, BM);
                snprintf(more, sizeof more, " slots=%lld", (long long)p.slots);
                if ((status = p.status) == NNF_OK) mu_report_left(stdout, m, n, (int)r, t, vec, BM, p, more);
            } else {
                const mu_right_plan p = mu_plan_right(cur, (int)C, m, n, ld, m, (int)r, t.MT, BM);
                snprintf(more, sizeof more, " ncb=%d ws_max=%lld", p.ncb, (long long)p.split.ws_max);
                if ((status = p.split.status) == NNF_OK) mu_report_right(stdout, m, n, (int)r, t, vec, BM, p, more);
            }
        } else {
            status = NNF_ERR_ARG;
        }
        if (status != NNF_OK) printf("status=%d\n", status);
    }
    return 0;
}

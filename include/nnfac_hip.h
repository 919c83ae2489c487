/*
 * nnfac_hip.h -- C ABI of libnnfac_hip.so, the MI355X (gfx950) inner-update engine behind
 * nn_fac's HALS-NNLS / beta-divergence MU hot path.
 *
 * The reference (ax-le/nn-fac) is pure Python: it has no FFI layer.  Each entry point below
 * names the reference statement(s) it replaces (file:line under /root/reference); the Python
 * host in nn_fac_amd/ keeps the reference's function signatures and calls these through ctypes
 * (INTEGRATION.md shows the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - every pointer except `ctx`, `out_ctx` is a DEVICE pointer owned by the caller (fp32 unless
 *     the name says f64); the library never frees or keeps them;
 *   - matrices are row-major with an explicit leading dimension in ELEMENTS;
 *   - factors are passed "transposed": an m-by-r factor U is handed over as Ut (r-by-m, ld >= m), which is the
 *     layout hals_nnls_acc itself works on (nnls.py:147 takes U_in^T, V_in as r-by-n_cols);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *     allocates nothing: scratch comes from the context workspace (sized at nnf_ctx_create);
 *   - return value: 0 = NNF_OK, negative = error (nnf_status_string); no exception crosses the ABI;
 *   - a context is bound to one device and must not be used from two threads at once; one context
 *     per stream if calls on different streams may overlap (they share the workspace otherwise).
 *   - rank limit: 1 <= r <= 128 (NNF_ERR_UNSUPPORTED above).
 *
 * Non-finite operands
 *   Every projection of the reference is np.maximum (nnls.py:162-170, mu.py:84-97, deep_mu.py:11) or np.minimum (ntd.py:613),
 *   and both keep a NaN: one NaN in a solve's operands makes that column of the factor NaN, the sum of squared steps NaN and
 *   ends hals_nnls_acc after that sweep (`eps >= delta * eps0` is false); one NaN in X makes a row of an MU update NaN, and
 *   nmf() returns all-NaN factors and NaN costs two iterations later.  NaN and Inf are ordinary data to every kernel here (no
 *   address, trip count or wait depends on an operand's value; a stopping decision is taken by every workgroup from the one
 *   exchanged total), and a NaN is never projected away.  Against the reference operation evaluated in fp64 on the same fp32
 *   operands (magnitudes such that nothing overflows fp32 that does not overflow fp64):
 *     1. an output column of a solve, or a row / column of an MU update, that the reference leaves all finite is within the
 *        kernel's tolerance;
 *     2. in any other column or row every entry that is NaN in the reference is NaN here, every entry that is non-finite
 *        there is non-finite here, and an entry the reference leaves finite is within tolerance or NaN -- a kernel may poison
 *        a whole column, it never returns it clean;
 *     3. the status of a solve: cnt is the reference's, eps is NaN exactly when the reference's is, eps0 is within tolerance
 *        or non-finite of the same kind, err stays 0;
 *     4. blind sweeps: nodelta[s] is NaN exactly for the sweeps where the reference's sum is;   5. snapshots obey 2;
 *     6. the cost entries (frob_resid, betadiv, cp3_betadiv, cp3_partial_cost, nmf_gram_cost: out[0] with out[1] = 1) return
 *        NaN when the reference's sum is NaN, frob_resid_rows in exactly the affected rows;
 *     7. the products (xty, xht, gram and their fused forms, mttkrp3, mttkrp3_from_partial, ttm3, small_gemm, mu_left_num,
 *        mu_right_accum) have no projection: the set of NaN outputs equals the reference's entry for entry (0 * NaN counts,
 *        as in numpy), every other entry is within tolerance.
 *   The sweep kernels whose row update is ONE v_max_f32 -- an instruction that returns the operand that is not NaN --
 *   (k_hals_wave.hip, the resident rank 33 .. 52 form of k_hals_fast.hip, k_hals_mfma.hip) run that form on finite data only:
 *   each has a second form of the row update (a compare-and-select, two instructions) and picks it, once per launch, where a
 *   non-finite value can reach a row update -- a wave of the wave kernel from its start values, right-hand side and first
 *   residual; a wave of the lane kernel from its loaded column (start values, scaled right-hand side) and the prep kernel's
 *   flag "the Gram is finite and has no zero on its diagonal"; a workgroup of the matrix-core kernel from its first residual.
 *   Finite operands stay finite, so the choice costs nothing per row; a finite problem whose fp32 intermediates overflow is
 *   outside this contract (tests/test_gpu_nonfinite.py).
 */
#ifndef NNFAC_HIP_H
#define NNFAC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNF_OK 0
#define NNF_ERR_ARG (-1)         /* bad size / null pointer / bad flag combination            */
#define NNF_ERR_LAUNCH (-2)      /* HIP runtime error on launch (hipGetLastError)              */
#define NNF_ERR_UNSUPPORTED (-3) /* shape outside the built kernels (tensor rank > 128, ...)      */
#define NNF_ERR_WORKSPACE (-4)   /* context workspace too small for this call                  */
#define NNF_ERR_DEVICE (-5)      /* wrong / unavailable device                                 */

/* One launch per product / cost pass and the register- or LDS-resident sweep kernels up to this rank.  The matrix and CP entry
 * points (nnf_gram / xty / xht / frob_resid / betadiv / mu_ratio / nmf_gram_cost / hals_solve / hals_sweeps / hals_row_* /
 * mttkrp3 / mttkrp3_from_partial / cp3_betadiv / ttm3 along the first and last axis) go on above it, as the reference does
 * (nn_fac/nmf.py:175-178: any rank <= min(shape); nnls.py:158 loops range(r)): the contractions and cost passes walk the rank
 * in chunks of 128, the sweeps run in the generic kernel on columns in global memory.  The fused MU updates (nnf_mu_left /
 * mu_right / mu_right_accum: every beta up to this rank, beta = 2 beyond it as well), nnf_ttm3_f32 along the middle axis and
 * the Tucker core update return NNF_ERR_UNSUPPORTED above it; the cost-carrying fused forms (nnf_mu_left_kl_cost_f32,
 * nnf_mu_left_num_f32, nnf_cp3_partial_cost_f32) stop at rank 64. */
#define NNF_MAX_RANK 128

/* hals flags */
#define NNF_HALS_SPARSITY 1u  /* subtract `sparsity` in the row update (nnls.py:162-164)       */
#define NNF_HALS_NORMALIZE 2u /* l2-normalise each row after its update (nnls.py:179-185)      */
#define NNF_HALS_NONZERO 4u   /* all-zero row -> 1e-16*max(V) (nnls.py:173-174)                */

typedef struct nnf_ctx nnf_ctx;

/* status block written by nnf_hals_solve_f32 (device memory, 8 doubles) */
#define NNF_HALS_ST_EPS 0     /* nodelta of the last executed sweep        (nnls.py:195)       */
#define NNF_HALS_ST_CNT 1     /* cnt as returned by the reference = sweeps done + 1 (:196)     */
#define NNF_HALS_ST_EPS0 2    /* nodelta of the first sweep                (nnls.py:188)       */
#define NNF_HALS_ST_ERR 3     /* 0 ok; 1 = grid barrier timed out (result invalid);
                                 2 = zero Gram diagonal met with NONZERO set (nnls.py:176-177);
                                 5 = nnf_hals_solve_group_f32: the group's column range is not valid */
#define NNF_HALS_ST_WORDS 8

int nnf_version(void);
/* The values the timing-only ablation / A-B switches of the kernel sources were COMPILED with, one "unit: NAME=value ..."
 * entry per translation unit, sorted by unit, separated by "; " (e.g. "k_xht: XHT_ABL=0; ...").  Every switch has a
 * product default; a stray -D in a build would silently ship a kernel that skips work, so tests/test_abi_and_host.py
 * compares this string with the defaults.  Writes at most `cap` bytes (NUL-terminated), returns the full length. */
size_t nnf_build_flags(char* buf, size_t cap);
const char* nnf_status_string(int status);

/* Create a context on HIP device `device` with `workspace_bytes` of scratch (0 = default 256 MiB). */
int nnf_ctx_create(nnf_ctx** out_ctx, int device, size_t workspace_bytes);
int nnf_ctx_destroy(nnf_ctx* ctx);
size_t nnf_ctx_workspace_bytes(const nnf_ctx* ctx);
/* Caller-owned device scratch for temporaries that grow with the DATA: nnf_frob_resid_f32 / nnf_betadiv_f32 at a rank above
 * NNF_MAX_RANK build the m x n model over rank chunks in 4*m*ldp bytes, ldp = n rounded up to 4 (taken from here, else from
 * the tail of the context workspace, else NNF_ERR_WORKSPACE).  16-byte aligned; not freed by the library; must stay alive
 * until the calls using it have finished on their streams.  (NULL, 0) withdraws it. */
int nnf_ctx_set_scratch(nnf_ctx* ctx, void* device_buf, size_t bytes);

/* Measurement hook: two caller-owned hipEvent_t (passed as void*; NULL, NULL removes them) that nnf_xty_f32 records on its
 * launch stream immediately before and after its main kernel, so that a benchmark can time the dominant kernel alone --
 * without the slab reduction that follows it -- with HIP events on the stream the kernel runs on. */
int nnf_ctx_set_probe(nnf_ctx* ctx, void* ev_begin, void* ev_end);
/* Which main kernel the two events bracket (default NNF_PROBE_XTY): the streaming kernel of nnf_xty_f32 / nnf_xht_f32 /
 * the cost entry points / nnf_mu_left_f32 / nnf_mu_right_f32 / nnf_mttkrp3_f32, or the persistent sweep kernel of
 * nnf_hals_solve_f32 / nnf_hals_sweeps_f32 -- each without the small preparation / reduction kernels around it. */
#define NNF_PROBE_XTY 0
#define NNF_PROBE_XHT 1
#define NNF_PROBE_COST 2
#define NNF_PROBE_HALS 3
#define NNF_PROBE_MU_LEFT 4
#define NNF_PROBE_MU_RIGHT 5
#define NNF_PROBE_MTTKRP 6
#define NNF_PROBE_COUNT 7
int nnf_ctx_set_probe_kernel(nnf_ctx* ctx, int kernel_id);
/* The same hook for a whole timed region: `npairs` (begin, end) pairs of caller-owned events, events[2i], events[2i + 1];
 * the i-th launch of the selected kernel after this call records pair i, launches beyond `npairs` record nothing (no wrap).
 * The library copies the pointers.  NULL / 0 removes the ring.  While a ring is set it takes precedence over the single pair.
 * This is how bench.py times the dominant kernel on the launches INSIDE its timed loop (next to whatever shares the chip
 * with it there) rather than in a stand-alone loop. */
int nnf_ctx_set_probe_ring(nnf_ctx* ctx, void* const* events, int npairs);
/* Number of pairs of the current ring that have been recorded so far (0 without a ring). */
int nnf_ctx_probe_ring_count(const nnf_ctx* ctx);

/* ---- multi-GPU exchange of the row-sharded path: RCCL all-reduce (sum, in place) over xGMI -------------
 * One process per GPU.  Rank 0 draws a 128-byte id (nnf_comm_unique_id) and hands it to the other ranks by any channel of
 * the host application; every rank then calls nnf_comm_create(its ctx, nranks, rank, id) -- collective, like
 * ncclCommInitRank.  What a sharded NMF iteration exchanges (nn_fac_amd/nmf.py does the same through torch.distributed):
 *   V update: UtM (r x n) | UtU (r x r) in ONE buffer -> nnf_allreduce_f32;  U update: the per-sweep stopping sums
 *   (nnf_hals_sweeps_f32 -> nnf_allreduce_f64 -> nnf_hals_stop_restore_f32);  cost: one double -> nnf_allreduce_f64.
 * RCCL is bound at run time (dlopen); NNF_ERR_DEVICE when it is not available. */
typedef struct nnf_comm nnf_comm;
int nnf_comm_unique_id(void* id_out_128_bytes);
int nnf_comm_create(nnf_comm** out_comm, nnf_ctx* ctx, int nranks, int rank, const void* id_128_bytes);
int nnf_comm_destroy(nnf_comm* comm);
int nnf_comm_size(const nnf_comm* comm);
int nnf_comm_rank(const nnf_comm* comm);
int nnf_allreduce_f32(nnf_comm* comm, float* buf, int64_t count, void* stream);
int nnf_allreduce_f64(nnf_comm* comm, double* buf, int64_t count, void* stream);

/* G[r x r] = A[r x K] * A^T.   Replaces VVt = np.dot(V, V.T) (nmf.py:407), UtU = np.dot(U.T, U) (nmf.py:432),
 * and each factor Gram in ntf.py:442-445.  Split-K partials are summed in fp64 in a fixed order. */
int nnf_gram_f32(nnf_ctx* ctx, const float* A, int r, int64_t K, int64_t lda, float* G, int64_t ldg, void* stream);
/* The same Gram and, next to it, the sums BEFORE they are rounded to fp32 (G64: r x r doubles, contiguous) -- the split-K
 * partials are added in fp64 anyway.  For nnf_nmf_gram_cost_g64_f32: fp32 storage of U^T U alone (3.4e-8 relative rms per
 * entry) bounds the Gram-identity cost at ~1e-4 of a late-run cost at 10^6 x 4000 rank 100. */
int nnf_gram_f64_f32(nnf_ctx* ctx, const float* A, int r, int64_t K, int64_t lda, float* G, int64_t ldg, double* G64, void* stream);

/* out[r x m] = V[r x n] * X[m x n]^T.   Replaces VMt = np.dot(V, data.T) (nmf.py:408), the "X H^T" product. */
int nnf_xht_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* V, int r, int64_t ldv,
                float* out, int64_t ldo, void* stream);

/* out[r x n] = Ut[r x m] * X[m x n].   Replaces UtM = np.dot(U.T, data) (nmf.py:433), the "W^T X" product.
 * Split over m across workgroups; partial slabs summed in a fixed order (bitwise reproducible). */
int nnf_xty_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int r, int64_t ldu,
                float* out, int64_t ldo, void* stream);

/* A cross product and the Gram of its small factor in ONE main launch and ONE slab reduction (the two are independent of each
 * other, nmf.py:407-408 / :432-433): the Gram's split-K workgroups ride behind the cross product's in the same grid, and one
 * reduction adds the slab sets of both.  Kernel bodies, split plans and slab order are those of the separate entry points, so
 * every output is bit for bit what nnf_xty_f32 + nnf_gram_f32 (nnf_gram_f64_f32 with G64 != NULL) and nnf_xht_f32 +
 * nnf_gram_f32 write.  Where the Gram cannot ride (its one-workgroup forms for K <= 1024, ranks above NNF_MAX_RANK, the
 * LDS-staged X H^T of ranks <= 32, a workspace too small for both carves) the call runs the two one after the other.
 *   nnf_xty_gram_f32: out[r x n] = Ut X,   G[r x r] = Ut Ut^T (pitch ldg), G64 (may be NULL): its sums before rounding
 *   nnf_xht_gram_f32: out[r x m] = V X^T,  G[r x r] = V V^T   (pitch ldg)
 * The NNF_PROBE_XTY / NNF_PROBE_XHT events bracket the main launch with its rider. */
int nnf_xty_gram_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int r, int64_t ldu,
                     float* out, int64_t ldo, float* G, int64_t ldg, double* G64, void* stream);
int nnf_xht_gram_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* V, int r, int64_t ldv,
                     float* out, int64_t ldo, float* G, int64_t ldg, void* stream);

/* *out_f64 = sum_ij (X[i,j] - sum_k Ut[k,i] V[k,j])^2.   Replaces np.linalg.norm(data - U@V, 'fro')**2 (nmf.py:452)
 * without materialising U@V.  Per-lane fp32, then fp64 from the wave level up, fixed order. */
int nnf_frob_resid_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                       const float* V, int64_t ldv, int r, double* out_f64, void* stream);

/* The same cost (nmf.py:452) from what a HALS iteration has on hand after its V update, without another pass over X:
 *     ||X - U V||^2 = ||X||^2 - 2 <V, U^T X> + sum_j v_j^T (U^T U) v_j
 * UtM = U^T X (r x n) and UtU (r x r) are the fp32 operands of the V update (nmf.py:432-433: they belong to the final U of
 * the iteration), V (r x n) is its result, *normx2_f64 = ||X||^2 (device scalar: computed once per run, all-reduced once in
 * a row-sharded run -- every other operand is replicated there, so this cost needs no collective).  The three inner
 * products and the quadratic forms are taken in fp64; the fp32 rounding of UtM and UtU leaves an absolute error of
 * ~1e-9 ||X||^2 (measured: tools/probes/gram_cost_probe.py), which is only acceptable while the
 * residual is not that small.  The kernel estimates it and says so:
 *   out_f64[0] = cost,  out_f64[1] = 0 if the estimate is below 5e-4 of the cost, else 1 (the caller then evaluates
 *   nnf_frob_resid_f32 for this iterate),  out_f64[2] = the estimate (4 sigma).
 * UtU_b (may be NULL): the Gram is the Hadamard product UtU .* UtU_b -- the `cross` of one_ntf_step (ntf.py:442-445), whose
 * own cost line IS this identity (ntf.py:462-470): V = the last updated factor (transposed), UtM = its MTTKRP right-hand side. */
int nnf_nmf_gram_cost_f32(nnf_ctx* ctx, const float* V, int64_t ldv, const float* UtM, int64_t ldm, const float* UtU, const float* UtU_b,
                          int64_t ldg, int r, int64_t n, const double* normx2_f64, double* out_f64, void* stream);
/* The same with the caller's figures for the rounding of the cross term: sigma_a = relative rms error of a UtM entry, bias_a =
 * |relative mean error| (both >= 0).  nnf_nmf_gram_cost_f32 assumes 6e-8 / 0 -- what the W^T X kernel leaves at 100000 rows;
 * the error grows with the rows one workgroup sums in fp32 (1e6 x 4000 rank 100 on one device: 9.5e-7 rms, -2.2e-7 mean,
 * tools/probes/accum_error_probe.py), and a mean error does not average down: the estimate becomes
 *     4 sqrt((2 sigma_a ||V .* UtM||_F)^2 + sigma_B^2) + 4 bias_a |<V, UtM>|.
 * A driver measures the two once per run (nn_fac_amd/nmf.py: the cross product summed in one piece against the same summed
 * in 16 row blocks). */
int nnf_nmf_gram_cost_cal_f32(nnf_ctx* ctx, const float* V, int64_t ldv, const float* UtM, int64_t ldm, const float* UtU,
                              const float* UtU_b, int64_t ldg, int r, int64_t n, const double* normx2_f64, double sigma_a,
                              double bias_a, double* out_f64, void* stream);
/* The same with the quadratic form taken on UtU64 (nnf_gram_f64_f32; UtU, the fp32 Gram the solve used, still provides max|UtU|)
 * and sigma_g = the caller's figure for the relative rms error of a UtU64 entry (what the fp32 accumulation inside a split
 * leaves) in place of the 4e-8 of fp32 storage in sigma_B = sigma_g max|UtU| ||V||_F^2.  No Hadamard form (NMF loop only). */
int nnf_nmf_gram_cost_g64_f32(nnf_ctx* ctx, const float* V, int64_t ldv, const float* UtM, int64_t ldm, const float* UtU,
                              const double* UtU64, int64_t ldg, int r, int64_t n, const double* normx2_f64, double sigma_a,
                              double bias_a, double sigma_g, double* out_f64, void* stream);

/* hals_nnls_acc (nnls.py:147-198) on device: V (r x ncols, in/out) is swept in place until
 *   eps >= delta*eps0 fails, or sweeps == max_sweeps                         (nnls.py:156)
 * max_sweeps is min(maxiter, floor(1+alpha*rho)) resolved by the host; the wall-clock rule of nnls.py:190-194 stays
 * on the host side (nn_fac_amd/update_rules/nnls.py).  UtU is r x r (ldg), UtM r x ncols (ldm).
 * status_f64: NNF_HALS_ST_WORDS doubles.  The sweep loop, the global sum of squared steps and the stopping decision
 * all run inside one persistent launch (grid barrier per sweep); nothing is read back by the host. */
int nnf_hals_solve_f32(nnf_ctx* ctx, const float* UtM, int64_t ldm, const float* UtU, int64_t ldg, float* V, int64_t ldv,
                       int r, int64_t ncols, int max_sweeps, double delta, float sparsity, unsigned flags,
                       double* status_f64, void* stream);

/* hals_nnls_acc as one_ntf_step calls it (ntf.py:442-456): Gram = UtU_a .* UtU_b (the `cross` of two factor Grams; UtU_b may be
 * NULL), start values V_in, result in V_out (may alias V_in) -- nnf_hals_solve_f32 without the Hadamard launch and the copy
 * in front of it.  max_sweeps <= 1000. */
int nnf_hals_solve_cross_f32(nnf_ctx* ctx, const float* UtM, int64_t ldm, const float* UtU_a, const float* UtU_b, int64_t ldg,
                             const float* V_in, int64_t ldvi, float* V_out, int64_t ldvo, int r, int64_t ncols, int max_sweeps,
                             double delta, float sparsity, unsigned flags, double* status_f64, void* stream);

/* max_sweeps above 1000 (one launch tags at most 1000 sweeps; nnf_hals_solve_f32 answers NNF_ERR_UNSUPPORTED): chain
 * nnf_hals_solve_f32(..., 1000, ...) with nnf_hals_solve_continue_f32(..., sweeps_done = 1000, 2000, ..., max_sweeps = the
 * next slice <= 1000, ...) on the same stream and status block.  A continuation whose predecessor already ended the solve
 * (nnls.py:156) returns at once; the block finally holds eps / cnt / eps0 of the whole solve.  No host round trip. */
int nnf_hals_solve_continue_f32(nnf_ctx* ctx, const float* UtM, int64_t ldm, const float* UtU, int64_t ldg, float* V,
                                int64_t ldv, int r, int64_t ncols, int sweeps_done, int max_sweeps, double delta,
                                float sparsity, unsigned flags, double* status_f64, void* stream);

/* Same sweeps, fixed count, no stopping rule: runs exactly `nsweeps` sweeps and writes the LOCAL sum of squared steps of
 * each sweep to nodelta_f64[0..nsweeps).  Building block of the row-sharded solve (the stopping scalar is all-reduced by
 * the host between chunks).
 * snapshots (may be NULL): nsweeps blocks of r x ncols floats (row stride ncols, block stride snap_stride elements); block s
 * receives V after sweep s+1, so an overshoot of the global stopping rule is undone by copying one block (no replay). */
int nnf_hals_sweeps_f32(nnf_ctx* ctx, const float* UtM, int64_t ldm, const float* UtU, int64_t ldg, float* V, int64_t ldv,
                        int r, int64_t ncols, int nsweeps, float sparsity, unsigned flags, double* nodelta_f64,
                        float* snapshots, int64_t snap_stride, void* stream);

/* The same blind sweeps as a CONTINUATION of a solve (the chunks of the row-sharded protocol; nnls.py:156-196 run in pieces):
 * `sweeps_done` sweeps of this solve have run in earlier calls.  At ranks 64..100 and many columns the sweeps run on the matrix
 * cores (k_hals_mfma.hip) and keep a scaled residual per column next to V; resid_in / resid_out (nnf_hals_resid_floats() floats
 * each, opaque layout, caller-owned; distinct buffers) hand it from call to call, and then the chunks of a solve leave bit for
 * bit what ONE call of all the sweeps leaves.  resid_in NULL (first chunk, or a caller that does not care): the residual is
 * formed from V; resid_out NULL: not kept.  The other kernel layouts carry no state and ignore both.
 * snap_first: the first sweep of this call (0-based) that writes a snapshot -- `head` blind sweeps and a window of snapshots
 * are ONE launch; snapshot block j receives V after sweep snap_first + j + 1 of this call (nsweeps - snap_first blocks). */
int nnf_hals_sweeps_ex_f32(nnf_ctx* ctx, const float* UtM, int64_t ldm, const float* UtU, int64_t ldg, float* V, int64_t ldv,
                           int r, int64_t ncols, int nsweeps, int sweeps_done, float sparsity, unsigned flags,
                           double* nodelta_f64, float* snapshots, int64_t snap_stride, int snap_first, const float* resid_in,
                           float* resid_out, void* stream);
/* Floats per residual-state buffer of nnf_hals_sweeps_ex_f32 for an r x ncols factor; 0 when the layout that runs keeps none. */
int nnf_hals_resid_floats(nnf_ctx* ctx, int r, int64_t ncols, int64_t* floats_out);

/* Row-sharded solves that normalise the SHARDED factor (nmf(normalize=[True, .]) over several ranks): the row
 * norm of nnls.py:179-185 runs over the columns of all ranks, once per row update, so the host walks the rows:
 *   nnf_hals_row_update_f32  row k of V (r x ncols: this rank's columns) gets the update of nnls.py:162-170;
 *                            out2_f64 = {sum of squared steps, sum of squares of the updated row} over the local columns
 *   (the caller all-reduces the two doubles)
 *   nnf_hals_row_scale_f32   row k /= sqrt(*normsq_f64), or := 1/sqrt(ncols_total) when the norm is 0 (nnls.py:181-185) */
int nnf_hals_row_update_f32(nnf_ctx* ctx, const float* UtM, int64_t ldm, const float* UtU, int64_t ldg, float* V, int64_t ldv, int r,
                            int64_t ncols, int k, float sparsity, unsigned flags, double* out2_f64, void* stream);
int nnf_hals_row_scale_f32(nnf_ctx* ctx, float* V, int64_t ldv, int64_t ncols, int k, const double* normsq_f64, int64_t ncols_total,
                           void* stream);

/* Columns the sweep kernels of rank r keep resident on this device (all workgroups co-resident).
 * r <= 128: the register-resident kernel (one lane per column).  More columns than that: nnf_hals_solve_f32 /
 * nnf_hals_sweeps_f32 stream the factor through HBM once per sweep and nnf_hals_sweeps_f32 refuses `snapshots`; a caller that
 * runs blind chunks of sweeps (the row-sharded protocol of nnls.py:156, or the solve of a 10^6-column factor on one device)
 * splits the columns into blocks of at most this many and adds the blocks' per-sweep sums.
 * r > 128: the generic kernel with the column in global memory, one column per thread -- the most columns a persistent solve
 * (or sweeps with NNF_HALS_NORMALIZE / NNF_HALS_NONZERO) takes at that rank; blind sweeps without those flags take any number. */
int nnf_hals_resident_columns(nnf_ctx* ctx, int r, int64_t* columns_out);

/* Row-sharded solve, device-side stopping decision (no host round trip): after `nsweeps` blind sweeps of
 * nnf_hals_sweeps_f32 (snapshots for the last nsweeps - head of them) and an all-reduce of their per-sweep sums over the
 * ranks, replay nnls.py:156 over the sums: stop = first s with !(sum[s] >= delta*sum[0]) or s + 1 == budget.  A stop inside the
 * snapshot window restores V from that snapshot and writes {eps, cnt, eps0, 0} to status_f64; a stop before the window writes
 * error 3, no stop within these sweeps error 4 (the caller redoes the solve with a host-synchronous protocol). */
int nnf_hals_stop_restore_f32(nnf_ctx* ctx, const double* sums_f64, int nsweeps, int head, int budget, double delta, float* V,
                              int64_t ldv, int r, int64_t ncols, const float* snapshots, int64_t snap_stride,
                              double* status_f64, void* stream);

/* mu_betadivmin (mu.py:79-97) for the left factor, transposed storage:
 *   Ut_out[k,i] = max(Ut[k,i] * (num[k,i]/den[k,i])^gamma(beta), 1e-12),
 *   num = ((UV)^(beta-2) .* X) V^T, den = (UV)^(beta-1) V^T       (beta=1: den = rowsum(V); beta=2: Gram form)
 * One pass over X; U@V is never materialised and no data-sized temporary is used (device memory: the context workspace).
 * Ut_out must not alias Ut.  beta != 2 needs r <= NNF_MAX_RANK (else NNF_ERR_UNSUPPORTED). */
int nnf_mu_left_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                    const float* V, int64_t ldv, int r, double beta, float* Ut_out, int64_t lduo, void* stream);

/* mu_betadivmin (mu.py:79-97) for the factor of ONE mode of a tensor, on the tensor's own layout -- no unfolding is formed.
 * T is contiguous and seen as (L, I, K): for mode n of an order-N tensor L is the product of the extents before n, I = I_n,
 * K the product of those behind.  Ft (r x I, pitch ldf) is the mode's transposed factor, V (r x L*K, pitch ldv) the other
 * operand -- khatri_rao(others)^T or the expanded core -- whose column l*K + k belongs to the entries T[l, :, k]:
 *   out[k,i] = max(Ft[k,i] * (num[k,i]/den[k,i])^gamma(beta), 1e-12),  P[l,i,j] = sum_k Ft[k,i] V[k, l*K+j],
 *   num[k,i] = sum_{l,j} T[l,i,j] P^(beta-2) V[k, l*K+j],  den[k,i] = sum_{l,j} P^(beta-1) V[k, l*K+j]  (beta=1: rowsum(V), fp64)
 * One pass over T in place; the partial sums of the column splits go to the context workspace and are added in a fixed order
 * in fp64 (two calls are bitwise equal).  Any beta >= 0, any L, I, K >= 1.  r <= 64 (else NNF_ERR_UNSUPPORTED); a workspace
 * that cannot hold one set of r x I partial sums is refused with NNF_ERR_WORKSPACE; `out` must not alias Ft. */
int nnf_mu_mode_f32(nnf_ctx* ctx, const float* T, int64_t L, int64_t I, int64_t K, const float* Ft, int64_t ldf,
                    const float* V, int64_t ldv, int r, double beta, float* out, int64_t ldo, void* stream);

/* The sums of nnf_mu_mode_f32 under a weight per entry: Wg (contiguous, seen as (L, I, K) like T) holds finite weights >= 0,
 *   num[k,i] = sum_{l,j} Wg T P^(beta-2) V[k, l*K+j],  den[k,i] = sum_{l,j} Wg P^(beta-1) V[k, l*K+j]      (both r x I, fp32)
 * for any beta >= 0 (beta = 1 and beta = 2 exact: x/p and w, x and p).  The call returns the raw sums, as nnf_mu_left_w_f32 does;
 * nnf_mu_apply_f32 finishes.  An entry of weight zero is out of both sums whatever T holds there (NaN, Inf): a slice whose
 * weights are all zero gets num = den = 0 exactly.  Under a positive weight a zero of T is an observed zero.  The partial sums
 * of the column splits (two sets of r x I in the context workspace, nothing else) are added in split order in fp64: two calls
 * are bitwise equal.  16-byte loads need T, Wg and V aligned.  r <= 64 (else NNF_ERR_UNSUPPORTED). */
int nnf_mu_mode_w_f32(nnf_ctx* ctx, const float* T, const float* Wg, int64_t L, int64_t I, int64_t K, const float* Ft, int64_t ldf,
                      const float* V, int64_t ldv, int r, double beta, float* num, int64_t ldn, float* den, int64_t ldd,
                      void* stream);

/* nnf_mu_left_f32 with beta = 1 that also returns *cost_f64 = beta_divergence(X, U V, 1) of the factors it STARTS from
 * (mu.py:84-88 + nmf.py:455): the update forms every entry of U V anyway, so the cost of outer iteration i is a by-product of
 * the left update of iteration i+1 and the separate pass over X (nnf_betadiv_f32) is only needed after the last one.
 * Same update as nnf_mu_left_f32 bit for bit.  r <= 64. */
int nnf_mu_left_kl_cost_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                            const float* V, int64_t ldv, int r, float* Ut_out, int64_t lduo, double* cost_f64, void* stream);

/* switch_alternate_mu(..., "V") (mu.py:26-27): V_out[k,j] = max(V[k,j] * (num/den)^gamma, 1e-12) with
 *   num = U^T((UV)^(beta-2) .* X), den = U^T (UV)^(beta-1); split over m, fixed-order slab reduction.
 * beta != 2 needs r <= NNF_MAX_RANK (else NNF_ERR_UNSUPPORTED), like nnf_mu_right_accum_f32 below. */
int nnf_mu_right_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                     const float* V, int64_t ldv, int r, double beta, float* V_out, int64_t ldvo, void* stream);

/* Row-sharded right update (mu.py:79-97 on the transposed problem): the sums over the rows of X are
 * additive over row blocks, so every rank accumulates
 *   num = U^T((UV)^(beta-2) .* X)  (r x n)   and   den = U^T (UV)^(beta-1)  (r x n)
 * for its block (beta = 1: den_vec_f64[k] = sum_i U[i,k], r doubles, `den` unused; beta = 2: num = U^T X,
 * den = (U^T U) V), the caller all-reduces them, and nnf_mu_apply_f32 finishes:
 *   out[k,j] = max(F[k,j] * (num[k,j]/den[k,j])^gamma(beta), 1e-12)    (den_vec_f64 != NULL: den[k,j] = den_vec_f64[k]). */
int nnf_mu_right_accum_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                           const float* V, int64_t ldv, int r, double beta, float* num, int64_t ldnum, float* den,
                           int64_t ldden, double* den_vec_f64, void* stream);
int nnf_mu_apply_f32(nnf_ctx* ctx, const float* F, int64_t ldf, int r, int64_t cols, const float* num, int64_t ldnum,
                     const float* den, int64_t ldden, const double* den_vec_f64, double beta, float* out, int64_t ldo,
                     void* stream);

/* simplex_proj_mu at beta = 1 (mu.py:161-175) from already formed operands, with the multiplier solve of
 * update_lagragian_multipliers_simplex_projection (normalize_wh.py:24-58): H (r x cols) with its columns on the unit simplex.
 *   num = C = W^T(X ./ (WH)),  den = D = W^T 1  -- the num / den_vec_f64 of nnf_mu_right_accum_f32 at beta = 1; exactly one of
 *   `den` (r x cols matrix) and `den_vec_f64` (r doubles: den[k,j] = den_vec_f64[k]) is given, as in nnf_mu_apply_f32.
 *   lambda[j] starts from lambda0_f64[j], or (NULL) from the reference's D[0,j] - C[0,j] H[0,j]; up to max_iter times, all columns
 *   together:  den = D - lambda[j];  lambda[j] -= (sum_k H C/(den + 1e-8) - 1) / (sum_k H C/den^2 + 1e-8);  stop after the first
 *   iteration whose max_j |lambda - lambda_prev| is <= tol (ONE test over all columns);  then
 *   H_out = max(H .* (C ./ ((D - lambda) + 1e-12)), 1e-12).
 * The operands are fp32, every statement of the solve and of the update runs in fp64 (sums over k included), a NaN is kept:
 * a NaN operand makes its column NaN and the call run all max_iter iterations, as np.max does in the reference.
 * Two stream-ordered launches of one kernel and no wait between workgroups (nn_fac_amd/csrc/k_simplex.hip); two calls are
 * bitwise equal.  status_f64 (device, 2 doubles): {iterations run, max_j |dlambda| of the last one} -- the reference warns
 * 'Maximum of iterations reached ...' exactly when status[0] == max_iter and not status[1] <= tol.
 * H_out may be NULL (multipliers only) and may alias H; lambda_out_f64 (cols doubles) may be NULL.
 * Refused before anything is launched, every output untouched: r > NNF_MAX_RANK or max_iter outside 1 .. 1024
 * (NNF_ERR_UNSUPPORTED), both or neither of den / den_vec_f64 (NNF_ERR_ARG), a workspace that cannot hold max_iter + 1 64-bit
 * words (NNF_ERR_WORKSPACE).  beta != 1 has no entry point: the reference's rule does not reach the simplex there. */
int nnf_simplex_proj_kl_f32(nnf_ctx* ctx, const float* H, int64_t ldh, int r, int64_t cols, const float* num, int64_t ldnum,
                            const float* den, int64_t ldden, const double* den_vec_f64, const double* lambda0_f64, double tol,
                            int max_iter, float* H_out, int64_t ldo, double* lambda_out_f64, double* status_f64, void* stream);

/* Ranks beyond the fused kernels (r > NNF_MAX_RANK, every beta): the element-wise operands of mu_betadivmin (mu.py:84-97),
 *   R1 = X .* (UV)^(beta-2)   and, unless beta == 1,   R2 = (UV)^(beta-1)        (both m x n, row stride ldr, caller-owned),
 * written in one pass over X; the two contractions are then plain nnf_xht_f32 / nnf_xty_f32 calls on R1 / R2 and
 * nnf_mu_apply_f32 finishes (nn_fac_amd/engine.py composes them when the fused entry points return NNF_ERR_UNSUPPORTED).
 * Callable at every rank r >= 1.  Above NNF_MAX_RANK the model U V builds up over rank chunks of NNF_MAX_RANK inside R1 (no other
 * scratch): R1 is written before it is read, so what it held before the call is ignored.  Where X is 0, R1 is +0.  beta == 1
 * leaves R2 untouched (it may be NULL).  NNF_ERR_ARG, nothing launched and R1 / R2 untouched: ldr < n, R1 == NULL, R2 == NULL with
 * beta != 1, beta negative or NaN. */
int nnf_mu_ratio_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                     const float* V, int64_t ldv, int r, double beta, float* R1, float* R2, int64_t ldr, void* stream);

/* Deep KL-NMF (deep_nmf.py:84-113, update_rules/deep_mu.py:8-14), the three device pieces of deep_KL_mu:
 *   nnf_mu_left_num_f32   num[k,i] = sum_j (X[i,j]/(UV)[i,j]) V[k,j]  -- the raw KL numerator of the left update (the fused
 *                         kernel of nnf_mu_left_f32 without its division by rowsum(V)); b = U .* num  (deep_mu.py:10); r <= 64;
 *   nnf_small_gemm_f32    out[p x cols] = A[p x q] B[q x cols], q <= 2048 (eight rows of A at a time in LDS) -- (W_{l+1} H_{l+1})^T = H_{l+1}^T W_{l+1}^T
 *                         (deep_nmf.py:93,109), also the rank-sized links of the NTD contraction chains (ntd.py:539-557);
 *   nnf_deep_kl_apply_f32 out[k,i] = max(1e-12, (b/lambda) / (W0(b exp(a/lambda)/lambda) + 1e-12)),  b = F .* num,
 *                         a[k,i] = hsum_f64[k] - lambda log(WHnext[k,i])   (deep_mu.py:9-12; hsum = row sums of H_l, i.e.
 *                         ONES @ H_l^T; W0 = principal Lambert W, evaluated in fp64 from the LOGARITHM of its argument so
 *                         that exp(a/lambda) cannot overflow). */
int nnf_mu_left_num_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                        const float* V, int64_t ldv, int r, float* num, int64_t ldnum, void* stream);
int nnf_small_gemm_f32(nnf_ctx* ctx, const float* A, int64_t lda, int p, int q, const float* B, int64_t ldb, int64_t cols,
                       float* out, int64_t ldo, void* stream);
int nnf_deep_kl_apply_f32(nnf_ctx* ctx, const float* F, int64_t ldf, int r, int64_t cols, const float* num, int64_t ldnum,
                          const double* hsum_f64, const float* WHnext, int64_t ldw, double lambda, float* out, int64_t ldo,
                          void* stream);

/* beta_divergence(X, U@V, beta) (beta_divergence.py:45-52) fused with the product; *out_f64 = the sum. */
int nnf_betadiv_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                    const float* V, int64_t ldv, int r, double beta, double* out_f64, void* stream);

/* MTTKRP of a dense 3-way tensor T[I x J x K] (C order) with the Khatri-Rao product of the two other factors
 * generated on the fly: replaces khatri_rao + np.dot(unfolded[mode], krao) (ntf.py:448-449).
 * Factors are passed transposed (Ft_a: R x dim_a, ld = ld_a).  out is R x dim_mode (the rhs^T hals_nnls_acc wants). */
int nnf_mttkrp3_f32(nnf_ctx* ctx, const float* T, int64_t I, int64_t J, int64_t K, const float* Ft0, int64_t ld0,
                    const float* Ft1, int64_t ld1, const float* Ft2, int64_t ld2, int R, int mode, float* out,
                    int64_t ldo, void* stream);

/* MTTKRP from a shared partial product (dimension tree).  F2 does not change between the mode-0 and the mode-1 update of
 * one_ntf_step (ntf.py:437-456), so both right-hand sides are contractions of Y[r][i][j] = sum_k T[i][j][k] F2[k][r]
 * (= nnf_ttm3_f32(T, F2t, mode 2): ONE pass over T):  axis 2: out[r][a] = sum_b Y[r][a][b] Ft[r][b] (mode 0, Ft = F1t);
 * axis 1: out[r][b] = sum_a Y[r][a][b] Ft[r][a] (mode 1, Ft = the updated F0t).  Y is R x A x B, contiguous. */
int nnf_mttkrp3_from_partial_f32(nnf_ctx* ctx, const float* Y, int64_t A, int64_t B, const float* Ft, int64_t ldf, int R,
                                 int axis, float* out, int64_t ldo, void* stream);

/* Fused pass over T for an NTF iteration loop: the squared residual of the CURRENT CP model (ntf.py:470, evaluated
 * directly) and the partial product Y[r][i][j] = sum_k T[i][j][k] F2[k][r] the NEXT iteration's mode-0 / mode-1 right-hand
 * sides are contracted from -- both need the final factors and the whole tensor.  With the mode-2 MTTKRP an iteration then
 * reads T twice instead of four times.  R <= 64 (NNF_ERR_UNSUPPORTED above: use nnf_cp3_betadiv_f32 + nnf_ttm3_f32). */
int nnf_cp3_partial_cost_f32(nnf_ctx* ctx, const float* T, int64_t I, int64_t J, int64_t K, const float* Ft0, int64_t ld0,
                             const float* Ft1, int64_t ld1, const float* Ft2, int64_t ld2, int R, float* Y, double* cost_f64,
                             void* stream);

/* beta_divergence(T, [[F0,F1,F2]], beta) for a dense 3-way tensor and its CP model (factors transposed, R x dim): the cost
 * of ntf.py:470 (HALS: 2x the beta=2 value = ||T - model||^2) and ntf.py:473 (MU), Khatri-Rao operand generated on the fly. */
int nnf_cp3_betadiv_f32(nnf_ctx* ctx, const float* T, int64_t I, int64_t J, int64_t K, const float* Ft0, int64_t ld0,
                        const float* Ft1, int64_t ld1, const float* Ft2, int64_t ld2, int R, double beta, double* out_f64,
                        void* stream);

/* small helpers used by the drivers (all deterministic, fixed-order) */
/* Mode-n product of the 3-way data tensor with a transposed factor: out = T x_mode F^T
 * (tl.tenalg.mode_dot(T, F.T, mode); the contractions of ntd.py:550,581 and of mu_tensorial, mu.py:159, are chains of
 * these).  T is I x J x K row-major, Ft is r x I_mode (row stride ldf).  The new axis comes out FIRST for the two outer
 * modes -- mode 0: out[r][J][K], mode 2: out[r][I][J] -- and in place for the middle one -- mode 1: out[I][r][K]. */
int nnf_ttm3_f32(nnf_ctx* ctx, const float* T, int64_t I, int64_t J, int64_t K, const float* Ft, int64_t ldf, int r, int mode,
                 float* out, void* stream);

/* Projected-gradient update of the NTD core (ntd.py:588-619) and the Gram-form reconstruction error (ntd.py:639), one
 * single-workgroup launch, fp64 arithmetic in LDS:
 *   step = round(prod_i 1/sigma_max(M_i), 6);  repeat (<= max_iter, while update >= delta * first update):
 *       grad = core x_0 M0 x_1 M1 x_2 M2 - MtX + sparse;  core -= min(step*grad, core)
 * core (d0 x d1 x d2, updated in place), MtX same shape, M_i = F_i^T F_i (d_i x d_i, dense).
 * status_f64[6] = {iterations, last update norm, first update norm, step, norm_sq - 2<MtX,core> + <core x M, core>, 0}.
 * Cores whose four fp64 copies exceed one workgroup's LDS (~4500 entries) work out of the context workspace instead. */
int nnf_ntd_core_pg_f32(nnf_ctx* ctx, float* core, const float* MtX, const float* M0, const float* M1, const float* M2, int d0,
                        int d1, int d2, double sparse, double delta, int max_iter, double norm_sq, double* status_f64,
                        void* stream);

/* The same update for a core of any order: ndim modes, dims[i] the extents (host array), M[i] = F_i^T F_i (host array of ndim
 * device pointers, each dims[i] x dims[i], dense); core and MtX are dims[0] x ... x dims[ndim-1], row-major.  Semantics,
 * status block and arithmetic (fp64 accumulation, fixed summation order) are those of nnf_ntd_core_pg_f32, the power
 * iterations and the mode products run in mode order; with ndim = 3 the result is bit-identical to that entry's.
 * Limits: 3 <= ndim <= 8, every extent 1..128, S = prod dims <= 2^22; anything else returns NNF_ERR_ARG / NNF_ERR_UNSUPPORTED
 * before anything is launched or written.  Forms (S1 = S / dims[0]; a Gram "image" is the transposed Gram with rows padded
 * to a multiple of four floats, sum_i dims[i] * roundup4(dims[i]) * 4 bytes for all modes):
 *   multi  S >= 2048, 4 <= dims[0] <= CUs and 3.2 KB + images of modes 1.. + 4 S1 doubles <= 150 KB: one workgroup per
 *          mode-0 slab holds its slab of core, MtX and two scratch arrays (fp64) and those images in LDS; the slabs'
 *          partial products are exchanged through the workspace, one grid barrier per step (bounded spin: status[5] = 1).
 *   lds64  one workgroup; all images + four S-sized fp64 arrays in LDS (<= 160 KB with 2.2 KB of vectors).
 *   lds32  the same with the four arrays stored as fp32 (accumulation stays fp64).
 *   ws     one workgroup; the four fp64 arrays in the context workspace (32 S bytes); the images stay in LDS while they
 *          fit in 64 KB with the vectors, else they too are read from the workspace (reported as ws_gram).
 * No form asks for more than 160 KB of LDS.  NNF_NTD_DEBUG: "[nnf ntd] pgn d=(..) S=.. form=.." on stderr per call. */
int nnf_ntd_core_pgn_f32(nnf_ctx* ctx, float* core, const float* MtX, const float* const* M, int ndim, const int* dims,
                         double sparse, double delta, int max_iter, double norm_sq, double* status_f64, void* stream);

/* *out_f64 = sum_ij A[i,j]*B[i,j]   (fp64 accumulate)  -- inner products of ntf.py:470 */
int nnf_dot_f32(nnf_ctx* ctx, const float* A, int64_t lda, const float* B, int64_t ldb, int64_t rows, int64_t cols,
                double* out_f64, void* stream);
/* C = A .* B elementwise, r x r  (Hadamard of Grams, ntf.py:442-445) */
int nnf_hadamard_f32(nnf_ctx* ctx, const float* A, const float* B, float* C, int64_t count, void* stream);
/* The two fixed-order fp64 reductions every split launch of the library ends in, on the caller's data (tests/test_gpu_reduce.py
 * checks every form of them bit for bit; tests/reduce_restatement.py states the form a set of slabs takes and the order of its
 * sums; NNF_REDUCE_DEBUG: "[nnf reduce] rows= cols= nslab= lds= ldo= out64= form= blocks= set= block0=" on stderr, one line per
 * set of every reduction launch of the library).  Both refuse with NNF_ERR_ARG, launching nothing: a null pointer (but out64),
 * nslab, rows, cols or count < 1, lds < cols, ldo < cols, slab_stride < (rows - 1) * lds + cols. */
/* out[row][col] = (float) sum_s slabs[s*slab_stride + row*lds + col], fp64, slab order; out64 (may be NULL): the sums
 * before rounding, rows x cols contiguous.  The reduction behind every split launch, on the caller's slabs. */
int nnf_reduce_slabs_f32(nnf_ctx* ctx, const float* slabs, int nslab, int64_t slab_stride, int rows, int64_t cols,
                         int64_t lds, float* out, int64_t ldo, double* out64, void* stream);
/* out_f64[0] = scale * sum of count doubles, index order, one workgroup (the tail of the cost kernels). */
int nnf_sum_f64(nnf_ctx* ctx, const double* partial_f64, int64_t count, double scale, double* out_f64, void* stream);

/* ---- grouped kernels: the K slices of nonnegative PARAFAC2 (nn_fac/parafac2.py:509-600) in one launch each --------------
 * Group g owns the columns [off[g], off[g+1]) of stacked operands with `total_cols` columns; `off` is a DEVICE array of
 * ngroups + 1 int64 (non-decreasing, within [0, total_cols]).  The host cannot see it, so the caller declares what it needs to
 * know (max_group_cols) and the kernels check each group against that: a group whose range is not valid is skipped whole --
 * nothing of it is read or written (the solve marks its status block with NNF_HALS_ST_ERR = 5).  fp32 storage, sums in a
 * fixed order (two calls are bitwise equal), r <= NNF_MAX_RANK (NNF_ERR_UNSUPPORTED above), every refusal before anything is
 * launched or written.  No kernel here exchanges anything between workgroups (no grid barrier, no flag in memory), and none
 * asks for more than 132 KB of LDS. */

/* The longest group nnf_hals_solve_group_f32 takes.  One workgroup of 128 threads owns a group and walks its columns in
 * tiles of 128 once per sweep, so a group is r*r*len/128 dependent FMAs per sweep on ONE compute unit, and what it re-reads
 * per sweep, r*len floats, is 4 MiB -- one XCD's L2 -- at r = 128 and 8192 columns.  A longer group belongs to
 * nnf_hals_solve_f32, which spreads one solve over all compute units. */
#define NNF_HALS_GROUP_MAX_COLUMNS 8192
int nnf_hals_group_max_columns(nnf_ctx* ctx, int r, int64_t* columns_out);

/* ngroups independent solves with the semantics of nnf_hals_solve_f32 without flags (Gauss-Seidel over the rows, projection,
 * rows with a zero Gram diagonal left alone, eps0 from the first sweep, on while eps >= delta*eps0 and sweeps < max_sweeps;
 * fp32 row dots in index order, squared steps summed in fp64).  UtM and V: r x total_cols (ldm, ldv), V in/out; the Gram of
 * group g is the dense r x r matrix at UtU + g*gstride (row stride ldg); status_f64: ngroups blocks of NNF_HALS_ST_WORDS
 * doubles in the NNF_HALS_ST_* layout.  One workgroup per group: the stopping rule is a sum over that workgroup.
 * max_group_cols: the caller's bound on the group lengths, <= NNF_HALS_GROUP_MAX_COLUMNS (else NNF_ERR_UNSUPPORTED).  Groups of
 * one column (K diagonal updates in one launch) and empty groups are fine (an empty group changes nothing and reports eps 0,
 * cnt max_sweeps + 1, eps0 0); max_sweeps = 1 on a copy is a probe sweep, max_sweeps = 0 leaves V alone and reports eps 1,
 * cnt 1, eps0 0.  A NaN in a group's operands is not projected away ("Non-finite operands" at the head of this file, which
 * every solve obeys): as with np.maximum it stays in that group's V, makes its sum of squared steps NaN and ends its loop after
 * that sweep (eps NaN); the other groups do not see it. */
int nnf_hals_solve_group_f32(nnf_ctx* ctx, const float* UtM, int64_t ldm, const float* UtU, int64_t ldg, int64_t gstride,
                             float* V, int64_t ldv, int r, const int64_t* off, int ngroups, int64_t max_group_cols,
                             int64_t total_cols, int max_sweeps, double delta, double* status_f64, void* stream);

/* Per group, one pass over A (r x total_cols): G (may be NULL) receives A_g A_g^T as fp32 at G + g*gstride (row stride ldg)
 * and G64 (may be NULL; needs G) the same sums before their rounding, ngroups contiguous r x r blocks of doubles (as
 * nnf_gram_f64_f32 gives them: the Gram of a product A = W W*^T carries the square of its condition number);
 * dots_f64 (may be NULL; then B is ignored) receives c_g[q] = sum_i A[q,i] B[q,i] at dots_f64[g*r + q]; err_f64 (may be NULL;
 * then T is ignored) receives ||A_g - T_g||_F^2 at err_f64[g].  All sums in fp64.  Any group length. */
int nnf_group_gram_f32(nnf_ctx* ctx, const float* A, int64_t lda, int r, const int64_t* off, int ngroups, int64_t total_cols,
                       float* G, int64_t ldg, int64_t gstride, double* G64, const float* B, int64_t ldb, double* dots_f64,
                       const float* T, int64_t ldt, double* err_f64, void* stream);

/* out[:, seg g] = M_g A[:, seg g]:  M_g is p x q at M + g*mstride (row stride ldm), A q x total_cols, out p x total_cols (must
 * not alias A), p, q <= 128 (NNF_ERR_UNSUPPORTED above).  max_group_cols sizes the launch only (longer groups are still
 * computed).  fp32 FMAs in index order. */
int nnf_group_gemm_f32(nnf_ctx* ctx, const float* M, int64_t ldm, int64_t mstride, int p, int q, const float* A, int64_t lda,
                       const int64_t* off, int ngroups, int64_t max_group_cols, int64_t total_cols, float* out, int64_t ldo,
                       void* stream);

/* rows_f64[i] = sum_j (X[i,j] - sum_k Ut[k,i] V[k,j])^2, i < m: the per-row form of nnf_frob_resid_f32 in one streaming pass
 * over X; the model tile comes from the 16x16x4 fp32 MFMA and is never stored.  Per-slice costs of stacked slices are segment
 * sums of it.  r <= NNF_MAX_RANK. */
int nnf_frob_resid_rows_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Ut, int64_t ldu,
                            const float* V, int64_t ldv, int r, double* rows_f64, void* stream);

/* ---- sparse data: NMF on a CSR matrix, over the stored entries only (nn_fac_amd/sparse_nmf.py) ----------------------------
 * The matrix (nrows x ncols, nnz < 2^31 stored entries) is canonical CSR on the device: rowptr int64 [nrows + 1] with
 * rowptr[0] = 0, colidx int32 sorted inside a row and without duplicates, vals float; stored zeros are allowed.  A factor that
 * is GATHERED is passed node-major: ncols x ldn, row j holds the r components of node j, ldn >= r a multiple of 4 floats, the
 * base 16-byte aligned (one stored entry is one contiguous read; the columns r .. ldn are never used).  Results are
 * component-major (r x nrows), what nnf_hals_solve_f32 and nnf_mu_apply_f32 take.
 * Work is cut into chunks of at most `ch` consecutive stored entries of one row, one wave each, so that the time does not
 * depend on how the row lengths are distributed.  The chunk table is built ONCE per matrix by the caller (on the device):
 *   rowchunk int64 [nrows + 1] = exclusive prefix sum of ceil(len_i / ch)  (an empty row owns no chunk),
 *   chunk_row int32 [nchunks]  = the row of every chunk,  nchunks = rowchunk[nrows],
 * with ch = nnf_csr_chunk_entries (a power of two in 64 .. 1024 from the CU count and nnz: k_sparse_plan.h; NNF_SPARSE_CH in the
 * environment overrides it for measurements); any 1 <= ch <= 2^20 the table was built with is accepted.  The host cannot see
 * the tables: the kernels hold every index they read from them against nrows, ncols, nnz and nchunks, so that a table that does
 * not belong to the matrix gives wrong sums and never an access outside the arrays.
 * Every chunk leaves its r sums (fp32 FMAs in a fixed order) in one node-major row of the context workspace (4 nchunks
 * roundup4(r) bytes, NNF_ERR_WORKSPACE if that does not fit); a second kernel adds the rows of each matrix row's chunks in
 * chunk order in fp64, rounds once and writes the component-major result.  No atomics and no waiting between workgroups: two
 * calls are bitwise equal.  NaN / Inf in vals or the factors propagate.  r <= NNF_MAX_RANK (NNF_ERR_UNSUPPORTED above, as for
 * nnz or ncols >= 2^31); NNF_ERR_ARG, nothing launched: null pointers, ldn not a multiple of 4 or < r, a misaligned node-major
 * operand, short output pitches, nchunks outside [nnz / ch, nnz]. */
int nnf_csr_chunk_entries(nnf_ctx* ctx, int64_t nnz, int64_t* out);
/* out[k,i] = sum_{p in row i} vals[p] Fn[colidx[p], k]   (r x nrows, pitch ldo).  With the CSR of X and Fn = V^T this is V X^T
 * (r x m); with the CSR of X^T and Fn = U it is U^T X (r x n). */
int nnf_csr_xf_f32(nnf_ctx* ctx, const int64_t* rowptr, const int32_t* colidx, const float* vals, int64_t nrows, int64_t ncols,
                   int64_t nnz, const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, const float* Fn,
                   int64_t ldn, int r, float* out, int64_t ldo, void* stream);
/* The beta = 1 sums over the stored entries (mu.py:84-97 and beta_divergence at beta = 1 vanish wherever x = 0, up to the
 * terms the caller adds): per stored entry x at (i, j),  p = <Own_n[i, :], Fn[j, :]> (fp32: four products per lane in index
 * order, then a fixed tree),  q = x / p,
 *   num[k,i] = sum q Fn[j,k]     (r x nrows, pitch ldnum; may be NULL: cost only),
 *   cost_f64[0] = sum (x log(x / p) - x) in fp64     (may be NULL: numerator only);
 * a stored x = 0 adds 0 to both (0 log 0 := 0).  Own_n: nrows x ldo_n, node-major like Fn.  The caller adds
 * colsum(U) . rowsum(V) to the cost and hands num with the row sums to nnf_mu_apply_f32.  The U side takes the CSR of X
 * (Own_n = U, Fn = V^T), the V side the CSR of X^T (Own_n = V^T, Fn = U).  The three forms (both, num only, cost only) give the
 * same bits for what they share. */
int nnf_csr_kl_f32(nnf_ctx* ctx, const int64_t* rowptr, const int32_t* colidx, const float* vals, int64_t nrows, int64_t ncols,
                   int64_t nnz, const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, const float* Own_n,
                   int64_t ldo_n, const float* Fn, int64_t ldn, int r, float* num, int64_t ldnum, double* cost_f64, void* stream);

/* ---- sparse data: NTF on a COO tensor, over the stored entries only (nn_fac_amd/sparse_ntf.py) -----------------------------
 * A tensor of order N = 3, 4 or 5 (every extent and nnz < 2^31) is held as N sorted copies of its canonical coordinate list
 * (lexicographic order, no coordinate twice, stored zeros allowed), one per mode.  The copy of mode n is sorted by i_n with a
 * stable sort, so that a slice keeps its entries in lexicographic order of the other modes; it is the CSR layout above with
 * ng = N - 1 indices per entry:
 *   ptr  int64 [extent + 1]   the role of rowptr: slice i of mode n owns the entries [ptr[i], ptr[i + 1]),
 *   idx  int32 [ng][nnz]      planar: plane m holds the index of the m-th OTHER mode (increasing mode order) of every entry,
 *   vals float [nnz],
 * and the chunk table (rowchunk, chunk_row, nchunks, ch) of the CSR entries built from ptr.  The ng gathered factors are passed
 * node-major as a HOST array of ng device pointers Fn[m] (extents[m] x ldn, one common pitch ldn >= r, a multiple of 4 floats,
 * every base 16-byte aligned) in the order of the planes of idx.  Per stored entry x at p the kernels form
 *   h = Fn[0][idx[0][p], :] .* Fn[1][idx[1][p], :] .* ...      (fp32, in that order)
 * and leave each chunk's sums in the context workspace exactly as the CSR entries do; the same second kernel adds a slice's
 * chunks in chunk order in fp64.  No atomics and no waiting between workgroups: two calls are bitwise equal.  The kernels hold
 * every index they read from ptr, idx and the chunk table against the extents, nnz and nchunks (a table that does not belong to
 * the tensor gives wrong sums and never an access outside the arrays; an entry with an index outside its factor is dropped).
 * NNF_ERR_UNSUPPORTED: r > NNF_MAX_RANK, nnz or an extent >= 2^31.  NNF_ERR_ARG, nothing launched: null pointers, ng outside
 * 2 .. 4, ldn not a multiple of 4 or < r, a misaligned node-major operand, short output pitches, nchunks outside [nnz / ch, nnz]. */
/* The MTTKRP of mode n:  out[k,i] = sum_{p in slice i} vals[p] h_p[k]   (r x extent, pitch ldo), acc = fmaf(x, h, acc) in entry
 * order inside a chunk. */
int nnf_sptensor_mttkrp_f32(nnf_ctx* ctx, const int64_t* ptr, const int32_t* idx, const float* vals, int64_t extent, int64_t nnz,
                            const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, int ng,
                            const float* const* Fn, const int64_t* extents, int64_t ldn, int r, float* out, int64_t ldo, void* stream);
/* The beta = 1 sums of mode n, as nnf_csr_kl_f32 with h in the place of the gathered row:  p = <Own_n[i, :], h> (fp32: four
 * products per lane in index order, then a fixed tree),  q = x / p,
 *   num[k,i] = sum q h[k]     (r x extent, pitch ldnum; may be NULL: cost only),
 *   cost_f64[0] = sum (x log(x / p) - x) in fp64     (may be NULL: numerator only);
 * a stored x = 0 adds 0 to both.  Own_n: the factor of mode n, extent x ldo_n, node-major.  The three forms (both, num only, cost
 * only) give the same bits for what they share. */
int nnf_sptensor_kl_f32(nnf_ctx* ctx, const int64_t* ptr, const int32_t* idx, const float* vals, int64_t extent, int64_t nnz,
                        const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, int ng, const float* const* Fn,
                        const int64_t* extents, int64_t ldn, const float* Own_n, int64_t ldo_n, int r, float* num, int64_t ldnum,
                        double* cost_f64, void* stream);

/* ---- sparse data with MISSING entries: the MU sums of any beta >= 0 over the stored entries only ------------------------------
 * (nn_fac_amd/sparse_nmf.py, sparse_ntf.py with unstored="missing": an unstored entry is unknown, not zero.)  The layouts, the
 * chunk table, the workspace rows, the second pass and the refusals are those of nnf_csr_kl_f32 / nnf_sptensor_kl_f32 above.
 * Per stored entry x with h the gathered row (a tensor: the Hadamard product of the ng gathered rows, fp32 in mode order) and
 * p = <Own_n[i, :], h> (fp32: four products per lane in index order, then a fixed tree; formed once per entry),
 *   num[k,i] = sum x p^(beta - 2) h[k],   den[k,i] = sum p^(beta - 1) h[k]     (r x nrows, pitches ldnum / ldden; fp32 FMAs in entry
 *                                                                              order; given together or both NULL: cost only),
 *   cost_f64[0] = sum d_beta(x | p) in fp64 from the fp32 p     (may be NULL: sums only; the beta-divergence per entry of
 *                                                               beta_divergence.py:45-52, 1/2 (x - p)^2 at beta = 2).
 * This is mu_betadivmin (mu.py:82-97) with every sum cut down to the stored entries: F <- max(F (num / den)^gamma, eps) is
 * nnf_mu_apply_f32 on the two outputs.  beta = 0, 1, 2, 3 use multiplications and divisions only, any other beta a
 * single-precision power p^e = exp2(e log2 p).  A stored x = 0 is an OBSERVED zero: nothing to num, its term to den (h at
 * beta = 1), d_beta(0 | p) to the cost -- as nnf_betadiv_f32 has it for a zero entry, p at beta = 1 and +inf at beta = 0 (no
 * 0 log 0 := 0 here: the entry is data), p^beta / beta otherwise.  A slice without stored entries gets num = den = 0: the caller
 * keeps its factor row (0 / 0 otherwise).  Each chunk leaves two node-major rows in the context workspace (8 nchunks
 * roundup4(r) bytes); the three forms (both, sums only, cost only) give the same bits for what they share.  NNF_ERR_ARG, nothing
 * launched: what the KL entries refuse, one of num / den without the other, nothing asked for, beta < 0 or not finite. */
int nnf_csr_obs_f32(nnf_ctx* ctx, const int64_t* rowptr, const int32_t* colidx, const float* vals, int64_t nrows, int64_t ncols,
                    int64_t nnz, const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, const float* Own_n,
                    int64_t ldo_n, const float* Fn, int64_t ldn, int r, double beta, float* num, int64_t ldnum, float* den,
                    int64_t ldden, double* cost_f64, void* stream);
int nnf_sptensor_obs_f32(nnf_ctx* ctx, const int64_t* ptr, const int32_t* idx, const float* vals, int64_t extent, int64_t nnz,
                         const int64_t* rowchunk, const int32_t* chunk_row, int64_t nchunks, int ch, int ng, const float* const* Fn,
                         const int64_t* extents, int64_t ldn, const float* Own_n, int64_t ldo_n, int r, double beta, float* num,
                         int64_t ldnum, float* den, int64_t ldden, double* cost_f64, void* stream);

/* ---- weighted NMF on dense data: a weight per entry next to X (nn_fac_amd/weighted_nmf.py) -----------------------------------
 * Wg (m x n, pitch ldw >= n, independent of ldx) holds finite weights >= 0; the fit minimises sum_ij Wg[i,j] d_beta(X[i,j] |
 * (U V)[i,j]).  A 0/1 mask is the special case; Wg == 1 everywhere is plain mu_betadivmin.  With P = U V (never written):
 *   left :  num[k,i] = sum_j Wg[i,j] X[i,j] P[i,j]^(beta-2) V[k,j]     den[k,i] = sum_j Wg[i,j] P[i,j]^(beta-1) V[k,j]     (r x m)
 *   right:  num[k,j] = sum_i Wg[i,j] X[i,j] P[i,j]^(beta-2) U[i,k]     den[k,j] = sum_i Wg[i,j] P[i,j]^(beta-1) U[i,k]     (r x n)
 *   cost :  *out_f64 = sum_ij Wg[i,j] d_beta(X[i,j] | P[i,j])          (not normalised; 1/2 (x - p)^2 at beta = 2, as nnf_betadiv_f32)
 * The update itself is nnf_mu_apply_f32(F, num, den, NULL, beta).  The fused two-MFMA kernels of nnf_mu_left_f32 /
 * nnf_mu_right_f32 in their two-accumulator form, at every beta (beta = 1 and beta = 2 have no shortcut under weights: r1 = w x /
 * p, r2 = w and r1 = w x, r2 = w p per entry; any other beta the log2 / exp2 pair times w), with the general-beta launch plans; the
 * 32-bit offset bounds of the plans hold for max(ldx, ldw); 16-byte loads when X and Wg are both 16-byte aligned with pitches in
 * fours.  Where Wg[i,j] == 0 the entry adds exactly 0 to num, den and the cost WHATEVER X[i,j] holds, NaN and +-Inf included (a
 * select, not a product: Wg = !isnan(X) is a valid mask).  Under a positive weight a NaN or Inf of X goes through as in the
 * unweighted kernels, and x = 0 is an observed zero (nothing to num, its term to den, d_beta(0 | p) to the cost).  A row of U (a
 * column of V) whose weights are all zero gets num = den = 0 exactly: the caller keeps that factor row (0 / 0 otherwise).  The
 * right update adds its row splits in a fixed order (two calls are bitwise equal).  Any beta >= 0.  Nothing is launched and the
 * outputs are untouched on: r > NNF_MAX_RANK (NNF_ERR_UNSUPPORTED); a null pointer, a pitch below the row length, beta < 0 or
 * NaN (NNF_ERR_ARG); a workspace that cannot hold one pair of r x n slabs (right update: NNF_ERR_WORKSPACE). */
int nnf_mu_left_w_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Wg, int64_t ldw,
                      const float* Ut, int64_t ldu, const float* V, int64_t ldv, int r, double beta, float* num, int64_t ldnum,
                      float* den, int64_t ldden, void* stream);
int nnf_mu_right_w_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Wg, int64_t ldw,
                       const float* Ut, int64_t ldu, const float* V, int64_t ldv, int r, double beta, float* num, int64_t ldnum,
                       float* den, int64_t ldden, void* stream);
int nnf_betadiv_w_f32(nnf_ctx* ctx, const float* X, int64_t m, int64_t n, int64_t ldx, const float* Wg, int64_t ldw,
                      const float* Ut, int64_t ldu, const float* V, int64_t ldv, int r, double beta, double* out_f64,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NNFAC_HIP_H */

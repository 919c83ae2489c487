// What the sparse units share (k_sparse.hip: CSR matrices; k_sptensor.hip: one mode's sorted copy of a COO tensor): the argument
// checks of a chunked table and the second pass, both defined in k_sparse.hip.
#pragma once
#include "nnf_internal.h"
#include "k_sparse_plan.h"

static inline bool nnf_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the checks every entry over a chunked table shares; `nnz`, `nchunks` and `ch` are the caller's word on the device tables (the
// kernels hold every index they read from them against these extents).  `ncols`: the extent of the gathered operand Fn.
int nnf_csr_args_ok(const nnf_ctx* ctx, const void* rowptr, const void* colidx, const void* vals, int64_t nrows, int64_t ncols, int64_t nnz,
                    const void* rowchunk, const void* chunk_row, int64_t nchunks, int ch, const float* Fn, int64_t ldn, int r);

// nnf_csr_rowsum_kernel: out[k, i] = the workspace rows `part` of the chunks of row i, added in chunk order in fp64
int nnf_csr_rowsum_launch(const sparse_plan& p, hipStream_t st, const float* part, const int64_t* rowchunk, int64_t nrows, int64_t nchunks,
                          int r, float* out, int64_t ldo);

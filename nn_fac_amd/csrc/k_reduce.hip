// Fixed-order fp64 reductions behind the split launches of the library (W^T X, the X H^T tail, the Gram, the MU updates, MTTKRP,
// NTD): the slabs of a split added in slab order, and a vector of fp64 partials added in index order.  Bitwise reproducible.
// Which form a set of slabs takes is decided in k_stream_plan.h (nnf_plan_reduce_set; tools/nnf_plan.cpp `reduce` prints it
// without a device) and reported per set under NNF_REDUCE_DEBUG ("[nnf reduce] ... form= blocks= set= block0="); the kernels and
// launchers are here.  nnf_reduce_slabs_f32 and nnf_sum_f64 (include/nnfac_hip.h, at the end of this file) run the two
// reductions on the caller's data: tests/test_gpu_reduce.py checks every form bit for bit against tests/reduce_restatement.py
// (the rule of the plan and the order of the sums, restated), tests/test_reduce_plan.py holds the plan to it on the CPU, and
// tests/test_gpu_fused_cross.py the multi-set launch.
#include "nnf_internal.h"

// One set of slabs and where its sums go, with the form nnf_plan_reduce_set chose for it.  A launch handles one set
// (nnf_launch_reduce_slabs) or a short list of them behind one fused cross-product launch (nnf_launch_reduce_sets): workgroups
// [block0, block0 + blocks) of the launch belong to the set and walk it exactly as a launch of `blocks` workgroups of its own would.
//   out[row][col] = sum_s slabs[s][row][col]  (fp64 accumulate, slab order fixed -> bitwise reproducible)

// form 0 (lg = 0, scalar): one thread per element, eight slabs in flight
__device__ __forceinline__ void nnf_reduce_plain_body(const nnf_reduce_set& q, int blk) {
    const int64_t total = (int64_t)q.rows * q.cols;
    for (int64_t e = (int64_t)blk * 256 + threadIdx.x; e < total; e += (int64_t)q.blocks * 256) {
        const int64_t row = e / q.cols, col = e - row * q.cols;
        const float* p = q.slabs + row * q.lds + col;
        double s = 0.0;
        // eight slabs in flight, added in slab order (a load per trip waited for alone is a memory round trip per slab)
        for (int k = 0; k < q.nslab; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(k + u < q.nslab ? k + u : q.nslab - 1) * q.slab_stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (k + u < q.nslab) ? (double)v[u] : 0.0;
        }
        q.out[row * q.ldo + col] = (float)s;
        if (q.out64) q.out64[e] = s;          // (the Gram before it is rounded to fp32: nnf_gram_f64_f32)
    }
}

// same sums, four columns per thread (16-byte slab loads); needs lds % 4 == 0 and 16-byte aligned slabs
__device__ __forceinline__ void nnf_reduce_vec4_body(const nnf_reduce_set& q, int blk) {
    const int64_t cq = (q.cols + 3) >> 2, total = (int64_t)q.rows * cq;
    for (int64_t e = (int64_t)blk * 256 + threadIdx.x; e < total; e += (int64_t)q.blocks * 256) {
        const int64_t row = e / cq, col = 4 * (e - row * cq);
        const float* p = q.slabs + row * q.lds + col;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int k = 0; k < q.nslab; k += 4) {   // four slabs in flight, added in slab order
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(p + (int64_t)(k + u < q.nslab ? k + u : q.nslab - 1) * q.slab_stride);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool in = k + u < q.nslab;
                s0 += in ? (double)v[u][0] : 0.0;
                s1 += in ? (double)v[u][1] : 0.0;
                s2 += in ? (double)v[u][2] : 0.0;
                s3 += in ? (double)v[u][3] : 0.0;
            }
        }
        float* o = q.out + row * q.ldo + col;
        o[0] = (float)s0;
        if (col + 1 < q.cols) o[1] = (float)s1;
        if (col + 2 < q.cols) o[2] = (float)s2;
        if (col + 3 < q.cols) o[3] = (float)s3;
    }
}

// Few output elements, many slabs (MTTKRP: 15000 elements x 256 slabs took 64 us with one thread per element): P threads
// per element, each summing every P-th... a contiguous range of slabs, the P partials combined in part order through LDS.
// Fixed order -> bitwise reproducible.  Threads with the same part are consecutive in the element index (coalesced).
// part_sum: 256 doubles of LDS.  Every thread of the workgroup calls (barriers inside).
template <int P>
__device__ __forceinline__ void nnf_reduce_par_body(const nnf_reduce_set& q, int blk, double* part_sum) {
    constexpr int EPB = 256 / P;                 // elements per workgroup
    const int el = threadIdx.x % EPB, part = threadIdx.x / EPB;
    const int64_t total = (int64_t)q.rows * q.cols;
    const int per = (q.nslab + P - 1) / P;
    const int k0 = part * per, k1 = (k0 + per < q.nslab) ? (k0 + per) : q.nslab;
    for (int64_t e0 = (int64_t)blk * EPB; e0 < total; e0 += (int64_t)q.blocks * EPB) {
        const int64_t e = e0 + el;
        double s = 0.0;
        if (e < total) {
            const int64_t row = e / q.cols, col = e - row * q.cols;
            const float* p = q.slabs + row * q.lds + col;
            // this part's slabs eight at a time: all loads of a batch in flight, added in slab order (one load per trip, each
            // waited for alone, was 12-16 dependent memory round trips: 16 us behind W^T X at config B)
            for (int k = k0; k < k1; k += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(k + u < k1 ? k + u : k1 - 1) * q.slab_stride];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += (k + u < k1) ? (double)v[u] : 0.0;
            }
        }
        part_sum[part * EPB + el] = s;
        __syncthreads();
        if (part == 0 && e < total) {
            double t = part_sum[el];
#pragma unroll
            for (int c = 1; c < P; ++c) t += part_sum[c * EPB + el];
            const int64_t row = e / q.cols, col = e - row * q.cols;
            q.out[row * q.ldo + col] = (float)t;
            if (q.out64) q.out64[e] = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void nnf_reduce_slabs_kernel(nnf_reduce_set q) { nnf_reduce_plain_body(q, (int)blockIdx.x); }
__global__ __launch_bounds__(256) void nnf_reduce_slabs4_kernel(nnf_reduce_set q) { nnf_reduce_vec4_body(q, (int)blockIdx.x); }
template <int P>
__global__ __launch_bounds__(256) void nnf_reduce_slabs_par_kernel(nnf_reduce_set q) {
    __shared__ double part_sum[256];
    nnf_reduce_par_body<P>(q, (int)blockIdx.x, part_sum);
}

// Up to NNF_REDUCE_MAX_SETS sets in one launch: a workgroup finds its set from the block ranges (uniform per workgroup, so the
// barriers of the parts form stay legal) and runs that set's own form.
struct nnf_reduce_sets { nnf_reduce_set set[NNF_REDUCE_MAX_SETS]; int nsets; };
__global__ __launch_bounds__(256) void nnf_reduce_sets_kernel(nnf_reduce_sets a) {
    __shared__ double part_sum[256];
    const int b = (int)blockIdx.x;
    int i = 0;
    while (i + 1 < a.nsets && b >= a.set[i + 1].block0) ++i;
    const nnf_reduce_set& q = a.set[i];
    const int blk = b - q.block0;
    switch (q.lg) {
        case 0: if (q.vec4) nnf_reduce_vec4_body(q, blk); else nnf_reduce_plain_body(q, blk); break;
        case 1: nnf_reduce_par_body<2>(q, blk, part_sum); break;
        case 2: nnf_reduce_par_body<4>(q, blk, part_sum); break;
        case 3: nnf_reduce_par_body<8>(q, blk, part_sum); break;
        default: nnf_reduce_par_body<16>(q, blk, part_sum); break;
    }
}

// NNF_REDUCE_DEBUG (read once): one "[nnf reduce]" line per set of every launch below (nnf_report_reduce, k_stream_plan.h)
static inline bool nnf_reduce_debug() {
    static const bool dbg = getenv("NNF_REDUCE_DEBUG") != nullptr;
    return dbg;
}

int nnf_launch_reduce_slabs(const float* slabs, int nslab, int64_t slab_stride, int rows, int64_t cols, int64_t lds,
                            float* out, int64_t ldo, hipStream_t st, double* out64) {
    const nnf_reduce_set q = nnf_plan_reduce_set(slabs, nslab, slab_stride, rows, cols, lds, out, ldo, out64);
    if (nnf_reduce_debug()) nnf_report_reduce(stderr, q, 0, 1);
    if (q.lg > 0)
        return nnf_dispatch<4>(q.lg, [&](auto k) -> int {
            constexpr int P = 1 << decltype(k)::value;
            hipLaunchKernelGGL(nnf_reduce_slabs_par_kernel<P>, dim3(q.blocks), dim3(256), 0, st, q);
            NNF_CHECK_LAUNCH();
            return NNF_OK;
        });
    if (q.vec4) hipLaunchKernelGGL(nnf_reduce_slabs4_kernel, dim3(q.blocks), dim3(256), 0, st, q);
    else hipLaunchKernelGGL(nnf_reduce_slabs_kernel, dim3(q.blocks), dim3(256), 0, st, q);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// the sets of a fused cross-product launch (its slabs, the X H^T tail, the rider's Gram) in ONE launch: each set's sums are the
// bits nnf_launch_reduce_slabs gives it
int nnf_launch_reduce_sets(const nnf_reduce_set* sets, int nsets, hipStream_t st) {
    if (nsets < 1 || nsets > NNF_REDUCE_MAX_SETS) return NNF_ERR_ARG;
    if (nsets == 1)
        return nnf_launch_reduce_slabs(sets[0].slabs, sets[0].nslab, sets[0].slab_stride, sets[0].rows, sets[0].cols, sets[0].lds,
                                       sets[0].out, sets[0].ldo, st, sets[0].out64);
    nnf_reduce_sets a{};
    a.nsets = nsets;
    int grid = 0;
    for (int i = 0; i < nsets; ++i) {
        a.set[i] = sets[i];
        a.set[i].block0 = grid;
        grid += sets[i].blocks;
        if (nnf_reduce_debug()) nnf_report_reduce(stderr, a.set[i], i, nsets);
    }
    hipLaunchKernelGGL(nnf_reduce_sets_kernel, dim3(grid), dim3(256), 0, st, a);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// sum of `count` doubles in index order by one workgroup -> out[0]
__global__ __launch_bounds__(256) void nnf_sum_partials_kernel(const double* __restrict__ partial, int64_t count,
                                                               double scale, double* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < count; e += 8 * 256) {   // eight loads in flight, added in index order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = partial[e + 256 * u < count ? e + 256 * u : count - 1];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (e + 256 * u < count) ? v[u] : 0.0;
    }
    const double t = nnf_block_sum_f64(s, red);
    if (threadIdx.x == 0) out[0] = t * scale;
}

int nnf_launch_sum_f64(const double* partial, int64_t count, double scale, double* out, hipStream_t st) {
    hipLaunchKernelGGL(nnf_sum_partials_kernel, dim3(1), dim3(256), 0, st, partial, count, scale, out);
    NNF_CHECK_LAUNCH();
    return NNF_OK;
}

// ---- the two reductions on the caller's data (include/nnfac_hip.h; tests/test_gpu_reduce.py) ----
extern "C" int nnf_reduce_slabs_f32(nnf_ctx* ctx, const float* slabs, int nslab, int64_t slab_stride, int rows, int64_t cols,
                                    int64_t lds, float* out, int64_t ldo, double* out64, void* stream) {
    if (!ctx || !slabs || !out || nslab < 1 || rows < 1 || cols < 1 || lds < cols || ldo < cols ||
        slab_stride < (int64_t)(rows - 1) * lds + cols)
        return NNF_ERR_ARG;
    return nnf_launch_reduce_slabs(slabs, nslab, slab_stride, rows, cols, lds, out, ldo, (hipStream_t)stream, out64);
}

extern "C" int nnf_sum_f64(nnf_ctx* ctx, const double* partial_f64, int64_t count, double scale, double* out_f64, void* stream) {
    if (!ctx || !partial_f64 || !out_f64 || count < 1) return NNF_ERR_ARG;
    return nnf_launch_sum_f64(partial_f64, count, scale, out_f64, (hipStream_t)stream);
}

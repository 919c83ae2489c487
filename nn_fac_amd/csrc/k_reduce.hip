// Fixed-order fp64 reductions behind the split launches of the library (W^T X, the X H^T tail, the Gram, the MU updates, MTTKRP,
// NTD): the slabs of a split added in slab order, and a vector of fp64 partials added in index order.  Bitwise reproducible.
#include "nnf_internal.h"

// out[row][col] = sum_s slabs[s][row][col]  (fp64 accumulate, slab order fixed -> bitwise reproducible)
__global__ __launch_bounds__(256) void nnf_reduce_slabs_kernel(const float* __restrict__ slabs, int nslab,
                                                               int64_t slab_stride, int rows, int64_t cols, int64_t lds,
                                                               float* __restrict__ out, int64_t ldo, double* __restrict__ out64) {
    const int64_t total = (int64_t)rows * cols;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = e / cols, col = e - row * cols;
        const float* p = slabs + row * lds + col;
        double s = 0.0;
        // eight slabs in flight, added in slab order (a load per trip waited for alone is a memory round trip per slab)
        for (int k = 0; k < nslab; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(k + u < nslab ? k + u : nslab - 1) * slab_stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (k + u < nslab) ? (double)v[u] : 0.0;
        }
        out[row * ldo + col] = (float)s;
        if (out64) out64[e] = s;          // (the Gram before it is rounded to fp32: nnf_gram_f64_f32)
    }
}

// same sums, four columns per thread (16-byte slab loads); needs lds % 4 == 0 and 16-byte aligned slabs
__global__ __launch_bounds__(256) void nnf_reduce_slabs4_kernel(const float* __restrict__ slabs, int nslab,
                                                                int64_t slab_stride, int rows, int64_t cols, int64_t lds,
                                                                float* __restrict__ out, int64_t ldo) {
    const int64_t cq = (cols + 3) >> 2, total = (int64_t)rows * cq;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = e / cq, col = 4 * (e - row * cq);
        const float* p = slabs + row * lds + col;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int k = 0; k < nslab; k += 4) {   // four slabs in flight, added in slab order
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(p + (int64_t)(k + u < nslab ? k + u : nslab - 1) * slab_stride);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool in = k + u < nslab;
                s0 += in ? (double)v[u][0] : 0.0;
                s1 += in ? (double)v[u][1] : 0.0;
                s2 += in ? (double)v[u][2] : 0.0;
                s3 += in ? (double)v[u][3] : 0.0;
            }
        }
        float* o = out + row * ldo + col;
        o[0] = (float)s0;
        if (col + 1 < cols) o[1] = (float)s1;
        if (col + 2 < cols) o[2] = (float)s2;
        if (col + 3 < cols) o[3] = (float)s3;
    }
}

// Few output elements, many slabs (MTTKRP: 15000 elements x 256 slabs took 64 us with one thread per element): P threads
// per element, each summing every P-th... a contiguous range of slabs, the P partials combined in part order through LDS.
// Fixed order -> bitwise reproducible.  Threads with the same part are consecutive in the element index (coalesced).
template <int P>
__global__ __launch_bounds__(256) void nnf_reduce_slabs_par_kernel(const float* __restrict__ slabs, int nslab,
                                                                   int64_t slab_stride, int rows, int64_t cols, int64_t lds,
                                                                   float* __restrict__ out, int64_t ldo, double* __restrict__ out64) {
    constexpr int EPB = 256 / P;                 // elements per workgroup
    __shared__ double part_sum[P][EPB];
    const int el = threadIdx.x % EPB, part = threadIdx.x / EPB;
    const int64_t total = (int64_t)rows * cols;
    const int per = (nslab + P - 1) / P;
    const int k0 = part * per, k1 = (k0 + per < nslab) ? (k0 + per) : nslab;
    for (int64_t e0 = (int64_t)blockIdx.x * EPB; e0 < total; e0 += (int64_t)gridDim.x * EPB) {
        const int64_t e = e0 + el;
        double s = 0.0;
        if (e < total) {
            const int64_t row = e / cols, col = e - row * cols;
            const float* p = slabs + row * lds + col;
            // this part's slabs eight at a time: all loads of a batch in flight, added in slab order (one load per trip, each
            // waited for alone, was 12-16 dependent memory round trips: 16 us behind W^T X at config B)
            for (int k = k0; k < k1; k += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(k + u < k1 ? k + u : k1 - 1) * slab_stride];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += (k + u < k1) ? (double)v[u] : 0.0;
            }
        }
        part_sum[part][el] = s;
        __syncthreads();
        if (part == 0 && e < total) {
            double t = part_sum[0][el];
#pragma unroll
            for (int q = 1; q < P; ++q) t += part_sum[q][el];
            const int64_t row = e / cols, col = e - row * cols;
            out[row * ldo + col] = (float)t;
            if (out64) out64[e] = t;
        }
        __syncthreads();
    }
}

int nnf_launch_reduce_slabs(const float* slabs, int nslab, int64_t slab_stride, int rows, int64_t cols, int64_t lds,
                            float* out, int64_t ldo, hipStream_t st, double* out64) {
    const int64_t total = (int64_t)rows * cols;
    // enough threads to fill the chip: 2^lg parts per element when the output is small
    int lg = 0;
    while (lg < 4 && (total << lg) < ((int64_t)1 << 19) && (2 << lg) <= nslab) ++lg;
    if (lg > 0)
        return nnf_dispatch<4>(lg, [&](auto k) -> int {
            constexpr int P = 1 << decltype(k)::value;
            int64_t grid = nnf_cdiv(total, 256 / P);
            if (grid > 4096) grid = 4096;
            hipLaunchKernelGGL(nnf_reduce_slabs_par_kernel<P>, dim3((int)grid), dim3(256), 0, st, slabs, nslab, slab_stride, rows, cols,
                               lds, out, ldo, out64);
            NNF_CHECK_LAUNCH();
            return NNF_OK;
        });
    // (four columns per thread only when that still leaves enough threads to fill the chip: 20 vs 16 us at r x n = 1e5)
    if (out64 == nullptr && (lds & 3) == 0 && (slab_stride & 3) == 0 && (((uintptr_t)slabs) & 15) == 0 && total >= ((int64_t)1 << 21)) {
        const int64_t total4 = (int64_t)rows * ((cols + 3) >> 2);
        int grid4 = (int)((total4 + 255) / 256);
        if (grid4 > 2048) grid4 = 2048;
        hipLaunchKernelGGL(nnf_reduce_slabs4_kernel, dim3(grid4), dim3(256), 0, st, slabs, nslab, slab_stride, rows, cols, lds, out,
                           ldo);
        NNF_CHECK_LAUNCH();
        return NNF_OK;
    }
    int grid = (int)((total + 255) / 256);
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(nnf_reduce_slabs_kernel, dim3(grid), dim3(256), 0, st, slabs, nslab, slab_stride, rows, cols, lds,
                       out, ldo, out64);
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

// The error of sparse_obs_pow (nn_fac_amd/csrc/k_sparse_obs_pow.h) -- that function alone, not the kernels that call it -- against
// fp64 pow, in ulps of the fp32 result: 10^6 values of p, log-uniform in [1e-6, 1e3], at every exponent on the command line
// (default: -1.5 and -0.5, what beta = 0.5 asks of the observed-entries kernels).  One JSON line per exponent.  The K of
// tests/test_gpu_observed_kernels.py and DESIGN.md section 3 is twice the largest figure, rounded up.
//
//   hipcc --offload-arch=gfx950 -I nn_fac_amd/csrc tools/probes/obs_pow_probe.hip -o obs_pow_probe && ./obs_pow_probe [e ...]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>

#include "k_sparse_obs_pow.h"

__global__ void pow_kernel(const float* __restrict__ p, float e, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sparse_obs_pow(p[i], e);
}

#define OK(call)                                                                \
    do {                                                                        \
        if ((call) != hipSuccess) {                                             \
            fprintf(stderr, "obs_pow_probe: %s failed\n", #call);               \
            return 1;                                                           \
        }                                                                       \
    } while (0)

int main(int argc, char** argv) {
    const int n = 1000000;
    std::vector<double> exps;
    for (int a = 1; a < argc; ++a) exps.push_back(atof(argv[a]));
    if (exps.empty()) exps = {-1.5, -0.5};
    std::mt19937_64 gen(1);
    std::uniform_real_distribution<double> uni(log(1e-6), log(1e3));
    std::vector<float> p(n), got(n);
    for (int i = 0; i < n; ++i) p[i] = (float)exp(uni(gen));
    float *dp = nullptr, *dout = nullptr;
    OK(hipMalloc(&dp, n * sizeof(float)));
    OK(hipMalloc(&dout, n * sizeof(float)));
    OK(hipMemcpy(dp, p.data(), n * sizeof(float), hipMemcpyHostToDevice));
    for (double e : exps) {
        hipLaunchKernelGGL(pow_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dp, (float)e, dout, n);
        OK(hipGetLastError());
        OK(hipMemcpy(got.data(), dout, n * sizeof(float), hipMemcpyDeviceToHost));
        double worst = 0.0, at = 0.0, sum = 0.0;
        for (int i = 0; i < n; ++i) {
            const double want = pow((double)p[i], (double)(float)e);
            int ex = 0;
            frexp(want, &ex);                                    // want = f 2^ex, 1/2 <= f < 1: one ulp of fp32 is 2^(ex - 24)
            const double ulps = fabs((double)got[i] - want) / ldexp(1.0, ex - 24);
            sum += ulps;
            if (ulps > worst) worst = ulps, at = p[i];
        }
        printf("{\"probe\": \"obs_pow\", \"exponent\": %g, \"values\": %d, \"p_range\": [1e-6, 1e3], \"max_ulp\": %.3f, \"at_p\": %.9g, "
               "\"mean_ulp\": %.4f}\n", e, n, worst, at, sum / n);
    }
    (void)hipFree(dp);
    (void)hipFree(dout);
    return 0;
}

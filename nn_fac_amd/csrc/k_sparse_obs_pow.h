// The single-precision power of the observed-entries kernels (k_sparse_obs.hip) on its own, so that tools/probes/obs_pow_probe.hip
// measures this function and nothing else against fp64 pow: p^e = exp2(e log2 p) on the hardware transcendental units
// (v_log_f32, v_exp_f32: about 1 ulp each).  The error grows with |e log2 p| -- the product is rounded once before the exponential,
// and the logarithm's own ulp is scaled the same way: DESIGN.md section 3 has the largest error seen over p in [1e-6, 1e3].
// p = 0 gives 0 or +inf by the sign of e, p = +inf the other way round, NaN stays NaN.
#pragma once

__device__ __forceinline__ float sparse_obs_pow(float p, float e) { return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(p)); }

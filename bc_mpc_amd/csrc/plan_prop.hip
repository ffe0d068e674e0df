// plan_prop.hip -- proposals in the batched planners' population (gfx950).  The definition is
// bc_mpc_amd/proposals.py; the kernel matches it bit for bit.
//
// plan_sample_prop is plan_noise.hip's plan_sample_corr -- the same thread map, recursion, arithmetic and carried
// columns -- with one more copy branch: the LAST n_prop columns of every environment are given action sequences,
//
//   out[h][b * K + K - n_prop + p][j] = clip(prop[b * env_stride + p * seq_stride + h * step_stride + j])
//
// clipped by the samplers' own expression, so a NaN stays NaN and -0.0 against a bound of 0.0 stays -0.0.  A
// proposal column draws nothing: its Philox draws are simply unused and no index shifts, so every other column holds
// the bits plan_sample_corr writes there.  The source is read only, through three element strides, which covers the
// canonical [n_envs][P][H][A] and the policy engines' output [H][n_envs * P][A].  It is a unit of its own so that
// plan_noise.hip's kernels stay byte-identical.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "kernels.h"
#include "device_common.h"

namespace bcmpc {

__global__ __launch_bounds__(256) void plan_sample_prop(const PlanSamplePropArgs p) {
    const PlanSampleCorrArgs& a = p.s;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.Ktot * a.A) return;
    const int64_t col = i / a.A;
    const int j = (int)(i - col * a.A);
    const int64_t b = col / a.K, k = col - b * a.K;    // environment, column within it
    const int64_t step = a.Ktot * a.A;                 // out[h + 1][col][j] - out[h][col][j]
    const double lo = a.consts[6 * kConstCols + j], hi = a.consts[7 * kConstCols + j];
    if (k >= a.K - p.n_prop) {                         // a proposal: its clipped sequence, nothing drawn
        const double* src = p.prop + b * p.env_stride + (k - (a.K - p.n_prop)) * p.seq_stride + j;
        for (int h = 0; h < a.H; ++h) {
            const double v = src[(int64_t)h * p.step_stride];
            a.out[h * step + i] = v < lo ? lo : (v > hi ? hi : v);   // cem_action's clip
        }
        return;
    }
    if (a.keep) {
        int32_t n = a.keep_count[b];
        n = n < a.n_elite ? n : a.n_elite;
        if (k < n) {                                   // a carried elite: its stored sequence, nothing drawn
            const double* src = a.keep + ((b * a.n_elite + k) * a.H) * a.A + j;
            for (int h = 0; h < a.H; ++h) a.out[h * step + i] = src[(int64_t)h * a.A];
            return;
        }
    }
    const double* mu = a.mu + b * a.H * a.A + j;
    const double* sd = a.sigma + b * a.H * a.A + j;
    const uint64_t g = (uint64_t)(a.cand_offset + col);
    double n = 0.0;
    for (int h = 0; h < a.H; ++h) {
        const double z = cem_normal(a.seed, g, h, j, a.iter);
        n = h == 0 ? z : __dadd_rn(__dmul_rn(a.rho, n), __dmul_rn(a.c, z));
        const double v = __dadd_rn(mu[h * a.A], __dmul_rn(sd[h * a.A], n));
        a.out[h * step + i] = v < lo ? lo : (v > hi ? hi : v);   // cem_action's clip
    }
}

hipError_t launch_plan_sample_prop(const PlanSamplePropArgs& p, hipStream_t st) {
    const PlanSampleCorrArgs& a = p.s;
    if (a.K < 1 || a.Ktot < a.K || a.Ktot % a.K != 0 || a.H < 1 || a.A < 1 || a.A > BCMPC_MAX_ACTION)
        return hipErrorInvalidValue;
    if ((a.keep != nullptr) != (a.keep_count != nullptr) || (a.keep && a.n_elite < 1)) return hipErrorInvalidValue;
    if (!p.prop || p.n_prop < 1 || p.n_prop > a.K) return hipErrorInvalidValue;
    if (a.keep && (int64_t)p.n_prop + a.n_elite > a.K) return hipErrorInvalidValue;
    const int64_t blocks = (a.Ktot * a.A + 255) / 256;
    if (blocks < 1 || blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plan_sample_prop, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace bcmpc

// ensemble.hip -- the model ensemble's one device stage (gfx950): E cost vectors -> one value vector.
//
// An ensemble of E dynamics nets scores every candidate E times (one rollout launch per member, each into
// its row of member_costs[E][ld]).  ensemble_reduce_kernel turns the E costs of candidate k into the value
// v[k] the argmin / CEM select / MPPI update then read, under one of three rules (the NumPy
// definition is bc_mpc_amd/ensemble.py combine):
//
//   MEAN      t = c[0]; for e = 1..E-1: t = t + c[e]; v = t / E
//   MEAN_STD  m as above; q = 0.0; for e = 0..E-1: d = c[e] - m; q = q + d * d; v = m + kappa * sqrt(q / E)
//   WORST     np.maximum.reduce(c): w = c[0]; for e = 1..E-1: w = (w >= c[e] or w is NaN) ? w : c[e]
//
// every operation one rounded IEEE f64 operation (the unit is built with -ffp-contract=off; the division and
// the square root are the correctly rounded ones).  MEAN starts from c[0], so E == 1 returns c[0]'s bits.
//
// One lane per candidate: lanes are adjacent in k, so each member row is read coalesced (8 bytes per lane,
// 512 bytes per wave and row).  E is a run-time value <= BCMPC_MAX_MEMBERS: the member loop is unrolled over
// the maximum with a wave-uniform guard, all loads first, the arithmetic after them.  Tail lanes return.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "kernels.h"

namespace bcmpc {

__global__ __launch_bounds__(256) void ensemble_reduce_kernel(const EnsembleReduceArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.K) return;
    const int E = a.E;
    double c[BCMPC_MAX_MEMBERS];
#pragma unroll
    for (int e = 0; e < BCMPC_MAX_MEMBERS; ++e)
        if (e < E) c[e] = a.member_costs[(int64_t)e * a.ld + k];
    double v;
    if (a.mode == BCMPC_ENSEMBLE_WORST) {
        double w = c[0];
#pragma unroll
        for (int e = 1; e < BCMPC_MAX_MEMBERS; ++e)
            if (e < E) w = (w >= c[e] || w != w) ? w : c[e];
        v = w;
    } else {
        double t = c[0];
#pragma unroll
        for (int e = 1; e < BCMPC_MAX_MEMBERS; ++e)
            if (e < E) t = t + c[e];
        const double n = (double)E;
        const double m = __ddiv_rn(t, n);
        v = m;
        if (a.mode == BCMPC_ENSEMBLE_MEAN_STD) {
            double q = 0.0;
#pragma unroll
            for (int e = 0; e < BCMPC_MAX_MEMBERS; ++e)
                if (e < E) {
                    const double d = c[e] - m;
                    const double dd = d * d;
                    q = q + dd;
                }
            const double s = __dsqrt_rn(__ddiv_rn(q, n));
            const double ks = a.kappa * s;
            v = m + ks;
        }
    }
    a.out[k] = v;
}

hipError_t launch_ensemble_reduce(const EnsembleReduceArgs& a, hipStream_t st) {
    if (!a.member_costs || !a.out || a.K < 1 || a.ld < a.K || a.E < 1 || a.E > BCMPC_MAX_MEMBERS ||
        a.mode < BCMPC_ENSEMBLE_MEAN || a.mode > BCMPC_ENSEMBLE_WORST)
        return hipErrorInvalidValue;
    const int64_t blocks = (a.K + 255) / 256;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ensemble_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace bcmpc

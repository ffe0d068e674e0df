// plan_noise.hip -- what the batched planners sample (gfx950): temporally correlated noise and the CEM
// elite carry-over.  The definition is bc_mpc_amd/sampling.py; both kernels match it bit for bit.
//
// plan_batch.hip's plan_sample draws every stored action from an independent normal.  plan_sample_corr
// writes the same array [H][n_envs * K][A] from an AR(1) sequence over the horizon,
//
//   n[0] = z[0],   n[h] = rho * n[h-1] + c * z[h],   c = sqrt(1 - rho^2)   (two products, one add, no FMA)
//   out[h][col][j] = clip(mu[b][h][j] + sigma[b][h][j] * n[h])             (cem_action's arithmetic and clip)
//
// with z[h] = cem_normal(seed, cand_offset + col, h, j, iter), the draw plan_sample makes.  The variance of
// n[h] stays 1, so sigma keeps its meaning, and rho == 0 gives plan_sample's bits.  The rollout, argmin,
// refit and MPPI kernels read the stored array and do not change.
//
//   plan_sample_corr   one thread per (column, action dim): the H-step recursion in registers, one store per
//                      step; adjacent threads are adjacent in (column, j), so every step's stores of a wave are
//                      one contiguous run.  With a keep buffer, the first keep_count[b] columns of environment b
//                      are copied from it (the previous iteration's elites) and draw nothing.
//   plan_keep          one thread per (environment, elite record, h, j): copies the elites' sequences out of
//                      the stored array before the next plan_sample_corr overwrites it; every environment's first
//                      workgroup also counts its leading valid records (a minimum in LDS).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "kernels.h"
#include "device_common.h"

namespace bcmpc {

__global__ __launch_bounds__(256) void plan_sample_corr(const PlanSampleCorrArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.Ktot * a.A) return;
    const int64_t col = i / a.A;
    const int j = (int)(i - col * a.A);
    const int64_t b = col / a.K, k = col - b * a.K;    // environment, column within it
    const int64_t step = a.Ktot * a.A;                 // out[h + 1][col][j] - out[h][col][j]
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
    const double lo = a.consts[6 * kConstCols + j], hi = a.consts[7 * kConstCols + j];
    const uint64_t g = (uint64_t)(a.cand_offset + col);
    double n = 0.0;
    for (int h = 0; h < a.H; ++h) {
        const double z = cem_normal(a.seed, g, h, j, a.iter);
        n = h == 0 ? z : __dadd_rn(__dmul_rn(a.rho, n), __dmul_rn(a.c, z));
        const double v = __dadd_rn(mu[h * a.A], __dmul_rn(sd[h * a.A], n));
        a.out[h * step + i] = v < lo ? lo : (v > hi ? hi : v);   // cem_action's clip
    }
}

// environment b's record e names a column of b's own K columns of the stored array
__device__ __forceinline__ bool keep_column(const PlanKeepArgs& a, int64_t b, int e, int64_t& col) {
    const int64_t index = a.elite[b * a.n_elite + e].index;
    col = index - a.cand_offset;
    return index >= 0 && col >= b * a.K && col < (b + 1) * a.K;
}

__global__ __launch_bounds__(256) void plan_keep(const PlanKeepArgs a) {
    __shared__ int32_t first;                          // environment b's first record that is not carried
    const int64_t per = (int64_t)a.n_elite * a.H * a.A;             // values per environment
    const int64_t nblk = (per + 255) / 256;                         // workgroups per environment
    const int64_t b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    int32_t n = a.count[b];
    n = n < a.n_elite ? n : a.n_elite;
    int64_t col;
    const int64_t i = blk * 256 + threadIdx.x;
    if (i < per) {
        const int ha = a.H * a.A;
        const int e = (int)(i / ha), r = (int)(i - (int64_t)e * ha);
        const int h = r / a.A, j = r - h * a.A;
        if (e < n && keep_column(a, b, e, col)) a.keep[b * per + i] = a.actions[((int64_t)h * a.Ktot + col) * a.A + j];
    }
    if (blk != 0) return;                              // (uniform per workgroup)
    // the environment's first workgroup also counts the leading valid records: what the sampler carries
    if (threadIdx.x == 0) first = n > 0 ? n : 0;
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256)
        if (!keep_column(a, b, e, col)) atomicMin(&first, e);
    __syncthreads();
    if (threadIdx.x == 0) a.keep_count[b] = first;
}

static bool grid_ok(int64_t blocks) { return blocks >= 1 && blocks <= INT32_MAX; }

hipError_t launch_plan_sample_corr(const PlanSampleCorrArgs& a, hipStream_t st) {
    if (a.K < 1 || a.Ktot < a.K || a.Ktot % a.K != 0 || a.H < 1 || a.A < 1 || a.A > BCMPC_MAX_ACTION)
        return hipErrorInvalidValue;
    if ((a.keep != nullptr) != (a.keep_count != nullptr) || (a.keep && a.n_elite < 1)) return hipErrorInvalidValue;
    const int64_t blocks = (a.Ktot * a.A + 255) / 256;
    if (!grid_ok(blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plan_sample_corr, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_plan_keep(const PlanKeepArgs& a, hipStream_t st) {
    if (a.K < 1 || a.n_envs < 1 || a.Ktot != a.K * a.n_envs || a.n_elite < 1 || a.H < 1 || a.A < 1 ||
        a.A > BCMPC_MAX_ACTION)
        return hipErrorInvalidValue;
    const int64_t blocks = (((int64_t)a.n_elite * a.H * a.A + 255) / 256) * a.n_envs;
    if (!grid_ok(blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plan_keep, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace bcmpc

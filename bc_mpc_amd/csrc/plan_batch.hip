// plan_batch.hip -- batched CEM and MPPI (gfx950): n_envs environments x K candidates per launch chain,
// every environment with its own plan mu[b], sigma[b] ([H][A]), elite set, weighted mean and record.
//
// The rollout kernels read ONE sampling distribution per launch, so the batched step does not sample in
// them: plan_sample materialises the iteration's actions [H][n_envs * K][A] from the n_envs plans -- every
// value by cem_action (device_common.h), bit for bit what the rollout kernels draw for one environment --
// and the existing batched chain (batch.hip tile_states, then the rollout on per-candidate states) rolls
// that array out as an explicit action array.  Candidate column c = b * K + j belongs to environment b;
// its Philox index is cand_offset + c.
//
//   plan_sample        one thread per stored action.
//   plan_argmin        one 256-thread workgroup per environment: np.argmin (np.argmax for the learned
//                      reward) over this iteration's K costs, merged into the running record out[b] by
//                      ArgminArgs::merge's rule (argmin_common.h), best_index = iter * K + j; the winner's
//                      step-0 action is read from the stored array, so it must run before the next
//                      plan_sample overwrites it.
//   select_batch       select_kernel's body (cem_common.h), one 1024-thread workgroup per environment.
//   refit_batch        refit_kernel's body, one wave per (environment, h, j).
//   mppi_*_batch       the three stages of mppi.hip (mppi_common.h) with the environment as the slow grid
//                      index; workgroup size rule, partial counts and summation order are those of one
//                      update at m = K.
//
// The refit and the MPPI update read the stored array when they are given it (kernels.h RefitArgs::actions)
// instead of regenerating three Philox blocks per action; the values are the same bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "kernels.h"
#include "device_common.h"
#include "argmin_common.h"
#include "cem_common.h"
#include "mppi_common.h"

namespace bcmpc {

__global__ __launch_bounds__(256) void plan_sample(const PlanSampleArgs a) {
    const int64_t n = (int64_t)a.H * a.Ktot * a.A;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t row = i / a.A;                       // h * Ktot + c
    const int j = (int)(i - row * a.A);
    const int h = (int)(row / a.Ktot);
    const int64_t c = row - (int64_t)h * a.Ktot;
    const int64_t p = ((c / a.K) * a.H + h) * a.A + j; // environment c / K's (h, j)
    a.out[i] = cem_action(a.seed, (uint64_t)(a.cand_offset + c), h, j, a.iter, a.mu[p], a.sigma[p],
                          a.consts[6 * kConstCols + j], a.consts[7 * kConstCols + j]);
}

__global__ __launch_bounds__(256) void plan_argmin(const PlanArgminArgs a) {
    __shared__ double sc[4];
    __shared__ int64_t si[4];
    const int64_t c0 = (int64_t)blockIdx.x * a.K;      // the environment's first column
    Best best{__builtin_inf(), INT64_MAX};
    for (int64_t i = threadIdx.x; i < a.K; i += blockDim.x) {
        const double v = a.costs[c0 + i];
        const Best c{a.maximize ? -v : v, i};          // (environment-local index)
        if (better(c, best)) best = c;
    }
    best = block_best(best, sc, si);
    // the single-environment writer on the environment's own K columns of the stored step-0 actions
    ArgminArgs w{};
    w.actions = a.actions + c0 * a.A;
    w.consts = a.consts;
    w.out = a.out + blockIdx.x;
    w.K = a.K;
    w.A = a.A;
    w.maximize = a.maximize;
    w.merge = a.merge;
    w.pos_base = (int64_t)a.iter * a.K;
    w.cand_offset = w.pos_base;                        // (merge == 0: the writer adds cand_offset)
    argmin_write_block(w, best, sc, si);
}

__device__ __forceinline__ SelectArgs env_args(const SelectBatchArgs& a, int64_t b) {
    SelectArgs s = a.one;
    s.costs += b * s.m;
    s.index_base += b * s.m;
    s.out += b * s.n_elite;
    s.count += b;
    return s;
}

__device__ __forceinline__ RefitArgs env_args(const RefitBatchArgs& a, int64_t b) {
    RefitArgs r = a.one;
    const int64_t ha = (int64_t)r.H * r.A;
    r.elite += b * a.n_elite;
    r.count += b;
    r.mu += b * ha;
    r.sigma += b * ha;
    return r;
}

__device__ __forceinline__ MppiArgs env_args(const MppiBatchArgs& a, int64_t b) {
    MppiArgs m = a.one;
    const int64_t ha = (int64_t)m.H * m.A;
    m.costs += b * m.m;
    m.mu += b * ha;
    m.sigma += b * ha;
    m.pmin += b * kMppiMinParts;
    m.pcnt += b * kMppiMinParts;
    m.part += b * (ha + 2) * m.nparts;
    m.stats += b;
    m.cand_offset += b * m.m;
    return m;
}

__global__ __launch_bounds__(1024) void select_batch(const SelectBatchArgs a) { select_block(env_args(a, blockIdx.x)); }

template <bool STORED>
__global__ __launch_bounds__(64) void refit_batch(const RefitBatchArgs a) {
    const int ha = a.one.H * a.one.A;
    const int b = blockIdx.x / ha;
    refit_wave<STORED>(env_args(a, b), blockIdx.x - b * ha);
}

__global__ __launch_bounds__(256) void mppi_min_batch(const MppiBatchArgs a) {
    const int b = blockIdx.x / a.one.nmin;
    mppi_min_block(env_args(a, b), blockIdx.x - b * a.one.nmin);
}

template <bool STORED>
__global__ __launch_bounds__(kMppiThreads) void mppi_partial_batch(const MppiBatchArgs a) {
    const int64_t b = blockIdx.x / a.one.nparts;
    mppi_partial_block<STORED>(env_args(a, b), blockIdx.x - b * a.one.nparts);
}

__global__ __launch_bounds__(64) void mppi_final_batch(const MppiBatchArgs a) {
    const int per = a.one.H * a.one.A + 1;
    const int b = blockIdx.x / per;
    mppi_final_wave(env_args(a, b), blockIdx.x - b * per);
}

static bool grid_ok(int64_t blocks) { return blocks >= 1 && blocks <= INT32_MAX; }

hipError_t launch_plan_sample(const PlanSampleArgs& a, hipStream_t st) {
    if (a.K < 1 || a.Ktot < a.K || a.Ktot % a.K != 0 || a.H < 1 || a.A < 1 || a.A > BCMPC_MAX_ACTION)
        return hipErrorInvalidValue;
    const int64_t blocks = ((int64_t)a.H * a.Ktot * a.A + 255) / 256;
    if (!grid_ok(blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plan_sample, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_plan_argmin(const PlanArgminArgs& a, hipStream_t st) {
    if (a.K < 1 || a.n_envs < 1 || a.A < 0 || a.A > BCMPC_MAX_ACTION) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plan_argmin, dim3((unsigned)a.n_envs), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_select_batch(const SelectBatchArgs& a, hipStream_t st) {
    if (a.n_envs < 1 || a.one.m < 0 || a.one.n_elite < 1 || a.one.pairs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_batch, dim3((unsigned)a.n_envs), dim3(1024), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_refit_batch(const RefitBatchArgs& a, hipStream_t st) {
    const int64_t blocks = (int64_t)a.n_envs * a.one.H * a.one.A;
    if (a.n_envs < 1 || a.n_elite < 1 || !grid_ok(blocks)) return hipErrorInvalidValue;
    if (a.one.actions)
        hipLaunchKernelGGL(refit_batch<true>, dim3((unsigned)blocks), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL(refit_batch<false>, dim3((unsigned)blocks), dim3(64), 0, st, a);
    return hipGetLastError();
}

size_t mppi_batch_scratch(int64_t K, int32_t n_envs, int32_t HA) {
    return (size_t)n_envs * (2 * (size_t)kMppiMinParts + ((size_t)HA + 2) * (size_t)mppi_parts(K));
}

hipError_t launch_mppi_update_batch(const MppiBatchArgs& a, hipStream_t st) {
    const MppiArgs& m = a.one;
    const int64_t g1 = (int64_t)a.n_envs * m.nmin, g2 = (int64_t)a.n_envs * m.nparts,
                  g3 = (int64_t)a.n_envs * (m.H * m.A + 1);
    if (a.n_envs < 1 || m.m < 1 || m.nmin < 1 || m.nmin > kMppiMinParts || !grid_ok(g1) || !grid_ok(g2) || !grid_ok(g3))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mppi_min_batch, dim3((unsigned)g1), dim3(256), 0, st, a);
    if (m.actions)
        hipLaunchKernelGGL(mppi_partial_batch<true>, dim3((unsigned)g2), dim3(kMppiThreads), 0, st, a);
    else
        hipLaunchKernelGGL(mppi_partial_batch<false>, dim3((unsigned)g2), dim3(kMppiThreads), 0, st, a);
    hipLaunchKernelGGL(mppi_final_batch, dim3((unsigned)g3), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace bcmpc

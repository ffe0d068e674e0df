// batch.hip -- the batched control step's own kernels (gfx950): many environments per rollout launch.
//
// One engine of Ktot = n_envs * K candidates answers n_envs independent get_action calls in one launch
// chain.  Candidate column c = b * K + j belongs to environment b and starts from states[b]; its Philox
// index stays cand_offset + c, so environment b's columns are exactly the candidates a K-candidate
// engine rolls out at cand_offset + b * K.
//
//   tile_states      [n_envs][S] -> [Ktot][S]: row c is a copy of row c / K.  The rollout kernels then
//                    read per-candidate states (RolloutArgs::state_stride == S) unchanged.
//   argmin_segments  one 256-thread workgroup per environment: np.argmin (np.argmax for the learned
//                    reward) over costs[b*K .. (b+1)*K) with the total order of better(), then the
//                    record out[b] written as argmin_write_block writes the single-environment one.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "kernels.h"
#include "device_common.h"
#include "argmin_common.h"

namespace bcmpc {

__global__ __launch_bounds__(256) void tile_states(const TileStatesArgs a) {
    const int64_t n = a.Ktot * a.S;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t c = i / a.S;
    const int64_t d = i - c * a.S;
    a.out[i] = a.states[(c / a.K) * a.S + d];
}

__global__ __launch_bounds__(256) void argmin_segments(const SegmentArgminArgs a) {
    __shared__ double sc[4];
    __shared__ int64_t si[4];
    const int64_t c0 = (int64_t)blockIdx.x * a.K;      // the environment's first column
    Best best{__builtin_inf(), INT64_MAX};
    for (int64_t i = c0 + threadIdx.x; i < c0 + a.K; i += blockDim.x) {
        const double v = a.costs[i];
        const Best c{a.maximize ? -v : v, i};          // argmax(x) == argmin(-x), NaN-first and ties alike
        if (better(c, best)) best = c;
    }
    best = block_best(best, sc, si);
    // the record of environment blockIdx.x: the single-environment writer on the launch's column indices
    // (best.i is the column; the index written is cand_offset + column, the action actions[0][column]
    // or Philox at cand_offset + column)
    ArgminArgs w{};
    w.actions = a.actions;
    w.consts = a.consts;
    w.out = a.out + blockIdx.x;
    w.seed = a.seed;
    w.cand_offset = a.cand_offset;
    w.K = a.K * a.n_envs;
    w.A = a.A;
    w.maximize = a.maximize;
    argmin_write_block(w, best, sc, si);
}

hipError_t launch_tile_states(const TileStatesArgs& a, hipStream_t st) {
    if (a.K < 1 || a.Ktot < a.K || a.S < 1) return hipErrorInvalidValue;
    const int64_t blocks = (a.Ktot * a.S + 255) / 256;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_states, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_argmin_segments(const SegmentArgminArgs& a, hipStream_t st) {
    if (a.K < 1 || a.n_envs < 1 || a.A < 0 || a.A > BCMPC_MAX_ACTION) return hipErrorInvalidValue;
    hipLaunchKernelGGL(argmin_segments, dim3((unsigned)a.n_envs), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace bcmpc

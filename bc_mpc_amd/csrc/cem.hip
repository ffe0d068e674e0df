// cem.hip -- CEM outer loop kernels (DESIGN.md "CEM"): elite selection and the
// mean / std refit.  The per-iteration rollout is the ordinary rollout kernel
// with CEM action sampling (cem_action, device_common.h).
//
// select_kernel: the n_elite smallest records under the total order
//   (orderable(cost), index) -- NaN after every number, ties to the lower index,
//   i.e. np.argsort(costs, kind="stable")[:E] -- by an 8-pass radix select on the
//   64-bit orderable cost (LDS histograms), then an index-ordered compaction
//   (block scans), so the output is in ascending index order whatever the input
//   sharding.  One 1024-thread block; the input (K or ranks*E records, <= a few MB)
//   is re-read from L2 per pass.
//
// refit_kernel: one wave per (h, j).  Lane l regenerates the actions of elites
//   l, l+64, ... (Philox, no stored action tensor) and sums them in that order; the
//   64 partials are combined by the xor butterfly (offsets 32..1); mean = sum / n.
//   Second pass the same for (a - mean)^2; std = sqrt(var / n) (np.std, ddof 0).
//   mu' = alpha*mu + (1-alpha)*mean, sigma' likewise.  f64, no FMA, fixed order
//   (restated by oracle.cem_refit).
//
// Both bodies live in cem_common.h, shared with the per-environment kernels of plan_batch.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "cem_common.h"
#include "device_common.h"
#include "kernels.h"

namespace bcmpc {

__global__ __launch_bounds__(1024) void select_kernel(const SelectArgs a) { select_block(a); }

__global__ __launch_bounds__(64) void refit_kernel(const RefitArgs a) {
    refit_wave<false>(a, blockIdx.x);                  // b = h * A + j
}

hipError_t launch_select(const SelectArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_refit(const RefitArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(refit_kernel, dim3((unsigned)(a.H * a.A)), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace bcmpc

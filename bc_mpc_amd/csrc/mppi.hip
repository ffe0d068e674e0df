// mppi.hip -- the MPPI plan update (DESIGN.md "MPPI"): softmin weights over ALL candidates and the
// weighted mean of their [H][A] actions, regenerated from Philox (cem_action, device_common.h) like
// refit_kernel does for the elites -- no stored action tensor.  Three launches on one stream, the
// kernel boundaries are the only synchronisation (no atomics, no tickets):
//
// mppi_min_kernel: grid-stride over the m scores v = +-cost; every workgroup leaves the minimum of its
//   finite scores (+inf: none) and their count.  min and an integer count do not depend on the order.
//
// mppi_partial_kernel (stage 1): workgroup b owns the C = 64 * cpl candidates [b C, (b + 1) C).  Its
//   first C threads compute w = exp(-(v - v_min) / lambda) (0 for a non-finite score) ONCE per candidate
//   into LDS; wave 0 sums W and sum w^2; then wave q of the 16 takes the (h, j) pairs q, q + 16, ...:
//   lane l adds w a of its candidates l, l + 64, ... (ascending) and the 64 lane sums are combined by
//   the xor butterfly (offsets 32..1).  One partial per (value, workgroup), stored [value][workgroup].
//   The kernel is bound by the Philox integer multiplies (three blocks per action), not by its shape:
//   4, 8 or 16 waves and 64 / 128 / 256 candidates per workgroup measured 66-84 us per update at
//   K = 65,536, H = 20 (16 waves, 256 candidates: the fastest, DESIGN.md "MPPI").
//
// mppi_final_kernel (stage 2): one wave per (h, j) and one for the statistics.  Lane l adds the
//   workgroups' partials l, l + 64, ... in ascending order, then the xor butterfly; mu' = N / W.
//   Nothing is written to mu when no candidate is valid (the count is read on the device).
//
// f64, __dadd_rn / __dmul_rn / __ddiv_rn (no contraction), exp from the device library: the order of
// every sum is a function of (m, cpl) alone, so equal inputs give bit-equal outputs.
//
// The three bodies live in mppi_common.h, shared with the per-environment kernels of plan_batch.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "device_common.h"
#include "kernels.h"
#include "mppi_common.h"

namespace bcmpc {

__global__ __launch_bounds__(256) void mppi_min_kernel(const MppiArgs a) { mppi_min_block(a, blockIdx.x); }

__global__ __launch_bounds__(kMppiThreads) void mppi_partial_kernel(const MppiArgs a) {
    mppi_partial_block<false>(a, blockIdx.x);
}

__global__ __launch_bounds__(64) void mppi_final_kernel(const MppiArgs a) { mppi_final_wave(a, blockIdx.x); }

int mppi_cpl(int64_t m) { return m > kMppiSmall ? kMppiMaxCpl : 1; }
int64_t mppi_parts(int64_t m) {
    const int64_t C = 64 * mppi_cpl(m);
    return (m + C - 1) / C;
}
int mppi_min_blocks(int64_t m) { return (int)((m < 256 * (int64_t)kMppiMinParts ? m + 255 : 256 * (int64_t)kMppiMinParts) / 256); }

hipError_t launch_mppi_update(const MppiArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(mppi_min_kernel, dim3((unsigned)a.nmin), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mppi_partial_kernel, dim3((unsigned)a.nparts), dim3(kMppiThreads), 0, st, a);
    hipLaunchKernelGGL(mppi_final_kernel, dim3((unsigned)(a.H * a.A + 1)), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace bcmpc

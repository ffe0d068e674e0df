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

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "device_common.h"
#include "kernels.h"

namespace bcmpc {

constexpr int kMppiThreads = 64 * kMppiWaves;

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = __dadd_rn(s, __shfl_xor(s, off));
    return s;
}

__device__ __forceinline__ double wave_min(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = fmin(s, __shfl_xor(s, off));
    return s;
}

// minimum over the min kernel's per-workgroup minima (every lane gets it)
__device__ __forceinline__ double parts_min(const double* pmin, int nmin, int lane) {
    double vm = __builtin_inf();
    for (int i = lane; i < nmin; i += 64) vm = fmin(vm, pmin[i]);
    return wave_min(vm);
}

__global__ __launch_bounds__(256) void mppi_min_kernel(const MppiArgs a) {
    __shared__ double s_min[4];
    __shared__ long long s_cnt[4];
    double vm = __builtin_inf();
    long long n = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < a.m; k += (int64_t)gridDim.x * 256) {
        const double c = a.costs[k];
        const double v = a.maximize ? -c : c;
        if (__builtin_isfinite(v)) {
            vm = fmin(vm, v);
            ++n;
        }
    }
    vm = wave_min(vm);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_min[w] = vm; s_cnt[w] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.pmin[blockIdx.x] = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
        a.pcnt[blockIdx.x] = (int64_t)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
    }
}

__global__ __launch_bounds__(kMppiThreads) void mppi_partial_kernel(const MppiArgs a) {
    __shared__ double s_w[64 * kMppiMaxCpl];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int C = 64 * a.cpl;
    const int64_t base = (int64_t)blockIdx.x * C;
    const int64_t P = a.nparts;
    if (tid < C) {                                     // (whole waves: C is a multiple of 64)
        const double vmin = parts_min(a.pmin, a.nmin, lane);
        const int64_t k = base + tid;
        double w = 0.0;
        if (k < a.m) {
            const double c = a.costs[k];
            const double v = a.maximize ? -c : c;
            if (__builtin_isfinite(v)) w = exp(-__ddiv_rn(__dsub_rn(v, vmin), a.lambda));
        }
        s_w[tid] = w;
    }
    __syncthreads();
    const int HA = a.H * a.A;
    if (q == 0) {
        double sw = 0.0, sw2 = 0.0;
        for (int i = 0; i < a.cpl; ++i) {
            const double w = s_w[lane + 64 * i];
            sw = __dadd_rn(sw, w);
            sw2 = __dadd_rn(sw2, __dmul_rn(w, w));
        }
        sw = wave_sum(sw);
        sw2 = wave_sum(sw2);
        if (lane == 0) {
            a.part[(int64_t)HA * P + blockIdx.x] = sw;
            a.part[(int64_t)(HA + 1) * P + blockIdx.x] = sw2;
        }
    }
    for (int b = q; b < HA; b += kMppiWaves) {         // b = h * A + j
        const int h = b / a.A, j = b - h * a.A;
        const double mu0 = a.mu[b], sd0 = a.sigma[b];
        const double lo = a.consts[6 * kConstCols + j], hi = a.consts[7 * kConstCols + j];
        double s = 0.0;
        for (int i = 0; i < a.cpl; ++i) {
            const double w = s_w[lane + 64 * i];
            const int64_t k = base + lane + 64 * i;
            if (w != 0.0)                              // (k < m: candidates past the end have w == 0)
                s = __dadd_rn(s, __dmul_rn(w, cem_action(a.seed, (uint64_t)(a.cand_offset + k), h, j, a.iter,
                                                          mu0, sd0, lo, hi)));
        }
        s = wave_sum(s);
        if (lane == 0) a.part[(int64_t)b * P + blockIdx.x] = s;
    }
}

// lane l adds partials l, l + 64, ... of one value, then the butterfly
__device__ __forceinline__ double parts_sum(const double* p, int64_t n, int lane) {
    double s = 0.0;
    for (int64_t i = lane; i < n; i += 64) s = __dadd_rn(s, p[i]);
    return wave_sum(s);
}

__global__ __launch_bounds__(64) void mppi_final_kernel(const MppiArgs a) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int HA = a.H * a.A;
    const int64_t P = a.nparts;
    long long n = 0;
    for (int i = lane; i < a.nmin; i += 64) n += a.pcnt[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    const double W = parts_sum(a.part + (int64_t)HA * P, P, lane);
    if (b < HA) {
        const double N = parts_sum(a.part + (int64_t)b * P, P, lane);
        if (n > 0 && lane == 0) a.mu[b] = __ddiv_rn(N, W);   // no valid candidate: mu unchanged
        return;
    }
    const double S2 = parts_sum(a.part + (int64_t)(HA + 1) * P, P, lane);
    const double vmin = parts_min(a.pmin, a.nmin, lane);
    if (lane == 0) {
        bcmpc_mppi_stats st;
        st.weight_sum = n > 0 ? W : 0.0;
        st.ess = n > 0 ? __ddiv_rn(__dmul_rn(W, W), S2) : 0.0;
        st.min_cost = n > 0 ? (a.maximize ? -vmin : vmin) : __builtin_nan("");
        st.n_valid = n;
        *a.stats = st;
    }
}

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

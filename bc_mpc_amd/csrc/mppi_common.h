// mppi_common.h -- the bodies of the three MPPI update kernels, shared by the single-environment kernels
// (mppi.hip) and their per-environment forms (plan_batch.hip).  Every body takes its workgroup's index
// instead of reading blockIdx, so that environment b of a batched call sums in exactly the single update's
// order at m = K.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "cem_common.h"
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

// workgroup bx of a.nmin (256 threads): grid-stride minimum and count of the finite scores
__device__ __forceinline__ void mppi_min_block(const MppiArgs& a, int bx) {
    __shared__ double s_min[4];
    __shared__ long long s_cnt[4];
    double vm = __builtin_inf();
    long long n = 0;
    for (int64_t k = (int64_t)bx * 256 + threadIdx.x; k < a.m; k += (int64_t)a.nmin * 256) {
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
        a.pmin[bx] = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));
        a.pcnt[bx] = (int64_t)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
    }
}

// stage 1, workgroup bx of a.nparts (kMppiThreads threads); STORED: plan_action (cem_common.h)
template <bool STORED>
__device__ __forceinline__ void mppi_partial_block(const MppiArgs& a, int64_t bx) {
    __shared__ double s_w[64 * kMppiMaxCpl];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int C = 64 * a.cpl;
    const int64_t base = bx * C;
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
            a.part[(int64_t)HA * P + bx] = sw;
            a.part[(int64_t)(HA + 1) * P + bx] = sw2;
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
                s = __dadd_rn(s, __dmul_rn(w, plan_action<STORED>(a, a.cand_offset + k, h, j, mu0, sd0, lo, hi)));
        }
        s = wave_sum(s);
        if (lane == 0) a.part[(int64_t)b * P + bx] = s;
    }
}

// lane l adds partials l, l + 64, ... of one value, then the butterfly
__device__ __forceinline__ double parts_sum(const double* p, int64_t n, int lane) {
    double s = 0.0;
    for (int64_t i = lane; i < n; i += 64) s = __dadd_rn(s, p[i]);
    return wave_sum(s);
}

// stage 2, wave b of H * A + 1: (h, j) = b, or the statistics
__device__ __forceinline__ void mppi_final_wave(const MppiArgs& a, int b) {
    const int lane = threadIdx.x;
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

}  // namespace bcmpc

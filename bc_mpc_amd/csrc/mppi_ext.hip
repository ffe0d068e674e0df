// mppi_ext.hip -- what the MPPI update adds around the softmin weights (gfx950; DESIGN.md 9l, defined by
// bc_mpc_amd/mppi_update.py): the control-cost term lambda u^T Sigma^-1 eps before the update, and the weighted
// standard deviation about the updated mean after it.  Every kernel takes the environment as the slow grid index,
// as plan_batch.hip does (the single call is one environment), and reads the iteration's stored actions
// [H][n_envs * K][A] -- there is no Philox form: under correlated noise the stored array IS the sample.
//
// mppi_control_cost: one thread per candidate, 256 per workgroup.  The workgroup first computes the gain table
//   g[h][j] = mu / (sigma * sigma) (0 where sigma == 0) and a copy of mu into LDS -- one f64 divide per (h, j)
//   and workgroup, none per element -- then every thread walks h and its A contiguous doubles (a wave reads
//   64 A 8 contiguous bytes per step): q += g (a - mu), a sequential chain in the definition's order, and writes
//   c~ = cost +- weight q.  No atomics, no cross-lane operation.
//
// mppi_ext_min: mppi_min_block (mppi_common.h) on the score vector: the sigma update recomputes the minimum and
//   the count itself, so it needs no scratch of an earlier call.
//
// mppi_sigma_partial: mppi_partial_block's shape.  Workgroup b owns C = 64 cpl candidates (mppi_cpl(K)); its
//   first C threads compute the update's weights -- the same expression on the same v_min, the same bits -- once
//   into LDS; wave 0 sums W; wave q of the 16 takes the (h, j) pairs q, q + 16, ..: lane l adds w (a - mu')^2 of
//   its candidates l, l + 64, .. (ascending), then the xor butterfly.  One partial per (value, workgroup).
//
// mppi_sigma_final: one wave per (environment, h, j): the partials of V[h][j] and of W in parts_sum's order,
//   s = sqrt(V / W), sigma' = min(max(alpha sigma + (1 - alpha) s, min_std), max_std).  Nothing is written when
//   no candidate is valid.
//
// f64, __dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn (no contraction): the order of every sum is a
// function of K alone, so equal inputs give bit-equal outputs and environment b of a batch sums as a single call.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "device_common.h"
#include "kernels.h"
#include "mppi_common.h"

namespace bcmpc {

constexpr int kCtrlThreads = 256;

__global__ __launch_bounds__(kCtrlThreads) void mppi_control_cost(const MppiControlArgs a) {
    extern __shared__ double s_tab[];                  // [HA] g, then [HA] mu
    const int HA = a.H * a.A;
    const int64_t b = blockIdx.x / a.bpe;              // the environment
    const int64_t k = (int64_t)(blockIdx.x - b * a.bpe) * kCtrlThreads + threadIdx.x;
    double* s_g = s_tab;
    double* s_mu = s_tab + HA;
    for (int p = threadIdx.x; p < HA; p += kCtrlThreads) {
        const double m = a.mu[b * HA + p], s = a.sigma[b * HA + p];
        s_g[p] = s == 0.0 ? 0.0 : __ddiv_rn(m, __dmul_rn(s, s));
        s_mu[p] = m;
    }
    __syncthreads();
    if (k >= a.K) return;
    const int64_t c = b * a.K + k;                     // the candidate's column
    double q = 0.0;
    for (int h = 0; h < a.H; ++h) {
        const double* row = a.actions + ((int64_t)h * a.Ktot + c) * a.A;
        const int p0 = h * a.A;
        for (int j = 0; j < a.A; ++j) q = __dadd_rn(q, __dmul_rn(s_g[p0 + j], __dsub_rn(row[j], s_mu[p0 + j])));
    }
    const double wq = __dmul_rn(a.weight, q);
    const double cost = a.costs[c];
    a.out[c] = a.maximize ? __dsub_rn(cost, wq) : __dadd_rn(cost, wq);
}

// environment b's view of the update's argument block: what mppi_min_block and the weights read
__device__ __forceinline__ MppiArgs env_args(const MppiSigmaArgs& a, int64_t b) {
    MppiArgs m{};
    m.costs = a.scores + b * a.K;
    m.pmin = a.pmin + b * kMppiMinParts;
    m.pcnt = a.pcnt + b * kMppiMinParts;
    m.m = a.K;
    m.nmin = a.nmin;
    m.maximize = a.maximize;
    return m;
}

__global__ __launch_bounds__(256) void mppi_ext_min(const MppiSigmaArgs a) {
    const int b = blockIdx.x / a.nmin;
    mppi_min_block(env_args(a, b), blockIdx.x - b * a.nmin);
}

__global__ __launch_bounds__(kMppiThreads) void mppi_sigma_partial(const MppiSigmaArgs a) {
    __shared__ double s_w[64 * kMppiMaxCpl];
    const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
    const int64_t P = a.nparts;
    const int64_t b = blockIdx.x / P, bx = blockIdx.x - b * P;
    const int C = 64 * a.cpl;
    const int64_t base = bx * C;
    const int HA = a.H * a.A;
    const double* scores = a.scores + b * a.K;
    double* part = a.part + b * (HA + 1) * P;
    if (tid < C) {                                     // (whole waves: C is a multiple of 64)
        const double vmin = parts_min(a.pmin + b * kMppiMinParts, a.nmin, lane);
        const int64_t k = base + tid;
        double w = 0.0;
        if (k < a.K) {
            const double c = scores[k];
            const double v = a.maximize ? -c : c;
            if (__builtin_isfinite(v)) w = exp(-__ddiv_rn(__dsub_rn(v, vmin), a.lambda));   // (mppi_partial_block's line)
        }
        s_w[tid] = w;
    }
    __syncthreads();
    if (q == 0) {
        double sw = 0.0;
        for (int i = 0; i < a.cpl; ++i) sw = __dadd_rn(sw, s_w[lane + 64 * i]);
        sw = wave_sum(sw);
        if (lane == 0) part[(int64_t)HA * P + bx] = sw;
    }
    const double* acts = a.actions + (b * a.K + base) * a.A;   // the workgroup's first column, step 0
    for (int p = q; p < HA; p += kMppiWaves) {         // p = h * A + j
        const int h = p / a.A, j = p - h * a.A;
        const double m = a.mu_new[b * HA + p];
        const double* col = acts + (int64_t)h * a.Ktot * a.A + j;
        double s = 0.0;
        for (int i = 0; i < a.cpl; ++i) {
            const double w = s_w[lane + 64 * i];
            if (w != 0.0) {                            // (k < K: candidates past the end have w == 0)
                const double d = __dsub_rn(col[(int64_t)(lane + 64 * i) * a.A], m);
                s = __dadd_rn(s, __dmul_rn(w, __dmul_rn(d, d)));
            }
        }
        s = wave_sum(s);
        if (lane == 0) part[(int64_t)p * P + bx] = s;
    }
}

__global__ __launch_bounds__(64) void mppi_sigma_final(const MppiSigmaArgs a) {
    const int lane = threadIdx.x;
    const int HA = a.H * a.A;
    const int64_t P = a.nparts;
    const int b = blockIdx.x / HA, p = blockIdx.x - b * HA;
    const int64_t* pcnt = a.pcnt + (int64_t)b * kMppiMinParts;
    const double* part = a.part + (int64_t)b * (HA + 1) * P;
    long long n = 0;
    for (int i = lane; i < a.nmin; i += 64) n += pcnt[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    const double W = parts_sum(part + (int64_t)HA * P, P, lane);
    const double V = parts_sum(part + (int64_t)p * P, P, lane);
    if (n > 0 && lane == 0) {                          // no valid candidate: sigma unchanged
        const double s = __dsqrt_rn(__ddiv_rn(V, W));
        const double beta = __dsub_rn(1.0, a.alpha);
        double x = __dadd_rn(__dmul_rn(a.alpha, a.sigma[(int64_t)b * HA + p]), __dmul_rn(beta, s));
        x = x < a.min_std ? a.min_std : x;             // (np.maximum / np.minimum: a NaN stays)
        x = x > a.max_std ? a.max_std : x;
        a.sigma[(int64_t)b * HA + p] = x;
    }
}

static bool grid_ok(int64_t blocks) { return blocks >= 1 && blocks <= INT32_MAX; }

size_t mppi_control_lds(int32_t HA) { return 2 * (size_t)HA * sizeof(double); }

hipError_t launch_mppi_control_cost(const MppiControlArgs& a, hipStream_t st) {
    const int64_t blocks = (int64_t)a.n_envs * a.bpe;
    const size_t lds = mppi_control_lds(a.H * a.A);
    if (a.n_envs < 1 || a.K < 1 || a.Ktot != a.K * a.n_envs || a.bpe != (a.K + kCtrlThreads - 1) / kCtrlThreads ||
        a.H < 1 || a.A < 1 || a.A > BCMPC_MAX_ACTION || lds > kMppiControlMaxLds || !grid_ok(blocks))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mppi_control_cost, dim3((unsigned)blocks), dim3(kCtrlThreads), lds, st, a);
    return hipGetLastError();
}

size_t mppi_sigma_scratch(int64_t K, int32_t n_envs, int32_t HA) {
    return (size_t)n_envs * (2 * (size_t)kMppiMinParts + ((size_t)HA + 1) * (size_t)mppi_parts(K));
}

hipError_t launch_mppi_sigma_update(const MppiSigmaArgs& a, hipStream_t st) {
    const int64_t g1 = (int64_t)a.n_envs * a.nmin, g2 = (int64_t)a.n_envs * a.nparts,
                  g3 = (int64_t)a.n_envs * a.H * a.A;
    if (a.n_envs < 1 || a.K < 1 || a.Ktot != a.K * a.n_envs || a.nmin != mppi_min_blocks(a.K) ||
        a.cpl != mppi_cpl(a.K) || a.nparts != mppi_parts(a.K) || a.H < 1 || a.A < 1 || a.A > BCMPC_MAX_ACTION ||
        !grid_ok(g1) || !grid_ok(g2) || !grid_ok(g3))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mppi_ext_min, dim3((unsigned)g1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(mppi_sigma_partial, dim3((unsigned)g2), dim3(kMppiThreads), 0, st, a);
    hipLaunchKernelGGL(mppi_sigma_final, dim3((unsigned)g3), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace bcmpc

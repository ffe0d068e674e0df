// cem_common.h -- the bodies of the CEM selection and refit kernels, shared by the single-environment
// kernels (cem.hip) and their per-environment forms (plan_batch.hip): one body, so that environment b of a
// batched call orders and sums exactly as the single call does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "device_common.h"
#include "kernels.h"

namespace bcmpc {

// total order on f64 (NaN greatest, -0 == +0), as an unsigned key
__device__ __forceinline__ uint64_t orderable(double c) {
    if (c != c) return ~0ull;
    if (c == 0.0) c = 0.0;                             // -0 == +0, as np.argsort compares them
    const uint64_t b = __double_as_longlong(c);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// exclusive prefix sum of one flag per thread over the 1024-thread block, and the total
__device__ __forceinline__ int block_scan(int flag, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t bal = __ballot(flag);
    const int inwave = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int k = 0; k < 16; ++k) {
        const int v = wsum[k];
        before += k < w ? v : 0;
        total += v;
    }
    __syncthreads();                                   // wsum is reused by the next call
    return before + inwave;
}

// One 1024-thread block selects a.n_elite of a's m records (select_kernel, cem.hip).
__device__ __forceinline__ void select_block(const SelectArgs& a) {
    __shared__ uint32_t hist[256];
    __shared__ int wsum[16];
    __shared__ uint64_t s_prefix;
    __shared__ int64_t s_remaining;
    __shared__ uint32_t s_valid;
    const int tid = threadIdx.x;

    auto rec = [&](int64_t i, uint64_t& key, int64_t& idx, double& cost) -> bool {
        if (a.pairs) {
            cost = a.pairs[i].cost;
            idx = a.pairs[i].index;
        } else {
            cost = a.costs[i];
            idx = a.index_base + i;
        }
        key = orderable(a.maximize ? -cost : cost);
        return idx >= 0;
    };

    if (tid == 0) { s_valid = 0; s_prefix = 0; }
    __syncthreads();
    {   // count valid records
        uint32_t n = 0;
        for (int64_t i = tid; i < a.m; i += blockDim.x) {
            uint64_t k; int64_t ix; double c;
            n += rec(i, k, ix, c) ? 1u : 0u;
        }
        atomicAdd(&s_valid, n);
    }
    __syncthreads();
    const int64_t E = a.n_elite < (int64_t)s_valid ? a.n_elite : (int64_t)s_valid;
    if (tid == 0) s_remaining = E;
    uint64_t mask = 0;
    for (int pass = 0; pass < 8 && E > 0; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int i = tid; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        const uint64_t prefix = s_prefix;
        for (int64_t i = tid; i < a.m; i += blockDim.x) {
            uint64_t k; int64_t ix; double c;
            if (rec(i, k, ix, c) && (k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {                                // digit where the cumulative count reaches `remaining`
            int64_t rem = s_remaining, cum = 0;
            int d = 0;
            for (; d < 256; ++d) {
                if (cum + hist[d] >= rem) break;
                cum += hist[d];
            }
            s_remaining = rem - cum;
            s_prefix = prefix | ((uint64_t)d << shift);
        }
        mask |= 255ull << shift;
        __syncthreads();
    }
    // threshold key T; take every record below T and the first `need_eq` (by index) equal to T
    const uint64_t T = s_prefix;
    const int64_t need_eq = s_remaining;
    int64_t base = 0, eq_taken = 0;
    for (int64_t tile = 0; tile < a.m && E > 0; tile += blockDim.x) {
        const int64_t i = tile + tid;
        uint64_t k = 0; int64_t ix = -1; double c = 0.0;
        const bool v = i < a.m && rec(i, k, ix, c);
        const int is_eq = v && k == T;
        int tot_eq;
        const int eq_rank = block_scan(is_eq, wsum, tot_eq);
        const int sel = (v && k < T) || (is_eq && eq_taken + eq_rank < need_eq);
        int tot_sel;
        const int pos = block_scan(sel, wsum, tot_sel);
        if (sel) a.out[base + pos] = bcmpc_elite{c, ix};
        base += tot_sel;
        eq_taken += tot_eq;
    }
    for (int64_t i = E + tid; i < a.n_elite; i += blockDim.x) a.out[i] = bcmpc_elite{__builtin_nan(""), -1};
    if (tid == 0) *a.count = (int32_t)E;
}

// The sampled action (h, j) of global candidate g at iteration a.iter.  STORED: read from the iteration's
// materialised array a.actions [H][a.act_cols][A] (column g - a.act_g0; plan_batch.hip's sampling kernel
// wrote cem_action's value there, so the bits are the same); a candidate outside the array, and every
// candidate when !STORED, is regenerated from Philox.
template <bool STORED, class Args>
__device__ __forceinline__ double plan_action(const Args& a, int64_t g, int h, int j, double mu, double sd,
                                              double lo, double hi) {
    if constexpr (STORED) {
        const int64_t col = g - a.act_g0;
        if (col >= 0 && col < a.act_cols) return a.actions[((int64_t)h * a.act_cols + col) * a.A + j];
    }
    return cem_action(a.seed, (uint64_t)g, h, j, a.iter, mu, sd, lo, hi);
}

// One wave refits (h, j) = (b / A, b % A) of a's distribution from its elites (refit_kernel, cem.hip).
template <bool STORED>
__device__ __forceinline__ void refit_wave(const RefitArgs& a, int b) {
    const int h = b / a.A, j = b - h * a.A;
    const int lane = threadIdx.x;
    const int n = *a.count;
    if (n <= 0) return;                                // nothing selected: distribution unchanged
    const double mu0 = a.mu[b], sd0 = a.sigma[b];
    const double lo = a.consts[6 * kConstCols + j], hi = a.consts[7 * kConstCols + j];
    double s = 0.0;
    for (int e = lane; e < n; e += 64)
        s = __dadd_rn(s, plan_action<STORED>(a, a.elite[e].index, h, j, mu0, sd0, lo, hi));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = __dadd_rn(s, __shfl_xor(s, off));
    const double mean = __ddiv_rn(s, (double)n);
    double v = 0.0;
    for (int e = lane; e < n; e += 64) {
        const double d = __dsub_rn(plan_action<STORED>(a, a.elite[e].index, h, j, mu0, sd0, lo, hi), mean);
        v = __dadd_rn(v, __dmul_rn(d, d));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off));
    const double sd = __dsqrt_rn(__ddiv_rn(v, (double)n));
    if (lane == 0) {
        const double beta = __dsub_rn(1.0, a.alpha);
        a.mu[b] = __dadd_rn(__dmul_rn(a.alpha, mu0), __dmul_rn(beta, mean));
        a.sigma[b] = __dadd_rn(__dmul_rn(a.alpha, sd0), __dmul_rn(beta, sd));
    }
}

}  // namespace bcmpc

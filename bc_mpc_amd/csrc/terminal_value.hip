// terminal_value.hip -- a learned terminal value added to the candidates' costs (gfx950).
//
// v[k] = V(states[k]) for the critic the reference trains beside its policy (ppo_bc_policy.py:56-64, pi/vf):
//   obz = clip((f32(s) - ob_mean) / ob_std, -5, 5);  h = tanh(h W + b) x L;  v = h w_final + b_final
// and, in the same launch, costs[k] = costs[k] + weight * (double)v[k] (with termination steps given: only where
// term_step[k] == horizon, the candidate that never terminated; values[k] is written either way) -- the stage
// between "cost vector" and "argmin / select / update" of an engine with a value set (capi.cpp rollout_impl).
// The definition is bc_mpc_amd/value.py terminal_values; obz is bit-identical to it (one f64 -> f32 conversion, one f32 subtract,
// one correctly rounded f32 divide, a clip by compares so that NaN stays NaN), the dense layers are f32 fma
// chains on v_mfma_f32_16x16x4_f32 with tanh_fast (device_common.h), no f16 anywhere.
//
// Layout: the transposed MLP of rollout.hip.  A wave owns 16 candidates as MFMA columns; a layer is
// D[neuron][cand] = W^T X with the weights as the A operand, packed once per weight version by pack_layer
// (pack.cpp) in blocks of TB output tiles, so the accumulators of output tile t ARE the B fragments of k-steps
// 4t .. 4t + 3 of the next layer: activations never leave the lane's registers (no LDS slab: at hidden 256
// the 16 input tiles and the 16 output tiles are 128 VGPRs of the 512 a one-wave-per-SIMD block may hold).
// The hidden width is padded to HP = 16 T, T in {1, 2, 4, 8, 16}, with zero weights and biases; the input
// layer to two k-tiles (S <= 32); the final layer is one more tile of which row 0 is live.
// Weights stream from L2 as 1-KiB fragments (one f4 per lane); the four waves of a workgroup walk the same
// stream and share it through the CU's L1.  ob_mean, ob_std and the biases are staged in LDS once per block.
//
// Tail: a partial last column computes on the clamped row K - 1 and stores nothing; a wave whose 16
// candidates are all past K leaves after the staging barrier.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/bcmpc.h"
#include "kernels.h"
#include "device_common.h"

namespace bcmpc {

namespace {

// waves (16-candidate columns) per workgroup: at cfg3 2 and 4 measure alike, 8 is 5% slower
#ifndef BCMPC_TV_WAVES
#define BCMPC_TV_WAVES 4
#endif
constexpr int kTvWaves = BCMPC_TV_WAVES;

// one dense layer [TIN tiles -> TOUT tiles] of the wave's 16 columns: y = act(W^T x + b)
template <int TIN, int TOUT, int TB, bool ACT>
__device__ __forceinline__ void tv_dense(const f4* __restrict__ w, const float (&x)[TIN][4], const float* bias,
                                         float (&y)[TOUT][4], int lane) {
    static_assert(TOUT % TB == 0, "TOUT must be a multiple of TB");
    const int q = lane >> 4;
#pragma unroll
    for (int tb = 0; tb < TOUT / TB; ++tb) {
        f4 acc[TB];
#pragma unroll
        for (int j = 0; j < TB; ++j) acc[j] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < TIN; ++u) {
            f4 wv[TB];
#pragma unroll
            for (int j = 0; j < TB; ++j) wv[j] = w[((tb * TIN + u) * TB + j) * 64 + lane];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < TB; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[j][r], x[u][r], acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const int t = tb * TB + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc[j][r] + bias[16 * t + 4 * q + r];        // BiasAdd (f32), then tanh
                y[t][r] = ACT ? tanh_fast(v) : v;
            }
        }
    }
}

template <int T>
__global__ __launch_bounds__(kTvWaves * 64) void terminal_value_kernel(const TerminalValueArgs a) {
    constexpr int HP = 16 * T;
    constexpr int TB = T < 4 ? T : 4;
    __shared__ float P[kTvParamFloats];
    const int L = a.L;
    const int np = 64 + L * HP + 16;                         // <= kTvParamFloats (launch_terminal_value)
    for (int i = threadIdx.x; i < np; i += blockDim.x) P[i] = a.params[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, m = lane & 15;
    const int64_t col0 = ((int64_t)blockIdx.x * kTvWaves + wave) * 16;
    if (col0 >= a.K) return;                                 // (no barrier follows)
    const int64_t cand = col0 + m;
    const bool valid = cand < a.K;
    const int64_t row = valid ? cand : a.K - 1;

    // obz of the lane's input rows d = 16 v + 4 q + r (0 on the padded rows)
    float x0[2][4];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * v + 4 * q + r;
            float z = 0.f;
            if (d < a.S) {
                const float x = (float)a.states[row * a.row_stride + d];
                z = __fdiv_rn(__fsub_rn(x, P[d]), P[32 + d]);
                z = z < -5.0f ? -5.0f : (z > 5.0f ? 5.0f : z);            // np.clip: NaN stays NaN
            }
            x0[v][r] = z;
        }

    float x[T][4], y[T][4];
    tv_dense<2, T, TB, true>(a.w[0], x0, P + 64, x, lane);
#pragma unroll 1
    for (int l = 1; l < L; ++l) {
        tv_dense<T, T, TB, true>(a.w[l], x, P + 64 + l * HP, y, lane);
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) x[t][r] = y[t][r];
    }
    float o[1][4];
    tv_dense<T, 1, 1, false>(a.w[L], x, P + 64 + L * HP, o, lane);
    if (valid && q == 0) {                                   // row 0 of the final tile: lane group 0, r = 0
        const float v = o[0][0];
        if (a.values) a.values[cand] = v;
        // (a terminated candidate has no future return: its total is left as it is, not "+ weight * 0")
        if (a.costs && (!a.term_step || a.term_step[cand] == a.horizon))
            a.costs[cand] = __dadd_rn(a.costs[cand], __dmul_rn(a.weight, (double)v));
    }
}

template <int T>
hipError_t launch_t(const TerminalValueArgs& a, unsigned blocks, hipStream_t st) {
    hipLaunchKernelGGL((terminal_value_kernel<T>), dim3(blocks), dim3(kTvWaves * 64), 0, st, a);
    return hipGetLastError();
}

}  // namespace

int terminal_value_padded(int hidden) {
    for (int hp : {16, 32, 64, 128, 256})
        if (hidden >= 1 && hidden <= hp) return hp;
    return -1;
}

hipError_t launch_terminal_value(const TerminalValueArgs& a, hipStream_t st) {
    if (!a.states || !a.params || a.K < 1 || a.S < 1 || a.S > BCMPC_MAX_STATE || a.row_stride < a.S || a.L < 1 ||
        a.L > BCMPC_VALUE_MAX_LAYERS || !std::isfinite(a.weight))
        return hipErrorInvalidValue;
    for (int l = 0; l <= a.L; ++l)
        if (!a.w[l]) return hipErrorInvalidValue;
    const int64_t blocks = (a.K + kTvWaves * 16 - 1) / (kTvWaves * 16);
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    switch (a.HP) {
        case 16: return launch_t<1>(a, (unsigned)blocks, st);
        case 32: return launch_t<2>(a, (unsigned)blocks, st);
        case 64: return launch_t<4>(a, (unsigned)blocks, st);
        case 128: return launch_t<8>(a, (unsigned)blocks, st);
        case 256: return launch_t<16>(a, (unsigned)blocks, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace bcmpc

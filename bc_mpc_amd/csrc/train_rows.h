// train_rows.h -- the device helpers the three row-block trainers share (fit.hip, ac_fit.hip, ac_ppo.hip): the
// MFMA row-tile GEMM of a 16-row workgroup, the DPP wave sum and one element of TF1 ApplyAdam.  Every function is
// inlined into its kernel; a change here moves all three units' kernels together (tools/kernel_digest.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace bcmpc::rows {

typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kWaves = 16;                  // waves of the row-block workgroup
constexpr int kFK = 8;                      // k-steps (of 4) per weight chunk
constexpr int kFRing = 4;                   // weight chunks in flight per wave
constexpr int kPK = 32;                     // batch steps (of 4) per load batch of a weight-gradient tile

// one chunk of kFK k-steps of the B operand through a buffer descriptor: one 32-bit lane offset
// (vo) for the whole GEMM, the chunk position in the scalar offset; rows past the matrix and the
// masked columns (vo beyond the range) read 0
__device__ __forceinline__ void rows_load(float* b, __amdgpu_buffer_rsrc_t rsrc, int vo, int kb, int kstride) {
#pragma unroll
    for (int s = 0; s < kFK; ++s)
        b[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, vo, (kb + 4 * s) * kstride, 0));
}

__device__ __forceinline__ f4v rows_mma(f4v acc, const float* b, const float* X, int kb, int K, int r16, int k4,
                                        int lds) {
#pragma unroll
    for (int s = 0; s < kFK; ++s) {
        const int k = kb + 4 * s + k4;
        const float x = k < K ? X[r16 * lds + k] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x, b[s], acc, 0, 0, 0);
    }
    return acc;
}

// Every weight load of a GEMM has been consumed by its end, but the compiler's wait analysis cannot
// see it through the conditional prefetches and keeps them "pending": the row phase after the GEMM
// then gets vmcnt(0) waits at register reuse -- which also wait for that phase's own global stores,
// a full HBM write trip (~2 us) per phase.  A real s_waitcnt vmcnt(0) here (nothing is in flight by
// then) clears the analysis.
__device__ __forceinline__ void rows_drained() {
    __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
}

// acc += sum over k in [k0, k1) of X[r][k] W[k*ldw + n] for this lane's column n (a 16-wide tile),
// kFRing chunks of weights in flight
__device__ __forceinline__ f4v rows_tile(f4v acc, const float* X, int k0, int k1, __amdgpu_buffer_rsrc_t rsrc,
                                         int vo, int ldw, int r16, int k4, int lds) {
    constexpr int CK = 4 * kFK;
    float ring[kFRing][kFK];
#pragma unroll
    for (int j = 0; j < kFRing; ++j)
        if (k0 + j * CK < k1) rows_load(ring[j], rsrc, vo, k0 + j * CK, 4 * ldw);
    for (int kb = k0; kb < k1; kb += kFRing * CK) {
#pragma unroll
        for (int j = 0; j < kFRing; ++j) {
            const int kc = kb + j * CK;
            if (kc < k1) {
                acc = rows_mma(acc, ring[j], X, kc, k1, r16, k4, lds);
                if (kc + kFRing * CK < k1) rows_load(ring[j], rsrc, vo, kc + kFRing * CK, 4 * ldw);
            }
        }
    }
    return acc;
}

// C[r][n] = sum_k X[r][k] W[k*ldw + n] (+ bias[n]) for the 16 LDS rows X (stride lds), n < N, W row-major
// [K][ldw].  16-column tiles over the 16 waves; with at most 8 tiles (N <= 128: an output layer, a narrow
// hidden layer) the K range is split over the idle waves and the partials (LDS, `kp`, [kWaves][256]) are added
// in wave order.
__device__ __forceinline__ void rows_gemm(const float* X, int K, const float* __restrict__ W, int ldw, int N,
                                          const float* __restrict__ bias, float* C, int lds, float* kp) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r16 = lane & 15, k4 = lane >> 4;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, K * ldw * 4, 0x00020000);
    const int nt = (N + 15) / 16;
    if (nt * 2 > kWaves) {
        for (int n0 = 16 * wv; n0 < N; n0 += 16 * kWaves) {
            const int n = n0 + r16;
            const int vo = n < N ? (k4 * ldw + n) * 4 : 0x40000000;
            const float bv = bias && n < N ? bias[n] : 0.f;          // requested before the weights
            f4v acc = rows_tile((f4v){0.f, 0.f, 0.f, 0.f}, X, 0, K, rsrc, vo, ldw, r16, k4, lds);
            rows_drained();
            if (n < N)
#pragma unroll
                for (int r = 0; r < 4; ++r) C[(4 * k4 + r) * lds + n] = bias ? acc[r] + bv : acc[r];
        }
        return;
    }
    // K split: wave wv takes tile wv % nt, K slice wv / nt of ks (whole 4-k-steps)
    const int ks = kWaves / nt;
    const int t = wv % nt, q = wv / nt;
    const int n = 16 * t + r16;
    if (q < ks) {
        const int kq = ((K + 4 * ks - 1) / (4 * ks)) * 4;       // slice length, multiple of 4
        const int k0 = min(K, q * kq), k1 = min(K, k0 + kq);
        const int vo = n < N ? (k4 * ldw + n) * 4 : 0x40000000;
        f4v acc = (f4v){0.f, 0.f, 0.f, 0.f};
        if (k0 < k1) acc = rows_tile(acc, X, k0, k1, rsrc, vo, ldw, r16, k4, lds);
        rows_drained();
#pragma unroll
        for (int r = 0; r < 4; ++r) kp[(q * nt + t) * 256 + (4 * k4 + r) * 16 + r16] = acc[r];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * nt * 16; i += 64 * kWaves) {
        const int tt = i / 256, e = i % 256, r = e / 16, c = 16 * tt + e % 16;
        if (c < N) {
            float s = 0.f;
            for (int qq = 0; qq < ks; ++qq) s += kp[(qq * nt + tt) * 256 + e];
            C[r * lds + c] = bias ? s + bias[c] : s;
        }
    }
}

// wave sum without the LDS crossbar: DPP butterflies inside each 16-lane row (quad_perm xor 1, xor 2,
// row_ror 4, 8), then the four row totals in a fixed order (deterministic, wave-uniform)
template <int CTRL>
__device__ __forceinline__ float dpp_t(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float wave_sum_fast(float v) {
    v += dpp_t<0xB1>(v);                    // quad_perm [1,0,3,2]
    v += dpp_t<0x4E>(v);                    // quad_perm [2,3,0,1]
    v += dpp_t<0x124>(v);                   // row_ror 4
    v += dpp_t<0x128>(v);                   // row_ror 8
    const int b = __builtin_bit_cast(int, v);
    return (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)) +
            __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16))) +
           (__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)) +
            __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48)));
}

// TF1 ApplyAdam on element i from operands loaded earlier: m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2);
// w -= (m lr_t) / (sqrt(v) + eps), the division and the square root correctly rounded; returns the new w
__device__ __forceinline__ float adam_elem(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                           size_t i, float gi, float w0, float m0, float v0, float lr_t, float b1,
                                           float b2, float eps) {
    const float mi = m0 + (gi - m0) * (1.0f - b1);
    const float vi = v0 + (gi * gi - v0) * (1.0f - b2);
    const float wi = w0 - __fdiv_rn(mi * lr_t, __fsqrt_rn(vi) + eps);
    m[i] = mi;
    v[i] = vi;
    w[i] = wi;
    return wi;
}

}  // namespace bcmpc::rows

// ac_fit.hip -- the actor-critic fitter on the GPU (include/bcmpc.h bcmpc_acfit_*): Adam on one head of the
// reference's MlpPolicy, the BC distillation loss sqrt(mean((ac - ac_mean(ob))^2)) (ppo_bc_policy.py:114,
// update_op_bc) or the critic regression mean((vpred - ret)^2) (ppo_bc_policy.py:108), restated as explicit
// forward / backward kernels in f32.  bc_mpc_amd/ac_fit.py is the definition (operation order of the loss
// gradients, TF1 ApplyAdam); tests/test_gpu_ac_fit.py holds these kernels to it.
//
// One Adam step is two launches, the structure of fit.hip's fused step without LayerNorm:
//   acfit_rows_kernel    one workgroup per 16 batch rows: the gather by host-drawn indices, the observation
//                        filter and clip, every forward layer (MFMA row-tile GEMM + tanh in LDS), the output,
//                        the loss partial, dP, and every backward data gradient -- all row-local given the
//                        weights, so no workgroup waits for another;
//   acfit_params_kernel  one workgroup per 16 x 16 weight tile (the bias is the tile row k == in, fed by a
//                        column of ones): the batch sum in a fixed order, then TF1 ApplyAdam in place and the
//                        transposed copy the next step's backward GEMMs read; one more workgroup finishes the
//                        loss and advances the step counter.
// The policy head's gradient carries the global scalar (0.5 / loss) / N.  The backward pass is linear in dP, so
// the row kernel propagates the unscaled residual -(2 d) and every parameter workgroup forms the loss from the
// row blocks' partials in one fixed order and scales its tile's batch sum before Adam: no third launch, no
// grid-wide barrier, no workgroup waits for another.  The kernel boundary is the only global synchronisation.
// At loss == 0 the scalar is inf and every sum is 0: NaN parameters, as TF's SqrtGrad gives.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../include/bcmpc.h"
#include "ac_fit_internal.h"
#include "ac_fit_plan.h"
#include "train_rows.h"

namespace bcmpc::acfit {

using rows::adam_elem;                      // the row-tile GEMM, the wave sum and Adam: train_rows.h
using rows::f4v;
using rows::kPK;
using rows::rows_gemm;
using rows::wave_sum_fast;
static_assert(rows::kWaves == kWaves, "the plan's LDS layout and the row GEMM agree on the workgroup's waves");

struct Args {
    const double* obs; const double* tgt;               // the data [n][S], [n][N]
    const int64_t* idx_base; int32_t stride; int32_t* iter;
    const float* filt;                                  // [2][32] ob_mean, ob_std
    float* w; float* wt; float* m; float* v;            // params, transposed kernel copy, Adam slots
    int32_t w_off[BCMPC_ACFIT_MAX_LAYERS + 1], b_off[BCMPC_ACFIT_MAX_LAYERS + 1];
    float* x0; float* dp;                               // obz [Bcap][S], dP [Bcap][N]
    float* act; float* dzs;                             // [L][Bcap][h]
    float* loss_part; float* loss; float* bp; const float* lr;
    const Tile* tiles;
    int32_t B, Bcap, S, N, L, h, head, ld;
    float b1, b2, eps;
};

__global__ __launch_bounds__(1024) void acfit_rows_kernel(const Args a) {
    extern __shared__ float sm[];
    const int ld = a.ld, S = a.S, N = a.N, L = a.L, h = a.h;
    float* bufA = sm;                       // [16][ld]: the current layer input / backward operand
    float* bufB = bufA + kRows * ld;        // [16][ld]: GEMM output
    float* tsm = bufB + kRows * ld;         // [16][16] targets
    float* red = tsm + kRows * kTgtLd;      // [kWaves] loss partials per wave
    float* kp = red + kWaves;               // [kWaves][256] K-split partials
    float* acache = kp + kWaves * 256;      // [L][16][ld] activation rows A_l
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r0 = blockIdx.x * kRows;
    const int nr = min(kRows, a.B - r0);
    const int it = *a.iter;
    const int64_t* idx = a.idx_base + (int64_t)it * a.stride;
    if (blockIdx.x == 0 && tid == 0 && it > 0) {          // the previous step's finish (AdamOptimizer._finish)
        a.bp[0] = __fmul_rn(a.bp[0], a.b1);
        a.bp[1] = __fmul_rn(a.bp[1], a.b2);
    }
    // ---- gather: obz = clip((f32(ob) - mean) / std, -5, 5) in f32, targets fed as f32 ----
    for (int i = tid; i < kRows * (S + N); i += 64 * kWaves) {
        const int r = i / (S + N), c = i % (S + N);
        float val = 0.f;
        if (r < nr) {
            const int64_t row = idx[r0 + r];
            if (c < S) {
                const float x = (float)a.obs[row * S + c];
                val = __fdiv_rn(__fsub_rn(x, a.filt[c]), a.filt[32 + c]);
                val = val < -5.0f ? -5.0f : (val > 5.0f ? 5.0f : val);
            } else {
                val = (float)a.tgt[row * N + c - S];
            }
        }
        if (c < S) {
            bufA[r * ld + c] = val;
            if (r < nr) a.x0[(size_t)(r0 + r) * S + c] = val;
        } else {
            tsm[r * kTgtLd + c - S] = val;
        }
    }
    __syncthreads();
    const size_t BH = (size_t)a.Bcap * h;
    // ---- forward: one row per wave after each GEMM ----
    for (int l = 0; l < L; ++l) {
        rows_gemm(bufA, l == 0 ? S : h, a.w + a.w_off[l], h, h, a.w + a.b_off[l], bufB, ld, kp);
        __syncthreads();
        {
            const int r = wv;
            const float* z = bufB + r * ld;
            float* hx = bufA + r * ld;
            float* ac = acache + (l * kRows + r) * ld;
            const size_t go = (size_t)l * BH + (size_t)(r0 + r) * h;
#pragma unroll 4
            for (int f = lane; f < h; f += 64) {
                const float v = tanhf(z[f]);
                hx[f] = v;
                ac[f] = v;
                if (r < nr) a.act[go + f] = v;
            }
        }
        __syncthreads();
    }
    // ---- output, loss partial, dP ----
    rows_gemm(bufA, h, a.w + a.w_off[L], N, N, a.w + a.b_off[L], bufB, ld, kp);
    __syncthreads();
    const float inv = 1.0f / (float)(a.B * N);
    float sl = 0.f;
    for (int i = tid; i < kRows * N; i += 64 * kWaves) {
        const int r = i / N, c = i % N;
        float g = 0.f;
        if (r < nr) {
            const float pv = bufB[r * ld + c], tv = tsm[r * kTgtLd + c];
            if (a.head == BCMPC_ACFIT_POLICY) {
                const float d = tv - pv;                  // ac - mean
                sl += d * d;
                g = -(d * 2.0f);                          // unscaled: acfit_params_kernel applies (0.5 / loss) / N
            } else {
                const float d = pv - tv;                  // vpred - ret
                sl += d * d;
                g = inv * (d * 2.0f);
            }
            a.dp[(size_t)(r0 + r) * N + c] = g;
        }
        bufA[r * ld + c] = g;
    }
    sl = wave_sum_fast(sl);
    if (lane == 0) red[wv] = sl;
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int w = 0; w < kWaves; ++w) t += red[w];
        a.loss_part[blockIdx.x] = t;
    }
    // ---- backward data gradients: dH_l = dZ_{l+1} W_{l+1}^T, dZ_l = dH_l (1 - A_l^2) ----
    for (int l = L - 1; l >= 0; --l) {
        const int out = l + 1 == L ? N : h;                 // dZ_{l+1} width; W_{l+1}^T is [out][h]
        rows_gemm(bufA, out, a.wt + a.w_off[l + 1], h, h, nullptr, bufB, ld, kp);
        __syncthreads();
        {
            const int r = wv;
            const float* dh = bufB + r * ld;
            float* dz = bufA + r * ld;
            const float* av = acache + (l * kRows + r) * ld;
            const size_t go = (size_t)l * BH + (size_t)(r0 + r) * h;
#pragma unroll 4
            for (int f = lane; f < h; f += 64) {
                const float avv = av[f];
                const float dzv = r < nr ? dh[f] * (1.0f - avv * avv) : 0.f;
                if (r < nr) a.dzs[go + f] = dzv;
                dz[f] = dzv;
            }
        }
        __syncthreads();
    }
}

// one workgroup per task; its 4 waves take contiguous quarters of the batch and their partials are added in
// wave order (deterministic)
__global__ __launch_bounds__(256) void acfit_params_kernel(const Args a) {
    __shared__ float tp[4][4][64];          // weight-tile partials per wave
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int B = a.B, S = a.S, N = a.N, L = a.L, h = a.h;
    const size_t BH = (size_t)a.Bcap * h;
    const Tile tl = a.tiles[blockIdx.x];
    const int l = tl.layer;
    // the loss from the row blocks' partials, in block order: the same bits in every workgroup
    const int nblk = (B + kRows - 1) / kRows;
    float tot = 0.f;
    for (int k = 0; k < nblk; ++k) tot += a.loss_part[k];
    const float msq = tot * (1.0f / (float)(B * N));
    const float loss = a.head == BCMPC_ACFIT_POLICY ? __fsqrt_rn(msq) : msq;
    if (tl.kind == 3) {
        if (threadIdx.x == 0) {
            const int it = *a.iter;
            a.loss[it] = loss;
            *a.iter = it + 1;
        }
        return;
    }
    // policy head: the scalar of SqrtGrad and MeanGrad, (0.5 / loss) / N (inf at loss == 0)
    const float scale = a.head == BCMPC_ACFIT_POLICY ? __fdiv_rn(__fdiv_rn(0.5f, loss), (float)(B * N)) : 1.0f;
    const float lr_t = __fdiv_rn(__fmul_rn(*a.lr, __fsqrt_rn(__fsub_rn(1.0f, a.bp[1]))), __fsub_rn(1.0f, a.bp[0]));
    // dW_l[k][n] = sum_b Hin[b][k] dZ[b][n], row k == in of the tile: the bias (Hin = 1)
    // (A = Hin^T: lane (k = r16, b = k4); B = dZ: (b = k4, n = r16))
    const int in = l == 0 ? S : h, out = l == L ? N : h;
    const float* Hin = l == 0 ? a.x0 : a.act + (size_t)(l - 1) * BH;
    const float* dZ = l == L ? a.dp : a.dzs + (size_t)l * BH;
    const int r16 = lane & 15, k4 = lane >> 4;
    const int k = tl.k0 + r16, n = tl.n0 + r16;
    // this lane's Adam operands (wave 0 updates), requested with the gradient operands
    float w0[4], m0[4], v0[4];
    size_t pi[4];
    if (wv == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = tl.k0 + 4 * k4 + r;
            pi[r] = kk < in ? (size_t)a.w_off[l] + (size_t)kk * out + n : (size_t)a.b_off[l] + n;
            const bool ok = kk <= in && n < out;
            w0[r] = ok ? a.w[pi[r]] : 0.f;
            m0[r] = ok ? a.m[pi[r]] : 0.f;
            v0[r] = ok ? a.v[pi[r]] : 0.f;
        }
    const int q0 = (B * wv) / 4, q1 = (B * (wv + 1)) / 4;
    f4v acc = (f4v){0.f, 0.f, 0.f, 0.f};
    for (int bb = q0; bb < q1; bb += 4 * kPK) {
        float x[kPK], y[kPK];
#pragma unroll
        for (int s = 0; s < kPK; ++s) {
            const int b = bb + 4 * s + k4;
            x[s] = b < q1 ? (k < in ? Hin[(size_t)b * in + k] : (k == in ? 1.f : 0.f)) : 0.f;
            y[s] = (b < q1 && n < out) ? dZ[(size_t)b * out + n] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < kPK; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[s], y[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) tp[wv][r][lane] = acc[r];
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float gsum = ((tp[0][r][lane] + tp[1][r][lane]) + tp[2][r][lane]) + tp[3][r][lane];
            if (a.head == BCMPC_ACFIT_POLICY) gsum = gsum * scale;
            const int kk = tl.k0 + 4 * k4 + r;
            if (kk <= in && n < out) {
                const float wn = adam_elem(a.w, a.m, a.v, pi[r], gsum, w0[r], m0[r], v0[r], lr_t, a.b1, a.b2, a.eps);
                if (kk < in && l > 0) a.wt[(size_t)a.w_off[l] + (size_t)n * in + kk] = wn;   // W^T copy
            }
        }
    }
}

}  // namespace bcmpc::acfit

using namespace bcmpc::acfit;
namespace train = bcmpc::train;

// ------------------------------------------------------------------ C ABI ---
namespace bcmpc::acfit {

// activation buffers for batches of up to `rows` rows (no run is in flight: bcmpc_acfit_run synchronises)
bool acfit_reserve(bcmpc_acfit* f, int32_t rows) {
    if (rows <= f->bcap) return true;
    f->graph.drop();
    const Plan& p = f->plan;
    const size_t B = (size_t)rows, nblk = (B + kRows - 1) / kRows;
    return train::grow(&f->bcap, rows, {{&f->d_x0, B * p.S * 4}, {&f->d_dp, B * p.N * 4},
                                        {&f->d_act, (size_t)p.L * B * p.h * 4},
                                        {&f->d_dzs, (size_t)p.L * B * p.h * 4}, {&f->d_lpart, nblk * 4}});
}

}  // namespace bcmpc::acfit

extern "C" {

int bcmpc_acfit_is_graph(const bcmpc_acfit* f) { return f && f->last_graph ? f->graph.captures : 0; }

int bcmpc_acfit_create(const bcmpc_acfit_config* c, bcmpc_acfit** out) {
    if (!c || !out) return fail(BCMPC_ERR_ARG, "null argument");
    *out = nullptr;
    Plan plan;
    if (const int rc = make_plan(c, &plan)) return rc;            // every refusal, before any HIP call
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || c->device >= ndev)
        return fail(BCMPC_ERR_ARG, "device ordinal out of range");
    if (hipSetDevice(c->device) != hipSuccess) return fail(BCMPC_ERR_HIP, "hipSetDevice failed");
    bcmpc_acfit* f = new bcmpc_acfit();
    f->plan = std::move(plan);
    const Plan& p = f->plan;
    const size_t np = p.n_params;
    bool ok = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc(&f->d_w, np * 4) == hipSuccess && hipMalloc(&f->d_wt, np * 4) == hipSuccess &&
              hipMalloc(&f->d_m, np * 4) == hipSuccess && hipMalloc(&f->d_v, np * 4) == hipSuccess &&
              hipMalloc(&f->d_filt, 64 * 4) == hipSuccess && hipMalloc(&f->d_state, 4 * 4) == hipSuccess &&
              hipMalloc(&f->d_iter, 4) == hipSuccess &&
              hipMalloc(&f->d_tiles, p.tiles.size() * sizeof(Tile)) == hipSuccess &&
              hipMemcpy(f->d_tiles, p.tiles.data(), p.tiles.size() * sizeof(Tile), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(f->d_m, 0, np * 4) == hipSuccess && hipMemset(f->d_v, 0, np * 4) == hipSuccess &&
              hipMemset(f->d_wt, 0, np * 4) == hipSuccess && acfit_reserve(f, c->batch_size) &&
              (p.lds_words * 4 <= 65536 ||
               hipFuncSetAttribute((const void*)acfit_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(p.lds_words * 4)) == hipSuccess);
    if (!ok) { bcmpc_acfit_destroy(f); return fail(BCMPC_ERR_HIP, "device allocation failed"); }
    f->h_state[0] = c->beta1;
    f->h_state[1] = c->beta2;
    *out = f;
    return BCMPC_OK;
}

int bcmpc_acfit_destroy(bcmpc_acfit* f) {
    if (!f) return BCMPC_OK;
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    f->graph.drop();
    for (void* p : {(void*)f->d_w, (void*)f->d_wt, (void*)f->d_m, (void*)f->d_v, (void*)f->d_x0, (void*)f->d_dp,
                    (void*)f->d_act, (void*)f->d_dzs, (void*)f->d_lpart, (void*)f->d_filt, (void*)f->d_state,
                    (void*)f->d_iter, (void*)f->d_tiles, (void*)f->d_obs, (void*)f->d_tgt, (void*)f->d_idx,
                    (void*)f->d_loss})
        if (p) (void)hipFree(p);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
    return BCMPC_OK;
}

int bcmpc_acfit_set_params(bcmpc_acfit* f, const float* const* kernels, const float* const* biases) {
    if (!f || !kernels || !biases) return fail(BCMPC_ERR_ARG, "null argument");
    const Plan& p = f->plan;
    std::vector<float> hw(p.n_params, 0.f), hwt(p.n_params, 0.f);
    for (int l = 0; l <= p.L; ++l) {
        const size_t in = p.lin[l], o = p.lout[l];
        if (!kernels[l] || !biases[l]) return fail(BCMPC_ERR_ARG, "null kernel / bias");
        std::copy(kernels[l], kernels[l] + in * o, hw.begin() + p.w_off[l]);
        std::copy(biases[l], biases[l] + o, hw.begin() + p.b_off[l]);
        if (l > 0)                                        // W_l^T [out][in] at the same offset (the backward GEMMs)
            for (size_t i = 0; i < in; ++i)
                for (size_t j = 0; j < o; ++j) hwt[p.w_off[l] + j * in + i] = hw[p.w_off[l] + i * o + j];
    }
    if (hipSetDevice(p.cfg.device) != hipSuccess ||
        hipMemcpyAsync(f->d_w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, f->stream) != hipSuccess ||
        hipMemcpyAsync(f->d_wt, hwt.data(), hwt.size() * 4, hipMemcpyHostToDevice, f->stream) != hipSuccess ||
        hipStreamSynchronize(f->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "parameter upload failed");
    f->has_weights = true;
    return BCMPC_OK;
}

int bcmpc_acfit_get_params(bcmpc_acfit* f, float* const* kernels, float* const* biases) {
    if (!f || !kernels || !biases) return fail(BCMPC_ERR_ARG, "null argument");
    if (!f->has_weights) return fail(BCMPC_ERR_STATE, "bcmpc_acfit_set_params has not been called");
    const Plan& p = f->plan;
    std::vector<float> hw(p.n_params);
    if (hipSetDevice(p.cfg.device) != hipSuccess ||
        hipMemcpyAsync(hw.data(), f->d_w, hw.size() * 4, hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
        hipStreamSynchronize(f->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "parameter download failed");
    for (int l = 0; l <= p.L; ++l) {
        if (!kernels[l] || !biases[l]) return fail(BCMPC_ERR_ARG, "null kernel / bias");
        std::copy(hw.begin() + p.w_off[l], hw.begin() + p.w_off[l] + (size_t)p.lin[l] * p.lout[l], kernels[l]);
        std::copy(hw.begin() + p.b_off[l], hw.begin() + p.b_off[l] + p.lout[l], biases[l]);
    }
    return BCMPC_OK;
}

int bcmpc_acfit_set_filter(bcmpc_acfit* f, const float* ob_mean, const float* ob_std) {
    if (!f) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = check_filter(ob_mean, ob_std, f->plan.S)) return rc;
    float hf[64];
    filter_image(ob_mean, ob_std, f->plan.S, hf);
    if (hipSetDevice(f->plan.cfg.device) != hipSuccess ||
        hipMemcpyAsync(f->d_filt, hf, sizeof(hf), hipMemcpyHostToDevice, f->stream) != hipSuccess ||
        hipStreamSynchronize(f->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "filter upload failed");
    f->has_filter = true;
    return BCMPC_OK;
}

int bcmpc_acfit_set_data(bcmpc_acfit* f, const double* obs, const double* targets, int64_t n) {
    if (!f || n < 0 || (n > 0 && (!obs || !targets))) return fail(BCMPC_ERR_ARG, "bad argument");
    const Plan& p = f->plan;
    if (hipSetDevice(p.cfg.device) != hipSuccess) return fail(BCMPC_ERR_HIP, "hipSetDevice failed");
    if (n > f->data_cap) {
        f->graph.drop();                                  // the graph holds the data buffers' addresses
        f->n_data = 0;
        if (!train::grow(&f->data_cap, n, {{&f->d_obs, (size_t)n * p.S * 8}, {&f->d_tgt, (size_t)n * p.N * 8}}))
            return fail(BCMPC_ERR_HIP, "data buffer allocation failed");
    }
    if (n > 0 &&
        (hipMemcpyAsync(f->d_obs, obs, (size_t)n * p.S * 8, hipMemcpyHostToDevice, f->stream) != hipSuccess ||
         hipMemcpyAsync(f->d_tgt, targets, (size_t)n * p.N * 8, hipMemcpyHostToDevice, f->stream) != hipSuccess ||
         hipStreamSynchronize(f->stream) != hipSuccess))
        return fail(BCMPC_ERR_HIP, "data upload failed");
    f->n_data = n;
    return BCMPC_OK;
}

}  // extern "C"

namespace bcmpc::acfit {

// one Adam step: 2 launches
int acfit_step(bcmpc_acfit* f, hipStream_t stream, const int64_t* d_idx, int stride, int B) {
    const Plan& p = f->plan;
    Args a{};
    a.obs = f->d_obs; a.tgt = f->d_tgt;
    a.idx_base = d_idx; a.stride = stride; a.iter = f->d_iter; a.filt = f->d_filt;
    a.w = f->d_w; a.wt = f->d_wt; a.m = f->d_m; a.v = f->d_v;
    for (int l = 0; l <= p.L; ++l) { a.w_off[l] = p.w_off[l]; a.b_off[l] = p.b_off[l]; }
    a.x0 = f->d_x0; a.dp = f->d_dp; a.act = f->d_act; a.dzs = f->d_dzs;
    a.loss_part = f->d_lpart; a.loss = f->d_loss; a.bp = f->d_state; a.lr = f->d_state + 2;
    a.tiles = f->d_tiles;
    a.B = B; a.Bcap = f->bcap; a.S = p.S; a.N = p.N; a.L = p.L; a.h = p.h; a.head = p.cfg.head; a.ld = p.ld;
    a.b1 = p.cfg.beta1; a.b2 = p.cfg.beta2; a.eps = p.cfg.epsilon;
    hipLaunchKernelGGL(acfit_rows_kernel, dim3((B + kRows - 1) / kRows), dim3(64 * kWaves), p.lds_words * 4,
                       stream, a);
    if (hipGetLastError() != hipSuccess) return fail(BCMPC_ERR_HIP, "acfit_rows_kernel launch failed");
    hipLaunchKernelGGL(acfit_params_kernel, dim3((unsigned)p.tiles.size()), dim3(256), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return fail(BCMPC_ERR_HIP, "acfit_params_kernel launch failed");
    return BCMPC_OK;
}

int acfit_prepare(bcmpc_acfit* f, hipStream_t stream, const int64_t* indices, int64_t total, int32_t bmax,
                  int32_t iterations, float learning_rate) {
    if (hipSetDevice(f->plan.cfg.device) != hipSuccess) return fail(BCMPC_ERR_HIP, "hipSetDevice failed");
    if (!acfit_reserve(f, bmax)) return fail(BCMPC_ERR_HIP, "activation buffer allocation failed");
    if (!train::grow(&f->idx_cap, total, {{&f->d_idx, (size_t)total * 8}}))
        return fail(BCMPC_ERR_HIP, "index buffer allocation failed");
    if (hipMemcpyAsync(f->d_idx, indices, (size_t)total * 8, hipMemcpyHostToDevice, stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "index upload failed");
    if (!train::grow(&f->loss_cap, iterations, {{&f->d_loss, (size_t)iterations * 4}}))
        return fail(BCMPC_ERR_HIP, "loss buffer allocation failed");
    // device step state: counter 0, the host mirror's beta powers, this run's learning rate
    f->h_state[2] = learning_rate;
    if (hipMemsetAsync(f->d_iter, 0, 4, stream) != hipSuccess ||
        hipMemcpyAsync(f->d_state, f->h_state, 12, hipMemcpyHostToDevice, stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "step state upload failed");
    return BCMPC_OK;
}

int acfit_finish(bcmpc_acfit* f, hipStream_t stream, int32_t iterations, float* losses) {
    if (losses && hipMemcpyAsync(losses, f->d_loss, (size_t)iterations * 4, hipMemcpyDeviceToHost, stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "loss download failed");
    if (hipStreamSynchronize(stream) != hipSuccess) return fail(BCMPC_ERR_HIP, "fit failed");
    for (int i = 0; i < iterations; ++i) {       // host mirror of the device beta powers (same f32 products)
        f->h_state[0] *= f->plan.cfg.beta1;
        f->h_state[1] *= f->plan.cfg.beta2;
    }
    return BCMPC_OK;
}

// the steps of a run: a uniform run as one captured graph (a single chain of kernel nodes on one stream),
// anything else launched step by step
static int acfit_enqueue(bcmpc_acfit* f, const int32_t* batch_sizes, int32_t iterations) {
    bool uniform = true;
    for (int i = 1; i < iterations; ++i) uniform = uniform && batch_sizes[i] == batch_sizes[0];
    const char* ge = std::getenv("BCMPC_ACFIT_GRAPH");
    const bool use_graph = uniform && !(ge && ge[0] == '0');
    if (use_graph) {
        const intptr_t key[train::GraphRun::kKey] = {iterations, batch_sizes[0], (intptr_t)f->d_idx,
                                                     (intptr_t)f->d_loss};
        const int rc = f->graph.run(f->stream, key, fail, [&] {
            int rs = BCMPC_OK;
            for (int i = 0; i < iterations && rs == BCMPC_OK; ++i)
                rs = acfit_step(f, f->stream, f->d_idx, batch_sizes[0], batch_sizes[0]);
            return rs;
        });
        if (rc != BCMPC_OK) return rc;
    } else {
        int64_t pos = 0;
        for (int i = 0; i < iterations; ++i) {
            const int rc = acfit_step(f, f->stream, f->d_idx + pos, 0, batch_sizes[i]);
            if (rc != BCMPC_OK) return rc;
            pos += batch_sizes[i];
        }
    }
    f->last_graph = use_graph;
    return BCMPC_OK;
}

}  // namespace bcmpc::acfit

extern "C" int bcmpc_acfit_run(bcmpc_acfit* f, const int64_t* indices, const int32_t* batch_sizes, int32_t iterations,
                               float learning_rate, float* losses) {
    if (!f) return fail(BCMPC_ERR_ARG, "null argument");
    int64_t total = 0;
    int32_t bmax = 0;
    if (const int rc = check_run(indices, batch_sizes, iterations, learning_rate, f->n_data, &total, &bmax)) return rc;
    if (!f->has_weights) return fail(BCMPC_ERR_STATE, "bcmpc_acfit_set_params has not been called");
    if (!f->has_filter) return fail(BCMPC_ERR_STATE, "bcmpc_acfit_set_filter has not been called");
    if (iterations == 0) return BCMPC_OK;
    if (const int rc = acfit_prepare(f, f->stream, indices, total, bmax, iterations, learning_rate)) return rc;
    if (const int rc = acfit_enqueue(f, batch_sizes, iterations)) return rc;
    return acfit_finish(f, f->stream, iterations, losses);
}

// ac_ppo.hip -- the PPO trainer on the GPU (include/bcmpc.h bcmpc_acppo_*): the reference's lossandupdate_ppo
// (ppo_bc_policy.py:90-144), one Adam step on pol_surr + pol_entpen + vf_loss over pol/, vf/ and logstd against a
// frozen old policy, restated as explicit forward / backward kernels in f32.  bc_mpc_amd/ppo.py is the definition
// (operation order of the surrogate, its gradient, TF1 ApplyAdam); tests/test_gpu_ac_ppo.py holds these kernels to
// it.
//
// One PPO step is two launches, the structure of ac_fit.hip with both stacks in each:
//   acppo_rows_kernel    grid (ceil(B / 16), 2): blockIdx.y == 0 runs the policy stack, 1 the value stack, on the
//                        same 16 gathered rows -- the two stacks share no data, so no workgroup waits for another.
//                        The policy block's epilogue forms z, both negative log-likelihoods, the ratio, the clip
//                        mask and dlogp per row; it writes dmean as the backward operand, the row's
//                        dlogp (z^2 - 1) for the logstd sum and the block partials of min(surr1, surr2), the kl
//                        summand and (ac - mean)^2.  The value block's epilogue is ac_fit.hip's value head.
//   acppo_params_kernel  one workgroup per 16 x 16 weight tile of either stack (batch sum in a fixed order, TF1
//                        ApplyAdam on the fitter's weights with the trainer's PPO slots, the transposed copy), one
//                        for logstd (the rows' contributions in row order, minus entcoeff, Adam), one that
//                        finishes the six losses from the partials and advances the step counter.
// mode 1 of the row kernel is forward-only: the same GEMM path over all n data rows with the old weights and the
// old filter, no activation stores, and mean goes to oldmean.  mean and oldmean come from one instruction
// sequence, so a step whose parameters equal the old ones has ratio == 1 and kl == 0 exactly.
//
// The trainer trains in place on its two fitters' d_w / d_wt and uses their activation buffers; the interleaved
// BC step is the policy fitter's own acfit_step enqueued into the same chain (ac_fit_internal.h).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "../../include/bcmpc.h"
#include "ac_fit_internal.h"
#include "ac_ppo_plan.h"
#include "train_rows.h"

namespace bcmpc::acppo {

using acfit::kRows;
using acfit::kTgtLd;
using acfit::kWaves;
using acfit::fail;

using rows::adam_elem;                      // the row-tile GEMM and Adam: train_rows.h
using rows::f4v;
using rows::kPK;
using rows::rows_gemm;
static_assert(rows::kWaves == kWaves, "the plan's LDS layout and the row GEMM agree on the workgroup's waves");

constexpr int kLsLd = 16;                   // stride of the rows' logstd contributions (A <= 16)
constexpr float kHalfLog2Pi = 0.91893853320467274178f;        // f32(0.5 log 2 pi)
constexpr float kHalfLog2PiE = 1.41893853320467274178f;       // f32(0.5 log(2 pi e))

struct Stack {
    float* w; float* wt; float* m; float* v;            // the fitter's params and W^T copy; the PPO Adam slots
    float* x0; float* dp; float* act; float* dzs;       // the fitter's activation buffers: [Bcap][S], [Bcap][N], [L][Bcap][h]
    int32_t w_off[BCMPC_ACFIT_MAX_LAYERS + 1], b_off[BCMPC_ACFIT_MAX_LAYERS + 1];
    int32_t N, Bcap;
};

struct Args {
    const double* obs;                                  // [n][S]
    const float* acs; const float* atarg; const float* ret;      // [n][A], [n], [n]
    float* oldmean;                                     // [n][A]
    const int64_t* idx_base; int32_t stride; int32_t* iter;
    const float* filt;                                  // [2][32] the current filter (the policy fitter's)
    const float* old_w; const float* old_filt; const float* oldlogstd;
    Stack st[2];
    float* logstd; float* ls_m; float* ls_v;            // [16]
    float* rowls;                                       // [rcap][kLsLd] dlogp (z^2 - 1)
    float* part;                                        // [blocks][4] sum min(surr), sum kl, sum (ac - mean)^2, sum (v - ret)^2
    float* ent;                                         // [1] this step's entropy (taken before logstd moves)
    float* loss;                                        // [iterations][6]
    float* bp;                                          // [beta1_power, beta2_power, lr, eps, entcoeff]
    const Task* tasks;
    int32_t B, S, A, L, h, ld, mode;
    float b1, b2, eps;
};

__global__ __launch_bounds__(1024) void acppo_rows_kernel(const Args a) {
    extern __shared__ float sm[];
    const int ld = a.ld, S = a.S, A = a.A, L = a.L, h = a.h;
    const bool fwd = a.mode != 0;                         // the old policy's means over all rows
    const int sk = fwd ? 0 : (int)blockIdx.y;             // 0: pol/, 1: vf/
    const Stack& st = a.st[sk];
    const int N = st.N;
    float* bufA = sm;                       // [16][ld]: the current layer input / backward operand
    float* bufB = bufA + kRows * ld;        // [16][ld]: GEMM output
    float* tsm = bufB + kRows * ld;         // [16][16] actions
    float* red = tsm + kRows * kTgtLd;      // [kWaves] (ac_fit.hip's layout; unused)
    float* kp = red + kWaves;               // [kWaves][256] K-split partials
    float* acache = kp + kWaves * 256;      // [L][16][ld] activation rows A_l
    float* osm = acache + L * kRows * ld;   // [16][16] old means
    float* rs = osm + kRows * kTgtLd;       // [8][16] per row: atarg / ret, min(surr), kl, (ac - mean)^2; logstd, oldlogstd
    float* sd = rs + 8 * kRows;             // [2][16] std, old std
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r0 = blockIdx.x * kRows;
    const int nr = min(kRows, a.B - r0);
    const int it = fwd ? 0 : *a.iter;
    const int64_t* idx = fwd ? nullptr : a.idx_base + (int64_t)it * a.stride;
    const float* W = fwd ? a.old_w : st.w;
    const float* filt = fwd ? a.old_filt : a.filt;
    if (!fwd && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        if (it > 0) {                                     // the previous step's finish (AdamOptimizer._finish)
            a.bp[0] = __fmul_rn(a.bp[0], a.b1);
            a.bp[1] = __fmul_rn(a.bp[1], a.b2);
        }
        float e = 0.f;                                    // the entropy, before this step's update of logstd
        for (int j = 0; j < A; ++j) e += a.logstd[j] + kHalfLog2PiE;
        a.ent[0] = e;
    }
    // ---- gather: obz = clip((f32(ob) - mean) / std, -5, 5) in f32; ac, oldmean, atarg / ret as fed ----
    for (int i = tid; i < kRows * S; i += 64 * kWaves) {
        const int r = i / S, c = i % S;
        float val = 0.f;
        if (r < nr) {
            const int64_t row = fwd ? (int64_t)(r0 + r) : idx[r0 + r];
            const float x = (float)a.obs[row * S + c];
            val = __fdiv_rn(__fsub_rn(x, filt[c]), filt[32 + c]);
            val = val < -5.0f ? -5.0f : (val > 5.0f ? 5.0f : val);
            if (!fwd) st.x0[(size_t)(r0 + r) * S + c] = val;
        }
        bufA[r * ld + c] = val;
    }
    if (!fwd) {
        if (sk == 0) {
            for (int i = tid; i < kRows * A; i += 64 * kWaves) {
                const int r = i / A, c = i % A;
                float av = 0.f, ov = 0.f;
                if (r < nr) {
                    const int64_t row = idx[r0 + r];
                    av = a.acs[row * A + c];
                    ov = a.oldmean[row * A + c];
                }
                tsm[r * kTgtLd + c] = av;
                osm[r * kTgtLd + c] = ov;
            }
            if (tid < A) {
                const float ls = a.logstd[tid], ols = a.oldlogstd[tid];
                rs[4 * kRows + tid] = ls;
                rs[5 * kRows + tid] = ols;
                sd[tid] = expf(ls);
                sd[kRows + tid] = expf(ols);
            }
        }
        if (tid >= 64 && tid < 64 + kRows) {
            const int r = tid - 64;
            rs[r] = r < nr ? (sk == 0 ? a.atarg[idx[r0 + r]] : a.ret[idx[r0 + r]]) : 0.f;
        }
    }
    __syncthreads();
    const size_t BH = (size_t)st.Bcap * h;
    // ---- forward: one row per wave after each GEMM ----
    for (int l = 0; l < L; ++l) {
        rows_gemm(bufA, l == 0 ? S : h, W + st.w_off[l], h, h, W + st.b_off[l], bufB, ld, kp);
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
                if (r < nr && !fwd) st.act[go + f] = v;
            }
        }
        __syncthreads();
    }
    rows_gemm(bufA, h, W + st.w_off[L], N, N, W + st.b_off[L], bufB, ld, kp);
    __syncthreads();
    if (fwd) {                                            // the old means; nothing else
        for (int i = tid; i < kRows * A; i += 64 * kWaves) {
            const int r = i / A, c = i % A;
            if (r < nr) a.oldmean[(size_t)(r0 + r) * A + c] = bufB[r * ld + c];
        }
        return;
    }
    const float fB = (float)a.B;
    if (sk == 0) {
        // ---- the surrogate, row by row (one thread per row: A <= 16 terms in column order) ----
        if (tid < kRows) {
            const int r = tid;
            float mn = 0.f, klr = 0.f, sq = 0.f;
            if (r < nr) {
                float sz = 0.f, szo = 0.f, sls = 0.f, sols = 0.f;
                for (int j = 0; j < A; ++j) {
                    const float mean = bufB[r * ld + j], acv = tsm[r * kTgtLd + j], om = osm[r * kTgtLd + j];
                    const float sdv = sd[j], osd = sd[kRows + j], ls = rs[4 * kRows + j], ols = rs[5 * kRows + j];
                    const float d = acv - mean;
                    const float z = __fdiv_rn(d, sdv), zo = __fdiv_rn(acv - om, osd);
                    sz += z * z;
                    szo += zo * zo;
                    sls += ls;
                    sols += ols;
                    const float dm = om - mean;
                    klr += ((ls - ols) + __fdiv_rn(osd * osd + dm * dm, 2.0f * sdv * sdv)) - 0.5f;
                    sq += d * d;
                }
                const float nlp = (0.5f * sz + kHalfLog2Pi * (float)A) + sls;
                const float nlpo = (0.5f * szo + kHalfLog2Pi * (float)A) + sols;
                const float ratio = expf(nlpo - nlp);
                const float at = rs[r], ce = a.bp[3];
                const float lo = 1.0f - ce, hi = 1.0f + ce;
                const float s1 = ratio * at;
                const float s2 = fminf(fmaxf(ratio, lo), hi) * at;
                const bool take1 = s1 <= s2, inside = lo <= ratio && ratio <= hi;
                const float g = -__fdiv_rn(at, fB) * (take1 ? 1.0f : (inside ? 1.0f : 0.f));
                const float dlogp = g * ratio;
                mn = s1 <= s2 ? s1 : s2;
                for (int j = 0; j < A; ++j) {
                    const float sdv = sd[j];
                    const float z = __fdiv_rn(tsm[r * kTgtLd + j] - bufB[r * ld + j], sdv);
                    const float dmean = dlogp * __fdiv_rn(z, sdv);
                    bufA[r * ld + j] = dmean;
                    st.dp[(size_t)(r0 + r) * A + j] = dmean;
                    a.rowls[(size_t)(r0 + r) * kLsLd + j] = dlogp * (z * z - 1.0f);
                }
            } else {
                for (int j = 0; j < A; ++j) bufA[r * ld + j] = 0.f;
            }
            rs[1 * kRows + r] = mn;
            rs[2 * kRows + r] = klr;
            rs[3 * kRows + r] = sq;
        }
        __syncthreads();
        if (tid < 3) {                                    // block partials, rows in order
            float t = 0.f;
            for (int r = 0; r < nr; ++r) t += rs[(1 + tid) * kRows + r];
            a.part[blockIdx.x * 4 + tid] = t;
        }
    } else {
        // ---- the value head: d = v - ret, dv = (1 / B) (d * 2) ----
        if (tid < kRows) {
            const int r = tid;
            float sq = 0.f, g = 0.f;
            if (r < nr) {
                const float d = bufB[r * ld] - rs[r];
                sq = d * d;
                g = __fdiv_rn(1.0f, fB) * (d * 2.0f);
                st.dp[(size_t)(r0 + r)] = g;
            }
            bufA[r * ld] = g;
            rs[1 * kRows + r] = sq;
        }
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
            for (int r = 0; r < nr; ++r) t += rs[1 * kRows + r];
            a.part[blockIdx.x * 4 + 3] = t;
        }
    }
    __syncthreads();
    // ---- backward data gradients: dH_l = dZ_{l+1} W_{l+1}^T, dZ_l = dH_l (1 - A_l^2) ----
    for (int l = L - 1; l >= 0; --l) {
        const int out = l + 1 == L ? N : h;                 // dZ_{l+1} width; W_{l+1}^T is [out][h]
        rows_gemm(bufA, out, st.wt + st.w_off[l + 1], h, h, nullptr, bufB, ld, kp);
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
                if (r < nr) st.dzs[go + f] = dzv;
                dz[f] = dzv;
            }
        }
        __syncthreads();
    }
}

// one workgroup per task; a weight tile's 4 waves take contiguous quarters of the batch and their partials are
// added in wave order (deterministic)
__global__ __launch_bounds__(256) void acppo_params_kernel(const Args a) {
    __shared__ float tp[4][4][64];          // weight-tile partials per wave
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int B = a.B, S = a.S, A = a.A, L = a.L, h = a.h;
    const Task tk = a.tasks[blockIdx.x];
    const float lr_t = __fdiv_rn(__fmul_rn(a.bp[2], __fsqrt_rn(__fsub_rn(1.0f, a.bp[1]))), __fsub_rn(1.0f, a.bp[0]));
    if (tk.kind == 3) {
        if (threadIdx.x == 0) {
            // the six losses from the row blocks' partials, in block order
            const int nblk = (B + kRows - 1) / kRows;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
            for (int k = 0; k < nblk; ++k) {
                s0 += a.part[4 * k + 0];
                s1 += a.part[4 * k + 1];
                s2 += a.part[4 * k + 2];
                s3 += a.part[4 * k + 3];
            }
            const float fB = (float)B, ent = a.ent[0];
            const int it = *a.iter;
            float* out = a.loss + (size_t)it * 6;
            out[0] = -__fdiv_rn(s0, fB);                          // pol_surr
            out[1] = -(a.bp[4] * ent);                            // pol_entpen
            out[2] = __fdiv_rn(s3, fB);                           // vf_loss
            out[3] = __fdiv_rn(s1, fB);                           // kl
            out[4] = ent;
            out[5] = __fsqrt_rn(__fdiv_rn(s2, (float)(B * A)));   // bc_loss
            *a.iter = it + 1;
        }
        return;
    }
    if (tk.kind == 2) {
        // logstd: the rows' contributions in row order, minus entcoeff, then Adam
        if (threadIdx.x < A) {
            const int j = threadIdx.x;
            float s = 0.f;
            for (int b = 0; b < B; ++b) s += a.rowls[(size_t)b * kLsLd + j];
            const float g = s - a.bp[4];
            adam_elem(a.logstd, a.ls_m, a.ls_v, j, g, a.logstd[j], a.ls_m[j], a.ls_v[j], lr_t, a.b1, a.b2, a.eps);
        }
        return;
    }
    const Stack& st = a.st[tk.stack];
    const int N = st.N, l = tk.layer;
    const size_t BH = (size_t)st.Bcap * h;
    // dW_l[k][n] = sum_b Hin[b][k] dZ[b][n], row k == in of the tile: the bias (Hin = 1)
    // (A = Hin^T: lane (k = r16, b = k4); B = dZ: (b = k4, n = r16))
    const int in = l == 0 ? S : h, out = l == L ? N : h;
    const float* Hin = l == 0 ? st.x0 : st.act + (size_t)(l - 1) * BH;
    const float* dZ = l == L ? st.dp : st.dzs + (size_t)l * BH;
    const int r16 = lane & 15, k4 = lane >> 4;
    const int k = tk.k0 + r16, n = tk.n0 + r16;
    // this lane's Adam operands (wave 0 updates), requested with the gradient operands
    float w0[4], m0[4], v0[4];
    size_t pi[4];
    if (wv == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = tk.k0 + 4 * k4 + r;
            pi[r] = kk < in ? (size_t)st.w_off[l] + (size_t)kk * out + n : (size_t)st.b_off[l] + n;
            const bool ok = kk <= in && n < out;
            w0[r] = ok ? st.w[pi[r]] : 0.f;
            m0[r] = ok ? st.m[pi[r]] : 0.f;
            v0[r] = ok ? st.v[pi[r]] : 0.f;
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
            const float gsum = ((tp[0][r][lane] + tp[1][r][lane]) + tp[2][r][lane]) + tp[3][r][lane];
            const int kk = tk.k0 + 4 * k4 + r;
            if (kk <= in && n < out) {
                const float wn = adam_elem(st.w, st.m, st.v, pi[r], gsum, w0[r], m0[r], v0[r], lr_t, a.b1, a.b2, a.eps);
                if (kk < in && l > 0) st.wt[(size_t)st.w_off[l] + (size_t)n * in + kk] = wn;   // W^T copy
            }
        }
    }
}

}  // namespace bcmpc::acppo

using namespace bcmpc::acppo;
namespace train = bcmpc::train;
using bcmpc::acfit::acfit_finish;
using bcmpc::acfit::acfit_prepare;
using bcmpc::acfit::acfit_reserve;
using bcmpc::acfit::acfit_step;

// ------------------------------------------------------------------ C ABI ---
struct bcmpc_acppo {
    Plan plan;
    bcmpc_acfit* pol = nullptr;
    bcmpc_acfit* val = nullptr;
    hipStream_t stream = nullptr;
    float *d_m[2] = {nullptr, nullptr}, *d_v[2] = {nullptr, nullptr};     // the PPO Adam slots of pol/, vf/
    float* d_ls = nullptr;                        // [3][16] logstd, its m, its v
    float* d_old = nullptr;                       // old policy weights (the policy fitter's layout)
    float* d_oldf = nullptr;                      // [2][32] old filter, then [16] oldlogstd
    float* d_state = nullptr;                     // [beta1_power, beta2_power, lr, eps, entcoeff, -, -, ent]
    float h_state[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int32_t* d_iter = nullptr;
    Task* d_tasks = nullptr;
    double* d_obs = nullptr;
    float *d_acs = nullptr, *d_atarg = nullptr, *d_ret = nullptr, *d_oldmean = nullptr;
    int64_t n_data = 0, data_cap = 0;
    float *d_rowls = nullptr, *d_part = nullptr; int32_t rcap = 0;
    int64_t* d_idx = nullptr; int64_t idx_cap = 0;
    float* d_loss = nullptr; int32_t loss_cap = 0;
    // one captured graph of a whole uniform run: a single chain of kernel nodes.  It is reused while everything
    // it holds by address or by value stands (the key); lr, eps, entcoeff and the filter are read from device
    // memory at fixed addresses.
    train::GraphRun graph;
    bool last_graph = false;
    bool has_logstd = false, has_old = false, has_data = false;
};

static Args acppo_args(const bcmpc_acppo* t, const int64_t* d_idx, int stride, int B, int mode) {
    const Plan& p = t->plan;
    Args a{};
    a.obs = t->d_obs; a.acs = t->d_acs; a.atarg = t->d_atarg; a.ret = t->d_ret; a.oldmean = t->d_oldmean;
    a.idx_base = d_idx; a.stride = stride; a.iter = t->d_iter;
    a.filt = t->pol->d_filt;
    a.old_w = t->d_old; a.old_filt = t->d_oldf; a.oldlogstd = t->d_oldf + 64;
    bcmpc_acfit* fs[2] = {t->pol, t->val};
    for (int s = 0; s < 2; ++s) {
        Stack& st = a.st[s];
        const bcmpc_acfit* f = fs[s];
        st.w = f->d_w; st.wt = f->d_wt; st.m = t->d_m[s]; st.v = t->d_v[s];
        st.x0 = f->d_x0; st.dp = f->d_dp; st.act = f->d_act; st.dzs = f->d_dzs;
        for (int l = 0; l <= p.L; ++l) { st.w_off[l] = f->plan.w_off[l]; st.b_off[l] = f->plan.b_off[l]; }
        st.N = f->plan.N; st.Bcap = f->bcap;
    }
    a.logstd = t->d_ls; a.ls_m = t->d_ls + 16; a.ls_v = t->d_ls + 32;
    a.rowls = t->d_rowls; a.part = t->d_part; a.ent = t->d_state + 7; a.loss = t->d_loss; a.bp = t->d_state;
    a.tasks = t->d_tasks;
    a.B = B; a.S = p.S; a.A = p.A; a.L = p.L; a.h = p.h; a.ld = p.ld; a.mode = mode;
    a.b1 = p.cfg.beta1; a.b2 = p.cfg.beta2; a.eps = p.cfg.epsilon;
    return a;
}

// one PPO step: 2 launches
static int acppo_step(bcmpc_acppo* t, const int64_t* d_idx, int stride, int B) {
    const Plan& p = t->plan;
    const Args a = acppo_args(t, d_idx, stride, B, 0);
    hipLaunchKernelGGL(acppo_rows_kernel, dim3((B + kRows - 1) / kRows, 2), dim3(64 * kWaves), p.lds_words * 4,
                       t->stream, a);
    if (hipGetLastError() != hipSuccess) return fail(BCMPC_ERR_HIP, "acppo_rows_kernel launch failed");
    hipLaunchKernelGGL(acppo_params_kernel, dim3((unsigned)p.tasks.size()), dim3(256), 0, t->stream, a);
    if (hipGetLastError() != hipSuccess) return fail(BCMPC_ERR_HIP, "acppo_params_kernel launch failed");
    return BCMPC_OK;
}

// the old policy's means of all n data rows: the row kernel, forward only
static int acppo_snapshot(bcmpc_acppo* t) {
    const Plan& p = t->plan;
    const Args a = acppo_args(t, nullptr, 0, (int)t->n_data, 1);
    hipLaunchKernelGGL(acppo_rows_kernel, dim3((unsigned)((t->n_data + kRows - 1) / kRows), 1), dim3(64 * kWaves),
                       p.lds_words * 4, t->stream, a);
    if (hipGetLastError() != hipSuccess) return fail(BCMPC_ERR_HIP, "acppo_rows_kernel (old means) launch failed");
    return BCMPC_OK;
}

extern "C" {

int bcmpc_acppo_is_graph(const bcmpc_acppo* t) { return t && t->last_graph ? t->graph.captures : 0; }

int bcmpc_acppo_create(const bcmpc_acppo_config* c, bcmpc_acfit* pol, bcmpc_acfit* val, bcmpc_acppo** out) {
    if (!c || !pol || !val || !out) return fail(BCMPC_ERR_ARG, "null argument");
    *out = nullptr;
    Plan plan;
    if (const int rc = make_plan(c, &pol->plan.cfg, &val->plan.cfg, &plan)) return rc;   // before any HIP call
    if (hipSetDevice(plan.device) != hipSuccess) return fail(BCMPC_ERR_HIP, "hipSetDevice failed");
    bcmpc_acppo* t = new bcmpc_acppo();
    t->plan = std::move(plan);
    t->pol = pol;
    t->val = val;
    const Plan& p = t->plan;
    const size_t np[2] = {pol->plan.n_params, val->plan.n_params};
    bool ok = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) == hipSuccess;
    for (int s = 0; s < 2 && ok; ++s)
        ok = hipMalloc(&t->d_m[s], np[s] * 4) == hipSuccess && hipMalloc(&t->d_v[s], np[s] * 4) == hipSuccess &&
             hipMemset(t->d_m[s], 0, np[s] * 4) == hipSuccess && hipMemset(t->d_v[s], 0, np[s] * 4) == hipSuccess;
    ok = ok && hipMalloc(&t->d_ls, 48 * 4) == hipSuccess && hipMemset(t->d_ls, 0, 48 * 4) == hipSuccess &&
         hipMalloc(&t->d_old, np[0] * 4) == hipSuccess && hipMalloc(&t->d_oldf, 80 * 4) == hipSuccess &&
         hipMalloc(&t->d_state, 8 * 4) == hipSuccess && hipMemset(t->d_state, 0, 8 * 4) == hipSuccess &&
         hipMalloc(&t->d_iter, 4) == hipSuccess &&
         hipMalloc(&t->d_tasks, p.tasks.size() * sizeof(Task)) == hipSuccess &&
         hipMemcpy(t->d_tasks, p.tasks.data(), p.tasks.size() * sizeof(Task), hipMemcpyHostToDevice) == hipSuccess &&
         (p.lds_words * 4 <= 65536 ||
          hipFuncSetAttribute((const void*)acppo_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(p.lds_words * 4)) == hipSuccess);
    if (!ok) { bcmpc_acppo_destroy(t); return fail(BCMPC_ERR_HIP, "device allocation failed"); }
    t->h_state[0] = c->beta1;
    t->h_state[1] = c->beta2;
    *out = t;
    return BCMPC_OK;
}

int bcmpc_acppo_destroy(bcmpc_acppo* t) {
    if (!t) return BCMPC_OK;
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    t->graph.drop();
    for (void* p : {(void*)t->d_m[0], (void*)t->d_m[1], (void*)t->d_v[0], (void*)t->d_v[1], (void*)t->d_ls,
                    (void*)t->d_old, (void*)t->d_oldf, (void*)t->d_state, (void*)t->d_iter, (void*)t->d_tasks,
                    (void*)t->d_obs, (void*)t->d_acs, (void*)t->d_atarg, (void*)t->d_ret, (void*)t->d_oldmean,
                    (void*)t->d_rowls, (void*)t->d_part, (void*)t->d_idx, (void*)t->d_loss})
        if (p) (void)hipFree(p);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
    return BCMPC_OK;
}

int bcmpc_acppo_set_logstd(bcmpc_acppo* t, const float* logstd) {
    if (!t || !logstd) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = check_finite(logstd, t->plan.A, "logstd")) return rc;
    float h[16] = {};
    std::copy(logstd, logstd + t->plan.A, h);
    if (hipSetDevice(t->plan.device) != hipSuccess ||
        hipMemcpyAsync(t->d_ls, h, sizeof(h), hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipStreamSynchronize(t->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "logstd upload failed");
    t->has_logstd = true;
    return BCMPC_OK;
}

int bcmpc_acppo_get_logstd(bcmpc_acppo* t, float* logstd) {
    if (!t || !logstd) return fail(BCMPC_ERR_ARG, "null argument");
    if (!t->has_logstd) return fail(BCMPC_ERR_STATE, "bcmpc_acppo_set_logstd has not been called");
    float h[16];
    if (hipSetDevice(t->plan.device) != hipSuccess ||
        hipMemcpyAsync(h, t->d_ls, sizeof(h), hipMemcpyDeviceToHost, t->stream) != hipSuccess ||
        hipStreamSynchronize(t->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "logstd download failed");
    std::copy(h, h + t->plan.A, logstd);
    return BCMPC_OK;
}

int bcmpc_acppo_set_old(bcmpc_acppo* t, const float* const* kernels, const float* const* biases, const float* ob_mean,
                        const float* ob_std, const float* oldlogstd) {
    if (!t || !kernels || !biases || !oldlogstd) return fail(BCMPC_ERR_ARG, "null argument");
    const bcmpc::acfit::Plan& fp = t->pol->plan;
    if (const int rc = bcmpc::acfit::check_filter(ob_mean, ob_std, fp.S)) return rc;
    if (const int rc = check_finite(oldlogstd, fp.N, "oldlogstd")) return rc;
    std::vector<float> hw(fp.n_params, 0.f);
    for (int l = 0; l <= fp.L; ++l) {
        if (!kernels[l] || !biases[l]) return fail(BCMPC_ERR_ARG, "null kernel / bias");
        std::copy(kernels[l], kernels[l] + (size_t)fp.lin[l] * fp.lout[l], hw.begin() + fp.w_off[l]);
        std::copy(biases[l], biases[l] + fp.lout[l], hw.begin() + fp.b_off[l]);
    }
    if (const int rc = check_finite(hw.data(), (int64_t)hw.size(), "the old policy's weights")) return rc;
    float hf[80];
    bcmpc::acfit::filter_image(ob_mean, ob_std, fp.S, hf);
    for (int i = 0; i < 16; ++i) hf[64 + i] = i < fp.N ? oldlogstd[i] : 0.f;
    if (hipSetDevice(t->plan.device) != hipSuccess ||
        hipMemcpyAsync(t->d_old, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipMemcpyAsync(t->d_oldf, hf, sizeof(hf), hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipStreamSynchronize(t->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "old policy upload failed");
    t->has_old = true;
    return BCMPC_OK;
}

int bcmpc_acppo_set_data(bcmpc_acppo* t, const double* obs, const float* acs, const float* atarg, const float* ret,
                         int64_t n) {
    if (!t || n < 1 || !obs || !acs || !atarg || !ret) return fail(BCMPC_ERR_ARG, "bad argument");
    if (n > INT32_MAX / 64) return fail(BCMPC_ERR_UNSUPPORTED, "too many data rows");
    const Plan& p = t->plan;
    if (const int rc = check_finite(acs, n * p.A, "actions")) return rc;
    if (const int rc = check_finite(atarg, n, "advantages")) return rc;
    if (const int rc = check_finite(ret, n, "returns")) return rc;
    if (hipSetDevice(p.device) != hipSuccess) return fail(BCMPC_ERR_HIP, "hipSetDevice failed");
    if (n > t->data_cap) {
        t->graph.drop();                                  // the graph holds the data buffers' addresses
        t->n_data = 0;
        t->has_data = false;
        if (!train::grow(&t->data_cap, n, {{&t->d_obs, (size_t)n * p.S * 8}, {&t->d_acs, (size_t)n * p.A * 4},
                                           {&t->d_atarg, (size_t)n * 4}, {&t->d_ret, (size_t)n * 4},
                                           {&t->d_oldmean, (size_t)n * p.A * 4}}))
            return fail(BCMPC_ERR_HIP, "data buffer allocation failed");
    }
    if (hipMemcpyAsync(t->d_obs, obs, (size_t)n * p.S * 8, hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipMemcpyAsync(t->d_acs, acs, (size_t)n * p.A * 4, hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipMemcpyAsync(t->d_atarg, atarg, (size_t)n * 4, hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipMemcpyAsync(t->d_ret, ret, (size_t)n * 4, hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipStreamSynchronize(t->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "data upload failed");
    t->n_data = n;
    t->has_data = true;
    return BCMPC_OK;
}

int bcmpc_acppo_run(bcmpc_acppo* t, const int64_t* indices, const int32_t* batch_sizes, int32_t iterations,
                    float learning_rate, float eps, float entcoeff, const int64_t* bc_indices,
                    const int32_t* bc_batch_sizes, float bc_learning_rate, float* losses, float* bc_losses) {
    if (!t) return fail(BCMPC_ERR_ARG, "null argument");
    bcmpc_acfit *pol = t->pol, *val = t->val;
    const bool bc = bc_indices != nullptr;
    if (const int rc = check_hyper(learning_rate, eps, entcoeff)) return rc;
    if (const int rc = check_state(t->has_logstd, t->has_old, t->has_data, pol->has_weights, val->has_weights,
                                   pol->has_filter))
        return rc;
    int64_t total = 0, bc_total = 0;
    int32_t bmax = 0, bc_bmax = 0;
    if (const int rc = bcmpc::acfit::check_run(indices, batch_sizes, iterations, learning_rate, t->n_data, &total, &bmax))
        return rc;
    if (bc)
        if (const int rc = bcmpc::acfit::check_run(bc_indices, bc_batch_sizes, iterations, bc_learning_rate, pol->n_data,
                                                   &bc_total, &bc_bmax))
            return rc;
    if (iterations == 0) return BCMPC_OK;
    const Plan& p = t->plan;
    if (hipSetDevice(p.device) != hipSuccess) return fail(BCMPC_ERR_HIP, "hipSetDevice failed");
    // no run of either fitter is in flight: their runs synchronise
    if (!acfit_reserve(pol, std::max(bmax, bc_bmax)) || !acfit_reserve(val, bmax))
        return fail(BCMPC_ERR_HIP, "activation buffer allocation failed");
    const size_t nblk = ((size_t)bmax + kRows - 1) / kRows;
    if (!train::grow(&t->rcap, bmax, {{&t->d_rowls, (size_t)bmax * kLsLd * 4}, {&t->d_part, nblk * 4 * 4}}))
        return fail(BCMPC_ERR_HIP, "row buffer allocation failed");
    if (!train::grow(&t->idx_cap, total, {{&t->d_idx, (size_t)total * 8}}))
        return fail(BCMPC_ERR_HIP, "index buffer allocation failed");
    if (!train::grow(&t->loss_cap, iterations, {{&t->d_loss, (size_t)iterations * 6 * 4}}))
        return fail(BCMPC_ERR_HIP, "loss buffer allocation failed");
    // device step state: counter 0, the host mirror's beta powers, this run's lr / eps / entcoeff
    t->h_state[2] = learning_rate;
    t->h_state[3] = eps;
    t->h_state[4] = entcoeff;
    if (hipMemcpyAsync(t->d_idx, indices, (size_t)total * 8, hipMemcpyHostToDevice, t->stream) != hipSuccess ||
        hipMemsetAsync(t->d_iter, 0, 4, t->stream) != hipSuccess ||
        hipMemcpyAsync(t->d_state, t->h_state, 20, hipMemcpyHostToDevice, t->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "step state upload failed");
    if (bc)
        if (const int rc = acfit_prepare(pol, t->stream, bc_indices, bc_total, bc_bmax, iterations, bc_learning_rate))
            return rc;
    if (const int rc = acppo_snapshot(t)) return rc;      // oldmean, once per call
    bool uniform = true;
    for (int i = 1; i < iterations; ++i)
        uniform = uniform && batch_sizes[i] == batch_sizes[0] && (!bc || bc_batch_sizes[i] == bc_batch_sizes[0]);
    const char* ge = std::getenv("BCMPC_ACPPO_GRAPH");
    const bool use_graph = uniform && !(ge && ge[0] == '0');
    if (use_graph) {
        const intptr_t key[train::GraphRun::kKey] = {iterations, batch_sizes[0], bc ? bc_batch_sizes[0] : 0,
                                  (intptr_t)t->d_idx, (intptr_t)t->d_loss, (intptr_t)t->d_rowls, (intptr_t)t->d_obs,
                                  (intptr_t)pol->d_x0, (intptr_t)val->d_x0,
                                  bc ? (intptr_t)pol->d_idx : 0, bc ? (intptr_t)pol->d_loss : 0,
                                  bc ? (intptr_t)pol->d_obs : 0, bc ? (intptr_t)pol->d_tgt : 0,
                                  pol->bcap, val->bcap, (intptr_t)pol->d_act};
        const int rc = t->graph.run(t->stream, key, fail, [&] {
            int rs = BCMPC_OK;
            for (int i = 0; i < iterations && rs == BCMPC_OK; ++i) {
                rs = acppo_step(t, t->d_idx, batch_sizes[0], batch_sizes[0]);
                if (bc && rs == BCMPC_OK)
                    rs = acfit_step(pol, t->stream, pol->d_idx, bc_batch_sizes[0], bc_batch_sizes[0]);
            }
            return rs;
        });
        if (rc != BCMPC_OK) return rc;
    } else {
        int64_t pos = 0, bpos = 0;
        for (int i = 0; i < iterations; ++i) {
            if (const int rc = acppo_step(t, t->d_idx + pos, 0, batch_sizes[i])) return rc;
            pos += batch_sizes[i];
            if (bc) {
                if (const int rc = acfit_step(pol, t->stream, pol->d_idx + bpos, 0, bc_batch_sizes[i])) return rc;
                bpos += bc_batch_sizes[i];
            }
        }
    }
    t->last_graph = use_graph;
    if (losses && hipMemcpyAsync(losses, t->d_loss, (size_t)iterations * 6 * 4, hipMemcpyDeviceToHost, t->stream) != hipSuccess)
        return fail(BCMPC_ERR_HIP, "loss download failed");
    if (bc) {
        if (const int rc = acfit_finish(pol, t->stream, iterations, bc_losses)) return rc;
    } else if (hipStreamSynchronize(t->stream) != hipSuccess) {
        return fail(BCMPC_ERR_HIP, "PPO run failed");
    }
    for (int i = 0; i < iterations; ++i) {       // host mirror of the device beta powers (same f32 products)
        t->h_state[0] *= p.cfg.beta1;
        t->h_state[1] *= p.cfg.beta2;
    }
    return BCMPC_OK;
}

}  // extern "C"

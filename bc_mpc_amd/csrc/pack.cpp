// pack.cpp -- weight packing (pack.h).  Every sum that is rounded once runs in f64, in the order written here; the
// operand scales are exact powers of two.  The kernels' layout notes say what each order is for.
#include "pack.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace bcmpc::host {

void pack_layer(const float* W, int in, int out, int Tin, int Tout, int TB, float* dst) {
    for (int t = 0; t < Tout; ++t) {
        const int tb = t / TB, j = t % TB;
        for (int u = 0; u < Tin; ++u)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * u + 4 * (lane >> 4) + r;
                    const int n = 16 * t + (lane & 15);
                    const size_t o = ((((size_t)tb * Tin + u) * TB + j) * 64 + lane) * 4 + r;
                    dst[o] = (k < in && n < out) ? W[(size_t)k * out + n] : 0.f;
                }
    }
}

void pack_out_rows(const float* W, int in, int out, int Tin, const int* rowmap, float* dst) {
    for (int u = 0; u < Tin; ++u)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) {
                const int k = 16 * u + 4 * (lane >> 4) + r;
                const int c = rowmap[lane & 15];
                const size_t o = (((size_t)u * 64) + lane) * 4 + r;
                dst[o] = (k < in && c >= 0 && c < out) ? W[(size_t)k * out + c] : 0.f;
            }
}

void pack_x3_layer(const float* W, int in, int out, int Pin, int Tout, int TWp, float sw, _Float16* dst) {
    for (int t = 0; t < Tout; ++t) {
        const int ws = t / TWp, j = t % TWp;
        for (int p = 0; p < Pin; ++p)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 8; ++i) {
                    const int k = 32 * p + 16 * (i >> 2) + 4 * (lane >> 4) + (i & 3);
                    const int n = 16 * t + (lane & 15);
                    const float v = (k < in && n < out) ? W[(size_t)k * out + n] * sw : 0.f;
                    const _Float16 hi = (_Float16)v;
                    const _Float16 lo = (_Float16)(v - (float)hi);
                    const size_t o = ((((size_t)ws * Pin + p) * TWp + j) * 2 * 64 + lane) * 8 + i;
                    dst[o] = hi;
                    dst[o + 64 * 8] = lo;
                }
    }
}

float x3_scale(const float* W, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(W[i]));
    if (!(mx > 0.f) || !std::isfinite(mx)) return 1.f;
    int e = 0;
    (void)std::frexp(mx, &e);
    return std::ldexp(1.0f, std::max(-100, std::min(100, 12 - e)));
}

std::vector<float> fold_layer0_rows(const float* W, int in, int out, int* row_exp) {
    std::vector<float> Wf(W, W + (size_t)in * out);
    std::vector<float> rmx(in, 0.f);
    float mx = 0.f;
    for (int k = 0; k < in; ++k) {
        for (int n = 0; n < out; ++n) rmx[k] = std::max(rmx[k], std::fabs(W[(size_t)k * out + n]));
        mx = std::max(mx, rmx[k]);
    }
    for (int k = 0; k < in; ++k) row_exp[k] = 0;
    if (!(mx > 0.f) || !std::isfinite(mx)) return Wf;
    int e = 0;
    (void)std::frexp(mx, &e);
    for (int k = 0; k < in; ++k) {
        if (!(rmx[k] > 0.f)) continue;               // (an all-zero row, or one that holds a NaN: left as it is)
        int ek = 0;
        (void)std::frexp(rmx[k], &ek);
        const int q = std::min(e - ek, kRowFoldMax);
        if (q < kRowFoldMin) continue;
        row_exp[k] = q;
        for (int n = 0; n < out; ++n) Wf[(size_t)k * out + n] = std::ldexp(W[(size_t)k * out + n], q);
    }
    return Wf;
}

float ln_out_scale(const float* gamma, const float* beta, int h) {
    float gm = 0.f, bm = 0.f;
    for (int i = 0; i < h; ++i) {
        gm = std::max(gm, std::fabs(gamma[i]));
        bm = std::max(bm, std::fabs(beta[i]));
    }
    const float bound = std::sqrt((float)h) * gm + bm;
    int ex = 0;
    if (bound > 0.f && std::isfinite(bound)) (void)std::frexp(bound, &ex);
    return std::ldexp(1.0f, std::max(-100, std::min(100, 12 - ex)));
}

namespace {

// the packed split kernels: two halves per weight, the same sizes as the f32 layout
_Float16* halves(PackedNet* o, size_t float_off) { return reinterpret_cast<_Float16*>(o->w.data()) + 2 * float_off; }

void copy_ln(const EnginePlan& p, const bcmpc_weights& w, int nln, PackedNet* o) {   // [gamma: nln x HP][beta: nln x HP]
    for (int l = 0; l < nln && p.cfg.layer_norm; ++l) {
        std::memcpy(o->ln.data() + (size_t)l * p.HP, w.ln_gamma[l], sizeof(float) * p.cfg.hidden);
        std::memcpy(o->ln.data() + (size_t)(nln + l) * p.HP, w.ln_beta[l], sizeof(float) * p.cfg.hidden);
    }
}

// the reward net in split precision: trunk | delta head | delta out | reward head | reward out
void pack_split_reward(const EnginePlan& p, const bcmpc_weights& w, PackedNet* o) {
    const bcmpc_config& c = p.cfg;
    const int S = c.state_dim, A = c.action_dim, h = c.hidden, HP = p.HP, T = p.T, P = T / 2;
    const bool ln = c.layer_norm != 0;                // (team kernel only: plan_engine)
    const std::vector<float> w0 = fold_layer0_rows(w.kernels[0], S + A, h, o->row_exp);
    const float s0 = x3_scale(w0.data(), (size_t)(S + A) * h);
    pack_x3_layer(w0.data(), S + A, h, 1, T, p.pack_tb, s0, halves(o, p.w_off[0]));
    o->winv[0] = 1.0f / s0;
    // the heads' input: the trunk's tanh x 2^12, or its LayerNorm output x hsc[0] (|LN(x)_i| <=
    // sqrt(h) |gamma_i| + |beta_i|, the power of two that keeps it below 2^12)
    float hin = 4096.0f;
    if (ln) o->hsc[0] = hin = ln_out_scale(w.ln_gamma[0], w.ln_beta[0], h);
    const float sd = x3_scale(w.kernels[1], (size_t)h * h), sr = x3_scale(w.kernels[3], (size_t)h * h);
    pack_x3_layer(w.kernels[1], h, h, P, T, p.head_tb, sd, halves(o, p.w_off[1]));
    pack_x3_layer(w.kernels[3], h, h, P, T, p.head_tb, sr, halves(o, p.w_off[3]));
    o->winv[1] = (1.0f / sd) / hin;
    o->winv[3] = (1.0f / sr) / hin;
    // LayerNorm heads (rollout_team.hip HLN): out = rsqrt(var + eps) (dense_2 diag(gamma))^T (h - mean)
    // + (dense_2^T beta + b): gamma folded into the output kernels, beta into their biases
    std::vector<float> w2((size_t)h * S), w4((size_t)h);
    for (int k = 0; k < h; ++k) {
        const float gd = ln ? w.ln_gamma[1][k] : 1.0f, gr = ln ? w.ln_gamma[2][k] : 1.0f;
        for (int n = 0; n < S; ++n) w2[(size_t)k * S + n] = w.kernels[2][(size_t)k * S + n] * gd;
        w4[k] = w.kernels[4][k] * gr;
    }
    // both output kernels feed one accumulator: one scale (the smaller of the two)
    const float so = std::min(x3_scale(w2.data(), (size_t)h * S), x3_scale(w4.data(), (size_t)h));
    pack_x3_layer(w2.data(), h, S, P, 2, 2, so, halves(o, p.w_off[2]));
    std::vector<float> wr((size_t)h * 16, 0.f);      // dense_4 at row S of the second output tile
    for (int k = 0; k < h; ++k) wr[(size_t)k * 16 + (S - 16)] = w4[k];
    pack_x3_layer(wr.data(), h, 16, P, 1, 1, so, halves(o, p.w_off[4]));
    // (LN: the heads' normalised output carries no 2^12 -- rsqrt of the x 2^12 variance undoes it)
    o->winv[2] = o->winv[4] = ln ? 1.0f / so : (1.0f / so) / 4096.0f;
    float* hb = o->b.data();
    std::memcpy(hb + p.b_off[0], w.biases[0], sizeof(float) * h);
    std::memcpy(hb + p.b_off[1], w.biases[1], sizeof(float) * h);
    std::memcpy(hb + p.b_off[2], w.biases[3], sizeof(float) * h);
    std::memcpy(hb + p.b_off[3], w.biases[2], sizeof(float) * S);
    hb[p.b_off[3] + S] = w.biases[4][0];
    if (ln) {
        for (int n = 0; n <= S; ++n) {                // b + kernel^T beta (f64 sum, one rounding)
            double acc = n < S ? (double)w.biases[2][n] : (double)w.biases[4][0];
            for (int k = 0; k < h; ++k)
                acc += n < S ? (double)w.kernels[2][(size_t)k * S + n] * (double)w.ln_beta[1][k]
                             : (double)w.kernels[4][k] * (double)w.ln_beta[2][k];
            hb[p.b_off[3] + n] = (float)acc;
        }
        // centring table: member t's rows [64 t, 64 t + 64) of the folded, scaled output kernels
        for (int t = 0; t < 8; ++t)
            for (int n = 0; n <= S; ++n) {
                double acc = 0.0;
                for (int k = 64 * t; k < std::min(h, 64 * t + 64); ++k)
                    acc += n < S ? (double)w2[(size_t)k * S + n] * so : (double)w4[k] * so;
                hb[p.b_off[4] + (size_t)t * 32 + n] = (float)acc;
            }
        std::memcpy(o->ln.data(), w.ln_gamma[0], sizeof(float) * h);                   // trunk gamma
        std::memcpy(o->ln.data() + (size_t)3 * HP, w.ln_beta[0], sizeof(float) * h);   // trunk beta
    }
}

// the team kernel's deferred last LayerNorm (rollout_team.hip DEFER; relu + LN, T = 1): the output
// kernel as dense_2 diag(gamma_1), scaled by its own power of two, its inputs the activations centred
// on each wave's column mean (no hsc); bias row b + dense_2^T beta_1 (f64 sum, one rounding); in
// gamma_1's slot the per-wave row sums c_w[n] = so sum_{k in wave w} (dense_2 diag(gamma_1))[k][n]
void pack_team_defer(const EnginePlan& p, const bcmpc_weights& w, PackedNet* o) {
    const bcmpc_config& c = p.cfg;
    const int L = c.n_layers, S = c.state_dim, h = c.hidden, HP = p.HP, P = p.T / 2;
    const int tpw = p.head_tb, nwv = HP / 16 / tpw;
    std::vector<float> wg((size_t)h * S);
    for (int k = 0; k < h; ++k)
        for (int n = 0; n < S; ++n) wg[(size_t)k * S + n] = w.kernels[L][(size_t)k * S + n] * w.ln_gamma[L - 1][k];
    const float so = x3_scale(wg.data(), (size_t)h * S);
    pack_x3_layer(wg.data(), h, S, P, 2, 2, so, halves(o, p.w_off[L]));
    o->winv[L] = 1.0f / so;
    for (int n = 0; n < S; ++n) {
        double acc = w.biases[L][n];
        for (int k = 0; k < h; ++k) acc += (double)w.kernels[L][(size_t)k * S + n] * (double)w.ln_beta[L - 1][k];
        o->b[p.b_off[L] + n] = (float)acc;
    }
    std::fill(o->ln.begin() + HP, o->ln.begin() + 2 * HP, 0.f);
    for (int x = 0; x < nwv; ++x)
        for (int n = 0; n < S; ++n) {
            double acc = 0.0;
            for (int k = 16 * tpw * x; k < std::min(h, 16 * tpw * (x + 1)); ++k) acc += (double)wg[(size_t)k * S + n];
            o->ln[(size_t)HP + x * 32 + n] = (float)(acc * so);
        }
}

// the delta net in split precision (single-pass f16 too: the kernel reads the hi halves)
void pack_split_delta(const EnginePlan& p, const bcmpc_weights& w, PackedNet* o) {
    const bcmpc_config& c = p.cfg;
    const int L = c.n_layers, S = c.state_dim, A = c.action_dim, h = c.hidden, T = p.T, P = T / 2;
    // rollout_pp's folded operands: the hidden-producing layers as f16(W x 2 log2 e), unscaled, when that
    // stays well inside f16's range (else the scaled single-pass layout of the same kernel)
    constexpr float kTanhKh = 2.8853900817779268f;     // 2 log2(e) (split_common.h kTanhK)
    bool fold = p.pp && p.pp_fold;
    for (int l = 0; l < L && fold; ++l) {
        const int in = l == 0 ? S + A : h;
        float mx = 0.f;
        for (size_t i = 0; i < (size_t)in * h; ++i) mx = std::max(mx, std::fabs(w.kernels[l][i]));
        fold = std::isfinite(mx) && mx * kTanhKh < 16384.0f;
    }
    o->pp_fold_w = fold;
    const std::vector<float> w0 = fold_layer0_rows(w.kernels[0], S + A, h, o->row_exp);
    for (int l = 0; l <= L; ++l) {
        const int in = l == 0 ? S + A : h, out = l == L ? S : h;
        const float sw = fold && l < L ? kTanhKh : x3_scale(l == 0 ? w0.data() : w.kernels[l], (size_t)in * out);
        // (team kernel: layer 0 in pack_tb = team_layer0_tiles per wave, hidden layers in head_tb = team_layer1_tiles)
        if (l == 0) pack_x3_layer(w0.data(), in, out, 1, T, p.pack_tb, sw, halves(o, p.w_off[0]));
        else if (l < L) pack_x3_layer(w.kernels[l], in, out, P, T, p.head_tb, sw, halves(o, p.w_off[l]));
        else pack_x3_layer(w.kernels[L], in, out, P, 2, 2, sw, halves(o, p.w_off[L]));
        // layer 0's input scale is per candidate (kernel); hidden inputs are tanh * 2^12, an LN
        // output x hsc[l-1] (static), or relu x its column's power of two (undone in the kernel)
        float in_scale = 4096.0f;
        if (l > 0 && c.layer_norm) {
            o->hsc[l - 1] = in_scale = ln_out_scale(w.ln_gamma[l - 1], w.ln_beta[l - 1], h);
        } else if (l > 0 && c.activation == BCMPC_ACT_RELU) {
            in_scale = 1.0f;
        }
        if (fold) in_scale = 1.0f;                     // (folded: hidden activations are tanh in [-1, 1])
        o->winv[l] = (1.0f / sw) * (l == 0 ? 1.0f : 1.0f / in_scale);
    }
    for (int l = 0; l < L; ++l) std::memcpy(o->b.data() + p.b_off[l], w.biases[l], sizeof(float) * h);
    std::memcpy(o->b.data() + p.b_off[L], w.biases[L], sizeof(float) * S);
    copy_ln(p, w, L, o);
    o->team_defer = TEAM_DEFER && p.kernel == BCMPC_KERNEL_TEAM && p.team_kind == 0 && c.layer_norm &&
                    c.activation == BCMPC_ACT_RELU && L == 2 && team_members(p.HP, p.team_kind) == 1;
    if (o->team_defer) pack_team_defer(p, w, o);
}

// the reward net in fp32: trunk, both heads' hidden layers side by side, a block-diagonal output layer
void pack_fp32_reward(const EnginePlan& p, const bcmpc_weights& w, PackedNet* o) {
    const bcmpc_config& c = p.cfg;
    const int S = c.state_dim, A = c.action_dim, h = c.hidden, HP = p.HP, T = p.T;
    pack_layer(w.kernels[0], S + A, h, 2, T, p.pack_tb, o->w.data() + p.w_off[0]);
    // heads' hidden layers side by side: W1c[k][n] = dense_1 (n < HP) | dense_3 (n >= HP)
    std::vector<float> w1((size_t)h * 2 * HP, 0.f), wo((size_t)2 * HP * 32, 0.f);
    for (int k = 0; k < h; ++k)
        for (int n = 0; n < h; ++n) {
            w1[(size_t)k * 2 * HP + n] = w.kernels[1][(size_t)k * h + n];
            w1[(size_t)k * 2 * HP + HP + n] = w.kernels[3][(size_t)k * h + n];
        }
    // block-diagonal output: rows [0,h) x cols [0,S) = dense_2; rows [HP,HP+h) x col S = dense_4
    for (int k = 0; k < h; ++k) {
        for (int n = 0; n < S; ++n) wo[(size_t)k * 32 + n] = w.kernels[2][(size_t)k * S + n];
        wo[(size_t)(HP + k) * 32 + S] = w.kernels[4][k];
    }
    pack_layer(w1.data(), h, 2 * HP, T, 2 * T, 2 * T / p.nw, o->w.data() + p.w_off[1]);
    pack_layer(wo.data(), 2 * HP, 32, 2 * T, 2, 2, o->w.data() + p.w_off[2]);
    float* hb = o->b.data();
    std::memcpy(hb, w.biases[0], sizeof(float) * h);
    std::memcpy(hb + HP, w.biases[1], sizeof(float) * h);
    std::memcpy(hb + 2 * HP, w.biases[3], sizeof(float) * h);
    std::memcpy(hb + 3 * HP, w.biases[2], sizeof(float) * S);
    hb[3 * HP + S] = w.biases[4][0];
    // LN: [gamma trunk HP | delta HP | reward HP][beta ...], i.e. the heads' params side by side
    copy_ln(p, w, 3, o);
}

void pack_fp32_delta(const EnginePlan& p, const bcmpc_weights& w, PackedNet* o) {
    const bcmpc_config& c = p.cfg;
    const int L = c.n_layers, S = c.state_dim, A = c.action_dim, h = c.hidden, T = p.T;
    pack_layer(w.kernels[0], S + A, h, 2, T, p.pack_tb, o->w.data() + p.w_off[0]);
    for (int l = 1; l < L; ++l) pack_layer(w.kernels[l], h, h, T, T, p.pack_tb, o->w.data() + p.w_off[l]);
    pack_layer(w.kernels[L], h, S, T, 2, 2, o->w.data() + p.w_off[L]);
    for (int l = 0; l < L; ++l) std::memcpy(o->b.data() + p.b_off[l], w.biases[l], sizeof(float) * h);
    std::memcpy(o->b.data() + p.b_off[L], w.biases[L], sizeof(float) * S);
    copy_ln(p, w, L, o);
}

}  // namespace

void pack_weights(const EnginePlan& p, const bcmpc_weights& w, PackedNet* out) {
    *out = PackedNet{};
    out->w.assign(p.w_floats, 0.f);
    out->b.assign(p.b_floats, 0.f);
    out->ln.assign(p.ln_floats, 0.f);
    if (p.split && p.reward) pack_split_reward(p, w, out);
    else if (p.split) pack_split_delta(p, w, out);
    else if (p.reward) pack_fp32_reward(p, w, out);
    else pack_fp32_delta(p, w, out);
    if (p.reward) {
        out->mean_reward = w.mean_reward[0];
        out->std_reward = w.std_reward[0];
    }
    const int S = p.cfg.state_dim, A = p.cfg.action_dim;
    double* C = out->consts;
    for (int i = 0; i < kConstCols; ++i) {
        C[0 * 32 + i] = i < S ? w.mean_obs[i] : 0.0;
        C[1 * 32 + i] = i < S ? w.std_obs[i] + 1e-10 : 1.0;       // dynamics.py:109 (std + 1e-10)
        C[2 * 32 + i] = i < A ? w.mean_action[i] : 0.0;
        C[3 * 32 + i] = i < A ? w.std_action[i] + 1e-10 : 1.0;    // dynamics.py:110
        C[4 * 32 + i] = i < S ? w.mean_deltas[i] : 0.0;
        C[5 * 32 + i] = i < S ? w.std_deltas[i] : 0.0;
        // a layer-0 row's power of two moved out of the packed kernel (fold_layer0_rows) divides its input instead
        if (i < S) C[1 * 32 + i] = std::ldexp(C[1 * 32 + i], out->row_exp[i]);
        if (i < A) C[3 * 32 + i] = std::ldexp(C[3 * 32 + i], out->row_exp[S + i]);
        C[8 * 32 + i] = 1.0 / C[1 * 32 + i];
        C[9 * 32 + i] = 1.0 / C[3 * 32 + i];
    }
}

void pack_policy(const EnginePlan& p, const bcmpc_policy& pol, PackedPolicy* out) {
    *out = PackedPolicy{};
    const bcmpc_config& c = p.cfg;
    const int S = c.state_dim, A = c.action_dim, ph = c.policy_hidden, PL = p.PL, TP = p.TP, PHP = p.PHP;
    out->w.assign(p.pw_floats, 0.f);
    int rowmap[16];
    for (int n = 0; n < 16; ++n) {
        const int j = n - (S - 16);                     // action j sits at output-tile row S-16+j
        rowmap[n] = (j >= 0 && j < A) ? j : -1;
    }
    if (p.split) {
        // one tile per wave (TWp = 1); same byte sizes as the f32 layout.  Input scales:
        // obz (|z| <= 5) x 2^11, hidden tanh x 2^12
        _Float16* hh = reinterpret_cast<_Float16*>(out->w.data());
        const int PP = PHP / 32;
        for (int l = 0; l < PL; ++l) {
            const int in = l == 0 ? S : ph;
            const float sw = x3_scale(pol.kernels[l], (size_t)in * ph);
            pack_x3_layer(pol.kernels[l], in, ph, l == 0 ? 1 : PP, TP, 1, sw, hh + 2 * p.pw_off[l]);
            out->pwinv[l] = (1.0f / sw) * (l == 0 ? 1.0f / 2048.0f : 1.0f / 4096.0f);
        }
        std::vector<float> wo((size_t)ph * 16, 0.f);    // output kernel with its columns at rows S-16+j
        for (int k = 0; k < ph; ++k)
            for (int n = 0; n < 16; ++n)
                if (rowmap[n] >= 0) wo[(size_t)k * 16 + n] = pol.kernels[PL][(size_t)k * A + rowmap[n]];
        const float sw = x3_scale(pol.kernels[PL], (size_t)ph * A);
        pack_x3_layer(wo.data(), ph, 16, PP, 1, 1, sw, hh + 2 * p.pw_off[PL]);
        out->pwinv[PL] = (1.0f / sw) * (1.0f / 4096.0f);
    } else {
        const int tb = TP / p.nw;
        pack_layer(pol.kernels[0], S, ph, 2, TP, tb, out->w.data() + p.pw_off[0]);
        for (int l = 1; l < PL; ++l) pack_layer(pol.kernels[l], ph, ph, TP, TP, tb, out->w.data() + p.pw_off[l]);
        pack_out_rows(pol.kernels[PL], ph, A, TP, rowmap, out->w.data() + p.pw_off[PL]);
    }
    out->b.assign((size_t)PL * PHP + kPolParams, 0.f);
    for (int l = 0; l < PL; ++l) std::memcpy(out->b.data() + (size_t)l * PHP, pol.biases[l], sizeof(float) * ph);
    float* pm = out->b.data() + (size_t)PL * PHP;       // [obmean 32][obstd 32][logstd 16][outbias 16]
    for (int d = 0; d < 32; ++d) {
        pm[d] = d < S ? pol.ob_mean[d] : 0.f;
        pm[32 + d] = d < S ? pol.ob_std[d] : 1.f;
    }
    for (int j = 0; j < A; ++j) {
        pm[64 + j] = pol.logstd[j];
        pm[80 + (S - 16 + j)] = pol.biases[PL][j];
    }
}

void pack_value_net(const bcmpc_value_net& v, PackedValue* out) {
    *out = PackedValue{};
    const int L = v.n_layers, h = v.hidden, S = v.state_dim;
    const int HP = out->HP = terminal_value_padded(h), T = HP / 16, TB = std::min(T, 4);
    // packed kernels: [2 -> T] [T -> T] x (L - 1) [T -> 1], 256 floats per fragment
    size_t* off = out->off;
    off[0] = 0;
    off[1] = (size_t)2 * T * 256;
    for (int l = 1; l < L; ++l) off[l + 1] = off[l] + (size_t)T * T * 256;
    off[L + 1] = off[L] + (size_t)T * 256;
    out->w.assign(off[L + 1], 0.f);
    out->params.assign((size_t)kTvParamFloats, 0.f);
    float* hp = out->params.data();
    pack_layer(v.kernels[0], S, h, 2, T, TB, out->w.data() + off[0]);
    for (int l = 1; l < L; ++l) pack_layer(v.kernels[l], h, h, T, T, TB, out->w.data() + off[l]);
    pack_layer(v.kernels[L], h, 1, T, 1, 1, out->w.data() + off[L]);
    for (int i = 0; i < S; ++i) {
        hp[i] = v.ob_mean[i];
        hp[32 + i] = v.ob_std[i];
    }
    for (int i = S; i < 32; ++i) hp[32 + i] = 1.f;
    for (int l = 0; l < L; ++l) std::copy(v.biases[l], v.biases[l] + h, hp + 64 + (size_t)l * HP);
    hp[64 + (size_t)L * HP] = v.biases[L][0];
}

// ---- the owning copies ----

const float* const* LayerCopy::ptrs() const {
    p.clear();
    for (const auto& x : v) p.push_back(x.data());
    return p.empty() ? nullptr : p.data();
}

void WeightsCopy::capture(const EnginePlan& p, const bcmpc_weights& w) {
    *this = WeightsCopy{};
    const bcmpc_config& c = p.cfg;
    const int L = c.n_layers, S = c.state_dim, A = c.action_dim, h = c.hidden;
    const bool rw = p.reward;
    const int nk = rw ? 5 : L + 1, nln = rw ? 3 : L;
    const int nin[5] = {S + A, h, h, h, h}, nout[5] = {h, h, S, h, 1};   // (reward net: dense .. dense_4)
    for (int l = 0; l < nk; ++l) {
        const int in = rw ? nin[l] : (l == 0 ? S + A : h), out = rw ? nout[l] : (l == L ? S : h);
        k.add(w.kernels[l], (size_t)in * out);
        b.add(w.biases[l], out);
    }
    for (int l = 0; l < nln && c.layer_norm; ++l) {
        g.add(w.ln_gamma[l], h);
        beta.add(w.ln_beta[l], h);
    }
    mean_obs.assign(w.mean_obs, w.mean_obs + S);
    std_obs.assign(w.std_obs, w.std_obs + S);
    mean_action.assign(w.mean_action, w.mean_action + A);
    std_action.assign(w.std_action, w.std_action + A);
    mean_deltas.assign(w.mean_deltas, w.mean_deltas + S);
    std_deltas.assign(w.std_deltas, w.std_deltas + S);
    if (rw) {
        mean_reward.assign(w.mean_reward, w.mean_reward + 1);
        std_reward.assign(w.std_reward, w.std_reward + 1);
    }
}

bcmpc_weights WeightsCopy::view() const {
    bcmpc_weights w{};
    w.kernels = k.ptrs(); w.biases = b.ptrs();
    w.ln_gamma = g.ptrs(); w.ln_beta = beta.ptrs();     // (null without LayerNorm)
    w.mean_obs = mean_obs.data(); w.std_obs = std_obs.data();
    w.mean_action = mean_action.data(); w.std_action = std_action.data();
    w.mean_deltas = mean_deltas.data(); w.std_deltas = std_deltas.data();
    w.mean_reward = mean_reward.empty() ? nullptr : mean_reward.data();
    w.std_reward = std_reward.empty() ? nullptr : std_reward.data();
    return w;
}

void PolicyCopy::capture(const EnginePlan& p, const bcmpc_policy& pol) {
    *this = PolicyCopy{};
    const int S = p.cfg.state_dim, A = p.cfg.action_dim, ph = p.cfg.policy_hidden;
    for (int l = 0; l <= p.PL; ++l) {
        const int in = l == 0 ? S : ph, out = l == p.PL ? A : ph;
        k.add(pol.kernels[l], (size_t)in * out);
        b.add(pol.biases[l], out);
    }
    ob_mean.assign(pol.ob_mean, pol.ob_mean + S);
    ob_std.assign(pol.ob_std, pol.ob_std + S);
    logstd.assign(pol.logstd, pol.logstd + A);
}

bcmpc_policy PolicyCopy::view(double explore) const {
    return bcmpc_policy{k.ptrs(), b.ptrs(), ob_mean.data(), ob_std.data(), logstd.data(), explore};
}

void ValueCopy::capture(const bcmpc_value_net& v) {
    *this = ValueCopy{};
    L = v.n_layers; hidden = v.hidden; S = v.state_dim;
    for (int l = 0; l <= L; ++l) {
        const int in = l == 0 ? S : hidden, out = l == L ? 1 : hidden;
        k.add(v.kernels[l], (size_t)in * out);
        b.add(v.biases[l], out);
    }
    ob_mean.assign(v.ob_mean, v.ob_mean + S);
    ob_std.assign(v.ob_std, v.ob_std + S);
}

bcmpc_value_net ValueCopy::view() const {
    return bcmpc_value_net{k.ptrs(), b.ptrs(), ob_mean.data(), ob_std.data(), L, hidden, S, 0};
}

}  // namespace bcmpc::host

// ac_fit_plan.cpp -- the host checks and sizing of the actor-critic fitter (include/bcmpc.h bcmpc_acfit_*).
// No HIP here: everything in this unit answers without a device, so every refusal is testable on a CPU.
#include "ac_fit_plan.h"

#include <algorithm>
#include <cmath>

namespace {
thread_local std::string g_acfit_error;
}

namespace bcmpc::acfit {

int fail(int code, const std::string& msg) {
    g_acfit_error = msg;
    return code;
}

int check_shape(int head, int state_dim, int out_dim, int hidden, int n_layers) {
    if (head != BCMPC_ACFIT_POLICY && head != BCMPC_ACFIT_VALUE)
        return fail(BCMPC_ERR_ARG, "head must be BCMPC_ACFIT_POLICY or BCMPC_ACFIT_VALUE");
    if (n_layers < 1 || n_layers > BCMPC_ACFIT_MAX_LAYERS)
        return fail(BCMPC_ERR_UNSUPPORTED, "n_layers outside [1, 4]");
    if (hidden < 1 || hidden > BCMPC_ACFIT_MAX_HIDDEN) return fail(BCMPC_ERR_UNSUPPORTED, "hidden outside [1, 256]");
    if (state_dim < 1 || state_dim > BCMPC_MAX_STATE) return fail(BCMPC_ERR_UNSUPPORTED, "state_dim outside [1, 32]");
    if (head == BCMPC_ACFIT_POLICY && (out_dim < 1 || out_dim > BCMPC_MAX_ACTION))
        return fail(BCMPC_ERR_UNSUPPORTED, "policy head: out_dim (the action dim) outside [1, 16]");
    if (head == BCMPC_ACFIT_VALUE && out_dim != 1) return fail(BCMPC_ERR_UNSUPPORTED, "value head: out_dim must be 1");
    return BCMPC_OK;
}

size_t lds_words(int hidden, int n_layers, int state_dim, int out_dim) {
    const int wmax = std::max(hidden, std::max(state_dim, out_dim));
    const size_t ld = (size_t)(wmax + 3) / 4 * 4 + 4;
    return (size_t)(2 + n_layers) * kRows * ld + (size_t)kRows * kTgtLd + kWaves + (size_t)kWaves * 256;
}

int make_plan(const bcmpc_acfit_config* c, Plan* out) {
    if (!c || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = check_shape(c->head, c->state_dim, c->out_dim, c->hidden, c->n_layers)) return rc;
    if (c->batch_size < 1) return fail(BCMPC_ERR_ARG, "batch_size must be >= 1");
    if (!(c->beta1 >= 0.f && c->beta1 < 1.f) || !(c->beta2 >= 0.f && c->beta2 < 1.f))
        return fail(BCMPC_ERR_ARG, "beta1 / beta2 outside [0, 1)");
    if (!(c->epsilon >= 0.f) || !std::isfinite(c->epsilon)) return fail(BCMPC_ERR_ARG, "epsilon negative or not finite");
    if (c->device < 0) return fail(BCMPC_ERR_ARG, "device ordinal out of range");
    Plan p;
    p.cfg = *c;
    p.S = c->state_dim; p.N = c->out_dim; p.h = c->hidden; p.L = c->n_layers;
    const int wmax = std::max(p.h, std::max(p.S, p.N));
    p.ld = (wmax + 3) / 4 * 4 + 4;
    p.lds_words = lds_words(p.h, p.L, p.S, p.N);
    if (p.lds_words > kLdsMaxWords) return fail(BCMPC_ERR_UNSUPPORTED, "the row block does not fit the LDS");
    size_t off = 0;
    for (int l = 0; l <= p.L; ++l) {
        const int in = l == 0 ? p.S : p.h, o = l == p.L ? p.N : p.h;
        p.lin[l] = in; p.lout[l] = o;
        p.w_off[l] = (int32_t)off; off += (size_t)in * o;
        p.b_off[l] = (int32_t)off; off += o;
        for (int k0 = 0; k0 <= in; k0 += 16)              // weight tiles incl. the bias row k == in
            for (int n0 = 0; n0 < o; n0 += 16) p.tiles.push_back({0, l, k0, n0});
    }
    p.tiles.push_back({3, 0, 0, 0});                      // loss + step counter
    p.n_params = off;
    *out = std::move(p);
    return BCMPC_OK;
}

int check_run(const int64_t* indices, const int32_t* batch_sizes, int32_t iterations, float lr, int64_t n_data,
              int64_t* total, int32_t* bmax) {
    if (iterations < 0 || (iterations > 0 && (!indices || !batch_sizes))) return fail(BCMPC_ERR_ARG, "null argument");
    if (!std::isfinite(lr)) return fail(BCMPC_ERR_ARG, "learning_rate must be finite");
    int64_t t = 0;
    int32_t bm = 0;
    for (int i = 0; i < iterations; ++i) {
        if (batch_sizes[i] < 1) return fail(BCMPC_ERR_ARG, "batch size must be >= 1");
        t += batch_sizes[i];
        bm = std::max(bm, batch_sizes[i]);
    }
    for (int64_t i = 0; i < t; ++i)
        if (indices[i] < 0 || indices[i] >= n_data) return fail(BCMPC_ERR_ARG, "sample index out of range");
    *total = t;
    *bmax = bm;
    return BCMPC_OK;
}

int check_filter(const float* mean, const float* std, int S) {
    if (!mean || !std) return fail(BCMPC_ERR_ARG, "null argument");
    for (int i = 0; i < S; ++i)
        if (!std::isfinite(mean[i]) || !std::isfinite(std[i]) || !(std[i] > 0.f))
            return fail(BCMPC_ERR_ARG, "ob_mean / ob_std must be finite, ob_std > 0");
    return BCMPC_OK;
}

void filter_image(const float* mean, const float* std, int S, float* out) {
    for (int i = 0; i < 32; ++i) {
        out[i] = i < S ? mean[i] : 0.f;
        out[32 + i] = i < S ? std[i] : 1.f;
    }
}

}  // namespace bcmpc::acfit

extern "C" {

const char* bcmpc_acfit_last_error(void) { return g_acfit_error.c_str(); }

int64_t bcmpc_acfit_lds_words(int32_t hidden, int32_t n_layers, int32_t state_dim, int32_t out_dim, int32_t head) {
    if (bcmpc::acfit::check_shape(head, state_dim, out_dim, hidden, n_layers)) return -1;
    const size_t w = bcmpc::acfit::lds_words(hidden, n_layers, state_dim, out_dim);
    return w <= bcmpc::acfit::kLdsMaxWords ? (int64_t)w : -1;
}

}  // extern "C"

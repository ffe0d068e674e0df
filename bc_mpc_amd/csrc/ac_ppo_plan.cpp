// ac_ppo_plan.cpp -- the host checks and sizing of the PPO trainer (include/bcmpc.h bcmpc_acppo_*).  No HIP here:
// everything in this unit answers without a device, so every refusal is testable on a CPU.  Errors share the
// actor-critic fitter's text slot (bcmpc_acfit_last_error): a PPO run reports the policy fitter's BC step too.
#include "ac_ppo_plan.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace bcmpc::acppo {

using acfit::fail;

size_t lds_words(int hidden, int n_layers, int state_dim, int action_dim) {
    return acfit::lds_words(hidden, n_layers, state_dim, action_dim) + 16 * 16 + 8 * 16 + 2 * 16;
}

int make_plan(const bcmpc_acppo_config* c, const bcmpc_acfit_config* pol, const bcmpc_acfit_config* val, Plan* out) {
    if (!c || !pol || !val || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (pol->head != BCMPC_ACFIT_POLICY) return fail(BCMPC_ERR_ARG, "the first fitter must be a BCMPC_ACFIT_POLICY head");
    if (val->head != BCMPC_ACFIT_VALUE) return fail(BCMPC_ERR_ARG, "the second fitter must be a BCMPC_ACFIT_VALUE head");
    if (const int rc = acfit::check_shape(pol->head, pol->state_dim, pol->out_dim, pol->hidden, pol->n_layers)) return rc;
    if (const int rc = acfit::check_shape(val->head, val->state_dim, val->out_dim, val->hidden, val->n_layers)) return rc;
    if (pol->state_dim != val->state_dim) return fail(BCMPC_ERR_ARG, "the fitters differ in state_dim");
    if (pol->hidden != val->hidden) return fail(BCMPC_ERR_ARG, "the fitters differ in hidden");
    if (pol->n_layers != val->n_layers) return fail(BCMPC_ERR_ARG, "the fitters differ in n_layers");
    if (pol->device != val->device) return fail(BCMPC_ERR_ARG, "the fitters are on different devices");
    if (!(c->beta1 >= 0.f && c->beta1 < 1.f) || !(c->beta2 >= 0.f && c->beta2 < 1.f))
        return fail(BCMPC_ERR_ARG, "beta1 / beta2 outside [0, 1)");
    if (!(c->epsilon >= 0.f) || !std::isfinite(c->epsilon)) return fail(BCMPC_ERR_ARG, "epsilon negative or not finite");
    Plan p;
    p.cfg = *c;
    p.S = pol->state_dim; p.A = pol->out_dim; p.h = pol->hidden; p.L = pol->n_layers; p.device = pol->device;
    const int wmax = std::max(p.h, std::max(p.S, p.A));
    p.ld = (wmax + 3) / 4 * 4 + 4;
    p.lds_words = lds_words(p.h, p.L, p.S, p.A);
    if (p.lds_words > acfit::kLdsMaxWords) return fail(BCMPC_ERR_UNSUPPORTED, "the row block does not fit the LDS");
    for (int s = 0; s < 2; ++s)
        for (int l = 0; l <= p.L; ++l) {
            const int in = l == 0 ? p.S : p.h, o = l == p.L ? (s == 0 ? p.A : 1) : p.h;
            for (int k0 = 0; k0 <= in; k0 += 16)          // weight tiles incl. the bias row k == in
                for (int n0 = 0; n0 < o; n0 += 16) p.tasks.push_back({0, s, l, k0, n0});
        }
    p.tasks.push_back({2, 0, 0, 0, 0});                   // logstd
    p.tasks.push_back({3, 0, 0, 0, 0});                   // losses + step counter
    *out = std::move(p);
    return BCMPC_OK;
}

int check_hyper(float lr, float eps, float entcoeff) {
    if (!std::isfinite(lr)) return fail(BCMPC_ERR_ARG, "learning_rate must be finite");
    if (!std::isfinite(eps) || eps < 0.f) return fail(BCMPC_ERR_ARG, "eps (clip_param * cur_lrmult) must be finite and >= 0");
    if (!std::isfinite(entcoeff)) return fail(BCMPC_ERR_ARG, "entcoeff must be finite");
    return BCMPC_OK;
}

int check_state(bool has_logstd, bool has_old, bool has_data, bool pol_weights, bool val_weights, bool pol_filter) {
    if (!pol_weights || !val_weights) return fail(BCMPC_ERR_STATE, "bcmpc_acfit_set_params has not been called on both fitters");
    if (!pol_filter) return fail(BCMPC_ERR_STATE, "bcmpc_acfit_set_filter has not been called on the policy fitter");
    if (!has_logstd) return fail(BCMPC_ERR_STATE, "bcmpc_acppo_set_logstd has not been called");
    if (!has_old) return fail(BCMPC_ERR_STATE, "bcmpc_acppo_set_old has not been called");
    if (!has_data) return fail(BCMPC_ERR_STATE, "bcmpc_acppo_set_data has not been called");
    return BCMPC_OK;
}

int check_finite(const float* x, int64_t n, const char* what) {
    if (!x) return fail(BCMPC_ERR_ARG, "null argument");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return fail(BCMPC_ERR_ARG, std::string(what) + " must be finite");
    return BCMPC_OK;
}

}  // namespace bcmpc::acppo

extern "C" {

const char* bcmpc_acppo_last_error(void) { return bcmpc_acfit_last_error(); }

int64_t bcmpc_acppo_lds_words(int32_t hidden, int32_t n_layers, int32_t state_dim, int32_t action_dim) {
    if (bcmpc::acfit::check_shape(BCMPC_ACFIT_POLICY, state_dim, action_dim, hidden, n_layers)) return -1;
    const size_t w = bcmpc::acppo::lds_words(hidden, n_layers, state_dim, action_dim);
    return w <= bcmpc::acfit::kLdsMaxWords ? (int64_t)w : -1;
}

int bcmpc_acppo_check_pair(const bcmpc_acppo_config* cfg, const bcmpc_acfit_config* policy,
                           const bcmpc_acfit_config* value) {
    bcmpc::acppo::Plan p;
    return bcmpc::acppo::make_plan(cfg, policy, value, &p);
}

int bcmpc_acppo_check_run(const int64_t* indices, const int32_t* batch_sizes, int32_t iterations, int64_t n_data,
                          float learning_rate, float eps, float entcoeff) {
    if (const int rc = bcmpc::acppo::check_hyper(learning_rate, eps, entcoeff)) return rc;
    int64_t total = 0;
    int32_t bmax = 0;
    return bcmpc::acfit::check_run(indices, batch_sizes, iterations, learning_rate, n_data, &total, &bmax);
}

}  // extern "C"

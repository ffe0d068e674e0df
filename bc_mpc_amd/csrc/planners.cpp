// planners.cpp -- CEM and MPPI on the device: the single-plan chain, the batched plans (plan_batch.hip), what
// they sample (plan_noise.hip) and the model ensembles.
#include "host_internal.h"

using namespace bcmpc::host;

extern "C" {

static int cem_buffers(bcmpc_engine* e, int32_t n_elite) {
    const size_t ha = (size_t)e->cfg.horizon * e->cfg.action_dim;
    if (!e->d_mu) {
        HIP_TRY(hipMalloc(&e->d_mu, ha * sizeof(double)));
        HIP_TRY(hipMalloc(&e->d_sigma, ha * sizeof(double)));
        HIP_TRY(hipMalloc(&e->d_count, sizeof(int32_t)));
    }
    if (n_elite > e->elite_cap) {
        if (e->d_elite) (void)hipFree(e->d_elite);
        e->d_elite = nullptr;
        e->elite_cap = 0;
        HIP_TRY(hipMalloc(&e->d_elite, (size_t)n_elite * sizeof(bcmpc_elite)));
        e->elite_cap = n_elite;
    }
    return BCMPC_OK;
}

static int select_impl(bcmpc_engine* e, const bcmpc_elite* d_pairs, const double* d_costs, int64_t m,
                       int64_t index_base, int32_t n_elite, bcmpc_elite* d_out, int32_t* d_count, hipStream_t st) {
    if (n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (m < 0 || (!d_pairs && !d_costs) || !d_out || !d_count) return fail(BCMPC_ERR_ARG, "null argument");
    SelectArgs s{};
    s.pairs = d_pairs; s.costs = d_costs; s.m = m; s.index_base = index_base; s.n_elite = n_elite;
    s.maximize = e->cfg.cost == BCMPC_COST_REWARD;
    s.out = d_out; s.count = d_count;
    HIP_TRY(launch_select(s, st));
    return BCMPC_OK;
}

static int refit_impl(bcmpc_engine* e, const bcmpc_elite* d_elite, const int32_t* d_count, uint64_t seed,
                      int32_t iter, double alpha, double* d_mu, double* d_sigma, hipStream_t st) {
    if (!d_elite || !d_count || !d_mu || !d_sigma) return fail(BCMPC_ERR_ARG, "null argument");
    RefitArgs r{};
    r.elite = d_elite; r.count = d_count; r.mu = d_mu; r.sigma = d_sigma; r.consts = e->d_consts;
    r.seed = seed; r.iter = iter; r.H = e->cfg.horizon; r.A = e->cfg.action_dim; r.alpha = alpha;
    HIP_TRY(launch_refit(r, st));
    return BCMPC_OK;
}

// one MPPI update on st (mppi.hip): the scratch is grown like cem_buffers grows the elite buffer
static int mppi_update_impl(bcmpc_engine* e, const double* d_costs, int64_t m, int64_t cand_offset, uint64_t seed,
                            int32_t iter, double lambda, double* d_mu, const double* d_sigma,
                            bcmpc_mppi_stats* d_stats, hipStream_t st) {
    if (!d_costs || !d_mu || !d_sigma || !d_stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (m < 1) return fail(BCMPC_ERR_ARG, "m must be >= 1");
    if (iter < 0 || iter >= (1 << 22)) return fail(BCMPC_ERR_ARG, "iteration must be in [0, 2^22)");
    if (!(std::isfinite(lambda) && lambda > 0.0)) return fail(BCMPC_ERR_ARG, "lambda must be finite and > 0");
    // (the action bounds reach the device with the weights or with bcmpc_set_action_bounds)
    if (!e->has_weights) return fail(BCMPC_ERR_STATE, "bcmpc_set_weights has not been called");
    const int64_t parts = mppi_parts(m);
    if (parts > 0x7fffffff) return fail(BCMPC_ERR_UNSUPPORTED, "m is too large for one update");
    const size_t ha = (size_t)e->cfg.horizon * e->cfg.action_dim;
    const size_t need = 2 * (size_t)kMppiMinParts + (ha + 2) * (size_t)parts;
    if (need > e->mppi_cap) {
        if (e->d_mppi) (void)hipFree(e->d_mppi);
        e->d_mppi = nullptr;
        e->mppi_cap = 0;
        HIP_TRY(hipMalloc(&e->d_mppi, need * sizeof(double)));
        e->mppi_cap = need;
    }
    MppiArgs a{};
    a.costs = d_costs; a.mu = d_mu; a.sigma = d_sigma; a.consts = e->d_consts;
    a.pmin = e->d_mppi;
    a.pcnt = reinterpret_cast<int64_t*>(e->d_mppi + kMppiMinParts);
    a.part = e->d_mppi + 2 * kMppiMinParts;
    a.stats = d_stats;
    a.seed = seed; a.m = m; a.cand_offset = cand_offset; a.nparts = parts;
    a.iter = iter; a.H = e->cfg.horizon; a.A = e->cfg.action_dim;
    a.cpl = mppi_cpl(m); a.nmin = mppi_min_blocks(m);
    a.maximize = e->cfg.cost == BCMPC_COST_REWARD;
    a.lambda = lambda;
    HIP_TRY(launch_mppi_update(a, st));
    return BCMPC_OK;
}

// The planner parameters' checks of the synchronous entry points: iterations and n_elite or lambda, then (after
// whatever check of its own an entry ranks between them) k_global against the entry's K, spelled k_text in the message
static int cem_param_check(const bcmpc_cem* p) {
    if (p->iterations < 1 || p->iterations > (1 << 22)) return fail(BCMPC_ERR_ARG, "iterations must be in [1, 2^22]");
    if (p->n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    return BCMPC_OK;
}
static int mppi_param_check(const bcmpc_mppi* p) {
    if (p->iterations < 1 || p->iterations > (1 << 22)) return fail(BCMPC_ERR_ARG, "iterations must be in [1, 2^22]");
    if (!(std::isfinite(p->lambda) && p->lambda > 0.0)) return fail(BCMPC_ERR_ARG, "lambda must be finite and > 0");
    return BCMPC_OK;
}
static int k_global_check(int64_t k_global, const char* prefix, int64_t K, const char* k_text = "num_paths") {
    if (k_global != 0 && k_global != K) return fail(BCMPC_ERR_ARG, std::string(prefix) + ": k_global must be 0 or " + k_text);
    return BCMPC_OK;
}

// The sampling distribution of a planner call (bcmpc_sampling; nullptr: the default -- white noise, nothing carried)
static bool sampling_default(const bcmpc_sampling* s) { return !s || (s->rho == 0.0 && s->keep_elites == 0); }
static int rho_check(double rho) {
    if (!(std::isfinite(rho) && rho >= 0.0 && rho < 1.0)) return fail(BCMPC_ERR_ARG, "rho must be finite and in [0, 1)");
    return BCMPC_OK;
}
static int sampling_check(const bcmpc_sampling* s, bool mppi) {
    if (!s) return BCMPC_OK;
    if (const int rc = rho_check(s->rho)) return rc;
    if (s->keep_elites != 0 && s->keep_elites != 1) return fail(BCMPC_ERR_ARG, "keep_elites must be 0 or 1");
    if (mppi && s->keep_elites) return fail(BCMPC_ERR_ARG, "keep_elites is a CEM setting: MPPI has no elites to carry");
    return BCMPC_OK;
}

// MPPI's control-cost term and sigma update (bcmpc_mppi_ext; nullptr or both switched off: the plain update)
static bool mppi_ext_default(const bcmpc_mppi_ext* x) { return !x || (x->control_weight == 0.0 && x->adapt_sigma == 0); }
static int control_weight_check(double w) {
    if (!(std::isfinite(w) && w >= 0.0)) return fail(BCMPC_ERR_ARG, "control_weight must be finite and >= 0");
    return BCMPC_OK;
}
static int sigma_step_check(double alpha, double min_std, double max_std) {
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(BCMPC_ERR_ARG, "sigma_alpha must be in [0, 1]");
    if (!(std::isfinite(min_std) && min_std >= 0.0)) return fail(BCMPC_ERR_ARG, "min_std must be finite and >= 0");
    if (!(max_std >= min_std)) return fail(BCMPC_ERR_ARG, "max_std must be >= min_std");
    return BCMPC_OK;
}
static int mppi_ext_check(const bcmpc_mppi_ext* x) {
    if (!x) return BCMPC_OK;
    if (const int rc = control_weight_check(x->control_weight)) return rc;
    if (x->adapt_sigma != 0 && x->adapt_sigma != 1) return fail(BCMPC_ERR_ARG, "adapt_sigma must be 0 or 1");
    if (x->reserved != 0) return fail(BCMPC_ERR_ARG, "bcmpc_mppi_ext.reserved must be zero");
    return sigma_step_check(x->sigma_alpha, x->min_std, x->max_std);
}

// Proposals (bcmpc_proposals; nullptr or count == 0: none).  The source's three element strides over the extents
// (n_envs, P, H), j innermost with stride 1 and extent A: refused when two elements could share an address --
// taken from the smallest stride to the largest over the dimensions of extent > 1, each must cover what lies below it
static bool proposals_none(const bcmpc_proposals* q) { return !q || q->count == 0; }
static int prop_strides_check(int32_t n_envs, int32_t P, int32_t H, int32_t A, int64_t env_stride, int64_t seq_stride,
                              int64_t step_stride) {
    struct Dim { int64_t stride, extent; } d[3] = {{env_stride, n_envs}, {seq_stride, P}, {step_stride, H}};
    for (const Dim& x : d)
        if (x.stride < 0) return fail(BCMPC_ERR_ARG, "proposals: the strides must be >= 0");
    std::sort(d, d + 3, [](const Dim& x, const Dim& y) { return x.stride < y.stride; });
    int64_t below = A;                                  // elements the dimensions so far span
    for (const Dim& x : d) {
        if (x.extent <= 1) continue;
        if (x.stride < below) return fail(BCMPC_ERR_ARG, "proposals: the strides alias (two elements share an address)");
        if (x.stride > INT64_MAX / x.extent) return fail(BCMPC_ERR_ARG, "proposals: a stride is too large");
        below = x.stride * x.extent;
    }
    return BCMPC_OK;
}
// what a call's struct shows on its own, asked before the engine is looked at ...
static int proposals_struct_check(const bcmpc_proposals* q) {
    if (q->count < 0) return fail(BCMPC_ERR_ARG, "proposals: count must be >= 0");
    if (!q->sequences) return fail(BCMPC_ERR_ARG, "proposals: sequences is NULL");
    if (q->device != 0 && q->device != 1) return fail(BCMPC_ERR_ARG, "proposals: device must be 0 (host) or 1 (device)");
    if (q->env_stride < 0 || q->seq_stride < 0 || q->step_stride < 0)
        return fail(BCMPC_ERR_ARG, "proposals: the strides must be >= 0");
    return BCMPC_OK;
}
// ... and against the call's K candidates per environment; n_elite: CEM's with keep_elites, else 0
static int proposals_check(const bcmpc_proposals* q, const bcmpc_engine* e, int32_t n_envs, int64_t K, int32_t n_elite) {
    if ((int64_t)q->count + n_elite > K)
        return fail(BCMPC_ERR_ARG, n_elite ? "proposals: count + n_elite must be <= K (the carried elites keep the first columns)"
                                           : "proposals: count must be <= K (candidates per environment)");
    const int32_t H = e->cfg.horizon, A = e->cfg.action_dim;
    if (q->device == 0) {
        const bool zero = q->env_stride == 0 && q->seq_stride == 0 && q->step_stride == 0;
        const bool canon = q->env_stride == (int64_t)q->count * H * A && q->seq_stride == (int64_t)H * A && q->step_stride == A;
        if (!zero && !canon)
            return fail(BCMPC_ERR_ARG, "proposals: host sequences are [n_envs][P][H][A] (strides 0, or P*H*A, H*A, A)");
        return BCMPC_OK;
    }
    return prop_strides_check(n_envs, q->count, H, A, q->env_stride, q->seq_stride, q->step_stride);
}

// Knot plans (bcmpc_knots; nullptr or count == 0: off -- the plans are [H][A] and every step is sampled)
static bool knots_none(const bcmpc_knots* k) { return !k || k->count == 0; }
static int knots_check(int32_t count, int32_t kind, int32_t horizon) {
    if (count < 1 || count > horizon)
        return fail(BCMPC_ERR_ARG, "knots: count must be in [1, horizon = " + std::to_string(horizon) + "]");
    if (kind < BCMPC_KNOTS_HOLD || kind > BCMPC_KNOTS_CUBIC)
        return fail(BCMPC_ERR_ARG, "knots: kind must be 0 (hold), 1 (linear) or 2 (cubic)");
    return BCMPC_OK;
}
static int steps_check(int32_t steps, int32_t horizon) {
    if (steps < 1 || steps > horizon)
        return fail(BCMPC_ERR_ARG, "steps must be in [1, horizon = " + std::to_string(horizon) + "]");
    return BCMPC_OK;
}

// a synchronous planner call's input plans, kept on a team engine for the rerun after a give-up: n doubles of
// mu, and of sigma where the call writes it back (CEM)
struct PlanInputs {
    std::vector<double> mu, sigma;
    PlanInputs(bool keep, const double* mu_in, const double* sigma_in, size_t n) {
        if (keep) mu.assign(mu_in, mu_in + n);
        if (keep && sigma_in) sigma.assign(sigma_in, sigma_in + n);
    }
    void restore(double* mu_out, double* sigma_out) const {
        std::memcpy(mu_out, mu.data(), mu.size() * sizeof(double));
        if (!sigma.empty()) std::memcpy(sigma_out, sigma.data(), sigma.size() * sizeof(double));
    }
};

int bcmpc_cem_rollout_async(bcmpc_engine* e, const double* d_state, const double* d_mu, const double* d_sigma,
                            uint64_t seed, int32_t iteration, int64_t cand_offset, int64_t k_global,
                            double* d_costs, bcmpc_result* d_result, int32_t merge, void* stream) {
    if (!e || !d_state || !d_mu || !d_sigma || !d_costs) return fail(BCMPC_ERR_ARG, "null argument");
    if (iteration < 0 || iteration >= (1 << 22)) return fail(BCMPC_ERR_ARG, "iteration must be in [0, 2^22)");
    if (k_global < e->cfg.num_paths + cand_offset) return fail(BCMPC_ERR_ARG, "k_global smaller than this shard's range");
    HIP_TRY(hipSetDevice(e->cfg.device));
    const CemLaunch cl{d_mu, d_sigma, iteration, merge != 0, (int64_t)iteration * k_global + cand_offset};
    RolloutLaunch r;
    r.state = d_state; r.seed = seed; r.cand_offset = cand_offset; r.costs = d_costs; r.result = d_result;
    r.stream = (hipStream_t)stream; r.cem = &cl;
    return rollout_impl(e, r);
}

int bcmpc_select_async(bcmpc_engine* e, const bcmpc_elite* d_pairs, const double* d_costs, int64_t m,
                       int64_t index_base, int32_t n_elite, bcmpc_elite* d_out, int32_t* d_count, void* stream) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return select_impl(e, d_pairs, d_costs, m, index_base, n_elite, d_out, d_count, (hipStream_t)stream);
}

int bcmpc_cem_refit_async(bcmpc_engine* e, const bcmpc_elite* d_elite, const int32_t* d_count, uint64_t seed,
                          int32_t iteration, double alpha, double* d_mu, double* d_sigma, void* stream) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return refit_impl(e, d_elite, d_count, seed, iteration, alpha, d_mu, d_sigma, (hipStream_t)stream);
}

int bcmpc_mppi_update_async(bcmpc_engine* e, const double* d_costs, int64_t m, int64_t cand_offset, uint64_t seed,
                            int32_t iteration, double lambda, double* d_mu, const double* d_sigma,
                            bcmpc_mppi_stats* d_stats, void* stream) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    // (arguments first: a bad call is answered before any HIP call)
    if (!d_costs || !d_mu || !d_sigma || !d_stats) return fail(BCMPC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return mppi_update_impl(e, d_costs, m, cand_offset, seed, iteration, lambda, d_mu, d_sigma, d_stats,
                            (hipStream_t)stream);
}

// ---- batched CEM / MPPI: n_envs plans per launch chain (plan_batch.hip) ----------------------
// The rollout kernels take one sampling distribution per launch, so the iteration's actions are
// materialised from the n_envs plans (plan_sample) and rolled out as an explicit action array by the
// batched chain; the outer-loop kernels run once per iteration with the environment as a grid index.
static int plan_block_check(const bcmpc_engine* e, int32_t n_envs, int64_t K, int32_t iteration) {
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (K < 1) return fail(BCMPC_ERR_ARG, "K (candidates per environment) must be >= 1");
    if (iteration < 0 || iteration >= (1 << 22)) return fail(BCMPC_ERR_ARG, "iteration must be in [0, 2^22)");
    // (the action bounds reach the device with the weights or with bcmpc_set_action_bounds)
    if (!e->has_weights) return fail(BCMPC_ERR_STATE, "bcmpc_set_weights has not been called");
    return BCMPC_OK;
}

static int plan_sample_impl(bcmpc_engine* e, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                            uint64_t seed, int32_t iteration, int64_t cand_offset, double* d_actions, hipStream_t st) {
    PlanSampleArgs a{};
    a.mu = d_mu; a.sigma = d_sigma; a.consts = e->d_consts; a.out = d_actions;
    a.seed = seed; a.cand_offset = cand_offset; a.K = K; a.Ktot = K * n_envs;
    a.iter = iteration; a.H = e->cfg.horizon; a.A = e->cfg.action_dim;
    HIP_TRY(launch_plan_sample(a, st));
    return BCMPC_OK;
}

// d_keep / d_keep_count (both or neither): the carried sequences [n_envs][n_elite][H][A] and their counts
static int plan_sample_corr_impl(bcmpc_engine* e, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                                 uint64_t seed, int32_t iteration, int64_t cand_offset, double rho, const double* d_keep,
                                 const int32_t* d_keep_count, int32_t n_elite, double* d_actions, hipStream_t st) {
    PlanSampleCorrArgs a{};
    a.mu = d_mu; a.sigma = d_sigma; a.consts = e->d_consts; a.out = d_actions;
    a.keep = d_keep; a.keep_count = d_keep_count;
    a.seed = seed; a.cand_offset = cand_offset; a.K = K; a.Ktot = K * n_envs;
    a.iter = iteration; a.H = e->cfg.horizon; a.A = e->cfg.action_dim; a.n_elite = n_elite;
    a.rho = rho; a.c = std::sqrt(1.0 - rho * rho);
    HIP_TRY(launch_plan_sample_corr(a, st));
    return BCMPC_OK;
}

// ... with environment b's last n_prop columns given: d_prop read through the three strides (plan_prop.hip)
static int plan_sample_prop_impl(bcmpc_engine* e, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                                 uint64_t seed, int32_t iteration, int64_t cand_offset, double rho, const double* d_keep,
                                 const int32_t* d_keep_count, int32_t n_elite, const double* d_prop, int32_t n_prop,
                                 int64_t env_stride, int64_t seq_stride, int64_t step_stride, double* d_actions,
                                 hipStream_t st) {
    PlanSamplePropArgs p{};
    PlanSampleCorrArgs& a = p.s;
    a.mu = d_mu; a.sigma = d_sigma; a.consts = e->d_consts; a.out = d_actions;
    a.keep = d_keep; a.keep_count = d_keep_count;
    a.seed = seed; a.cand_offset = cand_offset; a.K = K; a.Ktot = K * n_envs;
    a.iter = iteration; a.H = e->cfg.horizon; a.A = e->cfg.action_dim; a.n_elite = n_elite;
    a.rho = rho; a.c = std::sqrt(1.0 - rho * rho);
    p.prop = d_prop; p.n_prop = n_prop;
    p.env_stride = env_stride; p.seq_stride = seq_stride; p.step_stride = step_stride;
    HIP_TRY(launch_plan_sample_prop(p, st));
    return BCMPC_OK;
}

// ... in knot space (plan_knots.hip): the plans [n_envs][M][A], d_keep [n_envs][n_elite][M][A]; the clipped knots
// into d_knots [M][n_envs * K][A], their expansion into d_actions [H][n_envs * K][A]
static int plan_sample_knots_impl(bcmpc_engine* e, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                                  uint64_t seed, int32_t iteration, int64_t cand_offset, double rho, const double* d_keep,
                                  const int32_t* d_keep_count, int32_t n_elite, int32_t M, int32_t kind, double* d_knots,
                                  double* d_actions, hipStream_t st) {
    PlanSampleKnotsArgs p{};
    PlanSampleCorrArgs& a = p.s;
    a.mu = d_mu; a.sigma = d_sigma; a.consts = e->d_consts; a.out = d_actions;
    a.keep = d_keep; a.keep_count = d_keep_count;
    a.seed = seed; a.cand_offset = cand_offset; a.K = K; a.Ktot = K * n_envs;
    a.iter = iteration; a.H = e->cfg.horizon; a.A = e->cfg.action_dim; a.n_elite = n_elite;
    a.rho = rho; a.c = std::sqrt(1.0 - rho * rho);
    p.knots = d_knots; p.M = M; p.kind = kind;
    HIP_TRY(launch_plan_sample_knots(p, st));
    return BCMPC_OK;
}

static int plan_keep_impl(bcmpc_engine* e, const bcmpc_elite* d_elite, const int32_t* d_count, const double* d_actions,
                          int32_t n_envs, int64_t K, int64_t cand_offset, int32_t n_elite, double* d_keep,
                          int32_t* d_keep_count, hipStream_t st, int32_t steps = 0) {
    PlanKeepArgs a{};
    a.elite = d_elite; a.count = d_count; a.actions = d_actions; a.keep = d_keep; a.keep_count = d_keep_count;
    a.cand_offset = cand_offset; a.K = K; a.Ktot = K * n_envs;
    a.n_envs = n_envs; a.n_elite = n_elite; a.H = steps ? steps : e->cfg.horizon; a.A = e->cfg.action_dim;
    HIP_TRY(launch_plan_keep(a, st));
    return BCMPC_OK;
}

static int plan_argmin_impl(bcmpc_engine* e, const double* d_costs, const double* d_actions, int32_t n_envs, int64_t K,
                            int32_t iteration, int32_t merge, bcmpc_result* d_results, hipStream_t st) {
    PlanArgminArgs a{};
    a.costs = d_costs; a.actions = d_actions; a.consts = e->d_consts; a.out = d_results;
    a.K = K; a.n_envs = n_envs; a.A = e->cfg.action_dim; a.iter = iteration; a.merge = merge != 0;
    a.maximize = e->cfg.cost == BCMPC_COST_REWARD;
    HIP_TRY(launch_plan_argmin(a, st));
    return BCMPC_OK;
}

static int select_batch_impl(bcmpc_engine* e, const double* d_costs, int32_t n_envs, int64_t K, int64_t index_base,
                             int32_t n_elite, bcmpc_elite* d_out, int32_t* d_count, hipStream_t st) {
    SelectBatchArgs a{};
    a.one.costs = d_costs; a.one.m = K; a.one.index_base = index_base; a.one.n_elite = n_elite;
    a.one.maximize = e->cfg.cost == BCMPC_COST_REWARD;
    a.one.out = d_out; a.one.count = d_count;
    a.n_envs = n_envs;
    HIP_TRY(launch_select_batch(a, st));
    return BCMPC_OK;
}

// d_actions (optional): the iteration's stored actions [H][n_envs * K][A], column 0 = candidate cand_offset
static int refit_batch_impl(bcmpc_engine* e, const bcmpc_elite* d_elite, const int32_t* d_count, int32_t n_envs,
                            int32_t n_elite, uint64_t seed, int32_t iteration, double alpha, double* d_mu,
                            double* d_sigma, const double* d_actions, int64_t K, int64_t cand_offset, hipStream_t st,
                            int32_t steps = 0) {
    RefitBatchArgs a{};
    a.one.elite = d_elite; a.one.count = d_count; a.one.mu = d_mu; a.one.sigma = d_sigma; a.one.consts = e->d_consts;
    a.one.seed = seed; a.one.iter = iteration; a.one.H = steps ? steps : e->cfg.horizon; a.one.A = e->cfg.action_dim;
    a.one.alpha = alpha;
    a.one.actions = d_actions; a.one.act_cols = d_actions ? K * n_envs : 0; a.one.act_g0 = cand_offset;
    a.n_envs = n_envs; a.n_elite = n_elite;
    HIP_TRY(launch_refit_batch(a, st));
    return BCMPC_OK;
}

static int mppi_update_batch_impl(bcmpc_engine* e, const double* d_costs, int32_t n_envs, int64_t K,
                                  int64_t cand_offset, uint64_t seed, int32_t iteration, double lambda, double* d_mu,
                                  const double* d_sigma, bcmpc_mppi_stats* d_stats, const double* d_actions,
                                  hipStream_t st, int32_t steps = 0) {
    if (!(std::isfinite(lambda) && lambda > 0.0)) return fail(BCMPC_ERR_ARG, "lambda must be finite and > 0");
    const int64_t parts = mppi_parts(K);
    if (parts * n_envs > 0x7fffffff) return fail(BCMPC_ERR_UNSUPPORTED, "n_envs * K is too large for one update");
    const int32_t H = steps ? steps : e->cfg.horizon, ha = H * e->cfg.action_dim;
    const size_t need = mppi_batch_scratch(K, n_envs, ha);
    if (need > e->mppi_cap) {
        if (e->d_mppi) (void)hipFree(e->d_mppi);
        e->d_mppi = nullptr;
        e->mppi_cap = 0;
        HIP_TRY(hipMalloc(&e->d_mppi, need * sizeof(double)));
        e->mppi_cap = need;
    }
    MppiBatchArgs b{};
    MppiArgs& a = b.one;
    a.costs = d_costs; a.mu = d_mu; a.sigma = d_sigma; a.consts = e->d_consts;
    a.pmin = e->d_mppi;
    a.pcnt = reinterpret_cast<int64_t*>(e->d_mppi + (size_t)n_envs * kMppiMinParts);
    a.part = e->d_mppi + 2 * (size_t)n_envs * kMppiMinParts;
    a.stats = d_stats;
    a.seed = seed; a.m = K; a.cand_offset = cand_offset; a.nparts = parts;
    a.iter = iteration; a.H = H; a.A = e->cfg.action_dim;
    a.cpl = mppi_cpl(K); a.nmin = mppi_min_blocks(K);          // (the workgroup size rule follows K, not n_envs * K)
    a.maximize = e->cfg.cost == BCMPC_COST_REWARD;
    a.lambda = lambda;
    a.actions = d_actions; a.act_cols = d_actions ? K * n_envs : 0; a.act_g0 = cand_offset;
    b.n_envs = n_envs;
    HIP_TRY(launch_mppi_update_batch(b, st));
    return BCMPC_OK;
}

// c~ = costs +- weight q into d_scores (mppi_ext.hip): the plans are the ones the actions were sampled from
static int control_cost_impl(bcmpc_engine* e, const double* d_costs, const double* d_actions, int32_t n_envs, int64_t K,
                             const double* d_mu, const double* d_sigma, double weight, double* d_scores,
                             hipStream_t st, int32_t steps = 0) {
    const int32_t H = steps ? steps : e->cfg.horizon, ha = H * e->cfg.action_dim;
    if (mppi_control_lds(ha) > kMppiControlMaxLds)
        return fail(BCMPC_ERR_UNSUPPORTED, "horizon * action_dim is too large for the control-cost kernel's table");
    if ((K + 255) / 256 * n_envs > 0x7fffffff) return fail(BCMPC_ERR_UNSUPPORTED, "n_envs * K is too large for one launch");
    MppiControlArgs a{};
    a.costs = d_costs; a.actions = d_actions; a.mu = d_mu; a.sigma = d_sigma; a.out = d_scores;
    a.K = K; a.Ktot = K * n_envs; a.bpe = (K + 255) / 256;
    a.n_envs = n_envs; a.H = H; a.A = e->cfg.action_dim;
    a.maximize = e->cfg.cost == BCMPC_COST_REWARD;
    a.weight = weight;
    HIP_TRY(launch_mppi_control_cost(a, st));
    return BCMPC_OK;
}

// sigma' from the weights of d_scores about d_mu_new (mppi_ext.hip); the scratch is the update's, grown like it
static int sigma_update_impl(bcmpc_engine* e, const double* d_scores, const double* d_actions, int32_t n_envs, int64_t K,
                             double lambda, const double* d_mu_new, double* d_sigma, double alpha, double min_std,
                             double max_std, hipStream_t st, int32_t steps = 0) {
    const int64_t parts = mppi_parts(K);
    if (parts * n_envs > 0x7fffffff) return fail(BCMPC_ERR_UNSUPPORTED, "n_envs * K is too large for one update");
    const int32_t H = steps ? steps : e->cfg.horizon, ha = H * e->cfg.action_dim;
    const size_t need = mppi_sigma_scratch(K, n_envs, ha);
    if (need > e->mppi_cap) {
        if (e->d_mppi) (void)hipFree(e->d_mppi);
        e->d_mppi = nullptr;
        e->mppi_cap = 0;
        HIP_TRY(hipMalloc(&e->d_mppi, need * sizeof(double)));
        e->mppi_cap = need;
    }
    MppiSigmaArgs a{};
    a.scores = d_scores; a.actions = d_actions; a.mu_new = d_mu_new; a.sigma = d_sigma;
    a.pmin = e->d_mppi;
    a.pcnt = reinterpret_cast<int64_t*>(e->d_mppi + (size_t)n_envs * kMppiMinParts);
    a.part = e->d_mppi + 2 * (size_t)n_envs * kMppiMinParts;
    a.K = K; a.Ktot = K * n_envs; a.nparts = parts;
    a.n_envs = n_envs; a.H = H; a.A = e->cfg.action_dim;
    a.cpl = mppi_cpl(K); a.nmin = mppi_min_blocks(K);
    a.maximize = e->cfg.cost == BCMPC_COST_REWARD;
    a.lambda = lambda; a.alpha = alpha; a.min_std = min_std; a.max_std = max_std;
    HIP_TRY(launch_mppi_sigma_update(a, st));
    return BCMPC_OK;
}

int bcmpc_mppi_control_cost_async(bcmpc_engine* e, const double* d_costs, const double* d_actions, int32_t n_envs,
                                  int64_t K, const double* d_mu, const double* d_sigma, double weight,
                                  double* d_scores, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_costs || !d_actions || !d_mu || !d_sigma || !d_scores) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = control_weight_check(weight)) return rc;
    if (const int rc = plan_block_check(e, n_envs, K, 0)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return control_cost_impl(e, d_costs, d_actions, n_envs, K, d_mu, d_sigma, weight, d_scores, (hipStream_t)stream);
}

int bcmpc_mppi_sigma_update_async(bcmpc_engine* e, const double* d_scores, const double* d_actions, int32_t n_envs,
                                  int64_t K, double lambda, const double* d_mu_new, double* d_sigma, double alpha,
                                  double min_std, double max_std, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_scores || !d_actions || !d_mu_new || !d_sigma) return fail(BCMPC_ERR_ARG, "null argument");
    if (!(std::isfinite(lambda) && lambda > 0.0)) return fail(BCMPC_ERR_ARG, "lambda must be finite and > 0");
    if (const int rc = sigma_step_check(alpha, min_std, max_std)) return rc;
    if (const int rc = plan_block_check(e, n_envs, K, 0)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return sigma_update_impl(e, d_scores, d_actions, n_envs, K, lambda, d_mu_new, d_sigma, alpha, min_std, max_std,
                             (hipStream_t)stream);
}

int bcmpc_plan_sample_async(bcmpc_engine* e, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                            uint64_t seed, int32_t iteration, int64_t cand_offset, double* d_actions, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_mu || !d_sigma || !d_actions) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = plan_block_check(e, n_envs, K, iteration)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return plan_sample_impl(e, d_mu, d_sigma, n_envs, K, seed, iteration, cand_offset, d_actions, (hipStream_t)stream);
}

int bcmpc_plan_sample_corr_async(bcmpc_engine* e, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                                 uint64_t seed, int32_t iteration, int64_t cand_offset, double rho, const double* d_keep,
                                 const int32_t* d_keep_count, int32_t n_elite, double* d_actions, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_mu || !d_sigma || !d_actions) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = rho_check(rho)) return rc;
    if ((d_keep != nullptr) != (d_keep_count != nullptr))
        return fail(BCMPC_ERR_ARG, "d_keep and d_keep_count go together (both, or both NULL)");
    if (d_keep && n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (const int rc = plan_block_check(e, n_envs, K, iteration)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return plan_sample_corr_impl(e, d_mu, d_sigma, n_envs, K, seed, iteration, cand_offset, rho, d_keep, d_keep_count,
                                 n_elite, d_actions, (hipStream_t)stream);
}

int bcmpc_plan_sample_prop_async(bcmpc_engine* e, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                                 uint64_t seed, int32_t iteration, int64_t cand_offset, double rho, const double* d_keep,
                                 const int32_t* d_keep_count, int32_t n_elite, const double* d_proposals, int32_t n_prop,
                                 int64_t env_stride, int64_t seq_stride, int64_t step_stride, double* d_actions,
                                 void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_mu || !d_sigma || !d_actions || !d_proposals) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = rho_check(rho)) return rc;
    if ((d_keep != nullptr) != (d_keep_count != nullptr))
        return fail(BCMPC_ERR_ARG, "d_keep and d_keep_count go together (both, or both NULL)");
    if (d_keep && n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (const int rc = plan_block_check(e, n_envs, K, iteration)) return rc;
    if (n_prop < 1) return fail(BCMPC_ERR_ARG, "n_prop must be >= 1");
    if ((int64_t)n_prop + (d_keep ? n_elite : 0) > K)
        return fail(BCMPC_ERR_ARG, d_keep ? "n_prop + n_elite must be <= K (the carried elites keep the first columns)"
                                          : "n_prop must be <= K");
    if (const int rc = prop_strides_check(n_envs, n_prop, e->cfg.horizon, e->cfg.action_dim, env_stride, seq_stride,
                                          step_stride))
        return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return plan_sample_prop_impl(e, d_mu, d_sigma, n_envs, K, seed, iteration, cand_offset, rho, d_keep, d_keep_count,
                                 n_elite, d_proposals, n_prop, env_stride, seq_stride, step_stride, d_actions,
                                 (hipStream_t)stream);
}

int bcmpc_plan_keep_async(bcmpc_engine* e, const bcmpc_elite* d_elite, const int32_t* d_count, const double* d_actions,
                          int32_t n_envs, int64_t K, int64_t cand_offset, int32_t n_elite, double* d_keep,
                          int32_t* d_keep_count, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_elite || !d_count || !d_actions || !d_keep || !d_keep_count) return fail(BCMPC_ERR_ARG, "null argument");
    if (n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (const int rc = plan_block_check(e, n_envs, K, 0)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return plan_keep_impl(e, d_elite, d_count, d_actions, n_envs, K, cand_offset, n_elite, d_keep, d_keep_count,
                          (hipStream_t)stream);
}

int bcmpc_plan_argmin_async(bcmpc_engine* e, const double* d_costs, const double* d_actions, int32_t n_envs, int64_t K,
                            int32_t iteration, int32_t merge, bcmpc_result* d_results, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_costs || !d_actions || !d_results) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = plan_block_check(e, n_envs, K, iteration)) return rc;
    if (e->cfg.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "argmin needs the fused cost");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return plan_argmin_impl(e, d_costs, d_actions, n_envs, K, iteration, merge, d_results, (hipStream_t)stream);
}

int bcmpc_select_batch_async(bcmpc_engine* e, const double* d_costs, int32_t n_envs, int64_t K, int64_t index_base,
                             int32_t n_elite, bcmpc_elite* d_out, int32_t* d_count, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_costs || !d_out || !d_count) return fail(BCMPC_ERR_ARG, "null argument");
    if (n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (const int rc = plan_block_check(e, n_envs, K, 0)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return select_batch_impl(e, d_costs, n_envs, K, index_base, n_elite, d_out, d_count, (hipStream_t)stream);
}

int bcmpc_cem_refit_batch_async(bcmpc_engine* e, const bcmpc_elite* d_elite, const int32_t* d_count, int32_t n_envs,
                                int32_t n_elite, uint64_t seed, int32_t iteration, double alpha, double* d_mu,
                                double* d_sigma, const double* d_actions, int64_t K, int64_t cand_offset,
                                void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_elite || !d_count || !d_mu || !d_sigma) return fail(BCMPC_ERR_ARG, "null argument");
    if (n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (const int rc = plan_block_check(e, n_envs, d_actions ? K : 1, iteration)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return refit_batch_impl(e, d_elite, d_count, n_envs, n_elite, seed, iteration, alpha, d_mu, d_sigma, d_actions, K,
                            cand_offset, (hipStream_t)stream);
}

int bcmpc_mppi_update_batch_async(bcmpc_engine* e, const double* d_costs, int32_t n_envs, int64_t K,
                                  int64_t cand_offset, uint64_t seed, int32_t iteration, double lambda, double* d_mu,
                                  const double* d_sigma, bcmpc_mppi_stats* d_stats, const double* d_actions,
                                  void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_costs || !d_mu || !d_sigma || !d_stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (!(std::isfinite(lambda) && lambda > 0.0)) return fail(BCMPC_ERR_ARG, "lambda must be finite and > 0");
    if (const int rc = plan_block_check(e, n_envs, K, iteration)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return mppi_update_batch_impl(e, d_costs, n_envs, K, cand_offset, seed, iteration, lambda, d_mu, d_sigma, d_stats,
                                  d_actions, (hipStream_t)stream);
}

// ---- knot plans (plan_knots.hip): the sampler, and the outer-loop blocks with the step count given ----
int bcmpc_plan_sample_knots_async(bcmpc_engine* e, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                                  uint64_t seed, int32_t iteration, int64_t cand_offset, double rho, const double* d_keep,
                                  const int32_t* d_keep_count, int32_t n_elite, int32_t knots, int32_t kind,
                                  double* d_knots, double* d_actions, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_mu || !d_sigma || !d_knots || !d_actions) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = knots_check(knots, kind, e->cfg.horizon)) return rc;
    if (const int rc = rho_check(rho)) return rc;
    if ((d_keep != nullptr) != (d_keep_count != nullptr))
        return fail(BCMPC_ERR_ARG, "d_keep and d_keep_count go together (both, or both NULL)");
    if (d_keep && n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (const int rc = plan_block_check(e, n_envs, K, iteration)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return plan_sample_knots_impl(e, d_mu, d_sigma, n_envs, K, seed, iteration, cand_offset, rho, d_keep, d_keep_count,
                                  n_elite, knots, kind, d_knots, d_actions, (hipStream_t)stream);
}

int bcmpc_cem_refit_batch_steps_async(bcmpc_engine* e, const bcmpc_elite* d_elite, const int32_t* d_count,
                                      int32_t n_envs, int32_t n_elite, uint64_t seed, int32_t iteration, double alpha,
                                      double* d_mu, double* d_sigma, const double* d_actions, int64_t K,
                                      int64_t cand_offset, int32_t steps, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_elite || !d_count || !d_mu || !d_sigma || !d_actions) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = steps_check(steps, e->cfg.horizon)) return rc;
    if (n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (const int rc = plan_block_check(e, n_envs, K, iteration)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return refit_batch_impl(e, d_elite, d_count, n_envs, n_elite, seed, iteration, alpha, d_mu, d_sigma, d_actions, K,
                            cand_offset, (hipStream_t)stream, steps);
}

int bcmpc_mppi_update_batch_steps_async(bcmpc_engine* e, const double* d_costs, int32_t n_envs, int64_t K,
                                        int64_t cand_offset, uint64_t seed, int32_t iteration, double lambda,
                                        double* d_mu, const double* d_sigma, bcmpc_mppi_stats* d_stats,
                                        const double* d_actions, int32_t steps, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_costs || !d_mu || !d_sigma || !d_stats || !d_actions) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = steps_check(steps, e->cfg.horizon)) return rc;
    if (!(std::isfinite(lambda) && lambda > 0.0)) return fail(BCMPC_ERR_ARG, "lambda must be finite and > 0");
    if (const int rc = plan_block_check(e, n_envs, K, iteration)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return mppi_update_batch_impl(e, d_costs, n_envs, K, cand_offset, seed, iteration, lambda, d_mu, d_sigma, d_stats,
                                  d_actions, (hipStream_t)stream, steps);
}

int bcmpc_plan_keep_steps_async(bcmpc_engine* e, const bcmpc_elite* d_elite, const int32_t* d_count,
                                const double* d_actions, int32_t n_envs, int64_t K, int64_t cand_offset,
                                int32_t n_elite, double* d_keep, int32_t* d_keep_count, int32_t steps, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_elite || !d_count || !d_actions || !d_keep || !d_keep_count) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = steps_check(steps, e->cfg.horizon)) return rc;
    if (n_elite < 1) return fail(BCMPC_ERR_ARG, "n_elite must be >= 1");
    if (const int rc = plan_block_check(e, n_envs, K, 0)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return plan_keep_impl(e, d_elite, d_count, d_actions, n_envs, K, cand_offset, n_elite, d_keep, d_keep_count,
                          (hipStream_t)stream, steps);
}

int bcmpc_mppi_control_cost_steps_async(bcmpc_engine* e, const double* d_costs, const double* d_actions,
                                        int32_t n_envs, int64_t K, const double* d_mu, const double* d_sigma,
                                        double weight, double* d_scores, int32_t steps, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_costs || !d_actions || !d_mu || !d_sigma || !d_scores) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = steps_check(steps, e->cfg.horizon)) return rc;
    if (const int rc = control_weight_check(weight)) return rc;
    if (const int rc = plan_block_check(e, n_envs, K, 0)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return control_cost_impl(e, d_costs, d_actions, n_envs, K, d_mu, d_sigma, weight, d_scores, (hipStream_t)stream,
                             steps);
}

int bcmpc_mppi_sigma_update_steps_async(bcmpc_engine* e, const double* d_scores, const double* d_actions,
                                        int32_t n_envs, int64_t K, double lambda, const double* d_mu_new,
                                        double* d_sigma, double alpha, double min_std, double max_std, int32_t steps,
                                        void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !d_scores || !d_actions || !d_mu_new || !d_sigma) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = steps_check(steps, e->cfg.horizon)) return rc;
    if (!(std::isfinite(lambda) && lambda > 0.0)) return fail(BCMPC_ERR_ARG, "lambda must be finite and > 0");
    if (const int rc = sigma_step_check(alpha, min_std, max_std)) return rc;
    if (const int rc = plan_block_check(e, n_envs, K, 0)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return sigma_update_impl(e, d_scores, d_actions, n_envs, K, lambda, d_mu_new, d_sigma, alpha, min_std, max_std,
                             (hipStream_t)stream, steps);
}

// the synchronous calls' device buffers: plans, counts and statistics per environment, the elite records
static int plan_buffers(bcmpc_engine* e, int32_t n_envs, size_t n_elite_total) {
    const size_t ha = (size_t)e->cfg.horizon * e->cfg.action_dim;
    if (n_envs > e->plan_cap) {
        for (void* p : {(void*)e->d_bmu, (void*)e->d_bsigma, (void*)e->d_bcount, (void*)e->d_bstats})
            if (p) (void)hipFree(p);
        e->d_bmu = e->d_bsigma = nullptr; e->d_bcount = nullptr; e->d_bstats = nullptr;
        e->plan_cap = 0;
        HIP_TRY(hipMalloc(&e->d_bmu, (size_t)n_envs * ha * sizeof(double)));
        HIP_TRY(hipMalloc(&e->d_bsigma, (size_t)n_envs * ha * sizeof(double)));
        HIP_TRY(hipMalloc(&e->d_bcount, (size_t)n_envs * sizeof(int32_t)));
        HIP_TRY(hipMalloc(&e->d_bstats, (size_t)n_envs * sizeof(bcmpc_mppi_stats)));
        e->plan_cap = n_envs;
    }
    if (n_elite_total > e->belite_cap) {
        if (e->d_belite) (void)hipFree(e->d_belite);
        e->d_belite = nullptr;
        e->belite_cap = 0;
        HIP_TRY(hipMalloc(&e->d_belite, n_elite_total * sizeof(bcmpc_elite)));
        e->belite_cap = n_elite_total;
    }
    return BCMPC_OK;
}

// ... and the carried elites' sequences of a CEM call with carry-over
static int keep_buffers(bcmpc_engine* e, int32_t n_envs, int32_t n_elite) {
    const size_t need = (size_t)n_envs * (size_t)n_elite * (size_t)e->cfg.horizon * (size_t)e->cfg.action_dim;
    if (need > e->keep_cap) {
        if (e->d_keep) (void)hipFree(e->d_keep);
        e->d_keep = nullptr;
        e->keep_cap = 0;
        HIP_TRY(hipMalloc(&e->d_keep, need * sizeof(double)));
        e->keep_cap = need;
    }
    if (n_envs > e->keep_count_cap) {
        if (e->d_keep_count) (void)hipFree(e->d_keep_count);
        e->d_keep_count = nullptr;
        e->keep_count_cap = 0;
        HIP_TRY(hipMalloc(&e->d_keep_count, (size_t)n_envs * sizeof(int32_t)));
        e->keep_count_cap = n_envs;
    }
    return BCMPC_OK;
}

// The synchronous batched planner: states and plans up, tile_states once, then per iteration plan_sample ->
// rollout (explicit actions, per-candidate states) -> plan_argmin -> the planner's update; records and
// plans down, one stream synchronisation.  cem != nullptr: CEM, else MPPI (mp).  A non-default smp (checked by
// the caller): plan_sample_corr instead of plan_sample, and with keep_elites plan_keep behind every refit that
// another iteration follows -- iteration it >= 1 then starts with iteration it - 1's elites.
// A non-default ext (MPPI; checked by the caller): the control-cost launch in front of the update, whose augmented
// scores replace the costs in it (the record stays on the raw costs), and with adapt_sigma the sigma launches
// behind it; sigma_io is then written back like CEM's.
// Knots (kn; checked by the caller, never with proposals): the plans are [n_envs][M][A]; plan_sample_knots writes the
// clipped knots into d_knots and their expansion into d_actions, the rollout and the record read d_actions, and
// everything behind select -- refit or update, control cost, sigma update, plan_keep -- runs on d_knots with the step
// count M.
static int plan_get_actions(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_cem* cem,
                            const bcmpc_mppi* mp, const bcmpc_sampling* smp, uint64_t seed, int64_t cand_offset,
                            double* mu, double* sigma_io, const double* sigma_in, bcmpc_result* out,
                            bcmpc_mppi_stats* stats, double* costs_out, const bcmpc_mppi_ext* ext = nullptr,
                            const bcmpc_proposals* prop = nullptr, const bcmpc_knots* kn = nullptr) {
    const bcmpc_config& c = e->cfg;
    const int32_t iterations = cem ? cem->iterations : mp->iterations;
    const int64_t K = c.num_paths / n_envs;
    HIP_TRY(hipSetDevice(c.device));
    const SyncCall sync_guard(e);
    const int32_t M = knots_none(kn) ? 0 : kn->count;   // the outer loop's step count (0: the horizon)
    const size_t ha = (size_t)c.horizon * c.action_dim, nplan = (size_t)n_envs * (M ? (size_t)M * c.action_dim : ha);
    if (const int rc = batch_buffers(e, n_envs)) return rc;
    if (const int rc = plan_buffers(e, n_envs, cem ? (size_t)n_envs * cem->n_elite : 0)) return rc;
    if (const int rc = actions_buffer(e)) return rc;
    const bool corr = !sampling_default(smp), carry = corr && cem && smp->keep_elites && iterations > 1;
    if (carry)
        if (const int rc = keep_buffers(e, n_envs, cem->n_elite)) return rc;
    const size_t nknots = (size_t)M * (size_t)c.num_paths * c.action_dim;
    if (nknots > e->knots_cap) {
        if (e->d_knots) (void)hipFree(e->d_knots);
        e->d_knots = nullptr;
        e->knots_cap = 0;
        HIP_TRY(hipMalloc(&e->d_knots, nknots * sizeof(double)));
        e->knots_cap = nknots;
    }
    const double* const d_drawn = M ? e->d_knots : e->d_actions;   // what select's followers read
    // proposals (checked by the caller): host sequences go up with the plans, device ones are read where they are
    const int32_t P = proposals_none(prop) ? 0 : prop->count;
    const size_t nprop = (size_t)n_envs * (size_t)P * ha;
    if (P && !prop->device && nprop > e->prop_cap) {
        if (e->d_prop) (void)hipFree(e->d_prop);
        e->d_prop = nullptr;
        e->prop_cap = 0;
        HIP_TRY(hipMalloc(&e->d_prop, nprop * sizeof(double)));
        e->prop_cap = nprop;
    }
    const double* d_prop = !P ? nullptr : prop->device ? prop->sequences : e->d_prop;
    const int64_t prop_env = !P ? 0 : prop->device ? prop->env_stride : (int64_t)P * (int64_t)ha;
    const int64_t prop_seq = !P ? 0 : prop->device ? prop->seq_stride : (int64_t)ha;
    const int64_t prop_step = !P ? 0 : prop->device ? prop->step_stride : (int64_t)c.action_dim;
    if (!e->d_tiled) HIP_TRY(hipMalloc(&e->d_tiled, (size_t)c.num_paths * c.state_dim * sizeof(double)));
    const bool control = ext && !cem && ext->control_weight != 0.0, adapt = ext && !cem && ext->adapt_sigma != 0;
    if (control && (size_t)c.num_paths > e->mppi_scores_cap) {
        if (e->d_mppi_scores) (void)hipFree(e->d_mppi_scores);
        e->d_mppi_scores = nullptr;
        e->mppi_scores_cap = 0;
        HIP_TRY(hipMalloc(&e->d_mppi_scores, (size_t)c.num_paths * sizeof(double)));
        e->mppi_scores_cap = (size_t)c.num_paths;
    }
    const bool sigma_out = cem || adapt;               // the call writes sigma back
    const double* sigma = sigma_out ? sigma_io : sigma_in;
    const PlanInputs inputs(e->kernel == BCMPC_KERNEL_TEAM, mu, sigma_out ? sigma_io : nullptr, nplan);
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(e->d_bstates, states, sizeof(double) * (size_t)n_envs * c.state_dim, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_bmu, mu, nplan * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_bsigma, sigma, nplan * sizeof(double), hipMemcpyHostToDevice, st));
    if (P && !prop->device)
        HIP_TRY(hipMemcpyAsync(e->d_prop, prop->sequences, nprop * sizeof(double), hipMemcpyHostToDevice, st));
    if (e->timing) HIP_TRY(hipEventRecord(e->ev[0], st));
    TileStatesArgs t{};
    t.states = e->d_bstates; t.out = e->d_tiled; t.K = K; t.Ktot = c.num_paths; t.S = c.state_dim;
    HIP_TRY(launch_tile_states(t, st));
    for (int it = 0; it < iterations; ++it) {
        const bool kept = carry && it > 0;
        if (const int rc = M ? plan_sample_knots_impl(e, e->d_bmu, e->d_bsigma, n_envs, K, seed, it, cand_offset,
                                                      smp ? smp->rho : 0.0, kept ? e->d_keep : nullptr,
                                                      kept ? e->d_keep_count : nullptr, cem ? cem->n_elite : 0, M,
                                                      kn->kind, e->d_knots, e->d_actions, st)
                           : P ? plan_sample_prop_impl(e, e->d_bmu, e->d_bsigma, n_envs, K, seed, it, cand_offset,
                                                     smp ? smp->rho : 0.0, kept ? e->d_keep : nullptr,
                                                     kept ? e->d_keep_count : nullptr, cem ? cem->n_elite : 0, d_prop,
                                                     P, prop_env, prop_seq, prop_step, e->d_actions, st)
                           : !corr ? plan_sample_impl(e, e->d_bmu, e->d_bsigma, n_envs, K, seed, it, cand_offset,
                                                    e->d_actions, st)
                                 : plan_sample_corr_impl(e, e->d_bmu, e->d_bsigma, n_envs, K, seed, it, cand_offset,
                                                         smp->rho, kept ? e->d_keep : nullptr,
                                                         kept ? e->d_keep_count : nullptr, cem ? cem->n_elite : 0,
                                                         e->d_actions, st))
            return rc;
        RolloutLaunch r;
        r.state = e->d_tiled; r.state_stride = c.state_dim; r.actions = e->d_actions; r.seed = seed;
        r.cand_offset = cand_offset; r.costs = e->d_costs; r.stream = st; r.record_events = false;
        r.n_envs = n_envs;
        if (const int rc = rollout_impl(e, r)) return rc;
        if (costs_out)
            HIP_TRY(hipMemcpyAsync(costs_out + (size_t)it * c.num_paths, e->d_costs, sizeof(double) * c.num_paths,
                                   hipMemcpyDeviceToHost, st));
        // the record before the update, and before the next plan_sample overwrites the array it reads
        int rc = plan_argmin_impl(e, e->d_costs, e->d_actions, n_envs, K, it, it > 0, e->d_bresults, st);
        if (rc == BCMPC_OK && cem)
            rc = select_batch_impl(e, e->d_costs, n_envs, K, cand_offset, cem->n_elite, e->d_belite, e->d_bcount, st);
        // (MPPI with the control-cost term: the update and the sigma launches read the augmented scores)
        const double* scores = control ? e->d_mppi_scores : e->d_costs;
        if (rc == BCMPC_OK && control)
            rc = control_cost_impl(e, e->d_costs, d_drawn, n_envs, K, e->d_bmu, e->d_bsigma, ext->control_weight,
                                   e->d_mppi_scores, st, M);
        if (rc == BCMPC_OK)
            rc = cem ? refit_batch_impl(e, e->d_belite, e->d_bcount, n_envs, cem->n_elite, seed, it, cem->alpha, e->d_bmu,
                                        e->d_bsigma, d_drawn, K, cand_offset, st, M)
                     : mppi_update_batch_impl(e, scores, n_envs, K, cand_offset, seed, it, mp->lambda, e->d_bmu,
                                              e->d_bsigma, e->d_bstats, d_drawn, st, M);
        if (rc == BCMPC_OK && adapt)
            rc = sigma_update_impl(e, scores, d_drawn, n_envs, K, mp->lambda, e->d_bmu, e->d_bsigma,
                                   ext->sigma_alpha, ext->min_std, ext->max_std, st, M);
        // the elites' sequences out of the array, before the next iteration's sampling overwrites it
        if (rc == BCMPC_OK && carry && it + 1 < iterations)
            rc = plan_keep_impl(e, e->d_belite, e->d_bcount, d_drawn, n_envs, K, cand_offset, cem->n_elite,
                                e->d_keep, e->d_keep_count, st, M);
        if (rc != BCMPC_OK) return rc;
    }
    if (e->timing) {
        HIP_TRY(hipEventRecord(e->ev[1], st));
        HIP_TRY(hipEventRecord(e->ev[2], st));
    }
    e->timed = e->timing;
    HIP_TRY(hipMemcpyAsync(e->h_bresults, e->d_bresults, (size_t)n_envs * sizeof(bcmpc_result), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(mu, e->d_bmu, nplan * sizeof(double), hipMemcpyDeviceToHost, st));
    if (sigma_out) HIP_TRY(hipMemcpyAsync(sigma_io, e->d_bsigma, nplan * sizeof(double), hipMemcpyDeviceToHost, st));
    if (!cem) HIP_TRY(hipMemcpyAsync(stats, e->d_bstats, (size_t)n_envs * sizeof(bcmpc_mppi_stats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (team_failed(e)) {                              // the whole call again, from the original plans
        if (const int fr = team_fallback(e)) return fr;
        inputs.restore(mu, sigma_io);
        return plan_get_actions(e->fb, states, n_envs, cem, mp, smp, seed, cand_offset, mu, sigma_io, sigma_in, out,
                                stats, costs_out, ext, prop, kn);
    }
    std::memcpy(out, e->h_bresults, (size_t)n_envs * sizeof(bcmpc_result));
    return BCMPC_OK;
}

int bcmpc_cem_get_actions_batch_s(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_cem* p,
                                  const bcmpc_sampling* sampling, uint64_t seed, int64_t cand_offset, double* mu,
                                  double* sigma, bcmpc_result* out, double* costs_out) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !states || !p || !mu || !sigma || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = cem_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, false)) return rc;
    if (const int rc = batch_check(e, n_envs)) return rc;
    if (const int rc = k_global_check(p->k_global, "batched CEM", e->cfg.num_paths / n_envs, "num_paths / n_envs")) return rc;
    return plan_get_actions(e, states, n_envs, p, nullptr, sampling, seed, cand_offset, mu, sigma, nullptr, out,
                            nullptr, costs_out);
}

int bcmpc_cem_get_actions_batch(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_cem* p,
                                uint64_t seed, int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out,
                                double* costs_out) {
    return bcmpc_cem_get_actions_batch_s(e, states, n_envs, p, nullptr, seed, cand_offset, mu, sigma, out, costs_out);
}

int bcmpc_mppi_get_actions_batch_s(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_mppi* p,
                                   const bcmpc_sampling* sampling, uint64_t seed, int64_t cand_offset, double* mu,
                                   const double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats, double* costs_out) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !states || !p || !mu || !sigma || !out || !stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = mppi_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, true)) return rc;
    if (const int rc = batch_check(e, n_envs)) return rc;
    if (const int rc = k_global_check(p->k_global, "batched MPPI", e->cfg.num_paths / n_envs, "num_paths / n_envs")) return rc;
    return plan_get_actions(e, states, n_envs, nullptr, p, sampling, seed, cand_offset, mu, nullptr, sigma, out,
                            stats, costs_out);
}

int bcmpc_mppi_get_actions_batch(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_mppi* p,
                                 uint64_t seed, int64_t cand_offset, double* mu, const double* sigma, bcmpc_result* out,
                                 bcmpc_mppi_stats* stats, double* costs_out) {
    return bcmpc_mppi_get_actions_batch_s(e, states, n_envs, p, nullptr, seed, cand_offset, mu, sigma, out, stats,
                                          costs_out);
}

int bcmpc_mppi_get_actions_batch_x(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_mppi* p,
                                   const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext, uint64_t seed,
                                   int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out,
                                   bcmpc_mppi_stats* stats, double* costs_out) {
    // (arguments first: a bad call is answered before any HIP call)
    if (const int rc = mppi_ext_check(ext)) return rc;
    if (mppi_ext_default(ext))
        return bcmpc_mppi_get_actions_batch_s(e, states, n_envs, p, sampling, seed, cand_offset, mu, sigma, out, stats,
                                              costs_out);
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !states || !p || !mu || !sigma || !out || !stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = mppi_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, true)) return rc;
    if (const int rc = batch_check(e, n_envs)) return rc;
    if (const int rc = k_global_check(p->k_global, "batched MPPI", e->cfg.num_paths / n_envs, "num_paths / n_envs")) return rc;
    return plan_get_actions(e, states, n_envs, nullptr, p, sampling, seed, cand_offset, mu, sigma, sigma, out, stats,
                            costs_out, ext);
}

// ---- model ensembles: E member engines, one launch chain on member 0's stream -----------
// Per iteration: every member's rollout (no result record) into its row of d_member [E][num_paths], the
// reduce (ensemble.hip) into member 0's d_costs, then what a single engine runs on its costs -- the argmin
// launch, select + refit or the MPPI update -- on member 0.  The members run one after the other on ONE
// stream: the team kernel needs its whole grid resident, which is what team_order_* guards across streams.
struct bcmpc_ensemble {
    std::vector<bcmpc_engine*> m;       // the members (owned; a fallback view: the members' fallback engines)
    double* d_member = nullptr;         // [E][num_paths] member costs, allocated at create
    int32_t mode = BCMPC_ENSEMBLE_MEAN;
    double kappa = 0.0;
    bool owns = true;
    bcmpc_ensemble* fb = nullptr;       // the ensemble of the members' fallback engines (team give-up)
};

static const char* ensemble_rule_error(int32_t mode, double kappa) {
    if (mode < BCMPC_ENSEMBLE_MEAN || mode > BCMPC_ENSEMBLE_WORST) return "unknown ensemble mode";
    if (!std::isfinite(kappa)) return "kappa must be finite";
    return nullptr;
}

static int ensemble_reduce_impl(const double* d_member, int64_t ld, int32_t E, int64_t K, int32_t mode, double kappa,
                                double* d_out, hipStream_t st) {
    EnsembleReduceArgs r{};
    r.member_costs = d_member; r.out = d_out; r.ld = ld; r.K = K; r.E = E; r.mode = mode; r.kappa = kappa;
    HIP_TRY(launch_ensemble_reduce(r, st));
    return BCMPC_OK;
}

// refusals of a call that need no HIP call: a member with a communicator attached
static int ensemble_call_check(const bcmpc_ensemble* s) {
    for (const bcmpc_engine* e : s->m)
        if (e->comm)
            return fail(BCMPC_ERR_UNSUPPORTED, "ensemble calls do not cover members with a communicator attached");
    return BCMPC_OK;
}

// any member's team gave up (every member's flag is read, which clears it)
static bool ensemble_failed(bcmpc_ensemble* s) {
    bool any = false;
    for (bcmpc_engine* e : s->m) any = team_failed(e) || any;
    return any;
}

// the ensemble a failed call reruns on: every team member's fallback engine, in member order
static int ensemble_fallback(bcmpc_ensemble* s, bcmpc_ensemble** r) {
    if (!s->fb) {
        s->fb = new bcmpc_ensemble();
        s->fb->owns = false;
    }
    bcmpc_ensemble* f = s->fb;
    f->m.clear();
    for (bcmpc_engine* e : s->m) {
        if (e->kernel == BCMPC_KERNEL_TEAM) {
            if (const int fr = team_fallback(e)) return fr;
            f->m.push_back(e->fb);
        } else {
            f->m.push_back(e);
        }
    }
    if (!f->d_member)
        HIP_TRY(hipMalloc(&f->d_member, s->m.size() * (size_t)std::max<int64_t>(1, s->m[0]->cfg.num_paths) * sizeof(double)));
    f->mode = s->mode;
    f->kappa = s->kappa;
    *r = f;
    return BCMPC_OK;
}

int bcmpc_ensemble_create(const bcmpc_config* cfg, int32_t n_members, bcmpc_ensemble** out) {
    if (!cfg || !out) return fail(BCMPC_ERR_ARG, "null argument");
    *out = nullptr;
    if (n_members < 1 || n_members > BCMPC_MAX_MEMBERS)
        return fail(BCMPC_ERR_ARG, "n_members must be in [1, " + std::to_string(BCMPC_MAX_MEMBERS) + "]");
    if (cfg->policy_hidden > 0) return fail(BCMPC_ERR_UNSUPPORTED, "ensembles do not cover engines with a fused policy");
    if (cfg->model == BCMPC_MODEL_REWARD || cfg->cost == BCMPC_COST_REWARD)
        return fail(BCMPC_ERR_UNSUPPORTED, "ensembles do not cover the reward model / the learned-reward objective");
    if (cfg->cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_UNSUPPORTED, "ensembles need a fused cost (cheetah or terms)");
    bcmpc_ensemble* s = new bcmpc_ensemble();
    CreateOpts opts;
    opts.no_pp3 = true;                               // (members run rollout_x3: DESIGN.md 6.9)
    for (int i = 0; i < n_members; ++i) {
        bcmpc_engine* e = nullptr;
        const int rc = create_engine(cfg, opts, &e);
        if (rc != BCMPC_OK) {
            (void)bcmpc_ensemble_destroy(s);
            return rc;
        }
        s->m.push_back(e);
    }
    if (hipMalloc(&s->d_member, (size_t)n_members * (size_t)std::max<int64_t>(1, cfg->num_paths) * sizeof(double)) !=
        hipSuccess) {
        (void)bcmpc_ensemble_destroy(s);
        return fail(BCMPC_ERR_HIP, "hipMalloc of the member cost buffer failed");
    }
    *out = s;
    return BCMPC_OK;
}

int bcmpc_ensemble_destroy(bcmpc_ensemble* s) {
    if (!s) return BCMPC_OK;
    if (!s->m.empty() && s->m[0]->stream) {
        (void)hipSetDevice(s->m[0]->cfg.device);
        (void)hipStreamSynchronize(s->m[0]->stream);
    }
    if (s->fb) {
        if (s->fb->d_member) (void)hipFree(s->fb->d_member);
        delete s->fb;
    }
    if (s->d_member) (void)hipFree(s->d_member);
    if (s->owns)
        for (bcmpc_engine* e : s->m) (void)bcmpc_destroy(e);
    delete s;
    return BCMPC_OK;
}

int bcmpc_ensemble_size(const bcmpc_ensemble* s) { return s ? (int)s->m.size() : 0; }

int bcmpc_ensemble_member(bcmpc_ensemble* s, int32_t i, bcmpc_engine** out) {
    if (!s || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (i < 0 || i >= (int32_t)s->m.size()) return fail(BCMPC_ERR_ARG, "member index out of range");
    *out = s->m[i];
    return BCMPC_OK;
}

int bcmpc_ensemble_set_rule(bcmpc_ensemble* s, int32_t mode, double kappa) {
    if (const char* why = ensemble_rule_error(mode, kappa)) return fail(BCMPC_ERR_ARG, why);
    if (!s) return fail(BCMPC_ERR_ARG, "null argument");
    s->mode = mode;
    s->kappa = kappa;
    return BCMPC_OK;
}

int bcmpc_ensemble_reduce_async(bcmpc_engine* e, const double* d_member_costs, int64_t ld, int32_t n_members,
                                int64_t K, int32_t mode, double kappa, double* d_out, void* stream) {
    // (scalars first, then pointers: a bad call is answered before any HIP call)
    if (n_members < 1 || n_members > BCMPC_MAX_MEMBERS)
        return fail(BCMPC_ERR_ARG, "n_members must be in [1, " + std::to_string(BCMPC_MAX_MEMBERS) + "]");
    if (const char* why = ensemble_rule_error(mode, kappa)) return fail(BCMPC_ERR_ARG, why);
    if (K < 1) return fail(BCMPC_ERR_ARG, "K must be >= 1");
    if (ld < K) return fail(BCMPC_ERR_ARG, "ld must be >= K");
    if (!e || !d_member_costs || !d_out) return fail(BCMPC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return ensemble_reduce_impl(d_member_costs, ld, n_members, K, mode, kappa, d_out, (hipStream_t)stream);
}

int bcmpc_ensemble_get_action(bcmpc_ensemble* s, const double* state, const double* actions, uint64_t seed,
                              int64_t cand_offset, bcmpc_result* out, double* costs_out, double* member_costs_out) {
    if (!s || !state || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = ensemble_call_check(s)) return rc;
    bcmpc_engine* e0 = s->m[0];
    const bcmpc_config& c = e0->cfg;
    const int32_t E = (int32_t)s->m.size();
    const int64_t K = c.num_paths;
    if (K == 0) return fail(BCMPC_ERR_EMPTY, "attempt to get argmin of an empty sequence");
    HIP_TRY(hipSetDevice(c.device));
    const SyncCall sync_guard(s->m.data(), s->m.size());
    hipStream_t st = e0->stream;
    const double* d_act = nullptr;                     // (one upload, read by every member)
    if (const int rc = upload_actions(e0, actions, st, &d_act)) return rc;
    RolloutLaunch r;                                   // the state travels in the kernel arguments
    r.state_inline = state; r.actions = d_act; r.seed = seed; r.cand_offset = cand_offset; r.stream = st;
    r.record_events = false;
    for (int32_t i = 0; i < E; ++i) {
        r.costs = s->d_member + (size_t)i * K;
        if (const int rc = rollout_impl(s->m[i], r)) return rc;
    }
    if (const int rc = ensemble_reduce_impl(s->d_member, K, E, K, s->mode, s->kappa, e0->d_costs, st)) return rc;
    // the ordinary argmin launch on v; its record goes straight into mapped host memory
    e0->want_done = !costs_out && !member_costs_out;
    const ArgminArgs am = argmin_args(e0, e0->d_costs, d_act, nullptr, seed, cand_offset, e0->d_result_map, nullptr);
    const bool spin = e0->want_done;
    e0->want_done = false;
    HIP_TRY(launch_argmin(am, st));
    if (costs_out) HIP_TRY(hipMemcpyAsync(costs_out, e0->d_costs, sizeof(double) * K, hipMemcpyDeviceToHost, st));
    if (member_costs_out)
        HIP_TRY(hipMemcpyAsync(member_costs_out, s->d_member, sizeof(double) * (size_t)E * K, hipMemcpyDeviceToHost, st));
    if (spin) {
        if (const int wr = wait_done(e0, e0->seq)) return wr;
    } else {
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (ensemble_failed(s)) {                          // a team gave up: the whole call on the fallback engines
        bcmpc_ensemble* f = nullptr;
        if (const int fr = ensemble_fallback(s, &f)) return fr;
        return bcmpc_ensemble_get_action(f, state, actions, seed, cand_offset, out, costs_out, member_costs_out);
    }
    *out = *e0->h_result_map;
    return BCMPC_OK;
}

int bcmpc_ensemble_get_actions_batch(bcmpc_ensemble* s, const double* states, int32_t n_envs, const double* actions,
                                     uint64_t seed, int64_t cand_offset, bcmpc_result* out, double* costs_out,
                                     double* member_costs_out) {
    if (!s || !states || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = ensemble_call_check(s)) return rc;
    bcmpc_engine* e0 = s->m[0];
    if (const int rc = batch_check(e0, n_envs)) return rc;
    const bcmpc_config& c = e0->cfg;
    const int32_t E = (int32_t)s->m.size();
    const int64_t Ktot = c.num_paths, K = Ktot / n_envs;
    HIP_TRY(hipSetDevice(c.device));
    const SyncCall sync_guard(s->m.data(), s->m.size());
    if (const int rc = batch_buffers(e0, n_envs)) return rc;
    if (!e0->d_tiled) HIP_TRY(hipMalloc(&e0->d_tiled, (size_t)Ktot * c.state_dim * sizeof(double)));
    hipStream_t st = e0->stream;
    HIP_TRY(hipMemcpyAsync(e0->d_bstates, states, sizeof(double) * (size_t)n_envs * c.state_dim, hipMemcpyHostToDevice, st));
    const double* d_act = nullptr;
    if (const int rc = upload_actions(e0, actions, st, &d_act)) return rc;
    TileStatesArgs t{};
    t.states = e0->d_bstates; t.out = e0->d_tiled; t.K = K; t.Ktot = Ktot; t.S = c.state_dim;
    HIP_TRY(launch_tile_states(t, st));
    RolloutLaunch r;
    r.state = e0->d_tiled; r.state_stride = c.state_dim; r.actions = d_act; r.seed = seed; r.cand_offset = cand_offset;
    r.stream = st; r.record_events = false; r.n_envs = n_envs;
    for (int32_t i = 0; i < E; ++i) {
        r.costs = s->d_member + (size_t)i * Ktot;
        if (const int rc = rollout_impl(s->m[i], r)) return rc;
    }
    if (const int rc = ensemble_reduce_impl(s->d_member, Ktot, E, Ktot, s->mode, s->kappa, e0->d_costs, st)) return rc;
    SegmentArgminArgs m{};
    m.costs = e0->d_costs; m.actions = d_act; m.consts = e0->d_consts; m.out = e0->d_bresults;
    m.seed = seed; m.cand_offset = cand_offset; m.K = K; m.n_envs = n_envs; m.A = c.action_dim;
    m.maximize = 0;
    HIP_TRY(launch_argmin_segments(m, st));
    HIP_TRY(hipMemcpyAsync(e0->h_bresults, e0->d_bresults, (size_t)n_envs * sizeof(bcmpc_result), hipMemcpyDeviceToHost, st));
    if (costs_out) HIP_TRY(hipMemcpyAsync(costs_out, e0->d_costs, sizeof(double) * Ktot, hipMemcpyDeviceToHost, st));
    if (member_costs_out)
        HIP_TRY(hipMemcpyAsync(member_costs_out, s->d_member, sizeof(double) * (size_t)E * Ktot, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ensemble_failed(s)) {
        bcmpc_ensemble* f = nullptr;
        if (const int fr = ensemble_fallback(s, &f)) return fr;
        return bcmpc_ensemble_get_actions_batch(f, states, n_envs, actions, seed, cand_offset, out, costs_out,
                                                member_costs_out);
    }
    std::memcpy(out, e0->h_bresults, (size_t)n_envs * sizeof(bcmpc_result));
    return BCMPC_OK;
}

// ---- the synchronous single-plan chain: CEM and MPPI on one engine or over an ensemble -----------------
// State and plans up; per iteration one scoring of the candidates with its argmin record, then the planner's update
// (cem: select + refit, else mp: the MPPI update); record, plans and statistics down; one stream synchronisation.
// s == nullptr: e scores with one rollout_impl that carries the record, so the argmin (fused or not) and the cost
// terms stay inside it, and the chain records the timing events.  Otherwise e is the ensemble's member 0: every
// member's rollout into its row of d_member, the reduce into e's d_costs and the ordinary argmin launch behind it
// -- also for an ensemble of one.  A team that gave up: the call again, from the original plans, on the fallback.
static int plan_chain(bcmpc_engine* e, bcmpc_ensemble* s, const double* state, const bcmpc_cem* cem,
                      const bcmpc_mppi* mp, uint64_t seed, double* mu, double* sigma_io, const double* sigma_in,
                      bcmpc_result* out, bcmpc_mppi_stats* stats) {
    const bcmpc_config& c = e->cfg;
    const int64_t K = c.num_paths;
    const int32_t iterations = cem ? cem->iterations : mp->iterations;
    bcmpc_engine* const* m = s ? s->m.data() : &e;
    const size_t E = s ? s->m.size() : 1;
    HIP_TRY(hipSetDevice(c.device));
    const SyncCall sync_guard(m, E);
    if (const int rc = cem_buffers(e, cem ? cem->n_elite : 0)) return rc;
    if (mp && !e->d_mppi_stats) HIP_TRY(hipMalloc(&e->d_mppi_stats, sizeof(bcmpc_mppi_stats)));
    const size_t ha = (size_t)c.horizon * c.action_dim;
    hipStream_t st = e->stream;
    const bool events = !s && e->timing;
    bool team = false;
    for (size_t i = 0; i < E; ++i) team = team || m[i]->kernel == BCMPC_KERNEL_TEAM;
    const PlanInputs inputs(team, mu, cem ? sigma_io : nullptr, ha);
    HIP_TRY(hipMemcpyAsync(e->d_state, state, sizeof(double) * c.state_dim, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_mu, mu, ha * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_sigma, cem ? sigma_io : sigma_in, ha * sizeof(double), hipMemcpyHostToDevice, st));
    if (events) HIP_TRY(hipEventRecord(e->ev[0], st));
    for (int it = 0; it < iterations; ++it) {
        const CemLaunch cl{e->d_mu, e->d_sigma, it, it > 0, (int64_t)it * K};
        RolloutLaunch r;
        r.state = e->d_state; r.seed = seed; r.stream = st; r.cem = &cl; r.record_events = false;
        if (!s) {
            r.costs = e->d_costs; r.result = e->d_result;
            if (const int rc = rollout_impl(e, r)) return rc;
        } else {
            for (size_t i = 0; i < E; ++i) {
                r.costs = s->d_member + i * (size_t)K;
                if (const int rc = rollout_impl(m[i], r)) return rc;
            }
            if (const int rc = ensemble_reduce_impl(s->d_member, K, (int32_t)E, K, s->mode, s->kappa, e->d_costs, st))
                return rc;
            HIP_TRY(launch_argmin(argmin_args(e, e->d_costs, nullptr, nullptr, seed, 0, e->d_result, &cl), st));
        }
        if (cem) {
            if (const int rc = select_impl(e, nullptr, e->d_costs, K, 0, cem->n_elite, e->d_elite, e->d_count, st)) return rc;
            if (const int rc = refit_impl(e, e->d_elite, e->d_count, seed, it, cem->alpha, e->d_mu, e->d_sigma, st)) return rc;
        } else {
            if (const int rc = mppi_update_impl(e, e->d_costs, K, 0, seed, it, mp->lambda, e->d_mu, e->d_sigma,
                                                e->d_mppi_stats, st))
                return rc;
        }
    }
    if (events) {
        HIP_TRY(hipEventRecord(e->ev[1], st));
        HIP_TRY(hipEventRecord(e->ev[2], st));
    }
    if (!s) e->timed = e->timing;
    HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(bcmpc_result), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(mu, e->d_mu, ha * sizeof(double), hipMemcpyDeviceToHost, st));
    if (cem) HIP_TRY(hipMemcpyAsync(sigma_io, e->d_sigma, ha * sizeof(double), hipMemcpyDeviceToHost, st));
    else HIP_TRY(hipMemcpyAsync(stats, e->d_mppi_stats, sizeof(*stats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (s ? ensemble_failed(s) : team_failed(e)) {
        bcmpc_ensemble* fs = nullptr;
        if (const int fr = s ? ensemble_fallback(s, &fs) : team_fallback(e)) return fr;
        inputs.restore(mu, sigma_io);
        // (one engine: fs stays nullptr, so the rerun is again the single-engine form, on the fallback engine)
        return plan_chain(s ? fs->m[0] : e->fb, fs, state, cem, mp, seed, mu, sigma_io, sigma_in, out, stats);
    }
    *out = *e->h_result;
    return BCMPC_OK;
}

int bcmpc_cem_get_action(bcmpc_engine* e, const double* state, const bcmpc_cem* p, uint64_t seed, double* mu,
                         double* sigma, bcmpc_result* out) {
    if (!e || !state || !p || !mu || !sigma || !out) return fail(BCMPC_ERR_ARG, "null argument");
    const bcmpc_config& c = e->cfg;
    if (c.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "CEM needs a fused objective");
    if (const int rc = cem_param_check(p)) return rc;
    if (const int rc = k_global_check(p->k_global, "single-device CEM", c.num_paths)) return rc;
    if (c.num_paths == 0) return fail(BCMPC_ERR_EMPTY, "attempt to get argmin of an empty sequence");
    return plan_chain(e, nullptr, state, p, nullptr, seed, mu, sigma, nullptr, out, nullptr);
}

int bcmpc_mppi_get_action(bcmpc_engine* e, const double* state, const bcmpc_mppi* p, uint64_t seed, double* mu,
                          const double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats) {
    if (!e || !state || !p || !mu || !sigma || !out || !stats) return fail(BCMPC_ERR_ARG, "null argument");
    const bcmpc_config& c = e->cfg;
    if (const int rc = mppi_param_check(p)) return rc;
    if (c.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "MPPI needs a fused objective");
    if (const int rc = k_global_check(p->k_global, "single-device MPPI", c.num_paths)) return rc;
    if (c.num_paths == 0) return fail(BCMPC_ERR_EMPTY, "attempt to get argmin of an empty sequence");
    if (e->comm)
        return fail(BCMPC_ERR_UNSUPPORTED, "MPPI with a communicator attached is not supported (the ranks' "
                                           "(v_min, W, N) partials are not combined yet)");
    if (e->PL > 0) return fail(BCMPC_ERR_UNSUPPORTED, "MPPI runs on engines without a fused policy");
    return plan_chain(e, nullptr, state, nullptr, p, seed, mu, nullptr, sigma, out, stats);
}

// The single-plan calls with a sampling distribution: the default runs plan_chain as ever (the rollout kernels
// sample white noise themselves); anything else is the batched chain with one environment at cand_offset 0,
// whose answer at the default equals the single call's.
int bcmpc_cem_get_action_s(bcmpc_engine* e, const double* state, const bcmpc_cem* p, const bcmpc_sampling* sampling,
                           uint64_t seed, double* mu, double* sigma, bcmpc_result* out) {
    if (sampling_default(sampling)) return bcmpc_cem_get_action(e, state, p, seed, mu, sigma, out);
    if (!e || !state || !p || !mu || !sigma || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (e->cfg.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "CEM needs a fused objective");
    if (const int rc = cem_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, false)) return rc;
    if (const int rc = k_global_check(p->k_global, "single-device CEM", e->cfg.num_paths)) return rc;
    if (const int rc = batch_check(e, 1)) return rc;
    return plan_get_actions(e, state, 1, p, nullptr, sampling, seed, 0, mu, sigma, nullptr, out, nullptr, nullptr);
}

int bcmpc_mppi_get_action_s(bcmpc_engine* e, const double* state, const bcmpc_mppi* p, const bcmpc_sampling* sampling,
                            uint64_t seed, double* mu, const double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats) {
    if (sampling_default(sampling)) return bcmpc_mppi_get_action(e, state, p, seed, mu, sigma, out, stats);
    if (!e || !state || !p || !mu || !sigma || !out || !stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = mppi_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, true)) return rc;
    if (e->cfg.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "MPPI needs a fused objective");
    if (const int rc = k_global_check(p->k_global, "single-device MPPI", e->cfg.num_paths)) return rc;
    if (const int rc = batch_check(e, 1)) return rc;
    return plan_get_actions(e, state, 1, nullptr, p, sampling, seed, 0, mu, nullptr, sigma, out, stats, nullptr);
}

// ... and with the control-cost term / the sigma update: off, the call above; on, the batched chain as for rho
int bcmpc_mppi_get_action_x(bcmpc_engine* e, const double* state, const bcmpc_mppi* p, const bcmpc_sampling* sampling,
                            const bcmpc_mppi_ext* ext, uint64_t seed, double* mu, double* sigma, bcmpc_result* out,
                            bcmpc_mppi_stats* stats) {
    if (const int rc = mppi_ext_check(ext)) return rc;
    if (mppi_ext_default(ext)) return bcmpc_mppi_get_action_s(e, state, p, sampling, seed, mu, sigma, out, stats);
    if (!e || !state || !p || !mu || !sigma || !out || !stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = mppi_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, true)) return rc;
    if (e->cfg.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "MPPI needs a fused objective");
    if (const int rc = k_global_check(p->k_global, "single-device MPPI", e->cfg.num_paths)) return rc;
    if (const int rc = batch_check(e, 1)) return rc;
    return plan_get_actions(e, state, 1, nullptr, p, sampling, seed, 0, mu, sigma, sigma, out, stats, nullptr, ext);
}

// ... and with proposals: none, the calls above; else the batched chain with plan_sample_prop as its
// sampler.  One body per planner: the single calls are its n_envs = 1, cand_offset = 0 form with the single
// calls' own refusals in front.
static int cem_proposals_call(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_cem* p,
                              const bcmpc_sampling* sampling, const bcmpc_proposals* prop, uint64_t seed,
                              int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out, double* costs_out,
                              bool single) {
    // (arguments first: a bad call is answered before any HIP call)
    if (const int rc = proposals_struct_check(prop)) return rc;
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !states || !p || !mu || !sigma || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (single && e->cfg.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "CEM needs a fused objective");
    if (const int rc = cem_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, false)) return rc;
    if (const int rc = batch_check(e, n_envs)) return rc;
    const int64_t K = e->cfg.num_paths / n_envs;
    if (const int rc = single ? k_global_check(p->k_global, "single-device CEM", K)
                              : k_global_check(p->k_global, "batched CEM", K, "num_paths / n_envs"))
        return rc;
    const bool keep = sampling && sampling->keep_elites;
    if (const int rc = proposals_check(prop, e, n_envs, K, keep ? p->n_elite : 0)) return rc;
    return plan_get_actions(e, states, n_envs, p, nullptr, sampling, seed, cand_offset, mu, sigma, nullptr, out, nullptr,
                            costs_out, nullptr, prop);
}

static int mppi_proposals_call(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_mppi* p,
                               const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext, const bcmpc_proposals* prop,
                               uint64_t seed, int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out,
                               bcmpc_mppi_stats* stats, double* costs_out, bool single) {
    // (arguments first: a bad call is answered before any HIP call)
    if (const int rc = mppi_ext_check(ext)) return rc;
    if (const int rc = proposals_struct_check(prop)) return rc;
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !states || !p || !mu || !sigma || !out || !stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = mppi_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, true)) return rc;
    if (single && e->cfg.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "MPPI needs a fused objective");
    if (const int rc = batch_check(e, n_envs)) return rc;
    const int64_t K = e->cfg.num_paths / n_envs;
    if (const int rc = single ? k_global_check(p->k_global, "single-device MPPI", K)
                              : k_global_check(p->k_global, "batched MPPI", K, "num_paths / n_envs"))
        return rc;
    if (const int rc = proposals_check(prop, e, n_envs, K, 0)) return rc;
    // (sigma is written back only under adapt_sigma, as in the _x calls)
    return plan_get_actions(e, states, n_envs, nullptr, p, sampling, seed, cand_offset, mu, sigma, sigma, out, stats,
                            costs_out, mppi_ext_default(ext) ? nullptr : ext, prop);
}

int bcmpc_cem_get_action_p(bcmpc_engine* e, const double* state, const bcmpc_cem* p, const bcmpc_sampling* sampling,
                           const bcmpc_proposals* prop, uint64_t seed, double* mu, double* sigma, bcmpc_result* out) {
    if (proposals_none(prop)) return bcmpc_cem_get_action_s(e, state, p, sampling, seed, mu, sigma, out);
    return cem_proposals_call(e, state, 1, p, sampling, prop, seed, 0, mu, sigma, out, nullptr, true);
}

int bcmpc_mppi_get_action_p(bcmpc_engine* e, const double* state, const bcmpc_mppi* p, const bcmpc_sampling* sampling,
                            const bcmpc_mppi_ext* ext, const bcmpc_proposals* prop, uint64_t seed, double* mu,
                            double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats) {
    if (proposals_none(prop)) return bcmpc_mppi_get_action_x(e, state, p, sampling, ext, seed, mu, sigma, out, stats);
    return mppi_proposals_call(e, state, 1, p, sampling, ext, prop, seed, 0, mu, sigma, out, stats, nullptr, true);
}

int bcmpc_cem_get_actions_batch_p(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_cem* p,
                                  const bcmpc_sampling* sampling, const bcmpc_proposals* prop, uint64_t seed,
                                  int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out, double* costs_out) {
    if (proposals_none(prop))
        return bcmpc_cem_get_actions_batch_s(e, states, n_envs, p, sampling, seed, cand_offset, mu, sigma, out, costs_out);
    return cem_proposals_call(e, states, n_envs, p, sampling, prop, seed, cand_offset, mu, sigma, out, costs_out, false);
}

int bcmpc_mppi_get_actions_batch_p(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_mppi* p,
                                   const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext,
                                   const bcmpc_proposals* prop, uint64_t seed, int64_t cand_offset, double* mu,
                                   double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats, double* costs_out) {
    if (proposals_none(prop))
        return bcmpc_mppi_get_actions_batch_x(e, states, n_envs, p, sampling, ext, seed, cand_offset, mu, sigma, out,
                                              stats, costs_out);
    return mppi_proposals_call(e, states, n_envs, p, sampling, ext, prop, seed, cand_offset, mu, sigma, out, stats,
                               costs_out, false);
}

// ... and with knot plans: off, the calls above; else the batched chain with plan_sample_knots as its
// sampler and the outer loop in knot space.  One body per planner, as for proposals.
static int cem_knots_call(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_cem* p,
                          const bcmpc_sampling* sampling, const bcmpc_proposals* prop, const bcmpc_knots* kn,
                          uint64_t seed, int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out,
                          double* costs_out, bool single) {
    // (arguments first: a bad call is answered before any HIP call)
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !states || !p || !mu || !sigma || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = knots_check(kn->count, kn->kind, e->cfg.horizon)) return rc;
    if (single && e->cfg.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "CEM needs a fused objective");
    if (const int rc = cem_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, false)) return rc;
    if (!proposals_none(prop))
        return fail(BCMPC_ERR_UNSUPPORTED, "knots with proposals are not supported (a given action sequence has no "
                                           "knot representation to refit on)");
    if (const int rc = batch_check(e, n_envs)) return rc;
    const int64_t K = e->cfg.num_paths / n_envs;
    if (const int rc = single ? k_global_check(p->k_global, "single-device CEM", K)
                              : k_global_check(p->k_global, "batched CEM", K, "num_paths / n_envs"))
        return rc;
    return plan_get_actions(e, states, n_envs, p, nullptr, sampling, seed, cand_offset, mu, sigma, nullptr, out, nullptr,
                            costs_out, nullptr, nullptr, kn);
}

static int mppi_knots_call(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_mppi* p,
                           const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext, const bcmpc_proposals* prop,
                           const bcmpc_knots* kn, uint64_t seed, int64_t cand_offset, double* mu, double* sigma,
                           bcmpc_result* out, bcmpc_mppi_stats* stats, double* costs_out, bool single) {
    // (arguments first: a bad call is answered before any HIP call)
    if (const int rc = mppi_ext_check(ext)) return rc;
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (!e || !states || !p || !mu || !sigma || !out || !stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = knots_check(kn->count, kn->kind, e->cfg.horizon)) return rc;
    if (const int rc = mppi_param_check(p)) return rc;
    if (const int rc = sampling_check(sampling, true)) return rc;
    if (single && e->cfg.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "MPPI needs a fused objective");
    if (!proposals_none(prop))
        return fail(BCMPC_ERR_UNSUPPORTED, "knots with proposals are not supported (a given action sequence has no "
                                           "knot representation to refit on)");
    if (const int rc = batch_check(e, n_envs)) return rc;
    const int64_t K = e->cfg.num_paths / n_envs;
    if (const int rc = single ? k_global_check(p->k_global, "single-device MPPI", K)
                              : k_global_check(p->k_global, "batched MPPI", K, "num_paths / n_envs"))
        return rc;
    // (sigma is written back only under adapt_sigma, as in the _x calls)
    return plan_get_actions(e, states, n_envs, nullptr, p, sampling, seed, cand_offset, mu, sigma, sigma, out, stats,
                            costs_out, mppi_ext_default(ext) ? nullptr : ext, nullptr, kn);
}

int bcmpc_cem_get_action_k(bcmpc_engine* e, const double* state, const bcmpc_cem* p, const bcmpc_sampling* sampling,
                           const bcmpc_proposals* prop, const bcmpc_knots* knots, uint64_t seed, double* mu,
                           double* sigma, bcmpc_result* out) {
    if (knots_none(knots)) return bcmpc_cem_get_action_p(e, state, p, sampling, prop, seed, mu, sigma, out);
    return cem_knots_call(e, state, 1, p, sampling, prop, knots, seed, 0, mu, sigma, out, nullptr, true);
}

int bcmpc_mppi_get_action_k(bcmpc_engine* e, const double* state, const bcmpc_mppi* p, const bcmpc_sampling* sampling,
                            const bcmpc_mppi_ext* ext, const bcmpc_proposals* prop, const bcmpc_knots* knots,
                            uint64_t seed, double* mu, double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats) {
    if (knots_none(knots)) return bcmpc_mppi_get_action_p(e, state, p, sampling, ext, prop, seed, mu, sigma, out, stats);
    return mppi_knots_call(e, state, 1, p, sampling, ext, prop, knots, seed, 0, mu, sigma, out, stats, nullptr, true);
}

int bcmpc_cem_get_actions_batch_k(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_cem* p,
                                  const bcmpc_sampling* sampling, const bcmpc_proposals* prop,
                                  const bcmpc_knots* knots, uint64_t seed, int64_t cand_offset, double* mu,
                                  double* sigma, bcmpc_result* out, double* costs_out) {
    if (knots_none(knots))
        return bcmpc_cem_get_actions_batch_p(e, states, n_envs, p, sampling, prop, seed, cand_offset, mu, sigma, out,
                                             costs_out);
    return cem_knots_call(e, states, n_envs, p, sampling, prop, knots, seed, cand_offset, mu, sigma, out, costs_out,
                          false);
}

int bcmpc_mppi_get_actions_batch_k(bcmpc_engine* e, const double* states, int32_t n_envs, const bcmpc_mppi* p,
                                   const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext,
                                   const bcmpc_proposals* prop, const bcmpc_knots* knots, uint64_t seed,
                                   int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out,
                                   bcmpc_mppi_stats* stats, double* costs_out) {
    if (knots_none(knots))
        return bcmpc_mppi_get_actions_batch_p(e, states, n_envs, p, sampling, ext, prop, seed, cand_offset, mu, sigma,
                                              out, stats, costs_out);
    return mppi_knots_call(e, states, n_envs, p, sampling, ext, prop, knots, seed, cand_offset, mu, sigma, out, stats,
                           costs_out, false);
}

int bcmpc_ensemble_cem_get_action(bcmpc_ensemble* s, const double* state, const bcmpc_cem* p, uint64_t seed,
                                  double* mu, double* sigma, bcmpc_result* out) {
    if (!s || !state || !p || !mu || !sigma || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = ensemble_call_check(s)) return rc;
    const bcmpc_config& c = s->m[0]->cfg;
    if (const int rc = cem_param_check(p)) return rc;
    if (const int rc = k_global_check(p->k_global, "ensemble CEM", c.num_paths)) return rc;
    if (c.num_paths == 0) return fail(BCMPC_ERR_EMPTY, "attempt to get argmin of an empty sequence");
    return plan_chain(s->m[0], s, state, p, nullptr, seed, mu, sigma, nullptr, out, nullptr);
}

int bcmpc_ensemble_mppi_get_action(bcmpc_ensemble* s, const double* state, const bcmpc_mppi* q, uint64_t seed,
                                   double* mu, const double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats) {
    if (!s || !state || !q || !mu || !sigma || !out || !stats) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = ensemble_call_check(s)) return rc;
    const bcmpc_config& c = s->m[0]->cfg;
    if (const int rc = mppi_param_check(q)) return rc;
    if (const int rc = k_global_check(q->k_global, "ensemble MPPI", c.num_paths)) return rc;
    if (c.num_paths == 0) return fail(BCMPC_ERR_EMPTY, "attempt to get argmin of an empty sequence");
    return plan_chain(s->m[0], s, state, nullptr, q, seed, mu, nullptr, sigma, out, stats);
}

}  // extern "C"

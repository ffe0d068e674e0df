// capi.cpp -- C ABI of libbcmpc (include/bcmpc.h): engine lifetime, the setters' uploads, the rollout launch, team
// ordering and fallback, the plain control steps, introspection (engine_plan.cpp: the checks and the kernel choice;
// pack.cpp: weight packing; cost_terms.cpp: the cost-term lists; mt_draw.cpp, planners.cpp: the rest)
#include "host_internal.h"

using namespace bcmpc::host;

namespace {

thread_local std::string g_last_error;

}  // namespace

namespace bcmpc {
int set_error(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
}  // namespace bcmpc

// Diagnostic hooks: the per-phase stamps of STAMP variant kernels (BCMPC_X3_STAMPS, BCMPC_STAMP_DUMP) are read
// only by a diagnostic build (-DBCMPC_DIAG_VARIANT: tools/build_variants.sh, tools/team_variants.sh); the
// production library never consults them.
static const char* diag_env(const char* name) {
#ifdef BCMPC_DIAG_VARIANT
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// Fault-injection hooks the GPU tests use (BCMPC_TEAM_SPINS=-1: every team gives up; comm.hip's
// BCMPC_COMM_FORCE_FLAGS): read in every build, and announced on stderr once per process when set, so a stray
// variable on a production run is visible.
namespace bcmpc {
void announce_test_hook(const char* name, const char* value) {
    static std::atomic<unsigned> said{0};
    const unsigned bit = name[6] == 'C' ? 1u : 2u;      // BCMPC_COMM_* / BCMPC_TEAM_*
    if (!(said.fetch_or(bit) & bit))
        std::fprintf(stderr, "libbcmpc: test hook %s=%s is active (fault injection; unset it for real runs)\n",
                     name, value);
}
}  // namespace bcmpc

// (team launch ordering across streams: team_order_before / team_order_after below)
struct TeamOrder {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t ev_stream = nullptr;
    bool pending = false;
};
static TeamOrder g_team_order[64];

int bcmpc::host::create_engine(const bcmpc_config* cfg, const CreateOpts& opts, bcmpc_engine** out) {
    if (!cfg || !out) return fail(BCMPC_ERR_ARG, "null argument");
    *out = nullptr;
    const bcmpc_config& c = *cfg;
    if (const int rc = check_config(c)) return rc;      // (the config's own refusals come before any HIP call)
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (c.device < 0 || c.device >= ndev) return fail(BCMPC_ERR_ARG, "device ordinal out of range");
    HIP_TRY(hipSetDevice(c.device));
    int ncu = 0;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c.device);
    EnginePlan plan;
    if (const int rc = plan_engine(c, opts, ncu, &plan)) return rc;

    bcmpc_engine* e = new bcmpc_engine(plan);
    e->ncu = ncu;
    auto cleanup = [&](int code) { bcmpc_destroy(e); return code; };
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&e->d_w, e->w_floats * sizeof(float)) != hipSuccess ||
        hipMalloc(&e->d_b, e->b_floats * sizeof(float)) != hipSuccess ||
        hipMalloc(&e->d_ln, e->ln_floats * sizeof(float)) != hipSuccess ||
        hipMalloc(&e->d_consts, sizeof(e->h_consts)) != hipSuccess ||
        hipMalloc(&e->d_state, BCMPC_MAX_STATE * sizeof(double)) != hipSuccess ||
        hipMalloc(&e->d_costs, std::max<int64_t>(1, c.num_paths) * sizeof(double)) != hipSuccess ||
        hipMalloc(&e->d_result, sizeof(bcmpc_result)) != hipSuccess ||
        // (the split kernel's fused argmin keeps one record per workgroup)
        hipMalloc(&e->d_amin_c, (e->amin_cap = std::max<size_t>(kArgminParts, (size_t)(c.num_paths + 15) / 16)) *
                                    sizeof(double)) != hipSuccess ||
        hipMalloc(&e->d_amin_i, e->amin_cap * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&e->d_amin_ticket, sizeof(unsigned)) != hipSuccess ||
        hipMemset(e->d_amin_ticket, 0, sizeof(unsigned)) != hipSuccess ||
        hipHostMalloc(&e->h_result, sizeof(bcmpc_result), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&e->h_result_map, sizeof(bcmpc_result), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&e->d_result_map, e->h_result_map, 0) != hipSuccess ||
        hipHostMalloc(&e->h_done, sizeof(unsigned long long), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&e->d_done, e->h_done, 0) != hipSuccess) {
        g_last_error = "device allocation failed";
        return cleanup(BCMPC_ERR_HIP);
    }
    for (int i = 0; i < 3; ++i)
        if (hipEventCreate(&e->ev[i]) != hipSuccess) { g_last_error = "event create failed"; return cleanup(BCMPC_ERR_HIP); }
    if (e->kernel == BCMPC_KERNEL_TEAM) {
        const size_t tb = team_buf_bytes(c.num_paths, e->HP, e->team_kind);
        if ((tb && hipMalloc(&e->d_team, tb) != hipSuccess) ||
            (tb && hipMemset(e->d_team, 0, tb) != hipSuccess) ||
            hipMalloc(&e->d_team_ctl, 4 * sizeof(unsigned)) != hipSuccess ||
            hipMemset(e->d_team_ctl, 0, 4 * sizeof(unsigned)) != hipSuccess ||
            hipHostMalloc(&e->h_team_err, sizeof(unsigned), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer((void**)&e->d_team_err, e->h_team_err, 0) != hipSuccess) {
            g_last_error = "device allocation failed";
            return cleanup(BCMPC_ERR_HIP);
        }
        *e->h_team_err = 0;
    }
    if (e->PL > 0) {
        if (hipMalloc(&e->d_pw, e->pw_floats * sizeof(float)) != hipSuccess ||
            hipMalloc(&e->d_pb, ((size_t)e->PL * e->PHP + kPolParams) * sizeof(float)) != hipSuccess ||
            hipMalloc(&e->d_first, std::max<int64_t>(1, c.num_paths) * c.action_dim * sizeof(double)) != hipSuccess) {
            g_last_error = "device allocation failed";
            return cleanup(BCMPC_ERR_HIP);
        }
    }
    if (c.cost == BCMPC_COST_TERMS &&
        hipMalloc(&e->d_tc_traj, (size_t)(c.horizon + 1) * (size_t)std::max<int64_t>(1, c.num_paths) * c.state_dim *
                                     sizeof(double)) != hipSuccess) {
        g_last_error = "device allocation failed (the trajectory scratch of the cost terms)";
        return cleanup(BCMPC_ERR_HIP);
    }
    if (e->reward) {
        if (hipMalloc(&e->d_gpow, (size_t)c.horizon * sizeof(double)) != hipSuccess) {
            g_last_error = "device allocation failed";
            return cleanup(BCMPC_ERR_HIP);
        }
        std::vector<double> ones((size_t)c.horizon, 1.0);
        if (hipMemcpy(e->d_gpow, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
            g_last_error = "gamma upload failed";
            return cleanup(BCMPC_ERR_HIP);
        }
    }
    // default action bounds: HalfCheetah ctrlrange [-1, 1]
    for (int j = 0; j < BCMPC_MAX_ACTION && j < kConstCols; ++j) {
        e->h_consts[6 * kConstCols + j] = -1.0;
        e->h_consts[7 * kConstCols + j] = 1.0;
    }
    *out = e;
    return BCMPC_OK;
}

extern "C" {

int bcmpc_abi_version(void) { return BCMPC_ABI_VERSION; }
const char* bcmpc_last_error(void) { return g_last_error.c_str(); }

int bcmpc_create(const bcmpc_config* cfg, bcmpc_engine** out) { return create_engine(cfg, CreateOpts{}, out); }

int bcmpc_destroy(bcmpc_engine* e) {
    if (!e) return BCMPC_OK;
    if (e->fb) (void)bcmpc_destroy(e->fb);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->stream && e->cfg.device >= 0 && e->cfg.device < 64) {   // its team launches have completed
        TeamOrder& d = g_team_order[e->cfg.device];
        std::lock_guard<std::mutex> lk(d.mu);
        if (d.ev_stream == e->stream) {
            d.pending = false;
            d.ev_stream = nullptr;
        }
    }
    if (e->spec_st) {
        (void)hipStreamSynchronize(e->spec_st);
        (void)hipStreamDestroy(e->spec_st);
    }
    for (hipEvent_t ev : {e->spec_in_ev, e->spec_done_ev})
        if (ev) (void)hipEventDestroy(ev);
    for (void* p : {(void*)e->d_spec_xs, (void*)e->d_spec_part})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)e->d_w, (void*)e->d_b, (void*)e->d_ln, (void*)e->d_consts, (void*)e->d_state,
                    (void*)e->d_actions, (void*)e->d_costs, (void*)e->d_result, (void*)e->d_pw, (void*)e->d_pb,
                    (void*)e->d_first, (void*)e->d_gpow, (void*)e->d_mu, (void*)e->d_sigma, (void*)e->d_elite,
                    (void*)e->d_count, (void*)e->d_mppi, (void*)e->d_mppi_stats, (void*)e->d_mppi_scores, (void*)e->d_amin_c, (void*)e->d_amin_i,
                    (void*)e->d_amin_ticket, (void*)e->d_team, (void*)e->d_team_ctl, (void*)e->d_mt_io, (void*)e->d_mt_bounds, (void*)e->d_mt_xs,
                    (void*)e->d_mt_polys, (void*)e->d_mt_chunks, (void*)e->d_mt_part, (void*)e->d_tiled,
                    (void*)e->d_bstates, (void*)e->d_bresults, (void*)e->d_bmu, (void*)e->d_bsigma, (void*)e->d_bcount,
                    (void*)e->d_bstats, (void*)e->d_belite, (void*)e->d_keep, (void*)e->d_keep_count, (void*)e->d_prop,
                    (void*)e->d_knots, (void*)e->d_tc_traj,
                    (void*)e->d_vw, (void*)e->d_vparams, (void*)e->d_vvalues, (void*)e->d_tc_steps,
                    (void*)e->d_tc_ref, (void*)e->d_tc_prev})
        if (p) (void)hipFree(p);
    if (e->h_bresults) (void)hipHostFree(e->h_bresults);
    if (e->h_result) (void)hipHostFree(e->h_result);
    if (e->h_result_map) (void)hipHostFree(e->h_result_map);
    if (e->h_team_err) (void)hipHostFree(e->h_team_err);
    if (e->h_done) (void)hipHostFree(e->h_done);
    if (e->h_stage) (void)hipHostFree(e->h_stage);
    if (e->pre.th.joinable()) {
        {
            std::lock_guard<std::mutex> lk(e->pre.mu);
            e->pre.quit = true;
            e->pre.quit_a.store(true, std::memory_order_release);
        }
        e->pre.cv.notify_all();
        e->pre.th.join();
    }
    for (double* p : e->h_zc)
        if (p) (void)hipHostFree(p);
    if (e->h_rows_seq) (void)hipHostFree(e->h_rows_seq);
    if (e->copy_st) (void)hipStreamSynchronize(e->copy_st);
    for (int i = 0; i < 2; ++i) {
        if (e->d_rows[i]) (void)hipFree(e->d_rows[i]);
        if (e->copy_ev[i]) (void)hipEventDestroy(e->copy_ev[i]);
    }
    if (e->copy_st) (void)hipStreamDestroy(e->copy_st);
    if (e->h_mt_io) (void)hipHostFree(e->h_mt_io);
    for (auto& sp : e->spec) {
        if (sp.d_io) (void)hipFree(sp.d_io);
        if (sp.h_io) (void)hipHostFree(sp.h_io);
        if (sp.d_act) (void)hipFree(sp.d_act);
    }
    for (auto& ev : e->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return BCMPC_OK;
}

uint64_t bcmpc_weights_version(const bcmpc_engine* e) { return e ? e->version : 0; }

int bcmpc_predraw_stats(const bcmpc_engine* e, uint64_t* out5) {
    if (!e || !out5) return fail(BCMPC_ERR_ARG, "null argument");
    out5[0] = e->pre.hits;
    out5[1] = e->pre.late;
    out5[2] = e->pre.misses;
    out5[3] = e->spec_hits;
    out5[4] = e->spec_misses;
    return BCMPC_OK;
}

int bcmpc_set_weights(bcmpc_engine* e, const bcmpc_weights* w, uint64_t version) {
    if (!e || !w || !w->kernels || !w->biases) return fail(BCMPC_ERR_ARG, "null argument");
    if (e->has_weights && version == e->version) return BCMPC_OK;    // idempotent re-sync
    const bcmpc_config& c = e->cfg;
    const int L = c.n_layers;
    if (c.layer_norm && (!w->ln_gamma || !w->ln_beta)) return fail(BCMPC_ERR_ARG, "layer_norm enabled but LN params missing");
    if (!w->mean_obs || !w->std_obs || !w->mean_action || !w->std_action || !w->mean_deltas || !w->std_deltas)
        return fail(BCMPC_ERR_ARG, "normalization stats missing");
    const bool rw = e->reward;
    if (rw && (!w->mean_reward || !w->std_reward)) return fail(BCMPC_ERR_ARG, "reward model: mean_reward / std_reward missing");
    const int NK = rw ? 5 : L + 1, NLN = rw ? 3 : L;      // kernels, LayerNorms
    for (int l = 0; l < NK; ++l)
        if (!w->kernels[l] || !w->biases[l]) return fail(BCMPC_ERR_ARG, "null kernel/bias pointer");
    if (c.layer_norm)
        for (int l = 0; l < NLN; ++l)
            if (!w->ln_gamma[l] || !w->ln_beta[l]) return fail(BCMPC_ERR_ARG, "null LayerNorm pointer");
    PackedNet pk;
    pack_weights(*e, *w, &pk);
    HIP_TRY(hipSetDevice(c.device));
    for (int row : {0, 1, 2, 3, 4, 5, 8, 9})              // (rows 6, 7: the action bounds stay)
        std::memcpy(e->h_consts + row * kConstCols, pk.consts + row * kConstCols, sizeof(double) * kConstCols);
    HIP_TRY(hipMemcpyAsync(e->d_w, pk.w.data(), pk.w.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_b, pk.b.data(), pk.b.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_ln, pk.ln.data(), pk.ln.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_consts, e->h_consts, sizeof(e->h_consts), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));   // the packed vectors die at scope exit
    std::copy(std::begin(pk.winv), std::end(pk.winv), e->winv);
    std::copy(std::begin(pk.hsc), std::end(pk.hsc), e->hsc);
    e->pp_fold_w = pk.pp_fold_w;
    e->team_defer = pk.team_defer;
    e->mean_reward = pk.mean_reward;
    e->std_reward = pk.std_reward;
    // (the fallback engine's copy: created only if a team ever fails to meet)
    if (e->kernel == BCMPC_KERNEL_TEAM) e->hw_copy.capture(*e, *w);
    e->version = version;
    e->has_weights = true;
    return BCMPC_OK;
}

int bcmpc_set_policy(bcmpc_engine* e, const bcmpc_policy* p, uint64_t version) {
    if (!e || !p || !p->kernels || !p->biases || !p->ob_mean || !p->ob_std || !p->logstd)
        return fail(BCMPC_ERR_ARG, "null argument");
    if (e->PL == 0) return fail(BCMPC_ERR_STATE, "engine was created without a policy (config.policy_hidden == 0)");
    if (e->has_policy && version == e->pol_version) { e->explore = p->explore; return BCMPC_OK; }
    const bcmpc_config& c = e->cfg;
    for (int l = 0; l <= e->PL; ++l)
        if (!p->kernels[l] || !p->biases[l]) return fail(BCMPC_ERR_ARG, "null policy kernel/bias pointer");
    PackedPolicy pk;
    pack_policy(*e, *p, &pk);
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipMemcpyAsync(e->d_pw, pk.w.data(), pk.w.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->d_pb, pk.b.data(), pk.b.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    std::copy(std::begin(pk.pwinv), std::end(pk.pwinv), e->pwinv);
    if (e->kernel == BCMPC_KERNEL_TEAM) e->hp_copy.capture(*e, *p);   // (the fallback engine's copy)
    e->explore = p->explore;
    e->pol_version = version;
    e->has_policy = true;
    return BCMPC_OK;
}

int bcmpc_first_actions(bcmpc_engine* e, double* out) {
    if (!e || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (!e->d_first) return fail(BCMPC_ERR_STATE, "engine has no policy");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpy(out, e->d_first, sizeof(double) * e->cfg.num_paths * e->cfg.action_dim, hipMemcpyDeviceToHost));
    return BCMPC_OK;
}

// (the three list setters: every check, the stored lists and the launch template are cost_terms.cpp's)
int bcmpc_set_cost_terms(bcmpc_engine* e, const bcmpc_cost_term* terms, int32_t n) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = set_terms(e->cfg, &e->cost, terms, n)) return rc;
    if (e->fb) return bcmpc_set_cost_terms(e->fb, terms, n);
    return BCMPC_OK;
}

int bcmpc_set_cost_terms_x(bcmpc_engine* e, const bcmpc_cost_term_x* terms, int32_t n, int32_t n_ref) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = set_terms_x(e->cfg, &e->cost, terms, n, n_ref)) return rc;
    if (e->fb) return bcmpc_set_cost_terms_x(e->fb, terms, n, n_ref);
    return BCMPC_OK;
}

int bcmpc_set_termination(bcmpc_engine* e, const bcmpc_cost_term* conds, int32_t n, double done_cost) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    const bcmpc_config& c = e->cfg;
    if (const int rc = check_termination(c, e->cost, conds, n, done_cost)) return rc;
    if (n > 0 && !e->d_tc_steps) {
        HIP_TRY(hipSetDevice(c.device));
        HIP_TRY(hipMalloc(&e->d_tc_steps, (size_t)std::max<int64_t>(1, c.num_paths) * sizeof(int32_t)));
    }
    store_termination(c, &e->cost, conds, n, done_cost);
    if (e->fb) return bcmpc_set_termination(e->fb, conds, n, done_cost);
    return BCMPC_OK;
}

int bcmpc_set_cost_inputs(bcmpc_engine* e, const double* ref, int32_t ref_envs, int32_t ref_steps,
                          const double* prev_action, int32_t prev_envs) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    const bcmpc_config& c = e->cfg;
    if (c.cost != BCMPC_COST_TERMS || !e->cost.has_terms || !e->cost.ext)
        return fail(BCMPC_ERR_ARG, "cost inputs need a list set with bcmpc_set_cost_terms_x that names a reference "
                                   "channel or has a RATE term");
    const int n_ref = e->cost.n_ref;
    const int64_t env_cap = std::max<int64_t>(1, c.num_paths);
    if (n_ref > 0) {
        if (!ref) return fail(BCMPC_ERR_ARG, "the list names reference channels: ref must not be null");
        if (ref_steps != 1 && ref_steps != c.horizon)
            return fail(BCMPC_ERR_ARG, "ref_steps must be 1 or the horizon (" + std::to_string(c.horizon) + "), not " +
                                           std::to_string(ref_steps));
        if (ref_envs < 1 || ref_envs > env_cap) return fail(BCMPC_ERR_ARG, "ref_envs must be in [1, num_paths]");
    } else if (ref) {
        return fail(BCMPC_ERR_ARG, "the list names no reference channel: ref must be null");
    }
    if (prev_action && !e->cost.tpl.has_rate) return fail(BCMPC_ERR_ARG, "the list has no RATE term: prev_action must be null");
    if (prev_action && (prev_envs < 1 || prev_envs > env_cap))
        return fail(BCMPC_ERR_ARG, "prev_envs must be in [1, num_paths]");
    const size_t nr = n_ref > 0 ? (size_t)ref_envs * (size_t)ref_steps * (size_t)n_ref : 0;
    const size_t np = prev_action ? (size_t)prev_envs * (size_t)c.action_dim : 0;
    HIP_TRY(hipSetDevice(c.device));
    if (nr > e->tc_ref_cap) {                            // (grow only: the same sizes keep their addresses)
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->d_tc_ref) HIP_TRY(hipFree(e->d_tc_ref));
        e->d_tc_ref = nullptr; e->tc_ref_cap = 0;
        HIP_TRY(hipMalloc(&e->d_tc_ref, nr * sizeof(double)));
        e->tc_ref_cap = nr;
    }
    if (np > e->tc_prev_cap) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->d_tc_prev) HIP_TRY(hipFree(e->d_tc_prev));
        e->d_tc_prev = nullptr; e->tc_prev_cap = 0;
        HIP_TRY(hipMalloc(&e->d_tc_prev, np * sizeof(double)));
        e->tc_prev_cap = np;
    }
    e->cost.has_inputs = false;
    if (nr) {
        e->h_in_ref.assign(ref, ref + nr);
        HIP_TRY(hipMemcpyAsync(e->d_tc_ref, e->h_in_ref.data(), nr * sizeof(double), hipMemcpyHostToDevice, e->stream));
    } else {
        e->h_in_ref.clear();
    }
    if (np) {
        e->h_in_prev.assign(prev_action, prev_action + np);
        HIP_TRY(hipMemcpyAsync(e->d_tc_prev, e->h_in_prev.data(), np * sizeof(double), hipMemcpyHostToDevice, e->stream));
    } else {
        e->h_in_prev.clear();
    }
    // the uploads have landed when the call returns: an entry on any other stream (bcmpc_rollout_async on the
    // caller's, a graph replay) needs no ordering of its own against them
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->cost.in_ref_envs = nr ? ref_envs : 0;
    e->cost.in_ref_steps = nr ? ref_steps : 0;
    e->cost.in_prev_envs = np ? prev_envs : 0;
    e->cost.has_inputs = true;
    if (e->fb) return bcmpc_set_cost_inputs(e->fb, ref, ref_envs, ref_steps, prev_action, prev_envs);
    return BCMPC_OK;
}

int bcmpc_cost_input_buffers(bcmpc_engine* e, void** d_ref, void** d_prev) {
    if (!e || !d_ref || !d_prev) return fail(BCMPC_ERR_ARG, "null argument");
    *d_ref = e->d_tc_ref;
    *d_prev = e->d_tc_prev;
    return BCMPC_OK;
}

int bcmpc_last_termination_steps(bcmpc_engine* e, const int64_t* idx, int32_t n, int32_t* out) {
    if (!e || !idx || !out || n < 1) return fail(BCMPC_ERR_ARG, "null argument");
    if (e->cost.conds.empty() || !e->d_tc_steps) return fail(BCMPC_ERR_STATE, "bcmpc_set_termination has not been called");
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= e->cfg.num_paths) return fail(BCMPC_ERR_ARG, "candidate index outside [0, num_paths)");
    const bcmpc_engine* src = e->steps_on_fb && e->fb && e->fb->d_tc_steps ? e->fb : e;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipStreamSynchronize(src->stream));
    for (int i = 0; i < n; ++i)
        HIP_TRY(hipMemcpy(out + i, src->d_tc_steps + idx[i], sizeof(int32_t), hipMemcpyDeviceToHost));
    return BCMPC_OK;
}

// one term-cost launch on st: the engine's template plus this launch's trajectory, action source and K; in: the
// inputs of an extended list (else nullptr)
static int term_cost_launch(bcmpc_engine* e, const double* d_traj, const double* d_actions, uint64_t seed,
                            int64_t cand_offset, const double* d_mu, const double* d_sigma, int32_t cem_iter,
                            int64_t K, double* d_costs, int32_t* d_term_step, hipStream_t st,
                            const CostInputs* in = nullptr) {
    TermCostXArgs x = e->cost.tpl;
    TermCostArgs& a = x.b;
    a.traj = d_traj; a.actions = d_actions; a.costs = d_costs;
    a.term_step = d_term_step;                           // (read by the DONE instances only)
    a.cem_mu = d_mu; a.cem_sigma = d_sigma; a.cem_iter = cem_iter;
    a.seed = seed; a.cand_offset = cand_offset; a.K = K;
    for (int j = 0; j < e->cfg.action_dim; ++j) {
        a.low[j] = e->h_consts[6 * kConstCols + j];
        a.high[j] = e->h_consts[7 * kConstCols + j];
    }
    if (!e->cost.ext) {
        HIP_TRY(launch_term_cost(a, st));
        return BCMPC_OK;
    }
    bind_inputs(*in, e->cfg.action_dim, &x);
    HIP_TRY(launch_term_cost_x(x, st));
    return BCMPC_OK;
}

// the inputs of an extended list for a launch over n_envs environments, from what bcmpc_set_cost_inputs left
static int engine_cost_inputs(const bcmpc_engine* e, int64_t K, int32_t n_envs, CostInputs* in) {
    return stored_inputs(e->cost, K, n_envs, e->d_tc_ref, e->d_tc_prev, in);
}

static int trajectory_cost_check(bcmpc_engine* e, const double* d_traj, const double* d_mu, const double* d_sigma,
                                 int32_t cem_iter, int64_t K, const double* d_costs) {
    if (!e || !d_traj || !d_costs) return fail(BCMPC_ERR_ARG, "null argument");
    if (e->cfg.cost != BCMPC_COST_TERMS) return fail(BCMPC_ERR_ARG, "trajectory_cost needs an engine created with BCMPC_COST_TERMS");
    if (K < 1) return fail(BCMPC_ERR_ARG, "K must be >= 1");
    if (d_mu && !d_sigma) return fail(BCMPC_ERR_ARG, "d_mu without d_sigma");
    if (cem_iter < 0 || cem_iter >= (1 << 22)) return fail(BCMPC_ERR_ARG, "cem_iter must be in [0, 2^22)");
    if (!e->cost.has_terms) return fail(BCMPC_ERR_STATE, "bcmpc_set_cost_terms has not been called");
    return BCMPC_OK;
}

int bcmpc_trajectory_cost_steps_async(bcmpc_engine* e, const double* d_traj, const double* d_actions, uint64_t seed,
                                      int64_t cand_offset, const double* d_mu, const double* d_sigma,
                                      int32_t cem_iter, int64_t K, double* d_costs, int32_t* d_term_step,
                                      void* stream) {
    if (const int rc = trajectory_cost_check(e, d_traj, d_mu, d_sigma, cem_iter, K, d_costs)) return rc;
    CostInputs in{};
    if (e->cost.ext) {                                   // an extended list: one environment, the engine's inputs
        if (const int rc = stored_inputs_one_env(e->cost, K, e->d_tc_ref, e->d_tc_prev, &in)) return rc;
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    return term_cost_launch(e, d_traj, d_actions, seed, cand_offset, d_mu, d_sigma, cem_iter, K, d_costs, d_term_step,
                            (hipStream_t)stream, &in);
}

int bcmpc_trajectory_cost_inputs_async(bcmpc_engine* e, const double* d_traj, const double* d_actions, uint64_t seed,
                                       int64_t cand_offset, const double* d_mu, const double* d_sigma,
                                       int32_t cem_iter, int64_t K, double* d_costs, int32_t* d_term_step,
                                       int64_t env_paths, const double* d_ref, int32_t ref_envs, int32_t ref_steps,
                                       const double* d_prev, int32_t prev_envs, void* stream) {
    if (const int rc = trajectory_cost_check(e, d_traj, d_mu, d_sigma, cem_iter, K, d_costs)) return rc;
    if (!e->cost.ext) return fail(BCMPC_ERR_STATE, "bcmpc_set_cost_terms_x has not set a list with reference channels or RATE terms");
    if (env_paths < 1 || K % env_paths != 0) return fail(BCMPC_ERR_ARG, "K must be a multiple of env_paths >= 1");
    const int64_t n_envs = K / env_paths;
    if (e->cost.tpl.n_ref_slots > 0) {
        if (!d_ref) return fail(BCMPC_ERR_ARG, "the list names reference channels: d_ref must not be null");
        if (ref_envs != 1 && ref_envs != n_envs) return fail(BCMPC_ERR_ARG, "ref_envs must be 1 or K / env_paths");
        if (ref_steps != 1 && ref_steps != e->cfg.horizon) return fail(BCMPC_ERR_ARG, "ref_steps must be 1 or the horizon");
    }
    if (d_prev && e->cost.tpl.has_rate && prev_envs != 1 && prev_envs != n_envs)
        return fail(BCMPC_ERR_ARG, "prev_envs must be 1 or K / env_paths");
    CostInputs in{};
    in.env_paths = env_paths;
    in.ref = d_ref; in.ref_envs = ref_envs; in.ref_steps = ref_steps;
    in.prev = d_prev; in.prev_envs = d_prev ? prev_envs : 0;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return term_cost_launch(e, d_traj, d_actions, seed, cand_offset, d_mu, d_sigma, cem_iter, K, d_costs, d_term_step,
                            (hipStream_t)stream, &in);
}

int bcmpc_trajectory_cost_async(bcmpc_engine* e, const double* d_traj, const double* d_actions, uint64_t seed,
                                int64_t cand_offset, const double* d_mu, const double* d_sigma, int32_t cem_iter,
                                int64_t K, double* d_costs, void* stream) {
    return bcmpc_trajectory_cost_steps_async(e, d_traj, d_actions, seed, cand_offset, d_mu, d_sigma, cem_iter, K,
                                             d_costs, nullptr, stream);
}

int bcmpc_terminal_value_supported(const bcmpc_config* cfg) {
    if (!cfg) return fail(BCMPC_ERR_ARG, "null argument");
    if (cfg->policy_hidden > 0)
        return fail(BCMPC_ERR_UNSUPPORTED, "terminal value: engines with a fused policy are not covered");
    if (cfg->model == BCMPC_MODEL_REWARD || cfg->cost == BCMPC_COST_REWARD)
        return fail(BCMPC_ERR_UNSUPPORTED, "terminal value: the reward model / BCMPC_COST_REWARD is not covered");
    if (cfg->cost == BCMPC_COST_NONE)
        return fail(BCMPC_ERR_UNSUPPORTED, "terminal value: a BCMPC_COST_NONE engine has no cost vector to add it to");
    return BCMPC_OK;
}

int bcmpc_set_terminal_value(bcmpc_engine* e, const bcmpc_value_net* v, double weight, uint64_t version) {
    // the net first, then the engine: every check before any HIP call
    if (v) {
        if (!v->kernels || !v->biases || !v->ob_mean || !v->ob_std) return fail(BCMPC_ERR_ARG, "value net: null argument");
        if (v->n_layers < 1 || v->n_layers > BCMPC_VALUE_MAX_LAYERS)
            return fail(BCMPC_ERR_ARG, "value net: n_layers must be in [1, 4]");
        if (v->hidden < 1 || v->hidden > BCMPC_VALUE_MAX_HIDDEN)
            return fail(BCMPC_ERR_ARG, "value net: hidden must be in [1, 256]");
        if (v->state_dim < 1 || v->state_dim > BCMPC_MAX_STATE)
            return fail(BCMPC_ERR_ARG, "value net: state_dim must be in [1, 32]");
        if (v->reserved != 0) return fail(BCMPC_ERR_ARG, "value net: reserved must be zero");
        if (!std::isfinite(weight)) return fail(BCMPC_ERR_ARG, "terminal value: weight must be finite");
        for (int l = 0; l <= v->n_layers; ++l) {
            if (!v->kernels[l] || !v->biases[l]) return fail(BCMPC_ERR_ARG, "value net: null argument");
            const int in = l == 0 ? v->state_dim : v->hidden, out = l == v->n_layers ? 1 : v->hidden;
            for (int i = 0; i < in * out; ++i)
                if (!std::isfinite(v->kernels[l][i])) return fail(BCMPC_ERR_ARG, "value net: a kernel entry is not finite");
            for (int i = 0; i < out; ++i)
                if (!std::isfinite(v->biases[l][i])) return fail(BCMPC_ERR_ARG, "value net: a bias entry is not finite");
        }
        for (int i = 0; i < v->state_dim; ++i) {
            if (!std::isfinite(v->ob_mean[i])) return fail(BCMPC_ERR_ARG, "value net: ob_mean must be finite");
            if (!std::isfinite(v->ob_std[i]) || !(v->ob_std[i] > 0.f))
                return fail(BCMPC_ERR_ARG, "value net: ob_std must be finite and > 0");
        }
    }
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    if (!v) {
        e->has_value = false;
        e->value_version = 0;
        if (e->fb) return bcmpc_set_terminal_value(e->fb, nullptr, 0.0, 0);
        return BCMPC_OK;
    }
    const bcmpc_config& c = e->cfg;
    if (const int rc = bcmpc_terminal_value_supported(&c)) return rc;
    if (e->comm)
        return fail(BCMPC_ERR_UNSUPPORTED, "terminal value: engines with a communicator attached do not exchange "
                                           "records inside the library yet");
    if (e->has_value && e->value_version == version) {
        e->tv.weight = weight;
        if (e->fb) return bcmpc_set_terminal_value(e->fb, v, weight, version);
        return BCMPC_OK;
    }
    // (S is the net's: a net over another state_dim runs through bcmpc_terminal_value_async alone; the rollout
    //  entries refuse it, rollout_impl)
    PackedValue pk;
    pack_value_net(*v, &pk);
    HIP_TRY(hipSetDevice(c.device));
    constexpr size_t kMaxW = (size_t)(2 * 16 + (BCMPC_VALUE_MAX_LAYERS - 1) * 16 * 16 + 16) * 256;
    if (!e->d_vw) HIP_TRY(hipMalloc(&e->d_vw, kMaxW * sizeof(float)));
    if (!e->d_vparams) HIP_TRY(hipMalloc(&e->d_vparams, (size_t)kTvParamFloats * sizeof(float)));
    if (!e->d_vvalues)
        HIP_TRY(hipMalloc(&e->d_vvalues, (size_t)std::max<int64_t>(1, c.num_paths) * sizeof(float)));
    if (!e->d_tc_traj)
        HIP_TRY(hipMalloc(&e->d_tc_traj, (size_t)(c.horizon + 1) * (size_t)std::max<int64_t>(1, c.num_paths) *
                                             c.state_dim * sizeof(double)));
    // (launches of the previous net on any stream of this device have to be over before its weights change)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(e->d_vw, pk.w.data(), pk.w.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_vparams, pk.params.data(), pk.params.size() * sizeof(float), hipMemcpyHostToDevice));
    TerminalValueArgs a{};
    for (int l = 0; l <= v->n_layers; ++l)
        a.w[l] = reinterpret_cast<const float __attribute__((ext_vector_type(4)))*>(e->d_vw + pk.off[l]);
    a.params = e->d_vparams;
    a.weight = weight;
    a.S = v->state_dim; a.L = v->n_layers; a.HP = pk.HP;
    e->tv = a;
    e->has_value = true;
    e->value_version = version;
    e->hv_copy.capture(*v);
    if (e->fb) return bcmpc_set_terminal_value(e->fb, v, weight, version);
    return BCMPC_OK;
}

// one terminal-value launch on st: the engine's template plus this launch's rows and outputs
static int terminal_value_launch(bcmpc_engine* e, const double* d_states, int64_t row_stride, int64_t K,
                                 float* d_values, double* d_costs, const int32_t* d_term_step, int32_t horizon,
                                 hipStream_t st) {
    TerminalValueArgs a = e->tv;
    a.states = d_states; a.row_stride = row_stride; a.K = K;
    a.values = d_values; a.costs = d_costs;
    a.term_step = d_term_step; a.horizon = horizon;
    HIP_TRY(launch_terminal_value(a, st));
    return BCMPC_OK;
}

int bcmpc_terminal_value_masked_async(bcmpc_engine* e, const double* d_states, int64_t row_stride, int64_t K,
                                      float* d_values, double* d_costs_inout, const int32_t* d_term_step,
                                      int32_t horizon, void* stream) {
    if (!e || !d_states) return fail(BCMPC_ERR_ARG, "null argument");
    if (!d_values && !d_costs_inout) return fail(BCMPC_ERR_ARG, "terminal_value needs d_values or d_costs_inout");
    if (K < 1) return fail(BCMPC_ERR_ARG, "K must be >= 1");
    if (!e->has_value) return fail(BCMPC_ERR_STATE, "bcmpc_set_terminal_value has not been called");
    if (row_stride < e->tv.S) return fail(BCMPC_ERR_ARG, "row_stride must be >= the value net's state_dim");
    HIP_TRY(hipSetDevice(e->cfg.device));
    return terminal_value_launch(e, d_states, row_stride, K, d_values, d_costs_inout, d_term_step, horizon,
                                 (hipStream_t)stream);
}

int bcmpc_terminal_value_async(bcmpc_engine* e, const double* d_states, int64_t row_stride, int64_t K,
                               float* d_values, double* d_costs_inout, void* stream) {
    return bcmpc_terminal_value_masked_async(e, d_states, row_stride, K, d_values, d_costs_inout, nullptr, 0, stream);
}

int bcmpc_last_terminal_values(bcmpc_engine* e, const int64_t* idx, int32_t n, float* out) {
    if (!e || !idx || !out || n < 1) return fail(BCMPC_ERR_ARG, "null argument");
    if (!e->has_value || !e->d_vvalues) return fail(BCMPC_ERR_STATE, "bcmpc_set_terminal_value has not been called");
    for (int i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= e->cfg.num_paths) return fail(BCMPC_ERR_ARG, "candidate index outside [0, num_paths)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n; ++i)
        HIP_TRY(hipMemcpy(out + i, e->d_vvalues + idx[i], sizeof(float), hipMemcpyDeviceToHost));
    return BCMPC_OK;
}

int bcmpc_set_action_bounds(bcmpc_engine* e, const double* low, const double* high) {
    if (!e || !low || !high) return fail(BCMPC_ERR_ARG, "null argument");
    for (int j = 0; j < e->cfg.action_dim; ++j) {
        e->h_consts[6 * 32 + j] = low[j];
        e->h_consts[7 * 32 + j] = high[j];
    }
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpyAsync(e->d_consts, e->h_consts, sizeof(e->h_consts), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return BCMPC_OK;
}

int bcmpc_set_discount(bcmpc_engine* e, double gamma) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    if (!e->reward) return fail(BCMPC_ERR_STATE, "discount applies to reward engines (config.model == BCMPC_MODEL_REWARD)");
    std::vector<double> g((size_t)e->cfg.horizon);
    for (int i = 0; i < e->cfg.horizon; ++i) g[i] = std::pow(gamma, (double)i);   // Python float ** int
    e->gamma = gamma;
    HIP_TRY(hipSetDevice(e->cfg.device));
    HIP_TRY(hipMemcpyAsync(e->d_gpow, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return BCMPC_OK;
}

void* bcmpc_stream(bcmpc_engine* e) { return e ? (void*)e->stream : nullptr; }

}  // extern "C"

namespace bcmpc::host {

// team kernel: a team whose workgroups could not all become resident gives up after its bounded
// spin and raises the mapped flag (rollout_team.hip).  Synchronous calls check it after their
// synchronisation and rerun on the fallback engine (team_rerun); stream-ordered callers read it with
// bcmpc_engine_status once their stream is done.  Reading clears it.
bool team_failed(bcmpc_engine* e) {
    if (e->h_team_err && __atomic_load_n(e->h_team_err, __ATOMIC_ACQUIRE) != 0) {
        __atomic_store_n(e->h_team_err, 0u, __ATOMIC_RELEASE);
        return true;
    }
    return false;
}
// a synchronous control step's failure check after its stream completed.  With a communicator
// attached, the exchange carried every rank's team status (comm.hip, wire record flags): the answer
// is the OR over the ranks, identical on every rank, so every rank reruns the step together (each on
// its fallback engine, which exchanges again) or none does
bool step_failed(bcmpc_engine* e) {
    const bool local = team_failed(e);
    if (e->comm) return comm_any_flags(e->comm);
    return local;
}

// the stream synchronisation of a synchronous call; with a communicator attached it is bounded
// (BCMPC_COMM_TIMEOUT_MS, default 60 s): a rank that never joins the exchange aborts the
// communicator and fails the call instead of holding every other rank forever
int sync_step(bcmpc_engine* e, hipStream_t st) {
    if (!e->comm) {
        const hipError_t se = hipStreamSynchronize(st);
        if (se != hipSuccess) return fail(BCMPC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
        return BCMPC_OK;
    }
    static const int64_t timeout_ms = [] {
        const char* v = std::getenv("BCMPC_COMM_TIMEOUT_MS");
        return v && *v ? std::max<int64_t>(1, std::atoll(v)) : int64_t(60000);
    }();
    std::string err;
    const int rc = comm_wait(e->comm, st, timeout_ms, &err);
    return rc == BCMPC_OK ? BCMPC_OK : fail(rc, err);
}

// the fallback engine of a team engine, created on first need and kept in sync with the team
// engine's weights / policy / discount / action bounds (host copies)
int team_fallback(bcmpc_engine* e, bool collective) {
    // (collective: every rank learned of the failure from the exchange and reruns with it; otherwise a
    //  rank with a communicator attached cannot rerun one step alone)
    if (e->comm && !collective)
        return fail(BCMPC_ERR_HIP, "team kernel: a workgroup team did not meet; with a communicator attached "
                                   "the ranks cannot rerun the step alone");
    if (!e->fb) {
        bcmpc_config c = e->cfg;
        c.kernel = BCMPC_KERNEL_AUTO;
        c.precision = BCMPC_PREC_SPLIT_F16;
        CreateOpts opts;
        opts.no_team = true;
        int rc = create_engine(&c, opts, &e->fb);
        if (rc == BCMPC_ERR_UNSUPPORTED) {               // split precision only on the team kernel: fp32
            c.precision = BCMPC_PREC_FP32;
            rc = create_engine(&c, opts, &e->fb);
        }
        if (rc != BCMPC_OK) return rc;
    }
    bcmpc_engine* f = e->fb;
    f->comm = collective ? e->comm : nullptr;        // (the rerun's exchange: every rank reruns)
    if (!e->fb_wset || e->fb_wver != e->version) {
        const bcmpc_weights w = e->hw_copy.view();
        if (const int rc = bcmpc_set_weights(f, &w, e->version)) return rc;
        e->fb_wver = e->version;
        e->fb_wset = true;
    }
    if (e->PL > 0) {
        if (!e->fb_pset || e->fb_pver != e->pol_version) {
            const bcmpc_policy p = e->hp_copy.view(e->explore);
            if (const int rc = bcmpc_set_policy(f, &p, e->pol_version)) return rc;
            e->fb_pver = e->pol_version;
            e->fb_pset = true;
        }
        f->explore = e->explore;
    }
    if (e->reward)
        if (const int rc = bcmpc_set_discount(f, e->gamma)) return rc;
    CostState& fc = f->cost;
    const CostState& ec = e->cost;
    if (ec.has_terms) {                              // (the same shape: the launch template carries over)
        if (fc.ext != ec.ext || fc.n_ref != ec.n_ref) fc.has_inputs = false;
        fc.terms = ec.terms;
        fc.refs = ec.refs;
        fc.n_ref = ec.n_ref;
        fc.ext = ec.ext;
        fc.tpl = ec.tpl;
        fc.has_terms = true;
        if (ec.ext && ec.has_inputs && !fc.has_inputs)       // (set before the fallback existed)
            if (const int rc = bcmpc_set_cost_inputs(f, e->h_in_ref.empty() ? nullptr : e->h_in_ref.data(), ec.in_ref_envs,
                                                     ec.in_ref_steps, e->h_in_prev.empty() ? nullptr : e->h_in_prev.data(),
                                                     ec.in_prev_envs))
                return rc;
    }
    fc.conds = ec.conds;                             // (a synchronous call: the fallback's step buffer may be made here)
    fc.done_cost = ec.done_cost;
    if (!fc.conds.empty() && !f->d_tc_steps)
        HIP_TRY(hipMalloc(&f->d_tc_steps, (size_t)std::max<int64_t>(1, f->cfg.num_paths) * sizeof(int32_t)));
    if (e->has_value && (!f->has_value || f->value_version != e->value_version || f->tv.weight != e->tv.weight)) {
        const bcmpc_value_net vn = e->hv_copy.view();
        if (const int rc = bcmpc_set_terminal_value(f, &vn, e->tv.weight, e->value_version)) return rc;
    } else if (!e->has_value && f->has_value) {
        if (const int rc = bcmpc_set_terminal_value(f, nullptr, 0.0, 0)) return rc;
    }
    double lo[BCMPC_MAX_ACTION], hi[BCMPC_MAX_ACTION];
    for (int j = 0; j < e->cfg.action_dim; ++j) {
        lo[j] = e->h_consts[6 * kConstCols + j];
        hi[j] = e->h_consts[7 * kConstCols + j];
    }
    if (const int rc = bcmpc_set_action_bounds(f, lo, hi)) return rc;
    f->timing = e->timing;
    ++e->team_reruns;
    e->steps_on_fb = true;                           // (bcmpc_last_termination_steps: the rerun's steps)
    return BCMPC_OK;
}

// the engine a failed synchronous step reruns on: a team engine's fallback engine.  With a communicator
// attached the failure is the OR over the ranks (step_failed), so a rank whose own kernel is not the team
// kernel also sees it: that rank reruns the same call on its own engine, which joins the collective
// rerun's exchange (it has no fallback engine and no host copies of its weights to build one from)
int rerun_engine(bcmpc_engine* e, bcmpc_engine** r) {
    if (e->comm && e->kernel != BCMPC_KERNEL_TEAM) {
        *r = e;
        return BCMPC_OK;
    }
    if (const int fr = team_fallback(e, e->comm != nullptr)) return fr;
    *r = e->fb;
    return BCMPC_OK;
}

// Team launches of one process on a device are ordered across streams: two team grids running at
// once could each hold part of the CUs the other needs.  A synchronous call's launch has completed
// when the call returns (the host waits for its argmin), so only stream-ordered launches can still
// be in flight: each records an event, and a team launch on another stream waits for it while it is
// pending.  No call on the earlier stream is made later (it may be gone by then); graph capture
// skips the ordering.

// (the same-stream shortcut only for an engine's own stream, which lives as long as the engine and is
//  cleared from the record in bcmpc_destroy: a caller's stream may be destroyed and its handle handed to a
//  new stream, whose team launch must then still wait for the old grid)
static int team_order_before(int device, hipStream_t st, hipStream_t own) {
    if (device < 0 || device >= 64) return BCMPC_OK;
    TeamOrder& d = g_team_order[device];
    std::lock_guard<std::mutex> lk(d.mu);
    if (!d.pending || (d.ev_stream == st && st == own)) return BCMPC_OK;
    const hipError_t q = hipEventQuery(d.ev);
    if (q == hipSuccess) {
        d.pending = false;
        return BCMPC_OK;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (cs == hipStreamCaptureStatusNone) HIP_TRY(hipStreamWaitEvent(st, d.ev, 0));
    return BCMPC_OK;
}

static int team_order_after(int device, hipStream_t st) {
    if (device < 0 || device >= 64) return BCMPC_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cs);
    if (cs != hipStreamCaptureStatusNone) return BCMPC_OK;
    TeamOrder& d = g_team_order[device];
    std::lock_guard<std::mutex> lk(d.mu);
    if (!d.ev) HIP_TRY(hipEventCreateWithFlags(&d.ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(d.ev, st));
    d.ev_stream = st;
    d.pending = true;
    return BCMPC_OK;
}

// A synchronous control step's completion: spin on the mapped word the argmin raises after its
// record (system-scope release) instead of a stream synchronisation, whose completion signal
// arrives several microseconds later; a stream synchronisation after 2 s (or BCMPC_SYNC=stream)
// reports whatever went wrong.  The stream may still run the argmin's epilogue: later work on it
// is stream-ordered.
int wait_done(bcmpc_engine* e, unsigned long long seq) {
    static const bool stream_sync = [] {
        const char* v = std::getenv("BCMPC_SYNC");
        return v && std::strcmp(v, "stream") == 0;
    }();
    if (!stream_sync) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i = 1;; ++i) {
            if (__atomic_load_n(e->h_done, __ATOMIC_ACQUIRE) == seq) return BCMPC_OK;
            if ((i & 4095) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
            __builtin_ia32_pause();
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return BCMPC_OK;
}

// diagnostics: STAMP variant kernels record 10 per-phase cycle counts per wave (BCMPC_X3_STAMPS=1 prints them).
// begin() grows and zeroes the buffer ahead of the launch, print() reads it back behind it: the team kernel's wave 0
// against its others, else a workgroup's older half of waves (it wins the MFMA / VALU arbitration) against the younger
#ifdef BCMPC_DIAG_VARIANT
struct StampRun {
    size_t blocks = 0, waves = 0;
    uint64_t* d = nullptr;                            // RolloutArgs.stamps; nullptr: stamps are off
    int begin(size_t nblocks, size_t nwaves, hipStream_t st) {
        static uint64_t* buf = nullptr;
        static size_t cap = 0;
        if (!diag_env("BCMPC_X3_STAMPS")) return BCMPC_OK;
        blocks = nblocks; waves = nwaves;
        if (cap < blocks * waves * 10) {
            if (buf) (void)hipFree(buf);
            cap = blocks * waves * 10;
            HIP_TRY(hipMalloc(&buf, cap * sizeof(uint64_t)));
        }
        HIP_TRY(hipMemsetAsync(buf, 0, cap * sizeof(uint64_t), st));
        d = buf;
        return BCMPC_OK;
    }
    int print(const char* const* names, bool team, const bcmpc_config& c, hipStream_t st) const {
        if (!d) return BCMPC_OK;
        std::vector<uint64_t> h(blocks * waves * 10);
        HIP_TRY(hipMemcpyAsync(h.data(), d, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        auto mean = [&](int k, bool first) {          // (team: over the waves that recorded the phase)
            double sum = 0;
            size_t n = 0;
            for (size_t b = 0; b < blocks; ++b)
                for (size_t w = 0; w < waves; ++w) {
                    const double v = (double)h[(b * waves + w) * 10 + k];
                    if ((team ? w == 0 : 2 * w < waves) != first || (team && v == 0)) continue;
                    sum += v;
                    ++n;
                }
            return n ? sum / n : 0.0;
        };
        if (team) {
            const char* dump = diag_env("BCMPC_STAMP_DUMP");        // raw [blocks][waves][10] records
            if (FILE* f = dump ? std::fopen(dump, "ab") : nullptr) {
                const int32_t hdr[4] = {(int32_t)blocks, (int32_t)waves, c.horizon, (int32_t)c.num_paths};
                std::fwrite(hdr, sizeof(hdr), 1, f);
                std::fwrite(h.data(), sizeof(uint64_t), h.size(), f);
                std::fclose(f);
            }
            std::fprintf(stderr, "team stamps (per step, s_memtime ticks; wave 0 | others):");
            for (int k = 0; k < 10; ++k) {
                const double div = k == 9 ? 1.0 : (double)c.horizon;
                std::fprintf(stderr, " %s=%.0f|%.0f", names[k], mean(k, true) / div, mean(k, false) / div);
            }
            std::fprintf(stderr, "\n");
            return BCMPC_OK;
        }
        for (int grp = 0; grp < 2; ++grp) {
            std::fprintf(stderr, "x3 stamps %s:", grp == 0 ? "waves<nw/2 " : "waves>=nw/2");
            for (int k = 0; k < 9; ++k) std::fprintf(stderr, " %s=%.0f", names[k], mean(k, grp == 0) / c.horizon);
            std::fprintf(stderr, "  (per step, s_memtime ticks)\n");
        }
        return BCMPC_OK;
    }
};
#else
struct StampRun {
    uint64_t* d = nullptr;
    int begin(size_t, size_t, hipStream_t) { return BCMPC_OK; }
    int print(const char* const*, bool, const bcmpc_config&, hipStream_t) const { return BCMPC_OK; }
};
#endif

// the argmin launch's arguments over d_costs [num_paths]: np.argmin (np.argmax for the learned reward), the
// first action from d_actions / the policy's output / Philox / the CEM sampler, CEM's cross-iteration merge,
// the completion word of a lean synchronous step.  rollout_impl launches it behind its rollout (or hands it
// to a kernel that reduces in its own tail); the ensemble calls launch it behind their reduce
ArgminArgs argmin_args(bcmpc_engine* e, const double* d_costs, const double* d_actions,
                              const double* act_out_all, uint64_t seed, int64_t cand_offset, bcmpc_result* d_result,
                              const CemLaunch* cem) {
    const bcmpc_config& c = e->cfg;
    ArgminArgs m{};
    m.costs = d_costs; m.actions = d_actions; m.consts = e->d_consts; m.out = d_result;
    m.act_out = e->PL > 0 ? (act_out_all ? act_out_all : e->d_first) : nullptr;
    m.seed = seed; m.cand_offset = cand_offset; m.K = c.num_paths; m.A = c.action_dim;
    m.maximize = c.cost == BCMPC_COST_REWARD;
    m.scratch_c = e->d_amin_c;
    m.scratch_i = e->d_amin_i;
    m.nparts = argmin_parts(c.num_paths);
    if (e->want_done && !e->comm) {
        m.done = e->d_done;
        m.seq = ++e->seq;
    }
    if (cem) {
        m.cem_mu = cem->mu; m.cem_sigma = cem->sigma; m.cem_iter = cem->iter;
        m.merge = cem->merge; m.pos_base = cem->pos_base;
    }
    return m;
}

int rollout_impl(bcmpc_engine* e, const RolloutLaunch& r) {
    const double *d_state = r.state, *d_actions = r.actions, *state_inline = r.state_inline;
    double *d_costs = r.costs, *d_traj = r.traj, *act_out_all = r.act_out_all;
    const int64_t stride = r.state_stride, cand_offset = r.cand_offset;
    const uint64_t seed = r.seed;
    bcmpc_result* const d_result = r.result;
    const hipStream_t st = r.stream;
    const CemLaunch* const cem = r.cem;
    const bcmpc_config& c = e->cfg;
    if (!e->has_weights) return fail(BCMPC_ERR_STATE, "bcmpc_set_weights has not been called");
    if (c.num_paths == 0) return fail(BCMPC_ERR_EMPTY, "attempt to get argmin of an empty sequence");
    if (stride != 0 && stride != c.state_dim) return fail(BCMPC_ERR_ARG, "state_stride must be 0 or state_dim");
    if (c.cost != BCMPC_COST_NONE && !d_costs) return fail(BCMPC_ERR_ARG, "the fused objective needs a costs buffer");
    if (d_result && c.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "argmin needs the fused cost");
    // cost terms: the rollout kernel runs as a BCMPC_COST_NONE launch that writes the trajectory (the caller's
    // or the scratch), term_cost_kernel turns it into d_costs, and the ordinary argmin launch follows
    const bool terms = c.cost == BCMPC_COST_TERMS;
    if (terms && !e->cost.has_terms) return fail(BCMPC_ERR_STATE, "bcmpc_set_cost_terms has not been called");
    CostInputs cost_in{};                                // an extended list: this call's reference / previous actions
    if (terms && e->cost.ext)
        if (const int rc = engine_cost_inputs(e, e->cfg.num_paths, r.n_envs, &cost_in)) return rc;
    // terminal value: the rollout also writes the trajectory (beside its fused cost), terminal_value_kernel adds
    // weight * V(traj[H][k]) to d_costs[k], and the ordinary argmin launch follows -- no fused argmin tail
    const bool value = e->has_value;
    if (value && e->comm)
        return fail(BCMPC_ERR_UNSUPPORTED, "engines with a terminal value do not exchange records inside the library yet");
    if (value && !d_costs) return fail(BCMPC_ERR_ARG, "the terminal value needs a costs buffer");
    if (value && e->tv.S != c.state_dim)
        return fail(BCMPC_ERR_ARG, "the value net reads " + std::to_string(e->tv.S) + " state dims, the engine has " +
                                       std::to_string(c.state_dim));
    if (terms || value) d_traj = d_traj ? d_traj : e->d_tc_traj;
    // termination: term_cost_kernel leaves every candidate's terminating step in the engine's buffer and
    // terminal_value_kernel adds the value only where that step is the horizon (the candidate is alive)
    int32_t* const d_steps = terms && e->cost.tpl.b.n_done > 0 ? e->d_tc_steps : nullptr;
    e->steps_on_fb = false;
    RolloutArgs a{};
    for (int l = 0; l < e->nwl; ++l) {
        const size_t end = l + 1 < e->nwl ? e->w_off[l + 1] : e->w_floats;
        a.wbytes[l] = (int32_t)((end - e->w_off[l]) * sizeof(float));
        a.w[l] = reinterpret_cast<const float __attribute__((ext_vector_type(4)))*>(e->d_w + e->w_off[l]);
    }
    for (int l = 0; l < (e->split && e->reward ? 4 : e->nwl); ++l) a.b[l] = e->d_b + e->b_off[l];
    if (e->reward) {   // trunk LN, then the two heads' LN params side by side (2*HP)
        a.lng[0] = e->d_ln;               a.lng[1] = e->d_ln + e->HP;
        a.lnb[0] = e->d_ln + 3 * e->HP;   a.lnb[1] = e->d_ln + 4 * e->HP;
        if (e->split) a.head_rs = e->d_b + e->b_off[4];
        a.model = BCMPC_MODEL_REWARD;
        a.mean_reward = e->mean_reward;
        a.std_reward = e->std_reward;
        a.gpow = e->d_gpow;
    } else {
        for (int l = 0; l < c.n_layers; ++l) {
            a.lng[l] = e->d_ln + (size_t)l * e->HP;
            a.lnb[l] = e->d_ln + (size_t)(c.n_layers + l) * e->HP;
        }
    }
    a.f16_single = e->f16 ? 1 : 0;
    a.x3_nw = e->nw;
    a.x3_pp = e->pp ? (e->pp_fold_w ? 2 : 1) : 0;
    a.consts = e->d_consts;
    a.state = d_state; a.state_stride = stride;
    if (state_inline) {                       // the tiled state by value in the kernel arguments
        a.state_inline = 1;
        for (int i = 0; i < c.state_dim; ++i) a.state_v[i] = state_inline[i];
    }
    a.actions = d_actions; a.costs = terms ? nullptr : d_costs; a.traj = d_traj;
    a.seed = seed; a.cand_offset = cand_offset; a.K = c.num_paths;
    a.H = c.horizon; a.S = c.state_dim; a.A = c.action_dim; a.L = c.n_layers;
    a.hidden = c.hidden; a.act = c.activation; a.ln = c.layer_norm; a.cost = terms ? BCMPC_COST_NONE : c.cost;
    if (e->PL > 0) {
        if (!e->has_policy) return fail(BCMPC_ERR_STATE, "bcmpc_set_policy has not been called");
        if (c.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_UNSUPPORTED, "policy engines need the fused cost");
        for (int l = 0; l <= e->PL; ++l) {
            const size_t end = l < e->PL ? e->pw_off[l + 1] : e->pw_floats;
            a.pwbytes[l] = (int32_t)((end - e->pw_off[l]) * sizeof(float));
            a.pw[l] = reinterpret_cast<const float __attribute__((ext_vector_type(4)))*>(e->d_pw + e->pw_off[l]);
        }
        for (int l = 0; l < e->PL; ++l) a.pb[l] = e->d_pb + (size_t)l * e->PHP;
        a.pparams = e->d_pb + (size_t)e->PL * e->PHP;
        a.pL = e->PL;
        a.phidden_padded = e->PHP;
        a.pol_mode = c.policy_mode;
        a.explore = e->explore;
        a.act_out = act_out_all ? act_out_all : e->d_first;      // [H][K][A] or step 0 only
        a.act_out_steps = act_out_all ? c.horizon : 1;
    }
    for (int l = 0; l < e->nwl; ++l) a.winv[l] = e->winv[l];
    for (int l = 0; l <= e->PL; ++l) a.pwinv[l] = e->pwinv[l];
    for (int l = 0; l < c.n_layers; ++l) a.hsc[l] = e->hsc[l];
    if (cem) {
        if (e->kernel == BCMPC_KERNEL_SOLO || e->PL > 0)
            return fail(BCMPC_ERR_UNSUPPORTED, "CEM runs on group-kernel engines without a policy");
        a.cem_mu = cem->mu;
        a.cem_sigma = cem->sigma;
        a.cem_iter = cem->iter;
    }
    ArgminArgs m{};
    if (d_result) m = argmin_args(e, d_costs, d_actions, act_out_all, seed, cand_offset, d_result, cem);
    // BCMPC_FUSED_ARGMIN=1: the split kernel reduces np.argmin in its own tail (one launch per
    // get_action).  Off by default: the tail's ticket + acquire cost ~6 us in-kernel, as much as the
    // two argmin launches it replaces, and p50 did not move (cfg1/cfg2/run.sh recipe)
    // The team kernel (small K: a few dozen workgroups) reduces it in its tail by default (round 3; one
    // launch per control step instead of two; BCMPC_TEAM_FUSED_ARGMIN=0 restores the argmin launch)
    const char* fa = std::getenv("BCMPC_FUSED_ARGMIN");
    static const bool team_fused = [] {
        const char* v = std::getenv("BCMPC_TEAM_FUSED_ARGMIN");
        return !(v && v[0] == '0');
    }();
    const bool fused = d_result && !cem && !terms && !value &&
                       (e->kernel == BCMPC_KERNEL_TEAM ? team_fused
                                                       : e->split && fa && fa[0] == '1');
    if (fused) {
        a.fused_argmin = 1;
        a.amin = m;
        a.amin_ticket = e->d_amin_ticket;
    }
    const bool record_events = r.record_events && e->timing;
    e->timed = false;
    if (record_events) HIP_TRY(hipEventRecord(e->ev[0], st));
    bool team_skipped = false;
    if (e->kernel == BCMPC_KERNEL_TEAM) {
        a.team_buf = e->d_team;
        a.team_ctl = e->d_team_ctl;
        a.team_err = e->d_team_err;
        a.rows_flag = e->rows_wait_seq ? e->d_rows_seq : nullptr;
        a.rows_seq = e->rows_wait_seq;
        e->rows_wait_seq = 0;
        // BCMPC_TEAM_SPINS (tests): exchange polls before a member gives up; -1: the launch is skipped and
        // reported as a team that gave up (forces the fallback path deterministically)
        const char* sv = std::getenv("BCMPC_TEAM_SPINS");
        if (sv && *sv) announce_test_hook("BCMPC_TEAM_SPINS", sv);
        a.team_spins = sv && *sv ? std::max(-1, std::atoi(sv)) : 0;
        if (const int rc = team_order_before(c.device, st, e->stream)) return rc;
        // (TEAM_STAMP variant builds)
        static const char* const names[10] = {"tail", "fill", "l0in", "layer0", "slabbar", "l1mm", "l1epi", "out+bar",
                                              "xchg", "prologue"};
        StampRun stamps;
        if (const int rc = stamps.begin((size_t)team_blocks(c.num_paths, e->HP, e->team_kind),
                                        (size_t)(e->HP / 16 / team_layer0_tiles(e->HP, e->team_kind)), st))
            return rc;
        a.stamps = stamps.d;
        if (a.team_spins < 0) {
            __atomic_store_n(e->h_team_err, 1u, __ATOMIC_RELEASE);
            team_skipped = true;                      // (no tail ran: the argmin launch raises the done word)
        } else {
            HIP_TRY(launch_rollout_team(a, e->HP, st));
        }
        if (!e->sync_call)
            if (const int rc = team_order_after(c.device, st)) return rc;
        if (const int rc = stamps.print(names, true, c, st)) return rc;
    } else if (e->split) {
        const bool pp3 = e->pp3 && !terms && x3_pp3_args_ok(a, e->HP);
        const int cpb = pp3 ? 128 : 16 * e->nc;           // candidates per workgroup
        // (X3_STAMP variant builds)
        static const char* const names_x3[10] = {"owner", "input", "B1", "layer0", "slab", "mm", "epi", "out", "B3B4", "-"};
        static const char* const names_pp3[10] = {"EC:tanh+out", "EC:wait", "EC:owner", "EC:layer0", "M:slab+wait", "M:mm",
                                                  "-", "barrier", "-", "-"};
        StampRun stamps;
        if (const int rc = stamps.begin((size_t)((c.num_paths + cpb - 1) / cpb), (size_t)e->nw, st)) return rc;
        a.stamps = stamps.d;
        HIP_TRY(e->f16 ? launch_rollout_x3_f16(a, e->HP, e->nc, st)
                : pp3  ? launch_rollout_pp3(a, e->HP, st)
                       : launch_rollout_x3(a, e->HP, e->nc, st));
        if (const int rc = stamps.print(pp3 ? names_pp3 : names_x3, false, c, st)) return rc;
    } else if (e->kernel == BCMPC_KERNEL_SOLO) {
        HIP_TRY(launch_rollout(a, e->HP, e->wpb, st));
    } else {
        HIP_TRY(launch_rollout_grp(a, e->HP, e->nw, st));
    }
    if (terms)
        if (const int rc = term_cost_launch(e, d_traj, d_actions, seed, cand_offset, cem ? cem->mu : nullptr,
                                            cem ? cem->sigma : nullptr, cem ? cem->iter : 0, c.num_paths, d_costs,
                                            d_steps, st, &cost_in))
            return rc;
    if (value)
        if (const int rc = terminal_value_launch(e, d_traj + (size_t)c.horizon * (size_t)c.num_paths * c.state_dim,
                                                 c.state_dim, c.num_paths, e->d_vvalues, d_costs, d_steps, c.horizon,
                                                 st))
            return rc;
    if (record_events) HIP_TRY(hipEventRecord(e->ev[1], st));
    if (d_result && (!fused || team_skipped)) HIP_TRY(launch_argmin(m, st));
    if (d_result && e->comm && !cem) {
        // the one collective of a sharded control step: every rank's record, then np.argmin's rule
        std::string err;
        if (const int xr = comm_exchange(e->comm, d_result, c.cost == BCMPC_COST_REWARD, st, &err,
                                         e->kernel == BCMPC_KERNEL_TEAM ? e->d_team_err : nullptr))
            return fail(xr, err);
    }
    if (record_events) HIP_TRY(hipEventRecord(e->ev[2], st));
    e->timed = record_events && d_result != nullptr;
    return BCMPC_OK;
}

// ---- batched control step: n_envs environments x K candidates per launch chain --------------
// Column c = b * K + j of the engine's num_paths candidates belongs to environment b.  The states are
// expanded to the candidates by a kernel of their own (batch.hip tile_states), so that the rollout
// kernels run exactly as for bcmpc_rollout_async with per-candidate states; argmin_segments then
// reduces each environment's K costs to its record.
int batch_check(const bcmpc_engine* e, int32_t n_envs) {
    const bcmpc_config& c = e->cfg;
    if (c.cost == BCMPC_COST_NONE)
        return fail(BCMPC_ERR_ARG, "the batched step needs a fused objective (cheetah cost or learned reward)");
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (c.num_paths % n_envs != 0)
        return fail(BCMPC_ERR_ARG, "num_paths (" + std::to_string(c.num_paths) + ") is not a multiple of n_envs (" +
                                       std::to_string(n_envs) + ")");
    if (e->PL > 0) return fail(BCMPC_ERR_UNSUPPORTED, "the batched step does not cover engines with a fused policy yet");
    if (e->comm)
        return fail(BCMPC_ERR_UNSUPPORTED, "the batched step does not cover engines with a communicator attached yet");
    if (!e->has_weights) return fail(BCMPC_ERR_STATE, "bcmpc_set_weights has not been called");
    if (c.num_paths == 0) return fail(BCMPC_ERR_EMPTY, "attempt to get argmin of an empty sequence");
    return BCMPC_OK;
}

// the synchronous batched calls' buffers, grown on demand: the environments' states and records ...
int batch_buffers(bcmpc_engine* e, int32_t n_envs) {
    if (n_envs <= e->batch_cap) return BCMPC_OK;
    for (void* p : {(void*)e->d_bstates, (void*)e->d_bresults})
        if (p) (void)hipFree(p);
    if (e->h_bresults) (void)hipHostFree(e->h_bresults);
    e->d_bstates = nullptr; e->d_bresults = nullptr; e->h_bresults = nullptr;
    e->batch_cap = 0;
    HIP_TRY(hipMalloc(&e->d_bstates, (size_t)n_envs * e->cfg.state_dim * sizeof(double)));
    HIP_TRY(hipMalloc(&e->d_bresults, (size_t)n_envs * sizeof(bcmpc_result)));
    HIP_TRY(hipHostMalloc(&e->h_bresults, (size_t)n_envs * sizeof(bcmpc_result), hipHostMallocDefault));
    e->batch_cap = n_envs;
    return BCMPC_OK;
}

// ... and the explicit action array d_actions [H][num_paths][A]
int actions_buffer(bcmpc_engine* e) {
    const size_t n = (size_t)e->cfg.horizon * (size_t)e->cfg.num_paths * (size_t)e->cfg.action_dim;
    if (n <= e->actions_cap) return BCMPC_OK;
    if (e->d_actions) (void)hipFree(e->d_actions);
    e->d_actions = nullptr;
    e->actions_cap = 0;
    HIP_TRY(hipMalloc(&e->d_actions, n * sizeof(double)));
    e->actions_cap = n;
    return BCMPC_OK;
}

// a synchronous call's explicit actions, uploaded into it on st: *d_act is what the launch reads (none: nullptr)
int upload_actions(bcmpc_engine* e, const double* actions, hipStream_t st, const double** d_act) {
    *d_act = nullptr;
    if (!actions) return BCMPC_OK;
    if (const int rc = actions_buffer(e)) return rc;
    const size_t n = (size_t)e->cfg.horizon * (size_t)e->cfg.num_paths * (size_t)e->cfg.action_dim;
    HIP_TRY(hipMemcpyAsync(e->d_actions, actions, n * sizeof(double), hipMemcpyHostToDevice, st));
    *d_act = e->d_actions;
    return BCMPC_OK;
}

// tile_states -> rollout (per-candidate states, no argmin) -> argmin_segments, all on st
static int batch_impl(bcmpc_engine* e, const double* d_states, int32_t n_envs, const double* d_actions,
                      uint64_t seed, int64_t cand_offset, double* d_costs, bcmpc_result* d_results,
                      hipStream_t st) {
    const bcmpc_config& c = e->cfg;
    if (!e->d_tiled) HIP_TRY(hipMalloc(&e->d_tiled, (size_t)c.num_paths * c.state_dim * sizeof(double)));
    const int64_t K = c.num_paths / n_envs;
    const bool timing = e->timing;
    if (timing) HIP_TRY(hipEventRecord(e->ev[0], st));
    TileStatesArgs t{};
    t.states = d_states; t.out = e->d_tiled; t.K = K; t.Ktot = c.num_paths; t.S = c.state_dim;
    HIP_TRY(launch_tile_states(t, st));
    RolloutLaunch r;
    r.state = e->d_tiled; r.state_stride = c.state_dim; r.actions = d_actions; r.seed = seed; r.cand_offset = cand_offset;
    r.costs = d_costs; r.stream = st; r.record_events = false; r.n_envs = n_envs;
    if (const int rc = rollout_impl(e, r)) return rc;
    if (timing) HIP_TRY(hipEventRecord(e->ev[1], st));
    SegmentArgminArgs m{};
    m.costs = d_costs; m.actions = d_actions; m.consts = e->d_consts; m.out = d_results;
    m.seed = seed; m.cand_offset = cand_offset; m.K = K; m.n_envs = n_envs; m.A = c.action_dim;
    m.maximize = c.cost == BCMPC_COST_REWARD;
    HIP_TRY(launch_argmin_segments(m, st));
    if (timing) HIP_TRY(hipEventRecord(e->ev[2], st));
    e->timed = timing;                                 // (bcmpc_last_kernel_ms: tile + rollout | argmin)
    return BCMPC_OK;
}

}  // namespace bcmpc::host

extern "C" {

int bcmpc_rollout_async(bcmpc_engine* e, const double* d_state, int64_t state_stride, const double* d_actions,
                        uint64_t seed, int64_t cand_offset, double* d_costs, double* d_traj,
                        bcmpc_result* d_result, void* stream) {
    if (!e || !d_state) return fail(BCMPC_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(e->cfg.device));
    // `stream` is used verbatim: NULL is HIP's null stream (bcmpc_stream() gives the engine's own)
    RolloutLaunch r;
    r.state = d_state; r.state_stride = state_stride; r.actions = d_actions; r.seed = seed; r.cand_offset = cand_offset;
    r.costs = d_costs; r.traj = d_traj; r.result = d_result; r.stream = (hipStream_t)stream;
    return rollout_impl(e, r);
}

int bcmpc_rollout_policy_async(bcmpc_engine* e, const double* d_state, const double* d_actions, uint64_t seed,
                               int64_t cand_offset, double* d_costs, double* d_traj, double* d_actions_out,
                               bcmpc_result* d_result, void* stream) {
    if (!e || !d_state || !d_actions_out) return fail(BCMPC_ERR_ARG, "null argument");
    if (e->PL == 0) return fail(BCMPC_ERR_STATE, "engine was created without a policy (config.policy_hidden == 0)");
    HIP_TRY(hipSetDevice(e->cfg.device));
    RolloutLaunch r;
    r.state = d_state; r.actions = d_actions; r.seed = seed; r.cand_offset = cand_offset;
    r.costs = d_costs; r.traj = d_traj; r.result = d_result; r.stream = (hipStream_t)stream;
    r.act_out_all = d_actions_out;
    return rollout_impl(e, r);
}

// ... with one start state per environment: tile_states, then the same launch with per-candidate states
int bcmpc_rollout_policy_batch_async(bcmpc_engine* e, const double* d_states, int32_t n_envs, const double* d_actions,
                                     uint64_t seed, int64_t cand_offset, double* d_costs, double* d_traj,
                                     double* d_actions_out, void* stream) {
    // (arguments first: a bad call is answered before any HIP call)
    if (!e || !d_states || !d_actions_out) return fail(BCMPC_ERR_ARG, "null argument");
    if (e->PL == 0) return fail(BCMPC_ERR_STATE, "engine was created without a policy (config.policy_hidden == 0)");
    const bcmpc_config& c = e->cfg;
    if (n_envs < 1) return fail(BCMPC_ERR_ARG, "n_envs must be >= 1");
    if (c.num_paths == 0) return fail(BCMPC_ERR_EMPTY, "attempt to get argmin of an empty sequence");
    if (c.num_paths % n_envs != 0)
        return fail(BCMPC_ERR_ARG, "num_paths (" + std::to_string(c.num_paths) + ") is not a multiple of n_envs (" +
                                       std::to_string(n_envs) + ")");
    HIP_TRY(hipSetDevice(c.device));
    const hipStream_t st = (hipStream_t)stream;
    if (!e->d_tiled) HIP_TRY(hipMalloc(&e->d_tiled, (size_t)c.num_paths * c.state_dim * sizeof(double)));
    TileStatesArgs t{};
    t.states = d_states; t.out = e->d_tiled; t.K = c.num_paths / n_envs; t.Ktot = c.num_paths; t.S = c.state_dim;
    HIP_TRY(launch_tile_states(t, st));
    RolloutLaunch r;
    r.state = e->d_tiled; r.state_stride = c.state_dim; r.actions = d_actions; r.seed = seed; r.cand_offset = cand_offset;
    r.costs = d_costs; r.traj = d_traj; r.stream = st; r.n_envs = n_envs;
    r.act_out_all = d_actions_out;
    return rollout_impl(e, r);
}

int bcmpc_get_action(bcmpc_engine* e, const double* state, const double* actions, uint64_t seed,
                     int64_t cand_offset, bcmpc_result* out, double* costs_out) {
    if (!e || !state || !out) return fail(BCMPC_ERR_ARG, "null argument");
    const bcmpc_config& c = e->cfg;
    if (c.cost == BCMPC_COST_NONE) return fail(BCMPC_ERR_ARG, "get_action needs a fused objective (cheetah cost or learned reward)");
    HIP_TRY(hipSetDevice(c.device));
    const SyncCall sync_guard(e);
    // one launch chain per control step: the state travels in the kernel arguments and the argmin
    // writes the result record straight into mapped host memory (a communicator all-gathers the
    // device record instead)
    const bool lean = e->comm == nullptr;
    if (!lean) HIP_TRY(hipMemcpyAsync(e->d_state, state, sizeof(double) * c.state_dim, hipMemcpyHostToDevice, e->stream));
    const double* d_act = nullptr;
    if (const int rc = upload_actions(e, actions, e->stream, &d_act)) return rc;
    e->want_done = lean && !costs_out;
    RolloutLaunch r;
    if (lean) r.state_inline = state; else r.state = e->d_state;
    r.actions = d_act; r.seed = seed; r.cand_offset = cand_offset; r.costs = e->d_costs;
    r.result = lean ? e->d_result_map : e->d_result; r.stream = e->stream;
    const int rc = rollout_impl(e, r);
    const bool spin = e->want_done;
    e->want_done = false;
    if (rc != BCMPC_OK) return rc;
    if (!lean) HIP_TRY(hipMemcpyAsync(e->h_result, e->d_result, sizeof(bcmpc_result), hipMemcpyDeviceToHost, e->stream));
    if (costs_out)
        HIP_TRY(hipMemcpyAsync(costs_out, e->d_costs, sizeof(double) * c.num_paths, hipMemcpyDeviceToHost, e->stream));
    if (spin) {
        if (const int wr = wait_done(e, e->seq)) return wr;
    } else {
        if (const int sr = sync_step(e, e->stream)) return sr;
    }
    if (step_failed(e)) {
        bcmpc_engine* re = nullptr;
        if (const int fr = rerun_engine(e, &re)) return fr;
        return bcmpc_get_action(re, state, actions, seed, cand_offset, out, costs_out);
    }
    *out = lean ? *e->h_result_map : *e->h_result;
    return BCMPC_OK;
}

int bcmpc_rollout_batch_async(bcmpc_engine* e, const double* d_states, int32_t n_envs, const double* d_actions,
                              uint64_t seed, int64_t cand_offset, double* d_costs, bcmpc_result* d_results,
                              void* stream) {
    if (!e || !d_states || !d_costs || !d_results) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = batch_check(e, n_envs)) return rc;
    HIP_TRY(hipSetDevice(e->cfg.device));
    return batch_impl(e, d_states, n_envs, d_actions, seed, cand_offset, d_costs, d_results, (hipStream_t)stream);
}

int bcmpc_get_actions_batch(bcmpc_engine* e, const double* states, int32_t n_envs, const double* actions,
                            uint64_t seed, int64_t cand_offset, bcmpc_result* out, double* costs_out) {
    if (!e || !states || !out) return fail(BCMPC_ERR_ARG, "null argument");
    if (const int rc = batch_check(e, n_envs)) return rc;
    const bcmpc_config& c = e->cfg;
    HIP_TRY(hipSetDevice(c.device));
    const SyncCall sync_guard(e);
    if (const int rc = batch_buffers(e, n_envs)) return rc;
    hipStream_t st = e->stream;
    HIP_TRY(hipMemcpyAsync(e->d_bstates, states, sizeof(double) * (size_t)n_envs * c.state_dim, hipMemcpyHostToDevice, st));
    const double* d_act = nullptr;
    if (const int rc = upload_actions(e, actions, st, &d_act)) return rc;
    if (const int rc = batch_impl(e, e->d_bstates, n_envs, d_act, seed, cand_offset, e->d_costs, e->d_bresults, st))
        return rc;
    HIP_TRY(hipMemcpyAsync(e->h_bresults, e->d_bresults, (size_t)n_envs * sizeof(bcmpc_result), hipMemcpyDeviceToHost, st));
    if (costs_out)
        HIP_TRY(hipMemcpyAsync(costs_out, e->d_costs, sizeof(double) * c.num_paths, hipMemcpyDeviceToHost, st));
    if (const int sr = sync_step(e, st)) return sr;
    if (step_failed(e)) {                              // the team gave up: the whole batch on the fallback engine
        bcmpc_engine* re = nullptr;
        if (const int fr = rerun_engine(e, &re)) return fr;
        return bcmpc_get_actions_batch(re, states, n_envs, actions, seed, cand_offset, out, costs_out);
    }
    std::memcpy(out, e->h_bresults, (size_t)n_envs * sizeof(bcmpc_result));
    return BCMPC_OK;
}

int bcmpc_engine_set_comm(bcmpc_engine* e, bcmpc_comm* comm) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    if (comm && comm_device(comm) != e->cfg.device)
        return fail(BCMPC_ERR_ARG, "the communicator was created for another device");
    if (comm && e->cfg.cost == BCMPC_COST_NONE)
        return fail(BCMPC_ERR_ARG, "the exchange needs the fused objective (argmin records)");
    if (comm && e->cfg.cost == BCMPC_COST_TERMS)
        return fail(BCMPC_ERR_UNSUPPORTED, "cost-term engines do not exchange records inside the library yet");
    if (comm && e->has_value)
        return fail(BCMPC_ERR_UNSUPPORTED, "engines with a terminal value do not exchange records inside the library yet");
    e->comm = comm;
    return BCMPC_OK;
}

int bcmpc_engine_status(bcmpc_engine* e) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    if (team_failed(e))
        return fail(BCMPC_ERR_HIP, "team kernel: a workgroup team did not meet (its grid was not resident -- "
                                   "another kernel holding the CUs?)");
    return BCMPC_OK;
}

int bcmpc_engine_team_reruns(const bcmpc_engine* e, uint64_t* reruns) {
    if (!e || !reruns) return fail(BCMPC_ERR_ARG, "null argument");
    *reruns = e->team_reruns;
    return BCMPC_OK;
}

int bcmpc_engine_set_timing(bcmpc_engine* e, int32_t on) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    e->timing = on != 0;
    return BCMPC_OK;
}

int bcmpc_last_kernel_ms(bcmpc_engine* e, float* rollout_ms, float* argmin_ms) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    if (!e->timed) return fail(BCMPC_ERR_ARG, "the last launch was not timed (bcmpc_engine_set_timing(eng, 1) first)");
    float r = 0.f, m = 0.f;
    HIP_TRY(hipEventSynchronize(e->ev[2]));
    HIP_TRY(hipEventElapsedTime(&r, e->ev[0], e->ev[1]));
    HIP_TRY(hipEventElapsedTime(&m, e->ev[1], e->ev[2]));
    if (rollout_ms) *rollout_ms = r;
    if (argmin_ms) *argmin_ms = m;
    return BCMPC_OK;
}

int bcmpc_engine_layout(const bcmpc_engine* e, char* buf, int32_t cap) {
    if (!e || !buf || cap <= 0) return fail(BCMPC_ERR_ARG, "null argument");
    const char* prec = e->f16 ? "f16" : e->split ? "split" : "fp32";
    char s[160];
    switch (e->kernel) {
        case BCMPC_KERNEL_SOLO: std::snprintf(s, sizeof(s), "rollout_fp32<%d> fp32", e->HP); break;
        case BCMPC_KERNEL_GROUP4:
        case BCMPC_KERNEL_GROUP8: std::snprintf(s, sizeof(s), "rollout_grp<%d,NW=%d> fp32", e->HP, e->nw); break;
        case BCMPC_KERNEL_TEAM:
            std::snprintf(s, sizeof(s), "rollout_team<%d,kind=%d%s> split", e->HP, e->team_kind,
                          e->team_defer ? ",deferLN" : "");
            break;
        default:
            if (e->pp)
                std::snprintf(s, sizeof(s), "rollout_pp<%d%s> %s", e->HP, e->pp_fold_w ? ",fold" : "", prec);
            else if (e->pp3)
                std::snprintf(s, sizeof(s), "rollout_pp3<%d> %s", e->HP, prec);
            else
                std::snprintf(s, sizeof(s), "rollout_x3<%d,NC=%d,NW=%d> %s", e->HP, e->nc, e->nw, prec);
    }
    std::snprintf(buf, (size_t)cap, "%s%s%s%s", s, e->cfg.cost == BCMPC_COST_TERMS ? "+terms" : "",
                  e->has_value ? "+value" : "", e->cost.conds.empty() ? "" : "+done");
    return BCMPC_OK;
}

int64_t bcmpc_split_pp_lds_bytes(int32_t hidden, int32_t n_layers, int32_t state_dim, int32_t action_dim) {
    if (hidden < 1 || hidden > 1024) return -1;
    const int hp = padded_hidden(hidden);
    return x3_pp3_ok(hp, n_layers, state_dim, action_dim) ? (int64_t)x3_pp3_lds(hp, state_dim, action_dim) : -1;
}

int bcmpc_engine_info(const bcmpc_engine* e, int32_t* hidden_padded, int64_t* packed_weight_bytes,
                      int32_t* waves_per_block, int32_t* kernel) {
    if (!e) return fail(BCMPC_ERR_ARG, "null argument");
    if (hidden_padded) *hidden_padded = e->HP;
    if (packed_weight_bytes) *packed_weight_bytes = (int64_t)(e->w_floats * sizeof(float));
    if (waves_per_block) *waves_per_block = e->kernel == BCMPC_KERNEL_SOLO ? e->wpb : e->nw;
    if (kernel) *kernel = e->kernel;
    return BCMPC_OK;
}

}  // extern "C"

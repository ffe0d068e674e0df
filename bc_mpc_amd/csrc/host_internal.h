// host_internal.h -- what the HIP-calling host units of libbcmpc (capi.cpp, mt_draw.cpp, planners.cpp) share: the
// engine, the error channel, the launch helpers more than one of them calls.  Not installed; the C ABI is include/bcmpc.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/bcmpc.h"
#include "kernels.h"
#include "mt19937.h"
#include "pack.h"

using namespace bcmpc;

struct bcmpc_engine : bcmpc::host::EnginePlan {   // (the plan: config, kernel, packed layout -- engine_plan.h)
    explicit bcmpc_engine(const bcmpc::host::EnginePlan& plan) : EnginePlan(plan) {}
    // what the last bcmpc_set_weights / bcmpc_set_policy left besides the buffers (pack.h PackedNet / PackedPolicy)
    bool pp_fold_w = false;            // rollout_pp's folded operands are active for the current weights
    float winv[BCMPC_MAX_LAYERS + 1]{};  // split kernel: 1 / operand scales per layer
    float pwinv[BCMPC_MAX_LAYERS + 1]{}; // ... and per fused-policy layer
    float hsc[BCMPC_MAX_LAYERS]{};       // split LN nets: output scale of hidden layer l
    hipStream_t stream = nullptr;
    // device buffers
    float* d_w = nullptr;   // [w_floats]
    float* d_b = nullptr;   // [b_floats]
    float* d_ln = nullptr;  // [2][L][HP]
    double* d_consts = nullptr;
    double* d_state = nullptr;
    double* d_actions = nullptr; size_t actions_cap = 0;
    double* h_stage = nullptr; size_t stage_cap = 0;   // pinned [H, K, A] staging (bcmpc_get_action_mt19937)
    // small NumPy-stream draws: two fine-grained (coherent) pinned row buffers and their device addresses
    // (the kernel reads them over the bus); a call uses one while the pre-draw worker fills the other
    double* h_zc[2] = {nullptr, nullptr}; size_t zc_cap = 0;
    double* d_zc[2] = {nullptr, nullptr};
    // late pre-draw hit (team kernel): the worker publishes each job's sequence number into this mapped
    // host word after its last row; a call that finds its rows still being drawn launches at once and the
    // kernel waits for the word (BCMPC_MT_PREDRAW_LATE=0: the call waits on the host instead)
    uint32_t* h_rows_seq = nullptr;
    uint32_t* d_rows_seq = nullptr;
    uint32_t rows_wait_seq = 0;         // (the next team launch waits for this sequence number; 0: none)
    // the pre-draw worker also copies its rows into device memory (copy stream + event per buffer) while the
    // caller's env step runs; a call whose copy has completed reads HBM instead of the bus (zero-copy rows
    // cost the K = 400 kernel 3.7 us; BCMPC_MT_PREDRAW_DEV=0 turns the copy off)
    double* d_rows[2] = {nullptr, nullptr};
    hipStream_t copy_st = nullptr;
    hipEvent_t copy_ev[2] = {nullptr, nullptr};
    bool copy_valid[2] = {false, false};
    int zc_last = 0;                    // the buffer the last successful call read
    // pre-draw (BCMPC_MT_PREDRAW, default on): after a successful small draw, a worker thread draws the
    // rows the NEXT call would draw -- from NumPy's advanced state, same bounds / shard -- into the other
    // buffer; the next call uses them only if NumPy's state is still exactly that state
    struct PreDraw {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        bool quit = false, pending = false, busy = false, ready = false;
        // lock-free mirrors for the spinning handshake: a job posted and not yet finished / shutting down
        std::atomic<bool> inflight{false}, quit_a{false};
        std::atomic<bool> claimed{false};   // a call already reads this job's pinned rows: no device copy
        uint32_t job = 0;                   // the posted job's sequence number (published to h_rows_seq)
        bool rows = true;               // false: only NumPy's state is needed (the stochastic policy)
        Mt19937 from, to;               // the state the rows were drawn from / leave behind
        std::vector<double> low, high;
        int64_t kg = 0, off = 0;
        int buf = 0;
        uint64_t hits = 0, late = 0, misses = 0;   // hits include the late ones
    } pre;
    double* d_costs = nullptr;
    bcmpc_result* d_result = nullptr;
    double* d_amin_c = nullptr;         // argmin scratch: per-block best
    int64_t* d_amin_i = nullptr;
    size_t amin_cap = 0;                // records the scratch holds
    unsigned* d_amin_ticket = nullptr;  // fused argmin (split kernel): last-workgroup ticket
    // batched control step (bcmpc_get_actions_batch / bcmpc_rollout_batch_async), allocated on first use
    double* d_tiled = nullptr;          // [num_paths][S] the environments' states expanded to the candidates
    double* d_bstates = nullptr;        // [batch_cap][S] the environments' states (synchronous call)
    bcmpc_result* d_bresults = nullptr; // [batch_cap] records
    bcmpc_result* h_bresults = nullptr; // pinned mirror
    int32_t batch_cap = 0;              // environments d_bstates / d_bresults / h_bresults hold
    // batched CEM / MPPI (bcmpc_cem_get_actions_batch / bcmpc_mppi_get_actions_batch, plan_batch.hip)
    double* d_bmu = nullptr;            // [plan_cap][H][A] the environments' plans
    double* d_bsigma = nullptr;
    int32_t* d_bcount = nullptr;        // [plan_cap] elites selected
    bcmpc_mppi_stats* d_bstats = nullptr;   // [plan_cap]
    int32_t plan_cap = 0;
    bcmpc_elite* d_belite = nullptr; size_t belite_cap = 0;   // [n_envs][n_elite] records
    // CEM elite carry-over (plan_noise.hip): the elites' sequences [n_envs][n_elite][H][A] and their counts
    double* d_keep = nullptr; size_t keep_cap = 0;
    int32_t* d_keep_count = nullptr; int32_t keep_count_cap = 0;
    // proposals (plan_prop.hip): a synchronous call's host sequences [n_envs][P][H][A], uploaded with the plans
    double* d_prop = nullptr; size_t prop_cap = 0;
    // knot plans (plan_knots.hip): a synchronous call's clipped knot values [M][num_paths][A]; it only grows
    double* d_knots = nullptr; size_t knots_cap = 0;
    // policy engines' batched rollout (bcmpc_rollout_policy_batch_async) tiles its states into d_tiled, above
    // team kernel (rollout_team.hip): exchange granules, {ticket, generation}, mapped timeout flag
    unsigned long long* d_team = nullptr;
    bool team_defer = false;            // the weights are packed for rollout_team's deferred last LayerNorm
    unsigned* d_team_ctl = nullptr;
    unsigned* h_team_err = nullptr;
    unsigned* d_team_err = nullptr;
    bcmpc_result* h_result = nullptr;   // pinned
    // the synchronous control steps' result: pinned, mapped, coherent host memory the argmin kernel
    // writes directly (no device-to-host copy; the stream synchronisation orders it)
    bcmpc_result* h_result_map = nullptr;
    bcmpc_result* d_result_map = nullptr;
    // ... and its completion word (argmin_write raises seq; wait_done spins on it)
    unsigned long long* h_done = nullptr;
    unsigned long long* d_done = nullptr;
    unsigned long long seq = 0;
    bool want_done = false;             // the next rollout_impl's argmin raises the done word
    double h_consts[kConstRows * kConstCols]{};
    uint64_t version = 0;
    bool has_weights = false;
    hipEvent_t ev[3]{};
    bool timed = false;                 // the last launch chain recorded ev[0..2]
    bool timing = false;                // bcmpc_engine_set_timing: bracket launches with HIP events
    // fused policy (MPCcontrollerPolicyNet)
    float* d_pw = nullptr;                          // [pw_floats]
    float* d_pb = nullptr;                          // [PL][PHP] + kPolParams
    double* d_first = nullptr;                      // [K][A] step-0 actions
    // learned reward (NNDynamicsRewardModel)
    double* d_gpow = nullptr;                       // [H] gamma**h
    double mean_reward = 0.0, std_reward = 0.0;
    // CEM (bcmpc_cem_get_action)
    double* d_mu = nullptr;                         // [H][A] each
    double* d_sigma = nullptr;
    bcmpc_elite* d_elite = nullptr; int32_t elite_cap = 0;
    int32_t* d_count = nullptr;
    // MPPI (bcmpc_mppi_get_action / bcmpc_mppi_update_async): the update's scratch -- [256] minima,
    // [256] counts, [H * A + 2][partials] -- grown on demand, and the synchronous call's statistics
    double* d_mppi = nullptr; size_t mppi_cap = 0;
    bcmpc_mppi_stats* d_mppi_stats = nullptr;
    // ... and the control-cost term's augmented scores [num_paths] (bcmpc_mppi_get_action_x, mppi_ext.hip)
    double* d_mppi_scores = nullptr; size_t mppi_scores_cap = 0;
    double explore = 0.0;
    uint64_t pol_version = 0;
    bool has_policy = false;
    // NumPy-stream draw on the device (bcmpc_get_action_mt19937, mt_device.hip): chunk plan and jump
    // polynomials per (k_global, cand_offset), built on the first call of that shape
    int64_t mt_kg = -1, mt_off = -1;
    int32_t mt_nchunks = 0, mt_cj = 0, mt_s = 0;
    uint32_t* d_mt_io = nullptr;        // [0, 625) key + pos in, [640, 1265) final key + pos out
    double* d_mt_bounds = nullptr;      // [2][A] low, high
    uint32_t* d_mt_xs = nullptr;        // [kMtStream]
    uint32_t* d_mt_polys = nullptr;     // [Cj][kMtPolyWords]
    MtChunk* d_mt_chunks = nullptr;
    uint32_t* d_mt_part = nullptr;      // [Cj][S][624]
    uint32_t* h_mt_io = nullptr;        // pinned mirror of d_mt_io (+ bounds at word 1280)
    // speculative device draw (BCMPC_MT_SPECULATE, default on): right behind a device-path call's argmin, the
    // NEXT call's draw is enqueued from this draw's final state -- still on the device, no host round trip --
    // into a slot of its own; the next call uses it when NumPy's state, bounds and shard equal its start
    // (else it is discarded: two misses in a row pause speculation for kSpecPause calls)
    struct Spec {
        uint32_t* d_io = nullptr;       // [0, 625) final key + pos, then [2][A] bounds (f64) from word 640
        uint32_t* h_io = nullptr;       // pinned mirror
        double* d_act = nullptr;        // the shard's [H][K][A] rows
    } spec[2];
    size_t spec_cap = 0;
    bool spec_armed = false;
    int spec_slot = 0, spec_miss_run = 0, spec_pause = 0;
    uint32_t spec_key[624];
    int32_t spec_pos = 0;
    int64_t spec_kg = 0, spec_off = 0;
    double spec_low[BCMPC_MAX_ACTION], spec_high[BCMPC_MAX_ACTION];
    uint64_t spec_hits = 0, spec_misses = 0;
    // slab-kernel engines draw beside the rollout: the speculative draw runs on spec_st, concurrently with
    // this call's rollout (spec_in_ev: this call's draw has left its final state), with scratch of its own;
    // spec_done_ev closes it and every later draw / rollout that touches its slots waits for it
    hipStream_t spec_st = nullptr;
    hipEvent_t spec_in_ev = nullptr, spec_done_ev = nullptr;
    bool spec_side_pending = false;
    int ncu = 0;                        // the device's CUs
    uint32_t* d_spec_xs = nullptr;
    uint32_t* d_spec_part = nullptr;
    bcmpc_comm* comm = nullptr;         // attached communicator: results exchanged after every argmin
    // BCMPC_COST_TERMS (term_cost.hip): the lists the setters stored and the launch template digested from them
    // (cost_terms.h), and the trajectory scratch [H+1][num_paths][S] the rollout writes when the caller passes no
    // d_traj -- allocated at create, never inside a stream-ordered entry (a captured graph keeps the address)
    bcmpc::host::CostState cost;
    double* d_tc_traj = nullptr;
    // termination (bcmpc_set_termination): the launch chains' termination steps [num_paths], allocated by the
    // setter (a captured graph keeps the address).  steps_on_fb: the last synchronous call reran on fb
    int32_t* d_tc_steps = nullptr;
    bool steps_on_fb = false;
    // reference tracking (bcmpc_set_cost_inputs): device buffers that the setter allocates (they only grow) and
    // fills, with host copies for the fallback engine
    double *d_tc_ref = nullptr, *d_tc_prev = nullptr;
    size_t tc_ref_cap = 0, tc_prev_cap = 0;             // in doubles
    std::vector<double> h_in_ref, h_in_prev;
    // terminal value (terminal_value.hip): the launch template bcmpc_set_terminal_value builds.  The packed
    // kernels and the parameter block are allocated once at their largest size (a captured graph keeps the
    // addresses over a change of net); d_tc_traj, above, is allocated on first use for engines without terms
    TerminalValueArgs tv{};
    bool has_value = false;
    uint64_t value_version = 0;
    float* d_vw = nullptr;
    float* d_vparams = nullptr;
    float* d_vvalues = nullptr;         // [num_paths] the last launch chain's values (bcmpc_last_terminal_values)
    bcmpc::host::ValueCopy hv_copy;     // the last net, copied (the fallback engine is set from it)
    // team kernel: a team that could not meet (its workgroups not all resident: another process or
    // kernel holding CUs for ~1 s) makes a synchronous call rerun on this fallback engine -- the same
    // net on the split slab kernel, or the fp32 group kernel where only the team kernel takes the net
    // in split precision -- created on first need and synced from the host copies kept below
    bcmpc_engine* fb = nullptr;
    uint64_t fb_wver = 0, fb_pver = 0;
    bool fb_wset = false, fb_pset = false;
    uint64_t team_reruns = 0;
    bool sync_call = false;             // inside a synchronous entry point (its launches complete before it returns)
    bcmpc::host::WeightsCopy hw_copy;   // the last bcmpc_set_weights / bcmpc_set_policy, copied (team engines)
    bcmpc::host::PolicyCopy hp_copy;
    double gamma = 1.0;
};

// (hidden: no dynamic symbols of the library; calls between the units bind directly, as they did inside one unit)
#pragma GCC visibility push(hidden)
namespace bcmpc::host {

// (fail(code, msg), bcmpc_last_error's text: engine_plan.h; the text itself lives in capi.cpp)

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(BCMPC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct CemLaunch {           // one CEM iteration's sampling distribution + result merge rule
    const double* mu;
    const double* sigma;
    int32_t iter;
    int32_t merge;
    int64_t pos_base;
};

struct SyncCall {                                   // marks a synchronous entry point's launches, on its engine(s)
    bcmpc_engine* const one;
    bcmpc_engine* const* m;   size_t n;
    explicit SyncCall(bcmpc_engine* x) : one(x), m(&one), n(1) { set(true); }
    SyncCall(bcmpc_engine* const* members, size_t count) : one(nullptr), m(members), n(count) { set(true); }
    ~SyncCall() { set(false); }
    void set(bool on) const { for (size_t i = 0; i < n; ++i) m[i]->sync_call = on; }
};

int create_engine(const bcmpc_config* cfg, const CreateOpts& opts, bcmpc_engine** out);

// one rollout launch chain (rollout_impl): a call site names what it sets
struct RolloutLaunch {
    const double* state = nullptr;          // device state: one (stride 0) or one per candidate (stride state_dim)
    int64_t state_stride = 0;
    const double* state_inline = nullptr;   // ... or a host state that travels in the kernel arguments
    const double* actions = nullptr;        // [H][K][A]; none: Philox, the CEM sampler or the policy
    uint64_t seed = 0;
    int64_t cand_offset = 0;
    double *costs = nullptr, *traj = nullptr;   // (cost terms: traj defaults to the engine's scratch)
    bcmpc_result* result = nullptr;         // the argmin's record; none: no argmin
    hipStream_t stream = nullptr;
    const CemLaunch* cem = nullptr;
    bool record_events = true;              // (and bcmpc_engine_set_timing is on)
    int32_t n_envs = 1;                     // environments the candidates belong to (the cost inputs of each)
    double* act_out_all = nullptr;          // policy engines: every step's actions [H][K][A]
};
int rollout_impl(bcmpc_engine* e, const RolloutLaunch& r);
ArgminArgs argmin_args(bcmpc_engine* e, const double* d_costs, const double* d_actions, const double* act_out_all,
                       uint64_t seed, int64_t cand_offset, bcmpc_result* d_result, const CemLaunch* cem);

// the tail of a synchronous call (capi.cpp): completion, the team give-up flag, the engine a rerun runs on
bool team_failed(bcmpc_engine* e);
bool step_failed(bcmpc_engine* e);
int sync_step(bcmpc_engine* e, hipStream_t st);
int wait_done(bcmpc_engine* e, unsigned long long seq);
int team_fallback(bcmpc_engine* e, bool collective = false);
int rerun_engine(bcmpc_engine* e, bcmpc_engine** r);

// buffers grown on demand and the batched step's argument check (capi.cpp)
int actions_buffer(bcmpc_engine* e);
int upload_actions(bcmpc_engine* e, const double* actions, hipStream_t st, const double** d_act);
int batch_buffers(bcmpc_engine* e, int32_t n_envs);
int batch_check(const bcmpc_engine* e, int32_t n_envs);

}  // namespace bcmpc::host
#pragma GCC visibility pop

// kernels.h -- device-side argument blocks and launchers (internal to libbcmpc).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/bcmpc.h"
#include "cost_terms.h"
#include "shapes.h"

namespace bcmpc {

// (the consts block [kConstRows][kConstCols] and the host shape queries of every kernel unit: shapes.h)

struct ArgminArgs {
    const double* costs;
    const double* act_out;   // [.][K][A] actions written by the rollout (policy mode) or nullptr
    const double* actions;   // [H][K][A] or nullptr
    const double* consts;
    bcmpc_result* out;
    uint64_t seed;
    int64_t cand_offset;
    int64_t K;
    int32_t A;
    int32_t maximize;        // np.argmax (learned reward, controllers.py:152) instead of np.argmin
    // CEM: first action regenerated from the sampler; merge with the running best by stream position
    const double* cem_mu;
    const double* cem_sigma;
    int32_t cem_iter;
    int32_t merge;           // keep out's previous best unless strictly better (np.argmin over iterations)
    int64_t pos_base;        // position of candidate 0 in the concatenated stream (iter * K_global + offset)
    double* scratch_c;       // [kArgminParts] per-block best (argmin_partial -> argmin_final)
    int64_t* scratch_i;
    int32_t nparts;          // argmin_parts(K)
    // synchronous control steps: after the record, a system-scope release of seq into this mapped
    // host word (the host spins on it instead of a stream synchronisation), or nullptr
    unsigned long long* done;
    unsigned long long seq;
};
struct RolloutArgs {
    const float __attribute__((ext_vector_type(4)))* w[BCMPC_MAX_LAYERS + 1];  // packed kernels
    int32_t wbytes[BCMPC_MAX_LAYERS + 1];    // packed bytes per layer (buffer num_records)
    const float* b[BCMPC_MAX_LAYERS + 1];    // padded biases
    const float* lng[BCMPC_MAX_LAYERS];      // padded LN gamma (0 on pad lanes)
    const float* lnb[BCMPC_MAX_LAYERS];      // padded LN beta
    const double* consts;
    const double* state;
    int64_t state_stride;                    // 0 (tiled, controllers.py:63) or S (per-candidate)
    int32_t state_inline;                    // 1: the (tiled) state is state_v, carried in the kernel
    double state_v[BCMPC_MAX_STATE];         //    arguments (no host-to-device copy per control step)
    const double* actions;                   // [H][K][A] or nullptr => Philox
    double* costs;                           // [K] or nullptr
    double* traj;                            // [H+1][K][S] or nullptr
    uint64_t seed;
    int64_t cand_offset;
    int64_t K;
    int32_t H, S, A, L, hidden, act, ln, cost;
    // fused policy (MPCcontrollerPolicyNet, controllers.py:189-237); pL == 0: none
    const float __attribute__((ext_vector_type(4)))* pw[BCMPC_MAX_LAYERS + 1];
    int32_t pwbytes[BCMPC_MAX_LAYERS + 1];
    const float* pb[BCMPC_MAX_LAYERS];       // padded hidden biases
    const float* pparams;                    // kPolParams floats: obmean[32] obstd[32] logstd[16] outbias[16]
    int32_t pL, phidden_padded, pol_mode;
    double explore;
    double* act_out;                         // [act_out_steps][K][A] f64 actions actually rolled out, or nullptr
    int32_t act_out_steps;
    // learned-reward net (NNDynamicsRewardModel, dynamics.py:121-238); model == BCMPC_MODEL_REWARD
    int32_t model;
    double mean_reward, std_reward;          // dynamics.py:236 denomalize
    const double* gpow;                      // [H] gamma**h (controllers.py:139)
    // CEM sampling (DESIGN.md "CEM"): actions = clip(mu + sigma * IrwinHall12(seed, g, h, j, iter))
    const double* cem_mu;                    // [H][A] or nullptr
    const double* cem_sigma;                 // [H][A]
    int32_t cem_iter;
    // split kernel (BCMPC_PREC_SPLIT_F16): 1 / (operand scales) of layer l's MFMA result,
    // exact powers of two (layer 0: weight scale only; its input scale is per candidate)
    float winv[BCMPC_MAX_LAYERS + 1];
    float pwinv[BCMPC_MAX_LAYERS + 1];       // the same for the fused policy's layers
    float hsc[BCMPC_MAX_LAYERS];             // split LN nets: power-of-two scale of hidden layer l's output
    int32_t f16_single;                      // BCMPC_PREC_F16: one f16 MFMA pass (hi x hi), no lo operands
    int32_t x3_nw;                           // split kernel: waves per workgroup (0: x3_waves' default)
    int32_t x3_pp;                           // single-pass f16: the two-group pipelined kernel (rollout_pp)
    uint64_t* stamps;                        // diagnostics (X3_STAMP builds): [blocks][NW][10] phase cycles
    // split kernel: np.argmin fused into the launch's tail (fused_argmin != 0): every workgroup
    // leaves its best (cost, index) in amin.scratch_c/i[blockIdx.x], the last to finish (ticket)
    // reduces them and writes amin.out like argmin_final
    int32_t fused_argmin;
    unsigned* amin_ticket;
    ArgminArgs amin;
    // team kernel (rollout_team.hip, T > 1 members per column): exchange granules
    // [columns + 8][2][T][8][64], launch control {ticket, generation}, timeout flag (mapped host word)
    unsigned long long* team_buf;
    unsigned* team_ctl;
    unsigned* team_err;
    int32_t team_spins;                      // exchange polls before a member gives up (0: the default, ~1 s)
    // (team kernel, the drop-in's late pre-draw hit) the actions are host rows that the pre-draw worker is
    // still writing: every workgroup waits until this mapped host word equals rows_seq before its first
    // read of them (nullptr: the rows are complete at launch)
    const uint32_t* rows_flag;
    uint32_t rows_seq;
    // (team kernel, the reward net with LayerNorm heads) [8 members][32 rows]: sum over member t's head
    // rows of the gamma-folded, scaled output weights (the centring correction, rollout_team.hip)
    const float* head_rs;
};

struct SelectArgs {                          // top-E of (cost, index) pairs, NaN last, ties -> lower index
    const bcmpc_elite* pairs;                // [m] pairs (index < 0: empty), or nullptr =>
    const double* costs;                     // [m] costs with index = index_base + i
    int64_t m, index_base;
    int32_t n_elite;
    int32_t maximize;                        // learned reward: the n_elite LARGEST
    bcmpc_elite* out;                        // [n_elite], ascending index, padded with index -1
    int32_t* count;                          // number selected
};

struct RefitArgs {                           // per-(h, j) elite mean / std, smoothed in place
    const bcmpc_elite* elite;
    const int32_t* count;
    double* mu;                              // [H][A]
    double* sigma;
    const double* consts;                    // action bounds (rows 6, 7)
    uint64_t seed;
    int32_t iter, H, A;
    double alpha;
    // (plan_batch.hip) the iteration's materialised actions [H][act_cols][A], column = index - act_g0, read
    // instead of regenerating them; nullptr / outside the array: Philox (the same bits either way)
    const double* actions;
    int64_t act_cols, act_g0;
};
// ---- MPPI plan update (mppi.hip): softmin weights over all m candidates, weighted mean of their actions ----
constexpr int kMppiWaves = 16;               // waves per stage-1 workgroup (they split the (h, j) pairs)
constexpr int kMppiMaxCpl = 4;               // candidates per lane of a stage-1 workgroup: 1, or this beyond
constexpr int64_t kMppiSmall = 16384;        //   kMppiSmall candidates (64 / 256 candidates per workgroup)
constexpr int kMppiMinParts = 256;           // workgroups of the min reduction, at most
struct MppiArgs {
    const double* costs;                     // [m]
    double* mu;                              // [H][A], in / out
    const double* sigma;                     // [H][A]
    const double* consts;                    // action bounds (rows 6, 7)
    double* pmin;                            // [nmin] per-workgroup minimum of the finite scores (+inf: none)
    int64_t* pcnt;                           // [nmin] ... and their count
    double* part;                            // [H * A + 2][nparts]: N[h][j], then W, then sum w^2
    bcmpc_mppi_stats* stats;
    uint64_t seed;
    int64_t m, cand_offset, nparts;
    int32_t iter, H, A, cpl, nmin;
    int32_t maximize;                        // learned reward: the score is -cost
    double lambda;
    const double* actions;                   // (plan_batch.hip) as RefitArgs::actions: column = candidate - act_g0
    int64_t act_cols, act_g0;
};
int mppi_cpl(int64_t m);                     // candidates per lane stage 1 uses for m candidates
int64_t mppi_parts(int64_t m);               // stage-1 workgroups (partials per value)
int mppi_min_blocks(int64_t m);
hipError_t launch_mppi_update(const MppiArgs& a, hipStream_t st);

// ---- NumPy's legacy MT19937 stream drawn on the device (mt_device.hip) ----
// One chunk = a contiguous range of the draw's generator words [s, s + n) (both even: whole
// random_sample doubles), drawn by one workgroup starting from the 624-word window of stream block
// f = floor(s / 624) (block 0 = the caller's key; block 1 = twist(key); block f >= 2 = jump
// polynomial jidx applied to block 1), then written as uniforms to out[out0 ..).  final != 0: the
// chunk ends the draw and leaves NumPy's (key, pos) in MtDrawArgs::final_state.
struct MtChunk {
    int64_t s;        // first draw word (relative to the caller's pos)
    int64_t n;        // words (even)
    int64_t out0;     // output double index of the first double, < 0: not stored
    int32_t f;        // start block
    int32_t jidx;     // jump polynomial (f >= 2), else -1
    int32_t final_;   // 1: write final_state after the last word
    int32_t j0;       // (s / 2) % A: action column of the first double
};
constexpr int kMtN = 624;
constexpr int kMtPolyWords = 624;                // 19937 coefficient bits, padded to 624 u32
constexpr int kMtStream = 32 * kMtPolyWords + 768; // words of the block-1 stream the jumps correlate with
struct MtDrawArgs {
    const uint32_t* in;        // [624] key, [624] = pos (NumPy's get_state()[1], [2])
    const double* bounds;      // [2][A]: low, high (np.random.uniform's low / high as f64)
    uint32_t* xs;              // [kMtStream] scratch: x[0..) = block 1 onwards
    const uint32_t* polys;     // [Cj][kMtPolyWords] x^(624 (f - 1)) mod phi, bit i = coefficient of x^i
    const MtChunk* chunks;     // [nchunks]
    uint32_t* part;            // [Cj][S][624] scratch: partial jumped windows (XOR-combined)
    uint32_t* final_state;     // [625] NumPy's key + pos after the whole draw
    double* out;               // the shard's [H][K][A] action array
    int32_t nchunks, Cj, S, A;
};
hipError_t launch_mt_draw(const MtDrawArgs& a, hipStream_t st);

// ---- library-owned min-loc exchange (comm.hip) ----
int set_error(int code, const std::string& msg);          // bcmpc_last_error() text (capi.cpp)
void announce_test_hook(const char* name, const char* value);   // stderr, once per hook per process (capi.cpp)
int comm_exchange(bcmpc_comm* c, bcmpc_result* d_result, int maximize, hipStream_t st, std::string* err,
                  const unsigned* d_team_err);
bool comm_any_flags(bcmpc_comm* c);
int comm_wait(bcmpc_comm* c, hipStream_t st, int64_t timeout_ms, std::string* err);
int comm_rank(const bcmpc_comm* c);
int comm_size(const bcmpc_comm* c);
int comm_device(const bcmpc_comm* c);

hipError_t launch_rollout(const RolloutArgs& a, int hidden_padded, int waves_per_block, hipStream_t st);
hipError_t launch_rollout_grp(const RolloutArgs& a, int hidden_padded, int nw, hipStream_t st);
// rollout_pp3: the launch arguments it implements (every other launch runs rollout_x3 on the same packed weights)
bool x3_pp3_args_ok(const RolloutArgs& a, int hidden_padded);
hipError_t launch_rollout_pp3(const RolloutArgs& a, int hidden_padded, hipStream_t st);
// (rollout_pp: what launch_rollout_x3_f16 runs when a.x3_pp is set)
hipError_t launch_rollout_pp(const RolloutArgs& a, int hidden_padded, hipStream_t st);
hipError_t launch_rollout_x3(const RolloutArgs& a, int hidden_padded, int nc, hipStream_t st);
hipError_t launch_rollout_x3_f16(const RolloutArgs& a, int hidden_padded, int nc, hipStream_t st);
hipError_t launch_rollout_team(const RolloutArgs& a, int hidden_padded, hipStream_t st);
hipError_t launch_argmin(const ArgminArgs& a, hipStream_t st);
hipError_t launch_select(const SelectArgs& a, hipStream_t st);
hipError_t launch_refit(const RefitArgs& a, hipStream_t st);

// ---- batched control step (batch.hip): n_envs environments x K candidates per launch chain; candidate
// column c = b * K + j belongs to environment b ----
struct TileStatesArgs {                      // out[c][:] = states[c / K][:]
    const double* states;                    // [n_envs][S]
    double* out;                             // [Ktot][S]
    int64_t K, Ktot;
    int32_t S;
};
struct SegmentArgminArgs {                   // one np.argmin record per environment
    const double* costs;                     // [n_envs * K]
    const double* actions;                   // [H][n_envs * K][A] or nullptr => Philox
    const double* consts;
    bcmpc_result* out;                       // [n_envs]
    uint64_t seed;
    int64_t cand_offset;                     // Philox / global index of column 0
    int64_t K;                               // candidates per environment
    int32_t n_envs, A;
    int32_t maximize;                        // np.argmax (learned reward)
};
// ---- declarative cost terms (term_cost.hip; TermCostArgs / TermCostXArgs and the host logic: cost_terms.h) ----
hipError_t launch_term_cost(const TermCostArgs& a, hipStream_t st);      // the plain variant
hipError_t launch_term_cost_x(const TermCostXArgs& a, hipStream_t st);   // lists with reference channels or RATE terms

// ---- model ensembles (ensemble.hip): out[k] = rule over member_costs[0..E-1][k] ----
struct EnsembleReduceArgs {
    const double* member_costs;              // [E][ld], row e = member e's costs
    double* out;                             // [K]
    int64_t ld, K;                           // ld >= K
    int32_t E, mode;                         // 1 <= E <= BCMPC_MAX_MEMBERS; bcmpc_ensemble_mode
    double kappa;                            // MEAN_STD only
};
hipError_t launch_ensemble_reduce(const EnsembleReduceArgs& a, hipStream_t st);

// ---- terminal value (terminal_value.hip): values[k] = V(states[k]), costs[k] += weight * values[k] ----
// (with term_step: the add only for a candidate that never terminated; values[k] is written regardless)
// params: [32] ob_mean, [32] ob_std, [L][HP] hidden biases, [16] final bias (row 0), all zero-padded.
// w[l]: pack.cpp pack_layer(kernel l, Tin, Tout, TB) with Tin = 2 (layer 0) or HP / 16, Tout = HP / 16 and
// TB = min(4, Tout) for the hidden layers, Tout = TB = 1 for the final one.
struct TerminalValueArgs {
    const float __attribute__((ext_vector_type(4)))* w[BCMPC_VALUE_MAX_LAYERS + 1];
    const float* params;
    const double* states;                    // row k: S doubles at states + k * row_stride
    int64_t row_stride, K;
    float* values;                           // [K] or nullptr
    double* costs;                           // [K] in / out, or nullptr
    double weight;
    int32_t S, L, HP;                        // HP: terminal_value_padded(hidden)
    const int32_t* term_step;                // [K] or nullptr: the cost add only where term_step[k] == horizon
    int32_t horizon;
};
hipError_t launch_terminal_value(const TerminalValueArgs& a, hipStream_t st);

hipError_t launch_tile_states(const TileStatesArgs& a, hipStream_t st);
hipError_t launch_argmin_segments(const SegmentArgminArgs& a, hipStream_t st);

// ---- batched CEM / MPPI (plan_batch.hip): one plan, elite set and weighted mean per environment; the
// columns are laid out as above, environment b's arrays follow environment b - 1's ----
struct PlanSampleArgs {                      // out[h][c][j] = cem_action(seed, cand_offset + c, h, j, iter,
    const double* mu;                        //                           mu[c / K][h][j], sigma[c / K][h][j], ..)
    const double* sigma;                     // [n_envs][H][A] each
    const double* consts;
    double* out;                             // [H][Ktot][A]
    uint64_t seed;
    int64_t cand_offset, K, Ktot;
    int32_t iter, H, A;
};
struct PlanArgminArgs {                      // the running best of every environment (ArgminArgs::merge's rule)
    const double* costs;                     // [n_envs * K] this iteration's costs
    const double* actions;                   // [H][n_envs * K][A] this iteration's actions (step 0 is read)
    const double* consts;
    bcmpc_result* out;                       // [n_envs]: best_index = iter * K + j, environment-local
    int64_t K;
    int32_t n_envs, A, iter;
    int32_t merge;                           // keep out[b] unless this iteration's best is strictly better
    int32_t maximize;
};
struct SelectBatchArgs {                     // environment b: SelectArgs{costs + b K, m = K, index_base + b K,
    SelectArgs one;                          //                out + b n_elite, count + b} (one: environment 0's)
    int32_t n_envs;
};
struct RefitBatchArgs {                      // environment b: elite + b n_elite, count + b, mu / sigma + b H A
    RefitArgs one;
    int32_t n_envs, n_elite;
};
struct MppiBatchArgs {                       // environment b: costs + b K, mu / sigma + b H A, stats + b,
    MppiArgs one;                            // cand_offset + b K, pmin / pcnt + b kMppiMinParts,
    int32_t n_envs;                          // part + b (H A + 2) nparts; m = K sets cpl, nparts, nmin
};
size_t mppi_batch_scratch(int64_t K, int32_t n_envs, int32_t HA);   // doubles: [B][256] [B][256] [B][HA + 2][parts]
hipError_t launch_plan_sample(const PlanSampleArgs& a, hipStream_t st);
hipError_t launch_plan_argmin(const PlanArgminArgs& a, hipStream_t st);
hipError_t launch_select_batch(const SelectBatchArgs& a, hipStream_t st);
hipError_t launch_refit_batch(const RefitBatchArgs& a, hipStream_t st);
hipError_t launch_mppi_update_batch(const MppiBatchArgs& a, hipStream_t st);

// ---- correlated sampling noise and the CEM elite carry-over (plan_noise.hip; bc_mpc_amd/sampling.py) ----
struct PlanSampleCorrArgs {                  // PlanSampleArgs with n[h] = rho n[h-1] + c z[h] for cem_normal's z[h]
    const double* mu;
    const double* sigma;                     // [n_envs][H][A] each
    const double* consts;
    double* out;                             // [H][Ktot][A]
    const double* keep;                      // [n_envs][n_elite][H][A] carried sequences, or nullptr: none
    const int32_t* keep_count;               // [n_envs]: environment b's first keep_count[b] columns are copies
    uint64_t seed;
    int64_t cand_offset, K, Ktot;
    int32_t iter, H, A, n_elite;
    double rho, c;                           // c = sqrt(1 - rho^2), rounded once on the host
};
struct PlanKeepArgs {                        // keep[b][e] = the stored sequence of elite[b][e], e < count[b]
    const bcmpc_elite* elite;                // [n_envs][n_elite] (select_batch's output)
    const int32_t* count;                    // [n_envs]
    const double* actions;                   // [H][Ktot][A], column = index - cand_offset
    double* keep;                            // [n_envs][n_elite][H][A]
    int32_t* keep_count;                     // [n_envs]: the leading records that name one of b's own K columns
    int64_t cand_offset, K, Ktot;
    int32_t n_envs, n_elite, H, A;
};
hipError_t launch_plan_sample_corr(const PlanSampleCorrArgs& a, hipStream_t st);
hipError_t launch_plan_keep(const PlanKeepArgs& a, hipStream_t st);

// ---- proposals: given action sequences in every environment's last columns (plan_prop.hip; bc_mpc_amd/proposals.py) ----
struct PlanSamplePropArgs {                  // plan_sample_corr, then column K - n_prop + p of environment b at (h, j) =
    PlanSampleCorrArgs s;                    //   clip(prop[b * env_stride + p * seq_stride + h * step_stride + j])
    const double* prop;                      // the source; read only, strides in doubles
    int64_t env_stride, seq_stride, step_stride;
    int32_t n_prop;                          // 1 <= n_prop <= K
};
hipError_t launch_plan_sample_prop(const PlanSamplePropArgs& a, hipStream_t st);

// ---- knot plans: M <= H sampled knots per column, interpolated to H steps (plan_knots.hip; bc_mpc_amd/knots.py) ----
struct PlanSampleKnotsArgs {                 // s: plan_sample_corr's block with mu / sigma [n_envs][M][A], keep
    PlanSampleCorrArgs s;                    //   [n_envs][n_elite][M][A]; s.H the horizon, s.out the actions [H][Ktot][A]
    double* knots;                           // [M][Ktot][A] the clipped knot values (what refit / update / keep read)
    int32_t M, kind;                         // 1 <= M <= H; bcmpc_knots.kind
};
hipError_t launch_plan_sample_knots(const PlanSampleKnotsArgs& a, hipStream_t st);

// ---- MPPI's control-cost term and weighted sigma update (mppi_ext.hip; bc_mpc_amd/mppi_update.py) ----
// Both read the iteration's stored actions [H][n_envs * K][A]; environment b: costs / scores / out + b K,
// mu / sigma / mu_new + b H A.
constexpr size_t kMppiControlMaxLds = 65536;     // the gain table and mu in LDS: H * A <= 4096
struct MppiControlArgs {                         // out[c] = costs[c] +- weight * sum_h sum_j g[h][j] (a[h][c][j] - mu[h][j])
    const double* costs;                         // [n_envs * K] raw costs
    const double* actions;                       // [H][Ktot][A]
    const double* mu;                            // [n_envs][H][A] the plan the iteration sampled from
    const double* sigma;
    double* out;                                 // [n_envs * K] the augmented scores
    int64_t K, Ktot, bpe;                        // bpe: workgroups per environment, ceil(K / 256)
    int32_t n_envs, H, A;
    int32_t maximize;                            // learned reward: costs - weight * q
    double weight;
};
struct MppiSigmaArgs {                           // sigma' = clamp(alpha sigma + (1 - alpha) sqrt(sum w (a - mu')^2 / sum w))
    const double* scores;                        // [n_envs * K] the vector the update ran on
    const double* actions;                       // [H][Ktot][A]
    const double* mu_new;                        // [n_envs][H][A] the updated plan
    double* sigma;                               // [n_envs][H][A], in / out
    double* pmin;                                // [n_envs][kMppiMinParts], as MppiArgs
    int64_t* pcnt;
    double* part;                                // [n_envs][H * A + 1][nparts]: V[h][j], then W
    int64_t K, Ktot, nparts;                     // nparts = mppi_parts(K)
    int32_t n_envs, H, A, cpl, nmin;             // cpl = mppi_cpl(K), nmin = mppi_min_blocks(K)
    int32_t maximize;
    double lambda, alpha, min_std, max_std;
};
size_t mppi_control_lds(int32_t HA);             // bytes of dynamic LDS the control-cost kernel takes
size_t mppi_sigma_scratch(int64_t K, int32_t n_envs, int32_t HA);   // doubles: [B][256] [B][256] [B][HA + 1][parts]
hipError_t launch_mppi_control_cost(const MppiControlArgs& a, hipStream_t st);
hipError_t launch_mppi_sigma_update(const MppiSigmaArgs& a, hipStream_t st);   // min, partial, final

}  // namespace bcmpc

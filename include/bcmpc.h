/*
 * bcmpc.h -- C ABI of the MI355X random-shooting MPC rollout engine.
 *
 * This is the drop-in boundary for the reference's hot path
 *   controllers.MPCcontroller.get_action            (controllers.py:57-88)
 *     -> H x dynamics.NNDynamicsModel.predict       (dynamics.py:106-119, MLP dynamics.py:54-71)
 *     -> cost_functions.trajectory_cost_fn(cheetah) (cost_functions.py:9-30, :59-63)
 *     -> np.argmin + first action                   (controllers.py:82-85)
 * and its siblings on the same engine:
 *   MPCcontrollerPolicyNet.get_action      (controllers.py:160-237; policy fused, bcmpc_set_policy)
 *   MPCcontrollerReward.get_action         (controllers.py:90-158; NNDynamicsRewardModel,
 *                                           dynamics.py:121-238; argmax of the discounted reward)
 *   MPCcontrollerPolicyNetReward.get_action (controllers.py:289-363)
 * The reference binds that path in-process from Python; the host mirror
 * (bc_mpc_amd/controllers.py) binds these symbols through ctypes.
 *
 * Plain C: pointers + sizes, no torch/HIP types in the signatures (streams
 * are passed as void*).  Every entry point returns a bcmpc_status; on error
 * bcmpc_last_error() returns a thread-local message.  One engine per device
 * per host thread; an engine is not re-entrant.
 */
#ifndef BCMPC_H_
#define BCMPC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BCMPC_ABI_VERSION 5
#define BCMPC_MAX_LAYERS 8      /* hidden layers supported (dynamics.py:66 n_layers) */
#define BCMPC_MAX_STATE 32      /* S: observation dim (HalfCheetah: 20, cheetah_env.py:21-27) */
#define BCMPC_MAX_INPUT 32      /* S + A (dynamics.py:26 concat) */
#define BCMPC_MAX_ACTION 16

typedef enum bcmpc_status {
    BCMPC_OK = 0,
    BCMPC_ERR_ARG = 1,          /* bad argument (Python: ValueError)          */
    BCMPC_ERR_UNSUPPORTED = 2,  /* shape/mode this build does not implement    */
    BCMPC_ERR_HIP = 3,          /* HIP runtime failure (Python: RuntimeError)  */
    BCMPC_ERR_STATE = 4,        /* e.g. rollout before set_weights             */
    BCMPC_ERR_EMPTY = 5         /* K == 0: np.argmin of an empty sequence      */
} bcmpc_status;

typedef enum bcmpc_activation {  /* dynamics.py:60 activation / train_mpc_ppo.py:539 */
    BCMPC_ACT_TANH = 0,
    BCMPC_ACT_RELU = 1
} bcmpc_activation;

typedef enum bcmpc_cost {
    BCMPC_COST_CHEETAH = 0,     /* fused cheetah_cost_fn (cost_functions.py:10-30), argmin  */
    BCMPC_COST_NONE = 1,        /* no fused cost: caller scores the trajectory              */
    BCMPC_COST_REWARD = 2,      /* learned reward: sum_h reward_h * gamma**h, ARGMAX
                                   (controllers.py:139,150-152); needs BCMPC_MODEL_REWARD  */
    BCMPC_COST_TERMS = 3        /* a list of bcmpc_cost_term (bcmpc_set_cost_terms) scored from the
                                   rolled-out trajectory by a kernel of its own, argmin; any state_dim;
                                   BCMPC_MODEL_DELTA engines without a fused policy.  Additive to ABI 5:
                                   callers detect it by the symbol bcmpc_set_cost_terms           */
} bcmpc_cost;

/* Declarative cost ("terms"): the per-step cost of (s, a, s') is acc = 0.0, then for each term in list
 * order, x being the value `source`/`index` names,
 *   THRESHOLD  if (x cmp param) acc = acc + weight          (NaN compares false, as in NumPy)
 *   DIFF       acc = acc + weight * ((s'[index] - s[index]) / param)       source must be STATE
 *   LINEAR     acc = acc + weight * x
 *   QUADRATIC  d = x - param; acc = acc + weight * (d * d)
 * every operation an individually rounded IEEE f64 operation (no contraction; the division correctly
 * rounded).  The trajectory cost is total = 0.0; for h in 0..H-1: total = total + c_h
 * (trajectory_cost_fn's order, cost_functions.py:59-63); the engine minimises it.
 * {THRESHOLD s[5] >= 0.2 +10, THRESHOLD s[6] >= 0 +10, THRESHOLD s[7] >= 0 +10, DIFF 17 / 0.01 weight -1}
 * is cheetah_cost_fn (cost_functions.py:10-30). */
#define BCMPC_MAX_COST_TERMS 32
typedef enum bcmpc_term_kind { BCMPC_TERM_THRESHOLD = 0, BCMPC_TERM_DIFF = 1, BCMPC_TERM_LINEAR = 2,
                               BCMPC_TERM_QUADRATIC = 3 } bcmpc_term_kind;
typedef enum bcmpc_term_source { BCMPC_SRC_STATE = 0, BCMPC_SRC_NEXT_STATE = 1, BCMPC_SRC_ACTION = 2 } bcmpc_term_source;
typedef enum bcmpc_term_cmp { BCMPC_CMP_GE = 0, BCMPC_CMP_GT = 1, BCMPC_CMP_LE = 2, BCMPC_CMP_LT = 3 } bcmpc_term_cmp;
typedef struct bcmpc_cost_term {   /* 32 bytes */
    int32_t kind, source, index, cmp;   /* bcmpc_term_kind, bcmpc_term_source, dim (< S, or < A for ACTION),
                                           bcmpc_term_cmp (THRESHOLD only) */
    double weight, param;               /* param: threshold / divisor / unused / target */
} bcmpc_cost_term;

typedef enum bcmpc_model {      /* which dynamics net (dynamics.py)                          */
    BCMPC_MODEL_DELTA = 0,      /* NNDynamicsModel: L x dense(h) -> dense(S) (:54-71)        */
    BCMPC_MODEL_REWARD = 1      /* NNDynamicsRewardModel: tanh trunk dense(h) -> {delta head
                                   dense(h) -> dense(S), reward head dense(h) -> dense(1)},
                                   LayerNorm per head (:150-177); n_layers must be 2         */
} bcmpc_model;

typedef enum bcmpc_precision {
    BCMPC_PREC_FP32 = 0,        /* f32 MLP on v_mfma_f32_16x16x4_f32 (exact f32 fma chain) */
    BCMPC_PREC_SPLIT_F16 = 1,   /* f32-accurate MLP on the f16 matrix cores: every operand as
                                   hi + lo f16 halves (22 bits), three v_mfma_f32_16x16x32_f16
                                   passes hi*hi + hi*lo + lo*hi, f32 accumulate (DESIGN.md
                                   "split kernel"); tanh, no LayerNorm, NNDynamicsModel only */
    BCMPC_PREC_F16 = 2          /* BASELINE cfg3's "bf16 MFMA GEMM + fp32 cost": one f16 pass
                                   (11-bit operands, f32 accumulate, f64 state / cost) on the
                                   split slab kernels; the tanh NNDynamicsModel only.  NOT the
                                   fp32 tolerance: DESIGN.md "single-pass f16"               */
} bcmpc_precision;

typedef enum bcmpc_kernel {     /* rollout kernel layout (DESIGN.md "kernels")              */
    BCMPC_KERNEL_AUTO = 0,
    BCMPC_KERNEL_SOLO = 1,      /* one wave owns 16 candidates, activations in VGPRs     */
    BCMPC_KERNEL_GROUP2 = 2,    /* retired in round 6 (A/B only, never chosen by auto):
                                   bcmpc_create returns BCMPC_ERR_UNSUPPORTED             */
    BCMPC_KERNEL_GROUP4 = 3,    /* 4 waves share 16 candidates                           */
    BCMPC_KERNEL_GROUP8 = 4,    /* 8 waves share 16 candidates (small K)                 */
    BCMPC_KERNEL_SPLIT1 = 5,    /* BCMPC_PREC_SPLIT_F16: one workgroup = 1 x 16 candidates  */
    BCMPC_KERNEL_SPLIT2 = 6,    /*                                      2 x 16 candidates  */
    BCMPC_KERNEL_SPLIT4 = 7,    /*                                      4 x 16 candidates  */
    BCMPC_KERNEL_SPLITR = 8,    /* retired in round 6 (the resident-column rollout_rr, slower
                                   than SPLIT4 at every K): bcmpc_create returns
                                   BCMPC_ERR_UNSUPPORTED; the value stays reserved            */
    BCMPC_KERNEL_TEAM = 9       /* BCMPC_PREC_SPLIT_F16, small K: 2-layer NNDynamicsModel (tanh
                                   / relu, LayerNorm up to hidden 256), and at hidden 449..512
                                   (tanh) with a fused policy (<= 2 x 128) and / or the
                                   NNDynamicsRewardModel: one 16-candidate column per team of 1
                                   (hidden <= 256), 4 (512) or 8 (reward net) workgroups, every
                                   weight resident in registers, the output layer's partial sums
                                   exchanged between the team's workgroups once per step
                                   (rollout_team.hip).  Needs the whole grid resident:
                                   ceil(K/128)*8*members <= the device's CUs                 */
} bcmpc_kernel;

typedef enum bcmpc_policy_mode {   /* MPCcontrollerPolicyNet.self_exp (controllers.py:201-208) */
    BCMPC_POLICY_EXPLORE = 0,      /* self_exp=False: (1-explore)*mean + explore*U(low,high)   */
    BCMPC_POLICY_STOCHASTIC = 1    /* self_exp=True: mean + exp(logstd)*N(0,1) (device Philox)  */
} bcmpc_policy_mode;

/* Replaces the constructor arguments of MPCcontroller (controllers.py:28-35)
 * plus the NNDynamicsModel shape (dynamics.py:8-19, build_network :54-62). */
typedef struct bcmpc_config {
    int32_t state_dim;    /* S  (env.observation_space.shape[0], dynamics.py:23)  */
    int32_t action_dim;   /* A  (env.action_space.shape[0], dynamics.py:24)       */
    int32_t hidden;       /* h  (dynamics.py:59 size)                              */
    int32_t n_layers;     /* L  (dynamics.py:58 n_layers)                          */
    int32_t activation;   /* bcmpc_activation                                      */
    int32_t layer_norm;   /* FLAGS.LAYER_NORM (dynamics.py:68)                     */
    int32_t horizon;      /* H  (controllers.py:31 horizon)                        */
    int32_t cost;         /* bcmpc_cost                                            */
    int64_t num_paths;    /* K on this device (controllers.py:33 num_simulated_paths) */
    int32_t precision;    /* bcmpc_precision                                       */
    int32_t device;       /* HIP device ordinal                                    */
    int32_t kernel;       /* bcmpc_kernel: 0 = auto                                */
    int32_t policy_hidden;  /* 0: MPCcontroller; >0: MPCcontrollerPolicyNet policy width (hid_size) */
    int32_t policy_layers;  /* policy hidden layers (num_hid_layers, train_mpc_ppo.py:178)         */
    int32_t policy_mode;    /* bcmpc_policy_mode                                                   */
    int32_t model;        /* bcmpc_model                                           */
    int32_t reserved[3];  /* must be zero                                          */
} bcmpc_config;

/* Replaces the state NNDynamicsModel holds: TF variables
 * NNDynamicsModel/dense{,_1,..}/{kernel,bias} (+ LayerNorm/{gamma,beta}) and
 * the normalization stats of dynamics.py:41.  Host pointers, copied.
 * BCMPC_MODEL_REWARD (dynamics.py:150-177) passes the variables in TF creation
 * order: kernels/biases = dense (trunk [S+A,h]), dense_1 (delta hidden [h,h]),
 * dense_2 (delta out [h,S]), dense_3 (reward hidden [h,h]), dense_4 (reward out
 * [h,1]); ln_gamma/ln_beta = LayerNorm (trunk), LayerNorm_1 (delta), LayerNorm_2
 * (reward); plus mean_reward / std_reward (dynamics.py:143, 236). */
typedef struct bcmpc_weights {
    const float* const* kernels;   /* L+1 arrays, kernel[l] is [in, out] row-major  */
    const float* const* biases;    /* L+1 arrays of length out                      */
    const float* const* ln_gamma;  /* L arrays of length h, or NULL when LN is off  */
    const float* const* ln_beta;   /* L arrays of length h, or NULL                 */
    const double* mean_obs;        /* S */
    const double* std_obs;         /* S */
    const double* mean_action;     /* A */
    const double* std_action;      /* A */
    const double* mean_deltas;     /* S */
    const double* std_deltas;      /* S */
    const double* mean_reward;     /* 1 (BCMPC_MODEL_REWARD only, else NULL) */
    const double* std_reward;      /* 1 (BCMPC_MODEL_REWARD only, else NULL) */
} bcmpc_weights;

/* Output of one control step (controllers.py:82-85). */
typedef struct bcmpc_result {
    int64_t best_index;                       /* global candidate index, np.argmin semantics
                                                 (np.argmax for BCMPC_COST_REWARD)           */
    double best_cost;                         /* costs[best_index] (controllers.py:83); the best
                                                 discounted reward sum for BCMPC_COST_REWARD */
    double first_action[BCMPC_MAX_ACTION];    /* action_paths[0, best_index, :]              */
} bcmpc_result;

/* Replaces the policy net MPCcontrollerPolicyNet consults each step
 * (ppo_bc_policy.py:54-88): obz = clip((ob - ob_mean)/ob_std, -5, 5);
 * tanh dense x policy_layers; mean = dense(., A); logstd.  Host pointers, copied. */
typedef struct bcmpc_policy {
    const float* const* kernels;   /* policy_layers+1 arrays [in,out] (pi/pol/fc1.., final) */
    const float* const* biases;
    const float* ob_mean;          /* S (RunningMeanStd.mean, f32)   */
    const float* ob_std;           /* S (RunningMeanStd.std, f32)    */
    const float* logstd;           /* A                              */
    double explore;                /* MPCcontrollerPolicyNet.explore */
} bcmpc_policy;

/* CEM outer loop (BASELINE cfg5 "CEM outer loop (4 elite iters)"; not in the reference,
 * semantics in DESIGN.md "CEM").  Iteration i samples every candidate's actions as
 * clip(mu + sigma * z, low, high), z = Irwin-Hall(12) - 6 from Philox keyed by
 * (seed, global candidate, h, j, i); scores them like get_action; keeps the n_elite
 * lowest (cost, index) (NaN last, ties -> lower index); refits mu / sigma [H][A] to
 * the elites' mean / std (fixed reduction order) smoothed by alpha.  The answer is
 * the first action of the best candidate over ALL iterations (np.argmin over the
 * iteration-major concatenation of the cost vectors). */
typedef struct bcmpc_cem {
    int32_t iterations;   /* CEM iterations (cfg5: 4)                                   */
    int32_t n_elite;      /* elites per iteration, over all ranks (>= 1)               */
    double alpha;         /* new = alpha * old + (1 - alpha) * elite statistic         */
    int64_t k_global;     /* candidates over all ranks; result positions are
                             iteration * k_global + global index                      */
} bcmpc_cem;

typedef struct bcmpc_elite {   /* one (cost, global candidate index) record; index < 0 = empty */
    double cost;
    int64_t index;
} bcmpc_elite;

/* MPPI outer loop (model-predictive path integral control; not in the reference, semantics in
 * DESIGN.md "MPPI").  An iteration samples and scores the candidates exactly like a CEM iteration,
 * then replaces mu by the softmin-weighted mean of ALL candidates' actions: score v = cost (-cost
 * for the learned reward), a candidate is valid iff v is finite, w = exp(-(v - v_min) / lambda)
 * (0 when invalid), mu'[h][j] = sum w a[h][j] / sum w.  sigma is not modified.  Additive to ABI 5:
 * callers detect it by the symbol bcmpc_mppi_get_action. */
typedef struct bcmpc_mppi {
    int32_t iterations;   /* rollout + update rounds (>= 1)                            */
    double lambda;        /* temperature, finite and > 0                               */
    int64_t k_global;     /* 0 or num_paths (single device)                            */
} bcmpc_mppi;

typedef struct bcmpc_mppi_stats {   /* of one update; no valid candidate: 0, 0, NaN, 0 */
    double weight_sum;    /* W = sum w (>= 1: the best candidate has w = 1)            */
    double ess;           /* effective sample size W^2 / sum w^2, in [1, n_valid]      */
    double min_cost;      /* best valid cost (largest reward sum for the learned reward) */
    int64_t n_valid;      /* candidates with a finite score                            */
} bcmpc_mppi_stats;

typedef struct bcmpc_engine bcmpc_engine;

int bcmpc_abi_version(void);
const char* bcmpc_last_error(void);

/* MPCcontroller.__init__ (controllers.py:28-41) + device allocation. */
int bcmpc_create(const bcmpc_config* cfg, bcmpc_engine** out);
int bcmpc_destroy(bcmpc_engine* eng);

/* Weight re-sync hook: idempotent on `version`; a new version
 * re-packs the dense kernels into MFMA fragment order on the device. */
int bcmpc_set_weights(bcmpc_engine* eng, const bcmpc_weights* w, uint64_t version);
uint64_t bcmpc_weights_version(const bcmpc_engine* eng);

/* Policy weights for MPCcontrollerPolicyNet engines (config.policy_hidden > 0). */
int bcmpc_set_policy(bcmpc_engine* eng, const bcmpc_policy* p, uint64_t version);

/* MPCcontrollerReward.gamma (controllers.py:99,139): step h's reward is scaled by
 * gamma**h (host pow, as Python's float ** int).  Default 1.0.  Reward engines only. */
int bcmpc_set_discount(bcmpc_engine* eng, double gamma);

/* The cost of a BCMPC_COST_TERMS engine (BCMPC_ERR_ARG on any other): n terms, 0 <= n <=
 * BCMPC_MAX_COST_TERMS, copied.  n == 0: every cost is 0 and index 0 wins.  BCMPC_ERR_ARG: unknown kind /
 * source / cmp, index outside the state (ACTION: the action), a DIFF whose source is not STATE, weight or
 * param not finite, a DIFF param of 0, more than BCMPC_MAX_COST_TERMS entries together with the done conditions
 * the engine holds (bcmpc_set_termination).  Every rollout entry of such an engine returns BCMPC_ERR_STATE
 * before this call.  May be called again between launches (the next launch uses the new list). */
int bcmpc_set_cost_terms(bcmpc_engine* eng, const bcmpc_cost_term* terms, int32_t n);

/* The term-cost kernel alone, stream-ordered, on a caller's trajectory:
 *   d_traj    : device [H+1][K][S] doubles (the layout bcmpc_rollout_async's d_traj has)
 *   d_actions : device [H][K][A] doubles read by ACTION terms, or NULL => regenerated: the Philox shooting
 *               draw (seed, cand_offset + k, h, j) when d_mu is NULL, else the CEM / MPPI sample of
 *               iteration cem_iter from d_mu / d_sigma [H][A]; never touched without an ACTION term
 *   K         : candidates (>= 1; need not equal num_paths); H, S, A and the action bounds are the engine's
 *   d_costs   : device K doubles
 * BCMPC_ERR_ARG: null pointers, K < 1, cem_iter outside [0, 2^22), not a BCMPC_COST_TERMS engine.
 * BCMPC_ERR_STATE: no terms set. */
int bcmpc_trajectory_cost_async(bcmpc_engine* eng, const double* d_traj, const double* d_actions, uint64_t seed,
                                int64_t cand_offset, const double* d_mu, const double* d_sigma, int32_t cem_iter,
                                int64_t K, double* d_costs, void* stream);

/* ---- Terminal value: total[k] = cost[k] + weight * (double)V(s_H[k]) ------------------------------------
 * V is the critic the reference trains beside its policy (ppo_bc_policy.py:56-64, scope pi/vf) over the
 * policy's obfilter:  obz = clip((f32(s) - ob_mean) / ob_std, -5, 5);  h = tanh(h W + b) per hidden layer;
 * v = h w_final + b_final, all f32 (definition: bc_mpc_amd/value.py terminal_values).  total is one rounded
 * f64 multiply and one rounded f64 add.  The argmin, CEM's elite selection, the MPPI weights and the ensemble
 * rules then run on total with the rules they have on cost (a NaN total wins the argmin).  Additive to ABI 5:
 * callers detect the feature by the symbol bcmpc_set_terminal_value. */
#define BCMPC_VALUE_MAX_LAYERS 4     /* hidden layers of a value net */
#define BCMPC_VALUE_MAX_HIDDEN 256   /* ... and their width          */
typedef struct bcmpc_value_net {
    const float* const* kernels;   /* n_layers+1 arrays [in,out] row-major (pi/vf/fc1.., final [hidden,1]) */
    const float* const* biases;    /* n_layers+1 arrays of length out                                      */
    const float* ob_mean;          /* state_dim (RunningMeanStd.mean, f32)                                 */
    const float* ob_std;           /* state_dim, finite and > 0                                            */
    int32_t n_layers;              /* hidden layers, 1 .. BCMPC_VALUE_MAX_LAYERS                           */
    int32_t hidden;                /* their width, 1 .. BCMPC_VALUE_MAX_HIDDEN                             */
    int32_t state_dim;             /* 1 .. 32; the rollout entries need it to equal the engine's           */
    int32_t reserved;              /* must be zero                                                         */
} bcmpc_value_net;

/* BCMPC_OK if an engine of this config takes a terminal value, else BCMPC_ERR_UNSUPPORTED with a message:
 * a fused policy, the reward model / BCMPC_COST_REWARD and BCMPC_COST_NONE do not.  No HIP call. */
int bcmpc_terminal_value_supported(const bcmpc_config* cfg);

/* Sets (v != NULL) or removes (v == NULL) the engine's terminal value.  Idempotent on `version`: with the
 * version already set only `weight` is updated; a new version validates, packs the kernels into MFMA fragment
 * order and uploads them.  The first call also allocates what the launch chain needs -- the trajectory scratch
 * [H+1][num_paths][S] (a BCMPC_COST_TERMS engine already owns one) -- here, never inside a stream-ordered
 * entry, so a captured graph keeps its addresses.  From then on every entry built on the rollout launch --
 * bcmpc_get_action, bcmpc_rollout_async, the batched step, bcmpc_cem_*, bcmpc_mppi_*, the batched planners,
 * the ensemble entries (each member adds the value of ITS final state to its row before the reduce) -- runs
 * rollout -> (term cost) -> terminal value into the cost vector -> argmin; the fused argmin tails are off, as
 * for cost terms.
 * BCMPC_ERR_ARG (all checked before any HIP call, the net before the engine): v's pointers null, n_layers or
 * hidden outside their ranges, reserved != 0, a non-finite kernel / bias / ob_mean, ob_std not finite or
 * <= 0, weight not finite, a null engine.  A net over another state_dim than the engine's is accepted for
 * bcmpc_terminal_value_async alone: every rollout entry answers it with BCMPC_ERR_ARG.
 * BCMPC_ERR_UNSUPPORTED: bcmpc_terminal_value_supported's cases; a communicator attached.
 * bcmpc_get_action_mt19937 refuses an engine with a value (draw with NumPy on the host and pass the actions). */
int bcmpc_set_terminal_value(bcmpc_engine* eng, const bcmpc_value_net* v, double weight, uint64_t version);

/* The value kernel alone, stream-ordered, allocates nothing:
 *   d_states      : device rows of the NET's state_dim doubles, row k at d_states + k * row_stride (>= it)
 *   d_values      : device K floats, or NULL
 *   d_costs_inout : device K doubles, updated in place: c[k] = c[k] + weight * (double)v[k], or NULL
 * BCMPC_ERR_ARG: null engine / d_states, both outputs NULL, K < 1, row_stride < the net's state_dim.
 * BCMPC_ERR_STATE: no value set. */
int bcmpc_terminal_value_async(bcmpc_engine* eng, const double* d_states, int64_t row_stride, int64_t K,
                               float* d_values, double* d_costs_inout, void* stream);

/* Diagnostics: v of local candidates idx[0..n) as the engine's LAST launch chain computed them (a CEM / MPPI
 * call: its last iteration), after a synchronisation of the engine's stream.  BCMPC_ERR_ARG: null pointers,
 * n < 1, an index outside [0, num_paths).  BCMPC_ERR_STATE: no value set. */
int bcmpc_last_terminal_values(bcmpc_engine* eng, const int64_t* idx, int32_t n, float* out);

/* ---- Episode termination for cost terms (definition: bc_mpc_amd/cost_functions.py episode_cost) ------------
 *   total = 0; t = H
 *   for h in 0 .. H-1:  total = total + c_h;  if any condition holds on s_{h+1}: total = total + done_cost;
 *                                                                             t = h; stop
 * every operation one rounded f64 operation, in this order; the terminating step is still paid.  With a
 * terminal value set, total = total + weight * (double)V(s_H) only where t == H; a terminated candidate's total
 * is left untouched.  The argmin, CEM's elite selection, the MPPI weights and the ensemble rules then run on
 * total as before; every ensemble member terminates on its own trajectory.  Additive to ABI 5: callers detect
 * the feature by the symbol bcmpc_set_termination.
 *
 * bcmpc_set_termination: n done conditions, ORed, copied; n == 0 removes termination.  A condition is a
 * bcmpc_cost_term of kind BCMPC_TERM_THRESHOLD and source BCMPC_SRC_NEXT_STATE with a valid cmp, an index
 * inside the state, a finite param and weight 0 (a NaN compares false).  done_cost is finite and added once, at
 * the terminating step.  Cost terms plus conditions are at most BCMPC_MAX_COST_TERMS: whichever of
 * bcmpc_set_cost_terms and bcmpc_set_termination is called second checks it.  The call allocates the engine's
 * termination-step buffer int32 [num_paths] -- here, never inside a stream-ordered entry, so a captured graph
 * keeps its addresses -- and from then on every entry built on the rollout launch applies the conditions.
 * BCMPC_ERR_ARG (every check before any HIP call): a null engine, not a BCMPC_COST_TERMS engine, n outside
 * [0, 32], any of the above violated, the budget exceeded. */
int bcmpc_set_termination(bcmpc_engine* eng, const bcmpc_cost_term* conds, int32_t n, double done_cost);

/* bcmpc_trajectory_cost_async plus d_term_step: device K int32, candidate k's terminating step in [0, H], H
 * exactly when it never terminated; may be NULL.  On an engine without termination nothing is written to it.
 * bcmpc_trajectory_cost_async itself applies the engine's termination to d_costs and writes no steps. */
int bcmpc_trajectory_cost_steps_async(bcmpc_engine* eng, const double* d_traj, const double* d_actions,
                                      uint64_t seed, int64_t cand_offset, const double* d_mu,
                                      const double* d_sigma, int32_t cem_iter, int64_t K, double* d_costs,
                                      int32_t* d_term_step, void* stream);

/* bcmpc_terminal_value_async plus the gate: with d_term_step (device K int32) the cost add is made only where
 * d_term_step[k] == horizon; elsewhere d_costs_inout[k] keeps its bits.  d_values[k] is written regardless.
 * d_term_step == NULL: bcmpc_terminal_value_async, bit for bit. */
int bcmpc_terminal_value_masked_async(bcmpc_engine* eng, const double* d_states, int64_t row_stride, int64_t K,
                                      float* d_values, double* d_costs_inout, const int32_t* d_term_step,
                                      int32_t horizon, void* stream);

/* Diagnostics: the terminating steps of local candidates idx[0..n) from the engine's LAST launch chain (a CEM /
 * MPPI call: its last iteration; a team engine's rerun: the fallback's), after a synchronisation of the
 * engine's stream.  BCMPC_ERR_ARG: null pointers, n < 1, an index outside [0, num_paths).  BCMPC_ERR_STATE: no
 * termination set. */
int bcmpc_last_termination_steps(bcmpc_engine* eng, const int64_t* idx, int32_t n, int32_t* out);

/* ---- Reference tracking: per-call targets and action-rate terms (definition: cost_functions.py episode_cost
 * with reference / previous_action) ---------------------------------------------------------------------------
 * A call carries a reference r[env][h][c] of n_ref channels and, optionally, a previous action per environment.
 * A THRESHOLD or QUADRATIC term whose `ref` is a channel c reads p = r[env][h][c] at step h in place of `param`,
 * whatever its source; the arithmetic is the term's otherwise, and a non-finite reference value propagates as
 * IEEE says.  A RATE term is  d = a_h[index] - a_{h-1}[index]; acc = acc + weight * (d * d)  with a_{-1} the
 * call's previous action, or a_0 itself when the call has none.  Candidate k of a launch over n_envs
 * environments belongs to environment k / (num_paths / n_envs).  What a list reads per row -- its state dims,
 * actions and channels, each counted once, the done conditions' dims included -- is at most
 * BCMPC_MAX_COST_TERMS slots.  Additive to ABI 5: callers detect the feature by the symbol
 * bcmpc_set_cost_terms_x. */
#define BCMPC_TERM_RATE 4            /* a bcmpc_term_kind of bcmpc_cost_term_x alone: source ACTION, ref -1 */
#define BCMPC_MAX_REF_CHANNELS 16
typedef struct bcmpc_cost_term_x {   /* 48 bytes: bcmpc_cost_term's fields, then ref */
    int32_t kind, source, index, cmp;
    double weight, param;
    int32_t ref;                     /* -1: param is the constant; else the channel, < n_ref */
    int32_t reserved[3];             /* must be zero */
} bcmpc_cost_term_x;

/* bcmpc_set_cost_terms with the extended record: every check of bcmpc_set_cost_terms, plus BCMPC_ERR_ARG for
 * n_ref outside [0, 16], a ref outside [-1, n_ref), a ref on a kind other than THRESHOLD / QUADRATIC, a RATE
 * whose source is not ACTION, reserved != 0, more than 32 slots, more than 32 entries together with the done
 * conditions the engine holds.  A list that names no channel and has no RATE term is bcmpc_set_cost_terms'.
 * bcmpc_set_cost_terms replaces an extended list with a plain one (and still refuses kind 4).  All argument
 * checks come before any HIP call. */
int bcmpc_set_cost_terms_x(bcmpc_engine* eng, const bcmpc_cost_term_x* terms, int32_t n, int32_t n_ref);

/* The inputs of the calls that follow, copied from HOST memory into the engine's buffers on the engine's stream
 * (behind what that stream was given before); the call returns when the copies have landed, so an entry on any
 * stream, or a graph replay, that is issued afterwards reads the new data.  The caller must not replace the inputs
 * while a launch it issued on ANOTHER stream may still read them.  Valid until replaced:
 *   ref         : [ref_envs][ref_steps][n_ref] doubles, ref_steps 1 (constant over the horizon) or H; NULL with
 *                 an engine whose list names no channel
 *   prev_action : [prev_envs][A] doubles, or NULL: no previous action (a_{-1} := a_0)
 * ref_envs / prev_envs are 1 (shared by every environment of a call) or the n_envs of the calls that follow; a
 * call over another n_envs returns BCMPC_ERR_ARG.  The buffers are allocated here, never inside a stream-ordered
 * entry, and only grow: calls with the same (or smaller) sizes keep their addresses, so a captured graph replays
 * on the new data.  BCMPC_ERR_ARG (before any HIP call): a null engine, not an
 * extended list, ref NULL where the list names a channel, ref_steps outside {1, H}, ref_envs / prev_envs outside
 * [1, num_paths].  A rollout entry on an engine whose list names a channel returns BCMPC_ERR_STATE before this
 * call, with nothing launched. */
int bcmpc_set_cost_inputs(bcmpc_engine* eng, const double* ref, int32_t ref_envs, int32_t ref_steps,
                          const double* prev_action, int32_t prev_envs);

/* bcmpc_trajectory_cost_steps_async for an extended list, on DEVICE inputs: candidate k reads environment
 * k / env_paths (K a multiple of env_paths); d_ref [ref_envs][ref_steps][n_ref] (NULL only where no channel is
 * named), d_prev [prev_envs][A] or NULL; ref_envs / prev_envs 1 or K / env_paths, ref_steps 1 or H.  Allocates
 * nothing.  BCMPC_ERR_ARG on any of that violated; BCMPC_ERR_STATE: no extended list set. */
int bcmpc_trajectory_cost_inputs_async(bcmpc_engine* eng, const double* d_traj, const double* d_actions,
                                       uint64_t seed, int64_t cand_offset, const double* d_mu,
                                       const double* d_sigma, int32_t cem_iter, int64_t K, double* d_costs,
                                       int32_t* d_term_step, int64_t env_paths, const double* d_ref,
                                       int32_t ref_envs, int32_t ref_steps, const double* d_prev,
                                       int32_t prev_envs, void* stream);

/* Diagnostics: the device addresses of the engine's input buffers (NULL before they exist). */
int bcmpc_cost_input_buffers(bcmpc_engine* eng, void** d_ref, void** d_prev);

/* env.action_space.low / .high (controllers.py:53). Defaults: [-1, 1]^A. */
int bcmpc_set_action_bounds(bcmpc_engine* eng, const double* low, const double* high);

/* MPCcontroller.get_action (controllers.py:57-88), synchronous, host memory.
 *   state    : S doubles (tiled K times, controllers.py:63)
 *   actions  : [H, K, A] doubles in C order (the array np.random.uniform returns
 *              at controllers.py:53), or NULL => draw them on the device with
 *              Philox4x32-10 keyed by (seed, cand_offset + k, h, j)
 *   cand_offset : global index of this device's first candidate (multi-GPU shard)
 *   out      : best index (global) / cost / first action
 *   costs_out: optional K doubles, per-candidate trajectory cost (cost_functions.py:59-63),
 *              or discounted reward sum (BCMPC_COST_REWARD, controllers.py:150)
 * Without a communicator the state travels in the kernel arguments and the argmin writes the
 * result into mapped host memory: one rollout + one argmin launch, one stream synchronisation. */
int bcmpc_get_action(bcmpc_engine* eng, const double* state, const double* actions,
                     uint64_t seed, int64_t cand_offset, bcmpc_result* out, double* costs_out);

/* MPCcontroller.get_action with the reference's RNG contract (controllers.py:53): the
 * [H, k_global, A] array np.random.uniform(low, high, size) would return is drawn from NumPy's
 * legacy MT19937 state (mt_key[624] / mt_pos as np.random.get_state() holds them; advanced in
 * place, as the one NumPy call would advance them, and only when the call succeeds) -- only this
 * shard's [cand_offset, cand_offset + K) slice of each step is produced:
 *   default: ON THE GPU (mt_device.hip): the draw is cut into chunks, each chunk's start window
 *     reached by an MT19937 jump-ahead polynomial (GF(2) correlation on the device) and its words
 *     generated, tempered and scaled by one workgroup straight into HBM; no host draw, no PCIe
 *     upload of the array (the key, 2.5 KB, goes up; the final state comes back with the result);
 *   BCMPC_MT_PATH=host: on the host into pinned memory, step by step or split over host threads
 *     by jump-ahead (bcmpc_mt19937_uniform_par), each slice copied as soon as it is drawn.
 * Then as bcmpc_get_action (seed: the stochastic policy's Philox normals); out->first_action is
 * action_paths[0, best] of that same array (policy engines: the mixed action, the array being the
 * exploration draw of controllers.py:191). */
int bcmpc_get_action_mt19937(bcmpc_engine* eng, const double* state, uint32_t* mt_key, int32_t* mt_pos,
                             const double* low, const double* high, int64_t k_global, int64_t cand_offset,
                             uint64_t seed, bcmpc_result* out, double* costs_out);

/* Small draws (<= BCMPC_MT_ZC_WORDS generator words, the reference's K = 400 steps) of
 * bcmpc_get_action_mt19937: after a call, a worker thread draws the NEXT call's rows from the advanced
 * state; a call whose (key, pos, bounds, shard) equal that job's start uses them -- a hit (rows
 * complete, copied into HBM when the copy has landed) or, on team-kernel engines, a late hit (the job
 * still running: the kernel waits for the rows' sequence word in mapped memory) -- else it draws itself
 * (a miss).  Larger draws (the device path): the NEXT call's draw is enqueued on the device from this
 * draw's final state -- behind a synchronous call's argmin, or beside its rollout on a stream of its own
 * when the slab grid leaves CUs free (K <= 32 per CU) -- (BCMPC_MT_SPECULATE=0: off), used by the
 * next call when NumPy's state, bounds and shard equal its start (two misses in a row pause it for 32
 * calls).  out5 = {hits incl. late, late hits, misses, speculative hits, speculative misses} since
 * bcmpc_create. */
int bcmpc_predraw_stats(const bcmpc_engine* eng, uint64_t* out5);

/* The same draw as bcmpc_get_action_mt19937 on the device, alone: this engine's shard
 * [H, K, A] of np.random.uniform(low, high, [H, k_global, A]) (controllers.py:53) drawn on the GPU
 * from (mt_key, mt_pos), copied to `out` (host, H*K*A doubles); mt_key / mt_pos advance as the one
 * NumPy call would advance them.  For tests and for callers that want the array itself. */
int bcmpc_mt19937_uniform_device(bcmpc_engine* eng, uint32_t* mt_key, int32_t* mt_pos, const double* low,
                                 const double* high, int64_t k_global, int64_t cand_offset, double* out);

/* Host only (no GPU): n_rows x action_dim doubles of np.random.uniform(low, high) from the
 * legacy MT19937 state (mt_key / mt_pos in/out) -- the generator bcmpc_get_action_mt19937 uses. */
int bcmpc_mt19937_uniform(uint32_t* mt_key, int32_t* mt_pos, const double* low, const double* high,
                          int32_t action_dim, int64_t n_rows, double* out);

/* Host only (no GPU): the same stream as bcmpc_mt19937_uniform, drawn by up to `threads` host
 * threads (<= 0: BCMPC_MT_THREADS, else min(8, hardware threads)) that each jump ahead to their own
 * block of the stream (MT19937 jump-ahead, csrc/mt_jump.cpp) and draw at least
 * min_words_per_thread generator words (< 0: the library's default, 2^20).  n_rows rows in
 * repeating groups of `period` rows; only rows r with r % period in [keep_lo, keep_hi) are stored
 * (a shard's candidates of each step: period = k_global), densely in row order.  mt_key / mt_pos
 * end exactly where the serial draw leaves them; *used_threads (optional) = threads used (1: serial).
 * The path bcmpc_get_action_mt19937 takes for large draws. */
int bcmpc_mt19937_uniform_par(uint32_t* mt_key, int32_t* mt_pos, const double* low, const double* high,
                              int32_t action_dim, int64_t n_rows, int64_t period, int64_t keep_lo, int64_t keep_hi,
                              double* out, int32_t threads, int64_t min_words_per_thread, int32_t* used_threads);

/* Actions the last rollout actually used for step 0 (policy engines:
 * action_paths[0] of controllers.py:233), copied to host K x A doubles. */
int bcmpc_first_actions(bcmpc_engine* eng, double* out);

/* Device-memory, asynchronous form (no host sync; graph-capturable).
 *   d_state      : device, S doubles, or [K, S] when state_stride == S (predict mode,
 *                  dynamics.py:106 on per-candidate states)
 *   d_actions    : device [H, K, A] doubles, or NULL => device RNG
 *   d_costs      : device K doubles (required when cost == CHEETAH, REWARD or TERMS)
 *   d_traj       : device [H+1, K, S] doubles or NULL (states_paths_all, controllers.py:65-74; a
 *                  BCMPC_COST_TERMS engine scores the trajectory it writes here, or its own scratch)
 *   d_result     : device bcmpc_result or NULL (argmin + first action)
 *   stream       : hipStream_t the launches are enqueued on, used verbatim (NULL is HIP's
 *                  null stream; pass bcmpc_stream(eng) for the engine's own stream) */
int bcmpc_rollout_async(bcmpc_engine* eng, const double* d_state, int64_t state_stride,
                        const double* d_actions, uint64_t seed, int64_t cand_offset,
                        double* d_costs, double* d_traj, bcmpc_result* d_result, void* stream);

/* Batched control step (ABI 5): n_envs environments per launch chain, K = num_paths / n_envs
 * candidates each (num_paths % n_envs must be 0).  Candidate column c = b * K + j (0 <= j < K) belongs
 * to environment b and starts from states[b]; its Philox index is cand_offset + c.  For every b,
 *   out[b] == bcmpc_get_action(states[b], seed, cand_offset + b * K)
 * of a K-candidate engine of the same kernel layout: best_index is global (cand_offset + b * K + j*,
 * j* by np.argmin over the environment's K costs, np.argmax for BCMPC_COST_REWARD), best_cost that
 * candidate's cost, first_action its step-0 action.
 *   states    : host [n_envs][S] doubles
 *   actions   : host [H][num_paths][A] doubles (column c as above), or NULL => device Philox
 *   out       : host [n_envs] records
 *   costs_out : optional host [num_paths] doubles (environment b's costs at [b * K, (b + 1) * K))
 * One chain on the engine's stream: the states expanded to the candidates (tile_states), the rollout
 * on per-candidate states, one argmin workgroup per environment (argmin_segments); the records come
 * back in one device-to-host copy, one stream synchronisation.  A team-kernel engine whose team gave
 * up reruns the call on its fallback engine, as bcmpc_get_action does.
 * BCMPC_ERR_ARG: null pointers, n_envs < 1, num_paths % n_envs != 0, cost == BCMPC_COST_NONE.
 * BCMPC_ERR_UNSUPPORTED (not batched yet): engines with a fused policy, engines with a communicator
 * attached.  CEM and MPPI: bcmpc_cem_get_actions_batch / bcmpc_mppi_get_actions_batch below. */
int bcmpc_get_actions_batch(bcmpc_engine* eng, const double* states, int32_t n_envs, const double* actions,
                            uint64_t seed, int64_t cand_offset, bcmpc_result* out, double* costs_out);

/* The same chain on device memory, stream-ordered, no host synchronisation:
 *   d_states  : device [n_envs][S] doubles
 *   d_actions : device [H][num_paths][A] doubles or NULL => device Philox
 *   d_costs   : device [num_paths] doubles (required)
 *   d_results : device [n_envs] records
 *   stream    : as bcmpc_rollout_async
 * Team-kernel engines: bcmpc_engine_status once the stream has completed, as for every
 * stream-ordered launch. */
int bcmpc_rollout_batch_async(bcmpc_engine* eng, const double* d_states, int32_t n_envs, const double* d_actions,
                              uint64_t seed, int64_t cand_offset, double* d_costs, bcmpc_result* d_results,
                              void* stream);

/* MPCcontrollerPolicyNet engines: bcmpc_rollout_async plus the actions actually rolled out at
 * EVERY step -- d_actions_out [H, K, A] f64, the reference's action_paths (controllers.py:208-213:
 * the policy mean mixed with the exploration draw, or mean + exp(logstd) * N(0,1) when self_exp)
 * -- and optionally the states (d_traj [H+1, K, S]), so a caller (or a test) can replay each step.
 * d_actions: the [H, K, A] exploration draw or NULL (device Philox). */
int bcmpc_rollout_policy_async(bcmpc_engine* eng, const double* d_state, const double* d_actions, uint64_t seed,
                               int64_t cand_offset, double* d_costs, double* d_traj, double* d_actions_out,
                               bcmpc_result* d_result, void* stream);

/* CEM, single device, synchronous: all iterations on the engine's stream.
 *   mu, sigma : host [H][A] doubles, in: the initial distribution, out: the refit one
 *   out       : best_index = iteration * K + candidate, best_cost, first action
 * Needs a group-kernel engine with the fused objective (cheetah cost or learned reward;
 * for the reward objective "best" is the argmax). */
int bcmpc_cem_get_action(bcmpc_engine* eng, const double* state, const bcmpc_cem* params, uint64_t seed,
                         double* mu, double* sigma, bcmpc_result* out);

/* CEM building blocks for multi-device runs (device pointers, stream-ordered):
 *   cem_rollout : one iteration's sampling + rollout of this device's shard into d_costs;
 *                 with d_result, also the shard's best, merged (merge != 0) with the
 *                 running best already in d_result
 *   select      : the n_elite lowest of m records -- d_pairs, or d_costs (index =
 *                 index_base + i) when d_pairs is NULL -- written in ascending index
 *                 order to d_out (padded with index -1), the count to d_count
 *   cem_refit   : mu / sigma update from the selected elites (regenerated from Philox) */
int bcmpc_cem_rollout_async(bcmpc_engine* eng, const double* d_state, const double* d_mu, const double* d_sigma,
                            uint64_t seed, int32_t iteration, int64_t cand_offset, int64_t k_global,
                            double* d_costs, bcmpc_result* d_result, int32_t merge, void* stream);
int bcmpc_select_async(bcmpc_engine* eng, const bcmpc_elite* d_pairs, const double* d_costs, int64_t m,
                       int64_t index_base, int32_t n_elite, bcmpc_elite* d_out, int32_t* d_count, void* stream);
int bcmpc_cem_refit_async(bcmpc_engine* eng, const bcmpc_elite* d_elite, const int32_t* d_count, uint64_t seed,
                          int32_t iteration, double alpha, double* d_mu, double* d_sigma, void* stream);

/* MPPI, single device, synchronous: `iterations` rounds of CEM-style rollout + update on the
 * engine's stream, one host synchronisation.
 *   mu    : host [H][A] doubles, in: the sampling mean, out: the updated plan (the action to apply is
 *           mu[0] of the output)
 *   sigma : host [H][A] doubles, the sampling std (read only)
 *   out   : the best single candidate over all rounds (best_index = iteration * K + candidate), as CEM
 *   stats : the last round's update statistics
 * Engines as for bcmpc_cem_get_action; a team-kernel engine whose team gave up reruns the call on its
 * fallback engine.  BCMPC_ERR_ARG: null pointers, iterations outside [1, 2^22], lambda not finite or
 * <= 0, cost == BCMPC_COST_NONE, k_global not 0 / num_paths.  BCMPC_ERR_EMPTY: num_paths == 0.
 * BCMPC_ERR_UNSUPPORTED: engines with a communicator attached, engines with a fused policy. */
int bcmpc_mppi_get_action(bcmpc_engine* eng, const double* state, const bcmpc_mppi* params, uint64_t seed,
                          double* mu, const double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats);

/* The update alone (device pointers, stream-ordered; next to bcmpc_cem_rollout_async, which leaves
 * d_costs): d_costs [m] are the costs of candidates cand_offset + [0, m) sampled at `iteration` from
 * (d_mu, d_sigma); d_mu [H][A] is replaced by the weighted mean (left alone when no cost is finite),
 * d_stats receives the statistics.  m need not equal num_paths: the update uses the engine's H, A,
 * action bounds and objective direction only.  The engine's scratch serves one update at a time:
 * updates of one engine on different streams must be ordered by the caller.
 * BCMPC_ERR_ARG: null pointers, m < 1, iteration outside [0, 2^22), lambda not finite or <= 0. */
int bcmpc_mppi_update_async(bcmpc_engine* eng, const double* d_costs, int64_t m, int64_t cand_offset,
                            uint64_t seed, int32_t iteration, double lambda, double* d_mu,
                            const double* d_sigma, bcmpc_mppi_stats* d_stats, void* stream);

/* Batched CEM and MPPI (additive to ABI 5; callers detect them by the symbol
 * bcmpc_cem_get_actions_batch): n_envs environments per launch chain, K = num_paths / n_envs candidates
 * each, columns as for bcmpc_get_actions_batch (column c = b * K + j belongs to environment b, starts
 * from states[b], Philox index cand_offset + c).  Environment b samples from its own plan mu[b],
 * sigma[b] and gets its own elite set or softmin weights, updated plan, record and statistics.  With
 * off_b = cand_offset + b * K, for every b and iteration `it`:
 *   costs   == bcmpc_cem_rollout_async(states[b], mu_b, sigma_b, seed, it, off_b, ..) of a K-candidate
 *              engine of the same kernel layout, bit for bit
 *   elites  == bcmpc_select_async(costs_b, K, index_base = off_b, n_elite)
 *   CEM     mu_b', sigma_b' == bcmpc_cem_refit_async on those elites
 *   MPPI    mu_b', stats[b] == bcmpc_mppi_update_async(costs_b, K, off_b, seed, it, lambda, ..)
 *   out[b]  np.argmin (np.argmax for BCMPC_COST_REWARD) over environment b's iteration-major
 *           concatenated costs: best_index = it * K + j (environment-local, as the single calls report
 *           it), best_cost, first_action that sample's step-0 action
 * and with n_envs == 1, cand_offset == 0 the call equals bcmpc_cem_get_action / bcmpc_mppi_get_action.
 * The rollout kernels are not told about the plans: each iteration's actions [H][num_paths][A] are
 * written by a sampling kernel (the values the rollout kernels would draw) and rolled out as an
 * explicit action array, so the solo layout works here too.
 *   states    : host [n_envs][S]
 *   mu, sigma : host [n_envs][H][A]; mu in/out; sigma in/out (CEM) or in (MPPI)
 *   params    : n_elite is per environment; k_global is 0 or K
 *   out       : host [n_envs] records;  stats: host [n_envs], the last iteration's
 *   costs_out : optional host [iterations][num_paths]
 * BCMPC_ERR_ARG: null pointers, n_envs < 1, num_paths % n_envs != 0, iterations outside [1, 2^22],
 * n_elite < 1, lambda not finite or <= 0, k_global, cost == BCMPC_COST_NONE.  BCMPC_ERR_UNSUPPORTED:
 * engines with a fused policy, engines with a communicator attached.  BCMPC_ERR_EMPTY: num_paths == 0.
 * A team-kernel engine whose team gave up reruns the whole call on its fallback engine from the
 * original mu / sigma. */
int bcmpc_cem_get_actions_batch(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_cem* params,
                                uint64_t seed, int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out,
                                double* costs_out);
int bcmpc_mppi_get_actions_batch(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_mppi* params,
                                 uint64_t seed, int64_t cand_offset, double* mu, const double* sigma,
                                 bcmpc_result* out, bcmpc_mppi_stats* stats, double* costs_out);

/* The batched planners' building blocks (device pointers, stream-ordered, no host synchronisation).
 * n_envs and K are explicit: only plan_sample's output has to fit a rollout; the others use the
 * engine's H, A, action bounds and objective direction only, so n_envs * K need not be num_paths.
 *   plan_sample  d_actions[h][c][j] (f64 [H][n_envs * K][A]) = the CEM sample of candidate
 *                cand_offset + c at `iteration` from d_mu / d_sigma [n_envs][H][A], plan c / K; roll it
 *                out with bcmpc_rollout_batch_async or bcmpc_rollout_async (state_stride == S)
 *   plan_argmin  environment b's best of d_costs[b * K .. (b + 1) * K) into d_results[b] (best_index =
 *                iteration * K + j, first_action read from d_actions' step 0), merged (merge != 0) with
 *                the running best already there; before the next plan_sample overwrites d_actions
 *   select_batch bcmpc_select_async per environment on costs (index = index_base + b * K + j):
 *                d_out [n_envs][n_elite] in ascending index, padded with index -1; d_count [n_envs]
 *   cem_refit_batch   bcmpc_cem_refit_async per environment: d_elite [n_envs][n_elite], d_count
 *                [n_envs], d_mu / d_sigma [n_envs][H][A] in place
 *   mppi_update_batch bcmpc_mppi_update_async per environment at m = K (its workgroup size rule and
 *                summation order follow K, not n_envs * K): d_costs [n_envs * K], d_mu [n_envs][H][A]
 *                in place, d_sigma read, d_stats [n_envs]; the engine's scratch serves one update at a time
 * d_actions of the refit and the update is optional: the array plan_sample wrote for this iteration
 * ([H][n_envs * K][A], column 0 = candidate cand_offset) is then read instead of regenerating the
 * samples from Philox -- the same bits (NULL: regenerate; K and cand_offset of the refit are then unused).
 * BCMPC_ERR_ARG: null pointers, n_envs < 1, K < 1, n_elite < 1, iteration outside [0, 2^22), lambda.
 * Team-kernel engines: bcmpc_engine_status after the rollout's stream has completed, as always. */
int bcmpc_plan_sample_async(bcmpc_engine* eng, const double* d_mu, const double* d_sigma, int32_t n_envs, int64_t K,
                            uint64_t seed, int32_t iteration, int64_t cand_offset, double* d_actions, void* stream);
int bcmpc_plan_argmin_async(bcmpc_engine* eng, const double* d_costs, const double* d_actions, int32_t n_envs,
                            int64_t K, int32_t iteration, int32_t merge, bcmpc_result* d_results, void* stream);
int bcmpc_select_batch_async(bcmpc_engine* eng, const double* d_costs, int32_t n_envs, int64_t K, int64_t index_base,
                             int32_t n_elite, bcmpc_elite* d_out, int32_t* d_count, void* stream);
int bcmpc_cem_refit_batch_async(bcmpc_engine* eng, const bcmpc_elite* d_elite, const int32_t* d_count, int32_t n_envs,
                                int32_t n_elite, uint64_t seed, int32_t iteration, double alpha, double* d_mu,
                                double* d_sigma, const double* d_actions, int64_t K, int64_t cand_offset,
                                void* stream);
int bcmpc_mppi_update_batch_async(bcmpc_engine* eng, const double* d_costs, int32_t n_envs, int64_t K,
                                  int64_t cand_offset, uint64_t seed, int32_t iteration, double lambda, double* d_mu,
                                  const double* d_sigma, bcmpc_mppi_stats* d_stats, const double* d_actions,
                                  void* stream);

/* ------------------------------------------------------------------------
 * The planners' sampling distribution (additive to ABI 5; callers detect it by the symbol
 * bcmpc_cem_get_action_s; semantics in DESIGN.md 9j, defined bit for bit by bc_mpc_amd/sampling.py).
 *   rho          temporally correlated noise: candidate g's action (h, j) of an iteration is
 *                clip(mu[h][j] + sigma[h][j] * n[h]) with n[0] = z[0], n[h] = rho * n[h-1] + c * z[h],
 *                c = sqrt(1 - rho * rho) (f64, rounded once), z[h] the independent normal the planners draw
 *                at (seed, g, h, j, iteration); every product and sum an individually rounded f64 operation.
 *                The variance of n[h] is 1 for every h.  0 <= rho < 1; rho == 0: the independent draw.
 *   keep_elites  (CEM) iteration it >= 1 of an environment starts with ALL elites of iteration it - 1: its
 *                candidate column j < count is the sequence of the j-th elite (select's order: ascending
 *                index), columns j >= count are sampled as ever at their own Philox index.  The best
 *                sequence of an iteration therefore survives, and the per-iteration minimum does not rise.
 *                Nothing is carried from one call to the next.
 * A NULL pointer or {0, 0, 0} is the default and runs exactly what the calls without _s run.  Anything else
 * runs the batched chain (n_envs = 1, cand_offset = 0 for the single calls): plan_sample_corr instead of
 * plan_sample and, with keep_elites, plan_keep behind every refit that another iteration follows.
 * BCMPC_ERR_ARG (before any HIP call): rho not finite or outside [0, 1), keep_elites not 0 / 1, keep_elites on
 * an MPPI call, and what the calls without _s refuse.  BCMPC_ERR_UNSUPPORTED: a communicator attached, a fused
 * policy.  Ensembles have no _s entry. */
typedef struct bcmpc_sampling {
    double rho;
    int32_t keep_elites;
    int32_t reserved;
} bcmpc_sampling;

int bcmpc_cem_get_action_s(bcmpc_engine* eng, const double* state, const bcmpc_cem* params,
                           const bcmpc_sampling* sampling, uint64_t seed, double* mu, double* sigma,
                           bcmpc_result* out);
int bcmpc_mppi_get_action_s(bcmpc_engine* eng, const double* state, const bcmpc_mppi* params,
                            const bcmpc_sampling* sampling, uint64_t seed, double* mu, const double* sigma,
                            bcmpc_result* out, bcmpc_mppi_stats* stats);
int bcmpc_cem_get_actions_batch_s(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_cem* params,
                                  const bcmpc_sampling* sampling, uint64_t seed, int64_t cand_offset, double* mu,
                                  double* sigma, bcmpc_result* out, double* costs_out);
int bcmpc_mppi_get_actions_batch_s(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_mppi* params,
                                   const bcmpc_sampling* sampling, uint64_t seed, int64_t cand_offset, double* mu,
                                   const double* sigma, bcmpc_result* out, bcmpc_mppi_stats* stats,
                                   double* costs_out);

/* Their building blocks (device pointers, stream-ordered, as bcmpc_plan_sample_async and its siblings).
 *   plan_sample_corr  bcmpc_plan_sample_async with the correlated noise above.  d_keep [n_envs][n_elite][H][A]
 *                and d_keep_count [n_envs] (both, or both NULL; n_elite is d_keep's stride and unused without
 *                it): environment b's first min(d_keep_count[b], n_elite) columns are copied from d_keep[b]
 *                and draw nothing.
 *   plan_keep    d_keep[b][e][h][j] = d_actions[h][d_elite[b][e].index - cand_offset][j] for e < d_count[b]
 *                (d_elite [n_envs][n_elite], d_count [n_envs]: bcmpc_select_batch_async's output on the costs of
 *                d_actions, [H][n_envs * K][A]).  A record with index < 0 or a column outside environment b's
 *                own K columns is not copied; d_keep_count[b] counts the leading records that were.  It runs
 *                after the refit and before the next sampling overwrites d_actions.
 * With correlated noise or carried elites, bcmpc_cem_refit_batch_async and bcmpc_mppi_update_batch_async MUST
 * be given d_actions: their Philox fallback regenerates the independent draw, not what was rolled out. */
int bcmpc_plan_sample_corr_async(bcmpc_engine* eng, const double* d_mu, const double* d_sigma, int32_t n_envs,
                                 int64_t K, uint64_t seed, int32_t iteration, int64_t cand_offset, double rho,
                                 const double* d_keep, const int32_t* d_keep_count, int32_t n_elite,
                                 double* d_actions, void* stream);
int bcmpc_plan_keep_async(bcmpc_engine* eng, const bcmpc_elite* d_elite, const int32_t* d_count,
                          const double* d_actions, int32_t n_envs, int64_t K, int64_t cand_offset, int32_t n_elite,
                          double* d_keep, int32_t* d_keep_count, void* stream);

/* ------------------------------------------------------------------------
 * MPPI's control-cost term and a weighted sigma update (additive to ABI 5; callers detect them by the symbol
 * bcmpc_mppi_get_action_x; semantics in DESIGN.md 9l, defined by bc_mpc_amd/mppi_update.py).  One round with the
 * options on, (mu, sigma) the plan it samples from:
 *   record   the argmin runs over the RAW costs: best_cost, best_index and costs_out never hold the control cost
 *   scores   c~[k] = cost[k] + control_weight * q[k] (BCMPC_COST_REWARD: cost[k] - control_weight * q[k]) with
 *            q[k] = sum_h sum_j g[h][j] * (a[h][k][j] - mu[h][j]), g = mu / (sigma * sigma), 0 where sigma == 0;
 *            a: the clipped sampled actions.  From 0.0, h ascending and j inside it, every operation an
 *            individually rounded f64 one.  Under correlated noise this is the diagonal (marginal-variance)
 *            form of Sigma^-1.  control_weight == 0: no launch, the scores are the costs
 *   update   mu', stats == bcmpc_mppi_update_batch_async on c~, bit for bit -- stats.min_cost is therefore the
 *            minimum AUGMENTED score
 *   sigma    (adapt_sigma) sigma' = min(max(sigma_alpha * sigma + (1 - sigma_alpha) * s, min_std), max_std),
 *            s[h][j] = sqrt(sum_k w[k] (a[h][k][j] - mu'[h][j])^2 / sum_k w[k]) with the update's weights w; no
 *            valid candidate: sigma unchanged, as mu.  The next round samples from (mu', sigma').
 * A NULL ext or one with control_weight == 0 and adapt_sigma == 0 forwards to the _s entry point: today's call,
 * bit for bit.  Anything else runs the batched chain (n_envs = 1, cand_offset = 0 for the single call) with the
 * control-cost launch before every update and the sigma launches behind it.
 *   sigma : host [n_envs][H][A] (single call: [H][A]); read, and written back only when adapt_sigma is set
 * BCMPC_ERR_ARG (before any HIP call): control_weight negative or not finite, adapt_sigma not 0 / 1, reserved
 * not zero, sigma_alpha outside [0, 1], min_std negative or not finite, max_std < min_std (or NaN), and what the
 * _s calls refuse.  BCMPC_ERR_UNSUPPORTED: a communicator attached, a fused policy, horizon * action_dim > 4096
 * (the control-cost kernel's table).  Ensembles have no _x entry. */
typedef struct bcmpc_mppi_ext {
    double  control_weight;  /* >= 0, finite; 0: off */
    int32_t adapt_sigma;     /* 0 | 1 */
    int32_t reserved;        /* must be zero */
    double  sigma_alpha;     /* in [0, 1] */
    double  min_std;         /* >= 0 */
    double  max_std;         /* >= min_std, +inf allowed */
} bcmpc_mppi_ext;

int bcmpc_mppi_get_action_x(bcmpc_engine* eng, const double* state, const bcmpc_mppi* params,
                            const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext, uint64_t seed, double* mu,
                            double* sigma /* in/out */, bcmpc_result* out, bcmpc_mppi_stats* stats);
int bcmpc_mppi_get_actions_batch_x(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_mppi* params,
                                   const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext, uint64_t seed,
                                   int64_t cand_offset, double* mu, double* sigma /* in/out */, bcmpc_result* out,
                                   bcmpc_mppi_stats* stats, double* costs_out);

/* Their building blocks (device pointers, stream-ordered, as bcmpc_plan_sample_async and its siblings; n_envs and K
 * are explicit, the engine gives H, A and the objective's direction).  d_actions is the iteration's stored array
 * [H][n_envs * K][A] and is required: there is no Philox form.
 *   control_cost  d_scores[c] = c~ of column c from d_costs [n_envs * K] and the plans d_mu / d_sigma
 *                 [n_envs][H][A] the actions were sampled from; d_scores may be d_costs itself (every thread
 *                 reads and writes its own entry) and may overlap it in no other way
 *   sigma_update  d_sigma [n_envs][H][A] in place from the weights of d_scores (the vector the update ran on)
 *                 about d_mu_new, the UPDATED plans.  Self-contained: it recomputes v_min, the count and W as the
 *                 update does and relies on no scratch of an earlier call; the engine's scratch serves one update
 *                 or sigma update at a time.
 * BCMPC_ERR_ARG: null pointers, n_envs < 1, K < 1, weight, lambda, sigma_alpha / min_std / max_std as above. */
int bcmpc_mppi_control_cost_async(bcmpc_engine* eng, const double* d_costs, const double* d_actions, int32_t n_envs,
                                  int64_t K, const double* d_mu, const double* d_sigma, double weight,
                                  double* d_scores, void* stream);
int bcmpc_mppi_sigma_update_async(bcmpc_engine* eng, const double* d_scores, const double* d_actions, int32_t n_envs,
                                  int64_t K, double lambda, const double* d_mu_new, double* d_sigma, double alpha,
                                  double min_std, double max_std, void* stream);

/* ------------------------------------------------------------------------
 * Proposals: given action sequences in every iteration's population (additive to ABI 5; callers detect them by the
 * symbol bcmpc_cem_get_action_p; semantics in DESIGN.md 9m, defined bit for bit by bc_mpc_amd/proposals.py).
 * A call carries count = P >= 1 sequences [H][A] per environment.  In EVERY iteration environment b's population is
 * the one the call would have had, with its LAST P columns replaced: column K - P + p at (h, j) holds
 *   v = sequences[b * env_stride + p * seq_stride + h * step_stride + j];  v < low[j] ? low[j] : (v > high[j] ? high[j] : v)
 * -- the samplers' own clip: a NaN stays NaN (last in select, no weight in MPPI), -0.0 against a bound of 0.0 stays
 * -0.0.  The replaced columns' Philox draws are unused and no index shifts: every other column holds today's bits.
 * Carried elites keep the FIRST columns: P + n_elite <= K with keep_elites, P <= K otherwise (P == K: nothing is
 * sampled).  Everything downstream reads the stored array, as under rho: the record (best_index = iteration * K +
 * column may name a proposal column, first_action is then the stored, clipped one), select, the refit, plan_keep, the
 * MPPI update, the control cost and the sigma update.  In MPPI a proposal is not a draw from N(mu, sigma): its
 * softmin weight and its control-cost term (eps = a - mu) are the heuristic TD-MPC uses.  Nothing is carried
 * between calls.
 *   device == 0  sequences is host memory in the canonical layout [n_envs][P][H][A], uploaded with the plans; the
 *                strides are all 0 or the canonical (P * H * A, H * A, A)
 *   device == 1  sequences is device memory, read in the engine's stream order through the three element strides
 *                (in doubles; j has stride 1): the canonical layout, or (P * A, A, n_envs * P * A) for the policy
 *                engines' output [H][n_envs * P][A] (bcmpc_rollout_policy_batch_async).  The strides are >= 0 and,
 *                taken from the smallest to the largest over the dimensions of extent > 1, each is at least the
 *                extent it steps over (A, then stride * extent of the one before): no two elements alias.
 * A NULL pointer or count == 0 forwards to the _s / _x entry: today's call, bit for bit.  Anything else runs the
 * batched chain (n_envs = 1, cand_offset = 0 for the single calls) with plan_sample_prop as its sampler -- one
 * sampler launch per iteration, as ever; at rho == 0 the sampled columns hold plan_sample's bits.  A team-kernel
 * engine whose team gave up reruns the whole call, proposals included, on its fallback engine.
 * BCMPC_ERR_ARG (before any HIP call): count < 0 or beyond the limits above, NULL sequences, device not 0 / 1,
 * strides that alias (or, on the host, are not canonical), and what the _s / _x calls refuse.
 * BCMPC_ERR_UNSUPPORTED: a communicator attached, a fused policy on the planning engine.  Ensembles have no _p
 * entry. */
typedef struct bcmpc_proposals {
    const double* sequences;
    int32_t count;           /* P: sequences per environment; 0: none */
    int32_t device;          /* 0: host memory, canonical | 1: device memory */
    int64_t env_stride;      /* in doubles */
    int64_t seq_stride;
    int64_t step_stride;
} bcmpc_proposals;

int bcmpc_cem_get_action_p(bcmpc_engine* eng, const double* state, const bcmpc_cem* params,
                           const bcmpc_sampling* sampling, const bcmpc_proposals* proposals, uint64_t seed,
                           double* mu, double* sigma, bcmpc_result* out);
int bcmpc_mppi_get_action_p(bcmpc_engine* eng, const double* state, const bcmpc_mppi* params,
                            const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext,
                            const bcmpc_proposals* proposals, uint64_t seed, double* mu, double* sigma /* in/out */,
                            bcmpc_result* out, bcmpc_mppi_stats* stats);
int bcmpc_cem_get_actions_batch_p(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_cem* params,
                                  const bcmpc_sampling* sampling, const bcmpc_proposals* proposals, uint64_t seed,
                                  int64_t cand_offset, double* mu, double* sigma, bcmpc_result* out,
                                  double* costs_out);
int bcmpc_mppi_get_actions_batch_p(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_mppi* params,
                                   const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext,
                                   const bcmpc_proposals* proposals, uint64_t seed, int64_t cand_offset, double* mu,
                                   double* sigma /* in/out */, bcmpc_result* out, bcmpc_mppi_stats* stats,
                                   double* costs_out);

/* Their building blocks (device pointers, stream-ordered, no host synchronisation).
 *   plan_sample_prop      bcmpc_plan_sample_corr_async plus the proposal columns: d_proposals, n_prop (1 <= n_prop <=
 *                K, n_prop + n_elite <= K with a keep buffer) and the three strides, as device == 1 above.  The
 *                source is read only.
 *   rollout_policy_batch  bcmpc_rollout_policy_async with one start state per environment: d_states [n_envs][S],
 *                num_paths % n_envs == 0, environment b owns columns [b * K, (b + 1) * K), K = num_paths / n_envs,
 *                and every one of them starts from d_states[b] (the states are tiled, then rolled out with a state
 *                stride of S -- no kernel differs).  d_actions_out [H][num_paths][A] is then the source layout
 *                (P * A, A, n_envs * P * A) with P = K.  n_envs == 1 gives bcmpc_rollout_policy_async's bits.
 *                Team-kernel engines: bcmpc_engine_status once the stream has completed, as always. */
int bcmpc_plan_sample_prop_async(bcmpc_engine* eng, const double* d_mu, const double* d_sigma, int32_t n_envs,
                                 int64_t K, uint64_t seed, int32_t iteration, int64_t cand_offset, double rho,
                                 const double* d_keep, const int32_t* d_keep_count, int32_t n_elite,
                                 const double* d_proposals, int32_t n_prop, int64_t env_stride, int64_t seq_stride,
                                 int64_t step_stride, double* d_actions, void* stream);
int bcmpc_rollout_policy_batch_async(bcmpc_engine* eng, const double* d_states, int32_t n_envs,
                                     const double* d_actions, uint64_t seed, int64_t cand_offset, double* d_costs,
                                     double* d_traj, double* d_actions_out, void* stream);

/* ------------------------------------------------------------------------
 * Knot plans: the planners sample M <= H knots per action dimension and interpolate them to the H steps (additive to
 * ABI 5; callers detect them by the symbol bcmpc_cem_get_action_k; semantics in DESIGN.md 9n, defined bit for bit by
 * bc_mpc_amd/knots.py).  The search runs in M * A dimensions, every candidate is smooth by construction, and the plans
 * a call reads and writes are in knot space:
 *   mu / sigma : host [n_envs][M][A] (single calls: [M][A]) with M = knots->count
 *   knot m of candidate g   clip(mu[m][j] + sigma[m][j] * n[m]): the planners' own normal at (seed, g, m, j, iteration)
 *                -- the knot index in the place of h -- with the AR(1) recursion of bcmpc_sampling.rho over the knots
 *   step h       kind 0 (hold): knot (h * M) / H (integer division; action repeat).  Kinds 1 (linear) and 2 (cubic,
 *                Catmull-Rom with the end knots repeated): the knots sit at both ends of the horizon; with
 *                m0 = h * (M - 1) / (H - 1), r the remainder (both 0 when H == 1 or M == 1), r == 0 gives knot m0
 *                untouched, else f = (double)r / (double)(H - 1) and the formulas of knots.py, every operation an
 *                individually rounded f64 one.  Every step's value is clipped to the action box again (the cubic
 *                overshoots).
 *   refit / update   select, the CEM refit, the MPPI update, the control cost, the sigma update and the elite carry-over
 *                run on the clipped KNOT values: the existing kernels launched with the step count M on the knot array
 *                [M][n_envs * K][A].  The rollout and the record read the expanded array [H][n_envs * K][A]; no rollout
 *                kernel differs.  MPPI's answer stays mu'[0]: knot 0 sits at step 0 in all three kinds.
 * The _k entry points take every option of the _p entry points plus the knots.  A NULL knots or count == 0 forwards
 * to the _p entry point: today's call, bit for bit.  Anything else -- count == H included -- runs the batched chain
 * (n_envs = 1, cand_offset = 0 for the single calls) with plan_sample_knots as its sampler.
 * BCMPC_ERR_ARG (before any HIP call): count outside [1, horizon], an unknown kind, and what the _s / _x calls refuse.
 * BCMPC_ERR_UNSUPPORTED: knots together with proposals (count != 0) -- a given action sequence has no knot
 * representation to refit on --, a communicator attached, a fused policy.  Ensembles have no _k entry. */
#define BCMPC_KNOTS_HOLD   0
#define BCMPC_KNOTS_LINEAR 1
#define BCMPC_KNOTS_CUBIC  2
typedef struct bcmpc_knots {
    int32_t count;           /* M: knots per action dimension, 1 <= M <= horizon; 0: off */
    int32_t kind;            /* BCMPC_KNOTS_HOLD | _LINEAR | _CUBIC */
} bcmpc_knots;

int bcmpc_cem_get_action_k(bcmpc_engine* eng, const double* state, const bcmpc_cem* params,
                           const bcmpc_sampling* sampling, const bcmpc_proposals* proposals, const bcmpc_knots* knots,
                           uint64_t seed, double* mu, double* sigma, bcmpc_result* out);
int bcmpc_mppi_get_action_k(bcmpc_engine* eng, const double* state, const bcmpc_mppi* params,
                            const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext,
                            const bcmpc_proposals* proposals, const bcmpc_knots* knots, uint64_t seed, double* mu,
                            double* sigma /* in/out */, bcmpc_result* out, bcmpc_mppi_stats* stats);
int bcmpc_cem_get_actions_batch_k(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_cem* params,
                                  const bcmpc_sampling* sampling, const bcmpc_proposals* proposals,
                                  const bcmpc_knots* knots, uint64_t seed, int64_t cand_offset, double* mu,
                                  double* sigma, bcmpc_result* out, double* costs_out);
int bcmpc_mppi_get_actions_batch_k(bcmpc_engine* eng, const double* states, int32_t n_envs, const bcmpc_mppi* params,
                                   const bcmpc_sampling* sampling, const bcmpc_mppi_ext* ext,
                                   const bcmpc_proposals* proposals, const bcmpc_knots* knots, uint64_t seed,
                                   int64_t cand_offset, double* mu, double* sigma /* in/out */, bcmpc_result* out,
                                   bcmpc_mppi_stats* stats, double* costs_out);

/* Their building blocks (device pointers, stream-ordered, no host synchronisation).
 *   plan_sample_knots  bcmpc_plan_sample_corr_async in knot space: d_mu / d_sigma [n_envs][M][A], d_keep
 *                [n_envs][n_elite][M][A]; it writes d_knots [M][n_envs * K][A] (the clipped knot values) and d_actions
 *                [H][n_envs * K][A] (their expansion).  M == H: d_actions holds plan_sample_corr's bits.
 *   *_steps      bcmpc_cem_refit_batch_async, bcmpc_mppi_update_batch_async, bcmpc_plan_keep_async,
 *                bcmpc_mppi_control_cost_async and bcmpc_mppi_sigma_update_async with the step count given instead of
 *                taken from the engine's horizon (1 <= steps <= horizon): d_actions is [steps][n_envs * K][A], the
 *                plans [n_envs][steps][A], d_keep [n_envs][n_elite][steps][A].  steps == horizon: the call without
 *                the suffix.  The refit and the update need d_actions here: their Philox form regenerates a full-length
 *                independent draw, which is not what a knot array holds. */
int bcmpc_plan_sample_knots_async(bcmpc_engine* eng, const double* d_mu, const double* d_sigma, int32_t n_envs,
                                  int64_t K, uint64_t seed, int32_t iteration, int64_t cand_offset, double rho,
                                  const double* d_keep, const int32_t* d_keep_count, int32_t n_elite, int32_t knots,
                                  int32_t kind, double* d_knots, double* d_actions, void* stream);
int bcmpc_cem_refit_batch_steps_async(bcmpc_engine* eng, const bcmpc_elite* d_elite, const int32_t* d_count,
                                      int32_t n_envs, int32_t n_elite, uint64_t seed, int32_t iteration, double alpha,
                                      double* d_mu, double* d_sigma, const double* d_actions, int64_t K,
                                      int64_t cand_offset, int32_t steps, void* stream);
int bcmpc_mppi_update_batch_steps_async(bcmpc_engine* eng, const double* d_costs, int32_t n_envs, int64_t K,
                                        int64_t cand_offset, uint64_t seed, int32_t iteration, double lambda,
                                        double* d_mu, const double* d_sigma, bcmpc_mppi_stats* d_stats,
                                        const double* d_actions, int32_t steps, void* stream);
int bcmpc_plan_keep_steps_async(bcmpc_engine* eng, const bcmpc_elite* d_elite, const int32_t* d_count,
                                const double* d_actions, int32_t n_envs, int64_t K, int64_t cand_offset,
                                int32_t n_elite, double* d_keep, int32_t* d_keep_count, int32_t steps, void* stream);
int bcmpc_mppi_control_cost_steps_async(bcmpc_engine* eng, const double* d_costs, const double* d_actions,
                                        int32_t n_envs, int64_t K, const double* d_mu, const double* d_sigma,
                                        double weight, double* d_scores, int32_t steps, void* stream);
int bcmpc_mppi_sigma_update_steps_async(bcmpc_engine* eng, const double* d_scores, const double* d_actions,
                                        int32_t n_envs, int64_t K, double lambda, const double* d_mu_new,
                                        double* d_sigma, double alpha, double min_std, double max_std, int32_t steps,
                                        void* stream);

/* ------------------------------------------------------------------------
 * Model ensembles (additive to ABI 5; callers detect them by the symbol bcmpc_ensemble_create; not in
 * the reference, semantics in DESIGN.md 9g).  An ensemble holds E dynamics nets of one architecture and
 * one configuration -- E member engines of the same config, hence the same kernel layout.  Candidate k
 * of a call has ONE action sequence (the explicit array's column, the Philox draw at cand_offset + k, or
 * the CEM / MPPI sample at that index); member e scores it as c[e][k], bit for bit what a single engine
 * holding member e's weights returns; the candidate's value is
 *   MEAN      t = c[0]; for e = 1..E-1: t = t + c[e]; v = t / E
 *   MEAN_STD  m as above; q = 0.0; for e = 0..E-1: d = c[e] - m; q = q + d * d; v = m + kappa * sqrt(q / E)
 *   WORST     np.maximum.reduce(c): the largest member cost, NaN if any member's is NaN
 * every operation an individually rounded IEEE f64 operation (no contraction; division and square root
 * correctly rounded).  MEAN starts from c[0]: E == 1 returns c[0]'s bits.  The argmin, CEM's elite
 * selection and refit and the MPPI update then run on v with the rules they have on a single engine's
 * costs (a NaN value wins the argmin).
 * Launch order: everything on member 0's stream -- per iteration the members' rollouts in member order,
 * each into its row of an ensemble-owned [E][num_paths] buffer (allocated at create), the reduce into
 * member 0's cost vector, the ordinary argmin, then select + refit or the MPPI update.  Members never run
 * concurrently.  One host synchronisation per call.  Team-kernel members: if any member's team gave up,
 * the whole call reruns on the members' fallback engines from the saved inputs (the answer is then that
 * of an ensemble of the fallback layout).
 * Not covered: a fused policy, the reward model / BCMPC_COST_REWARD, BCMPC_COST_NONE (create returns
 * BCMPC_ERR_UNSUPPORTED); batched CEM / MPPI; members with a communicator attached (refused at call time). */
#define BCMPC_MAX_MEMBERS 16
typedef enum bcmpc_ensemble_mode {
    BCMPC_ENSEMBLE_MEAN = 0,
    BCMPC_ENSEMBLE_MEAN_STD = 1,
    BCMPC_ENSEMBLE_WORST = 2
} bcmpc_ensemble_mode;

typedef struct bcmpc_ensemble bcmpc_ensemble;

/* 1 <= n_members <= BCMPC_MAX_MEMBERS, else BCMPC_ERR_ARG (checked before any HIP call). */
int bcmpc_ensemble_create(const bcmpc_config* cfg, int32_t n_members, bcmpc_ensemble** out);
int bcmpc_ensemble_destroy(bcmpc_ensemble* ens);
int bcmpc_ensemble_size(const bcmpc_ensemble* ens);   /* E, or 0 for NULL */
/* Member i, lent out (owned by the ensemble) for bcmpc_set_weights, bcmpc_set_cost_terms,
 * bcmpc_set_action_bounds, bcmpc_engine_info, bcmpc_engine_layout, bcmpc_engine_team_reruns. */
int bcmpc_ensemble_member(bcmpc_ensemble* ens, int32_t i, bcmpc_engine** out);
/* The rule of the following calls (default MEAN, kappa 0).  BCMPC_ERR_ARG: unknown mode, kappa not finite. */
int bcmpc_ensemble_set_rule(bcmpc_ensemble* ens, int32_t mode, double kappa);

/* bcmpc_get_action over the ensemble.  costs_out: optional [K] values v; member_costs_out: optional
 * [E][K] member costs.  out->best_cost is v[best]. */
int bcmpc_ensemble_get_action(bcmpc_ensemble* ens, const double* state, const double* actions, uint64_t seed,
                              int64_t cand_offset, bcmpc_result* out, double* costs_out, double* member_costs_out);
/* bcmpc_get_actions_batch over the ensemble (segment layout as there): costs_out [num_paths] values,
 * member_costs_out [E][num_paths]. */
int bcmpc_ensemble_get_actions_batch(bcmpc_ensemble* ens, const double* states, int32_t n_envs,
                                     const double* actions, uint64_t seed, int64_t cand_offset, bcmpc_result* out,
                                     double* costs_out, double* member_costs_out);
/* bcmpc_cem_get_action / bcmpc_mppi_get_action over the ensemble: every iteration's elites / weights
 * come from v. */
int bcmpc_ensemble_cem_get_action(bcmpc_ensemble* ens, const double* state, const bcmpc_cem* params, uint64_t seed,
                                  double* mu, double* sigma, bcmpc_result* out);
int bcmpc_ensemble_mppi_get_action(bcmpc_ensemble* ens, const double* state, const bcmpc_mppi* params,
                                   uint64_t seed, double* mu, const double* sigma, bcmpc_result* out,
                                   bcmpc_mppi_stats* stats);
/* The reduce alone (device pointers, stream-ordered, allocates nothing; `eng` names the device):
 * d_member_costs [n_members][ld] (ld >= K), d_out [K].  BCMPC_ERR_ARG: null pointers, n_members outside
 * [1, BCMPC_MAX_MEMBERS], K < 1, ld < K, unknown mode, kappa not finite. */
int bcmpc_ensemble_reduce_async(bcmpc_engine* eng, const double* d_member_costs, int64_t ld, int32_t n_members,
                                int64_t K, int32_t mode, double kappa, double* d_out, void* stream);

/* ------------------------------------------------------------------------
 * NNDynamicsModel.fit (dynamics.py:81-104) on the GPU:
 * `iterations` Adam steps (TF1 AdamOptimizer, dynamics.py:50-52) on the mean
 * squared error of the normalised state deltas, batches gathered on the device
 * from a resident copy of the model data buffer by host-chosen row indices (the
 * caller draws them exactly as DataBufferGeneral.sample does, data_buffer.py:45-57).
 * A fitter owns the f32 parameters and the Adam slots (m, v, beta powers), which
 * persist across runs like the reference's optimizer variables. */
typedef struct bcmpc_fit_config {
    int32_t state_dim;     /* S */
    int32_t action_dim;    /* A */
    int32_t hidden;        /* h (true width, no padding) */
    int32_t n_layers;      /* L */
    int32_t activation;    /* bcmpc_activation */
    int32_t layer_norm;    /* FLAGS.LAYER_NORM (dynamics.py:68) */
    int32_t batch_size;    /* dynamics.py:48 batch_size (max rows per step) */
    int32_t device;
    float learning_rate;   /* dynamics.py:47 */
    float beta1, beta2, epsilon;   /* tf.train.AdamOptimizer defaults 0.9, 0.999, 1e-8 */
    int32_t model;         /* bcmpc_model: BCMPC_MODEL_REWARD fits NNDynamicsRewardModel (dynamics.py:153-160,
                              195-219: loss_dynamic + loss_reward over the two-head net; n_layers 2, tanh;
                              kernels / biases dense .. dense_4, LayerNorm trunk / delta / reward) */
} bcmpc_fit_config;

typedef struct bcmpc_fitter bcmpc_fitter;

int bcmpc_fit_create(const bcmpc_fit_config* cfg, bcmpc_fitter** out);
int bcmpc_fit_destroy(bcmpc_fitter* f);
/* 1: the fused two-launch step (fit_rows_kernel + fit_params_kernel); 0: the per-op kernels (the reward
 * model, BCMPC_FIT_FUSED=0, or a net whose row block does not fit the LDS).  Additive to ABI 5. */
int bcmpc_fit_is_fused(const bcmpc_fitter* f);
/* parameters (TF layout [in, out] kernels, biases, LN gamma/beta) + the normalization stats */
int bcmpc_fit_set_params(bcmpc_fitter* f, const bcmpc_weights* w);
int bcmpc_fit_get_params(bcmpc_fitter* f, float* const* kernels, float* const* biases, float* const* ln_gamma,
                         float* const* ln_beta);
/* the model data buffer: n rows of state (S), action (A), state delta (S), f64, uploaded to HBM */
int bcmpc_fit_set_data(bcmpc_fitter* f, const double* states, const double* actions, const double* deltas,
                       int64_t n);
/* `iterations` steps; step i uses batch_sizes[i] rows, indices concatenated in `indices`;
 * losses (optional, host, [iterations]) = each step's loss before its update */
int bcmpc_fit_run(bcmpc_fitter* f, const int64_t* indices, const int32_t* batch_sizes, int32_t iterations,
                  float* losses);
/* reward model: the buffer's rewards (one f64 per row of bcmpc_fit_set_data; normalised with
 * mean_reward / std_reward of bcmpc_fit_set_params, dynamics.py:203); after a run, its per-step
 * reward losses ([iterations], before each update; bcmpc_fit_run's losses are the dynamics losses) */
int bcmpc_fit_set_rewards(bcmpc_fitter* f, const double* rewards, int64_t n);
int bcmpc_fit_reward_losses(bcmpc_fitter* f, float* losses);
const char* bcmpc_fit_last_error(void);

/* ------------------------------------------------------------------------
 * Actor-critic fitting (bc_mpc_amd/ac_fit.py is the definition): Adam steps on one head of the reference's
 * MlpPolicy -- BCMPC_ACFIT_POLICY: the BC distillation loss sqrt(mean((ac - ac_mean(ob))^2))
 * (ppo_bc_policy.py:114, update_op_bc); BCMPC_ACFIT_VALUE: the critic regression mean((vpred - ret)^2)
 * (ppo_bc_policy.py:108) -- over a tanh stack [S -> hidden x L -> out] behind the observation filter
 * obz = clip((f32(ob) - ob_mean) / ob_std, -5, 5).  A fitter owns the head's f32 parameters, its Adam slots and
 * beta powers (they persist across runs like update_op_bc's optimizer variables), the filter and a copy of the
 * data.  Two launches per step (csrc/ac_fit.hip); a run of equal batch sizes replays one captured graph.
 * Additive to ABI 5: callers detect the feature by the symbols.
 *
 * bcmpc_acfit_create refuses, before any HIP call (csrc/ac_fit_plan.cpp), with BCMPC_ERR_UNSUPPORTED: n_layers
 * outside [1, 4], hidden outside [1, 256], state_dim outside [1, 32], a policy head's out_dim outside [1, 16], a
 * value head's out_dim != 1; with BCMPC_ERR_ARG: null pointers, a head other than the two, batch_size < 1, betas
 * outside [0, 1), epsilon negative or not finite. */
enum { BCMPC_ACFIT_POLICY = 0, BCMPC_ACFIT_VALUE = 1 };
#define BCMPC_ACFIT_MAX_LAYERS 4
#define BCMPC_ACFIT_MAX_HIDDEN 256
typedef struct bcmpc_acfit_config {
    int32_t state_dim;     /* S */
    int32_t out_dim;       /* A (policy head) or 1 (value head) */
    int32_t hidden;        /* true width, no padding */
    int32_t n_layers;      /* L hidden layers */
    int32_t head;          /* BCMPC_ACFIT_POLICY / BCMPC_ACFIT_VALUE */
    int32_t batch_size;    /* rows per step the buffers are first sized for (a larger batch grows them) */
    int32_t device;
    float beta1, beta2, epsilon;   /* tf.train.AdamOptimizer defaults 0.9, 0.999, 1e-8 */
} bcmpc_acfit_config;

typedef struct bcmpc_acfit bcmpc_acfit;

int bcmpc_acfit_create(const bcmpc_acfit_config* cfg, bcmpc_acfit** out);
int bcmpc_acfit_destroy(bcmpc_acfit* f);
/* L + 1 kernels (TF layout [in, out]) and biases; the Adam slots and beta powers are kept */
int bcmpc_acfit_set_params(bcmpc_acfit* f, const float* const* kernels, const float* const* biases);
int bcmpc_acfit_get_params(bcmpc_acfit* f, float* const* kernels, float* const* biases);
/* the observation filter's f32 mean / std [S] (std > 0, both finite: else BCMPC_ERR_ARG) */
int bcmpc_acfit_set_filter(bcmpc_acfit* f, const float* ob_mean, const float* ob_std);
/* n rows of observations [n][S] and targets [n][out_dim] (actions / returns), f64, copied to the device */
int bcmpc_acfit_set_data(bcmpc_acfit* f, const double* obs, const double* targets, int64_t n);
/* `iterations` Adam steps at `learning_rate` (read from device memory by the kernels: a new rate needs no new
 * graph); step i uses batch_sizes[i] rows, their indices concatenated in `indices`; losses (optional, host,
 * [iterations]) = each step's loss before its update.  BCMPC_ERR_ARG: a batch size < 1, an index outside the
 * data, a learning rate that is not finite.  BCMPC_ERR_STATE: parameters, filter or data not set. */
int bcmpc_acfit_run(bcmpc_acfit* f, const int64_t* indices, const int32_t* batch_sizes, int32_t iterations,
                    float learning_rate, float* losses);
/* 0: the last run launched its steps one by one (ragged batches, BCMPC_ACFIT_GRAPH=0); n >= 1: it replayed a
 * captured graph, the n-th this fitter has captured (a new capture: another step count or batch size, an index,
 * loss or data buffer that moved) */
int bcmpc_acfit_is_graph(const bcmpc_acfit* f);
/* f32 words of LDS of the row kernel for a net shape, or -1 where bcmpc_acfit_create refuses it.  No device call. */
int64_t bcmpc_acfit_lds_words(int32_t hidden, int32_t n_layers, int32_t state_dim, int32_t out_dim, int32_t head);
const char* bcmpc_acfit_last_error(void);

/* ------------------------------------------------------------------------
 * PPO on the actor-critic (bc_mpc_amd/ppo.py is the definition): the reference's lossandupdate_ppo
 * (ppo_bc_policy.py:90-144), one Adam step on pol_surr + pol_entpen + vf_loss over pol/, vf/ and logstd against a
 * frozen old policy.  A trainer is built OVER a policy and a value fitter: it trains in place on their device
 * weights (and their transposed copies) and uses their activation buffers; it owns the PPO Adam slots of both
 * stacks, logstd and its slots, one pair of beta powers, the old snapshot (old policy weights, old filter,
 * oldlogstd, oldmean [n][A]) and the PPO data.  The fitters must outlive the trainer.  Two launches per step
 * (csrc/ac_ppo.hip: both stacks in one launch pair); with a BC block every PPO step is followed by the policy
 * fitter's own BC step (its kernels, its Adam state) in the same chain.  A run of equal batch sizes replays one
 * captured graph, a single chain of kernel nodes; lr, eps, entcoeff and the filter are read from device memory.
 * Additive to ABI 5: callers detect the feature by the symbols.
 *
 * Refusals, before any HIP call (csrc/ac_ppo_plan.cpp): BCMPC_ERR_ARG for null pointers, fitters of the wrong
 * heads or of different state_dim / hidden / n_layers / device, betas outside [0, 1), a negative or non-finite
 * epsilon, a non-finite learning rate, eps or entcoeff, eps < 0, non-finite logstd / old policy / data, a batch
 * size < 1, an index outside the data; BCMPC_ERR_STATE for a run before set_logstd, set_old or set_data. */
typedef struct bcmpc_acppo_config {
    float beta1, beta2, epsilon;   /* the PPO optimizer's own Adam constants */
} bcmpc_acppo_config;

typedef struct bcmpc_acppo bcmpc_acppo;

int bcmpc_acppo_create(const bcmpc_acppo_config* cfg, bcmpc_acfit* policy_fitter, bcmpc_acfit* value_fitter,
                       bcmpc_acppo** out);
int bcmpc_acppo_destroy(bcmpc_acppo* t);
/* logstd [A]; the Adam slots and beta powers are kept */
int bcmpc_acppo_set_logstd(bcmpc_acppo* t, const float* logstd);
int bcmpc_acppo_get_logstd(bcmpc_acppo* t, float* logstd);
/* the old policy (assign_old_eq_new): L + 1 kernels and biases of pol/, its filter [S] and its logstd [A] */
int bcmpc_acppo_set_old(bcmpc_acppo* t, const float* const* kernels, const float* const* biases,
                        const float* ob_mean, const float* ob_std, const float* oldlogstd);
/* n rows: observations [n][S] f64, actions [n][A], advantages [n] and returns [n] as the f32 they are fed as */
int bcmpc_acppo_set_data(bcmpc_acppo* t, const double* obs, const float* acs, const float* atarg, const float* ret,
                         int64_t n);
/* `iterations` PPO steps; step i uses batch_sizes[i] rows of the PPO data.  eps = clip_param * cur_lrmult.
 * bc_indices != NULL: step i is followed by one BC step of the policy fitter on bc_batch_sizes[i] rows of ITS data
 * (bcmpc_acfit_set_data) at bc_learning_rate.  losses [iterations][6] = pol_surr, pol_entpen, vf_loss, kl, ent,
 * bc_loss before each update; bc_losses [iterations] (optional) the BC steps' losses.  oldmean is evaluated once
 * per call, by the row kernel's forward-only mode over all n rows. */
int bcmpc_acppo_run(bcmpc_acppo* t, const int64_t* indices, const int32_t* batch_sizes, int32_t iterations,
                    float learning_rate, float eps, float entcoeff, const int64_t* bc_indices,
                    const int32_t* bc_batch_sizes, float bc_learning_rate, float* losses, float* bc_losses);
/* 0: the last run launched its steps one by one (ragged batches, BCMPC_ACPPO_GRAPH=0); n >= 1: it replayed a
 * captured graph, the n-th this trainer has captured */
int bcmpc_acppo_is_graph(const bcmpc_acppo* t);
/* the checks alone, no device call: the pair of fitter configs; a run's arguments; the row kernel's LDS words
 * (-1 where refused) */
int bcmpc_acppo_check_pair(const bcmpc_acppo_config* cfg, const bcmpc_acfit_config* policy,
                           const bcmpc_acfit_config* value);
int bcmpc_acppo_check_run(const int64_t* indices, const int32_t* batch_sizes, int32_t iterations, int64_t n_data,
                          float learning_rate, float eps, float entcoeff);
int64_t bcmpc_acppo_lds_words(int32_t hidden, int32_t n_layers, int32_t state_dim, int32_t action_dim);
const char* bcmpc_acppo_last_error(void);

/* ------------------------------------------------------------------------
 * Candidate sharding over GPUs: one process per GPU, rank r owns the
 * global candidates [cand_offset, cand_offset + K).  The library owns the one
 * collective of a control step: a communicator attached to an engine makes every
 * bcmpc_get_action / bcmpc_get_action_mt19937 / bcmpc_rollout_async (with d_result)
 * of that engine all-gather the ranks' 144-byte result records over RCCL (xGMI)
 * right after the argmin launch, stream-ordered, and reduce them on the device with
 * np.argmin's rule (controllers.py:82: first NaN, else smallest cost, ties -> lowest
 * global index; np.argmax for BCMPC_COST_REWARD, controllers.py:152): every rank
 * returns the GLOBAL best.  All ranks must call with the same state and hold >= 1
 * candidate.  No Python or torch is needed: rank 0 makes the id, any out-of-band
 * channel (MPI, a file, a socket) carries its 128 bytes to the other ranks.
 * RCCL (librccl.so.1) is loaded on first use.  Replaces nothing in the reference's
 * hot path (single process); its only collective, train_mpc_ppo.py:388, gathers
 * episode statistics. */
#define BCMPC_COMM_ID_BYTES 128
typedef struct bcmpc_comm bcmpc_comm;
int bcmpc_comm_unique_id(uint8_t* id /* [BCMPC_COMM_ID_BYTES] */);             /* ncclGetUniqueId   */
int bcmpc_comm_init(const uint8_t* id, int32_t nranks, int32_t rank, int32_t device,
                    bcmpc_comm** out);                                          /* ncclCommInitRank  */
int bcmpc_comm_destroy(bcmpc_comm* comm);
/* attach (comm != NULL) or detach (NULL); the comm's device must be the engine's.
 * CEM calls (bcmpc_cem_*) do not exchange.  BCMPC_COST_TERMS engines: BCMPC_ERR_UNSUPPORTED for now. */
int bcmpc_engine_set_comm(bcmpc_engine* eng, bcmpc_comm* comm);
/* Host only: the np.argmin (maximize: np.argmax) winner of n result records, for hosts
 * that exchange the records themselves (e.g. MPI / gloo). */
int bcmpc_select_results(const bcmpc_result* recs, int32_t n, int32_t maximize, bcmpc_result* out);
/* The same select on the device, stream-ordered (the kernel the library's exchange runs after its
 * all-gather): d_recs [n] records -> d_out (must not overlap d_recs), 1 <= n <= 4096. */
int bcmpc_select_results_async(const bcmpc_result* d_recs, int32_t n, int32_t maximize, bcmpc_result* d_out,
                               void* stream);

/* Device stream the engine launches on (hipStream_t as void*). */
void* bcmpc_stream(bcmpc_engine* eng);

/* Small-K team kernel (bcmpc_engine_info kernel == BCMPC_KERNEL_TEAM): its workgroups wait for each
 * other once per step, so they must all be resident.  A team that cannot meet within ~1 s (another
 * process or kernel holding CUs) gives up and flags it; the synchronous entry points then rerun the
 * call on a fallback engine of the same net (the split slab kernel, else the fp32 group kernel;
 * not with a communicator attached: BCMPC_ERR_HIP).  Stream-ordered callers (bcmpc_rollout_async,
 * bcmpc_rollout_batch_async, bcmpc_rollout_policy_async, bcmpc_cem_rollout_async) call bcmpc_engine_status once their stream has
 * completed: BCMPC_ERR_HIP when a launch of this engine since the last check gave up (its outputs
 * are not valid), BCMPC_OK otherwise; reading clears the flag.  Team launches of one process on
 * different streams of a device are serialised (stream-ordered) by the library. */
int bcmpc_engine_status(bcmpc_engine* eng);
/* number of synchronous calls of this engine rerun on the fallback engine */
int bcmpc_engine_team_reruns(const bcmpc_engine* eng, uint64_t* reruns);

/* Kernel timing (off by default): with on != 0 every launch chain of this engine is bracketed
 * by HIP event markers (~6 us per synchronous get_action at small K, measured), which
 * bcmpc_last_kernel_ms reads.  Not part of the reference interface: a measurement switch. */
int bcmpc_engine_set_timing(bcmpc_engine* eng, int32_t on);
/* Timing of the last rollout kernel launched through bcmpc_get_action /
 * bcmpc_rollout_async / bcmpc_cem_get_action, in milliseconds (HIP events on the launch
 * stream); requires timing on for that launch (else BCMPC_ERR_ARG) and waits for it.  After a
 * batched call: rollout_ms = the state expansion + the rollout, argmin_ms = the per-environment argmin. */
int bcmpc_last_kernel_ms(bcmpc_engine* eng, float* rollout_ms, float* argmin_ms);

/* Static shape facts for tests: padded hidden size and packed weight bytes. */
int bcmpc_engine_info(const bcmpc_engine* eng, int32_t* hidden_padded, int64_t* packed_weight_bytes,
                      int32_t* waves_per_block, int32_t* kernel);
/* The device kernel instance the engine launches per rollout, as text (e.g. "rollout_pp<512> f16",
 * "rollout_x3<512,NC=4,NW=8> split"), NUL-terminated and truncated to cap bytes: tests and the bench
 * assert / report which layout the engine selected ("+terms" appended on BCMPC_COST_TERMS engines).  Round 5 (ABI 4). */
int bcmpc_engine_layout(const bcmpc_engine* eng, char* buf, int32_t cap);
/* LDS bytes per workgroup of the two-group pipelined split kernel (rollout_pp3: BCMPC_PREC_SPLIT_F16 under
 * kernel auto at large K, or forced with BCMPC_SPLIT_PP=1) for a net shape, or -1 where the layout does not
 * cover the shape (it covers n_layers == 2, hidden padded to 512, state_dim + action_dim <= 32, within the
 * CU's 160 KiB).  No device call. */
int64_t bcmpc_split_pp_lds_bytes(int32_t hidden, int32_t n_layers, int32_t state_dim, int32_t action_dim);

#ifdef __cplusplus
}
#endif
#endif /* BCMPC_H_ */

// engine_plan.cpp -- bcmpc_create's checks and kernel selection (team, split1/2/4, pp, pp3, group, solo) and the
// offsets of the packed weights.  No HIP: the device enters as its CU count.
#include "engine_plan.h"

#include <algorithm>
#include <cstdlib>

namespace bcmpc::host {

namespace {

int kern_waves(int kern) {
    return kern == BCMPC_KERNEL_GROUP8 ? 8 : kern == BCMPC_KERNEL_GROUP4 ? 4 : 1;
}

// BCMPC_SPLIT_PP: 1 forces the two-group pipelined split kernel (rollout_pp3) at any K, 0 turns it off, unset
// leaves the choice to kernel="auto" (kSplitPpAutoCols candidate columns and more, horizon >= kSplitPpAutoMinH)
// (the A/B that places the column threshold.  The horizon: the two-group pipeline runs 2H + 2
//  barrier intervals for 2H segments of work, each interval 0.90 of a rollout_x3 step per 128 candidates at
//  cfg3, so it breaks even at H = 10 and clears 3% from H = 14)
constexpr int64_t kSplitPpAutoCols = 2048;
constexpr int kSplitPpAutoMinH = 14;
int split_pp_env() {
    const char* v = std::getenv("BCMPC_SPLIT_PP");
    return !(v && *v) ? -1 : v[0] == '1' ? 1 : 0;
}

// the offsets of the packed kernels and biases, and the buffers' sizes
void plan_offsets(EnginePlan& p) {
    const bcmpc_config& c = p.cfg;
    const int L = c.n_layers, T = p.T;
    size_t off = 0, boff = 0;
    p.nwl = p.reward ? 3 : L + 1;
    if (p.reward && p.split) {
        // split layout: trunk, delta head hidden (dense_1), delta out (dense_2), reward head
        // hidden (dense_3), reward out (dense_4, one 16-row tile); 512 floats = one 2-KiB fragment pair
        const int P = T / 2;
        p.w_off[0] = off; off += (size_t)T * 512;
        p.w_off[1] = off; off += (size_t)T * P * 512;
        p.w_off[2] = off; off += (size_t)2 * P * 512;
        p.w_off[3] = off; off += (size_t)T * P * 512;
        p.w_off[4] = off; off += (size_t)P * 512;
        p.nwl = 5;
        // biases: trunk | delta head | reward head | out (rows 0..S-1 dense_2, row S dense_4) | (team kernel,
        // LayerNorm heads) the centring table [8 members][32 rows]
        p.b_off[0] = 0; p.b_off[1] = p.HP; p.b_off[2] = 2 * p.HP; p.b_off[3] = 3 * p.HP;
        p.b_off[4] = 3 * p.HP + 32;
        boff = 3 * p.HP + 32 + 8 * 32;
    } else if (p.reward) {
        // [S+A -> h] trunk, [h -> 2h] both heads' hidden layers, [2h -> S+1] block-diagonal output
        p.w_off[0] = off; off += (size_t)T * 2 * 64 * 4;
        p.w_off[1] = off; off += (size_t)2 * T * T * 64 * 4;
        p.w_off[2] = off; off += (size_t)2 * 2 * T * 64 * 4;
        p.b_off[0] = 0; p.b_off[1] = p.HP; p.b_off[2] = 3 * p.HP; boff = 3 * p.HP + 32 + 8 * 32;   // (same size as the split layout)
    } else {
        p.w_off[0] = off; off += (size_t)T * 2 * 64 * 4;                   // [S+A -> h]
        for (int l = 1; l < L; ++l) { p.w_off[l] = off; off += (size_t)T * T * 64 * 4; }
        p.w_off[L] = off; off += (size_t)2 * T * 64 * 4;                   // [h -> S]
        for (int l = 0; l < L; ++l) { p.b_off[l] = boff; boff += p.HP; }
        p.b_off[L] = boff; boff += 32;
    }
    p.w_floats = off;
    p.b_floats = boff;
    p.ln_floats = 2 * (size_t)(p.reward ? 3 : L) * p.HP;
    if (p.PL > 0) {
        size_t poff = 0;
        p.pw_off[0] = poff; poff += (size_t)p.TP * 2 * 64 * 4;                    // [S -> ph]
        for (int l = 1; l < p.PL; ++l) { p.pw_off[l] = poff; poff += (size_t)p.TP * p.TP * 64 * 4; }
        p.pw_off[p.PL] = poff; poff += (size_t)p.TP * 64 * 4;                  // [ph -> one 16-row tile]
        p.pw_floats = poff;
    }
}

}  // namespace

int padded_hidden(int h) {
    for (int hp : {64, 128, 256, 512, 768, 1024})
        if (h <= hp) return hp;
    return -1;
}

int check_config(const bcmpc_config& c) {
    if (c.state_dim < 1 || c.state_dim > BCMPC_MAX_STATE) return fail(BCMPC_ERR_UNSUPPORTED, "state_dim must be in [1, 32]");
    if (c.action_dim < 1 || c.action_dim > BCMPC_MAX_ACTION) return fail(BCMPC_ERR_UNSUPPORTED, "action_dim must be in [1, 16]");
    if (c.state_dim + c.action_dim > BCMPC_MAX_INPUT) return fail(BCMPC_ERR_UNSUPPORTED, "state_dim + action_dim must be <= 32");
    if (c.n_layers < 1 || c.n_layers > BCMPC_MAX_LAYERS) return fail(BCMPC_ERR_UNSUPPORTED, "n_layers must be in [1, 8]");
    if (padded_hidden(c.hidden) < 0 || c.hidden < 1) return fail(BCMPC_ERR_UNSUPPORTED, "hidden must be in [1, 1024] in this build");
    if (c.activation != BCMPC_ACT_TANH && c.activation != BCMPC_ACT_RELU) return fail(BCMPC_ERR_UNSUPPORTED, "activation must be tanh or relu");
    if (c.horizon < 1) return fail(BCMPC_ERR_ARG, "horizon must be >= 1");
    if (c.num_paths < 0) return fail(BCMPC_ERR_ARG, "num_paths must be >= 0");
    if (c.cost != BCMPC_COST_CHEETAH && c.cost != BCMPC_COST_NONE && c.cost != BCMPC_COST_REWARD &&
        c.cost != BCMPC_COST_TERMS)
        return fail(BCMPC_ERR_UNSUPPORTED, "unknown cost");
    if (c.model != BCMPC_MODEL_DELTA && c.model != BCMPC_MODEL_REWARD) return fail(BCMPC_ERR_ARG, "unknown model");
    const bool reward = c.model == BCMPC_MODEL_REWARD;
    if ((c.cost == BCMPC_COST_REWARD) != reward)
        return fail(BCMPC_ERR_ARG, "the learned-reward objective and BCMPC_MODEL_REWARD go together "
                                   "(MPCcontrollerReward needs NNDynamicsRewardModel, controllers.py:137)");
    if (reward) {
        if (c.n_layers != 2) return fail(BCMPC_ERR_ARG, "reward model: n_layers must be 2 (trunk + head, dynamics.py:167-174)");
        if (c.activation != BCMPC_ACT_TANH) return fail(BCMPC_ERR_UNSUPPORTED, "reward model is tanh (dynamics.py:150)");
        if (c.hidden > 512) return fail(BCMPC_ERR_UNSUPPORTED, "reward model: hidden must be <= 512 in this build");
        if (c.state_dim > 31) return fail(BCMPC_ERR_UNSUPPORTED, "reward model: state_dim must be <= 31");
    }
    if (c.cost == BCMPC_COST_CHEETAH && c.state_dim < 18) return fail(BCMPC_ERR_UNSUPPORTED, "cheetah cost needs state_dim >= 18");
    if (c.cost == BCMPC_COST_TERMS && c.policy_hidden > 0)
        return fail(BCMPC_ERR_UNSUPPORTED, "cost terms: engines with a fused policy need their fused cost");
    if (c.precision != BCMPC_PREC_FP32 && c.precision != BCMPC_PREC_SPLIT_F16 && c.precision != BCMPC_PREC_F16)
        return fail(BCMPC_ERR_UNSUPPORTED, "precision must be FP32, SPLIT_F16 or F16");
    // single-pass f16 (BASELINE cfg3's bf16-class GEMM): the split slab kernels' plain tanh delta net only
    const bool f16 = c.precision == BCMPC_PREC_F16;
    if (f16 && (reward || c.policy_hidden > 0 || c.activation != BCMPC_ACT_TANH || c.layer_norm))
        return fail(BCMPC_ERR_UNSUPPORTED, "F16 precision: the tanh NNDynamicsModel without LayerNorm / policy only");
    if (f16 && c.kernel != BCMPC_KERNEL_AUTO && (c.kernel < BCMPC_KERNEL_SPLIT1 || c.kernel > BCMPC_KERNEL_SPLIT4))
        return fail(BCMPC_ERR_ARG, "F16 precision runs on the split1/split2/split4 kernels");
    if (c.precision != BCMPC_PREC_FP32) {
        if (reward && c.state_dim < 16)
            return fail(BCMPC_ERR_UNSUPPORTED, "split reward engines need state_dim >= 16 (reward row in tile 1)");
        if (c.kernel != BCMPC_KERNEL_AUTO && (c.kernel < BCMPC_KERNEL_SPLIT1 || c.kernel > BCMPC_KERNEL_TEAM))
            return fail(BCMPC_ERR_ARG, "SPLIT_F16 precision runs on the split1/split2/split4/team kernels");
        if (c.kernel == BCMPC_KERNEL_SPLITR)
            return fail(BCMPC_ERR_UNSUPPORTED, "the splitr (resident-column) kernel was retired: slower than the "
                                               "split slab kernel at every K (DESIGN.md 6.5); use auto or split4");
    } else if (c.kernel >= BCMPC_KERNEL_SPLIT1) {
        return fail(BCMPC_ERR_ARG, "split kernels need precision SPLIT_F16");
    }
    if (c.kernel == BCMPC_KERNEL_GROUP2)
        return fail(BCMPC_ERR_UNSUPPORTED, "the group2 layout (2-wave f32 groups, A/B only, never chosen by auto) "
                                           "was retired; use auto, group4 or group8");
    return BCMPC_OK;
}

int plan_engine(const bcmpc_config& c, const CreateOpts& opts, int ncu, EnginePlan* out) {
    if (const int rc = check_config(c)) return rc;
    EnginePlan p;
    p.cfg = c;
    const bool reward = p.reward = c.model == BCMPC_MODEL_REWARD;
    const bool f16 = p.f16 = c.precision == BCMPC_PREC_F16;
    const bool split = p.split = c.precision != BCMPC_PREC_FP32;
    // relu / LayerNorm hidden layers (per-column scales or statistics exchanged across the workgroup)
    // on the split slab kernels: the plain delta net without a policy, hidden <= 512; beyond that only
    // the small-K team kernel takes them (checked once the kernel is chosen, below)
    const bool split_needs_team = split && (c.activation != BCMPC_ACT_TANH || c.layer_norm) &&
                                  (reward || c.policy_hidden > 0 || padded_hidden(c.hidden) > 512);
    const int HP = p.HP = reward ? std::max(128, padded_hidden(c.hidden)) : padded_hidden(c.hidden);
    p.T = HP / 16;
    // small K: one wave per block spreads candidates over more CUs
    const int64_t cols = (c.num_paths + 15) / 16;
    p.wpb = std::min(cols >= 4 * 256 ? 4 : 1, max_waves_per_block(HP, c.n_layers));
    const bool fp32_off_group = !split && c.kernel != BCMPC_KERNEL_AUTO && c.kernel != BCMPC_KERNEL_GROUP4 &&
                                c.kernel != BCMPC_KERNEL_GROUP8;
    // two-head net: 4-wave groups (16 head tiles per wave, spill-free at 2 waves/SIMD; the
    // 8-wave layout needs ~135 registers and spills at 4 waves/SIMD -- measured 2.5% slower)
    if (reward && fp32_off_group) return fail(BCMPC_ERR_UNSUPPORTED, "reward engines run on the group4 / group8 kernels");
    if (c.policy_hidden > 0) {
        // MPCcontrollerPolicyNet: the policy MLP is fused into the 4-wave group kernel
        if (c.policy_hidden > 128 || c.policy_layers < 1 || c.policy_layers > BCMPC_MAX_LAYERS)
            return fail(BCMPC_ERR_UNSUPPORTED, "policy: hidden must be in [1,128], layers in [1,8]");
        if (c.state_dim < 16) return fail(BCMPC_ERR_UNSUPPORTED, "policy engines need state_dim >= 16");
        if (HP < 128 || HP > (split ? 1024 : 512))
            return fail(BCMPC_ERR_UNSUPPORTED, "policy engines support dynamics hidden 65..512 (split: ..1024)");
        if (c.policy_mode != BCMPC_POLICY_EXPLORE && c.policy_mode != BCMPC_POLICY_STOCHASTIC)
            return fail(BCMPC_ERR_ARG, "unknown policy_mode");
        if (fp32_off_group) return fail(BCMPC_ERR_UNSUPPORTED, "policy engines run on the group4 / group8 kernels");
        p.PHP = 128;
        p.TP = 8;
        p.PL = c.policy_layers;
    }
    // small-K team kernel (rollout_team.hip): the 2-layer delta net at hidden <= 512 (LayerNorm: <=
    // 256), or at hidden 512 (tanh) with a fused policy of <= 2 layers and / or the reward net (the
    // run.sh recipe), when the whole grid fits one workgroup per CU (the team members of a column wait
    // for each other).  Auto: whenever it fits, unless BCMPC_TEAM=0
    const int tkind = reward ? 2 : p.PL > 0 ? 1 : 0;
    const int tmem = team_members(HP, tkind);
    // (a LayerNorm over a layer split across members: only the reward net's heads, whose statistics
    //  ride along with the output partials in the exchange -- rows 24..27, so S + 1 <= 24)
    const bool team_shape = split && !f16 && c.n_layers == 2 && HP <= 512 && c.state_dim + c.action_dim <= 32 &&
                            c.action_dim <= 15 && c.horizon <= 1022 && tmem > 0 &&
                            !(c.layer_norm && tmem > 1 && tkind != 2) &&
                            (tkind == 0 || (c.state_dim >= 16 && p.PL <= 2 &&
                                            (tmem == 1 || c.activation == BCMPC_ACT_TANH))) &&
                            !(tkind == 2 && c.layer_norm && (c.state_dim > 23 || !team_rw_ln_built()));
    const bool team_fits = team_shape && c.num_paths > 0 && team_blocks(c.num_paths, HP, tkind) <= (int64_t)ncu;
    if (c.kernel == BCMPC_KERNEL_TEAM && !team_fits)
        return fail(BCMPC_ERR_UNSUPPORTED, "team kernel: 2-layer net, hidden <= 512 (LayerNorm: <= 256; with a "
                                           "policy: hidden <= 256, or 512 tanh without LayerNorm; the reward "
                                           "net: 512, tanh, LayerNorm with S <= 23), S + A <= 32, "
                                           "ceil(K / 128) * 8 * members workgroups <= the device's CUs");
    const char* team_env = std::getenv("BCMPC_TEAM");
    const bool team_auto = c.kernel == BCMPC_KERNEL_AUTO && team_fits && !opts.no_team && !(team_env && team_env[0] == '0');
    // rollout_pp3 (two 64-candidate groups pipelined over one slab): the plain 2-layer tanh delta net at hidden
    // 512 under kernel="auto"; cost terms and ensemble members stay on rollout_x3.  Forced, it also replaces the
    // small-K team kernel
    const int pp3_env = split_pp_env();
    const bool pp3_shape = split && !f16 && !reward && p.PL == 0 && c.kernel == BCMPC_KERNEL_AUTO && !opts.no_pp3 &&
                           c.activation == BCMPC_ACT_TANH && !c.layer_norm && c.cost != BCMPC_COST_TERMS &&
                           c.horizon >= 1 && x3_pp3_ok(HP, c.n_layers, c.state_dim, c.action_dim);
    const bool pp3_forced = pp3_shape && pp3_env == 1 && c.num_paths >= 1;
    const bool team = c.kernel == BCMPC_KERNEL_TEAM || (team_auto && !pp3_forced);

    // the kernel and its waves per group, resolved here and nowhere else
    int kern, nw;
    if (team) {
        kern = BCMPC_KERNEL_TEAM;
        p.nc = 1;
        nw = HP / 16 / team_layer0_tiles(HP, tkind);
        p.team_kind = tkind;
    } else if (split) {
        // widest workgroup (most candidates per weight read) that still gives every CU work and fits LDS
        int nc = c.kernel == BCMPC_KERNEL_SPLIT1 ? 1 : c.kernel == BCMPC_KERNEL_SPLIT2 ? 2
               : c.kernel == BCMPC_KERNEL_SPLIT4 ? 4 : 0;
        const int nwx = x3_waves(HP);
        auto fits = [&](int n) {
            return n <= nwx && n <= x3_max_nc(HP) && (p.PL == 0 || x3_policy_ok(HP, n)) &&
                   x3_lds(HP, reward ? 3 : c.n_layers, n, c.action_dim, p.PL, p.PHP,
                          (c.activation == BCMPC_ACT_RELU ? 1 : 0) | (c.layer_norm ? 2 : 0)) <= 160 * 1024;
        };
        nw = nwx;
        if (f16) {
            // single-pass f16: the hi-only slab admits wider groups (x3_f16_layout_ok); BCMPC_F16_NC /
            // BCMPC_F16_NW pick a layout for A/B runs
            auto f16_fits = [&](int n, int w) {
                return x3_f16_layout_ok(HP, n, w) && x3_f16_lds(HP, c.n_layers, n, w, c.action_dim) <= 160 * 1024;
            };
            const char* en = std::getenv("BCMPC_F16_NC");
            const char* ew = std::getenv("BCMPC_F16_NW");
            const char* ep = std::getenv("BCMPC_F16_PP");
            // (default at large K, where it measured ahead of the two-group 4x4 layout below on every box:
            //  0.835-0.848 vs 0.898-0.900 ms at cfg3, profiles/r04_pp_ab.jsonl; BCMPC_F16_PP=1 forces it at any
            //  K, =0 turns it off)
            const bool pp_env = ep && *ep;
            if (!(en && *en) && !(ew && *ew) && x3_pp_ok(HP, c.n_layers, c.state_dim, c.action_dim) &&
                !reward && p.PL == 0 && c.activation == BCMPC_ACT_TANH && !c.layer_norm &&
                (pp_env ? ep[0] == '1' && cols >= 8 : cols >= 4 * 512)) {
                // the two-group pipelined kernel (rollout_pp): 128 candidates per workgroup, 4 waves per
                // group own 8 hidden tiles each (weights packed 8 tiles per wave)
                p.pp = true;
                // FOLD's input range: layer 0's normalised input goes to f16 without a power-of-two scale,
                // clamped to +-65504 (a dim normalising beyond saturates; the first tanh has saturated long
                // before) and below 6.1e-5 subnormal (< 6e-8 absolute error); the fold check of pack_weights bounds
                // only the weights.  Pinned by tests/test_gpu_f16.py::test_f16_pp_fold_input_range
                const char* ef = std::getenv("BCMPC_PP_FOLD");
                p.pp_fold = !(ef && ef[0] == '0');
                nc = 8;
                nw = 8;
            }
            if (en && *en) nc = std::atoi(en);
            if (ew && *ew) nw = std::atoi(ew);
            if (!p.pp && nc == 0 && !(ew && *ew) && HP == 512 && cols >= 4 * 512 && f16_fits(4, 4)) {
                // two 64-candidate 4-wave groups per CU: 0.90 ms at cfg3 against 0.94 (one 8-wave group of
                // 64) and 0.91 (one of 128), three boxes (profiles/r04_f16_layouts_ab.txt)
                nc = 4;
                nw = 4;
            }
            if (nc == 0) {
                nc = 1;
                for (int n : {8, 4, 2})
                    if (f16_fits(n, nw) && cols >= (int64_t)n * 256 && !(n >= 4 && HP <= 256)) { nc = n; break; }
            }
            if (!p.pp && !f16_fits(nc, nw))
                return fail(BCMPC_ERR_UNSUPPORTED, "F16 precision: no single-pass layout for this shape / NC / NW");
        } else if (nc == 0) {
            nc = 1;
            // (hidden <= 256: 32-candidate groups, two or three workgroups per CU, measured 6-18% ahead of 64)
            for (int n : {4, 2})
                if (fits(n) && cols >= (int64_t)n * 256 && !(n == 4 && HP <= 256)) { nc = n; break; }
            // rollout_pp3 reads rollout_x3<512, NC=4, NW=8>'s packed weights: the engine stays a split4 engine
            if (pp3_shape && nwx == 8 && fits(4) && (pp3_forced || (pp3_env != 0 && cols >= kSplitPpAutoCols && c.horizon >= kSplitPpAutoMinH))) {
                p.pp3 = true;
                nc = 4;
            }
        }
        if (!f16 && !fits(nc))
            return fail(BCMPC_ERR_UNSUPPORTED, p.PL ? "split kernel with a fused policy needs dynamics hidden 449..1024"
                                                    : "split kernel does not fit this shape");
        p.nc = nc;
        kern = nc == 1 ? BCMPC_KERNEL_SPLIT1 : nc == 2 ? BCMPC_KERNEL_SPLIT2 : BCMPC_KERNEL_SPLIT4;
    } else {
        // fp32.  auto: 4-wave groups; 8-wave groups when K is too small to give every SIMD two waves (the reward
        // net and the fused policy: always 4-wave groups, above)
        kern = c.kernel != BCMPC_KERNEL_AUTO ? c.kernel
             : reward || p.PL > 0 ? BCMPC_KERNEL_GROUP4
             : cols < 512 && p.T % 8 == 0 ? BCMPC_KERNEL_GROUP8 : BCMPC_KERNEL_GROUP4;
        if (kern < BCMPC_KERNEL_SOLO || kern > BCMPC_KERNEL_TEAM) return fail(BCMPC_ERR_ARG, "unknown kernel");
        nw = kern_waves(kern);
        if (kern != BCMPC_KERNEL_SOLO &&
            (p.T % nw != 0 || grp_lds_bytes(HP, c.n_layers, nw, p.PHP, p.PL, c.model) > 160 * 1024)) {
            if (c.kernel != BCMPC_KERNEL_AUTO) return fail(BCMPC_ERR_UNSUPPORTED, "group kernel does not fit this shape");
            kern = BCMPC_KERNEL_SOLO;
            nw = kern_waves(kern);
        }
        if (kern == BCMPC_KERNEL_SOLO && (p.wpb < 1 || HP > 512))
            return fail(BCMPC_ERR_UNSUPPORTED, "solo kernel supports hidden <= 512 and needs LDS for its slabs");
    }
    if (split_needs_team && !team)
        return fail(BCMPC_ERR_UNSUPPORTED, "SPLIT_F16 precision supports relu / LayerNorm nets with a policy, the "
                                           "reward net or hidden > 512 only on the small-K team kernel (use FP32)");
    p.kernel = kern;
    p.nw = nw;
    p.pack_tb = kern == BCMPC_KERNEL_SOLO ? 4 : p.pp ? p.T / 4 : p.T / nw;   // split: output tiles per wave
    p.head_tb = kern == BCMPC_KERNEL_TEAM ? team_layer1_tiles(HP, p.team_kind) : p.pack_tb;   // (team: head tiles per wave)
    plan_offsets(p);
    *out = p;
    return BCMPC_OK;
}

}  // namespace bcmpc::host

// engine_plan.h -- what bcmpc_create decides before it allocates anything: the checked config, the kernel that runs it
// and the layout of its packed weights.  Pure host arithmetic over shapes.h (no HIP): a plan is a plain value.
#pragma once
#include <string>

#include "shapes.h"

namespace bcmpc {
int set_error(int code, const std::string& msg);          // bcmpc_last_error() text (capi.cpp)
}

#pragma GCC visibility push(hidden)
namespace bcmpc::host {

struct CreateOpts {                     // bcmpc_create's internal options
    bool no_team = false;               // never pick the team kernel (fallback engines)
    bool no_pp3 = false;                // never pick rollout_pp3 (ensemble members)
};

struct EnginePlan {
    bcmpc_config cfg{};
    int HP = 0, T = 0, wpb = 4;
    int kernel = BCMPC_KERNEL_SOLO;    // resolved kernel layout
    int nw = 1;                        // waves per group (group kernels)
    int pack_tb = 4;                   // output tiles per packed block of layers 0..L-1
    int head_tb = 4;                   // ... of the hidden layers (team kernel: team_layer1_tiles; else pack_tb)
    bool split = false;                // BCMPC_PREC_SPLIT_F16 or F16 (rollout_x3)
    bool f16 = false;                  // BCMPC_PREC_F16: single MFMA pass
    bool pp = false;                   // BCMPC_PREC_F16 on the two-group pipelined kernel (rollout_pp)
    bool pp_fold = false;              // ... with the folded operands (rollout_pp<, FOLD>; BCMPC_PP_FOLD=0: off)
    bool pp3 = false;                  // BCMPC_PREC_SPLIT_F16 on the two-group pipelined kernel (rollout_pp3): the
                                       // launches it implements; the others run rollout_x3 on the same weights
    int nc = 0;                        // split kernel: 16-candidate columns per workgroup
    int nwl = 0;                       // packed weight layers (RolloutArgs.w entries)
    bool reward = false;               // BCMPC_MODEL_REWARD (NNDynamicsRewardModel)
    int team_kind = 0;                 // team kernel: 0 plain delta net, 1 + policy, 2 reward net (+ policy)
    // packed buffers, in floats: kernels (w_off per layer), biases (b_off), LayerNorm [2][L][HP]
    size_t w_floats = 0, w_off[BCMPC_MAX_LAYERS + 1]{};
    size_t b_floats = 0, b_off[BCMPC_MAX_LAYERS + 1]{};
    size_t ln_floats = 0;
    // fused policy (MPCcontrollerPolicyNet)
    int PHP = 0, TP = 0, PL = 0;
    size_t pw_floats = 0, pw_off[BCMPC_MAX_LAYERS + 1]{};
};

inline int fail(int code, const std::string& msg) { return set_error(code, msg); }

int padded_hidden(int hidden);       // 64 .. 1024 (-1: beyond)
// the config's own checks, in bcmpc_create's order: everything that needs no device (plan_engine runs them first)
int check_config(const bcmpc_config& c);
// every check and the whole kernel selection for a device of ncu CUs.  Fills *out; a refusal sets the error text and
// returns its code, with nothing to free.  Reads BCMPC_TEAM, BCMPC_SPLIT_PP, BCMPC_F16_NC / _NW / _PP, BCMPC_PP_FOLD
int plan_engine(const bcmpc_config& c, const CreateOpts& opts, int ncu, EnginePlan* out);

}  // namespace bcmpc::host
#pragma GCC visibility pop

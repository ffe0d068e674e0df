// ac_ppo_plan.h -- what the PPO trainer (include/bcmpc.h bcmpc_acppo_*) decides before it touches the device: the
// checked pair of fitters, the row kernel's LDS, the parameter kernel's work list over both stacks and every
// refusal of a run.  Pure host arithmetic (no HIP).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/bcmpc.h"
#include "ac_fit_plan.h"

#pragma GCC visibility push(hidden)
namespace bcmpc::acppo {

struct Task {                               // one workgroup of acppo_params_kernel
    int32_t kind;                           // 0: weight tile (+ bias row), 2: logstd, 3: losses and step counter
    int32_t stack;                          // 0: pol/, 1: vf/
    int32_t layer;
    int32_t k0, n0;                         // tile origin
};

struct Plan {
    bcmpc_acppo_config cfg{};
    int S = 0, A = 0, h = 0, L = 0, device = 0;
    int ld = 0;                             // row stride of the LDS row buffers: the policy fitter's
    size_t lds_words = 0;                   // acppo_rows_kernel's dynamic LDS
    std::vector<Task> tasks;
};

// LDS words of the row kernel: acfit's for the policy stack, plus the old means [16][16], the rows' scalars and
// partials [8][16], std and old std [2][16]
size_t lds_words(int hidden, int n_layers, int state_dim, int action_dim);
// the pair: a policy and a value fitter of one S / hidden / L / device; the trainer's Adam constants
int make_plan(const bcmpc_acppo_config* c, const bcmpc_acfit_config* pol, const bcmpc_acfit_config* val, Plan* out);
// lr, eps = clip_param * cur_lrmult and entcoeff finite, eps >= 0
int check_hyper(float lr, float eps, float entcoeff);
// what must have been set before a run
int check_state(bool has_logstd, bool has_old, bool has_data, bool pol_weights, bool val_weights, bool pol_filter);
int check_finite(const float* x, int64_t n, const char* what);

}  // namespace bcmpc::acppo
#pragma GCC visibility pop

// rollout_x3_plain.hip -- the split kernel (rollout_x3.h) for the plain tanh delta net without a policy
// at split precision (cfg2..cfg5): a unit of its own because it is built with the iterative-ILP
// scheduler (Makefile X3ILP), every other instantiation (rollout_x3.hip) with max-ILP.

#include "rollout_x3.h"

namespace bcmpc {

// (the single-pass instantiations live in rollout_x3.hip: iterative-ILP crashes the compiler on them)
template <int NC>
static hipError_t launch_x3_plain_nc(const RolloutArgs& a, int hidden_padded, hipStream_t st) {
    if (a.f16_single) return launch_rollout_x3_f16(a, hidden_padded, NC, st);
    return launch_x3_plain_ncf<NC, false>(a, hidden_padded, st);
}

hipError_t launch_rollout_x3_plain(const RolloutArgs& a, int hidden_padded, int nc, hipStream_t st) {
    switch (nc) {
        case 1: return launch_x3_plain_nc<1>(a, hidden_padded, st);
        case 2: return launch_x3_plain_nc<2>(a, hidden_padded, st);
        case 4: return launch_x3_plain_nc<4>(a, hidden_padded, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace bcmpc

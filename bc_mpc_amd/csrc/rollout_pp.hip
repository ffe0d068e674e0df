// rollout_pp.hip -- launchers and host shape queries of the two pipelined kernels (rollout_pp.h):
// rollout_pp (single-pass f16) and rollout_pp3 (split precision).  Built with the max-ILP scheduler
// (Makefile X3P2), as rollout_x3.hip.

#include "rollout_pp.h"

namespace bcmpc {

bool x3_pp_ok(int hidden_padded, int n_layers, int state_dim, int action_dim) {
    return hidden_padded == 512 && n_layers == 2 && state_dim + action_dim <= 32 &&
           pp_lds_total(512, action_dim) <= 160 * 1024;
}

// a.x3_pp: 1 the power-of-two operand scales, 2 the folded operands (FOLD)
hipError_t launch_rollout_pp(const RolloutArgs& a, int hidden_padded, hipStream_t st) {
    if (!x3_pp_ok(hidden_padded, a.L, a.S, a.A) || a.model != BCMPC_MODEL_DELTA || a.pL > 0 ||
        a.act != BCMPC_ACT_TANH || a.ln || !a.f16_single)
        return hipErrorInvalidValue;
    static bool attr_set = false;
    if (!attr_set) {
        for (const void* f : {(const void*)rollout_pp<512, false>, (const void*)rollout_pp<512, true>}) {
            const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
        }
        attr_set = true;
    }
    const int64_t blocks = (a.K + 127) / 128;
    if (a.x3_pp == 2)
        hipLaunchKernelGGL((rollout_pp<512, true>), dim3((unsigned)blocks), dim3(512), (size_t)pp_lds_total(512, a.A),
                           st, a);
    else
        hipLaunchKernelGGL((rollout_pp<512, false>), dim3((unsigned)blocks), dim3(512), (size_t)pp_lds_total(512, a.A),
                           st, a);
    return hipGetLastError();
}

// rollout_pp3's shapes: the plain 2-layer net at hidden 512 whose slab, partials and action inputs fit
// the CU's 160 KiB (at S + A <= 32: S <= 20 with A <= 10)
bool x3_pp3_ok(int hidden_padded, int n_layers, int state_dim, int action_dim) {
    return hidden_padded == 512 && n_layers == 2 && state_dim >= 1 && action_dim >= 1 &&
           state_dim + action_dim <= 32 && x3_pp3_lds(hidden_padded, state_dim, action_dim) <= 160 * 1024;
}
size_t x3_pp3_lds(int hidden_padded, int state_dim, int action_dim) {
    return (size_t)pp3_lds_total(hidden_padded, state_dim, action_dim);
}
// (the launch arguments rollout_pp3 implements: capi.cpp sends every other launch to rollout_x3)
bool x3_pp3_args_ok(const RolloutArgs& a, int hidden_padded) {
    return x3_pp3_ok(hidden_padded, a.L, a.S, a.A) && a.model == BCMPC_MODEL_DELTA && a.pL == 0 &&
           a.act == BCMPC_ACT_TANH && !a.ln && !a.f16_single && !a.fused_argmin &&
           (a.cost == BCMPC_COST_CHEETAH || a.cost == BCMPC_COST_NONE) && a.K >= 1 && a.H >= 1;
}
hipError_t launch_rollout_pp3(const RolloutArgs& a, int hidden_padded, hipStream_t st) {
    if (!x3_pp3_args_ok(a, hidden_padded)) return hipErrorInvalidValue;
    static bool attr_set = false;
    if (!attr_set) {
        const hipError_t e = hipFuncSetAttribute((const void*)rollout_pp3<512>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    const int64_t blocks = (a.K + 127) / 128;
    hipLaunchKernelGGL((rollout_pp3<512>), dim3((unsigned)blocks), dim3(512), x3_pp3_lds(512, a.S, a.A), st, a);
    return hipGetLastError();
}

}  // namespace bcmpc

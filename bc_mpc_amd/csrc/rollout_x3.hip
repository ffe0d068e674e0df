// rollout_x3.hip -- the split kernel (rollout_x3.h) for every net but the plain tanh delta net at split
// precision (rollout_x3_plain.hip): the fused policy, the learned reward, relu / LayerNorm nets and the
// single-pass f16 layouts (F1), with launch_rollout_x3 and the host shape queries.  Built with the max-ILP
// scheduler (Makefile X3P2).

#include "rollout_x3.h"

namespace bcmpc {

int x3_waves(int hidden_padded) { return x3_nw(hidden_padded); }

// widest candidate group (16-candidate columns) the build instantiates for a width:
// the accumulators of TW tiles x NC columns must fit beside the operand sets
int x3_max_nc(int hidden_padded) {
    const int tw = hidden_padded / 16 / x3_waves(hidden_padded);
    return tw >= 8 ? 2 : 4;
}

// fused policy: one 128-wide policy tile per wave of an 8-wave group
bool x3_policy_ok(int hidden_padded, int nc) {
    return x3_waves(hidden_padded) == 8 && 2 * nc <= 8 && hidden_padded >= 512;
}

size_t x3_lds(int hidden_padded, int n_layers, int nc, int action_dim, int policy_layers, int policy_hidden_padded,
              int ak) {
    return (size_t)x3_lds_bytes_rt(hidden_padded, nc, n_layers, action_dim, policy_layers, policy_hidden_padded, ak,
                                   x3_waves(hidden_padded));
}

// Single-pass layouts beyond the split kernel's (the hi-only slab is half the size): at hidden 512,
// 128-candidate groups (NC = 8, 8 waves: each 1-KiB weight fragment feeds 8 MFMAs) and two 64-candidate
// 4-wave groups per CU (NC = 4, NW = 4: one group's serial f64 / epilogue chain beside the other's
// MFMAs); at hidden 768 / 1024, 64-candidate groups (NC = 4).
bool x3_f16_layout_ok(int hidden_padded, int nc, int nw) {
    const int nwd = x3_waves(hidden_padded);
    if (nw == nwd && (nc == 1 || nc == 2)) return true;
    if (nw == nwd && nc == 4) return true;
    if (hidden_padded == 512) return (nc == 8 && nw == 8) || (nc == 4 && nw == 4);
    return false;
}
size_t x3_f16_lds(int hidden_padded, int n_layers, int nc, int nw, int action_dim) {
    return (size_t)x3_lds_bytes_rt(hidden_padded, nc, n_layers, action_dim, 0, 0, 0, nw, true);
}
hipError_t launch_rollout_x3_f16(const RolloutArgs& a, int hidden_padded, int nc, hipStream_t st) {
    if (a.x3_pp) return launch_rollout_pp(a, hidden_padded, st);
    const int nw = a.x3_nw ? a.x3_nw : x3_waves(hidden_padded);
    if (!x3_f16_layout_ok(hidden_padded, nc, nw)) return hipErrorInvalidValue;
    if (hidden_padded == 512 && nw == 4) return launch_x3_t<512, 4, 4, 0, false, 0, true>(a, st);
    if (hidden_padded == 512 && nc == 8) return launch_x3_t<512, 8, 8, 0, false, 0, true>(a, st);
    if (nc == 4 && hidden_padded == 768) return launch_x3_t<768, 4, 8, 0, false, 0, true>(a, st);
    if (nc == 4 && hidden_padded == 1024) return launch_x3_t<1024, 4, 8, 0, false, 0, true>(a, st);
    switch (nc) {
        case 1: return launch_x3_plain_ncf<1, true>(a, hidden_padded, st);
        case 2: return launch_x3_plain_ncf<2, true>(a, hidden_padded, st);
        case 4: return launch_x3_plain_ncf<4, true>(a, hidden_padded, st);
        default: return hipErrorInvalidValue;
    }
}

// relu and / or LayerNorm nets (AK != 0): the plain delta net, hidden <= 512
template <int NC, int AK>
static hipError_t launch_x3_ak(const RolloutArgs& a, int hidden_padded, hipStream_t st) {
    switch (hidden_padded) {
        case 64: return launch_x3_t<64, NC, x3_nw(64), 0, false, AK>(a, st);
        case 128: return launch_x3_t<128, NC, x3_nw(128), 0, false, AK>(a, st);
        case 256: return launch_x3_t<256, NC, x3_nw(256), 0, false, AK>(a, st);
        case 512: return launch_x3_t<512, NC, x3_nw(512), 0, false, AK>(a, st);
        default: return hipErrorInvalidValue;
    }
}

template <int NC>
static hipError_t launch_x3_nc(const RolloutArgs& a, int hidden_padded, hipStream_t st) {
    if (a.act == BCMPC_ACT_RELU || a.ln) {
        if (a.model == BCMPC_MODEL_REWARD || a.pL > 0) return hipErrorInvalidValue;
        if (a.act == BCMPC_ACT_RELU) return a.ln ? launch_x3_ak<NC, 3>(a, hidden_padded, st)
                                                 : launch_x3_ak<NC, 1>(a, hidden_padded, st);
        return launch_x3_ak<NC, 2>(a, hidden_padded, st);
    }
    if (a.model == BCMPC_MODEL_REWARD) {      // NNDynamicsRewardModel (hidden <= 512)
        if (a.pL > 0) {
            if (hidden_padded == 512 && a.phidden_padded == 128) return launch_x3_t<512, NC, 8, 128, true>(a, st);
            return hipErrorInvalidValue;
        }
        switch (hidden_padded) {
            case 64: return launch_x3_t<64, NC, x3_nw(64), 0, true>(a, st);
            case 128: return launch_x3_t<128, NC, x3_nw(128), 0, true>(a, st);
            case 256: return launch_x3_t<256, NC, x3_nw(256), 0, true>(a, st);
            case 512: return launch_x3_t<512, NC, x3_nw(512), 0, true>(a, st);
            default: return hipErrorInvalidValue;
        }
    }
    if (a.pL > 0) {                           // the fused policy: 8-wave groups (x3_policy_ok)
        if (a.phidden_padded != 128) return hipErrorInvalidValue;
        switch (hidden_padded) {
            case 512: return launch_x3_t<512, NC, 8, 128>(a, st);
            case 768:
                if constexpr (NC <= 2) return launch_x3_t<768, NC, 8, 128>(a, st);
                return hipErrorInvalidValue;
            case 1024:
                if constexpr (NC <= 2) return launch_x3_t<1024, NC, 8, 128>(a, st);
                return hipErrorInvalidValue;
            default: return hipErrorInvalidValue;
        }
    }
    return launch_rollout_x3_plain(a, hidden_padded, NC, st);
}

hipError_t launch_rollout_x3(const RolloutArgs& a, int hidden_padded, int nc, hipStream_t st) {
    switch (nc) {
        case 1: return launch_x3_nc<1>(a, hidden_padded, st);
        case 2: return launch_x3_nc<2>(a, hidden_padded, st);
        case 4: return launch_x3_nc<4>(a, hidden_padded, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace bcmpc

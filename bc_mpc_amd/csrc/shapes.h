// shapes.h -- the host shape queries of the kernel units (internal to libbcmpc): which shapes each kernel takes,
// its LDS bytes, how many tiles a wave owns.  No HIP include: the planner, the packers and the stand-alone tools
// under tools/micro read it as plain C++.  The definitions sit in the kernel units, beside the templates they describe.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/bcmpc.h"

namespace bcmpc {

// consts block: [10][32] doubles
//   0 mean_obs   1 std_obs + 1e-10   2 mean_action   3 std_action + 1e-10
//   4 mean_deltas  5 std_deltas      6 action low    7 action high
//   8 1 / (std_obs + 1e-10)   9 1 / (std_action + 1e-10)   (correctly rounded, for div_rn)
constexpr int kConstRows = 10;
constexpr int kConstCols = 32;

constexpr int kPolParams = 96;

constexpr int kArgminParts = 256;
int argmin_parts(int64_t K);

int max_waves_per_block(int hidden_padded, int n_layers);
size_t grp_lds_bytes(int hidden_padded, int n_layers, int nw, int policy_hidden_padded, int policy_layers, int model);
int x3_waves(int hidden_padded);
int x3_max_nc(int hidden_padded);
size_t x3_lds(int hidden_padded, int n_layers, int nc, int action_dim, int policy_layers, int policy_hidden_padded,
              int ak = 0);
bool x3_policy_ok(int hidden_padded, int nc);
// single-pass f16 layouts (BCMPC_PREC_F16): the (nc, nw) pairs this build instantiates, and their LDS
bool x3_f16_layout_ok(int hidden_padded, int nc, int nw);
size_t x3_f16_lds(int hidden_padded, int n_layers, int nc, int nw, int action_dim);
bool x3_pp_ok(int hidden_padded, int n_layers, int state_dim, int action_dim);   // rollout_pp's shapes
// split precision on the two-group pipelined kernel (rollout_pp3): its shapes, its LDS bytes (kernels.h: the launch
// arguments it implements)
bool x3_pp3_ok(int hidden_padded, int n_layers, int state_dim, int action_dim);
size_t x3_pp3_lds(int hidden_padded, int state_dim, int action_dim);
// rollout_team.hip; kind: 0 the plain delta net, 1 + fused policy, 2 the reward net (+ policy)
int team_members(int hidden_padded, int kind);          // workgroups per candidate column (0: unsupported)
// the team kernel's deferred last LayerNorm (relu + LN delta net at T = 1; rollout_team.hip DEFER): the host
// packs the output layer for it whenever the kernel takes it -- one switch for both sides
#ifndef TEAM_DEFER
#define TEAM_DEFER 1
#endif
int team_layer0_tiles(int hidden_padded, int kind);     // layer-0 tiles per wave (weight packing)
int team_layer1_tiles(int hidden_padded, int kind);     // hidden-layer (head) tiles per wave
int64_t team_blocks(int64_t K, int hidden_padded, int kind);
size_t team_buf_bytes(int64_t K, int hidden_padded, int kind);
bool team_rw_ln_built();                                // the reward net's LayerNorm heads are in this build

// terminal value (terminal_value.hip): the parameter block's floats (kernels.h TerminalValueArgs) and the padded hidden
constexpr int kTvParamFloats = 64 + BCMPC_VALUE_MAX_LAYERS * BCMPC_VALUE_MAX_HIDDEN + 16;
int terminal_value_padded(int hidden);       // 16, 32, 64, 128 or 256 (-1: outside [1, 256])

}  // namespace bcmpc

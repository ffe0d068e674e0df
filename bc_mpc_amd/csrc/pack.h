// pack.h -- the host arithmetic of bcmpc_set_weights / bcmpc_set_policy / bcmpc_set_terminal_value: kernels into MFMA
// fragment order, power-of-two operand scales, LayerNorm folding, the normalisation constants.  Plain values in,
// plain values out (no HIP): a setter packs, uploads what it got and copies the scalars into the engine.  Beside them
// the owning host copies of the last net, which a team engine's fallback engine is set from.
#pragma once
#include <vector>

#include "engine_plan.h"

#pragma GCC visibility push(hidden)
namespace bcmpc::host {

// Dense kernel W [in][out] (tf.layers.dense layout) -> fragment order
// [tb][u][j][lane][r], t = tb*TB + j: element W[16u + 4(lane>>4) + r][16t + (lane&15)]
// (zero outside in x out).  See the layout note at the top of rollout.hip.
void pack_layer(const float* W, int in, int out, int Tin, int Tout, int TB, float* dst);
// Output layer of the policy: one 16-row output tile whose row n holds action
// rowmap[n] (or zero): the host places action j at row S-16+j, i.e. in exactly
// the lanes/registers where the dynamics' layer-0 input expects action j.
void pack_out_rows(const float* W, int in, int out, int Tin, const int* rowmap, float* dst);
// Split-f16 kernel (rollout_x3.h): W [in][out] scaled by sw, every element as
// hi = f16(w), lo = f16(w - hi), in fragment order [ws][p][j][hi|lo][lane][i],
// t = ws*TWp + j: lane's 8 halves of tile t, k-step p are W[k][n] with
// n = 16t + (lane&15), k = 32p + 16(i>>2) + 4(lane>>4) + (i&3) -- the k order in
// which an output tile pair's accumulators ARE the next layer's B fragment.
void pack_x3_layer(const float* W, int in, int out, int Pin, int Tout, int TWp, float sw, _Float16* dst);
// power of two s with max|W| * s in [2^11, 2^12) (1 for an all-zero kernel)
float x3_scale(const float* W, size_t n);
// Layer 0's row k multiplies input dimension k alone, so a power of two moves freely between the two: (x 2^-q)(w 2^q)
// is the same f32 product.  The split kernels scale a whole kernel by one power of two, which leaves a row that sits
// 2^-p below the kernel's largest entry with a subnormal lo half from p ~ 15 and no hi half from p ~ 26 -- the row of
// a near-constant observation (std_obs ~ 0), whose normalised input is as many binades above the others.  A row
// kRowFoldMin binades or more below the largest entry is therefore returned lifted into the largest entry's binade
// (row_exp[k] = q, at most kRowFoldMax), and pack_weights multiplies that dimension's normalisation divisor by 2^q.
// Rows nearer than that keep 22 bits or more as they are, and an ordinary net packs bit for bit as before.
constexpr int kRowFoldMin = 8, kRowFoldMax = 120;
std::vector<float> fold_layer0_rows(const float* W, int in, int out, int* row_exp);
// the scale of a LayerNorm output as the next layer's f16 operand: |LN(x)_i| <= sqrt(h) |gamma_i| + |beta_i|,
// and the power of two that keeps it below 2^12
float ln_out_scale(const float* gamma, const float* beta, int h);

struct PackedNet {                              // bcmpc_set_weights
    std::vector<float> w, b, ln;                // d_w [w_floats], d_b [b_floats], d_ln [ln_floats]
    double consts[kConstRows * kConstCols]{};   // rows 0..5 and 8, 9 of the consts block (6, 7: the action bounds)
    float winv[BCMPC_MAX_LAYERS + 1]{};         // split kernel: 1 / operand scales per layer
    float hsc[BCMPC_MAX_LAYERS]{};              // split LN nets: output scale of hidden layer l
    int row_exp[kConstCols]{};                  // split kernels: fold_layer0_rows' power of two per input dimension
    bool pp_fold_w = false;                     // rollout_pp's folded operands hold for these weights
    bool team_defer = false;                    // packed for rollout_team's deferred last LayerNorm
    double mean_reward = 0.0, std_reward = 0.0;
};
struct PackedPolicy {                           // bcmpc_set_policy
    std::vector<float> w, b;                    // d_pw [pw_floats], d_pb [PL][PHP] + kPolParams
    float pwinv[BCMPC_MAX_LAYERS + 1]{};
};
struct PackedValue {                            // bcmpc_set_terminal_value
    std::vector<float> w, params;               // packed kernels, [kTvParamFloats]
    size_t off[BCMPC_VALUE_MAX_LAYERS + 2]{};   // layer l's kernel at w + off[l]
    int HP = 0;                                 // terminal_value_padded(hidden)
};
// (the callers have checked the pointers: every array the plan's / the net's shape names is there)
void pack_weights(const EnginePlan& p, const bcmpc_weights& w, PackedNet* out);
void pack_policy(const EnginePlan& p, const bcmpc_policy& pol, PackedPolicy* out);
void pack_value_net(const bcmpc_value_net& v, PackedValue* out);

// ---- owning copies of what the C structs point at: captured in one call, handed back as a view in one call ----
struct LayerCopy {                              // per-layer arrays and the pointer table a view hands out
    std::vector<std::vector<float>> v;
    mutable std::vector<const float*> p;
    void clear() { v.clear(); }
    void add(const float* src, size_t n) { v.emplace_back(src, src + n); }
    const float* const* ptrs() const;
};
struct WeightsCopy {
    LayerCopy k, b, g, beta;
    std::vector<double> mean_obs, std_obs, mean_action, std_action, mean_deltas, std_deltas, mean_reward, std_reward;
    void capture(const EnginePlan& p, const bcmpc_weights& w);
    bcmpc_weights view() const;
};
struct PolicyCopy {
    LayerCopy k, b;
    std::vector<float> ob_mean, ob_std, logstd;
    void capture(const EnginePlan& p, const bcmpc_policy& pol);
    bcmpc_policy view(double explore) const;
};
struct ValueCopy {
    LayerCopy k, b;
    std::vector<float> ob_mean, ob_std;
    int L = 0, hidden = 0, S = 0;
    void capture(const bcmpc_value_net& v);
    bcmpc_value_net view() const;
};

}  // namespace bcmpc::host
#pragma GCC visibility pop

// pack_dump.cpp -- prints what the GPU-free half of bcmpc_create and of the three setters computes, over a fixed list
// of configurations that reaches every branch: every EnginePlan field (or the refusal's text), the scalars the
// setters copy into the engine, and a 64-bit FNV-1a hash plus the length of every packed buffer.  Two builds that print
// the same text pack the same bytes.  Links the planner, the packers and the kernel objects that define the shape
// queries; calls no HIP API, so it runs -- and takes a host sanitizer -- on a machine without a GPU:
//   F="-O2 -std=c++17 -ffp-contract=off"        (add -fsanitize=address,undefined -fno-sanitize-recover=all)
//   for u in engine_plan pack; do /opt/rocm/llvm/bin/clang++ $F -c bc_mpc_amd/csrc/$u.cpp -o build/$u.host.o; done
//   /opt/rocm/llvm/bin/clang++ $F -c tools/micro/pack_dump.cpp -o build/pack_dump.o
//   hipcc $F build/pack_dump.o build/engine_plan.host.o build/pack.host.o build/rollout.o build/rollout_grp.o \
//         build/rollout_x3.o build/rollout_x3_plain.o build/rollout_pp.o build/rollout_team.o build/terminal_value.o \
//         -o tools/micro/pack_dump
// (profiles/pack_dump.txt is its output.)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bc_mpc_amd/csrc/pack.h"

using namespace bcmpc::host;

// ---- the nets: small integers over a power of two, from one 64-bit LCG ----
struct Gen {
    uint64_t s;
    int next(int span) {                                // uniform in [-span, span]
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (int)((s >> 33) % (uint64_t)(2 * span + 1)) - span;
    }
};
struct Layers {                                         // per-layer arrays and their pointer table
    std::vector<std::vector<float>> v;
    std::vector<const float*> p;
    void add(Gen& g, size_t n, float scale, float base = 0.f) {
        v.emplace_back(n);
        for (float& x : v.back()) x = base + (float)g.next(64) * scale;
    }
    const float* const* ptrs() {
        p.clear();
        for (auto& x : v) p.push_back(x.data());
        return p.data();
    }
};
static std::vector<double> stats(Gen& g, int n, bool positive) {
    std::vector<double> v((size_t)n);
    for (double& x : v) x = positive ? (1 + std::abs(g.next(16))) / 4.0 : g.next(16) / 8.0;
    return v;
}
static std::vector<float> fstats(Gen& g, int n, bool positive) {
    std::vector<float> v((size_t)n);
    for (float& x : v) x = positive ? (float)(1 + std::abs(g.next(16))) / 4.f : (float)g.next(16) / 8.f;
    return v;
}

// ---- printing ----
static uint64_t fnv1a(const void* data, size_t bytes) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    uint64_t h = 1469598103934665603ULL;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ p[i]) * 1099511628211ULL;
    return h;
}
static void buffer(const char* name, const void* data, size_t bytes) {
    std::printf("  %s: %zu bytes fnv1a %016" PRIx64 "\n", name, bytes, fnv1a(data, bytes));
}
static void floats(const char* name, const float* v, int n) {
    std::printf("  %s:", name);
    for (int i = 0; i < n; ++i) std::printf(" %a", (double)v[i]);
    std::printf("\n");
}
static void sizes(const char* name, const size_t* v, int n) {
    std::printf("  %s:", name);
    for (int i = 0; i < n; ++i) std::printf(" %zu", v[i]);
    std::printf("\n");
}
template <class P>
static void print_plan(const P& p, size_t b_floats, size_t ln_floats, int head_tb) {
    std::printf("  reward %d f16 %d split %d HP %d T %d wpb %d kernel %d nw %d nc %d pack_tb %d head_tb %d nwl %d\n",
                (int)p.reward, (int)p.f16, (int)p.split, p.HP, p.T, p.wpb, p.kernel, p.nw, p.nc, p.pack_tb, head_tb, p.nwl);
    std::printf("  pp %d pp_fold %d pp3 %d team_kind %d PHP %d TP %d PL %d\n", (int)p.pp, (int)p.pp_fold, (int)p.pp3,
                p.team_kind, p.PHP, p.TP, p.PL);
    std::printf("  w_floats %zu b_floats %zu ln_floats %zu pw_floats %zu\n", p.w_floats, b_floats, ln_floats, p.pw_floats);
    sizes("w_off", p.w_off, BCMPC_MAX_LAYERS + 1);
    sizes("b_off", p.b_off, BCMPC_MAX_LAYERS + 1);
    sizes("pw_off", p.pw_off, BCMPC_MAX_LAYERS + 1);
}

// ---- the code under test: plan, then pack; every function prints what it got ----
static std::string g_error;
namespace bcmpc {
int set_error(int code, const std::string& msg) {      // (the library's is in capi.cpp)
    g_error = msg;
    return code;
}
}  // namespace bcmpc
struct Subject {
    EnginePlan plan;
    bool make(const bcmpc_config& c, const CreateOpts& opts, int ncu) {
        g_error.clear();
        const int rc = plan_engine(c, opts, ncu, &plan);
        if (rc) {
            std::printf("  refused (%d): %s\n", rc, g_error.c_str());
            return false;
        }
        print_plan(plan, plan.b_floats, plan.ln_floats, plan.head_tb);
        return true;
    }
    void weights(const bcmpc_weights& w) {
        PackedNet pk;
        pack_weights(plan, w, &pk);
        floats("winv", pk.winv, BCMPC_MAX_LAYERS + 1);
        floats("hsc", pk.hsc, BCMPC_MAX_LAYERS);
        std::printf("  pp_fold_w %d team_defer %d mean_reward %a std_reward %a\n", (int)pk.pp_fold_w, (int)pk.team_defer,
                    pk.mean_reward, pk.std_reward);
        buffer("w", pk.w.data(), pk.w.size() * sizeof(float));
        buffer("b", pk.b.data(), pk.b.size() * sizeof(float));
        buffer("ln", pk.ln.data(), pk.ln.size() * sizeof(float));
        for (int row : {0, 1, 2, 3, 4, 5, 8, 9}) {
            char name[32];
            std::snprintf(name, sizeof(name), "consts row %d", row);
            buffer(name, pk.consts + row * bcmpc::kConstCols, sizeof(double) * bcmpc::kConstCols);
        }
    }
    void policy(const bcmpc_policy& pol) {
        PackedPolicy pk;
        pack_policy(plan, pol, &pk);
        floats("pwinv", pk.pwinv, BCMPC_MAX_LAYERS + 1);
        buffer("pw", pk.w.data(), pk.w.size() * sizeof(float));
        buffer("pb", pk.b.data(), pk.b.size() * sizeof(float));
    }
};
static void value_net(const bcmpc_value_net& v) {
    PackedValue pk;
    pack_value_net(v, &pk);
    std::printf("  HP %d\n", pk.HP);
    sizes("off", pk.off, v.n_layers + 2);
    buffer("vw", pk.w.data(), pk.w.size() * sizeof(float));
    buffer("vparams", pk.params.data(), pk.params.size() * sizeof(float));
}
// ---- end of the code under test ----

struct Env { const char* name; const char* value; };
struct Case {
    const char* name;
    bcmpc_config cfg;
    std::vector<Env> env;
    float wscale;                                       // weights are integers in [-64, 64] x wscale
    bool no_team, no_pp3;
};

static bcmpc_config config(int S, int A, int hidden, int act, int ln, int64_t K, int prec, int kernel, int H = 5) {
    bcmpc_config c{};
    c.state_dim = S; c.action_dim = A; c.hidden = hidden; c.n_layers = 2; c.activation = act; c.layer_norm = ln;
    c.horizon = H; c.cost = BCMPC_COST_CHEETAH; c.num_paths = K; c.precision = prec; c.kernel = kernel;
    return c;
}
static bcmpc_config with_reward(bcmpc_config c) { c.model = BCMPC_MODEL_REWARD; c.cost = BCMPC_COST_REWARD; return c; }
static bcmpc_config with_policy(bcmpc_config c, int ph, int pl) { c.policy_hidden = ph; c.policy_layers = pl; return c; }

static void run(const Case& cs, bool pack) {
    std::printf("%s\n", cs.name);
    for (const Env& e : cs.env) setenv(e.name, e.value, 1);
    CreateOpts opts;
    opts.no_team = cs.no_team;
    opts.no_pp3 = cs.no_pp3;
    Subject s;
    const bool ok = s.make(cs.cfg, opts, 256);
    for (const Env& e : cs.env) unsetenv(e.name);
    if (!ok || !pack) return;
    const bcmpc_config& c = cs.cfg;
    const int S = c.state_dim, A = c.action_dim, h = c.hidden, L = c.n_layers;
    const bool rw = c.model == BCMPC_MODEL_REWARD;
    Gen g{0x9e3779b97f4a7c15ULL ^ (uint64_t)(h * 131 + S * 7 + A)};
    Layers k, b, gam, beta;
    const int nin[5] = {S + A, h, h, h, h}, nout[5] = {h, h, S, h, 1};
    for (int l = 0; l < (rw ? 5 : L + 1); ++l) {
        const int in = rw ? nin[l] : (l == 0 ? S + A : h), out = rw ? nout[l] : (l == L ? S : h);
        k.add(g, (size_t)in * out, cs.wscale);
        b.add(g, (size_t)out, 1.f / 128.f);
    }
    for (int l = 0; l < (rw ? 3 : L) && c.layer_norm; ++l) {
        gam.add(g, (size_t)h, 1.f / 128.f, 1.f);
        beta.add(g, (size_t)h, 1.f / 64.f);
    }
    const std::vector<double> mo = stats(g, S, false), so = stats(g, S, true), ma = stats(g, A, false),
                              sa = stats(g, A, true), md = stats(g, S, false), sd = stats(g, S, true),
                              mr = stats(g, 1, false), sr = stats(g, 1, true);
    bcmpc_weights w{};
    w.kernels = k.ptrs(); w.biases = b.ptrs();
    if (c.layer_norm) { w.ln_gamma = gam.ptrs(); w.ln_beta = beta.ptrs(); }
    w.mean_obs = mo.data(); w.std_obs = so.data(); w.mean_action = ma.data(); w.std_action = sa.data();
    w.mean_deltas = md.data(); w.std_deltas = sd.data();
    if (rw) { w.mean_reward = mr.data(); w.std_reward = sr.data(); }
    s.weights(w);
    if (c.policy_hidden > 0) {
        const int ph = c.policy_hidden, PL = c.policy_layers;
        Layers pk, pb;
        for (int l = 0; l <= PL; ++l) {
            const int in = l == 0 ? S : ph, out = l == PL ? A : ph;
            pk.add(g, (size_t)in * out, 1.f / 256.f);
            pb.add(g, (size_t)out, 1.f / 128.f);
        }
        const std::vector<float> om = fstats(g, S, false), os = fstats(g, S, true), ls = fstats(g, A, false);
        const bcmpc_policy pol{pk.ptrs(), pb.ptrs(), om.data(), os.data(), ls.data(), 0.25};
        s.policy(pol);
    }
}

int main() {
    const int TANH = BCMPC_ACT_TANH, RELU = BCMPC_ACT_RELU, AUTO = BCMPC_KERNEL_AUTO;
    const int FP32 = BCMPC_PREC_FP32, SPLIT = BCMPC_PREC_SPLIT_F16, F16 = BCMPC_PREC_F16;
    const float W = 1.f / 256.f;
    for (const char* v : {"BCMPC_TEAM", "BCMPC_SPLIT_PP", "BCMPC_F16_NC", "BCMPC_F16_NW", "BCMPC_F16_PP", "BCMPC_PP_FOLD"})
        unsetenv(v);
    const Case packed[] = {
        // fp32: the delta net on solo, group4 and group8, with and without LayerNorm; the reward net
        {"fp32 solo 2x64 tanh", config(20, 6, 64, TANH, 0, 64, FP32, BCMPC_KERNEL_SOLO), {}, W, false, false},
        {"fp32 solo 2x64 relu LN", config(20, 6, 64, RELU, 1, 64, FP32, BCMPC_KERNEL_SOLO), {}, W, false, false},
        {"fp32 group4 2x100 tanh", config(20, 6, 100, TANH, 0, 64, FP32, BCMPC_KERNEL_GROUP4), {}, W, false, false},
        {"fp32 group4 2x100 relu LN", config(20, 6, 100, RELU, 1, 64, FP32, BCMPC_KERNEL_GROUP4), {}, W, false, false},
        {"fp32 auto (group8) 2x128 tanh K 64", config(20, 6, 128, TANH, 0, 64, FP32, AUTO), {}, W, false, false},
        {"fp32 auto (group4) 2x128 tanh K 8192", config(20, 6, 128, TANH, 0, 8192, FP32, AUTO), {}, W, false, false},
        {"fp32 auto 3 layers x 40 tanh LN", [&] { bcmpc_config c = config(17, 6, 40, TANH, 1, 64, FP32, AUTO); c.n_layers = 3; c.cost = BCMPC_COST_NONE; return c; }(), {}, W, false, false},
        {"fp32 reward 100", with_reward(config(20, 6, 100, TANH, 0, 64, FP32, AUTO)), {}, W, false, false},
        {"fp32 reward 100 LN", with_reward(config(20, 6, 100, TANH, 1, 64, FP32, AUTO)), {}, W, false, false},
        // split precision, the delta net on the slab kernels
        {"split 2x500 tanh split1", config(20, 6, 500, TANH, 0, 64, SPLIT, BCMPC_KERNEL_SPLIT1), {}, W, false, false},
        {"split 2x500 tanh auto BCMPC_TEAM=0 K 4096", config(20, 6, 500, TANH, 0, 4096, SPLIT, AUTO), {{"BCMPC_TEAM", "0"}}, W, false, false},
        {"split 2x500 tanh auto K 16384 H 5 (split4)", config(20, 6, 500, TANH, 0, 16384, SPLIT, AUTO), {}, W, false, false},
        {"split 2x64 relu no_team", config(20, 6, 64, RELU, 0, 64, SPLIT, AUTO), {}, W, true, false},
        {"split 2x256 relu LN no_team", config(20, 6, 256, RELU, 1, 400, SPLIT, AUTO), {}, W, true, false},
        {"split 2x256 tanh LN split2", config(20, 6, 256, TANH, 1, 400, SPLIT, BCMPC_KERNEL_SPLIT2), {}, W, false, false},
        {"split reward 500 no_team", with_reward(config(20, 6, 500, TANH, 0, 400, SPLIT, AUTO)), {}, W, true, false},
        // single-pass f16: the plain layout, the 4 x 4 layout, rollout_pp with the fold on, off and failing its test
        {"f16 2x500 K 64 (plain)", config(20, 6, 500, TANH, 0, 64, F16, AUTO), {}, W, false, false},
        {"f16 2x500 K 32768 BCMPC_F16_PP=0 (4x4)", config(20, 6, 500, TANH, 0, 32768, F16, AUTO), {{"BCMPC_F16_PP", "0"}}, W, false, false},
        {"f16 2x500 K 32768 BCMPC_F16_NC=2 BCMPC_F16_NW=8", config(20, 6, 500, TANH, 0, 32768, F16, AUTO), {{"BCMPC_F16_NC", "2"}, {"BCMPC_F16_NW", "8"}}, W, false, false},
        {"f16 2x500 K 32768 (pp by threshold, fold)", config(20, 6, 500, TANH, 0, 32768, F16, AUTO), {}, W, false, false},
        {"f16 2x500 K 128 BCMPC_F16_PP=1 (pp, fold)", config(20, 6, 500, TANH, 0, 128, F16, AUTO), {{"BCMPC_F16_PP", "1"}}, W, false, false},
        {"f16 2x500 K 128 BCMPC_F16_PP=1 BCMPC_PP_FOLD=0", config(20, 6, 500, TANH, 0, 128, F16, AUTO), {{"BCMPC_F16_PP", "1"}, {"BCMPC_PP_FOLD", "0"}}, W, false, false},
        {"f16 2x500 K 128 BCMPC_F16_PP=1, weights fail the fold test", config(20, 6, 500, TANH, 0, 128, F16, AUTO), {{"BCMPC_F16_PP", "1"}}, 128.f, false, false},
        // rollout_pp3: forced, by threshold, switched off, kept off an ensemble member
        {"split 2x500 tanh K 64 BCMPC_SPLIT_PP=1 (pp3 forced)", config(20, 6, 500, TANH, 0, 64, SPLIT, AUTO), {{"BCMPC_SPLIT_PP", "1"}}, W, false, false},
        {"split 2x500 tanh K 32768 H 14 (pp3 by threshold)", config(20, 6, 500, TANH, 0, 32768, SPLIT, AUTO, 14), {}, W, false, false},
        {"split 2x500 tanh K 32768 H 14 BCMPC_SPLIT_PP=0", config(20, 6, 500, TANH, 0, 32768, SPLIT, AUTO, 14), {{"BCMPC_SPLIT_PP", "0"}}, W, false, false},
        {"split 2x500 tanh K 32768 H 14 no_pp3", config(20, 6, 500, TANH, 0, 32768, SPLIT, AUTO, 14), {}, W, false, true},
        // the team kernel: kind 0 (plain, and the deferred LayerNorm), kind 1, kind 2 with and without LayerNorm
        {"team auto 2x500 tanh K 400", config(20, 6, 500, TANH, 0, 400, SPLIT, AUTO), {}, W, false, false},
        {"team auto 2x256 relu LN K 400 (deferred LN)", config(20, 6, 256, RELU, 1, 400, SPLIT, AUTO), {}, W, false, false},
        {"team 2x200 tanh LN K 400", config(20, 6, 200, TANH, 1, 400, SPLIT, BCMPC_KERNEL_TEAM), {}, W, false, false},
        {"team auto 2x500 tanh + policy 2x64 K 400", with_policy(config(20, 6, 500, TANH, 0, 400, SPLIT, AUTO), 64, 2), {}, W, false, false},
        {"team reward 500 K 400", with_reward(config(20, 6, 500, TANH, 0, 400, SPLIT, BCMPC_KERNEL_TEAM)), {}, W, false, false},
        {"team reward 500 LN K 400", with_reward(config(20, 6, 500, TANH, 1, 400, SPLIT, BCMPC_KERNEL_TEAM)), {}, W, false, false},
        {"team reward 500 LN + policy 1x128 K 128", with_policy(with_reward(config(20, 6, 500, TANH, 1, 128, SPLIT, AUTO)), 128, 1), {}, W, false, false},
        // a fused policy off the team kernel: fp32 and split precision
        {"fp32 2x128 tanh + policy 2x64", with_policy(config(20, 6, 128, TANH, 0, 64, FP32, AUTO), 64, 2), {}, W, false, false},
        {"fp32 reward 100 + policy 1x32", with_policy(with_reward(config(20, 6, 100, TANH, 0, 64, FP32, AUTO)), 32, 1), {}, W, false, false},
        {"split 2x500 tanh + policy 2x64 no_team", with_policy(config(20, 6, 500, TANH, 0, 400, SPLIT, AUTO), 64, 2), {}, W, true, false},
    };
    for (const Case& cs : packed) run(cs, true);

    for (int L : {1, 4})
        for (int hidden : {16, 256}) {
            std::printf("value net %d x %d\n", L, hidden);
            const int S = 20;
            Gen g{0xd1b54a32d192ed03ULL ^ (uint64_t)(L * 1000 + hidden)};
            Layers k, b;
            for (int l = 0; l <= L; ++l) {
                const int in = l == 0 ? S : hidden, out = l == L ? 1 : hidden;
                k.add(g, (size_t)in * out, W);
                b.add(g, (size_t)out, 1.f / 128.f);
            }
            const std::vector<float> om = fstats(g, S, false), os = fstats(g, S, true);
            const bcmpc_value_net v{k.ptrs(), b.ptrs(), om.data(), os.data(), L, hidden, S, 0};
            value_net(v);
        }

    // every refusal of plan_engine ("reward model: state_dim must be <= 31" is shadowed by state_dim + action_dim <= 32)
    auto mod = [](bcmpc_config c, auto f) { f(c); return c; };
    const bcmpc_config base = config(20, 6, 500, TANH, 0, 64, FP32, AUTO), sbase = config(20, 6, 500, TANH, 0, 64, SPLIT, AUTO);
    const Case refused[] = {
        {"refusal: state_dim", mod(base, [](bcmpc_config& c) { c.state_dim = 0; }), {}, W, false, false},
        {"refusal: action_dim", mod(base, [](bcmpc_config& c) { c.action_dim = 17; }), {}, W, false, false},
        {"refusal: state_dim + action_dim", mod(base, [](bcmpc_config& c) { c.action_dim = 13; }), {}, W, false, false},
        {"refusal: n_layers", mod(base, [](bcmpc_config& c) { c.n_layers = 9; }), {}, W, false, false},
        {"refusal: hidden", mod(base, [](bcmpc_config& c) { c.hidden = 1025; }), {}, W, false, false},
        {"refusal: activation", mod(base, [](bcmpc_config& c) { c.activation = 7; }), {}, W, false, false},
        {"refusal: horizon", mod(base, [](bcmpc_config& c) { c.horizon = 0; }), {}, W, false, false},
        {"refusal: num_paths", mod(base, [](bcmpc_config& c) { c.num_paths = -1; }), {}, W, false, false},
        {"refusal: cost", mod(base, [](bcmpc_config& c) { c.cost = 9; }), {}, W, false, false},
        {"refusal: model", mod(base, [](bcmpc_config& c) { c.model = 5; }), {}, W, false, false},
        {"refusal: reward cost without the reward model", mod(base, [](bcmpc_config& c) { c.cost = BCMPC_COST_REWARD; }), {}, W, false, false},
        {"refusal: reward n_layers", mod(with_reward(base), [](bcmpc_config& c) { c.n_layers = 3; }), {}, W, false, false},
        {"refusal: reward relu", mod(with_reward(base), [](bcmpc_config& c) { c.activation = BCMPC_ACT_RELU; }), {}, W, false, false},
        {"refusal: reward hidden", mod(with_reward(base), [](bcmpc_config& c) { c.hidden = 600; }), {}, W, false, false},
        {"refusal: cheetah state_dim", mod(base, [](bcmpc_config& c) { c.state_dim = 10; }), {}, W, false, false},
        {"refusal: cost terms with a policy", mod(with_policy(base, 64, 2), [](bcmpc_config& c) { c.cost = BCMPC_COST_TERMS; }), {}, W, false, false},
        {"refusal: precision", mod(base, [](bcmpc_config& c) { c.precision = 9; }), {}, W, false, false},
        {"refusal: f16 relu", mod(base, [](bcmpc_config& c) { c.precision = BCMPC_PREC_F16; c.activation = BCMPC_ACT_RELU; }), {}, W, false, false},
        {"refusal: f16 kernel", mod(base, [](bcmpc_config& c) { c.precision = BCMPC_PREC_F16; c.kernel = BCMPC_KERNEL_TEAM; }), {}, W, false, false},
        {"refusal: split reward state_dim", mod(with_reward(sbase), [](bcmpc_config& c) { c.state_dim = 10; }), {}, W, false, false},
        {"refusal: split kernel group4", mod(sbase, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_GROUP4; }), {}, W, false, false},
        {"refusal: splitr", mod(sbase, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_SPLITR; }), {}, W, false, false},
        {"refusal: fp32 kernel split1", mod(base, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_SPLIT1; }), {}, W, false, false},
        {"refusal: group2", mod(base, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_GROUP2; }), {}, W, false, false},
        {"refusal: fp32 reward kernel solo", mod(with_reward(base), [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_SOLO; }), {}, W, false, false},
        {"refusal: policy hidden", with_policy(base, 200, 2), {}, W, false, false},
        {"refusal: policy layers", with_policy(base, 64, 9), {}, W, false, false},
        {"refusal: policy state_dim", mod(with_policy(base, 64, 2), [](bcmpc_config& c) { c.state_dim = 10; c.cost = BCMPC_COST_NONE; }), {}, W, false, false},
        {"refusal: policy dynamics hidden", mod(with_policy(base, 64, 2), [](bcmpc_config& c) { c.hidden = 64; }), {}, W, false, false},
        {"refusal: policy_mode", mod(with_policy(base, 64, 2), [](bcmpc_config& c) { c.policy_mode = 9; }), {}, W, false, false},
        {"refusal: fp32 policy kernel solo", mod(with_policy(base, 64, 2), [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_SOLO; }), {}, W, false, false},
        {"refusal: team does not fit (K)", mod(sbase, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_TEAM; c.num_paths = 100000; }), {}, W, false, false},
        {"refusal: team does not fit (3 layers)", mod(sbase, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_TEAM; c.n_layers = 3; }), {}, W, false, false},
        {"refusal: f16 layout", mod(base, [](bcmpc_config& c) { c.precision = BCMPC_PREC_F16; }), {{"BCMPC_F16_NC", "3"}}, W, false, false},
        {"refusal: split policy dynamics hidden", mod(with_policy(sbase, 64, 2), [](bcmpc_config& c) { c.hidden = 128; }), {}, W, true, false},
        {"refusal: split does not fit", mod(sbase, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_SPLIT4; c.hidden = 64; }), {}, W, false, false},
        {"refusal: split relu + policy off the team kernel", mod(with_policy(sbase, 64, 2), [](bcmpc_config& c) { c.activation = BCMPC_ACT_RELU; }), {}, W, true, false},
        {"refusal: split LN hidden 600", mod(sbase, [](bcmpc_config& c) { c.hidden = 600; c.layer_norm = 1; }), {}, W, false, false},
        {"refusal: unknown kernel", mod(base, [](bcmpc_config& c) { c.kernel = -1; }), {}, W, false, false},
        {"refusal: group8 does not fit", mod(base, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_GROUP8; c.hidden = 64; }), {}, W, false, false},
        {"refusal: solo hidden", mod(base, [](bcmpc_config& c) { c.kernel = BCMPC_KERNEL_SOLO; c.hidden = 600; }), {}, W, false, false},
    };
    for (const Case& cs : refused) run(cs, false);
    return 0;
}

// cost_dump.cpp -- prints what the GPU-free half of the cost-term setters computes (bc_mpc_amd/csrc/cost_terms.cpp),
// over a fixed set of lists that reaches every branch: every refusal's text, and after every accepted call the whole
// launch template -- the slots, the slot bytes the kernel reads, every TermDev as hex bits, the extended fields --
// with the launcher's verdict on it and the fields a launch binds from stored inputs.  Two builds that print the same
// text digest the same lists into the same launches.  Calls no HIP API, so it runs -- and takes a host sanitizer --
// on a machine without a GPU:
//   F="-O1 -g -std=c++17 -ffp-contract=off"     (add -fsanitize=address,undefined -fno-sanitize-recover=all)
//   g++ $F -I bc_mpc_amd/csrc tools/micro/cost_dump.cpp bc_mpc_amd/csrc/cost_terms.cpp -o tools/micro/cost_dump
// (profiles/cost_dump.txt is its output, recorded from the functions as they stood in capi.cpp and the two kernel
// units before cost_terms.cpp took them over.)
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../bc_mpc_amd/csrc/cost_terms.h"

using namespace bcmpc;

static std::string g_error;
namespace bcmpc {
int set_error(int code, const std::string& msg) {      // (the library's is in capi.cpp)
    g_error = msg;
    return code;
}
}  // namespace bcmpc

static double g_traj[1], g_costs[1], g_ref[1], g_prev[1];   // stand-ins for device buffers: only their nullness is read

// ---- the code under test: an engine's cost state behind the three setters ----
namespace {
struct Subject {
    bcmpc_config cfg{};
    host::CostState s;
    int set(const bcmpc_cost_term* t, int32_t n) { return host::set_terms(cfg, &s, t, n); }
    int set_x(const bcmpc_cost_term_x* t, int32_t n, int32_t n_ref) { return host::set_terms_x(cfg, &s, t, n, n_ref); }
    int set_done(const bcmpc_cost_term* c, int32_t n, double done_cost) {
        if (const int rc = host::check_termination(cfg, s, c, n, done_cost)) return rc;
        host::store_termination(cfg, &s, c, n, done_cost);
        return 0;
    }
    void set_inputs(int32_t ref_envs, int32_t ref_steps, int32_t prev_envs) {   // bcmpc_set_cost_inputs' bookkeeping
        s.in_ref_envs = ref_envs; s.in_ref_steps = ref_steps; s.in_prev_envs = prev_envs;
        s.has_inputs = true;
    }
    bool has_terms() const { return s.has_terms; }
    bool ext() const { return s.ext; }
    bool has_inputs() const { return s.has_inputs; }
    TermCostXArgs tpl() const { return s.tpl; }         // (a plain list: b alone is meaningful)
    int inputs(int32_t n_envs, host::CostInputs* in) const {
        return host::stored_inputs(s, cfg.num_paths, n_envs, g_ref, g_prev, in);
    }
    int inputs_one_env(int64_t K, host::CostInputs* in) const {   // bcmpc_trajectory_cost_steps_async's
        return host::stored_inputs_one_env(s, K, g_ref, g_prev, in);
    }
    // one launch of K candidates as term_cost_launch assembles it: the slot words, the verdict, the bound fields
    bool launch(int64_t K, const host::CostInputs& in, TermCostXArgs* x) const {
        *x = s.tpl;
        x->b.traj = g_traj; x->b.costs = g_costs; x->b.K = K;
        if (s.ext) host::bind_inputs(in, cfg.action_dim, x);
        const bool ok = host::term_launch_ok(x->b, s.ext ? x : nullptr);
        host::pack_slots(&x->b);
        return ok;
    }
};
}  // namespace
// ---- end of the code under test ----

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u;
}

constexpr int32_t kOneEnv = -1;     // n_envs of print_state: the inputs as bcmpc_trajectory_cost_steps_async takes them

static void print_state(const Subject& e, int32_t n_envs = 1) {
    std::printf("  has_terms %d ext %d has_inputs %d\n", (int)e.has_terms(), (int)e.ext(), (int)e.has_inputs());
    if (!e.has_terms()) return;
    host::CostInputs in{};
    const int64_t K = n_envs == kOneEnv ? 77 : e.cfg.num_paths;   // (the entry without a layout takes any K)
    if (e.ext()) {
        g_error.clear();
        const int rc = n_envs == kOneEnv ? e.inputs_one_env(K, &in) : e.inputs(n_envs, &in);
        if (rc) {
            std::printf("  inputs for %d environments refused (%d): %s\n", n_envs, rc, g_error.c_str());
            in = host::CostInputs{};                    // (the template still prints, over no inputs)
            in.env_paths = K;
        } else {
            std::printf("  inputs for %d environments: env_paths %" PRId64 " ref %d envs %d steps %d prev %d envs %d\n",
                        n_envs, in.env_paths, (int)(in.ref != nullptr), in.ref_envs, in.ref_steps,
                        (int)(in.prev != nullptr), in.prev_envs);
        }
    }
    TermCostXArgs x;
    const bool ok = e.launch(K, in, &x);
    const TermCostArgs& a = x.b;
    std::printf("  H %d S %d A %d n_terms %d n_done %d n_slots %d n_state_slots %d done_cost %016" PRIx64 " launch_ok %d\n",
                a.H, a.S, a.A, a.n_terms, a.n_done, a.n_slots, a.n_state_slots, bits(a.done_cost), (int)ok);
    std::printf("  slots:");
    for (int i = 0; i < a.n_slots; ++i) std::printf(" %d%c", a.slot_index[i], "sac"[a.slot_action[i]]);
    std::printf("\n  slot bytes:");
    for (int j = 0; j < BCMPC_MAX_COST_TERMS / 4; ++j) std::printf(" %08x", a.slot_word[j]);
    std::printf("\n");
    for (int t = 0; t < a.n_terms + a.n_done; ++t) {
        const TermDev& d = a.terms[t];
        std::printf("  %s %2d: meta %08x pad %08x weight %016" PRIx64 " param %016" PRIx64 " rparam %016" PRIx64 "\n",
                    t < a.n_terms ? "term" : "done", t < a.n_terms ? t : t - a.n_terms, d.meta, d.pad, bits(d.weight),
                    bits(d.param), bits(d.rparam));
    }
    if (e.ext())
        std::printf("  x: n_ref_slots %d n_ref %d has_rate %d env_paths %" PRId64 " ref %d env_stride %" PRId64
                    " row_stride %" PRId64 " prev %d env_stride %" PRId64 "\n",
                    x.n_ref_slots, x.n_ref, x.has_rate, x.env_paths, (int)(x.ref != nullptr), x.ref_env_stride,
                    x.ref_row_stride, (int)(x.prev != nullptr), x.prev_env_stride);
}

static void report(const char* what, int rc, const Subject& e, int32_t n_envs = 1) {
    if (rc) {
        std::printf("%s\n  refused (%d): %s\n", what, rc, g_error.c_str());
        return;
    }
    std::printf("%s\n", what);
    print_state(e, n_envs);
}

using Terms = std::vector<bcmpc_cost_term>;
using TermsX = std::vector<bcmpc_cost_term_x>;
static bcmpc_cost_term T(int kind, int source, int index, int cmp, double weight, double param) {
    bcmpc_cost_term t{};
    t.kind = kind; t.source = source; t.index = index; t.cmp = cmp; t.weight = weight; t.param = param;
    return t;
}
static bcmpc_cost_term_x X(int kind, int source, int index, int cmp, double weight, double param, int ref) {
    bcmpc_cost_term_x t{};
    t.kind = kind; t.source = source; t.index = index; t.cmp = cmp; t.weight = weight; t.param = param; t.ref = ref;
    return t;
}
static Subject engine(int cost = BCMPC_COST_TERMS) {
    Subject e;
    e.cfg.state_dim = 20; e.cfg.action_dim = 6; e.cfg.horizon = 9; e.cfg.num_paths = 130; e.cfg.cost = cost;
    return e;
}
static int set(Subject& e, const Terms& t) { g_error.clear(); return e.set(t.data(), (int32_t)t.size()); }
static int set_x(Subject& e, const TermsX& t, int n_ref) { g_error.clear(); return e.set_x(t.data(), (int32_t)t.size(), n_ref); }
static int set_done(Subject& e, const Terms& c, double dc) { g_error.clear(); return e.set_done(c.data(), (int32_t)c.size(), dc); }

int main() {
    const int TH = BCMPC_TERM_THRESHOLD, LIN = BCMPC_TERM_LINEAR, DIFF = BCMPC_TERM_DIFF, QUAD = BCMPC_TERM_QUADRATIC,
              RATE = BCMPC_TERM_RATE;
    const int ST = BCMPC_SRC_STATE, NX = BCMPC_SRC_NEXT_STATE, AC = BCMPC_SRC_ACTION;
    const int GE = BCMPC_CMP_GE, GT = BCMPC_CMP_GT, LE = BCMPC_CMP_LE, LT = BCMPC_CMP_LT;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    {   // every kind x source, every cmp, NEXT_STATE, slots shared between terms
        Subject e = engine();
        report("plain: every kind x source, every cmp", set(e, {
            T(TH, ST, 3, GE, 1.5, 0.25), T(TH, NX, 3, GT, -2.0, 0.5), T(TH, AC, 1, LE, 0.75, -0.125), T(TH, ST, 19, LT, 3.0, 1.0),
            T(LIN, ST, 0, 0, 0.1, 0.0), T(LIN, NX, 7, 0, -0.3, 0.0), T(LIN, AC, 5, 0, 1e-3, 0.0),
            T(DIFF, ST, 17, 0, -1.0, 0.01),
            T(QUAD, ST, 7, 0, 2.0, 1.25), T(QUAD, NX, 0, 0, 0.5, -0.7), T(QUAD, AC, 1, 0, 0.05, 0.0)}), e);
        report("plain: DIFF whose 1 / param leaves div_rn's range, both ways", set(e, {
            T(DIFF, ST, 2, 0, 1.0, 1e-200), T(DIFF, ST, 2, 0, 1.0, 0x1p600), T(DIFF, ST, 4, 0, 1.0, 3.0)}), e);
        report("plain: no state term (actions only)", set(e, {T(QUAD, AC, 0, 0, 1.0, 0.0), T(LIN, AC, 5, 0, 1.0, 0.0)}), e);
        report("plain: the empty list", set(e, {}), e);
    }
    {   // every refusal of the plain setter
        Subject e = engine();
        const struct { const char* name; Terms t; } bad[] = {
            {"refusal: unknown kind", {T(9, ST, 0, 0, 1, 0)}},
            {"refusal: RATE through the plain setter", {T(RATE, AC, 0, 0, 1, 0)}},
            {"refusal: unknown source", {T(LIN, 3, 0, 0, 1, 0)}},
            {"refusal: unknown cmp", {T(LIN, ST, 0, 0, 1, 0), T(TH, ST, 0, 4, 1, 0)}},
            {"refusal: DIFF on NEXT_STATE", {T(DIFF, NX, 0, 0, 1, 1)}},
            {"refusal: DIFF on ACTION", {T(DIFF, AC, 0, 0, 1, 1)}},
            {"refusal: state index", {T(LIN, ST, 20, 0, 1, 0)}},
            {"refusal: next-state index", {T(LIN, NX, -1, 0, 1, 0)}},
            {"refusal: action index", {T(LIN, AC, 6, 0, 1, 0)}},
            {"refusal: weight inf", {T(LIN, ST, 0, 0, inf, 0)}},
            {"refusal: param nan", {T(QUAD, ST, 0, 0, 1, nan)}},
            {"refusal: DIFF param 0", {T(DIFF, ST, 0, 0, 1, 0.0)}},
        };
        for (const auto& b : bad) report(b.name, set(e, b.t), e);
        g_error.clear();
        report("refusal: n = -1", e.set(bad[0].t.data(), -1), e);
        g_error.clear();
        report("refusal: n = 33", e.set(bad[0].t.data(), 33), e);
        g_error.clear();
        report("refusal: null list", e.set(nullptr, 1), e);
        Subject h = engine(BCMPC_COST_CHEETAH);
        report("refusal: plain setter, engine without BCMPC_COST_TERMS", set(h, {T(LIN, ST, 0, 0, 1, 0)}), h);
        report("refusal: x setter, engine without BCMPC_COST_TERMS", set_x(h, {X(LIN, ST, 0, 0, 1, 0, -1)}, 0), h);
        report("refusal: termination, engine without BCMPC_COST_TERMS", set_done(h, {T(TH, NX, 0, GE, 0, 1)}, 1.0), h);
        report("after the refusals: nothing stored", 0, e);
    }
    {   // the extended setter: RATE with and without channels, channels shared between terms, every refusal
        Subject e = engine();
        report("x: RATE without channels", set_x(e, {X(RATE, AC, 2, 0, 0.5, 7.0, -1), X(QUAD, ST, 1, 0, 1.0, 0.5, -1)}, 0), e);
        e.set_inputs(0, 0, 1);
        report("x: ... with one previous action stored", 0, e);
        report("x: channels shared between terms, RATE beside them", set_x(e, {
            X(QUAD, ST, 4, 0, 1.0, 9.0, 2), X(TH, NX, 4, GE, 2.0, 9.0, 2), X(TH, AC, 3, LT, 1.0, 9.0, 0), X(QUAD, NX, 8, 0, 0.25, 0.5, -1),
            X(RATE, AC, 3, 0, 0.1, 0.0, -1), X(RATE, AC, 0, 0, 0.2, 0.0, -1), X(LIN, ST, 8, 0, 1.0, 0.0, -1), X(DIFF, ST, 8, 0, 1.0, 0.05, -1)}, 3), e);
        e.set_inputs(1, 9, 0);
        report("x: ... with a per-step reference for all environments", 0, e);
        e.set_inputs(2, 1, 2);
        report("x: ... with per-environment inputs, 2 environments", 0, e, 2);
        report("x: ... asked for 5 environments", 0, e, 5);
        report("x: ... asked for 0 environments", 0, e, 0);
        report("x: ... asked for 4 environments (130 is no multiple)", 0, e, 4);
        report("x: channels only, n_ref above the highest channel named", set_x(e, {X(QUAD, ST, 0, 0, 1.0, 0.0, 1)}, 16), e);
        report("x: nothing extended in the list: the plain setter's", set_x(e, {X(LIN, ST, 5, 0, 1.0, 0.0, -1), X(QUAD, AC, 5, 0, 1.0, 0.0, -1)}, 4), e);
        bcmpc_cost_term_x r = X(LIN, ST, 0, 0, 1, 0, -1);
        r.reserved[1] = 1;
        const struct { const char* name; TermsX t; int n_ref; } bad[] = {
            {"refusal: reserved", {r}, 0},
            {"refusal: RATE on STATE", {X(RATE, ST, 0, 0, 1, 0, -1)}, 0},
            {"refusal: RATE action index", {X(RATE, AC, 6, 0, 1, 0, -1)}, 0},
            {"refusal: RATE weight nan", {X(RATE, AC, 0, 0, nan, 0, -1)}, 0},
            {"refusal: x unknown kind", {X(5, ST, 0, 0, 1, 0, -1)}, 0},
            {"refusal: ref -2", {X(QUAD, ST, 0, 0, 1, 0, -2)}, 2},
            {"refusal: ref = n_ref", {X(QUAD, ST, 0, 0, 1, 0, 2)}, 2},
            {"refusal: channel on LINEAR", {X(LIN, ST, 0, 0, 1, 0, 0)}, 1},
            {"refusal: channel on DIFF", {X(DIFF, ST, 0, 0, 1, 1, 0)}, 1},
            {"refusal: channel on RATE", {X(RATE, AC, 0, 0, 1, 0, 0)}, 1},
            {"refusal: n_ref 17", {X(LIN, ST, 0, 0, 1, 0, -1)}, 17},
            {"refusal: n_ref -1", {X(LIN, ST, 0, 0, 1, 0, -1)}, -1},
        };
        for (const auto& b : bad) report(b.name, set_x(e, b.t, b.n_ref), e);
        g_error.clear();
        report("refusal: x n = 33", e.set_x(bad[0].t.data(), 33, 0), e);
        g_error.clear();
        report("refusal: x null list", e.set_x(nullptr, 2, 0), e);
    }
    {   // done conditions: state slots of their own, every refusal
        Subject e = engine();
        report("termination before any cost term", set_done(e, {T(TH, NX, 11, LT, 0.0, 0.2)}, 4.0), e);
        report("plain terms under it: the conditions add state slots", set(e, {T(QUAD, AC, 2, 0, 1.0, 0.0), T(LIN, ST, 3, 0, 1.0, 0.0)}), e);
        report("termination: every cmp, a dim the terms read and two they do not", set_done(e, {
            T(TH, NX, 3, GE, 0.0, 1.0), T(TH, NX, 12, GT, 0.0, -1.0), T(TH, NX, 12, LE, 0.0, -2.0), T(TH, NX, 0, LT, 0.0, 0.5)}, -3.5), e);
        const struct { const char* name; Terms c; double dc; } bad[] = {
            {"refusal: condition kind", {T(LIN, NX, 0, 0, 0, 0)}, 1.0},
            {"refusal: condition source", {T(TH, ST, 0, GE, 0, 0)}, 1.0},
            {"refusal: condition cmp", {T(TH, NX, 0, -1, 0, 0)}, 1.0},
            {"refusal: condition index", {T(TH, NX, 20, GE, 0, 0)}, 1.0},
            {"refusal: condition param", {T(TH, NX, 0, GE, 0, inf)}, 1.0},
            {"refusal: condition weight", {T(TH, NX, 0, GE, 1.0, 0)}, 1.0},
            {"refusal: done_cost", {T(TH, NX, 0, GE, 0, 0)}, inf},
        };
        for (const auto& b : bad) report(b.name, set_done(e, b.c, b.dc), e);
        g_error.clear();
        report("refusal: 33 conditions", e.set_done(bad[0].c.data(), 33, 1.0), e);
        g_error.clear();
        report("refusal: null conditions", e.set_done(nullptr, 1, 1.0), e);
        report("termination cleared: done_cost goes with it", set_done(e, {}, 8.0), e);
    }
    {   // the 32-entry limit from the three setters' sides
        Terms t32;
        for (int i = 0; i < 32; ++i) t32.push_back(T(i % 2 ? LIN : QUAD, i < 20 ? ST : AC, i < 20 ? i : i - 20 < 6 ? i - 20 : 0, 0, 1.0 + i, 0.5));
        TermsX x32;
        for (int i = 0; i < 32; ++i) x32.push_back(X(QUAD, i < 20 ? ST : AC, i < 20 ? i : (i - 20) % 6, 0, 1.0, 0.5, i < 20 ? i % 6 : -1));
        Subject e = engine();
        report("32 plain terms", set(e, t32), e);
        report("refusal: 32 terms + 1 condition, from the termination side", set_done(e, {T(TH, NX, 0, GE, 0, 0)}, 1.0), e);
        report("32 extended terms: 20 dims + 6 channels + 6 actions = 32 slots", set_x(e, x32, 6), e);
        report("refusal: 32 extended terms + 1 condition", set_done(e, {T(TH, NX, 0, GE, 0, 0)}, 1.0), e);
        Subject f = engine();
        report("one condition first", set_done(f, {T(TH, NX, 5, GE, 0, 0)}, 1.0), f);
        report("refusal: 1 condition + 32 terms, from the plain side", set(f, t32), f);
        report("refusal: 1 condition + 32 terms, from the x side", set_x(f, x32, 6), f);
    }
    {   // the 32-slot limit: an extended term can bring a slot and a channel
        TermsX x17;
        for (int i = 0; i < 16; ++i) x17.push_back(X(TH, ST, i, GE, 1.0, 0.0, i));
        Subject e = engine();
        report("16 dims + 16 channels = 32 slots", set_x(e, x17, 16), e);
        report("... and a condition on a dim already read", set_done(e, {T(TH, NX, 15, LT, 0, 0)}, 2.0), e);
        report("refusal: a condition on a 17th dim, from the termination side", set_done(e, {T(TH, NX, 16, LT, 0, 0)}, 2.0), e);
        x17.push_back(X(LIN, AC, 0, 0, 1.0, 0.0, -1));
        report("refusal: 33 slots from the x side", set_x(e, x17, 16), e);
        Subject f = engine();
        report("a condition on dim 19 first", set_done(f, {T(TH, NX, 19, LT, 0, 0)}, 2.0), f);
        x17.pop_back();
        report("refusal: 32 slots + the condition's, from the x side", set_x(f, x17, 16), f);
    }
    {   // set-x -> set-termination -> set-plain -> set-x with another n_ref: n_ref survives a re-digest, stored
        // inputs do not survive a change of n_ref
        Subject e = engine();
        const TermsX a = {X(QUAD, ST, 2, 0, 1.0, 0.0, 1), X(RATE, AC, 4, 0, 0.5, 0.0, -1)};
        report("sequence: set-x, n_ref 3", set_x(e, a, 3), e);
        e.set_inputs(1, 1, 1);
        report("sequence: inputs stored", 0, e);
        report("sequence: set-termination (n_ref stays 3)", set_done(e, {T(TH, NX, 9, GT, 0.0, 0.1)}, 10.0), e);
        report("sequence: set-x again, same n_ref (inputs stay)", set_x(e, a, 3), e);
        report("sequence: set-plain", set(e, {T(LIN, ST, 2, 0, 1.0, 0.0)}), e);
        report("sequence: set-x, n_ref 3 after a plain list (inputs dropped)", set_x(e, a, 3), e);
        e.set_inputs(1, 9, 0);
        report("sequence: inputs stored", 0, e);
        report("sequence: set-x, n_ref 2 (inputs dropped)", set_x(e, a, 2), e);
        report("sequence: termination cleared", set_done(e, {}, 0.0), e);
        const TermsX rate_only = {X(RATE, AC, 1, 0, 1.0, 0.0, -1)};
        report("sequence: RATE only, n_ref 0", set_x(e, rate_only, 0), e);
        e.set_inputs(0, 0, 1);
        report("sequence: previous action stored", 0, e);
        report("sequence: set-plain", set(e, {T(LIN, ST, 2, 0, 1.0, 0.0)}), e);
        report("sequence: RATE only again, n_ref 0 (0 == 0: inputs stay)", set_x(e, rate_only, 0), e);
    }
    {   // the entry without an environment layout (one environment of K candidates), before and after a change of n_ref
        Subject e = engine();
        const TermsX a = {X(QUAD, ST, 2, 0, 1.0, 0.0, 1), X(RATE, AC, 4, 0, 0.5, 0.0, -1)};
        report("one environment: channels, no inputs yet", set_x(e, a, 3), e, kOneEnv);
        e.set_inputs(1, 9, 1);
        report("one environment: inputs stored", 0, e, kOneEnv);
        e.set_inputs(2, 1, 1);
        report("one environment: a reference per environment stored", 0, e, kOneEnv);
        e.set_inputs(1, 1, 2);
        report("one environment: a previous action per environment stored", 0, e, kOneEnv);
        e.set_inputs(1, 9, 1);
        report("one environment: n_ref 3 -> 2, the inputs dropped", set_x(e, a, 2), e, kOneEnv);
        report("one environment: ... RATE only, n_ref 0: the previous action stored earlier is still bound",
               set_x(e, {X(RATE, AC, 4, 0, 0.5, 0.0, -1)}, 0), e, kOneEnv);
        report("one environment: ... the same list through the layout entry binds none", 0, e, 1);
        report("one environment: a plain list takes no inputs", set(e, {T(LIN, ST, 2, 0, 1.0, 0.0)}), e, kOneEnv);
    }
    return 0;
}

// cost_terms.cpp -- the list logic of the declarative cost path (cost_terms.h): no HIP call in this unit.
#include "cost_terms.h"

#include <algorithm>
#include <cmath>

namespace bcmpc::host {

namespace {

// one cost term's checks (a done condition passes them too, then its own)
int check_cost_term(const bcmpc_config& c, const bcmpc_cost_term& T, const std::string& at) {
    if (T.kind < BCMPC_TERM_THRESHOLD || T.kind > BCMPC_TERM_QUADRATIC) return fail(BCMPC_ERR_ARG, at + "unknown kind");
    if (T.source < BCMPC_SRC_STATE || T.source > BCMPC_SRC_ACTION) return fail(BCMPC_ERR_ARG, at + "unknown source");
    if (T.kind == BCMPC_TERM_THRESHOLD && (T.cmp < BCMPC_CMP_GE || T.cmp > BCMPC_CMP_LT))
        return fail(BCMPC_ERR_ARG, at + "unknown cmp");
    if (T.kind == BCMPC_TERM_DIFF && T.source != BCMPC_SRC_STATE)
        return fail(BCMPC_ERR_ARG, at + "a DIFF term's source must be STATE");
    const int lim = T.source == BCMPC_SRC_ACTION ? c.action_dim : c.state_dim;
    if (T.index < 0 || T.index >= lim)
        return fail(BCMPC_ERR_ARG, at + "index " + std::to_string(T.index) + " outside [0, " + std::to_string(lim) + ")");
    if (!std::isfinite(T.weight) || !std::isfinite(T.param))
        return fail(BCMPC_ERR_ARG, at + "weight and param must be finite");
    if (T.kind == BCMPC_TERM_DIFF && T.param == 0.0) return fail(BCMPC_ERR_ARG, at + "a DIFF term's param must not be 0");
    return BCMPC_OK;
}

// the slots a list reads per row: its state dims (the conditions' included), its channels and its actions, each
// counted once
int count_slots(const std::vector<bcmpc_cost_term>& terms, const std::vector<bcmpc_cost_term>& conds,
                const std::vector<int32_t>& refs) {
    uint32_t seen[3] = {0, 0, 0};                        // state dims, actions, channels
    for (const auto* v : {&terms, &conds})
        for (const bcmpc_cost_term& T : *v) seen[T.source == BCMPC_SRC_ACTION ? 1 : 0] |= 1u << T.index;
    for (const int32_t r : refs)
        if (r >= 0) seen[2] |= 1u << r;
    return __builtin_popcount(seen[0]) + __builtin_popcount(seen[1]) + __builtin_popcount(seen[2]);
}

// the refusals every cost-term setter opens with
int check_list_call(const bcmpc_config& c, const void* terms, int32_t n) {
    if (c.cost != BCMPC_COST_TERMS) return fail(BCMPC_ERR_ARG, "cost terms need an engine created with BCMPC_COST_TERMS");
    if (n < 0 || n > BCMPC_MAX_COST_TERMS) return fail(BCMPC_ERR_ARG, "the number of cost terms must be in [0, 32]");
    if (n > 0 && !terms) return fail(BCMPC_ERR_ARG, "null argument");
    return BCMPC_OK;
}

int check_entries(size_t n_terms, size_t n_conds) {
    if (n_terms + n_conds > BCMPC_MAX_COST_TERMS)
        return fail(BCMPC_ERR_ARG, "cost terms plus done conditions must be at most 32 (" + std::to_string(n_terms) +
                                       " + " + std::to_string(n_conds) + ")");
    return BCMPC_OK;
}

// the one path every setter ends in: the lists are stored, the template follows them
void redigest(const bcmpc_config& c, CostState* s) {
    s->tpl = digest_terms(c, s->terms, s->conds, s->refs, s->n_ref, s->done_cost);
}

}  // namespace

TermCostXArgs digest_terms(const bcmpc_config& c, const std::vector<bcmpc_cost_term>& terms,
                           const std::vector<bcmpc_cost_term>& conds, const std::vector<int32_t>& refs, int32_t n_ref,
                           double done_cost) {
    TermCostXArgs x{};
    TermCostArgs& a = x.b;
    const int n = (int)terms.size(), nall = n + (int)conds.size();
    int slot_of[2][BCMPC_MAX_STATE], chan_slot[BCMPC_MAX_REF_CHANNELS];
    for (auto& row : slot_of)
        for (int& v : row) v = -1;
    for (int& v : chan_slot) v = -1;
    for (int pass = 0; pass < 3; ++pass)
        for (int t = 0; t < nall; ++t) {
            const bcmpc_cost_term& T = t < n ? terms[t] : conds[t - n];
            if (pass == 1) {                             // the channels: slots between the state dims and the actions
                const int r = t < (int)refs.size() ? refs[t] : -1;
                if (r >= 0 && chan_slot[r] < 0) {
                    chan_slot[r] = a.n_slots++;
                    a.slot_index[chan_slot[r]] = (uint8_t)r;
                    a.slot_action[chan_slot[r]] = 2;
                    ++x.n_ref_slots;
                }
                continue;
            }
            const int is_act = T.source == BCMPC_SRC_ACTION ? 1 : 0;
            if (is_act != pass / 2) continue;
            int& sl = slot_of[is_act][T.index];
            if (sl < 0) {
                sl = a.n_slots++;
                a.slot_index[sl] = (uint8_t)T.index;
                a.slot_action[sl] = (uint8_t)is_act;
                if (!is_act) a.n_state_slots = a.n_slots;
            }
            TermDev& d = a.terms[t];
            d.weight = T.weight; d.param = T.param;
            const bool rate = T.kind == BCMPC_TERM_RATE;
            if (rate) x.has_rate = 1;
            d.meta = (rate ? (uint32_t)BCMPC_TERM_QUADRATIC | 1u << 7 : (uint32_t)T.kind) |
                     (T.kind == BCMPC_TERM_THRESHOLD ? (uint32_t)T.cmp << 2 : 0u) |
                     (T.source == BCMPC_SRC_NEXT_STATE ? 1u << 4 : 0u) | (uint32_t)sl << 8;
            if (T.kind == BCMPC_TERM_DIFF) {
                // div_rn's precondition (device_common.h): r = RN(1 / b), and neither near the subnormals
                const double r = 1.0 / T.param, mb = std::fabs(T.param), mr = std::fabs(r);
                d.rparam = r;
                if (mb > 0x1p-500 && mb < 0x1p500 && mr > 0x1p-500 && mr < 0x1p500) d.meta |= 1u << 5;
            }
        }
    for (int t = 0; t < n && t < (int)refs.size(); ++t)          // p of a term with a channel: that channel's slot
        if (refs[t] >= 0) {
            a.terms[t].meta |= 1u << 6;
            a.terms[t].pad = (uint32_t)chan_slot[refs[t]];
        }
    a.n_terms = n;
    a.n_done = (int32_t)conds.size();
    a.done_cost = done_cost;
    a.H = c.horizon; a.S = c.state_dim; a.A = c.action_dim;
    x.n_ref = n_ref;                                     // (the rows of a call's reference have n_ref channels)
    return x;
}

int set_terms(const bcmpc_config& c, CostState* s, const bcmpc_cost_term* terms, int32_t n) {
    if (const int rc = check_list_call(c, terms, n)) return rc;
    for (int t = 0; t < n; ++t)
        if (const int rc = check_cost_term(c, terms[t], "cost term " + std::to_string(t) + ": ")) return rc;
    // (every entry adds at most one slot, so the slots fit whenever the entries do)
    if (const int rc = check_entries((size_t)n, s->conds.size())) return rc;
    s->terms.assign(terms, terms + n);
    s->refs.clear();                                     // (an extended list is replaced by a plain one)
    s->n_ref = 0;
    s->ext = false;
    s->has_terms = true;
    redigest(c, s);
    return BCMPC_OK;
}

int set_terms_x(const bcmpc_config& c, CostState* s, const bcmpc_cost_term_x* terms, int32_t n, int32_t n_ref) {
    if (const int rc = check_list_call(c, terms, n)) return rc;
    if (n_ref < 0 || n_ref > BCMPC_MAX_REF_CHANNELS) return fail(BCMPC_ERR_ARG, "n_ref must be in [0, 16]");
    std::vector<bcmpc_cost_term> plain((size_t)n);
    std::vector<int32_t> refs((size_t)n);
    bool ext = false;
    for (int t = 0; t < n; ++t) {
        const bcmpc_cost_term_x& X = terms[t];
        const std::string at = "cost term " + std::to_string(t) + ": ";
        bcmpc_cost_term T{X.kind, X.source, X.index, X.cmp, X.weight, X.param};
        if (X.reserved[0] != 0 || X.reserved[1] != 0 || X.reserved[2] != 0) return fail(BCMPC_ERR_ARG, at + "reserved must be 0");
        if (X.kind == BCMPC_TERM_RATE) {
            if (X.source != BCMPC_SRC_ACTION) return fail(BCMPC_ERR_ARG, at + "a RATE term's source must be ACTION");
            T.kind = BCMPC_TERM_QUADRATIC;               // (the remaining checks are a QUADRATIC's on the action)
            T.param = 0.0;
        }
        if (const int rc = check_cost_term(c, T, at)) return rc;
        if (X.ref < -1 || X.ref >= n_ref)
            return fail(BCMPC_ERR_ARG, at + "ref " + std::to_string(X.ref) + " outside [-1, n_ref = " + std::to_string(n_ref) + ")");
        if (X.ref >= 0 && X.kind != BCMPC_TERM_THRESHOLD && X.kind != BCMPC_TERM_QUADRATIC)
            return fail(BCMPC_ERR_ARG, at + "a reference channel stands only for a THRESHOLD's or a QUADRATIC's param");
        T.kind = X.kind;
        plain[(size_t)t] = T;
        refs[(size_t)t] = X.ref;
        ext = ext || X.ref >= 0 || X.kind == BCMPC_TERM_RATE;
    }
    if (const int rc = check_entries((size_t)n, s->conds.size())) return rc;
    const int slots = count_slots(plain, s->conds, refs);
    if (slots > BCMPC_MAX_COST_TERMS)
        return fail(BCMPC_ERR_ARG, "the list reads " + std::to_string(slots) + " slots per row (state dims, actions "
                                   "and reference channels, the done conditions' included): at most 32 fit");
    if (!ext) return set_terms(c, s, plain.data(), n);   // nothing extended in it: the plain setter's list
    if (s->n_ref != n_ref) s->has_inputs = false;        // inputs of another channel count do not carry over
    s->terms = plain;
    s->refs = refs;
    s->n_ref = n_ref;
    s->ext = true;
    s->has_terms = true;
    redigest(c, s);
    return BCMPC_OK;
}

int check_termination(const bcmpc_config& c, const CostState& s, const bcmpc_cost_term* conds, int32_t n,
                      double done_cost) {
    if (c.cost != BCMPC_COST_TERMS) return fail(BCMPC_ERR_ARG, "termination needs an engine created with BCMPC_COST_TERMS");
    if (n < 0 || n > BCMPC_MAX_COST_TERMS) return fail(BCMPC_ERR_ARG, "the number of done conditions must be in [0, 32]");
    if (n > 0 && !conds) return fail(BCMPC_ERR_ARG, "null argument");
    if (!std::isfinite(done_cost)) return fail(BCMPC_ERR_ARG, "done_cost must be finite");
    for (int t = 0; t < n; ++t) {
        const bcmpc_cost_term& T = conds[t];
        const std::string at = "done condition " + std::to_string(t) + ": ";
        if (T.kind != BCMPC_TERM_THRESHOLD) return fail(BCMPC_ERR_ARG, at + "the kind must be THRESHOLD");
        if (T.source != BCMPC_SRC_NEXT_STATE) return fail(BCMPC_ERR_ARG, at + "the source must be NEXT_STATE");
        if (const int rc = check_cost_term(c, T, at)) return rc;
        if (T.weight != 0.0) return fail(BCMPC_ERR_ARG, at + "the weight must be 0");
    }
    if (const int rc = check_entries(s.terms.size(), (size_t)n)) return rc;
    if (s.ext) {                                         // (a plain list's slots fit whenever its entries do)
        const int slots = count_slots(s.terms, std::vector<bcmpc_cost_term>(conds, conds + n), s.refs);
        if (slots > BCMPC_MAX_COST_TERMS)
            return fail(BCMPC_ERR_ARG, "the cost terms and these done conditions read " + std::to_string(slots) +
                                           " slots per row: at most 32 fit");
    }
    return BCMPC_OK;
}

void store_termination(const bcmpc_config& c, CostState* s, const bcmpc_cost_term* conds, int32_t n, double done_cost) {
    s->conds.assign(conds, conds + n);
    s->done_cost = n > 0 ? done_cost : 0.0;
    redigest(c, s);
}

// One rule set for both variants, the extended one's with no channels for a plain launch.  That is stricter on a
// plain template than launch_term_cost used to be -- slot_action must be exactly 0 or 1, meta bits 6 (channel) and
// 7 (RATE) must be clear -- in ways no template of digest_terms can trip
bool term_launch_ok(const TermCostArgs& a, const TermCostXArgs* x) {
    const int n_ref_slots = x ? x->n_ref_slots : 0, n_ref = x ? x->n_ref : 0;
    if (!a.traj || !a.costs || a.K < 1 || a.H < 1 || a.S < 1 || a.S > BCMPC_MAX_STATE || a.A < 1 ||
        a.A > BCMPC_MAX_ACTION || a.n_terms < 0 || a.n_done < 0 || a.n_terms + a.n_done > BCMPC_MAX_COST_TERMS ||
        a.n_slots < 0 || a.n_slots > (x ? BCMPC_MAX_COST_TERMS : a.n_terms + a.n_done) || a.n_state_slots < 0 ||
        n_ref_slots < 0 || a.n_state_slots + n_ref_slots > a.n_slots || !std::isfinite(a.done_cost))
        return false;
    if (x && (x->env_paths < 1 || a.K % x->env_paths != 0 || n_ref < 0 || n_ref > BCMPC_MAX_REF_CHANNELS ||
              (n_ref_slots > 0 && !x->ref) || x->ref_env_stride < 0 || x->ref_row_stride < 0 || x->prev_env_stride < 0))
        return false;
    const int act0 = a.n_state_slots + n_ref_slots;      // state dims, channels, actions
    for (int i = 0; i < a.n_slots; ++i) {
        const int want = i < a.n_state_slots ? 0 : i < act0 ? 2 : 1;
        const int lim = want == 0 ? a.S : want == 2 ? n_ref : a.A;
        if (a.slot_action[i] != want || a.slot_index[i] >= lim) return false;
    }
    for (int t = 0; t < a.n_terms + a.n_done; ++t) {
        const TermDev& T = a.terms[t];
        const int sl = (int)(T.meta >> 8);
        if (sl >= a.n_slots || (sl >= a.n_state_slots && sl < act0)) return false;     // a term reads no channel as x
        if (((T.meta >> 6) & 1u) && ((int)T.pad < a.n_state_slots || (int)T.pad >= act0)) return false;
        if (((T.meta >> 7) & 1u) && sl < act0) return false;                           // RATE reads an action
        if (t >= a.n_terms && sl >= a.n_state_slots) return false;                     // a done condition: a state
    }
    return true;
}

void pack_slots(TermCostArgs* a) {
    for (uint32_t& w : a->slot_word) w = 0;
    for (int i = 0; i < a->n_slots; ++i)
        a->slot_word[i >> 2] |= (uint32_t)(a->slot_index[i] | (a->slot_action[i] == 1 ? 0x80 : 0) |
                                           (a->slot_action[i] == 2 ? 0x40 : 0)) << (8 * (i & 3));
}

// the stored inputs as a launch's, every environment reading env_paths candidates
static CostInputs inputs_of(const CostState& s, int64_t env_paths, const double* d_ref, const double* d_prev) {
    CostInputs in{};
    in.env_paths = env_paths;
    in.ref = s.in_ref_envs ? d_ref : nullptr;
    in.ref_envs = s.in_ref_envs; in.ref_steps = s.in_ref_steps;
    in.prev = s.in_prev_envs ? d_prev : nullptr;
    in.prev_envs = s.in_prev_envs;
    return in;
}

int stored_inputs_one_env(const CostState& s, int64_t K, const double* d_ref, const double* d_prev, CostInputs* in) {
    if (s.tpl.n_ref_slots > 0 && !s.has_inputs)
        return fail(BCMPC_ERR_STATE, "the cost terms name reference channels: bcmpc_set_cost_inputs has not been called");
    if (s.in_ref_envs > 1 || s.in_prev_envs > 1)
        return fail(BCMPC_ERR_ARG, "the inputs were set for several environments: bcmpc_trajectory_cost_inputs_async "
                                   "takes the environment layout");
    *in = inputs_of(s, K, d_ref, d_prev);
    return BCMPC_OK;
}

int stored_inputs(const CostState& s, int64_t num_paths, int32_t n_envs, const double* d_ref, const double* d_prev,
                  CostInputs* in) {
    if (s.tpl.n_ref_slots > 0 && !s.has_inputs)
        return fail(BCMPC_ERR_STATE, "the cost terms name reference channels: bcmpc_set_cost_inputs has not been called");
    if (n_envs < 1 || num_paths % n_envs != 0) return fail(BCMPC_ERR_ARG, "num_paths is not a multiple of n_envs");
    *in = CostInputs{};
    in->env_paths = std::max<int64_t>(1, num_paths / n_envs);
    if (!s.has_inputs) return BCMPC_OK;
    if (s.in_ref_envs > 1 && s.in_ref_envs != n_envs)
        return fail(BCMPC_ERR_ARG, "the reference was set for " + std::to_string(s.in_ref_envs) +
                                       " environments, this call has " + std::to_string(n_envs));
    if (s.in_prev_envs > 1 && s.in_prev_envs != n_envs)
        return fail(BCMPC_ERR_ARG, "the previous actions were set for " + std::to_string(s.in_prev_envs) +
                                       " environments, this call has " + std::to_string(n_envs));
    *in = inputs_of(s, in->env_paths, d_ref, d_prev);
    return BCMPC_OK;
}

void bind_inputs(const CostInputs& in, int32_t action_dim, TermCostXArgs* x) {
    x->env_paths = in.env_paths;
    x->ref = x->n_ref_slots > 0 ? in.ref : nullptr;
    x->ref_row_stride = in.ref_steps > 1 ? x->n_ref : 0;
    x->ref_env_stride = in.ref_envs > 1 ? (int64_t)in.ref_steps * x->n_ref : 0;
    x->prev = x->has_rate ? in.prev : nullptr;
    x->prev_env_stride = in.prev_envs > 1 ? action_dim : 0;
}

}  // namespace bcmpc::host

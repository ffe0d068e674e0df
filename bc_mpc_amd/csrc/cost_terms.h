// cost_terms.h -- the declarative cost path's host logic: the argument blocks of term_cost.hip, the checks of the
// three list setters, the digest of the stored lists into the launch template, the launch validation and the
// binding of a launch's inputs.  Plain values in, plain values out (no HIP): tools/micro/cost_dump.cpp runs all of
// it without a device.
#pragma once
#include <stdint.h>

#include <vector>

#include "engine_plan.h"

namespace bcmpc {

// ---- declarative cost terms (term_cost.hip): costs[K] from a stored trajectory ----
// The host compacts what the terms read into at most BCMPC_MAX_COST_TERMS slots: slot i of row r is the
// state dim slot_index[i] of traj[r][k] (slot_action[i] == 0) or action slot_index[i] of step r (== 1, last).  A term
// reads its slot of row h (STATE, ACTION, DIFF's s) or of row h + 1 (NEXT_STATE, DIFF's s').
struct TermDev {                             // one bcmpc_cost_term as the kernel reads it: one 32-byte scalar load
    double weight, param;
    double rparam;                           // DIFF: RN(1 / param), div_rn's r
    uint32_t meta;                           // kind | cmp << 2 | (NEXT_STATE) << 4 | (div_rn applies) << 5 | slot << 8
    uint32_t pad;
};
struct TermCostArgs {
    const double* traj;                      // [H+1][K][S]
    const double* actions;                   // [H][K][A] or nullptr => regenerated (action slots only)
    const double* cem_mu;                    // [H][A] or nullptr: cem_action instead of rng_action
    const double* cem_sigma;
    double* costs;                           // [K]
    uint64_t seed;
    int64_t cand_offset, K;
    int32_t H, S, A, cem_iter;
    int32_t n_terms, n_slots, n_state_slots;  // slots [n_state_slots, n_slots) are the action slots
    uint8_t slot_index[BCMPC_MAX_COST_TERMS];
    uint8_t slot_action[BCMPC_MAX_COST_TERMS];
    uint32_t slot_word[BCMPC_MAX_COST_TERMS / 4];   // (filled by launch_term_cost) the two arrays, a byte per slot
    double low[BCMPC_MAX_ACTION], high[BCMPC_MAX_ACTION];   // action bounds (regenerated actions)
    TermDev terms[BCMPC_MAX_COST_TERMS];     // by value: 32 x 32 bytes, no per-launch upload
    // termination (cost_functions.episode_cost): terms[n_terms .. n_terms + n_done) are the done conditions
    // (THRESHOLD on NEXT_STATE, a state slot each, ORed); n_terms + n_done <= BCMPC_MAX_COST_TERMS
    int32_t n_done;
    double done_cost;                        // added once, at the terminating step
    int32_t* term_step;                      // [K] the terminating step, H: never; or nullptr (n_done > 0 only)
};

// ---- reference tracking (term_cost.hip's extended variant): lists with reference channels or RATE terms ----
// An argument struct of its own, so that the plain instances keep TermCostArgs as their kernel-argument block.  b is
// read as there, with three differences.  The slots are the state dims, then the reference channels
// (slot_action == 2, slot_index the channel), then the actions: slots [b.n_state_slots, b.n_state_slots +
// n_ref_slots) are the channels.  A TermDev's meta has bit 6 set where its param is the channel slot in `pad`,
// and bit 7 set for a RATE term (kind bits QUADRATIC).  Candidate k reads environment k / env_paths.
struct TermCostXArgs {
    TermCostArgs b;
    const double* ref;                       // [ref_envs][ref_steps][n_ref] or nullptr (n_ref_slots == 0)
    const double* prev;                      // [prev_envs][A] or nullptr: a_{-1} := a_0
    int64_t env_paths;                       // K is a multiple of it
    int64_t ref_env_stride;                  // ref_steps * n_ref, 0: one reference for all environments
    int64_t ref_row_stride;                  // n_ref, 0: constant over the horizon
    int64_t prev_env_stride;                 // A, 0: one previous action for all environments
    int32_t n_ref_slots, n_ref;
    int32_t has_rate;                        // the list has a RATE term: row -1 of the action slots is filled
};

}  // namespace bcmpc

#pragma GCC visibility push(hidden)
namespace bcmpc::host {

// What the list setters leave in an engine: the lists as given, and the launch template digested from all of them
// by whichever setter was called last.
struct CostState {
    std::vector<bcmpc_cost_term> terms, conds;   // cost terms (RATE sits here as kind 4), done conditions
    std::vector<int32_t> refs;                   // every term's channel or -1; empty for a plain list
    int32_t n_ref = 0;                           // channels per row of a call's reference (0 for a plain list)
    double done_cost = 0.0;
    bool has_terms = false;                      // a cost-term setter has been called
    bool ext = false;                            // the list names a channel or has a RATE term: the extended variant
    TermCostXArgs tpl{};                         // the launch template; a plain list launches tpl.b alone
    // what bcmpc_set_cost_inputs stored (its buffers are the engine's); in_prev_envs == 0: no previous action
    bool has_inputs = false;
    int32_t in_ref_envs = 0, in_ref_steps = 0, in_prev_envs = 0;
};

// the launch template of checked lists (the conditions follow the terms in TermCostArgs::terms).  The slots: every
// state dim the terms and the conditions read, then every channel, then every action -- the kernel wants the
// regenerated actions last.  n_ref is the caller's row width, not the highest channel named
TermCostXArgs digest_terms(const bcmpc_config& c, const std::vector<bcmpc_cost_term>& terms,
                           const std::vector<bcmpc_cost_term>& conds, const std::vector<int32_t>& refs, int32_t n_ref,
                           double done_cost);

// bcmpc_set_cost_terms / bcmpc_set_cost_terms_x behind the engine's null check: every refusal, then the list is
// stored and the template digested again.  set_terms_x with nothing extended in the list is set_terms
int set_terms(const bcmpc_config& c, CostState* s, const bcmpc_cost_term* terms, int32_t n);
int set_terms_x(const bcmpc_config& c, CostState* s, const bcmpc_cost_term_x* terms, int32_t n, int32_t n_ref);
// bcmpc_set_termination in two halves (the caller allocates the step buffer between them)
int check_termination(const bcmpc_config& c, const CostState& s, const bcmpc_cost_term* conds, int32_t n,
                      double done_cost);
void store_termination(const bcmpc_config& c, CostState* s, const bcmpc_cost_term* conds, int32_t n, double done_cost);

// what a launcher refuses (hipErrorInvalidValue): x == nullptr for the plain variant
bool term_launch_ok(const TermCostArgs& a, const TermCostXArgs* x);
// slot_word from slot_index / slot_action, the slots as the kernel reads them: index | channel << 6 | action << 7
void pack_slots(TermCostArgs* a);

// the inputs of one launch of an extended list (device pointers)
struct CostInputs {
    int64_t env_paths;
    const double* ref;  int32_t ref_envs, ref_steps;
    const double* prev; int32_t prev_envs;               // prev == nullptr: no previous action
};
// the stored inputs (d_ref / d_prev: the engine's buffers) for a launch of num_paths candidates over n_envs
// environments (none once a change of n_ref has invalidated them).  Checked before anything is launched
int stored_inputs(const CostState& s, int64_t num_paths, int32_t n_envs, const double* d_ref, const double* d_prev,
                  CostInputs* in);
// ... for bcmpc_trajectory_cost_steps_async, which takes no layout: one environment of K candidates.  (It reads the
// stored counts whether or not has_inputs still holds, as it always has: after a change of n_ref on a list without
// channels a previous action stored earlier is still bound.)
int stored_inputs_one_env(const CostState& s, int64_t K, const double* d_ref, const double* d_prev, CostInputs* in);
// the x fields of a launch from its inputs
void bind_inputs(const CostInputs& in, int32_t action_dim, TermCostXArgs* x);

}  // namespace bcmpc::host
#pragma GCC visibility pop

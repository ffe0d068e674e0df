// term_cost.hip -- declarative cost terms scored from a stored trajectory (gfx950).
//
// costs[k] = sum_h c_h(traj[h][k], a[h][k], traj[h+1][k]) for a list of at most 32 terms (include/bcmpc.h,
// bcmpc_cost_term): the objective of a BCMPC_COST_TERMS engine, launched between the rollout kernel (which
// writes the trajectory and no cost) and the ordinary argmin / select / MPPI kernels (which read costs[K]).
// One kernel template in two variants: the plain one (X = false, TermCostArgs) and the extended one (X = true,
// TermCostXArgs) for lists with reference channels or RATE terms; a list without either never runs the latter.
//
// One lane owns one candidate.  The terms of a step are added in list order and the steps in step order,
// each with one explicit round-to-nearest f64 intrinsic (the file is built with -ffp-contract=off), so a
// cost has the bits of the NumPy definition (cost_functions.TermCost under trajectory_cost_fn).
//
// Access pattern: per-lane row loads.  A lane reads only the values its terms name ("slots", compacted by
// the host: state dims first, then actions), 8 bytes each, from its own row; neighbouring lanes are S * 8
// bytes apart, so a wave's load touches up to 64 cache lines -- every line is still fetched from HBM once
// (a step's rows are contiguous over the candidates); the price is line requests, not bytes.  The
// alternative, a coalesced [64][S] tile staged through LDS, moves the same bytes and needs a barrier per
// row; DESIGN.md 9f has the device times that decided it.
//
// The walk is in trips of PF steps.  Row r + 1 is step r's s' and step r + 1's s: it is loaded once into
// registers, PF rows ahead, and moved into an LDS ring of PF + 1 rows ([row][slot][lane], lane-private, so no
// barrier) when its trip begins -- LDS because the terms index the slots with values only known at run time.
// The next trip's loads are issued before this trip is scored, so at small K, where a wave is a chain of
// dependent latencies, the memory latency is paid once per trip and overlaps the arithmetic.  A trip is
// scored term by term over its PF steps at once (PF independent accumulators): the term's 32-byte scalar
// load from the kernel arguments and the branch on its kind are paid once per trip, not once per step.
//
// Action slots: a[h][k][j] from the explicit [H][K][A] array, prefetched like a state dim, or regenerated
// per trip with the functions the rollout kernels call (rng_action / cem_action at global index
// cand_offset + k).  A cost without an ACTION term has no action slot and never runs Philox.
//
// Termination (the DONE instances; cost_functions.episode_cost is the definition): done conditions are further
// TermDev entries after the cost terms -- thresholds on the next state, combined with OR.  In a trip a condition
// sets bit u of a per-lane flag word instead of adding to acc[u]; the fold after the trip pays a step only while
// the candidate is alive and, on a flagged step, adds done_cost once, notes the step and pays nothing after it.
// The padded steps of the last trip (scored on the repeated row) neither pay nor terminate.  Dead lanes ride
// along to the end of the walk: a wave that leaves once all of its lanes are dead measured no faster.
//
// What the extended variant adds (the NumPy definition is episode_cost with reference / previous_action); every
// difference is an `if constexpr (X)` or the compile-time row offset P (the chain over a term's kind is written once
// per variant), so the plain instances keep their kernel-argument block and all forty instances the machine code they
// had as two units (profiles/term_cost_merge_digest.txt):
//
// * The environment.  A launch covers K = n_envs * env_paths candidates; lane k reads the reference and the
//   previous action of environment k / env_paths (local k).  env_paths need not be a multiple of 64, so the
//   lanes of a wave may belong to two or more environments: the index is per lane, computed once.
//
// * A reference channel is one more slot.  Its per-lane base is ref + env * ref_env_stride + c and its row
//   stride is n_ref (a reference per step) or 0 (constant over the horizon); row h is step h's, clamped to
//   H - 1 like an action's.  It rides the prefetch-ahead ring with the state dims, and a term's p becomes a
//   ring read like its x: no load inside the term loop, every load unconditional and in bounds.  The slots are
//   ordered state dims, channels, actions (the regenerated actions stay last).
//
// * RATE needs a_{h-1}.  The ring is one row deeper (P = 1, PF + 2 rows): in the trip of steps
//   h0 .. h0 + PF - 1 it holds rows h0 - 1 .. h0 + PF, so step h0 finds the action of step h0 - 1 where the
//   previous trip left it -- loaded from the explicit array, or regenerated there with the functions the
//   rollout kernels call.  Row -1 is written before the first trip: the previous action of the lane's
//   environment, or, without one, a_0 itself (d is then a_0 - a_0, as the definition has it).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/bcmpc.h"
#include "kernels.h"
#include "device_common.h"

namespace bcmpc {

namespace {

constexpr int kTermLanes = 64;               // one wave per workgroup: LDS columns are lane-private

// action j of step h as the rollout kernels draw it for global candidate g
__device__ __forceinline__ double term_regen(const TermCostArgs& a, int h, int j, uint64_t g) {
    if (a.cem_mu)
        return cem_action(a.seed, g, h, j, a.cem_iter, a.cem_mu[h * a.A + j], a.cem_sigma[h * a.A + j], a.low[j],
                          a.high[j]);
    return rng_action(a.seed, g, h, j, a.low[j], a.high[j]);
}

// a / b correctly rounded: div_rn (3 f64 operations) where its residual is exact -- b and r = RN(1 / b)
// normal (the host's `fast`), the quotient finite and a far from the subnormals -- else __ddiv_rn
__device__ __forceinline__ double term_div(double a, double b, double r, bool fast) {
    const double m = __builtin_fabs(a);
    if (fast && (m == 0.0 || (m > 0x1p-500 && m < 0x1p500))) return div_rn(a, b, r);
    return __ddiv_rn(a, b);
}

// (extended) row r of a slot: a channel's and an explicit action's rows end at H - 1, a state dim's at H (by
// value: the strides are uniform and stay in scalar registers)
__device__ __forceinline__ double load_slot(const double* p, uint32_t chan, uint32_t act, int r, int H, int64_t RS,
                                            int64_t KA, int64_t KS) {
    const int rs = r < H ? r : H, ra = r < H ? r : H - 1;
    const int64_t row = chan | act ? ra : rs;
    const int64_t stride = chan ? RS : act ? KA : KS;
    return p[row * stride];
}

// what a variant's argument block holds: the block both share, and the extended fields read outside `if constexpr`
__host__ __device__ __forceinline__ const TermCostArgs& term_base(const TermCostArgs& a) { return a; }
__host__ __device__ __forceinline__ const TermCostArgs& term_base(const TermCostXArgs& ax) { return ax.b; }
__host__ __device__ __forceinline__ TermCostArgs& term_base(TermCostArgs& a) { return a; }
__host__ __device__ __forceinline__ TermCostArgs& term_base(TermCostXArgs& ax) { return ax.b; }
__device__ __forceinline__ int64_t term_env(const TermCostArgs&, int64_t) { return 0; }
__device__ __forceinline__ int64_t term_env(const TermCostXArgs& ax, int64_t k) { return k / ax.env_paths; }
__device__ __forceinline__ int64_t term_ref_stride(const TermCostArgs&) { return 0; }
__device__ __forceinline__ int64_t term_ref_stride(const TermCostXArgs& ax) { return ax.ref_row_stride; }

template <bool X, int ND, int PF, bool REGEN, bool DONE>
__global__ __launch_bounds__(kTermLanes) void term_cost_kernel(
    const std::conditional_t<X, TermCostXArgs, TermCostArgs> ax) {
    constexpr int P = X ? 1 : 0;                         // rows the ring keeps behind row h0 (extended: row h0 - 1)
    constexpr int R = PF + 1 + P;                        // LDS ring: row r lives in rows[(r + P) % R], r >= -P
    __shared__ double rows[R][ND][kTermLanes];
    const TermCostArgs& a = term_base(ax);
    const int lane = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * kTermLanes + lane;
    if (k >= a.K) return;                                // tail lanes (no barrier follows)
    const uint64_t g = (uint64_t)(a.cand_offset + k);
    const int64_t env = term_env(ax, k);                 // (extended) this lane's environment
    const int nd = a.n_slots, H = a.H;

    // Every slot is a load with a per-lane base and a uniform row stride, set up once.  The slots, a byte each:
    // index | channel << 6 | action << 7.  A state dim walks the trajectory's rows 0 .. H; an action of the
    // explicit array walks that array's rows 0 .. H - 1, and so does a channel its environment's reference
    // rows.  A regenerated action's slot is filled when its trip is scored; its load reads state dim 0 instead,
    // a value that is then overwritten.  amask: the explicit-action slots; rmask: the channel slots.
    uint32_t sw[ND / 4];
#pragma unroll
    for (int j = 0; j < ND / 4; ++j) sw[j] = a.slot_word[j];
    const bool have_actions = a.actions != nullptr;
    const int64_t KS = a.K * a.S, KA = a.K * a.A, RS = term_ref_stride(ax);
    const double* sp[ND];
    uint32_t amask = 0, rmask = 0;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const uint32_t b = (sw[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const bool act = (b >> 7) != 0;
        if (act && have_actions) amask |= 1u << i;
        if constexpr (X) {
            const bool chan = ((b >> 6) & 1u) != 0;
            if (chan) rmask |= 1u << i;
            sp[i] = chan ? ax.ref + env * ax.ref_env_stride + (b & 31u)
                  : act  ? (have_actions ? a.actions + k * a.A + (b & 31u) : a.traj + k * a.S)
                         : a.traj + k * a.S + (b & 31u);
        } else {
            sp[i] = act ? (have_actions ? a.actions + k * a.A + (b & 31u) : a.traj + k * a.S)
                        : a.traj + k * a.S + (b & 31u);
        }
    }
    // (one load instruction per slot and row, no branch around it: a load whose value passes through a select
    //  or a guarded block is waited for at once, and nothing would stay in flight.  Rows past the last -- H,
    //  or H - 1 of the action array or a reference -- repeat it, slots past n_slots read state dim 0: in
    //  bounds, never used)
    auto load = [&](int i, int r) -> double {
        if constexpr (X) {
            return load_slot(sp[i], (rmask >> i) & 1u, (amask >> i) & 1u, r, H, RS, KA, KS);
        } else {
            r = r < H ? r : H;
            const int64_t off = (amask >> i) & 1u ? (int64_t)(r < H ? r : H - 1) * KA : (int64_t)r * KS;
            return sp[i][off];
        }
    };

    // row 0 into LDS; rows 1 .. PF into the registers
#pragma unroll
    for (int i = 0; i < ND; ++i) rows[P][i][lane] = load(i, 0);
    double pf[PF][ND];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int i = 0; i < ND; ++i) pf[u][i] = load(i, u + 1);

    auto act0 = [&]() -> int {                           // the first action slot (the channels sit before it)
        if constexpr (X) return a.n_state_slots + ax.n_ref_slots;
        else return a.n_state_slots;
    };

    // (extended) row -1, the action slots of a list with RATE terms: the environment's previous action, else a_0
    if constexpr (X) {
        if (ax.has_rate) {
#pragma unroll 1
            for (int i = act0(); i < nd; ++i) {
                const int j = (a.slot_word[i >> 2] >> (8 * (i & 3))) & 31u;
                rows[0][i][lane] = ax.prev      ? ax.prev[env * ax.prev_env_stride + j]
                                   : have_actions ? rows[1][i][lane]
                                                  : term_regen(a, 0, j, g);
            }
        }
    }

    // The terms are uniform, one 32-byte scalar load each: term t + 1 (term 0 of the next trip after the
    // last) is requested before term t is evaluated.
    const int nc = a.n_terms;                            // the cost terms; the done conditions follow them
    const int nt = DONE ? nc + a.n_done : nc;
    TermDev cur = a.terms[0];
    int tn = 0;

    double total = 0.0;
    bool dead = false;                                   // (DONE) the candidate has terminated, at step tstep
    int tstep = H;
#pragma unroll 1
    for (int h0 = 0; h0 < H; h0 += PF) {
        // rows h0 + 1 .. h0 + PF arrive and go to the ring; their registers take the next trip's rows
        const int b0 = h0 % R;                           // ring position of row h0 - P
        auto pos = [&](int v) { return b0 + v < R ? b0 + v : b0 + v - R; };   // ... of row h0 - P + v
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int i = 0; i < ND; ++i) rows[pos(u + 1 + P)][i][lane] = pf[u][i];
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int i = 0; i < ND; ++i) pf[u][i] = load(i, h0 + PF + u + 1);

        if (REGEN && !have_actions) {                    // the action slots (the last ones) of the trip's steps
#pragma unroll 1
            for (int u = 0; u < PF; ++u) {
                if (h0 + u >= H) break;
#pragma unroll 1
                for (int i = act0(); i < nd; ++i)
                    rows[pos(u + P)][i][lane] =
                        term_regen(a, h0 + u, (a.slot_word[i >> 2] >> (8 * (i & 3))) & 31u, g);
            }
        }

        // steps past H - 1 in the last trip are scored on the repeated row and dropped below
        double acc[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) acc[u] = 0.0;
        uint32_t flags = 0;                              // (DONE) bit u: a condition holds on step h0 + u's s'
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            tn = tn + 1 < nt ? tn + 1 : 0;
            const TermDev T = cur;
            cur = a.terms[tn];
            // The chain over a term's kind is written once per variant.  Shared, with the channel read of p and the
            // RATE branch guarded, it compiled to the two-unit build's code in 30 of the 40 instances only: a local
            // that reads T.pad must not exist in a plain instance and must sit here, ahead of the chain, in an
            // extended one (profiles/term_cost_merge_digest.txt).  A new kind or comparison goes into both.
            if constexpr (X) {
                const uint32_t kind = T.meta & 3u, cmp = (T.meta >> 2) & 3u;
                const int sl = (int)(T.meta >> 8);
                const int nx = (T.meta >> 4) & 1u;           // NEXT_STATE: the value of row h + 1
                const bool chan = (T.meta >> 6) & 1u;        // p is the channel slot T.pad of row h
                const int psl = (int)T.pad;
                const double w = T.weight, p = T.param;
                if (DONE && t >= nc) {
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double x = rows[pos(u + 1 + P)][sl][lane];
                        const bool hit = cmp == BCMPC_CMP_GE ? x >= p : cmp == BCMPC_CMP_GT ? x > p
                                       : cmp == BCMPC_CMP_LE ? x <= p : x < p;
                        flags |= (hit ? 1u : 0u) << u;
                    }
                } else if ((T.meta >> 7) & 1u) {             // RATE
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double d = __dsub_rn(rows[pos(u + P)][sl][lane], rows[pos(u)][sl][lane]);
                        acc[u] = __dadd_rn(acc[u], __dmul_rn(w, __dmul_rn(d, d)));
                    }
                } else if (kind == BCMPC_TERM_DIFF) {
                    const bool fast = (T.meta >> 5) & 1u;
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double d = __dsub_rn(rows[pos(u + 1 + P)][sl][lane], rows[pos(u + P)][sl][lane]);
                        acc[u] = __dadd_rn(acc[u], __dmul_rn(w, term_div(d, p, T.rparam, fast)));
                    }
                } else if (kind == BCMPC_TERM_THRESHOLD) {
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double x = rows[nx ? pos(u + 1 + P) : pos(u + P)][sl][lane];
                        const double q = chan ? rows[pos(u + P)][psl][lane] : p;
                        const bool hit = cmp == BCMPC_CMP_GE ? x >= q : cmp == BCMPC_CMP_GT ? x > q
                                       : cmp == BCMPC_CMP_LE ? x <= q : x < q;
                        acc[u] = hit ? __dadd_rn(acc[u], w) : acc[u];
                    }
                } else if (kind == BCMPC_TERM_LINEAR) {
#pragma unroll
                    for (int u = 0; u < PF; ++u)
                        acc[u] = __dadd_rn(acc[u], __dmul_rn(w, rows[nx ? pos(u + 1 + P) : pos(u + P)][sl][lane]));
                } else {
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double q = chan ? rows[pos(u + P)][psl][lane] : p;
                        const double d = __dsub_rn(rows[nx ? pos(u + 1 + P) : pos(u + P)][sl][lane], q);
                        acc[u] = __dadd_rn(acc[u], __dmul_rn(w, __dmul_rn(d, d)));
                    }
                }
            } else {
                const uint32_t kind = T.meta & 3u, cmp = (T.meta >> 2) & 3u;
                const int sl = (int)(T.meta >> 8);
                const int nx = (T.meta >> 4) & 1u;           // NEXT_STATE: the value of row h + 1
                const double w = T.weight, p = T.param;
                if (DONE && t >= nc) {
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double x = rows[pos(u + 1)][sl][lane];
                        const bool hit = cmp == BCMPC_CMP_GE ? x >= p : cmp == BCMPC_CMP_GT ? x > p
                                       : cmp == BCMPC_CMP_LE ? x <= p : x < p;
                        flags |= (hit ? 1u : 0u) << u;
                    }
                } else if (kind == BCMPC_TERM_DIFF) {
                    const bool fast = (T.meta >> 5) & 1u;
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double d = __dsub_rn(rows[pos(u + 1)][sl][lane], rows[pos(u)][sl][lane]);
                        acc[u] = __dadd_rn(acc[u], __dmul_rn(w, term_div(d, p, T.rparam, fast)));
                    }
                } else if (kind == BCMPC_TERM_THRESHOLD) {
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double x = rows[nx ? pos(u + 1) : pos(u)][sl][lane];
                        const bool hit = cmp == BCMPC_CMP_GE ? x >= p : cmp == BCMPC_CMP_GT ? x > p
                                       : cmp == BCMPC_CMP_LE ? x <= p : x < p;
                        acc[u] = hit ? __dadd_rn(acc[u], w) : acc[u];
                    }
                } else if (kind == BCMPC_TERM_LINEAR) {
#pragma unroll
                    for (int u = 0; u < PF; ++u)
                        acc[u] = __dadd_rn(acc[u], __dmul_rn(w, rows[nx ? pos(u + 1) : pos(u)][sl][lane]));
                } else {
#pragma unroll
                    for (int u = 0; u < PF; ++u) {
                        const double d = __dsub_rn(rows[nx ? pos(u + 1) : pos(u)][sl][lane], p);
                        acc[u] = __dadd_rn(acc[u], __dmul_rn(w, __dmul_rn(d, d)));
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            if (DONE) {
                if (!dead && h0 + u < H) {
                    total = __dadd_rn(total, acc[u]);    // the terminating step is still paid
                    if ((flags >> u) & 1u) {
                        total = __dadd_rn(total, a.done_cost);
                        dead = true;
                        tstep = h0 + u;
                    }
                }
            } else if (h0 + u < H) {
                total = __dadd_rn(total, acc[u]);
            }
        }
    }
    a.costs[k] = total;
    if (DONE && a.term_step) a.term_step[k] = tstep;
}

template <bool X, int ND, int PF>
hipError_t launch_t(std::conditional_t<X, TermCostXArgs, TermCostArgs> ax, hipStream_t st) {
    TermCostArgs& a = term_base(ax);
    host::pack_slots(&a);                                // the slots as the kernel reads them, a byte each
    int n_ref_slots = 0;
    if constexpr (X) n_ref_slots = ax.n_ref_slots;
    const bool regen = !a.actions && a.n_state_slots + n_ref_slots < a.n_slots;   // Philox only where an ACTION
    const int64_t blocks = (a.K + kTermLanes - 1) / kTermLanes;                   // term needs it
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(kTermLanes);
    if (a.n_done > 0) {                                  // termination: the DONE instances, a family of their own
        if (regen) hipLaunchKernelGGL((term_cost_kernel<X, ND, PF, true, true>), grid, block, 0, st, ax);
        else hipLaunchKernelGGL((term_cost_kernel<X, ND, PF, false, true>), grid, block, 0, st, ax);
    } else if (regen) {
        hipLaunchKernelGGL((term_cost_kernel<X, ND, PF, true, false>), grid, block, 0, st, ax);
    } else {
        hipLaunchKernelGGL((term_cost_kernel<X, ND, PF, false, false>), grid, block, 0, st, ax);
    }
    return hipGetLastError();
}

// ND slots (every one is loaded: the smallest instance that holds n_slots, the channels counted in) x PF rows in
// flight: at most 32 doubles (64 VGPRs) of prefetch registers in every instance
template <bool X>
hipError_t launch_any(const std::conditional_t<X, TermCostXArgs, TermCostArgs>& ax, hipStream_t st) {
    const TermCostArgs& a = term_base(ax);
    const TermCostXArgs* x = nullptr;
    if constexpr (X) x = &ax;
    if (!host::term_launch_ok(a, x)) return hipErrorInvalidValue;
    if (a.n_slots <= 4) return launch_t<X, 4, 8>(ax, st);
    if (a.n_slots <= 8) return launch_t<X, 8, 4>(ax, st);
    if (a.n_slots <= 16) return launch_t<X, 16, 2>(ax, st);
    if (a.n_slots <= 24) return launch_t<X, 24, 1>(ax, st);
    return launch_t<X, 32, 1>(ax, st);
}

}  // namespace

hipError_t launch_term_cost(const TermCostArgs& a, hipStream_t st) { return launch_any<false>(a, st); }
hipError_t launch_term_cost_x(const TermCostXArgs& ax, hipStream_t st) { return launch_any<true>(ax, st); }

}  // namespace bcmpc

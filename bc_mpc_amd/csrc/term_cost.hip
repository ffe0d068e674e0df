// term_cost.hip -- declarative cost terms scored from a stored trajectory (gfx950).
//
// costs[k] = sum_h c_h(traj[h][k], a[h][k], traj[h+1][k]) for a list of at most 32 terms (include/bcmpc.h,
// bcmpc_cost_term): the objective of a BCMPC_COST_TERMS engine, launched between the rollout kernel (which
// writes the trajectory and no cost) and the ordinary argmin / select / MPPI kernels (which read costs[K]).
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

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

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

template <int ND, int PF, bool REGEN, bool DONE>
__global__ __launch_bounds__(kTermLanes) void term_cost_kernel(const TermCostArgs a) {
    constexpr int R = PF + 1;                            // LDS ring: row r lives in rows[r % R]
    __shared__ double rows[R][ND][kTermLanes];
    const int lane = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * kTermLanes + lane;
    if (k >= a.K) return;                                // tail lanes (no barrier follows)
    const uint64_t g = (uint64_t)(a.cand_offset + k);
    const int nd = a.n_slots, H = a.H;

    // Every slot is a load with a per-lane base and a uniform row stride, set up once: a state dim walks the
    // trajectory's rows 0 .. H; an action of the explicit array walks that array's rows 0 .. H - 1.  A
    // regenerated action's slot is filled when its trip is scored; its load reads state dim 0 instead, a
    // value that is then overwritten.  amask: the explicit-action slots.
    uint32_t sw[ND / 4];
#pragma unroll
    for (int j = 0; j < ND / 4; ++j) sw[j] = a.slot_word[j];
    const bool have_actions = a.actions != nullptr;
    const int64_t KS = a.K * a.S, KA = a.K * a.A;
    const double* sp[ND];
    uint32_t amask = 0;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const uint32_t b = (sw[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const bool act = (b >> 7) != 0;
        if (act && have_actions) amask |= 1u << i;
        sp[i] = act ? (have_actions ? a.actions + k * a.A + (b & 31u) : a.traj + k * a.S)
                    : a.traj + k * a.S + (b & 31u);
    }
    // (one load instruction per slot and row, no branch around it: a load whose value passes through a select
    //  or a guarded block is waited for at once, and nothing would stay in flight.  Rows past the last -- H,
    //  or H - 1 of the action array -- repeat it, slots past n_slots read state dim 0: in bounds, never used)
    auto load = [&](int i, int r) -> double {
        r = r < H ? r : H;
        const int64_t off = (amask >> i) & 1u ? (int64_t)(r < H ? r : H - 1) * KA : (int64_t)r * KS;
        return sp[i][off];
    };

    // row 0 into LDS; rows 1 .. PF into the registers
#pragma unroll
    for (int i = 0; i < ND; ++i) rows[0][i][lane] = load(i, 0);
    double pf[PF][ND];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int i = 0; i < ND; ++i) pf[u][i] = load(i, u + 1);

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
        const int b0 = h0 % R;                           // ring position of row h0
        auto pos = [&](int u) { return b0 + u < R ? b0 + u : b0 + u - R; };   // ... of row h0 + u
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int i = 0; i < ND; ++i) rows[pos(u + 1)][i][lane] = pf[u][i];
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int i = 0; i < ND; ++i) pf[u][i] = load(i, h0 + PF + u + 1);

        if (REGEN && !have_actions) {                    // the action slots (the last ones) of the trip's steps
#pragma unroll 1
            for (int u = 0; u < PF; ++u) {
                if (h0 + u >= H) break;
#pragma unroll 1
                for (int i = a.n_state_slots; i < nd; ++i)
                    rows[pos(u)][i][lane] =
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

template <int ND, int PF>
hipError_t launch_t(TermCostArgs a, hipStream_t st) {
    for (int i = 0; i < a.n_slots; ++i)          // the slots as the kernel reads them: index | action << 7, a byte each
        a.slot_word[i >> 2] |= (uint32_t)(a.slot_index[i] | (a.slot_action[i] ? 0x80 : 0)) << (8 * (i & 3));
    const bool regen = !a.actions && a.n_state_slots < a.n_slots;     // Philox only where an ACTION term needs it
    const int64_t blocks = (a.K + kTermLanes - 1) / kTermLanes;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(kTermLanes);
    if (a.n_done > 0) {                                  // termination: the DONE instances, a family of their own
        if (regen) hipLaunchKernelGGL((term_cost_kernel<ND, PF, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((term_cost_kernel<ND, PF, false, true>), grid, block, 0, st, a);
    } else if (regen) {
        hipLaunchKernelGGL((term_cost_kernel<ND, PF, true, false>), grid, block, 0, st, a);
    } else {
        hipLaunchKernelGGL((term_cost_kernel<ND, PF, false, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace

// ND slots (every one is loaded: the smallest instance that holds n_slots) x PF rows in flight: at most 32
// doubles (64 VGPRs) of prefetch registers in every instance
hipError_t launch_term_cost(const TermCostArgs& a, hipStream_t st) {
    if (!a.traj || !a.costs || a.K < 1 || a.H < 1 || a.S < 1 || a.S > BCMPC_MAX_STATE || a.A < 1 ||
        a.A > BCMPC_MAX_ACTION || a.n_terms < 0 || a.n_done < 0 || a.n_terms + a.n_done > BCMPC_MAX_COST_TERMS ||
        a.n_slots < 0 || a.n_slots > a.n_terms + a.n_done || a.n_state_slots < 0 || a.n_state_slots > a.n_slots ||
        !std::isfinite(a.done_cost))
        return hipErrorInvalidValue;
    for (int i = 0; i < a.n_slots; ++i)
        if ((a.slot_action[i] != 0) != (i >= a.n_state_slots) || a.slot_index[i] >= (a.slot_action[i] ? a.A : a.S))
            return hipErrorInvalidValue;
    for (int t = 0; t < a.n_terms + a.n_done; ++t)
        if ((int)(a.terms[t].meta >> 8) >= a.n_slots) return hipErrorInvalidValue;
    for (int t = a.n_terms; t < a.n_terms + a.n_done; ++t)      // a done condition reads a state slot
        if ((int)(a.terms[t].meta >> 8) >= a.n_state_slots) return hipErrorInvalidValue;
    if (a.n_slots <= 4) return launch_t<4, 8>(a, st);
    if (a.n_slots <= 8) return launch_t<8, 4>(a, st);
    if (a.n_slots <= 16) return launch_t<16, 2>(a, st);
    if (a.n_slots <= 24) return launch_t<24, 1>(a, st);
    return launch_t<32, 1>(a, st);
}

}  // namespace bcmpc

// term_cost_x.hip -- term_cost.hip's kernel for lists with reference channels or RATE terms (gfx950).
//
// The walk, the arithmetic and the termination are term_cost.hip's (read that file first); the NumPy definition
// is cost_functions.episode_cost with reference / previous_action.  A unit and an argument struct of its own
// (kernels.h TermCostXArgs), so that the instances of term_cost.hip keep their machine code and their
// kernel-argument layout: a list without a channel or a RATE term never comes here.
//
// What is new:
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
// * RATE needs a_{h-1}.  The ring is one row deeper than term_cost.hip's (PF + 2 rows): in the trip of steps
//   h0 .. h0 + PF - 1 it holds rows h0 - 1 .. h0 + PF, so step h0 finds the action of step h0 - 1 where the
//   previous trip left it -- loaded from the explicit array, or regenerated there with the functions the
//   rollout kernels call.  Row -1 is written before the first trip: the previous action of the lane's
//   environment, or, without one, a_0 itself (d is then a_0 - a_0, as the definition has it).

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

// a / b correctly rounded (term_cost.hip term_div)
__device__ __forceinline__ double term_div(double a, double b, double r, bool fast) {
    const double m = __builtin_fabs(a);
    if (fast && (m == 0.0 || (m > 0x1p-500 && m < 0x1p500))) return div_rn(a, b, r);
    return __ddiv_rn(a, b);
}

// row r of a slot: a channel's and an explicit action's rows end at H - 1, a state dim's at H (by value: the
// strides are uniform and stay in scalar registers)
__device__ __forceinline__ double load_slot(const double* p, uint32_t chan, uint32_t act, int r, int H, int64_t RS,
                                            int64_t KA, int64_t KS) {
    const int rs = r < H ? r : H, ra = r < H ? r : H - 1;
    const int64_t row = chan | act ? ra : rs;
    const int64_t stride = chan ? RS : act ? KA : KS;
    return p[row * stride];
}

template <int ND, int PF, bool REGEN, bool DONE>
__global__ __launch_bounds__(kTermLanes) void term_cost_x_kernel(const TermCostXArgs ax) {
    constexpr int R = PF + 2;                            // LDS ring: row r lives in rows[(r + 1) % R], r >= -1
    __shared__ double rows[R][ND][kTermLanes];
    const TermCostArgs& a = ax.b;
    const int lane = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * kTermLanes + lane;
    if (k >= a.K) return;                                // tail lanes (no barrier follows)
    const uint64_t g = (uint64_t)(a.cand_offset + k);
    const int64_t env = k / ax.env_paths;                // this lane's environment
    const int nd = a.n_slots, H = a.H;

    // The slots, a byte each: index | channel << 6 | action << 7.  A state dim walks the trajectory's rows
    // 0 .. H; a channel walks its environment's reference rows and an explicit action the action array's,
    // rows 0 .. H - 1.  A regenerated action's slot loads state dim 0, a value that is then overwritten.
    uint32_t sw[ND / 4];
#pragma unroll
    for (int j = 0; j < ND / 4; ++j) sw[j] = a.slot_word[j];
    const bool have_actions = a.actions != nullptr;
    const int64_t KS = a.K * a.S, KA = a.K * a.A, RS = ax.ref_row_stride;
    const double* sp[ND];
    uint32_t amask = 0, rmask = 0;                       // the explicit-action slots, the channel slots
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const uint32_t b = (sw[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const bool act = (b >> 7) != 0, chan = ((b >> 6) & 1u) != 0;
        if (act && have_actions) amask |= 1u << i;
        if (chan) rmask |= 1u << i;
        sp[i] = chan ? ax.ref + env * ax.ref_env_stride + (b & 31u)
              : act  ? (have_actions ? a.actions + k * a.A + (b & 31u) : a.traj + k * a.S)
                     : a.traj + k * a.S + (b & 31u);
    }
    // (one load instruction per slot and row, no branch around it; rows past the last repeat it, slots past
    //  n_slots read state dim 0: in bounds, never used)
    auto load = [&](int i, int r) -> double {
        return load_slot(sp[i], (rmask >> i) & 1u, (amask >> i) & 1u, r, H, RS, KA, KS);
    };

    // row 0 into LDS; rows 1 .. PF into the registers
#pragma unroll
    for (int i = 0; i < ND; ++i) rows[1][i][lane] = load(i, 0);
    double pf[PF][ND];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int i = 0; i < ND; ++i) pf[u][i] = load(i, u + 1);

    // row -1, the action slots of a list with RATE terms: the environment's previous action, else a_0
    if (ax.has_rate) {
#pragma unroll 1
        for (int i = a.n_state_slots + ax.n_ref_slots; i < nd; ++i) {
            const int j = (a.slot_word[i >> 2] >> (8 * (i & 3))) & 31u;
            rows[0][i][lane] = ax.prev      ? ax.prev[env * ax.prev_env_stride + j]
                               : have_actions ? rows[1][i][lane]
                                              : term_regen(a, 0, j, g);
        }
    }

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
        const int b0 = h0 % R;                           // ring position of row h0 - 1
        auto pos = [&](int v) { return b0 + v < R ? b0 + v : b0 + v - R; };   // ... of row h0 - 1 + v
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int i = 0; i < ND; ++i) rows[pos(u + 2)][i][lane] = pf[u][i];
#pragma unroll
        for (int u = 0; u < PF; ++u)
#pragma unroll
            for (int i = 0; i < ND; ++i) pf[u][i] = load(i, h0 + PF + u + 1);

        if (REGEN && !have_actions) {                    // the action slots (the last ones) of the trip's steps
#pragma unroll 1
            for (int u = 0; u < PF; ++u) {
                if (h0 + u >= H) break;
#pragma unroll 1
                for (int i = a.n_state_slots + ax.n_ref_slots; i < nd; ++i)
                    rows[pos(u + 1)][i][lane] =
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
            const bool chan = (T.meta >> 6) & 1u;        // p is the channel slot T.pad of row h
            const int psl = (int)T.pad;
            const double w = T.weight, p = T.param;
            if (DONE && t >= nc) {
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const double x = rows[pos(u + 2)][sl][lane];
                    const bool hit = cmp == BCMPC_CMP_GE ? x >= p : cmp == BCMPC_CMP_GT ? x > p
                                   : cmp == BCMPC_CMP_LE ? x <= p : x < p;
                    flags |= (hit ? 1u : 0u) << u;
                }
            } else if ((T.meta >> 7) & 1u) {             // RATE
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const double d = __dsub_rn(rows[pos(u + 1)][sl][lane], rows[pos(u)][sl][lane]);
                    acc[u] = __dadd_rn(acc[u], __dmul_rn(w, __dmul_rn(d, d)));
                }
            } else if (kind == BCMPC_TERM_DIFF) {
                const bool fast = (T.meta >> 5) & 1u;
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const double d = __dsub_rn(rows[pos(u + 2)][sl][lane], rows[pos(u + 1)][sl][lane]);
                    acc[u] = __dadd_rn(acc[u], __dmul_rn(w, term_div(d, p, T.rparam, fast)));
                }
            } else if (kind == BCMPC_TERM_THRESHOLD) {
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const double x = rows[nx ? pos(u + 2) : pos(u + 1)][sl][lane];
                    const double q = chan ? rows[pos(u + 1)][psl][lane] : p;
                    const bool hit = cmp == BCMPC_CMP_GE ? x >= q : cmp == BCMPC_CMP_GT ? x > q
                                   : cmp == BCMPC_CMP_LE ? x <= q : x < q;
                    acc[u] = hit ? __dadd_rn(acc[u], w) : acc[u];
                }
            } else if (kind == BCMPC_TERM_LINEAR) {
#pragma unroll
                for (int u = 0; u < PF; ++u)
                    acc[u] = __dadd_rn(acc[u], __dmul_rn(w, rows[nx ? pos(u + 2) : pos(u + 1)][sl][lane]));
            } else {
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const double q = chan ? rows[pos(u + 1)][psl][lane] : p;
                    const double d = __dsub_rn(rows[nx ? pos(u + 2) : pos(u + 1)][sl][lane], q);
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
hipError_t launch_t(TermCostXArgs ax, hipStream_t st) {
    TermCostArgs& a = ax.b;
    for (int j = 0; j < BCMPC_MAX_COST_TERMS / 4; ++j) a.slot_word[j] = 0;
    for (int i = 0; i < a.n_slots; ++i)          // the slots as the kernel reads them, a byte each
        a.slot_word[i >> 2] |= (uint32_t)(a.slot_index[i] | (a.slot_action[i] == 1 ? 0x80 : 0) |
                                          (a.slot_action[i] == 2 ? 0x40 : 0)) << (8 * (i & 3));
    const bool regen = !a.actions && a.n_state_slots + ax.n_ref_slots < a.n_slots;
    const int64_t blocks = (a.K + kTermLanes - 1) / kTermLanes;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(kTermLanes);
    if (a.n_done > 0) {
        if (regen) hipLaunchKernelGGL((term_cost_x_kernel<ND, PF, true, true>), grid, block, 0, st, ax);
        else hipLaunchKernelGGL((term_cost_x_kernel<ND, PF, false, true>), grid, block, 0, st, ax);
    } else if (regen) {
        hipLaunchKernelGGL((term_cost_x_kernel<ND, PF, true, false>), grid, block, 0, st, ax);
    } else {
        hipLaunchKernelGGL((term_cost_x_kernel<ND, PF, false, false>), grid, block, 0, st, ax);
    }
    return hipGetLastError();
}

}  // namespace

// the instance rule of launch_term_cost, on the slots with the channels counted in
hipError_t launch_term_cost_x(const TermCostXArgs& ax, hipStream_t st) {
    const TermCostArgs& a = ax.b;
    if (!a.traj || !a.costs || a.K < 1 || a.H < 1 || a.S < 1 || a.S > BCMPC_MAX_STATE || a.A < 1 ||
        a.A > BCMPC_MAX_ACTION || a.n_terms < 0 || a.n_done < 0 || a.n_terms + a.n_done > BCMPC_MAX_COST_TERMS ||
        a.n_slots < 0 || a.n_slots > BCMPC_MAX_COST_TERMS || a.n_state_slots < 0 || ax.n_ref_slots < 0 ||
        a.n_state_slots + ax.n_ref_slots > a.n_slots || !std::isfinite(a.done_cost))
        return hipErrorInvalidValue;
    if (ax.env_paths < 1 || a.K % ax.env_paths != 0 || ax.n_ref < 0 || ax.n_ref > BCMPC_MAX_REF_CHANNELS ||
        (ax.n_ref_slots > 0 && !ax.ref) || ax.ref_env_stride < 0 || ax.ref_row_stride < 0 || ax.prev_env_stride < 0)
        return hipErrorInvalidValue;
    const int act0 = a.n_state_slots + ax.n_ref_slots;
    for (int i = 0; i < a.n_slots; ++i) {
        const int want = i < a.n_state_slots ? 0 : i < act0 ? 2 : 1;
        const int lim = want == 0 ? a.S : want == 2 ? ax.n_ref : a.A;
        if (a.slot_action[i] != want || a.slot_index[i] >= lim) return hipErrorInvalidValue;
    }
    for (int t = 0; t < a.n_terms + a.n_done; ++t) {
        const TermDev& T = a.terms[t];
        const int sl = (int)(T.meta >> 8);
        if (sl >= a.n_slots || (sl >= a.n_state_slots && sl < act0)) return hipErrorInvalidValue;
        if (((T.meta >> 6) & 1u) && ((int)T.pad < a.n_state_slots || (int)T.pad >= act0)) return hipErrorInvalidValue;
        if (((T.meta >> 7) & 1u) && sl < act0) return hipErrorInvalidValue;             // RATE reads an action
        if (t >= a.n_terms && sl >= a.n_state_slots) return hipErrorInvalidValue;       // a done condition: a state
    }
    if (a.n_slots <= 4) return launch_t<4, 8>(ax, st);
    if (a.n_slots <= 8) return launch_t<8, 4>(ax, st);
    if (a.n_slots <= 16) return launch_t<16, 2>(ax, st);
    if (a.n_slots <= 24) return launch_t<24, 1>(ax, st);
    return launch_t<32, 1>(ax, st);
}

}  // namespace bcmpc

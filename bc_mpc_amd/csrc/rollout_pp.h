// rollout_pp.h -- the two pipelined rollout kernels: rollout_pp (single-pass f16) and rollout_pp3 (split
// precision), each two 64-candidate groups per workgroup, one segment out of phase.  They build on
// rollout_x3.h's primitives (mfma16, sidx, epi_pair, the X3_STAMP instrument); the launchers and shape
// queries are in rollout_pp.hip.
#pragma once
#include <type_traits>

#include "rollout_x3.h"

namespace bcmpc {

// ------------------------------------------------------------ rollout_pp ----
// Single-pass f16 (BCMPC_PREC_F16) as a two-group software pipeline (round 4; the plain 2-layer tanh
// delta net at hidden 512).  rollout_x3's step is a lock-step chain: every wave of the workgroup runs the
// same phase at once (f64 state update, layer 0 and its tanh, the hidden layer's MFMAs, its tanh and the
// output layer), so the SIMDs' matrix pipes idle through the VALU phases and the VALU through the MFMA
// phase (PMC + stamps + ablations: profiles/r04_pmc_f16/).  Here a 512-thread workgroup holds TWO
// independent 64-candidate groups, waves 0-3 and 4-7 (waves w and w + 4 share a SIMD), each with its own
// hi-only slab.  A group's control step is three segments:
//   C  (wave wl owns column wl of its group, all 32 state dims): the output partials of the previous step
//      summed in fixed order, f64 de-normalise + residual + cheetah cost, f64 normalise of the next input
//      (column power-of-two scale), layer 0 for its OWN column from registers (all 32 tiles: the B fragment
//      is the lane's own 8 inputs, no slab, no barrier), its tanh, its column of the hidden-layer slab;
//   M  the hidden layer's MFMAs (wave wl: tiles [8wl, 8wl + 8) of all 4 columns, slab B fragments);
//   E  its tanh, the K-split output layer (the wave's own 4 k-steps from registers), the partials into
//      the slab, the next action inputs staged.
// Every segment ends at the workgroup barrier, and group 1 runs one segment ahead of group 0, so each
// barrier interval pairs C with E (VALU beside VALU: the two waves of a SIMD interleave their VALU), M with
// C and E with M (the matrix pipe of one wave beside the other's VALU).  C touches only its own column of
// the slab (partials and layer input alike: fragment index = c mod NC), so it needs no barrier of its own;
// M reads what every C of its group wrote (one interval earlier); E overwrites the slab only after every M
// of its group has read it (one interval earlier).  Arithmetic as rollout_x3<..., F1 = true>: the same
// f16 operands and power-of-two scales, f32 accumulate, f64 state / cost.
#ifndef PP_NCH
#define PP_NCH 4                 // steps of action inputs staged per fill
#endif
__host__ __device__ constexpr int pp_xa_bytes(int A) { return (PP_NCH * 64 * A * 4 + 15) & ~15; }
__host__ __device__ constexpr int pp_group_bytes(int HP, int A) { return pp_xa_bytes(A) + (HP / 32) * 4 * 1024; }
__host__ __device__ constexpr int pp_lds_bytes(int HP, int A) { return param_bytes(2, HP) + 2 * pp_group_bytes(HP, A); }
// (+ the groups' counters [2][2] ints | layer-0 slabs [2][NC] fragments | column factors [2][64])
__host__ __device__ constexpr int pp_lds_total(int HP, int A) { return pp_lds_bytes(HP, A) + 16 + 2 * 4 * 1024 + 2 * 64 * 4; }

// The hidden layer of one group (single pass, hi operands): acc[j][c] += W[tile j] x X[c] over the P
// k-steps, fully unrolled (no loop-carried operand sets: fixed accumulator registers).  Weights in units of
// PG tiles through PD + 1 register sets, PD units in flight ahead of the MFMAs (the wave is alone on its
// SIMD's matrix pipe in this segment: nothing else hides its L2 latency); s0 holds units 0..PD-1.
// (round 5, folded operands: PP_G 1 x PP_D 4 -- the same 4 KiB in flight per wave, one tile per unit --
//  measured 0.78 vs 0.785 ms, G2 x D2 / G1 x D6 / + a one-k-step B prefetch within +-0.5%: the segment is not
//  bound by its weight loads' latency; profiles/r05_pp_prefetch_ab.txt, profiles/r05_pp_prio_ab.txt)
#ifndef PP_G
#define PP_G 1
#endif
#ifndef PP_D
#define PP_D 4
#endif
// wave priority per segment (s_setprio).  Without it the arbiter's age order favours group 0 in both of its
// segments (stamps: group 1's C segment 20k ticks, group 0's 13.7k; profiles/r04_pp_stamps.log).  C ahead
// of ME evens the groups out (profiles/r04_ppprio_stamps.log) but the interval stays bound by ME; ME ahead
// measured best by 1-2% (profiles/r04_ppprio_ab.jsonl: 0.860-0.867 vs 0.876-0.887 ms C-first, 0.867-0.873 none);
// round 5 with the folded operands (C and ME now ~18k ticks each): ME-first 0.785 ms, equal 0.811, C-first 0.835
// (profiles/r05_pp_prio_ab.txt)
#ifndef PP_PRIO_C
#define PP_PRIO_C 0
#endif
#ifndef PP_PRIO_ME
#define PP_PRIO_ME 2
#endif
// byte offset of operand j of mm_pp's first units (unit j / PP_G: k-step u / NG, tile group u % NG of the half
// [T0, T0 + TWH); the order mm_pp loads them in)
__device__ __forceinline__ constexpr int pp_unit_off(int j, int T0, int TW, int TWH) {
    return ((j / PP_G) / (TWH / PP_G)) * TW * 2048 + (T0 + ((j / PP_G) % (TWH / PP_G)) * PP_G + j % PP_G) * 2048;
}
template <int TW, int NC, int P, int PG, int PD, int TWH = TW, int T0 = 0, bool BIAS = false>
__device__ __forceinline__ void mm_pp(__amdgpu_buffer_rsrc_t rs, int wbase, const f4* slab, f4 (&acc)[TWH][NC],
                                      int lane, const h8 (&s0)[PD * PG], const f4* bias = nullptr) {
    // (BIAS: the first k-step's MFMAs take bias[tile] as their C operand -- the accumulators start from the
    //  bias, no separate initialisation)
    // (TWH < TW: tiles [T0, T0 + TWH) of the wave's TW only)
    constexpr int NG = TWH / PG, NU = P * NG, NS = PD + 1;
    const int voff = lane * 16;
    h8 sr[NS][PG], bh[NC];
#pragma unroll
    for (int d = 0; d < PD; ++d)
#pragma unroll
        for (int j = 0; j < PG; ++j) sr[d][j] = s0[d * PG + j];
    // (each k-step's B fragments are read at its first unit; reading them one k-step ahead into a second
    //  register set measured within +-0.5%, profiles/r05_pp_prefetch_ab.txt)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        if (u + PD < NU) {
            const int un = u + PD;
#pragma unroll
            for (int j = 0; j < PG; ++j)
                sr[un % NS][j] = fload(rs, voff, wbase + (un / NG) * TW * 2048 + (T0 + (un % NG) * PG + j) * 2048);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (u % NG == 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) bh[c] = sread(slab + sidx<NC, true>(u / NG, c, 0, lane));
        }
        const int g = u % NG;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int j = 0; j < PG; ++j)
                acc[g * PG + j][c] = mfma16(sr[u % NS][j], bh[c],
                                            BIAS && u < NG ? bias[g * PG + j] : acc[g * PG + j][c]);
    }
}

// FOLD (the default, BCMPC_PP_FOLD=0 turns it off): the host packs both hidden-producing layers as
// f16(W x 2 log2 e) with no power-of-two scales, the MFMAs start from the bias x 2 log2 e, so the
// accumulators are z and the epilogue is epi_pair_fold (one VALU operation per element fewer); the
// layer-0 input goes to f16 unscaled (|x| clamped below f16's overflow, NaN kept), no per-column power of
// two; the hidden activations are tanh in [-1, 1] (the output layer's scale is 1 / its weight scale)
template <int HP, bool FOLD>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void rollout_pp(const RolloutArgs a) {
    constexpr int NC = 4;                         // 16-candidate columns per group
    constexpr int T = HP / 16, P = T / 2;         // hidden tiles, k-steps
    constexpr int TW = T / 4, PW = TW / 2;        // per wave (4 waves per group)
    constexpr int CB = 16 * NC;                   // candidates per group
    static_assert(T == 32 && TW == 8 && PW == 4, "hidden 512");
    static_assert(PP_D <= P * (TW / 2 / PP_G) && (TW / 2) % PP_G == 0, "prefetch within one tile half's units");
    extern __shared__ __attribute__((aligned(16))) f4 lds[];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = w >> 2, wl = w & 3;
    const int q = lane >> 4, m = lane & 15;
    const int64_t gc0 = (int64_t)blockIdx.x * (2 * CB) + grp * CB;     // the group's first candidate
    const int64_t cand = gc0 + 16 * wl + m;                           // this lane's candidate (column wl)
    const bool valid = cand < a.K;
    const int S = a.S, A = a.A;

    double* C = reinterpret_cast<double*>(lds);
    float* Bl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + kConstRows * kConstCols * 8);
    for (int i = threadIdx.x; i < kConstRows * kConstCols; i += blockDim.x) C[i] = a.consts[i];
    for (int l = 0; l < 2; ++l)
        for (int i = threadIdx.x; i < HP; i += blockDim.x) Bl[l * HP + i] = a.b[l][i] * kTanhK;
    float* const Bout = Bl + 2 * HP;
    for (int i = threadIdx.x; i < 32; i += blockDim.x) Bout[i] = a.b[2][i];
    char* const gbase = reinterpret_cast<char*>(lds) + param_bytes(2, HP) + grp * pp_group_bytes(HP, A);
    float* const xa = reinterpret_cast<float*>(gbase);                  // [PP_NCH][CB][A] normalised actions
    f4* const slab = reinterpret_cast<f4*>(gbase + pp_xa_bytes(A));     // [P][NC] hi fragments | partials

    // lane (q, m) holds dims 16k + 4q + r (k = 0, 1) of its candidate: the MFMA B-fragment order
    double s[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * k + 4 * q + r;
            s[k][r] = (valid && d < S) ? (a.state_inline ? a.state_v[d] : a.state[cand * a.state_stride + d]) : 0.0;
        }
    if (a.traj && valid) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * k + 4 * q + r;
                if (d < S) a.traj[cand * S + d] = s[k][r];
            }
    }
    double cost = 0.0;                                  // trajectory_cost = 0 (cost_functions.py:60)

    // the group's action inputs of PP_NCH steps from h0: f64 normalise (dynamics.py:110), f32 (the TF
    // feed); the group's 256 threads
    const int gt = threadIdx.x - 256 * grp;
    auto fill_actions = [&](int h0) __attribute__((always_inline)) {
        const int nhs = (a.H - h0 < PP_NCH) ? a.H - h0 : PP_NCH;
        if (!a.cem_mu && !a.actions) {
            const int AP = (A + 1) >> 1, per = CB * AP;
            for (int i = gt; i < nhs * per; i += 256) {
                const int hh = i / per, rem = i - hh * per, kl = rem / AP, p2 = rem - kl * AP;
                const int j0 = 2 * p2, j1 = min(2 * p2 + 1, A - 1);
                float x0 = 0.f, x1 = 0.f;
                if (gc0 + kl < a.K) {
                    double v0, v1;
                    rng_action_pair(a.seed, (uint64_t)(a.cand_offset + gc0 + kl), h0 + hh, p2, C[6 * 32 + j0],
                                    C[7 * 32 + j0], C[6 * 32 + j1], C[7 * 32 + j1], v0, v1);
                    x0 = (float)div_rn(__dsub_rn(v0, C[2 * 32 + j0]), C[3 * 32 + j0], C[9 * 32 + j0]);
                    x1 = (float)div_rn(__dsub_rn(v1, C[2 * 32 + j1]), C[3 * 32 + j1], C[9 * 32 + j1]);
                }
                float* const dst = xa + (hh * CB + kl) * A;
                dst[j0] = x0;
                if (2 * p2 + 1 < A) dst[j1] = x1;
            }
            return;
        }
        const int per = CB * A;
        for (int i = gt; i < nhs * per; i += 256) {
            const int hh = i / per, rem = i - hh * per, kl = rem / A, j = rem - kl * A;
            float xv = 0.f;
            if (gc0 + kl < a.K) {
                const int64_t c = gc0 + kl;
                const uint64_t gg = (uint64_t)(a.cand_offset + c);
                const double v = a.cem_mu ? cem_action(a.seed, gg, h0 + hh, j, a.cem_iter, a.cem_mu[(h0 + hh) * A + j],
                                                       a.cem_sigma[(h0 + hh) * A + j], C[6 * 32 + j], C[7 * 32 + j])
                                          : a.actions[((int64_t)(h0 + hh) * a.K + c) * A + j];
                xv = (float)div_rn(__dsub_rn(v, C[2 * 32 + j]), C[3 * 32 + j], C[9 * 32 + j]);
            }
            xa[(hh * CB + kl) * A + j] = xv;
        }
    };
    fill_actions(0);
    __syncthreads();

    const int voff = lane * 16;
    const __amdgpu_buffer_rsrc_t rs0 = layer_rsrc(a.w[0], a.wbytes[0]);
    const __amdgpu_buffer_rsrc_t rs1 = layer_rsrc(a.w[1], a.wbytes[1]);
    const __amdgpu_buffer_rsrc_t rso = layer_rsrc(a.w[2], a.wbytes[2]);
    const float f1 = a.winv[1] * kTanhK, fo = a.winv[2];
    const int wbase1 = wl * P * TW * 2048;              // this wave's hidden-layer weight slice
    f4* const slab0 = reinterpret_cast<f4*>(reinterpret_cast<char*>(lds) + pp_lds_bytes(HP, A) + 16) + grp * NC * 64;
    float* const colf = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + pp_lds_bytes(HP, A) + 16 +
                                                 2 * NC * 1024) + grp * CB;
    // per-group LDS counters (monotone over the steps): C's layer-0 inputs published, M's slab reads done
    int* const cnt = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + pp_lds_bytes(HP, A)) + 2 * grp;
    if (threadIdx.x < 4) reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + pp_lds_bytes(HP, A))[threadIdx.x] = 0;
    __syncthreads();

    f4 acc[TW][NC];
    h8 uh[PP_D * PP_G];                                 // ME's first PP_D operand units (issued in C)
    // (X3_STAMP variant builds: s_memtime per phase; slots 0 C/owner, 1 C/wait for the group's inputs,
    //  2 C/layer 0 + tanh, 3 ME/MFMAs, 4 ME/tanh + output, 5 ME/group wait, 6 ME/partials + fill,
    //  7 barrier, 8 idle segments)
    uint64_t ph_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t tp_ = X3_STAMP ? __builtin_amdgcn_s_memtime() : 0;
    const int nseg = 2 * a.H + 1;                       // C(0) ME(0) ... ME(H-1) C(H) (the last cost)
    for (int k = 0; k < nseg + 1; ++k) {
        // (an opaque zero added to every weight offset and LDS table base: the weights and tables are the
        //  same every step, and without it the compiler hoists the loop-invariant loads out of the loop)
        int wz = 0;
        asm volatile("" : "+s"(wz));
        const double* const Cz = C + wz;
        const float* const Blz = Bl + wz;
        const float* const Boutz = Bout + wz;
        const int seg = k - (grp == 0 ? 1 : 0);         // group 1 runs one segment ahead
        if (seg >= 0 && seg < nseg) {
            const int h = seg >> 1;
            if ((seg & 1) == 0) {
                // ---------------- C(h) ----------------
                __builtin_amdgcn_s_setprio(PP_PRIO_C);
                // this wave's layer-0 fragments, in flight through the owner phase
                h8 a0[TW];
#pragma unroll
                for (int j = 0; j < TW; ++j) a0[j] = fload(rs0, voff, wz + (wl * TW + j) * 2048);
                if (h > 0) {
                    f4 o[2];
#pragma unroll
                    for (int v = 0; v < 2; ++v) o[v] = slab[((0 * 2 + v) * NC + wl) * 64 + lane];
#pragma unroll
                    for (int g2 = 1; g2 < 4; ++g2)                 // fixed summation order
#pragma unroll
                        for (int v = 0; v < 2; ++v) o[v] += slab[((g2 * 2 + v) * NC + wl) * 64 + lane];
                    // cheetah penalties on the current state (cost_functions.py:16-26): dims 5..7 in row q = 1
                    const int npen = partner_row16((s[0][1] >= 0.2) + (s[0][2] >= 0.0) + (s[0][3] >= 0.0));
                    const double s17 = s[1][1];
                    // de-normalise + residual (dynamics.py:113,116), f64, no FMA
#pragma unroll
                    for (int v = 0; v < 2; ++v) {
                        const f4 bv = *reinterpret_cast<const f4*>(Boutz + 16 * v + 4 * q);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int d = 16 * v + 4 * q + r;
                            if (d < S) {
                                const float dn = fmaf(o[v][r], fo, bv[r]);
                                const double ud = __dadd_rn(__dmul_rn((double)dn, Cz[5 * 32 + d]), Cz[4 * 32 + d]);
                                s[v][r] = __dadd_rn(s[v][r], ud);
                            }
                        }
                    }
                    if (a.cost == BCMPC_COST_CHEETAH) {
                        const double score = __dsub_rn(10.0 * (double)npen,
                                                       div_rn(__dsub_rn(s[1][1], s17), 0.01, 1.0 / 0.01));
                        cost = __dadd_rn(cost, score);
                    }
                    if (a.traj && valid) {
#pragma unroll
                        for (int v = 0; v < 2; ++v)
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int d = 16 * v + 4 * q + r;
                                if (d < S) a.traj[((int64_t)h * a.K + cand) * S + d] = s[v][r];
                            }
                    }
                }
                if (h < a.H) {
                    // normalise the state (dynamics.py:109), f32 (TF feed), the staged actions; the column's
                    // power-of-two scale; its B fragment into the layer-0 slab
                    const float* xr = xa + ((h % PP_NCH) * CB + 16 * wl + m) * A;
                    float xin[8];
#pragma unroll
                    for (int v = 0; v < 2; ++v)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int d = 16 * v + 4 * q + r;
                            float xv = 0.f;
                            if (d < S) xv = (float)div_rn(__dsub_rn(s[v][r], Cz[0 * 32 + d]), Cz[1 * 32 + d], Cz[8 * 32 + d]);
                            else if (d < S + A) xv = xr[d - S];
                            xin[4 * v + r] = xv;
                        }
                    h8 bown;                                   // (the k order of pack_x3_layer)
                    if constexpr (FOLD) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) {          // |x| below f16's overflow, NaN kept
                            const float xc = fminf(fmaxf(xin[i], -65504.0f), 65504.0f);
                            bown[i] = (_Float16)(xin[i] == xin[i] ? xc : xin[i]);
                        }
                    } else {
                        float mx = 0.f;
#pragma unroll
                        for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(xin[i]));
                        mx = max_rows32(max_rows16(mx));
                        int e = 0;
                        (void)frexpf(mx, &e);                  // column scale: max |x| -> [2^11, 2^12)
                        int sh = 12 - e;
                        sh = mx > 0.f ? (sh < -100 ? -100 : (sh > 100 ? 100 : sh)) : 0;
                        const float sc = ldexpf(1.0f, sh);
#pragma unroll
                        for (int i = 0; i < 8; ++i) bown[i] = (_Float16)(xin[i] * sc);
                        if (q == 0) colf[16 * wl + m] = ldexpf(a.winv[0], -sh) * kTanhK;
                    }
                    swrite(slab0 + wl * 64 + lane, bown);
                }
                // publish: a workgroup-scope release of this wave's LDS writes (slab0 / colf, and its reads of
                // the partials), then the count; LDS only ("local"), so the weight loads stay in flight
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                if (lane == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                X3_ST(0);
                if (h < a.H) {
                    // the group's four layer-0 inputs published (and every partial of the slab read)
                    while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 4 * (h + 1))
                        __builtin_amdgcn_s_sleep(1);
                    // (acquire: the slab0 / colf reads below cannot move above the wait)
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                    X3_ST(1);
                    // layer 0 [S+A -> h]: this wave's 8 tiles x the group's 4 columns
                    h8 b0[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) b0[c] = sread(slab0 + c * 64 + lane);
                    f4 z4[TW];
#pragma unroll
                    for (int j = 0; j < TW; ++j)
                        z4[j] = FOLD ? *reinterpret_cast<const f4*>(Blz + 16 * (wl * TW + j) + 4 * q)
                                     : (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < NC; ++c)
#pragma unroll
                        for (int j = 0; j < TW; ++j) acc[j][c] = mfma16(a0[j], b0[c], z4[j]);
                    // ME's first operand units, in flight through the tanh below and the barrier
#pragma unroll
                    for (int j = 0; j < PP_D * PP_G; ++j)          // (units 0..PP_D-1 of tile half 0)
                        uh[j] = fload(rs1, voff, wz + wbase1 + pp_unit_off(j, 0, TW, TW / 2));
                    // tanh, this wave's 4 k-steps of the hidden-layer slab (all 4 columns)
#pragma unroll
                    for (int pp = 0; pp < PW; ++pp)
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            h8 xh, xl;
                            if constexpr (FOLD)
                                xh = epi_pair_fold(acc[2 * pp][c], acc[2 * pp + 1][c]);
                            else
                                epi_pair(acc[2 * pp][c], acc[2 * pp + 1][c], colf[16 * c + m], Blz, wl * TW + 2 * pp,
                                         q, xh, xl);
                            swrite(slab + ((wl * PW + pp) * NC + c) * 64 + lane, xh);
                        }
                }
                X3_ST(2);
            } else {
                // ---------------- ME(h): the hidden layer's MFMAs, its tanh, the output layer ----------------
                __builtin_amdgcn_s_setprio(PP_PRIO_ME);
                f4 po[2][NC];
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int c = 0; c < NC; ++c) po[v][c] = (f4){0.f, 0.f, 0.f, 0.f};
                // in two halves of the wave's 8 tiles (64 accumulator registers instead of 128; each slab k-step
                // read twice): half 0's tanh and output MFMAs run after its MFMAs while half 1's first weight
                // units are in flight
                auto half = [&](auto HFc) __attribute__((always_inline)) {
                    constexpr int hf = decltype(HFc)::value;
                    constexpr int TWH = TW / 2;
                    f4 ah[TWH][NC];
                    if constexpr (FOLD) {
                        f4 bias1[TWH];                          // (the accumulators start from the bias)
#pragma unroll
                        for (int j = 0; j < TWH; ++j)
                            bias1[j] = *reinterpret_cast<const f4*>(Blz + HP + 16 * (wl * TW + hf * TWH + j) + 4 * q);
                        mm_pp<TW, NC, P, PP_G, PP_D, TWH, hf * TWH, true>(rs1, wz + wbase1, slab, ah, lane, uh, bias1);
                    } else {
#pragma unroll
                        for (int j = 0; j < TWH; ++j)
#pragma unroll
                            for (int c = 0; c < NC; ++c) ah[j][c] = (f4){0.f, 0.f, 0.f, 0.f};
                        mm_pp<TW, NC, P, PP_G, PP_D, TWH, hf * TWH>(rs1, wz + wbase1, slab, ah, lane, uh);
                    }
                    if constexpr (hf == 0) {
#pragma unroll
                        for (int j = 0; j < PP_D * PP_G; ++j)      // half 1's first units
                            uh[j] = fload(rs1, voff, wz + wbase1 + pp_unit_off(j, TWH, TW, TWH));
                    } else {
                        // this wave's slab reads have returned: count it (the group's partials overwrite the
                        // slab only once all 4 waves have, below)
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                        if (lane == 0) __hip_atomic_fetch_add(cnt + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
#pragma unroll
                    for (int pp2 = 0; pp2 < PW / 2; ++pp2) {
                        const int pp = hf * (PW / 2) + pp2;            // this wave's k-step of the output layer
                        h8 oh[2];
#pragma unroll
                        for (int v = 0; v < 2; ++v)
                            oh[v] = fload(rso, voff, wz + (((wl * PW + pp) * 2 + v) * 2) * 1024);
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            h8 xh, xl;
                            if constexpr (FOLD)
                                xh = epi_pair_fold(ah[2 * pp2][c], ah[2 * pp2 + 1][c]);
                            else
                                epi_pair(ah[2 * pp2][c], ah[2 * pp2 + 1][c], f1, Blz + HP, wl * TW + 2 * pp, q, xh, xl);
#pragma unroll
                            for (int v = 0; v < 2; ++v) po[v][c] = mfma16(oh[v], xh, po[v][c]);
                        }
                    }
                };
                half(std::integral_constant<int, 0>{});
                half(std::integral_constant<int, 1>{});
                X3_ST(3);
                X3_ST(4);
                // every wave of the group has finished reading the slab (by now the others are normally long
                // past their MFMAs)
                while (__hip_atomic_load(cnt + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 4 * (h + 1))
                    __builtin_amdgcn_s_sleep(1);
                // (acquire: the partial writes below cannot move above the wait)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                X3_ST(5);
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int c = 0; c < NC; ++c) slab[((wl * 2 + v) * NC + c) * 64 + lane] = po[v][c];
                if ((h + 1) % PP_NCH == 0 && h + 1 < a.H) fill_actions(h + 1);
                X3_ST(6);
            }
        } else {
            X3_ST(8);
        }
        __syncthreads();
        X3_ST(7);
    }
    if constexpr (X3_STAMP) {
        if (a.stamps && lane == 0)
            for (int k2 = 0; k2 < 10; ++k2) a.stamps[((size_t)blockIdx.x * 8 + w) * 10 + k2] = ph_[k2];
    }

    const bool holder = valid && q == 0;                // cost in row 0 (dims 1, 17 and the penalty count)
    if (a.costs && holder) a.costs[cand] = cost;
    if (a.fused_argmin) {
        // np.argmin fused (as rollout_x3): this workgroup's best, the last workgroup reduces the records
        const ArgminArgs& am = a.amin;
        Best best{__builtin_inf(), INT64_MAX};
        if (holder) best = Best{am.maximize ? -cost : cost, cand};
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const Best o{__shfl_xor(best.c, off), __shfl_xor(best.i, off)};
            if (better(o, best)) best = o;
        }
        double* rc = reinterpret_cast<double*>(reinterpret_cast<char*>(lds) + param_bytes(2, HP) + pp_xa_bytes(A));
        int64_t* ri = reinterpret_cast<int64_t*>(rc + 16);
        if (lane == 0) { rc[w] = best.c; ri[w] = best.i; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < 8; ++k) {
                const Best o{rc[k], ri[k]};
                if (better(o, best)) best = o;
            }
            __hip_atomic_store(&am.scratch_c[blockIdx.x], best.c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&am.scratch_i[blockIdx.x], best.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned tk = __hip_atomic_fetch_add(a.amin_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool last = tk == gridDim.x - 1;
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            ri[16] = last ? 1 : 0;
        }
        __syncthreads();
        if (ri[16] == 0) return;
        best = Best{__builtin_inf(), INT64_MAX};
        for (unsigned b = threadIdx.x; b < gridDim.x; b += blockDim.x) {
            const Best o{am.scratch_c[b], am.scratch_i[b]};
            if (better(o, best)) best = o;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const Best o{__shfl_xor(best.c, off), __shfl_xor(best.i, off)};
            if (better(o, best)) best = o;
        }
        __syncthreads();
        if (lane == 0) { rc[w] = best.c; ri[w] = best.i; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < 8; ++k) {
                const Best o{rc[k], ri[k]};
                if (better(o, best)) best = o;
            }
            argmin_write(am, best);
            *a.amin_ticket = 0;
        }
    }
}

// ----------------------------------------------------------- rollout_pp3 ----
// Split precision (hi + lo operands, three MFMA passes) as rollout_pp's two-group pipeline over ONE
// time-shared slab.  A 512-thread workgroup holds two 64-candidate groups, waves 0-3 and
// 4-7 (waves w and w + 4 share a SIMD); within a group wave wl owns candidate column wl (all 32 state
// dims) and hidden tiles [8wl, 8wl + 8) of all four columns.  A group's control step is two segments:
//   M   its own column of the hidden-layer input (packed hi | lo pairs, in registers since the previous
//       interval) into the slab, the group's "inputs published" counter, the hidden layer (16 k-steps x
//       8 tiles x 4 columns x 3 passes); the accumulators stay in registers across the barrier;
//   EC  tanh + split of those accumulators, the K-split output layer from registers, the partials into
//       their own region, the group's "partials published" counter, the four partials summed in fixed
//       wave order, f64 de-normalise + residual + cost, the next input (column power-of-two scale,
//       split), layer 0 for the wave's OWN column from registers (all 32 tiles, no slab), its tanh and
//       split -- which stay in the registers the accumulators occupied.
// Every segment ends at the workgroup barrier and group 1 runs one segment ahead, so every interval
// pairs one group's M (the matrix pipe) with the other's EC (the VALU).  At the barrier the M group has
// finished reading the slab and the EC group everything, so the one slab and the one partials region are
// never live for both groups.  The 128 registers R carry the hidden accumulators out of M and the packed
// layer-0 output out of EC.  Weights in rollout_x3's NW = 8 packing (4 tiles per block: wave wl reads the
// blocks 2wl and 2wl + 1), so an engine can launch either kernel on the same buffers.  Arithmetic as
// rollout_x3; the output partials are four sums of four k-steps (there: eight of two).
// wave priority per segment (s_setprio).  The interval is bound by EC, one in-order wave's VALU chain beside its
// SIMD partner's MFMAs (stamps: EC 40.1k ticks, M 32.0k + 8.4k at the barrier, profiles/pp3_stamps.txt), so EC goes
// first: cfg3 1.736 / 1.741 ms per step against 1.759 / 1.763 with equal priorities and 1.789 / 1.789 with M first
// (M at 2: 1.790 / 1.791; profiles/pp3_prio_ab.txt)
#ifndef PP3_PRIO_M
#define PP3_PRIO_M 0
#endif
#ifndef PP3_PRIO_EC
#define PP3_PRIO_EC 1
#endif
// a scheduling barrier that only vector-memory instructions cannot cross: the weight loads of the unrolled
// EC phases stay in their slots (without it the scheduler issues every fragment load of a phase up front and
// spills), the MFMAs and the VALU around them still interleave
#define PP3_PIN_LOADS() __builtin_amdgcn_sched_barrier(0x78F)
// LDS: consts | biases | slab [P][4 columns][hi|lo] | tile-0 partials [4 waves][4 columns][64 lanes] |
// tile-1 partials, the lane rows that hold a state dim only [4][4][16 x rows] | action inputs of one step
// [2 groups][64][A] | counters [2 groups][2]
__host__ __device__ constexpr int pp3_xa_bytes(int A) { return (64 * A * 4 + 15) & ~15; }
__host__ __device__ constexpr int pp3_tile1_rows(int S) { return S > 16 ? (S - 16 + 3) / 4 : 0; }
__host__ __device__ constexpr int pp3_part_bytes(int S) { return 16 * (1024 + 256 * pp3_tile1_rows(S)); }
__host__ __device__ constexpr int pp3_lds_total(int HP, int S, int A) {
    return param_bytes(2, HP) + (HP / 32) * 4 * 2048 + pp3_part_bytes(S) + 2 * pp3_xa_bytes(A) + 16;
}

template <int HP>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
void rollout_pp3(const RolloutArgs a) {
    constexpr int NC = 4;                         // 16-candidate columns per group
    constexpr int T = HP / 16, P = T / 2;         // hidden tiles, k-steps
    constexpr int TW = T / 4, PW = TW / 2;        // per wave (4 waves per group)
    constexpr int CB = 16 * NC;                   // candidates per group
    static_assert(T == 32 && TW == 8 && PW == 4, "hidden 512");
    extern __shared__ __attribute__((aligned(16))) f4 lds[];

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = w >> 2, wl = w & 3;
    // (q, m: re-derived from an opaque copy of the lane index after every M segment, so that nothing derived
    //  from them stays in registers across the hidden layer, where the accumulators and operand sets fill the file)
    int ln = lane, q = lane >> 4, m = lane & 15;
    const int64_t gc0 = (int64_t)blockIdx.x * (2 * CB) + grp * CB;     // the group's first candidate
    const int64_t cand = gc0 + 16 * wl + m;                           // this lane's candidate (column wl)
    const bool valid = cand < a.K;
    const int S = a.S, A = a.A;
    const int nq1 = pp3_tile1_rows(S);            // lane rows of output tile 1 that hold a state dim

    double* C = reinterpret_cast<double*>(lds);
    float* Bl = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + kConstRows * kConstCols * 8);
    for (int i = threadIdx.x; i < kConstRows * kConstCols; i += blockDim.x) C[i] = a.consts[i];
    for (int l = 0; l < 2; ++l)
        for (int i = threadIdx.x; i < HP; i += blockDim.x) Bl[l * HP + i] = a.b[l][i] * kTanhK;
    float* const Bout = Bl + 2 * HP;
    for (int i = threadIdx.x; i < 32; i += blockDim.x) Bout[i] = a.b[2][i];
    f4* const slab = reinterpret_cast<f4*>(reinterpret_cast<char*>(lds) + param_bytes(2, HP));
    f4* const part0 = slab + P * NC * 2 * 64;
    f4* const part1 = part0 + 4 * NC * 64;
    float* const xa = reinterpret_cast<float*>(part1 + 4 * NC * 16 * nq1) + grp * (pp3_xa_bytes(A) / 4);
    int* const cnt0 = reinterpret_cast<int*>(reinterpret_cast<char*>(lds) + pp3_lds_total(HP, S, A) - 16);
    int* const cnt = cnt0 + 2 * grp;              // [0] M's inputs published, [1] EC's partials published
    if (threadIdx.x < 4) cnt0[threadIdx.x] = 0;

    // lane (q, m) holds dims 16k + 4q + r (k = 0, 1) of its candidate: the MFMA B-fragment order
    double s[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * k + 4 * q + r;
            s[k][r] = (valid && d < S) ? (a.state_inline ? a.state_v[d] : a.state[cand * a.state_stride + d]) : 0.0;
        }
    if (a.traj && valid) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * k + 4 * q + r;
                if (d < S) a.traj[cand * S + d] = s[k][r];
            }
    }
    double cost = 0.0;                                  // trajectory_cost = 0 (cost_functions.py:60)

    // the group's action inputs of step h: f64 normalise (dynamics.py:110), f32 (the TF feed); the group's
    // 256 threads
    const int gt = threadIdx.x - 256 * grp;
    auto fill_actions = [&](int h) __attribute__((always_inline)) {
        if (!a.cem_mu && !a.actions) {
            const int AP = (A + 1) >> 1;
            for (int i = gt; i < CB * AP; i += 256) {
                const int kl = i / AP, p2 = i - kl * AP;
                const int j0 = 2 * p2, j1 = min(2 * p2 + 1, A - 1);
                float x0 = 0.f, x1 = 0.f;
                if (gc0 + kl < a.K) {
                    double v0, v1;
                    rng_action_pair(a.seed, (uint64_t)(a.cand_offset + gc0 + kl), h, p2, C[6 * 32 + j0],
                                    C[7 * 32 + j0], C[6 * 32 + j1], C[7 * 32 + j1], v0, v1);
                    x0 = (float)div_rn(__dsub_rn(v0, C[2 * 32 + j0]), C[3 * 32 + j0], C[9 * 32 + j0]);
                    x1 = (float)div_rn(__dsub_rn(v1, C[2 * 32 + j1]), C[3 * 32 + j1], C[9 * 32 + j1]);
                }
                float* const dst = xa + kl * A;
                dst[j0] = x0;
                if (2 * p2 + 1 < A) dst[j1] = x1;
            }
            return;
        }
        for (int i = gt; i < CB * A; i += 256) {
            const int kl = i / A, j = i - kl * A;
            float xv = 0.f;
            if (gc0 + kl < a.K) {
                const int64_t c = gc0 + kl;
                const uint64_t gg = (uint64_t)(a.cand_offset + c);
                const double v = a.cem_mu ? cem_action(a.seed, gg, h, j, a.cem_iter, a.cem_mu[h * A + j],
                                                       a.cem_sigma[h * A + j], C[6 * 32 + j], C[7 * 32 + j])
                                          : a.actions[((int64_t)h * a.K + c) * A + j];
                xv = (float)div_rn(__dsub_rn(v, C[2 * 32 + j]), C[3 * 32 + j], C[9 * 32 + j]);
            }
            xa[kl * A + j] = xv;
        }
    };
    __syncthreads();

    const int voff = lane * 16;
    const __amdgpu_buffer_rsrc_t rs0 = layer_rsrc(a.w[0], a.wbytes[0]);
    const __amdgpu_buffer_rsrc_t rs1 = layer_rsrc(a.w[1], a.wbytes[1]);
    const __amdgpu_buffer_rsrc_t rso = layer_rsrc(a.w[2], a.wbytes[2]);
    const float f1 = a.winv[1] * kTanhK, fo = a.winv[2];

    // M: the hidden accumulators, tile j x column c at R[4j + c]; EC: the wave's own column of the hidden-layer
    // input, k-step p's packed hi at R[2p] and lo at R[2p + 1]
    f4 R[TW * NC];
    // (X3_STAMP variant builds: s_memtime per phase; slots 0 EC/tanh + output + fill, 1 EC/group wait, 2 EC/owner,
    //  3 EC/layer 0 + tanh, 4 M/slab write + group wait, 5 M/MFMAs, 7 barrier)
    uint64_t ph_[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t tp_ = X3_STAMP ? __builtin_amdgcn_s_memtime() : 0;
    // (an opaque zero, refreshed every step, added to every weight offset and LDS table base: the weights and
    //  tables are the same every step, and without it the compiler hoists the loop-invariant loads out of the loop)
    int wz = 0;
    const double* Cz = C;
    const float* Blz = Bl;
    const float* Boutz = Bout;
    auto refresh = [&]() __attribute__((always_inline)) {
        wz = 0;
        asm volatile("" : "+s"(wz));
        Cz = C + wz;
        Blz = Bl + wz;
        Boutz = Bout + wz;
    };

    // layer 0's fragments: tile pairs through three register sets, two pairs ahead of the MFMAs
    h8 a0h[3][2], a0l[3][2];
    auto load0 = [&](int p, auto SETc) __attribute__((always_inline)) {
        constexpr int st = decltype(SETc)::value;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            a0h[st][v] = fload(rs0, voff, wz + (2 * p + v) * 2048);
            a0l[st][v] = fload(rs0, voff, wz + (2 * p + v) * 2048 + 1024);
        }
    };
    // EC's hand-off inside the group: a workgroup-scope release of this wave's LDS writes (partials, action
    // inputs), the count, layer 0's first fragments (in flight through the wait and the owner phase), the wait
    // for the group's four waves, an acquire.  LDS only ("local"), so the weight loads stay in flight
    auto ec_sync = [&](int h) __attribute__((always_inline)) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if (lane == 0) __hip_atomic_fetch_add(cnt + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        load0(0, std::integral_constant<int, 0>{});
        load0(1, std::integral_constant<int, 1>{});
        PP3_PIN_LOADS();
        X3_ST(0);
        while (__hip_atomic_load(cnt + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 4 * (h + 1))
            __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        X3_ST(1);
    };
    // EC, step h's head: normalise the state (dynamics.py:109), f32 (TF feed), the staged actions; the column's
    // power-of-two scale (max |x| -> [2^11, 2^12)); the split (this lane's B fragment of layer 0); layer 0
    // [S+A -> h] for the own column, its tanh and split: every tile pair is one k-step of the hidden-layer input
    auto ec_head = [&]() __attribute__((always_inline)) {
        const float* xr = xa + (16 * wl + m) * A;
        float xin[8];
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = 16 * v + 4 * q + r;
                float xv = 0.f;
                if (d < S) xv = (float)div_rn(__dsub_rn(s[v][r], Cz[0 * 32 + d]), Cz[1 * 32 + d], Cz[8 * 32 + d]);
                else if (d < S + A) xv = xr[d - S];
                xin[4 * v + r] = xv;
            }
        float mx = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(xin[i]));
        mx = max_rows32(max_rows16(mx));
        int e = 0;
        (void)frexpf(mx, &e);                          // mx in [2^(e-1), 2^e)
        int sh = 12 - e;
        sh = mx > 0.f ? (sh < -100 ? -100 : (sh > 100 ? 100 : sh)) : 0;
        const float sc = ldexpf(1.0f, sh);
#pragma unroll
        for (int i = 0; i < 8; ++i) xin[i] *= sc;
        h8 bh, bl;
        split8(xin, bh, bl);
        const float cf = ldexpf(a.winv[0], -sh) * kTanhK;   // this lane's column factor
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (p + 2 < P) {
                if (p % 3 == 0) load0(p + 2, std::integral_constant<int, 2>{});
                else if (p % 3 == 1) load0(p + 2, std::integral_constant<int, 0>{});
                else load0(p + 2, std::integral_constant<int, 1>{});
            }
            PP3_PIN_LOADS();
            f4 z0 = (f4){0.f, 0.f, 0.f, 0.f}, z1 = (f4){0.f, 0.f, 0.f, 0.f};
            z0 = mfma16(a0h[p % 3][0], bh, z0);
            z1 = mfma16(a0h[p % 3][1], bh, z1);
            z0 = mfma16(a0h[p % 3][0], bl, z0);
            z1 = mfma16(a0h[p % 3][1], bl, z1);
            z0 = mfma16(a0l[p % 3][0], bh, z0);
            z1 = mfma16(a0l[p % 3][1], bh, z1);
            h8 xh, xl;
            epi_pair(z0, z1, cf, Blz, 2 * p, q, xh, xl);
            R[2 * p] = __builtin_bit_cast(f4, xh);
            R[2 * p + 1] = __builtin_bit_cast(f4, xl);
        }
        X3_ST(3);
    };

    // Group 1 runs one segment ahead: group 0 sits out the first interval, group 1 the last.  Every wave
    // executes every increment, spin and barrier, whatever its candidates.
    if (grp == 0) __syncthreads();
    // ---------------- EC(0): step 0's head ----------------
    refresh();
    __builtin_amdgcn_s_setprio(PP3_PRIO_EC);
    fill_actions(0);
    ec_sync(0);
    ec_head();
    __syncthreads();
    for (int h = 0;; ++h) {
        refresh();
        // ---------------- M(h): the hidden layer ----------------
        __builtin_amdgcn_s_setprio(PP3_PRIO_M);
        X3_ST(7);
        {
            // weights in units of one tile (hi | lo) through four register sets, three units ahead of the
            // MFMAs; tile jj of this wave is tile jj & 3 of block 2wl + (jj >> 2) (rollout_x3's packing)
            auto woff = [&](int p, int jj) __attribute__((always_inline)) {
                return wz + (((2 * wl + (jj >> 2)) * P + p) * 4 + (jj & 3)) * 2048;
            };
            h8 th[4], tl[4];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                th[u] = fload(rs1, voff, woff(0, u));
                tl[u] = fload(rs1, voff, woff(0, u) + 1024);
            }
#pragma unroll
            for (int p = 0; p < P; ++p) {
                swrite(slab + sidx<NC>(p, wl, 0, lane), __builtin_bit_cast(h8, R[2 * p]));
                swrite(slab + sidx<NC>(p, wl, 1, lane), __builtin_bit_cast(h8, R[2 * p + 1]));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            if (lane == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
            for (int i = 0; i < TW * NC; ++i) R[i] = (f4){0.f, 0.f, 0.f, 0.f};
            // the group's four columns of the layer input published
            while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 4 * (h + 1))
                __builtin_amdgcn_s_sleep(1);
            // (acquire: the slab reads below cannot move above the wait)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
            X3_ST(4);
#pragma unroll 1
            for (int p = 0; p < P; ++p) {
                h8 bh[NC], bl[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) bh[c] = sread(slab + sidx<NC>(p, c, 0, lane));
#pragma unroll
                for (int c = 0; c < NC; ++c) bl[c] = sread(slab + sidx<NC>(p, c, 1, lane));
                const int pn = (p + 1) & (P - 1);              // (the last k-step's look-ahead wraps: unconditional loads)
#pragma unroll
                for (int u = 0; u < TW; ++u) {
                    const int o = woff(u + 3 < TW ? p : pn, (u + 3) % TW);
                    th[(u + 3) % 4] = fload(rs1, voff, o);
                    tl[(u + 3) % 4] = fload(rs1, voff, o + 1024);
                    __builtin_amdgcn_sched_barrier(0);         // keep the loads ahead of the MFMAs they overlap
#pragma unroll
                    for (int c = 0; c < NC; ++c) R[u * NC + c] = mfma16(th[u % 4], bh[c], R[u * NC + c]);
#pragma unroll
                    for (int c = 0; c < NC; ++c) R[u * NC + c] = mfma16(th[u % 4], bl[c], R[u * NC + c]);
#pragma unroll
                    for (int c = 0; c < NC; ++c) R[u * NC + c] = mfma16(tl[u % 4], bh[c], R[u * NC + c]);
                }
            }
            X3_ST(5);
        }
        __syncthreads();
        X3_ST(7);
        {
            int lz = lane;
            asm volatile("" : "+v"(lz));
            ln = lz;
            q = lz >> 4;
            m = lz & 15;
        }
        // ---------------- EC(h + 1): step h's tail, step h + 1's head ----------------
        __builtin_amdgcn_s_setprio(PP3_PRIO_EC);
        const bool more = h + 1 < a.H;
        if (more) fill_actions(h + 1);
        {
            f4 po[2][NC];
#pragma unroll
            for (int v = 0; v < 2; ++v)
#pragma unroll
                for (int c = 0; c < NC; ++c) po[v][c] = (f4){0.f, 0.f, 0.f, 0.f};
            h8 oh[2][2], ol[2][2];                             // the output layer's k-step wl * PW + pp, one ahead
            auto load_o = [&](int pp, auto SETc) __attribute__((always_inline)) {
                constexpr int st = decltype(SETc)::value;
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const int o = wz + (((wl * PW + pp) * 2 + v) * 2) * 1024;
                    oh[st][v] = fload(rso, voff, o);
                    ol[st][v] = fload(rso, voff, o + 1024);
                }
            };
            load_o(0, std::integral_constant<int, 0>{});
            PP3_PIN_LOADS();
#pragma unroll
            for (int pp = 0; pp < PW; ++pp) {
                if (pp + 1 < PW) {
                    if (pp % 2 == 0) load_o(pp + 1, std::integral_constant<int, 1>{});
                    else load_o(pp + 1, std::integral_constant<int, 0>{});
                }
                PP3_PIN_LOADS();
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    h8 xh, xl;
                    epi_pair(R[(2 * pp) * NC + c], R[(2 * pp + 1) * NC + c], f1, Blz + HP, wl * TW + 2 * pp, q, xh, xl);
#pragma unroll
                    for (int v = 0; v < 2; ++v) {
                        po[v][c] = mfma16(oh[pp % 2][v], xh, po[v][c]);
                        po[v][c] = mfma16(oh[pp % 2][v], xl, po[v][c]);
                        po[v][c] = mfma16(ol[pp % 2][v], xh, po[v][c]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                part0[(wl * NC + c) * 64 + ln] = po[0][c];
                if (q < nq1) part1[(wl * NC + c) * 16 * nq1 + ln] = po[1][c];
            }
        }
        ec_sync(h + 1);
        {
            f4 o[2];
            o[0] = part0[(0 * NC + wl) * 64 + ln];
            o[1] = q < nq1 ? part1[(0 * NC + wl) * 16 * nq1 + ln] : (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g2 = 1; g2 < 4; ++g2) {                   // fixed summation order
                o[0] += part0[(g2 * NC + wl) * 64 + ln];
                if (q < nq1) o[1] += part1[(g2 * NC + wl) * 16 * nq1 + ln];
            }
            // cheetah penalties on the current state (cost_functions.py:16-26): dims 5..7 in row q = 1
            const int npen = partner_row16((s[0][1] >= 0.2) + (s[0][2] >= 0.0) + (s[0][3] >= 0.0));
            const double s17 = s[1][1];
            // de-normalise + residual (dynamics.py:113,116), f64, no FMA
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const f4 bv = *reinterpret_cast<const f4*>(Boutz + 16 * v + 4 * q);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int d = 16 * v + 4 * q + r;
                    if (d < S) {
                        const float dn = fmaf(o[v][r], fo, bv[r]);                 // BiasAdd (f32)
                        const double ud = __dadd_rn(__dmul_rn((double)dn, Cz[5 * 32 + d]), Cz[4 * 32 + d]);
                        s[v][r] = __dadd_rn(s[v][r], ud);
                    }
                }
            }
            if (a.cost == BCMPC_COST_CHEETAH) {
                const double score = __dsub_rn(10.0 * (double)npen, div_rn(__dsub_rn(s[1][1], s17), 0.01, 1.0 / 0.01));
                cost = __dadd_rn(cost, score);
            }
            const int64_t cd = gc0 + 16 * wl + m;
            if (a.traj && cd < a.K) {
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int d = 16 * v + 4 * q + r;
                        if (d < S) a.traj[((int64_t)(h + 1) * a.K + cd) * S + d] = s[v][r];
                    }
            }
        }
        X3_ST(2);
        if (!more) break;
        ec_head();
        __syncthreads();
    }
    __syncthreads();                                    // the last EC's interval
    if (grp == 1) __syncthreads();
    if constexpr (X3_STAMP) {
        if (a.stamps && lane == 0)
            for (int k2 = 0; k2 < 10; ++k2) a.stamps[((size_t)blockIdx.x * 8 + w) * 10 + k2] = ph_[k2];
    }
    // the cost holder: row 0 (dims 1, 17 and the penalty count)
    const int64_t cd = gc0 + 16 * wl + (lane & 15);
    if (a.costs && cd < a.K && (lane >> 4) == 0) a.costs[cd] = cost;
}

}  // namespace bcmpc

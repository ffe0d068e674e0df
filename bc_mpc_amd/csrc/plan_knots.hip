// plan_knots.hip -- knot plans for the batched planners (gfx950): the action sequence is sampled at M <= H knots
// and interpolated to H steps.  The definition is bc_mpc_amd/knots.py; the kernel matches it bit
// for bit.
//
// plan_sample_knots writes two arrays from the environments' knot plans mu / sigma [n_envs][M][A]:
//
//   knots[m][col][j]  = clip(mu[b][m][j] + sigma[b][m][j] * n[m]),   n[0] = z[0],  n[m] = rho * n[m-1] + c * z[m]
//                       with z[m] = cem_normal(seed, cand_offset + col, m, j, iter): plan_sample_corr's arithmetic
//                       with the knot index in the place of h.  Select-refit, the MPPI updates and plan_keep read
//                       it with H := M.
//   out[h][col][j]    = clip(interpolant of the column's knots at step h)   (hold | linear | Catmull-Rom)
//                       what the rollout and plan_argmin read; no rollout kernel knows about knots.
//
// One thread per (column, action dim), as plan_sample_corr: adjacent threads are adjacent in (column, j), so every
// store of a wave, to either array, is one contiguous run.  M is a run-time value, so the knots are NOT held in a
// local array (it would go to scratch): the segment index m0 never decreases as h rises, so knot m is drawn, with
// the AR(1) state in a register, exactly when the interpolation window first needs it, stored, and kept in a
// sliding window of four registers (q3 = the newest knot).  One pass, no scratch, no LDS.  The segment (m0, r) of
// step h advances by an add and a conditional subtract (M <= H: at most one knot per step), so there is no integer
// division in the loop.  With a keep buffer, the first keep_count[b] columns of environment b take their knots from
// it (the previous iteration's elites, [n_envs][n_elite][M][A]) instead of drawing; they are stored and expanded
// by the same code.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bcmpc.h"
#include "kernels.h"
#include "device_common.h"

namespace bcmpc {

__global__ __launch_bounds__(256) void plan_sample_knots(const PlanSampleKnotsArgs p) {
    const PlanSampleCorrArgs& a = p.s;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.Ktot * a.A) return;
    const int64_t col = i / a.A;
    const int j = (int)(i - col * a.A);
    const int64_t b = col / a.K, k = col - b * a.K;    // environment, column within it
    const int64_t step = a.Ktot * a.A;                 // [m + 1][col][j] - [m][col][j] in either array
    const int M = p.M, H = a.H, kind = p.kind;
    const double* src = nullptr;                       // a carried elite's knots, or nullptr: drawn
    if (a.keep) {
        int32_t n = a.keep_count[b];
        n = n < a.n_elite ? n : a.n_elite;
        if (k < n) src = a.keep + ((b * a.n_elite + k) * M) * a.A + j;
    }
    const double* mu = a.mu + b * M * a.A + j;
    const double* sd = a.sigma + b * M * a.A + j;
    const double lo = a.consts[6 * kConstCols + j], hi = a.consts[7 * kConstCols + j];
    const uint64_t g = (uint64_t)(a.cand_offset + col);
    // the knot coordinate of step h is m0 + r / den: hold h * M / H, else h * (M - 1) / (H - 1)
    const int inc = kind == BCMPC_KNOTS_HOLD ? M : M - 1, den = kind == BCMPC_KNOTS_HOLD ? H : H - 1;
    const int look = kind == BCMPC_KNOTS_HOLD ? 0 : kind == BCMPC_KNOTS_LINEAR ? 1 : 2;   // knots the window runs ahead
    const double fden = (double)den;
    int m0 = 0, r = 0, top = -1;                       // top: the newest knot drawn
    double n = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
    for (int h = 0; h < H; ++h) {
        int need = m0 + look;
        need = need < M - 1 ? need : M - 1;
        while (top < need) {
            ++top;
            double v;
            if (src) {
                v = src[(int64_t)top * a.A];
            } else {
                const double z = cem_normal(a.seed, g, top, j, a.iter);
                n = top == 0 ? z : __dadd_rn(__dmul_rn(a.rho, n), __dmul_rn(a.c, z));
                v = __dadd_rn(mu[top * a.A], __dmul_rn(sd[top * a.A], n));
                v = v < lo ? lo : (v > hi ? hi : v);   // cem_action's clip
            }
            p.knots[top * step + i] = v;
            if (top == 0) q0 = q1 = q2 = v;            // the first knot repeated to the left
            else { q0 = q1; q1 = q2; q2 = q3; }
            q3 = v;
        }
        // q3, q2, q1, q0 = knots top, top - 1, top - 2, top - 3 (clamped at 0); d = top - m0 in [0, look]
        const int d = top - m0;
        double v;
        if (look == 0 || r == 0) {                     // hold, or a knot on the step:
            v = d == 0 ? q3 : (d == 1 ? q2 : q1);      // theta[m0], untouched
        } else {
            // (r != 0 implies m0 + 1 <= M - 1, so d >= 1; cubic with d == 1: the last knot repeated to the right)
            const double f = __ddiv_rn((double)r, fden);
            const double p1 = d == 2 ? q1 : q2, p2 = d == 2 ? q2 : q3;
            if (kind == BCMPC_KNOTS_LINEAR) {
                v = __dadd_rn(p1, __dmul_rn(f, __dsub_rn(p2, p1)));
            } else {
                const double p0 = d == 2 ? q0 : q1, p3 = q3;
                const double ca = __dsub_rn(p2, p0);
                const double cb = __dsub_rn(__dadd_rn(__dsub_rn(__dmul_rn(2.0, p0), __dmul_rn(5.0, p1)), __dmul_rn(4.0, p2)), p3);
                const double cc = __dsub_rn(__dadd_rn(__dmul_rn(3.0, __dsub_rn(p1, p2)), p3), p0);
                const double t = __dadd_rn(cb, __dmul_rn(f, cc));
                const double u = __dadd_rn(ca, __dmul_rn(f, t));
                v = __dadd_rn(p1, __dmul_rn(0.5, __dmul_rn(f, u)));
            }
        }
        a.out[h * step + i] = v < lo ? lo : (v > hi ? hi : v);
        if (inc > 0 && (r += inc) >= den) { r -= den; ++m0; }      // (inc <= den: one knot per step at most)
    }
}

hipError_t launch_plan_sample_knots(const PlanSampleKnotsArgs& p, hipStream_t st) {
    const PlanSampleCorrArgs& a = p.s;
    if (a.K < 1 || a.Ktot < a.K || a.Ktot % a.K != 0 || a.H < 1 || a.A < 1 || a.A > BCMPC_MAX_ACTION)
        return hipErrorInvalidValue;
    if (p.M < 1 || p.M > a.H || p.kind < BCMPC_KNOTS_HOLD || p.kind > BCMPC_KNOTS_CUBIC || !p.knots || !a.out)
        return hipErrorInvalidValue;
    if ((a.keep != nullptr) != (a.keep_count != nullptr) || (a.keep && a.n_elite < 1)) return hipErrorInvalidValue;
    const int64_t blocks = (a.Ktot * a.A + 255) / 256;
    if (blocks < 1 || blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plan_sample_knots, dim3((unsigned)blocks), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace bcmpc

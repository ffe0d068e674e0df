"""The PPO tests' shared regime (tests/test_ppo_host.py on the CPU, tests/test_gpu_ac_ppo.py on the device).

* ``orc.synthetic_policy`` weights for both stacks, observations at 1.5 sigma of its filter, ``logstd = -0.5``; the
  old policy is the initial policy; ``ac = oldmean + std N(0, 1)`` (actions the old policy would draw); ``atarg`` a
  standardised N(0, 1), ``ret = 3 N(0, 1)``; ``clip_param = 0.2``, ``cur_lrmult = 1``, ``entcoeff = 0.01``.
* Adam is tests/test_fit_oracle.py's ``HP`` betas and epsilon (0.5 / 0.75 / 0.5) at lr = 0.03: ``HP``'s own 0.25
  drives the ratios to 1e-10 .. 47 within six steps; 0.03 keeps clipped and unclipped rows in every later step.
* Runs are ``_three_and_ragged(n, B)``: three uniform batches, then ``[B, max(1, B - 5), B]``.

``trajectory`` is ``ppo.run``'s loop with carried state over several runs, optionally broken the ways a wrong
kernel would break it (``kind``).  ``mask_guard`` is the condition on the inputs under which a parity bound means
something across the clip's discontinuity.  ``ppo_parity_terms`` is ``parity_terms``' rule for the parameters and,
for the losses, the same rule on scales that hold where a loss crosses or starts at zero:

    pol_surr    against mean |min(surr1, surr2)| of the f64 definition
    pol_entpen  against entcoeff * |ent|
    kl          steps with kl64 == 0 must be exactly 0, the others are relative
    vf_loss, ent, bc_loss (and a BC step's loss)  relative
"""
import functools

import numpy as np

from bc_mpc_amd import ac_fit, ppo
from oracle import mpc_oracle as orc
from test_fit_oracle import HP, _three_and_ragged, parity_terms

N_ROWS = 600
LR = 0.03
CLIP, LRMULT, ENTCOEFF = 0.2, 1.0, 0.01
ADAM = dict(beta1=HP["beta1"], beta2=HP["beta2"], adam_eps=HP["eps"])
M = 32


def flat_params(w):
    out = []
    for k, b in zip(w.kernels, w.biases):
        out += [k, b]
    return out


class Problem:
    def __init__(self, S, A, hidden, L, n=N_ROWS, seed=5):
        wp, wv = orc.synthetic_policy(S, A, hidden, L), orc.synthetic_policy(S, 1, hidden, L, seed=2025)
        rs = np.random.RandomState(seed)
        self.S, self.A, self.hidden, self.L, self.n = S, A, hidden, L, n
        self.pol, self.vf = flat_params(wp), flat_params(wv)
        self.flt = (wp.ob_mean, wp.ob_std)
        self.obs = wp.ob_mean.astype(np.float64) + 1.5 * wp.ob_std.astype(np.float64) * rs.standard_normal((n, S))
        self.logstd = np.full(A, -0.5, np.float32)
        self.oldmean = ppo.snapshot_old(self.pol, self.flt, self.obs)
        self.acs = self.oldmean.astype(np.float64) + np.exp(-0.5) * rs.standard_normal((n, A))
        self.atarg = ppo.standardize(rs.standard_normal(n))
        self.ret = 3.0 * rs.standard_normal(n)
        self.bc_obs = wp.ob_mean.astype(np.float64) + 1.5 * wp.ob_std.astype(np.float64) * rs.standard_normal((n, S))
        self.bc_acs = rs.uniform(-1, 1, (n, A))


def _stale_tile(pol, prev, L):
    """``pol`` with the 16 x 16 tile at the origin of kernel 1 taken from ``prev``: a W^T copy one step behind."""
    out = list(pol)
    k = pol[2].copy()
    k[:16, :16] = prev[2][:16, :16]
    out[2] = k
    return out


def _mutated_grads(kind, state, pol, vf, logstd, obz, a, at, rt, om, oldls, eps, entc, f):
    """ppo.grads' gradient assembled again from its traced row quantities, with one thing wrong."""
    tr = {}
    losses, _ = ppo.grads(pol, vf, logstd, obz, a, at, rt, om, oldls, eps, entc, f, trace=tr)
    B = a.shape[0]
    e = f(np.float32(entc))
    hp, _mean = ppo._forward(pol, obz, f)
    hv, _v = ppo._forward(vf, obz, f)
    z, std, ratio = tr["z"], tr["std"], tr["ratio"]
    mask = np.where(tr["take1"], f(1), tr["inside"].astype(f)).astype(f)
    if kind == "mask":                                    # the clip mask ignored
        mask = np.ones_like(mask)
    g = (-(at / f(B)) * mask).astype(f)
    dlogp = g.copy() if kind == "noratio" else (g * ratio).astype(f)      # the ratio factor dropped
    if kind == "last_row":                                # the last batch row left out of the policy's sums
        dlogp[-1] = 0
    dmean = (dlogp[:, None] * (z / std)).astype(f)
    one = f(0) if kind == "minus1" else f(1)              # the -1 of (z^2 - 1) missing
    dls = np.sum(dlogp[:, None] * (z * z - one), axis=0, dtype=f) - (f(0) if kind == "noent" else e)
    dv = ((f(1) / f(B)) * ((tr["v"] - rt) * f(2))).astype(f)
    if kind == "vf_last_row":                             # the vf gradient's last row left out
        dv[-1] = 0
    polT = _stale_tile(pol, state["prev"], len(pol) // 2 - 1) if kind == "wt_stale" and "prev" in state else pol
    return losses, ppo._backward(polT, hp, dmean, f) + ppo._backward(vf, hv, dv[:, None], f) + [dls.astype(f)]


def trajectory(p, runs, dtype, kind="none", hypers=None, bc_runs=None, bc_lr=LR, traces=None, tail=None):
    """(snapshots, losses) of ``ppo.run``'s loop with carried Adam state over ``runs``: a snapshot is the flat list
    ``pol + vf + [logstd]`` after a run, losses are [steps, 6] (with ``bc_runs``, one BC batch list per run: a
    seventh column, the BC steps' losses).  ``hypers``: one (lr, eps, entcoeff) per run.  ``kind``: the mutation.
    ``tail = (bc_batches, value_batches, out)``: afterwards a plain BC run that continues the BC Adam state and a
    plain critic run with a fresh state on (obs, ret); ``out`` receives ``bc`` / ``value`` = (snapshots, losses) in
    tests/test_fit_oracle.py's form."""
    f = dtype
    pol, vf = [np.asarray(x, f) for x in p.pol], [np.asarray(x, f) for x in p.vf]
    logstd = p.logstd.astype(f)
    st = ac_fit.AdamState.zeros_like(pol + vf + [logstd], ADAM["beta1"], ADAM["beta2"], dtype=f)
    bst = ac_fit.AdamState.zeros_like(pol, ADAM["beta1"], ADAM["beta2"], dtype=f)
    oldls = p.logstd.astype(f)
    snaps, losses, state = [], [], {}
    for ri, batches in enumerate(runs):
        lr, eps, entc = (LR, CLIP * LRMULT, ENTCOEFF) if hypers is None else hypers[ri]
        if kind == "beta_powers":                         # the powers not carried between two runs
            if ri == 0:
                state["bp"] = (st.beta1_power, st.beta2_power)
            else:
                st.beta1_power, st.beta2_power = state["bp"]
        if kind == "none":
            bl, tr = [], ([] if traces is not None else None)
            got = ppo.run(pol, vf, logstd, st, p.flt, p.obs, p.acs, p.atarg, p.ret, p.oldmean, oldls, batches, lr, eps,
                          entc, dtype=f, bc=None if bc_runs is None else (p.bc_obs, p.bc_acs, bc_runs[ri], bc_lr),
                          bc_state=bst, bc_losses=bl, trace=tr, **ADAM)
            if traces is not None:
                traces += tr
            losses += [list(x) + ([bl[i]] if bc_runs is not None else []) for i, x in enumerate(got)]
        else:
            for si, idx in enumerate(batches):
                obz, a, at, rt, om = ppo.batch(p.flt, p.obs, p.acs, p.atarg, p.ret, p.oldmean, idx, f)
                if kind == "stale":                       # the old snapshot follows the policy
                    om = ppo._forward(pol, obz, f)[1]
                ls, g = _mutated_grads(kind, state, pol, vf, logstd, obz, a, at, rt, om, oldls, eps, entc, f)
                flat = pol + vf + [logstd]
                ac_fit.adam_apply(flat, g, st, lr, ADAM["beta1"], ADAM["beta2"], ADAM["adam_eps"], f)
                pol[:], vf[:] = flat[:len(pol)], flat[len(pol):-1]
                logstd[...] = flat[-1]
                state["prev"] = [x.copy() for x in pol]
                row = list(ls)
                if bc_runs is not None:
                    row += ac_fit.run(pol, bst, "policy", p.flt, p.bc_obs, p.bc_acs, [bc_runs[ri][si]], bc_lr,
                                      ADAM["beta1"], ADAM["beta2"], ADAM["adam_eps"], dtype=f)
                losses.append(row)
        snaps.append([x.copy() for x in pol + vf + [logstd]])
    if tail is not None:
        bcb, vb, out = tail
        if kind == "fresh_bc_tail":                       # the BC optimizer's state not carried into the plain run
            bst = ac_fit.AdamState.zeros_like(pol, ADAM["beta1"], ADAM["beta2"], dtype=f)
        lb = ac_fit.run(pol, bst, "policy", p.flt, p.bc_obs, p.bc_acs, bcb, bc_lr, ADAM["beta1"], ADAM["beta2"],
                        ADAM["adam_eps"], dtype=f)
        out["bc"] = ([[x.copy() for x in pol]], np.array([[x] for x in lb], np.float64))
        vst = ac_fit.AdamState.zeros_like(vf, ADAM["beta1"], ADAM["beta2"], dtype=f)
        lv = ac_fit.run(vf, vst, "value", p.flt, p.obs, p.ret[:, None], vb, LR, ADAM["beta1"], ADAM["beta2"],
                        ADAM["adam_eps"], dtype=f)
        out["value"] = ([[x.copy() for x in vf]], np.array([[x] for x in lv], np.float64))
    return snaps, np.array(losses, np.float64)


def mask_guard(tr32, tr64, run_lengths, B, M=M):
    """None when the inputs pass, else what failed.  ``tr32`` / ``tr64``: the traced row quantities of every step of
    the f32 and f64 definition trajectories.
    * take1 / inside identical in both;
    * every row's relative distance to its active boundary (hi where atarg >= 0, lo otherwise) at least 4 M times
      that step's max |ratio32 - ratio64|;
    * every run contains, after its first step, a clipped row (zero gradient) and an unclipped one; a run of
      one-row steps contains, after its first step, a clipped step and an unclipped one."""
    lo_ = 0
    for ri, n in enumerate(run_lengths):
        clipped = unclipped = 0
        for si in range(lo_, lo_ + n):
            a, b = tr32[si], tr64[si]
            if not (np.array_equal(a["take1"], b["take1"]) and np.array_equal(a["inside"], b["inside"])):
                return f"step {si}: the masks differ between f32 and f64"
            r64 = b["ratio"]
            err = float(np.max(np.abs(a["ratio"].astype(np.float64) - r64)))
            at = b["surr1"] / r64                         # (atarg's sign)
            bound = np.where(at >= 0, b["hi"], b["lo"])
            dist = float(np.min(np.abs(r64 - bound) / bound))
            if dist < 4 * M * err:
                return f"step {si}: a ratio is {dist:.3g} from its boundary, 4 M err = {4 * M * err:.3g}"
            if si > lo_:
                cut = ~(b["take1"] | b["inside"])
                clipped += int(cut.sum())
                unclipped += int((~cut).sum())
        if not (clipped and unclipped):
            return f"run {ri}: {clipped} clipped / {unclipped} unclipped rows after its first step"
        lo_ += n
    return None


def _scales(tr64, losses64, entcoeff_by_step):
    """Per step and loss column the scale an error is measured against (see the module docstring)."""
    s = np.abs(losses64[:, :6]).copy()
    for i, t in enumerate(tr64):
        s[i, 0] = float(np.mean(np.abs(np.minimum(t["surr1"], t["surr2"]))))
        s[i, 1] = abs(entcoeff_by_step[i]) * abs(losses64[i, 4])
    return s


def ppo_parity_terms(got, ref64, ref32, run_lengths, tr64, entcoeffs=None):
    """[(label, error of ``got``, the definition's f32 error, 2-ulp slack)]: ``parity_terms``' rule for every
    parameter; for the losses the same rule per run and column on the scales above."""
    empty = np.zeros((ref64[1].shape[0], 0))
    out = parity_terms((got[0], empty), (ref64[0], empty), (ref32[0], empty), run_lengths)
    entc = []
    for ri, n in enumerate(run_lengths):
        entc += [ENTCOEFF if entcoeffs is None else entcoeffs[ri]] * n
    sc = _scales(tr64, ref64[1], entc)
    lo = 0
    for ri, n in enumerate(run_lengths):
        for k in range(ref64[1].shape[1]):
            l64, lg, l32 = ref64[1][lo:lo + n, k], got[1][lo:lo + n, k], ref32[1][lo:lo + n, k]
            scale = sc[lo:lo + n, k] if k < 6 else np.abs(l64)
            use = np.ones(n, bool)
            if k == 3:                                    # kl: an exact zero stays an exact zero
                use = l64 != 0
                if np.any(lg[~use] != 0):
                    out.append((f"run{ri}/loss{k}/zero", np.inf, 0.0, 0.0))
            if not use.any() or np.all(scale[use] == 0):
                if np.any(lg[use] != l64[use]):
                    out.append((f"run{ri}/loss{k}/scale0", np.inf, 0.0, 0.0))
                continue
            eg = np.max(np.abs(lg[use] - l64[use]) / scale[use])
            eo = np.max(np.abs(l32[use] - l64[use]) / scale[use])
            out.append((f"run{ri}/loss{k}", float(eg), float(eo),
                        2.0 * float(np.max(np.spacing(scale[use].astype(np.float32)) / scale[use]))))
        lo += n
    return out


# the tiling's edges: tests/test_gpu_ac_fit.py's list for one pair of stacks
WIDTHS = [(20, 6, h, 2, 33) for h in (7, 16, 17, 128, 129, 256)]
DEPTHS = [(20, 6, 64, L, 33) for L in (1, 2, 4)]
DIMS = [(1, 1, 64, 2, 33), (20, 6, 64, 2, 33), (31, 16, 64, 2, 33)]
BATCHES = [(20, 6, 64, 2, B) for B in (1, 15, 16, 17, 33, 77, 128)]
CASES = list(dict.fromkeys(WIDTHS + DEPTHS + DIMS + BATCHES))
# a case that fails the mask guard gets another seed (the guard stays as it is)
SEEDS = {(20, 6, 7, 2, 33): 6, (20, 6, 17, 2, 33): 7,     # seed 5: no clipped row in the first run's later steps
         (31, 16, 64, 2, 33): 6,                            # seed 5: a ratio 0.008 from its boundary at 4 M err = 0.03
         (20, 6, 64, 2, 1): 20}                             # seed 5: no clipped step in the first run


@functools.lru_cache(maxsize=None)
def case(S, A, hidden, L, B):
    """The problem, its two runs, the definition's f64 / f32 trajectories with their traces, and the guard's
    verdict (computed once, read-only)."""
    p = Problem(S, A, hidden, L, seed=SEEDS.get((S, A, hidden, L, B), 5))
    runs = _three_and_ragged(N_ROWS, B)
    t64, t32 = [], []
    ref64 = trajectory(p, runs, np.float64, traces=t64)
    ref32 = trajectory(p, runs, np.float32, traces=t32)
    return p, runs, ref64, ref32, t64, t32, mask_guard(t32, t64, [3, 3], B)

"""PPO on the actor-critic: the definition of one clipped-surrogate step, and the GAE targets it trains on.

The reference's ``lossandupdate_ppo`` (ppo_bc_policy.py:90-144) is one Adam step on ``pol_surr + pol_entpen +
vf_loss`` over ``pol/``, ``vf/`` and ``logstd`` against a frozen ``old_pi`` (``assign_old_eq_new``); its outer loop
interleaves one such step with one BC step per epoch (train_mpc_ppo.py:355-372).  This module is THE definition of
that step, in NumPy, as ``ac_fit.py`` defines the BC and critic steps; csrc/ac_ppo.hip is tested against ``run``
(tests/test_gpu_ac_ppo.py).

One step on a batch of B rows ``ob`` [S], ``ac`` [A], ``atarg``, ``ret`` (all fed as f32), the old policy's
``oldmean`` [B, A] (f32 data) and ``oldlogstd`` [A].  Every operation is in ``dtype``; constants are f32 first.

    obz   = observe(filter, ob)                       the current filter, not differentiated
    mean  = pol(obz) [B, A];    v = vf(obz)[:, 0]     tanh stacks, as ac_fit.grads
    std   = exp(logstd);        z = (ac - mean) / std
    nlp   = (0.5 * sum_j z^2 + f32(0.5 log 2pi) * A) + sum_j logstd
    zo    = (ac - oldmean) / exp(oldlogstd);          nlp_old likewise from zo, oldlogstd
    ratio = exp(nlp_old - nlp)
    lo = 1 - eps;  hi = 1 + eps                       eps = f32(clip_param * cur_lrmult)
    surr1 = ratio * atarg;      surr2 = clip(ratio, lo, hi) * atarg
    pol_surr   = -mean_b min(surr1, surr2)
    ent        = sum_j (logstd_j + f32(0.5 log(2 pi e)))          the same for every row
    pol_entpen = -entcoeff * ent
    vf_loss    = mean_b (v - ret)^2
    kl         = mean_b sum_j (((logstd_j - oldlogstd_j) + (oldstd_j^2 + (oldmean - mean)^2) / (2 std_j^2)) - 0.5)
    bc_loss    = sqrt(mean over B*A of (ac - mean)^2)
    losses     = [pol_surr, pol_entpen, vf_loss, kl, ent, bc_loss]         (the reference's order)

The gradient is TF's autodiff of ``pol_surr + pol_entpen + vf_loss``:

    take1  = surr1 <= surr2            MinimumGrad: a tie goes to the first operand
    inside = lo <= ratio <= hi         clip_by_value = min(max(x, lo), hi): both ends pass the gradient
    g      = -(atarg / B) * (1 if take1 else inside)
    dlogp  = g * ratio                 (ExpGrad; d(nlp_old - nlp) / d(-nlp) = 1)
    dmean  = dlogp[:, None] * (z / std)                 -> backward through pol/ as ac_fit.grads
    dlogstd_j = sum_b dlogp_b * (z_bj^2 - 1)  -  entcoeff
    dv     = (1 / B) * ((v - ret) * 2)                  -> backward through vf/

The reference builds its distribution's flat parameter as ``concat(mean, mean * 0.0 + logstd)``; the product with
0.0 passes the gradient 0 to ``mean``, so it is left out here.  While the parameters equal the old ones, ``mean``
and ``oldmean`` are the same bits, ``ratio == 1`` and ``kl == 0`` exactly, and ``g = -atarg / B`` for every row.

ONE Adam state covers the flat list ``pol params + vf params + [logstd]`` (the reference's ``update_op_ppo``): one
pair of beta powers, one ``lr_t``.  It is not the optimizer of ``update_op_bc`` nor the critic fit's.

``gae`` and ``standardize`` are the targets of the outer loop (the reference's ``add_vtarg_and_adv`` and its
advantage normalisation), host NumPy: T is a few thousand and the scan is sequential.

``PpoTrainer`` wraps the device trainer (``bcmpc_acppo_*``, include/bcmpc.h): all arithmetic of a device run is in
csrc/ac_ppo.hip, this file only marshals arrays.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import ac_fit
from .ac_fit import AdamState, adam_apply, observe

HALF_LOG_2PI = np.float32(0.5 * np.log(2.0 * np.pi))
HALF_LOG_2PIE = np.float32(0.5 * np.log(2.0 * np.pi * np.e))
LOSS_NAMES = ("pol_surr", "pol_entpen", "vf_loss", "kl", "ent", "bc_loss")


# ------------------------------------------------------------------ targets
def gae(rew, vpred, new, nextvpred, gamma, lam):
    """(adv f32 [T], tdlamret [T]) of one segment: ``new[t]`` is 1 where step t starts an episode, ``nextvpred``
    the value after the last step (0 where the segment ends an episode).

        nonterminal_{t+1} = 1 - new[t + 1]              (new[T] = 0: the segment's end is bootstrapped)
        delta_t = rew_t + gamma * V_{t+1} * nonterminal_{t+1} - V_t
        adv_t   = delta_t + gamma * lam * nonterminal_{t+1} * adv_{t+1}        backwards from adv_T = 0
        tdlamret = adv + vpred
    """
    rew = np.asarray(rew, dtype=np.float64).reshape(-1)
    T = rew.shape[0]
    v = np.append(np.asarray(vpred, dtype=np.float64).reshape(-1), float(nextvpred))
    nw = np.append(np.asarray(new, dtype=np.float64).reshape(-1), 0.0)
    if v.shape[0] != T + 1 or nw.shape[0] != T + 1:
        raise ValueError("gae: rew, vpred and new must have the same length")
    adv = np.empty(T, np.float32)
    last = 0.0
    for t in range(T - 1, -1, -1):
        nonterminal = 1.0 - nw[t + 1]
        delta = rew[t] + gamma * v[t + 1] * nonterminal - v[t]
        last = delta + gamma * lam * nonterminal * last
        adv[t] = last
    return adv, adv + v[:-1]


def standardize(adv):
    """``(adv - mean) / std`` (train_mpc_ppo.py's advantage normalisation)."""
    adv = np.asarray(adv)
    return (adv - adv.mean()) / adv.std()


# ------------------------------------------------------------------ the step
def _forward(params, obz, f):
    L = len(params) // 2 - 1
    ks, bs = params[0::2], params[1::2]
    hs, h = [obz], obz
    for l in range(L):
        h = np.tanh(h @ ks[l] + bs[l]).astype(f)
        hs.append(h)
    return hs, (h @ ks[L] + bs[L]).astype(f)


def _backward(params, hs, dz, f):
    L = len(params) // 2 - 1
    ks = params[0::2]
    out = [None] * (2 * L + 2)
    for l in range(L, -1, -1):
        out[2 * l] = (hs[l].T @ dz).astype(f)
        out[2 * l + 1] = np.sum(dz, axis=0, dtype=f)
        if l > 0:
            a = hs[l]
            dz = ((dz @ ks[l].T) * (f(1) - a * a)).astype(f)
    return out


def _nlp(z, logstd, f):
    A = z.shape[1]
    return (f(0.5) * np.sum(z * z, axis=1, dtype=f) + f(HALF_LOG_2PI) * f(A)) + np.sum(logstd, dtype=f)


def surrogate(mean, logstd, ac, atarg, oldmean, oldlogstd, eps, dtype=np.float32):
    """The row quantities of the clipped surrogate: dict of z, std, ratio, surr1, surr2, take1, inside, lo, hi."""
    f = dtype
    std, ostd = np.exp(logstd).astype(f), np.exp(oldlogstd).astype(f)
    z = ((ac - mean) / std).astype(f)
    zo = ((ac - oldmean) / ostd).astype(f)
    ratio = np.exp(_nlp(zo, oldlogstd, f) - _nlp(z, logstd, f)).astype(f)
    lo, hi = f(1) - f(np.float32(eps)), f(1) + f(np.float32(eps))
    surr1 = ratio * atarg
    surr2 = np.minimum(np.maximum(ratio, lo), hi) * atarg
    return dict(z=z, std=std, ostd=ostd, ratio=ratio, surr1=surr1, surr2=surr2, take1=surr1 <= surr2,
                inside=(lo <= ratio) & (ratio <= hi), lo=lo, hi=hi)


def grads(pol, vf, logstd, obz, ac, atarg, ret, oldmean, oldlogstd, eps, entcoeff, dtype=np.float32, trace=None):
    """(losses [6], d (pol_surr + pol_entpen + vf_loss) / d (pol + vf + [logstd])) of one batch; every array
    already of ``dtype``.  ``trace``: a dict that receives the row quantities (the tests' mask guard)."""
    f = dtype
    B, A = ac.shape
    entcoeff = f(np.float32(entcoeff))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hp, mean = _forward(pol, obz, f)
        hv, vout = _forward(vf, obz, f)
        v = vout[:, 0]
        s = surrogate(mean, logstd, ac, atarg, oldmean, oldlogstd, eps, f)
        z, std, ostd, ratio = s["z"], s["std"], s["ostd"], s["ratio"]
        pol_surr = f(-np.mean(np.minimum(s["surr1"], s["surr2"]), dtype=f))
        ent = f(np.sum(logstd + f(HALF_LOG_2PIE), dtype=f))
        pol_entpen = f(-entcoeff * ent)
        dvr = v - ret
        vf_loss = f(np.mean(dvr * dvr, dtype=f))
        dm = oldmean - mean
        kl = f(np.mean(np.sum(((logstd - oldlogstd) + (ostd * ostd + dm * dm) / (f(2) * std * std)) - f(0.5),
                              axis=1, dtype=f), dtype=f))
        d = ac - mean
        bc_loss = f(np.sqrt(np.mean(d * d, dtype=f)))
        mask = np.where(s["take1"], f(1), s["inside"].astype(f)).astype(f)
        g = (-(atarg / f(B)) * mask).astype(f)
        dlogp = (g * ratio).astype(f)
        dmean = (dlogp[:, None] * (z / std)).astype(f)
        dlogstd = (np.sum(dlogp[:, None] * (z * z - f(1)), axis=0, dtype=f) - entcoeff).astype(f)
        dv = ((f(1) / f(B)) * (dvr * f(2)))[:, None].astype(f)
        out = _backward(pol, hp, dmean, f) + _backward(vf, hv, dv, f) + [dlogstd]
    if trace is not None:
        trace.update(s, mean=mean, v=v, dlogp=dlogp)
    return np.array([pol_surr, pol_entpen, vf_loss, kl, ent, bc_loss], dtype=f), out


def batch(flt, obs, acs, atarg, ret, oldmean, idx, dtype=np.float32):
    """(obz, ac, atarg, ret, oldmean) of the rows ``idx``: the filter in f32, everything else fed as f32, then
    widened to ``dtype``."""
    idx = np.asarray(idx)
    f32 = np.float32
    return (observe(flt, np.asarray(obs, dtype=np.float64)[idx]).astype(dtype),
            np.asarray(acs, dtype=np.float64)[idx].astype(f32).reshape(len(idx), -1).astype(dtype),
            np.asarray(atarg, dtype=np.float64).reshape(-1)[idx].astype(f32).astype(dtype),
            np.asarray(ret, dtype=np.float64).reshape(-1)[idx].astype(f32).astype(dtype),
            np.asarray(oldmean, dtype=f32)[idx].astype(dtype))


def snapshot_old(old_pol: Sequence[np.ndarray], old_filter, obs) -> np.ndarray:
    """``oldmean`` [n, A] f32 of all data rows from the old parameters and the old filter, in f32.  It is data of
    every trajectory, the f64 one too: an input, like ``ac``."""
    ps = [np.asarray(p, np.float32) for p in old_pol]
    with np.errstate(invalid="ignore"):
        return _forward(ps, observe(old_filter, obs), np.float32)[1]


def run(pol: List[np.ndarray], vf: List[np.ndarray], logstd: np.ndarray, adam_state: AdamState, spec_filter, obs, acs,
        atarg, ret, oldmean, oldlogstd, batches: Sequence[np.ndarray], lr, eps, entcoeff=0.0, beta1=0.9, beta2=0.999,
        adam_eps=1e-8, dtype=np.float32, bc=None, bc_state: Optional[AdamState] = None, bc_losses: Optional[list] = None,
        trace: Optional[list] = None) -> np.ndarray:
    """THE definition of a PPO run: one Adam step per index array of ``batches`` on rows of the data (f64 arrays
    ``obs`` [n, S], ``acs`` [n, A], ``atarg`` [n], ``ret`` [n]; ``oldmean`` [n, A] f32 of ``snapshot_old``).  ``pol``,
    ``vf`` (flat ``[W_0, b_0, ..]`` lists), ``logstd`` [A] and ``adam_state`` (over ``pol + vf + [logstd]``) are
    updated in place.  ``lr``: one learning rate or one per step; ``eps = clip_param * cur_lrmult``.

    ``bc=(obs, acs, batches, lr)`` follows every PPO step with one ``ac_fit`` BC step on ``pol`` with the policy
    head's own Adam state ``bc_state`` (its losses are appended to ``bc_losses``).  Returns the losses [steps, 6],
    each taken before its update."""
    f = dtype
    ac_fit.check_params("policy", pol)
    ac_fit.check_params("value", vf)
    if logstd.dtype != np.dtype(f):
        raise ValueError("run: logstd must be an array of dtype")
    steps = len(batches)
    lrs = np.broadcast_to(np.asarray(lr, dtype=np.float64), (steps,))
    if bc is not None:
        bobs, bacs, bbatches, blr = bc
        if len(bbatches) != steps or bc_state is None:
            raise ValueError("run: bc needs one batch per PPO step and bc_state")
        blrs = np.broadcast_to(np.asarray(blr, dtype=np.float64), (steps,))
    oldls = np.asarray(oldlogstd, np.float32).astype(f)
    npol = len(pol)
    losses = np.empty((steps, 6), dtype=f)
    for i, idx in enumerate(batches):
        obz, a, at, rt, om = batch(spec_filter, obs, acs, atarg, ret, oldmean, idx, f)
        tr = {} if trace is not None else None
        losses[i], g = grads(pol, vf, logstd, obz, a, at, rt, om, oldls, eps, entcoeff, f, trace=tr)
        if trace is not None:
            trace.append(tr)
        flat = list(pol) + list(vf) + [logstd]
        adam_apply(flat, g, adam_state, lrs[i], beta1, beta2, adam_eps, f)
        pol[:] = flat[:npol]
        vf[:] = flat[npol:-1]
        logstd[...] = flat[-1]
        if bc is not None:
            bl = ac_fit.run(pol, bc_state, "policy", spec_filter, bobs, bacs, [bbatches[i]], blrs[i], beta1, beta2,
                            adam_eps, dtype=f)
            if bc_losses is not None:
                bc_losses += bl
    return losses


def lds_words(hidden: int, n_layers: int, state_dim: int, action_dim: int) -> int:
    """f32 words of LDS of acppo_rows_kernel (csrc/ac_ppo_plan.cpp): the row kernel's of ``ac_fit.lds_words`` plus
    the old means [16][16], the rows' scalars and partials [8][16] and the two std vectors [2][16]."""
    return ac_fit.lds_words(hidden, n_layers, state_dim, action_dim) + 16 * 16 + 8 * 16 + 2 * 16


# ------------------------------------------------------------------ device ---
_FP = ctypes.POINTER(ctypes.c_float)
_DP = ctypes.POINTER(ctypes.c_double)
_IP = ctypes.POINTER(ctypes.c_int64)
_SP = ctypes.POINTER(ctypes.c_int32)


def _check(lib, code: int) -> None:
    if code == 0:
        return
    msg = lib.bcmpc_acppo_last_error().decode(errors="replace")
    if code in (1, 2):                                   # BCMPC_ERR_ARG / BCMPC_ERR_UNSUPPORTED
        raise ValueError(f"[bcmpc status {code}] {msg}")
    from ._lib import BcmpcError
    raise BcmpcError(code, msg)


def _indices(batches):
    sizes = np.asarray([len(b) for b in batches], dtype=np.int32)
    idx = np.ascontiguousarray(np.concatenate(batches) if len(batches) else np.zeros(0), dtype=np.int64)
    return idx, sizes


class PpoTrainer:
    """The device PPO trainer (``bcmpc_acppo``) over a policy and a value ``ActorCriticFitter``: it trains in place
    on their device weights and owns the PPO Adam slots, ``logstd``, the old snapshot and the PPO data.  ``run``
    makes one PPO step per index array (two launches; with ``bc_batches`` one BC step of the policy fitter after
    each, two more) and returns the losses; uniform batches replay one captured graph."""

    def __init__(self, policy_fitter: ac_fit.ActorCriticFitter, value_fitter: ac_fit.ActorCriticFitter,
                 beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8):
        from . import _lib
        self._lib = _lib.load()
        self._h = None
        if not hasattr(self._lib, "bcmpc_acppo_create"):
            raise RuntimeError("libbcmpc has no PPO trainer (bcmpc_acppo_create)")
        c = _lib.AcPpoConfig(float(beta1), float(beta2), float(epsilon))
        h = ctypes.c_void_p()
        _check(self._lib, self._lib.bcmpc_acppo_create(ctypes.byref(c), policy_fitter._h, value_fitter._h,
                                                       ctypes.byref(h)))
        self._h = h
        self._pol, self._vf = policy_fitter, value_fitter        # kept alive: the trainer holds their buffers
        self.S, self.A = policy_fitter.S, policy_fitter.out

    def set_logstd(self, logstd) -> None:
        ls = np.ascontiguousarray(logstd, dtype=np.float32).reshape(-1)
        if ls.shape != (self.A,):
            raise ValueError(f"set_logstd: logstd must have shape ({self.A},)")
        _check(self._lib, self._lib.bcmpc_acppo_set_logstd(self._h, ls.ctypes.data_as(_FP)))

    def get_logstd(self) -> np.ndarray:
        ls = np.empty(self.A, np.float32)
        _check(self._lib, self._lib.bcmpc_acppo_get_logstd(self._h, ls.ctypes.data_as(_FP)))
        return ls

    def set_old(self, kernels, biases, ob_mean, ob_std, oldlogstd) -> None:
        """The old policy: its weights, its filter and its logstd (``assign_old_eq_new``'s copies)."""
        ks = [np.ascontiguousarray(k, dtype=np.float32) for k in kernels]
        bs = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in biases]
        shapes = self._pol._shapes()
        if [k.shape for k in ks] != shapes or [b.shape for b in bs] != [(s[1],) for s in shapes]:
            raise ValueError(f"set_old: kernels must have shapes {shapes}")
        mean, std = ac_fit._filter((ob_mean, ob_std))
        ls = np.ascontiguousarray(oldlogstd, dtype=np.float32).reshape(-1)
        if mean.shape != (self.S,) or std.shape != (self.S,) or ls.shape != (self.A,):
            raise ValueError("set_old: ob_mean / ob_std [S], oldlogstd [A]")
        _check(self._lib, self._lib.bcmpc_acppo_set_old(
            self._h, (_FP * len(ks))(*[k.ctypes.data_as(_FP) for k in ks]),
            (_FP * len(bs))(*[b.ctypes.data_as(_FP) for b in bs]), mean.ctypes.data_as(_FP), std.ctypes.data_as(_FP),
            ls.ctypes.data_as(_FP)))

    def set_data(self, obs, acs, atarg, ret) -> None:
        o = np.ascontiguousarray(obs, dtype=np.float64)
        n = o.shape[0]
        a = np.ascontiguousarray(np.asarray(acs, dtype=np.float64).astype(np.float32)).reshape(n, -1)
        at = np.ascontiguousarray(np.asarray(atarg, dtype=np.float64).astype(np.float32)).reshape(-1)
        rt = np.ascontiguousarray(np.asarray(ret, dtype=np.float64).astype(np.float32)).reshape(-1)
        if o.shape != (n, self.S) or a.shape != (n, self.A) or at.shape != (n,) or rt.shape != (n,):
            raise ValueError(f"set_data: obs [n, {self.S}], acs [n, {self.A}], atarg [n], ret [n]")
        _check(self._lib, self._lib.bcmpc_acppo_set_data(self._h, o.ctypes.data_as(_DP), a.ctypes.data_as(_FP),
                                                         at.ctypes.data_as(_FP), rt.ctypes.data_as(_FP), n))

    def run(self, batches: Sequence[np.ndarray], lr: float, eps: float, entcoeff: float = 0.0, bc_batches=None,
            bc_lr: float = 0.0):
        """One PPO step per index array; returns losses [steps, 6] f32, and with ``bc_batches`` (one per step, rows
        of the policy fitter's data) ``(losses, bc_losses [steps])``."""
        idx, sizes = _indices(batches)
        losses = np.empty((len(batches), 6), dtype=np.float32)
        if bc_batches is None:
            bidx = bsizes = bl = None
            pb, ps, pl = _IP(), _SP(), _FP()
        else:
            if len(bc_batches) != len(batches):
                raise ValueError("run: one BC batch per PPO step")
            bidx, bsizes = _indices(bc_batches)
            bl = np.empty(len(batches), dtype=np.float32)
            pb, ps, pl = bidx.ctypes.data_as(_IP), bsizes.ctypes.data_as(_SP), bl.ctypes.data_as(_FP)
        _check(self._lib, self._lib.bcmpc_acppo_run(
            self._h, idx.ctypes.data_as(_IP), sizes.ctypes.data_as(_SP), len(batches), ctypes.c_float(lr),
            ctypes.c_float(eps), ctypes.c_float(entcoeff), pb, ps, ctypes.c_float(bc_lr), losses.ctypes.data_as(_FP), pl))
        return losses if bc_batches is None else (losses, bl)

    @property
    def graph_captures(self) -> int:
        """0: the last run launched its steps one by one; n >= 1: it replayed a captured graph, and the trainer has
        captured n graphs so far (bcmpc_acppo_is_graph)."""
        return int(self._lib.bcmpc_acppo_is_graph(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.bcmpc_acppo_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

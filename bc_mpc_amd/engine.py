"""RolloutEngine: one device's share of MPCcontroller.get_action on libbcmpc.

Thin host wrapper over the C ABI (include/bcmpc.h).  All arithmetic happens in
the HIP kernels; this file only marshals pointers.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import knots as _knots
from . import mppi_update as _mppi_update
from . import proposals as _proposals
from . import sampling as _sampling

_ACT = {"tanh": _lib.ACT_TANH, "relu": _lib.ACT_RELU}


@dataclass
class MLPSpec:
    """Dense stack in TF layout: kernels[l] is ``[in, out]`` (tf.layers.dense,
    dynamics.py:67,70), biases[l] ``[out]``; LN params per hidden layer.

    ``model="reward"``: the two-head NNDynamicsRewardModel net (dynamics.py:150-177),
    kernels in TF creation order dense (trunk), dense_1 (delta hidden), dense_2
    (delta out), dense_3 (reward hidden), dense_4 (reward out [h, 1]); LN params
    LayerNorm (trunk), LayerNorm_1 (delta), LayerNorm_2 (reward); tanh."""
    kernels: List[np.ndarray]
    biases: List[np.ndarray]
    activation: str = "tanh"
    ln_gamma: Optional[List[np.ndarray]] = None
    ln_beta: Optional[List[np.ndarray]] = None
    model: str = "delta"

    @property
    def n_layers(self) -> int:
        return 2 if self.model == "reward" else len(self.kernels) - 1

    @property
    def hidden(self) -> int:
        return int(np.shape(self.kernels[0])[1])

    @property
    def layer_norm(self) -> bool:
        return self.ln_gamma is not None


@dataclass
class PolicySpec:
    """MlpPolicy 'pi/pol' stack (ppo_bc_policy.py:66-80): tanh dense layers then
    'final' (no activation), TF layout [in, out]; the obfilter's f32 mean/std
    (RunningMeanStd, ppo_bc_policy.py:57-60) and the DiagGaussian logstd (:79)."""
    kernels: List[np.ndarray]
    biases: List[np.ndarray]
    ob_mean: np.ndarray
    ob_std: np.ndarray
    logstd: np.ndarray

    @property
    def n_layers(self) -> int:
        return len(self.kernels) - 1

    @property
    def hidden(self) -> int:
        return int(np.shape(self.kernels[0])[1])


@dataclass
class StepResult:
    best_index: int            # global candidate index (np.argmin semantics)
    best_cost: float
    first_action: np.ndarray   # (A,) f64
    costs: Optional[np.ndarray] = None


@dataclass
class BatchResult:
    """RolloutEngine.get_actions: one record per environment (B environments, K candidates each)."""
    best_index: np.ndarray     # [B] int64, global candidate indices (cand_offset + b*K + j*)
    best_cost: np.ndarray      # [B] f64
    first_action: np.ndarray   # [B, A] f64
    costs: Optional[np.ndarray] = None   # [B, K] f64 (cem_get_actions / mppi_get_actions: [iterations, B, K])


@dataclass
class DeviceProposals:
    """Proposals in device memory for the planners' ``proposals=`` (proposals.py): ``ptr`` a device address of
    f64, ``count`` sequences per environment, read in the engine's stream order through the element strides (in
    doubles; the action dimension has stride 1).  ``keep``: whatever owns the memory, held for the call."""
    ptr: int
    count: int
    env_stride: int
    seq_stride: int
    step_stride: int
    keep: object = None


# bcmpc_mppi_stats as a NumPy record (mppi_get_actions returns one per environment)
MPPI_STATS = np.dtype([("weight_sum", "<f8"), ("ess", "<f8"), ("min_cost", "<f8"), ("n_valid", "<i8")])


def _f32(a) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# RolloutEngine.get_action's prepared-argument path for the per-step call (BCMPC_PY_FASTPATH=0: build the
# ctypes arguments every call, for A/B runs)
_GA_FAST = os.environ.get("BCMPC_PY_FASTPATH", "1") != "0"


_MT_STATE = [None]          # (bit generator, key pointer, pos pointer) of the verified global MT19937


def _legacy_mt_state():
    """NumPy's global legacy RandomState, when it runs MT19937: its bit generator and pointers to the C
    state behind ``np.random.get_state()`` -- numpy's ``mt19937_state {uint32 key[624]; int pos}`` at
    ``MT19937.ctypes.state_address`` -- which bcmpc_get_action_mt19937 reads and advances in place
    (only on success, as with the tuple path).  The layout is verified once against get_state() per
    generator object; None (the get_state / set_state path) when anything does not match."""
    bg = getattr(getattr(np.random.mtrand, "_rand", None), "_bit_generator", None)
    if type(bg) is not np.random.MT19937:
        return None
    cached = _MT_STATE[0]
    if cached is not None and cached[0] is bg:
        return cached if cached[1] is not None else None
    try:
        addr = bg.ctypes.state_address
        key_p = ctypes.cast(addr, ctypes.POINTER(ctypes.c_uint32))
        pos_p = ctypes.cast(addr + 624 * 4, ctypes.POINTER(ctypes.c_int32))
        with bg.lock:
            st = np.random.get_state()
            ok = (st[0] == "MT19937" and pos_p[0] == int(st[2])
                  and np.array_equal(np.ctypeslib.as_array(key_p, shape=(624,)), np.asarray(st[1], np.uint32)))
    except Exception:
        ok = False
    _MT_STATE[0] = (bg, key_p, pos_p) if ok else (bg, None, None)
    return _MT_STATE[0] if ok else None


def _engine_config(state_dim: int, action_dim: int, hidden: int, n_layers: int, activation: str, layer_norm: bool,
                   horizon: int, num_paths: int, device: int, cost: str, kernel: Optional[str], policy_hidden: int,
                   policy_layers: int, policy_mode: str, model: str, precision: Optional[str]):
    """The bcmpc_config of RolloutEngine's constructor arguments (and of ensemble.EnsembleEngine's): returns
    (config, resolved precision name, whether a refused split-precision create is retried in fp32)."""
    if activation not in _ACT:
        raise ValueError(f"unsupported activation {activation!r} (tanh | relu)")
    cfg = _lib.Config()
    cfg.state_dim, cfg.action_dim, cfg.hidden, cfg.n_layers = state_dim, action_dim, hidden, n_layers
    cfg.activation = _ACT[activation]
    cfg.layer_norm = int(bool(layer_norm))
    cfg.horizon = int(horizon)
    costs = {"cheetah": _lib.COST_CHEETAH, "none": _lib.COST_NONE, "reward": _lib.COST_REWARD,
             "terms": _lib.COST_TERMS}
    models = {"delta": _lib.MODEL_DELTA, "reward": _lib.MODEL_REWARD}
    if cost not in costs or model not in models:
        raise ValueError(f"cost must be one of {sorted(costs)}, model one of {sorted(models)}")
    cfg.cost, cfg.model = costs[cost], models[model]
    cfg.num_paths = int(num_paths)
    cfg.device = int(device)
    kernel = kernel or os.environ.get("BCMPC_KERNEL", "auto")
    if kernel not in _lib.KERNELS:
        raise ValueError(f"unknown kernel {kernel!r}; one of {sorted(_lib.KERNELS)}")
    cfg.kernel = _lib.KERNELS[kernel]
    if precision is None:
        precision = "split" if kernel.startswith("split") or kernel == "team" else os.environ.get("BCMPC_PRECISION", "auto")
    if precision == "auto":
        # a fused policy runs in the split kernel's 8-wave groups (dynamics hidden 449..1024;
        # the reward net: hidden <= 512)
        top = 512 if model == "reward" else 1024
        plain = activation == "tanh" and not layer_norm
        split_ok = ((plain or (model == "delta" and not policy_hidden and hidden <= 512))
                    and (model == "delta" or state_dim >= 16)
                    and (not policy_hidden or 448 < hidden <= top)
                    and kernel in ("auto", "split1", "split2", "split4", "team"))
        # the small-K team kernel also takes relu / LayerNorm dynamics under a fused policy (hidden
        # <= 256: train_mpc_ppo.py's 2x256 relu + LN net) and the LayerNorm reward net (the run.sh
        # recipe) when its grid is resident: tried in split, fp32 when bcmpc_create refuses
        team_try = (not split_ok and kernel == "auto" and n_layers == 2 and state_dim >= 16
                    and bool(policy_hidden or model == "reward"))
        precision = "split" if split_ok or team_try else "fp32"
    else:
        team_try = False
    if precision not in _lib.PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}; one of {sorted(_lib.PRECISIONS)}")
    cfg.precision = _lib.PRECISIONS[precision]
    if policy_mode not in _lib.POLICY_MODES:
        raise ValueError(f"unknown policy_mode {policy_mode!r}")
    cfg.policy_hidden, cfg.policy_layers = int(policy_hidden), int(policy_layers)
    cfg.policy_mode = _lib.POLICY_MODES[policy_mode]
    return cfg, precision, team_try


class _EngineCalls:
    """What RolloutEngine and ensemble.EnsembleEngine share: the host state of a fresh handle, the argument checks
    and the single-plan CEM / MPPI calls, which differ between the two only in the C entry point (``_CEM`` /
    ``_MPPI``).  The class provides ``_lib``, ``_h``, ``state_dim``, ``action_dim``, ``horizon``, ``num_paths``."""
    _CEM, _MPPI = "bcmpc_cem_get_action", "bcmpc_mppi_get_action"
    _CEM_S, _MPPI_S = "bcmpc_cem_get_action_s", "bcmpc_mppi_get_action_s"     # (None: no such entry)
    _MPPI_X = "bcmpc_mppi_get_action_x"
    _CEM_P, _MPPI_P = "bcmpc_cem_get_action_p", "bcmpc_mppi_get_action_p"
    _CEM_K, _MPPI_K = "bcmpc_cem_get_action_k", "bcmpc_mppi_get_action_k"

    def _fresh(self) -> None:
        """The wrapper's host state for a handle nothing has been set on yet."""
        self._keep = []
        self._wver = None
        self._pol = None
        self._gamma = None          # the discount the library holds (set_discount); None: never set
        self.comm = None
        self._mt_fast = None        # get_action_numpy_stream's prepared ctypes arguments
        self._ga_fast = None        # get_action's (device actions, no cost vector) prepared ctypes arguments
        self.cost_terms = None      # the TermCost of a cost="terms" engine (set_cost_terms)
        self._cost_inputs = None    # the arrays of the last set_cost_inputs
        self._value = None          # the terminal value the library holds (set_terminal_value)

    def _state(self, state) -> np.ndarray:
        st = _f64(state).reshape(-1)
        if st.shape[0] != self.state_dim:
            raise ValueError(f"state has {st.shape[0]} dims, expected {self.state_dim}")
        return st

    def _actions(self, actions, dims: str = "(H, K, A)"):
        """``actions`` as the kernels' ``[H, num_paths, A]`` f64 array and its pointer; (None, None): device Philox."""
        if actions is None:
            return None, None
        actions = _f64(actions)
        if actions.shape != (self.horizon, self.num_paths, self.action_dim):
            raise ValueError(f"actions shape {actions.shape} != {dims} = "
                             f"{(self.horizon, self.num_paths, self.action_dim)}")
        return actions, _dp(actions)

    def _sampling(self, rho, keep_elites=False):
        """The ``_lib.Sampling`` of a planner call's ``rho`` / ``keep_elites`` (sampling.py), or None at the
        defaults: the call then goes to the entry point it has always gone to."""
        rho, keep = _sampling.check_rho(rho), _sampling.check_keep_elites(keep_elites)
        return _lib.Sampling(rho, int(keep), 0) if rho != 0.0 or keep else None

    def _mppi_ext(self, control_cost, adapt_sigma, sigma_alpha, min_std, max_std, temperature):
        """The ``_lib.MppiExt`` of an MPPI call's control-cost weight and sigma update (mppi_update.py), or None
        with both switched off: the call then goes to the entry point it has always gone to."""
        weight, adapt, alpha, lo, hi = _mppi_update.check_options(control_cost, adapt_sigma, sigma_alpha, min_std,
                                                                  max_std, temperature)
        return _lib.MppiExt(weight, int(adapt), 0, alpha, lo, hi) if weight != 0.0 or adapt else None

    def _proposals(self, proposals, n_envs: Optional[int], n_elite: int = 0):
        """The ``_lib.Proposals`` of a planner call's ``proposals=`` (proposals.py) and what keeps its memory alive,
        or ``(None, None)`` without: the call then goes to the entry point it has always gone to.  A host array is
        ``[P, H, A]`` (``n_envs`` None: the single calls) or ``[n_envs, P, H, A]``; ``DeviceProposals`` names device
        memory.  ``n_elite``: the carried elites of a CEM call with ``keep_elites`` (they keep the first columns)."""
        if proposals is None:
            return None, None
        B = 1 if n_envs is None else int(n_envs)
        K = self.num_paths // B
        if isinstance(proposals, DeviceProposals):
            d = proposals
            _proposals.check_count(d.count, K, n_elite)
            _proposals.check_strides(B, d.count, self.horizon, self.action_dim, d.env_stride, d.seq_stride, d.step_stride)
            return _lib.Proposals(int(d.ptr), int(d.count), 1, int(d.env_stride), int(d.seq_stride),
                                  int(d.step_stride)), d
        arr = _proposals.as_sequences(proposals, self.horizon, self.action_dim, n_envs)
        P = _proposals.check_count(arr.shape[-3], K, n_elite)
        return _lib.Proposals(arr.ctypes.data, P, 0, *_proposals.canonical_strides(P, self.horizon, self.action_dim)), arr

    def _knots(self, knots, knot_interp, proposals):
        """The ``_lib.Knots`` of a planner call's ``knots`` / ``knot_interp`` (knots.py), or None with ``knots=None``:
        the call then goes to the entry point it has always gone to.  Knots with proposals are refused here."""
        M = _knots.check_knots(knots, self.horizon)
        kind = _knots.check_interp(knot_interp)
        if M is None:
            return None
        if proposals is not None:
            raise NotImplementedError(f"{type(self).__name__}: knots with proposals are not built (a given action "
                                      "sequence has no knot representation to refit on)")
        return _lib.Knots(M, _knots.KINDS.index(kind))

    def _step_result(self, res, costs=None) -> StepResult:
        return StepResult(int(res.best_index), float(res.best_cost),
                          np.array(res.first_action[: self.action_dim], dtype=np.float64), costs)

    # ------------------------------------------------------------------ CEM / MPPI, one plan
    def _s_entry(self, name: Optional[str], what: str, options: str = "correlated noise and elite carry-over"):
        if name is None:
            raise NotImplementedError(f"{type(self).__name__}.{what}: {options} are not built for ensembles")
        return getattr(self._lib, name)

    def cem_get_action(self, state, mu, sigma, iterations: int, n_elite: int, alpha: float,
                       seed: int, rho: float = 0.0, keep_elites: bool = False, proposals=None,
                       knots: Optional[int] = None, knot_interp: str = "linear"
                       ) -> Tuple[StepResult, np.ndarray, np.ndarray]:
        """All CEM iterations on this device (bcmpc_cem_get_action; an ensemble: bcmpc_ensemble_cem_get_action,
        the elites of every iteration chosen by the combined value).  ``mu``/``sigma`` are ``[H, A]``; returns
        (result with best_index = iteration*K + candidate, mu', sigma').  ``rho`` / ``keep_elites``:
        temporally correlated noise and elite carry-over (sampling.py; bcmpc_cem_get_action_s).  ``proposals``
        (``[P, H, A]`` or ``DeviceProposals``): given sequences in the last P columns of every iteration's
        population (proposals.py; bcmpc_cem_get_action_p).  ``knots`` (M in ``[1, H]``) / ``knot_interp``: the
        plan is sampled at M knots and interpolated (knots.py; bcmpc_cem_get_action_k); ``mu`` / ``sigma`` and
        the returned plan are then ``[M, A]``."""
        smp = self._sampling(rho, keep_elites)
        kn = self._knots(knots, knot_interp, proposals)
        prop, _alive = self._proposals(proposals, None, int(n_elite) if smp is not None and smp.keep_elites else 0)
        st = self._state(state)
        shape = (self.horizon if kn is None else kn.count, self.action_dim)
        m = np.array(mu, dtype=np.float64, copy=True).reshape(shape)
        s = np.array(sigma, dtype=np.float64, copy=True).reshape(shape)
        p = _lib.Cem(int(iterations), int(n_elite), float(alpha), 0)
        res = _lib.Result()
        if kn is not None:
            _lib.check(self._s_entry(self._CEM_K, "cem_get_action", "knot plans")(
                self._h, _dp(st), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None, None,
                ctypes.byref(kn), ctypes.c_uint64(seed & (2**64 - 1)), _dp(m), _dp(s), ctypes.byref(res)))
        elif prop is not None:
            _lib.check(self._s_entry(self._CEM_P, "cem_get_action", "proposals")(
                self._h, _dp(st), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None, ctypes.byref(prop),
                ctypes.c_uint64(seed & (2**64 - 1)), _dp(m), _dp(s), ctypes.byref(res)))
        elif smp is None:
            _lib.check(getattr(self._lib, self._CEM)(self._h, _dp(st), ctypes.byref(p),
                                                     ctypes.c_uint64(seed & (2**64 - 1)), _dp(m), _dp(s),
                                                     ctypes.byref(res)))
        else:
            _lib.check(self._s_entry(self._CEM_S, "cem_get_action")(
                self._h, _dp(st), ctypes.byref(p), ctypes.byref(smp), ctypes.c_uint64(seed & (2**64 - 1)), _dp(m),
                _dp(s), ctypes.byref(res)))
        return self._step_result(res), m, s

    def mppi_get_action(self, state, mu, sigma, iterations: int, temperature: float,
                        seed: int, rho: float = 0.0, control_cost=0.0, adapt_sigma: bool = False,
                        sigma_alpha: float = 0.0, min_std: float = 0.0, max_std: Optional[float] = None,
                        proposals=None, knots: Optional[int] = None, knot_interp: str = "linear"):
        """``iterations`` rounds of CEM-style rollout + MPPI update on this device (bcmpc_mppi_get_action; an
        ensemble: bcmpc_ensemble_mppi_get_action, the softmin weights from the combined value; DESIGN.md "MPPI").
        ``mu``/``sigma`` are ``[H, A]``; returns (the best single candidate over all rounds, best_index =
        iteration*K + candidate; the updated plan mu', whose row 0 is the action to apply; the last round's
        statistics).  sigma is not modified.  ``rho``: temporally correlated noise (sampling.py;
        bcmpc_mppi_get_action_s).

        ``control_cost`` (a weight >= 0, or True for the temperature) adds MPPI's control-cost term to the score
        the weights see -- the record stays on the raw costs, ``stats.min_cost`` is the minimum augmented score --
        and ``adapt_sigma`` refits sigma after every round as ``clamp(sigma_alpha * sigma + (1 - sigma_alpha) *
        weighted std, min_std, max_std)`` (mppi_update.py; bcmpc_mppi_get_action_x).  With
        ``adapt_sigma`` a fourth element, sigma' ``[H, A]``, is returned.

        ``proposals`` (``[P, H, A]`` or ``DeviceProposals``): given sequences in the last P columns of every round's
        population (proposals.py; bcmpc_mppi_get_action_p).  A proposal is weighted like a sample although it is
        not a draw from ``N(mu, sigma)``.

        ``knots`` (M in ``[1, H]``) / ``knot_interp``: the plan is sampled at M knots and interpolated (knots.py;
        bcmpc_mppi_get_action_k); ``mu`` / ``sigma`` and the returned plan(s) are then ``[M, A]``, and row 0 of the
        plan is still the action to apply (knot 0 sits at step 0)."""
        smp = self._sampling(rho)
        ext = self._mppi_ext(control_cost, adapt_sigma, sigma_alpha, min_std, max_std, temperature)
        kn = self._knots(knots, knot_interp, proposals)
        prop, _alive = self._proposals(proposals, None)
        st = self._state(state)
        shape = (self.horizon if kn is None else kn.count, self.action_dim)
        m = np.array(mu, dtype=np.float64, copy=True).reshape(shape)
        s = np.ascontiguousarray(np.asarray(sigma, dtype=np.float64).reshape(shape))
        p = _lib.Mppi(int(iterations), float(temperature), 0)
        res, stats = _lib.Result(), _lib.MppiStats()
        if kn is not None:
            s = np.array(s, dtype=np.float64, copy=True)           # (in / out: the caller's array is not written)
            _lib.check(self._s_entry(self._MPPI_K, "mppi_get_action", "knot plans")(
                self._h, _dp(st), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None,
                ctypes.byref(ext) if ext is not None else None, None, ctypes.byref(kn),
                ctypes.c_uint64(seed & (2**64 - 1)), _dp(m), _dp(s), ctypes.byref(res), ctypes.byref(stats)))
            adapt = ext is not None and ext.adapt_sigma
            return (self._step_result(res), m, stats, s) if adapt else (self._step_result(res), m, stats)
        if prop is not None:
            s = np.array(s, dtype=np.float64, copy=True)           # (in / out: the caller's array is not written)
            _lib.check(self._s_entry(self._MPPI_P, "mppi_get_action", "proposals")(
                self._h, _dp(st), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None,
                ctypes.byref(ext) if ext is not None else None, ctypes.byref(prop),
                ctypes.c_uint64(seed & (2**64 - 1)), _dp(m), _dp(s), ctypes.byref(res), ctypes.byref(stats)))
            adapt = ext is not None and ext.adapt_sigma
            return (self._step_result(res), m, stats, s) if adapt else (self._step_result(res), m, stats)
        if ext is not None:
            s = np.array(s, dtype=np.float64, copy=True)           # (in / out: the caller's array is not written)
            _lib.check(self._s_entry(self._MPPI_X, "mppi_get_action", "MPPI's control cost and sigma update")(
                self._h, _dp(st), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None, ctypes.byref(ext),
                ctypes.c_uint64(seed & (2**64 - 1)), _dp(m), _dp(s), ctypes.byref(res), ctypes.byref(stats)))
            return (self._step_result(res), m, stats, s) if ext.adapt_sigma else (self._step_result(res), m, stats)
        if smp is None:
            _lib.check(getattr(self._lib, self._MPPI)(self._h, _dp(st), ctypes.byref(p),
                                                      ctypes.c_uint64(seed & (2**64 - 1)), _dp(m), _dp(s),
                                                      ctypes.byref(res), ctypes.byref(stats)))
        else:
            _lib.check(self._s_entry(self._MPPI_S, "mppi_get_action")(
                self._h, _dp(st), ctypes.byref(p), ctypes.byref(smp), ctypes.c_uint64(seed & (2**64 - 1)), _dp(m),
                _dp(s), ctypes.byref(res), ctypes.byref(stats)))
        return self._step_result(res), m, stats


class RolloutEngine(_EngineCalls):
    """Owns one bcmpc_engine (one device, one candidate shard of size K)."""

    def __init__(self, state_dim: int, action_dim: int, hidden: int, n_layers: int,
                 activation: str, layer_norm: bool, horizon: int, num_paths: int,
                 device: int = 0, cost: str = "cheetah", kernel: Optional[str] = None,
                 policy_hidden: int = 0, policy_layers: int = 0, policy_mode: str = "explore",
                 model: str = "delta", precision: Optional[str] = None):
        """``cost``: "cheetah" (fused cheetah_cost_fn, needs state_dim >= 18), "reward" (the learned reward of
        ``model="reward"``), "terms" (a ``cost_functions.TermCost`` given with set_cost_terms, scored on the device
        from the trajectory; any state_dim, no fused policy) or "none" (no objective: the caller scores the
        trajectory rollout_async returns).
        ``precision``: "fp32" (v_mfma_f32_16x16x4_f32), "split" (f32-accurate hi/lo f16
        operands on v_mfma_f32_16x16x32_f16, rollout_x3.h; relu / LayerNorm only for the plain delta net
        with hidden <= 512; a fused policy needs a tanh net of hidden 449..1024, 449..512 with the reward
        net), "f16" (one f16 MFMA pass on the split slab kernels: BASELINE cfg3's "bf16 MFMA GEMM + fp32
        cost accumulate", the tanh delta net only; NOT the fp32 tolerance) or "auto" (split
        where it applies, else fp32).
        Default: "split" for the split* kernels, else $BCMPC_PRECISION or "auto"."""
        self._lib = _lib.load()
        cfg, precision, team_try = _engine_config(state_dim, action_dim, hidden, n_layers, activation, layer_norm,
                                                  horizon, num_paths, device, cost, kernel, policy_hidden,
                                                  policy_layers, policy_mode, model, precision)
        self.precision = precision
        h = ctypes.c_void_p()
        rc = self._lib.bcmpc_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc == _lib.ERR_UNSUPPORTED and team_try:
            precision = "fp32"
            cfg.precision = _lib.PRECISIONS[precision]
            self.precision = precision
            rc = self._lib.bcmpc_create(ctypes.byref(cfg), ctypes.byref(h))
        _lib.check(rc)
        self._h = h
        self.state_dim, self.action_dim = state_dim, action_dim
        self.hidden, self.n_layers, self.activation = hidden, n_layers, activation
        self.layer_norm, self.horizon, self.num_paths = bool(layer_norm), horizon, num_paths
        self.device, self.cost, self.model = device, cost, model
        self.policy_hidden, self.policy_layers, self.policy_mode = policy_hidden, policy_layers, policy_mode
        self._fresh()

    # ------------------------------------------------------------------ weights
    def set_weights(self, spec: MLPSpec, normalization: Sequence, version: int) -> None:
        """Re-sync hook; idempotent on ``version``."""
        if spec.model != self.model or spec.n_layers != self.n_layers or spec.hidden != self.hidden:
            raise ValueError("weight shapes do not match the engine configuration")
        if version == self._wver:       # bcmpc_set_weights returns at once on a known version: skip the marshalling
            return
        ks = [_f32(k) for k in spec.kernels]
        bs = [_f32(b) for b in spec.biases]
        S, A, h = self.state_dim, self.action_dim, self.hidden
        if self.model == "reward":
            exp = [(S + A, h), (h, h), (h, S), (h, h), (h, 1)]
        else:
            exp = [(S + A, h)] + [(h, h)] * (self.n_layers - 1) + [(h, S)]
        if len(ks) != len(exp) or len(bs) != len(exp):
            raise ValueError(f"expected {len(exp)} dense layers, got {len(ks)} kernels / {len(bs)} biases")
        for k, b, e in zip(ks, bs, exp):
            if k.shape != e or b.shape != (e[1],):
                raise ValueError(f"kernel {k.shape}/bias {b.shape} != expected {e}")
        FP = ctypes.POINTER(ctypes.c_float)
        karr = (FP * len(ks))(*[k.ctypes.data_as(FP) for k in ks])
        barr = (FP * len(bs))(*[b.ctypes.data_as(FP) for b in bs])
        w = _lib.Weights()
        w.kernels, w.biases = karr, barr
        keep = [ks, bs, karr, barr]
        if self.layer_norm:
            if not spec.layer_norm:
                raise ValueError("engine built with layer_norm but weights have no LN params")
            gs = [_f32(g) for g in spec.ln_gamma]
            bts = [_f32(b) for b in spec.ln_beta]
            n_ln = 3 if self.model == "reward" else self.n_layers
            if len(gs) != n_ln or len(bts) != n_ln or any(x.shape != (h,) for x in gs + bts):
                raise ValueError(f"expected {n_ln} LayerNorm gamma/beta pairs of shape ({h},)")
            garr = (FP * len(gs))(*[g.ctypes.data_as(FP) for g in gs])
            btarr = (FP * len(bts))(*[b.ctypes.data_as(FP) for b in bts])
            w.ln_gamma, w.ln_beta = garr, btarr
            keep += [gs, bts, garr, btarr]
        (mean_obs, std_obs, mean_action, std_action, *_rest) = normalization
        mean_deltas, std_deltas = normalization[8], normalization[9]
        stats = [_f64(x) for x in (mean_obs, std_obs, mean_action, std_action, mean_deltas, std_deltas)]
        for x, n in zip(stats, (S, S, A, A, S, S)):
            if x.shape != (n,):
                raise ValueError(f"normalization vector of shape {x.shape}, expected ({n},)")
        (w.mean_obs, w.std_obs, w.mean_action, w.std_action, w.mean_deltas, w.std_deltas) = [_dp(x) for x in stats]
        keep.append(stats)
        if self.model == "reward":      # dynamics.py:236 (mean_reward / std_reward: one value each)
            rstats = [_f64(normalization[4]).reshape(-1), _f64(normalization[5]).reshape(-1)]
            if any(x.shape != (1,) for x in rstats):
                raise ValueError("mean_reward / std_reward must hold exactly one value")
            w.mean_reward, w.std_reward = _dp(rstats[0]), _dp(rstats[1])
            keep.append(rstats)
        _lib.check(self._lib.bcmpc_set_weights(self._h, ctypes.byref(w), ctypes.c_uint64(version)))
        self._wver = version

    def set_policy(self, spec: PolicySpec, explore: float, version: int) -> None:
        """Policy weights of MPCcontrollerPolicyNet (controllers.py:160-178)."""
        if spec.n_layers != self.policy_layers or spec.hidden != self.policy_hidden:
            raise ValueError("policy shapes do not match the engine configuration")
        if self._pol is not None and version == self._pol[0]:   # known version: only ``explore`` can change
            self._pol[1].explore = float(explore)
            _lib.check(self._lib.bcmpc_set_policy(self._h, ctypes.byref(self._pol[1]), ctypes.c_uint64(version)))
            return
        S, A, ph = self.state_dim, self.action_dim, self.policy_hidden
        ks = [_f32(k) for k in spec.kernels]
        bs = [_f32(b) for b in spec.biases]
        exp = [(S, ph)] + [(ph, ph)] * (self.policy_layers - 1) + [(ph, A)]
        for k, b, e in zip(ks, bs, exp):
            if k.shape != e or b.shape != (e[1],):
                raise ValueError(f"policy kernel {k.shape}/bias {b.shape} != expected {e}")
        vecs = [_f32(spec.ob_mean).reshape(-1), _f32(spec.ob_std).reshape(-1), _f32(spec.logstd).reshape(-1)]
        if vecs[0].shape != (S,) or vecs[1].shape != (S,) or vecs[2].shape != (A,):
            raise ValueError("policy ob_mean/ob_std must be (S,), logstd (A,)")
        FP = ctypes.POINTER(ctypes.c_float)
        karr = (FP * len(ks))(*[k.ctypes.data_as(FP) for k in ks])
        barr = (FP * len(bs))(*[b.ctypes.data_as(FP) for b in bs])
        p = _lib.Policy(karr, barr, vecs[0].ctypes.data_as(FP), vecs[1].ctypes.data_as(FP),
                        vecs[2].ctypes.data_as(FP), float(explore))
        _lib.check(self._lib.bcmpc_set_policy(self._h, ctypes.byref(p), ctypes.c_uint64(version)))
        self._pol = (version, p, ks, bs, vecs, karr, barr)     # the struct's pointers stay valid while held here

    def first_actions(self) -> np.ndarray:
        """Step-0 actions of every candidate of the last rollout (policy engines), [K, A] f64."""
        out = np.empty((self.num_paths, self.action_dim), dtype=np.float64)
        _lib.check(self._lib.bcmpc_first_actions(self._h, _dp(out)))
        return out

    def set_discount(self, gamma: float) -> None:
        """MPCcontrollerReward.gamma (controllers.py:139): step h's reward is scaled by gamma**h.  Idempotent on
        the value: the library is told once per change (and once on a fresh engine)."""
        gamma = float(gamma)
        if gamma == self._gamma:
            return
        _lib.check(self._lib.bcmpc_set_discount(self._h, ctypes.c_double(gamma)))
        self._gamma = gamma

    @property
    def weights_version(self) -> int:
        return int(self._lib.bcmpc_weights_version(self._h))

    def predraw_stats(self) -> dict:
        """The NumPy-stream draw's counters (bcmpc_predraw_stats): the small draws' host pre-draw (hits incl.
        late, late, misses) and the large draws' speculative device draw (spec_hits, spec_misses)."""
        out = (ctypes.c_uint64 * 5)()
        _lib.check(self._lib.bcmpc_predraw_stats(self._h, out))
        return {"hits": int(out[0]), "late": int(out[1]), "misses": int(out[2]), "spec_hits": int(out[3]),
                "spec_misses": int(out[4])}

    def set_cost_terms(self, term_cost) -> None:
        """The objective of a ``cost="terms"`` engine (bcmpc_set_cost_terms): a ``cost_functions.TermCost``
        (or an iterable of its terms).  Every rollout entry raises until this has been called; calling it
        again replaces the list for the next launch.  A ``TermCost`` with ``done`` conditions also sets the
        engine's termination (bcmpc_set_termination), one without removes it; idempotent on ``key()``.  A cost
        with ``ref(c)`` values or ``rate`` terms goes through bcmpc_set_cost_terms_x, and the calls that follow
        read what ``set_cost_inputs`` left; any other cost is sent exactly as before there were such terms."""
        from .cost_functions import TermCost
        tc = term_cost if isinstance(term_cost, TermCost) else TermCost(term_cost)
        if self.cost_terms is not None and tc.key() == self.cost_terms.key():
            return
        tc.validate(self.state_dim, self.action_dim)
        if tc.extended:
            self._set_cost_terms_x(tc)
            return

        def pack(terms):
            arr = (_lib.CostTerm * max(1, len(terms)))()
            for dst, t in zip(arr, terms):
                dst.kind, dst.source, dst.index, dst.cmp = t.kind, t.source, t.index, t.cmp
                dst.weight, dst.param = t.weight, t.param
            return arr, ctypes.c_int32(len(terms))

        # the terms, then the termination (the library holds both to one budget of 32 entries: the conditions
        # it still has from the previous cost go first when the new terms would not fit beside them)
        held = self.cost_terms.done_conditions if self.cost_terms is not None else ()
        if len(tc.terms) + len(held) > _lib.MAX_COST_TERMS:
            _lib.check(self._lib.bcmpc_set_termination(self._h, None, ctypes.c_int32(0), ctypes.c_double(0.0)))
            self.cost_terms, held = None, ()
        _lib.check(self._lib.bcmpc_set_cost_terms(self._h, *pack(tc.terms)))
        self.cost_terms = None                  # (until both calls have succeeded: the next call sends all again)
        if tc.done_conditions or held:
            _lib.check(self._lib.bcmpc_set_termination(self._h, *pack(tc.done_conditions),
                                                       ctypes.c_double(tc.done_cost)))
        self.cost_terms = tc

    def _set_cost_terms_x(self, tc) -> None:
        """set_cost_terms for a cost with reference channels or rate terms: the termination first where the new
        terms would not fit beside the conditions still held, as there."""
        def pack(terms):
            arr = (_lib.CostTerm * max(1, len(terms)))()
            for dst, t in zip(arr, terms):
                dst.kind, dst.source, dst.index, dst.cmp = t.kind, t.source, t.index, t.cmp
                dst.weight, dst.param = t.weight, t.param
            return arr, ctypes.c_int32(len(terms))

        arr = (_lib.CostTermX * max(1, len(tc.terms)))()
        for dst, t in zip(arr, tc.terms):
            dst.kind, dst.source, dst.index, dst.cmp = t.kind, t.source, t.index, t.cmp
            dst.weight, dst.param, dst.ref = t.weight, t.param, t.ref
        held = self.cost_terms.done_conditions if self.cost_terms is not None else ()
        if held:        # (the slot budget counts the held conditions' dims: clear them, the new ones follow)
            _lib.check(self._lib.bcmpc_set_termination(self._h, None, ctypes.c_int32(0), ctypes.c_double(0.0)))
        self.cost_terms = None
        self._cost_inputs = None
        _lib.check(self._lib.bcmpc_set_cost_terms_x(self._h, arr, ctypes.c_int32(len(tc.terms)),
                                                    ctypes.c_int32(tc.n_ref)))
        if tc.done_conditions:
            _lib.check(self._lib.bcmpc_set_termination(self._h, *pack(tc.done_conditions),
                                                       ctypes.c_double(tc.done_cost)))
        self.cost_terms = tc

    def set_cost_inputs(self, reference=None, previous_action=None) -> None:
        """The inputs of the calls that follow on an engine whose cost has ``ref(c)`` values or ``rate`` terms
        (bcmpc_set_cost_inputs): ``reference`` ``[R]``, ``[H, R]``, ``[B, 1, R]`` or ``[B, H, R]`` f64 with
        ``R >= cost.n_ref`` (one environment, or ``B`` environments for the batched calls),
        ``previous_action`` ``[A]`` or ``[B, A]`` or None (``a_{-1} := a_0``).  One small stream-ordered upload
        each into buffers the engine owns; they stay valid until replaced."""
        tc = self.cost_terms
        if tc is None or not tc.extended:
            raise ValueError("set_cost_inputs needs a cost with reference channels or rate terms (set_cost_terms)")
        ref = None
        ref_envs = ref_steps = 0
        if tc.n_ref:
            if reference is None:
                raise ValueError(f"the cost names reference channels (n_ref = {tc.n_ref}): a reference is needed")
            ref = np.asarray(reference, dtype=np.float64)
            if ref.ndim < 1 or ref.ndim > 3:
                raise ValueError(f"reference must be [R], [H, R] or [B, H, R], not {ref.shape}")
            ref = ref.reshape((1,) * (3 - ref.ndim) + ref.shape)
            if ref.shape[2] < tc.n_ref:
                raise ValueError(f"the reference has {ref.shape[2]} channels, the cost names {tc.n_ref}")
            if ref.shape[1] not in (1, self.horizon):
                raise ValueError(f"the reference has {ref.shape[1]} steps: 1 or the horizon ({self.horizon})")
            ref = np.ascontiguousarray(ref[:, :, :tc.n_ref])
            ref_envs, ref_steps = ref.shape[0], ref.shape[1]
        elif reference is not None:
            raise ValueError("the cost names no reference channel: reference must be None")
        prev, prev_envs = None, 0
        if previous_action is not None:
            if not tc.uses_rate:
                raise ValueError("the cost has no rate term: previous_action must be None")
            prev = np.asarray(previous_action, dtype=np.float64)
            if prev.ndim not in (1, 2) or prev.shape[-1] != self.action_dim:
                raise ValueError(f"previous_action must be [A] or [B, A] with A = {self.action_dim}, not {prev.shape}")
            prev = np.ascontiguousarray(prev.reshape(-1, self.action_dim))
            prev_envs = prev.shape[0]
        _lib.check(self._lib.bcmpc_set_cost_inputs(
            self._h, _dp(ref) if ref is not None else None, ctypes.c_int32(ref_envs), ctypes.c_int32(ref_steps),
            _dp(prev) if prev is not None else None, ctypes.c_int32(prev_envs)))
        self._cost_inputs = (ref, prev)

    def cost_input_buffers(self):
        """(device address of the reference buffer, of the previous-action buffer), 0 before they exist."""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self._lib.bcmpc_cost_input_buffers(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value or 0), int(b.value or 0)

    def trajectory_cost_inputs_async(self, d_traj: int, K: int, d_costs: int, env_paths: int,
                                     d_ref: Optional[int] = None, ref_envs: int = 1, ref_steps: int = 1,
                                     d_prev: Optional[int] = None, prev_envs: int = 1,
                                     d_actions: Optional[int] = None, seed: int = 0, cand_offset: int = 0,
                                     d_mu: Optional[int] = None, d_sigma: Optional[int] = None, cem_iter: int = 0,
                                     stream: Optional[int] = None, d_term_step: Optional[int] = None) -> None:
        """``trajectory_cost_async`` for a cost with reference channels or rate terms, on device inputs
        (bcmpc_trajectory_cost_inputs_async): candidate k reads environment ``k // env_paths`` of ``d_ref``
        ``[ref_envs, ref_steps, n_ref]`` and ``d_prev`` ``[prev_envs, A]`` (None: no previous action);
        ``ref_envs`` / ``prev_envs`` are 1 or ``K // env_paths``, ``ref_steps`` 1 or the horizon."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_trajectory_cost_inputs_async(
            self._h, vp(d_traj), vp(d_actions), ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset),
            vp(d_mu), vp(d_sigma), ctypes.c_int32(cem_iter), ctypes.c_int64(K), vp(d_costs), vp(d_term_step),
            ctypes.c_int64(env_paths), vp(d_ref), ctypes.c_int32(ref_envs), ctypes.c_int32(ref_steps), vp(d_prev),
            ctypes.c_int32(prev_envs), ctypes.c_void_p(stream)))

    def trajectory_cost_async(self, d_traj: int, K: int, d_costs: int, d_actions: Optional[int] = None,
                              seed: int = 0, cand_offset: int = 0, d_mu: Optional[int] = None,
                              d_sigma: Optional[int] = None, cem_iter: int = 0,
                              stream: Optional[int] = None, d_term_step: Optional[int] = None) -> None:
        """The term-cost kernel alone on device pointers (bcmpc_trajectory_cost_async), stream-ordered:
        ``d_traj`` ``[H+1, K, S]`` f64 -> ``d_costs`` ``[K]`` f64 under the terms of set_cost_terms.  ACTION
        terms read ``d_actions`` ``[H, K, A]``, or, when it is None, the actions the rollout kernels draw
        for (``seed``, ``cand_offset + k``): the Philox shooting draw, or the CEM / MPPI sample of
        ``cem_iter`` from ``d_mu`` / ``d_sigma`` ``[H, A]``.  ``K`` need not equal ``num_paths``.  A cost with
        ``done`` conditions is scored as ``cost_functions.episode_cost`` defines; ``d_term_step`` (``[K]`` int32)
        then receives every candidate's terminating step, H where it never terminated
        (bcmpc_trajectory_cost_steps_async)."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        if d_term_step:
            _lib.check(self._lib.bcmpc_trajectory_cost_steps_async(
                self._h, vp(d_traj), vp(d_actions), ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset),
                vp(d_mu), vp(d_sigma), ctypes.c_int32(cem_iter), ctypes.c_int64(K), vp(d_costs), vp(d_term_step),
                ctypes.c_void_p(stream)))
            return
        _lib.check(self._lib.bcmpc_trajectory_cost_async(
            self._h, vp(d_traj), vp(d_actions), ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset),
            vp(d_mu), vp(d_sigma), ctypes.c_int32(cem_iter), ctypes.c_int64(K), vp(d_costs),
            ctypes.c_void_p(stream)))

    def set_terminal_value(self, spec, weight: float = -1.0, version: int = 0) -> None:
        """The engine's terminal value (bcmpc_set_terminal_value): from now on every rollout entry scores a
        candidate by ``cost + weight * float64(V(s_H))`` (``value.terminal_values`` is the definition).
        ``spec``: a ``value.ValueSpec``, or None to remove it.  Idempotent: with the same ``version`` only
        ``weight`` is passed on (no validation, packing or upload), with the same weight too nothing is."""
        if spec is None:
            if self._value is not None:
                _lib.check(self._lib.bcmpc_set_terminal_value(self._h, None, ctypes.c_double(0.0), ctypes.c_uint64(0)))
                self._value = None
            return
        from .value import ValueSpec, check_weight
        weight = check_weight(weight)
        held = self._value
        if held is not None and held[0] == version:
            if held[1] != weight:
                _lib.check(self._lib.bcmpc_set_terminal_value(self._h, ctypes.byref(held[2]), ctypes.c_double(weight),
                                                              ctypes.c_uint64(version & (2**64 - 1))))
                self._value = (version, weight) + held[2:]
            return
        if not isinstance(spec, ValueSpec):
            raise ValueError("set_terminal_value takes a bc_mpc_amd.value.ValueSpec (or None)")
        FP = ctypes.POINTER(ctypes.c_float)
        ks, bs = list(spec.kernels), list(spec.biases)
        karr = (FP * len(ks))(*[k.ctypes.data_as(FP) for k in ks])
        barr = (FP * len(bs))(*[b.ctypes.data_as(FP) for b in bs])
        v = _lib.ValueNet(karr, barr, spec.ob_mean.ctypes.data_as(FP), spec.ob_std.ctypes.data_as(FP),
                          spec.n_layers, spec.hidden, spec.state_dim, 0)
        _lib.check(self._lib.bcmpc_set_terminal_value(self._h, ctypes.byref(v), ctypes.c_double(weight),
                                                      ctypes.c_uint64(version & (2**64 - 1))))
        self._value = (version, weight, v, spec, karr, barr)     # the struct's pointers stay valid while held here

    @property
    def terminal_value(self):
        """(spec, weight, version) of the value set, or None."""
        return None if self._value is None else (self._value[3], self._value[1], self._value[0])

    def terminal_value_async(self, d_states: int, K: int, d_values: Optional[int] = None,
                             d_costs: Optional[int] = None, row_stride: Optional[int] = None,
                             stream: Optional[int] = None, d_term_step: Optional[int] = None,
                             horizon: Optional[int] = None) -> None:
        """The value kernel alone on device pointers (bcmpc_terminal_value_async), stream-ordered: row k of
        ``d_states`` (the net's ``state_dim`` f64 at ``k * row_stride``, default dense) -> ``d_values[k]`` f32
        and / or ``d_costs[k] += weight * float64(v_k)`` in place.  ``K`` need not equal ``num_paths``.  With
        ``d_term_step`` (``[K]`` int32) the add is made only where ``d_term_step[k] == horizon`` (default: the
        engine's), ``value.add_to_costs``'s gated form (bcmpc_terminal_value_masked_async)."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        stride = ctypes.c_int64((self._value[3].state_dim if self._value else self.state_dim)
                                if row_stride is None else row_stride)
        if d_term_step:
            _lib.check(self._lib.bcmpc_terminal_value_masked_async(
                self._h, vp(d_states), stride, ctypes.c_int64(K), vp(d_values), vp(d_costs), vp(d_term_step),
                ctypes.c_int32(self.horizon if horizon is None else horizon), ctypes.c_void_p(stream)))
            return
        _lib.check(self._lib.bcmpc_terminal_value_async(
            self._h, vp(d_states), stride, ctypes.c_int64(K), vp(d_values), vp(d_costs), ctypes.c_void_p(stream)))

    def last_terminal_values(self, local_indices) -> np.ndarray:
        """f32 values of the local candidates ``local_indices`` from the engine's last launch chain
        (bcmpc_last_terminal_values; a CEM / MPPI call: its last iteration).  Diagnostics: one small copy."""
        idx = np.ascontiguousarray(np.asarray(local_indices, dtype=np.int64).reshape(-1))
        out = np.empty(idx.shape[0], dtype=np.float32)
        _lib.check(self._lib.bcmpc_last_terminal_values(
            self._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.c_int32(idx.shape[0]),
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out

    def last_termination_steps(self, local_indices) -> np.ndarray:
        """int32 terminating steps (H: never) of the local candidates ``local_indices`` from the engine's last
        launch chain (bcmpc_last_termination_steps; a CEM / MPPI call: its last iteration), on an engine whose
        ``TermCost`` has ``done`` conditions.  Diagnostics: one small copy."""
        idx = np.ascontiguousarray(np.asarray(local_indices, dtype=np.int64).reshape(-1))
        out = np.empty(idx.shape[0], dtype=np.int32)
        _lib.check(self._lib.bcmpc_last_termination_steps(
            self._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.c_int32(idx.shape[0]),
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return out

    def set_action_bounds(self, low, high) -> None:
        lo, hi = _f64(low), _f64(high)
        _lib.check(self._lib.bcmpc_set_action_bounds(self._h, _dp(lo), _dp(hi)))

    # ------------------------------------------------------------------ rollout
    def get_action(self, state, actions: Optional[np.ndarray] = None, seed: int = 0,
                   cand_offset: int = 0, return_costs: bool = False) -> StepResult:
        """Synchronous host-memory control step (bcmpc_get_action)."""
        if actions is None and not return_costs and _GA_FAST:
            # the per-step call with in-kernel actions: ctypes arguments built once per shard offset and
            # reused (state copied into an engine-owned buffer, the first action out of a NumPy view on the
            # result record) -- as get_action_numpy_stream's fast path, several us of Python less per call
            fa = self._ga_fast
            if fa is None or fa[0] != cand_offset:
                sbuf = np.zeros(self.state_dim, dtype=np.float64)
                res = _lib.Result()
                first = np.ctypeslib.as_array(res.first_action)[: self.action_dim]
                cseed = ctypes.c_uint64(0)
                args = (self._h, _dp(sbuf), None, cseed, ctypes.c_int64(cand_offset), ctypes.byref(res), None)
                fa = self._ga_fast = (cand_offset, sbuf, res, first, args, cseed)
            _, sbuf, res, first, args, cseed = fa
            s = state if type(state) is np.ndarray else _f64(state)
            if s.size != self.state_dim:
                raise ValueError(f"state has {s.size} dims, expected {self.state_dim}")
            np.copyto(sbuf, s.reshape(-1), casting="unsafe")
            cseed.value = seed & (2**64 - 1)
            rc = self._lib.bcmpc_get_action(*args)
            if rc:
                _lib.check(rc)
            return StepResult(res.best_index, res.best_cost, first.copy(), None)
        st = self._state(state)
        actions, act_p = self._actions(actions)
        res = _lib.Result()
        costs = np.empty(self.num_paths, dtype=np.float64) if return_costs else None
        _lib.check(self._lib.bcmpc_get_action(
            self._h, _dp(st), act_p, ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset),
            ctypes.byref(res), _dp(costs) if costs is not None else None))
        return self._step_result(res, costs)

    def _n_envs(self, n_envs: int) -> int:
        n_envs = int(n_envs)
        if n_envs < 1:
            raise ValueError("the batched step needs at least one environment")
        if self.num_paths % n_envs != 0:
            raise ValueError(f"num_paths = {self.num_paths} is not a multiple of the {n_envs} environments")
        return n_envs

    def get_actions(self, states, actions: Optional[np.ndarray] = None, seed: int = 0,
                    cand_offset: int = 0, return_costs: bool = False) -> BatchResult:
        """Synchronous batched control step (bcmpc_get_actions_batch): ``states`` is ``[B, S]``, the
        engine's ``num_paths`` candidates are split into B runs of ``K = num_paths // B``; candidate column
        ``c = b*K + j`` belongs to environment ``b``, starts from ``states[b]`` and has the Philox index
        ``cand_offset + c``.  Record ``b`` equals ``get_action(states[b], seed=seed, cand_offset=cand_offset
        + b*K)`` of a K-candidate engine of the same kernel layout.  ``actions``: ``[H, num_paths, A]``
        (the kernels' layout, columns as above) or None (device Philox)."""
        st = _f64(states)
        if st.ndim != 2 or st.shape[1] != self.state_dim:
            raise ValueError(f"states shape {st.shape} != (B, S) = (B, {self.state_dim})")
        B = self._n_envs(st.shape[0])
        actions, act_p = self._actions(actions, "(H, B*K, A)")
        res = (_lib.Result * B)()
        costs = np.empty(self.num_paths, dtype=np.float64) if return_costs else None
        _lib.check(self._lib.bcmpc_get_actions_batch(
            self._h, _dp(st), ctypes.c_int32(B), act_p, ctypes.c_uint64(seed & (2**64 - 1)),
            ctypes.c_int64(cand_offset), res, _dp(costs) if costs is not None else None))
        rec = np.frombuffer(res, dtype=np.float64).reshape(B, 2 + _lib.MAX_ACTION)
        return BatchResult(rec[:, 0].copy().view(np.int64), rec[:, 1].copy(),
                           rec[:, 2:2 + self.action_dim].copy(),
                           costs.reshape(B, -1) if costs is not None else None)

    def rollout_batch_async(self, d_states: int, n_envs: int, d_actions: Optional[int], seed: int,
                            cand_offset: int, d_costs: int, d_results: int, stream: Optional[int] = None) -> None:
        """Device-pointer form of get_actions (bcmpc_rollout_batch_async); no host synchronisation.
        ``d_states`` ``[n_envs, S]`` f64, ``d_actions`` ``[H, num_paths, A]`` f64 or None, ``d_costs``
        ``[num_paths]`` f64 (required), ``d_results`` ``n_envs`` result records; ``stream`` as rollout_async."""
        n_envs = self._n_envs(n_envs)
        if not d_states or not d_costs or not d_results:
            raise ValueError("d_states, d_costs and d_results are required")
        if stream is None:
            stream = self.stream
        _lib.check(self._lib.bcmpc_rollout_batch_async(
            self._h, ctypes.c_void_p(d_states), ctypes.c_int32(n_envs),
            ctypes.c_void_p(d_actions) if d_actions else None, ctypes.c_uint64(seed & (2**64 - 1)),
            ctypes.c_int64(cand_offset), ctypes.c_void_p(d_costs), ctypes.c_void_p(d_results),
            ctypes.c_void_p(stream)))

    def _numpy_bounds(self, low, high):
        """Per-action f64 bounds with a finite range (np.random.uniform would not raise), else None
        (checked once per bounds content: every env step passes the same action_space arrays)."""
        key = None
        if isinstance(low, np.ndarray) and isinstance(high, np.ndarray):
            key = (low.dtype.str, low.tobytes(), high.dtype.str, high.tobytes())
            hit = getattr(self, "_bounds_cache", None)
            if hit is not None and hit[0] == key:
                return hit[1]
        lo = np.asarray(low, dtype=np.float64)
        hi = np.asarray(high, dtype=np.float64)
        if lo.shape != (self.action_dim,) or hi.shape != (self.action_dim,) or not np.all(np.isfinite(hi - lo)):
            return None
        out = (np.ascontiguousarray(lo), np.ascontiguousarray(hi))
        if key is not None:
            self._bounds_cache = (key, out)
        return out

    def numpy_stream_available(self, low, high) -> bool:
        """The global generator is NumPy's legacy MT19937 and the bounds are per-action vectors
        with a finite range (np.random.uniform would not raise)."""
        st = np.random.get_state()
        lo = np.asarray(low, dtype=np.float64)
        hi = np.asarray(high, dtype=np.float64)
        return (isinstance(st, tuple) and st[0] == "MT19937" and lo.shape == (self.action_dim,)
                and hi.shape == (self.action_dim,) and bool(np.all(np.isfinite(hi - lo))))

    def get_action_numpy_stream(self, state, low, high, k_global: int, cand_offset: int = 0,
                                return_costs: bool = False, seed: int = 0) -> Optional[StepResult]:
        """get_action on the actions ``np.random.uniform(low, high, [H, k_global, A])`` would
        return from the global legacy stream (controllers.py:53), drawn by the library's MT19937
        restatement from ``np.random.get_state()`` on the GPU (default) or on the host
        (BCMPC_MT_PATH=host) by bcmpc_get_action_mt19937; the global stream is then advanced
        exactly as that one NumPy call advances it -- only when the call succeeds (a failing call
        raises and leaves the stream untouched).  Returns None (nothing drawn) when the global
        generator is not the legacy MT19937 or the bounds are not per-action vectors."""
        mt = _legacy_mt_state()
        if mt is not None:
            # NumPy's own MT19937 state struct, read and advanced in place by the library (under the
            # generator's lock): no get_state / set_state tuple round trips (~30 us each)
            bounds = self._numpy_bounds(low, high)
            if bounds is None:
                return None
            bg, key_p, pos_p = mt
            if return_costs:
                s = self._state(state)
                res = _lib.Result()
                costs = np.empty(self.num_paths, dtype=np.float64)
                with bg.lock:
                    _lib.check(self._lib.bcmpc_get_action_mt19937(
                        self._h, _dp(s), key_p, pos_p, _dp(bounds[0]), _dp(bounds[1]), ctypes.c_int64(k_global),
                        ctypes.c_int64(cand_offset), ctypes.c_uint64(seed & (2**64 - 1)), ctypes.byref(res),
                        _dp(costs)))
                return self._step_result(res, costs)
            # the per-env-step call (no cost vector): ctypes arguments built once per (generator, bounds,
            # shard, seed) and reused -- the state goes into an engine-owned buffer, the first action is
            # copied out of a NumPy view on the result record (~6 us of Python per call less)
            key = (k_global, cand_offset)
            fa = self._mt_fast
            if fa is None or fa[0] != key or fa[5] is not bg or fa[6] is not bounds:
                sbuf = np.zeros(self.state_dim, dtype=np.float64)
                res = _lib.Result()
                first = np.ctypeslib.as_array(res.first_action)[: self.action_dim]
                cseed = ctypes.c_uint64(0)
                args = (self._h, _dp(sbuf), key_p, pos_p, _dp(bounds[0]), _dp(bounds[1]), ctypes.c_int64(k_global),
                        ctypes.c_int64(cand_offset), cseed, ctypes.byref(res), None)
                fa = self._mt_fast = (key, sbuf, res, first, args, bg, bounds, cseed)
            _, sbuf, res, first, args = fa[:5]
            fa[7].value = seed & (2**64 - 1)           # (the policy controllers' per-call Philox seed)
            s = state if type(state) is np.ndarray else _f64(state)
            if s.size != self.state_dim:
                raise ValueError(f"state has {s.size} dims, expected {self.state_dim}")
            np.copyto(sbuf, s.reshape(-1), casting="unsafe")
            with bg.lock:
                rc = self._lib.bcmpc_get_action_mt19937(*args)
            if rc:
                _lib.check(rc)
            return StepResult(res.best_index, res.best_cost, first.copy(), None)
        if not self.numpy_stream_available(low, high):
            return None
        st = np.random.get_state()
        lo = np.asarray(low, dtype=np.float64)
        hi = np.asarray(high, dtype=np.float64)
        s = self._state(state)
        key = np.array(st[1], dtype=np.uint32)
        pos = ctypes.c_int32(int(st[2]))
        res = _lib.Result()
        costs = np.empty(self.num_paths, dtype=np.float64) if return_costs else None
        _lib.check(self._lib.bcmpc_get_action_mt19937(
            self._h, _dp(s), key.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(pos), _dp(lo),
            _dp(hi), ctypes.c_int64(k_global), ctypes.c_int64(cand_offset), ctypes.c_uint64(seed & (2**64 - 1)),
            ctypes.byref(res),
            _dp(costs) if costs is not None else None))
        np.random.set_state((st[0], key, pos.value, st[3], st[4]))
        return self._step_result(res, costs)

    def numpy_stream_draw(self, low, high, k_global: int, cand_offset: int = 0) -> np.ndarray:
        """This engine's shard ``[:, cand_offset:cand_offset + K]`` of the array
        ``np.random.uniform(low, high, [H, k_global, A])`` would return from the global legacy stream,
        drawn on the GPU (bcmpc_mt19937_uniform_device); the global stream is advanced exactly as that
        one NumPy call advances it."""
        st = np.random.get_state()
        if not (isinstance(st, tuple) and st[0] == "MT19937"):
            raise ValueError("the global generator is not NumPy's legacy MT19937")
        lo, hi = _f64(low).reshape(-1), _f64(high).reshape(-1)
        if lo.shape != (self.action_dim,) or hi.shape != (self.action_dim,):
            raise ValueError("low / high must be per-action vectors")
        key = np.array(st[1], dtype=np.uint32)
        pos = ctypes.c_int32(int(st[2]))
        out = np.empty((self.horizon, self.num_paths, self.action_dim), dtype=np.float64)
        _lib.check(self._lib.bcmpc_mt19937_uniform_device(
            self._h, key.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(pos), _dp(lo), _dp(hi),
            ctypes.c_int64(k_global), ctypes.c_int64(cand_offset), _dp(out)))
        np.random.set_state((st[0], key, pos.value, st[3], st[4]))
        return out

    def rollout_async(self, d_state: int, state_stride: int, d_actions: Optional[int], seed: int,
                      cand_offset: int, d_costs: Optional[int], d_traj: Optional[int],
                      d_result: Optional[int], stream: Optional[int] = None) -> None:
        """Device-pointer form (bcmpc_rollout_async); no host synchronisation.

        ``stream`` is a raw hipStream_t (e.g. ``torch.cuda.current_stream().cuda_stream``;
        0 is the null stream); ``None`` means the engine's own stream."""
        if stream is None:
            stream = self.stream
        _lib.check(self._lib.bcmpc_rollout_async(
            self._h, ctypes.c_void_p(d_state), ctypes.c_int64(state_stride),
            ctypes.c_void_p(d_actions) if d_actions else None, ctypes.c_uint64(seed & (2**64 - 1)),
            ctypes.c_int64(cand_offset), ctypes.c_void_p(d_costs) if d_costs else None,
            ctypes.c_void_p(d_traj) if d_traj else None, ctypes.c_void_p(d_result) if d_result else None,
            ctypes.c_void_p(stream)))

    def rollout_policy_async(self, d_state: int, d_actions: Optional[int], seed: int, cand_offset: int,
                             d_costs: Optional[int], d_traj: Optional[int], d_actions_out: int,
                             d_result: Optional[int], stream: Optional[int] = None) -> None:
        """Policy engines: rollout_async plus every step's rolled-out actions ``d_actions_out``
        ``[H, K, A]`` f64 (the reference's action_paths, controllers.py:208-213)."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_rollout_policy_async(
            self._h, ctypes.c_void_p(d_state), vp(d_actions), ctypes.c_uint64(seed & (2**64 - 1)),
            ctypes.c_int64(cand_offset), vp(d_costs), vp(d_traj), ctypes.c_void_p(d_actions_out), vp(d_result),
            ctypes.c_void_p(stream)))

    def rollout_policy_batch_async(self, d_states: int, n_envs: int, d_actions: Optional[int], seed: int,
                                   cand_offset: int, d_costs: Optional[int], d_traj: Optional[int],
                                   d_actions_out: int, stream: Optional[int] = None) -> None:
        """Policy engines: rollout_policy_async with one start state per environment (bcmpc_rollout_policy_batch_async).
        ``d_states`` ``[n_envs, S]``; environment b owns columns ``[b * K, (b + 1) * K)``, ``K = num_paths //
        n_envs``, all started from ``d_states[b]``.  ``d_actions_out`` ``[H, num_paths, A]`` is then a proposal
        source with ``proposals.policy_strides(n_envs, K, A)``."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_rollout_policy_batch_async(
            self._h, ctypes.c_void_p(d_states), int(n_envs), vp(d_actions), ctypes.c_uint64(seed & (2**64 - 1)),
            ctypes.c_int64(cand_offset), vp(d_costs), vp(d_traj), ctypes.c_void_p(d_actions_out),
            ctypes.c_void_p(stream)))

    # ------------------------------------------------------------------ CEM
    def cem_rollout_async(self, d_state: int, d_mu: int, d_sigma: int, seed: int, iteration: int,
                          cand_offset: int, k_global: int, d_costs: int, d_result: Optional[int], merge: bool,
                          stream: Optional[int] = None) -> None:
        stream = self.stream if stream is None else stream
        _lib.check(self._lib.bcmpc_cem_rollout_async(
            self._h, ctypes.c_void_p(d_state), ctypes.c_void_p(d_mu), ctypes.c_void_p(d_sigma),
            ctypes.c_uint64(seed & (2**64 - 1)), int(iteration), int(cand_offset), int(k_global),
            ctypes.c_void_p(d_costs), ctypes.c_void_p(d_result) if d_result else None, int(bool(merge)),
            ctypes.c_void_p(stream)))

    def select_async(self, d_pairs: Optional[int], d_costs: Optional[int], m: int, index_base: int, n_elite: int,
                     d_out: int, d_count: int, stream: Optional[int] = None) -> None:
        stream = self.stream if stream is None else stream
        _lib.check(self._lib.bcmpc_select_async(
            self._h, ctypes.c_void_p(d_pairs) if d_pairs else None, ctypes.c_void_p(d_costs) if d_costs else None,
            int(m), int(index_base), int(n_elite), ctypes.c_void_p(d_out), ctypes.c_void_p(d_count),
            ctypes.c_void_p(stream)))

    def cem_refit_async(self, d_elite: int, d_count: int, seed: int, iteration: int, alpha: float, d_mu: int,
                        d_sigma: int, stream: Optional[int] = None) -> None:
        stream = self.stream if stream is None else stream
        _lib.check(self._lib.bcmpc_cem_refit_async(
            self._h, ctypes.c_void_p(d_elite), ctypes.c_void_p(d_count), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), float(alpha), ctypes.c_void_p(d_mu), ctypes.c_void_p(d_sigma), ctypes.c_void_p(stream)))

    # ------------------------------------------------------------------ MPPI
    def mppi_update_async(self, d_costs: int, m: int, cand_offset: int, seed: int, iteration: int,
                          temperature: float, d_mu: int, d_sigma: int, d_stats: int,
                          stream: Optional[int] = None) -> None:
        """The MPPI update alone on device pointers (bcmpc_mppi_update_async): ``d_costs`` ``[m]`` f64 are
        the costs of candidates ``cand_offset + [0, m)`` sampled at ``iteration`` from (``d_mu``,
        ``d_sigma``) ``[H, A]``; ``d_mu`` is replaced by the weighted mean, ``d_stats`` receives one
        ``_lib.MppiStats`` record.  ``m`` need not equal ``num_paths``."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_mppi_update_async(
            self._h, vp(d_costs), int(m), int(cand_offset), ctypes.c_uint64(seed & (2**64 - 1)), int(iteration),
            float(temperature), vp(d_mu), vp(d_sigma), vp(d_stats), ctypes.c_void_p(stream)))

    # ------------------------------------------------------------------ batched CEM / MPPI
    def _plan_batch_args(self, states, mu, sigma, copy_sigma: bool, steps: Optional[int] = None):
        st = _f64(states)
        if st.ndim != 2 or st.shape[1] != self.state_dim:
            raise ValueError(f"states shape {st.shape} != (B, S) = (B, {self.state_dim})")
        B = self._n_envs(st.shape[0])
        shape = (B, self.horizon if steps is None else steps, self.action_dim)
        if np.shape(mu) != shape or np.shape(sigma) != shape:
            raise ValueError(f"mu / sigma shapes {np.shape(mu)} / {np.shape(sigma)} != "
                             f"{'(B, H, A)' if steps is None else '(B, M, A)'} = {shape}")
        m = np.array(mu, dtype=np.float64, copy=True, order="C")
        s = (np.array(sigma, dtype=np.float64, copy=True, order="C") if copy_sigma
             else np.ascontiguousarray(sigma, dtype=np.float64))
        return st, B, m, s

    def _batch_result(self, res, B: int, costs, iterations: int) -> BatchResult:
        rec = np.frombuffer(res, dtype=np.float64).reshape(B, 2 + _lib.MAX_ACTION)
        return BatchResult(rec[:, 0].copy().view(np.int64), rec[:, 1].copy(), rec[:, 2:2 + self.action_dim].copy(),
                           costs.reshape(iterations, B, -1) if costs is not None else None)

    def cem_get_actions(self, states, mu, sigma, iterations: int, n_elite: int, alpha: float, seed: int,
                        cand_offset: int = 0, return_costs: bool = False, rho: float = 0.0,
                        keep_elites: bool = False, proposals=None, knots: Optional[int] = None,
                        knot_interp: str = "linear") -> Tuple[BatchResult, np.ndarray, np.ndarray]:
        """Batched CEM (bcmpc_cem_get_actions_batch): ``states`` ``[B, S]``, ``mu`` / ``sigma``
        ``[B, H, A]``, ``K = num_paths // B`` candidates and ``n_elite`` elites per environment, columns
        as for get_actions.  Returns (records with ``best_index = iteration*K + candidate`` per
        environment and ``costs`` ``[iterations, B, K]`` when asked for, mu' ``[B, H, A]``, sigma').
        ``rho`` / ``keep_elites``: temporally correlated noise and elite carry-over (sampling.py;
        bcmpc_cem_get_actions_batch_s).  ``proposals`` (``[B, P, H, A]`` or ``DeviceProposals``): every
        environment's given sequences in its last P columns (proposals.py; bcmpc_cem_get_actions_batch_p).
        ``knots`` / ``knot_interp``: as cem_get_action, the plans ``[B, M, A]`` (bcmpc_cem_get_actions_batch_k)."""
        smp = self._sampling(rho, keep_elites)
        kn = self._knots(knots, knot_interp, proposals)
        st, B, m, s = self._plan_batch_args(states, mu, sigma, True, None if kn is None else kn.count)
        prop, _alive = self._proposals(proposals, B, int(n_elite) if smp is not None and smp.keep_elites else 0)
        p = _lib.Cem(int(iterations), int(n_elite), float(alpha), 0)
        res = (_lib.Result * B)()
        costs = np.empty((max(int(iterations), 0), self.num_paths), dtype=np.float64) if return_costs else None
        if kn is not None:
            _lib.check(self._lib.bcmpc_cem_get_actions_batch_k(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None,
                None, ctypes.byref(kn), ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset), _dp(m),
                _dp(s), res, _dp(costs) if costs is not None else None))
        elif prop is not None:
            _lib.check(self._lib.bcmpc_cem_get_actions_batch_p(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None,
                ctypes.byref(prop), ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset), _dp(m), _dp(s),
                res, _dp(costs) if costs is not None else None))
        elif smp is None:
            _lib.check(self._lib.bcmpc_cem_get_actions_batch(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.c_uint64(seed & (2**64 - 1)),
                ctypes.c_int64(cand_offset), _dp(m), _dp(s), res, _dp(costs) if costs is not None else None))
        else:
            _lib.check(self._lib.bcmpc_cem_get_actions_batch_s(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.byref(smp),
                ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset), _dp(m), _dp(s), res,
                _dp(costs) if costs is not None else None))
        return self._batch_result(res, B, costs, int(iterations)), m, s

    def mppi_get_actions(self, states, mu, sigma, iterations: int, temperature: float, seed: int,
                         cand_offset: int = 0, return_costs: bool = False, rho: float = 0.0, control_cost=0.0,
                         adapt_sigma: bool = False, sigma_alpha: float = 0.0, min_std: float = 0.0,
                         max_std: Optional[float] = None, proposals=None, knots: Optional[int] = None,
                         knot_interp: str = "linear"):
        """Batched MPPI (bcmpc_mppi_get_actions_batch): as cem_get_actions, with the softmin update of
        mppi_get_action per environment.  Returns (records, mu' ``[B, H, A]`` whose rows ``[b, 0]`` are the
        actions to apply, the last round's statistics as a ``[B]`` array of MPPI_STATS).  sigma is not
        modified.  ``rho``: temporally correlated noise (sampling.py; bcmpc_mppi_get_actions_batch_s).
        ``control_cost`` / ``adapt_sigma`` / ``sigma_alpha`` / ``min_std`` / ``max_std``: as mppi_get_action
        (bcmpc_mppi_get_actions_batch_x); the returned costs stay the raw ones, and with ``adapt_sigma`` a fourth
        element, sigma' ``[B, H, A]``, is returned.  ``proposals`` (``[B, P, H, A]`` or ``DeviceProposals``): every
        environment's given sequences in its last P columns (proposals.py; bcmpc_mppi_get_actions_batch_p).
        ``knots`` / ``knot_interp``: as mppi_get_action, the plans ``[B, M, A]`` (bcmpc_mppi_get_actions_batch_k)."""
        smp = self._sampling(rho)
        ext = self._mppi_ext(control_cost, adapt_sigma, sigma_alpha, min_std, max_std, temperature)
        kn = self._knots(knots, knot_interp, proposals)
        st, B, m, s = self._plan_batch_args(states, mu, sigma, ext is not None or proposals is not None or kn is not None,
                                            None if kn is None else kn.count)
        prop, _alive = self._proposals(proposals, B)
        p = _lib.Mppi(int(iterations), float(temperature), 0)
        res = (_lib.Result * B)()
        stats = np.zeros(B, dtype=MPPI_STATS)
        costs = np.empty((max(int(iterations), 0), self.num_paths), dtype=np.float64) if return_costs else None
        d_stats, d_costs = stats.ctypes.data_as(ctypes.POINTER(_lib.MppiStats)), _dp(costs) if costs is not None else None
        if kn is not None:
            _lib.check(self._lib.bcmpc_mppi_get_actions_batch_k(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None,
                ctypes.byref(ext) if ext is not None else None, None, ctypes.byref(kn),
                ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset), _dp(m), _dp(s), res, d_stats, d_costs))
            out = self._batch_result(res, B, costs, int(iterations))
            return (out, m, stats, s) if ext is not None and ext.adapt_sigma else (out, m, stats)
        if prop is not None:
            _lib.check(self._lib.bcmpc_mppi_get_actions_batch_p(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None,
                ctypes.byref(ext) if ext is not None else None, ctypes.byref(prop), ctypes.c_uint64(seed & (2**64 - 1)),
                ctypes.c_int64(cand_offset), _dp(m), _dp(s), res, d_stats, d_costs))
            out = self._batch_result(res, B, costs, int(iterations))
            return (out, m, stats, s) if ext is not None and ext.adapt_sigma else (out, m, stats)
        if ext is not None:
            _lib.check(self._lib.bcmpc_mppi_get_actions_batch_x(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.byref(smp) if smp is not None else None,
                ctypes.byref(ext), ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset), _dp(m), _dp(s),
                res, d_stats, d_costs))
            out = self._batch_result(res, B, costs, int(iterations))
            return (out, m, stats, s) if ext.adapt_sigma else (out, m, stats)
        if smp is None:
            _lib.check(self._lib.bcmpc_mppi_get_actions_batch(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.c_uint64(seed & (2**64 - 1)),
                ctypes.c_int64(cand_offset), _dp(m), _dp(s), res, d_stats, d_costs))
        else:
            _lib.check(self._lib.bcmpc_mppi_get_actions_batch_s(
                self._h, _dp(st), ctypes.c_int32(B), ctypes.byref(p), ctypes.byref(smp),
                ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset), _dp(m), _dp(s), res, d_stats, d_costs))
        return self._batch_result(res, B, costs, int(iterations)), m, stats

    def plan_sample_async(self, d_mu: int, d_sigma: int, n_envs: int, K: int, seed: int, iteration: int,
                          cand_offset: int, d_actions: int, stream: Optional[int] = None) -> None:
        """bcmpc_plan_sample_async: ``d_actions`` ``[H, n_envs*K, A]`` f64 from the plans ``d_mu`` /
        ``d_sigma`` ``[n_envs, H, A]``."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_plan_sample_async(
            self._h, vp(d_mu), vp(d_sigma), int(n_envs), int(K), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), int(cand_offset), vp(d_actions), ctypes.c_void_p(stream)))

    def plan_sample_corr_async(self, d_mu: int, d_sigma: int, n_envs: int, K: int, seed: int, iteration: int,
                               cand_offset: int, rho: float, d_actions: int, d_keep: Optional[int] = None,
                               d_keep_count: Optional[int] = None, n_elite: int = 0,
                               stream: Optional[int] = None) -> None:
        """bcmpc_plan_sample_corr_async: plan_sample_async with AR(1) noise of coefficient ``rho``
        (sampling.correlated_actions).  ``d_keep`` ``[n_envs, n_elite, H, A]`` f64 and ``d_keep_count``
        ``[n_envs]`` i32: environment b's first ``d_keep_count[b]`` columns are copies of ``d_keep[b]``
        (sampling.carry_elites)."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_plan_sample_corr_async(
            self._h, vp(d_mu), vp(d_sigma), int(n_envs), int(K), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), int(cand_offset), float(rho), vp(d_keep), vp(d_keep_count), int(n_elite),
            vp(d_actions), ctypes.c_void_p(stream)))

    def plan_sample_prop_async(self, d_mu: int, d_sigma: int, n_envs: int, K: int, seed: int, iteration: int,
                               cand_offset: int, rho: float, d_actions: int, d_proposals: int, n_prop: int,
                               env_stride: int, seq_stride: int, step_stride: int, d_keep: Optional[int] = None,
                               d_keep_count: Optional[int] = None, n_elite: int = 0,
                               stream: Optional[int] = None) -> None:
        """bcmpc_plan_sample_prop_async: plan_sample_corr_async with environment b's LAST ``n_prop`` columns given --
        column ``K - n_prop + p`` at ``(h, j)`` is the clipped ``d_proposals[b * env_stride + p * seq_stride + h *
        step_stride + j]`` (f64, strides in doubles; proposals.inject).  The source is read only."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_plan_sample_prop_async(
            self._h, vp(d_mu), vp(d_sigma), int(n_envs), int(K), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), int(cand_offset), float(rho), vp(d_keep), vp(d_keep_count), int(n_elite),
            vp(d_proposals), int(n_prop), int(env_stride), int(seq_stride), int(step_stride), vp(d_actions),
            ctypes.c_void_p(stream)))

    def plan_keep_async(self, d_elite: int, d_count: int, d_actions: int, n_envs: int, K: int, cand_offset: int,
                        n_elite: int, d_keep: int, d_keep_count: int, stream: Optional[int] = None) -> None:
        """bcmpc_plan_keep_async: the sequences of the elites ``d_elite`` ``[n_envs, n_elite]`` / ``d_count``
        out of ``d_actions`` ``[H, n_envs*K, A]`` into ``d_keep`` ``[n_envs, n_elite, H, A]``; ``d_keep_count``
        ``[n_envs]`` receives the number of leading records copied."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_plan_keep_async(
            self._h, vp(d_elite), vp(d_count), vp(d_actions), int(n_envs), int(K), int(cand_offset), int(n_elite),
            vp(d_keep), vp(d_keep_count), ctypes.c_void_p(stream)))

    def plan_sample_knots_async(self, d_mu: int, d_sigma: int, n_envs: int, K: int, seed: int, iteration: int,
                                cand_offset: int, rho: float, knots: int, knot_interp, d_knots: int, d_actions: int,
                                d_keep: Optional[int] = None, d_keep_count: Optional[int] = None, n_elite: int = 0,
                                stream: Optional[int] = None) -> None:
        """bcmpc_plan_sample_knots_async: plan_sample_corr_async in knot space (knots.py).  The plans ``d_mu`` /
        ``d_sigma`` are ``[n_envs, M, A]`` with ``M = knots``, ``d_keep`` ``[n_envs, n_elite, M, A]``; it writes the
        clipped knots ``d_knots`` ``[M, n_envs*K, A]`` (knots.knot_values) and their expansion ``d_actions``
        ``[H, n_envs*K, A]`` (knots.expand).  ``knot_interp``: a name of ``knots.KINDS`` or its index."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        kind = _knots.KINDS.index(knot_interp) if isinstance(knot_interp, str) and knot_interp in _knots.KINDS \
            else int(knot_interp)
        _lib.check(self._lib.bcmpc_plan_sample_knots_async(
            self._h, vp(d_mu), vp(d_sigma), int(n_envs), int(K), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), int(cand_offset), float(rho), vp(d_keep), vp(d_keep_count), int(n_elite), int(knots),
            kind, vp(d_knots), vp(d_actions), ctypes.c_void_p(stream)))

    def cem_refit_batch_steps_async(self, d_elite: int, d_count: int, n_envs: int, n_elite: int, seed: int,
                                    iteration: int, alpha: float, d_mu: int, d_sigma: int, d_actions: int, K: int,
                                    cand_offset: int, steps: int, stream: Optional[int] = None) -> None:
        """bcmpc_cem_refit_batch_steps_async: cem_refit_batch_async on ``d_actions`` ``[steps, n_envs*K, A]`` and
        plans ``[n_envs, steps, A]`` (a knot array: ``steps = M``)."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_cem_refit_batch_steps_async(
            self._h, vp(d_elite), vp(d_count), int(n_envs), int(n_elite), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), float(alpha), vp(d_mu), vp(d_sigma), vp(d_actions), int(K), int(cand_offset), int(steps),
            ctypes.c_void_p(stream)))

    def mppi_update_batch_steps_async(self, d_costs: int, n_envs: int, K: int, cand_offset: int, seed: int,
                                      iteration: int, temperature: float, d_mu: int, d_sigma: int, d_stats: int,
                                      d_actions: int, steps: int, stream: Optional[int] = None) -> None:
        """bcmpc_mppi_update_batch_steps_async: mppi_update_batch_async on ``d_actions`` ``[steps, n_envs*K, A]``."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_mppi_update_batch_steps_async(
            self._h, vp(d_costs), int(n_envs), int(K), int(cand_offset), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), float(temperature), vp(d_mu), vp(d_sigma), vp(d_stats), vp(d_actions), int(steps),
            ctypes.c_void_p(stream)))

    def plan_keep_steps_async(self, d_elite: int, d_count: int, d_actions: int, n_envs: int, K: int, cand_offset: int,
                              n_elite: int, d_keep: int, d_keep_count: int, steps: int,
                              stream: Optional[int] = None) -> None:
        """bcmpc_plan_keep_steps_async: plan_keep_async on ``d_actions`` ``[steps, n_envs*K, A]`` into ``d_keep``
        ``[n_envs, n_elite, steps, A]``."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_plan_keep_steps_async(
            self._h, vp(d_elite), vp(d_count), vp(d_actions), int(n_envs), int(K), int(cand_offset), int(n_elite),
            vp(d_keep), vp(d_keep_count), int(steps), ctypes.c_void_p(stream)))

    def mppi_control_cost_steps_async(self, d_costs: int, d_actions: int, n_envs: int, K: int, d_mu: int, d_sigma: int,
                                      weight: float, d_scores: int, steps: int, stream: Optional[int] = None) -> None:
        """bcmpc_mppi_control_cost_steps_async: mppi_control_cost_async on ``d_actions`` ``[steps, n_envs*K, A]``."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_mppi_control_cost_steps_async(
            self._h, vp(d_costs), vp(d_actions), int(n_envs), int(K), vp(d_mu), vp(d_sigma), float(weight),
            vp(d_scores), int(steps), ctypes.c_void_p(stream)))

    def mppi_sigma_update_steps_async(self, d_scores: int, d_actions: int, n_envs: int, K: int, temperature: float,
                                      d_mu_new: int, d_sigma: int, steps: int, alpha: float = 0.0,
                                      min_std: float = 0.0, max_std: Optional[float] = None,
                                      stream: Optional[int] = None) -> None:
        """bcmpc_mppi_sigma_update_steps_async: mppi_sigma_update_async on ``d_actions`` ``[steps, n_envs*K, A]``."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_mppi_sigma_update_steps_async(
            self._h, vp(d_scores), vp(d_actions), int(n_envs), int(K), float(temperature), vp(d_mu_new), vp(d_sigma),
            float(alpha), float(min_std), float("inf") if max_std is None else float(max_std), int(steps),
            ctypes.c_void_p(stream)))

    def plan_argmin_async(self, d_costs: int, d_actions: int, n_envs: int, K: int, iteration: int, merge: bool,
                          d_results: int, stream: Optional[int] = None) -> None:
        """bcmpc_plan_argmin_async: every environment's running best into ``d_results`` (n_envs records)."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_plan_argmin_async(
            self._h, vp(d_costs), vp(d_actions), int(n_envs), int(K), int(iteration), int(bool(merge)),
            vp(d_results), ctypes.c_void_p(stream)))

    def select_batch_async(self, d_costs: int, n_envs: int, K: int, index_base: int, n_elite: int, d_out: int,
                           d_count: int, stream: Optional[int] = None) -> None:
        """bcmpc_select_batch_async: ``d_out`` ``[n_envs, n_elite]`` elite records, ``d_count`` ``[n_envs]``."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_select_batch_async(
            self._h, vp(d_costs), int(n_envs), int(K), int(index_base), int(n_elite), vp(d_out), vp(d_count),
            ctypes.c_void_p(stream)))

    def cem_refit_batch_async(self, d_elite: int, d_count: int, n_envs: int, n_elite: int, seed: int, iteration: int,
                              alpha: float, d_mu: int, d_sigma: int, d_actions: Optional[int] = None, K: int = 0,
                              cand_offset: int = 0, stream: Optional[int] = None) -> None:
        """bcmpc_cem_refit_batch_async; ``d_actions`` (with ``K``, ``cand_offset``): read the iteration's
        stored samples instead of regenerating them."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_cem_refit_batch_async(
            self._h, vp(d_elite), vp(d_count), int(n_envs), int(n_elite), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), float(alpha), vp(d_mu), vp(d_sigma), vp(d_actions), int(K), int(cand_offset),
            ctypes.c_void_p(stream)))

    def mppi_update_batch_async(self, d_costs: int, n_envs: int, K: int, cand_offset: int, seed: int, iteration: int,
                                temperature: float, d_mu: int, d_sigma: int, d_stats: int,
                                d_actions: Optional[int] = None, stream: Optional[int] = None) -> None:
        """bcmpc_mppi_update_batch_async: mppi_update_async per environment at ``m = K``; ``d_stats`` holds
        ``n_envs`` MPPI_STATS records."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_mppi_update_batch_async(
            self._h, vp(d_costs), int(n_envs), int(K), int(cand_offset), ctypes.c_uint64(seed & (2**64 - 1)),
            int(iteration), float(temperature), vp(d_mu), vp(d_sigma), vp(d_stats), vp(d_actions),
            ctypes.c_void_p(stream)))

    def mppi_control_cost_async(self, d_costs: int, d_actions: int, n_envs: int, K: int, d_mu: int, d_sigma: int,
                                weight: float, d_scores: int, stream: Optional[int] = None) -> None:
        """bcmpc_mppi_control_cost_async: ``d_scores`` ``[n_envs*K]`` = the costs ``d_costs`` plus (a reward
        engine: minus) ``weight`` times the control cost of the stored actions ``d_actions`` ``[H, n_envs*K, A]``
        under the plans ``d_mu`` / ``d_sigma`` ``[n_envs, H, A]`` they were sampled from
        (mppi_update.control_cost / augmented)."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_mppi_control_cost_async(
            self._h, vp(d_costs), vp(d_actions), int(n_envs), int(K), vp(d_mu), vp(d_sigma), float(weight),
            vp(d_scores), ctypes.c_void_p(stream)))

    def mppi_sigma_update_async(self, d_scores: int, d_actions: int, n_envs: int, K: int, temperature: float,
                                d_mu_new: int, d_sigma: int, alpha: float = 0.0, min_std: float = 0.0,
                                max_std: Optional[float] = None, stream: Optional[int] = None) -> None:
        """bcmpc_mppi_sigma_update_async: ``d_sigma`` ``[n_envs, H, A]`` in place from the softmin weights of
        ``d_scores`` (the vector the update ran on) about the UPDATED plans ``d_mu_new``
        (mppi_update.weighted_sigma / sigma_step).  It relies on no scratch of an earlier call."""
        stream = self.stream if stream is None else stream
        vp = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
        _lib.check(self._lib.bcmpc_mppi_sigma_update_async(
            self._h, vp(d_scores), vp(d_actions), int(n_envs), int(K), float(temperature), vp(d_mu_new), vp(d_sigma),
            float(alpha), float(min_std), float("inf") if max_std is None else float(max_std),
            ctypes.c_void_p(stream)))

    def set_comm(self, comm) -> None:
        """Attach a ``distributed.LibraryComm`` (None detaches): every get_action of this engine then
        exchanges the ranks' result records over RCCL inside the library and returns the GLOBAL best
        (bcmpc_engine_set_comm)."""
        _lib.check(self._lib.bcmpc_engine_set_comm(self._h, comm.handle if comm is not None else None))
        self.comm = comm

    @property
    def stream(self) -> int:
        return int(self._lib.bcmpc_stream(self._h) or 0)

    def check_status(self) -> None:
        """After the stream of a stream-ordered launch (rollout_async, rollout_policy_async,
        cem_rollout_async) has completed: raise BcmpcError when a team-kernel launch of this engine
        gave up because its workgroups could not all be resident (its outputs are not valid);
        bcmpc_engine_status.  Synchronous calls rerun on a fallback engine instead."""
        _lib.check(self._lib.bcmpc_engine_status(self._h))

    @property
    def team_reruns(self) -> int:
        """Synchronous calls of this engine rerun on its fallback engine (bcmpc_engine_team_reruns)."""
        n = ctypes.c_uint64()
        _lib.check(self._lib.bcmpc_engine_team_reruns(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_timing(self, on: bool = True) -> None:
        """Bracket this engine's launches with HIP events (off by default: ~6 us per synchronous
        get_action at small K) so that last_kernel_ms() can read them (bcmpc_engine_set_timing)."""
        _lib.check(self._lib.bcmpc_engine_set_timing(self._h, 1 if on else 0))

    def last_kernel_ms(self) -> Tuple[float, float]:
        r, m = ctypes.c_float(), ctypes.c_float()
        _lib.check(self._lib.bcmpc_last_kernel_ms(self._h, ctypes.byref(r), ctypes.byref(m)))
        return float(r.value), float(m.value)

    def info(self) -> dict:
        hp, wb, wpb, kn = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self._lib.bcmpc_engine_info(self._h, ctypes.byref(hp), ctypes.byref(wb), ctypes.byref(wpb),
                                               ctypes.byref(kn)))
        names = {v: k for k, v in _lib.KERNELS.items()}
        buf = ctypes.create_string_buffer(160)
        _lib.check(self._lib.bcmpc_engine_layout(self._h, buf, len(buf)))
        return dict(hidden_padded=hp.value, packed_weight_bytes=wb.value, waves_per_block=wpb.value,
                    kernel=names.get(kn.value, str(kn.value)), layout=buf.value.decode())

    def close(self) -> None:
        # (the prepared ctypes arguments of the fast paths hold the handle: dropped with it, so a call after
        #  close() passes NULL and gets the library's clean error instead of a freed engine)
        self._ga_fast = None
        self._mt_fast = None
        if getattr(self, "_h", None):
            self.comm = None
            self._lib.bcmpc_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

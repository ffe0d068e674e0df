"""Model ensembles: the planners score every candidate under E dynamics nets.

A sampling planner that trusts one learned model picks exactly the candidates on which that model is
most wrong.  An ensemble of E bootstrapped nets rolls every candidate out under every member and combines
the members' costs -- by their mean, pessimistically by mean + kappa * std, or by the worst member --
before the argmin, CEM's elite selection or the MPPI weights see them.

* ``combine(costs[E, K], rule, kappa)`` IS the definition of the three rules (NumPy f64, one rounded
  operation per step); libbcmpc's ``ensemble_reduce_kernel`` computes the same bits on the device.
* ``EnsembleEngine`` owns one bcmpc_ensemble: E member engines of one configuration, all launches of a call
  on one stream (members in order, reduce, argmin / select + refit / MPPI update), one host synchronisation.
* ``EnsembleDynamicsModel`` holds E ``NNDynamicsModel`` members of one architecture and one normalisation,
  fitted on bootstrap resamples; ``MPCcontroller``, ``CEMcontroller`` and ``MPPIcontroller`` accept it as
  ``dyn_model`` and read its ``rule`` / ``kappa`` on every call.

Not covered: batched CEM / MPPI over ensembles, reward-model and policy-guided ensembles, candidate
sharding over ranks, per-step member switching (TS-1), members running concurrently.
"""
from __future__ import annotations

import ctypes
import math
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from . import distributed as _dist
from . import weights as _weights
from .controllers import (_batch_inputs_check, _batch_rng_check, _batch_states, _cached_engine, _device, _device_terms,
                          _send_cost_inputs, _shape)
from .cost_functions import is_cheetah_cost
from .engine import BatchResult, MLPSpec, RolloutEngine, StepResult, _dp, _engine_config, _EngineCalls, _f64

RULES = ("mean", "mean_std", "worst")
MAX_MEMBERS = _lib.MAX_MEMBERS


def combine(costs, rule: str = "mean", kappa: float = 0.0) -> np.ndarray:
    """The value of every candidate from its E member costs ``costs[E, ...]`` (reduced over axis 0):

    * ``"mean"``      ``t = c[0]; for e in 1..E-1: t = t + c[e]; v = t / E``
    * ``"mean_std"``  ``m`` as above; ``q = 0.0; for e in 0..E-1: d = c[e] - m; q = q + d*d``;
                      ``v = m + kappa * sqrt(q / E)`` (the population standard deviation about ``m``)
    * ``"worst"``     ``np.maximum.reduce(c)``: the largest member cost, NaN if any member's is NaN

    every operation one rounded IEEE f64 operation.  The mean starts from ``c[0]``, so ``E == 1`` returns
    ``c[0]`` bit for bit (``-0.0`` and NaN included)."""
    c = np.asarray(costs, dtype=np.float64)
    if c.ndim < 1 or c.shape[0] < 1:
        raise ValueError("costs must be [E, ...] with E >= 1")
    if rule not in RULES:
        raise ValueError(f"unknown ensemble rule {rule!r}; one of {RULES}")
    kappa = float(kappa)
    if not math.isfinite(kappa):
        raise ValueError("kappa must be finite")
    E = c.shape[0]
    with np.errstate(all="ignore"):
        if rule == "worst":
            return np.maximum.reduce(c, axis=0)
        t = c[0].copy()
        for e in range(1, E):
            t = t + c[e]
        n = np.float64(E)
        m = t / n
        if rule == "mean":
            return m
        q = np.zeros_like(m)
        for e in range(E):
            d = c[e] - m
            q = q + d * d
        return m + np.float64(kappa) * np.sqrt(q / n)


@dataclass
class EnsembleStepResult(StepResult):
    """``costs``: the values ``v`` ``[K]``; ``member_costs``: ``[E, K]``."""
    member_costs: Optional[np.ndarray] = None


@dataclass
class EnsembleBatchResult(BatchResult):
    """``costs``: ``[B, K]`` values; ``member_costs``: ``[E, B, K]``."""
    member_costs: Optional[np.ndarray] = None


class _Member(RolloutEngine):
    """Member i of an ensemble as a RolloutEngine view: the handle is lent by the bcmpc_ensemble (which owns
    it), so set_weights / set_cost_terms / set_action_bounds / info / team_reruns work as on any engine."""

    def __init__(self, owner: "EnsembleEngine", handle):  # noqa: D107  (no bcmpc_create: the handle is lent)
        self._lib = owner._lib
        self._h = handle
        for name in ("state_dim", "action_dim", "hidden", "n_layers", "activation", "layer_norm", "horizon",
                     "num_paths", "device", "cost", "precision"):
            setattr(self, name, getattr(owner, name))
        self.model, self.policy_hidden, self.policy_layers, self.policy_mode = "delta", 0, 0, "explore"
        self._fresh()

    def close(self) -> None:
        self._ga_fast = None
        self._mt_fast = None
        self._h = None


class EnsembleEngine(_EngineCalls):
    """Owns one bcmpc_ensemble: ``n_members`` engines of one configuration (hence one kernel layout) on one
    device.  The constructor arguments after ``n_members`` are RolloutEngine's (no policy, ``cost`` "cheetah"
    or "terms", the delta model); ``cem_get_action`` / ``mppi_get_action`` are RolloutEngine's too, on the
    ensemble's entry points."""
    _CEM, _MPPI = "bcmpc_ensemble_cem_get_action", "bcmpc_ensemble_mppi_get_action"
    _CEM_S = _MPPI_S = None             # (correlated noise and elite carry-over: single engines only)
    _MPPI_X = None                      # (MPPI's control cost and sigma update: single engines only)
    _CEM_P = _MPPI_P = None             # (proposals: single engines only)
    _CEM_K = _MPPI_K = None             # (knot plans: single engines only)

    def __init__(self, n_members: int, state_dim: int, action_dim: int, hidden: int, n_layers: int,
                 activation: str, layer_norm: bool, horizon: int, num_paths: int, device: int = 0,
                 cost: str = "cheetah", kernel: Optional[str] = None, precision: Optional[str] = None):
        self._lib = _lib.load()
        self._h = None
        cfg, precision, _ = _engine_config(state_dim, action_dim, hidden, n_layers, activation, layer_norm, horizon,
                                           num_paths, device, cost, kernel, 0, 0, "explore", "delta", precision)
        h = ctypes.c_void_p()
        _lib.check(self._lib.bcmpc_ensemble_create(ctypes.byref(cfg), ctypes.c_int32(int(n_members)),
                                                   ctypes.byref(h)))
        self._h = h
        self.n_members = int(n_members)
        self.state_dim, self.action_dim = state_dim, action_dim
        self.hidden, self.n_layers, self.activation = hidden, n_layers, activation
        self.layer_norm, self.horizon, self.num_paths = bool(layer_norm), horizon, num_paths
        self.device, self.cost, self.precision = device, cost, precision
        self.rule, self.kappa = "mean", 0.0
        self.members: List[_Member] = []
        for i in range(self.n_members):
            mh = ctypes.c_void_p()
            _lib.check(self._lib.bcmpc_ensemble_member(self._h, ctypes.c_int32(i), ctypes.byref(mh)))
            self.members.append(_Member(self, mh))

    # ------------------------------------------------------------------ configuration
    def set_weights(self, member: int, spec: MLPSpec, normalization: Sequence, version: int) -> None:
        """Member ``member``'s weights (RolloutEngine.set_weights; idempotent on ``version``)."""
        self.members[member].set_weights(spec, normalization, version)

    def set_cost_terms(self, term_cost) -> None:
        for m in self.members:
            m.set_cost_terms(term_cost)

    def set_cost_inputs(self, reference=None, previous_action=None) -> None:
        """Every member gets the same inputs (RolloutEngine.set_cost_inputs)."""
        for m in self.members:
            m.set_cost_inputs(reference, previous_action)

    def set_action_bounds(self, low, high) -> None:
        for m in self.members:
            m.set_action_bounds(low, high)

    def set_terminal_value(self, spec, weight: float = -1.0, version: int = 0) -> None:
        """RolloutEngine.set_terminal_value on every member: each adds the value of ITS final state to its row
        of the member costs before the reduce."""
        for m in self.members:
            m.set_terminal_value(spec, weight, version)

    @property
    def terminal_value(self):
        """(spec, weight, version) of the value the members hold, or None."""
        return self.members[0].terminal_value

    def set_rule(self, rule: str = "mean", kappa: float = 0.0) -> None:
        """The rule of the following calls (bcmpc_ensemble_set_rule); see ``combine``."""
        if rule not in _lib.ENSEMBLE_RULES:
            raise ValueError(f"unknown ensemble rule {rule!r}; one of {RULES}")
        if rule == self.rule and float(kappa) == self.kappa:
            return
        _lib.check(self._lib.bcmpc_ensemble_set_rule(self._h, ctypes.c_int32(_lib.ENSEMBLE_RULES[rule]),
                                                     ctypes.c_double(float(kappa))))
        self.rule, self.kappa = rule, float(kappa)

    # ------------------------------------------------------------------ calls
    def get_action(self, state, actions: Optional[np.ndarray] = None, seed: int = 0, cand_offset: int = 0,
                   return_costs: bool = False, return_member_costs: bool = False) -> EnsembleStepResult:
        """bcmpc_ensemble_get_action: every candidate scored by every member, the argmin over ``v``."""
        st = self._state(state)
        actions, act_p = self._actions(actions)
        res = _lib.Result()
        v = np.empty(self.num_paths, dtype=np.float64) if return_costs or return_member_costs else None
        mc = np.empty((self.n_members, self.num_paths), dtype=np.float64) if return_member_costs else None
        _lib.check(self._lib.bcmpc_ensemble_get_action(
            self._h, _dp(st), act_p, ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_int64(cand_offset),
            ctypes.byref(res), _dp(v) if v is not None else None, _dp(mc) if mc is not None else None))
        return EnsembleStepResult(int(res.best_index), float(res.best_cost),
                                  np.array(res.first_action[: self.action_dim], dtype=np.float64), v, mc)

    def get_actions(self, states, actions: Optional[np.ndarray] = None, seed: int = 0, cand_offset: int = 0,
                    return_costs: bool = False, return_member_costs: bool = False) -> EnsembleBatchResult:
        """bcmpc_ensemble_get_actions_batch: ``states`` ``[B, S]``, columns as RolloutEngine.get_actions."""
        st = _f64(states)
        if st.ndim != 2 or st.shape[1] != self.state_dim:
            raise ValueError(f"states shape {st.shape} != (B, S) = (B, {self.state_dim})")
        B = int(st.shape[0])
        if B < 1:
            raise ValueError("the batched step needs at least one environment")
        if self.num_paths % B != 0:
            raise ValueError(f"num_paths = {self.num_paths} is not a multiple of the {B} environments")
        actions, act_p = self._actions(actions)
        res = (_lib.Result * B)()
        v = np.empty(self.num_paths, dtype=np.float64) if return_costs or return_member_costs else None
        mc = np.empty((self.n_members, self.num_paths), dtype=np.float64) if return_member_costs else None
        _lib.check(self._lib.bcmpc_ensemble_get_actions_batch(
            self._h, _dp(st), ctypes.c_int32(B), act_p, ctypes.c_uint64(seed & (2**64 - 1)),
            ctypes.c_int64(cand_offset), res, _dp(v) if v is not None else None,
            _dp(mc) if mc is not None else None))
        rec = np.frombuffer(res, dtype=np.float64).reshape(B, 2 + _lib.MAX_ACTION)
        return EnsembleBatchResult(rec[:, 0].copy().view(np.int64), rec[:, 1].copy(),
                                   rec[:, 2:2 + self.action_dim].copy(),
                                   v.reshape(B, -1) if v is not None else None,
                                   mc.reshape(self.n_members, B, -1) if mc is not None else None)

    def reduce_async(self, d_member_costs: int, ld: int, n_members: int, K: int, rule: str, kappa: float,
                     d_out: int, stream: Optional[int] = None) -> None:
        """The reduce kernel alone on device pointers (bcmpc_ensemble_reduce_async), stream-ordered:
        ``d_member_costs`` ``[n_members, ld]`` f64 (``ld >= K``) -> ``d_out`` ``[K]``."""
        reduce_async(self.members[0], d_member_costs, ld, n_members, K, rule, kappa, d_out, stream)

    @property
    def stream(self) -> int:
        """The stream every launch of this ensemble goes on: member 0's."""
        return self.members[0].stream

    @property
    def team_reruns(self) -> int:
        """Calls rerun on the members' fallback engines (member 0's count: every member reruns together)."""
        return self.members[0].team_reruns

    def info(self) -> dict:
        out = self.members[0].info()
        out.update(n_members=self.n_members, rule=self.rule, kappa=self.kappa)
        return out

    def close(self) -> None:
        for m in getattr(self, "members", []):
            m.close()
        if getattr(self, "_h", None):
            self._lib.bcmpc_ensemble_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def reduce_async(engine: RolloutEngine, d_member_costs: int, ld: int, n_members: int, K: int, rule: str,
                 kappa: float, d_out: int, stream: Optional[int] = None) -> None:
    """bcmpc_ensemble_reduce_async on any engine's device (``engine`` only names the device)."""
    if rule not in _lib.ENSEMBLE_RULES:
        raise ValueError(f"unknown ensemble rule {rule!r}; one of {RULES}")
    stream = engine.stream if stream is None else stream
    _lib.check(engine._lib.bcmpc_ensemble_reduce_async(
        engine._h, ctypes.c_void_p(d_member_costs), ctypes.c_int64(ld), ctypes.c_int32(n_members),
        ctypes.c_int64(K), ctypes.c_int32(_lib.ENSEMBLE_RULES[rule]), ctypes.c_double(float(kappa)),
        ctypes.c_void_p(d_out), ctypes.c_void_p(stream)))


# ---------------------------------------------------------------------- the model
def member_rng(seed: int, member: int) -> random.Random:
    """Member ``member``'s private generator of an ensemble seeded with ``seed`` (bootstrap resamples and
    batch draws): a ``random.Random`` of its own, so fitting consumes neither the global ``random`` stream
    nor ``np.random``."""
    return random.Random(f"bc_mpc_amd.ensemble:{int(seed)}:{int(member)}")


def bootstrap_batches(rng: random.Random, size: int, batch_size: int, iterations: int) -> List[np.ndarray]:
    """One ``fit`` call's row indices for one member: a bootstrap resample ``boot = rng.choices(range(size),
    k=size)`` of the buffer, then ``iterations`` batches drawn from it as DataBufferGeneral.sample draws
    them (``fit.sample_batches`` on ``rng``), mapped through ``boot``."""
    from .fit import sample_batches
    boot = np.asarray(rng.choices(range(size), k=size), dtype=np.int64)
    return [boot[b] for b in sample_batches(size, batch_size, iterations, rng)]


class EnsembleDynamicsModel:
    """E ``NNDynamicsModel`` members of one architecture and one normalisation; member i is initialised from
    seed ``seed + i``.  ``rule`` / ``kappa`` (see ``combine``) are read by the controllers on every call and
    may be changed between calls.  ``diagnostics=True``: the controllers also fetch the member costs and
    expose the winner's (``last_member_costs``, ``last_disagreement``)."""

    is_ensemble = True

    def __init__(self, env, n_models, n_layers, size, activation, output_activation, normalization, batch_size,
                 iterations, learning_rate, *, layer_norm: bool = False, seed: int = 0, rule: str = "mean",
                 kappa: float = 0.0, diagnostics: bool = False, device: Optional[int] = None):
        from .dynamics import NNDynamicsModel
        n_models = int(n_models)
        if not 1 <= n_models <= MAX_MEMBERS:
            raise ValueError(f"n_models must be in [1, {MAX_MEMBERS}]")
        if rule not in RULES:
            raise ValueError(f"unknown ensemble rule {rule!r}; one of {RULES}")
        if not math.isfinite(float(kappa)):
            raise ValueError("kappa must be finite")
        self.env = env
        self.members = [NNDynamicsModel(env, n_layers, size, activation, output_activation, normalization,
                                        batch_size, iterations, learning_rate, layer_norm=layer_norm,
                                        seed=int(seed) + i, device=device) for i in range(n_models)]
        self.seed = int(seed)
        self.rule, self.kappa, self.diagnostics = rule, float(kappa), bool(diagnostics)
        self.batch_size, self.iterations, self.learning_rate = batch_size, iterations, learning_rate
        self.device = device
        self._rngs = [member_rng(self.seed, i) for i in range(n_models)]
        m0 = self.members[0]
        self.state_dim, self.action_dim = m0.state_dim, m0.action_dim
        self.n_layers, self.size, self.activation, self.layer_norm = m0.n_layers, m0.size, m0.activation, m0.layer_norm

    @property
    def n_models(self) -> int:
        return len(self.members)

    @property
    def version(self) -> int:
        """Changes whenever any member's weights change (the sum of the members' stamps, which only grow)."""
        return sum(int(m.version) for m in self.members)

    def load_weights(self, member: int, kernels: Sequence, biases: Sequence, ln_gamma: Optional[Sequence] = None,
                     ln_beta: Optional[Sequence] = None) -> None:
        self.members[member].load_weights(kernels, biases, ln_gamma, ln_beta)

    def normalization(self) -> List[np.ndarray]:
        return self.members[0].normalization()

    def predict_members(self, unnormalized_state, unnormalized_action) -> np.ndarray:
        """Every member's ``predict``: ``[E, K, S]`` f64."""
        return np.stack([m.predict(unnormalized_state, unnormalized_action) for m in self.members])

    def predict(self, unnormalized_state, unnormalized_action) -> np.ndarray:
        """The members' predictions combined element by element with the ``"mean"`` expression."""
        return combine(self.predict_members(unnormalized_state, unnormalized_action), "mean")

    def fit(self, data):
        """Every member fits its own bootstrap resample of ``data`` on its own persistent GPUFitter (the Adam
        slots persist across calls, like NNDynamicsModel.fit's): member i draws ``bootstrap_batches`` from
        its own generator (kept across calls).  Returns (mean of the members' last losses, 0)."""
        import torch
        from .fit import GPUFitter, buffer_arrays
        states, actions, deltas = buffer_arrays(data)
        size = int(getattr(data, "size", states.shape[0]))
        print("Model fitting for ", self.iterations, "times ... ")
        last = []
        for m, rng in zip(self.members, self._rngs):
            dev = m.device if m.device is not None else torch.cuda.current_device()
            if getattr(m, "_fitter", None) is None:
                m._fitter = GPUFitter(m.state_dim, m.action_dim, m.size, m.n_layers, m.activation, m.layer_norm,
                                      int(self.batch_size), float(self.learning_rate), dev)
                m._fit_version = None
            if m._fit_version != m.version:                 # weights changed outside fit: re-upload
                m._fitter.set_params(m.mlp_spec(), m.normalization())
            m._fitter.set_data(states, actions, deltas)
            losses = m._fitter.run(bootstrap_batches(rng, size, int(self.batch_size), int(self.iterations)))
            ks, bs, gs, bes = m._fitter.get_params()
            m.load_weights(ks, bs, gs if m.layer_norm else None, bes if m.layer_norm else None)
            m._fit_version = m.version
            if len(losses):
                last.append(float(losses[-1]))
        return (float(np.mean(last)) if last else None), 0


# ---------------------------------------------------------------------- the controllers' ensemble paths
def is_ensemble(dyn_model) -> bool:
    return bool(getattr(dyn_model, "is_ensemble", False))


def _ctrl_engine(ctrl, S: int, A: int, k_total: int, slot: str) -> EnsembleEngine:
    """The controller's EnsembleEngine for (shape, K) in ``ctrl._ens_engines[slot]`` (``controllers._cached_engine``);
    the members' weights, the cost terms and the model's rule are brought up to date on every call (each a no-op
    when unchanged)."""
    model = ctrl.dyn_model
    _, ws = _dist.world(ctrl._group)
    if ws > 1:
        raise NotImplementedError(f"{type(ctrl).__name__} with an EnsembleDynamicsModel runs on one rank "
                                  f"(world size {ws}): ensembles do not shard their candidates")
    terms = _device_terms(ctrl.cost_fn, S, A)
    if terms is None and not is_cheetah_cost(ctrl.cost_fn, S, A):
        raise ValueError(f"{type(ctrl).__name__} with an EnsembleDynamicsModel needs the cheetah cost_fn or a "
                         "TermCost (a host cost callable cannot be combined on the device)")
    specs = [_weights.extract(m) for m in model.members]
    spec = specs[0][0]
    if any(s[0].model != "delta" for s in specs):
        raise TypeError("EnsembleDynamicsModel members must be NNDynamicsModel nets (reward-model ensembles "
                        "are not covered)")
    eng = _cached_engine(ctrl, "_ens_engines", slot, len(specs), S, A, spec.hidden, spec.n_layers, spec.activation,
                         spec.layer_norm, int(ctrl.horizon), int(k_total), make=EnsembleEngine, device=_device(ctrl),
                         cost="cheetah" if terms is None else "terms")
    if terms is not None:
        eng.set_cost_terms(terms)
        _send_cost_inputs(ctrl, eng, terms)
    for i, (s, norm, version) in enumerate(specs):
        eng.set_weights(i, s, norm, version)
    eng.set_rule(model.rule, model.kappa)
    ctrl._apply_terminal_value(eng)
    return eng


def _diagnose(ctrl, member_costs, local_index) -> None:
    """``last_member_costs``: the winner's E member costs (``[E]``, batched ``[B, E]``); ``last_disagreement``:
    their population standard deviation."""
    if member_costs is None:
        ctrl.last_member_costs = ctrl.last_disagreement = None
        return
    if member_costs.ndim == 2:
        mc = member_costs[:, int(local_index)].copy()
        ctrl.last_member_costs, ctrl.last_disagreement = mc, float(np.std(mc))
    else:
        idx = np.asarray(local_index, dtype=np.int64)
        mc = np.stack([member_costs[:, b, idx[b]] for b in range(idx.shape[0])])
        ctrl.last_member_costs, ctrl.last_disagreement = mc, np.std(mc, axis=1)


def mpc_get_action(ctrl, state):
    """MPCcontroller.get_action on an EnsembleDynamicsModel.  ``rng="numpy"``: the reference's one
    ``np.random.uniform`` draw, made on the host and uploaded once as the explicit action array of every
    member; ``rng="device"``: Philox in the kernels, one seed per call."""
    S, A, K = _shape(ctrl)
    state = np.asarray(state, dtype=np.float64).reshape(-1)
    if K == 0:
        if ctrl.rng == "numpy":
            ctrl.sample_random_actions()
        else:
            ctrl._next_seed()
        raise ValueError("attempt to get argmin of an empty sequence")
    eng = _ctrl_engine(ctrl, S, A, K, "single")
    diag = bool(ctrl.dyn_model.diagnostics)
    action_paths, seed = None, 0
    if ctrl.rng == "numpy":
        action_paths = np.asarray(ctrl.sample_random_actions(), dtype=np.float64)
    else:
        seed = ctrl._next_seed()
    res = eng.get_action(state, action_paths, seed=seed, return_costs=ctrl.keep_costs, return_member_costs=diag)
    ctrl.last_costs = res.costs if ctrl.keep_costs else None
    ctrl.last_cost, ctrl.last_index = res.best_cost, res.best_index
    _diagnose(ctrl, res.member_costs, res.best_index)
    ctrl._note_terminal_value(eng, np.int64(res.best_index))
    if action_paths is not None:
        return action_paths[:, res.best_index, :][0].copy()
    return res.first_action


def mpc_get_actions(ctrl, states):
    """MPCcontroller.get_actions on an EnsembleDynamicsModel (``rng="device"``, one rank)."""
    _batch_rng_check(ctrl.rng)
    S, A, K = _shape(ctrl)
    states = _batch_states(states, S, ctrl._group)
    seed = ctrl._next_seed()
    if K == 0:
        raise ValueError("attempt to get argmin of an empty sequence")
    B = states.shape[0]
    _batch_inputs_check(ctrl, getattr(ctrl, "_inputs", (None, None)), B)
    eng = _ctrl_engine(ctrl, S, A, B * K, "batch")
    diag = bool(ctrl.dyn_model.diagnostics)
    res = eng.get_actions(states, None, seed=seed, return_costs=ctrl.keep_costs, return_member_costs=diag)
    ctrl.last_costs = res.costs if ctrl.keep_costs else None
    ctrl.last_cost, ctrl.last_index = res.best_cost, res.best_index
    _diagnose(ctrl, res.member_costs, res.best_index - np.arange(B) * K)
    ctrl._note_terminal_value(eng, np.asarray(res.best_index, dtype=np.int64))
    return res.first_action

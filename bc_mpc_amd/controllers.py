"""Drop-in controllers with the reference's API (controllers.py:6-88).

``MPCcontroller(env, dyn_model, horizon, cost_fn, num_simulated_paths, gamma)``
and ``get_action(state) -> np.ndarray (A,) float64`` keep the reference's
signatures so ``train_mpc_ppo.py:218-222`` / ``utils.py:202`` run unchanged.
The rollout itself -- state fan-out, H x dynamics MLP, cheetah cost, argmin --
runs in libbcmpc's HIP kernels (``bc_mpc_amd/csrc/rollout.hip``).

Action source (``rng=``):

* ``"numpy"`` (default, parity mode): exactly one
  ``np.random.uniform(low, high, size=[H, K, A])`` draw from the global legacy
  stream per call, as controllers.py:53 does, so a seeded driver
  (train_mpc_ppo.py:499) sees the same RNG side effects and the same actions.
  The returned action is ``action_paths[0, argmin, :].copy()`` of that array
  (controllers.py:84-85), bit-identical to the reference.
* ``"device"`` (perf mode): actions are drawn inside the kernel with
  Philox4x32-10 keyed by (seed, global candidate, step, draw); one 64-bit seed
  per call is taken from ``np.random`` (or from ``seed=`` if given).

Multi-GPU: when torch.distributed is initialised each rank owns a contiguous
slice of the K candidates (``distributed.shard_range``) and the ranks agree on
the argmin through one all-gather of (3 + A) doubles per step.

The siblings run on the same engine:

* ``MPCcontrollerPolicyNet`` (controllers.py:160-239): policy MLP fused into
  the rollout kernel;
* ``MPCcontrollerReward`` (controllers.py:90-158) and
  ``MPCcontrollerPolicyNetReward`` (controllers.py:289-363): the two-head
  ``NNDynamicsRewardModel`` net (dynamics.py:121-238) in the kernel, objective =
  argmax of the (discounted) predicted reward sum;
* ``MCTScontrollerPolicyNetReward`` (controllers.py:365-457): two engine
  launches per step (first-stage actions, then the policy-guided follow-up paths).
"""
from __future__ import annotations

import copy
import math
import os
from typing import Optional

import numpy as np

from . import _lib
from . import distributed as _dist
from . import knots as _knots
from . import policy as _policy
from . import proposals as _proposals
from . import sampling as _sampling
from . import value as _value
from . import weights as _weights
from .cost_functions import TermCost, is_cheetah_cost, trajectory_cost_fn
from .engine import RolloutEngine


class Controller():
    """controllers.py:6-12."""

    def __init__(self):
        pass

    def get_action(self, state):
        pass


class RandomController(Controller):
    """controllers.py:15-24 (uniform env.action_space.sample())."""

    def __init__(self, env):
        self.env = env

    def get_action(self, state):
        return self.env.action_space.sample()


def _stock(fn):
    """Mark a sample_random_actions body that is the reference's np.random.uniform draw verbatim:
    get_action may then make that same draw in the library (same values, same stream advance)."""
    fn._bcmpc_stock_sampler = True
    return fn


def _stock_sampler(obj) -> bool:
    return ("sample_random_actions" not in obj.__dict__
            and getattr(type(obj).sample_random_actions, "_bcmpc_stock_sampler", False))


def _default_device() -> int:
    if "LOCAL_RANK" in os.environ:
        return int(os.environ["LOCAL_RANK"])
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except Exception:  # pragma: no cover
        pass
    return 0


def _comm_device(ctrl) -> int:
    """The GPU of a controller's engine: the min-loc record goes through it under RCCL."""
    if ctrl._engine is not None:
        return ctrl._engine.device
    return _default_device() if ctrl._device is None else ctrl._device


def _attach_comm(ctrl, eng: RolloutEngine, fused: bool = True) -> RolloutEngine:
    """Under RCCL, give the engine the library's communicator (created once per controller, a
    collective on the first call every rank makes together): its get_action then returns the global
    best itself.  Only when every rank holds candidates (K >= world) and the cost is fused."""
    rank, ws = _dist.world(ctrl._group)
    want = fused and ws > 1 and int(ctrl.num_simulated_paths) >= ws and _dist.use_library_comm(ctrl._group)
    if want and getattr(eng, "comm", None) is None:
        if getattr(ctrl, "_comm", None) is None:
            ctrl._comm = _dist.LibraryComm(eng.device, ctrl._group)
        eng.set_comm(ctrl._comm)
    elif not want and getattr(eng, "comm", None) is not None:
        # (K fell below the world size: a rank may hold no candidates and must join the torch
        #  all-gather, so every rank's engine drops the communicator -- every rank decides alike)
        eng.set_comm(None)
    return eng


def _minloc(ctrl, eng, valid, cost, index, first, A):
    """The ranks' agreement on (cost, index, first action): already made inside the library when the
    engine that ran THIS step (``eng``: None when this rank launched nothing) has a communicator, else
    one torch all-gather of the records."""
    if valid and _dist.world(ctrl._group)[1] == 1:      # one rank: nothing to agree on
        return float(cost), int(index), np.array(first, dtype=np.float64)
    if eng is not None and getattr(eng, "comm", None) is not None:
        return float(cost), int(index), np.asarray(first, dtype=np.float64).copy()
    return _dist.allgather_minloc(valid, cost, index, first, A, ctrl._group, device=_comm_device(ctrl))


def _device_terms(cost_fn, S: int, A: int):
    """The ``TermCost`` a controller evaluates on the device (an engine of ``cost="terms"``), or None: the
    cheetah cost is fused into the rollout kernels, and any other callable stays on the host."""
    if isinstance(cost_fn, TermCost) and not is_cheetah_cost(cost_fn, S, A):
        return cost_fn
    return None


def _cost_inputs(ctrl, reference, previous_action, batch: bool):
    """A call's ``reference`` / ``previous_action`` checked against the controller's cost and brought to the
    engine's form -- ``(reference [B or 1, 1 or H, R] or None, previous_action [B or 1, A] or None)`` -- or
    ValueError.  Called first in ``get_action`` / ``get_actions``: before any seed or ``np.random`` draw and
    before an engine is built or touched.  The controllers do not remember their last action."""
    cost_fn = ctrl.cost_fn
    if reference is None and previous_action is None and not isinstance(cost_fn, TermCost):
        return None, None
    S, A, _ = _shape(ctrl)
    terms = _device_terms(cost_fn, S, A)
    n_ref = terms.n_ref if terms is not None else 0
    who, lead = type(ctrl).__name__, "[B, " if batch else "["
    ref = prev = None
    if reference is None:
        if n_ref:
            raise ValueError(f"{who}: the cost names reference channels (n_ref = {n_ref}): pass reference=")
    else:
        if not n_ref:
            raise ValueError(f"{who}: reference= needs a TermCost with ref(c) values; this cost names no channel")
        ref = np.asarray(reference, dtype=np.float64)
        H = int(ctrl.horizon)
        if ref.ndim not in ((2, 3) if batch else (1, 2)) or (ref.ndim == 2 + batch and ref.shape[-2] != H):
            raise ValueError(f"{who}: reference must be {lead}R] or {lead}H, R] with H = {H}, not {ref.shape}")
        if ref.shape[-1] < n_ref:
            raise ValueError(f"{who}: the reference has {ref.shape[-1]} channels, the cost names {n_ref}")
        ref = ref.reshape((ref.shape[0] if batch else 1, -1, ref.shape[-1]))
    if previous_action is not None:
        if terms is None or not terms.uses_rate:
            raise ValueError(f"{who}: previous_action= needs a TermCost with rate terms")
        prev = np.asarray(previous_action, dtype=np.float64)
        if prev.ndim != 1 + batch or prev.shape[-1] != A:
            raise ValueError(f"{who}: previous_action must be {lead}A] with A = {A}, not {prev.shape}")
        prev = prev.reshape(-1, A)
    return ref, prev


def _batch_inputs_check(ctrl, inputs, B: int) -> None:
    for name, x in zip(("reference", "previous_action"), inputs):
        if x is not None and x.shape[0] != B:
            raise ValueError(f"{type(ctrl).__name__}: {name} is for {x.shape[0]} environments, states for {B}")


def _send_cost_inputs(ctrl, eng, terms) -> None:
    """The call's inputs to an engine whose cost takes them (after ``set_cost_terms``; every member of an
    ensemble, every rank's shard engine)."""
    if terms is not None and terms.extended:
        eng.set_cost_inputs(*getattr(ctrl, "_inputs", (None, None)))


def _opt(terms) -> tuple:
    """The trailing ``terms`` argument of the ``_engine_for`` methods, passed only when there is one (a
    subclass or test double that replaces ``_engine_for`` with the earlier signature keeps working)."""
    return () if terms is None else (terms,)


def _batch_rng_check(rng: str) -> None:
    """get_actions draws in the kernel only: the host-stream modes promise ONE draw per get_action call
    in the reference's order, and a batch of environments in one launch cannot keep that order."""
    if rng != "device":
        raise ValueError(f"get_actions needs rng='device': rng={rng!r} promises one host-stream draw per "
                         "get_action call in the reference's order, which a batched step cannot keep")


def _batch_states(states, S: int, group) -> np.ndarray:
    states = np.ascontiguousarray(states, dtype=np.float64)
    if states.ndim != 2 or states.shape[1] != S or states.shape[0] < 1:
        raise ValueError(f"states shape {states.shape} != (B, S) = (B >= 1, {S})")
    if _dist.world(group)[1] != 1:
        raise ValueError("get_actions runs on a single rank (candidate sharding is not batched yet)")
    return states


def _shape(ctrl):
    """``(S, A, K)`` of a controller's problem; an empty horizon is refused as the reference's indexing
    refuses it (controllers.py:85 at H = 0)."""
    S = int(math.prod(ctrl.env.observation_space.shape))
    A = len(ctrl.env.action_space.high)
    K = int(ctrl.num_simulated_paths)
    if ctrl.horizon < 1:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    return S, A, K


def _device(ctrl) -> int:
    return _default_device() if ctrl._device is None else ctrl._device


def _bounds(ctrl):
    """The environment's action box as f64 vectors (what a new engine is given, and the planners' plans sit in)."""
    return (np.asarray(ctrl.env.action_space.low, dtype=np.float64),
            np.asarray(ctrl.env.action_space.high, dtype=np.float64))


def _cached_engine(ctrl, store: str, slot: str, *args, make=None, **kwargs):
    """The controllers' one engine cache: the engine in ``ctrl.<store>[slot]`` (kept there as ``(key, engine)``)
    for the constructor arguments ``args`` / ``kwargs``.  The arguments ARE the key: an engine is closed and
    built anew exactly when one of them differs from those it was built with, and a new engine gets the
    environment's action bounds.  ``make``: the engine class when it is not RolloutEngine.  What may change
    from call to call without a rebuild (weights, cost terms, discount, communicator, ensemble rule) is set by
    the caller after the lookup; each of those setters returns at once on a value the engine already has."""
    cache = ctrl.__dict__.setdefault(store, {})
    key = (args, kwargs)
    hit = cache.get(slot)
    if hit is None or hit[0] != key:
        if hit is not None:
            cache.pop(slot)[1].close()      # (popped first: a constructor that raises leaves no closed engine behind)
        eng = RolloutEngine(*args, **kwargs) if make is None else make(*args, **kwargs)
        eng.set_action_bounds(*_bounds(ctrl))
        cache[slot] = hit = (key, eng)
    return hit[1]


class _TerminalValue:
    """The controllers' ``terminal_value=`` / ``terminal_weight=`` (value.py): a container ``value.extract`` reads
    (or None), applied to the engine of every call after the cache lookup -- an idempotent setter, never a cache
    key, so a new weight or a new version of the net rebuilds no engine."""
    terminal_value = None
    terminal_weight = -1.0
    _tv_last = None             # (engine, local candidate indices or None) of the last call
    _ts_last = None             # the same for last_termination_step (a TermCost with done conditions)

    def _init_terminal_value(self, terminal_value, terminal_weight) -> None:
        self.terminal_value = terminal_value
        self.terminal_weight = _value.check_weight(terminal_weight)
        if terminal_value is not None:
            _value.extract(terminal_value)          # a container that cannot be read fails here, not mid-episode

    def _apply_terminal_value(self, eng) -> None:
        self._tv_last = self._ts_last = None
        if self.terminal_value is None:
            if getattr(eng, "terminal_value", None) is not None:    # (an engine that never held one is not asked)
                eng.set_terminal_value(None)
            return
        spec, version = _value.extract(self.terminal_value)
        if spec.state_dim != eng.state_dim:
            raise ValueError(f"terminal_value reads {spec.state_dim} state dims, the environment has {eng.state_dim}")
        eng.set_terminal_value(spec, _value.check_weight(self.terminal_weight), version)

    def _note_terminal_value(self, eng, local_indices) -> None:
        self._tv_last = (eng, local_indices) if self.terminal_value is not None else None
        terms = getattr(getattr(eng, "members", [eng])[0], "cost_terms", None)
        self._ts_last = (eng, local_indices) if terms is not None and terms.done_conditions else None

    @property
    def last_terminal_value(self):
        """Diagnostics: the winner's ``v`` (f32) of the last call -- a float, ``[B]`` for ``get_actions``,
        ``[E]`` (every member's value of its own final state) on an ensemble -- or None: no terminal value, or
        a CEM / MPPI winner from an iteration before the last (the engine keeps the last iteration's values)."""
        if self._tv_last is None or self._tv_last[1] is None:
            return None
        eng, idx = self._tv_last
        members = getattr(eng, "members", None)
        if members is not None:
            return np.array([m.last_terminal_values(idx)[0] for m in members], dtype=np.float32)
        v = eng.last_terminal_values(idx)
        return float(v[0]) if np.ndim(idx) == 0 else v

    @property
    def last_termination_step(self):
        """Diagnostics: the winner's terminating step ``t`` of the last call (``cost_functions.episode_cost``; the
        horizon: it never terminated) -- an int, ``[B]`` for ``get_actions``, ``[E]`` (every member on its own
        trajectory) on an ensemble -- or None: the cost is no ``TermCost`` with ``done`` conditions, or a CEM /
        MPPI winner from an iteration before the last (the same rule as ``last_terminal_value``)."""
        if self._ts_last is None or self._ts_last[1] is None:
            return None
        eng, idx = self._ts_last
        members = getattr(eng, "members", None)
        if members is not None:
            return np.array([m.last_termination_steps(idx)[0] for m in members], dtype=np.int32)
        t = eng.last_termination_steps(idx)
        return int(t[0]) if np.ndim(idx) == 0 else t


def _refuse_terminal_value(who: str, terminal_value) -> None:
    if terminal_value is not None:
        raise ValueError(f"{who} does not take a terminal_value: value nets over a fused policy, the reward "
                         "model or MCTS are not covered (MPCcontroller, CEMcontroller and MPPIcontroller are)")


class Planner(_TerminalValue, Controller):
    """What CEMcontroller (cem.py) and MPPIcontroller (mppi.py) share: a plan ``mu`` ``[H, A]`` refined over
    ``iterations`` rounds of sampling around it, warm-started from the previous call's plan; ``get_actions``
    keeps one plan per environment and the B*K-candidate engine next to ``get_action``'s own.  A subclass names
    itself (``_KIND``), adds its constructor arguments and runs its engine call in ``_solve`` / ``_solve_batch``,
    which publish the ``last_*`` attributes, store the plan and return the action(s)."""
    _KIND = None            # "CEM" | "MPPI": the refusals' wording
    # what is sampled (sampling.py): read on every call, never an engine constructor argument
    noise_rho = 0.0
    keep_elites = False
    # knot plans (knots.py): ``knots`` = M in [1, horizon] samples the plan at M knots and interpolates it
    # (``knot_interp``: "hold" | "linear" | "cubic"); None: off.  Read on every call, like noise_rho.  With knots
    # the plans -- last_mu, last_sigma, the warm start -- are in KNOT space, [M, A]; last_plan is the [H, A] view
    knots = None
    knot_interp = "linear"
    _plan_view = None       # what last_plan returns

    @property
    def last_plan(self):
        """``knots.expand_plan(last_mu)`` of the last call, ``[H, A]`` / ``[B, H, A]``; without knots it is
        ``last_mu``.  (A property: the instance's ``last_*`` attributes are what they were before knots.)"""
        return self._plan_view

    # proposals (proposals.py): a policy net rolled through the model gives every call's last candidates
    policy_prior = None
    policy_paths = 0
    policy_stochastic = True
    policy_explore = 0.0
    last_proposal_costs = None      # [P] / [B, P]: the final iteration's costs of the proposal columns
    last_best_from_proposal = None  # bool / [B] bool: the best sample's column is a proposal column

    def __init__(self, env, dyn_model, horizon, cost_fn, num_simulated_paths, gamma, iterations, init_std,
                 warm_start, seed, device, process_group, terminal_value=None, terminal_weight=-1.0, noise_rho=0.0,
                 keep_elites=False, policy_prior=None, policy_paths=0, policy_stochastic=True, policy_explore=0.0,
                 knots=None, knot_interp="linear"):
        self._init_terminal_value(terminal_value, terminal_weight)
        self._init_policy_prior(policy_prior, policy_paths, policy_stochastic, policy_explore)
        self.noise_rho = _sampling.check_rho(noise_rho)
        self.keep_elites = _sampling.check_keep_elites(keep_elites)
        self.knots = _knots.check_knots(knots, horizon)
        self.knot_interp = _knots.check_interp(knot_interp)
        self.env = env
        self.dyn_model = dyn_model
        self.horizon = horizon
        self.cost_fn = cost_fn
        self.num_simulated_paths = num_simulated_paths
        self.gamma = gamma
        if iterations < 1:
            raise ValueError("iterations must be >= 1")
        self.iterations = int(iterations)
        self.init_std = init_std
        self.warm_start = warm_start
        self._seed_rng = np.random.RandomState(seed)
        self._device = device
        self._group = process_group
        self._engine: Optional[RolloutEngine] = None
        self._batch_engine: Optional[RolloutEngine] = None
        self._mu = None         # [H, A] ([M, A] with knots): get_action's last plan
        self._bmu = None        # [B, H, A] ([B, M, A]): the last batched call's plans
        self._bkeep = None      # [B] bool: plan b is shifted and reused (False after reset([b]))
        self.last_mu = None
        self.last_cost = None
        self.last_position = None

    def reset(self, env_ids=None) -> None:
        """Forget the warm-start plan (call at episode boundaries).  ``env_ids``: forget only those
        environments' plans of ``get_actions`` (an episode boundary in one simulator of a batch)."""
        if env_ids is None:
            self._mu = None
        self._reset_plans(env_ids)

    def _reset_plans(self, env_ids) -> None:
        if env_ids is None:
            self._bmu = self._bkeep = None
        elif self._bmu is not None:
            self._bkeep[np.asarray(env_ids, dtype=np.int64).reshape(-1)] = False

    def _bounds(self):
        return _bounds(self)

    def _refuse_ranks(self, ws: int) -> None:
        """Called first thing on more than one rank: a planner that cannot shard its candidates raises here."""

    def _sharded(self, rank, ws, state, spec, norm, version, terms, mu0, sd0, seed, S, A, K):
        """get_action on ``ws`` > 1 ranks, after the checks and the draws of the one-rank call."""
        raise NotImplementedError(f"{self._KIND}controller runs on one rank (world size {ws})")

    def initial_distribution(self):
        """mu0: the previous plan shifted by one step with the box centre appended (warm start), or the box
        centre; sigma0: init_std, default (high - low) / 4."""
        low, high = self._bounds()
        H = int(self.horizon)
        mid = (low + high) / 2.0
        sd = np.full_like(low, self.init_std) if self.init_std is not None else (high - low) / 4.0
        kn = self._knot_args()
        if kn:              # a knot plan [M, A]: the previous plan's interpolant one step later (knots.shift_plan)
            M = kn["knots"]
            if self.warm_start and self._mu is not None and self._mu.shape == (M, low.shape[0]):
                mu = _knots.shift_plan(self._mu, H, kn["knot_interp"], mid)
            else:
                mu = np.tile(mid, (M, 1))
            return mu, np.tile(sd, (M, 1))
        if self.warm_start and self._mu is not None and self._mu.shape == (H, low.shape[0]):
            mu = np.vstack([self._mu[1:], mid[None]])
        else:
            mu = np.tile(mid, (H, 1))
        return mu, np.tile(sd, (H, 1))

    def batch_initial_distribution(self, n_envs: int):
        """``initial_distribution()`` per environment, ``[B, H, A]`` each: plan b of the last batched call
        shifted by one step with the box centre appended, or the box centre in every step where there is
        none (first call, after ``reset``, B changed, ``warm_start=False``)."""
        low, high = self._bounds()
        H, B = int(self.horizon), int(n_envs)
        mid = (low + high) / 2.0
        sd = np.full_like(low, self.init_std) if self.init_std is not None else (high - low) / 4.0
        kn = self._knot_args()
        if kn:              # knot plans [B, M, A], each shifted by knots.shift_plan
            M = kn["knots"]
            mu = np.tile(mid, (B, M, 1))
            if self.warm_start and self._bmu is not None and self._bmu.shape == mu.shape:
                for b in np.flatnonzero(self._bkeep):
                    mu[b] = _knots.shift_plan(self._bmu[b], H, kn["knot_interp"], mid)
            return mu, np.tile(sd, (B, M, 1))
        mu = np.tile(mid, (B, H, 1))
        if self.warm_start and self._bmu is not None and self._bmu.shape == mu.shape:
            mu[self._bkeep, :-1] = self._bmu[self._bkeep, 1:]
        return mu, np.tile(sd, (B, H, 1))

    def _store_plans(self, mu: np.ndarray) -> None:
        self._bmu = mu
        self._bkeep = np.ones(mu.shape[0], dtype=bool)

    def _plan_states(self, states, S: int) -> np.ndarray:
        _, ws = _dist.world(self._group)
        if ws > 1:
            raise NotImplementedError(f"{type(self).__name__}.get_actions runs on one rank (world size {ws}): "
                                      "the batched planners do not shard their candidates")
        states = np.ascontiguousarray(states, dtype=np.float64)
        if states.ndim != 2 or states.shape[1] != S or states.shape[0] < 1:
            raise ValueError(f"states shape {states.shape} != (B, S) = (B >= 1, {S})")
        return states

    def _note_planner_value(self, eng, position, K: int) -> None:
        """``last_terminal_value``'s source: the engine keeps its LAST iteration's values, so the winner's is
        there when its position ``iteration * K + candidate`` (batched: per environment) lies in that iteration."""
        pos = np.asarray(position, dtype=np.int64)
        last = (self.iterations - 1) * K
        if (pos < last).any():
            self._note_terminal_value(eng, None)
        elif pos.ndim == 0:
            self._note_terminal_value(eng, np.int64(pos - last))
        else:
            self._note_terminal_value(eng, pos - last + np.arange(pos.shape[0], dtype=np.int64) * K)

    def _next_seed(self) -> int:
        return int(self._seed_rng.randint(0, 2**62, dtype=np.int64))

    def _sampling_args(self) -> dict:
        """The engine calls' ``rho`` / ``keep_elites``, passed only when they differ from the defaults (the call
        at the defaults is the call it has always been, also on an engine double of the earlier signature)."""
        rho, keep = _sampling.check_rho(self.noise_rho), _sampling.check_keep_elites(self.keep_elites)
        kw = {}
        if rho != 0.0:
            kw["rho"] = rho
        if keep:
            kw["keep_elites"] = True
        return kw

    def _refuse_sampling(self, where: str) -> None:
        """Correlated noise and elite carry-over run on one engine of one rank; raised before a seed is drawn."""
        if self._sampling_args():
            raise NotImplementedError(f"{self._KIND}controller: noise_rho / keep_elites are not built {where}")

    # ------------------------------------------------------------------ knot plans (knots.py)
    def _knot_args(self) -> dict:
        """The engine calls' ``knots`` / ``knot_interp``, passed only with knots on (the call with ``knots=None`` is
        the call it has always been); ValueError for a count outside ``[1, horizon]`` or an unknown kind."""
        M, kind = _knots.check_knots(self.knots, self.horizon), _knots.check_interp(self.knot_interp)
        return {} if M is None else {"knots": M, "knot_interp": kind}

    def _refuse_knots(self, where: str) -> None:
        """Knot plans run on one engine of one rank, without proposals; raised before a seed is drawn."""
        if self._knot_args():
            raise NotImplementedError(f"{self._KIND}controller: knots are not built {where}")

    def _publish_plan(self) -> None:
        """``last_plan``: the ``[H, A]`` / ``[B, H, A]`` view of ``last_mu`` (with knots: its expansion, clipped)."""
        kn = self._knot_args()
        mu = self.last_mu
        if not kn or mu is None:
            self._plan_view = mu
            return
        low, high = self._bounds()
        one = lambda m: _knots.expand_plan(m, int(self.horizon), kn["knot_interp"], low, high)   # noqa: E731
        self._plan_view = one(mu) if np.ndim(mu) == 2 else np.stack([one(m) for m in mu])

    # ------------------------------------------------------------------ proposals (proposals.py)
    def _init_policy_prior(self, policy_prior, policy_paths, policy_stochastic, policy_explore) -> None:
        paths, explore = int(policy_paths), float(policy_explore)
        if policy_prior is None and paths != 0:
            raise ValueError(f"policy_paths = {policy_paths!r} needs a policy_prior")
        if policy_prior is not None and paths < 1:
            raise ValueError(f"policy_prior needs policy_paths >= 1, got {policy_paths!r}")
        if not (math.isfinite(explore) and 0.0 <= explore <= 1.0):
            raise ValueError(f"policy_explore must be in [0, 1], got {policy_explore!r}")
        if policy_prior is not None:
            _policy.extract(policy_prior)               # a container that cannot be read fails here, not mid-episode
        self.policy_prior, self.policy_paths = policy_prior, paths
        self.policy_stochastic, self.policy_explore = bool(policy_stochastic), explore

    def _user_proposals(self, proposals, A: int, n_envs):
        """A call's ``proposals=`` as ``[P, H, A]`` / ``[B, P, H, A]`` f64 or None; ValueError before anything is drawn."""
        if proposals is None:
            return None
        return _proposals.as_sequences(proposals, int(self.horizon), A, n_envs)

    def _forget_proposal_report(self) -> None:
        """``last_proposal_costs`` / ``last_best_from_proposal`` of an earlier call (a controller that never carried
        proposals keeps the class's None and gains no attribute)."""
        if "last_proposal_costs" in self.__dict__:
            self.last_proposal_costs = self.last_best_from_proposal = None

    def _refuse_proposals(self, user, where: str) -> None:
        """Proposals run on one engine of one rank; raised before a seed is drawn."""
        if user is not None or self.policy_prior is not None:
            raise NotImplementedError(f"{self._KIND}controller: proposals= / policy_prior are not built {where}")

    def _prior_engine(self, slot: str, spec, norm, version, S: int, A: int, n_envs: int, user, K: int, kernel=None):
        """The checks of a call's proposals against its K candidates and, with a ``policy_prior``, the engine that
        rolls the policy through the model: a second engine in a slot of its own with ``n_envs * policy_paths``
        candidates, under the policy engines' limits (a prior outside them is refused here with the engine's
        message).  Everything here happens before a seed is drawn.  Returns the engine or None."""
        n_user = 0 if user is None else user.shape[-3]
        prior = self.policy_prior is not None
        if not n_user and not prior:
            return None
        carried = min(int(self.n_elite), K) if _sampling.check_keep_elites(self.keep_elites) else 0
        _proposals.check_count(n_user + (int(self.policy_paths) if prior else 0), K, carried)
        if not prior:
            return None
        if spec.model == "reward":
            raise ValueError(f"{self._KIND}controller: policy_prior over a learned-reward dyn_model is not covered "
                             "(proposals= is)")
        pspec, pversion = _policy.extract(self.policy_prior)
        extra = {} if kernel is None else dict(kernel=kernel[0], precision=kernel[1])
        # (cost="cheetah": policy engines need a fused cost; its values are ignored)
        eng = _cached_engine(self, "_engines", slot, S, A, spec.hidden, spec.n_layers, spec.activation,
                             spec.layer_norm, int(self.horizon), n_envs * int(self.policy_paths), device=_device(self),
                             cost="cheetah", model=spec.model, policy_hidden=pspec.hidden,
                             policy_layers=pspec.n_layers,
                             policy_mode="stochastic" if self.policy_stochastic else "explore", **extra)
        eng.set_weights(spec, norm, version)
        eng.set_policy(pspec, float(self.policy_explore), pversion)
        return eng

    def _prior_fallback(self, slot: str, spec, norm, version, S: int, A: int, n_envs: int, user, K: int):
        """The prior on a kernel that needs no resident team (what a synchronous call's rerun runs on): the split slab
        kernel, or the fp32 group kernel where the net is in split precision on the team kernel only."""
        try:
            return self._prior_engine(slot + "_fb", spec, norm, version, S, A, n_envs, user, K, ("split2", "split"))
        except ValueError:
            return self._prior_engine(slot + "_fb", spec, norm, version, S, A, n_envs, user, K, ("group4", "fp32"))

    def _prior_rollout(self, peng, eng, states, user, pseed: int):
        """The prior block: ``policy_paths`` closed-loop policy rollouts per state on ``peng``, on the planning
        engine's stream, into a torch device buffer -- handed on as device proposals in the policy engines' output
        layout.  A user's proposals come first, the policy's follow."""
        import torch
        from .engine import DeviceProposals
        dev = torch.device("cuda", eng.device)
        B, Pp, H, A = states.shape[0], int(self.policy_paths), int(self.horizon), peng.action_dim
        f64 = dict(dtype=torch.float64, device=dev)
        with torch.cuda.stream(torch.cuda.ExternalStream(eng.stream, device=dev)):
            d_states = torch.from_numpy(np.array(states, copy=True)).to(dev)      # (a copy: states may be read-only)
            d_out = torch.empty((H, B * Pp, A), **f64)
            d_costs = torch.empty(B * Pp, **f64)
            peng.rollout_policy_batch_async(d_states.data_ptr(), B, None, pseed, 0, d_costs.data_ptr(), None,
                                            d_out.data_ptr(), eng.stream)
            if user is None:
                return DeviceProposals(d_out.data_ptr(), Pp, *_proposals.policy_strides(B, Pp, A),
                                       keep=(d_states, d_out, d_costs))
            Pu = user.shape[1]
            d_all = torch.empty((H, B, Pu + Pp, A), **f64)
            d_all[:, :, :Pu] = torch.from_numpy(np.array(user, copy=True)).to(dev).permute(2, 0, 1, 3)
            d_all[:, :, Pu:] = d_out.view(H, B, Pp, A)
        return DeviceProposals(d_all.data_ptr(), Pu + Pp, *_proposals.policy_strides(B, Pu + Pp, A),
                               keep=(d_states, d_out, d_costs, d_all))

    def _with_proposals(self, eng, states, mu0, sd0, seed, K, user, peng, prior_args):
        """A call with proposals: the prior block (a second draw from the seed stream, made only with a prior), then
        the batched engine call -- ``get_action`` is its ``B = 1`` form, which equals the single call bit for bit and
        also returns the costs.  A team-kernel prior that gave up is never used: the call is answered again with
        the prior on its fallback kernel.  Returns ``_call_proposals``' tuple."""
        src = user
        if peng is not None:
            pseed = self._next_seed()
            src = self._prior_rollout(peng, eng, states, user, pseed)
        out = self._call_proposals(eng, states, mu0, sd0, seed, src)
        if peng is not None:
            try:
                peng.check_status()
            except _lib.BcmpcError:
                fb = self._prior_fallback(*prior_args)
                out = self._call_proposals(eng, states, mu0, sd0, seed, self._prior_rollout(fb, eng, states, user, pseed))
                fb.check_status()
        P = (0 if user is None else user.shape[1]) + (int(self.policy_paths) if peng is not None else 0)
        res = out[0]
        self.last_proposal_costs = res.costs[-1][:, K - P:].copy()
        self.last_best_from_proposal = (np.asarray(res.best_index) % K) >= K - P
        return out

    def _model(self, S: int, A: int):
        """(spec, normalisation, version, the TermCost scored on the device or None) of a supported pair of
        model and cost: the learned reward of a reward model, else the fused cheetah cost or a TermCost."""
        spec, norm, version = _weights.extract(self.dyn_model)
        terms = None
        if spec.model != "reward":
            _check_model(spec, "delta", type(self).__name__)
            terms = _device_terms(self.cost_fn, S, A)
            if terms is None and not is_cheetah_cost(self.cost_fn, S, A):
                raise ValueError(f"{self._KIND}controller needs the fused cheetah cost_fn or a learned-reward "
                                 "dyn_model")
        return spec, norm, version, terms

    def _cached(self, slot: str, spec, S, A, k, terms) -> RolloutEngine:
        reward = spec.model == "reward"
        eng = _cached_engine(self, "_engines", slot, S, A, spec.hidden, spec.n_layers, spec.activation,
                             spec.layer_norm, int(self.horizon), int(k), device=_device(self),
                             cost="reward" if reward else "terms" if terms is not None else "cheetah",
                             model=spec.model)
        if terms is not None:
            eng.set_cost_terms(terms)
            _send_cost_inputs(self, eng, terms)
        if reward:
            eng.set_discount(float(self.gamma))
        if reward and self.terminal_value is not None:
            raise ValueError(f"{self._KIND}controller: terminal_value over a learned-reward dyn_model is not covered")
        self._apply_terminal_value(eng)
        return eng

    def _engine_for(self, spec, S, A, k_local, terms=None) -> RolloutEngine:
        self._engine = self._cached("single", spec, S, A, k_local, terms)
        return self._engine

    def _batch_engine_for(self, spec, S: int, A: int, k_total: int, terms=None) -> RolloutEngine:
        self._batch_engine = self._cached("batch", spec, S, A, k_total, terms)
        return self._batch_engine

    def get_action(self, state, reference=None, previous_action=None, proposals=None):
        """``reference`` (``[R]`` or ``[H, R]``) and ``previous_action`` (``[A]``): the inputs of a ``TermCost``
        with ``ref(c)`` values / ``rate`` terms (cost_functions.py), explicit on every call.  ``proposals``
        (``[P, H, A]``): action sequences that sit, clipped to the box, in the last P candidates of every
        iteration (proposals.py); with a ``policy_prior`` the policy's ``policy_paths`` rollouts follow them.
        With ``knots`` the plan is sampled at M knots (knots.py): ``last_mu`` / ``last_sigma`` are ``[M, A]`` and
        ``last_plan`` is the ``[H, A]`` sequence they expand to."""
        action = self._get_action(state, reference, previous_action, proposals)
        self._publish_plan()
        return action

    def _get_action(self, state, reference, previous_action, proposals):
        self._inputs = _cost_inputs(self, reference, previous_action, False)
        S, A, K = _shape(self)
        if K == 0:
            raise ValueError("attempt to get argmin of an empty sequence")
        user = self._user_proposals(proposals, A, None)
        self._forget_proposal_report()
        if self._knot_args():
            self._refuse_proposals(user, "together with knots (a given sequence has no knot representation)")
        if getattr(self.dyn_model, "is_ensemble", False):
            # an EnsembleDynamicsModel (ensemble.py): its engine has RolloutEngine's planner calls, scored on the
            # members' combined value; it refuses ranks, costs and members itself, before anything is drawn
            from . import ensemble as _ensemble
            self._refuse_sampling("over an EnsembleDynamicsModel")
            self._refuse_knots("over an EnsembleDynamicsModel")
            self._refuse_proposals(user, "over an EnsembleDynamicsModel")
            state = np.asarray(state, dtype=np.float64).reshape(-1)
            eng = _ensemble._ctrl_engine(self, S, A, K, "single")
            mu0, sd0 = self.initial_distribution()
            return self._solve(eng, state, mu0, sd0, self._next_seed(), K)
        rank, ws = _dist.world(self._group)
        if ws > 1:
            self._refuse_ranks(ws)
            self._refuse_sampling(f"for more than one rank (world size {ws})")
            self._refuse_knots(f"for more than one rank (world size {ws})")
            self._refuse_proposals(user, f"for more than one rank (world size {ws})")
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        spec, norm, version, terms = self._model(S, A)
        prior_args = ("prior", spec, norm, version, S, A, 1, user, K)
        peng = self._prior_engine(*prior_args)
        mu0, sd0 = self.initial_distribution()
        seed = self._next_seed()
        if ws > 1:
            return self._sharded(rank, ws, state, spec, norm, version, terms, mu0, sd0, seed, S, A, K)
        eng = self._engine_for(spec, S, A, K, *_opt(terms))
        eng.set_weights(spec, norm, version)
        if user is None and peng is None:
            return self._solve(eng, state, mu0, sd0, seed, K)
        out = self._with_proposals(eng, state[None], mu0[None], sd0[None], seed, K,
                                   None if user is None else user[None], peng, prior_args)
        self.last_proposal_costs = self.last_proposal_costs[0]
        self.last_best_from_proposal = bool(self.last_best_from_proposal[0])
        return self._publish_proposals(eng, out, K, True)

    def get_actions(self, states, reference=None, previous_action=None, proposals=None):
        """Batched control step: ``states`` is ``[B, S]``, one independent answer per row with
        ``num_simulated_paths`` candidates each, all environments in one launch chain.  Every environment
        keeps its own warm-start plan (see ``reset``); one seed is drawn per call.  Returns ``[B, A]``
        float64; ``last_mu`` is ``[B, H, A]`` and the other ``last_*`` hold one entry per environment.  One
        rank only.  ``reference`` (``[B, R]`` or ``[B, H, R]``) and ``previous_action`` (``[B, A]``): every
        environment's inputs of a ``TermCost`` with ``ref(c)`` values / ``rate`` terms.  ``proposals``
        (``[B, P, H, A]``): every environment's own sequences, as in ``get_action``; a ``policy_prior`` is rolled
        out from every environment's state (``B * policy_paths`` rollouts in one launch).  With ``knots``:
        ``last_mu`` ``[B, M, A]``, ``last_plan`` ``[B, H, A]``."""
        actions = self._get_actions(states, reference, previous_action, proposals)
        self._publish_plan()
        return actions

    def _get_actions(self, states, reference, previous_action, proposals):
        if getattr(self.dyn_model, "is_ensemble", False):
            raise NotImplementedError(f"batched {self._KIND} over an EnsembleDynamicsModel is not built yet: "
                                      "use get_action")
        self._inputs = _cost_inputs(self, reference, previous_action, True)
        S, A, K = _shape(self)
        states = self._plan_states(states, S)
        _batch_inputs_check(self, self._inputs, states.shape[0])
        if K == 0:
            raise ValueError("attempt to get argmin of an empty sequence")
        B = states.shape[0]
        user = self._user_proposals(proposals, A, B)
        self._forget_proposal_report()
        if self._knot_args():
            self._refuse_proposals(user, "together with knots (a given sequence has no knot representation)")
        spec, norm, version, terms = self._model(S, A)
        prior_args = ("prior_batch", spec, norm, version, S, A, B, user, K)
        peng = self._prior_engine(*prior_args)
        mu0, sd0 = self.batch_initial_distribution(B)
        seed = self._next_seed()
        eng = self._batch_engine_for(spec, S, A, B * K, *_opt(terms))
        eng.set_weights(spec, norm, version)
        if user is None and peng is None:
            return self._solve_batch(eng, states, mu0, sd0, seed, K)
        return self._publish_proposals(eng, self._with_proposals(eng, states, mu0, sd0, seed, K, user, peng, prior_args),
                                       K, False)


class MPCcontroller(_TerminalValue, Controller):
    """Random-shooting MPC (controllers.py:26-88) on the MI355X rollout engine.  ``terminal_value`` (a container
    ``value.extract`` reads) and ``terminal_weight`` add ``weight * V(s_H)`` to every candidate's cost on the
    device (value.py); with it ``rng="numpy"`` draws on the host and uploads the array."""

    def __init__(self,
                 env,
                 dyn_model,
                 horizon=5,
                 cost_fn=None,
                 num_simulated_paths=10,
                 gamma=1.,
                 *,
                 rng: str = "numpy",
                 seed: Optional[int] = None,
                 device: Optional[int] = None,
                 process_group=None,
                 terminal_value=None,
                 terminal_weight: float = -1.0):
        self._init_terminal_value(terminal_value, terminal_weight)
        self.env = env
        self.dyn_model = dyn_model
        self.horizon = horizon
        self.cost_fn = cost_fn
        self.num_simulated_paths = num_simulated_paths
        self.gamma = gamma                      # stored, unused (as in the reference)
        if rng not in ("numpy", "device"):
            raise ValueError("rng must be 'numpy' or 'device'")
        self.rng = rng
        self._seed_rng = np.random.RandomState(seed) if seed is not None else None
        self._device = device
        self._group = process_group
        self._engine: Optional[RolloutEngine] = None
        self._fast = None                       # get_action's repeat-call fast path (see there)
        # diagnostics of the last call (not part of the reference API)
        self.last_cost = None
        self.last_index = None
        self.last_costs = None
        self.keep_costs = False

    # controllers.py:43-55
    @_stock
    def sample_random_actions(self):
        np_action_paths = np.random.uniform(low=self.env.action_space.low, high=self.env.action_space.high,
                                            size=[self.horizon, self.num_simulated_paths,
                                                  len(self.env.action_space.high)])
        return np_action_paths

    # ------------------------------------------------------------------ engine
    def _cached(self, slot: str, spec, S, A, k, cost: str, terms) -> RolloutEngine:
        eng = _cached_engine(self, "_engines", slot, S, A, spec.hidden, spec.n_layers, spec.activation,
                             spec.layer_norm, int(self.horizon), int(k), device=_device(self), cost=cost)
        if terms is not None:
            eng.set_cost_terms(terms)
            _send_cost_inputs(self, eng, terms)
        return eng

    def _engine_for(self, spec, S, A, k_local, fused, terms=None) -> RolloutEngine:
        self._engine = self._cached("single", spec, S, A, k_local,
                                    "cheetah" if fused else "terms" if terms is not None else "none", terms)
        # (a value engine exchanges no records inside the library: the ranks agree through the torch all-gather)
        eng = _attach_comm(self, self._engine, fused and self.terminal_value is None)
        if fused or terms is not None:
            self._apply_terminal_value(eng)
        return eng

    def _next_seed(self) -> int:
        src = self._seed_rng if self._seed_rng is not None else np.random
        return int(src.randint(0, 2**62, dtype=np.int64))

    # controllers.py:57-88
    def get_action(self, state, reference=None, previous_action=None):
        """``reference`` (``[R]`` or ``[H, R]``) and ``previous_action`` (``[A]``): the inputs of a ``TermCost``
        with ``ref(c)`` values / ``rate`` terms (cost_functions.py), explicit on every call."""
        self._inputs = _cost_inputs(self, reference, previous_action, False)
        if getattr(self.dyn_model, "is_ensemble", False):   # an EnsembleDynamicsModel (ensemble.py)
            from . import ensemble as _ensemble
            return _ensemble.mpc_get_action(self, state)
        fp = getattr(self, "_fast", None)
        if fp is not None:
            # the per-env-step repeat (utils.py:202): same env / model / cost / shape as the last call, the
            # model's weights version and normalisation objects unchanged, one rank -- the checks below
            # were all made by that call, so only the NumPy-stream launch remains
            if (fp[0] == (self.env, self.dyn_model, self.cost_fn, self.horizon, self.num_simulated_paths, self.rng,
                          self.keep_costs) and _weights.same_token(self.dyn_model, fp[1])
                    and self.terminal_value is None
                    and "sample_random_actions" not in self.__dict__ and _dist.world(self._group)[1] == 1):
                space = self.env.action_space
                res = fp[2].get_action_numpy_stream(state, space.low, space.high, fp[3])
                if res is not None:
                    self.last_costs = None
                    self.last_cost, self.last_index = res.best_cost, res.best_index
                    return res.first_action
            self._fast = None
        S, A, K = _shape(self)
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        rank, ws = _dist.world(self._group)
        lo, hi = _dist.shard_range(K, rank, ws)
        spec, norm, version = _weights.extract(self.dyn_model)
        if spec.model != "delta":
            raise TypeError("MPCcontroller needs an NNDynamicsModel: NNDynamicsRewardModel.predict returns "
                            "(next_state, reward) (dynamics.py:238); use MPCcontrollerReward")
        fused = is_cheetah_cost(self.cost_fn, S, A)
        terms = _device_terms(self.cost_fn, S, A)          # a TermCost is scored on the device, either rng
        if not fused and terms is None and self.rng != "numpy":
            raise ValueError("a non-cheetah cost_fn needs rng='numpy' (actions must exist on the host)")
        if self.terminal_value is not None and not fused and terms is None:
            raise ValueError("terminal_value needs a cost the device scores (the cheetah cost_fn or a TermCost): "
                             "a host cost callable cannot be combined with it on the device")

        if K == 0:                                          # (the reference draws before failing)
            if self.rng == "numpy":
                self.sample_random_actions()
            else:
                self._next_seed()
            raise ValueError("attempt to get argmin of an empty sequence")
        # the reference's draw, made by the library straight into pinned memory and uploaded step
        # by step (same values, same stream advance) unless sample_random_actions is overridden
        if self.rng == "numpy" and fused and hi > lo and _stock_sampler(self) and self.terminal_value is None:
            eng = self._engine_for(spec, S, A, hi - lo, fused)
            eng.set_weights(spec, norm, version)
            res = eng.get_action_numpy_stream(state, self.env.action_space.low, self.env.action_space.high, K, lo,
                                              return_costs=self.keep_costs)
            if res is not None:
                self.last_costs = res.costs
                cost, index, first_g = _minloc(self, eng, True, res.best_cost, res.best_index, res.first_action, A)
                self.last_cost, self.last_index = cost, index
                tok = _weights.weight_token(self.dyn_model)
                if ws == 1 and not self.keep_costs and tok is not None and eng.comm is None:
                    self._fast = ((self.env, self.dyn_model, self.cost_fn, self.horizon, self.num_simulated_paths,
                                   self.rng, self.keep_costs), tok, eng, K)
                return first_g                               # = action_paths[0, index] (controllers.py:84-85)

        action_paths = None
        seed = 0
        if self.rng == "numpy":
            action_paths = self.sample_random_actions()      # every rank draws the full [H, K, A]
        else:
            seed = self._next_seed()

        valid, cost, index, first = False, float("inf"), -1, None
        if hi > lo:
            eng = self._engine_for(spec, S, A, hi - lo, fused, *_opt(terms))
            eng.set_weights(spec, norm, version)            # no-op unless the version changed
            local = None if action_paths is None else np.ascontiguousarray(action_paths[:, lo:hi, :])
            if fused or terms is not None:
                res = eng.get_action(state, local, seed=seed, cand_offset=lo, return_costs=self.keep_costs)
                valid, cost, index, first = True, res.best_cost, res.best_index, res.first_action
                self.last_costs = res.costs
                self._note_terminal_value(eng, np.int64(res.best_index - lo))
            else:
                costs = self._trajectory_costs(eng, state, local)
                i = int(np.argmin(costs))
                valid, cost, index, first = True, float(costs[i]), lo + i, local[0, i, :].copy()
                self.last_costs = costs

        cost, index, first_g = _minloc(self, self._engine if valid else None, valid, cost, index, first, A)
        self.last_cost, self.last_index = cost, index
        if not (valid and lo <= index < hi):
            self._tv_last = self._ts_last = None            # (another rank's candidate won)
        if action_paths is not None:
            opt_action_path = action_paths[:, index, :]     # controllers.py:84-85
            return opt_action_path[0].copy()
        return first_g

    def get_actions(self, states, reference=None, previous_action=None):
        """Batched control step (not in the reference): ``states`` is ``[B, S]``, one independent
        random-shooting answer per row with ``num_simulated_paths`` candidates each, all rolled out in one
        launch chain (``RolloutEngine.get_actions``).  Returns ``[B, A]`` float64.  Row ``b`` is what
        ``get_action(states[b])`` returns on the Philox candidates ``b*K .. (b+1)*K`` of the call's seed
        (one seed is drawn per call, as ``get_action`` draws one).  ``rng="device"`` on one rank with the
        fused cheetah cost or a ``TermCost`` only.  ``reference`` (``[B, R]`` or ``[B, H, R]``) and
        ``previous_action`` (``[B, A]``): every environment's inputs of a ``TermCost`` with ``ref(c)`` values /
        ``rate`` terms."""
        self._inputs = _cost_inputs(self, reference, previous_action, True)
        if getattr(self.dyn_model, "is_ensemble", False):
            from . import ensemble as _ensemble
            return _ensemble.mpc_get_actions(self, states)
        _batch_rng_check(self.rng)
        S, A, K = _shape(self)
        states = _batch_states(states, S, self._group)
        _batch_inputs_check(self, self._inputs, states.shape[0])
        spec, norm, version = _weights.extract(self.dyn_model)
        if spec.model != "delta":
            raise TypeError("MPCcontroller needs an NNDynamicsModel; use MPCcontrollerReward")
        terms = _device_terms(self.cost_fn, S, A)
        if terms is None and not is_cheetah_cost(self.cost_fn, S, A):
            raise ValueError("get_actions needs the fused cheetah cost_fn")
        seed = self._next_seed()
        if K == 0:
            raise ValueError("attempt to get argmin of an empty sequence")
        self._batch_engine = eng = self._cached("batch", spec, S, A, states.shape[0] * K,
                                                "cheetah" if terms is None else "terms", terms)
        eng.set_weights(spec, norm, version)
        self._apply_terminal_value(eng)
        res = eng.get_actions(states, None, seed=seed, return_costs=self.keep_costs)
        self.last_costs, self.last_cost, self.last_index = res.costs, res.best_cost, res.best_index
        self._note_terminal_value(eng, np.asarray(res.best_index, dtype=np.int64))
        return res.first_action

    def _trajectory_costs(self, eng: RolloutEngine, state, local_actions) -> np.ndarray:
        """Non-fused cost_fn: the engine returns states_paths_all (controllers.py:65-74)
        and the caller's cost_fn scores them through trajectory_cost_fn (:80)."""
        import torch
        dev = torch.device("cuda", eng.device)
        H, Kl, A = local_actions.shape
        S = eng.state_dim
        d_state = torch.from_numpy(state).to(dev)
        d_act = torch.from_numpy(local_actions).to(dev)
        d_traj = torch.empty((H + 1, Kl, S), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev)
        eng.rollout_async(d_state.data_ptr(), 0, d_act.data_ptr(), 0, 0, None, d_traj.data_ptr(), None,
                          stream.cuda_stream)
        traj = d_traj.cpu().numpy()                       # synchronises the stream
        eng.check_status()
        return np.asarray(trajectory_cost_fn(self.cost_fn, traj[:-1], local_actions, traj[1:]), dtype=np.float64)


class _SeedStream:
    """A controller's per-call Philox seeds: ``RandomState(seed).randint(0, 2**62)``, one per call, drawn 64 at
    a time (legacy randint fills a batch in call order, so the sequence is the one-at-a-time sequence) -- a call
    pays a list pop instead of a ~3-us scalar randint.  ``get_state`` / ``set_state`` carry the unread seeds."""

    def __init__(self, seed):
        self._rs = np.random.RandomState(seed)
        self._buf = []                          # unread seeds, next last

    def next(self) -> int:
        if not self._buf:
            self._buf = self._rs.randint(0, 2**62, size=64, dtype=np.int64).tolist()[::-1]
        return self._buf.pop()

    def unread(self, seed: int) -> None:
        self._buf.append(seed)

    def get_state(self):
        return self._rs.get_state(), tuple(self._buf)

    def set_state(self, state) -> None:
        self._rs.set_state(state[0])
        self._buf = list(state[1])


class MPCcontrollerPolicyNet(Controller):
    """Policy-guided MPC (controllers.py:160-237) on the MI355X rollout engine.

    Each horizon step the policy net's action for every candidate is computed
    inside the rollout kernel (fused 20->h->h->6 tanh MLP, ppo_bc_policy.py:
    54-88), mixed with the exploration draw and fed to the dynamics MLP:

    * ``self_exp=False`` (train_mpc_ppo.py default, FLAGS.SELFEXP):
      ``(1 - explore) * mean + explore * exploration[i]`` (controllers.py:204-208)
      -- deterministic given the global NumPy stream, bit-for-bit parity;
    * ``self_exp=True``: ``mean + exp(logstd) * N(0, 1)`` (DiagGaussianPd.sample).
      TF's random_normal stream cannot be reproduced outside TF; the engine
      draws N(0,1) with Philox (seed from ``seed=`` or a private generator, so
      the global NumPy stream is consumed exactly as the reference does).

    ``sample_random_actions`` is still called once per step in both modes
    (controllers.py:191), preserving the reference's RNG side effect.
    """

    def __init__(self,
                 env,
                 dyn_model,
                 policy_net,
                 explore=1.,
                 self_exp=True,
                 horizon=5,
                 cost_fn=None,
                 num_simulated_paths=10,
                 *,
                 seed: Optional[int] = None,
                 device: Optional[int] = None,
                 process_group=None,
                 terminal_value=None,
                 terminal_weight: float = -1.0):
        _refuse_terminal_value('MPCcontrollerPolicyNet', terminal_value)
        self.env = env
        self.dyn_model = dyn_model
        self.policy_net = policy_net
        self.horizon = horizon
        self.cost_fn = cost_fn
        self.num_simulated_paths = num_simulated_paths
        self.self_exp = self_exp
        self.explore = explore
        self._seed_rng = _SeedStream(0x5EEDF00D if seed is None else seed)
        self._device = device
        self._group = process_group
        self._engine = None
        self._fast = None                       # get_action's repeat-call fast path
        self.last_cost = None
        self.last_index = None
        self.last_costs = None
        self.keep_costs = False

    # controllers.py:181-186
    @_stock
    def sample_random_actions(self):
        np_action_paths = np.random.uniform(low=self.env.action_space.low, high=self.env.action_space.high,
                                            size=[self.horizon, self.num_simulated_paths,
                                                  len(self.env.action_space.high)])
        return np_action_paths

    def _engine_for(self, spec, pspec, S, A, k_local) -> RolloutEngine:
        self._engine = _cached_engine(
            self, "_engines", "single", S, A, spec.hidden, spec.n_layers, spec.activation, spec.layer_norm,
            int(self.horizon), int(k_local), device=_device(self),
            cost="reward" if spec.model == "reward" else "cheetah", model=spec.model, policy_hidden=pspec.hidden,
            policy_layers=pspec.n_layers, policy_mode="stochastic" if self.self_exp else "explore")
        return _attach_comm(self, self._engine)

    _MODEL = "delta"     # NNDynamicsModel + cheetah cost, argmin

    def _fast_key(self):
        return (self.env, self.dyn_model, self.policy_net, self.cost_fn, self.horizon, self.num_simulated_paths,
                self.explore, self.self_exp, self.keep_costs)

    # controllers.py:189-237
    def get_action(self, state):
        fp = getattr(self, "_fast", None)
        if fp is not None:
            # the per-env-step repeat (as MPCcontroller.get_action): same env / models / cost / shape /
            # exploration as the last call, the dynamics weights version and normalisation objects and the
            # policy's integer version unchanged, one rank, NumPy's verified legacy stream
            from .engine import _legacy_mt_state
            if (fp[0] == self._fast_key() and _weights.same_token(self.dyn_model, fp[1])
                    and _policy.int_version(self.policy_net) == fp[2] and "sample_random_actions" not in self.__dict__
                    and _dist.world(self._group)[1] == 1 and _legacy_mt_state() is not None):
                space = self.env.action_space
                seed = self._seed_rng.next()
                res = fp[3].get_action_numpy_stream(state, space.low, space.high, fp[4], 0, seed=seed)
                if res is not None:
                    self.last_costs = None
                    self.last_cost, self.last_index = res.best_cost, res.best_index
                    return res.first_action
                self._seed_rng.unread(seed)                      # (nothing drawn: the slow path draws it)
            self._fast = None
        S, A, K = _shape(self)
        reward = self._MODEL == "reward"
        if not reward and not is_cheetah_cost(self.cost_fn, S, A):
            raise ValueError("MPCcontrollerPolicyNet on the engine needs the fused cheetah cost_fn")
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        rank, ws = _dist.world(self._group)
        lo, hi = _dist.shard_range(K, rank, ws)
        spec, norm, version = _weights.extract(self.dyn_model)
        _check_model(spec, self._MODEL, type(self).__name__)
        pspec, pversion = _policy.extract(self.policy_net)
        sign = -1.0 if reward else 1.0                         # argmax(r) == argmin(-r), ties and NaN alike
        if K > 0 and hi > lo and _stock_sampler(self):
            # the exploration draw (controllers.py:191) made by the library into pinned memory,
            # same values and stream advance as sample_random_actions
            eng = self._engine_for(spec, pspec, S, A, hi - lo)
            eng.set_weights(spec, norm, version)
            eng.set_policy(pspec, float(self.explore), pversion)
            seed = self._seed_rng.next()
            res = eng.get_action_numpy_stream(state, self.env.action_space.low, self.env.action_space.high, K,
                                              lo, return_costs=self.keep_costs, seed=seed)
            if res is None:
                self._seed_rng.unread(seed)                  # (nothing drawn: the host path draws the seed)
            if res is not None:
                self.last_costs = res.costs
                cost, index, first_g = _minloc(self, eng, True, sign * res.best_cost, res.best_index,
                                               res.first_action, A)
                self.last_cost, self.last_index = sign * cost, index
                tok, pv = _weights.weight_token(self.dyn_model), _policy.int_version(self.policy_net)
                if ws == 1 and not self.keep_costs and tok is not None and pv is not None and eng.comm is None:
                    self._fast = (self._fast_key(), tok, pv, eng, K)
                return first_g
        exploration = self.sample_random_actions()           # every rank draws the full [H, K, A]
        seed = self._seed_rng.next()
        if K == 0:
            raise ValueError(f"attempt to get {'argmax' if reward else 'argmin'} of an empty sequence")
        valid, cost, index, first = False, float("inf"), -1, None
        if hi > lo:
            eng = self._engine_for(spec, pspec, S, A, hi - lo)
            eng.set_weights(spec, norm, version)
            eng.set_policy(pspec, float(self.explore), pversion)
            local = np.ascontiguousarray(exploration[:, lo:hi, :])
            res = eng.get_action(state, local, seed=seed, cand_offset=lo, return_costs=self.keep_costs)
            valid, cost, index, first = True, res.best_cost, res.best_index, res.first_action
            self.last_costs = res.costs
        cost, index, first_g = _minloc(self, self._engine if valid else None, valid, sign * cost, index, first, A)
        self.last_cost, self.last_index = sign * cost, index
        return first_g                                         # copy of action_paths[0, argmin] (:233-235)

    get_action_mcs = get_action                                # controllers.py:239 (identical body)


def _check_model(spec, want: str, who: str) -> None:
    if spec.model != want:
        need = "NNDynamicsRewardModel (dynamics.py:121)" if want == "reward" else "NNDynamicsModel (dynamics.py:7)"
        raise TypeError(f"{who} needs an {need}; got a {spec.model!r} dynamics net")


class MPCcontrollerReward(Controller):
    """Learned-reward random-shooting MPC (controllers.py:90-158) on the engine.

    ``dyn_model`` is an ``NNDynamicsRewardModel`` (dynamics.py:121-238): the
    kernel runs its two-head net each step and accumulates
    ``sum_h reward_h * gamma**h`` (controllers.py:139,150); the controller
    returns the first action of the ARGMAX path (controllers.py:152-156).

    Action source (``rng=``):

    * ``"env"`` (default, parity mode): ``sample_random_actions`` makes K*H
      ``env.action_space.sample()`` calls and reshapes them to ``[H, K, A]``
      exactly as controllers.py:108-119 (same env-RNG side effect, same dtype --
      a float32 Box gives float32 actions, widened exactly to f64 for the engine);
    * ``"device"`` (perf mode): Philox draws in the kernel, one 64-bit seed per
      call from a private generator (``seed=``), env RNG untouched.
    """

    def __init__(self,
                 env,
                 dyn_model,
                 horizon=5,
                 cost_fn=None,
                 num_simulated_paths=10,
                 gamma=1.,
                 *,
                 rng: str = "env",
                 seed: Optional[int] = None,
                 device: Optional[int] = None,
                 process_group=None,
                 terminal_value=None,
                 terminal_weight: float = -1.0):
        _refuse_terminal_value('MPCcontrollerReward', terminal_value)
        self.env = env
        self.dyn_model = dyn_model
        self.horizon = horizon
        self.cost_fn = cost_fn                  # stored, unused (as in the reference)
        self.num_simulated_paths = num_simulated_paths
        self.gamma = gamma
        if rng not in ("env", "device"):
            raise ValueError("rng must be 'env' or 'device'")
        self.rng = rng
        self._seed_rng = np.random.RandomState(0x5EED0BAD if seed is None else seed)
        self._device = device
        self._group = process_group
        self._engine: Optional[RolloutEngine] = None
        self.last_reward = None
        self.last_index = None
        self.last_rewards = None
        self.keep_costs = False

    # controllers.py:108-119
    def sample_random_actions(self):
        actions = []
        for n in range(self.num_simulated_paths):
            for h in range(self.horizon):
                actions.append(self.env.action_space.sample())
        np_action_paths = np.asarray(actions)
        np_action_paths = np.reshape(np_action_paths, [self.horizon, self.num_simulated_paths, -1])
        return np_action_paths

    def _cached(self, slot: str, spec, S, A, k) -> RolloutEngine:
        eng = _cached_engine(self, "_engines", slot, S, A, spec.hidden, 2, "tanh", spec.layer_norm,
                             int(self.horizon), int(k), device=_device(self), cost="reward", model="reward")
        eng.set_discount(float(self.gamma))
        return eng

    def _engine_for(self, spec, S, A, k_local) -> RolloutEngine:
        self._engine = self._cached("single", spec, S, A, k_local)
        return _attach_comm(self, self._engine)

    # controllers.py:121-158
    def get_action(self, state):
        S, A, K = _shape(self)
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        rank, ws = _dist.world(self._group)
        lo, hi = _dist.shard_range(K, rank, ws)
        spec, norm, version = _weights.extract(self.dyn_model)
        _check_model(spec, "reward", type(self).__name__)
        action_paths, seed = None, 0
        if self.rng == "env":
            action_paths = self.sample_random_actions()      # every rank draws the full [H, K, A]
        else:
            seed = int(self._seed_rng.randint(0, 2**62, dtype=np.int64))
        if K == 0:
            raise ValueError("attempt to get argmax of an empty sequence")
        valid, neg, index, first = False, float("inf"), -1, None
        if hi > lo:
            eng = self._engine_for(spec, S, A, hi - lo)
            eng.set_weights(spec, norm, version)
            local = None if action_paths is None else np.ascontiguousarray(action_paths[:, lo:hi, :],
                                                                           dtype=np.float64)
            res = eng.get_action(state, local, seed=seed, cand_offset=lo, return_costs=self.keep_costs)
            valid, neg, index, first = True, -res.best_cost, res.best_index, res.first_action
            self.last_rewards = res.costs
        neg, index, first_g = _minloc(self, self._engine if valid else None, valid, neg, index, first, A)
        self.last_reward, self.last_index = -neg, index
        if action_paths is not None:
            return copy.copy(action_paths[:, index, :][0])    # controllers.py:154-156
        return first_g

    def get_actions(self, states):
        """Batched control step (not in the reference): ``states`` ``[B, S]`` -> ``[B, A]`` float64, row ``b``
        the ARGMAX answer for ``states[b]`` on the Philox candidates ``b*K .. (b+1)*K`` of the call's seed
        (one seed per call), all environments in one launch chain (``RolloutEngine.get_actions``).
        ``rng="device"`` on one rank only."""
        _batch_rng_check(self.rng)
        S, A, K = _shape(self)
        states = _batch_states(states, S, self._group)
        spec, norm, version = _weights.extract(self.dyn_model)
        _check_model(spec, "reward", type(self).__name__)
        seed = int(self._seed_rng.randint(0, 2**62, dtype=np.int64))
        if K == 0:
            raise ValueError("attempt to get argmax of an empty sequence")
        self._batch_engine = eng = self._cached("batch", spec, S, A, states.shape[0] * K)
        eng.set_weights(spec, norm, version)
        res = eng.get_actions(states, None, seed=seed, return_costs=self.keep_costs)
        self.last_rewards, self.last_reward, self.last_index = res.costs, res.best_cost, res.best_index
        return res.first_action


class MPCcontrollerPolicyNetReward(MPCcontrollerPolicyNet):
    """Policy-guided learned-reward MPC (controllers.py:289-363) on the engine:
    the fused policy of ``MPCcontrollerPolicyNet`` plus the two-head reward net;
    argmax of the UNdiscounted reward sum (``gamma`` is stored but unused,
    controllers.py:345).  The reference's debug print of the reward-vector
    shape (controllers.py:351) is not reproduced."""

    _MODEL = "reward"

    def __init__(self,
                 env,
                 dyn_model,
                 policy_net,
                 explore=1.,
                 self_exp=True,
                 horizon=5,
                 cost_fn=None,
                 num_simulated_paths=10,
                 gamma=1.,
                 *,
                 seed: Optional[int] = None,
                 device: Optional[int] = None,
                 process_group=None):
        super().__init__(env, dyn_model, policy_net, explore=explore, self_exp=self_exp, horizon=horizon,
                         cost_fn=cost_fn, num_simulated_paths=num_simulated_paths, seed=seed, device=device,
                         process_group=process_group)
        self.gamma = gamma

    # controllers.py:310-316
    @_stock
    def sample_random_actions(self):
        np_action_paths = np.random.uniform(low=self.env.action_space.low, high=self.env.action_space.high,
                                            size=[self.horizon, self.num_simulated_paths,
                                                  len(self.env.action_space.high)])
        return np_action_paths


class MCTScontrollerPolicyNetReward(Controller):
    """Two-stage policy-guided search (controllers.py:365-457) on the engine.

    Stage 1 (controllers.py:403-425): ``num_first_stage_actions`` (N) first actions from the root
    state -- the policy's stochastic sample (``self_exp=True``, Philox normals as in
    ``MPCcontrollerPolicyNet``), its mean (``self_exp=False``), or ``env.action_space.sample()``
    (``random_first_stage_action``) -- each scored by one ``predict`` step of the two-head
    ``NNDynamicsRewardModel``: one engine launch of N candidates, horizon 1, returning the first
    actions, the rewards and the next states.  Stage 2 (controllers.py:427-449): every next state
    tiled ``random_path_per_action`` (R) times and rolled ``horizon`` steps with the DETERMINISTIC
    policy (the reference's ``stochastic=False``): one launch of N*R candidates with per-candidate
    initial states and the fused policy at ``explore = 0``, returning the reward sums.  The mean over
    the R paths, the sum with the first reward and the argmax stay NumPy (:442-451).  Returns the
    chosen first action with the reference's shape ``[1, A]`` (float32 for the policy's actions).
    The reference's follow-up paths of one first action are identical (deterministic policy and
    model), so the engine computes N*R equal rows exactly as the reference does.
    """

    def __init__(self,
                 env,
                 dyn_model,
                 policy_net,
                 explore=1.,
                 self_exp=True,
                 horizon=5,
                 cost_fn=None,
                 num_first_stage_actions=10,
                 random_path_per_action=10,
                 random_first_stage_action=False,
                 *,
                 seed: Optional[int] = None,
                 device: Optional[int] = None,
                 terminal_value=None,
                 terminal_weight: float = -1.0):
        _refuse_terminal_value('MCTScontrollerPolicyNetReward', terminal_value)
        self.env = env
        self.dyn_model = dyn_model
        self.policy_net = policy_net
        self.horizon = horizon
        self.cost_fn = cost_fn
        self.num_first_stage_actions = num_first_stage_actions
        self.random_path_per_action = random_path_per_action
        self.self_exp = self_exp
        self.explore = explore
        self.random_first_stage_action = random_first_stage_action
        self._seed_rng = np.random.RandomState(0x5EEDC0DE if seed is None else seed)
        self._device = device
        self._engines = {}
        self.last_index = None
        self.last_total_rewards = None
        self.last_first_actions = None
        self.last_seeds = None

    # controllers.py:390-395, verbatim: __init__ never sets num_simulated_paths, so (as in the
    # reference) calling it raises AttributeError; get_action does not use it
    def sample_random_actions(self):
        np_action_paths = np.random.uniform(low=self.env.action_space.low, high=self.env.action_space.high,
                                            size=[self.horizon, self.num_simulated_paths,
                                                  len(self.env.action_space.high)])
        return np_action_paths

    def _engine_for(self, stage, spec, pspec, S, A, K, H, mode, dev) -> RolloutEngine:
        return _cached_engine(self, "_engines", stage, S, A, spec.hidden, 2, "tanh", spec.layer_norm, int(H), int(K),
                              device=dev, cost="reward", model="reward", policy_hidden=pspec.hidden,
                              policy_layers=pspec.n_layers, policy_mode=mode)

    # controllers.py:397-457
    def get_action(self, state):
        import torch
        S = int(math.prod(self.env.observation_space.shape))
        A = len(self.env.action_space.high)
        N, R = int(self.num_first_stage_actions), int(self.random_path_per_action)
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        spec, norm, version = _weights.extract(self.dyn_model)
        _check_model(spec, "reward", type(self).__name__)
        pspec, pversion = _policy.extract(self.policy_net)
        dev = _device(self)
        tdev = torch.device("cuda", dev)
        stream = torch.cuda.current_stream(tdev).cuda_stream
        if N == 0:
            raise ValueError("attempt to get argmax of an empty sequence")
        # ---- first stage (controllers.py:403-418) ----
        action_1s, d_act = None, None
        if self.random_first_stage_action:
            action_1s = [np.expand_dims(self.env.action_space.sample(), axis=0) for _ in range(N)]
            mode, explore = "explore", 1.0                       # (1 - 1) * mean + 1 * U = U exactly
            d_act = torch.from_numpy(np.concatenate(action_1s).astype(np.float64)[None]).to(tdev)
        elif self.self_exp:
            mode, explore = "stochastic", float(self.explore)    # mean + exp(logstd) * N(0, 1)
        else:
            mode, explore = "explore", 0.0                       # the mean
        seed1 = int(self._seed_rng.randint(0, 2**62, dtype=np.int64))
        e1 = self._engine_for("first", spec, pspec, S, A, N, 1, mode, dev)
        e1.set_weights(spec, norm, version)
        e1.set_policy(pspec, explore, pversion)
        d_state = torch.from_numpy(state).to(tdev)
        d_r1 = torch.empty(N, dtype=torch.float64, device=tdev)
        d_traj = torch.empty((2, N, S), dtype=torch.float64, device=tdev)
        e1.rollout_async(d_state.data_ptr(), 0, d_act.data_ptr() if d_act is not None else None, seed1, 0,
                         d_r1.data_ptr(), d_traj.data_ptr(), None, stream)
        reward_1s = d_r1.cpu().numpy()                           # reward_1[0][0] of each predict (:418)
        e1.check_status()
        first = e1.first_actions()
        if action_1s is None:                                    # policy.act's f32 [1, A] rows
            action_1s = [first[i:i + 1].astype(np.float32) for i in range(N)]
        # ---- following stages (controllers.py:421-440): next states tiled R times, action-major ----
        if self.horizon >= 1 and R >= 1:
            seed2 = int(self._seed_rng.randint(0, 2**62, dtype=np.int64))
            e2 = self._engine_for("follow", spec, pspec, S, A, N * R, self.horizon, "explore", dev)
            e2.set_weights(spec, norm, version)
            e2.set_policy(pspec, 0.0, pversion)                  # stochastic=False: the mean
            d_states = torch.repeat_interleave(d_traj[1], R, dim=0).contiguous()
            d_rsum = torch.empty(N * R, dtype=torch.float64, device=tdev)
            e2.rollout_async(d_states.data_ptr(), S, None, seed2, 0, d_rsum.data_ptr(), None, None, stream)
            rewards_all = d_rsum.cpu().numpy().reshape((-1, 1))  # sum over steps of [N*R, 1] (:442-443)
            e2.check_status()
        else:
            seed2 = None
            rewards_all = np.sum(np.asarray([]), axis=0)         # the reference's empty horizon
        rewards_all = rewards_all.reshape((N, -1))              # (:445)
        rewards_all_mean = np.mean(rewards_all, axis=1)
        total_rewards = np.asarray(reward_1s) + rewards_all_mean
        best_action1_idx = int(np.argmax(total_rewards))
        self.last_index, self.last_total_rewards = best_action1_idx, total_rewards
        self.last_first_actions, self.last_seeds = first, (seed1, seed2)
        return action_1s[best_action1_idx]

    def close(self):
        for _, eng in self._engines.values():
            eng.close()
        self._engines = {}

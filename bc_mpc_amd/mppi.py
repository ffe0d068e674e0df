"""MPPI-MPC: model-predictive path integral control (the information-theoretic MPC of
Williams et al.) on the rollout engine.

The reference has no MPPI, so this controller defines it -- DESIGN.md "MPPI" -- with the
reference's constructor and ``get_action(state)`` contract, keyword extras only:

* a round samples every candidate's ``[H, A]`` actions as ``clip(mu + sigma * z, low, high)``
  in the rollout kernel, exactly as a CEM iteration does (same Philox stream);
* the candidates are scored like ``MPCcontroller.get_action`` (fused cheetah cost, or a
  ``cost_functions.TermCost`` on any state size) or like
  ``MPCcontrollerReward`` (learned reward, negated so that lower is better);
* EVERY candidate with a finite score gets the weight ``exp(-(v - v_min) / temperature)`` and
  the plan becomes the weighted mean of the candidates' actions; sigma stays as it is;
* the answer is the first step of the updated plan, ``mu'[0]`` -- a smooth action, not one
  noisy sample.  The best single candidate over all rounds is kept as ``last_cost`` /
  ``last_position``.

Not included: MPPI's control-cost term ``lambda * u^T Sigma^-1 eps`` and a sigma update.

Single GPU only: one ``bcmpc_mppi_get_action`` call (all rounds stream-ordered on the device,
one host sync).  With more than one rank the per-rank ``(v_min, W, N)`` partials would have to be
combined; that is not built yet and ``get_action`` raises NotImplementedError.

Many environments per call: ``get_actions(states[B, S])`` runs B independent MPPI problems, one
warm-start plan per environment, in one ``bcmpc_mppi_get_actions_batch`` call.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import distributed as _dist
from . import weights as _weights
from .controllers import Controller, _BatchPlans, _check_model, _default_device, _device_terms, _opt
from .cost_functions import is_cheetah_cost
from .engine import RolloutEngine


class MPPIcontroller(_BatchPlans, Controller):
    """MPPI on the MI355X engine: softmin-weighted plan update over all sampled candidates."""

    def __init__(self,
                 env,
                 dyn_model,
                 horizon=5,
                 cost_fn=None,
                 num_simulated_paths=10,
                 gamma=1.,
                 *,
                 temperature: float = 1.0,
                 iterations: int = 1,
                 init_std: Optional[float] = None,
                 warm_start: bool = True,
                 seed: Optional[int] = None,
                 device: Optional[int] = None,
                 process_group=None):
        self.env = env
        self.dyn_model = dyn_model
        self.horizon = horizon
        self.cost_fn = cost_fn
        self.num_simulated_paths = num_simulated_paths
        self.gamma = gamma
        if iterations < 1:
            raise ValueError("iterations must be >= 1")
        if not (math.isfinite(temperature) and temperature > 0):
            raise ValueError("temperature must be finite and > 0")
        self.iterations = int(iterations)
        self.temperature = float(temperature)
        self.init_std = init_std
        self.warm_start = warm_start
        self._seed_rng = np.random.RandomState(0x3B9AC1 if seed is None else seed)
        self._device = device
        self._group = process_group
        self._engine: Optional[RolloutEngine] = None
        self._engine_key = None
        self._gamma_set = None
        self._mu = None
        self.last_mu = None
        self.last_cost = None
        self.last_position = None
        self.last_ess = None
        self.last_stats = None

    def reset(self, env_ids=None) -> None:
        """Forget the warm-start plan (call at episode boundaries).  ``env_ids``: forget only those
        environments' plans of ``get_actions`` (an episode boundary in one simulator of a batch)."""
        if env_ids is None:
            self._mu = None
        self._reset_plans(env_ids)

    def _bounds(self):
        return (np.asarray(self.env.action_space.low, dtype=np.float64),
                np.asarray(self.env.action_space.high, dtype=np.float64))

    def initial_distribution(self):
        """mu0: the previous plan shifted by one step with the box centre appended (warm start), or
        the box centre; sigma0: init_std, default (high - low) / 4."""
        low, high = self._bounds()
        H = int(self.horizon)
        mid = (low + high) / 2.0
        sd = np.full_like(low, self.init_std) if self.init_std is not None else (high - low) / 4.0
        if self.warm_start and self._mu is not None and self._mu.shape == (H, low.shape[0]):
            mu = np.vstack([self._mu[1:], mid[None]])
        else:
            mu = np.tile(mid, (H, 1))
        return mu, np.tile(sd, (H, 1))

    def _engine_for(self, spec, S, A, k_local, terms=None) -> RolloutEngine:
        dev = _default_device() if self._device is None else self._device
        key = (S, A, spec.model, spec.hidden, spec.n_layers, spec.activation, spec.layer_norm, int(self.horizon),
               int(k_local), dev, terms is not None)
        if self._engine is None or self._engine_key != key:
            if self._engine is not None:
                self._engine.close()
            reward = spec.model == "reward"
            self._engine = RolloutEngine(S, A, spec.hidden, spec.n_layers, spec.activation, spec.layer_norm,
                                         int(self.horizon), int(k_local), device=dev,
                                         cost="reward" if reward else "terms" if terms is not None else "cheetah",
                                         model=spec.model)
            self._engine.set_action_bounds(*self._bounds())
            self._engine_key = key
            self._gamma_set = None
        if terms is not None:
            self._engine.set_cost_terms(terms)
        if spec.model == "reward" and self._gamma_set != float(self.gamma):
            self._engine.set_discount(float(self.gamma))
            self._gamma_set = float(self.gamma)
        return self._engine

    def get_action(self, state):
        if getattr(self.dyn_model, "is_ensemble", False):   # an EnsembleDynamicsModel (ensemble.py)
            from . import ensemble as _ensemble
            return _ensemble.mppi_get_action(self, state)
        S = int(math.prod(self.env.observation_space.shape))
        A = len(self.env.action_space.high)
        K = int(self.num_simulated_paths)
        if self.horizon < 1:
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")
        if K == 0:
            raise ValueError("attempt to get argmin of an empty sequence")
        _, ws = _dist.world(self._group)
        if ws > 1:
            raise NotImplementedError(
                f"MPPIcontroller runs on one rank (world size {ws}): combining the ranks' (v_min, W, N) "
                "partials of the weighted mean is not built yet")
        state = np.asarray(state, dtype=np.float64).reshape(-1)
        spec, norm, version = _weights.extract(self.dyn_model)
        terms = None
        if spec.model != "reward":
            _check_model(spec, "delta", type(self).__name__)
            terms = _device_terms(self.cost_fn, S, A)
            if terms is None and not is_cheetah_cost(self.cost_fn, S, A):
                raise ValueError("MPPIcontroller needs the fused cheetah cost_fn or a learned-reward dyn_model")
        mu0, sd0 = self.initial_distribution()
        seed = int(self._seed_rng.randint(0, 2**62, dtype=np.int64))
        eng = self._engine_for(spec, S, A, K, *_opt(terms))
        eng.set_weights(spec, norm, version)
        res, mu, stats = eng.mppi_get_action(state, mu0, sd0, self.iterations, self.temperature, seed)
        self._mu = mu
        self.last_mu = mu
        self.last_cost, self.last_position = res.best_cost, res.best_index
        self.last_ess, self.last_stats = float(stats.ess), stats
        return mu[0].copy()

    def get_actions(self, states):
        """Batched control step: ``states`` is ``[B, S]``, one independent MPPI answer per row with
        ``num_simulated_paths`` candidates each, all environments in one launch chain
        (``RolloutEngine.mppi_get_actions``).  Every environment keeps its own warm-start plan (see
        ``reset``); one seed is drawn per call.  Returns ``[B, A]`` float64: ``mu'[b, 0]``.  ``last_mu``
        (``[B, H, A]``), ``last_ess`` / ``last_cost`` / ``last_position`` (``[B]``) and ``last_stats`` (a
        ``[B]`` record array) describe the call.  One rank only."""
        if getattr(self.dyn_model, "is_ensemble", False):
            raise NotImplementedError("batched MPPI over an EnsembleDynamicsModel is not built yet: use get_action")
        S = int(math.prod(self.env.observation_space.shape))
        A = len(self.env.action_space.high)
        K = int(self.num_simulated_paths)
        if self.horizon < 1:
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")
        states = self._plan_states(states, S)
        if K == 0:
            raise ValueError("attempt to get argmin of an empty sequence")
        spec, norm, version = _weights.extract(self.dyn_model)
        terms = None
        if spec.model != "reward":
            _check_model(spec, "delta", type(self).__name__)
            terms = _device_terms(self.cost_fn, S, A)
            if terms is None and not is_cheetah_cost(self.cost_fn, S, A):
                raise ValueError("MPPIcontroller needs the fused cheetah cost_fn or a learned-reward dyn_model")
        B = states.shape[0]
        mu0, sd0 = self.batch_initial_distribution(B)
        seed = int(self._seed_rng.randint(0, 2**62, dtype=np.int64))
        eng = self._batch_engine_for(spec, S, A, B * K, *_opt(terms))
        eng.set_weights(spec, norm, version)
        res, mu, stats = eng.mppi_get_actions(states, mu0, sd0, self.iterations, self.temperature, seed)
        self._store_plans(mu)
        self.last_mu = mu
        self.last_cost, self.last_position = res.best_cost, res.best_index
        self.last_ess, self.last_stats = stats["ess"].copy(), stats
        return mu[:, 0].copy()

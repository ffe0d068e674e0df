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

Two options complete the textbook update (mppi_update.py), both off by default:

* ``control_cost`` adds MPPI's control-cost term ``weight * u^T Sigma^-1 eps`` to the score the weights see
  (``True``: the temperature, the textbook weight).  ``last_cost`` stays the best RAW cost;
* ``adapt_sigma`` refits sigma after every round of a call from the weighted standard deviation about the
  updated plan, smoothed by ``sigma_alpha`` and clamped to ``[min_std, max_std]``.  Every call still starts
  from ``init_std``; ``last_sigma`` is the call's final sigma.

Single GPU only: one ``bcmpc_mppi_get_action`` call (all rounds stream-ordered on the device,
one host sync).  With more than one rank the per-rank ``(v_min, W, N)`` partials would have to be
combined; that is not built yet and ``get_action`` raises NotImplementedError.

Many environments per call: ``get_actions(states[B, S])`` runs B independent MPPI problems, one
warm-start plan per environment, in one ``bcmpc_mppi_get_actions_batch`` call.
"""
from __future__ import annotations

import math
from typing import Optional

from . import mppi_update as _mppi_update
from .controllers import Planner


class MPPIcontroller(Planner):
    """MPPI on the MI355X engine: softmin-weighted plan update over all sampled candidates.  ``get_action`` /
    ``get_actions`` return the first step of the updated plan, ``mu'[0]``; ``last_mu`` holds the plan,
    ``last_cost`` / ``last_position`` the best single sample, ``last_ess`` / ``last_stats`` the last round's
    statistics (batched: ``[B, H, A]``, ``[B]``, and ``last_stats`` a ``[B]`` record array).  ``noise_rho`` in
    ``[0, 1)``: AR(1) noise over the horizon instead of independent draws (sampling.py; read on
    every call, one rank and one dynamics model only).  ``control_cost`` / ``adapt_sigma`` / ``sigma_alpha`` /
    ``min_std`` / ``max_std``: the control-cost term and the sigma update (module docstring; read on every call,
    one rank and one dynamics model only); ``last_sigma`` is the sigma the call ended with (``[H, A]``, batched
    ``[B, H, A]``) and, with the control cost on, ``last_stats.min_cost`` the minimum augmented score.
    ``proposals=`` on a call and ``policy_prior`` / ``policy_paths`` / ``policy_stochastic`` / ``policy_explore``: given
    action sequences, and a policy net's closed-loop rollouts, in the last candidates of every round (proposals.py,
    DESIGN.md 9m; one rank and one dynamics model only).  A proposal is no draw from ``N(mu, sigma)``: its softmin
    weight and its control-cost term (``eps = a - mu``) are the heuristic TD-MPC uses for its policy trajectories.
    ``knots`` (M in ``[1, horizon]``) / ``knot_interp`` (``"hold" | "linear" | "cubic"``): the plan is sampled at M
    knots and interpolated to the horizon (knots.py; read on every call, one rank and one dynamics
    model only, not with proposals or a policy prior).  ``last_mu`` / ``last_sigma`` and the warm start are then in
    KNOT space, ``[M, A]`` (batched ``[B, M, A]``); the answer is still ``mu'[0]`` (knot 0 sits at step 0) and
    ``last_plan`` is the ``[H, A]`` sequence ``last_mu`` expands to (without knots it equals ``last_mu``)."""
    _KIND = "MPPI"
    # what the update adds (mppi_update.py): read on every call, never an engine constructor argument
    control_cost = 0.0
    adapt_sigma = False
    sigma_alpha = 0.0
    min_std = 0.0
    max_std = None

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
                 process_group=None,
                 terminal_value=None,
                 terminal_weight: float = -1.0,
                 noise_rho: float = 0.0,
                 control_cost=0.0,
                 adapt_sigma: bool = False,
                 sigma_alpha: float = 0.0,
                 min_std: float = 0.0,
                 max_std: Optional[float] = None,
                 policy_prior=None,
                 policy_paths: int = 0,
                 policy_stochastic: bool = True,
                 policy_explore: float = 0.0,
                 knots: Optional[int] = None,
                 knot_interp: str = "linear"):
        super().__init__(env, dyn_model, horizon, cost_fn, num_simulated_paths, gamma, iterations, init_std,
                         warm_start, 0x3B9AC1 if seed is None else seed, device, process_group,
                         terminal_value=terminal_value, terminal_weight=terminal_weight, noise_rho=noise_rho,
                         policy_prior=policy_prior, policy_paths=policy_paths, policy_stochastic=policy_stochastic,
                         policy_explore=policy_explore, knots=knots, knot_interp=knot_interp)
        if not (math.isfinite(temperature) and temperature > 0):
            raise ValueError("temperature must be finite and > 0")
        self.temperature = float(temperature)
        _mppi_update.check_options(control_cost, adapt_sigma, sigma_alpha, min_std, max_std, self.temperature)
        self.control_cost, self.adapt_sigma = control_cost, adapt_sigma
        self.sigma_alpha, self.min_std, self.max_std = sigma_alpha, min_std, max_std
        self.last_ess = None
        self.last_stats = None
        self.last_sigma = None

    def _refuse_ranks(self, ws):
        raise NotImplementedError(f"MPPIcontroller runs on one rank (world size {ws}): combining the ranks' "
                                  "(v_min, W, N) partials of the weighted mean is not built yet")

    def _update_args(self) -> dict:
        """The engine calls' ``control_cost`` / ``adapt_sigma`` and the sigma step's parameters, passed only when
        one of the two is on (the call at the defaults is the call it has always been)."""
        weight, adapt, alpha, lo, hi = _mppi_update.check_options(
            self.control_cost, self.adapt_sigma, self.sigma_alpha, self.min_std, self.max_std, self.temperature)
        kw = {}
        if weight != 0.0:
            kw["control_cost"] = weight
        if adapt:
            kw.update(adapt_sigma=True, sigma_alpha=alpha, min_std=lo, max_std=hi)
        return kw

    def _refuse_sampling(self, where: str) -> None:
        super()._refuse_sampling(where)
        if self._update_args():
            raise NotImplementedError(f"MPPIcontroller: control_cost / adapt_sigma are not built {where}")

    def _solve(self, eng, state, mu0, sd0, seed, K):
        res, mu, stats, *sd = eng.mppi_get_action(state, mu0, sd0, self.iterations, self.temperature, seed,
                                                  **self._sampling_args(), **self._update_args(), **self._knot_args())
        self._note_planner_value(eng, res.best_index, K)
        self._mu = mu
        self.last_mu = mu
        self.last_sigma = sd[0] if sd else sd0
        self.last_cost, self.last_position = res.best_cost, res.best_index
        self.last_ess, self.last_stats = float(stats.ess), stats
        return mu[0].copy()

    def _call_proposals(self, eng, states, mu0, sd0, seed, src):
        res, mu, stats, *sd = eng.mppi_get_actions(states, mu0, sd0, self.iterations, self.temperature, seed,
                                                   return_costs=True, proposals=src, **self._sampling_args(),
                                                   **self._update_args())
        return res, mu, stats, sd[0] if sd else sd0

    def _publish_proposals(self, eng, out, K, single: bool):
        res, mu, stats, sd = out
        if single:
            from . import _lib
            self._note_planner_value(eng, int(res.best_index[0]), K)
            self._mu = self.last_mu = mu[0]
            self.last_sigma = sd[0]
            self.last_cost, self.last_position = float(res.best_cost[0]), int(res.best_index[0])
            self.last_stats = _lib.MppiStats(*stats[0].tolist())
            self.last_ess = float(self.last_stats.ess)
            return mu[0, 0].copy()
        self._note_planner_value(eng, res.best_index, K)
        self._store_plans(mu)
        self.last_mu, self.last_sigma = mu, sd
        self.last_cost, self.last_position = res.best_cost, res.best_index
        self.last_ess, self.last_stats = stats["ess"].copy(), stats
        return mu[:, 0].copy()

    def _solve_batch(self, eng, states, mu0, sd0, seed, K):
        res, mu, stats, *sd = eng.mppi_get_actions(states, mu0, sd0, self.iterations, self.temperature, seed,
                                                   **self._sampling_args(), **self._update_args(), **self._knot_args())
        self._note_planner_value(eng, res.best_index, K)
        self._store_plans(mu)
        self.last_mu = mu
        self.last_sigma = sd[0] if sd else sd0
        self.last_cost, self.last_position = res.best_cost, res.best_index
        self.last_ess, self.last_stats = stats["ess"].copy(), stats
        return mu[:, 0].copy()

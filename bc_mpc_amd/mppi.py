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

from .controllers import Planner


class MPPIcontroller(Planner):
    """MPPI on the MI355X engine: softmin-weighted plan update over all sampled candidates.  ``get_action`` /
    ``get_actions`` return the first step of the updated plan, ``mu'[0]``; ``last_mu`` holds the plan,
    ``last_cost`` / ``last_position`` the best single sample, ``last_ess`` / ``last_stats`` the last round's
    statistics (batched: ``[B, H, A]``, ``[B]``, and ``last_stats`` a ``[B]`` record array).  ``noise_rho`` in
    ``[0, 1)``: AR(1) noise over the horizon instead of independent draws (sampling.py; read on
    every call, one rank and one dynamics model only)."""
    _KIND = "MPPI"

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
                 noise_rho: float = 0.0):
        super().__init__(env, dyn_model, horizon, cost_fn, num_simulated_paths, gamma, iterations, init_std,
                         warm_start, 0x3B9AC1 if seed is None else seed, device, process_group,
                         terminal_value=terminal_value, terminal_weight=terminal_weight, noise_rho=noise_rho)
        if not (math.isfinite(temperature) and temperature > 0):
            raise ValueError("temperature must be finite and > 0")
        self.temperature = float(temperature)
        self.last_ess = None
        self.last_stats = None

    def _refuse_ranks(self, ws):
        raise NotImplementedError(f"MPPIcontroller runs on one rank (world size {ws}): combining the ranks' "
                                  "(v_min, W, N) partials of the weighted mean is not built yet")

    def _solve(self, eng, state, mu0, sd0, seed, K):
        res, mu, stats = eng.mppi_get_action(state, mu0, sd0, self.iterations, self.temperature, seed,
                                             **self._sampling_args())
        self._note_planner_value(eng, res.best_index, K)
        self._mu = mu
        self.last_mu = mu
        self.last_cost, self.last_position = res.best_cost, res.best_index
        self.last_ess, self.last_stats = float(stats.ess), stats
        return mu[0].copy()

    def _solve_batch(self, eng, states, mu0, sd0, seed, K):
        res, mu, stats = eng.mppi_get_actions(states, mu0, sd0, self.iterations, self.temperature, seed,
                                              **self._sampling_args())
        self._note_planner_value(eng, res.best_index, K)
        self._store_plans(mu)
        self.last_mu = mu
        self.last_cost, self.last_position = res.best_cost, res.best_index
        self.last_ess, self.last_stats = stats["ess"].copy(), stats
        return mu[:, 0].copy()

"""CEM-MPC: the cross-entropy-method outer loop of BASELINE cfg5 on the rollout engine.

The reference has no CEM ("Listed in BASELINE configs, but not
in the reference"), so this controller defines it -- DESIGN.md "CEM" -- with the
reference's constructor and ``get_action(state)`` contract, keyword extras only:

* iteration i samples every candidate's ``[H, A]`` actions as
  ``clip(mu + sigma * z, low, high)`` with z = Irwin-Hall(12) - 6 drawn in the
  rollout kernel (Philox keyed by seed, global candidate, h, j, i);
* the candidates are scored exactly like ``MPCcontroller.get_action`` (fused
  cheetah cost or a ``cost_functions.TermCost``, argmin) or like
  ``MPCcontrollerReward`` (learned reward, argmax);
* the ``n_elite`` best (NaN last, ties to the lower index) refit mu / sigma to
  their mean / std, smoothed by ``alpha``;
* the answer is the first action of the best candidate of ALL iterations.

Single GPU: one ``bcmpc_cem_get_action`` call (all iterations stream-ordered on
the device, one host sync).  Multi-GPU (torch.distributed, one rank per GPU):
each rank rolls out its contiguous candidate shard; per iteration the ranks
all-gather their local top-E (cost, index) records (E x 16 bytes each), every
rank selects the same global top-E from the gathered records and refits the
same mu / sigma by regenerating the elites' actions from Philox -- no second
collective.  One final all-gather min-loc picks the answer.

Many environments per call (one rank): ``get_actions(states[B, S])`` runs B independent CEM
problems, one warm-start plan per environment, in one ``bcmpc_cem_get_actions_batch`` call
(DESIGN.md 9e).
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from . import distributed as _dist
from .controllers import Planner

_ELITE_BYTES = ctypes.sizeof(_lib.Elite)


class CEMcontroller(Planner):
    """Cross-entropy-method MPC on the MI355X engine (BASELINE cfg5 CEM outer loop).  ``get_action`` /
    ``get_actions`` return the first action of the best sample of all iterations; ``last_mu`` / ``last_sigma``
    hold the refitted distribution, ``last_cost`` / ``last_position`` the best sample (batched: ``[B, H, A]``
    and ``[B]``).  ``noise_rho`` in ``[0, 1)``: AR(1) noise over the horizon instead of independent draws;
    ``keep_elites``: every iteration after the first starts with all elites of the one before (sampling.py,
    DESIGN.md 9j; both are read on every call, one rank and one dynamics model only).  ``proposals=`` on a call
    and ``policy_prior`` / ``policy_paths`` / ``policy_stochastic`` / ``policy_explore``: given action sequences, and
    a policy net's closed-loop rollouts, in the last candidates of every iteration (proposals.py; one
    rank and one dynamics model only); ``last_proposal_costs`` / ``last_best_from_proposal`` report on them.
    ``knots`` (M in ``[1, horizon]``) / ``knot_interp`` (``"hold" | "linear" | "cubic"``): the plan is sampled at M
    knots and interpolated to the horizon (knots.py; read on every call, one rank and one dynamics
    model only, not with proposals or a policy prior).  ``last_mu`` / ``last_sigma`` and the warm start are then in
    KNOT space, ``[M, A]`` (batched ``[B, M, A]``); ``last_plan`` is the ``[H, A]`` sequence ``last_mu`` expands to
    (without knots it equals ``last_mu``)."""
    _KIND = "CEM"

    def __init__(self,
                 env,
                 dyn_model,
                 horizon=5,
                 cost_fn=None,
                 num_simulated_paths=10,
                 gamma=1.,
                 *,
                 iterations: int = 4,
                 elite_frac: float = 0.1,
                 n_elite: Optional[int] = None,
                 alpha: float = 0.1,
                 init_std: Optional[float] = None,
                 warm_start: bool = True,
                 seed: Optional[int] = None,
                 device: Optional[int] = None,
                 process_group=None,
                 terminal_value=None,
                 terminal_weight: float = -1.0,
                 noise_rho: float = 0.0,
                 keep_elites: bool = False,
                 policy_prior=None,
                 policy_paths: int = 0,
                 policy_stochastic: bool = True,
                 policy_explore: float = 0.0,
                 knots: Optional[int] = None,
                 knot_interp: str = "linear"):
        super().__init__(env, dyn_model, horizon, cost_fn, num_simulated_paths, gamma, iterations, init_std,
                         warm_start, 0xCE5EED if seed is None else seed, device, process_group,
                         terminal_value=terminal_value, terminal_weight=terminal_weight, noise_rho=noise_rho,
                         keep_elites=keep_elites, policy_prior=policy_prior, policy_paths=policy_paths,
                         policy_stochastic=policy_stochastic, policy_explore=policy_explore, knots=knots,
                         knot_interp=knot_interp)
        self.elite_frac = float(elite_frac)
        self._n_elite = n_elite
        self.alpha = float(alpha)
        self.last_sigma = None

    @property
    def n_elite(self) -> int:
        if self._n_elite is not None:
            return int(self._n_elite)
        return max(1, int(round(self.elite_frac * int(self.num_simulated_paths))))

    def _solve(self, eng, state, mu0, sd0, seed, K):
        res, mu, sd = eng.cem_get_action(state, mu0, sd0, self.iterations, min(self.n_elite, K), self.alpha, seed,
                                         **self._sampling_args(), **self._knot_args())
        self._note_planner_value(eng, res.best_index, K)
        return self._publish(res.best_cost, res.best_index, res.first_action, mu, sd)

    def _sharded(self, rank, ws, state, spec, norm, version, terms, mu0, sd0, seed, S, A, K):
        """Every rank rolls out its shard of the K candidates (cem_multi_rank)."""
        lo, hi = _dist.shard_range(K, rank, ws)
        if terms is not None:
            raise NotImplementedError("multi-rank CEM with a TermCost is not built yet (one rank only)")
        if K < ws:
            raise ValueError(f"multi-rank CEM needs num_simulated_paths >= world size ({K} < {ws})")
        shard = _EngineShard(self, spec, norm, version, S, A, hi - lo)
        return self._publish(*cem_multi_rank(shard, state, mu0, sd0, self.iterations, min(self.n_elite, K), self.alpha,
                                             seed, lo, hi, K, A, spec.model == "reward", self._group))

    def _publish(self, cost, pos, first, mu, sd):
        self._mu = mu
        self.last_mu, self.last_sigma = mu, sd
        self.last_cost, self.last_position = cost, pos
        return first

    def _call_proposals(self, eng, states, mu0, sd0, seed, src):
        return eng.cem_get_actions(states, mu0, sd0, self.iterations, min(self.n_elite, eng.num_paths // states.shape[0]),
                                   self.alpha, seed, return_costs=True, proposals=src, **self._sampling_args())

    def _publish_proposals(self, eng, out, K, single: bool):
        res, mu, sd = out
        if single:
            self._note_planner_value(eng, int(res.best_index[0]), K)
            return self._publish(float(res.best_cost[0]), int(res.best_index[0]), res.first_action[0].copy(), mu[0], sd[0])
        self._note_planner_value(eng, res.best_index, K)
        self._store_plans(mu)
        self.last_mu, self.last_sigma = mu, sd
        self.last_cost, self.last_position = res.best_cost, res.best_index
        return res.first_action

    def _solve_batch(self, eng, states, mu0, sd0, seed, K):
        res, mu, sd = eng.cem_get_actions(states, mu0, sd0, self.iterations, min(self.n_elite, K), self.alpha, seed,
                                          **self._sampling_args(), **self._knot_args())
        self._note_planner_value(eng, res.best_index, K)
        self._store_plans(mu)
        self.last_mu, self.last_sigma = mu, sd
        self.last_cost, self.last_position = res.best_cost, res.best_index
        return res.first_action


class _EngineShard:
    """This rank's engine behind the tensor-level interface cem_multi_rank drives
    (tests substitute a NumPy double with the same methods)."""

    def __init__(self, ctrl: CEMcontroller, spec, norm, version, S, A, k_local):
        import torch
        self.eng = ctrl._engine_for(spec, S, A, k_local)
        self.eng.set_weights(spec, norm, version)
        self.device = torch.device("cuda", self.eng.device)

    def stream(self) -> int:
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def rollout(self, d_state, d_mu, d_sigma, seed, it, lo, k_global, d_costs, d_res, merge):
        self.eng.cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sigma.data_ptr(), seed, it, lo, k_global,
                                   d_costs.data_ptr(), d_res.data_ptr(), merge, self.stream())

    def check_status(self):
        self.eng.check_status()

    def select(self, d_pairs, d_costs, m, index_base, n_elite, d_out, d_count):
        self.eng.select_async(d_pairs.data_ptr() if d_pairs is not None else None,
                              d_costs.data_ptr() if d_costs is not None else None, m, index_base, n_elite,
                              d_out.data_ptr(), d_count.data_ptr(), self.stream())

    def refit(self, d_elite, d_count, seed, it, alpha, d_mu, d_sigma):
        self.eng.cem_refit_async(d_elite.data_ptr(), d_count.data_ptr(), seed, it, alpha, d_mu.data_ptr(),
                                 d_sigma.data_ptr(), self.stream())


def cem_multi_rank(shard, state, mu0, sd0, iterations, n_elite, alpha, seed, lo, hi, k_global, A, maximize,
                   group=None):
    """The multi-rank CEM loop (one RCCL all-gather of E (cost, index) records per
    iteration + one final min-loc); every rank owns >= 1 candidate.  Returns
    (objective, position, first_action, mu, sigma), identical on every rank."""
    import torch
    import torch.distributed as dist
    rank, ws = _dist.world(group)
    backend = dist.get_backend(group)
    dev = shard.device
    comm_dev = dev if backend == "nccl" else torch.device("cpu")
    k_local = hi - lo
    f64 = dict(dtype=torch.float64, device=dev)
    d_state = torch.from_numpy(np.ascontiguousarray(state, dtype=np.float64)).to(dev)
    d_mu = torch.from_numpy(np.ascontiguousarray(mu0, dtype=np.float64)).to(dev)
    d_sigma = torch.from_numpy(np.ascontiguousarray(sd0, dtype=np.float64)).to(dev)
    d_costs = torch.empty(max(1, k_local), **f64)
    d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    nbytes = n_elite * _ELITE_BYTES
    d_local = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    d_gath = torch.empty(ws * nbytes, dtype=torch.uint8, device=dev)
    d_elite = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d_gcount = torch.zeros(1, dtype=torch.int32, device=dev)
    for it in range(iterations):
        shard.rollout(d_state, d_mu, d_sigma, seed, it, lo, k_global, d_costs, d_res, it > 0)
        shard.select(None, d_costs, k_local, lo, n_elite, d_local, d_count)
        send = d_local.to(comm_dev)
        recv = torch.empty(ws * nbytes, dtype=torch.uint8, device=comm_dev)
        dist.all_gather_into_tensor(recv, send, group=group)          # ws x E records, rank order
        d_gath.copy_(recv.to(dev))
        shard.select(d_gath, None, ws * n_elite, 0, n_elite, d_elite, d_gcount)
        shard.refit(d_elite, d_gcount, seed, it, alpha, d_mu, d_sigma)
    raw = d_res.cpu().numpy()
    if hasattr(shard, "check_status"):                 # a team-kernel launch that gave up raises here
        shard.check_status()
    best_i = int(raw[:8].view(np.int64)[0])
    best_c = float(raw[8:16].view(np.float64)[0])
    first = raw[16:16 + 8 * A].view(np.float64).copy()
    sign = -1.0 if maximize else 1.0
    cost, pos, first_g = _dist.allgather_minloc(True, sign * best_c, best_i, first, A, group)
    return sign * cost, pos, first_g, d_mu.cpu().numpy(), d_sigma.cpu().numpy()

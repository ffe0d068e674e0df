"""Proposals: given action sequences in every iteration's population of the CEM and MPPI planners.

This module IS the definition: pure NumPy float64, which the device sampler
(csrc/plan_prop.hip) matches bit for bit -- as ``sampling.py`` and ``mppi_update.py`` define their kernels.

A call may carry ``P >= 1`` proposals per environment, each an action sequence ``[H, A]``.  In EVERY iteration of
the call, an environment's population ``[H, K, A]`` is the population the call would have had with its LAST ``P``
columns replaced: column ``K - P + p`` at step ``h`` and dimension ``j`` is

    v = proposals[p][h][j];   v < low[j] ? low[j] : (v > high[j] ? high[j] : v)

* the samplers' own clip expression (csrc/plan_noise.hip), written with ``np.where``: ``np.clip`` answers
  ``0.0`` for ``-0.0`` against a bound of ``0.0``, the expression keeps ``-0.0``; a NaN stays NaN (last in
  ``select``, no weight in MPPI), ``+-inf`` becomes the bound;
* carried elites (``keep_elites``) keep the FIRST columns, so ``P + n_elite <= K`` with them and ``P <= K``
  otherwise; ``P == K`` is legal and samples nothing;
* the replaced columns' own Philox draws are simply unused: no index shifts, every other column holds the bits it
  holds without proposals;
* everything downstream reads the stored array, as under ``noise_rho``: the argmin record, ``select``, the CEM
  refit, ``plan_keep``, the MPPI update, the control cost and the sigma update.  ``best_index = iteration * K +
  column`` may therefore name a proposal column; its first action is the stored (clipped) one;
* in MPPI a proposal is not a draw from ``N(mu, sigma)``: its softmin weight and its control-cost term (with
  ``eps = a - mu``) are the heuristic TD-MPC uses for its policy trajectories;
* nothing is carried between calls.

Sources of proposals: a caller's own sequences (``proposals=`` on the engines' and controllers' calls -- the
previous step's elites shifted by one step, a hand-written gait, another planner's answer) and closed-loop rollouts
of a policy net on the device (``policy_prior=`` on ``CEMcontroller`` / ``MPPIcontroller``).
"""
from __future__ import annotations

import numpy as np


def clip(v, low, high) -> np.ndarray:
    """``v < low ? low : (v > high ? high : v)`` over the last axis: the samplers' clip.  NaN stays NaN and a
    ``-0.0`` equal to a bound stays ``-0.0``."""
    v = np.asarray(v, dtype=np.float64)
    low = np.asarray(low, dtype=np.float64)
    high = np.asarray(high, dtype=np.float64)
    return np.where(v < low, low, np.where(v > high, high, v))


def check_count(P: int, K: int, n_elite: int = 0) -> int:
    """``P`` proposals fit ``K`` candidates per environment next to ``n_elite`` carried elites, or ValueError."""
    P, K, n_elite = int(P), int(K), int(n_elite)
    if P < 1:
        raise ValueError(f"proposals: at least one sequence is needed, got {P}")
    if P + n_elite > K:
        if n_elite:
            raise ValueError(f"proposals: {P} sequences + {n_elite} carried elites do not fit {K} candidates "
                             "(the carried elites keep the first columns)")
        raise ValueError(f"proposals: {P} sequences do not fit {K} candidates per environment")
    return P


def as_sequences(proposals, H: int, A: int, n_envs=None) -> np.ndarray:
    """A call's ``proposals=`` as the canonical C-contiguous float64 ``[P, H, A]`` (``n_envs`` None) or
    ``[n_envs, P, H, A]``, or ValueError.  The values are not looked at: NaN and out-of-box entries are legal."""
    p = np.ascontiguousarray(proposals, dtype=np.float64)
    want = "[P, H, A]" if n_envs is None else "[B, P, H, A]"
    if p.ndim != (3 if n_envs is None else 4) or p.shape[-2:] != (int(H), int(A)) or p.shape[-3] < 1:
        raise ValueError(f"proposals shape {p.shape} != {want} with P >= 1, H = {H}, A = {A}")
    if n_envs is not None and p.shape[0] != int(n_envs):
        raise ValueError(f"proposals are for {p.shape[0]} environments, states for {n_envs}")
    return p


def inject(actions, proposals, low, high, n_elite: int = 0) -> np.ndarray:
    """One environment's population ``[H, K, A]`` with its last ``P`` columns replaced by the clipped
    ``proposals`` ``[P, H, A]``; every other column keeps its bits.  ``n_elite``: the carried elites in front."""
    actions = np.asarray(actions, dtype=np.float64)
    prop = np.asarray(proposals, dtype=np.float64)
    if actions.ndim != 3 or prop.ndim != 3 or prop.shape[1:] != (actions.shape[0], actions.shape[2]):
        raise ValueError(f"proposals shape {prop.shape} != [P, H, A] of the population {actions.shape} = [H, K, A]")
    K = actions.shape[1]
    P = check_count(prop.shape[0], K, n_elite)
    out = actions.copy()
    out[:, K - P:, :] = clip(prop, low, high).transpose(1, 0, 2)
    return out


def inject_batch(actions, proposals, low, high, n_envs: int, n_elite: int = 0) -> np.ndarray:
    """``inject`` per environment on the batched array ``[H, n_envs * K, A]`` (environment ``b`` owns columns
    ``[b * K, (b + 1) * K)``) with ``proposals`` ``[n_envs, P, H, A]``."""
    actions = np.asarray(actions, dtype=np.float64)
    B = int(n_envs)
    if actions.ndim != 3 or B < 1 or actions.shape[1] % B != 0:
        raise ValueError(f"actions shape {actions.shape} != [H, n_envs * K, A] with n_envs = {n_envs}")
    K = actions.shape[1] // B
    prop = as_sequences(proposals, actions.shape[0], actions.shape[2], B)
    out = actions.copy()
    for b in range(B):
        out[:, b * K:(b + 1) * K, :] = inject(actions[:, b * K:(b + 1) * K, :], prop[b], low, high, n_elite)
    return out


def canonical_strides(P: int, H: int, A: int) -> tuple:
    """``(env_stride, seq_stride, step_stride)`` in doubles of ``[n_envs, P, H, A]``."""
    return int(P) * int(H) * int(A), int(H) * int(A), int(A)


def policy_strides(n_envs: int, P: int, A: int) -> tuple:
    """... and of the policy engines' output ``[H, n_envs * P, A]``, environment ``b`` owning columns
    ``[b * P, (b + 1) * P)`` (``RolloutEngine.rollout_policy_batch_async``)."""
    return int(P) * int(A), int(A), int(n_envs) * int(P) * int(A)


def check_strides(n_envs: int, P: int, H: int, A: int, env_stride: int, seq_stride: int, step_stride: int) -> None:
    """The library's rule for a device source, or ValueError: strides >= 0 and, from the smallest to the largest
    over the dimensions of extent > 1, each at least the extent it steps over -- no two elements alias."""
    dims = sorted([(int(env_stride), int(n_envs)), (int(seq_stride), int(P)), (int(step_stride), int(H))])
    if dims[0][0] < 0:
        raise ValueError("proposals: the strides must be >= 0")
    below = int(A)
    for stride, extent in dims:
        if extent <= 1:
            continue
        if stride < below:
            raise ValueError("proposals: the strides alias (two elements share an address)")
        below = stride * extent

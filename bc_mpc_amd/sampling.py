"""What the CEM and MPPI planners sample: temporally correlated noise and the CEM elite carry-over.

This module IS the definition: pure NumPy float64 arithmetic, one rounded IEEE operation per
step, which the device kernels (csrc/plan_noise.hip, and the refit / MPPI update reading the stored action
array) match bit for bit -- as ``ensemble.combine`` and ``TermCost.__call__`` define their kernels.  It draws
nothing itself: the independent normals ``z`` are the planners' Irwin-Hall draws, one per
``(candidate, h, j, iteration)`` (csrc/device_common.h ``cem_normal``), handed in as ``[H, K, A]``.

* ``ar1_noise``: ``n[0] = z[0]``, ``n[h] = rho * n[h-1] + sqrt(1 - rho^2) * z[h]``.  A first-order
  autoregression over the horizon with stationary variance 1, so ``sigma`` keeps its meaning; ``rho = 0`` is the
  independent draw.  White noise averages out in the state over a long horizon; correlated noise moves it.
* ``carry_elites``: iteration ``it >= 1`` of an environment starts with ALL elites of iteration ``it - 1``, so
  the best sequence found so far is never lost and the per-iteration best cost cannot rise.
* ``refit_from_actions``: the CEM refit's statistics on given elite actions, in the device's summation order.

Not built: power-law (FFT) noise, carrying a fraction of the elites, ensembles and more than one rank.  The
library itself carries no elites from one control step to the next; a caller who keeps them passes them (shifted)
as ``proposals=`` of the next call (proposals.py).  (MPPI's control-cost term: mppi_update.py; sampling the
sequence at fewer knots than steps, where the recursion runs over the knots: knots.py.)
"""
from __future__ import annotations

import math

import numpy as np


def check_rho(rho) -> float:
    """``rho`` as a float in ``[0, 1)``, or ValueError."""
    try:
        r = float(rho)
    except (TypeError, ValueError):
        raise ValueError(f"noise rho must be a number in [0, 1), got {rho!r}") from None
    if not (math.isfinite(r) and 0.0 <= r < 1.0):
        raise ValueError(f"noise rho must be finite and in [0, 1), got {rho!r}")
    return r


def check_keep_elites(keep_elites) -> bool:
    """``keep_elites`` as a bool (True / False / 0 / 1), or ValueError."""
    if isinstance(keep_elites, (bool, np.bool_)) or (isinstance(keep_elites, (int, np.integer))
                                                    and int(keep_elites) in (0, 1)):
        return bool(keep_elites)
    raise ValueError(f"keep_elites must be True or False, got {keep_elites!r}")


def ar1_noise(z, rho) -> np.ndarray:
    """The correlated normals of independent ones: ``z`` is ``[H, ...]`` float64 (``oracle.cem_normals``'
    layout ``[H, K, A]``), the recursion runs over axis 0.  ``c = sqrt(1 - rho*rho)`` is rounded once;
    every step is two products and one sum, each rounded on its own (no FMA).  ``rho == 0`` and ``H == 1``
    return ``z``'s bits."""
    rho = check_rho(rho)
    z = np.asarray(z, dtype=np.float64)
    c = math.sqrt(1.0 - rho * rho)
    n = np.empty_like(z)
    if z.shape[0] == 0:
        return n
    n[0] = z[0]
    for h in range(1, z.shape[0]):
        n[h] = rho * n[h - 1] + c * z[h]
    return n


def correlated_actions(z, rho, mu, sigma, low, high) -> np.ndarray:
    """``clip(mu + sigma * ar1_noise(z, rho), low, high)`` as ``[H, K, A]``: ``z`` ``[H, K, A]``, ``mu`` /
    ``sigma`` ``[H, A]``, the planners' product, sum and np.clip (csrc/device_common.h ``cem_action``)."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    n = ar1_noise(z, rho)
    return np.clip(mu[:, None, :] + sigma[:, None, :] * n, np.asarray(low, np.float64), np.asarray(high, np.float64))


def carry_elites(actions, prev_actions, elite_cols) -> np.ndarray:
    """One environment's population ``[H, K, A]`` at iteration ``it >= 1`` with carry-over: column ``j < n =
    len(elite_cols)`` is ``prev_actions[:, elite_cols[j], :]`` -- the previous iteration's population and its
    elites' columns in select's output order, ascending candidate index -- and column ``j >= n`` is
    ``actions[:, j, :]``, that candidate's own sample.  Iteration 0 carries nothing (``elite_cols`` empty)."""
    actions = np.asarray(actions, dtype=np.float64)
    prev_actions = np.asarray(prev_actions, dtype=np.float64)
    cols = np.asarray(elite_cols, dtype=np.int64).reshape(-1)
    if cols.size > actions.shape[1]:
        raise ValueError(f"{cols.size} elites do not fit {actions.shape[1]} candidates")
    out = actions.copy()
    out[:, :cols.size, :] = prev_actions[:, cols, :]
    return out


def _wave_sum(x: np.ndarray) -> float:
    """Lane l of 64 adds elements l, l + 64, ... in order from 0.0; the 64 partials are combined by the xor
    butterfly, offsets 32, 16, .., 1 (csrc/cem_common.h ``refit_wave``)."""
    p = np.zeros(64, dtype=np.float64)
    for start in range(0, x.shape[0], 64):
        chunk = x[start:start + 64]
        p[:chunk.shape[0]] = p[:chunk.shape[0]] + chunk
    off = 32
    while off >= 1:
        p = p[:off] + p[off:2 * off]
        off //= 2
    return float(p[0])


def refit_from_actions(elite_actions, mu, sigma, alpha: float):
    """The CEM refit on given elite actions ``[n, H, A]`` (elites in ascending candidate index): per ``(h, j)``
    the mean and the standard deviation (ddof 0, two passes) in the device's summation order, smoothed as
    ``alpha * old + (1 - alpha) * stat``.  Returns ``(mu', sigma')``; no elite: the distribution unchanged."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    acts = np.asarray(elite_actions, dtype=np.float64)
    n = acts.shape[0]
    if n == 0:
        return mu.copy(), sigma.copy()
    H, A = mu.shape
    if acts.shape != (n, H, A):
        raise ValueError(f"elite_actions shape {acts.shape} != (n, H, A) = {(n, H, A)}")
    new_mu, new_sd = np.empty_like(mu), np.empty_like(sigma)
    beta = 1.0 - alpha
    for h in range(H):
        for j in range(A):
            a = acts[:, h, j]
            mean = _wave_sum(a) / float(n)
            d = a - mean
            sd = np.sqrt(_wave_sum(d * d) / float(n))
            new_mu[h, j] = alpha * mu[h, j] + beta * mean
            new_sd[h, j] = alpha * sigma[h, j] + beta * sd
    return new_mu, new_sd

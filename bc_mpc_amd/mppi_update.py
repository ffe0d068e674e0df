"""What the MPPI update adds to the rollout cost and how it moves sigma: the control-cost term of
information-theoretic MPC (Williams et al.) and the weighted standard deviation with a floor that TD-MPC- and
PETS-style planners use.

This module IS the definition: pure NumPy float64 arithmetic, one rounded IEEE operation per
step, no FMA, which the device kernels (csrc/mppi_ext.hip) match -- the control cost and the smoothing step bit
for bit, the weighted sums in the device's order -- as ``sampling.py`` defines its kernels.  The oracle is never
imported here.

One MPPI round with the options on (``mu``, ``sigma``: the plan the round sampled from):

1. sample, roll out, take the record: the argmin runs over the RAW costs, so ``best_cost``, ``best_index``, the
   returned costs and ``last_cost`` never contain the control cost;
2. ``c~ = augmented(costs, control_cost(actions, mu, sigma), weight, maximize)``;
3. the softmin update runs on ``c~`` instead of the costs: ``mu'`` and the statistics are the plain update's on
   that vector, so ``stats.min_cost`` is the minimum AUGMENTED score;
4. with ``adapt_sigma``: ``sigma' = sigma_step(sigma, weighted_sigma(w, actions, mu'), alpha, min_std, max_std)``
   with the update's own weights ``w``; no valid candidate: sigma stays, as mu does.  The next round samples
   from ``(mu', sigma')``.

``control_cost`` is the textbook ``u^T Sigma^-1 eps`` with ``u = mu`` and ``eps`` the CLIPPED action minus the
mean it was drawn around.  With correlated noise (``noise_rho != 0``) it is the diagonal form of ``Sigma^-1``:
every (h, j) is weighted by its marginal variance ``sigma[h, j]^2``, which the AR(1) recursion keeps, and the
correlation between steps is ignored.

Not built: elite-restricted (top-k) weights, the full (non-diagonal) ``Sigma^-1`` under correlated noise, a sigma
carried from one control step to the next, ensembles and more than one rank.
"""
from __future__ import annotations

import math

import numpy as np

# csrc/kernels.h: kMppiSmall, kMppiMaxCpl -- a stage-1 workgroup owns 64 candidates up to SMALL, 256 beyond
SMALL, MAX_CPL = 16384, 4


def check_options(control_cost=0.0, adapt_sigma=False, sigma_alpha=0.0, min_std=0.0, max_std=None,
                  temperature=None):
    """The options as ``(weight, adapt, alpha, min_std, max_std)`` -- floats, a bool, ``max_std`` ``inf`` for
    None -- or ValueError.  ``control_cost=True`` is the textbook weight, the temperature; False is 0."""
    if isinstance(control_cost, (bool, np.bool_)):
        if control_cost and temperature is None:
            raise ValueError("control_cost=True means the temperature: none was given")
        control_cost = float(temperature) if control_cost else 0.0
    try:
        weight = float(control_cost)
    except (TypeError, ValueError):
        raise ValueError(f"control_cost must be a number >= 0 or True, got {control_cost!r}") from None
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"control_cost must be finite and >= 0, got {control_cost!r}")
    if not (isinstance(adapt_sigma, (bool, np.bool_)) or (isinstance(adapt_sigma, (int, np.integer))
                                                          and int(adapt_sigma) in (0, 1))):
        raise ValueError(f"adapt_sigma must be True or False, got {adapt_sigma!r}")
    try:
        alpha, lo = float(sigma_alpha), float(min_std)
        hi = math.inf if max_std is None else float(max_std)
    except (TypeError, ValueError):
        raise ValueError("sigma_alpha, min_std and max_std must be numbers") from None
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"sigma_alpha must be in [0, 1], got {sigma_alpha!r}")
    if not (math.isfinite(lo) and lo >= 0.0):
        raise ValueError(f"min_std must be finite and >= 0, got {min_std!r}")
    if not hi >= lo:
        raise ValueError(f"max_std must be >= min_std ({lo}), got {max_std!r}")
    return weight, bool(adapt_sigma), alpha, lo, hi


def control_gain(mu, sigma) -> np.ndarray:
    """``g = mu / (sigma * sigma)`` per (h, j): one product, then one division; 0.0 where ``sigma == 0`` (that
    dimension has no noise)."""
    mu = np.asarray(mu, dtype=np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    var = sigma * sigma
    g = np.zeros_like(mu)
    np.divide(mu, var, out=g, where=sigma != 0.0)
    return g


def control_cost(actions, mu, sigma) -> np.ndarray:
    """``q[k] = sum_h sum_j g[h, j] * (actions[h, k, j] - mu[h, j])``: from 0.0, ``h`` ascending and inside it
    ``j`` ascending, every difference, product and sum rounded on its own.  ``actions`` ``[H, K, A]`` are the
    clipped sampled actions, ``mu`` / ``sigma`` ``[H, A]`` the plan they were sampled from.  Under correlated
    noise this is the diagonal (marginal-variance) form of ``Sigma^-1`` (module docstring)."""
    actions = np.asarray(actions, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    H, K, A = actions.shape
    if mu.shape != (H, A) or np.shape(sigma) != (H, A):
        raise ValueError(f"mu / sigma shapes {mu.shape} / {np.shape(sigma)} != (H, A) = {(H, A)}")
    g = control_gain(mu, sigma)
    q = np.zeros(K, dtype=np.float64)
    for h in range(H):
        for j in range(A):
            q = q + g[h, j] * (actions[h, :, j] - mu[h, j])
    return q


def augmented(costs, q, weight: float, maximize: bool = False) -> np.ndarray:
    """``costs + weight * q`` on a cost engine, ``costs - weight * q`` on a learned-reward engine (the score
    ``-c~`` then rises with ``q``): one product, one sum.  A NaN or +-inf cost stays NaN or +-inf."""
    costs = np.asarray(costs, dtype=np.float64)
    wq = np.float64(weight) * np.asarray(q, dtype=np.float64)
    return costs - wq if maximize else costs + wq


def softmin_weights(scores, lam: float, maximize: bool = False) -> np.ndarray:
    """The update's weights of a cost (score) vector: ``exp(-((v - v_min) / lam))`` for a finite ``v = +-score``,
    0.0 for any other (the device's exp is its math library's, NumPy's is the host's)."""
    c = np.asarray(scores, dtype=np.float64)
    v = -c if maximize else c
    ok = np.isfinite(v)
    w = np.zeros(v.shape[0], dtype=np.float64)
    if ok.any():
        w[ok] = np.exp(-((v[ok] - v[ok].min()) / lam))
    return w


def cpl(K: int) -> int:
    """Candidates per lane of a stage-1 workgroup (csrc/mppi.hip ``mppi_cpl``)."""
    return MAX_CPL if K > SMALL else 1


def _butterfly(p: np.ndarray) -> np.ndarray:
    """The xor butterfly over axis 0 (64 lanes), offsets 32, 16, .., 1."""
    off = 32
    while off >= 1:
        p = p[:off] + p[off:2 * off]
        off //= 2
    return p[0]


def two_stage_sum(x) -> np.ndarray:
    """``sum_k x[k]`` over axis 0 in the device's order, a function of K alone: workgroup ``b`` owns the
    ``C = 64 * cpl(K)`` entries from ``b * C``, its lane ``l`` adds entries ``l, l + 64, ..`` from 0.0 and the 64
    lane sums are combined by the xor butterfly; then lane ``l`` adds the workgroups' partials ``l, l + 64, ..``
    and the butterfly again (csrc/mppi_common.h, csrc/mppi_ext.hip)."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    C = 64 * cpl(K)
    P = (K + C - 1) // C
    pad = np.zeros((P * C,) + x.shape[1:], dtype=np.float64)
    pad[:K] = x
    pad = pad.reshape((P, C // 64, 64) + x.shape[1:])
    lanes = np.zeros((P, 64) + x.shape[1:], dtype=np.float64)
    for i in range(C // 64):
        lanes = lanes + pad[:, i]
    parts = _butterfly(np.moveaxis(lanes, 1, 0))                # [P, ...]
    acc = np.zeros((64,) + x.shape[1:], dtype=np.float64)
    for start in range(0, P, 64):
        chunk = parts[start:start + 64]
        acc[:chunk.shape[0]] = acc[:chunk.shape[0]] + chunk
    return _butterfly(acc)


def weighted_sigma(w, actions, mu_new) -> np.ndarray:
    """``s[h, j] = sqrt(sum_k w[k] (actions[h, k, j] - mu_new[h, j])^2 / sum_k w[k])``: the second of two passes,
    about the UPDATED mean (the first pass is the update's weighted mean), like the CEM refit's two-pass
    standard deviation.  Per term one difference and two products (``d * d``, then ``w *``), the sums in
    ``two_stage_sum``'s order, one division, one square root.  ``w`` ``[K]``, ``actions`` ``[H, K, A]``."""
    w = np.asarray(w, dtype=np.float64)
    actions = np.asarray(actions, dtype=np.float64)
    mu_new = np.asarray(mu_new, dtype=np.float64)
    H, K, A = actions.shape
    if w.shape != (K,) or mu_new.shape != (H, A):
        raise ValueError(f"w / mu_new shapes {w.shape} / {mu_new.shape} != (K,) / (H, A) = {(K,)} / {(H, A)}")
    d = actions - mu_new[:, None, :]
    t = w[None, :, None] * (d * d)
    V = two_stage_sum(np.moveaxis(t, 1, 0))                     # [H, A]
    W = two_stage_sum(w)
    return np.sqrt(V / W)


def sigma_step(sigma_old, s, alpha: float, min_std: float = 0.0, max_std: float = math.inf) -> np.ndarray:
    """``min(max(alpha * sigma_old + (1 - alpha) * s, min_std), max_std)``: ``1 - alpha`` rounded once, two
    products, one sum, then the clamp.  ``alpha = 1`` and no clamp return ``sigma_old``'s bits."""
    sigma_old = np.asarray(sigma_old, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    beta = 1.0 - float(alpha)
    x = float(alpha) * sigma_old + beta * s
    return np.minimum(np.maximum(x, float(min_std)), float(max_std))

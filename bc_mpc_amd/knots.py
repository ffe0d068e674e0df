"""Knot plans for the CEM and MPPI planners: sample the action sequence at ``M <= H`` knots, interpolate to ``H`` steps.

This module IS the definition, as ``sampling.py`` is for 9j: pure NumPy float64 arithmetic, one
rounded IEEE operation per step and no FMA, which the device kernel (csrc/plan_knots.hip ``plan_sample_knots``)
matches bit for bit.  The planners then search ``M * A`` dimensions instead of ``H * A``; every candidate is smooth
by construction and the plan a controller carries between steps is ``[M, A]``.

* ``knot_values``: the knots of a population, ``sampling.correlated_actions`` over the knot axis -- the planners'
  own normals with the knot index in the place of ``h`` (``oracle.cem_normals(seed, it, off, K, M, A)``), the AR(1)
  recursion over knots, clipped to the box.  The refit and the MPPI updates read these clipped values.
* ``expand``: the ``[H, ...]`` action sequence of ``[M, ...]`` knots, every value clipped to the box.
    hold    step h takes knot ``(h * M) // H`` (action repeat; spans differ by at most one step).
    linear  the knots sit at both ends of the horizon.  ``m0, r = divmod(h * (M - 1), H - 1)`` (``m0 = r = 0`` when
            ``H == 1`` or ``M == 1``); ``r == 0`` gives ``theta[m0]`` untouched, else with ``f = float(r) /
            float(H - 1)`` (one division), ``p1 = theta[m0]``, ``p2 = theta[m0 + 1]``: ``p1 + f * (p2 - p1)``.
    cubic   Catmull-Rom on the same ``m0, r, f`` with the end knots repeated, ``p0 = theta[max(m0 - 1, 0)]``,
            ``p3 = theta[min(m0 + 2, M - 1)]``:
                a = p2 - p0
                b = ((2 * p0 - 5 * p1) + 4 * p2) - p3
                c = (3 * (p1 - p2) + p3) - p0
                v = p1 + 0.5 * (f * (a + f * (b + f * c)))
            in exactly this operation order.  It overshoots (about 3 values in 100 leave a +-1 box before the clip).
  ``M == H`` returns ``theta``'s bits, ``M == 1`` repeats knot 0, and a knot that falls on a step is returned bit
  for bit (knots inside the box).
* ``shift_plan``: the warm start, host only -- the ``[M, A]`` plan one control step later.
* ``expand_plan``: the ``[H, A]`` view of a knot plan.

Not built: knots for proposals and the policy prior (a given sequence has no knot representation to refit on),
ensembles, more than one rank, non-uniform knot spacing, B-splines.
"""
from __future__ import annotations

import numpy as np

from . import sampling as _sampling

KINDS = ("hold", "linear", "cubic")     # bcmpc_knots.kind 0, 1, 2


def check_knots(knots, H):
    """``knots`` as an int in ``[1, H]``, or None (the feature is off); ValueError otherwise."""
    if knots is None:
        return None
    if isinstance(knots, (bool, np.bool_)) or not isinstance(knots, (int, np.integer)):
        raise ValueError(f"knots must be None or an integer in [1, horizon], got {knots!r}")
    if not 1 <= int(knots) <= int(H):
        raise ValueError(f"knots must be in [1, horizon = {int(H)}], got {knots!r}")
    return int(knots)


def check_interp(kind) -> str:
    """``kind`` as one of ``"hold" | "linear" | "cubic"``, or ValueError."""
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError(f"knot_interp must be one of {KINDS}, got {kind!r}")
    return kind


def knot_values(z, rho, mu, sigma, low, high) -> np.ndarray:
    """The population's knots ``[M, K, A]``: ``z`` ``[M, K, A]`` independent normals (knot index in the place of
    ``h``), ``mu`` / ``sigma`` ``[M, A]``; AR(1) over the knot axis, clipped to the box."""
    return _sampling.correlated_actions(z, rho, mu, sigma, low, high)


def _clip(v, low, high):
    """The samplers' clip, ``v < low ? low : (v > high ? high : v)``; no bounds: ``v``."""
    if low is None and high is None:
        return v
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    return np.where(v < low, low, np.where(v > high, high, v))


def _segment(num: int, H: int, M: int):
    """``(m0, r)`` of the knot coordinate ``num / (H - 1)``; ``(0, 0)`` when ``H == 1`` or ``M == 1``."""
    if H == 1 or M == 1:
        return 0, 0
    return divmod(num, H - 1)


def _interp(theta, m0: int, r: int, H: int, kind: str):
    """The linear / cubic interpolant of the knots ``theta`` ``[M, ...]`` at knot coordinate ``m0 + r / (H - 1)``."""
    if r == 0:
        return theta[m0]
    M = theta.shape[0]
    f = float(r) / float(H - 1)
    p1, p2 = theta[m0], theta[m0 + 1]
    if kind == "linear":
        return p1 + f * (p2 - p1)
    p0, p3 = theta[max(m0 - 1, 0)], theta[min(m0 + 2, M - 1)]
    a = p2 - p0
    b = ((2.0 * p0 - 5.0 * p1) + 4.0 * p2) - p3
    c = (3.0 * (p1 - p2) + p3) - p0
    return p1 + 0.5 * (f * (a + f * (b + f * c)))


def expand(theta, H: int, kind: str, low=None, high=None) -> np.ndarray:
    """``[H, ...]`` from the knots ``theta`` ``[M, ...]`` (module docstring), every value clipped to ``low`` /
    ``high`` (broadcast against the trailing axes; both None: no clip)."""
    kind = check_interp(kind)
    theta = np.asarray(theta, dtype=np.float64)
    H = int(H)
    M = check_knots(int(theta.shape[0]), H)
    out = np.empty((H,) + theta.shape[1:], dtype=np.float64)
    for h in range(H):
        if kind == "hold":
            out[h] = theta[(h * M) // H]
        else:
            m0, r = _segment(h * (M - 1), H, M)
            out[h] = _interp(theta, m0, r, H, kind)
    return _clip(out, low, high)


def expand_plan(mu, H: int, kind: str, low=None, high=None) -> np.ndarray:
    """The ``[H, A]`` view of the knot plan ``mu`` ``[M, A]``."""
    return expand(mu, H, kind, low, high)


def shift_plan(mu, H: int, kind: str, fill) -> np.ndarray:
    """The warm start: the plan ``mu`` ``[M, A]`` one control step later, ``[M, A]``; ``fill`` ``[A]`` (the box
    centre) where the old plan has ended.  linear / cubic: knot m sits at step ``t_m = m (H - 1) / (M - 1)`` and
    ``mu'[m]`` is the old interpolant at ``t_m + 1`` -- ``m0, r = divmod(m * (H - 1) + (M - 1), H - 1)``, the
    formulas of ``expand`` without the clip -- or ``fill`` where ``t_m + 1 > H - 1``.  hold: knot m's first step
    is ``h_m = ceil(m * H / M)`` and ``mu'[m] = mu[((h_m + 1) * M) // H]``, or ``fill`` where ``h_m + 1 > H - 1``.
    ``M == H``: ``vstack([mu[1:], fill])``; ``H == 1``: ``fill``."""
    kind = check_interp(kind)
    mu = np.asarray(mu, dtype=np.float64)
    H = int(H)
    M = check_knots(int(mu.shape[0]), H)
    fill = np.asarray(fill, dtype=np.float64)
    out = np.empty_like(mu)
    for m in range(M):
        if kind == "hold":
            h1 = -((-m * H) // M) + 1
            out[m] = mu[(h1 * M) // H] if h1 <= H - 1 else fill
        elif M == 1:
            out[m] = mu[0] if 1 <= H - 1 else fill
        else:
            num = m * (H - 1) + (M - 1)
            if num > (H - 1) * (M - 1):
                out[m] = fill
            else:
                m0, r = divmod(num, H - 1)
                out[m] = _interp(mu, m0, r, H, kind)
    return out

"""Terminal value: the definition of what a planner adds to a candidate's cost after step H.

    total_k = cost_k + weight * float64(V(s_H[k]))

V is the critic the reference trains beside its policy (``ppo_bc_policy.MlpPolicy.build_network``,
ppo_bc_policy.py:56-64: scope ``pi/vf``, ``fc1..fcL`` tanh, ``final`` -> 1) over the same ``obfilter`` as the
policy head.  ``terminal_values`` below is THE definition, as ``TermCost.__call__`` is for cost terms and
``ensemble.combine`` for ensembles; csrc/terminal_value.hip is tested against it
(tests/test_gpu_terminal_value.py):

* ``x = states.astype(float32)`` (round to nearest), ``obz = np.clip((x - ob_mean) / ob_std, -5, 5)`` in f32:
  a NaN state dimension stays NaN (np.clip keeps NaN), +-inf clips to +-5.  The kernel's obz has these bits.
* ``h = tanh(h @ W + b)`` per hidden layer in f32, ``v = (h @ w_final + b_final)[:, 0]``.  A GPU f32 MLP
  cannot be bit-equal to BLAS; the accuracy bars are ``error_bound`` (per candidate, derived) and the RMS
  against ``terminal_values_seq32`` (strictly sequential f32 dot products), both measured against
  ``terminal_values_f64``.
* ``add_to_costs``: one rounded f64 multiply and one rounded f64 add, no contraction; with the termination steps
  of a ``TermCost`` with ``done`` only for the candidates that never terminated.

The controllers default ``weight`` to -1.0: a value is a return, a cost is minus a reward.  A discount is the
caller's: pass ``-gamma**H``.

``extract(container) -> (ValueSpec, version)`` mirrors ``policy.extract``: an object with ``value_spec()``, a
NumPy stand-in with ``.vf.kernels/.biases/.ob_mean/.ob_std``, or the reference's TF1 ``MlpPolicy`` through
``.sess`` (``pi/pi/vf/fc{i}/{kernel,bias}:0``, ``pi/pi/vf/final/...`` and the obfilter sums, with the mean /
std formulas of ``policy._tf_policy``).  The version is the container's integer ``version`` if it has one, else
a content digest.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

MAX_LAYERS = 4
MAX_HIDDEN = 256
MAX_STATE = 32
U32 = 2.0 ** -24                     # f32 unit roundoff
TANH_ULPS = 8.0                      # error_bound's allowance for one tanh, in units of U32 |tanh|


@dataclass(frozen=True)
class ValueSpec:
    """A tanh critic in TF layout: L hidden kernels [in, out] of width ``hidden`` (1 <= L <= 4,
    1 <= hidden <= 256), a last kernel [hidden, 1], and the observation filter's mean / std [S], all f32 and
    finite, ``ob_std`` > 0.  Anything else raises ValueError."""
    kernels: Sequence[np.ndarray]
    biases: Sequence[np.ndarray]
    ob_mean: np.ndarray
    ob_std: np.ndarray

    def __post_init__(self):
        def f32(a, what):
            a = np.asarray(a)
            if a.dtype == object or not np.issubdtype(a.dtype, np.number):
                raise ValueError(f"ValueSpec: {what} is not numeric")
            with np.errstate(over="ignore", invalid="ignore"):
                out = np.ascontiguousarray(a, dtype=np.float32)
            if not np.isfinite(out).all():
                raise ValueError(f"ValueSpec: {what} must be finite")
            return out
        try:
            ks, bs = list(self.kernels), list(self.biases)
        except TypeError:
            raise ValueError("ValueSpec: kernels and biases must be sequences of arrays") from None
        if len(ks) != len(bs) or not 2 <= len(ks) <= MAX_LAYERS + 1:
            raise ValueError(f"ValueSpec: need 1 <= L <= {MAX_LAYERS} hidden layers plus the final one "
                             f"(got {len(ks)} kernels, {len(bs)} biases)")
        ks = [f32(k, f"kernel {i}") for i, k in enumerate(ks)]
        bs = [f32(b, f"bias {i}").reshape(-1) for i, b in enumerate(bs)]
        mean, std = f32(self.ob_mean, "ob_mean").reshape(-1), f32(self.ob_std, "ob_std").reshape(-1)
        if any(k.ndim != 2 for k in ks):
            raise ValueError("ValueSpec: kernels must be [in, out] matrices")
        S, hidden = ks[0].shape
        if not 1 <= S <= MAX_STATE:
            raise ValueError(f"ValueSpec: state dim {S} outside [1, {MAX_STATE}]")
        if not 1 <= hidden <= MAX_HIDDEN:
            raise ValueError(f"ValueSpec: hidden {hidden} outside [1, {MAX_HIDDEN}]")
        for i, (k, b) in enumerate(zip(ks, bs)):
            want = (S if i == 0 else hidden, 1 if i == len(ks) - 1 else hidden)
            if k.shape != want or b.shape != (want[1],):
                raise ValueError(f"ValueSpec: layer {i} has kernel {k.shape} / bias {b.shape}, expected {want} / "
                                 f"({want[1]},)")
        if mean.shape != (S,) or std.shape != (S,):
            raise ValueError(f"ValueSpec: ob_mean / ob_std must have shape ({S},)")
        if not (std > 0).all():
            raise ValueError("ValueSpec: ob_std must be > 0")
        object.__setattr__(self, "kernels", tuple(ks))
        object.__setattr__(self, "biases", tuple(bs))
        object.__setattr__(self, "ob_mean", mean)
        object.__setattr__(self, "ob_std", std)

    @property
    def n_layers(self) -> int:
        return len(self.kernels) - 1

    @property
    def hidden(self) -> int:
        return int(self.kernels[0].shape[1])

    @property
    def state_dim(self) -> int:
        return int(self.kernels[0].shape[0])


def _states(spec: ValueSpec, states) -> np.ndarray:
    s = np.asarray(states, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != spec.state_dim:
        raise ValueError(f"states must be [K, {spec.state_dim}]")
    return s


def observe(spec: ValueSpec, states) -> np.ndarray:
    """obz [K, S] f32: the clipped, filtered observation (the definition's first two steps)."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = _states(spec, states).astype(np.float32)
        return np.clip((x - spec.ob_mean) / spec.ob_std, np.float32(-5), np.float32(5)).astype(np.float32)


def terminal_values(spec: ValueSpec, states) -> np.ndarray:
    """THE definition: f32[K] values of states [K, S] f64."""
    h = observe(spec, states)
    with np.errstate(invalid="ignore"):
        for W, b in zip(spec.kernels[:-1], spec.biases[:-1]):
            h = np.tanh(h @ W + b).astype(np.float32)
        return (h @ spec.kernels[-1] + spec.biases[-1])[:, 0].astype(np.float32)


def terminal_values_f64(spec: ValueSpec, obz32) -> np.ndarray:
    """The same net evaluated in f64 from the f32 obz: what the accuracy bars measure against."""
    h = np.asarray(obz32, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        for W, b in zip(spec.kernels[:-1], spec.biases[:-1]):
            h = np.tanh(h @ W.astype(np.float64) + b.astype(np.float64))
        return (h @ spec.kernels[-1].astype(np.float64) + spec.biases[-1].astype(np.float64))[:, 0]


def terminal_values_seq32(spec: ValueSpec, obz32) -> np.ndarray:
    """The f32 yardstick of the RMS bar: every dot product strictly sequential,
    acc = f32(acc + f32(x_k w_k)) in k order (a loop over k <= 256, vectorised over the candidates), bias added
    last, np.tanh in f32."""
    h = np.asarray(obz32, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for i, (W, b) in enumerate(zip(spec.kernels, spec.biases)):
            acc = np.zeros((h.shape[0], W.shape[1]), dtype=np.float32)
            for k in range(W.shape[0]):
                acc = acc + h[:, k:k + 1] * W[k][None, :]          # f32 multiply, f32 add: two roundings
            z = acc + b
            h = np.tanh(z).astype(np.float32) if i < len(spec.kernels) - 1 else z
    return h[:, 0].astype(np.float32)


def error_bound(spec: ValueSpec, obz32) -> np.ndarray:
    """E_k, the per-candidate bound of |v_f32 - v_f64|, evaluated in f64: the standard running error bound.

    u = 2^-24, gamma_m = m u / (1 - m u).  A layer with n inputs x (the f64 evaluation's) and input error
    e_in propagates

        e_out = |W|^T e_in + gamma_{n+1} (|W|^T |x| + |b|)

    (n products, n - 1 additions and the bias add: at most n + 1 roundings on any path of a dot product,
    whatever its order, fused or not).  tanh is 1-Lipschitz, so it passes e_out on, and adds 8 u |tanh|:
    8 ulp is twice the roughly 4 ulp DESIGN.md section 4 documents for the f32 kernels' tanh (tanh_fast
    against float64 tanh).  The input error is 0: obz is bit-identical on both sides."""
    h = np.asarray(obz32, dtype=np.float32).astype(np.float64)
    e = np.zeros_like(h)
    last = len(spec.kernels) - 1
    with np.errstate(invalid="ignore"):
        for i, (W, b) in enumerate(zip(spec.kernels, spec.biases)):
            W64, b64 = W.astype(np.float64), b.astype(np.float64)
            n = W.shape[0]
            g = (n + 1) * U32 / (1.0 - (n + 1) * U32)
            aW = np.abs(W64)
            e = e @ aW + g * (np.abs(h) @ aW + np.abs(b64))
            h = h @ W64 + b64
            if i < last:
                h = np.tanh(h)
                e = e + TANH_ULPS * U32 * np.abs(h)
    return e[:, 0]


def add_to_costs(costs, values, weight: float, term_step=None, horizon=None) -> np.ndarray:
    """total = cost + weight * float64(v): one rounded f64 multiply, one rounded f64 add.

    ``term_step`` (with ``horizon``; ``cost_functions.episode_cost``'s second result): the add is made only where
    ``term_step == horizon``, the candidates that never terminated.  A terminated episode has no future return:
    its total is left untouched -- not ``+ weight * 0``, which would turn a ``-0.0`` into ``+0.0``."""
    costs = np.asarray(costs, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        total = costs + np.float64(weight) * np.asarray(values, dtype=np.float32).astype(np.float64)
    if term_step is None:
        return total
    if horizon is None:
        raise ValueError("add_to_costs: term_step needs the horizon")
    return np.where(np.asarray(term_step) == int(horizon), total, costs)


def check_weight(weight) -> float:
    w = float(weight)
    if not np.isfinite(w):
        raise ValueError("terminal_weight must be finite")
    return w


try:
    import xxhash as _xxhash
except Exception:  # pragma: no cover
    _xxhash = None


def _digest(spec: ValueSpec) -> int:
    d = _xxhash.xxh3_64() if _xxhash is not None else hashlib.blake2b(digest_size=8)
    shapes = []
    for a in list(spec.kernels) + list(spec.biases) + [spec.ob_mean, spec.ob_std]:
        d.update(a)
        shapes.append(a.shape)
    d.update(repr(shapes).encode())
    return int.from_bytes(d.digest(), "little") & (2**63 - 1)


def _value_prefix(names, scope: str) -> str:
    """``scope/scope`` (MlpPolicy builds its net inside ``variable_scope(scope)``, ppo_bc_policy.py:31-32, 56)
    or a net built directly under ``scope``."""
    for p in (f"{scope}/{scope}", scope):
        if f"{p}/vf/fc1/kernel:0" in names and f"{p}/obfilter/runningsum:0" in names:
            return p
    raise KeyError(f"no MlpPolicy critic under {scope!r}: expected '{scope}/{scope}/vf/fc1/kernel:0' "
                   f"(ppo_bc_policy.py:31-32,59)")


def _tf_value(policy_net, tf=None) -> ValueSpec:
    """Read the 'pi' critic of ppo_bc_policy.MlpPolicy through its session: only vf/ and obfilter/."""
    if tf is None:
        import tensorflow as tf
    scope = getattr(policy_net, "pi_scope", "pi")
    by_name = {v.name: v for v in tf.global_variables()}
    p = _value_prefix(by_name, scope)
    L = int(getattr(policy_net, "num_hid_layers"))
    want = ([f"{p}/vf/fc{i + 1}/{w}:0" for w in ("kernel", "bias") for i in range(L)]
            + [f"{p}/vf/final/kernel:0", f"{p}/vf/final/bias:0",
               f"{p}/obfilter/runningsum:0", f"{p}/obfilter/runningsumsq:0", f"{p}/obfilter/count:0"])
    vals = dict(zip(want, policy_net.sess.run([by_name[n] for n in want])))
    ks = [vals[f"{p}/vf/fc{i + 1}/kernel:0"] for i in range(L)] + [vals[f"{p}/vf/final/kernel:0"]]
    bs = [vals[f"{p}/vf/fc{i + 1}/bias:0"] for i in range(L)] + [vals[f"{p}/vf/final/bias:0"]]
    ssum, ssq, cnt = (vals[f"{p}/obfilter/{n}:0"] for n in ("runningsum", "runningsumsq", "count"))
    mean = (ssum / cnt).astype(np.float32)
    std = np.sqrt(np.maximum((ssq / cnt).astype(np.float32) - np.square(mean), np.float32(1e-2)))
    return ValueSpec(ks, bs, mean, std.astype(np.float32))


def extract(container) -> Tuple[ValueSpec, int]:
    if isinstance(container, ValueSpec):
        spec = container
    elif hasattr(container, "value_spec"):
        spec = container.value_spec()
    elif hasattr(container, "vf") and hasattr(container.vf, "ob_mean"):
        w = container.vf
        spec = ValueSpec([np.asarray(k) for k in w.kernels], [np.asarray(b) for b in w.biases],
                         np.asarray(w.ob_mean), np.asarray(w.ob_std))
    elif hasattr(container, "sess"):
        spec = _tf_value(container)
    else:
        raise TypeError(f"cannot read a value net from {type(container).__name__}")
    v = getattr(container, "version", None)
    if isinstance(v, int) and not isinstance(v, bool):
        return spec, v
    return spec, _digest(spec)

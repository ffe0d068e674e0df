"""Actor-critic fitting: the definition of one BC-distillation step and one critic-regression step.

The reference clones MPC's actions into its policy with ``update_op_bc`` (ppo_bc_policy.py:52, 111-114, 146-151;
train_mpc_ppo.py:358-372) and regresses its critic on ``vf_loss`` (ppo_bc_policy.py:108).  This module is THE
definition of those two steps, in NumPy, the way ``knots.py``, ``sampling.py`` and ``mppi_update.py`` define what
their kernels compute; csrc/ac_fit.hip is tested against ``run`` (tests/test_gpu_ac_fit.py).

* Input.  ``obz = observe(filter, ob)``: f64 -> f32 (round to nearest), ``(x - ob_mean) / ob_std``, clip to +-5, all
  in f32 -- ``value.observe``'s arithmetic.  The filter is a constant of the step: it is not differentiated.
* Net.  ``h = tanh(h @ W + b)`` per hidden layer in f32, then ``p = h @ W_final + b_final`` with no activation.
  Parameters are the flat list ``[W_0, b_0, ..., W_L, b_L]`` in TF layout ``[in, out]``.
* Head ``"policy"`` (output width A, targets ``ac`` fed as f32):

      d = ac - p;  m = mean over all B*A elements of d*d;  loss = sqrt(m)

  and the gradient is TF's autodiff of exactly that expression, in this operation order:

      s  = 0.5 / loss                      (SqrtGrad: 0.5 * grad / y, grad = 1)
      s  = s / N                           (MeanGrad: truediv by the element count N = B*A)
      dd = s * (d * 2)                     (SquareGrad: grad * (x * 2))
      dp = -dd                             (SubGrad, second operand)

  At ``loss == 0`` s is inf and d is 0, so every gradient element is NaN, as TF's SqrtGrad gives; the step then
  writes NaN into every parameter of the head.  This is stated, not guarded.
* Head ``"value"`` (output width 1, targets ``ret`` fed as f32):

      d = v - ret;  loss = mean(d*d);  dv = (1 / N) * (d * 2)

* Backward.  ``dW_l = H_l^T dZ_l``, ``db_l = colsum(dZ_l)``, ``dH_l = dZ_{l+1} W_{l+1}^T``,
  ``dZ_l = dH_l * (1 - A_l * A_l)`` (TanhGrad).
* Adam.  TF1 ``ApplyAdam`` with f32 beta powers: ``lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t)``;
  ``m += (g - m)(1 - b1)``; ``v += (g*g - v)(1 - b2)``; ``w -= (m lr_t) / (sqrt(v) + eps)``; then the powers are
  multiplied by their betas.  The learning rate is an argument of every run (the reference feeds
  ``bc_lr * cur_lrmult`` per step), not of the optimizer.

``run(..., dtype=np.float64)`` is the high-precision trajectory on the same f32-rounded inputs: parameters, slots
and beta powers in f64, the hyperparameters still the f32-rounded ones.

``ActorCriticFitter`` wraps the device fitter (``bcmpc_acfit_*``, include/bcmpc.h): all arithmetic of a device run
is in csrc/ac_fit.hip, this file only marshals arrays.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

HEADS = ("policy", "value")
MAX_LAYERS = 4
MAX_HIDDEN = 256
MAX_STATE = 32
MAX_ACTION = 16


def check_shape(head: str, state_dim: int, out_dim: int, hidden: int, n_layers: int) -> None:
    """The limits of both the definition and the device fitter (``ValueSpec``'s, plus the action cap)."""
    if head not in HEADS:
        raise ValueError(f"head must be 'policy' or 'value' (got {head!r})")
    if not 1 <= n_layers <= MAX_LAYERS:
        raise ValueError(f"n_layers {n_layers} outside [1, {MAX_LAYERS}]")
    if not 1 <= hidden <= MAX_HIDDEN:
        raise ValueError(f"hidden {hidden} outside [1, {MAX_HIDDEN}]")
    if not 1 <= state_dim <= MAX_STATE:
        raise ValueError(f"state dim {state_dim} outside [1, {MAX_STATE}]")
    if head == "policy" and not 1 <= out_dim <= MAX_ACTION:
        raise ValueError(f"action dim {out_dim} outside [1, {MAX_ACTION}]")
    if head == "value" and out_dim != 1:
        raise ValueError("the value head has one output")


def check_params(head: str, params: Sequence[np.ndarray]):
    """(S, out, hidden, L) of a flat parameter list ``[W_0, b_0, ..., W_L, b_L]``; ValueError when malformed."""
    if len(params) < 4 or len(params) % 2:
        raise ValueError("params: [W_0, b_0, ..., W_L, b_L] with at least one hidden layer")
    L = len(params) // 2 - 1
    ks, bs = params[0::2], params[1::2]
    if any(np.ndim(k) != 2 for k in ks):
        raise ValueError("params: kernels must be [in, out] matrices")
    S, hidden = ks[0].shape
    out = ks[-1].shape[1]
    check_shape(head, S, out, hidden, L)
    for i, (k, b) in enumerate(zip(ks, bs)):
        want = (S if i == 0 else hidden, out if i == L else hidden)
        if k.shape != want or np.shape(b) != (want[1],):
            raise ValueError(f"params: layer {i} has kernel {k.shape} / bias {np.shape(b)}, expected {want}")
    return S, out, hidden, L


def _filter(flt):
    mean, std = (flt.ob_mean, flt.ob_std) if hasattr(flt, "ob_mean") else flt
    return (np.ascontiguousarray(mean, dtype=np.float32).reshape(-1),
            np.ascontiguousarray(std, dtype=np.float32).reshape(-1))


def observe(flt, ob) -> np.ndarray:
    """obz [B, S] f32 of observations [B, S]; ``flt``: anything with ``ob_mean`` / ``ob_std`` (a ``ValueSpec``, a
    ``PolicySpec``) or a ``(mean, std)`` pair.  The arithmetic of ``value.observe``."""
    mean, std = _filter(flt)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.asarray(ob, dtype=np.float64).astype(np.float32)
        return np.clip((x - mean) / std, np.float32(-5), np.float32(5)).astype(np.float32)


def grads(params: Sequence[np.ndarray], head: str, obz: np.ndarray, target: np.ndarray, dtype=np.float32):
    """(loss, d loss / d params) of one batch; ``obz`` [B, S] and ``target`` [B, out] already of ``dtype``."""
    f = dtype
    L = len(params) // 2 - 1
    ks, bs = params[0::2], params[1::2]
    hs = [obz]
    h = obz
    with np.errstate(divide="ignore", invalid="ignore"):
        for l in range(L):
            h = np.tanh(h @ ks[l] + bs[l]).astype(f)
            hs.append(h)
        p = (h @ ks[L] + bs[L]).astype(f)
        n = f(p.size)
        if head == "policy":
            d = target - p
            loss = f(np.sqrt(np.mean(np.square(d), dtype=f)))
            s = (f(0.5) / loss) / n
            dp = -(s * (d * f(2.0)))
        elif head == "value":
            d = p - target
            loss = f(np.mean(np.square(d), dtype=f))
            dp = (f(1.0) / n) * (d * f(2.0))
        else:
            raise ValueError(f"head must be 'policy' or 'value' (got {head!r})")
        dz = dp.astype(f)
        out = [None] * (2 * L + 2)
        for l in range(L, -1, -1):
            out[2 * l] = (hs[l].T @ dz).astype(f)
            out[2 * l + 1] = np.sum(dz, axis=0, dtype=f)
            if l > 0:
                a = hs[l]
                dz = ((dz @ ks[l].T) * (f(1) - a * a)).astype(f)
    return loss, out


@dataclass
class AdamState:
    """One head's Adam slots and f32 beta powers; they persist across runs like ``update_op_bc``'s variables."""
    m: List[np.ndarray]
    v: List[np.ndarray]
    beta1_power: np.floating
    beta2_power: np.floating

    @classmethod
    def zeros_like(cls, params, beta1=0.9, beta2=0.999, dtype=np.float32) -> "AdamState":
        return cls([np.zeros_like(p, dtype=dtype) for p in params], [np.zeros_like(p, dtype=dtype) for p in params],
                   dtype(np.float32(beta1)), dtype(np.float32(beta2)))


def adam_apply(params: List[np.ndarray], g: Sequence[np.ndarray], st: AdamState, lr, beta1=0.9, beta2=0.999,
               eps=1e-8, dtype=np.float32) -> None:
    """TF1 ApplyAdam in place, then the beta powers advance (AdamOptimizer._finish)."""
    f = dtype
    beta1, beta2, lr, eps = (np.float32(x) for x in (beta1, beta2, lr, eps))
    b1, b2 = f(beta1), f(beta2)
    with np.errstate(invalid="ignore"):
        lr_t = f(lr) * np.sqrt(f(1) - st.beta2_power) / (f(1) - st.beta1_power)
        for i, gi in enumerate(g):
            st.m[i] = (st.m[i] + (gi - st.m[i]) * (f(1) - b1)).astype(f)
            st.v[i] = (st.v[i] + (gi * gi - st.v[i]) * (f(1) - b2)).astype(f)
            params[i] = (params[i] - (st.m[i] * lr_t) / (np.sqrt(st.v[i]) + f(eps))).astype(f)
    st.beta1_power = f(st.beta1_power * b1)
    st.beta2_power = f(st.beta2_power * b2)


def batch(flt, obs, targets, idx, dtype=np.float32):
    """(obz, target) of the rows ``idx``: the filter in f32, the targets fed as f32, then widened to ``dtype``."""
    t = np.asarray(targets, dtype=np.float64)[idx].astype(np.float32)
    return observe(flt, np.asarray(obs, dtype=np.float64)[idx]).astype(dtype), t.reshape(len(idx), -1).astype(dtype)


def run(params: List[np.ndarray], adam_state: AdamState, head: str, spec_filter, obs, targets,
        batches: Sequence[np.ndarray], lr, beta1=0.9, beta2=0.999, eps=1e-8, dtype=np.float32) -> List:
    """THE definition of a fitting run: one Adam step per index array of ``batches`` on rows of ``obs`` [n, S] /
    ``targets`` [n, out] (f64).  ``params`` and ``adam_state`` are updated in place; returns each step's loss, taken
    before its update.  ``lr``: one learning rate, or one per step."""
    check_params(head, params)
    lrs = np.broadcast_to(np.asarray(lr, dtype=np.float64), (len(batches),))
    losses = []
    for idx, step_lr in zip(batches, lrs):
        obz, t = batch(spec_filter, obs, targets, np.asarray(idx), dtype)
        loss, g = grads(params, head, obz, t, dtype)
        adam_apply(params, g, adam_state, step_lr, beta1, beta2, eps, dtype)
        losses.append(loss)
    return losses


def lds_words(hidden: int, n_layers: int, state_dim: int, out_dim: int) -> int:
    """f32 words of LDS of the row kernel (acfit_rows_kernel), the formula of csrc/ac_fit_plan.cpp: two row
    buffers and one activation buffer per hidden layer of 16 rows with stride ld, the targets [16][16], the loss
    partials [16] and the K-split partials [16][256]."""
    ld = (max(hidden, state_dim, out_dim) + 3) // 4 * 4 + 4
    return (2 + n_layers) * 16 * ld + 16 * 16 + 16 + 16 * 256


# ------------------------------------------------------------------ device ---
_FP = ctypes.POINTER(ctypes.c_float)
_DP = ctypes.POINTER(ctypes.c_double)


def _check(lib, code: int) -> None:
    if code == 0:
        return
    msg = lib.bcmpc_acfit_last_error().decode(errors="replace")
    if code in (1, 2):                                   # BCMPC_ERR_ARG / BCMPC_ERR_UNSUPPORTED
        raise ValueError(f"[bcmpc status {code}] {msg}")
    from ._lib import BcmpcError
    raise BcmpcError(code, msg)


class ActorCriticFitter:
    """One head's device fitter (``bcmpc_acfit``): the head's f32 parameters, its Adam slots and beta powers, the
    observation filter and a copy of the data live on the device; ``run`` makes one Adam step per index array
    (two kernel launches each; uniform batches replay one captured graph) and returns the losses."""

    def __init__(self, head: str, state_dim: int, out_dim: int, hidden: int, n_layers: int, batch_size: int = 128,
                 device: int = 0, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8):
        from . import _lib
        self._lib = _lib.load()
        self._h = None
        code = HEADS.index(head) if head in HEADS else -1
        c = _lib.AcFitConfig(int(state_dim), int(out_dim), int(hidden), int(n_layers), code, int(batch_size),
                             int(device), float(beta1), float(beta2), float(epsilon))
        h = ctypes.c_void_p()
        _check(self._lib, self._lib.bcmpc_acfit_create(ctypes.byref(c), ctypes.byref(h)))
        self._h = h
        self.head, self.S, self.out, self.hidden, self.L = head, int(state_dim), int(out_dim), int(hidden), int(n_layers)

    def _shapes(self):
        dims = [self.S] + [self.hidden] * self.L + [self.out]
        return [(dims[i], dims[i + 1]) for i in range(self.L + 1)]

    def set_params(self, kernels, biases) -> None:
        ks = [np.ascontiguousarray(k, dtype=np.float32) for k in kernels]
        bs = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in biases]
        if [k.shape for k in ks] != self._shapes() or [b.shape for b in bs] != [(s[1],) for s in self._shapes()]:
            raise ValueError(f"set_params: kernels must have shapes {self._shapes()}")
        _check(self._lib, self._lib.bcmpc_acfit_set_params(
            self._h, (_FP * len(ks))(*[k.ctypes.data_as(_FP) for k in ks]),
            (_FP * len(bs))(*[b.ctypes.data_as(_FP) for b in bs])))

    def get_params(self):
        ks = [np.empty(s, np.float32) for s in self._shapes()]
        bs = [np.empty(s[1], np.float32) for s in self._shapes()]
        _check(self._lib, self._lib.bcmpc_acfit_get_params(
            self._h, (_FP * len(ks))(*[k.ctypes.data_as(_FP) for k in ks]),
            (_FP * len(bs))(*[b.ctypes.data_as(_FP) for b in bs])))
        return ks, bs

    def set_filter(self, ob_mean, ob_std) -> None:
        mean, std = _filter((ob_mean, ob_std))
        if mean.shape != (self.S,) or std.shape != (self.S,):
            raise ValueError(f"set_filter: ob_mean / ob_std must have shape ({self.S},)")
        _check(self._lib, self._lib.bcmpc_acfit_set_filter(self._h, mean.ctypes.data_as(_FP), std.ctypes.data_as(_FP)))

    def set_data(self, obs, targets) -> None:
        o = np.ascontiguousarray(obs, dtype=np.float64)
        t = np.ascontiguousarray(targets, dtype=np.float64)
        n = o.shape[0]
        t = t.reshape(n, -1) if t.ndim == 1 else t
        if o.shape != (n, self.S) or t.shape != (n, self.out):
            raise ValueError(f"set_data: obs [n, {self.S}], targets [n, {self.out}]")
        _check(self._lib, self._lib.bcmpc_acfit_set_data(self._h, o.ctypes.data_as(_DP), t.ctypes.data_as(_DP), n))

    def run(self, batches: Sequence[np.ndarray], lr: float) -> np.ndarray:
        """One Adam step per index array at learning rate ``lr``; each step's loss before its update."""
        sizes = np.asarray([len(b) for b in batches], dtype=np.int32)
        idx = np.ascontiguousarray(np.concatenate(batches) if len(batches) else np.zeros(0), dtype=np.int64)
        losses = np.empty(len(batches), dtype=np.float32)
        _check(self._lib, self._lib.bcmpc_acfit_run(
            self._h, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(batches), ctypes.c_float(lr),
            losses.ctypes.data_as(_FP)))
        return losses

    @property
    def graph_captures(self) -> int:
        """0: the last run launched its steps one by one; n >= 1: it replayed a captured graph, and the fitter
        has captured n graphs so far (bcmpc_acfit_is_graph)."""
        return int(self._lib.bcmpc_acfit_is_graph(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.bcmpc_acfit_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

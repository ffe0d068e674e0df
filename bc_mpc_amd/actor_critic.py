"""``MlpActorCritic``: the reference ``MlpPolicy``'s ``pi`` scope (ppo_bc_policy.py:54-88) without TF.

The container the controllers consume (``policy_net=``, ``policy_prior=``, ``terminal_value=``) and the package can
train: ``fit_bc`` clones (ob, ac) pairs into the policy head (``update_op_bc``, ppo_bc_policy.py:52, 114, 146-151;
train_mpc_ppo.py:358-372), ``fit_value`` regresses the critic on returns (``vf_loss``, ppo_bc_policy.py:108).  Both
run on the device (csrc/ac_fit.hip); ``ac_fit.py`` is their definition.  ``fit_ppo`` / ``lossandupdate_ppo`` make
the clipped-surrogate step of ``lossandupdate_ppo`` (ppo_bc_policy.py:90-144) against the policy frozen by
``assign_old_eq_new``, optionally interleaved with BC steps (train_mpc_ppo.py:355-372), on the device
(csrc/ac_ppo.hip); ``ppo.py`` is its definition.

* ``pol/`` and ``vf/`` stacks in TF layout, f32: ``fc1..fcL`` tanh then ``final``; ``normc`` initialisation
  (baselines ``U.normc_initializer``: a standard normal draw, every column scaled to norm ``std``), std 1.0 for the
  hidden layers and ``vf/final``, 0.01 for ``pol/final``; zero biases; ``logstd [A]`` zero.
* ``ob_rms``: baselines' ``RunningMeanStd`` -- f64 ``sum`` 0, ``sumsq`` 1e-2, ``count`` 1e-2; ``update(ob)``
  accumulates; ``mean = f32(sum / count)``, ``std = sqrt(max(f32(sumsq / count) - mean^2, 1e-2))``, the formulas of
  ``policy._tf_policy``.
* ``version``: an integer bumped by every mutation (a fit, a filter update, ``set_weights``), so ``policy.extract`` /
  ``value.extract`` trust it and the engines' setters re-upload exactly when something changed, without a digest.
* A BC step moves only ``pol/fc*`` and ``pol/final``; ``logstd``, ``vf/`` and the filter get no gradient (the BC
  loss does not reach them).  A value step moves only ``vf/``.  Each head has its own Adam slots and beta powers,
  on the device for the container's life.  A PPO step moves ``pol/``, ``vf/`` and ``logstd`` under a third
  optimizer (``update_op_ppo``) with its own slots and one pair of beta powers; it trains in place on the two
  heads' device weights.
* The old policy (``assign_old_eq_new``) is a copy of ``pol/``, ``logstd`` and the filter's mean / std.  The engines
  do not see it, so taking it does not bump ``version``.
"""
from __future__ import annotations

import random
from typing import Optional, Tuple

import numpy as np

from . import ac_fit, ppo
from .engine import PolicySpec
from .value import ValueSpec, terminal_values


def normc(rs: np.random.RandomState, shape, std: float) -> np.ndarray:
    """baselines ``normc_initializer(std)``: columns of a standard normal draw scaled to norm ``std``, f32."""
    out = rs.standard_normal(shape).astype(np.float32)
    out *= np.float32(std) / np.sqrt(np.square(out).sum(axis=0, keepdims=True))
    return out.astype(np.float32)


def filter_mean_std(total, sumsq, count) -> Tuple[np.ndarray, np.ndarray]:
    """RunningMeanStd.mean / .std as the f32 tensors the net sees (``policy._tf_policy``'s formulas)."""
    mean = (np.asarray(total, np.float64) / count).astype(np.float32)
    std = np.sqrt(np.maximum((np.asarray(sumsq, np.float64) / count).astype(np.float32) - np.square(mean),
                             np.float32(1e-2)))
    return mean, std.astype(np.float32)


class RunningMeanStd:
    """baselines' observation filter (mpi_running_mean_std.py, one process): f64 sums, epsilon 1e-2."""

    def __init__(self, shape, on_change=None):
        self.sum = np.zeros(shape, np.float64)
        self.sumsq = np.full(shape, 1e-2, np.float64)
        self.count = 1e-2
        self._on_change = on_change

    def update(self, ob) -> None:
        x = np.asarray(ob, dtype=np.float64)
        x = x.reshape(-1, *self.sum.shape)
        if not np.isfinite(x).all():
            raise ValueError("ob_rms.update: observations must be finite")
        self.sum = self.sum + x.sum(axis=0)
        self.sumsq = self.sumsq + np.square(x).sum(axis=0)
        self.count = self.count + float(x.shape[0])
        if self._on_change is not None:
            self._on_change()

    @property
    def mean(self) -> np.ndarray:
        return filter_mean_std(self.sum, self.sumsq, self.count)[0]

    @property
    def std(self) -> np.ndarray:
        return filter_mean_std(self.sum, self.sumsq, self.count)[1]


def _dim(space) -> int:
    shape = tuple(space.shape)
    if len(shape) != 1:
        raise ValueError("MlpActorCritic: observation and action spaces must be one-dimensional")
    return int(shape[0])


class MlpActorCritic:
    def __init__(self, env, hid_size: int = 128, num_hid_layers: int = 2, seed: Optional[int] = None,
                 device: int = 0, clip_param: float = 0.2, entcoeff: float = 0.0):
        S, A = _dim(env.observation_space), _dim(env.action_space)
        ac_fit.check_shape("policy", S, A, int(hid_size), int(num_hid_layers))
        self.ob_dim, self.ac_dim = S, A
        self.hid_size, self.num_hid_layers, self.device = int(hid_size), int(num_hid_layers), int(device)
        rs = np.random.RandomState(seed)
        L, h = self.num_hid_layers, self.hid_size

        def stack(out, final_std):
            dims = [S] + [h] * L + [out]
            ks = [normc(rs, (dims[i], dims[i + 1]), 1.0 if i < L else final_std) for i in range(L + 1)]
            return ks, [np.zeros(dims[i + 1], np.float32) for i in range(L + 1)]
        self.vf_kernels, self.vf_biases = stack(1, 1.0)            # the reference builds vf/ first
        self.pol_kernels, self.pol_biases = stack(A, 0.01)
        self.logstd = np.zeros(A, np.float32)
        self.version = 0
        self._fitters = {}                                         # head -> [fitter, params stamp, filter stamp]
        self._stamp = {"policy": 0, "value": 0, "filter": 0, "logstd": 0, "old": 0}   # what the device copies are compared with
        self.clip_param, self.entcoeff = float(clip_param), float(entcoeff)
        self._old = None                                           # assign_old_eq_new's copies
        self._ppo = None                                           # [trainer, logstd stamp, old stamp]
        self.ob_rms = RunningMeanStd((S,), on_change=self._bump)

    # ------------------------------------------------------------ state ---
    def _bump(self) -> None:
        self.version += 1
        self._stamp["filter"] += 1

    def policy_spec(self) -> PolicySpec:
        return PolicySpec(list(self.pol_kernels), list(self.pol_biases), self.ob_rms.mean, self.ob_rms.std, self.logstd)

    def value_spec(self) -> ValueSpec:
        return ValueSpec(list(self.vf_kernels), list(self.vf_biases), self.ob_rms.mean, self.ob_rms.std)

    def get_weights(self) -> dict:
        """Copies of every array: ``pol`` / ``vf`` (kernels, biases), ``logstd`` and the filter's sums."""
        return {"pol": ([k.copy() for k in self.pol_kernels], [b.copy() for b in self.pol_biases]),
                "vf": ([k.copy() for k in self.vf_kernels], [b.copy() for b in self.vf_biases]),
                "logstd": self.logstd.copy(),
                "ob_rms": (self.ob_rms.sum.copy(), self.ob_rms.sumsq.copy(), float(self.ob_rms.count))}

    def set_weights(self, weights: dict) -> None:
        """Replace any of ``get_weights``' entries; the Adam slots of the heads are kept."""
        def stack(pair, out):
            dims = [self.ob_dim] + [self.hid_size] * self.num_hid_layers + [out]
            ks = [np.array(k, dtype=np.float32) for k in pair[0]]
            bs = [np.array(b, dtype=np.float32).reshape(-1) for b in pair[1]]
            if ([k.shape for k in ks] != [(dims[i], dims[i + 1]) for i in range(len(dims) - 1)]
                    or [b.shape for b in bs] != [(d,) for d in dims[1:]]):
                raise ValueError("set_weights: kernel / bias shapes do not match the container")
            if not all(np.isfinite(x).all() for x in ks + bs):
                raise ValueError("set_weights: weights must be finite")
            return ks, bs
        new = {}
        if "pol" in weights:
            new["pol"] = stack(weights["pol"], self.ac_dim)
        if "vf" in weights:
            new["vf"] = stack(weights["vf"], 1)
        if "logstd" in weights:
            ls = np.array(weights["logstd"], dtype=np.float32).reshape(-1)
            if ls.shape != (self.ac_dim,) or not np.isfinite(ls).all():
                raise ValueError("set_weights: logstd must be finite with shape (A,)")
            new["logstd"] = ls
        if "ob_rms" in weights:
            s, q, c = weights["ob_rms"]
            s, q = np.array(s, dtype=np.float64).reshape(-1), np.array(q, dtype=np.float64).reshape(-1)
            if s.shape != (self.ob_dim,) or q.shape != (self.ob_dim,) or not float(c) > 0:
                raise ValueError("set_weights: ob_rms is (sum [S], sumsq [S], count > 0)")
            new["ob_rms"] = (s, q, float(c))
        if "pol" in new:
            self.pol_kernels, self.pol_biases = new["pol"]
            self._stamp["policy"] += 1
        if "vf" in new:
            self.vf_kernels, self.vf_biases = new["vf"]
            self._stamp["value"] += 1
        if "logstd" in new:
            self.logstd = new["logstd"]
            self._stamp["logstd"] += 1
        if "ob_rms" in new:
            self.ob_rms.sum, self.ob_rms.sumsq, self.ob_rms.count = new["ob_rms"]
            self._stamp["filter"] += 1
        self.version += 1

    # -------------------------------------------------------------- act ---
    def act(self, ob, stochastic: bool = True, rng=None):
        """(ac [B, A], vpred [B]) f32 on the host (ppo_bc_policy.py:174-185); stochastic:
        ``mean + exp(logstd) * N(0, 1)`` with the normals of ``rng.standard_normal`` (default ``np.random``)."""
        ob = np.asarray(ob, dtype=np.float64)
        if ob.ndim == 1:
            ob = ob[None]
        if ob.ndim != 2 or ob.shape[1] != self.ob_dim:
            raise ValueError(f"act: ob must be [B, {self.ob_dim}]")
        h = ac_fit.observe((self.ob_rms.mean, self.ob_rms.std), ob)
        with np.errstate(invalid="ignore"):
            for W, b in zip(self.pol_kernels[:-1], self.pol_biases[:-1]):
                h = np.tanh(h @ W + b)
            mean = (h @ self.pol_kernels[-1] + self.pol_biases[-1]).astype(np.float32)
        vpred = terminal_values(self.value_spec(), ob)
        if stochastic:
            rng = np.random if rng is None else rng
            mean = (mean + np.exp(self.logstd) * rng.standard_normal(mean.shape).astype(np.float32)).astype(np.float32)
        return mean, vpred

    # -------------------------------------------------------------- fit ---
    def _checked(self, what: str, obs, targets, out: int):
        try:
            o = np.ascontiguousarray(obs, dtype=np.float64)
            t = np.ascontiguousarray(targets, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: data must be numeric arrays") from None
        if o.ndim == 1 and o.shape[0] == self.ob_dim:
            o = o[None]
        if o.ndim != 2 or o.shape[1] != self.ob_dim:
            raise ValueError(f"{what}: observations must be [n, {self.ob_dim}]")
        n = o.shape[0]
        if n == 0:
            raise ValueError(f"{what}: the data is empty")
        if t.size != n * out:
            raise ValueError(f"{what}: targets must be [n, {out}] for n = {n} observations")
        t = t.reshape(n, out)
        if not (np.isfinite(o).all() and np.isfinite(t).all()):
            raise ValueError(f"{what}: data must be finite")
        return o, t

    def _fitter(self, head: str) -> "ac_fit.ActorCriticFitter":
        """The head's device fitter with the container's current weights and filter on the device."""
        out = self.ac_dim if head == "policy" else 1
        ent = self._fitters.get(head)
        if ent is None:
            f = ac_fit.ActorCriticFitter(head, self.ob_dim, out, self.hid_size, self.num_hid_layers, device=self.device)
            ent = self._fitters[head] = [f, None, None]
        f = ent[0]
        if ent[1] != self._stamp[head]:
            ks, bs = (self.pol_kernels, self.pol_biases) if head == "policy" else (self.vf_kernels, self.vf_biases)
            f.set_params(ks, bs)
            ent[1] = self._stamp[head]
        if ent[2] != self._stamp["filter"]:
            f.set_filter(self.ob_rms.mean, self.ob_rms.std)
            ent[2] = self._stamp["filter"]
        return f

    def _run(self, head: str, obs, targets, batches, learning_rate) -> np.ndarray:
        lr = float(learning_rate)
        if not np.isfinite(lr):
            raise ValueError("learning_rate must be finite")
        f = self._fitter(head)
        f.set_data(obs, targets)
        losses = f.run(batches, lr)
        ks, bs = f.get_params()
        if head == "policy":
            self.pol_kernels, self.pol_biases = ks, bs
        else:
            self.vf_kernels, self.vf_biases = ks, bs
        self.version += 1                                     # (the device copy is this result: its stamp stands)
        return losses

    @staticmethod
    def _sizes(iterations, batch_size):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        if int(iterations) < 0:
            raise ValueError("iterations must be >= 0")
        return int(iterations), int(batch_size)

    def update_bc(self, ob, ac, learning_rate) -> np.ndarray:
        """One BC step on the whole batch (ppo_bc_policy.py:146-151); returns its loss [1] (before the update)."""
        o, t = self._checked("update_bc", ob, ac, self.ac_dim)
        return self._run("policy", o, t, [np.arange(o.shape[0], dtype=np.int64)], learning_rate)

    def fit_bc(self, data, iterations: int, batch_size: int, learning_rate, rng=random) -> np.ndarray:
        """``iterations`` BC steps on batches of ``data``: a ``DataBufferGeneral(.., 2)`` of ``[ob, ac]`` items or
        an ``(obs, acs)`` tuple.  Each step's rows are the ones ``DataBufferGeneral.sample(batch_size)`` draws
        (``fit.sample_batches`` on ``rng``, default Python's global ``random``).  Returns the f32 losses."""
        iterations, batch_size = self._sizes(iterations, batch_size)
        if isinstance(data, tuple):
            if len(data) != 2:
                raise ValueError("fit_bc: data is an (obs, acs) tuple or a buffer of [ob, ac] items")
            obs, acs = data
        else:
            items = list(data.buffer)
            if not items:
                raise ValueError("fit_bc: the data is empty")
            try:
                obs = np.asarray([it[0] for it in items], np.float64)
                acs = np.asarray([it[1] for it in items], np.float64)
            except (TypeError, ValueError, IndexError):
                raise ValueError("fit_bc: buffer items must be [ob, ac] with equal shapes") from None
        o, t = self._checked("fit_bc", obs, acs, self.ac_dim)
        from .fit import sample_batches
        return self._run("policy", o, t, sample_batches(o.shape[0], batch_size, iterations, rng), learning_rate)

    def fit_value(self, obs, returns, iterations: int, batch_size: int, learning_rate, rng=random) -> np.ndarray:
        """``iterations`` critic steps on ``mean((vpred - ret)^2)`` over batches drawn like ``fit_bc``'s."""
        iterations, batch_size = self._sizes(iterations, batch_size)
        o, t = self._checked("fit_value", obs, returns, 1)
        from .fit import sample_batches
        return self._run("value", o, t, sample_batches(o.shape[0], batch_size, iterations, rng), learning_rate)

    # -------------------------------------------------------------- PPO ---
    def assign_old_eq_new(self) -> None:
        """Freeze the current policy as the old one (ppo_bc_policy.py ``assign_old_eq_new``): copies of ``pol/``,
        ``logstd`` and the filter's mean / std.  ``version`` stands: the engines do not see the old policy."""
        self._old = dict(kernels=[k.copy() for k in self.pol_kernels], biases=[b.copy() for b in self.pol_biases],
                         logstd=self.logstd.copy(), ob_mean=self.ob_rms.mean.copy(), ob_std=self.ob_rms.std.copy())
        self._stamp["old"] += 1

    def _make_trainer(self, policy_fitter, value_fitter) -> "ppo.PpoTrainer":
        return ppo.PpoTrainer(policy_fitter, value_fitter)

    def _trainer(self) -> "ppo.PpoTrainer":
        """The device trainer over both heads' fitters with the container's weights, filter, logstd and old policy
        on the device."""
        pf, vf = self._fitter("policy"), self._fitter("value")
        if self._ppo is None:
            self._ppo = [self._make_trainer(pf, vf), None, None]
        t = self._ppo[0]
        if self._ppo[1] != self._stamp["logstd"]:
            t.set_logstd(self.logstd)
            self._ppo[1] = self._stamp["logstd"]
        if self._ppo[2] != self._stamp["old"]:
            o = self._old
            t.set_old(o["kernels"], o["biases"], o["ob_mean"], o["ob_std"], o["logstd"])
            self._ppo[2] = self._stamp["old"]
        return t

    def _run_ppo(self, data, batches, lr, eps, entcoeff, bc=None) -> np.ndarray:
        t = self._trainer()
        t.set_data(*data)
        if bc is None:
            losses = t.run(batches, lr, eps, entcoeff)
        else:
            (bobs, bacs), bbatches, blr = bc
            self._fitters["policy"][0].set_data(bobs, bacs)
            losses, _bc_losses = t.run(batches, lr, eps, entcoeff, bc_batches=bbatches, bc_lr=blr)
        self.pol_kernels, self.pol_biases = self._fitters["policy"][0].get_params()
        self.vf_kernels, self.vf_biases = self._fitters["value"][0].get_params()
        self.logstd = t.get_logstd()
        self.version += 1                                     # (the device copies are this result: their stamps stand)
        return losses

    def _checked_ppo(self, what: str, ob, ac, atarg, ret):
        if self._old is None:
            raise ValueError(f"{what}: assign_old_eq_new has not been called")
        o, a = self._checked(what, ob, ac, self.ac_dim)
        _, at = self._checked(what, o, atarg, 1)
        _, rt = self._checked(what, o, ret, 1)
        return o, a, at[:, 0], rt[:, 0]

    def fit_ppo(self, ob, ac, atarg, ret, iterations: int, batch_size: int, learning_rate, clip_param: float = 0.2,
                entcoeff: float = 0.0, cur_lrmult: float = 1.0, bc_data=None, bc_learning_rate=None,
                rng=random) -> np.ndarray:
        """``iterations`` PPO steps (``lossandupdate_ppo``) against the policy of ``assign_old_eq_new`` on batches of
        the rows ``ob`` [n, S], ``ac`` [n, A], ``atarg`` [n], ``ret`` [n]; with ``bc_data = (obs, acs)`` every PPO
        step is followed by one BC step at ``bc_learning_rate``.  Per iteration ``rng.sample(range(n), k)`` draws
        the PPO rows, then (with ``bc_data``) one draw over the BC data: the two ``DataBufferGeneral.sample`` calls
        of train_mpc_ppo.py:363, 368 in their order.  The learning rates are used as given (the caller multiplies
        by ``cur_lrmult``, as the reference does); ``cur_lrmult`` scales only the clip range.  Returns the losses
        [iterations, 6] f32: pol_surr, pol_entpen, vf_loss, kl, ent, bc_loss, each before its update."""
        iterations, batch_size = self._sizes(iterations, batch_size)
        o, a, at, rt = self._checked_ppo("fit_ppo", ob, ac, atarg, ret)
        lr, eps, ec = float(learning_rate), float(clip_param) * float(cur_lrmult), float(entcoeff)
        if not (np.isfinite(lr) and np.isfinite(eps) and np.isfinite(ec)) or eps < 0:
            raise ValueError("fit_ppo: learning_rate, clip_param * cur_lrmult >= 0 and entcoeff must be finite")
        bc = None
        if bc_data is not None:
            if not isinstance(bc_data, tuple) or len(bc_data) != 2:
                raise ValueError("fit_ppo: bc_data is an (obs, acs) tuple")
            if bc_learning_rate is None or not np.isfinite(float(bc_learning_rate)):
                raise ValueError("fit_ppo: bc_data needs a finite bc_learning_rate")
            bc = self._checked("fit_ppo", bc_data[0], bc_data[1], self.ac_dim)
        n, k = o.shape[0], min(batch_size, o.shape[0])
        batches, bbatches = [], []
        for _ in range(iterations):
            batches.append(np.asarray(rng.sample(range(n), k), dtype=np.int64))
            if bc is not None:
                nb = bc[0].shape[0]
                bbatches.append(np.asarray(rng.sample(range(nb), min(batch_size, nb)), dtype=np.int64))
        return self._run_ppo((o, a, at, rt), batches, lr, eps, ec,
                             None if bc is None else (bc, bbatches, float(bc_learning_rate)))

    def lossandupdate_ppo(self, ob, ac, atarg, ret, cur_lrmult, learning_rate) -> np.ndarray:
        """One PPO step on the whole batch (ppo_bc_policy.py:134-144, its name and argument order) with the
        container's ``clip_param`` and ``entcoeff``; returns the six losses (before the update)."""
        o, a, at, rt = self._checked_ppo("lossandupdate_ppo", ob, ac, atarg, ret)
        lr, eps = float(learning_rate), self.clip_param * float(cur_lrmult)
        if not (np.isfinite(lr) and np.isfinite(eps)) or eps < 0:
            raise ValueError("lossandupdate_ppo: learning_rate and clip_param * cur_lrmult >= 0 must be finite")
        return self._run_ppo((o, a, at, rt), [np.arange(o.shape[0], dtype=np.int64)], lr, eps, self.entcoeff)[0]

    def close(self) -> None:
        if self._ppo is not None:                             # before the fitters it is built over
            self._ppo[0].close()
            self._ppo = None
        for ent in self._fitters.values():
            ent[0].close()
        self._fitters = {}

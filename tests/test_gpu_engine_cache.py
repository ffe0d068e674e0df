"""The controllers' engine cache on the GPU (controllers._cached_engine), at the smallest shapes at which it can go
wrong: 2 x 64 nets, H = 3, K = 40 (two full 16-candidate columns and one half-filled; 56 after the rebuild), B = 2,
two ensemble members, ``rng="device"`` with fixed seeds.

Every step of a case changes one thing on a long-lived controller and then checks (a) whether the engine object was
kept or replaced -- and that a replaced engine is closed -- and (b) that the call's result and every ``last_*``
attribute equal, byte for byte, those of a controller constructed afresh at the same settings and the same position
of the seed stream.  The planners run with ``warm_start=False`` so that a fresh controller starts from the same plan."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S, A, H, K, K2, B = 20, 6, 3, 40, 56, 2


class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32)


class _Env:
    def __init__(self):
        self.observation_space, self.action_space = _Space(S), _Space(A)


_MODELS = {}


def _model(kind):
    """One model per kind for the whole module (the controllers only read it)."""
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel
    from oracle import mpc_oracle as orc
    if kind not in _MODELS:
        norm = orc.synthetic_normalization(S, A)
        if kind == "delta":
            m = orc.NumpyDynamics(orc.synthetic_weights(S, A, 64, 2, "tanh", False), norm)
        elif kind == "reward":
            m = orc.NumpyRewardDynamics(orc.synthetic_reward_weights(S, A, 64, False, seed_base=321),
                                        orc.synthetic_normalization(S, A, seed=5, reward=True))
        else:
            m = EnsembleDynamicsModel(_Env(), 2, 2, 64, "tanh", None, norm, 32, 3, 1e-3, device=0)
            for e in range(2):
                w = orc.synthetic_weights(S, A, 64, 2, "tanh", False, seed_base=1000 + 100 * e)
                m.load_weights(e, w.kernels, w.biases, None, None)
        _MODELS[kind] = m
    return _MODELS[kind]


def _terms():
    from bc_mpc_amd import TermCost
    from bc_mpc_amd.cost_functions import linear, threshold
    return TermCost([threshold(5, ">=", 0.2, 10.0), linear(2, 0.1, on="action")])


def _make(cls, model, horizon, cost_fn, k, gamma):
    import bc_mpc_amd
    kw = dict(rng="device") if cls.startswith("MPCcontroller") else dict(warm_start=False, iterations=2)
    return getattr(bc_mpc_amd, cls)(_Env(), _model(model), horizon, cost_fn, k, gamma, seed=9, **kw)


def _engine(ctrl, model, batched):
    if model == "ens":
        return ctrl._ens_engines["batch" if batched else "single"][1]
    return ctrl._batch_engine if batched else ctrl._engine


def _close(ctrl):
    for eng in [ctrl._engine, getattr(ctrl, "_batch_engine", None)] + [e for _, e in ctrl.__dict__.get("_ens_engines",
                                                                                                      {}).values()]:
        if eng is not None:
            eng.close()


def _bytes(x) -> bytes:
    if x is None:
        return b"None"
    if isinstance(x, ctypes.Structure):
        return bytes(x)
    a = np.ascontiguousarray(np.asarray(x))
    return f"{a.dtype.str}{a.shape}".encode() + a.tobytes()


def _answers(ctrl, call, arg) -> dict:
    out = {"return": _bytes(getattr(ctrl, call)(arg))}
    out.update({k: _bytes(v) for k, v in vars(ctrl).items() if k.startswith("last_")})
    return out


# (controller, model): single and batched, but for the planners on an ensemble, which have no batched form
CASES = [("MPCcontroller", "delta"), ("MPCcontroller", "ens"), ("MPCcontrollerReward", "reward"),
         ("CEMcontroller", "delta"), ("CEMcontroller", "reward"), ("CEMcontroller", "ens"),
         ("MPPIcontroller", "delta"), ("MPPIcontroller", "reward"), ("MPPIcontroller", "ens")]
CASES = [pytest.param(c, m, b, id=f"{c}-{m}-{'batched' if b else 'single'}") for c, m in CASES for b in (False, True)
         if not (b and m == "ens" and c != "MPCcontroller")]


@pytest.mark.parametrize("cls,model,batched", CASES)
def test_engine_is_kept_or_rebuilt_and_answers_like_a_fresh_controller(cls, model, batched):
    from bc_mpc_amd import cheetah_cost_fn
    from oracle import mpc_oracle as orc
    norm = orc.synthetic_normalization(S, A)
    arg = np.stack([orc.synthetic_state(norm, seed=11 + b) for b in range(B)]) if batched else \
        orc.synthetic_state(norm, seed=11)
    call = "get_actions" if batched else "get_action"
    cost0 = None if model == "reward" else cheetah_cost_fn
    ctrl = _make(cls, model, H, cost0, K, 0.9)
    ens = _model("ens")

    def step(change, rebuilt):
        """Apply ``change``; the next call keeps or replaces the engine and answers like a fresh controller."""
        before = _engine(ctrl, model, batched) if change is not None else None
        if change is not None:
            change()
        ref = _make(cls, model, ctrl.horizon, ctrl.cost_fn, ctrl.num_simulated_paths, ctrl.gamma)
        ref._seed_rng.set_state(ctrl._seed_rng.get_state())
        got, want = _answers(ctrl, call, arg), _answers(ref, call, arg)
        _close(ref)
        assert got.keys() == want.keys() and [k for k in got if got[k] != want[k]] == []
        now = _engine(ctrl, model, batched)
        assert now._h is not None and now.num_paths == (B if batched else 1) * ctrl.num_simulated_paths
        if before is not None:
            assert (now is not before) == rebuilt
            assert (before._h is None) == rebuilt            # a replaced engine is closed, a kept one is not
        return now

    try:
        first = step(None, False)
        assert step(lambda: None, False) is first                              # two calls at one shape
        step(lambda: setattr(ctrl, "num_simulated_paths", K2), True)
        step(lambda: setattr(ctrl, "horizon", H - 1), True)
        if model != "reward":                                                  # the cost kind, there and back
            step(lambda: setattr(ctrl, "cost_fn", _terms()), True)
            step(lambda: setattr(ctrl, "cost_fn", _terms()), False)            # an equal TermCost: the same kind
            step(lambda: setattr(ctrl, "cost_fn", cheetah_cost_fn), True)
        else:                                                                  # the discount alone
            step(lambda: setattr(ctrl, "gamma", 0.5), False)
            step(lambda: setattr(ctrl, "gamma", 0.9), False)
        if model == "ens":                                                     # the rule alone
            step(lambda: setattr(ens, "rule", "mean_std"), False)
            step(lambda: setattr(ens, "kappa", 1.5), False)
            step(lambda: setattr(ens, "rule", "worst"), False)
    finally:
        ens.rule, ens.kappa = "mean", 0.0
        _close(ctrl)

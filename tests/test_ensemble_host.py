"""Model ensembles, host side (no GPU call): the definition ``ensemble.combine``, the bootstrap index lists,
the argument checks of the new C entry points (answered before any HIP call), the controllers' refusals,
and the constants ``_lib`` mirrors from include/bcmpc.h."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from conftest import REPO

S, A = 20, 6
RULES = ("mean", "mean_std", "worst")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).tobytes()


# ------------------------------------------------------------------ combine
@pytest.mark.parametrize("E", [1, 2, 3, 5, 16])
def test_combine_matches_independent_numpy_expressions(E):
    from bc_mpc_amd.ensemble import combine
    rs = np.random.RandomState(100 + E)
    c = rs.randn(E, 257) * 10.0 ** rs.randint(-3, 4, size=(1, 257))
    m = np.add.reduce(c, axis=0) / E                        # (in order: axis 0 of a 2-D array is not pairwise)
    seq = c[0].copy()
    for e in range(1, E):
        seq = seq + c[e]
    assert _bits(np.add.reduce(c, axis=0)) == _bits(seq)
    assert _bits(combine(c, "mean")) == _bits(m)
    for kappa in (0.0, 0.5, -1.0):
        # np.std about the same m: sqrt(mean(|c - m|^2)), the squares summed in member order
        q = np.add.reduce((c - m) * (c - m), axis=0)
        assert _bits(combine(c, "mean_std", kappa)) == _bits(m + kappa * np.sqrt(q / E))
    np.testing.assert_allclose(combine(c, "mean_std", 1.0), c.mean(0) + c.std(0), rtol=1e-12, atol=1e-12)
    assert _bits(combine(c, "worst")) == _bits(np.maximum.reduce(c))
    assert np.array_equal(combine(c, "worst"), c.max(axis=0))


def test_combine_special_values():
    from bc_mpc_amd.ensemble import combine
    nan, inf = np.nan, np.inf
    #             one NaN  all NaN  +inf  -inf  both   -0.0  overflow equal
    c = np.array([[1.0, nan, inf, -inf, inf, -0.0, 1e308, 2.5],
                  [nan, nan, 1.0, 1.0, -inf, -0.0, 1e308, 2.5],
                  [3.0, nan, 2.0, 2.0, 0.0, -0.0, 0.0, 2.5]])
    mean, std, worst = combine(c, "mean"), combine(c, "mean_std", 1.0), combine(c, "worst")
    assert np.array_equal(np.isnan(mean), [1, 1, 0, 0, 1, 0, 0, 0])
    assert mean[2] == inf and mean[3] == -inf and mean[6] == inf and mean[7] == 2.5
    assert _bits(mean[5]) == _bits(-0.0)
    assert np.array_equal(np.isnan(std), [1, 1, 1, 1, 1, 0, 0, 0])
    assert std[6] == inf and np.isnan(combine(c, "mean_std", -1.0)[6])      # inf + inf, inf - inf
    assert std[7] == 2.5 and _bits(combine(c, "mean_std", 3.0)[7]) == _bits(2.5)   # equal members: std exactly 0
    assert np.array_equal(np.isnan(worst), [1, 1, 0, 0, 0, 0, 0, 0])
    assert worst[2] == inf and worst[3] == 2.0 and worst[4] == inf and worst[6] == 1e308
    assert _bits(worst[5]) == _bits(-0.0)
    # E = 1 returns c[0] bit for bit under every rule that has no spread term, -0.0 and NaN included
    one = np.array([[-0.0, 1.5, nan, inf, -inf, 1e308]])
    for rule in ("mean", "worst"):
        got = combine(one, rule)
        assert np.array_equal(np.isnan(got), np.isnan(one[0]))
        ok = ~np.isnan(one[0])
        assert _bits(got[ok]) == _bits(one[0][ok])
    assert _bits(combine(one[:, :2], "mean_std", -1.0)) == _bits(one[0, :2])
    # any leading shape: elementwise over axis 0
    x = np.random.RandomState(0).randn(3, 4, 5)
    assert _bits(combine(x, "mean")) == _bits(((x[0] + x[1]) + x[2]) / 3.0)


def test_combine_refuses_bad_arguments():
    from bc_mpc_amd.ensemble import combine
    with pytest.raises(ValueError, match="rule"):
        combine(np.zeros((2, 3)), "median")
    with pytest.raises(ValueError, match="kappa"):
        combine(np.zeros((2, 3)), "mean_std", np.nan)
    with pytest.raises(ValueError):
        combine(np.zeros((0, 3)))


# ------------------------------------------------------------------ bootstrap index lists
def test_bootstrap_batches_are_deterministic_per_member_and_in_range():
    from bc_mpc_amd.ensemble import bootstrap_batches, member_rng
    state, np_state = random.getstate(), np.random.get_state()
    size, bs, iters = 200, 32, 3
    a = bootstrap_batches(member_rng(7, 0), size, bs, iters)
    b = bootstrap_batches(member_rng(7, 0), size, bs, iters)
    other = bootstrap_batches(member_rng(7, 1), size, bs, iters)
    reseeded = bootstrap_batches(member_rng(8, 0), size, bs, iters)
    assert len(a) == iters and all(x.shape == (bs,) and x.dtype == np.int64 for x in a)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not all(np.array_equal(x, y) for x, y in zip(a, other))
    assert not all(np.array_equal(x, y) for x, y in zip(a, reseeded))
    assert all(0 <= int(x.min()) and int(x.max()) < size for x in a + other)
    # a generator kept across calls goes on: the second fit's lists differ from the first's
    rng = member_rng(7, 0)
    first, second = bootstrap_batches(rng, size, bs, iters), bootstrap_batches(rng, size, bs, iters)
    assert all(np.array_equal(x, y) for x, y in zip(a, first))
    assert not all(np.array_equal(x, y) for x, y in zip(first, second))
    # a buffer smaller than the batch: every step takes all `size` rows of the resample
    small = bootstrap_batches(member_rng(1, 2), 5, 32, 2)
    assert all(x.shape == (5,) and int(x.max()) < 5 for x in small)
    # the global streams are not consumed
    assert random.getstate() == state
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), np_state))


# ------------------------------------------------------------------ the C entry points' argument checks
def _cfg(**kw):
    from bc_mpc_amd import _lib
    c = _lib.Config(state_dim=S, action_dim=A, hidden=64, n_layers=2, horizon=5, num_paths=16)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_ensemble_entry_points_check_arguments_without_a_gpu():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    cfg = _cfg()
    assert lib.bcmpc_ensemble_create(None, 3, ctypes.byref(h)) == _lib.ERR_ARG
    assert lib.bcmpc_ensemble_create(ctypes.byref(cfg), 3, None) == _lib.ERR_ARG
    for n in (0, 17, -1):
        assert lib.bcmpc_ensemble_create(ctypes.byref(cfg), n, ctypes.byref(h)) == _lib.ERR_ARG
        assert b"n_members" in lib.bcmpc_last_error() and not h.value
    for bad, word in ((dict(policy_hidden=64, policy_layers=2), b"policy"), (dict(model=_lib.MODEL_REWARD), b"reward"),
                      (dict(cost=_lib.COST_REWARD), b"reward"), (dict(cost=_lib.COST_NONE), b"fused cost")):
        c = _cfg(**bad)
        assert lib.bcmpc_ensemble_create(ctypes.byref(c), 2, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
        assert word in lib.bcmpc_last_error()
    assert lib.bcmpc_ensemble_destroy(None) == _lib.OK
    assert lib.bcmpc_ensemble_size(None) == 0
    assert lib.bcmpc_ensemble_member(None, 0, ctypes.byref(h)) == _lib.ERR_ARG
    # the rule: mode and kappa are judged before the handle
    assert lib.bcmpc_ensemble_set_rule(None, 3, 0.0) == _lib.ERR_ARG and b"mode" in lib.bcmpc_last_error()
    assert lib.bcmpc_ensemble_set_rule(None, -1, 0.0) == _lib.ERR_ARG and b"mode" in lib.bcmpc_last_error()
    for k in (float("nan"), float("inf")):
        assert lib.bcmpc_ensemble_set_rule(None, _lib.ENSEMBLE_MEAN_STD, k) == _lib.ERR_ARG
        assert b"kappa" in lib.bcmpc_last_error()
    assert lib.bcmpc_ensemble_set_rule(None, _lib.ENSEMBLE_MEAN, 0.0) == _lib.ERR_ARG
    assert b"null" in lib.bcmpc_last_error()
    # the calls
    res, st = _lib.Result(), (ctypes.c_double * S)()
    assert lib.bcmpc_ensemble_get_action(None, st, None, 0, 0, ctypes.byref(res), None, None) == _lib.ERR_ARG
    assert lib.bcmpc_ensemble_get_actions_batch(None, st, 1, None, 0, 0, ctypes.byref(res), None, None) == _lib.ERR_ARG
    cem, mppi, stats = _lib.Cem(3, 5, 0.1, 0), _lib.Mppi(3, 1.0, 0), _lib.MppiStats()
    mu = (ctypes.c_double * 30)()
    assert lib.bcmpc_ensemble_cem_get_action(None, st, ctypes.byref(cem), 0, mu, mu, ctypes.byref(res)) == _lib.ERR_ARG
    assert lib.bcmpc_ensemble_mppi_get_action(None, st, ctypes.byref(mppi), 0, mu, mu, ctypes.byref(res),
                                              ctypes.byref(stats)) == _lib.ERR_ARG
    # the stream-ordered reduce: scalars first, then pointers
    red = lib.bcmpc_ensemble_reduce_async
    for n in (0, 17):
        assert red(None, None, 8, n, 8, 0, 0.0, None, None) == _lib.ERR_ARG and b"n_members" in lib.bcmpc_last_error()
    assert red(None, None, 8, 2, 8, 3, 0.0, None, None) == _lib.ERR_ARG and b"mode" in lib.bcmpc_last_error()
    assert red(None, None, 8, 2, 8, 1, float("nan"), None, None) == _lib.ERR_ARG and b"kappa" in lib.bcmpc_last_error()
    assert red(None, None, 8, 2, 0, 0, 0.0, None, None) == _lib.ERR_ARG and b"K" in lib.bcmpc_last_error()
    assert red(None, None, 7, 2, 8, 0, 0.0, None, None) == _lib.ERR_ARG and b"ld" in lib.bcmpc_last_error()
    assert red(None, None, 8, 2, 8, 0, 0.0, None, None) == _lib.ERR_ARG and b"null" in lib.bcmpc_last_error()


def test_lib_constants_mirror_the_header():
    from bc_mpc_amd import _lib
    text = open(os.path.join(REPO, "include", "bcmpc.h")).read()
    assert int(re.search(r"#define BCMPC_MAX_MEMBERS (\d+)", text).group(1)) == _lib.MAX_MEMBERS == 16
    assert int(re.search(r"#define BCMPC_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 5
    for name, value in (("MEAN", _lib.ENSEMBLE_MEAN), ("MEAN_STD", _lib.ENSEMBLE_MEAN_STD),
                        ("WORST", _lib.ENSEMBLE_WORST)):
        assert int(re.search(rf"BCMPC_ENSEMBLE_{name} = (\d+)", text).group(1)) == value
    assert _lib.ENSEMBLE_RULES == {"mean": 0, "mean_std": 1, "worst": 2}
    from bc_mpc_amd import ensemble
    assert ensemble.RULES == tuple(sorted(_lib.ENSEMBLE_RULES, key=_lib.ENSEMBLE_RULES.get))


# ------------------------------------------------------------------ the model and the controllers' refusals
class _Box:
    low, high = -np.ones(A), np.ones(A)
    shape = (A,)


class _Env:
    action_space = _Box()

    class observation_space:
        shape = (S,)


def _model(**kw):
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel
    from oracle import mpc_oracle as orc
    return EnsembleDynamicsModel(_Env(), 3, 2, 64, "tanh", None, orc.synthetic_normalization(), 32, 3, 1e-3, **kw)


def test_model_members_are_seeded_per_member():
    from bc_mpc_amd.dynamics import NNDynamicsModel
    from oracle import mpc_oracle as orc
    m = _model(seed=5)
    assert m.is_ensemble and m.n_models == 3 and m.rule == "mean" and m.kappa == 0.0 and not m.diagnostics
    for i, mem in enumerate(m.members):
        solo = NNDynamicsModel(_Env(), 2, 64, "tanh", None, orc.synthetic_normalization(), 32, 3, 1e-3, seed=5 + i)
        assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(mem.kernels, solo.kernels))
    assert not np.array_equal(m.members[0].kernels[0].numpy(), m.members[1].kernels[0].numpy())
    v = m.version
    spec = m.members[1].mlp_spec()
    m.load_weights(1, spec.kernels, spec.biases)
    assert m.version > v
    for bad in (dict(rule="median"), dict(kappa=float("inf"))):
        with pytest.raises(ValueError):
            _model(**bad)
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel
    for n in (0, 17):
        with pytest.raises(ValueError, match="n_models"):
            EnsembleDynamicsModel(_Env(), n, 2, 64, "tanh", None, orc.synthetic_normalization(), 32, 3, 1e-3)


def _controllers(model, cost_fn, **kw):
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller
    return [MPCcontroller(_Env(), model, horizon=5, cost_fn=cost_fn, num_simulated_paths=37, rng="device", seed=1, **kw),
            MPCcontroller(_Env(), model, horizon=5, cost_fn=cost_fn, num_simulated_paths=37, rng="numpy", **kw),
            CEMcontroller(_Env(), model, horizon=5, cost_fn=cost_fn, num_simulated_paths=37, **kw),
            MPPIcontroller(_Env(), model, horizon=5, cost_fn=cost_fn, num_simulated_paths=37, **kw)]


@pytest.fixture
def no_engines(monkeypatch):
    """No refusal may get as far as creating an engine."""
    from bc_mpc_amd import ensemble

    def boom(*a, **k):
        raise AssertionError("an EnsembleEngine was created")
    monkeypatch.setattr(ensemble, "EnsembleEngine", boom)


def test_controllers_refuse_a_user_cost_callable(no_engines):
    def my_cost(s, a, ns):
        return 0.0
    for c in _controllers(_model(), my_cost):
        with pytest.raises(ValueError, match="cheetah cost_fn or a TermCost"):
            c.get_action(np.zeros(S))
    from bc_mpc_amd import MPCcontroller
    c = MPCcontroller(_Env(), _model(), horizon=5, cost_fn=my_cost, num_simulated_paths=37, rng="device", seed=1)
    with pytest.raises(ValueError, match="cheetah cost_fn or a TermCost"):
        c.get_actions(np.zeros((2, S)))


def test_controllers_refuse_a_world_above_one(no_engines, monkeypatch):
    from bc_mpc_amd import cheetah_cost_fn, distributed
    monkeypatch.setattr(distributed, "world", lambda group=None: (0, 2))
    for c in _controllers(_model(), cheetah_cost_fn, process_group=object()):
        with pytest.raises(NotImplementedError, match="one rank"):
            c.get_action(np.zeros(S))


def test_controllers_refuse_reward_model_members(no_engines):
    from bc_mpc_amd import cheetah_cost_fn
    from bc_mpc_amd.dynamics import NNDynamicsRewardModel
    from oracle import mpc_oracle as orc
    m = _model()
    m.members = [NNDynamicsRewardModel(_Env(), orc.synthetic_normalization(reward=True), 32, 3, 1e-3, size=64, seed=i)
                 for i in range(2)]
    for c in _controllers(m, cheetah_cost_fn):
        with pytest.raises(TypeError, match="reward-model ensembles"):
            c.get_action(np.zeros(S))


def test_batched_planners_over_an_ensemble_are_not_built(no_engines):
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    for cls in (CEMcontroller, MPPIcontroller):
        c = cls(_Env(), _model(), horizon=5, cost_fn=cheetah_cost_fn, num_simulated_paths=37)
        with pytest.raises(NotImplementedError, match="EnsembleDynamicsModel"):
            c.get_actions(np.zeros((2, S)))

"""Batched CEM / MPPI, the host side, no GPU: the seven new symbols (ABI still 5), argument errors that are
answered before any HIP call, and the controllers' per-environment warm-start logic driven through a stub
engine.  The kernels are pinned in tests/test_gpu_plan_batch.py."""
import ctypes

import numpy as np
import pytest

NEW = {"bcmpc_cem_get_actions_batch": 10, "bcmpc_mppi_get_actions_batch": 11, "bcmpc_plan_sample_async": 10,
       "bcmpc_plan_argmin_async": 9, "bcmpc_select_batch_async": 9, "bcmpc_cem_refit_batch_async": 14,
       "bcmpc_mppi_update_batch_async": 13}


def test_symbols_are_exported_and_abi_is_still_5():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_abi_version() == 5 == _lib.ABI_VERSION
    bound = {s[0]: s for s in _lib.SIGNATURES}
    for name, nargs in NEW.items():
        assert name in bound
        fn = getattr(lib, name)                       # AttributeError on a library without the batched planners
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == bound[name][2]
        assert len(bound[name][2]) == nargs, name


def test_header_no_longer_says_cem_has_no_batched_form():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for rel in ("include/bcmpc.h", "INTEGRATION.md"):
        text = open(os.path.join(root, rel)).read()
        assert "CEM has no batched form" not in text, rel
        for name in NEW:
            assert name in text, (rel, name)


def _calls(lib, n_envs, null):
    """Every new entry point with n_envs environments; null=True: without an engine."""
    from bc_mpc_amd import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    B = max(n_envs, 1)
    states, mu, sd = np.zeros((B, 20)), np.zeros((B, 3, 6)), np.ones((B, 3, 6))
    out, stats = (_lib.Result * B)(), (_lib.MppiStats * B)()
    cem, mppi = _lib.Cem(1, 2, 0.1, 0), _lib.Mppi(1, 1.0, 0)
    e = None
    assert null
    P = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    return [
        lib.bcmpc_cem_get_actions_batch(e, P(states), n_envs, ctypes.byref(cem), 0, 0, P(mu), P(sd), out, None),
        lib.bcmpc_mppi_get_actions_batch(e, P(states), n_envs, ctypes.byref(mppi), 0, 0, P(mu), P(sd), out, stats, None),
        lib.bcmpc_plan_sample_async(e, None, None, n_envs, 4, 0, 0, 0, None, None),
        lib.bcmpc_plan_argmin_async(e, None, None, n_envs, 4, 0, 0, None, None),
        lib.bcmpc_select_batch_async(e, None, n_envs, 4, 0, 2, None, None, None),
        lib.bcmpc_cem_refit_batch_async(e, None, None, n_envs, 2, 0, 0, 0.1, None, None, None, 4, 0, None),
        lib.bcmpc_mppi_update_batch_async(e, None, n_envs, 4, 0, 0, 0, 1.0, None, None, None, None, None),
    ]


def test_null_arguments_are_argument_errors_without_hip():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    for rc in _calls(lib, 2, True):
        assert rc == _lib.ERR_ARG
        assert b"null" in lib.bcmpc_last_error()
    with pytest.raises(ValueError):
        _lib.check(_lib.ERR_ARG)


@pytest.mark.parametrize("n_envs", [0, -3])
def test_n_envs_below_one_is_an_argument_error_without_hip(n_envs):
    from bc_mpc_amd import _lib
    lib = _lib.load()
    for rc in _calls(lib, n_envs, True):
        assert rc == _lib.ERR_ARG
        assert b"n_envs" in lib.bcmpc_last_error()


def test_mppi_stats_record_matches_the_c_struct():
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import MPPI_STATS
    assert MPPI_STATS.itemsize == ctypes.sizeof(_lib.MppiStats) == 32
    assert list(MPPI_STATS.names) == [f[0] for f in _lib.MppiStats._fields_]
    assert [MPPI_STATS.fields[n][1] for n in MPPI_STATS.names] == [getattr(_lib.MppiStats, n).offset
                                                                  for n in MPPI_STATS.names]


# ------------------------------------------------------------------ controllers on a stub engine
H, A, S, K = 4, 6, 20, 16
LOW = np.array([-1, -1, -2, 0, -1, -1], np.float32)
HIGH = np.array([1, 1, 2, 4, 1, 1], np.float32)
MID = np.array([0, 0, 0, 2, 0, 0], np.float64)


class _Box:
    low, high = LOW, HIGH
    shape = (A,)


class _Env:
    action_space = _Box()

    class observation_space:
        shape = (S,)


class _StubEngine:
    """Records what the controller hands to the engine and answers with recognisable plans:
    mu'[b, h, j] = 1000 * call + 100 * b + 10 * h + j (clipped into the box by nobody: this is host logic)."""

    def __init__(self, k_total):
        self.k_total = k_total
        self.calls = []

    def set_weights(self, spec, norm, version):
        pass

    def _answer(self, states, mu):
        from bc_mpc_amd.engine import BatchResult
        B = states.shape[0]
        call = len(self.calls)
        new = (1000.0 * call + 100.0 * np.arange(B)[:, None, None] + 10.0 * np.arange(H)[None, :, None]
               + np.arange(A)[None, None, :])
        res = BatchResult(np.arange(B, dtype=np.int64), np.arange(B, dtype=np.float64), np.full((B, A), 0.25))
        return res, new

    def cem_get_actions(self, states, mu, sigma, iterations, n_elite, alpha, seed, cand_offset=0, return_costs=False):
        self.calls.append(dict(states=states.copy(), mu=mu.copy(), sigma=sigma.copy(), iterations=iterations,
                               n_elite=n_elite, alpha=alpha, seed=seed))
        res, new = self._answer(states, mu)
        return res, new, 0.5 * sigma

    def mppi_get_actions(self, states, mu, sigma, iterations, temperature, seed, cand_offset=0, return_costs=False):
        from bc_mpc_amd.engine import MPPI_STATS
        self.calls.append(dict(states=states.copy(), mu=mu.copy(), sigma=sigma.copy(), iterations=iterations,
                               temperature=temperature, seed=seed))
        res, new = self._answer(states, mu)
        stats = np.zeros(states.shape[0], dtype=MPPI_STATS)
        stats["ess"] = 2.0 + np.arange(states.shape[0])
        return res, new, stats


def _ctrl(kind, monkeypatch, **kw):
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    from oracle import mpc_oracle as orc
    dyn = orc.NumpyDynamics(orc.synthetic_weights(S, A, 32, 2, "tanh", False), orc.synthetic_normalization())
    cls = CEMcontroller if kind == "cem" else MPPIcontroller
    c = cls(_Env(), dyn, horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, seed=5, **kw)
    engines = []

    def engine_for(spec, S_, A_, k_total):
        if not engines or engines[-1].k_total != k_total:
            engines.append(_StubEngine(k_total))
        return engines[-1]
    monkeypatch.setattr(c, "_batch_engine_for", engine_for)
    return c, engines


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_per_environment_warm_start_reset_and_change_of_B(kind, monkeypatch):
    c, engines = _ctrl(kind, monkeypatch)
    B = 3
    states = np.arange(B * S, dtype=np.float64).reshape(B, S)
    cold = np.tile(MID, (B, H, 1))
    sd = np.tile(np.array([0.5, 0.5, 1, 1, 0.5, 0.5]), (B, H, 1))             # (high - low) / 4
    seeds = np.random.RandomState(5).randint(0, 2**62, size=4, dtype=np.int64)  # one seed per call

    got = c.get_actions(states)
    eng = engines[0]
    assert eng.k_total == B * K and len(eng.calls) == 1
    first = eng.calls[0]
    assert np.array_equal(first["states"], states) and first["seed"] == int(seeds[0])
    assert np.array_equal(first["mu"], cold) and np.array_equal(first["sigma"], sd)
    plan1 = c.last_mu.copy()
    assert plan1.shape == (B, H, A) and got.shape == (B, A) and got.dtype == np.float64
    if kind == "cem":
        assert first["n_elite"] == 2 and np.array_equal(got, np.full((B, A), 0.25))   # the best sample's action
        assert c.last_sigma.shape == (B, H, A)
    else:
        assert np.array_equal(got, plan1[:, 0])                                        # mu'[b, 0]
        assert np.array_equal(c.last_ess, [2.0, 3.0, 4.0]) and c.last_stats.shape == (B,)
    assert np.array_equal(c.last_cost, [0.0, 1.0, 2.0]) and np.array_equal(c.last_position, [0, 1, 2])

    # second call: every environment's own plan shifted by one step, the box centre appended; sigma afresh
    c.get_actions(states)
    second = eng.calls[1]
    assert second["seed"] == int(seeds[1])
    for b in range(B):
        assert np.array_equal(second["mu"][b, :-1], plan1[b, 1:]) and np.array_equal(second["mu"][b, -1], MID)
    assert np.array_equal(second["sigma"], sd)
    plan2 = c.last_mu.copy()

    # reset([1]) re-centres environment 1 only
    c.reset([1])
    c.get_actions(states)
    third = eng.calls[2]
    assert np.array_equal(third["mu"][1], cold[1])
    for b in (0, 2):
        assert np.array_equal(third["mu"][b, :-1], plan2[b, 1:]) and np.array_equal(third["mu"][b, -1], MID)

    # a change of B resets every plan (and asks for an engine of the new size); get_action's plan is separate
    c._mu = np.full((H, A), 7.0)
    c.get_actions(states[:2])
    assert engines[-1].k_total == 2 * K and np.array_equal(engines[-1].calls[0]["mu"], cold[:2])
    assert np.array_equal(c.initial_distribution()[0][:-1], np.full((H - 1, A), 7.0))
    c.reset([0])
    assert c._mu is not None                        # per-environment reset leaves get_action's plan alone
    c.reset()
    assert c._mu is None and c._bmu is None
    c.get_actions(states[:2])
    assert np.array_equal(engines[-1].calls[1]["mu"], cold[:2])


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_warm_start_off_and_shape_errors(kind, monkeypatch):
    c, engines = _ctrl(kind, monkeypatch, warm_start=False, init_std=0.3)
    states = np.zeros((2, S))
    c.get_actions(states)
    c.get_actions(states)
    assert np.array_equal(engines[0].calls[1]["mu"], np.tile(MID, (2, H, 1)))
    assert (engines[0].calls[1]["sigma"] == 0.3).all()
    for bad in (np.zeros(S), np.zeros((2, S + 1)), np.zeros((0, S))):
        with pytest.raises(ValueError, match="states shape"):
            c.get_actions(bad)
    c.horizon = 0
    with pytest.raises(IndexError):
        c.get_actions(states)
    c.horizon, c.num_simulated_paths = H, 0
    with pytest.raises(ValueError, match="empty sequence"):
        c.get_actions(states)


def test_world_size_above_one_is_not_implemented(monkeypatch):
    from bc_mpc_amd import distributed
    for kind in ("cem", "mppi"):
        c, engines = _ctrl(kind, monkeypatch)
        monkeypatch.setattr(distributed, "world", lambda group=None: (0, 2))
        with pytest.raises(NotImplementedError, match="one rank"):
            c.get_actions(np.zeros((2, S)))
        assert not engines


def test_constructor_checks_are_unchanged():
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    mk = lambda cls, **kw: cls(_Env(), object(), horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, **kw)   # noqa: E731
    with pytest.raises(ValueError):
        mk(CEMcontroller, iterations=0)
    with pytest.raises(ValueError):
        mk(MPPIcontroller, iterations=0)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mk(MPPIcontroller, temperature=t)
    c = mk(CEMcontroller, elite_frac=0.25)
    assert c.n_elite == 4 and c.last_mu is None and c._bmu is None and c._batch_engine is None
    m = mk(MPPIcontroller, temperature=2.5, iterations=3)
    assert m.temperature == 2.5 and m.iterations == 3 and m.last_ess is None and m._bmu is None

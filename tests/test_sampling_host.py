"""Correlated sampling noise and elite carry-over, the host side, no GPU: the definition (bc_mpc_amd/sampling.py),
the controllers' arguments and refusals, the bindings of the new symbols, and that the defaults keep calling the
symbols they have always called.  The kernels are pinned in tests/test_gpu_sampling.py.

The statistics' bound: on z = oracle.cem_normals(seed, 0, 0, 4096, 32, 6), seeds 1..3, rho in {0.5, 0.9}, the
largest deviation of the lag-1 product mean from rho and of the variance from 1 is 0.0121 (seed 1, rho 0.9) on
the definition; the bound 0.03 is 2.5 times that.  The inputs are fixed, so the test is deterministic."""
import ctypes
import functools

import numpy as np
import pytest

S, A, H, K = 20, 6, 4, 16
NEW = {"bcmpc_cem_get_action_s": 8, "bcmpc_mppi_get_action_s": 9, "bcmpc_cem_get_actions_batch_s": 11,
       "bcmpc_mppi_get_actions_batch_s": 12, "bcmpc_plan_sample_corr_async": 14, "bcmpc_plan_keep_async": 11}


# ------------------------------------------------------------------ ar1_noise
@functools.lru_cache(maxsize=None)
def _normals(seed):
    from oracle import mpc_oracle as orc
    z = orc.cem_normals(seed, 0, 0, 4096, 32, 6)
    z.setflags(write=False)
    return z


def test_ar1_rho_zero_and_one_step_are_the_input_bits():
    from bc_mpc_amd.sampling import ar1_noise
    from oracle import mpc_oracle as orc
    z = orc.cem_normals(7, 2, 100, 65, 7, 6)
    assert ar1_noise(z, 0.0).tobytes() == z.tobytes()
    for rho in (0.0, 0.5, 0.9):
        assert ar1_noise(z[:1], rho).tobytes() == z[:1].tobytes()
    assert ar1_noise(z, 0.5).tobytes() != z.tobytes()


@pytest.mark.parametrize("rho", [0.25, 0.5, 0.9, 0.999])
def test_ar1_recursion_is_the_scalar_loop(rho):
    import math
    from bc_mpc_amd.sampling import ar1_noise
    from oracle import mpc_oracle as orc
    z = orc.cem_normals(11, 1, 0, 9, 6, 3)
    n = ar1_noise(z, rho)
    c = math.sqrt(1.0 - rho * rho)
    for k in range(z.shape[1]):
        for j in range(z.shape[2]):
            prev = float(z[0, k, j])
            assert n[0, k, j] == prev
            for h in range(1, z.shape[0]):
                p, q = rho * prev, c * float(z[h, k, j])     # two rounded products, one rounded sum
                prev = p + q
                assert np.float64(prev).tobytes() == n[h, k, j].tobytes(), (h, k, j)


@pytest.mark.parametrize("rho", [0.5, 0.9])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ar1_statistics(seed, rho):
    from bc_mpc_amd.sampling import ar1_noise
    n = ar1_noise(_normals(seed), rho)
    lag1 = float(np.mean(n[1:] * n[:-1]))
    var = float(np.var(n))
    print(f"seed {seed} rho {rho}: lag-1 {lag1:.6f} (dev {abs(lag1 - rho):.6f}), var {var:.6f} (dev {abs(var - 1):.6f})")
    assert abs(lag1 - rho) <= 0.03
    assert abs(var - 1.0) <= 0.03


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf"), "x", None])
def test_ar1_refuses_rho_outside_the_unit_interval(bad):
    from bc_mpc_amd.sampling import ar1_noise
    with pytest.raises(ValueError, match="rho"):
        ar1_noise(np.zeros((2, 3)), bad)


def test_correlated_actions_is_clip_of_mu_plus_sigma_n():
    from bc_mpc_amd.sampling import ar1_noise, correlated_actions
    from oracle import mpc_oracle as orc
    Hh, Kk, Aa = 5, 33, 3
    rs = np.random.RandomState(0)
    mu, sd = rs.uniform(-0.5, 0.5, (Hh, Aa)), rs.uniform(0.2, 3.0, (Hh, Aa))
    low, high = -np.ones(Aa), np.ones(Aa)
    z = orc.cem_normals(5, 0, 0, Kk, Hh, Aa)
    got = correlated_actions(z, 0.5, mu, sd, low, high)
    n = ar1_noise(z, 0.5)
    for h in range(Hh):
        for j in range(Aa):
            want = np.minimum(np.maximum(mu[h, j] + sd[h, j] * n[h, :, j], low[j]), high[j])
            assert got[h, :, j].tobytes() == want.tobytes()
    assert (got == 1.0).any() and (got == -1.0).any() and (np.abs(got) < 1.0).any()
    # rho = 0: the planners' independent sample
    assert correlated_actions(z, 0.0, mu, sd, low, high).tobytes() == orc.cem_actions(5, 0, 0, Kk, Hh, mu, sd, low,
                                                                                    high).tobytes()


# ------------------------------------------------------------------ refit_from_actions, carry_elites
@pytest.mark.parametrize("n", [1, 40, 64, 65, 130])
def test_refit_from_actions_equals_the_oracle_refit_on_uncorrelated_elites(n):
    from bc_mpc_amd.sampling import refit_from_actions
    from oracle import mpc_oracle as orc
    Hh, Aa, seed, it, alpha = 3, 6, 0xFEED + n, 2, 0.1
    rs = np.random.RandomState(n)
    mu, sd = rs.uniform(-0.6, 0.6, (Hh, Aa)), rs.uniform(0.1, 0.9, (Hh, Aa))
    low, high = -np.ones(Aa), np.ones(Aa)
    elite = np.sort(rs.choice(400, n, replace=False)).astype(np.int64) + 1000
    want_mu, want_sd = orc.cem_refit(elite, seed, it, mu, sd, low, high, alpha)
    acts = orc.cem_actions(seed, it, 0, 0, Hh, mu, sd, low, high, index=elite)        # [H, n, A]
    got_mu, got_sd = refit_from_actions(acts.transpose(1, 0, 2), mu, sd, alpha)
    assert got_mu.tobytes() == want_mu.tobytes() and got_sd.tobytes() == want_sd.tobytes()


def test_refit_from_actions_without_elites_changes_nothing():
    from bc_mpc_amd.sampling import refit_from_actions
    mu, sd = np.full((2, 3), 0.25), np.full((2, 3), 0.5)
    m, s = refit_from_actions(np.zeros((0, 2, 3)), mu, sd, 0.1)
    assert m.tobytes() == mu.tobytes() and s.tobytes() == sd.tobytes() and m is not mu
    with pytest.raises(ValueError, match="shape"):
        refit_from_actions(np.zeros((2, 3, 3)), mu, sd, 0.1)


def test_carry_elites_column_bookkeeping():
    from bc_mpc_amd.sampling import carry_elites
    Hh, Kk, Aa = 3, 5, 2
    new = np.arange(Hh * Kk * Aa, dtype=np.float64).reshape(Hh, Kk, Aa)
    prev = 1000.0 + new
    # n = 0: iteration 0, or nothing selected
    assert carry_elites(new, prev, []).tobytes() == new.tobytes()
    # n = 1
    one = carry_elites(new, prev, [3])
    assert np.array_equal(one[:, 0], prev[:, 3]) and np.array_equal(one[:, 1:], new[:, 1:])
    # select's order is ascending index; the columns land in that order
    two = carry_elites(new, prev, [1, 4])
    assert np.array_equal(two[:, 0], prev[:, 1]) and np.array_equal(two[:, 1], prev[:, 4])
    assert np.array_equal(two[:, 2:], new[:, 2:])
    # n = K: the whole population is the previous one
    assert carry_elites(new, prev, np.arange(Kk)).tobytes() == prev.tobytes()
    assert new[0, 0, 0] == 0.0                           # (the inputs are not written)
    with pytest.raises(ValueError, match="do not fit"):
        carry_elites(new, prev, np.arange(Kk + 1) % Kk)


# ------------------------------------------------------------------ bindings
def test_new_symbols_are_bound_and_abi_is_still_5():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_abi_version() == 5 == _lib.ABI_VERSION
    bound = {s[0]: s for s in _lib.SIGNATURES}
    for name, nargs in NEW.items():
        assert name in bound
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == bound[name][2]
        assert len(bound[name][2]) == nargs, name
    assert ctypes.sizeof(_lib.Sampling) == 16
    assert [f[0] for f in _lib.Sampling._fields_] == ["rho", "keep_elites", "reserved"]


def test_null_engine_is_an_argument_error_without_hip():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    P = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    st, mu, sd = np.zeros((1, S)), np.zeros((1, H, A)), np.ones((1, H, A))
    out, stats = (_lib.Result * 1)(), (_lib.MppiStats * 1)()
    cem, mppi, smp = _lib.Cem(2, 2, 0.1, 0), _lib.Mppi(1, 1.0, 0), _lib.Sampling(0.5, 0, 0)
    rcs = [
        lib.bcmpc_cem_get_action_s(None, P(st), ctypes.byref(cem), ctypes.byref(smp), 0, P(mu), P(sd), out),
        lib.bcmpc_mppi_get_action_s(None, P(st), ctypes.byref(mppi), ctypes.byref(smp), 0, P(mu), P(sd), out, stats),
        lib.bcmpc_cem_get_actions_batch_s(None, P(st), 1, ctypes.byref(cem), ctypes.byref(smp), 0, 0, P(mu), P(sd), out,
                                          None),
        lib.bcmpc_mppi_get_actions_batch_s(None, P(st), 1, ctypes.byref(mppi), ctypes.byref(smp), 0, 0, P(mu), P(sd),
                                           out, stats, None),
        lib.bcmpc_plan_sample_corr_async(None, None, None, 1, 4, 0, 0, 0, 0.5, None, None, 0, None, None),
        lib.bcmpc_plan_keep_async(None, None, None, None, 1, 4, 0, 2, None, None, None),
    ]
    for rc in rcs:
        assert rc == _lib.ERR_ARG
    assert b"null" in lib.bcmpc_last_error()


# ------------------------------------------------------------------ the engine methods at the defaults
class _Recorder:
    """A stand-in for the loaded library: records the symbol every call goes to and answers BCMPC_OK."""

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        def fn(*args):
            self.names.append(name)
            return 0
        return fn


def _bare_engine(K_total=K):
    from bc_mpc_amd.engine import RolloutEngine
    eng = RolloutEngine.__new__(RolloutEngine)
    eng._lib, eng._h = _Recorder(), None
    eng.state_dim, eng.action_dim, eng.horizon, eng.num_paths = S, A, H, K_total
    return eng


def test_default_sampling_calls_the_symbols_it_always_called():
    eng = _bare_engine(2 * K)
    st, mu, sd = np.zeros(S), np.zeros((H, A)), np.ones((H, A))
    bst, bmu, bsd = np.zeros((2, S)), np.zeros((2, H, A)), np.ones((2, H, A))
    eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1)
    eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, rho=0.0, keep_elites=False)
    eng.mppi_get_action(st, mu, sd, 1, 1.0, 1)
    eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, rho=0.0)
    eng.cem_get_actions(bst, bmu, bsd, 2, 2, 0.1, 1)
    eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1)
    assert eng._lib.names == ["bcmpc_cem_get_action"] * 2 + ["bcmpc_mppi_get_action"] * 2 + [
        "bcmpc_cem_get_actions_batch", "bcmpc_mppi_get_actions_batch"]
    eng._lib.names.clear()
    eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, rho=0.5)
    eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, keep_elites=True)
    eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, rho=0.5)
    eng.cem_get_actions(bst, bmu, bsd, 2, 2, 0.1, 1, rho=0.9, keep_elites=True)
    eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, rho=0.9)
    assert eng._lib.names == ["bcmpc_cem_get_action_s"] * 2 + ["bcmpc_mppi_get_action_s",
                                                               "bcmpc_cem_get_actions_batch_s",
                                                               "bcmpc_mppi_get_actions_batch_s"]
    eng._lib.names.clear()
    for bad in (-0.5, 1.0, float("nan")):
        with pytest.raises(ValueError, match="rho"):
            eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, rho=bad)
        with pytest.raises(ValueError, match="rho"):
            eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, rho=bad)
    with pytest.raises(ValueError, match="keep_elites"):
        eng.cem_get_actions(bst, bmu, bsd, 2, 2, 0.1, 1, keep_elites=2)
    with pytest.raises(TypeError):
        eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, keep_elites=True)      # MPPI has no elites
    assert eng._lib.names == []


def test_ensemble_engine_has_no_sampling_entry():
    from bc_mpc_amd.ensemble import EnsembleEngine
    eng = EnsembleEngine.__new__(EnsembleEngine)
    eng._lib, eng._h = _Recorder(), None
    eng.state_dim, eng.action_dim, eng.horizon, eng.num_paths = S, A, H, K
    st, mu, sd = np.zeros(S), np.zeros((H, A)), np.ones((H, A))
    eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1)
    assert eng._lib.names == ["bcmpc_ensemble_cem_get_action"]
    with pytest.raises(NotImplementedError, match="ensembles"):
        eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, rho=0.5)
    with pytest.raises(NotImplementedError, match="ensembles"):
        eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, rho=0.5)
    assert eng._lib.names == ["bcmpc_ensemble_cem_get_action"]


# ------------------------------------------------------------------ controllers
class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32)


class _Env:
    def __init__(self):
        self.observation_space, self.action_space = _Space(S), _Space(A)


def _delta():
    from oracle import mpc_oracle as orc
    return orc.NumpyDynamics(orc.synthetic_weights(S, A, 64, 2, "tanh", False), orc.synthetic_normalization(S, A))


def _ensemble():
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel
    from oracle import mpc_oracle as orc
    return EnsembleDynamicsModel(_Env(), 2, 2, 64, "tanh", None, orc.synthetic_normalization(S, A), 32, 3, 1e-3)


def _mk(kind, model=None, **kw):
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    cls = CEMcontroller if kind == "cem" else MPPIcontroller
    return cls(_Env(), model if model is not None else object(), horizon=H, cost_fn=cheetah_cost_fn,
               num_simulated_paths=K, seed=5, **kw)


def test_controller_constructor_values():
    c = _mk("cem")
    assert c.noise_rho == 0.0 and c.keep_elites is False and c._sampling_args() == {}
    c = _mk("cem", noise_rho=0.5, keep_elites=True)
    assert c._sampling_args() == {"rho": 0.5, "keep_elites": True}
    assert _mk("cem", keep_elites=True)._sampling_args() == {"keep_elites": True}
    m = _mk("mppi", noise_rho=0.9)
    assert m.noise_rho == 0.9 and m._sampling_args() == {"rho": 0.9}
    for kind in ("cem", "mppi"):
        for bad in (-0.1, 1.0, 2.0, float("nan"), float("inf"), "half"):
            with pytest.raises(ValueError, match="rho"):
                _mk(kind, noise_rho=bad)
    for bad in (2, -1, "yes", None, 0.5):
        with pytest.raises(ValueError, match="keep_elites"):
            _mk("cem", keep_elites=bad)
    with pytest.raises(TypeError):
        _mk("mppi", keep_elites=True)
    # read on every call: a value set later is checked when it is used
    c = _mk("cem")
    c.noise_rho = 1.5
    with pytest.raises(ValueError, match="rho"):
        c._sampling_args()


class _StubEngine:
    def __init__(self):
        self.calls = []

    def set_weights(self, *a):
        pass

    def cem_get_action(self, state, mu, sigma, iterations, n_elite, alpha, seed, **kw):
        from bc_mpc_amd.engine import StepResult
        self.calls.append(("cem", seed, kw))
        return StepResult(0, 1.0, np.zeros(A), None), mu, sigma

    def cem_get_actions(self, states, mu, sigma, iterations, n_elite, alpha, seed, **kw):
        from bc_mpc_amd.engine import BatchResult
        self.calls.append(("cems", seed, kw))
        B = states.shape[0]
        return BatchResult(np.zeros(B, np.int64), np.zeros(B), np.zeros((B, A))), mu, sigma

    def mppi_get_action(self, state, mu, sigma, iterations, temperature, seed, **kw):
        from bc_mpc_amd import _lib
        from bc_mpc_amd.engine import StepResult
        self.calls.append(("mppi", seed, kw))
        return StepResult(0, 1.0, np.zeros(A), None), mu, _lib.MppiStats(1.0, 1.0, 0.0, 1)

    def mppi_get_actions(self, states, mu, sigma, iterations, temperature, seed, **kw):
        from bc_mpc_amd.engine import MPPI_STATS, BatchResult
        self.calls.append(("mppis", seed, kw))
        B = states.shape[0]
        return BatchResult(np.zeros(B, np.int64), np.zeros(B), np.zeros((B, A))), mu, np.zeros(B, dtype=MPPI_STATS)


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_controllers_hand_their_sampling_to_the_engine_calls(kind, monkeypatch):
    kw = dict(noise_rho=0.5, keep_elites=True) if kind == "cem" else dict(noise_rho=0.5)
    want = dict(rho=0.5, keep_elites=True) if kind == "cem" else dict(rho=0.5)
    c = _mk(kind, _delta(), **kw)
    eng = _StubEngine()
    monkeypatch.setattr(c, "_engine_for", lambda *a: eng)
    monkeypatch.setattr(c, "_batch_engine_for", lambda *a: eng)
    seeds = [int(x) for x in np.random.RandomState(5).randint(0, 2**62, size=3, dtype=np.int64)]
    c.get_action(np.zeros(S))
    c.get_actions(np.zeros((2, S)))
    c.noise_rho, c.keep_elites = 0.0, False                 # read on every call; nothing is rebuilt
    c.get_action(np.zeros(S))
    assert eng.calls == [(kind, seeds[0], want), (kind + "s", seeds[1], want), (kind, seeds[2], {})]


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_ensemble_and_rank_refusals_do_not_consume_a_seed(kind, monkeypatch):
    from bc_mpc_amd import distributed, ensemble
    kw = dict(noise_rho=0.5, keep_elites=True) if kind == "cem" else dict(noise_rho=0.5)

    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(ensemble, "_ctrl_engine", boom)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))   # noqa: E731
    # an EnsembleDynamicsModel
    c = _mk(kind, _ensemble(), **kw)
    before = c._seed_rng.get_state()
    with pytest.raises(NotImplementedError, match="noise_rho / keep_elites.*EnsembleDynamicsModel"):
        c.get_action(np.zeros(S))
    with pytest.raises(NotImplementedError, match="EnsembleDynamicsModel"):
        c.get_actions(np.zeros((2, S)))
    assert same(before, c._seed_rng.get_state()) and c._engine is None and c._batch_engine is None
    # more than one rank
    c = _mk(kind, _delta(), **kw)
    monkeypatch.setattr(c, "_engine_for", boom)
    monkeypatch.setattr(c, "_batch_engine_for", boom)
    monkeypatch.setattr(distributed, "world", lambda group=None: (0, 2))
    before = c._seed_rng.get_state()
    with pytest.raises(NotImplementedError, match="noise_rho / keep_elites.*rank" if kind == "cem" else "one rank"):
        c.get_action(np.zeros(S))
    with pytest.raises(NotImplementedError, match="one rank"):
        c.get_actions(np.zeros((2, S)))
    assert same(before, c._seed_rng.get_state())

"""MPPI's control-cost term and weighted sigma update, the host side, no GPU: the definition
(bc_mpc_amd/mppi_update.py), the controller's arguments and refusals, the bindings of the new symbols, and that the
defaults keep calling the symbols they have always called.  The kernels are pinned in tests/test_gpu_mppi_ext.py."""
import ctypes
import math

import numpy as np
import pytest

S, A, H, K = 20, 6, 4, 16
NEW = {"bcmpc_mppi_get_action_x": 10, "bcmpc_mppi_get_actions_batch_x": 13, "bcmpc_mppi_control_cost_async": 10,
       "bcmpc_mppi_sigma_update_async": 12}


# ------------------------------------------------------------------ the definition
def test_control_cost_hand_worked_case():
    from bc_mpc_amd.mppi_update import control_cost, control_gain
    # 2 steps, 2 action dimensions, 2 candidates; every number a dyadic rational, so the arithmetic is exact
    mu = np.array([[0.5, -1.0], [0.25, 2.0]])
    sigma = np.array([[0.5, 2.0], [0.25, 1.0]])
    g = control_gain(mu, sigma)
    assert np.array_equal(g, [[2.0, -0.25], [4.0, 2.0]])
    acts = np.empty((2, 2, 2))
    acts[:, 0, :] = mu + np.array([[0.5, 4.0], [-0.25, 0.5]])        # candidate 0: mu + eps
    acts[:, 1, :] = mu                                               # candidate 1: eps = 0
    # q0 = 2 * 0.5 + (-0.25) * 4 + 4 * (-0.25) + 2 * 0.5 = 1 - 1 - 1 + 1 = 0; the chain: 1, 0, -1, 0
    assert np.array_equal(control_cost(acts, mu, sigma), [0.0, 0.0])
    acts[1, 0, 1] = mu[1, 1] + 1.5                                   # the last term becomes 2 * 1.5 = 3
    assert np.array_equal(control_cost(acts, mu, sigma), [2.0, 0.0])
    with pytest.raises(ValueError, match="shapes"):
        control_cost(acts, mu[:1], sigma)


def test_control_cost_is_the_scalar_chain_in_h_then_j_order():
    from bc_mpc_amd.mppi_update import control_cost
    rs = np.random.RandomState(0)
    Hh, Kk, Aa = 5, 9, 3
    mu, sd = rs.uniform(-0.6, 0.6, (Hh, Aa)), rs.uniform(0.1, 0.9, (Hh, Aa))
    acts = np.clip(mu[:, None, :] + sd[:, None, :] * rs.standard_normal((Hh, Kk, Aa)), -1.0, 1.0)
    q = control_cost(acts, mu, sd)
    for k in range(Kk):
        t = 0.0
        for h in range(Hh):
            for j in range(Aa):
                g = float(mu[h, j]) / (float(sd[h, j]) * float(sd[h, j]))
                t = t + g * (float(acts[h, k, j]) - float(mu[h, j]))
        assert np.float64(t).tobytes() == q[k].tobytes(), k


def test_zero_sigma_entries_are_skipped():
    from bc_mpc_amd.mppi_update import control_cost, control_gain
    mu = np.array([[0.5, 0.75]])
    sigma = np.array([[0.0, 0.5]])
    with np.errstate(all="raise"):                                   # (no division by zero is even attempted)
        g = control_gain(mu, sigma)
    assert np.array_equal(g, [[0.0, 3.0]])
    acts = np.array([[[0.9, 1.0], [0.5, 0.25]]])                     # [1, 2, 2]; column 0 does not count
    assert np.array_equal(control_cost(acts, mu, sigma), [0.75, -1.5])


def test_augmented_flips_its_sign_on_maximize_and_keeps_nan_and_inf():
    from bc_mpc_amd.mppi_update import augmented
    costs = np.array([1.0, -2.0, np.nan, np.inf, -np.inf, 4.0])
    q = np.array([0.5, 2.0, 1.0, -3.0, 7.0, -1.0])
    plus, minus = augmented(costs, q, 2.0), augmented(costs, q, 2.0, maximize=True)
    assert np.array_equal(plus[[0, 1, 5]], [2.0, 2.0, 2.0]) and np.array_equal(minus[[0, 1, 5]], [0.0, -6.0, 6.0])
    for got in (plus, minus):
        assert np.isnan(got[2]) and got[3] == np.inf and got[4] == -np.inf
    assert np.array_equal(augmented(costs, q, 0.0)[[0, 1, 5]], costs[[0, 1, 5]])
    # on a reward engine the score v = -c~ rises with q, as on a cost engine
    assert np.array_equal(-minus[[0, 1, 5]], (-costs + 2.0 * q)[[0, 1, 5]])


@pytest.mark.parametrize("Kk", [1, 5, 64, 65, 1000])
def test_weighted_sigma_one_weight_and_equal_weights(Kk):
    from bc_mpc_amd.mppi_update import weighted_sigma
    rs = np.random.RandomState(Kk)
    acts = rs.uniform(-1.0, 1.0, (3, Kk, 2))
    w = np.zeros(Kk)
    i = int(rs.randint(Kk))
    w[i] = 0.37
    s = weighted_sigma(w, acts, acts[:, i, :])                       # all weight on candidate i: mu' is its actions
    assert s.tobytes() == np.zeros((3, 2)).tobytes()
    s = weighted_sigma(np.ones(Kk), acts, acts.mean(axis=1))
    assert np.max(np.abs(s - acts.std(axis=1))) <= 1e-15
    with pytest.raises(ValueError, match="shapes"):
        weighted_sigma(np.ones(Kk + 1), acts, acts.mean(axis=1))


@pytest.mark.parametrize("Kk", [1, 63, 64, 65, 4097, 16384, 16385])
def test_two_stage_sum_is_a_sum(Kk):
    from bc_mpc_amd.mppi_update import cpl, two_stage_sum
    assert cpl(Kk) == (4 if Kk > 16384 else 1)
    x = np.random.RandomState(Kk).uniform(0.0, 1.0, (Kk, 2))
    got = two_stage_sum(x)
    want = np.array([math.fsum(x[:, 0]), math.fsum(x[:, 1])])
    assert got.shape == (2,) and np.max(np.abs(got - want)) <= Kk * 2.0 ** -53 * want.max()
    assert two_stage_sum(np.arange(float(Kk))) == Kk * (Kk - 1) / 2      # (integers: exact in any order)


def test_sigma_step_alpha_one_and_a_high_floor():
    from bc_mpc_amd.mppi_update import sigma_step
    rs = np.random.RandomState(1)
    old, s = rs.uniform(0.01, 2.0, (3, 4)), rs.uniform(0.0, 2.0, (3, 4))
    assert sigma_step(old, s, 1.0).tobytes() == old.tobytes()
    assert sigma_step(old, s, 0.0).tobytes() == s.tobytes()
    assert np.array_equal(sigma_step(old, s, 0.3, min_std=5.0), np.full((3, 4), 5.0))
    assert np.array_equal(sigma_step(old, s, 0.3, 0.0, 1e-3), np.full((3, 4), 1e-3))
    mid = sigma_step(old, s, 0.25)
    assert mid.tobytes() == (0.25 * old + 0.75 * s).tobytes()
    assert np.array_equal(sigma_step(old, s, 0.25, 0.5, 1.0), np.clip(mid, 0.5, 1.0))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_equal_costs_pull_the_plan_towards_zero(seed):
    """All raw costs equal: the weights are exp(-weight (q - q_min) / lambda), decreasing in q, so the weighted mean
    of q is at most its plain mean (Chebyshev's sum inequality).  The weighted mean of q is sum_hj g (mu' - mu) --
    q is linear in the actions -- hence sum g (mu' - mu) <= mean(q) up to 1e-12: the pull towards small plans."""
    from bc_mpc_amd.mppi_update import augmented, control_cost, control_gain, softmin_weights
    rs = np.random.RandomState(seed)
    Hh, Kk, Aa, lam, weight = 4, 300, 3, 0.7, 0.7
    mu, sd = rs.uniform(-0.6, 0.6, (Hh, Aa)), rs.uniform(0.2, 0.6, (Hh, Aa))
    acts = np.clip(mu[:, None, :] + sd[:, None, :] * rs.standard_normal((Hh, Kk, Aa)), -1.0, 1.0)
    q = control_cost(acts, mu, sd)
    for maximize in (False, True):
        w = softmin_weights(augmented(np.full(Kk, 3.25), q, weight, maximize), lam, maximize)
        assert w.max() == 1.0 and (w > 0).all() and w.min() < 1.0
        mu_new = np.einsum("k,hka->ha", w, acts) / w.sum()
        pull = float(np.sum(control_gain(mu, sd) * (mu_new - mu)))
        print(f"seed {seed} maximize {maximize}: sum g (mu' - mu) = {pull:.6f}, mean(q) = {q.mean():.6f}")
        assert abs(pull - float(np.sum(w * q) / w.sum())) <= 1e-12
        assert pull <= q.mean() + 1e-12
        assert pull < q.mean() - 1e-3                    # (and here strictly: the weights are not all equal)


# ------------------------------------------------------------------ option checks
def test_check_options_values_and_refusals():
    from bc_mpc_amd.mppi_update import check_options
    assert check_options() == (0.0, False, 0.0, 0.0, math.inf)
    assert check_options(True, True, 0.5, 0.1, 2.0, temperature=3.0) == (3.0, True, 0.5, 0.1, 2.0)
    assert check_options(False, temperature=3.0)[0] == 0.0
    assert check_options(1.5, 1, 1.0, 0.0, 0.0) == (1.5, True, 1.0, 0.0, 0.0)
    for bad in (-0.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="control_cost"):
            check_options(bad)
    with pytest.raises(ValueError, match="temperature"):
        check_options(True)
    for bad in (2, "yes", None, 0.5):
        with pytest.raises(ValueError, match="adapt_sigma"):
            check_options(0.0, bad)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="sigma_alpha"):
            check_options(0.0, True, bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_std"):
            check_options(0.0, True, 0.0, bad)
    for lo, hi in ((0.5, 0.25), (0.0, -1.0), (0.1, float("nan"))):
        with pytest.raises(ValueError, match="max_std"):
            check_options(0.0, True, 0.0, lo, hi)


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
    assert ctypes.sizeof(_lib.MppiExt) == 40
    assert [f[0] for f in _lib.MppiExt._fields_] == ["control_weight", "adapt_sigma", "reserved", "sigma_alpha",
                                                     "min_std", "max_std"]


def test_bad_arguments_are_answered_without_hip():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    P = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    st, mu, sd = np.zeros((1, S)), np.zeros((1, H, A)), np.ones((1, H, A))
    out, stats = (_lib.Result * 1)(), (_lib.MppiStats * 1)()
    mppi = _lib.Mppi(1, 1.0, 0)

    def single(ext):
        return lib.bcmpc_mppi_get_action_x(None, P(st), ctypes.byref(mppi), None, ctypes.byref(ext), 0, P(mu), P(sd),
                                           out, stats)

    def batch(ext):
        return lib.bcmpc_mppi_get_actions_batch_x(None, P(st), 1, ctypes.byref(mppi), None, ctypes.byref(ext), 0, 0,
                                                  P(mu), P(sd), out, stats, None)

    inf = math.inf
    for call in (single, batch):
        # a null engine: an argument error, with the options on and with them off (the forwarded call's)
        for ext in (_lib.MppiExt(1.0, 0, 0, 0.0, 0.0, inf), _lib.MppiExt(0.0, 1, 0, 0.0, 0.0, inf),
                    _lib.MppiExt(0.0, 0, 0, 0.0, 0.0, inf)):
            assert call(ext) == _lib.ERR_ARG and b"null" in lib.bcmpc_last_error()
        for ext, text in ((_lib.MppiExt(-1.0, 0, 0, 0.0, 0.0, inf), b"control_weight"),
                          (_lib.MppiExt(math.nan, 0, 0, 0.0, 0.0, inf), b"control_weight"),
                          (_lib.MppiExt(inf, 0, 0, 0.0, 0.0, inf), b"control_weight"),
                          (_lib.MppiExt(1.0, 2, 0, 0.0, 0.0, inf), b"adapt_sigma"),
                          (_lib.MppiExt(1.0, 1, 7, 0.0, 0.0, inf), b"reserved"),
                          (_lib.MppiExt(1.0, 1, 0, 1.5, 0.0, inf), b"sigma_alpha"),
                          (_lib.MppiExt(1.0, 1, 0, math.nan, 0.0, inf), b"sigma_alpha"),
                          (_lib.MppiExt(1.0, 1, 0, 0.0, -1.0, inf), b"min_std"),
                          (_lib.MppiExt(1.0, 1, 0, 0.0, 1.0, 0.5), b"max_std"),
                          (_lib.MppiExt(1.0, 1, 0, 0.0, 0.0, math.nan), b"max_std")):
            assert call(ext) == _lib.ERR_ARG and text in lib.bcmpc_last_error(), text
    assert lib.bcmpc_mppi_control_cost_async(None, None, None, 1, 4, None, None, 1.0, None, None) == _lib.ERR_ARG
    assert lib.bcmpc_mppi_control_cost_async(None, None, None, 0, 4, None, None, 1.0, None, None) == _lib.ERR_ARG
    assert b"n_envs" in lib.bcmpc_last_error()
    assert lib.bcmpc_mppi_sigma_update_async(None, None, None, 1, 4, 1.0, None, None, 0.0, 0.0, inf,
                                             None) == _lib.ERR_ARG


# ------------------------------------------------------------------ the engine methods at the defaults
class _Recorder:
    """A stand-in for the loaded library: records the symbol every call goes to and answers BCMPC_OK."""

    def __init__(self):
        self.names, self.args = [], []

    def __getattr__(self, name):
        def fn(*args):
            self.names.append(name)
            self.args.append(args)
            return 0
        return fn


def _bare_engine(K_total=K):
    from bc_mpc_amd.engine import RolloutEngine
    eng = RolloutEngine.__new__(RolloutEngine)
    eng._lib, eng._h = _Recorder(), None
    eng.state_dim, eng.action_dim, eng.horizon, eng.num_paths = S, A, H, K_total
    return eng


def test_default_options_call_the_symbols_they_always_called():
    eng = _bare_engine(2 * K)
    st, mu, sd = np.zeros(S), np.zeros((H, A)), np.ones((H, A))
    bst, bmu, bsd = np.zeros((2, S)), np.zeros((2, H, A)), np.ones((2, H, A))
    assert len(eng.mppi_get_action(st, mu, sd, 1, 1.0, 1)) == 3
    assert len(eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, control_cost=0.0, adapt_sigma=False, sigma_alpha=0.5,
                                   min_std=0.1, max_std=2.0)) == 3
    assert len(eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, rho=0.5, control_cost=False)) == 3
    assert len(eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1)) == 3
    assert len(eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, rho=0.5)) == 3
    assert eng._lib.names == ["bcmpc_mppi_get_action"] * 2 + ["bcmpc_mppi_get_action_s", "bcmpc_mppi_get_actions_batch",
                                                              "bcmpc_mppi_get_actions_batch_s"]
    eng._lib.names.clear()
    eng._lib.args.clear()
    assert len(eng.mppi_get_action(st, mu, sd, 1, 2.5, 1, control_cost=True)) == 3
    out = eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, adapt_sigma=True, sigma_alpha=0.25, min_std=0.05)
    assert len(out) == 4 and out[3].shape == (H, A) and out[3] is not sd
    assert len(eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, control_cost=0.5, rho=0.9)) == 3
    out = eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, adapt_sigma=True, max_std=3.0)
    assert len(out) == 4 and out[3].shape == (2, H, A) and out[3] is not bsd
    assert eng._lib.names == ["bcmpc_mppi_get_action_x"] * 2 + ["bcmpc_mppi_get_actions_batch_x"] * 2
    exts = [a[4]._obj for a in eng._lib.args[:2]] + [a[5]._obj for a in eng._lib.args[2:]]
    got = [(e.control_weight, e.adapt_sigma, e.reserved, e.sigma_alpha, e.min_std, e.max_std) for e in exts]
    assert got == [(2.5, 0, 0, 0.0, 0.0, math.inf), (0.0, 1, 0, 0.25, 0.05, math.inf), (0.5, 0, 0, 0.0, 0.0, math.inf),
                   (0.0, 1, 0, 0.0, 0.0, 3.0)]
    assert eng._lib.args[0][3] is None and eng._lib.args[2][4]._obj.rho == 0.9     # the sampling travels along
    eng._lib.names.clear()
    for kw in (dict(control_cost=-1.0), dict(adapt_sigma=True, sigma_alpha=2.0), dict(adapt_sigma=True, min_std=1.0,
                                                                                     max_std=0.5)):
        with pytest.raises(ValueError):
            eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, **kw)
        with pytest.raises(ValueError):
            eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, **kw)
    assert eng._lib.names == []
    # the async wrappers go to their symbols; max_std None travels as +inf
    eng.mppi_control_cost_async(8, 16, 1, K, 24, 32, 0.5, 40, stream=0)
    eng.mppi_sigma_update_async(8, 16, 1, K, 1.0, 24, 32, stream=0)
    assert eng._lib.names == ["bcmpc_mppi_control_cost_async", "bcmpc_mppi_sigma_update_async"]
    assert eng._lib.args[-1][8:11] == (0.0, 0.0, math.inf)


def test_ensemble_engine_has_no_x_entry():
    from bc_mpc_amd.ensemble import EnsembleEngine
    eng = EnsembleEngine.__new__(EnsembleEngine)
    eng._lib, eng._h = _Recorder(), None
    eng.state_dim, eng.action_dim, eng.horizon, eng.num_paths = S, A, H, K
    st, mu, sd = np.zeros(S), np.zeros((H, A)), np.ones((H, A))
    eng.mppi_get_action(st, mu, sd, 1, 1.0, 1)
    with pytest.raises(NotImplementedError, match="control cost.*ensembles"):
        eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, control_cost=1.0)
    with pytest.raises(NotImplementedError, match="ensembles"):
        eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, adapt_sigma=True)
    assert eng._lib.names == ["bcmpc_ensemble_mppi_get_action"]


# ------------------------------------------------------------------ the controller
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


def _mk(model=None, **kw):
    from bc_mpc_amd import MPPIcontroller, cheetah_cost_fn
    return MPPIcontroller(_Env(), model if model is not None else object(), horizon=H, cost_fn=cheetah_cost_fn,
                          num_simulated_paths=K, seed=5, **kw)


def test_controller_argument_checks():
    c = _mk()
    assert (c.control_cost, c.adapt_sigma, c.sigma_alpha, c.min_std, c.max_std) == (0.0, False, 0.0, 0.0, None)
    assert c._update_args() == {} and c.last_sigma is None
    with pytest.raises(ValueError, match="control_cost"):
        _mk(control_cost=-0.5)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="sigma_alpha"):
            _mk(adapt_sigma=True, sigma_alpha=bad)
    with pytest.raises(ValueError, match="max_std"):
        _mk(adapt_sigma=True, min_std=0.5, max_std=0.25)
    with pytest.raises(ValueError, match="min_std"):
        _mk(min_std=-1.0)
    assert _mk(control_cost=True, temperature=2.5)._update_args() == {"control_cost": 2.5}
    assert _mk(control_cost=0.125)._update_args() == {"control_cost": 0.125}
    assert _mk(adapt_sigma=True, sigma_alpha=0.1, min_std=0.05, max_std=1.0)._update_args() == dict(
        adapt_sigma=True, sigma_alpha=0.1, min_std=0.05, max_std=1.0)
    assert _mk(adapt_sigma=True)._update_args() == dict(adapt_sigma=True, sigma_alpha=0.0, min_std=0.0, max_std=math.inf)
    # the sigma step's parameters alone switch nothing on
    assert _mk(sigma_alpha=0.5, min_std=0.1, max_std=2.0)._update_args() == {}
    # read on every call: a value set later is checked when it is used
    c.control_cost = -1.0
    with pytest.raises(ValueError, match="control_cost"):
        c._update_args()


class _StubEngine:
    """An engine double of the signature BEFORE the options existed, plus **kw to see what arrives."""

    def __init__(self):
        self.calls = []

    def set_weights(self, *a):
        pass

    def mppi_get_action(self, state, mu, sigma, iterations, temperature, seed, **kw):
        from bc_mpc_amd import _lib
        from bc_mpc_amd.engine import StepResult
        self.calls.append(("mppi", seed, kw))
        out = (StepResult(0, 1.0, np.zeros(A), None), mu, _lib.MppiStats(1.0, 1.0, 0.0, 1))
        return out + (0.5 * sigma,) if kw.get("adapt_sigma") else out

    def mppi_get_actions(self, states, mu, sigma, iterations, temperature, seed, **kw):
        from bc_mpc_amd.engine import MPPI_STATS, BatchResult
        self.calls.append(("mppis", seed, kw))
        B = states.shape[0]
        out = (BatchResult(np.zeros(B, np.int64), np.zeros(B), np.zeros((B, A))), mu, np.zeros(B, dtype=MPPI_STATS))
        return out + (0.5 * sigma,) if kw.get("adapt_sigma") else out


def test_keywords_reach_the_engine_only_when_non_default_and_last_sigma_is_published(monkeypatch):
    c = _mk(_delta(), control_cost=True, temperature=2.0, adapt_sigma=True, sigma_alpha=0.25, min_std=0.01,
            noise_rho=0.5)
    eng = _StubEngine()
    monkeypatch.setattr(c, "_engine_for", lambda *a: eng)
    monkeypatch.setattr(c, "_batch_engine_for", lambda *a: eng)
    seeds = [int(x) for x in np.random.RandomState(5).randint(0, 2**62, size=4, dtype=np.int64)]
    want = dict(rho=0.5, control_cost=2.0, adapt_sigma=True, sigma_alpha=0.25, min_std=0.01, max_std=math.inf)
    c.get_action(np.zeros(S))
    sd0 = np.full((H, A), 0.5)                                       # init_std None: (high - low) / 4
    assert c.last_sigma.shape == (H, A) and np.array_equal(c.last_sigma, 0.5 * sd0)
    c.get_actions(np.zeros((2, S)))
    assert c.last_sigma.shape == (2, H, A) and np.array_equal(c.last_sigma, 0.5 * np.tile(sd0, (2, 1, 1)))
    c.adapt_sigma, c.noise_rho = False, 0.0                          # read on every call; nothing is rebuilt
    c.get_action(np.zeros(S))
    assert np.array_equal(c.last_sigma, sd0)                         # not adapted: the sigma the call sampled with
    c.control_cost = 0.0
    c.get_action(np.zeros(S))
    assert eng.calls == [("mppi", seeds[0], want), ("mppis", seeds[1], want), ("mppi", seeds[2], dict(control_cost=2.0)),
                         ("mppi", seeds[3], {})]


@pytest.mark.parametrize("kw", [dict(control_cost=1.0), dict(adapt_sigma=True), dict(control_cost=True, adapt_sigma=True)])
def test_ensemble_and_rank_refusals_do_not_consume_a_seed(kw, monkeypatch):
    from bc_mpc_amd import distributed, ensemble

    def boom(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(ensemble, "_ctrl_engine", boom)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))   # noqa: E731
    # an EnsembleDynamicsModel
    c = _mk(_ensemble(), **kw)
    before = c._seed_rng.get_state()
    with pytest.raises(NotImplementedError, match="control_cost / adapt_sigma.*EnsembleDynamicsModel"):
        c.get_action(np.zeros(S))
    with pytest.raises(NotImplementedError, match="EnsembleDynamicsModel"):
        c.get_actions(np.zeros((2, S)))
    assert same(before, c._seed_rng.get_state()) and c._engine is None and c._batch_engine is None
    # more than one rank
    c = _mk(_delta(), **kw)
    monkeypatch.setattr(c, "_engine_for", boom)
    monkeypatch.setattr(c, "_batch_engine_for", boom)
    monkeypatch.setattr(distributed, "world", lambda group=None: (0, 2))
    before = c._seed_rng.get_state()
    with pytest.raises(NotImplementedError, match="one rank"):
        c.get_action(np.zeros(S))
    with pytest.raises(NotImplementedError, match="one rank"):
        c.get_actions(np.zeros((2, S)))
    assert same(before, c._seed_rng.get_state())

"""Terminal value, the parts that need no GPU: value.ValueSpec and value.terminal_values (the NumPy definition the
kernel is tested against, tests/test_gpu_terminal_value.py), the accuracy bars on the definition itself, the C
entry points' argument checks (made before any HIP call) and the controllers' refusals."""
import ctypes
import math
import types

import numpy as np
import pytest

import value_cases as vc


def _spec(S=5, hidden=4, L=2, **kw):
    s = vc.make_spec(S, hidden, L)
    d = dict(kernels=list(s.kernels), biases=list(s.biases), ob_mean=s.ob_mean, ob_std=s.ob_std)
    d.update(kw)
    return d


def test_symbols_exported_and_abi_still_5():
    import bc_mpc_amd
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_abi_version() == 5 == _lib.ABI_VERSION
    for name in ("bcmpc_set_terminal_value", "bcmpc_terminal_value_async", "bcmpc_terminal_value_supported",
                 "bcmpc_last_terminal_values"):
        assert hasattr(lib, name), name
    assert ctypes.sizeof(_lib.ValueNet) == 48
    assert hasattr(bc_mpc_amd, "value") and "ValueSpec" in bc_mpc_amd.__all__


def test_valuespec_validation():
    from bc_mpc_amd.value import ValueSpec
    ok = ValueSpec(**_spec())
    assert (ok.n_layers, ok.hidden, ok.state_dim) == (2, 4, 5)
    assert all(k.dtype == np.float32 for k in ok.kernels) and ok.ob_std.dtype == np.float32
    for L, h in ((1, 1), (4, 256), (1, 100)):
        s = ValueSpec(**_spec(20, h, L))
        assert (s.n_layers, s.hidden) == (L, h)
    base = _spec()
    k, b = base["kernels"], base["biases"]
    bad = [
        dict(kernels=k[:1], biases=b[:1]),                                      # L = 0
        dict(kernels=[k[0]] + [k[1]] * 4 + [k[2]], biases=[b[0]] + [b[1]] * 4 + [b[2]]),   # L = 5
        dict(kernels=k, biases=b[:2]),                                          # lengths differ
        dict(kernels=[k[0], k[1], np.zeros((4, 2), np.float32)]),               # last kernel not [hidden, 1]
        dict(kernels=[k[0], np.zeros((4, 5), np.float32), k[2]]),               # hidden layer not square
        dict(biases=[b[0], b[1], np.zeros(2, np.float32)]),                     # final bias not (1,)
        dict(ob_mean=np.zeros(4, np.float32)),                                  # wrong S
        dict(ob_std=np.array([1, 1, 0, 1, 1], np.float32)),                     # std == 0
        dict(ob_std=np.array([1, 1, -1, 1, 1], np.float32)),                    # std < 0
        dict(ob_std=np.array([1, 1, np.inf, 1, 1], np.float32)),                # std not finite
        dict(ob_std=np.array([1, 1, np.nan, 1, 1], np.float32)),
        dict(ob_mean=np.array([0, np.nan, 0, 0, 0], np.float32)),
        dict(kernels=[k[0], k[1] * np.float32(np.inf), k[2]]),                  # kernel not finite
        dict(biases=[b[0], b[1] + np.float32(np.nan), b[2]]),
        dict(kernels=[k[0].astype(np.float64) * 1e39, k[1], k[2]]),             # overflows f32
        dict(kernels=[k[0][:, :, None], k[1], k[2]]),                           # not a matrix
    ]
    for i, kw in enumerate(bad):
        with pytest.raises(ValueError):
            ValueSpec(**_spec(**kw))
            pytest.fail(f"rule {i} did not raise")
    with pytest.raises(ValueError):                                             # hidden = 257
        ValueSpec([np.zeros((3, 257), np.float32), np.zeros((257, 1), np.float32)],
                  [np.zeros(257, np.float32), np.zeros(1, np.float32)], np.zeros(3, np.float32), np.ones(3, np.float32))
    with pytest.raises(ValueError):                                             # S = 33
        ValueSpec([np.zeros((33, 4), np.float32), np.zeros((4, 1), np.float32)],
                  [np.zeros(4, np.float32), np.zeros(1, np.float32)], np.zeros(33, np.float32), np.ones(33, np.float32))


@pytest.mark.parametrize("S", vc.SS)
def test_identity_like_net_returns_obz_bit_for_bit(S):
    """obz on hand-made values: the definition's first two steps, read back through a net that is the identity
    on one dimension -- the same net pins the kernel's obz bits in the GPU test."""
    from bc_mpc_amd import value
    states = vc.identity_states(S)
    for d in sorted({0, S // 2, S - 1}):
        spec = vc.identity_like(S, d)
        with np.errstate(over="ignore"):
            x = states.astype(np.float32)
        want = np.minimum(np.maximum((x[:, d] - spec.ob_mean[d]) / spec.ob_std[d], np.float32(-5)), np.float32(5))
        got = value.terminal_values(spec, states)
        assert got.dtype == np.float32 and np.array_equal(got, want), d
        assert np.array_equal(value.observe(spec, states)[:, d], want)
        if d == 0:      # mean 0, std 1: the clip at exactly +-5, one ulp inside, far outside
            assert got[3] == 5 and got[4] == -5 and got[0] == 5 and got[1] == -5 and got[7] == 5
            assert got[5] == np.nextafter(np.float32(5), np.float32(0)) and got[6] == -got[5]


def test_nan_and_inf_state_dimensions():
    from bc_mpc_amd import value
    spec, cases = vc.case(17, 16, 2)
    c = cases[65]
    v = c.v_def
    assert np.isnan(v[1]) and np.isnan(v[9]) and np.isfinite(np.delete(v, [1, 9])).all()
    obz = c.obz
    assert obz[2, 0] == 5 and obz[3, 16] == -5 and obz[4, 16] == -5 and obz[5, 0] == 5 and obz[6, 0] == -5
    assert obz[7, 0] == 5 and obz[8, 0] == -5 and np.isnan(obz[1, 8]) and np.abs(obz[~np.isnan(obz)]).max() == 5
    # totals: one rounded multiply, one rounded add; a NaN value makes a NaN total, which wins np.argmin
    costs = np.linspace(-3, 3, 65)
    tot = value.add_to_costs(costs, v, -0.75)
    want = np.array([costs[i] + (-0.75) * float(v[i]) for i in range(65)])
    assert np.array_equal(tot, want, equal_nan=True) and int(np.argmin(tot)) == 1
    assert np.array_equal(value.add_to_costs(costs, np.where(np.isnan(v), 0, v).astype(np.float32), 0.0), costs)
    with pytest.raises(ValueError):
        value.terminal_values(spec, np.zeros((4, 16)))
    for w in (math.inf, math.nan):
        with pytest.raises(ValueError):
            value.check_weight(w)


@pytest.mark.parametrize("S,hidden,L", vc.CASES)
def test_the_definition_meets_both_accuracy_bars(S, hidden, L):
    """value.terminal_values (BLAS f32, np.tanh) against the f64 evaluation: within E_k per candidate, and its
    RMS error within 4x that of the strictly sequential f32 evaluation -- the bars the kernel has to meet, on
    every case of the GPU test."""
    spec, cases = vc.case(S, hidden, L)
    for K, c in cases.items():
        c.check(c.v_def, f"definition S={S} hidden={hidden} L={L} K={K}")
        assert (c.bound[c.finite] > 0).all()


def test_error_bound_is_the_documented_recurrence():
    """E_k restated with Python floats on a 2-input, 1-neuron, 1-layer net."""
    from bc_mpc_amd.value import ValueSpec, error_bound, observe
    u = 2.0 ** -24
    spec = ValueSpec([np.array([[0.5], [-2.0]], np.float32), np.array([[3.0]], np.float32)],
                     [np.array([0.25], np.float32), np.array([-1.0], np.float32)],
                     np.zeros(2, np.float32), np.ones(2, np.float32))
    obz = observe(spec, np.array([[1.5, 0.75]]))
    x0, x1 = float(obz[0, 0]), float(obz[0, 1])
    g3, g2 = 3 * u / (1 - 3 * u), 2 * u / (1 - 2 * u)
    e1 = g3 * (0.5 * abs(x0) + 2.0 * abs(x1) + 0.25)
    t = math.tanh(0.5 * x0 - 2.0 * x1 + 0.25)
    e1 = e1 + 8 * u * abs(t)
    e2 = 3.0 * e1 + g2 * (3.0 * abs(t) + 1.0)
    assert error_bound(spec, obz)[0] == pytest.approx(e2, rel=1e-12)


def _value_net(spec, **over):
    from bc_mpc_amd import _lib
    FP = ctypes.POINTER(ctypes.c_float)
    ks, bs = [np.array(k) for k in spec.kernels], [np.array(b) for b in spec.biases]
    mean, std = np.array(spec.ob_mean), np.array(spec.ob_std)
    keep = [ks, bs, mean, std]
    karr = (FP * len(ks))(*[k.ctypes.data_as(FP) for k in ks])
    barr = (FP * len(bs))(*[b.ctypes.data_as(FP) for b in bs])
    v = _lib.ValueNet(karr, barr, mean.ctypes.data_as(FP), std.ctypes.data_as(FP), spec.n_layers, spec.hidden,
                      spec.state_dim, 0)
    keep += [karr, barr]
    return v, keep


def test_c_argument_checks_run_before_any_hip_call():
    """The net is validated before the engine is looked at, so a NULL engine reaches every rule without a GPU:
    a bad net answers with its own message, a good one with the null-engine message."""
    from bc_mpc_amd import _lib
    lib = _lib.load()
    ARG = _lib.ERR_ARG
    spec = vc.make_spec(5, 4, 2)

    def call(v, weight=-1.0):
        rc = lib.bcmpc_set_terminal_value(None, ctypes.byref(v) if v is not None else None, weight, 1)
        return rc, lib.bcmpc_last_error().decode()
    v, keep = _value_net(spec)
    assert call(v) == (ARG, "null argument")                       # the net passed every check
    assert call(None) == (ARG, "null argument")
    for field in ("kernels", "biases", "ob_mean", "ob_std"):
        v, keep = _value_net(spec)
        setattr(v, field, type(getattr(v, field))())
        assert call(v) == (ARG, "value net: null argument"), field
    v, keep = _value_net(spec)
    v.kernels[1] = ctypes.POINTER(ctypes.c_float)()
    assert call(v) == (ARG, "value net: null argument")
    for L in (0, 5, -1):
        v, keep = _value_net(spec)
        v.n_layers = L
        rc, msg = call(v)
        assert rc == ARG and "n_layers must be in [1, 4]" in msg, L
    for h in (0, 257, -3):
        v, keep = _value_net(spec)
        v.hidden = h
        rc, msg = call(v)
        assert rc == ARG and "hidden must be in [1, 256]" in msg, h
    for S in (0, 33):
        v, keep = _value_net(spec)
        v.state_dim = S
        assert call(v)[0] == ARG and "state_dim" in call(v)[1]
    v, keep = _value_net(spec)
    v.reserved = 1
    assert "reserved" in call(v)[1]
    v, keep = _value_net(spec)
    for w in (math.inf, -math.inf, math.nan):
        rc, msg = call(v, w)
        assert rc == ARG and "weight must be finite" in msg
    for bad in (0.0, -1.0, math.inf, math.nan):
        v, keep = _value_net(spec)
        keep[3][2] = bad
        rc, msg = call(v)
        assert rc == ARG and "ob_std must be finite and > 0" in msg, bad
    v, keep = _value_net(spec)
    keep[2][0] = math.nan
    assert "ob_mean must be finite" in call(v)[1]
    v, keep = _value_net(spec)
    keep[0][1][3, 3] = math.inf
    assert "kernel entry is not finite" in call(v)[1]
    v, keep = _value_net(spec)
    keep[1][2][0] = math.nan
    assert "bias entry is not finite" in call(v)[1]
    # the kernel-alone entry and the diagnostics getter
    assert lib.bcmpc_terminal_value_async(None, None, 5, 1, None, None, None) == ARG
    assert lib.bcmpc_last_terminal_values(None, None, 1, None) == ARG
    assert lib.bcmpc_terminal_value_supported(None) == ARG


def test_engine_configs_that_take_no_terminal_value():
    """bcmpc_terminal_value_supported is the check bcmpc_set_terminal_value makes on its engine's config."""
    from bc_mpc_amd import _lib
    lib = _lib.load()

    def cfg(**kw):
        base = dict(state_dim=20, action_dim=6, hidden=64, n_layers=2, horizon=5, num_paths=16, cost=_lib.COST_CHEETAH)
        base.update(kw)
        return _lib.Config(**base)

    def ask(c):
        return lib.bcmpc_terminal_value_supported(ctypes.byref(c)), lib.bcmpc_last_error().decode()
    assert ask(cfg())[0] == _lib.OK and ask(cfg(cost=_lib.COST_TERMS))[0] == _lib.OK
    rc, msg = ask(cfg(policy_hidden=64, policy_layers=2))
    assert rc == _lib.ERR_UNSUPPORTED and "fused policy" in msg
    rc, msg = ask(cfg(cost=_lib.COST_REWARD, model=_lib.MODEL_REWARD))
    assert rc == _lib.ERR_UNSUPPORTED and "reward" in msg
    rc, msg = ask(cfg(model=_lib.MODEL_REWARD))
    assert rc == _lib.ERR_UNSUPPORTED and "reward" in msg
    rc, msg = ask(cfg(cost=_lib.COST_NONE))
    assert rc == _lib.ERR_UNSUPPORTED and "BCMPC_COST_NONE" in msg


class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32)


class _Env:
    def __init__(self, S, A):
        self.observation_space, self.action_space = _Space(S), _Space(A)


def _model(S, A):
    from oracle import mpc_oracle as orc
    return orc.NumpyDynamics(orc.synthetic_weights(S, A, 64, 2, "tanh", False), orc.synthetic_normalization(S, A))


def test_extract_containers_and_versions():
    from bc_mpc_amd import value
    spec = vc.make_spec(11, 8, 2)
    s1, v1 = value.extract(spec)
    assert s1 is spec and v1 == value.extract(spec)[1]
    holder = types.SimpleNamespace(value_spec=lambda: spec, version=41)
    assert value.extract(holder) == (spec, 41)
    standin = types.SimpleNamespace(vf=types.SimpleNamespace(kernels=spec.kernels, biases=spec.biases,
                                                             ob_mean=spec.ob_mean, ob_std=spec.ob_std))
    s2, v2 = value.extract(standin)
    assert v2 == v1 and all(np.array_equal(a, b) for a, b in zip(s2.kernels, spec.kernels))
    other = vc.make_spec(11, 8, 2, seed=1)
    assert value.extract(other)[1] != v1                                  # the digest follows the content
    standin.version = True                                                # a bool is no version stamp
    assert value.extract(standin)[1] == v1
    with pytest.raises(TypeError):
        value.extract(object())


def test_controller_refusals():
    """All before any engine exists."""
    from bc_mpc_amd import (CEMcontroller, MCTScontrollerPolicyNetReward, MPCcontroller, MPCcontrollerPolicyNet,
                            MPCcontrollerReward, MPPIcontroller)
    S, A = 11, 3
    env, dyn = _Env(S, A), _model(S, A)
    tv = vc.make_spec(S, 8, 2)
    fn = lambda s, a, ns: np.zeros(s.shape[0])   # noqa: E731
    state = np.zeros(S)
    # a cost the device cannot score
    c = MPCcontroller(env, dyn, horizon=3, cost_fn=fn, num_simulated_paths=8, terminal_value=tv)
    with pytest.raises(ValueError, match="terminal_value needs a cost the device scores"):
        c.get_action(state)
    assert c._engine is None
    for cls in (CEMcontroller, MPPIcontroller):
        c = cls(env, dyn, horizon=3, cost_fn=fn, num_simulated_paths=8, terminal_value=tv)
        with pytest.raises(ValueError, match="needs the fused cheetah cost_fn"):
            c.get_action(state)
    # weight and container are checked at construction
    for cls in (MPCcontroller, CEMcontroller, MPPIcontroller):
        with pytest.raises(ValueError, match="terminal_weight must be finite"):
            cls(env, dyn, horizon=3, num_simulated_paths=8, terminal_value=tv, terminal_weight=math.inf)
        with pytest.raises(TypeError, match="cannot read a value net"):
            cls(env, dyn, horizon=3, num_simulated_paths=8, terminal_value=object())
        with pytest.raises(TypeError):                                          # keyword-only
            cls(env, dyn, 3, None, 8, 1.0, tv)
        c = cls(env, dyn, horizon=3, num_simulated_paths=8)
        assert c.terminal_value is None and c.terminal_weight == -1.0 and c.last_terminal_value is None
    # the policy / reward / MCTS controllers do not take one
    with pytest.raises(ValueError, match="does not take a terminal_value"):
        MPCcontrollerPolicyNet(env, dyn, object(), terminal_value=tv)
    with pytest.raises(ValueError, match="does not take a terminal_value"):
        MPCcontrollerReward(env, dyn, terminal_value=tv)
    with pytest.raises(ValueError, match="does not take a terminal_value"):
        MCTScontrollerPolicyNetReward(env, dyn, object(), terminal_value=tv)


def test_the_value_is_applied_after_the_engine_lookup_and_is_no_cache_key():
    """The controllers hand (spec, weight, version) to the engine of every call; the engine constructor's
    arguments -- the cache key -- never see them."""
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller
    from bc_mpc_amd import controllers as ctl
    from bc_mpc_amd.cost_functions import TermCost, linear
    S, A = 11, 3
    env, dyn = _Env(S, A), _model(S, A)
    T = TermCost([linear(0, 1.0)])
    tv = types.SimpleNamespace(value_spec=lambda: vc.make_spec(S, 8, 2), version=3)

    class Stop(Exception):
        pass

    class FakeEngine:
        made = []

        def __init__(self, *a, **kw):
            FakeEngine.made.append((a, kw))
            self.calls = []
            self.comm = None
            self.state_dim = a[0]

        def set_action_bounds(self, lo, hi):
            pass

        def set_cost_terms(self, t):
            pass

        def set_weights(self, *a):
            raise Stop()

        terminal_value = None

        def set_terminal_value(self, spec, weight=-1.0, version=0):
            self.calls.append((spec, weight, version))
            self.terminal_value = None if spec is None else (spec, weight, version)

        def close(self):
            pass
    orig = ctl.RolloutEngine
    ctl.RolloutEngine = FakeEngine
    try:
        for cls in (MPCcontroller, CEMcontroller, MPPIcontroller):
            FakeEngine.made.clear()
            kw = dict(rng="device", seed=1) if cls is MPCcontroller else {}
            c = cls(env, dyn, horizon=3, cost_fn=T, num_simulated_paths=8, terminal_value=tv, terminal_weight=-0.5, **kw)
            with pytest.raises(Stop):
                c.get_action(np.zeros(S))
            c.terminal_weight = -0.25
            tv.version = 4
            with pytest.raises(Stop):
                c.get_action(np.zeros(S))
            c.terminal_value = None
            with pytest.raises(Stop):
                c.get_action(np.zeros(S))
            assert len(FakeEngine.made) == 1, cls.__name__                      # one engine for all three calls
            args, kwargs = FakeEngine.made[0]
            assert not any(isinstance(x, float) and x in (-0.5, -0.25) for x in args) and "terminal" not in repr(kwargs)
            eng = c._engine
            assert [(w, v) for _, w, v in eng.calls[:2]] == [(-0.5, 3), (-0.25, 4)] and eng.calls[2][0] is None
            tv.version = 3
    finally:
        ctl.RolloutEngine = orig

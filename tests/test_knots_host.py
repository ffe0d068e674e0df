"""Knot plans without a GPU: the definition (bc_mpc_amd/knots.py), the C entry points' argument refusals and the
controllers' refusals."""
import ctypes

import numpy as np
import pytest

from test_controller_refusals_host import A, H, K, S, STATE, STATES, _delta, _ensemble, _Env, _same, _seed_state, no_engines  # noqa: F401

KINDS = ("hold", "linear", "cubic")
SHAPES = [(Hh, M) for Hh in (1, 2, 5, 7, 20) for M in range(1, Hh + 1)]


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("kind", KINDS)
def test_expand_identities(kind):
    from bc_mpc_amd import knots as kn
    for Hh, M in SHAPES:
        theta = np.random.RandomState(100 * Hh + M).uniform(-1.0, 1.0, (M, 4, 3))
        out = kn.expand(theta, Hh, kind, -np.ones(3), np.ones(3))
        assert out.shape == (Hh, 4, 3)
        if M == Hh:
            assert out.tobytes() == theta.tobytes(), (Hh, M)
        if M == 1:
            assert out.tobytes() == np.repeat(theta, Hh, axis=0).tobytes(), (Hh, M)
        if kind == "hold":
            for h in range(Hh):
                assert out[h].tobytes() == theta[(h * M) // Hh].tobytes()
            spans = np.bincount([(h * M) // Hh for h in range(Hh)], minlength=M)
            assert spans.min() >= 1 and spans.max() - spans.min() <= 1
        elif M > 1:
            for m in range(M):                          # a knot that falls on a step is returned bit for bit
                h, r = divmod(m * (Hh - 1), M - 1)
                if r == 0:
                    assert out[h].tobytes() == theta[m].tobytes(), (Hh, M, m)
            assert out[0].tobytes() == theta[0].tobytes() and out[-1].tobytes() == theta[-1].tobytes()
        assert (np.abs(out) <= 1.0).all()


def test_expand_by_hand_at_7_3():
    from bc_mpc_amd import knots as kn
    th = np.array([[0.25], [-0.5], [0.75]])
    hold = kn.expand(th, 7, "hold")
    assert hold[:, 0].tolist() == [0.25, 0.25, 0.25, -0.5, -0.5, 0.75, 0.75]      # spans 3, 2, 2
    lin = kn.expand(th, 7, "linear")
    f = [float(r) / 6.0 for r in range(6)]                  # h * 2 = m0 * 6 + r: fractions in sixths
    want = [0.25, 0.25 + f[2] * (-0.5 - 0.25), 0.25 + f[4] * (-0.5 - 0.25), -0.5, -0.5 + f[2] * (0.75 + 0.5),
            -0.5 + f[4] * (0.75 + 0.5), 0.75]
    assert lin[:, 0].tolist() == want
    # Catmull-Rom at h = 1: m0 = 0, f = 2/6, p0 = p1 = th[0], p2 = th[1], p3 = th[2]
    p0 = p1 = 0.25
    p2, p3 = -0.5, 0.75
    a = p2 - p0
    b = ((2.0 * p0 - 5.0 * p1) + 4.0 * p2) - p3
    c = (3.0 * (p1 - p2) + p3) - p0
    assert kn.expand(th, 7, "cubic")[1, 0] == p1 + 0.5 * (f[2] * (a + f[2] * (b + f[2] * c)))


def test_cubic_clip_is_exercised():
    from bc_mpc_amd import knots as kn
    theta = np.random.RandomState(5).uniform(-1.0, 1.0, (5, 400, 6))
    theta[:, :40] = np.sign(theta[:, :40])                  # knots on the bounds: the spline overshoots between them
    raw = kn.expand(theta, 20, "cubic")
    out = kn.expand(theta, 20, "cubic", -np.ones(6), np.ones(6))
    assert (np.abs(raw) > 1.0).any() and (np.abs(out) <= 1.0).all()
    assert (out == 1.0).any() and (out == -1.0).any() and (np.abs(out) < 1.0).any()
    inside = np.abs(raw) <= 1.0
    assert out[inside].tobytes() == raw[inside].tobytes()
    lin = kn.expand(theta, 20, "linear")
    assert (np.abs(lin) <= 1.0).all()


def test_knot_values_is_correlated_actions_over_the_knot_axis():
    from bc_mpc_amd import knots as kn
    from bc_mpc_amd.sampling import correlated_actions
    rs = np.random.RandomState(2)
    z, mu, sd = rs.standard_normal((3, 9, 2)), rs.uniform(-0.5, 0.5, (3, 2)), rs.uniform(0.1, 2.0, (3, 2))
    got = kn.knot_values(z, 0.5, mu, sd, -np.ones(2), np.ones(2))
    assert got.tobytes() == correlated_actions(z, 0.5, mu, sd, -np.ones(2), np.ones(2)).tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_shift_plan(kind):
    from bc_mpc_amd import knots as kn
    fill = np.array([0.125, -0.25])
    for Hh, M in SHAPES:
        mu = np.random.RandomState(7 * Hh + M).uniform(-1.0, 1.0, (M, 2))
        got = kn.shift_plan(mu, Hh, kind, fill)
        assert got.shape == (M, 2)
        if M == Hh:                                         # today's shift
            assert got.tobytes() == np.vstack([mu[1:], fill[None]]).tobytes(), (Hh, M)
        if Hh == 1:
            assert got.tobytes() == fill[None].tobytes()
    mu = np.array([[0.25, 1.0], [-0.5, 0.0], [0.75, -1.0]])
    got = kn.shift_plan(mu, 7, kind, fill)
    if kind == "hold":
        # knots start at steps 0, 3, 5; one step later the old plan holds knots 0, 1, 2: nothing has ended
        assert got.tobytes() == mu.tobytes()
    elif kind == "linear":
        f = 2.0 / 6.0                                       # knots at steps 0, 3, 6; steps 1 and 4 are a third along
        want = np.stack([mu[0] + f * (mu[1] - mu[0]), mu[1] + f * (mu[2] - mu[1]), fill])
        assert got.tobytes() == want.tobytes()
    else:
        assert got[2].tobytes() == fill.tobytes()
        assert got[:2].tobytes() == kn.expand(mu, 7, "cubic")[[1, 4]].tobytes()
    # the shifted plan is the old plan's interpolant one step later, wherever the old plan still runs
    if kind != "hold":
        mu = np.random.RandomState(1).uniform(-1.0, 1.0, (4, 2))
        view = kn.expand(mu, 10, kind)
        got = kn.shift_plan(mu, 10, kind, fill)
        assert got[:3].tobytes() == view[[1, 4, 7]].tobytes() and got[3].tobytes() == fill.tobytes()


def test_checks():
    from bc_mpc_amd import knots as kn
    assert kn.check_knots(None, 5) is None and kn.check_knots(1, 5) == 1 and kn.check_knots(np.int64(5), 5) == 5
    for bad in (0, 6, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="knots"):
            kn.check_knots(bad, 5)
    assert [kn.check_interp(k) for k in KINDS] == list(KINDS)
    for bad in ("spline", None, 1):
        with pytest.raises(ValueError, match="knot_interp"):
            kn.check_interp(bad)
    with pytest.raises(ValueError):
        kn.expand(np.zeros((4, 2)), 3, "linear")


# ------------------------------------------------------------------ the C entry points, no device
def test_symbols_and_struct():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert ctypes.sizeof(_lib.Knots) == 8
    for name in ("bcmpc_cem_get_action_k", "bcmpc_mppi_get_action_k", "bcmpc_cem_get_actions_batch_k",
                 "bcmpc_mppi_get_actions_batch_k", "bcmpc_plan_sample_knots_async", "bcmpc_cem_refit_batch_steps_async",
                 "bcmpc_mppi_update_batch_steps_async", "bcmpc_plan_keep_steps_async",
                 "bcmpc_mppi_control_cost_steps_async", "bcmpc_mppi_sigma_update_steps_async"):
        assert hasattr(lib, name), name


def test_entry_points_refuse_bad_arguments_without_a_device():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    st, mu, sd = np.zeros(S), np.zeros((1, 3, A)), np.ones((1, 3, A))
    out, stats = (_lib.Result * 1)(), (_lib.MppiStats * 1)()
    cem, mp, kn = _lib.Cem(2, 4, 0.1, 0), _lib.Mppi(1, 1.0, 0), _lib.Knots(3, 1)
    # no engine: refused before any HIP call, knots on or off
    for k in (ctypes.byref(kn), None):
        assert lib.bcmpc_cem_get_action_k(None, dp(st), ctypes.byref(cem), None, None, k, 1, dp(mu), dp(sd), out) == _lib.ERR_ARG
        assert lib.bcmpc_mppi_get_action_k(None, dp(st), ctypes.byref(mp), None, None, None, k, 1, dp(mu), dp(sd), out,
                                           stats) == _lib.ERR_ARG
        assert lib.bcmpc_cem_get_actions_batch_k(None, dp(st), 1, ctypes.byref(cem), None, None, k, 1, 0, dp(mu), dp(sd),
                                                 out, None) == _lib.ERR_ARG
        assert lib.bcmpc_mppi_get_actions_batch_k(None, dp(st), 1, ctypes.byref(mp), None, None, None, k, 1, 0, dp(mu),
                                                  dp(sd), out, stats, None) == _lib.ERR_ARG
    assert lib.bcmpc_cem_get_actions_batch_k(None, dp(st), 0, ctypes.byref(cem), None, None, ctypes.byref(kn), 1, 0,
                                             dp(mu), dp(sd), out, None) == _lib.ERR_ARG
    assert b"n_envs" in lib.bcmpc_last_error()
    bad_ext = _lib.MppiExt(-1.0, 0, 0, 0.0, 0.0, 1.0)
    assert lib.bcmpc_mppi_get_action_k(None, dp(st), ctypes.byref(mp), None, ctypes.byref(bad_ext), None, ctypes.byref(kn),
                                       1, dp(mu), dp(sd), out, stats) == _lib.ERR_ARG
    assert b"control_weight" in lib.bcmpc_last_error()
    assert lib.bcmpc_plan_sample_knots_async(None, None, None, 1, 8, 1, 0, 0, 0.0, None, None, 0, 3, 1, None, None,
                                             None) == _lib.ERR_ARG
    assert lib.bcmpc_plan_sample_knots_async(None, None, None, 0, 8, 1, 0, 0, 0.0, None, None, 0, 3, 1, None, None,
                                             None) == _lib.ERR_ARG
    assert lib.bcmpc_cem_refit_batch_steps_async(None, None, None, 1, 4, 1, 0, 0.1, None, None, None, 8, 0, 3,
                                                 None) == _lib.ERR_ARG
    assert lib.bcmpc_mppi_update_batch_steps_async(None, None, 1, 8, 0, 1, 0, 1.0, None, None, None, None, 3,
                                                   None) == _lib.ERR_ARG
    assert lib.bcmpc_plan_keep_steps_async(None, None, None, None, 1, 8, 0, 4, None, None, 3, None) == _lib.ERR_ARG
    assert lib.bcmpc_mppi_control_cost_steps_async(None, None, None, 1, 8, None, None, 1.0, None, 3, None) == _lib.ERR_ARG
    assert lib.bcmpc_mppi_sigma_update_steps_async(None, None, None, 1, 8, 1.0, None, None, 0.0, 0.0, 1.0, 3,
                                                   None) == _lib.ERR_ARG


# ------------------------------------------------------------------ the controllers
@pytest.mark.parametrize("cls", ["CEMcontroller", "MPPIcontroller"])
def test_constructor_checks(cls):
    import bc_mpc_amd
    make = lambda **kw: getattr(bc_mpc_amd, cls)(_Env(), _delta(), H, bc_mpc_amd.cheetah_cost_fn, K, **kw)   # noqa: E731
    for bad in (0, H + 1, -2, 1.5):
        with pytest.raises(ValueError, match="knots"):
            make(knots=bad)
    with pytest.raises(ValueError, match="knot_interp"):
        make(knots=2, knot_interp="spline")
    c = make(knots=2, knot_interp="cubic")
    assert (c.knots, c.knot_interp) == (2, "cubic") and c.last_plan is None
    mu, sd = c.initial_distribution()
    assert mu.shape == sd.shape == (2, A)
    mu, sd = c.batch_initial_distribution(3)
    assert mu.shape == sd.shape == (3, 2, A)
    c = make()
    assert c.knots is None and c.initial_distribution()[0].shape == (H, A) and "last_plan" not in vars(c)


def _refused(ctrl, call, arg, exc, match):
    np.random.seed(77)
    before = _seed_state(ctrl), np.random.get_state()
    for _ in range(2):
        with pytest.raises(exc, match=match) as info:
            getattr(ctrl, call)(*arg)
        assert type(info.value) is exc
    assert ctrl._engine is None and getattr(ctrl, "_batch_engine", None) is None
    assert not ctrl.__dict__.get("_ens_engines")
    assert _same(before[0], _seed_state(ctrl)) and _same(before[1], np.random.get_state())


@pytest.mark.parametrize("cls,kind", [("CEMcontroller", "CEM"), ("MPPIcontroller", "MPPI")])
def test_controller_refusals(no_engines, monkeypatch, cls, kind):     # noqa: F811
    import bc_mpc_amd
    from bc_mpc_amd import distributed
    cheetah = bc_mpc_amd.cheetah_cost_fn
    make = lambda model=None, **kw: getattr(bc_mpc_amd, cls)(_Env(), model or _delta(), H, cheetah, K, **kw)   # noqa: E731
    # knots changed after construction are read, and checked, at the call
    for attr, bad, match in (("knots", H + 1, "knots must be in"), ("knots", 0, "knots must be in"),
                             ("knot_interp", "spline", "knot_interp")):
        c = make(knots=2)
        setattr(c, attr, bad)
        _refused(c, "get_action", (STATE,), ValueError, match)
        _refused(c, "get_actions", (STATES,), ValueError, match)
    # with proposals
    prop = np.zeros((2, H, A))
    _refused(make(knots=2), "get_action", (STATE, None, None, prop), NotImplementedError,
             f"{kind}controller: proposals= / policy_prior are not built together with knots")
    _refused(make(knots=2), "get_actions", (STATES, None, None, np.zeros((2, 2, H, A))), NotImplementedError,
             f"{kind}controller: proposals= / policy_prior are not built together with knots")
    # over an ensemble
    _refused(make(_ensemble(), knots=2), "get_action", (STATE,), NotImplementedError,
             f"{kind}controller: knots are not built over an EnsembleDynamicsModel")
    # on more than one rank (MPPI refuses the ranks themselves first)
    monkeypatch.setattr(distributed, "world", lambda group=None: (0, 2))
    _refused(make(knots=2), "get_action", (STATE,), NotImplementedError,
             "knots are not built for more than one rank" if kind == "CEM" else "MPPIcontroller runs on one rank")


def test_engine_wrapper_refusals():
    """The engine methods' own checks run before the library is called (an engine double without a handle)."""
    from bc_mpc_amd import engine, ensemble

    class Dummy(engine._EngineCalls):
        horizon, action_dim, state_dim, num_paths = H, A, S, K

    d = Dummy()
    assert d._knots(None, "linear", None) is None
    kn = d._knots(2, "cubic", None)
    assert (kn.count, kn.kind) == (2, 2)
    with pytest.raises(ValueError, match="knots"):
        d._knots(H + 1, "linear", None)
    with pytest.raises(ValueError, match="knot_interp"):
        d._knots(None, "spline", None)
    with pytest.raises(NotImplementedError, match="knots with proposals"):
        d._knots(2, "linear", np.zeros((1, H, A)))
    assert engine._EngineCalls._CEM_K == "bcmpc_cem_get_action_k" and engine._EngineCalls._MPPI_K == "bcmpc_mppi_get_action_k"
    assert ensemble.EnsembleEngine._CEM_K is None and ensemble.EnsembleEngine._MPPI_K is None

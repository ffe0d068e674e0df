"""MPPI's host side, no GPU: the two symbols (ABI still 5), argument errors answered before any HIP
call, and MPPIcontroller's constructor / warm start / reset logic.  The kernels are pinned in
tests/test_gpu_mppi.py."""
import ctypes

import numpy as np
import pytest


def test_mppi_symbols_are_exported_and_abi_is_still_5():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_abi_version() == 5 == _lib.ABI_VERSION
    bound = {s[0]: s for s in _lib.SIGNATURES}
    for name in ("bcmpc_mppi_get_action", "bcmpc_mppi_update_async"):
        assert name in bound
        fn = getattr(lib, name)                       # AttributeError on a library without MPPI
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == bound[name][2]
    assert len(bound["bcmpc_mppi_get_action"][2]) == 8 and len(bound["bcmpc_mppi_update_async"][2]) == 11


def test_mppi_record_layouts_match_the_c_structs():
    from bc_mpc_amd import _lib
    # bcmpc_mppi {int32, double, int64}: natural alignment puts lambda at 8
    assert ctypes.sizeof(_lib.Mppi) == 24 and _lib.Mppi.lambda_.offset == 8 and _lib.Mppi.k_global.offset == 16
    assert ctypes.sizeof(_lib.MppiStats) == 32
    assert [f[0] for f in _lib.MppiStats._fields_] == ["weight_sum", "ess", "min_cost", "n_valid"]


def test_null_arguments_are_argument_errors_without_hip():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    state, mu, sd = np.zeros(20), np.zeros((3, 6)), np.ones((3, 6))
    p = _lib.Mppi(1, 1.0, 0)
    res, stats = _lib.Result(), _lib.MppiStats()
    rc = lib.bcmpc_mppi_get_action(None, state.ctypes.data_as(dp), ctypes.byref(p), 0, mu.ctypes.data_as(dp),
                                   sd.ctypes.data_as(dp), ctypes.byref(res), ctypes.byref(stats))
    assert rc == _lib.ERR_ARG
    assert b"null" in lib.bcmpc_last_error()
    rc = lib.bcmpc_mppi_update_async(None, None, 1, 0, 0, 0, 1.0, None, None, None, None)
    assert rc == _lib.ERR_ARG
    assert b"null" in lib.bcmpc_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


class _Box:
    low, high = np.array([-1, -1, -2, 0, -1, -1], np.float32), np.array([1, 1, 2, 4, 1, 1], np.float32)
    shape = (6,)


class _Env:
    action_space = _Box()

    class observation_space:
        shape = (20,)


def _ctrl(**kw):
    from bc_mpc_amd import MPPIcontroller, cheetah_cost_fn
    kw.setdefault("horizon", 4)
    kw.setdefault("num_simulated_paths", 16)
    return MPPIcontroller(_Env(), object(), cost_fn=cheetah_cost_fn, **kw)


def test_constructor_checks():
    with pytest.raises(ValueError):
        _ctrl(iterations=0)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _ctrl(temperature=t)
    c = _ctrl(temperature=2.5, iterations=3)
    assert c.temperature == 2.5 and c.iterations == 3 and c.last_mu is None and c.last_ess is None


def test_initial_distribution_warm_start_and_reset():
    c = _ctrl()
    mid = np.array([0, 0, 0, 2, 0, 0], np.float64)
    mu, sd = c.initial_distribution()
    assert mu.shape == sd.shape == (4, 6) and mu.dtype == np.float64
    assert np.array_equal(mu, np.tile(mid, (4, 1)))
    assert np.array_equal(sd, np.tile(np.array([0.5, 0.5, 1, 1, 0.5, 0.5]), (4, 1)))     # (high - low) / 4
    prev = np.arange(24, dtype=np.float64).reshape(4, 6)
    c._mu = prev
    mu, _ = c.initial_distribution()
    assert np.array_equal(mu[:-1], prev[1:]) and np.array_equal(mu[-1], mid)            # shifted, centre appended
    c.reset()
    assert np.array_equal(c.initial_distribution()[0], np.tile(mid, (4, 1)))
    # a plan of another shape (the horizon changed) is not reused; warm_start=False never reuses
    c._mu = prev[:3]
    assert np.array_equal(c.initial_distribution()[0], np.tile(mid, (4, 1)))
    cold = _ctrl(warm_start=False, init_std=0.3)
    cold._mu = prev
    mu, sd = cold.initial_distribution()
    assert np.array_equal(mu, np.tile(mid, (4, 1))) and (sd == 0.3).all()


def test_empty_candidate_set_and_horizon_raise_like_cem():
    from bc_mpc_amd import CEMcontroller, cheetah_cost_fn
    state = np.zeros(20)
    for kw in (dict(num_simulated_paths=0), dict(horizon=0)):
        cem = CEMcontroller(_Env(), object(), cost_fn=cheetah_cost_fn, **{"horizon": 4, "num_simulated_paths": 16, **kw})
        with pytest.raises((ValueError, IndexError)) as want:
            cem.get_action(state)
        with pytest.raises(want.type) as got:
            _ctrl(**kw).get_action(state)
        assert str(got.value) == str(want.value)

"""The batched control step's host side, no GPU: ABI 5, the two new symbols, argument errors that are
answered before any HIP call, and the controllers' refusal of the host-stream RNG modes."""
import ctypes

import numpy as np
import pytest


def test_abi_is_5():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_abi_version() == 5 == _lib.ABI_VERSION


def test_batch_symbols_are_bound():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    bound = {s[0]: s for s in _lib.SIGNATURES}
    for name in ("bcmpc_get_actions_batch", "bcmpc_rollout_batch_async"):
        assert name in bound
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == bound[name][2]
    assert len(bound["bcmpc_get_actions_batch"][2]) == 8 and len(bound["bcmpc_rollout_batch_async"][2]) == 9


def test_null_engine_is_an_argument_error_without_hip():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    states = np.zeros((2, 20))
    out = (_lib.Result * 2)()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib.bcmpc_get_actions_batch(None, states.ctypes.data_as(dp), 2, None, 0, 0, out, None)
    assert rc == _lib.ERR_ARG
    assert b"null" in lib.bcmpc_last_error()
    rc = lib.bcmpc_rollout_batch_async(None, None, 2, None, 0, 0, None, None, None)
    assert rc == _lib.ERR_ARG
    with pytest.raises(ValueError):
        _lib.check(rc)


class _Box:
    low, high = -np.ones(6), np.ones(6)
    shape = (6,)


class _Env:
    action_space = _Box()

    class observation_space:
        shape = (20,)


def test_host_stream_rng_modes_refuse_the_batched_step():
    """rng="numpy" / "env" promise one host-stream draw per get_action call in the reference's order; the
    batched step cannot keep it and says so before any GPU work (no model is ever looked at)."""
    from bc_mpc_amd import MPCcontroller, MPCcontrollerReward, cheetah_cost_fn
    states = np.zeros((3, 20))
    st = np.random.get_state()
    ctrl = MPCcontroller(_Env(), object(), horizon=5, cost_fn=cheetah_cost_fn, num_simulated_paths=8, rng="numpy")
    with pytest.raises(ValueError, match="rng='device'"):
        ctrl.get_actions(states)
    assert ctrl._engine is None and getattr(ctrl, "_batch_engine", None) is None
    rew = MPCcontrollerReward(_Env(), object(), horizon=5, num_simulated_paths=8, rng="env")
    with pytest.raises(ValueError, match="rng='device'"):
        rew.get_actions(states)
    assert rew._engine is None and getattr(rew, "_batch_engine", None) is None
    now = np.random.get_state()
    assert np.array_equal(st[1], now[1]) and st[2] == now[2]      # nothing was drawn

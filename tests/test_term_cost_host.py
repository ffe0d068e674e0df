"""Declarative cost terms, the parts that need no GPU: the ABI additions, cost_functions.TermCost (the NumPy
definition the kernel is tested against, tests/test_gpu_term_cost.py) and the controllers' routing."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO


def test_symbols_exported_abi_still_5_and_term_struct_is_32_bytes():
    import bc_mpc_amd
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_abi_version() == 5 == _lib.ABI_VERSION
    for name in ("bcmpc_set_cost_terms", "bcmpc_trajectory_cost_async"):
        assert hasattr(lib, name), name
    assert _lib.COST_TERMS == 3 and _lib.MAX_COST_TERMS == 32
    assert ctypes.sizeof(_lib.CostTerm) == 32
    for name in ("TermCost", "cheetah_terms"):
        assert name in bc_mpc_amd.__all__ and hasattr(bc_mpc_amd, name)
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "bcmpc.h"
int main(void) {
  printf("%zu %zu %zu %d %d %d\n", sizeof(bcmpc_cost_term), offsetof(bcmpc_cost_term, cmp),
         offsetof(bcmpc_cost_term, param), (int)BCMPC_COST_TERMS, (int)BCMPC_MAX_COST_TERMS, (int)BCMPC_ABI_VERSION);
  printf("%d %d %d %d %d %d %d %d %d %d %d\n", BCMPC_TERM_THRESHOLD, BCMPC_TERM_DIFF, BCMPC_TERM_LINEAR,
         BCMPC_TERM_QUADRATIC, BCMPC_SRC_STATE, BCMPC_SRC_NEXT_STATE, BCMPC_SRC_ACTION, BCMPC_CMP_GE, BCMPC_CMP_GT,
         BCMPC_CMP_LE, BCMPC_CMP_LT);
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].split() == ["32", str(_lib.CostTerm.cmp.offset), str(_lib.CostTerm.param.offset), "3", "32", "5"]
    from bc_mpc_amd import cost_functions as cf
    want = [cf.THRESHOLD, cf.DIFF, cf.LINEAR, cf.QUADRATIC, cf.STATE, cf.NEXT_STATE, cf.ACTION, cf.GE, cf.GT, cf.LE,
            cf.LT]
    assert [int(x) for x in out[1].split()] == want
    assert want == [_lib.TERM_THRESHOLD, _lib.TERM_DIFF, _lib.TERM_LINEAR, _lib.TERM_QUADRATIC, _lib.SRC_STATE,
                    _lib.SRC_NEXT_STATE, _lib.SRC_ACTION, _lib.CMP_GE, _lib.CMP_GT, _lib.CMP_LE, _lib.CMP_LT]


def test_entry_points_validate_without_gpu():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_set_cost_terms(None, None, 0) == _lib.ERR_ARG
    assert lib.bcmpc_trajectory_cost_async(None, None, None, 0, 0, None, None, 0, 1, None, None) == _lib.ERR_ARG
    # argument validation runs before any HIP call: a cost-term engine cannot carry a fused policy
    cfg = _lib.Config(state_dim=20, action_dim=6, hidden=500, n_layers=2, horizon=5, num_paths=16,
                      cost=_lib.COST_TERMS, policy_hidden=64, policy_layers=2)
    h = ctypes.c_void_p()
    assert lib.bcmpc_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert b"policy" in lib.bcmpc_last_error()
    cfg.policy_hidden, cfg.cost = 0, 4
    assert lib.bcmpc_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert b"unknown cost" in lib.bcmpc_last_error()


def probe_batch(state_dim=20, action_dim=6):
    """cost_functions._probe's batch: rows exactly on each of the cheetah cost's thresholds."""
    rs = np.random.RandomState(20240601)
    s = rs.standard_normal((64, state_dim)) * 0.3
    s[:8, 5] = 0.2
    s[8:16, 6] = 0.0
    s[16:24, 7] = 0.0
    ns = s + rs.standard_normal((64, state_dim)) * 0.01
    a = rs.uniform(-1, 1, (64, action_dim))
    return s, a, ns


def test_cheetah_terms_is_cheetah_cost_fn_bit_for_bit():
    from bc_mpc_amd.cost_functions import (_probe, cheetah_cost_fn, cheetah_terms, is_cheetah_cost,
                                           trajectory_cost_fn)
    T = cheetah_terms()
    assert _probe(T, 20, 6)                         # the probe's own verdict on its own batch
    assert not is_cheetah_cost(T, 20, 6)            # ... but a TermCost always takes the terms path
    s, a, ns = probe_batch()
    want = cheetah_cost_fn(s, a, ns)
    assert (want >= 10).any() and np.array_equal(T(s, a, ns), want)
    for i in range(s.shape[0]):
        one = T(s[i], a[i], ns[i])
        assert isinstance(one, float) and np.array_equal(one, cheetah_cost_fn(s[i], a[i], ns[i])), i
    # through trajectory_cost_fn over H = 5: states chained so that step h's s' is step h + 1's s
    rs = np.random.RandomState(5)
    H, K = 5, 64
    traj = np.cumsum(np.concatenate([s[None], 0.01 * rs.standard_normal((H, K, 20))]), axis=0)
    traj[2, :8, 5], traj[3, 8:16, 6], traj[4, 16:24, 7] = 0.2, 0.0, 0.0
    acts = rs.uniform(-1, 1, (H, K, 6))
    got = trajectory_cost_fn(T, traj[:-1], acts, traj[1:])
    assert np.array_equal(got, trajectory_cost_fn(cheetah_cost_fn, traj[:-1], acts, traj[1:]))


def py_float_cost(terms, s, a, ns):
    """Section 1 of the cost language restated on Python floats, one transition (independent of NumPy's
    broadcasting and np.where): acc = 0.0, then the terms in order, one rounded operation at a time."""
    acc = 0.0
    for kind, source, index, cmp, weight, param in terms:
        x = float((s, ns, a)[source][index])
        if kind == 0:
            hit = (x >= param, x > param, x <= param, x < param)[cmp]
            if hit:
                acc = acc + weight
        elif kind == 1:
            d = float(ns[index]) - float(s[index])
            acc = acc + weight * (d / param)
        elif kind == 2:
            acc = acc + weight * x
        else:
            d = x - param
            acc = acc + weight * (d * d)
    return acc


def random_terms(rs, S, A, n):
    """n terms covering every kind, source and cmp (cycled), thresholds on values the data holds exactly."""
    from bc_mpc_amd import cost_functions as cf
    terms = []
    for i in range(n):
        kind = i % 4
        source = (i // 4) % 3
        index = int(rs.randint(A if source == cf.ACTION else S))
        w = float(rs.choice([-1.0, 10.0, 0.1, -2.5, 1e-3, 3.0]))
        if kind == cf.THRESHOLD:
            terms.append(cf.Term(kind, source, index, (i // 4) % 4, w, float(rs.choice([0.0, 0.2, -0.5, 0.25]))))
        elif kind == cf.DIFF:
            terms.append(cf.progress(int(rs.randint(S)), float(rs.choice([0.01, 0.05, -0.02, 3.0])), w))
        elif kind == cf.LINEAR:
            terms.append(cf.Term(kind, source, index, 0, w, 0.0))
        else:
            terms.append(cf.Term(kind, source, index, 0, w, float(rs.choice([0.0, 0.7, -1.25]))))
    return terms


@pytest.mark.parametrize("S,A,n", [(5, 2, 32), (20, 6, 32), (11, 3, 17), (20, 6, 0)])
def test_termcost_call_equals_the_python_float_restatement(S, A, n):
    from bc_mpc_amd import cost_functions as cf
    rs = np.random.RandomState(100 * S + n)
    terms = random_terms(rs, S, A, n)
    if n == 32:
        kinds = {(t.kind, t.source) for t in terms if t.kind != cf.DIFF}
        assert len(kinds) == 9 and {t.cmp for t in terms if t.kind == cf.THRESHOLD} == {0, 1, 2, 3}
    T = cf.TermCost(terms)
    N = 96
    s, ns = rs.standard_normal((N, S)), rs.standard_normal((N, S))
    a = rs.uniform(-1, 1, (N, A))
    for arr in (s, ns, a):                               # values exactly on the thresholds, NaN and +-inf
        flat = arr.reshape(-1)
        pos = rs.choice(flat.size, flat.size // 3, replace=False)
        flat[pos] = np.resize([0.0, 0.2, -0.5, 0.25, -0.0], pos.size)
    s[3, :], ns[4, :], a[5, :] = np.nan, np.inf, -np.inf
    s[6, 0] = np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        got = T(s, a, ns)
        assert got.shape == (N,) and got.dtype == np.float64
        want = np.array([py_float_cost(terms, s[i], a[i], ns[i]) for i in range(N)])
        assert np.array_equal(got, want, equal_nan=True)
        for i in range(N):
            one = T(s[i], a[i], ns[i])
            assert isinstance(one, float) and (one == want[i] or (math.isnan(one) and math.isnan(want[i])))
    if n == 0:
        assert not got.any()


def test_validation_rules_raise_value_error():
    from bc_mpc_amd import cost_functions as cf
    ok = cf.threshold(0, ">=", 0.0, 1.0)
    bad = [
        lambda: cf.threshold(0, "==", 0.0, 1.0),                       # unknown cmp
        lambda: cf.threshold(0, ">=", 0.0, 1.0, on="reward"),          # unknown source
        lambda: cf.TermCost([(7, 0, 0, 0, 1.0, 0.0)]),                 # unknown kind
        lambda: cf.TermCost([(0, 3, 0, 0, 1.0, 0.0)]),                 # unknown source
        lambda: cf.TermCost([(0, 0, 0, 4, 1.0, 0.0)]),                 # unknown cmp
        lambda: cf.TermCost([(1, 2, 0, 0, 1.0, 0.01)]),                # DIFF on an action
        lambda: cf.TermCost([(1, 1, 0, 0, 1.0, 0.01)]),                # DIFF on the next state
        lambda: cf.TermCost([cf.progress(0, 0.0)]),                    # dt == 0
        lambda: cf.TermCost([cf.progress(0, math.inf)]),               # dt not finite
        lambda: cf.TermCost([cf.linear(0, math.nan)]),                 # weight not finite
        lambda: cf.TermCost([cf.quadratic(0, 1.0, target=math.inf)]),  # param not finite
        lambda: cf.TermCost([cf.linear(-1, 1.0)]),                     # negative index
        lambda: cf.TermCost([ok] * 33),                                # more than 32 terms
        lambda: cf.TermCost([cf.linear(11, 1.0)]).validate(11, 3),     # index == S
        lambda: cf.TermCost([cf.linear(3, 1.0, on="action")]).validate(11, 3),   # index == A
        lambda: cf.TermCost([cf.linear(11, 1.0, on="next_state")]).validate(11, 3),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"rule {i} did not raise")
    cf.TermCost([ok] * 32).validate(1, 1)
    cf.TermCost([cf.linear(10, 1.0), cf.linear(2, 1.0, on="action")]).validate(11, 3)
    assert len(cf.TermCost()) == 0


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


def test_plain_callables_route_exactly_as_before():
    """A lambda is neither the cheetah cost nor a TermCost: the planners refuse it with the same messages,
    MPCcontroller sends it to the host path (rng="numpy") or refuses (rng="device", get_actions) -- all
    before any engine exists."""
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller
    S, A = 11, 3
    env, dyn = _Env(S, A), _model(S, A)
    fn = lambda s, a, ns: np.zeros(s.shape[0])   # noqa: E731
    state, states = np.zeros(S), np.zeros((2, S))
    for cls, name in ((CEMcontroller, "CEMcontroller"), (MPPIcontroller, "MPPIcontroller")):
        c = cls(env, dyn, horizon=3, cost_fn=fn, num_simulated_paths=8)
        for call, arg in ((c.get_action, state), (c.get_actions, states)):
            with pytest.raises(ValueError, match=f"{name} needs the fused cheetah cost_fn"):
                call(arg)
            assert c._engine is None and c._batch_engine is None
    c = MPCcontroller(env, dyn, horizon=3, cost_fn=fn, num_simulated_paths=8, rng="device", seed=1)
    with pytest.raises(ValueError, match="non-cheetah cost_fn needs rng='numpy'"):
        c.get_action(state)
    with pytest.raises(ValueError, match="get_actions needs the fused cheetah cost_fn"):
        c.get_actions(states)
    assert c._engine is None
    # rng="numpy": the host path -- an engine without a fused cost, the trajectory scored by the callable
    c = MPCcontroller(env, dyn, horizon=3, cost_fn=fn, num_simulated_paths=8)
    seen = {}

    def engine_for(spec, S_, A_, k_local, fused, *terms):
        seen["args"] = (fused, terms)
        raise RuntimeError("stop before the GPU")
    c._engine_for = engine_for
    with pytest.raises(RuntimeError, match="stop before the GPU"):
        c.get_action(state)
    assert seen["args"] == (False, ())


def test_a_termcost_routes_to_a_terms_engine():
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller, TermCost
    from bc_mpc_amd.cost_functions import linear, threshold
    S, A = 11, 3
    env, dyn = _Env(S, A), _model(S, A)
    T = TermCost([threshold(0, "<", 0.7, 5.0), linear(2, 0.1, on="action")])
    state, states = np.zeros(S), np.zeros((2, S))

    class Stop(Exception):
        pass

    def stopper(seen):
        def engine_for(*args):
            seen.append(args)
            raise Stop()
        return engine_for
    for rng in ("numpy", "device"):
        c = MPCcontroller(env, dyn, horizon=3, cost_fn=T, num_simulated_paths=8, rng=rng, seed=1)
        seen = []
        c._engine_for = stopper(seen)
        with pytest.raises(Stop):
            c.get_action(state)
        assert seen[0][4] is False and seen[0][5] is T        # not the fused cheetah cost; the terms
    for cls in (CEMcontroller, MPPIcontroller):
        c = cls(env, dyn, horizon=3, cost_fn=T, num_simulated_paths=8)
        seen = []
        c._engine_for = c._batch_engine_for = stopper(seen)
        for call, arg in ((c.get_action, state), (c.get_actions, states)):
            with pytest.raises(Stop):
                call(arg)
        assert [a[-1] for a in seen] == [T, T]

"""Episode termination for TermCost, the parts that need no GPU: cost_functions.done_when / TermCost.done /
episode_cost (the NumPy definition csrc/term_cost.hip is tested against, tests/test_gpu_termination.py), the gated
value add of value.add_to_costs, and the new C entry points' answers to a null engine.  Every comparison is bit
for bit."""
import ctypes

import numpy as np
import pytest

from bc_mpc_amd import cost_functions as cf
from bc_mpc_amd import value


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def hopper_cost(done_cost=0.0, done=True):
    terms = [cf.progress(5, 0.008), cf.threshold(1, ">=", 0.1, 3.0, on="next_state"), cf.linear(10, 0.05),
             cf.quadratic(2, 0.001, on="action")]
    conds = [cf.done_when(0, "<=", 0.7), cf.done_when(1, ">=", 0.2), cf.done_when(1, "<=", -0.2)]
    return cf.TermCost(terms, done=conds if done else (), done_cost=done_cost)


def random_traj(H, K, S=11, A=3, seed=0):
    rs = np.random.RandomState(seed)
    traj = rs.standard_normal((H + 1, K, S))
    traj[..., 0] += 1.5
    traj[..., 1] *= 0.1
    return traj, rs.uniform(-1, 1, (H, K, A))


@pytest.mark.parametrize("H,K", [(1, 1), (7, 65), (17, 400)])
def test_without_done_episode_cost_is_trajectory_cost_fn_bit_for_bit(H, K):
    traj, acts = random_traj(H, K, seed=H)
    traj[H // 2, K // 2, 5] = np.nan
    traj[0, 0, 10] = -0.0
    T = hopper_cost(done=False)
    costs, t = cf.episode_cost(T, traj[:-1], acts, traj[1:])
    with np.errstate(invalid="ignore"):
        want = np.asarray(cf.trajectory_cost_fn(T, traj[:-1], acts, traj[1:]), dtype=np.float64)
    assert costs.dtype == np.float64 and t.dtype == np.int32 and costs.shape == t.shape == (K,)
    assert np.array_equal(bits(costs), bits(want))
    assert (t == H).all()
    # conditions that never hold change nothing either
    never = cf.TermCost(T.terms, done=[cf.done_when(0, "<", -1e300)], done_cost=5.0)
    c2, t2 = cf.episode_cost(never, traj[:-1], acts, traj[1:])
    assert np.array_equal(bits(c2), bits(want)) and (t2 == H).all()


def test_hand_worked_three_steps_with_done_cost():
    # one state dim; cost = 2 * s'[0]; done when s'[0] <= 0.5; done_cost 100
    T = cf.TermCost([cf.linear(0, 2.0, on="next_state")], done=[cf.done_when(0, "<=", 0.5)], done_cost=100.0)
    #            never    at h=1     at h=0     at h=2 (= H - 1)
    s1 = np.array([1.0,   1.0,       0.5,       1.0])
    s2 = np.array([2.0,   0.25,      9.0,       1.0])
    s3 = np.array([3.0,   7.0,       9.0,       0.0])
    traj = np.stack([np.ones(4), s1, s2, s3])[..., None]
    acts = np.zeros((3, 4, 1))
    costs, t = cf.episode_cost(T, traj[:-1], acts, traj[1:])
    assert t.tolist() == [3, 1, 0, 2]
    assert costs.tolist() == [2.0 + 4.0 + 6.0, 2.0 + 0.5 + 100.0, 1.0 + 100.0, 2.0 + 2.0 + 0.0 + 100.0]
    assert T.done(traj[1:]).tolist() == [[False, False, True, False], [False, True, False, False],
                                         [False, False, False, True]]
    # the per-step cost and trajectory_cost_fn do not know about done
    assert np.array_equal(cf.trajectory_cost_fn(T, traj[:-1], acts, traj[1:]), 2.0 * (s1 + s2 + s3))
    # the order of the operations: (total + c_h) + done_cost, each rounded
    T2 = cf.TermCost([cf.linear(0, 1.0, on="next_state")], done=[cf.done_when(1, "<", 0.0)], done_cost=1.0)
    big = 2.0 ** 53
    tr = np.array([[0.0, 1.0], [big, 1.0], [1.0, -1.0]])[:, None, :]
    c, tt = cf.episode_cost(T2, tr[:-1], np.zeros((2, 1, 1)), tr[1:])
    assert tt.tolist() == [1] and c[0] == ((0.0 + big) + 1.0) + 1.0 == big and c[0] != big + (1.0 + 1.0)


def test_nan_never_terminates_and_termination_at_the_last_step():
    H, K = 5, 6
    traj = np.ones((H + 1, K, 2))
    traj[1:, 0, 0] = np.nan                     # NaN in the done dimension from step 0 on
    traj[3, 1, 0] = np.nan                      # a NaN row, then a real termination later
    traj[5, 1, 0] = 0.0
    traj[H, 2, 0] = 0.0                         # terminates on the last step: t = H - 1
    traj[H, 3, 0] = np.inf                      # +inf is not <= 0.5
    traj[2, 4, 0] = -np.inf                     # -inf is
    T = cf.TermCost([cf.linear(0, 1.0, on="next_state")], done=[cf.done_when(0, "<=", 0.5)], done_cost=-2.5)
    costs, t = cf.episode_cost(T, traj[:-1], np.zeros((H, K, 1)), traj[1:])
    assert t.tolist() == [H, H - 1, H - 1, H, 1, H]
    assert np.isnan(costs[0]) and np.isnan(costs[1])
    assert costs[2] == 4.0 + 0.0 - 2.5 and costs[3] == np.inf and costs[4] == -np.inf and costs[5] == 5.0
    assert not T.done(np.array([np.nan, 0.0]))
    # both signs of a comparison on one dimension, as Hopper's angle band
    band = cf.TermCost([], done=[cf.done_when(1, ">=", 0.2), cf.done_when(1, "<=", -0.2)])
    assert band.done(np.array([[0, 0.2], [0, 0.19], [0, -0.2], [0, np.nan]])).tolist() == [True, False, True, False]


def test_done_cost_zero_and_minus_zero():
    T = lambda dc: cf.TermCost([cf.linear(0, 1.0, on="next_state")], done=[cf.done_when(1, ">", 0.0)], done_cost=dc)
    traj = np.zeros((2, 1, 2))
    traj[1, 0] = [-0.0, 1.0]
    acts = np.zeros((1, 1, 1))
    # total = (0.0 + 1.0 * -0.0) + done_cost: +0.0 either way, but the keys differ
    for dc in (0.0, -0.0):
        c, t = cf.episode_cost(T(dc), traj[:-1], acts, traj[1:])
        assert t.tolist() == [0] and bits(c)[0] == bits(0.0 + -0.0 + dc)
    assert T(0.0).key() != T(-0.0).key() and T(0.0).key() == T(0.0).key()


def test_key_is_unchanged_without_done_and_differs_with_it():
    plain = hopper_cost(done=False)
    assert plain.key() == plain.terms and plain.key() is plain.terms
    assert cf.cheetah_terms().key() == cf.cheetah_terms().terms
    a, b, c = hopper_cost(0.0), hopper_cost(1.0), hopper_cost(0.0)
    assert a.key() == c.key() and a.key() != b.key() and a.key() != plain.key()
    fewer = cf.TermCost(a.terms, done=a.done_conditions[:2])
    assert fewer.key() != a.key()
    assert "done=" in repr(a) and "done=" not in repr(plain)
    assert len(a) == len(plain) == 4
    # __call__ ignores done
    traj, acts = random_traj(3, 9)
    assert np.array_equal(a(traj[0], acts[0], traj[1]), plain(traj[0], acts[0], traj[1]))


def test_constructor_refusals():
    terms = [cf.linear(0, 1.0)] * 30
    conds = [cf.done_when(0, "<", 0.0)] * 3
    cf.TermCost(terms, done=conds[:2])
    with pytest.raises(ValueError, match="at most 32"):
        cf.TermCost(terms, done=conds)
    with pytest.raises(ValueError, match="at most 32"):
        cf.TermCost([], done=[cf.done_when(0, "<", 0.0)] * 33)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="done_cost must be finite"):
            cf.TermCost([], done=conds[:1], done_cost=bad)
    for op in ("==", "!=", "ge", ""):
        with pytest.raises(ValueError, match="op must be one of"):
            cf.done_when(0, op, 0.0)
    with pytest.raises(ValueError, match="done condition 0"):
        cf.TermCost([], done=[cf.threshold(0, "<", 0.0, 1.0)])             # a weighted STATE threshold
    with pytest.raises(ValueError, match="done condition 0"):
        cf.TermCost([], done=[cf.linear(0, 0.0, on="next_state")])
    with pytest.raises(ValueError, match="done condition 1"):
        cf.TermCost([], done=[cf.done_when(0, "<", 0.0), cf.done_when(0, "<", np.nan)])
    with pytest.raises(ValueError, match="negative index"):
        cf.TermCost([], done=[cf.done_when(-1, "<", 0.0)])
    with pytest.raises(ValueError, match=r"done condition 0: index 11 outside \[0, 11\)"):
        cf.TermCost([], done=[cf.done_when(11, "<", 0.0)]).validate(11, 3)
    hopper_cost().validate(11, 3)


def test_the_gated_value_add_leaves_terminated_totals_untouched():
    H = 4
    costs = np.array([1.5, -0.0, -0.0, np.nan, 7.0, -0.0])
    v = np.array([2.0, 0.0, 3.0, 1.0, np.nan, 0.0], dtype=np.float32)
    t = np.array([H, 2, H, 0, H, H], dtype=np.int32)
    w = 0.5
    plain = value.add_to_costs(costs, v, w)
    assert np.array_equal(bits(plain), bits(costs + np.float64(w) * v.astype(np.float64)))      # the call form of before
    got = value.add_to_costs(costs, v, w, term_step=t, horizon=H)
    alive = t == H
    assert np.array_equal(bits(got)[alive], bits(plain)[alive])
    assert np.array_equal(bits(got)[~alive], bits(costs)[~alive])
    assert bits(got)[1] == bits(-0.0) and bits(plain)[1] == bits(0.0)          # -0.0 + 0.5 * 0 would be +0.0
    assert got[2] == 1.5 and np.isnan(got[3]) and np.isnan(got[4]) and bits(got)[5] == bits(0.0)
    with pytest.raises(ValueError, match="horizon"):
        value.add_to_costs(costs, v, w, term_step=t)


def test_new_symbols_exist_and_answer_a_null_engine_with_err_arg():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_abi_version() == 5 == _lib.ABI_VERSION
    for name in ("bcmpc_set_termination", "bcmpc_trajectory_cost_steps_async", "bcmpc_terminal_value_masked_async",
                 "bcmpc_last_termination_steps"):
        assert hasattr(lib, name), name
    cond = (_lib.CostTerm * 1)()
    cond[0].kind, cond[0].source, cond[0].cmp, cond[0].param = _lib.TERM_THRESHOLD, _lib.SRC_NEXT_STATE, _lib.CMP_LE, 0.7
    idx, out = (ctypes.c_int64 * 1)(0), (ctypes.c_int32 * 1)(0)
    dummy = ctypes.c_void_p(4096)
    calls = [
        lib.bcmpc_set_termination(None, cond, 1, 0.0),
        lib.bcmpc_set_termination(None, None, 0, 0.0),
        lib.bcmpc_trajectory_cost_steps_async(None, dummy, None, 0, 0, None, None, 0, 4, dummy, dummy, None),
        lib.bcmpc_terminal_value_masked_async(None, dummy, 4, 4, None, dummy, dummy, 3, None),
        lib.bcmpc_last_termination_steps(None, idx, 1, out),
    ]
    assert calls == [_lib.ERR_ARG] * len(calls)
    assert lib.bcmpc_last_error().decode() == "null argument"

"""The batched control step on the GPU: B environments x K candidates in one launch chain
(bcmpc_get_actions_batch / bcmpc_rollout_batch_async, csrc/batch.hip).

Contract: candidate column c = b*K + j belongs to environment b, starts from states[b] and has the
Philox index cand_offset + c; record b equals get_action(states[b], seed, cand_offset + b*K) of a
K-candidate engine of the same kernel layout.

The reference of each environment is composed from the oracle: device_rng_actions(seed, cand_offset +
b*K, K, ...) rolled out from synthetic_state(norm, seed=11 + b).  Cost bar: the suite's own (ATOL = 1e-4,
RTOL = 1e-5, capped by conftest.envelope), as in test_gpu_parity.py.  At these shapes every
environment's oracle top-2 gap is >= 0.13 (> 500x the bar) and no candidate is within 1e-4 of a penalty
threshold, so the argmin assertions run for every environment, none skipped.

Shapes: K = 37 and 17 straddle the rollout kernels' 16- and 64-candidate tiles (environment boundaries
fall inside tiles), K = 1 is the smallest segment; all are single-workgroup-per-environment argmins.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import RewardGolden, envelope
from test_gpu_parity import assert_costs_close, team_ok

pytestmark = pytest.mark.gpu

S, A = 20, 6
LOW, HIGH = -np.ones(A), np.ones(A)

#        hidden act    ln     H  K   B  seed
CASES = {
    "A": (64, "tanh", False, 5, 37, 5, 1234),
    "B": (128, "relu", True, 3, 17, 3, 77),
    "C": (64, "tanh", False, 1, 1, 4, 5),
}
PARITY = [("A", 0), ("A", 1000), ("B", 0), ("C", 0)]
KERNELS = ["auto", "solo", "group4", "split2", "team"]


class Ref:
    """One case's inputs and its per-environment oracle answers (read-only, shared by the tests)."""

    def __init__(self, case, cand_offset):
        from oracle import mpc_oracle as orc
        self.hidden, self.act, self.ln, self.H, self.K, self.B, self.seed = CASES[case]
        self.case, self.cand_offset = case, cand_offset
        self.w = orc.synthetic_weights(S, A, self.hidden, 2, self.act, self.ln)
        self.norm = orc.synthetic_normalization()
        dyn = orc.NumpyDynamics(self.w, self.norm)
        self.states = np.stack([orc.synthetic_state(self.norm, seed=11 + b) for b in range(self.B)])
        acts, costs = [], []
        for b in range(self.B):
            a = orc.device_rng_actions(self.seed, cand_offset + b * self.K, self.K, self.H, LOW, HIGH)
            c, _ = orc.rollout(dyn, self.states[b], a)
            acts.append(a)
            costs.append(c)
        self.actions = np.ascontiguousarray(np.concatenate(acts, axis=1))      # [H, B*K, A], kernels' layout
        self.costs = np.stack(costs)                                           # [B, K]
        self.argmin = np.argmin(self.costs, axis=1)
        for x in (self.states, self.actions, self.costs, self.argmin):
            x.setflags(write=False)
        self.env = envelope(self.ln, 2, self.hidden, self.H)

    def engine(self, kernel="auto", K=None, **kw):
        from bc_mpc_amd.engine import MLPSpec, RolloutEngine
        w = self.w
        eng = RolloutEngine(S, A, w.hidden, 2, w.activation, w.layer_norm, self.H,
                            self.B * self.K if K is None else K, device=0, kernel=kernel, **kw)
        if kernel != "auto":
            assert eng.info()["kernel"] == kernel
        eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta), self.norm, 1)
        return eng


@functools.lru_cache(maxsize=None)
def ref(case, cand_offset=0) -> Ref:
    return Ref(case, cand_offset)


def _skip_unsupported(r: Ref, kernel):
    """test_gpu_parity.py's rules for these shapes (group8 / hidden > 512 do not occur here)."""
    if kernel == "team" and not team_ok(r.hidden, r.ln, 2, r.B * r.K, S, A):
        pytest.skip("team: the 2-layer delta net at small K (grid resident)")


def same_record(a, b, ia=None, ib=None):
    """Bitwise equality of two records (BatchResult rows or StepResults)."""
    pick = lambda x, i, f: getattr(x, f) if i is None else getattr(x, f)[i]   # noqa: E731
    assert int(pick(a, ia, "best_index")) == int(pick(b, ib, "best_index"))
    ca, cb = np.float64(pick(a, ia, "best_cost")), np.float64(pick(b, ib, "best_cost"))
    assert ca.tobytes() == cb.tobytes() or (np.isnan(ca) and np.isnan(cb))
    assert np.array_equal(pick(a, ia, "first_action"), pick(b, ib, "first_action"), equal_nan=True)


# ------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case,cand_offset", PARITY)
def test_batch_matches_oracle(case, cand_offset, kernel):
    r = ref(case, cand_offset)
    _skip_unsupported(r, kernel)
    eng = r.engine(kernel)
    res = eng.get_actions(r.states, None, seed=r.seed, cand_offset=cand_offset, return_costs=True)
    eng.close()
    assert res.costs.shape == (r.B, r.K) and res.first_action.shape == (r.B, A)
    assert res.best_index.dtype == np.int64 and res.best_index.shape == (r.B,)
    for b in range(r.B):
        assert_costs_close(res.costs[b], r.costs[b], None, f"{case}+{cand_offset}/{kernel}/env{b}", env=r.env)
        j = int(res.best_index[b]) - cand_offset - b * r.K
        assert j == int(np.argmin(res.costs[b])) == int(r.argmin[b])
        assert np.array_equal(res.first_action[b], r.actions[0, b * r.K + j])
        assert res.best_cost[b] == res.costs[b, j]


# ------------------------------------------------------------------ 2. equivalence with the single call
@pytest.mark.parametrize("kernel", ["solo", "group4", "split2"])
@pytest.mark.parametrize("cand_offset", [0, 1000])
def test_batch_equals_single_calls(kernel, cand_offset):
    r = ref("A", cand_offset)
    eng = r.engine(kernel)
    res = eng.get_actions(r.states, None, seed=r.seed, cand_offset=cand_offset, return_costs=True)
    eng.close()
    one = r.engine(kernel, K=r.K)
    for b in range(r.B):
        s = one.get_action(r.states[b], None, seed=r.seed, cand_offset=cand_offset + b * r.K, return_costs=True)
        assert np.array_equal(res.costs[b], s.costs), f"env {b}: costs differ bitwise"
        same_record(res, s, b)
    # B = 1 on the K-candidate engine itself
    s = one.get_action(r.states[2], None, seed=r.seed, cand_offset=cand_offset, return_costs=True)
    b1 = one.get_actions(r.states[2:3], None, seed=r.seed, cand_offset=cand_offset, return_costs=True)
    one.close()
    assert b1.costs.shape == (1, r.K) and np.array_equal(b1.costs[0], s.costs)
    same_record(b1, s, 0)


# ------------------------------------------------------------------ 3. NaN
@pytest.mark.parametrize("kernel", ["auto", "solo"])
def test_batch_nan_wins_only_its_environment(kernel):
    r = ref("A", 0)
    eng = r.engine(kernel)
    clean = eng.get_actions(r.states, r.actions, return_costs=True)
    acts = r.actions.copy()
    acts[0, 1 * r.K + 3, 0] = np.nan
    acts[0, 1 * r.K + 9, 0] = np.nan
    res = eng.get_actions(r.states, acts, return_costs=True)
    eng.close()
    assert int(res.best_index[1]) - 1 * r.K == 3 and np.isnan(res.best_cost[1])
    assert np.array_equal(res.first_action[1], acts[0, r.K + 3], equal_nan=True)
    assert np.isnan(res.costs[1, 3]) and np.isnan(res.costs[1, 9]) and np.isnan(res.costs[1]).sum() == 2
    for b in (0, 2, 3, 4):
        assert np.array_equal(res.costs[b], clean.costs[b])
        same_record(res, clean, b, b)


# ------------------------------------------------------------------ 4. tie
@pytest.mark.parametrize("kernel", ["auto", "group4"])
def test_batch_tie_goes_to_the_lower_index(kernel):
    r = ref("A", 0)
    best = int(r.argmin[2])
    acts = r.actions.copy()
    for j in (4, 20):
        acts[:, 2 * r.K + j, :] = acts[:, 2 * r.K + best, :]
    eng = r.engine(kernel)
    res = eng.get_actions(r.states, acts, return_costs=True)
    eng.close()
    c = res.costs[2]
    assert c[4].tobytes() == c[20].tobytes() == c[best].tobytes()
    assert c[4] == c.min()
    assert int(res.best_index[2]) - 2 * r.K == min(4, 20, best) == int(np.argmin(c))
    for b in (0, 1, 3, 4):
        assert int(res.best_index[b]) - b * r.K == int(r.argmin[b])


# ------------------------------------------------------------------ 5. argmax (learned reward)
def test_batch_argmax_equals_single_calls():
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc
    g = RewardGolden("reward_tiny_g1")                  # hidden 64, no LayerNorm: the smallest reward net
    B, K, seed, off = 3, 17, 99, 40
    w = g.weights
    spec = MLPSpec(w.kernels, w.biases, "tanh", w.ln_gamma, w.ln_beta, model="reward")
    states = np.stack([orc.synthetic_state(g.norm, seed=11 + b) for b in range(B)])

    def mk(k):
        e = RolloutEngine(g.S, g.A, w.hidden, 2, "tanh", w.layer_norm, g.H, k, cost="reward", model="reward",
                          kernel="group4")
        e.set_weights(spec, g.norm, 1)
        e.set_discount(0.9)
        return e
    eng = mk(B * K)
    res = eng.get_actions(states, None, seed=seed, cand_offset=off, return_costs=True)
    eng.close()
    one = mk(K)
    for b in range(B):
        s = one.get_action(states[b], None, seed=seed, cand_offset=off + b * K, return_costs=True)
        assert np.array_equal(res.costs[b], s.costs)
        same_record(res, s, b)
        assert int(res.best_index[b]) - off - b * K == int(np.argmax(res.costs[b]))
    one.close()


# ------------------------------------------------------------------ 6. async form, timing
def test_batch_async_equals_sync():
    import torch
    from bc_mpc_amd import _lib
    r = ref("A", 1000)
    eng = r.engine("auto")
    want = eng.get_actions(r.states, None, seed=r.seed, cand_offset=1000, return_costs=True)
    dev = torch.device("cuda", 0)
    rec = ctypes.sizeof(_lib.Result)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d_states = torch.from_numpy(r.states.copy()).to(dev)
        d_costs = torch.full((r.B * r.K,), np.nan, dtype=torch.float64, device=dev)
        d_res = torch.zeros(r.B * rec, dtype=torch.uint8, device=dev)
        eng.rollout_batch_async(d_states.data_ptr(), r.B, None, r.seed, 1000, d_costs.data_ptr(), d_res.data_ptr(),
                                stream.cuda_stream)
    stream.synchronize()
    eng.check_status()
    raw = d_res.cpu().numpy().view(np.float64).reshape(r.B, rec // 8)
    assert np.array_equal(d_costs.cpu().numpy().reshape(r.B, r.K), want.costs)
    assert np.array_equal(raw[:, 0].copy().view(np.int64), want.best_index)
    assert np.array_equal(raw[:, 1], want.best_cost)
    assert np.array_equal(raw[:, 2:2 + A], want.first_action)
    assert not raw[:, 2 + A:].any()                      # the unused first_action slots are zeroed
    eng.close()


def test_batch_timing_reports_the_chain():
    r = ref("B", 0)
    eng = r.engine("auto")
    eng.set_timing(True)
    eng.get_actions(r.states, None, seed=r.seed)
    rollout_ms, argmin_ms = eng.last_kernel_ms()
    eng.close()
    assert 0.0 < rollout_ms < 1000.0 and 0.0 < argmin_ms < 1000.0


def test_batch_team_giveup_reruns_on_the_fallback(monkeypatch):
    """A team that gives up (forced with the library's test hook, as tests/test_gpu_team_progress.py does)
    makes the synchronous batched call rerun on the fallback engine: the oracle's answers."""
    r = ref("A", 0)
    eng = r.engine("team")
    monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
    res = eng.get_actions(r.states, None, seed=r.seed, return_costs=True)
    monkeypatch.delenv("BCMPC_TEAM_SPINS")
    assert eng.team_reruns == 1
    eng.close()
    for b in range(r.B):
        assert_costs_close(res.costs[b], r.costs[b], None, f"fallback/env{b}", env=r.env)
        assert int(res.best_index[b]) - b * r.K == int(r.argmin[b])


# ------------------------------------------------------------------ 7. controllers and errors
class _Box:
    low, high = LOW, HIGH
    shape = (A,)


class _Env:
    action_space = _Box()

    class observation_space:
        shape = (S,)


def test_controller_get_actions():
    from bc_mpc_amd import MPCcontroller, cheetah_cost_fn
    from oracle import mpc_oracle as orc
    r = ref("A", 0)
    ctrl = MPCcontroller(_Env(), orc.NumpyDynamics(r.w, r.norm), horizon=r.H, cost_fn=cheetah_cost_fn,
                         num_simulated_paths=r.K, rng="device", seed=3)
    got = ctrl.get_actions(r.states)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (r.B, A)
    seed = int(np.random.RandomState(3).randint(0, 2**62, dtype=np.int64))     # the one seed the call drew
    eng = r.engine("auto")
    want = eng.get_actions(r.states, None, seed=seed)
    eng.close()
    assert np.array_equal(got, want.first_action)
    assert np.array_equal(ctrl.last_index, want.best_index)
    ctrl._batch_engine.close()


def test_reward_controller_get_actions():
    from bc_mpc_amd import MPCcontrollerReward
    from oracle import mpc_oracle as orc
    g = RewardGolden("reward_tiny_g1")
    states = np.stack([orc.synthetic_state(g.norm, seed=11 + b) for b in range(3)])
    ctrl = MPCcontrollerReward(_Env(), g.dyn(), horizon=g.H, num_simulated_paths=17, gamma=0.9, rng="device", seed=8)
    got = ctrl.get_actions(states)
    assert got.dtype == np.float64 and got.shape == (3, g.A)
    seed = int(np.random.RandomState(8).randint(0, 2**62, dtype=np.int64))
    acts = orc.device_rng_actions(seed, 0, 3 * 17, g.H, LOW, HIGH)
    assert np.array_equal(got, acts[0, ctrl.last_index])
    assert all(0 <= int(i) - b * 17 < 17 for b, i in enumerate(ctrl.last_index))
    ctrl._batch_engine.close()


def test_batch_errors():
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import RolloutEngine
    r = ref("A", 0)
    eng = r.engine("auto")                               # 185 candidates
    with pytest.raises(ValueError, match="multiple"):
        eng.get_actions(r.states[:2])
    with pytest.raises(ValueError):
        eng.get_actions(r.states[0])                     # not [B, S]
    with pytest.raises(ValueError):
        eng.get_actions(r.states, np.zeros((r.H, r.K, A)))
    # the library's own check (the Python wrapper answers first)
    out = (_lib.Result * 2)()
    dp = ctypes.POINTER(ctypes.c_double)
    st = np.ascontiguousarray(r.states[:2])
    assert eng._lib.bcmpc_get_actions_batch(eng._h, st.ctypes.data_as(dp), 2, None, 0, 0, out, None) == _lib.ERR_ARG
    assert b"multiple" in eng._lib.bcmpc_last_error()
    assert eng._lib.bcmpc_get_actions_batch(eng._h, st.ctypes.data_as(dp), 0, None, 0, 0, out, None) == _lib.ERR_ARG
    eng.close()
    pol = RolloutEngine(S, A, 256, 2, "relu", False, 5, 64, policy_hidden=128, policy_layers=2, precision="fp32")
    with pytest.raises(ValueError, match="fused policy"):
        pol.get_actions(r.states[:4])
    pol.close()
    traj = RolloutEngine(S, A, 64, 2, "tanh", False, 5, 64, cost="none")
    with pytest.raises(ValueError, match="fused objective"):
        traj.get_actions(r.states[:4])
    traj.close()

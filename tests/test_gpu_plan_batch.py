"""Batched CEM and MPPI on the GPU: B environments x K candidates, one plan per environment, in one launch
chain (bcmpc_cem_get_actions_batch / bcmpc_mppi_get_actions_batch and their building blocks,
csrc/plan_batch.hip).

Contract (include/bcmpc.h): with off_b = cand_offset + b*K, environment b's per-iteration costs, elites,
refit / weighted mean, statistics and record are bit for bit those of the single-environment blocks
(cem_rollout_async, select_async, cem_refit_async, mppi_update_async) at off_b on a K-candidate engine of
the same kernel layout; B = 1 equals cem_get_action / mppi_get_action; environments are independent.

Tolerances are the suite's own: costs against the oracle by test_gpu_parity.assert_costs_close with
conftest.envelope; the MPPI update against test_gpu_mppi.mppi_ref within that file's derived bound
(16 K 2^-53 amax on mu', the same factor relative on weight_sum, twice on ess) with m = K.  Everything else
is bitwise.  S = 20, A = 6, bounds +-1; nets from oracle.synthetic_weights: 2x64 tanh and 2x128 relu + LN.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import RewardGolden, envelope
from test_gpu_mppi import STATS, _check, _engine as mppi_engine, _problem as mppi_problem, mppi_ref
from test_gpu_parity import assert_costs_close, team_ok

pytestmark = pytest.mark.gpu

S, A = 20, 6
LOW, HIGH = -np.ones(A), np.ones(A)
NETS = {"tanh64": (64, "tanh", False), "reluln128": (128, "relu", True)}
ELITE = np.dtype([("cost", "<f8"), ("index", "<i8")])
BIG = (1 << 32) + 12345


def _t():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(x):
    torch, dev = _t()
    return torch.from_numpy(np.array(x, order="C", copy=True)).to(dev)      # (a copy: x may be read-only)


def _stream():
    torch, dev = _t()
    return torch.cuda.current_stream(dev).cuda_stream


def _bytes(n):
    torch, dev = _t()
    return torch.zeros(n, dtype=torch.uint8, device=dev)


def _records(raw, n):
    """n bcmpc_result records -> (best_index [n], best_cost [n], first_action [n, A])."""
    from bc_mpc_amd import _lib
    rec = raw.cpu().numpy().view(np.float64).reshape(n, ctypes.sizeof(_lib.Result) // 8)
    return rec[:, 0].copy().view(np.int64), rec[:, 1].copy(), rec[:, 2:2 + A].copy()


class Net:
    """One net's weights, oracle dynamics and per-environment states (read-only, shared by the tests)."""

    def __init__(self, name):
        from oracle import mpc_oracle as orc
        self.hidden, self.act, self.ln = NETS[name]
        self.w = orc.synthetic_weights(S, A, self.hidden, 2, self.act, self.ln)
        self.norm = orc.synthetic_normalization()
        self.dyn = orc.NumpyDynamics(self.w, self.norm)
        self.states = np.stack([orc.synthetic_state(self.norm, seed=11 + b) for b in range(5)])
        self.states.setflags(write=False)

    def engine(self, kernel, K, H):
        from bc_mpc_amd.engine import MLPSpec, RolloutEngine
        w = self.w
        eng = RolloutEngine(S, A, w.hidden, 2, w.activation, w.layer_norm, H, K, device=0, kernel=kernel)
        if kernel != "auto":
            assert eng.info()["kernel"] == kernel
        eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta), self.norm, 1)
        return eng

    def score(self, state, acts):
        from oracle import mpc_oracle as orc
        c, states = orc.rollout(self.dyn, state, acts)
        return c, orc.near_threshold_mask(states)


@functools.lru_cache(maxsize=None)
def net(name) -> Net:
    return Net(name)


_BLOCK_ENGINES = {}


def block_engine(H, reward=False):
    """An engine for the building blocks that use only H, A, the bounds and the objective direction."""
    if (H, reward) not in _BLOCK_ENGINES:
        if reward:
            spec, norm, *_ = mppi_problem("reward")
            _BLOCK_ENGINES[(H, reward)] = mppi_engine(spec, norm, 64, H, "reward")
        else:
            _BLOCK_ENGINES[(H, reward)] = net("tanh64").engine("auto", 64, H)
    return _BLOCK_ENGINES[(H, reward)]


def plans(B, H, seed=0, clip_env=None):
    """Distinct per-environment plans [B, H, A]; clip_env: a plan whose samples clip at both bounds."""
    rs = np.random.RandomState(100 + seed)
    mu = rs.uniform(-0.6, 0.6, (B, H, A))
    sd = rs.uniform(0.1, 0.6, (B, H, A))
    if clip_env is not None:
        mu[clip_env], sd[clip_env] = 0.0, 4.0
    return mu, sd


# ------------------------------------------------------------------ 1. the sampling kernel
@pytest.mark.parametrize("it", [0, 2])
@pytest.mark.parametrize("off", [0, BIG])
@pytest.mark.parametrize("K,B,H", [(37, 5, 5), (1, 4, 1), (65, 3, 8)])
def test_sampler_is_bitwise_the_oracle_per_environment(K, B, H, off, it):
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    eng = block_engine(H)
    seed = 0xABCDEF + K
    mu, sd = plans(B, H, K, clip_env=1)
    d_mu, d_sd = _dev(mu), _dev(sd)
    d_act = torch.full((H, B * K, A), np.nan, dtype=torch.float64, device=dev)
    eng.plan_sample_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, d_act.data_ptr(), _stream())
    got = d_act.cpu().numpy()
    for b in range(B):
        want = orc.cem_actions(seed, it, off + b * K, K, H, mu[b], sd[b], LOW, HIGH)
        assert got[:, b * K:(b + 1) * K].tobytes() == want.tobytes(), f"environment {b}"
        if b == 1 and K * H * A >= 100:
            assert (want == 1.0).any() and (want == -1.0).any() and (np.abs(want) < 1.0).any()


# ------------------------------------------------------------------ 2. segmented select and refit
def _select_costs(K, rs):
    """[3, K]: ties and +-0; NaN / +-inf scattered among normals; all NaN."""
    c = np.empty((3, K))
    c[0] = rs.randint(-2, 3, K).astype(np.float64)
    c[0, rs.rand(K) < 0.3] *= -1.0                       # -0.0 among the zeros
    c[1] = 3.0 * rs.standard_normal(K)
    if K >= 8:
        pos = rs.choice(K, max(3, K // 7), replace=False)
        c[1, pos] = np.resize([np.nan, np.inf, -np.inf], pos.size)
    c[2] = np.nan
    return c


@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 1000])
def test_segmented_select_and_refit(K, maximize):
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    B, H, off, seed, it, alpha = 3, 3, 1000, 0x5E1EC7 + K, 1, 0.1
    eng = block_engine(H, reward=maximize)
    st = _stream()
    rs = np.random.RandomState(K)
    costs = _select_costs(K, rs)
    if maximize:
        costs = -costs                                   # the same scores on a reward engine
    mu, sd = plans(B, H, K)
    d_costs = _dev(costs.reshape(-1))
    d_act = torch.empty((H, B * K, A), dtype=torch.float64, device=dev)
    d_mu0, d_sd0 = _dev(mu), _dev(sd)                    # (held: the launch is asynchronous)
    eng.plan_sample_async(d_mu0.data_ptr(), d_sd0.data_ptr(), B, K, seed, it, off, d_act.data_ptr(), st)
    for E in sorted({1, max(1, K // 10), K, K + 5}):
        d_el = _bytes(B * E * ELITE.itemsize)
        d_el.fill_(0xEE)
        d_cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
        eng.select_batch_async(d_costs.data_ptr(), B, K, off, E, d_el.data_ptr(), d_cnt.data_ptr(), st)
        el = d_el.cpu().numpy().view(ELITE).reshape(B, E)
        cnt = d_cnt.cpu().numpy()
        want_el = []
        for b in range(B):
            idx = off + b * K + np.arange(K)
            w = orc.cem_select(costs[b], idx, E, maximize)
            want_el.append(w)
            n = min(E, K)
            assert cnt[b] == n == w.size
            assert np.array_equal(el[b, :n]["index"], w), f"K={K} E={E} env {b}"
            assert el[b, :n]["cost"].tobytes() == costs[b, w - off - b * K].tobytes()
            assert (el[b, n:]["index"] == -1).all() and np.isnan(el[b, n:]["cost"]).all()
        # the single-environment blocks on each slice
        one_el, one_cnt = _bytes(E * ELITE.itemsize), torch.zeros(1, dtype=torch.int32, device=dev)
        single = []
        for b in range(B):
            d_m1, d_s1 = _dev(mu[b]), _dev(sd[b])
            eng.select_async(None, d_costs.data_ptr() + 8 * b * K, K, off + b * K, E, one_el.data_ptr(),
                             one_cnt.data_ptr(), st)
            assert one_el.cpu().numpy().tobytes() == el[b].tobytes() and int(one_cnt.cpu()[0]) == cnt[b]
            eng.cem_refit_async(one_el.data_ptr(), one_cnt.data_ptr(), seed, it, alpha, d_m1.data_ptr(),
                                d_s1.data_ptr(), st)
            single.append((d_m1.cpu().numpy(), d_s1.cpu().numpy()))
        for stored in (True, False):
            d_mu, d_sd = _dev(mu), _dev(sd)
            eng.cem_refit_batch_async(d_el.data_ptr(), d_cnt.data_ptr(), B, E, seed, it, alpha, d_mu.data_ptr(),
                                      d_sd.data_ptr(), d_act.data_ptr() if stored else None, K, off, st)
            mu1, sd1 = d_mu.cpu().numpy(), d_sd.cpu().numpy()
            for b in range(B):
                rm, rsd = orc.cem_refit(want_el[b], seed, it, mu[b], sd[b], LOW, HIGH, alpha)
                label = f"K={K} E={E} env {b} stored={stored}"
                assert mu1[b].tobytes() == rm.tobytes() and sd1[b].tobytes() == rsd.tobytes(), label
                assert mu1[b].tobytes() == single[b][0].tobytes() and sd1[b].tobytes() == single[b][1].tobytes(), label


# ------------------------------------------------------------------ 3. segmented MPPI update
def _mppi_vectors(K, rs):
    """test_gpu_mppi.py's cost vectors for m = K: (name, costs); too-small K falls back to the normal one."""
    normal = 3.0 * rs.standard_normal(K)
    spread = rs.uniform(1.0, 1e6, K)
    imin = int(rs.randint(K))
    spread[imin] = 0.0
    tied = spread.copy()
    if K >= 2:
        tied[(imin + 1 + int(rs.randint(K - 1))) % K] = 0.0
    bad = normal.copy()
    if K >= 8:
        pos = np.unique(np.concatenate([[0, K - 1], rs.choice(K, max(3, K // 7), replace=False)]))
        bad[pos] = np.resize([np.nan, np.inf, -np.inf], pos.size)
        bad[0], bad[K - 1] = -np.inf, np.nan
    return [("normal", normal), ("equal", np.full(K, 3.25)), ("spread", spread), ("tied", tied),
            ("nonfinite", bad), ("all-nonfinite", np.resize([np.inf, np.nan, -np.inf], K))]


@pytest.mark.parametrize("B,K", [(3, 1), (3, 63), (3, 64), (3, 65), (3, 1000), (3, 4097), (2, 16384), (2, 16385)])
def test_segmented_mppi_update(B, K):
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    H, off, seed, it = 2, 777, 0x3B9A + K, 2
    eng = block_engine(H)
    st = _stream()
    rs = np.random.RandomState(K)
    vecs = _mppi_vectors(K, rs)
    mu, sd = plans(B, H, K)
    acts = [orc.cem_actions(seed, it, off + b * K, K, H, mu[b], sd[b], LOW, HIGH) for b in range(B)]
    d_act = torch.empty((H, B * K, A), dtype=torch.float64, device=dev)
    d_sd = _dev(sd)
    d_mu0 = _dev(mu)                                     # (held: the launch is asynchronous)
    eng.plan_sample_async(d_mu0.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, d_act.data_ptr(), st)
    d_costs = torch.empty(B * K, dtype=torch.float64, device=dev)
    d_stats, one_stats = _bytes(B * STATS.itemsize), _bytes(STATS.itemsize)
    for r, lam in enumerate((5.0, 1e-3, 5.0, 1e-3, 5.0, 1e-3, 1e-3, 5.0, 1e-3, 5.0, 1e-3, 5.0)):
        kinds = [(r + b) % len(vecs) for b in range(B)]     # different vectors in the same call, every vector
        costs = np.stack([vecs[k][1] for k in kinds])       # under both temperatures in every environment
        d_costs.copy_(torch.from_numpy(costs.reshape(-1)))
        d_mu = _dev(mu)
        d_stats.fill_(0xEE)
        stored = (r // 2) % 2 == 0                          # both forms of the update under both temperatures
        eng.mppi_update_batch_async(d_costs.data_ptr(), B, K, off, seed, it, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                    d_stats.data_ptr(), d_act.data_ptr() if stored else None, st)
        mu1, stats = d_mu.cpu().numpy(), d_stats.cpu().numpy().view(STATS)
        assert d_sd.cpu().numpy().tobytes() == sd.tobytes(), "sigma was modified"
        for b in range(B):
            label = f"B={B} K={K} round {r} env {b} {vecs[kinds[b]][0]} lam={lam}"
            d_m1 = _dev(mu[b])
            eng.mppi_update_async(d_costs.data_ptr() + 8 * b * K, K, off + b * K, seed, it, lam, d_m1.data_ptr(),
                                  d_sd.data_ptr() + 8 * b * H * A, one_stats.data_ptr(), st)
            assert mu1[b].tobytes() == d_m1.cpu().numpy().tobytes(), f"{label}: mu' differs from the single update"
            assert stats[b].tobytes() == one_stats.cpu().numpy().tobytes(), f"{label}: statistics differ"
            ref = mppi_ref(costs[b], acts[b], mu[b], lam)
            if ref[4] == 0:
                assert mu1[b].tobytes() == mu[b].tobytes(), f"{label}: mu was modified"
                s = stats[b]
                assert s["n_valid"] == 0 and s["weight_sum"] == 0.0 and s["ess"] == 0.0 and np.isnan(s["min_cost"])
            else:
                _check(label, (mu1[b], stats[b]), ref, K)


# ------------------------------------------------------------------ 4. the full step against the composition
CASE4 = dict(net="tanh64", H=5, K=37, B=5, iters=2, E=4, alpha=0.1, lam=1.0, seed=0xC0FFEE, off=1000)


def _case4_inputs():
    c = CASE4
    n = net(c["net"])
    mu, sd = plans(c["B"], c["H"], 4)
    return n, n.states[:c["B"]], mu, sd


def _skip_team(kernel, n, K):
    if kernel == "team" and not team_ok(n.hidden, n.ln, 2, K, S, A):
        pytest.skip("team: the 2-layer delta net at small K (grid resident)")


def _single_chain(one, planner, state, mu_b, sd_b, off_b, k_global):
    """Environment b's answer composed from the single-environment async blocks on the K-candidate engine."""
    torch, dev = _t()
    from bc_mpc_amd import _lib
    c = CASE4
    K, E = c["K"], c["E"]
    st = _stream()
    d_state, d_mu, d_sd = _dev(state), _dev(mu_b), _dev(sd_b)
    d_costs = torch.empty(K, dtype=torch.float64, device=dev)
    d_res = _bytes(ctypes.sizeof(_lib.Result))
    d_el, d_cnt = _bytes(E * ELITE.itemsize), torch.zeros(1, dtype=torch.int32, device=dev)
    d_stats = _bytes(STATS.itemsize)
    costs = []
    for it in range(c["iters"]):
        one.cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sd.data_ptr(), c["seed"], it, off_b, k_global,
                              d_costs.data_ptr(), d_res.data_ptr(), it > 0, st)
        costs.append(d_costs.cpu().numpy())
        if planner == "cem":
            one.select_async(None, d_costs.data_ptr(), K, off_b, E, d_el.data_ptr(), d_cnt.data_ptr(), st)
            one.cem_refit_async(d_el.data_ptr(), d_cnt.data_ptr(), c["seed"], it, c["alpha"], d_mu.data_ptr(),
                                d_sd.data_ptr(), st)
        else:
            one.mppi_update_async(d_costs.data_ptr(), K, off_b, c["seed"], it, c["lam"], d_mu.data_ptr(),
                                  d_sd.data_ptr(), d_stats.data_ptr(), st)
    torch.cuda.synchronize()
    one.check_status()
    pos, cost, first = _records(d_res, 1)
    it, g = divmod(int(pos[0]), k_global)                     # position = it * k_global + off_b + j
    return dict(costs=np.stack(costs), mu=d_mu.cpu().numpy(), sd=d_sd.cpu().numpy(),
                stats=d_stats.cpu().numpy().view(STATS)[0].copy(), index=it * K + g - off_b, cost=cost[0],
                first=first[0])


def _run_batch(eng, planner, states, mu, sd, **kw):
    c = CASE4
    off = kw.pop("off", c["off"])
    if planner == "cem":
        res, mu1, sd1 = eng.cem_get_actions(states, mu, sd, c["iters"], c["E"], c["alpha"], c["seed"], off, True)
        return res, mu1, sd1, None
    res, mu1, stats = eng.mppi_get_actions(states, mu, sd, c["iters"], c["lam"], c["seed"], off, True)
    return res, mu1, sd, stats


@pytest.mark.parametrize("planner", ["cem", "mppi"])
@pytest.mark.parametrize("kernel", ["group4", "split2", "team"])
def test_full_step_equals_the_single_environment_composition(kernel, planner):
    c = CASE4
    n, states, mu, sd = _case4_inputs()
    B, K, H = c["B"], c["K"], c["H"]
    _skip_team(kernel, n, B * K)
    eng = n.engine(kernel, B * K, H)
    res, mu1, sd1, stats = _run_batch(eng, planner, states, mu, sd)
    again = _run_batch(eng, planner, states, mu, sd)
    eng.close()
    assert res.costs.shape == (c["iters"], B, K) and mu1.shape == (B, H, A)
    # determinism: two calls, equal bits
    assert again[0].costs.tobytes() == res.costs.tobytes() and again[1].tobytes() == mu1.tobytes()
    assert again[2].tobytes() == sd1.tobytes() and again[0].best_index.tobytes() == res.best_index.tobytes()
    assert again[0].first_action.tobytes() == res.first_action.tobytes()
    one = n.engine(kernel, K, H)
    for b in range(B):
        s = _single_chain(one, planner, states[b], mu[b], sd[b], c["off"] + b * K, c["off"] + B * K)
        assert res.costs[:, b].tobytes() == s["costs"].tobytes(), f"env {b}: costs differ bitwise"
        assert mu1[b].tobytes() == s["mu"].tobytes(), f"env {b}: mu'"
        assert sd1[b].tobytes() == s["sd"].tobytes(), f"env {b}: sigma'"
        if planner == "mppi":
            assert stats[b].tobytes() == s["stats"].tobytes(), f"env {b}: statistics"
        assert int(res.best_index[b]) == s["index"], f"env {b}: position"
        assert np.float64(res.best_cost[b]).tobytes() == np.float64(s["cost"]).tobytes()
        assert res.first_action[b].tobytes() == s["first"].tobytes()
    # B = 1, cand_offset = 0 on the K-candidate engine: the single synchronous call
    b1 = _run_batch(one, planner, states[2:3], mu[2:3], sd[2:3], off=0)
    if planner == "cem":
        r, m1, s1 = one.cem_get_action(states[2], mu[2], sd[2], c["iters"], c["E"], c["alpha"], c["seed"])
        assert b1[2][0].tobytes() == s1.tobytes()
    else:
        r, m1, st1 = one.mppi_get_action(states[2], mu[2], sd[2], c["iters"], c["lam"], c["seed"])
        got = b1[3][0]
        assert (got["weight_sum"], got["ess"], got["min_cost"], got["n_valid"]) == (
            st1.weight_sum, st1.ess, st1.min_cost, st1.n_valid)
    one.close()
    assert b1[1][0].tobytes() == m1.tobytes()
    assert int(b1[0].best_index[0]) == r.best_index and b1[0].best_cost[0] == r.best_cost
    assert b1[0].first_action[0].tobytes() == r.first_action.tobytes()


# ------------------------------------------------------------------ 5. the full step against the oracle
def _check_records(res, costs, hist, seed, off, K, maximize=False):
    """best_index / best_cost / first_action of every environment against its own returned costs."""
    from oracle import mpc_oracle as orc
    for b in range(costs.shape[1]):
        flat = costs[:, b].reshape(-1)                    # iteration-major concatenation
        pos = int(np.argmax(flat) if maximize else np.argmin(flat))
        assert int(res.best_index[b]) == pos, f"env {b}"
        assert res.best_cost[b] == flat[pos]
        it, j = divmod(pos, K)
        m, s = hist[it]
        want = orc.cem_actions(seed, it, off + b * K + j, 1, 1, m[b], s[b], LOW, HIGH)[0, 0]
        assert res.first_action[b].tobytes() == want.tobytes(), f"env {b}: first action"


def _oracle_step(n_score, eng, planner, states, mu, sd, H, K, seed, off, env, label, maximize=False):
    from oracle import mpc_oracle as orc
    B = states.shape[0]
    iters, E, alpha, lam = (2, 4, 0.1, None) if planner == "cem" else (1, None, None, 1.0)
    if planner == "cem":
        res, mu1, sd1 = eng.cem_get_actions(states, mu, sd, iters, E, alpha, seed, off, True)
    else:
        res, mu1, stats = eng.mppi_get_actions(states, mu, sd, iters, lam, seed, off, True)
    m, s = mu.copy(), sd.copy()
    hist = []
    for it in range(iters):
        hist.append((m.copy(), s.copy()))
        for b in range(B):
            acts = orc.cem_actions(seed, it, off + b * K, K, H, m[b], s[b], LOW, HIGH)
            want, near = n_score(states[b], acts)
            assert_costs_close(res.costs[it, b], want, near, f"{label}/it{it}/env{b}", env=env)
            if planner == "cem":
                # the GPU's own costs drive the reference's selection: a cost within tolerance cannot flip an elite
                el = orc.cem_select(res.costs[it, b], off + b * K + np.arange(K), E, maximize)
                m[b], s[b] = orc.cem_refit(el, seed, it, m[b], s[b], LOW, HIGH, alpha)
            else:
                ref = mppi_ref(res.costs[it, b], acts, m[b], lam, maximize)
                _check(f"{label}/env{b}", (mu1[b], stats[b]), ref, K)
    if planner == "cem":
        assert mu1.tobytes() == m.tobytes() and sd1.tobytes() == s.tobytes(), f"{label}: final plan"
    _check_records(res, res.costs, hist, seed, off, K, maximize)


@pytest.mark.parametrize("planner", ["cem", "mppi"])
@pytest.mark.parametrize("kernel", ["auto", "solo", "group4", "split2", "team"])
@pytest.mark.parametrize("name", list(NETS))
def test_full_step_matches_the_oracle(name, kernel, planner):
    n = net(name)
    B, K, H = (5, 37, 5) if name == "tanh64" else (3, 17, 3)
    _skip_team(kernel, n, B * K)
    mu, sd = plans(B, H, 5, clip_env=1)
    eng = n.engine(kernel, B * K, H)
    _oracle_step(n.score, eng, planner, n.states[:B], mu, sd, H, K, 4242, 1000, envelope(n.ln, 2, n.hidden, H),
                 f"{name}/{kernel}/{planner}")
    eng.close()


@pytest.mark.parametrize("planner", ["cem", "mppi"])
def test_full_step_matches_the_oracle_learned_reward(planner):
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc
    g = RewardGolden("reward_tiny_g1")                  # hidden 64, no LayerNorm: the smallest reward net
    B, K = 3, 17
    w = g.weights
    eng = RolloutEngine(g.S, g.A, w.hidden, 2, "tanh", w.layer_norm, g.H, B * K, cost="reward", model="reward",
                        kernel="group4")
    eng.set_weights(MLPSpec(w.kernels, w.biases, "tanh", w.ln_gamma, w.ln_beta, model="reward"), g.norm, 1)
    eng.set_discount(0.9)
    dyn = g.dyn()
    states = np.stack([orc.synthetic_state(g.norm, seed=11 + b) for b in range(B)])
    mu, sd = plans(B, g.H, 6)
    score = lambda s, a: (orc.reward_rollout(dyn, s, a, 0.9)[0], None)   # noqa: E731
    _oracle_step(score, eng, planner, states, mu, sd, g.H, K, 99, 40, envelope(w.layer_norm, 2, w.hidden, g.H),
                 f"reward/{planner}", maximize=True)
    eng.close()


def test_team_giveup_reruns_the_whole_call_from_the_original_plans(monkeypatch):
    """A team that gives up (forced with the library's test hook, as tests/test_gpu_batch.py does) makes the
    synchronous call rerun on the fallback engine.  The final CEM plan is bitwise the oracle's refit chain from
    the ORIGINAL mu / sigma on the returned costs, so nothing of the abandoned attempt leaks into the rerun."""
    n = net("tanh64")
    B, K, H = 5, 37, 5
    assert team_ok(n.hidden, n.ln, 2, B * K, S, A)
    mu, sd = plans(B, H, 5, clip_env=1)
    eng = n.engine("team", B * K, H)
    monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
    for i, planner in enumerate(("cem", "mppi")):
        _oracle_step(n.score, eng, planner, n.states[:B], mu, sd, H, K, 4242, 1000, envelope(n.ln, 2, n.hidden, H),
                     f"fallback/{planner}")
        assert eng.team_reruns == i + 1
    monkeypatch.delenv("BCMPC_TEAM_SPINS")
    eng.close()


# ------------------------------------------------------------------ 6. independence and NaN
@pytest.mark.parametrize("planner", ["cem", "mppi"])
def test_a_nan_environment_changes_only_itself(planner):
    from oracle import mpc_oracle as orc
    c = CASE4
    n, states, mu, sd = _case4_inputs()
    B, K, H = c["B"], c["K"], c["H"]
    eng = n.engine("group4", B * K, H)
    clean = _run_batch(eng, planner, states, mu, sd)
    bad_states = states.copy()
    bad_states[2] = np.nan
    res, mu1, sd1, stats = _run_batch(eng, planner, bad_states, mu, sd)
    again = _run_batch(eng, planner, bad_states, mu, sd)
    eng.close()
    assert again[0].costs.tobytes() == res.costs.tobytes() and again[1].tobytes() == mu1.tobytes()
    assert again[2].tobytes() == sd1.tobytes() and again[0].first_action.tobytes() == res.first_action.tobytes()
    for b in (0, 1, 3, 4):
        assert res.costs[:, b].tobytes() == clean[0].costs[:, b].tobytes(), f"env {b}: costs changed"
        assert mu1[b].tobytes() == clean[1][b].tobytes() and sd1[b].tobytes() == clean[2][b].tobytes()
        assert res.best_index[b] == clean[0].best_index[b] and res.best_cost[b] == clean[0].best_cost[b]
        assert res.first_action[b].tobytes() == clean[0].first_action[b].tobytes()
        if planner == "mppi":
            assert stats[b].tobytes() == clean[3][b].tobytes()
    assert np.isnan(res.costs[:, 2]).all()
    # the record: NaN at the first NaN's position (iteration 0, candidate 0) with that sample's action
    assert int(res.best_index[2]) == 0 and np.isnan(res.best_cost[2])
    want = orc.cem_actions(c["seed"], 0, c["off"] + 2 * K, 1, 1, mu[2], sd[2], LOW, HIGH)[0, 0]
    assert res.first_action[2].tobytes() == want.tobytes()
    if planner == "mppi":
        assert stats[2]["n_valid"] == 0 and stats[2]["weight_sum"] == 0.0 and np.isnan(stats[2]["min_cost"])
        assert mu1[2].tobytes() == mu[2].tobytes(), "mu of the all-NaN environment was modified"
    else:
        # NaN last, ties to the lower index: the first E candidates are the elites of both iterations
        m, s = mu[2], sd[2]
        for it in range(c["iters"]):
            m, s = orc.cem_refit(c["off"] + 2 * K + np.arange(c["E"]), c["seed"], it, m, s, LOW, HIGH, c["alpha"])
        assert mu1[2].tobytes() == m.tobytes() and sd1[2].tobytes() == s.tobytes()


# ------------------------------------------------------------------ 7. controllers and errors
class _Box:
    low, high = LOW, HIGH
    shape = (A,)


class _Env:
    action_space = _Box()

    class observation_space:
        shape = (S,)


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_controller_get_actions_warm_start_and_reset(kind):
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    n = net("tanh64")
    B, K, H = 3, 37, 5
    states = n.states[:B]
    if kind == "cem":
        ctrl = CEMcontroller(_Env(), n.dyn, horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, iterations=2,
                             n_elite=4, seed=9)
    else:
        ctrl = MPPIcontroller(_Env(), n.dyn, horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, seed=9)
    seeds = [int(x) for x in np.random.RandomState(9).randint(0, 2**62, size=3, dtype=np.int64)]
    a1 = ctrl.get_actions(states)
    assert a1.shape == (B, A) and a1.dtype == np.float64 and (np.abs(a1) <= 1.0).all()
    plan1 = ctrl.last_mu.copy()
    assert plan1.shape == (B, H, A) and ctrl.last_cost.shape == (B,) and ctrl.last_position.shape == (B,)
    mu_w, sd_w = ctrl.batch_initial_distribution(B)         # the second call's sampling means
    for b in range(B):
        assert np.array_equal(mu_w[b, :-1], plan1[b, 1:]) and (mu_w[b, -1] == 0).all()
    a2 = ctrl.get_actions(states)
    assert (np.abs(a2) <= 1.0).all()
    eng = ctrl._batch_engine
    assert eng.num_paths == B * K
    if kind == "cem":
        res, mu2, sd2 = eng.cem_get_actions(states, mu_w, sd_w, 2, 4, ctrl.alpha, seeds[1])
        assert np.array_equal(a2, res.first_action) and np.array_equal(ctrl.last_sigma, sd2)
    else:
        res, mu2, stats = eng.mppi_get_actions(states, mu_w, sd_w, 1, ctrl.temperature, seeds[1])
        assert np.array_equal(a2, mu2[:, 0]) and np.array_equal(ctrl.last_ess, stats["ess"])
        assert ((1.0 <= ctrl.last_ess) & (ctrl.last_ess <= K)).all()
    assert np.array_equal(ctrl.last_mu, mu2) and np.array_equal(ctrl.last_position, res.best_index)
    ctrl.reset([1])
    mu_r, _ = ctrl.batch_initial_distribution(B)
    assert (mu_r[1] == 0).all()                             # re-centred
    for b in (0, 2):
        assert np.array_equal(mu_r[b, :-1], mu2[b, 1:])
    a3 = ctrl.get_actions(states)
    assert (np.abs(a3) <= 1.0).all()
    eng.close()


def test_errors_on_a_live_engine():
    from bc_mpc_amd.engine import RolloutEngine
    n = net("tanh64")
    B, K, H = 5, 37, 5
    eng = n.engine("auto", B * K, H)                      # 185 candidates
    mu, sd = plans(B, H)
    with pytest.raises(ValueError, match="multiple"):
        eng.cem_get_actions(n.states[:2], mu[:2], sd[:2], 1, 4, 0.1, 1)
    with pytest.raises(ValueError, match="multiple"):
        eng.mppi_get_actions(n.states[:2], mu[:2], sd[:2], 1, 1.0, 1)
    with pytest.raises(ValueError):
        eng.cem_get_actions(n.states[:B], mu[:2], sd[:2], 1, 4, 0.1, 1)       # plans of another B
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda"):
            eng.mppi_get_actions(n.states[:B], mu, sd, 1, lam, 1)
    with pytest.raises(ValueError, match="iterations"):
        eng.cem_get_actions(n.states[:B], mu, sd, 0, 4, 0.1, 1)
    with pytest.raises(ValueError, match="n_elite"):
        eng.cem_get_actions(n.states[:B], mu, sd, 1, 0, 0.1, 1)
    res, mu1, _ = eng.cem_get_actions(n.states[:B], mu, sd, 1, 4, 0.1, 1)      # the engine still works
    assert mu1.shape == (B, H, A) and ((0 <= res.best_index) & (res.best_index < K)).all()
    eng.close()
    pol = RolloutEngine(S, A, 256, 2, "relu", False, H, 64, policy_hidden=128, policy_layers=2, precision="fp32")
    with pytest.raises(ValueError, match=r"status 2\].*fused policy"):
        pol.cem_get_actions(n.states[:4], mu[:4], sd[:4], 1, 4, 0.1, 1)
    with pytest.raises(ValueError, match=r"status 2\].*fused policy"):
        pol.mppi_get_actions(n.states[:4], mu[:4], sd[:4], 1, 1.0, 1)
    pol.close()
    traj = RolloutEngine(S, A, 64, 2, "tanh", False, H, 64, cost="none")
    with pytest.raises(ValueError, match=r"status 1\].*fused objective"):
        traj.cem_get_actions(n.states[:4], mu[:4], sd[:4], 1, 4, 0.1, 1)
    traj.close()

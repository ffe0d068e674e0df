"""MPPI's control-cost term and weighted sigma update on the GPU (csrc/mppi_ext.hip, the _x entry points).

The definition is bc_mpc_amd/mppi_update.py.  The control-cost kernel, the smoothing step and everything between
two device computations that must agree are compared BIT FOR BIT (a NaN as a NaN: the definition says a NaN cost
stays NaN and gives its payload no meaning).  One tolerance, on the weighted variance, derived here and not fitted.

The sigma block's bound.  With alpha = 0 and no clamp the kernel returns sigma' = sqrt(V~ / W~), V~ = sum_k w~_k d_k^2
and W~ = sum_k w~_k in f64; the test compares sigma'^2 with ref = fsum(w d^2) / fsum(w), w from np.exp, d = a - mu'
with a and mu' inside the action box, so |d| <= D = max_j(high_j - low_j).  eps = 2^-53.
  * weights: |w~ - w| <= 3 eps, the bound tests/test_gpu_mppi.py derives; 0 <= w, w~ <= 1 and the minimum's weight
    is exactly 1 on both sides, so W, W~ >= 1;
  * a term w~ d^2 takes a difference, a square and a product: (1 + e)^4, 4 eps relative; with the weight's error
    |t~ - t| <= 3 eps D^2 + 4 eps w~ D^2.  Over K terms: 3 K eps D^2 + 4 eps W~ D^2;
  * a K-term sum of non-negative terms in any order adds at most K eps relative: K eps W~ D^2.  Divided by
    W~ >= 1 the numerator contributes (3 K + 4 + K) eps D^2;
  * W~ carries 3 K eps (weights) + K eps W~ (sum) <= 4 K eps W~, and V / W <= D^2: 4 K eps D^2;
  * the division, the square root and squaring it back: 4 eps D^2; the reference's own three roundings per term,
    its division and np.exp's ulp: below 7 eps D^2.
Sum: (8 K + 15) eps D^2, which is <= 16 K eps D^2 from K = 2 on; at K = 1 both weights are exactly 1, W = 1, and
what is left (3 + 3 + 3 roundings) is 9 eps D^2.  So |sigma'^2 - ref| <= 16 K 2^-53 D^2 for every K >= 1: the
factor 2 over 8 K is the room for the constant terms and everything of second order.  Each case prints its worst
ratio to that bound.

Engines: the 2x128 tanh net of tests/test_gpu_mppi.py (S = 20, A = 6, bounds +-1; its reward twin for the sign),
and one engine with A = 1 and one with A = 16 from tests/size_cases.py's helpers (S = 16, bounds that differ per
dimension, cost="none": the blocks read H, A, the bounds and the objective's direction only).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

import size_cases as sc
from test_gpu_mppi import STATS, _engine, _problem, _update_engine

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SIZES_A = [6, 1, 16]
CONTROL_K = [1, 2, 63, 64, 65, 1000, 4097]
SIGMA_K = CONTROL_K + [16384, 16385]            # both workgroup sizes of the stage-1 kernels (kMppiSmall)
PAD = 8                                         # sentinel doubles behind every output


def _t():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(x):
    torch, dev = _t()
    return torch.from_numpy(np.array(x, dtype=np.float64, order="C", copy=True)).to(dev)


def _stream():
    torch, dev = _t()
    return torch.cuda.current_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def block_engine(A, H, reward=False):
    """An engine whose H, A, bounds and objective direction the blocks read."""
    if A == 6:
        return _update_engine("reward" if reward else "delta", H)
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    assert not reward
    w = sc.weights(16, A, "2x64tanh")
    eng = RolloutEngine(16, A, 64, 2, "tanh", False, H, 64, device=0, cost="none")
    eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation), sc.normalization(16, A), 1)
    eng.set_action_bounds(*sc.bounds(A))
    return eng


def box(A):
    return (-np.ones(6), np.ones(6)) if A == 6 else sc.bounds(A)


def _inputs(A, K, H, B, seed):
    """Plans inside the box and a self-made clipped action array [H, B*K, A]."""
    low, high = box(A)
    rs = np.random.RandomState(seed)
    mu = low + (high - low) * rs.uniform(0.2, 0.8, (B, H, A))
    sd = (high - low) * rs.uniform(0.05, 0.5, (B, H, A))
    acts = np.empty((H, B * K, A))
    for b in range(B):
        acts[:, b * K:(b + 1) * K] = np.clip(mu[b][:, None, :] + sd[b][:, None, :] * rs.standard_normal((H, K, A)),
                                            low, high)
    return rs, mu, sd, acts


def _same_bits(got, want, label):
    """Byte equality, a NaN compared as a NaN."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{label}: NaN positions differ"
    ok = ~np.isnan(want)
    assert got[ok].tobytes() == want[ok].tobytes(), f"{label}: {int((got[ok] != want[ok]).sum())} entries differ"


# ------------------------------------------------------------------ 1. the control-cost block
@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("K", CONTROL_K)
@pytest.mark.parametrize("A", SIZES_A)
def test_control_cost_is_bitwise_the_definition(A, K, H):
    from bc_mpc_amd.mppi_update import augmented, control_cost
    torch, dev = _t()
    st = _stream()
    for B in ((1, 3) if K <= 1000 else (1,)):
        rs, mu, sd, acts = _inputs(A, K, H, B, 1000 * K + 10 * H + A + B)
        if A > 1:
            sd[:, :, A - 1] = 0.0                        # a sigma == 0 column: it does not count, whatever the actions hold
        elif H > 1:
            sd[:, 0, 0] = 0.0
        if H * A > 1:
            mu[0, 0, 0] = 0.0                            # (0 / sigma^2, and 0 / 0 under the zero sigma when A = 1)
        costs = 3.0 * rs.standard_normal(B * K)
        if K >= 8:                                       # NaN, +inf and -inf at scattered positions, 0 and K - 1 included
            pos = np.unique(np.concatenate([[0, K - 1], rs.choice(K, max(3, K // 7), replace=False)]))
            costs[pos] = np.resize([np.nan, np.inf, -np.inf], pos.size)
        d_act, d_mu, d_sd, d_costs = _dev(acts), _dev(mu), _dev(sd), _dev(costs)
        q = [control_cost(acts[:, b * K:(b + 1) * K], mu[b], sd[b]) for b in range(B)]
        for qb in q:
            assert np.isfinite(qb).all() and (K < 8 or np.ptp(qb) > 0.0)
        inf = np.isinf(costs)
        engines = [(block_engine(A, H), False)] + ([(block_engine(A, H, True), True)] if A == 6 else [])
        for eng, maximize in engines:
            for weight in (0.7, 3.0):
                want = np.concatenate([augmented(costs[b * K:(b + 1) * K], q[b], weight, maximize) for b in range(B)])
                d_out = torch.full((B * K + PAD,), -7.5, dtype=torch.float64, device=dev)
                eng.mppi_control_cost_async(d_costs.data_ptr(), d_act.data_ptr(), B, K, d_mu.data_ptr(),
                                            d_sd.data_ptr(), weight, d_out.data_ptr(), st)
                got = d_out.cpu().numpy()
                assert (got[B * K:] == -7.5).all(), "written past the scores"
                _same_bits(got[:B * K], want, f"A={A} K={K} H={H} B={B} w={weight} max={maximize}")
                assert np.array_equal(got[:B * K][inf], costs[inf])      # an infinite cost stays what it is
                # in place: the scores may be the cost buffer itself
                d_same = _dev(costs)
                eng.mppi_control_cost_async(d_same.data_ptr(), d_act.data_ptr(), B, K, d_mu.data_ptr(),
                                            d_sd.data_ptr(), weight, d_same.data_ptr(), st)
                _same_bits(d_same.cpu().numpy(), want, "in place")


# ------------------------------------------------------------------ 3. the sigma block
def _sigma_ref_sq(scores, acts, mu_new, lam, maximize=False):
    """The weighted variance [H, A] of one environment, restated: weights from np.exp, sums by math.fsum."""
    from bc_mpc_amd.mppi_update import softmin_weights
    w = softmin_weights(scores, lam, maximize)
    W = math.fsum(w)
    H, _, A = acts.shape
    out = np.empty((H, A))
    for h in range(H):
        for j in range(A):
            d = acts[h, :, j] - mu_new[h, j]
            out[h, j] = math.fsum(w * (d * d)) / W
    return out


class _SigmaDev:
    def __init__(self, B, K, H, A, acts):
        torch, dev = _t()
        self.B, self.K, self.H, self.A = B, K, H, A
        self.scores = torch.empty(B * K, dtype=torch.float64, device=dev)
        self.mu_new = torch.empty((B, H, A), dtype=torch.float64, device=dev)
        self.sigma = torch.empty(B * H * A + PAD, dtype=torch.float64, device=dev)
        self.acts = _dev(acts)
        self.st = _stream()

    def run(self, eng, scores, mu_new, sigma, lam, alpha=0.0, min_std=0.0, max_std=None):
        torch, _ = _t()
        n = self.B * self.H * self.A
        self.scores.copy_(torch.from_numpy(np.ascontiguousarray(scores)))
        self.mu_new.copy_(torch.from_numpy(np.ascontiguousarray(mu_new)))
        self.sigma.fill_(-7.5)
        self.sigma[:n].copy_(torch.from_numpy(np.ascontiguousarray(sigma).reshape(-1)))
        eng.mppi_sigma_update_async(self.scores.data_ptr(), self.acts.data_ptr(), self.B, self.K, lam,
                                    self.mu_new.data_ptr(), self.sigma.data_ptr(), alpha, min_std, max_std, self.st)
        got = self.sigma.cpu().numpy()
        assert (got[n:] == -7.5).all(), "written past sigma"
        assert self.mu_new.cpu().numpy().tobytes() == np.ascontiguousarray(mu_new).tobytes(), "mu' was modified"
        return got[:n].reshape(self.B, self.H, self.A)


@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("K", SIGMA_K)
@pytest.mark.parametrize("A", SIZES_A)
def test_sigma_update_within_the_derived_bound_and_its_exact_cases(A, K, H):
    low, high = box(A)
    D = float(np.max(high - low))
    bound = 16.0 * K * EPS * D * D
    eng = block_engine(A, H)
    lam = 2.0
    one = {}
    for B in ((1, 3) if K <= 1000 else (1,)):
        rs, mu_new, sd, acts = _inputs(A, K, H, 3, 77 * K + 10 * H + A)      # B = 1 is environment 0 of B = 3
        mu_new, sd, acts = mu_new[:B], sd[:B], np.ascontiguousarray(acts[:, :B * K])
        scores = (3.0 * rs.standard_normal(3 * K))[:B * K]
        if K >= 8:
            scores[[1, K - 2]] = [np.nan, np.inf]
        d = _SigmaDev(B, K, H, A, acts)
        got = d.run(eng, scores, mu_new, sd, lam)
        assert d.run(eng, scores, mu_new, sd, lam).tobytes() == got.tobytes(), "two calls differ"
        worst = 0.0
        for b in range(B):
            ref = _sigma_ref_sq(scores[b * K:(b + 1) * K], acts[:, b * K:(b + 1) * K], mu_new[b], lam)
            worst = max(worst, float(np.max(np.abs(got[b] * got[b] - ref))) / bound)
            if K > 1:
                assert ref.max() > 1e-4                  # (the comparison is not between two zeros)
        print(f"[A={A} K={K} H={H} B={B}] sigma'^2: worst ratio to the bound 16 K eps D^2 = {worst:.3e}")
        assert worst <= 1.0, f"sigma'^2 off by {worst:.2f}x the derived bound"
        if B == 1:
            one = dict(got=got, scores=scores, d=d, mu_new=mu_new, sd=sd, acts=acts)
        else:                                            # environment 0 of the batch: the single call's bytes
            assert got[0].tobytes() == one["got"][0].tobytes(), "environment 0 of B = 3 differs from the B = 1 call"
            # ... and environment 2 alone, as a B = 1 call on its own slices
            d2 = _SigmaDev(1, K, H, A, np.ascontiguousarray(acts[:, 2 * K:3 * K]))
            assert d2.run(eng, scores[2 * K:], mu_new[2:3], sd[2:3], lam)[0].tobytes() == got[2].tobytes()
    d, scores, mu_new, sd, acts = one["d"], one["scores"], one["mu_new"], one["sd"], one["acts"]
    # all weight on one candidate (a spread of 1e6 at lambda = 1e-3) whose actions are mu': exactly 0
    rs = np.random.RandomState(K)
    spread = rs.uniform(1.0, 1e6, K)
    i = int(rs.randint(K))
    spread[i] = 0.0
    got = d.run(eng, spread, acts[:, i, :][None], sd, 1e-3)
    assert got.tobytes() == np.zeros((1, H, A)).tobytes(), "one weighted candidate: sigma' is not exactly 0"
    # alpha = 1: sigma's bits;  a floor above everything: the floor;  a cap below everything: the cap
    assert d.run(eng, scores, mu_new, sd, lam, alpha=1.0).tobytes() == sd.tobytes()
    assert np.array_equal(d.run(eng, scores, mu_new, sd, lam, alpha=0.3, min_std=50.0), np.full((1, H, A), 50.0))
    assert np.array_equal(d.run(eng, scores, mu_new, sd, lam, alpha=0.3, max_std=2.0 ** -20), np.full((1, H, A), 2.0 ** -20))
    # the smoothing step on the kernel's own s is sigma_step, bit for bit
    from bc_mpc_amd.mppi_update import sigma_step
    s = one["got"]
    assert d.run(eng, scores, mu_new, sd, lam, alpha=0.3, min_std=0.2, max_std=0.9).tobytes() == sigma_step(
        sd, s, 0.3, 0.2, 0.9).tobytes()
    # no valid candidate: sigma unchanged
    for vec in (np.full(K, np.nan), np.resize([np.inf, np.nan, -np.inf], K)):
        assert d.run(eng, vec, mu_new, sd, lam, alpha=0.0, min_std=50.0).tobytes() == sd.tobytes()


def test_sigma_update_on_a_reward_engine_reads_the_negated_scores():
    K, H = 1000, 8
    rs, mu_new, sd, acts = _inputs(6, K, H, 1, 5)
    scores = 3.0 * rs.standard_normal(K)
    d = _SigmaDev(1, K, H, 6, acts)
    a = d.run(block_engine(6, H), scores, mu_new, sd, 2.0)
    b = d.run(block_engine(6, H, True), -scores, mu_new, sd, 2.0)
    assert a.tobytes() == b.tobytes() and d.run(block_engine(6, H, True), scores, mu_new, sd, 2.0).tobytes() != a.tobytes()


# ------------------------------------------------------------------ 2. and 4. the synchronous calls
def _chain(eng, states, mu, sd, B, K, H, iters, lam, seed, off, rho, weight, adapt, alpha, lo, hi):
    """plan_sample -> rollout -> control cost -> update -> sigma update, composed from the stream-ordered blocks."""
    from bc_mpc_amd import _lib
    torch, dev = _t()
    st = _stream()
    A = 6
    d_states, d_mu, d_sd = _dev(states), _dev(mu), _dev(sd)
    d_act = torch.empty((H, B * K, A), dtype=torch.float64, device=dev)
    d_costs = torch.empty(B * K, dtype=torch.float64, device=dev)
    d_scores = torch.empty(B * K, dtype=torch.float64, device=dev)
    d_tmp = torch.zeros(B * ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    d_res = torch.zeros(B * ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(B * STATS.itemsize, dtype=torch.uint8, device=dev)
    costs, scores = [], []
    for it in range(iters):
        if rho:
            eng.plan_sample_corr_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho, d_act.data_ptr(),
                                       stream=st)
        else:
            eng.plan_sample_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, d_act.data_ptr(), st)
        eng.rollout_batch_async(d_states.data_ptr(), B, d_act.data_ptr(), seed, off, d_costs.data_ptr(),
                                d_tmp.data_ptr(), st)
        costs.append(d_costs.cpu().numpy())
        eng.plan_argmin_async(d_costs.data_ptr(), d_act.data_ptr(), B, K, it, it > 0, d_res.data_ptr(), st)
        d_in = d_costs
        if weight:
            eng.mppi_control_cost_async(d_costs.data_ptr(), d_act.data_ptr(), B, K, d_mu.data_ptr(), d_sd.data_ptr(),
                                        weight, d_scores.data_ptr(), st)
            d_in = d_scores
        scores.append(d_in.cpu().numpy())
        eng.mppi_update_batch_async(d_in.data_ptr(), B, K, off, seed, it, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                    d_stats.data_ptr(), d_act.data_ptr(), st)
        if adapt:
            eng.mppi_sigma_update_async(d_in.data_ptr(), d_act.data_ptr(), B, K, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                        alpha, lo, hi, st)
    rec = d_res.cpu().numpy().view(np.float64).reshape(B, ctypes.sizeof(_lib.Result) // 8)
    return dict(mu=d_mu.cpu().numpy(), sd=d_sd.cpu().numpy(), stats=d_stats.cpu().numpy().view(STATS),
                costs=np.stack(costs), scores=np.stack(scores), index=rec[:, 0].copy().view(np.int64),
                cost=rec[:, 1].copy(), first=rec[:, 2:8].copy())


MODES = {"control": dict(weight=1.5, adapt=False), "adapt": dict(weight=0.0, adapt=True),
         "both": dict(weight=1.5, adapt=True)}
STEP = dict(alpha=0.25, lo=0.05, hi=0.45)


def _stats_tuple(s):
    return (s.weight_sum, s.ess, s.min_cost, s.n_valid)


@pytest.mark.parametrize("mode,rho", [("control", 0.0), ("adapt", 0.0), ("both", 0.0), ("both", 0.5)])
def test_synchronous_calls_equal_the_chain_of_blocks(mode, rho):
    spec, norm, _, _, state = _problem("delta")
    m = MODES[mode]
    H, iters, lam, seed = 7, 3, 2.0, 0xBEEF
    kw = dict(control_cost=m["weight"], adapt_sigma=m["adapt"], sigma_alpha=STEP["alpha"], min_std=STEP["lo"],
              max_std=STEP["hi"], rho=rho)
    # the single call: K = 400, the batched chain at B = 1 and cand_offset 0
    K = 400
    rs = np.random.RandomState(3)
    mu0, sd0 = rs.uniform(-0.5, 0.5, (1, H, 6)), rs.uniform(0.1, 0.5, (1, H, 6))
    eng = _engine(spec, norm, K, H, "delta")
    want = _chain(eng, state[None], mu0, sd0, 1, K, H, iters, lam, seed, 0, rho, m["weight"], m["adapt"], **STEP)
    res, mu1, stats, *sd1 = eng.mppi_get_action(state, mu0[0], sd0[0], iters, lam, seed, **kw)
    assert len(sd1) == (1 if m["adapt"] else 0)
    assert mu1.tobytes() == want["mu"][0].tobytes(), "single call: mu'"
    assert _stats_tuple(stats) == tuple(want["stats"][0].tolist()), "single call: statistics"
    assert (sd1[0] if sd1 else sd0[0]).tobytes() == want["sd"][0].tobytes(), "single call: sigma'"
    assert res.best_index == want["index"][0] and res.best_cost == want["cost"][0]
    assert res.first_action.tobytes() == want["first"][0].tobytes()
    # the record is the raw costs' argmin over all rounds; the statistics' minimum is the augmented scores'
    flat = want["costs"].reshape(-1)
    assert res.best_index == int(np.argmin(flat)) and res.best_cost == flat.min()
    assert stats.min_cost == want["scores"][-1].min()
    if m["weight"]:
        assert want["scores"].tobytes() != want["costs"].tobytes() and stats.min_cost != want["costs"][-1].min()
    if m["adapt"]:
        assert sd1[0].tobytes() != sd0[0].tobytes() and (sd1[0] >= STEP["lo"]).all() and (sd1[0] <= STEP["hi"]).all()
    # the B = 1 batched call on the same engine is the single call
    rb, mb, sb, *sdb = eng.mppi_get_actions(state[None], mu0, sd0, iters, lam, seed, 0, True, **kw)
    assert mb.tobytes() == mu1[None].tobytes() and rb.costs.tobytes() == want["costs"].tobytes()
    assert sb[0].tobytes() == want["stats"][0].tobytes() and (not sdb or sdb[0][0].tobytes() == sd1[0].tobytes())
    eng.close()
    # the batched call: 3 environments, 130 candidates each, at an offset
    B, K, off = 3, 130, 1000
    states = np.stack([state, 0.5 * state, -state])
    mu0, sd0 = rs.uniform(-0.5, 0.5, (B, H, 6)), rs.uniform(0.1, 0.5, (B, H, 6))
    eng = _engine(spec, norm, B * K, H, "delta")
    want = _chain(eng, states, mu0, sd0, B, K, H, iters, lam, seed, off, rho, m["weight"], m["adapt"], **STEP)
    res, mu1, stats, *sd1 = eng.mppi_get_actions(states, mu0, sd0, iters, lam, seed, off, True, **kw)
    again = eng.mppi_get_actions(states, mu0, sd0, iters, lam, seed, off, True, **kw)
    eng.close()
    assert mu1.tobytes() == want["mu"].tobytes() and again[1].tobytes() == mu1.tobytes(), "batched call: mu'"
    assert stats.tobytes() == want["stats"].tobytes(), "batched call: statistics"
    assert (sd1[0] if sd1 else sd0).tobytes() == want["sd"].tobytes(), "batched call: sigma'"
    assert res.costs.reshape(iters, B * K).tobytes() == want["costs"].tobytes(), "batched call: the costs are the raw ones"
    assert res.best_index.tobytes() == want["index"].tobytes() and res.best_cost.tobytes() == want["cost"].tobytes()
    assert res.first_action.tobytes() == want["first"].tobytes()
    for b in range(B):
        assert res.best_index[b] == int(np.argmin(res.costs[:, b].reshape(-1)))


def test_update_on_the_augmented_vector_is_the_plain_update_on_it():
    """mu' and the statistics of the _x call are bcmpc_mppi_update_batch_async's on c~, byte for byte; c~ is the
    definition's on the call's own raw costs and the sampled actions."""
    from bc_mpc_amd.mppi_update import augmented, control_cost
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    st = _stream()
    spec, norm, _, _, state = _problem("delta")
    B, K, H, lam, seed, off, weight = 3, 130, 7, 2.0, 99, 64, 2.0
    rs = np.random.RandomState(8)
    states = np.stack([state, 0.5 * state, -state])
    mu0, sd0 = rs.uniform(-0.5, 0.5, (B, H, 6)), rs.uniform(0.1, 0.5, (B, H, 6))
    eng = _engine(spec, norm, B * K, H, "delta")
    res, mu1, stats = eng.mppi_get_actions(states, mu0, sd0, 1, lam, seed, off, True, control_cost=weight)
    plain = eng.mppi_get_actions(states, mu0, sd0, 1, lam, seed, off, True)
    assert plain[0].costs.tobytes() == res.costs.tobytes() and plain[1].tobytes() != mu1.tobytes()
    acts = np.concatenate([orc.cem_actions(seed, 0, off + b * K, K, H, mu0[b], sd0[b], -np.ones(6), np.ones(6))
                           for b in range(B)], axis=1)
    scores = np.concatenate([augmented(res.costs[0, b], control_cost(acts[:, b * K:(b + 1) * K], mu0[b], sd0[b]), weight)
                             for b in range(B)])
    d_scores, d_mu, d_sd, d_act = _dev(scores), _dev(mu0), _dev(sd0), _dev(acts)
    d_stats = torch.zeros(B * STATS.itemsize, dtype=torch.uint8, device=dev)
    eng.mppi_update_batch_async(d_scores.data_ptr(), B, K, off, seed, 0, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                d_stats.data_ptr(), d_act.data_ptr(), st)
    assert d_mu.cpu().numpy().tobytes() == mu1.tobytes()
    assert d_stats.cpu().numpy().tobytes() == stats.tobytes()
    assert np.array_equal(stats["min_cost"], scores.reshape(B, K).min(axis=1))
    eng.close()


# ------------------------------------------------------------------ 5. the defaults
def test_x_entry_points_with_a_null_or_default_ext_are_the_plain_calls():
    from bc_mpc_amd import _lib
    spec, norm, _, _, state = _problem("delta")
    K, H, lam, seed = 130, 5, 1.5, 31337
    rs = np.random.RandomState(4)
    mu, sd = rs.uniform(-0.5, 0.5, (1, H, 6)), rs.uniform(0.1, 0.5, (1, H, 6))
    eng = _engine(spec, norm, K, H, "delta")
    lib, h = eng._lib, eng._h
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    r0, m0, s0 = eng.mppi_get_action(state, mu[0], sd[0], 2, lam, seed)
    b0, bm0, bs0 = eng.mppi_get_actions(state[None], mu, sd, 2, lam, seed, 7, True)
    mp, stt = _lib.Mppi(2, lam, 0), np.ascontiguousarray(state)
    zero = _lib.MppiExt()                                              # all zero: max_std == min_std == 0, both off
    for ext in (None, ctypes.byref(zero), ctypes.byref(_lib.MppiExt(0.0, 0, 0, 0.5, 0.1, math.inf))):
        m, s, res, stats = mu[0].copy(), sd[0].copy(), _lib.Result(), _lib.MppiStats()
        _lib.check(lib.bcmpc_mppi_get_action_x(h, dp(stt), ctypes.byref(mp), None, ext, seed, dp(m), dp(s),
                                               ctypes.byref(res), ctypes.byref(stats)))
        assert m.tobytes() == m0.tobytes() and s.tobytes() == sd[0].tobytes()
        assert (res.best_index, res.best_cost) == (r0.best_index, r0.best_cost) and _stats_tuple(stats) == _stats_tuple(s0)
        assert np.array(res.first_action[:6]).tobytes() == r0.first_action.tobytes()
        m, s, res, stats, costs = mu.copy(), sd.copy(), (_lib.Result * 1)(), np.zeros(1, dtype=STATS), np.empty((2, K))
        _lib.check(lib.bcmpc_mppi_get_actions_batch_x(h, dp(stt), 1, ctypes.byref(mp), None, ext, seed, 7, dp(m), dp(s),
                                                      res, stats.ctypes.data_as(ctypes.POINTER(_lib.MppiStats)),
                                                      dp(costs)))
        assert m.tobytes() == bm0.tobytes() and s.tobytes() == sd.tobytes() and costs.tobytes() == b0.costs.tobytes()
        assert stats.tobytes() == bs0.tobytes() and res[0].best_index == b0.best_index[0]
    # refusals by status code on a live engine, before anything runs
    bad = _lib.MppiExt(1.0, 0, 0, 0.0, 0.5, 0.25)
    m = mu[0].copy()
    rc = lib.bcmpc_mppi_get_action_x(h, dp(stt), ctypes.byref(mp), None, ctypes.byref(bad), seed, dp(m), dp(sd[0].copy()),
                                     ctypes.byref(_lib.Result()), ctypes.byref(_lib.MppiStats()))
    assert rc == _lib.ERR_ARG and b"max_std" in lib.bcmpc_last_error() and m.tobytes() == mu[0].tobytes()
    eng.close()
    from bc_mpc_amd.engine import RolloutEngine
    pol = RolloutEngine(20, 6, 128, 2, "tanh", False, H, 64, policy_hidden=64, policy_layers=2)
    with pytest.raises(ValueError, match=r"status 2\].*policy"):
        pol.mppi_get_action(state, mu[0], sd[0], 1, 1.0, 1, control_cost=1.0)
    pol.close()


class _Box:
    low, high, shape = -np.ones(6, np.float32), np.ones(6, np.float32), (6,)


class _Env:
    action_space = _Box()

    class observation_space:
        shape = (20,)


def test_controller_defaults_are_unchanged_and_the_options_reach_the_engine():
    from bc_mpc_amd import MPPIcontroller, cheetah_cost_fn
    spec, norm, dyn, _, state = _problem("delta")
    K, H, lam = 400, 6, 2.0
    seeds = [int(x) for x in np.random.RandomState(11).randint(0, 2**62, size=4, dtype=np.int64)]
    ctrl = MPPIcontroller(_Env(), dyn, horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, temperature=lam,
                          iterations=2, seed=11)
    fresh = _engine(spec, norm, K, H, "delta")
    # without the new keywords: the same actions from the same seeds as the plain engine call
    mu0, sd0 = ctrl.initial_distribution()
    a1 = ctrl.get_action(state)
    _, m1, _ = fresh.mppi_get_action(state, mu0, sd0, 2, lam, seeds[0])
    assert a1.tobytes() == m1[0].tobytes() and ctrl.last_sigma.tobytes() == sd0.tobytes()
    # switched on for the next call (read on every call, the same engine): the next seed, the _x call's answer
    ctrl.control_cost, ctrl.adapt_sigma, ctrl.sigma_alpha, ctrl.min_std = True, True, 0.2, 0.05
    engine_before = ctrl._engine
    mu0, sd0 = ctrl.initial_distribution()
    a2 = ctrl.get_action(state)
    assert ctrl._engine is engine_before
    r2, m2, st2, s2 = fresh.mppi_get_action(state, mu0, sd0, 2, lam, seeds[1], control_cost=lam, adapt_sigma=True,
                                            sigma_alpha=0.2, min_std=0.05)
    assert a2.tobytes() == m2[0].tobytes() and ctrl.last_sigma.tobytes() == s2.tobytes()
    assert ctrl.last_sigma.shape == (H, 6) and (ctrl.last_sigma >= 0.05).all() and s2.tobytes() != sd0.tobytes()
    assert ctrl.last_cost == r2.best_cost and ctrl.last_stats.min_cost == st2.min_cost
    # every call starts from init_std again
    assert ctrl.initial_distribution()[1].tobytes() == sd0.tobytes()
    # batched: last_sigma is [B, H, A]
    states = np.stack([state, 0.5 * state])
    acts = ctrl.get_actions(states)
    assert acts.shape == (2, 6) and ctrl.last_sigma.shape == (2, H, 6) and (ctrl.last_sigma >= 0.05).all()
    fresh.close()

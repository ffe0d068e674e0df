"""Single-engine CEM and MPPI (bcmpc_cem_get_action / bcmpc_mppi_get_action) on a team engine whose team gives up.

The give-up is forced with the library's test hook, exactly as tests/test_gpu_plan_batch.py's fallback test
forces it: the team launch is skipped and reported as a team that gave up, the planner's updates of that
attempt run on whatever the cost buffer held, and the call must then start over on the fallback engine from
the ORIGINAL plans.

The expected answer is the building blocks' composition (cem_rollout_async, select_async + cem_refit_async or
mppi_update_async) on a non-team engine of the fallback's layout, run from the original plans and held to the
oracle in every iteration the way tests/test_gpu_cem.py and tests/test_gpu_mppi.py hold a non-team engine:
costs within that file's tolerance and envelope, the elite set exactly oracle.cem_select of the GPU's own
costs, the refit bit-identical to oracle.cem_refit, the MPPI update within test_gpu_mppi's derived bound, the
record np.argmin over all iterations' costs.  The team engine's call under the forced give-up returns that
record, plan and statistics bit for bit, and team_reruns grows by one per call.

Shape: the smallest that takes the team kernel with a partial last column -- the 2x64 tanh net, S = 20,
A = 6, K = 37, H = 5, 3 iterations, 5 elites.
"""
import numpy as np
import pytest

from test_gpu_cem import ELITE, _bufs, _close, _result
from test_gpu_mppi import STATS, _check, mppi_ref
from test_gpu_parity import team_ok
from test_gpu_plan_batch import A, HIGH, LOW, S, net, plans

pytestmark = pytest.mark.gpu

K, H, ITERS, N_ELITE, ALPHA, LAM, SEED = 37, 5, 3, 5, 0.1, 1.0, 0xC0FFEE


def _composition(n, planner, state, mu0, sd0):
    """The blocks on a split1 engine (what a team engine of this shape falls back to), each iteration held
    to the oracle.  Returns (position, cost, first action, mu', sigma', MPPI statistics or None)."""
    import torch
    from oracle import mpc_oracle as orc
    eng = n.engine("split1", K, H)
    dev = torch.device("cuda", 0)
    b = _bufs(K, H, A, N_ELITE, dev)
    d_stats = torch.zeros(STATS.itemsize, dtype=torch.uint8, device=dev)
    d_state = torch.from_numpy(np.array(state)).to(dev)
    d_mu, d_sd = torch.from_numpy(mu0.copy()).to(dev), torch.from_numpy(sd0.copy()).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    all_costs, hist, stats = [], [], None
    for it in range(ITERS):
        mu_in, sd_in = d_mu.cpu().numpy(), d_sd.cpu().numpy()
        hist.append((mu_in, sd_in))
        eng.cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sd.data_ptr(), SEED, it, 0, K,
                              b["costs"].data_ptr(), b["res"].data_ptr(), it > 0, st)
        costs = b["costs"].cpu().numpy()
        acts = orc.cem_actions(SEED, it, 0, K, H, mu_in, sd_in, LOW, HIGH)
        want, near = n.score(state, acts)
        _close(costs, want, near, f"{planner} it{it}")
        all_costs.append(costs)
        if planner == "cem":
            eng.select_async(None, b["costs"].data_ptr(), K, 0, N_ELITE, b["el"].data_ptr(), b["cnt"].data_ptr(), st)
            rec = b["el"].cpu().numpy().view(ELITE)
            want_el = orc.cem_select(costs, np.arange(K), N_ELITE)
            assert int(b["cnt"].cpu()[0]) == N_ELITE and np.array_equal(rec["index"][:N_ELITE], want_el)
            eng.cem_refit_async(b["el"].data_ptr(), b["cnt"].data_ptr(), SEED, it, ALPHA, d_mu.data_ptr(),
                                d_sd.data_ptr(), st)
            m2, s2 = orc.cem_refit(want_el, SEED, it, mu_in, sd_in, LOW, HIGH, ALPHA)
            assert np.array_equal(d_mu.cpu().numpy(), m2), "refit mean not bit-identical"
            assert np.array_equal(d_sd.cpu().numpy(), s2), "refit std not bit-identical"
        else:
            eng.mppi_update_async(b["costs"].data_ptr(), K, 0, SEED, it, LAM, d_mu.data_ptr(), d_sd.data_ptr(),
                                  d_stats.data_ptr(), st)
            stats = d_stats.cpu().numpy().view(STATS)[0].copy()
            _check(f"mppi it{it}", (d_mu.cpu().numpy(), stats), mppi_ref(costs, acts, mu_in, LAM), K)
            assert np.array_equal(d_sd.cpu().numpy(), sd0)
    flat = np.concatenate(all_costs)
    pos, cost, first = _result(b["res"], A)
    assert pos == int(np.argmin(flat)) and cost == flat[pos]
    it, i = divmod(pos, K)
    assert np.array_equal(first, orc.cem_actions(SEED, it, i, 1, 1, *hist[it], LOW, HIGH)[0, 0])
    out = pos, cost, first.copy(), d_mu.cpu().numpy(), d_sd.cpu().numpy(), stats
    eng.close()
    return out


@pytest.mark.parametrize("planner", ["cem", "mppi"])
def test_team_giveup_reruns_the_single_engine_call_from_the_original_plans(planner, monkeypatch):
    n = net("tanh64")
    assert team_ok(n.hidden, n.ln, 2, K, S, A)
    state = n.states[0]
    mu, sd = plans(2, H, 5)
    mu0, sd0 = mu[0].copy(), sd[0].copy()
    pos, cost, first, mu_want, sd_want, stats_want = _composition(n, planner, state, mu0, sd0)
    assert not np.array_equal(mu_want, mu0)                     # (the plan moves: a rerun from a stale plan would show)
    eng = n.engine("team", K, H)
    monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
    for call in range(2):                                       # (the second call: the fallback engine exists)
        before = eng.team_reruns
        if planner == "cem":
            res, mu1, sd1 = eng.cem_get_action(state, mu0.copy(), sd0.copy(), ITERS, N_ELITE, ALPHA, SEED)
            assert sd1.tobytes() == sd_want.tobytes(), "sigma' is not the refit chain's from the original plans"
        else:
            res, mu1, st1 = eng.mppi_get_action(state, mu0.copy(), sd0.copy(), ITERS, LAM, SEED)
            assert (st1.weight_sum, st1.ess, st1.min_cost, st1.n_valid) == (
                stats_want["weight_sum"], stats_want["ess"], stats_want["min_cost"], stats_want["n_valid"])
        assert eng.team_reruns == before + 1
        assert mu1.tobytes() == mu_want.tobytes(), "mu' is not the update chain's from the original plans"
        assert res.best_index == pos and res.best_cost == cost
        assert res.first_action.tobytes() == first.tobytes()
    monkeypatch.delenv("BCMPC_TEAM_SPINS")
    eng.close()

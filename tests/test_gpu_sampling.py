"""Correlated sampling noise and the CEM elite carry-over on the GPU (csrc/plan_noise.hip, the _s entry points).

The definition is bc_mpc_amd/sampling.py on the planners' normals (oracle.cem_normals).  Sampled actions, carried
sequences, refits, records and everything between two calls that must agree are compared BIT FOR BIT.  The two
tolerances are the suite's own: costs against the oracle rollout by test_gpu_parity.assert_costs_close with
conftest.envelope, and the MPPI update against test_gpu_mppi.mppi_ref within that file's derived bound (16 K
2^-53 amax on mu', the same factor relative on weight_sum, twice on ess) with m = K.

Nets and helpers are tests/test_gpu_plan_batch.py's (S = 20, A = 6: 2x64 tanh, 2x128 relu + LN); the engines
with A = 1 and A = 3 are TermCost engines (tests/test_gpu_term_cost.py's nets).

SEED_RISES was chosen on the CPU with the oracle: on the tanh net, B = 3, K = 65, H = 7, 6 elites, rho = 0.5,
three iterations WITHOUT carry-over, environment 2's best cost rises by 4.67 from iteration 0 to iteration 1
under the oracle's costs (seeds 1 .. 39 were tried; 4, 5, 12, 22, 27 and 32 show a rise) -- five orders of
magnitude above the cost tolerance, so the device's costs show it too.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import envelope
from test_gpu_mppi import STATS, _check, mppi_ref
from test_gpu_parity import assert_costs_close, team_ok
from test_gpu_plan_batch import A, BIG, ELITE, HIGH, LOW, S, _bytes, _dev, _Env, _stream, _t, block_engine, net, plans

pytestmark = pytest.mark.gpu

CEM = dict(B=3, K=65, H=7, iters=3, E=6, alpha=0.1, off=1000, rho=0.5)
SEED_RISES = 12


@functools.lru_cache(maxsize=None)
def sample_engine(Aa, H):
    """An engine whose H, A and bounds (+-1) the sampling kernels read: A = 6 is test_gpu_plan_batch's, the
    others are TermCost engines."""
    if Aa == A:
        return block_engine(H)
    from bc_mpc_amd import cost_functions as cf
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from test_gpu_term_cost import net as term_net
    Ss = {1: 5, 3: 11}[Aa]
    nt = term_net(Ss, Aa)
    eng = RolloutEngine(Ss, Aa, 64, 2, "tanh", False, H, 64, device=0, cost="terms")      # (an engine of its own)
    eng.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, nt.w.activation), nt.norm, 1)
    eng.set_cost_terms(cf.TermCost([cf.linear(0, 1.0), cf.quadratic(0, 0.1, on="action")]))
    return eng


def _definition(seed, it, off, B, K, H, Aa, rho, mu, sd):
    """[H, B*K, Aa]: sampling.correlated_actions per environment on the planners' normals."""
    from bc_mpc_amd.sampling import correlated_actions
    from oracle import mpc_oracle as orc
    z = orc.cem_normals(seed, it, off, B * K, H, Aa)
    return np.concatenate([correlated_actions(z[:, b * K:(b + 1) * K], rho, mu[b], sd[b], LOW[:Aa], HIGH[:Aa])
                           for b in range(B)], axis=1), z


# ------------------------------------------------------------------ 1. the sampling kernel
@pytest.mark.parametrize("Aa", [1, 3, 6])
@pytest.mark.parametrize("H", [1, 2, 7])
def test_sampler_is_bitwise_the_definition(H, Aa):
    from bc_mpc_amd.sampling import correlated_actions
    torch, dev = _t()
    eng = sample_engine(Aa, H)
    st = _stream()
    clipped = False
    for K in (1, 63, 65, 400):
        for B in (1, 3):
            mu6, sd6 = plans(B, H, K, clip_env=B - 1)
            mu, sd = np.ascontiguousarray(mu6[:, :, :Aa]), np.ascontiguousarray(sd6[:, :, :Aa])
            d_mu, d_sd = _dev(mu), _dev(sd)
            d_act = torch.empty((H, B * K, Aa), dtype=torch.float64, device=dev)
            for off in (0, BIG):
                for it in (0, 3):
                    seed = 0x5A3D1E + 7 * K + it
                    white, z = _definition(seed, it, off, B, K, H, Aa, 0.0, mu, sd)
                    for rho in (0.0, 0.5, 0.9):
                        label = f"K={K} B={B} off={off} it={it} rho={rho}"
                        d_act.fill_(float("nan"))
                        eng.plan_sample_corr_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho,
                                                   d_act.data_ptr(), stream=st)
                        got = d_act.cpu().numpy()
                        for b in range(B):
                            cols = slice(b * K, (b + 1) * K)
                            want = (white[:, cols] if rho == 0.0 else
                                    correlated_actions(z[:, cols], rho, mu[b], sd[b], LOW[:Aa], HIGH[:Aa]))
                            assert got[:, cols].tobytes() == want.tobytes(), f"{label} env {b}"
                            if b == B - 1 and K * H * Aa >= 400:
                                assert (want == 1.0).any() and (want == -1.0).any() and (np.abs(want) < 1.0).any()
                                clipped = True
                        if rho == 0.0:                   # ... and bitwise the independent sampler's output
                            d_act.fill_(float("nan"))
                            eng.plan_sample_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off,
                                                  d_act.data_ptr(), st)
                            assert d_act.cpu().numpy().tobytes() == got.tobytes(), label
                        elif H > 1 and K >= 63:      # (a sanity check of the test: the noise is not white)
                            assert got[1:].tobytes() != white[1:].tobytes(), label
    assert clipped


# ------------------------------------------------------------------ 2. plan_keep and the carried columns
def _keep_case(n_elite, K, off):
    """Hand-made select output for B = 3: (records [3, n_elite], counts [3])."""
    el = np.zeros((3, n_elite), dtype=ELITE)
    el["cost"], el["index"] = np.nan, -1
    cnt = np.zeros(3, dtype=np.int32)
    g = lambda b, c: off + b * K + c   # noqa: E731
    if n_elite == K:
        cnt[:] = (K, K, 0)
        el["index"][0] = [g(0, c) for c in range(K)]             # the whole population, in order
        el["index"][1] = [g(1, c) for c in range(K)]
        el["index"][1, 4] = -1                                   # a padding record inside the count
    else:
        cnt[:] = (0, 1, n_elite)                                 # environment 0: nothing but padding
        el["index"][1, 0] = g(1, 5)
        el["index"][2, :4] = [g(2, 0), g(2, 3), g(0, 2), g(2, 8)]   # the third names environment 0's column
        el["index"][2, 4:] = [g(2, K - 1 - i) for i in range(n_elite - 4)]
    el["cost"][el["index"] >= 0] = 1.5
    return el, cnt


@pytest.mark.parametrize("Aa,H", [(6, 7), (3, 2), (1, 1)])
@pytest.mark.parametrize("n_elite", [4, 6, 9])
def test_keep_and_carried_columns_are_bitwise_the_definition(n_elite, Aa, H):
    from bc_mpc_amd.sampling import carry_elites
    torch, dev = _t()
    B, K, off, seed, it, rho = 3, 9, BIG, 0xCA44E, 2, 0.5
    eng = sample_engine(Aa, H)
    st = _stream()
    rs = np.random.RandomState(n_elite)
    prev = rs.uniform(-1.0, 1.0, (H, B * K, Aa))
    el, cnt = _keep_case(n_elite, K, off)
    d_prev, d_cnt = _dev(prev), _dev(cnt)
    d_el = torch.from_numpy(el.view(np.uint8).reshape(-1).copy()).to(dev)
    d_keep = torch.full((B, n_elite, H, Aa), -77.0, dtype=torch.float64, device=dev)
    d_kc = torch.full((B,), -7, dtype=torch.int32, device=dev)
    eng.plan_keep_async(d_el.data_ptr(), d_cnt.data_ptr(), d_prev.data_ptr(), B, K, off, n_elite, d_keep.data_ptr(),
                        d_kc.data_ptr(), st)
    keep, kc = d_keep.cpu().numpy(), d_kc.cpu().numpy()
    want_keep = np.full((B, n_elite, H, Aa), -77.0)
    want_kc, carried = np.zeros(B, dtype=np.int32), []
    for b in range(B):
        cols = el["index"][b, :cnt[b]] - off                     # array columns of the records inside the count
        valid = (el["index"][b, :cnt[b]] >= 0) & (cols >= b * K) & (cols < (b + 1) * K)
        for e in np.nonzero(valid)[0]:
            want_keep[b, e] = prev[:, cols[e]]
        want_kc[b] = int(np.argmin(valid)) if not valid.all() else cnt[b]
        carried.append(cols[:want_kc[b]] - b * K)
    assert np.array_equal(kc, want_kc), (kc, want_kc)
    assert keep.tobytes() == want_keep.tobytes()
    assert list(want_kc) == ([K, 4, 0] if n_elite == K else [0, 1, 2])
    # the sampler with the keep buffer: carried columns are the copies, every other column its own sample
    mu6, sd6 = plans(B, H, n_elite)
    mu, sd = np.ascontiguousarray(mu6[:, :, :Aa]), np.ascontiguousarray(sd6[:, :, :Aa])
    d_mu, d_sd = _dev(mu), _dev(sd)
    d_act = torch.full((H, B * K, Aa), float("nan"), dtype=torch.float64, device=dev)
    eng.plan_sample_corr_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho, d_act.data_ptr(),
                               d_keep.data_ptr(), d_kc.data_ptr(), n_elite, st)
    got = d_act.cpu().numpy()
    fresh, _ = _definition(seed, it, off, B, K, H, Aa, rho, mu, sd)
    for b in range(B):
        cols = slice(b * K, (b + 1) * K)
        want = carry_elites(fresh[:, cols], prev[:, cols], carried[b])
        assert got[:, cols].tobytes() == want.tobytes(), f"env {b}"
        assert got[:, b * K + want_kc[b]:(b + 1) * K].tobytes() == fresh[:, b * K + want_kc[b]:(b + 1) * K].tobytes()
    # without the buffer nothing is carried
    eng.plan_sample_corr_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho, d_act.data_ptr(), stream=st)
    assert d_act.cpu().numpy().tobytes() == fresh.tobytes()


# ------------------------------------------------------------------ 3. batched CEM
def reference_cem(n, states, mu, sd, seed, rho, keep, device_costs=None, env=None, label=""):
    """The CEM loop of the definition, per environment.  ``device_costs`` [iters, B, K]: they are checked against
    the oracle rollout of the definition's actions and drive the selection (a cost within tolerance cannot flip
    an elite of the reference); None: the oracle's own costs do.  Returns (mu', sigma', the populations
    [iters][B] as [H, K, A], the elite columns [iters][B], the costs [iters, B, K])."""
    from bc_mpc_amd.sampling import carry_elites, correlated_actions, refit_from_actions
    from oracle import mpc_oracle as orc
    c = CEM
    B, K, H, E, off = c["B"], c["K"], c["H"], c["E"], c["off"]
    m, s = mu.copy(), sd.copy()
    pops, elites, costs = [], [], np.empty((c["iters"], B, K))
    for it in range(c["iters"]):
        pops.append([])
        elites.append([])
        for b in range(B):
            z = orc.cem_normals(seed, it, off + b * K, K, H, A)
            acts = correlated_actions(z, rho, m[b], s[b], LOW, HIGH)
            if keep and it > 0:
                acts = carry_elites(acts, pops[it - 1][b], elites[it - 1][b])
            want, near = n.score(states[b], acts)
            if device_costs is not None:
                assert_costs_close(device_costs[it, b], want, near, f"{label}/it{it}/env{b}", env=env)
                want = device_costs[it, b]
            costs[it, b] = want
            cols = orc.cem_select(want, off + b * K + np.arange(K), E) - off - b * K
            m[b], s[b] = refit_from_actions(acts[:, cols].transpose(1, 0, 2), m[b], s[b], c["alpha"])
            pops[it].append(acts)
            elites[it].append(cols)
    return m, s, pops, elites, costs


def _cem_inputs(name):
    c = CEM
    n = net(name)
    mu, sd = plans(c["B"], c["H"], 5)
    return n, n.states[:c["B"]], mu, sd


def _rises(costs):
    """(iteration, environment) pairs whose minimum is above the previous iteration's."""
    mins = costs.min(axis=2)
    return [(it, b) for it in range(1, mins.shape[0]) for b in range(mins.shape[1]) if mins[it, b] > mins[it - 1, b]]


@pytest.mark.parametrize("name,kernel", [("tanh64", "team"), ("tanh64", "split2"), ("reluln128", "split2")])
def test_batched_cem_with_correlated_noise_and_carry_over(name, kernel):
    c = CEM
    B, K, H, E = c["B"], c["K"], c["H"], c["E"]
    n, states, mu, sd = _cem_inputs(name)
    assert kernel != "team" or team_ok(n.hidden, n.ln, 2, B * K, S, A)
    eng = n.engine(kernel, B * K, H)
    env = envelope(n.ln, 2, n.hidden, H)
    seed = SEED_RISES
    res, mu1, sd1 = eng.cem_get_actions(states, mu, sd, c["iters"], E, c["alpha"], seed, c["off"], True, rho=c["rho"],
                                        keep_elites=True)
    plain, pmu, psd = eng.cem_get_actions(states, mu, sd, c["iters"], E, c["alpha"], seed, c["off"], True, rho=c["rho"])
    eng.close()
    for r, m1, s1, keep in ((res, mu1, sd1, True), (plain, pmu, psd, False)):
        label = f"{name}/{kernel}/keep={keep}"
        m, s, pops, elites, _ = reference_cem(n, states, mu, sd, seed, c["rho"], keep, r.costs, env, label)
        assert m1.tobytes() == m.tobytes() and s1.tobytes() == s.tobytes(), f"{label}: final plan"
        for b in range(B):
            flat = r.costs[:, b].reshape(-1)
            pos = int(np.argmin(flat))
            assert int(r.best_index[b]) == pos and r.best_cost[b] == flat[pos], f"{label} env {b}"
            it, j = divmod(pos, K)
            assert r.first_action[b].tobytes() == pops[it][b][0, j].tobytes(), f"{label} env {b}: first action"
        if keep:
            for it in range(1, c["iters"]):
                for b in range(B):
                    cols = elites[it - 1][b]
                    assert cols.size == E
                    # a carried column's cost is bitwise its cost of the iteration before
                    assert r.costs[it, b, :E].tobytes() == r.costs[it - 1, b, cols].tobytes(), f"{label} it {it} env {b}"
            assert not _rises(r.costs), f"{label}: a per-iteration minimum rose"
    if name == "tanh64":
        assert _rises(plain.costs), "without carry-over this seed loses its best sequence (chosen with the oracle)"


# ------------------------------------------------------------------ 4. batched MPPI
@pytest.mark.parametrize("name,kernel", [("tanh64", "team"), ("reluln128", "split2")])
def test_batched_mppi_with_correlated_noise(name, kernel):
    c = CEM
    B, K, H, off, rho, lam, seed = c["B"], c["K"], c["H"], c["off"], c["rho"], 1.0, 777
    n, states, mu, sd = _cem_inputs(name)
    eng = n.engine(kernel, B * K, H)
    res, mu1, stats = eng.mppi_get_actions(states, mu, sd, 1, lam, seed, off, True, rho=rho)
    acts, _ = _definition(seed, 0, off, B, K, H, A, rho, mu, sd)
    for b in range(B):
        a = acts[:, b * K:(b + 1) * K]
        want, near = n.score(states[b], a)
        assert_costs_close(res.costs[0, b], want, near, f"{name}/env{b}", env=envelope(n.ln, 2, n.hidden, H))
        _check(f"{name}/{kernel}/env{b}", (mu1[b], stats[b]), mppi_ref(res.costs[0, b], a, mu[b], lam), K)
        pos = int(np.argmin(res.costs[0, b]))
        assert int(res.best_index[b]) == pos and res.first_action[b].tobytes() == a[0, pos].tobytes()
    white, wmu, _ = eng.mppi_get_actions(states, mu, sd, 1, lam, seed, off, True)
    assert white.costs.tobytes() != res.costs.tobytes()
    # environments are independent: another state for environment 1 changes environment 1 only (two rounds)
    two = eng.mppi_get_actions(states, mu, sd, 2, lam, seed, off, True, rho=rho)
    other = states.copy()
    other[1] = n.states[4]
    moved = eng.mppi_get_actions(other, mu, sd, 2, lam, seed, off, True, rho=rho)
    eng.close()
    for b in (0, 2):
        assert moved[0].costs[:, b].tobytes() == two[0].costs[:, b].tobytes() and moved[1][b].tobytes() == two[1][b].tobytes()
        assert moved[2][b].tobytes() == two[2][b].tobytes() and moved[0].best_index[b] == two[0].best_index[b]
        assert moved[0].first_action[b].tobytes() == two[0].first_action[b].tobytes()
    assert moved[0].costs[:, 1].tobytes() != two[0].costs[:, 1].tobytes()


# ------------------------------------------------------------------ 5. single calls
def _same_step(one, batch):
    assert one.best_index == int(batch.best_index[0]) and one.best_cost == batch.best_cost[0]
    assert one.first_action.tobytes() == batch.first_action[0].tobytes()


@pytest.mark.parametrize("kernel", ["auto", "split2"])
def test_single_calls_equal_the_batched_call_with_one_environment(kernel):
    from bc_mpc_amd import _lib
    n = net("tanh64")
    K, H, E, alpha, lam, seed = 65, 7, 6, 0.1, 0.8, 4242
    mu, sd = plans(1, H, 3)
    state = n.states[2]
    eng = n.engine(kernel, K, H)
    for keep in (False, True):
        r, m1, s1 = eng.cem_get_action(state, mu[0], sd[0], 3, E, alpha, seed, rho=0.5, keep_elites=keep)
        rb, mb, sb = eng.cem_get_actions(state[None], mu, sd, 3, E, alpha, seed, 0, True, rho=0.5, keep_elites=keep)
        _same_step(r, rb)
        assert m1.tobytes() == mb[0].tobytes() and s1.tobytes() == sb[0].tobytes()
    r, m1, st1 = eng.mppi_get_action(state, mu[0], sd[0], 2, lam, seed, rho=0.5)
    rb, mb, stb = eng.mppi_get_actions(state[None], mu, sd, 2, lam, seed, 0, True, rho=0.5)
    _same_step(r, rb)
    assert m1.tobytes() == mb[0].tobytes()
    assert (stb[0]["weight_sum"], stb[0]["ess"], stb[0]["min_cost"], stb[0]["n_valid"]) == (
        st1.weight_sum, st1.ess, st1.min_cost, st1.n_valid)
    # the _s symbols with the default sampling (a zeroed struct, or NULL) are the calls without _s
    lib, h = eng._lib, eng._h
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    r0, m0, s0 = eng.cem_get_action(state, mu[0], sd[0], 3, E, alpha, seed)
    q0, qm0, qst0 = eng.mppi_get_action(state, mu[0], sd[0], 2, lam, seed)
    b0, bm0, bs0 = eng.cem_get_actions(state[None], mu, sd, 3, E, alpha, seed, 0, True)
    p0, pm0, pst0 = eng.mppi_get_actions(state[None], mu, sd, 2, lam, seed, 0, True)
    cem, mp = _lib.Cem(3, E, alpha, 0), _lib.Mppi(2, lam, 0)
    stt = np.ascontiguousarray(state)
    for smp in (ctypes.byref(_lib.Sampling(0.0, 0, 0)), None):
        m, s, res = mu[0].copy(), sd[0].copy(), _lib.Result()
        _lib.check(lib.bcmpc_cem_get_action_s(h, dp(stt), ctypes.byref(cem), smp, seed, dp(m), dp(s), ctypes.byref(res)))
        assert (res.best_index, res.best_cost) == (r0.best_index, r0.best_cost)
        assert m.tobytes() == m0.tobytes() and s.tobytes() == s0.tobytes()
        assert np.array(res.first_action[:A]).tobytes() == r0.first_action.tobytes()
        m, res, stats = mu[0].copy(), _lib.Result(), _lib.MppiStats()
        _lib.check(lib.bcmpc_mppi_get_action_s(h, dp(stt), ctypes.byref(mp), smp, seed, dp(m), dp(sd[0].copy()),
                                               ctypes.byref(res), ctypes.byref(stats)))
        assert (res.best_index, res.best_cost, stats.ess) == (q0.best_index, q0.best_cost, qst0.ess)
        assert m.tobytes() == qm0.tobytes()
        m, s, res, costs = mu.copy(), sd.copy(), (_lib.Result * 1)(), np.empty((3, K))
        _lib.check(lib.bcmpc_cem_get_actions_batch_s(h, dp(stt), 1, ctypes.byref(cem), smp, seed, 0, dp(m), dp(s), res,
                                                     dp(costs)))
        assert costs.tobytes() == b0.costs.tobytes() and m.tobytes() == bm0.tobytes() and s.tobytes() == bs0.tobytes()
        assert res[0].best_index == b0.best_index[0]
        m, res, stats, costs = mu.copy(), (_lib.Result * 1)(), (_lib.MppiStats * 1)(), np.empty((2, K))
        _lib.check(lib.bcmpc_mppi_get_actions_batch_s(h, dp(stt), 1, ctypes.byref(mp), smp, seed, 0, dp(m), dp(sd.copy()),
                                                      res, stats, dp(costs)))
        assert costs.tobytes() == p0.costs.tobytes() and m.tobytes() == pm0.tobytes() and stats[0].ess == pst0["ess"][0]
    eng.close()


# ------------------------------------------------------------------ 6. controllers and refusals
def _seeds(seed, n):
    return [int(x) for x in np.random.RandomState(seed).randint(0, 2**62, size=n, dtype=np.int64)]


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_controllers_answer_what_the_engine_calls_answer(kind):
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    n = net("tanh64")
    K, H, B = 65, 7, 2
    kw = dict(horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, seed=9)
    if kind == "cem":
        ctrl = CEMcontroller(_Env(), n.dyn, iterations=3, n_elite=6, noise_rho=0.5, keep_elites=True, **kw)
    else:
        ctrl = MPPIcontroller(_Env(), n.dyn, iterations=2, temperature=0.8, noise_rho=0.5, **kw)
    one, many = n.engine("auto", K, H), n.engine("auto", B * K, H)
    seeds = _seeds(9, 4)
    for step in range(3):                                   # consecutive steps, warm-started
        mu0, sd0 = ctrl.initial_distribution()
        a = ctrl.get_action(n.states[step])
        if kind == "cem":
            r, mu, sd = one.cem_get_action(n.states[step], mu0, sd0, 3, 6, ctrl.alpha, seeds[step], rho=0.5,
                                           keep_elites=True)
            assert np.array_equal(a, r.first_action) and np.array_equal(ctrl.last_sigma, sd)
        else:
            r, mu, stats = one.mppi_get_action(n.states[step], mu0, sd0, 2, 0.8, seeds[step], rho=0.5)
            assert np.array_equal(a, mu[0]) and ctrl.last_ess == float(stats.ess)
        assert np.array_equal(ctrl.last_mu, mu) and ctrl.last_cost == r.best_cost and ctrl.last_position == r.best_index
        if step:
            assert np.array_equal(mu0[:-1], prev[1:])
        prev = mu
    mu0, sd0 = ctrl.batch_initial_distribution(B)
    a = ctrl.get_actions(n.states[:B])
    if kind == "cem":
        r, mu, sd = many.cem_get_actions(n.states[:B], mu0, sd0, 3, 6, ctrl.alpha, seeds[3], rho=0.5, keep_elites=True)
        assert np.array_equal(a, r.first_action) and np.array_equal(ctrl.last_sigma, sd)
    else:
        r, mu, stats = many.mppi_get_actions(n.states[:B], mu0, sd0, 2, 0.8, seeds[3], rho=0.5)
        assert np.array_equal(a, mu[:, 0]) and np.array_equal(ctrl.last_ess, stats["ess"])
    assert np.array_equal(ctrl.last_mu, mu) and np.array_equal(ctrl.last_position, r.best_index)
    # the defaults answer differently (the arguments reach the device), from the same seed
    if kind == "cem":
        w, _, _ = many.cem_get_actions(n.states[:B], mu0, sd0, 3, 6, ctrl.alpha, seeds[3])
    else:
        w, _, _ = many.mppi_get_actions(n.states[:B], mu0, sd0, 2, 0.8, seeds[3])
    assert not np.array_equal(w.best_cost, r.best_cost)
    for e in (one, many, ctrl._engine, ctrl._batch_engine):
        e.close()


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_controllers_with_termination_and_terminal_value(kind):
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from test_gpu_term_cost import net as term_net
    from test_gpu_terminal_value import W, _Holder, critic
    from test_gpu_termination import AH, SH, _Env as HopperEnv, hopper_cost
    K, H, iters = 100, 5, 2
    cls = CEMcontroller if kind == "cem" else MPPIcontroller
    extra = dict(iterations=iters, n_elite=5, keep_elites=True) if kind == "cem" else dict(iterations=iters, temperature=0.7)

    def engine_answer(eng, state, mu0, sd0, alpha, seed):
        if kind == "cem":
            r, mu, _ = eng.cem_get_action(state, mu0, sd0, iters, 5, alpha, seed, rho=0.5, keep_elites=True)
        else:
            r, mu, _ = eng.mppi_get_action(state, mu0, sd0, iters, 0.7, seed, rho=0.5)
        return r, mu

    # a TermCost with done conditions
    nt = term_net(SH, AH)
    T = hopper_cost(nt.states[0])
    ctrl = cls(HopperEnv(), nt.dyn, horizon=H, cost_fn=T, num_simulated_paths=K, seed=7, noise_rho=0.5, **extra)
    mu0, sd0 = ctrl.initial_distribution()
    a = ctrl.get_action(nt.states[0])
    one = RolloutEngine(SH, AH, 64, 2, "tanh", False, H, K, device=0, cost="terms")
    one.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, nt.w.activation), nt.norm, 1)
    one.set_cost_terms(T)
    r, mu = engine_answer(one, nt.states[0], mu0, sd0, getattr(ctrl, "alpha", None), _seeds(7, 1)[0])
    assert ctrl._engine.info()["layout"].endswith("+terms+done")
    assert np.array_equal(a, r.first_action if kind == "cem" else mu[0]) and ctrl.last_cost == r.best_cost
    steps = one.last_termination_steps(np.arange(K))
    if r.best_index >= (iters - 1) * K:
        assert ctrl.last_termination_step == steps[r.best_index - (iters - 1) * K]
    else:
        assert ctrl.last_termination_step is None
    one.close()
    ctrl._engine.close()
    # a terminal value
    n = net("tanh64")
    ctrl = cls(_Env(), n.dyn, horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, seed=8, noise_rho=0.5,
               terminal_value=_Holder(critic(), 1), terminal_weight=W, **extra)
    mu0, sd0 = ctrl.initial_distribution()
    a = ctrl.get_action(n.states[1])
    one = n.engine("auto", K, H)
    one.set_terminal_value(critic(), W, 1)
    r, mu = engine_answer(one, n.states[1], mu0, sd0, getattr(ctrl, "alpha", None), _seeds(8, 1)[0])
    assert ctrl._engine.info()["layout"].endswith("+value")
    assert np.array_equal(a, r.first_action if kind == "cem" else mu[0]) and ctrl.last_cost == r.best_cost
    if r.best_index >= (iters - 1) * K:
        assert ctrl.last_terminal_value == one.last_terminal_values([r.best_index - (iters - 1) * K])[0]
    else:
        assert ctrl.last_terminal_value is None
    one.close()
    ctrl._engine.close()


def test_argument_refusals_by_status_code():
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import RolloutEngine
    n = net("tanh64")
    K, H = 64, 3
    eng = n.engine("auto", K, H)
    lib, h = eng._lib, eng._h
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    st, mu, sd = np.ascontiguousarray(n.states[:1]), np.zeros((1, H, A)), np.full((1, H, A), 0.5)
    out, stats = (_lib.Result * 1)(), (_lib.MppiStats * 1)()
    cem, mp = _lib.Cem(2, 4, 0.1, 0), _lib.Mppi(1, 1.0, 0)

    def calls(handle, smp, mppi_too=True):
        p = ctypes.byref(smp)
        rcs = [lib.bcmpc_cem_get_action_s(handle, dp(st), ctypes.byref(cem), p, 1, dp(mu.copy()), dp(sd.copy()), out),
               lib.bcmpc_cem_get_actions_batch_s(handle, dp(st), 1, ctypes.byref(cem), p, 1, 0, dp(mu.copy()),
                                                 dp(sd.copy()), out, None)]
        if mppi_too:
            rcs += [lib.bcmpc_mppi_get_action_s(handle, dp(st), ctypes.byref(mp), p, 1, dp(mu.copy()), dp(sd), out, stats),
                    lib.bcmpc_mppi_get_actions_batch_s(handle, dp(st), 1, ctypes.byref(mp), p, 1, 0, dp(mu.copy()), dp(sd),
                                                       out, stats, None)]
        return rcs

    for rho in (1.0, -0.25, 1.5, float("nan"), float("inf")):
        assert calls(h, _lib.Sampling(rho, 0, 0)) == [_lib.ERR_ARG] * 4, rho
        assert b"rho" in lib.bcmpc_last_error()
    for keep in (2, -1):
        assert calls(h, _lib.Sampling(0.5, keep, 0), mppi_too=False) == [_lib.ERR_ARG] * 2
        assert b"keep_elites" in lib.bcmpc_last_error()
    assert calls(h, _lib.Sampling(0.5, 1, 0))[2:] == [_lib.ERR_ARG] * 2          # MPPI has no elites to carry
    assert b"keep_elites" in lib.bcmpc_last_error()
    torch, dev = _t()
    d = torch.zeros(H * K * A, dtype=torch.float64, device=dev)
    for rho in (1.0, float("nan")):
        assert lib.bcmpc_plan_sample_corr_async(h, d.data_ptr(), d.data_ptr(), 1, K, 1, 0, 0, rho, None, None, 0,
                                                d.data_ptr(), None) == _lib.ERR_ARG
    assert lib.bcmpc_plan_sample_corr_async(h, d.data_ptr(), d.data_ptr(), 1, K, 1, 0, 0, 0.5, d.data_ptr(), None, 4,
                                            d.data_ptr(), None) == _lib.ERR_ARG       # keep without its counts
    assert lib.bcmpc_plan_keep_async(h, d.data_ptr(), d.data_ptr(), d.data_ptr(), 1, K, 0, 0, d.data_ptr(),
                                     d.data_ptr(), None) == _lib.ERR_ARG            # n_elite < 1
    assert calls(h, _lib.Sampling(0.5, 0, 0)) == [_lib.OK] * 4                   # the engine still works
    eng.close()
    pol = RolloutEngine(S, A, 256, 2, "relu", False, H, 64, policy_hidden=128, policy_layers=2, precision="fp32")
    assert calls(pol._h, _lib.Sampling(0.5, 0, 0)) == [_lib.ERR_UNSUPPORTED] * 4
    assert b"fused policy" in lib.bcmpc_last_error()
    pol.close()

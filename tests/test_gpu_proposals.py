"""Proposals on the GPU: given action sequences in every iteration's population (csrc/plan_prop.hip, the _p entry
points, bcmpc_rollout_policy_batch_async, the controllers' policy prior).

The definition is bc_mpc_amd/proposals.py on top of bc_mpc_amd/sampling.py.  Populations, carried and proposal
columns, elites, refits, records and everything between two calls that must agree are compared BIT FOR BIT.  The
tolerances are the suite's own: costs against the oracle rollout by test_gpu_parity.assert_costs_close with
conftest.envelope; the MPPI update against test_gpu_mppi.mppi_ref within that file's derived bound (16 K 2^-53 amax
on mu', the same factor relative on weight_sum, twice on ess) with m = K; the policy rollout as
test_gpu_parity.test_policy_stochastic_mode_pinned_every_step pins it (1e-5 + 1e-5 |a| on actions, 1e-6 (1 + |s|)
on states).  Nets, plans and helpers are tests/test_gpu_plan_batch.py's and tests/test_gpu_sampling.py's.

WINNER was chosen on the CPU with the oracle: tanh64 net, state 2, K = 65, H = 7, 6 elites, alpha 0.1, three
iterations, white noise, plans(1, 7, 3).  The proposal is the best of 4096 uniform sequences of RandomState(5) under
the oracle.  Seeds 1 .. 20 were tried with and without keep_elites; the docstring of
test_a_proposal_that_should_win_does records the search and the gaps of the seed kept.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import envelope
from test_gpu_mppi import STATS, _check, mppi_ref
from test_gpu_parity import ATOL, RTOL, assert_costs_close, team_ok, team_policy_ok
from test_gpu_plan_batch import A, BIG, HIGH, LOW, S, _dev, _Env, _stream, _t, net, plans
from test_gpu_sampling import CEM, _definition, sample_engine

pytestmark = pytest.mark.gpu

ODD = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0, 1.5, -1.5, 0.25])     # values a proposal may hold


def _proposals(B, P, H, Aa, seed):
    """[B, P, H, Aa]: inside and outside the box, with NaN, +-inf and -0.0 sprinkled in."""
    rs = np.random.RandomState(seed)
    p = rs.uniform(-1.6, 1.6, (B, P, H, Aa))
    flat = p.reshape(-1)
    idx = rs.choice(flat.size, size=min(flat.size, max(1, flat.size // 5)), replace=False)
    flat[idx] = ODD[np.arange(idx.size) % ODD.size]
    return p


def _layouts(prop):
    """(name, array in that layout, its three strides) for the canonical and the policy engines' output layout."""
    from bc_mpc_amd import proposals as pp
    B, P, H, Aa = prop.shape
    return [("canonical", prop, pp.canonical_strides(P, H, Aa)),
            ("policy", np.ascontiguousarray(prop.transpose(2, 0, 1, 3)).reshape(H, B * P, Aa), pp.policy_strides(B, P, Aa))]


# ------------------------------------------------------------------ 1. the sampler
@pytest.mark.parametrize("Aa", [1, 3, 6])
@pytest.mark.parametrize("H", [1, 2, 7])
def test_sampler_is_bitwise_the_injected_definition(H, Aa):
    from bc_mpc_amd import proposals as pp
    torch, dev = _t()
    eng = sample_engine(Aa, H)
    st = _stream()
    lo, hi = LOW[:Aa], HIGH[:Aa]
    seen_nan = seen_clip = seen_keep_full = False
    for K in (1, 9, 65):
        for B in (1, 3):
            mu6, sd6 = plans(B, H, K, clip_env=B - 1)
            mu, sd = np.ascontiguousarray(mu6[:, :, :Aa]), np.ascontiguousarray(sd6[:, :, :Aa])
            d_mu, d_sd = _dev(mu), _dev(sd)
            d_act = torch.empty((H, B * K, Aa), dtype=torch.float64, device=dev)
            seed, it, off = 0x9E0905 + K, 2, BIG
            for P in sorted({1, min(4, K), K}):
                prop = _proposals(B, P, H, Aa, 31 * K + P)
                for rho in (0.0, 0.5):
                    fresh, _ = _definition(seed, it, off, B, K, H, Aa, rho, mu, sd)
                    want = pp.inject_batch(fresh, prop, lo, hi, B)
                    for name, src, strides in _layouts(prop):
                        label = f"K={K} B={B} P={P} rho={rho} {name}"
                        d_src = _dev(src)
                        d_act.fill_(7.0)
                        eng.plan_sample_prop_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho,
                                                   d_act.data_ptr(), d_src.data_ptr(), P, *strides, stream=st)
                        got = d_act.cpu().numpy()
                        assert got.tobytes() == want.tobytes(), label
                        assert d_src.cpu().numpy().tobytes() == src.tobytes(), f"{label}: the source was written"
                        for b in range(B):                 # every other column: the sampler's own bits
                            cols = slice(b * K, (b + 1) * K - P)
                            assert got[:, cols].tobytes() == fresh[:, cols].tobytes(), f"{label} env {b}"
                    seen_nan |= bool(np.isnan(want).any())
                    seen_clip |= bool((prop > 1.0).any() and (prop < -1.0).any())
                # with a keep buffer: the carried elites in front, the proposals behind, also when they fill K
                for n_elite in sorted({e for e in (K - P, 2) if 1 <= e <= K - P}):
                    rs = np.random.RandomState(K + P + n_elite)
                    keep = rs.uniform(-1.0, 1.0, (B, n_elite, H, Aa))
                    cnt = np.array([n_elite, 1, 0][:B], dtype=np.int32)
                    fresh, _ = _definition(seed, it, off, B, K, H, Aa, 0.5, mu, sd)
                    carried = fresh.copy()
                    for b in range(B):
                        carried[:, b * K:b * K + cnt[b]] = keep[b, :cnt[b]].transpose(1, 0, 2)
                    want = pp.inject_batch(carried, prop, lo, hi, B, n_elite)
                    d_keep, d_cnt, d_src = _dev(keep), _dev(cnt), _dev(prop)
                    d_act.fill_(7.0)
                    eng.plan_sample_prop_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, 0.5,
                                               d_act.data_ptr(), d_src.data_ptr(), P, *pp.canonical_strides(P, H, Aa),
                                               d_keep=d_keep.data_ptr(), d_keep_count=d_cnt.data_ptr(), n_elite=n_elite,
                                               stream=st)
                    assert d_act.cpu().numpy().tobytes() == want.tobytes(), f"K={K} B={B} P={P} keep {n_elite}"
                    seen_keep_full |= n_elite + P == K
    assert seen_nan and seen_clip and seen_keep_full


def test_negative_zero_against_a_zero_bound_and_the_refusals():
    """-0.0 is not below a bound of 0.0: the samplers' expression keeps it where np.clip answers +0.0."""
    from bc_mpc_amd import proposals as pp
    torch, dev = _t()
    H, K, B, P = 2, 9, 1, 2
    eng = net("tanh64").engine("auto", 64, H)
    low, high = np.zeros(A), np.ones(A)
    eng.set_action_bounds(low, high)
    mu, sd = plans(B, H, 1)
    prop = np.zeros((B, P, H, A))
    prop[0, 0] = -0.0
    prop[0, 1, :, ::2] = -0.0
    d_mu, d_sd, d_src = _dev(mu), _dev(sd), _dev(prop)
    d_act = torch.empty((H, K, A), dtype=torch.float64, device=dev)
    st = _stream()
    eng.plan_sample_prop_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, 5, 0, 0, 0.0, d_act.data_ptr(),
                               d_src.data_ptr(), P, *pp.canonical_strides(P, H, A), stream=st)
    got = d_act.cpu().numpy()[:, K - P:]
    want = pp.clip(prop[0], low, high).transpose(1, 0, 2)
    assert got.tobytes() == want.tobytes() and np.signbit(got[:, 0]).all()
    assert not np.signbit(np.clip(prop[0], low, high)).any()        # (what np.clip would have made of it)
    # refusals on a live engine, each before a launch: counts, aliasing strides, the keep rule
    p = d_src.data_ptr()
    args = (d_mu.data_ptr(), d_sd.data_ptr(), B, K, 5, 0, 0, 0.0, d_act.data_ptr(), p)
    for n_prop, strides, kw, word in ((0, (P * H * A, H * A, A), {}, "n_prop"), (K + 1, (0, H * A, A), {}, "n_prop"),
                                      (P, (0, H * A, A - 1), {}, "alias"), (P, (0, A, A), {}, "alias"),
                                      (P, (0, -1, A), {}, "strides"),
                                      (P, (0, H * A, A), dict(d_keep=p, d_keep_count=p, n_elite=K - 1), "n_elite")):
        with pytest.raises(ValueError, match=word):
            eng.plan_sample_prop_async(*args, n_prop, *strides, stream=st, **kw)
    st8, m8, s8 = net("tanh64").states[:1], mu, sd
    with pytest.raises(ValueError, match="fit"):
        eng.cem_get_actions(np.repeat(st8, 1, 0), m8, s8, 2, 2, 0.1, 1, proposals=np.zeros((1, 65, H, A)))
    with pytest.raises(ValueError, match="carried"):
        eng.cem_get_action(st8[0], m8[0], s8[0], 2, 4, 0.1, 1, keep_elites=True, proposals=np.zeros((61, H, A)))
    from bc_mpc_amd import _lib
    lib, dp = eng._lib, ctypes.POINTER(ctypes.c_double)
    cem, res = _lib.Cem(2, 2, 0.1, 0), _lib.Result()
    stt, m, s = np.ascontiguousarray(st8[0]), mu[0].copy(), sd[0].copy()
    for q, word in ((_lib.Proposals(prop.ctypes.data, 65, 0, 0, 0, 0), b"count"),
                    (_lib.Proposals(prop.ctypes.data, P, 0, 1, 2, 3), b"host"),
                    (_lib.Proposals(p, P, 1, 0, A, A), b"alias"), (_lib.Proposals(p, P, 2, 0, 0, 0), b"device")):
        rc = lib.bcmpc_cem_get_action_p(eng._h, stt.ctypes.data_as(dp), ctypes.byref(cem), None, ctypes.byref(q), 1,
                                        m.ctypes.data_as(dp), s.ctypes.data_as(dp), ctypes.byref(res))
        assert rc == _lib.ERR_ARG and word in lib.bcmpc_last_error(), (word, lib.bcmpc_last_error())
    eng.close()


# ------------------------------------------------------------------ 2. the policy rollout, one state per environment
def _policy_problem(kernel):
    from oracle import mpc_oracle as orc
    if kernel == "fp32":
        return orc.synthetic_weights(S, A, 256, 2, "relu", False), dict(precision="fp32")
    return orc.synthetic_weights(S, A, 500, 2, "tanh", False), dict(kernel=kernel)


def _policy_engine(w, kw, K, H, p, norm, mode="stochastic", explore=0.5):
    from bc_mpc_amd.engine import MLPSpec, PolicySpec, RolloutEngine
    e = RolloutEngine(S, A, w.hidden, 2, w.activation, w.layer_norm, H, K, policy_hidden=128, policy_layers=2,
                      policy_mode=mode, **kw)
    e.set_weights(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta), norm, 1)
    e.set_policy(PolicySpec(p.kernels, p.biases, p.ob_mean, p.ob_std, p.logstd), explore, 1)
    return e


@pytest.mark.parametrize("kernel", ["fp32", "split2", "team"])
def test_policy_rollout_batch_pinned_every_step(kernel):
    """B = 3 blocks of P = 8 candidates, each block started from its own state; every step pinned from the
    device's own trajectory as test_policy_stochastic_mode_pinned_every_step pins it."""
    import torch
    from oracle import mpc_oracle as orc
    B, P, H, seed, off = 3, 8, 7, 42, 100
    K = B * P
    w, kw = _policy_problem(kernel)
    assert kernel != "team" or team_policy_ok(w.hidden, w.activation, w.layer_norm, K, 128, 2)
    p = orc.synthetic_policy(S, A, 128, 2)
    norm = orc.synthetic_normalization()
    states = np.stack([orc.synthetic_state(norm, seed=11 + b) for b in range(B)])
    dyn, pol = orc.NumpyDynamics(w, norm), orc.NumpyPolicy(p)
    eng = _policy_engine(w, kw, K, H, p, norm)
    if kernel != "fp32":
        assert eng.info()["kernel"] == kernel
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def run(e, d_st, n_envs, batch=True):
        k = e.num_paths
        d_traj, d_out, d_costs = torch.empty((H + 1, k, S), **f64), torch.empty((H, k, A), **f64), torch.empty(k, **f64)
        if batch:
            e.rollout_policy_batch_async(d_st.data_ptr(), n_envs, None, seed, off, d_costs.data_ptr(), d_traj.data_ptr(),
                                         d_out.data_ptr(), st)
        else:
            e.rollout_policy_async(d_st.data_ptr(), None, seed, off, d_costs.data_ptr(), d_traj.data_ptr(),
                                   d_out.data_ptr(), None, st)
        out = d_traj.cpu().numpy(), d_out.cpu().numpy(), d_costs.cpu().numpy()
        e.check_status()
        return out
    traj, acts, costs = run(eng, _dev(states), B)
    for b in range(B):
        assert traj[0, b * P:(b + 1) * P].tobytes() == np.tile(states[b], (P, 1)).tobytes(), f"block {b}: start state"
    sd = np.exp(p.logstd.astype(np.float64))
    for h in range(H):
        want = pol.mean(traj[h]).astype(np.float64) + sd * orc.device_rng_normals(seed, off, K, h, A)
        da = np.abs(acts[h] - want)
        assert (da <= 1e-5 + 1e-5 * np.abs(want)).all(), f"step {h}: action off by {da.max():.3e}"
        nxt = dyn.predict(traj[h], acts[h])
        ds = np.abs(traj[h + 1] - nxt)
        assert (ds <= 1e-6 * (1 + np.abs(nxt))).all(), f"step {h}: state off by {ds.max():.3e}"
    assert len({acts[:, k].tobytes() for k in range(K)}) == K        # the stochastic mode: K distinct sequences
    # one environment: bitwise rollout_policy_async
    one = run(eng, _dev(states[1:2]), 1)
    ref = run(eng, _dev(states[1]), 1, batch=False)
    for a, b in zip(one, ref):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match="multiple"):
        eng.rollout_policy_batch_async(_dev(states).data_ptr(), 5, None, seed, off, None, None, 8, st)
    eng.close()


# ------------------------------------------------------------------ 3. batched CEM and MPPI with proposals
NP = 4      # proposals per environment in the planner tests


def reference_cem_p(n, states, mu, sd, seed, rho, keep, prop, device_costs=None, env=None, label="", c=CEM):
    """test_gpu_sampling.reference_cem with proposals.inject behind the carry-over: the definition's loop, driven
    by the device's own per-iteration costs when given (they are held to the oracle rollout of the definition's
    population first).  Returns (mu', sigma', populations [iters][B], elite columns [iters][B], costs)."""
    from bc_mpc_amd import proposals as pp
    from bc_mpc_amd.sampling import carry_elites, correlated_actions, refit_from_actions
    from oracle import mpc_oracle as orc
    B, K, H, E, off = states.shape[0], c["K"], c["H"], c["E"], c["off"]
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
            if prop is not None:
                acts = pp.inject(acts, prop[b], LOW, HIGH, E if keep else 0)
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


def _device_proposals(prop):
    """The same sequences in device memory in the policy engines' output layout."""
    from bc_mpc_amd import proposals as pp
    from bc_mpc_amd.engine import DeviceProposals
    B, P, H, Aa = prop.shape
    d = _dev(np.ascontiguousarray(prop.transpose(2, 0, 1, 3)))
    return DeviceProposals(d.data_ptr(), P, *pp.policy_strides(B, P, Aa), keep=d)


def _plan_inputs():
    c = CEM
    n = net("tanh64")
    mu, sd = plans(c["B"], c["H"], 5)
    prop = np.random.RandomState(77).uniform(-1.3, 1.3, (c["B"], NP, c["H"], A))
    return n, n.states[:c["B"]], mu, sd, prop


@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("keep", [False, True])
def test_batched_cem_with_proposals(keep, rho):
    c = CEM
    B, K, H, E = c["B"], c["K"], c["H"], c["E"]
    n, states, mu, sd, prop = _plan_inputs()
    eng = n.engine("split2", B * K, H)
    env = envelope(n.ln, 2, n.hidden, H)
    seed = 4321
    kw = dict(rho=rho, keep_elites=keep)
    res, mu1, sd1 = eng.cem_get_actions(states, mu, sd, c["iters"], E, c["alpha"], seed, c["off"], True, proposals=prop, **kw)
    dres, dmu, dsd = eng.cem_get_actions(states, mu, sd, c["iters"], E, c["alpha"], seed, c["off"], True,
                                         proposals=_device_proposals(prop), **kw)
    eng.close()
    label = f"keep={keep}/rho={rho}"
    # host and device proposals are one call
    assert dres.costs.tobytes() == res.costs.tobytes() and dmu.tobytes() == mu1.tobytes() and dsd.tobytes() == sd1.tobytes()
    assert dres.best_index.tobytes() == res.best_index.tobytes() and dres.first_action.tobytes() == res.first_action.tobytes()
    m, s, pops, elites, _ = reference_cem_p(n, states, mu, sd, seed, rho, keep, prop, res.costs, env, label)
    assert mu1.tobytes() == m.tobytes() and sd1.tobytes() == s.tobytes(), f"{label}: final plan"
    for b in range(B):
        flat = res.costs[:, b].reshape(-1)
        pos = int(np.argmin(flat))
        assert int(res.best_index[b]) == pos and res.best_cost[b] == flat[pos], f"{label} env {b}"
        it, j = divmod(pos, K)
        assert res.first_action[b].tobytes() == pops[it][b][0, j].tobytes(), f"{label} env {b}: first action"
        for it in range(1, c["iters"]):
            # a proposal column holds the same sequence from the same state in every iteration: the same cost bits
            assert res.costs[it, b, K - NP:].tobytes() == res.costs[0, b, K - NP:].tobytes(), f"{label} env {b}"
            if keep:
                cols = elites[it - 1][b]
                assert res.costs[it, b, :E].tobytes() == res.costs[it - 1, b, cols].tobytes(), f"{label} it {it} env {b}"


def test_team_giveup_rerun_carries_the_proposals(monkeypatch):
    """A team that gives up (forced with the library's test hook, as tests/test_gpu_plan_batch.py does) makes the
    synchronous call rerun on the fallback engine: host proposals are uploaded again there, device proposals are read
    where they are, and the answer is the definition's loop from the ORIGINAL plans with the proposals in it."""
    c = CEM
    B, K, H, E = c["B"], c["K"], c["H"], c["E"]
    n, states, mu, sd, prop = _plan_inputs()
    assert team_ok(n.hidden, n.ln, 2, B * K, S, A)
    eng = n.engine("team", B * K, H)
    env = envelope(n.ln, 2, n.hidden, H)
    monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
    for i, src in enumerate((prop, _device_proposals(prop))):
        res, mu1, sd1 = eng.cem_get_actions(states, mu, sd, c["iters"], E, c["alpha"], 99, c["off"], True, rho=0.5,
                                            keep_elites=True, proposals=src)
        assert eng.team_reruns == i + 1
        m, s, *_ = reference_cem_p(n, states, mu, sd, 99, 0.5, True, prop, res.costs, env, f"fallback/{i}")
        assert mu1.tobytes() == m.tobytes() and sd1.tobytes() == s.tobytes()
    monkeypatch.delenv("BCMPC_TEAM_SPINS")
    eng.close()


def _chain_p(eng, states, mu, sd, prop, B, K, H, iters, lam, seed, off, rho, weight, adapt, alpha, lo, hi):
    """plan_sample_prop -> rollout -> control cost -> update -> sigma update from the stream-ordered blocks."""
    from bc_mpc_amd import _lib
    from bc_mpc_amd import proposals as pp
    torch, dev = _t()
    st = _stream()
    P = prop.shape[1]
    d_states, d_mu, d_sd, d_prop = _dev(states), _dev(mu), _dev(sd), _dev(prop)
    f64 = dict(dtype=torch.float64, device=dev)
    d_act, d_costs, d_scores = torch.empty((H, B * K, A), **f64), torch.empty(B * K, **f64), torch.empty(B * K, **f64)
    d_tmp = torch.zeros(B * ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    d_res = torch.zeros(B * ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(B * STATS.itemsize, dtype=torch.uint8, device=dev)
    costs, pops = [], []
    for it in range(iters):
        eng.plan_sample_prop_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho, d_act.data_ptr(),
                                   d_prop.data_ptr(), P, *pp.canonical_strides(P, H, A), stream=st)
        pops.append(d_act.cpu().numpy())
        eng.rollout_batch_async(d_states.data_ptr(), B, d_act.data_ptr(), seed, off, d_costs.data_ptr(), d_tmp.data_ptr(), st)
        costs.append(d_costs.cpu().numpy())
        eng.plan_argmin_async(d_costs.data_ptr(), d_act.data_ptr(), B, K, it, it > 0, d_res.data_ptr(), st)
        d_in = d_costs
        if weight:
            eng.mppi_control_cost_async(d_costs.data_ptr(), d_act.data_ptr(), B, K, d_mu.data_ptr(), d_sd.data_ptr(), weight,
                                        d_scores.data_ptr(), st)
            d_in = d_scores
        eng.mppi_update_batch_async(d_in.data_ptr(), B, K, off, seed, it, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                    d_stats.data_ptr(), d_act.data_ptr(), st)
        if adapt:
            eng.mppi_sigma_update_async(d_in.data_ptr(), d_act.data_ptr(), B, K, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                        alpha, lo, hi, st)
    rec = d_res.cpu().numpy().view(np.float64).reshape(B, ctypes.sizeof(_lib.Result) // 8)
    return dict(mu=d_mu.cpu().numpy(), sd=d_sd.cpu().numpy(), stats=d_stats.cpu().numpy().view(STATS), costs=np.stack(costs),
                pops=pops, index=rec[:, 0].copy().view(np.int64), cost=rec[:, 1].copy(), first=rec[:, 2:2 + A].copy())


@pytest.mark.parametrize("rho,ext", [(0.0, False), (0.5, False), (0.5, True)])
def test_batched_mppi_with_proposals(rho, ext):
    """Round 0 against the definition: the population is inject(definition sample), its costs are the oracle's
    within the suite's tolerance and the update is test_gpu_mppi's reference on them within its derived bound.
    All rounds (with the control cost and the sigma update in one case): the synchronous call is, bit for bit, the
    chain of the stream-ordered blocks with plan_sample_prop as its sampler, whose populations are read back."""
    from bc_mpc_amd import proposals as pp
    c = CEM
    B, K, H, off, lam, seed, iters = c["B"], c["K"], c["H"], c["off"], 1.0, 777, c["iters"]
    n, states, mu, sd, prop = _plan_inputs()
    eng = n.engine("split2", B * K, H)
    kw = dict(control_cost=1.5, adapt_sigma=True, sigma_alpha=0.25, min_std=0.05, max_std=0.45) if ext else {}
    res, mu1, stats, *sd1 = eng.mppi_get_actions(states, mu, sd, iters, lam, seed, off, True, rho=rho, proposals=prop, **kw)
    dev_res = eng.mppi_get_actions(states, mu, sd, iters, lam, seed, off, True, rho=rho,
                                   proposals=_device_proposals(prop), **kw)
    want = _chain_p(eng, states, mu, sd, prop, B, K, H, iters, lam, seed, off, rho, 1.5 if ext else 0.0, ext, 0.25, 0.05, 0.45)
    first = eng.mppi_get_actions(states, mu, sd, 1, lam, seed, off, True, rho=rho, proposals=prop)
    eng.close()
    assert dev_res[0].costs.tobytes() == res.costs.tobytes() and dev_res[1].tobytes() == mu1.tobytes()
    assert res.costs.reshape(iters, B * K).tobytes() == want["costs"].tobytes() and mu1.tobytes() == want["mu"].tobytes()
    assert stats.tobytes() == want["stats"].tobytes() and (sd1[0] if sd1 else sd).tobytes() == want["sd"].tobytes()
    assert res.best_index.tobytes() == want["index"].tobytes() and res.best_cost.tobytes() == want["cost"].tobytes()
    assert res.first_action.tobytes() == want["first"].tobytes()
    fresh, _ = _definition(seed, 0, off, B, K, H, A, rho, mu, sd)
    pop0 = pp.inject_batch(fresh, prop, LOW, HIGH, B)
    assert want["pops"][0].tobytes() == pop0.tobytes()
    for it in range(iters):                                 # every round's proposal columns are the clipped proposals
        for b in range(B):
            assert want["pops"][it][:, (b + 1) * K - NP:(b + 1) * K].tobytes() == pop0[:, (b + 1) * K - NP:(b + 1) * K].tobytes()
    r0, m0, s0 = first
    assert ext or r0.costs[0].tobytes() == res.costs[0].tobytes()
    for b in range(B):
        a = pop0[:, b * K:(b + 1) * K]
        cost, near = n.score(states[b], a)
        assert_costs_close(r0.costs[0, b], cost, near, f"mppi/rho={rho}/env{b}", env=envelope(n.ln, 2, n.hidden, H))
        _check(f"mppi/rho={rho}/env{b}", (m0[b], s0[b]), mppi_ref(r0.costs[0, b], a, mu[b], lam), K)
        flat = res.costs[:, b].reshape(-1)
        assert int(res.best_index[b]) == int(np.argmin(flat))


@pytest.mark.parametrize("kernel", ["auto", "split2"])
def test_single_calls_equal_the_batched_call_and_null_is_todays_call(kernel):
    from bc_mpc_amd import _lib
    n = net("tanh64")
    K, H, E, alpha, lam, seed = 65, 7, 6, 0.1, 0.8, 4242
    mu, sd = plans(1, H, 3)
    state = n.states[2]
    prop = np.random.RandomState(9).uniform(-1.3, 1.3, (1, NP, H, A))
    eng = n.engine(kernel, K, H)
    for keep, rho in ((False, 0.0), (True, 0.5)):
        r, m1, s1 = eng.cem_get_action(state, mu[0], sd[0], 3, E, alpha, seed, rho=rho, keep_elites=keep, proposals=prop[0])
        rb, mb, sb = eng.cem_get_actions(state[None], mu, sd, 3, E, alpha, seed, 0, True, rho=rho, keep_elites=keep,
                                         proposals=prop)
        assert r.best_index == int(rb.best_index[0]) and r.best_cost == rb.best_cost[0]
        assert r.first_action.tobytes() == rb.first_action[0].tobytes()
        assert m1.tobytes() == mb[0].tobytes() and s1.tobytes() == sb[0].tobytes()
    for kw in (dict(), dict(rho=0.5, control_cost=1.5, adapt_sigma=True, sigma_alpha=0.25, min_std=0.05, max_std=0.45)):
        r, m1, st1, *q1 = eng.mppi_get_action(state, mu[0], sd[0], 2, lam, seed, proposals=prop[0], **kw)
        rb, mb, stb, *qb = eng.mppi_get_actions(state[None], mu, sd, 2, lam, seed, 0, True, proposals=prop, **kw)
        assert r.best_index == int(rb.best_index[0]) and r.best_cost == rb.best_cost[0] and m1.tobytes() == mb[0].tobytes()
        assert tuple(stb[0].tolist()) == (st1.weight_sum, st1.ess, st1.min_cost, st1.n_valid)
        assert len(q1) == len(qb) and all(a.tobytes() == b[0].tobytes() for a, b in zip(q1, qb))
    # _p with NULL proposals (or count 0) is the _s / _x call, bit for bit, whatever the other options
    lib, h, dp = eng._lib, eng._h, ctypes.POINTER(ctypes.c_double)
    P = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    stt = np.ascontiguousarray(state)
    cem, mp = _lib.Cem(3, E, alpha, 0), _lib.Mppi(2, lam, 0)
    none = _lib.Proposals(None, 0, 0, 0, 0, 0)
    for smp in (None, _lib.Sampling(0.5, 1, 0)):
        sref = ctypes.byref(smp) if smp is not None else None
        outs = []
        for q in ("s", None, none):
            m, s, res = mu[0].copy(), sd[0].copy(), _lib.Result()
            if q == "s":
                _lib.check(lib.bcmpc_cem_get_action_s(h, P(stt), ctypes.byref(cem), sref, seed, P(m), P(s), ctypes.byref(res)))
            else:
                _lib.check(lib.bcmpc_cem_get_action_p(h, P(stt), ctypes.byref(cem), sref,
                                                      ctypes.byref(q) if q is not None else None, seed, P(m), P(s),
                                                      ctypes.byref(res)))
            outs.append((m.tobytes(), s.tobytes(), bytes(res)))
        assert outs[0] == outs[1] == outs[2]
    for ext in (None, _lib.MppiExt(1.5, 1, 0, 0.25, 0.05, 0.45)):
        eref = ctypes.byref(ext) if ext is not None else None
        outs = []
        for q in ("x", None, none):
            m, s, res, stats = mu.copy(), sd.copy(), (_lib.Result * 1)(), (_lib.MppiStats * 1)()
            costs = np.zeros((2, K))
            if q == "x":
                _lib.check(lib.bcmpc_mppi_get_actions_batch_x(h, P(stt), 1, ctypes.byref(mp), None, eref, seed, 0, P(m),
                                                              P(s), res, stats, P(costs)))
            else:
                _lib.check(lib.bcmpc_mppi_get_actions_batch_p(h, P(stt), 1, ctypes.byref(mp), None, eref,
                                                              ctypes.byref(q) if q is not None else None, seed, 0, P(m),
                                                              P(s), res, stats, P(costs)))
            outs.append((m.tobytes(), s.tobytes(), bytes(res), bytes(stats), costs.tobytes()))
        assert outs[0] == outs[1] == outs[2]
    eng.close()


# ------------------------------------------------------------------ 4. a proposal that should win does
WINNER = dict(name="tanh64", state=2, K=65, H=7, E=6, alpha=0.1, iters=3, plan_seed=3, pool=4096, pool_seed=5, seed=1)


def winning_proposal(w=WINNER):
    """The best of ``pool`` uniform sequences under the oracle: [1, H, A]."""
    n = net(w["name"])
    acts = np.random.RandomState(w["pool_seed"]).uniform(-1.0, 1.0, (w["H"], w["pool"], A))
    cost, _ = n.score(n.states[w["state"]], acts)
    return acts[:, int(np.argmin(cost))][None].copy()


def oracle_gaps(seed, keep, w=WINNER):
    """Under the oracle's own costs: per iteration, (the best other column's cost) - (the proposal column's cost)."""
    n = net(w["name"])
    mu, sd = plans(1, w["H"], w["plan_seed"])
    c = dict(K=w["K"], H=w["H"], E=w["E"], off=0, iters=w["iters"], alpha=w["alpha"])
    prop = winning_proposal(w)[None]
    _, _, pops, _, costs = reference_cem_p(n, n.states[w["state"]][None], mu, sd, seed, 0.0, keep, prop, c=c)
    gaps = []
    for it in range(w["iters"]):
        pop, last = pops[it][0], w["K"] - 1
        # (with keep_elites the carried copies of the proposal itself tie with it, bit for bit: not "other" columns)
        other = [j for j in range(last) if pop[:, j].tobytes() != pop[:, last].tobytes()]
        assert len(other) >= last - (it if keep else 0)
        gaps.append(float(costs[it, 0, other].min() - costs[it, 0, last]))
    return gaps, float(costs[0, 0, last])


@pytest.mark.parametrize("keep", [False, True])
def test_a_proposal_that_should_win_does(keep):
    """WINNER's search (CPU, the oracle's costs, oracle_gaps below): the proposal costs 129.2466; at seed 1 the
    smallest gap to any other column over the three iterations is 29.548 without and 26.127 with keep_elites, and the
    call without the proposal ends 29.174 / 28.876 above it.  1000 x the cost tolerance ATOL + RTOL |cost| is 1.392,
    so the device's costs cannot order them otherwise.  Seeds 1 .. 20 were tried: without keep_elites every seed
    qualifies (gaps 11.7 .. 32.8); with it seeds 1 .. 19 do (20.2 .. 33.3) and seed 20 does not (a carried elite's
    neighbourhood beats the proposal by 6.4 in iteration 2).  The gaps are asserted again here from the oracle."""
    w = WINNER
    n = net(w["name"])
    K, H, E, seed = w["K"], w["H"], w["E"], w["seed"]
    mu, sd = plans(1, H, w["plan_seed"])
    state = n.states[w["state"]]
    prop = winning_proposal()
    gaps, pcost = oracle_gaps(seed, keep)
    assert min(gaps) >= 1000 * (ATOL + RTOL * abs(pcost)), (gaps, pcost)
    c = dict(K=K, H=H, E=E, off=0, iters=w["iters"], alpha=w["alpha"])
    *_, without = reference_cem_p(n, state[None], mu, sd, seed, 0.0, keep, None, c=c)
    assert without.min() - pcost >= 1000 * (ATOL + RTOL * abs(pcost))
    eng = n.engine("split2", K, H)
    rb, mb, sb = eng.cem_get_actions(state[None], mu, sd, w["iters"], E, w["alpha"], seed, 0, True, keep_elites=keep,
                                     proposals=prop[None])
    r, _, _ = eng.cem_get_action(state, mu[0], sd[0], w["iters"], E, w["alpha"], seed, keep_elites=keep, proposals=prop)
    plain, _, _ = eng.cem_get_actions(state[None], mu, sd, w["iters"], E, w["alpha"], seed, 0, True, keep_elites=keep)
    eng.close()
    from bc_mpc_amd import proposals as pp
    assert int(rb.best_index[0]) == K - 1 == r.best_index                  # iteration 0's proposal column
    assert rb.best_cost[0].tobytes() == rb.costs[0, 0, K - 1].tobytes() and r.best_cost == rb.best_cost[0]
    assert rb.first_action[0].tobytes() == pp.clip(prop[0, 0], LOW, HIGH).tobytes() == r.first_action.tobytes()
    mins = rb.costs[:, 0].min(axis=1)
    assert (mins == rb.costs[:, 0, K - 1]).all()                            # ... which is every iteration's best
    if keep:
        assert (np.diff(mins) <= 0).all()
    assert plain.best_cost[0] > rb.best_cost[0]                             # without the proposal: a worse answer


# ------------------------------------------------------------------ 5. controllers
def _controller(kind, n, policy, **kw):
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    common = dict(horizon=7, cost_fn=cheetah_cost_fn, num_simulated_paths=65, seed=11, **kw)
    extra = dict(policy_prior=policy, policy_paths=8) if policy is not None else {}
    if kind == "cem":
        return CEMcontroller(_Env(), n.dyn, iterations=3, n_elite=6, alpha=0.1, **common, **extra)
    return MPPIcontroller(_Env(), n.dyn, iterations=2, temperature=0.8, **common, **extra)


@functools.lru_cache(maxsize=None)
def _prior_problem():
    """A dynamics net inside the policy engines' limits (hidden 65 .. 512) and a 2 x 128 policy."""
    from oracle import mpc_oracle as orc
    n = net("reluln128")
    return n, orc.NumpyPolicy(orc.synthetic_policy(S, A, 128, 2))


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_controllers_with_a_policy_prior_are_the_engine_level_composition(kind):
    import torch
    from bc_mpc_amd import policy as _policy
    from bc_mpc_amd import proposals as pp
    from bc_mpc_amd.engine import DeviceProposals, RolloutEngine
    n, pol = _prior_problem()
    B, K, H, Pp = 3, 65, 7, 8
    states = n.states[:B]
    user = np.random.RandomState(3).uniform(-1.2, 1.2, (B, 2, H, A))
    ctrl, twin = _controller(kind, n, pol), _controller(kind, n, pol)
    seeds = np.random.RandomState(11)
    draw = lambda: int(seeds.randint(0, 2**62, dtype=np.int64))   # noqa: E731
    w = n.w
    pspec, _ = _policy.extract(pol)
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)

    def compose(sts, mu0, sd0, seed, pseed, usr):
        """The prior block on an engine of its own, then the engine's call with the same two seeds."""
        b = sts.shape[0]
        plan = n.engine("auto", b * K, H)
        peng = RolloutEngine(S, A, w.hidden, 2, w.activation, w.layer_norm, H, b * Pp, policy_hidden=pspec.hidden,
                             policy_layers=pspec.n_layers, policy_mode="stochastic")
        from bc_mpc_amd.engine import MLPSpec
        peng.set_weights(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta), n.norm, 1)
        peng.set_policy(pspec, 0.0, 1)
        d_out, d_costs = torch.empty((H, b * Pp, A), **f64), torch.empty(b * Pp, **f64)
        peng.rollout_policy_batch_async(_dev(sts).data_ptr(), b, None, pseed, 0, d_costs.data_ptr(), None, d_out.data_ptr(),
                                        _stream())
        torch.cuda.synchronize()
        peng.check_status()
        seqs = d_out.cpu().numpy().reshape(H, b, Pp, A).transpose(1, 2, 0, 3)          # [b, Pp, H, A]
        if usr is not None:
            seqs = np.concatenate([usr, seqs], axis=1)
        if kind == "cem":
            out = plan.cem_get_actions(sts, mu0, sd0, 3, 6, 0.1, seed, 0, True, proposals=np.ascontiguousarray(seqs))
        else:
            out = plan.mppi_get_actions(sts, mu0, sd0, 2, 0.8, seed, 0, True, proposals=np.ascontiguousarray(seqs))
        # the stored-array rollout of the same (clipped) sequences on the planning engine, in the proposal columns
        acts = np.zeros((H, b * K, A))
        P = seqs.shape[1]
        for e in range(b):
            acts[:, (e + 1) * K - P:(e + 1) * K] = pp.clip(seqs[e], LOW, HIGH).transpose(1, 0, 2)
        stored = plan.get_actions(sts, acts, return_costs=True).costs.reshape(b, K)[:, K - P:]
        plan.close(), peng.close()
        return out, stored

    # get_action, twice (the second call warm-starts), then get_actions with a user's proposals in front
    for step in range(2):
        mu0, sd0 = twin.initial_distribution()
        a = ctrl.get_action(states[step])
        seed, pseed = draw(), draw()
        out, stored = compose(states[step][None], mu0[None], sd0[None], seed, pseed, None)
        res, mu1 = out[0], out[1]
        twin._mu = mu1[0]
        assert ctrl.last_mu.tobytes() == mu1[0].tobytes() and ctrl.last_cost == res.best_cost[0]
        assert ctrl.last_position == int(res.best_index[0])
        assert a.tobytes() == (res.first_action[0] if kind == "cem" else mu1[0, 0]).tobytes()
        assert ctrl.last_proposal_costs.shape == (Pp,) and ctrl.last_proposal_costs.tobytes() == stored[0].tobytes()
        assert ctrl.last_best_from_proposal == bool(int(res.best_index[0]) % K >= K - Pp)
    mu0, sd0 = twin.batch_initial_distribution(B)
    acts = ctrl.get_actions(states, proposals=user)
    seed, pseed = draw(), draw()
    out, stored = compose(states, mu0, sd0, seed, pseed, user)
    res, mu1 = out[0], out[1]
    assert ctrl.last_mu.tobytes() == mu1.tobytes() and ctrl.last_cost.tobytes() == res.best_cost.tobytes()
    assert acts.tobytes() == (res.first_action if kind == "cem" else mu1[:, 0]).tobytes()
    assert ctrl.last_proposal_costs.shape == (B, 2 + Pp) and ctrl.last_proposal_costs.tobytes() == stored.tobytes()
    assert np.array_equal(ctrl.last_best_from_proposal, res.best_index % K >= K - 2 - Pp)
    # deterministic under a fixed seed; reset forgets the plans as before
    again = _controller(kind, n, pol)
    for step in range(2):
        again.get_action(states[step])
    assert again.get_actions(states, proposals=user).tobytes() == acts.tobytes()
    ctrl.reset()
    assert ctrl._mu is None and ctrl._bmu is None


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_controllers_with_the_options_off_are_unchanged(kind):
    n, _ = _prior_problem()
    a, b = _controller(kind, n, None), _controller(kind, n, None, policy_prior=None, policy_paths=0)
    for ctrl in (a, b):
        ctrl.out = [ctrl.get_action(n.states[0]), ctrl.get_action(n.states[1]), ctrl.get_actions(n.states[:3])]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.out, b.out))
    assert a._next_seed() == b._next_seed() == int(np.random.RandomState(11).randint(0, 2**62, size=4, dtype=np.int64)[3])
    assert b.last_proposal_costs is None and b.last_best_from_proposal is None

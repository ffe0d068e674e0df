"""Knot plans on the GPU (csrc/plan_knots.hip, the _k entry points and the step-count blocks).

The definition is bc_mpc_amd/knots.py on the planners' normals (oracle.cem_normals with the knot index in the place
of h).  Knot arrays, action arrays, carried knots, refits, records and everything between two device computations
that must agree are compared BIT FOR BIT.  The tolerances are the suite's own and no new one is introduced: costs
against the oracle rollout by test_gpu_parity.assert_costs_close with conftest.envelope; the MPPI update against
test_gpu_mppi.mppi_ref within that file's derived bound (16 K 2^-53 amax on mu', the same factor relative on
weight_sum, twice on ess) with m = K; the weighted variance within test_gpu_mppi_ext's derived 16 K 2^-53 D^2.

Nets and helpers are tests/test_gpu_plan_batch.py's and tests/test_gpu_sampling.py's (S = 20, A = 6: 2x64 tanh, 2x128
relu + LN; the engines with A = 1 and A = 3 are TermCost engines).
"""
import ctypes

import numpy as np
import pytest

from conftest import envelope
from test_gpu_mppi import STATS, _check, mppi_ref
from test_gpu_mppi_ext import EPS, _same_bits, _sigma_ref_sq
from test_gpu_parity import assert_costs_close
from test_gpu_plan_batch import A, BIG, ELITE, HIGH, LOW, _dev, _Env, _stream, _t, net, plans
from test_gpu_sampling import _keep_case, sample_engine

pytestmark = pytest.mark.gpu

KINDS = ("hold", "linear", "cubic")
CALL = dict(B=3, K=65, H=7, M=3, iters=3, E=6, alpha=0.1, off=1000)


def _definition(seed, it, off, B, K, H, M, Aa, rho, kind, mu, sd, z=None):
    """(knots [M, B*K, Aa], actions [H, B*K, Aa]): knots.knot_values / knots.expand per environment on the planners'
    normals; ``z`` [>= M, B*K, Aa]: the normals, when the caller has drawn them already."""
    from bc_mpc_amd import knots as kn
    from oracle import mpc_oracle as orc
    if z is None:
        z = orc.cem_normals(seed, it, off, B * K, M, Aa)
    th = np.concatenate([kn.knot_values(z[:M, b * K:(b + 1) * K], rho, mu[b], sd[b], LOW[:Aa], HIGH[:Aa])
                         for b in range(B)], axis=1)
    return th, kn.expand(th, H, kind, LOW[:Aa], HIGH[:Aa])


def _knot_counts(H):
    return sorted({m for m in (1, 2, 3, H - 1, H) if 1 <= m <= H})


# ------------------------------------------------------------------ 1. the sampler
@pytest.mark.parametrize("Aa", [1, 3, 6])
@pytest.mark.parametrize("H", [1, 2, 7])
def test_sampler_is_bitwise_the_definition(H, Aa):
    from bc_mpc_amd import knots as kn
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    eng = sample_engine(Aa, H)
    st = _stream()
    clipped = overshoot = False
    for K in (1, 63, 65, 400):
        for B in (1, 3):
            mu6, sd6 = plans(B, H, K, clip_env=B - 1)
            d_act = torch.empty((H, B * K, Aa), dtype=torch.float64, device=dev)
            d_ref = torch.empty((H, B * K, Aa), dtype=torch.float64, device=dev)
            for off in (0, BIG):
                for it in (0, 3):
                    seed = 0x5A3D1E + 7 * K + it
                    z = orc.cem_normals(seed, it, off, B * K, H, Aa)       # knot m's normal: step m's of the full draw
                    for M in _knot_counts(H):
                        mu, sd = np.ascontiguousarray(mu6[:, :M, :Aa]), np.ascontiguousarray(sd6[:, :M, :Aa])
                        d_mu, d_sd = _dev(mu), _dev(sd)
                        d_kn = torch.empty((M, B * K, Aa), dtype=torch.float64, device=dev)
                        for rho in (0.0, 0.5):
                            for kind in KINDS:
                                label = f"K={K} B={B} off={off} it={it} M={M} rho={rho} {kind}"
                                d_act.fill_(float("nan"))
                                d_kn.fill_(float("nan"))
                                eng.plan_sample_knots_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho, M,
                                                            kind, d_kn.data_ptr(), d_act.data_ptr(), stream=st)
                                th, acts = _definition(seed, it, off, B, K, H, M, Aa, rho, kind, mu, sd, z)
                                assert d_kn.cpu().numpy().tobytes() == th.tobytes(), f"{label}: knots"
                                got = d_act.cpu().numpy()
                                assert got.tobytes() == acts.tobytes(), f"{label}: actions"
                                if K * M * Aa >= 400:            # the last environment's plan clips at both bounds
                                    w = th[:, (B - 1) * K:]
                                    assert (w == 1.0).any() and (w == -1.0).any() and (np.abs(w) < 1.0).any()
                                    clipped = True
                                if kind == "cubic" and 2 < M < H and K >= 63:
                                    overshoot = overshoot or bool((np.abs(kn.expand(th, H, kind)) > 1.0).any())
                            if M == H:                           # every kind: plan_sample_corr's bits for these arguments
                                eng.plan_sample_corr_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho,
                                                           d_ref.data_ptr(), stream=st)
                                assert d_ref.cpu().numpy().tobytes() == got.tobytes(), f"{label}: M == H"
    assert clipped
    assert overshoot or H < 7                                    # (the cubic's second clip had something to clip)


def test_the_non_divisible_case_by_hand():
    """(H, M) = (7, 3): hold spans 3, 2, 2 steps; linear fractions in sixths."""
    torch, dev = _t()
    H, M, K, seed = 7, 3, 5, 99
    eng = sample_engine(A, H)
    mu, sd = plans(1, M, 3)
    d_mu, d_sd = _dev(mu), _dev(sd)
    d_kn = torch.empty((M, K, A), dtype=torch.float64, device=dev)
    d_act = torch.empty((H, K, A), dtype=torch.float64, device=dev)
    for kind in ("hold", "linear"):
        eng.plan_sample_knots_async(d_mu.data_ptr(), d_sd.data_ptr(), 1, K, seed, 0, 0, 0.0, M, kind, d_kn.data_ptr(),
                                    d_act.data_ptr(), stream=_stream())
        th, a = d_kn.cpu().numpy(), d_act.cpu().numpy()
        if kind == "hold":
            want = th[[0, 0, 0, 1, 1, 2, 2]]
        else:
            f2, f4 = 2.0 / 6.0, 4.0 / 6.0
            want = np.stack([th[0], th[0] + f2 * (th[1] - th[0]), th[0] + f4 * (th[1] - th[0]), th[1],
                             th[1] + f2 * (th[2] - th[1]), th[1] + f4 * (th[2] - th[1]), th[2]])
        assert a.tobytes() == want.tobytes(), kind


# ------------------------------------------------------------------ 2. plan_keep in knot space and the carried columns
@pytest.mark.parametrize("Aa,H,M,kind", [(6, 7, 3, "cubic"), (6, 7, 7, "linear"), (3, 2, 1, "hold"), (1, 1, 1, "linear")])
@pytest.mark.parametrize("n_elite", [4, 9])
def test_keep_and_carried_knots(n_elite, Aa, H, M, kind):
    from bc_mpc_amd import knots as kn
    torch, dev = _t()
    B, K, off, seed, it, rho = 3, 9, BIG, 0xCA44E, 2, 0.5
    eng = sample_engine(Aa, H)
    st = _stream()
    prev = np.random.RandomState(n_elite).uniform(-1.0, 1.0, (M, B * K, Aa))     # the previous iteration's knots
    el, cnt = _keep_case(n_elite, K, off)
    d_prev, d_cnt = _dev(prev), _dev(cnt)
    d_el = torch.from_numpy(el.view(np.uint8).reshape(-1).copy()).to(dev)
    d_keep = torch.full((B, n_elite, M, Aa), -77.0, dtype=torch.float64, device=dev)
    d_kc = torch.full((B,), -7, dtype=torch.int32, device=dev)
    eng.plan_keep_steps_async(d_el.data_ptr(), d_cnt.data_ptr(), d_prev.data_ptr(), B, K, off, n_elite,
                              d_keep.data_ptr(), d_kc.data_ptr(), M, st)
    keep, kc = d_keep.cpu().numpy(), d_kc.cpu().numpy()
    want_keep = np.full((B, n_elite, M, Aa), -77.0)
    want_kc, carried = np.zeros(B, dtype=np.int32), []
    for b in range(B):
        cols = el["index"][b, :cnt[b]] - off
        valid = (el["index"][b, :cnt[b]] >= 0) & (cols >= b * K) & (cols < (b + 1) * K)
        for e in np.nonzero(valid)[0]:
            want_keep[b, e] = prev[:, cols[e]]
        want_kc[b] = int(np.argmin(valid)) if not valid.all() else cnt[b]
        carried.append(cols[:want_kc[b]])
    assert np.array_equal(kc, want_kc) and keep.tobytes() == want_keep.tobytes()
    assert list(want_kc) == ([K, 4, 0] if n_elite == K else [0, 1, 2])
    # the sampler with the keep buffer: a carried column's knots are the copies and its actions their expansion
    mu6, sd6 = plans(B, M, n_elite)
    mu, sd = np.ascontiguousarray(mu6[:, :, :Aa]), np.ascontiguousarray(sd6[:, :, :Aa])
    d_mu, d_sd = _dev(mu), _dev(sd)
    d_kn = torch.full((M, B * K, Aa), float("nan"), dtype=torch.float64, device=dev)
    d_act = torch.full((H, B * K, Aa), float("nan"), dtype=torch.float64, device=dev)
    eng.plan_sample_knots_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho, M, kind, d_kn.data_ptr(),
                                d_act.data_ptr(), d_keep.data_ptr(), d_kc.data_ptr(), n_elite, st)
    th, _ = _definition(seed, it, off, B, K, H, M, Aa, rho, kind, mu, sd)
    fresh = th.copy()
    for b in range(B):
        th[:, b * K:b * K + want_kc[b]] = prev[:, carried[b]]
    assert d_kn.cpu().numpy().tobytes() == th.tobytes()
    assert d_act.cpu().numpy().tobytes() == kn.expand(th, H, kind, LOW[:Aa], HIGH[:Aa]).tobytes()
    # without the buffer nothing is carried
    eng.plan_sample_knots_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho, M, kind, d_kn.data_ptr(),
                                d_act.data_ptr(), stream=st)
    assert d_kn.cpu().numpy().tobytes() == fresh.tobytes()


# ------------------------------------------------------------------ 3. whole calls
def _chain(eng, planner, states, mu, sd, B, K, H, M, kind, iters, seed, off, rho, keep=False, E=0, alpha=0.0, lam=1.0,
           weight=0.0, adapt=None):
    """plan_sample_knots -> rollout -> plan_argmin -> select + refit | (control cost) update (sigma update) -> plan_keep,
    composed from the stream-ordered blocks; every iteration's input plans, arrays, costs and elites are read back."""
    from bc_mpc_amd import _lib
    torch, dev = _t()
    st = _stream()
    f64 = dict(dtype=torch.float64, device=dev)
    d_states, d_mu, d_sd = _dev(states), _dev(mu), _dev(sd)
    d_kn, d_act = torch.empty((M, B * K, A), **f64), torch.empty((H, B * K, A), **f64)
    d_costs, d_scores = torch.empty(B * K, **f64), torch.empty(B * K, **f64)
    d_tmp = torch.zeros(B * ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    d_res = torch.zeros(B * ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(B * STATS.itemsize, dtype=torch.uint8, device=dev)
    d_el = torch.zeros(B * max(E, 1) * ELITE.itemsize, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    d_keep = torch.zeros((B, max(E, 1), M, A), **f64)
    d_kc = torch.zeros(B, dtype=torch.int32, device=dev)
    its = []
    for it in range(iters):
        rec = dict(mu=d_mu.cpu().numpy(), sd=d_sd.cpu().numpy())
        kept = keep and it > 0
        eng.plan_sample_knots_async(d_mu.data_ptr(), d_sd.data_ptr(), B, K, seed, it, off, rho, M, kind, d_kn.data_ptr(),
                                    d_act.data_ptr(), d_keep.data_ptr() if kept else None,
                                    d_kc.data_ptr() if kept else None, E, st)
        rec.update(knots=d_kn.cpu().numpy(), acts=d_act.cpu().numpy())
        eng.rollout_batch_async(d_states.data_ptr(), B, d_act.data_ptr(), seed, off, d_costs.data_ptr(), d_tmp.data_ptr(), st)
        rec["costs"] = d_costs.cpu().numpy()
        eng.plan_argmin_async(d_costs.data_ptr(), d_act.data_ptr(), B, K, it, it > 0, d_res.data_ptr(), st)
        if planner == "cem":
            eng.select_batch_async(d_costs.data_ptr(), B, K, off, E, d_el.data_ptr(), d_cnt.data_ptr(), st)
            rec["elite"] = d_el.cpu().numpy().view(ELITE).reshape(B, E).copy()
            eng.cem_refit_batch_steps_async(d_el.data_ptr(), d_cnt.data_ptr(), B, E, seed, it, alpha, d_mu.data_ptr(),
                                            d_sd.data_ptr(), d_kn.data_ptr(), K, off, M, st)
            if keep and it + 1 < iters:
                eng.plan_keep_steps_async(d_el.data_ptr(), d_cnt.data_ptr(), d_kn.data_ptr(), B, K, off, E,
                                          d_keep.data_ptr(), d_kc.data_ptr(), M, st)
        else:
            d_in = d_costs
            if weight:
                eng.mppi_control_cost_steps_async(d_costs.data_ptr(), d_kn.data_ptr(), B, K, d_mu.data_ptr(),
                                                  d_sd.data_ptr(), weight, d_scores.data_ptr(), M, st)
                d_in = d_scores
            rec["scores"] = d_in.cpu().numpy()
            eng.mppi_update_batch_steps_async(d_in.data_ptr(), B, K, off, seed, it, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                              d_stats.data_ptr(), d_kn.data_ptr(), M, st)
            rec["mu_new"] = d_mu.cpu().numpy()
            if adapt:
                eng.mppi_sigma_update_steps_async(d_in.data_ptr(), d_kn.data_ptr(), B, K, lam, d_mu.data_ptr(),
                                                  d_sd.data_ptr(), M, adapt["alpha"], adapt["lo"], adapt["hi"], st)
            rec["stats"] = d_stats.cpu().numpy().view(STATS).copy()
        its.append(rec)
    r = d_res.cpu().numpy().view(np.float64).reshape(B, ctypes.sizeof(_lib.Result) // 8)
    return dict(mu=d_mu.cpu().numpy(), sd=d_sd.cpu().numpy(), stats=d_stats.cpu().numpy().view(STATS), its=its,
                costs=np.stack([x["costs"] for x in its]), index=r[:, 0].copy().view(np.int64), cost=r[:, 1].copy(),
                first=r[:, 2:2 + A].copy())


def _inputs(name):
    c = CALL
    n = net(name)
    mu, sd = plans(c["B"], c["M"], 5)
    return n, n.states[:c["B"]], mu, sd


def _check_populations(n, states, want, B, K, H, M, kind, seed, off, rho, label, carried=None):
    """Every iteration of a chain against the definition, given the device's own plans: both arrays bitwise, the costs
    within the suite's tolerance of the oracle rollout of the definition's action array."""
    from bc_mpc_amd import knots as kn
    env = envelope(n.ln, 2, n.hidden, H)
    for it, rec in enumerate(want["its"]):
        th, _ = _definition(seed, it, off, B, K, H, M, A, rho, kind, rec["mu"], rec["sd"])
        if carried and it > 0:
            for b in range(B):
                cols = carried[it - 1][b]
                th[:, b * K:b * K + cols.size] = want["its"][it - 1]["knots"][:, b * K + cols]
        acts = kn.expand(th, H, kind, LOW, HIGH)
        assert rec["knots"].tobytes() == th.tobytes(), f"{label}/it{it}: knots"
        assert rec["acts"].tobytes() == acts.tobytes(), f"{label}/it{it}: actions"
        for b in range(B):
            cost, near = n.score(states[b], acts[:, b * K:(b + 1) * K])
            assert_costs_close(rec["costs"][b * K:(b + 1) * K], cost, near, f"{label}/it{it}/env{b}", env=env)


@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("name,kernel,kind", [("tanh64", "split2", "linear"), ("reluln128", "split2", "cubic"),
                                              ("tanh64", "split2", "hold")])
def test_cem_calls(name, kernel, kind, rho):
    from bc_mpc_amd.sampling import refit_from_actions
    from oracle import mpc_oracle as orc
    c = CALL
    B, K, H, M, E, iters, off, alpha, seed = c["B"], c["K"], c["H"], c["M"], c["E"], c["iters"], c["off"], c["alpha"], 31
    n, states, mu, sd = _inputs(name)
    eng = n.engine(kernel, B * K, H)
    one = n.engine(kernel, K, H)
    kw = dict(rho=rho, keep_elites=True, knots=M, knot_interp=kind)
    res, mu1, sd1 = eng.cem_get_actions(states, mu, sd, iters, E, alpha, seed, off, True, **kw)
    want = _chain(eng, "cem", states, mu, sd, B, K, H, M, kind, iters, seed, off, rho, keep=True, E=E, alpha=alpha)
    assert mu1.shape == sd1.shape == (B, M, A)
    assert res.costs.reshape(iters, B * K).tobytes() == want["costs"].tobytes(), "costs"
    assert mu1.tobytes() == want["mu"].tobytes() and sd1.tobytes() == want["sd"].tobytes(), "plans"
    assert res.best_index.tobytes() == want["index"].tobytes() and res.best_cost.tobytes() == want["cost"].tobytes()
    assert res.first_action.tobytes() == want["first"].tobytes()
    # environment b of the batched call is the one-environment call at cand_offset + b * K; the single call is
    # the one-environment call at cand_offset 0
    for b in range(B):
        rb, mb, sb = one.cem_get_actions(states[b:b + 1], mu[b:b + 1], sd[b:b + 1], iters, E, alpha, seed, off + b * K,
                                         True, **kw)
        assert rb.costs[:, 0].tobytes() == res.costs[:, b].tobytes() and mb[0].tobytes() == mu1[b].tobytes()
        assert sb[0].tobytes() == sd1[b].tobytes() and rb.best_index[0] == res.best_index[b]
        assert rb.first_action[0].tobytes() == res.first_action[b].tobytes()
    r1, m1, s1 = one.cem_get_action(states[0], mu[0], sd[0], iters, E, alpha, seed, **kw)
    rb, mb, sb = one.cem_get_actions(states[:1], mu[:1], sd[:1], iters, E, alpha, seed, 0, True, **kw)
    assert m1.shape == (M, A) and m1.tobytes() == mb[0].tobytes() and s1.tobytes() == sb[0].tobytes()
    assert r1.best_index == int(rb.best_index[0]) and r1.best_cost == rb.best_cost[0]
    assert r1.first_action.tobytes() == rb.first_action[0].tobytes()
    eng.close()
    one.close()
    # against the definition, given the device's own refits and elites
    label = f"cem/{name}/{kernel}/{kind}/rho={rho}"
    carried = [[rec["elite"]["index"][b] - off - b * K for b in range(B)] for rec in want["its"]]
    _check_populations(n, states, want, B, K, H, M, kind, seed, off, rho, label, carried)
    for it, rec in enumerate(want["its"]):
        nxt_mu = want["its"][it + 1]["mu"] if it + 1 < iters else want["mu"]
        nxt_sd = want["its"][it + 1]["sd"] if it + 1 < iters else want["sd"]
        for b in range(B):
            cols = orc.cem_select(rec["costs"][b * K:(b + 1) * K], off + b * K + np.arange(K), E) - off - b * K
            assert np.array_equal(cols, carried[it][b]), f"{label}/it{it}/env{b}: elites"
            m, s = refit_from_actions(rec["knots"][:, b * K + cols].transpose(1, 0, 2), rec["mu"][b], rec["sd"][b], alpha)
            assert nxt_mu[b].tobytes() == m.tobytes() and nxt_sd[b].tobytes() == s.tobytes(), f"{label}/it{it}/env{b}: refit"
            if it > 0:                                   # a carried column's cost is its cost of the iteration before
                assert rec["costs"][b * K:b * K + E].tobytes() == want["its"][it - 1]["costs"][b * K + carried[it - 1][b]].tobytes()
    for b in range(B):
        flat = res.costs[:, b].reshape(-1)
        pos = int(np.argmin(flat))
        assert int(res.best_index[b]) == pos and res.best_cost[b] == flat[pos]
        it, j = divmod(pos, K)
        assert res.first_action[b].tobytes() == want["its"][it]["acts"][0, b * K + j].tobytes()


@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("name,kernel,kind", [("tanh64", "split2", "cubic"), ("reluln128", "split2", "linear")])
def test_mppi_calls(name, kernel, kind, rho):
    c = CALL
    B, K, H, M, iters, off, lam, seed = c["B"], c["K"], c["H"], c["M"], c["iters"], c["off"], 1.0, 777
    n, states, mu, sd = _inputs(name)
    eng = n.engine(kernel, B * K, H)
    one = n.engine(kernel, K, H)
    kw = dict(rho=rho, knots=M, knot_interp=kind)
    res, mu1, stats = eng.mppi_get_actions(states, mu, sd, iters, lam, seed, off, True, **kw)
    want = _chain(eng, "mppi", states, mu, sd, B, K, H, M, kind, iters, seed, off, rho, lam=lam)
    assert mu1.shape == (B, M, A)
    assert res.costs.reshape(iters, B * K).tobytes() == want["costs"].tobytes() and mu1.tobytes() == want["mu"].tobytes()
    assert stats.tobytes() == want["stats"].tobytes()
    assert res.best_index.tobytes() == want["index"].tobytes() and res.best_cost.tobytes() == want["cost"].tobytes()
    assert res.first_action.tobytes() == want["first"].tobytes()
    for b in range(B):
        rb, mb, sb = one.mppi_get_actions(states[b:b + 1], mu[b:b + 1], sd[b:b + 1], iters, lam, seed, off + b * K, True, **kw)
        assert rb.costs[:, 0].tobytes() == res.costs[:, b].tobytes() and mb[0].tobytes() == mu1[b].tobytes()
        assert sb[0].tobytes() == stats[b].tobytes() and rb.best_index[0] == res.best_index[b]
    r1, m1, st1 = one.mppi_get_action(states[0], mu[0], sd[0], iters, lam, seed, **kw)
    rb, mb, sb = one.mppi_get_actions(states[:1], mu[:1], sd[:1], iters, lam, seed, 0, True, **kw)
    assert m1.shape == (M, A) and m1.tobytes() == mb[0].tobytes() and r1.best_index == int(rb.best_index[0])
    assert (st1.weight_sum, st1.ess, st1.min_cost, st1.n_valid) == tuple(sb[0].tolist())
    # the control cost and the sigma update, in knot space: the call is the chain with the step-count blocks
    ext = dict(control_cost=1.5, adapt_sigma=True, sigma_alpha=0.25, min_std=0.05, max_std=0.45)
    rx, mx, sx, sdx = eng.mppi_get_actions(states, mu, sd, iters, lam, seed, off, True, **kw, **ext)
    wx = _chain(eng, "mppi", states, mu, sd, B, K, H, M, kind, iters, seed, off, rho, lam=lam, weight=1.5,
                adapt=dict(alpha=0.25, lo=0.05, hi=0.45))
    assert rx.costs.reshape(iters, B * K).tobytes() == wx["costs"].tobytes() and mx.tobytes() == wx["mu"].tobytes()
    assert sx.tobytes() == wx["stats"].tobytes() and sdx.shape == (B, M, A) and sdx.tobytes() == wx["sd"].tobytes()
    assert rx.best_index.tobytes() == wx["index"].tobytes() and rx.first_action.tobytes() == wx["first"].tobytes()
    eng.close()
    one.close()
    label = f"mppi/{name}/{kernel}/{kind}/rho={rho}"
    _check_populations(n, states, want, B, K, H, M, kind, seed, off, rho, label)
    for it, rec in enumerate(want["its"]):
        for b in range(B):
            cols = slice(b * K, (b + 1) * K)
            _check(f"{label}/it{it}/env{b}", (rec["mu_new"][b], rec["stats"][b]),
                   mppi_ref(rec["costs"][cols], rec["knots"][:, cols], rec["mu"][b], lam), K)


# ------------------------------------------------------------------ 4. knots = H is the stored-array chain of rho
@pytest.mark.parametrize("kind", KINDS)
def test_knots_equal_to_the_horizon_is_the_sampling_path(kind):
    c = CALL
    B, K, H, E, iters, off, alpha, seed = c["B"], c["K"], c["H"], c["E"], c["iters"], c["off"], c["alpha"], 5
    n = net("tanh64")
    states = n.states[:B]
    mu, sd = plans(B, H, 5)
    eng = n.engine("auto", B * K, H)
    for keep in (False, True):
        a = eng.cem_get_actions(states, mu, sd, iters, E, alpha, seed, off, True, rho=0.5, keep_elites=keep)
        b = eng.cem_get_actions(states, mu, sd, iters, E, alpha, seed, off, True, rho=0.5, keep_elites=keep, knots=H,
                                knot_interp=kind)
        assert a[0].costs.tobytes() == b[0].costs.tobytes() and a[1].tobytes() == b[1].tobytes()
        assert a[2].tobytes() == b[2].tobytes() and a[0].best_index.tobytes() == b[0].best_index.tobytes()
        assert a[0].best_cost.tobytes() == b[0].best_cost.tobytes() and a[0].first_action.tobytes() == b[0].first_action.tobytes()
    a = eng.mppi_get_actions(states, mu, sd, iters, 0.8, seed, off, True, rho=0.5)
    b = eng.mppi_get_actions(states, mu, sd, iters, 0.8, seed, off, True, rho=0.5, knots=H, knot_interp=kind)
    assert a[0].costs.tobytes() == b[0].costs.tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2].tobytes() == b[2].tobytes() and a[0].best_index.tobytes() == b[0].best_index.tobytes()
    assert a[0].first_action.tobytes() == b[0].first_action.tobytes()
    eng.close()


# ------------------------------------------------------------------ 5. the MPPI extensions' blocks on a knot array
@pytest.mark.parametrize("K", [65, 400])
def test_mppi_extension_blocks_in_knot_space(K):
    from bc_mpc_amd.mppi_update import augmented, control_cost, sigma_step
    torch, dev = _t()
    B, H, M, lam, weight = 3, 7, 3, 2.0, 1.5
    eng = sample_engine(A, H)                                    # horizon 7: the blocks are told steps = 3
    st = _stream()
    rs = np.random.RandomState(K)
    mu = rs.uniform(-0.6, 0.6, (B, M, A))
    sd = rs.uniform(0.1, 0.5, (B, M, A))
    th = np.concatenate([np.clip(mu[b][:, None] + sd[b][:, None] * rs.standard_normal((M, K, A)), -1, 1)
                         for b in range(B)], axis=1)
    costs = 3.0 * rs.standard_normal(B * K)
    costs[[1, K - 2]] = [np.nan, np.inf]
    d_th, d_mu, d_sd, d_costs = _dev(th), _dev(mu), _dev(sd), _dev(costs)
    d_scores = torch.full((B * K + 8,), -7.5, dtype=torch.float64, device=dev)
    eng.mppi_control_cost_steps_async(d_costs.data_ptr(), d_th.data_ptr(), B, K, d_mu.data_ptr(), d_sd.data_ptr(), weight,
                                      d_scores.data_ptr(), M, st)
    got = d_scores.cpu().numpy()
    want = np.concatenate([augmented(costs[b * K:(b + 1) * K], control_cost(th[:, b * K:(b + 1) * K], mu[b], sd[b]), weight)
                           for b in range(B)])
    assert (got[B * K:] == -7.5).all()
    _same_bits(got[:B * K], want, "control cost on the knots")
    mu_new = rs.uniform(-0.6, 0.6, (B, M, A))
    d_new = _dev(mu_new)
    d_s = torch.full((B * M * A + 8,), -7.5, dtype=torch.float64, device=dev)

    def run(alpha, lo, hi):
        d_s.fill_(-7.5)
        d_s[:B * M * A].copy_(torch.from_numpy(sd.reshape(-1)))
        eng.mppi_sigma_update_steps_async(d_scores.data_ptr(), d_th.data_ptr(), B, K, lam, d_new.data_ptr(), d_s.data_ptr(),
                                          M, alpha, lo, hi, st)
        out = d_s.cpu().numpy()
        assert (out[B * M * A:] == -7.5).all(), "written past sigma"
        return out[:B * M * A].reshape(B, M, A)

    s = run(0.0, 0.0, None)
    bound = 16.0 * K * EPS * 2.0 * 2.0                           # D = high - low = 2
    for b in range(B):
        ref = _sigma_ref_sq(want[b * K:(b + 1) * K], th[:, b * K:(b + 1) * K], mu_new[b], lam)
        worst = float(np.max(np.abs(s[b] * s[b] - ref))) / bound
        print(f"[K={K} env {b}] sigma'^2: worst ratio to 16 K eps D^2 = {worst:.3e}")
        assert worst <= 1.0 and ref.max() > 1e-4
    assert run(0.3, 0.2, 0.9).tobytes() == sigma_step(sd, s, 0.3, 0.2, 0.9).tobytes()


# ------------------------------------------------------------------ 6. controllers
def _seeds(seed, n):
    return [int(x) for x in np.random.RandomState(seed).randint(0, 2**62, size=n, dtype=np.int64)]


@pytest.mark.parametrize("kind", ["cem", "mppi"])
def test_controllers(kind):
    from bc_mpc_amd import CEMcontroller, MPPIcontroller, cheetah_cost_fn
    from bc_mpc_amd import knots as kn
    n = net("tanh64")
    K, H, B, M = 65, 7, 2, 3
    mid = np.zeros(A)
    kw = dict(horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, seed=9, knots=M)
    if kind == "cem":
        make = lambda: CEMcontroller(_Env(), n.dyn, iterations=3, n_elite=6, **kw)                        # noqa: E731
        interp = "linear"
    else:
        make = lambda: MPPIcontroller(_Env(), n.dyn, iterations=2, temperature=0.8, knot_interp="hold", **kw)   # noqa: E731
        interp = "hold"
    ctrl = make()
    one = n.engine("auto", K, H)
    seeds = _seeds(9, 2)
    prev = None
    for step in range(2):                                       # two consecutive steps, warm-started in knot space
        mu0, sd0 = ctrl.initial_distribution()
        assert mu0.shape == sd0.shape == (M, A)
        if prev is not None:
            assert mu0.tobytes() == kn.shift_plan(prev, H, interp, mid).tobytes()
        a = ctrl.get_action(n.states[step])
        if kind == "cem":
            r, mu, sd = one.cem_get_action(n.states[step], mu0, sd0, 3, 6, ctrl.alpha, seeds[step], knots=M, knot_interp=interp)
            assert np.array_equal(a, r.first_action) and np.array_equal(ctrl.last_sigma, sd)
        else:
            r, mu, stats = one.mppi_get_action(n.states[step], mu0, sd0, 2, 0.8, seeds[step], knots=M, knot_interp=interp)
            assert np.array_equal(a, mu[0]) and ctrl.last_ess == float(stats.ess)
        assert ctrl.last_mu.shape == (M, A) and np.array_equal(ctrl.last_mu, mu)
        assert ctrl.last_cost == r.best_cost and ctrl.last_position == r.best_index
        assert ctrl.last_plan.shape == (H, A)
        assert ctrl.last_plan.tobytes() == kn.expand_plan(ctrl.last_mu, H, interp, LOW, HIGH).tobytes()
        prev = mu
    # get_actions: every row is the single controller's answer (K candidates each, one seed per call); reset([b])
    # recentres plan b only
    many = make()
    singles = [make() for _ in range(B)]
    got = many.get_actions(n.states[:B])
    assert many.last_mu.shape == (B, M, A) and many.last_plan.shape == (B, H, A)
    seed0 = _seeds(9, 1)[0]
    eng = n.engine("auto", B * K, H)
    mu0 = np.zeros((B, M, A))
    sd0 = np.full((B, M, A), 0.5)
    if kind == "cem":
        r, mu, _ = eng.cem_get_actions(n.states[:B], mu0, sd0, 3, 6, many.alpha, seed0, knots=M, knot_interp=interp)
        assert np.array_equal(got, r.first_action)
    else:
        r, mu, _ = eng.mppi_get_actions(n.states[:B], mu0, sd0, 2, 0.8, seed0, knots=M, knot_interp=interp)
        assert np.array_equal(got, mu[:, 0])
    assert np.array_equal(many.last_mu, mu)
    for b in range(B):
        assert many.last_plan[b].tobytes() == kn.expand_plan(mu[b], H, interp, LOW, HIGH).tobytes()
    # a batch of one environment is the single controller's answer: the same seed, K candidates from offset 0, and
    # engines of the same size (the rows of a larger batch sit at their own candidate offsets b * K)
    a0 = singles[0].get_action(n.states[0])
    rows = singles[1].get_actions(n.states[:1])
    assert np.array_equal(rows[0], a0) and np.array_equal(singles[1].last_mu[0], singles[0].last_mu)
    assert np.array_equal(singles[1].last_plan[0], singles[0].last_plan)
    many.reset([1])
    mu1, _ = many.batch_initial_distribution(B)
    assert mu1[0].tobytes() == kn.shift_plan(mu[0], H, interp, mid).tobytes()
    assert mu1[1].tobytes() == np.zeros((M, A)).tobytes()
    for e in (one, eng, ctrl._engine, many._batch_engine, singles[0]._engine, singles[1]._batch_engine):
        e.close()


# ------------------------------------------------------------------ 7. refusals on a live engine
def test_refusals_on_a_live_engine():
    from bc_mpc_amd import _lib
    n = net("tanh64")
    K, H, M = 64, 3, 2
    eng = n.engine("auto", K, H)
    lib, h = eng._lib, eng._h
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
    st, mu, sd = np.ascontiguousarray(n.states[:1]), np.zeros((1, M, A)), np.full((1, M, A), 0.5)
    out, stats = (_lib.Result * 1)(), (_lib.MppiStats * 1)()
    cem, mp = _lib.Cem(2, 4, 0.1, 0), _lib.Mppi(1, 1.0, 0)
    seqs = np.zeros((1, 2, H, A))

    def calls(kn, prop=None):
        k = ctypes.byref(kn)
        q = ctypes.byref(prop) if prop is not None else None
        return [lib.bcmpc_cem_get_action_k(h, dp(st), ctypes.byref(cem), None, q, k, 1, dp(mu.copy()), dp(sd.copy()), out),
                lib.bcmpc_cem_get_actions_batch_k(h, dp(st), 1, ctypes.byref(cem), None, q, k, 1, 0, dp(mu.copy()),
                                                  dp(sd.copy()), out, None),
                lib.bcmpc_mppi_get_action_k(h, dp(st), ctypes.byref(mp), None, None, q, k, 1, dp(mu.copy()), dp(sd.copy()),
                                            out, stats),
                lib.bcmpc_mppi_get_actions_batch_k(h, dp(st), 1, ctypes.byref(mp), None, None, q, k, 1, 0, dp(mu.copy()),
                                                   dp(sd.copy()), out, stats, None)]

    def default_ok():
        m, s, res = np.zeros((H, A)), np.full((H, A), 0.5), _lib.Result()
        return lib.bcmpc_cem_get_action(h, dp(st), ctypes.byref(cem), 1, dp(m), dp(s), ctypes.byref(res)) == _lib.OK

    for count in (H + 1, -1):
        assert calls(_lib.Knots(count, 1)) == [_lib.ERR_ARG] * 4 and b"knots: count" in lib.bcmpc_last_error()
        assert default_ok()
    for kind in (3, -1):
        assert calls(_lib.Knots(M, kind)) == [_lib.ERR_ARG] * 4 and b"knots: kind" in lib.bcmpc_last_error()
        assert default_ok()
    prop = _lib.Proposals(seqs.ctypes.data, 2, 0, 0, 0, 0)
    assert calls(_lib.Knots(M, 1), prop) == [_lib.ERR_UNSUPPORTED] * 4
    assert b"knots with proposals" in lib.bcmpc_last_error()
    assert default_ok()
    assert calls(_lib.Knots(M, 1)) == [_lib.OK] * 4
    # count == 0 forwards to the _p entry points: the proposals run, the plans are [H][A]
    muH, sdH = np.zeros((1, H, A)), np.full((1, H, A), 0.5)
    assert lib.bcmpc_cem_get_action_k(h, dp(st), ctypes.byref(cem), None, ctypes.byref(prop), ctypes.byref(_lib.Knots(0, 0)),
                                      1, dp(muH), dp(sdH), out) == _lib.OK
    # the blocks' own refusals
    torch, dev = _t()
    d = torch.zeros(H * K * A, dtype=torch.float64, device=dev)
    p = d.data_ptr()
    assert lib.bcmpc_plan_sample_knots_async(h, p, p, 1, K, 1, 0, 0, 0.0, None, None, 0, H + 1, 1, p, p, None) == _lib.ERR_ARG
    assert lib.bcmpc_plan_sample_knots_async(h, p, p, 1, K, 1, 0, 0, 0.0, None, None, 0, M, 3, p, p, None) == _lib.ERR_ARG
    assert lib.bcmpc_plan_sample_knots_async(h, p, p, 1, K, 1, 0, 0, 1.0, None, None, 0, M, 1, p, p, None) == _lib.ERR_ARG
    assert lib.bcmpc_plan_sample_knots_async(h, p, p, 1, K, 1, 0, 0, 0.0, p, None, 4, M, 1, p, p, None) == _lib.ERR_ARG
    assert lib.bcmpc_plan_keep_steps_async(h, p, p, p, 1, K, 0, 4, p, p, 0, None) == _lib.ERR_ARG
    assert lib.bcmpc_plan_keep_steps_async(h, p, p, p, 1, K, 0, 4, p, p, H + 1, None) == _lib.ERR_ARG
    assert lib.bcmpc_cem_refit_batch_steps_async(h, p, p, 1, 4, 1, 0, 0.1, p, p, None, K, 0, M, None) == _lib.ERR_ARG
    assert default_ok()
    with pytest.raises(NotImplementedError, match="knots with proposals"):
        eng.cem_get_action(st[0], mu[0], sd[0], 2, 4, 0.1, 1, knots=M, proposals=seqs[0])
    with pytest.raises(ValueError, match="knots"):
        eng.mppi_get_action(st[0], mu[0], sd[0], 1, 1.0, 1, knots=H + 1)
    eng.close()

"""Terminal value on the GPU (csrc/terminal_value.hip, bcmpc_set_terminal_value).

The definition is value.terminal_values (NumPy f32); a GPU f32 MLP cannot be bit-equal to BLAS, so the kernel is
held to the two bars of value.py / value_cases.py -- (a) |v - v_f64| <= E_k per candidate, the derived running
error bound; (b) for K >= 64 the RMS of v - v_f64 at most 4x that of the strictly sequential NumPy f32
evaluation -- and to exact statements wherever they exist: the NaN pattern, obz bit for bit (through an
identity-like net), costs_out == costs_in + weight * float64(values_out) bit for bit.  In the chain everything
is exact: the costs of an engine with a value equal the costs of a plain engine plus weight * the kernel's own
values of that engine's final trajectory row.

Figures observed on an MI355X (worst |dv| / E_k, worst RMS ratio over all 60 nets x 8 K): see
profiles/terminal_value_accuracy.json, written by this module when BCMPC_TV_ACCURACY_JSON names a path.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import value_cases as vc
from test_gpu_term_cost import (_dev, _empty, _record, _stream, _t, cem_step, mppi_step, net, plans, same)

pytestmark = pytest.mark.gpu

S, A, HID = 20, 6, 64
W = -0.75
KERNELS = ["solo", "group4", "split2", "team"]
ACCURACY = {}


def _f32(n):
    torch, dev = _t()
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev)


@functools.lru_cache(maxsize=None)
def critic(seed=0):
    return vc.make_spec(S, HID, 2, seed=seed)


@functools.lru_cache(maxsize=None)
def value_engine(kernel, K, H, cost="cheetah"):
    """An engine of its own (never one of test_gpu_term_cost's) carrying critic() at weight W."""
    from bc_mpc_amd.cost_functions import cheetah_terms
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    nt = net(S, A)
    eng = RolloutEngine(S, A, HID, 2, "tanh", False, H, K, device=0, kernel=kernel, cost=cost)
    if kernel != "auto":
        assert eng.info()["kernel"] == kernel
    eng.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, nt.w.activation), nt.norm, 1)
    if cost == "terms":
        eng.set_cost_terms(cheetah_terms())
    eng.set_terminal_value(critic(), W, 1)
    return eng


def plain_engine(kernel, K, H, cost="cheetah"):
    from bc_mpc_amd.cost_functions import cheetah_terms
    return net(S, A).engine(kernel, K, H, cost=cost, terms=cheetah_terms() if cost == "terms" else None)


def kernel_values(eng, rows, K):
    """terminal_value_async on device rows [K, S] (dense) -> f32[K]."""
    d_v = _f32(K)
    eng.terminal_value_async(rows.data_ptr(), K, d_values=d_v.data_ptr(), stream=_stream())
    return d_v.cpu().numpy()


def plain_plus_value(plain, veng, d_state, stride, d_acts, seed, off, weight=W):
    """The reference of every chain test: a plain engine's costs and trajectory from ONE launch, the value
    engine's kernel on the trajectory's last row, the definition's f64 add."""
    from bc_mpc_amd import value
    K, H = plain.num_paths, plain.horizon
    d_costs, d_traj = _empty(K), _empty(H + 1, K, S)
    plain.rollout_async(d_state.data_ptr(), stride, d_acts.data_ptr() if d_acts is not None else None, seed, off,
                        d_costs.data_ptr(), d_traj.data_ptr(), None, _stream())
    v = kernel_values(veng, d_traj[H], K)
    plain.check_status()
    costs0 = d_costs.cpu().numpy()
    assert np.isfinite(costs0).all() and np.isfinite(v).all()
    return value.add_to_costs(costs0, v, weight), v, costs0


# ------------------------------------------------------------------ 1. the kernel alone
@functools.lru_cache(maxsize=None)
def alone_engine():
    """The kernel needs no weights: the engine lends its device and stream (a net over another state_dim than
    the engine's runs through terminal_value_async alone)."""
    from bc_mpc_amd.engine import RolloutEngine
    return RolloutEngine(S, A, HID, 2, "tanh", False, 3, 64, device=0, cost="cheetah")


@pytest.mark.parametrize("Sv,hidden,L", vc.CASES)
def test_kernel_alone_on_hand_made_states(Sv, hidden, L):
    torch, dev = _t()
    spec, cases = vc.case(Sv, hidden, L)
    eng = alone_engine()
    weight = 1.0 - 0.125 * L
    eng.set_terminal_value(spec, weight, 1000 * Sv + 10 * hidden + L)
    st = _stream()
    stride = Sv + 3
    for K, c in cases.items():
        label = f"S={Sv} hidden={hidden} L={L} K={K}"
        rows = np.full((K, stride), np.nan)
        rows[:, :Sv] = c.states
        d_rows = _dev(rows)
        costs_in = np.random.RandomState(K).standard_normal(K + 8) * 100.0
        d_v1, d_v2 = _f32(K + 8), _f32(K + 8)
        d_c2, d_c3 = _dev(costs_in), _dev(costs_in)
        eng.terminal_value_async(d_rows.data_ptr(), K, d_values=d_v1.data_ptr(), row_stride=stride, stream=st)
        eng.terminal_value_async(d_rows.data_ptr(), K, d_values=d_v2.data_ptr(), d_costs=d_c2.data_ptr(),
                                 row_stride=stride, stream=st)
        eng.terminal_value_async(d_rows.data_ptr(), K, d_costs=d_c3.data_ptr(), row_stride=stride, stream=st)
        v1, v2, c2, c3 = d_v1.cpu().numpy(), d_v2.cpu().numpy(), d_c2.cpu().numpy(), d_c3.cpu().numpy()
        assert np.isnan(v1[K:]).all() and np.isnan(v2[K:]).all(), f"{label}: values written past K"
        assert np.array_equal(c2[K:], costs_in[K:]) and np.array_equal(c3[K:], costs_in[K:]), f"{label}: costs past K"
        same(v2[:K], v1[:K], f"{label}: values with / without the cost add")
        worst, ratio = c.check(v1[:K], label)
        with np.errstate(invalid="ignore"):
            want = costs_in[:K] + np.float64(weight) * v1[:K].astype(np.float64)
        same(c2[:K], want, f"{label}: costs_out")
        same(c3[:K], want, f"{label}: costs_out without values")
        ACCURACY[label] = {"max_err_over_bound": worst, "rms_ratio": ratio}
    if K >= 15:
        assert np.isnan(v1[1]) and np.isnan(v1[9]) and np.isfinite(v1[2:9]).all()
    out = os.environ.get("BCMPC_TV_ACCURACY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump(ACCURACY, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("Sv", vc.SS)
def test_obz_is_bit_identical_through_an_identity_like_net(Sv):
    from bc_mpc_amd import value
    eng = alone_engine()
    states = vc.identity_states(Sv)
    K = states.shape[0]
    d_rows = _dev(states)
    for i, d in enumerate(sorted({0, Sv // 2, Sv - 1})):
        spec = vc.identity_like(Sv, d)
        eng.set_terminal_value(spec, -1.0, 50000 + 100 * Sv + i)
        got = kernel_values(eng, d_rows, K)
        same(got, value.observe(spec, states)[:, d], f"S={Sv} dim {d}")
        same(got, value.terminal_values(spec, states), f"S={Sv} dim {d}: the definition")


def test_setter_states_and_refusals():
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    nt = net(S, A)
    eng = RolloutEngine(S, A, HID, 2, "tanh", False, 3, 16, device=0, cost="cheetah")
    try:
        eng.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, "tanh"), nt.norm, 1)
        d = _empty(16 * S)
        with pytest.raises(_lib.BcmpcError, match="bcmpc_set_terminal_value has not been called"):
            eng.terminal_value_async(d.data_ptr(), 16, d_costs=d.data_ptr())
        assert "+value" not in eng.info()["layout"]
        eng.set_terminal_value(critic(), W, 7)
        assert eng.info()["layout"].endswith("+value") and eng.terminal_value == (critic(), W, 7)
        with pytest.raises(ValueError, match="d_values or d_costs_inout"):
            eng.terminal_value_async(d.data_ptr(), 16)
        with pytest.raises(ValueError, match="K must be >= 1"):
            eng.terminal_value_async(d.data_ptr(), 0, d_costs=d.data_ptr())
        with pytest.raises(ValueError, match="row_stride"):
            eng.terminal_value_async(d.data_ptr(), 4, d_costs=d.data_ptr(), row_stride=S - 1)
        with pytest.raises(ValueError, match="terminal value"):
            eng.get_action_numpy_stream(nt.states[0], nt.low, nt.high, 16, return_costs=True)
        # a net over another state_dim: the kernel alone takes it, the rollout entries do not
        eng.set_terminal_value(vc.make_spec(17, 16, 1), W, 8)
        with pytest.raises(ValueError, match="17 state dims"):
            eng.get_action(nt.states[0])
        eng.set_terminal_value(None)
        assert "+value" not in eng.info()["layout"] and eng.terminal_value is None
        eng.get_action(nt.states[0])
    finally:
        eng.close()
    for kw, msg in ((dict(cost="none"), "BCMPC_COST_NONE"), (dict(cost="reward", model="reward"), "reward"),
                    (dict(policy_hidden=64, policy_layers=2), "fused policy")):
        other = RolloutEngine(S, A, 128, 2, "tanh", False, 3, 16, device=0, **kw)
        try:
            with pytest.raises(ValueError, match=msg):
                other.set_terminal_value(critic(), W, 1)
        finally:
            other.close()


# ------------------------------------------------------------------ 2. the chain
@pytest.mark.parametrize("cost", ["cheetah", "terms"])
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kernel", KERNELS)
def test_costs_differ_from_the_plain_engine_by_exactly_the_value(kernel, H, cost):
    from bc_mpc_amd import _lib
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    nt = net(S, A)
    K, seed, off = 400, 0xA11CE + H, 3000
    plain, veng = plain_engine(kernel, K, H, cost), value_engine(kernel, K, H, cost)
    assert veng.info()["layout"].endswith("+value") and "+value" not in plain.info()["layout"]
    state = nt.states[1]
    d_state = _dev(state)
    want, v, costs0 = plain_plus_value(plain, veng, d_state, 0, None, seed, off)
    d_costs = _empty(K)
    d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    veng.rollout_async(d_state.data_ptr(), 0, None, seed, off, d_costs.data_ptr(), None, d_res.data_ptr(), _stream())
    got = d_costs.cpu().numpy()
    veng.check_status()
    same(got, want, f"{kernel} H={H} {cost}: rollout_async")
    assert not np.array_equal(got, costs0) and len(np.unique(v)) > K // 2
    acts = orc.device_rng_actions(seed, off, K, H, nt.low, nt.high)
    index, best_cost, first = _record(d_res, A)
    best = int(np.argmin(want))
    assert index == off + best and best_cost == want[best] and np.array_equal(first, acts[0, best])
    # the synchronous call: the trajectory stays in the engine's scratch
    res = veng.get_action(state, None, seed=seed, cand_offset=off, return_costs=True)
    same(res.costs, want, f"{kernel} H={H} {cost}: get_action")
    assert res.best_index == off + best and res.best_cost == want[best] and np.array_equal(res.first_action, acts[0, best])
    assert veng.last_terminal_values([best])[0] == v[best]
    # a caller's trajectory buffer and explicit actions
    d_traj = _empty(H + 1, K, S)
    d_acts = _dev(acts)
    d_costs.fill_(float("nan"))
    veng.rollout_async(d_state.data_ptr(), 0, d_acts.data_ptr(), 0, 0, d_costs.data_ptr(), d_traj.data_ptr(), None,
                       _stream())
    same(d_costs.cpu().numpy(), want, f"{kernel} H={H} {cost}: explicit actions, caller's trajectory")
    same(kernel_values(veng, d_traj[H], K), v, "the caller's trajectory row H")


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kernel", KERNELS)
def test_get_actions_with_four_environments(kernel, H):
    torch, dev = _t()
    nt = net(S, A)
    B, K, seed, off = 4, 100, 0xBA7C4 + H, 500
    plain, veng = plain_engine(kernel, B * K, H), value_engine(kernel, B * K, H)
    states = np.stack([nt.states[b % 3] + 0.01 * b for b in range(B)])
    tiled = _dev(np.repeat(states, K, axis=0))                           # column c = b K + j starts from states[b]
    want, v, _ = plain_plus_value(plain, veng, tiled, S, None, seed, off)
    res = veng.get_actions(states, None, seed=seed, cand_offset=off, return_costs=True)
    same(res.costs.reshape(-1), want, f"{kernel} H={H}: get_actions")
    for b in range(B):
        best = int(np.argmin(want[b * K:(b + 1) * K]))
        assert res.best_index[b] == off + b * K + best and res.best_cost[b] == want[b * K + best]
    assert len({c.tobytes() for c in res.costs}) == B


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kernel", KERNELS)
def test_ensemble_members_add_the_value_of_their_own_final_state(kernel, H):
    from bc_mpc_amd import ensemble
    from bc_mpc_amd.engine import MLPSpec
    from oracle import mpc_oracle as orc
    nt = net(S, A)
    E, K, seed = 3, 400, 0xE5 + H
    ws = [orc.synthetic_weights(S, A, HID, 2, "tanh", False, seed_base=1000 + 100 * e) for e in range(E)]
    ens = ensemble.EnsembleEngine(E, S, A, HID, 2, "tanh", False, H, K, device=0, cost="cheetah", kernel=kernel)
    plain, veng = plain_engine(kernel, K, H), value_engine(kernel, K, H)
    try:
        for e, w in enumerate(ws):
            ens.set_weights(e, MLPSpec(w.kernels, w.biases, w.activation), nt.norm, 1)
        ens.set_terminal_value(critic(), W, 1)
        assert ens.info()["layout"].endswith("+value")
        state = nt.states[2]
        d_state = _dev(state)
        rows = []
        for e, w in enumerate(ws):                                      # member e alone, on the plain engine
            plain.set_weights(MLPSpec(w.kernels, w.biases, w.activation), nt.norm, 100 + e)
            rows.append(plain_plus_value(plain, veng, d_state, 0, None, seed, 0)[0])
        rows = np.stack(rows)
        assert len({r.tobytes() for r in rows}) == E
        for rule in ("mean", "worst"):
            ens.set_rule(rule, 0.0)
            res = ens.get_action(state, None, seed=seed, return_costs=True, return_member_costs=True)
            same(res.member_costs, rows, f"{kernel} H={H} {rule}: member rows")
            want = ensemble.combine(rows, rule)
            same(res.costs, want, f"{kernel} H={H} {rule}: combined")
            best = int(np.argmin(want))
            assert res.best_index == best and res.best_cost == want[best]
    finally:
        ens.close()
        plain.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, nt.w.activation), nt.norm, 1)


def composed_iteration(plain, veng, nt, state, mu, sd, seed, it, off):
    """Iteration `it` from the stream-ordered blocks: the sampled actions rolled out on the PLAIN engine as an
    explicit array (costs + trajectory), terminal_value_async inserted on the cost vector in place; the value
    engine's cem_rollout_async (actions regenerated, value in its chain) must give the same bits."""
    from oracle import mpc_oracle as orc
    K, H = plain.num_paths, plain.horizon
    acts = orc.cem_actions(seed, it, off, K, H, mu, sd, nt.low, nt.high)
    d_state, d_acts, d_costs, d_traj = _dev(state), _dev(acts), _empty(K), _empty(H + 1, K, S)
    st = _stream()
    plain.rollout_async(d_state.data_ptr(), 0, d_acts.data_ptr(), seed, off, d_costs.data_ptr(), d_traj.data_ptr(),
                        None, st)
    veng.terminal_value_async(d_traj[H].data_ptr(), K, d_costs=d_costs.data_ptr(), stream=st)
    costs = d_costs.cpu().numpy()
    d_mu, d_sd, d_c2 = _dev(mu), _dev(sd), _empty(K)
    veng.cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sd.data_ptr(), seed, it, off, off + K,
                           d_c2.data_ptr(), None, False, st)
    same(d_c2.cpu().numpy(), costs, f"it={it} off={off}: cem_rollout_async on the value engine")
    veng.check_status()
    return costs, acts, d_costs


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kernel", ["group4", "split2", "team"])
def test_cem_and_mppi_equal_the_composed_chain_and_the_batched_planners_the_single_calls(kernel, H):
    nt = net(S, A)
    B, K, seed, off, iters, E, alpha, lam = 4, 100, 0x5EED5 + H, 1000, 2, 7, 0.1, 0.7
    plain, one, many = plain_engine(kernel, K, H), value_engine(kernel, K, H), value_engine(kernel, B * K, H)
    states = np.stack([nt.states[b % 3] + 0.01 * b for b in range(B)])
    mu0, sd0 = plans(B, H, A)
    rc, mu_c, sd_c = many.cem_get_actions(states, mu0, sd0, iters, E, alpha, seed, cand_offset=off, return_costs=True)
    rm, mu_m, st_m = many.mppi_get_actions(states, mu0, sd0, iters, lam, seed, cand_offset=off, return_costs=True)
    for b in range(B):
        ob = off + b * K
        for planner, r, mu_out in (("cem", rc, mu_c), ("mppi", rm, mu_m)):
            mu, sd, cat, acts_all = mu0[b], sd0[b], [], []
            for it in range(iters):
                costs, acts, d_costs = composed_iteration(plain, one, nt, states[b], mu, sd, seed, it, ob)
                same(r.costs[it, b], costs, f"{kernel} {planner} env {b} it {it}")
                cat.append(costs)
                acts_all.append(acts)
                if planner == "cem":
                    mu, sd = cem_step(one, d_costs, mu, sd, seed, it, ob, E, alpha)
                else:
                    mu, stats = mppi_step(one, d_costs, mu, sd, seed, it, ob, lam)
            assert mu_out[b].tobytes() == mu.tobytes(), f"{planner} env {b}: plan"
            if planner == "cem":
                assert sd_c[b].tobytes() == sd.tobytes()
            else:
                assert st_m[b].tobytes() == stats
            cat = np.concatenate(cat)
            best = int(np.argmin(cat))
            assert r.best_index[b] == best and r.best_cost[b] == cat[best]
            assert np.array_equal(r.first_action[b], acts_all[best // K][0, best % K])
    # the single calls (cand_offset 0) against the chain composed from the blocks
    state = states[0]
    for planner in ("cem", "mppi"):
        mu, sd, cat, acts_all = mu0[0], sd0[0], [], []
        for it in range(iters):
            costs, acts, d_costs = composed_iteration(plain, one, nt, state, mu, sd, seed, it, 0)
            cat.append(costs)
            acts_all.append(acts)
            if planner == "cem":
                mu, sd = cem_step(one, d_costs, mu, sd, seed, it, 0, E, alpha)
            else:
                mu, stats = mppi_step(one, d_costs, mu, sd, seed, it, 0, lam)
        cat = np.concatenate(cat)
        best = int(np.argmin(cat))
        if planner == "cem":
            res, mu1, sd1 = one.cem_get_action(state, mu0[0], sd0[0], iters, E, alpha, seed)
            assert mu1.tobytes() == mu.tobytes() and sd1.tobytes() == sd.tobytes()
        else:
            res, mu1, st1 = one.mppi_get_action(state, mu0[0], sd0[0], iters, lam, seed)
            assert mu1.tobytes() == mu.tobytes() and bytes(st1) == stats
        assert res.best_index == best and res.best_cost == cat[best], planner
        assert np.array_equal(res.first_action, acts_all[best // K][0, best % K])


# ------------------------------------------------------------------ 3. further cases
@pytest.mark.parametrize("kernel", KERNELS)
def test_weight_zero_and_removal_restore_the_plain_engine(kernel):
    nt = net(S, A)
    K, H, seed = 400, 5, 4242
    plain, veng = plain_engine(kernel, K, H), value_engine(kernel, K, H)
    state = nt.states[0]
    want = plain.get_action(state, None, seed=seed, return_costs=True)
    try:
        veng.set_terminal_value(critic(), 0.0, 1)                       # same version: only the weight moves
        got = veng.get_action(state, None, seed=seed, return_costs=True)
        same(got.costs, want.costs, f"{kernel}: weight 0")
        assert got.best_index == want.best_index and got.best_cost == want.best_cost
        veng.set_terminal_value(None)
        assert "+value" not in veng.info()["layout"]
        got = veng.get_action(state, None, seed=seed, return_costs=True)
        same(got.costs, want.costs, f"{kernel}: value removed")
        lean_v, lean_p = veng.get_action(state, None, seed=seed), plain.get_action(state, None, seed=seed)
        assert (lean_v.best_index, lean_v.best_cost) == (lean_p.best_index, lean_p.best_cost)    # (team: fused tail)
        assert np.array_equal(lean_v.first_action, lean_p.first_action)
    finally:
        veng.set_terminal_value(critic(), W, 1)
    back = veng.get_action(state, None, seed=seed, return_costs=True)
    assert not np.array_equal(back.costs, want.costs)


def test_a_team_that_gives_up_reruns_with_the_same_value(monkeypatch):
    """BCMPC_TEAM_SPINS=-1 (the suite's hook: the team launch is skipped and reported as a team that gave up): the
    synchronous call reruns on the fallback engine, which must carry the same net and weight -- its costs are those
    of a split1 value engine (the layout the fallback takes at this K), bit for bit; a new weight and the removal
    reach the fallback engine that now exists."""
    nt = net(S, A)
    K, H, seed = 37, 5, 77
    team, ref, plain = value_engine("team", K, H), value_engine("split1", K, H), plain_engine("split1", K, H)
    state = nt.states[1]
    want = ref.get_action(state, None, seed=seed, return_costs=True)
    before = team.team_reruns

    def rerun():
        monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
        try:
            return team.get_action(state, None, seed=seed, return_costs=True)
        finally:
            monkeypatch.delenv("BCMPC_TEAM_SPINS")
    got = rerun()
    assert team.team_reruns == before + 1
    same(got.costs, want.costs, "fallback engine")
    assert got.best_index == want.best_index and np.array_equal(got.first_action, want.first_action)
    try:
        team.set_terminal_value(critic(), -0.25, 1)
        ref.set_terminal_value(critic(), -0.25, 1)
        same(rerun().costs, ref.get_action(state, None, seed=seed, return_costs=True).costs, "fallback, new weight")
        team.set_terminal_value(None)
        same(rerun().costs, plain.get_action(state, None, seed=seed, return_costs=True).costs, "fallback, value removed")
    finally:
        team.set_terminal_value(critic(), W, 1)
        ref.set_terminal_value(critic(), W, 1)
    same(rerun().costs, want.costs, "fallback engine, value set again")


def test_a_value_that_changes_the_winner_against_the_oracle():
    """A critic with a large weight on one state dimension: the argmin moves away from the plain engine's, to
    the candidate the oracle composition (oracle rollout costs plus the definition) names."""
    from bc_mpc_amd import value
    from bc_mpc_amd.value import ValueSpec
    from oracle import mpc_oracle as orc
    nt = net(S, A)
    K, H, seed = 400, 5, 777
    w0 = np.zeros((S, 4), np.float32)
    w0[9, 0] = 8.0                                                      # V = 40 tanh(8 obz_9): one joint's state
    spec = ValueSpec([w0, np.array([[40.0], [0], [0], [0]], np.float32)], [np.zeros(4, np.float32), np.zeros(1, np.float32)],
                     np.zeros(S, np.float32), np.ones(S, np.float32))
    plain, veng = plain_engine("auto", K, H), value_engine("auto", K, H)
    state = nt.states[0]
    acts = orc.device_rng_actions(seed, 0, K, H, nt.low, nt.high)
    o_costs, o_traj = orc.rollout(nt.dyn, state, acts)
    o_total = value.add_to_costs(o_costs, value.terminal_values(spec, o_traj[H]), -1.0)
    try:
        veng.set_terminal_value(spec, -1.0, 99)
        got = veng.get_action(state, None, seed=seed, return_costs=True)
    finally:
        veng.set_terminal_value(critic(), W, 1)
    base = plain.get_action(state, None, seed=seed)
    o_best = int(np.argmin(o_total))
    margin = np.partition(o_total, 1)[1] - o_total[o_best]
    assert margin > 1e-3, "the oracle's winner is not clear enough for an f32 rollout to reproduce"
    assert np.max(np.abs(got.costs - o_total)) < 1e-3 + 1e-5 * np.max(np.abs(o_total))
    assert got.best_index == o_best != base.best_index == int(np.argmin(o_costs))
    assert np.array_equal(got.first_action, acts[0, o_best])


def test_rollout_async_on_a_value_engine_replays_in_a_graph():
    """One stream, no parallel branches; nothing in the chain allocates, so the replay gives the eager bits, also
    after the state changed."""
    from bc_mpc_amd import _lib
    torch, dev = _t()
    nt = net(S, A)
    K, H, seed = 400, 5, 31337
    eng = value_engine("group4", K, H)
    d_state = _dev(nt.states[0])
    d_costs = _empty(K)
    d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)

    def launch(stream):
        eng.rollout_async(d_state.data_ptr(), 0, None, seed, 0, d_costs.data_ptr(), None, d_res.data_ptr(), stream)
    eager = {}
    for i in (0, 1):
        d_state.copy_(_dev(nt.states[i]))
        launch(_stream())
        eager[i] = (d_costs.cpu().numpy(), d_res.cpu().numpy().tobytes())
    assert not np.array_equal(eager[0][0], eager[1][0])
    side = torch.cuda.Stream(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        d_state.copy_(_dev(nt.states[0]))
        side.synchronize()
        graph.capture_begin(capture_error_mode="thread_local")
        launch(side.cuda_stream)
        graph.capture_end()
    for i in (0, 1, 0):
        d_state.copy_(_dev(nt.states[i]))
        d_costs.fill_(float("nan"))
        torch.cuda.synchronize(dev)
        graph.replay()
        torch.cuda.synchronize(dev)
        same(d_costs.cpu().numpy(), eager[i][0], f"replay of state {i}")
        assert d_res.cpu().numpy().tobytes() == eager[i][1]


# ------------------------------------------------------------------ 4. controllers
class _Box:
    def __init__(self, n):
        self.low, self.high, self.shape = -np.ones(n, np.float32), np.ones(n, np.float32), (n,)


class _Env:
    action_space = _Box(A)
    observation_space = _Box(S)


class _Holder:
    """A value container with a version stamp of its own."""

    def __init__(self, spec, version):
        self.spec, self.version = spec, version

    def value_spec(self):
        return self.spec


def test_controllers_answer_what_the_engine_calls_answer():
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller
    from bc_mpc_amd.cost_functions import cheetah_cost_fn
    nt = net(S, A)
    K, H, B = 100, 5, 4
    states = np.stack([nt.states[b % 3] + 0.01 * b for b in range(B)])
    seed_of = lambda s: int(np.random.RandomState(s).randint(0, 2**62, dtype=np.int64))   # noqa: E731
    one, many = value_engine("auto", K, H), value_engine("auto", B * K, H)
    tv = _Holder(critic(), 1)
    kw = dict(horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, terminal_value=tv, terminal_weight=W)
    # random shooting, actions drawn in the kernel
    ctrl = MPCcontroller(_Env(), nt.dyn, rng="device", seed=5, **kw)
    a = ctrl.get_action(states[0])
    r = one.get_action(states[0], None, seed=seed_of(5))
    assert ctrl._engine.info()["layout"].endswith("+value")
    assert np.array_equal(a, r.first_action) and ctrl.last_index == r.best_index and ctrl.last_cost == r.best_cost
    assert ctrl.last_terminal_value == one.last_terminal_values([r.best_index])[0]
    made = ctrl._engine
    # a new weight, then a new version of the net: the same engine answers, with the new objective
    ctrl.terminal_weight = -0.25
    ctrl._seed_rng = np.random.RandomState(5)
    ctrl.get_action(states[0])
    one.set_terminal_value(critic(), -0.25, 1)
    r2 = one.get_action(states[0], None, seed=seed_of(5))
    assert ctrl._engine is made and ctrl.last_cost == r2.best_cost != r.best_cost
    tv.spec, tv.version = critic(1), 2
    ctrl._seed_rng = np.random.RandomState(5)
    ctrl.get_action(states[0])
    one.set_terminal_value(critic(1), -0.25, 2)
    r3 = one.get_action(states[0], None, seed=seed_of(5))
    assert ctrl._engine is made and ctrl.last_cost == r3.best_cost != r2.best_cost
    tv.spec, tv.version = critic(), 1
    one.set_terminal_value(critic(), W, 1)
    # rng="numpy": the reference's draw on the host, uploaded
    ctrl = MPCcontroller(_Env(), nt.dyn, **kw)
    np.random.seed(4242)
    a = ctrl.get_action(states[1])
    ref = np.random.RandomState(4242)
    paths = ref.uniform(_Env.action_space.low, _Env.action_space.high, [H, K, A])
    r = one.get_action(states[1], paths)
    assert np.array_equal(a, paths[0, r.best_index]) and ctrl.last_cost == r.best_cost
    assert ref.get_state()[2] == np.random.get_state()[2] and np.array_equal(ref.get_state()[1], np.random.get_state()[1])
    # get_actions
    ctrl = MPCcontroller(_Env(), nt.dyn, rng="device", seed=6, **kw)
    a = ctrl.get_actions(states)
    r = many.get_actions(states, None, seed=seed_of(6))
    assert np.array_equal(a, r.first_action) and np.array_equal(ctrl.last_index, r.best_index)
    assert np.array_equal(ctrl.last_terminal_value, many.last_terminal_values(r.best_index))
    # CEM and MPPI, single and batched
    cem = CEMcontroller(_Env(), nt.dyn, iterations=2, n_elite=5, seed=7, **kw)
    mu0, sd0 = cem.initial_distribution()
    a = cem.get_action(states[0])
    r, mu, sd = one.cem_get_action(states[0], mu0, sd0, 2, 5, cem.alpha, seed_of(7))
    assert np.array_equal(a, r.first_action) and cem.last_cost == r.best_cost and np.array_equal(cem.last_mu, mu)
    made = cem._engine
    cem.terminal_weight = -0.25
    cem.get_action(states[0])
    assert cem._engine is made and made.terminal_value[1] == -0.25
    cem = CEMcontroller(_Env(), nt.dyn, iterations=2, n_elite=5, seed=8, **kw)
    mu0, sd0 = cem.batch_initial_distribution(B)
    a = cem.get_actions(states)
    r, mu, sd = many.cem_get_actions(states, mu0, sd0, 2, 5, cem.alpha, seed_of(8))
    assert np.array_equal(a, r.first_action) and np.array_equal(cem.last_mu, mu) and np.array_equal(cem.last_sigma, sd)
    mp = MPPIcontroller(_Env(), nt.dyn, temperature=0.7, iterations=2, seed=9, **kw)
    mu0, sd0 = mp.initial_distribution()
    a = mp.get_action(states[0])
    r, mu, stats = one.mppi_get_action(states[0], mu0, sd0, 2, 0.7, seed_of(9))
    assert np.array_equal(a, mu[0]) and mp.last_cost == r.best_cost and mp.last_ess == float(stats.ess)
    mp = MPPIcontroller(_Env(), nt.dyn, temperature=0.7, iterations=2, seed=10, **kw)
    mu0, sd0 = mp.batch_initial_distribution(B)
    a = mp.get_actions(states)
    r, mu, stats = many.mppi_get_actions(states, mu0, sd0, 2, 0.7, seed_of(10))
    assert np.array_equal(a, mu[:, 0]) and np.array_equal(mp.last_cost, r.best_cost)
    for c in (cem, mp):
        assert c._batch_engine.info()["layout"].endswith("+value")
    # without a value the controllers' engines carry none
    ctrl = MPCcontroller(_Env(), nt.dyn, horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, rng="device", seed=5)
    ctrl.get_action(states[0])
    assert "+value" not in ctrl._engine.info()["layout"] and ctrl.last_terminal_value is None


def test_controllers_over_an_ensemble_model():
    """An EnsembleDynamicsModel as dyn_model: the controllers' EnsembleEngine carries the value on every member and
    answers what an EnsembleEngine set up by hand answers."""
    from bc_mpc_amd import CEMcontroller, MPCcontroller
    from bc_mpc_amd.cost_functions import cheetah_cost_fn
    from bc_mpc_amd.engine import MLPSpec
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel, EnsembleEngine
    from oracle import mpc_oracle as orc
    nt = net(S, A)
    E, K, H = 3, 100, 5
    ws = [orc.synthetic_weights(S, A, HID, 2, "tanh", False, seed_base=1000 + 100 * e) for e in range(E)]
    model = EnsembleDynamicsModel(_Env(), E, 2, HID, "tanh", None, nt.norm, 32, 3, 1e-3, device=0, rule="worst")
    for e, w in enumerate(ws):
        model.load_weights(e, w.kernels, w.biases, None, None)
    ens = EnsembleEngine(E, S, A, HID, 2, "tanh", False, H, K, device=0, cost="cheetah")
    try:
        for e, w in enumerate(ws):
            ens.set_weights(e, MLPSpec(w.kernels, w.biases, w.activation), nt.norm, 1)
        ens.set_rule("worst", 0.0)
        ens.set_terminal_value(critic(), W, 1)
        seed_of = lambda s: int(np.random.RandomState(s).randint(0, 2**62, dtype=np.int64))   # noqa: E731
        kw = dict(horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, terminal_value=_Holder(critic(), 1),
                  terminal_weight=W)
        ctrl = MPCcontroller(_Env(), model, rng="device", seed=5, **kw)
        a = ctrl.get_action(nt.states[0])
        r = ens.get_action(nt.states[0], None, seed=seed_of(5))
        assert np.array_equal(a, r.first_action) and ctrl.last_index == r.best_index and ctrl.last_cost == r.best_cost
        v = ctrl.last_terminal_value
        assert v.shape == (E,) and np.array_equal(v, [m.last_terminal_values([r.best_index])[0] for m in ens.members])
        plain = MPCcontroller(_Env(), model, horizon=H, cost_fn=cheetah_cost_fn, num_simulated_paths=K, rng="device",
                              seed=5)
        plain.get_action(nt.states[0])
        assert plain.last_cost != ctrl.last_cost and plain.last_terminal_value is None
        cem = CEMcontroller(_Env(), model, iterations=2, n_elite=5, seed=7, **kw)
        mu0, sd0 = cem.initial_distribution()
        a = cem.get_action(nt.states[0])
        r, mu, sd = ens.cem_get_action(nt.states[0], mu0, sd0, 2, 5, cem.alpha, seed_of(7))
        assert np.array_equal(a, r.first_action) and cem.last_cost == r.best_cost and np.array_equal(cem.last_mu, mu)
    finally:
        ens.close()

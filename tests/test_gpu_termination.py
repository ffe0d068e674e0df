"""Episode termination for TermCost on the GPU (csrc/term_cost.hip DONE instances, the gate of
csrc/terminal_value.hip, bcmpc_set_termination).

The definition is cost_functions.episode_cost (NumPy f64, elementwise) and value.add_to_costs' gated form; every
comparison below is BIT FOR BIT -- np.array_equal with equal NaN positions on the costs, exact equality on the
termination steps.  No tolerance is involved anywhere.

1. the kernel alone on synthetic trajectories whose termination steps the test plants;
2. the gate of the value kernel alone;
3. the chain: an engine with cheetah_terms() plus a done condition against the definition evaluated on the
   trajectory the engine itself returned, on every kernel layout, batched, in an ensemble, under CEM and MPPI;
4. refusals on a live engine, by status code;
5. the controllers on a Hopper-shaped task.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_term_cost import (_dev, _empty, _record, _stream, _t, cem_step, mppi_step, net, plans, same)
from test_gpu_terminal_value import A, HID, KERNELS, S, W, critic, kernel_values, plain_engine

pytestmark = pytest.mark.gpu

DIM = 4                 # the state dimension the chain tests' done condition reads
DC = 12.5               # ... and their done_cost


def _i32(n, fill=-7):
    torch, dev = _t()
    return torch.full((n,), fill, dtype=torch.int32, device=dev)


def episode(T, traj, acts):
    from bc_mpc_amd.cost_functions import episode_cost
    return episode_cost(T, traj[:-1], acts, traj[1:])


# ------------------------------------------------------------------ 1. the kernel alone
SA, AA = 26, 6          # 26 state dims + 6 actions: 32 slots
DD = SA - 1             # the done dimension (a slot of its own unless a term reads it too)
SLOTS = {3: 1, 8: 2, 16: 4, 24: 6, 32: 6}       # slot count -> action slots; one per kernel instance


@functools.lru_cache(maxsize=None)
def alone_engine(H):
    """The kernel needs no weights: the engine lends its H, S, A and action bounds."""
    from bc_mpc_amd.engine import RolloutEngine
    return RolloutEngine(SA, AA, 64, 2, "tanh", False, H, 64, device=0, cost="terms")


def slot_cost(n_slots, done_cost=DC, conds=None):
    """A cost reading exactly n_slots slots: n_slots - 1 - (actions) state dims, the actions, the done dimension."""
    from bc_mpc_amd import cost_functions as cf
    n_act = SLOTS[n_slots]
    n_state = n_slots - n_act - 1
    terms = [cf.linear(i, 0.5 + 0.03125 * i, on=("state", "next_state")[i % 2]) for i in range(n_state)]
    terms += [cf.quadratic(j, 0.1 + 0.01 * j, on="action") for j in range(n_act)]
    if len(terms) + 1 < 32:
        terms.append(cf.progress(0, 0.01))
    if len(terms) + 1 < 32:
        terms.append(cf.threshold(0, ">=", 0.2, 10.0, on="next_state"))
    conds = [cf.done_when(DD, "<=", 0.5)] if conds is None else conds
    return cf.TermCost(terms, done=conds, done_cost=done_cost)


def planted(H, K, seed=0, dead=(0.0,)):
    """[H+1, K, SA]: candidate k terminates first at step k % (H + 1), the value H meaning never -- the done
    dimension is 1.0 while alive and dead[k % len(dead)] from row t + 1 (step t's next state) on."""
    rs = np.random.RandomState(100 * H + K + seed)
    traj = rs.standard_normal((H + 1, K, SA))
    flat = traj.reshape(-1)
    pos = rs.choice(flat.size, flat.size // 4, replace=False)
    flat[pos] = np.resize([0.2, 0.0, -0.0], pos.size)                    # on the cost threshold, signed zeros
    t = np.arange(K) % (H + 1)
    traj[:, :, DD] = 1.0
    for k in range(K):
        traj[t[k] + 1:, k, DD] = dead[k % len(dead)]
    return traj, t.astype(np.int32)


def run_alone(eng, d_traj, K, **kw):
    d_costs, d_steps = _empty(K + 8), _i32(K + 8)
    eng.trajectory_cost_async(d_traj.data_ptr(), K, d_costs.data_ptr(), stream=_stream(),
                              d_term_step=d_steps.data_ptr(), **kw)
    d_plain = _empty(K)
    eng.trajectory_cost_async(d_traj.data_ptr(), K, d_plain.data_ptr(), stream=_stream(), **kw)
    costs, steps = d_costs.cpu().numpy(), d_steps.cpu().numpy()
    assert np.isnan(costs[K:]).all() and (steps[K:] == -7).all(), "wrote past K"
    same(d_plain.cpu().numpy(), costs[:K], "trajectory_cost_async (no steps) on the same engine")
    return costs[:K], steps[:K]


@pytest.mark.parametrize("n_slots", sorted(SLOTS))
@pytest.mark.parametrize("H", [1, 7, 8, 9, 17])
def test_kernel_alone_on_planted_terminations(H, n_slots):
    from oracle import mpc_oracle as orc
    eng = alone_engine(H)
    T = slot_cost(n_slots)
    eng.set_cost_terms(T)
    assert eng.info()["layout"].endswith("+terms+done")
    low, high = -np.ones(AA), np.ones(AA)
    seed, off = 0xD0FE + H, 1000
    rs = np.random.RandomState(H)
    mu, sd = rs.uniform(-0.6, 0.6, (H, AA)), rs.uniform(0.1, 2.0, (H, AA))
    d_mu, d_sd = _dev(mu), _dev(sd)
    for K in (1, 63, 64, 65, 400):
        traj, t = planted(H, K)
        if K > H:
            assert set(t.tolist()) == set(range(H + 1))                  # every t in 0 .. H occurs
        d_traj = _dev(traj)
        acts = np.random.RandomState(K).uniform(-1, 1, (H, K, AA))
        d_acts = _dev(acts)
        sources = [("explicit", dict(d_actions=d_acts.data_ptr()), acts),
                   ("philox", dict(seed=seed, cand_offset=off), orc.device_rng_actions(seed, off, K, H, low, high)),
                   ("cem", dict(seed=seed, cand_offset=off, d_mu=d_mu.data_ptr(), d_sigma=d_sd.data_ptr(), cem_iter=1),
                    orc.cem_actions(seed, 1, off, K, H, mu, sd, low, high))]
        for label, kw, want_acts in sources:
            want, want_t = episode(T, traj, want_acts)
            assert np.array_equal(want_t, t)
            got, got_t = run_alone(eng, d_traj, K, **kw)
            same(got, want, f"slots={n_slots} H={H} K={K} {label}: costs")
            assert got_t.dtype == np.int32 and np.array_equal(got_t, t), f"slots={n_slots} H={H} K={K} {label}: steps"
            assert np.array_equal(got_t == H, t == H)


@pytest.mark.parametrize("H", [1, 8, 9])
def test_kernel_alone_further_cases(H):
    from bc_mpc_amd import cost_functions as cf
    eng = alone_engine(H)
    K = 65
    acts = np.random.RandomState(3).uniform(-1, 1, (H, K, AA))
    d_acts = _dev(acts)
    # two conditions on one dimension (<= and >=), which a cost term reads too: the slot is shared
    band = [cf.done_when(DD, "<=", 0.5), cf.done_when(DD, ">=", 2.0)]
    T = cf.TermCost([cf.linear(DD, 1.5, on="next_state"), cf.quadratic(1, 0.25, on="action"), cf.progress(DD, 0.125)],
                    done=band, done_cost=-3.0)
    traj, t = planted(H, K, seed=1, dead=(0.0, 3.0, 0.5, 2.0))
    eng.set_cost_terms(T)
    got, got_t = run_alone(eng, _dev(traj), K, d_actions=d_acts.data_ptr())
    want, want_t = episode(T, traj, acts)
    assert np.array_equal(want_t, t)
    same(got, want, f"H={H}: two conditions")
    assert np.array_equal(got_t, t)
    # a NaN row does not terminate, and the cost goes NaN; the infinities terminate (one condition each)
    traj, t = planted(H, K, seed=2)
    traj[1:, 3, DD] = np.nan
    traj[1:, 4, DD] = np.inf
    traj[1:, 5, DD] = -np.inf
    got, got_t = run_alone(eng, _dev(traj), K, d_actions=d_acts.data_ptr())
    want, want_t = episode(T, traj, acts)
    same(got, want, f"H={H}: NaN row")
    assert np.array_equal(got_t, want_t)
    assert got_t[3] == H and np.isnan(got[3]) and got_t[4] == 0 and got_t[5] == 0       # (+inf >= 2.0, -inf <= 0.5)
    # done_cost 0.0 and -0.0, by the definition's bits
    traj, t = planted(H, K, seed=3)
    d_traj = _dev(traj)
    for dc in (0.0, -0.0):
        Tz = cf.TermCost(T.terms, done=band, done_cost=dc)
        eng.set_cost_terms(Tz)
        got, got_t = run_alone(eng, d_traj, K, d_actions=d_acts.data_ptr())
        want, want_t = episode(Tz, traj, acts)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.array_equal(got_t, t)
    # a cost without done on the same engine: the plain kernel again, and nothing is written to the steps
    plain = cf.TermCost(T.terms)
    eng.set_cost_terms(plain)
    assert eng.info()["layout"].endswith("+terms")
    d_costs, d_steps = _empty(K), _i32(K)
    eng.trajectory_cost_async(d_traj.data_ptr(), K, d_costs.data_ptr(), d_actions=d_acts.data_ptr(), stream=_stream(),
                              d_term_step=d_steps.data_ptr())
    want, want_t = episode(plain, traj, acts)
    same(d_costs.cpu().numpy(), want, f"H={H}: done removed")
    assert (want_t == H).all() and (d_steps.cpu().numpy() == -7).all()


# ------------------------------------------------------------------ 2. the gate
@functools.lru_cache(maxsize=None)
def done_engine(kernel, K, H, with_value=False):
    """An engine of this module's own with cost="terms"; the tests set its TermCost."""
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    nt = net(S, A)
    eng = RolloutEngine(S, A, HID, 2, "tanh", False, H, K, device=0, kernel=kernel, cost="terms")
    if kernel != "auto":
        assert eng.info()["kernel"] == kernel
    eng.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, nt.w.activation), nt.norm, 1)
    if with_value:
        eng.set_terminal_value(critic(), W, 1)
    return eng


@pytest.mark.parametrize("K", [1, 16, 17, 65])
def test_the_gate_of_the_value_kernel(K):
    torch, dev = _t()
    H = 5
    eng = done_engine("auto", 64, H, True)
    rs = np.random.RandomState(K)
    rows = rs.standard_normal((K, S))
    costs_in = rs.standard_normal(K + 8) * 100.0
    costs_in[::3] = -0.0
    steps = (np.arange(K + 8) % (H + 1)).astype(np.int32)
    steps[:K] = steps[:K][rs.permutation(K)]
    if K == 1:
        steps[0] = H - 1
    d_rows, d_steps = _dev(rows), torch.from_numpy(steps).to(dev)
    d_c0, d_c1 = _dev(costs_in), _dev(costs_in)
    d_v0, d_v1 = torch.full((K + 8,), float("nan"), dtype=torch.float32, device=dev), \
        torch.full((K + 8,), float("nan"), dtype=torch.float32, device=dev)
    st = _stream()
    eng.terminal_value_async(d_rows.data_ptr(), K, d_values=d_v0.data_ptr(), d_costs=d_c0.data_ptr(), stream=st)
    eng.terminal_value_async(d_rows.data_ptr(), K, d_values=d_v1.data_ptr(), d_costs=d_c1.data_ptr(), stream=st,
                             d_term_step=d_steps.data_ptr(), horizon=H)
    c0, c1, v0, v1 = d_c0.cpu().numpy(), d_c1.cpu().numpy(), d_v0.cpu().numpy(), d_v1.cpu().numpy()
    alive = steps[:K] == H
    bits = lambda a: a.view(np.uint64)   # noqa: E731
    assert np.array_equal(bits(c1[:K])[alive], bits(c0[:K])[alive]), "t == H: the ungated call's costs"
    assert np.array_equal(bits(c1[:K])[~alive], bits(costs_in[:K])[~alive]), "t < H: the input bits"
    assert np.array_equal(bits(c1[K:]), bits(costs_in[K:]))
    assert np.array_equal(v1.view(np.uint32), v0.view(np.uint32)) and np.isfinite(v1[:K]).all() and np.isnan(v1[K:]).all()
    assert (~alive).any() and (K == 1 or alive.any())
    assert not np.array_equal(bits(c0[:K])[~alive], bits(costs_in[:K])[~alive])
    # the engine's own horizon is the default; another horizon gates on that value
    d_c2 = _dev(costs_in)
    eng.terminal_value_async(d_rows.data_ptr(), K, d_costs=d_c2.data_ptr(), stream=st, d_term_step=d_steps.data_ptr())
    assert np.array_equal(bits(d_c2.cpu().numpy()), bits(c1))
    d_c3 = _dev(costs_in)
    eng.terminal_value_async(d_rows.data_ptr(), K, d_costs=d_c3.data_ptr(), stream=st, d_term_step=d_steps.data_ptr(),
                             horizon=H - 1)
    c3 = d_c3.cpu().numpy()
    at = steps[:K] == H - 1
    assert np.array_equal(bits(c3[:K])[at], bits(c0[:K])[at]) and np.array_equal(bits(c3[:K])[~at], bits(costs_in[:K])[~at])


# ------------------------------------------------------------------ 3. in the chain
def done_cost_fn(thr, done_cost=DC):
    from bc_mpc_amd import cost_functions as cf
    return cf.TermCost(cf.cheetah_terms().terms, done=[cf.done_when(DIM, "<=", thr)], done_cost=done_cost)


def plain_traj(plain, d_state, stride, d_acts, seed, off):
    """The plain terms engine's trajectory of one launch: (numpy, device)."""
    K, H = plain.num_paths, plain.horizon
    d_costs, d_traj = _empty(K), _empty(H + 1, K, S)
    plain.rollout_async(d_state.data_ptr(), stride, d_acts.data_ptr() if d_acts is not None else None, seed, off,
                        d_costs.data_ptr(), d_traj.data_ptr(), None, _stream())
    traj = d_traj.cpu().numpy()
    plain.check_status()
    assert np.isfinite(traj).all()
    return traj, d_traj


def threshold_of(traj):
    H = traj.shape[0] - 1
    return float(np.median(traj[max(1, H // 2), :, DIM]))


def definition(T, traj, veng=None, d_traj=None):
    """(total, t, plain episode costs): episode_cost on the trajectory; with a value engine the gated add of the
    kernel's own values of row H."""
    from bc_mpc_amd import value
    H, K = traj.shape[0] - 1, traj.shape[1]
    costs, t = episode(T, traj, np.zeros((H, K, A)))                    # (cheetah_terms reads no action)
    if veng is None:
        return costs, t, costs
    v = kernel_values(veng, d_traj[H], K)
    return value.add_to_costs(costs, v, W, term_step=t, horizon=H), t, costs


def nonvacuous(t, H):
    frac = float((t < H).mean())
    assert 0.1 <= frac <= 0.9, f"{frac:.2f} of the candidates terminate"
    if H == 5:
        assert len(np.unique(t)) >= 3, np.unique(t)


@pytest.mark.parametrize("with_value", [False, True])
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kernel", KERNELS)
def test_chain_costs_and_steps_equal_the_definition(kernel, H, with_value):
    from bc_mpc_amd import _lib
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    nt = net(S, A)
    K, seed, off = 400, 0xD0E + H, 3000
    plain, eng = plain_engine(kernel, K, H, "terms"), done_engine(kernel, K, H, with_value)
    state = nt.states[1]
    d_state = _dev(state)
    traj, d_traj = plain_traj(plain, d_state, 0, None, seed, off)
    T = done_cost_fn(threshold_of(traj))
    eng.set_cost_terms(T)
    assert eng.info()["layout"].endswith("+value+done" if with_value else "+terms+done")
    want, t, base = definition(T, traj, eng if with_value else None, d_traj)
    nonvacuous(t, H)
    d_costs, d_traj2 = _empty(K), _empty(H + 1, K, S)
    d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    eng.rollout_async(d_state.data_ptr(), 0, None, seed, off, d_costs.data_ptr(), d_traj2.data_ptr(), d_res.data_ptr(),
                      _stream())
    got = d_costs.cpu().numpy()
    eng.check_status()
    assert np.array_equal(d_traj2.cpu().numpy(), traj), "the rollout kernels do not know about termination"
    same(got, want, f"{kernel} H={H} value={with_value}: rollout_async")
    assert np.array_equal(eng.last_termination_steps(np.arange(K)), t)
    if with_value:
        assert not np.array_equal(got[t == H], base[t == H]) and np.array_equal(got[t < H], base[t < H])
    acts = orc.device_rng_actions(seed, off, K, H, nt.low, nt.high)
    index, best_cost, first = _record(d_res, A)
    best = int(np.argmin(want))
    assert index == off + best and best_cost == want[best] and np.array_equal(first, acts[0, best])
    # the synchronous call: the trajectory stays in the engine's scratch
    res = eng.get_action(state, None, seed=seed, cand_offset=off, return_costs=True)
    same(res.costs, want, f"{kernel} H={H} value={with_value}: get_action")
    assert res.best_index == off + best and res.best_cost == want[best] and np.array_equal(res.first_action, acts[0, best])
    assert eng.last_termination_steps([best])[0] == t[best]
    lean = eng.get_action(state, None, seed=seed, cand_offset=off)
    assert (lean.best_index, lean.best_cost) == (res.best_index, res.best_cost)


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kernel", KERNELS)
def test_get_actions_with_four_environments(kernel, H):
    nt = net(S, A)
    B, K, seed, off = 4, 100, 0xBA7C4 + H, 500
    plain, eng = plain_engine(kernel, B * K, H, "terms"), done_engine(kernel, B * K, H, True)
    states = np.stack([nt.states[b % 3] + 0.01 * b for b in range(B)])
    tiled = _dev(np.repeat(states, K, axis=0))
    traj, d_traj = plain_traj(plain, tiled, S, None, seed, off)
    T = done_cost_fn(threshold_of(traj))
    eng.set_cost_terms(T)
    want, t, _ = definition(T, traj, eng, d_traj)
    nonvacuous(t, H)
    res = eng.get_actions(states, None, seed=seed, cand_offset=off, return_costs=True)
    same(res.costs.reshape(-1), want, f"{kernel} H={H}: get_actions")
    assert np.array_equal(eng.last_termination_steps(np.arange(B * K)), t)
    for b in range(B):
        best = int(np.argmin(want[b * K:(b + 1) * K]))
        assert res.best_index[b] == off + b * K + best and res.best_cost[b] == want[b * K + best]


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kernel", KERNELS)
def test_ensemble_members_terminate_on_their_own_trajectories(kernel, H):
    from bc_mpc_amd import ensemble
    from bc_mpc_amd.engine import MLPSpec
    from oracle import mpc_oracle as orc
    nt = net(S, A)
    E, K, seed = 3, 400, 0xE5 + H
    ws = [orc.synthetic_weights(S, A, HID, 2, "tanh", False, seed_base=1000 + 100 * e) for e in range(E)]
    ens = ensemble.EnsembleEngine(E, S, A, HID, 2, "tanh", False, H, K, device=0, cost="terms", kernel=kernel)
    plain, veng = plain_engine(kernel, K, H, "terms"), done_engine(kernel, K, H, True)
    try:
        for e, w in enumerate(ws):
            ens.set_weights(e, MLPSpec(w.kernels, w.biases, w.activation), nt.norm, 1)
        state = nt.states[2]
        d_state = _dev(state)
        trajs = []
        for e, w in enumerate(ws):                                      # member e alone, on the plain engine
            plain.set_weights(MLPSpec(w.kernels, w.biases, w.activation), nt.norm, 100 + e)
            trajs.append(plain_traj(plain, d_state, 0, None, seed, 0))
        T = done_cost_fn(threshold_of(np.concatenate([tr for tr, _ in trajs], axis=1)))     # (pooled over the members)
        ens.set_cost_terms(T)
        for with_value in (False, True):
            if with_value:
                ens.set_terminal_value(critic(), W, 1)
            rows, steps = [], []
            for traj, d_traj in trajs:
                c, t, _ = definition(T, traj, veng if with_value else None, d_traj)
                rows.append(c)
                steps.append(t)
            rows, steps = np.stack(rows), np.stack(steps)
            nonvacuous(steps.reshape(-1), H)
            assert len({s.tobytes() for s in steps}) == E, "the members' steps do not differ"
            for rule in ("mean", "worst"):
                ens.set_rule(rule, 0.0)
                res = ens.get_action(state, None, seed=seed, return_costs=True, return_member_costs=True)
                same(res.member_costs, rows, f"{kernel} H={H} {rule} value={with_value}: member rows")
                want = ensemble.combine(rows, rule)
                same(res.costs, want, f"{kernel} H={H} {rule} value={with_value}: combined")
                best = int(np.argmin(want))
                assert res.best_index == best and res.best_cost == want[best]
                for e, m in enumerate(ens.members):
                    assert np.array_equal(m.last_termination_steps(np.arange(K)), steps[e])
    finally:
        ens.close()
        plain.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, nt.w.activation), nt.norm, 1)


def composed_iteration(plain, eng, T, nt, state, mu, sd, seed, it, off, with_value):
    """Iteration `it` from the stream-ordered blocks: the sampled actions rolled out on the PLAIN engine as an
    explicit array, the done engine's term-cost kernel on that trajectory (costs + steps), the gated value kernel
    on row H; the done engine's cem_rollout_async (actions regenerated, everything in its chain) must give the
    same bits, and both the definition's."""
    from oracle import mpc_oracle as orc
    K, H = plain.num_paths, plain.horizon
    acts = orc.cem_actions(seed, it, off, K, H, mu, sd, nt.low, nt.high)
    d_state, d_acts = _dev(state), _dev(acts)
    st = _stream()
    traj, d_traj = plain_traj(plain, d_state, 0, d_acts, seed, off)
    d_costs, d_steps = _empty(K), _i32(K)
    eng.trajectory_cost_async(d_traj.data_ptr(), K, d_costs.data_ptr(), d_actions=d_acts.data_ptr(), stream=st,
                              d_term_step=d_steps.data_ptr())
    if with_value:
        eng.terminal_value_async(d_traj[H].data_ptr(), K, d_costs=d_costs.data_ptr(), stream=st,
                                 d_term_step=d_steps.data_ptr(), horizon=H)
    costs = d_costs.cpu().numpy()
    want, t, _ = definition(T, traj, eng if with_value else None, d_traj)
    same(costs, want, f"it={it} off={off}: the composed blocks against the definition")
    assert np.array_equal(d_steps.cpu().numpy(), t)
    d_mu, d_sd, d_c2 = _dev(mu), _dev(sd), _empty(K)
    eng.cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sd.data_ptr(), seed, it, off, off + K,
                          d_c2.data_ptr(), None, False, st)
    same(d_c2.cpu().numpy(), costs, f"it={it} off={off}: cem_rollout_async on the done engine")
    eng.check_status()
    return costs, acts, d_costs, t


@pytest.mark.parametrize("with_value", [False, True])
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("kernel", ["group4", "split2", "team"])
def test_cem_and_mppi_equal_the_composed_chain_and_the_batched_planners_the_single_calls(kernel, H, with_value):
    nt = net(S, A)
    B, K, seed, off, iters, E, alpha, lam = 4, 100, 0x5EED5 + H, 1000, 2, 7, 0.1, 0.7
    plain = plain_engine(kernel, K, H, "terms")
    one, many = done_engine(kernel, K, H, with_value), done_engine(kernel, B * K, H, with_value)
    states = np.stack([nt.states[b % 3] + 0.01 * b for b in range(B)])
    mu0, sd0 = plans(B, H, A)
    # the threshold: from the environments' first samples, pooled
    from oracle import mpc_oracle as orc
    first = [plain_traj(plain, _dev(states[b]), 0, _dev(orc.cem_actions(seed, 0, off + b * K, K, H, mu0[b], sd0[b], nt.low,
                                                                         nt.high)), seed, off + b * K)[0] for b in range(B)]
    T = done_cost_fn(threshold_of(np.concatenate(first, axis=1)))
    one.set_cost_terms(T)
    many.set_cost_terms(T)
    rc, mu_c, sd_c = many.cem_get_actions(states, mu0, sd0, iters, E, alpha, seed, cand_offset=off, return_costs=True)
    rm, mu_m, st_m = many.mppi_get_actions(states, mu0, sd0, iters, lam, seed, cand_offset=off, return_costs=True)
    seen = []
    for b in range(B):
        ob = off + b * K
        for planner, r, mu_out in (("cem", rc, mu_c), ("mppi", rm, mu_m)):
            mu, sd, cat, acts_all = mu0[b], sd0[b], [], []
            for it in range(iters):
                costs, acts, d_costs, t = composed_iteration(plain, one, T, nt, states[b], mu, sd, seed, it, ob, with_value)
                seen.append(t)
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
    nonvacuous(np.concatenate(seen), H)
    # the single calls (cand_offset 0) against the chain composed from the blocks
    state = states[0]
    for planner in ("cem", "mppi"):
        mu, sd, cat, acts_all = mu0[0], sd0[0], [], []
        for it in range(iters):
            costs, acts, d_costs, t = composed_iteration(plain, one, T, nt, state, mu, sd, seed, it, 0, with_value)
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
        if best >= (iters - 1) * K:
            assert one.last_termination_steps([best - (iters - 1) * K])[0] == t[best - (iters - 1) * K]


@pytest.mark.parametrize("kernel", KERNELS)
def test_removing_termination_restores_the_plain_terms_engine(kernel):
    from bc_mpc_amd import _lib
    from bc_mpc_amd.cost_functions import cheetah_terms
    nt = net(S, A)
    K, H, seed = 400, 5, 4242
    plain, eng = plain_engine(kernel, K, H, "terms"), done_engine(kernel, K, H)
    state = nt.states[0]
    want = plain.get_action(state, None, seed=seed, return_costs=True)
    traj, _ = plain_traj(plain, _dev(state), 0, None, seed, 0)
    T = done_cost_fn(threshold_of(traj))
    eng.set_cost_terms(T)
    with_done = eng.get_action(state, None, seed=seed, return_costs=True)
    same(with_done.costs, definition(T, traj)[0], f"{kernel}: with done")
    assert not np.array_equal(with_done.costs, want.costs)
    eng.set_cost_terms(cheetah_terms())                                 # a TermCost without done
    assert eng.info()["layout"].endswith("+terms")
    got = eng.get_action(state, None, seed=seed, return_costs=True)
    same(got.costs, want.costs, f"{kernel}: a TermCost without done")
    assert got.best_index == want.best_index and got.best_cost == want.best_cost
    with pytest.raises(_lib.BcmpcError, match="bcmpc_set_termination has not been called"):
        eng.last_termination_steps([0])
    eng.set_cost_terms(T)
    same(eng.get_action(state, None, seed=seed, return_costs=True).costs, with_done.costs, f"{kernel}: set again")
    cond = (_lib.CostTerm * 1)()
    assert eng._lib.bcmpc_set_termination(eng._h, cond, 0, 0.0) == _lib.OK      # n == 0
    eng.cost_terms = None                                               # (the wrapper's idempotence record)
    assert eng.info()["layout"].endswith("+terms")
    same(eng.get_action(state, None, seed=seed, return_costs=True).costs, want.costs, f"{kernel}: n == 0")


def test_rollout_async_on_a_done_engine_replays_in_a_graph():
    """One stream, no parallel branches; nothing in the chain allocates (the step buffer is the setter's), so the
    replay gives the eager bits, also after the state changed."""
    from bc_mpc_amd import _lib
    torch, dev = _t()
    nt = net(S, A)
    K, H, seed = 400, 5, 31337
    plain, eng = plain_engine("group4", K, H, "terms"), done_engine("group4", K, H, True)
    traj, _ = plain_traj(plain, _dev(nt.states[0]), 0, None, seed, 0)
    eng.set_cost_terms(done_cost_fn(threshold_of(traj)))
    d_state = _dev(nt.states[0])
    d_costs = _empty(K)
    d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)

    def launch(stream):
        eng.rollout_async(d_state.data_ptr(), 0, None, seed, 0, d_costs.data_ptr(), None, d_res.data_ptr(), stream)
    eager = {}
    for i in (0, 1):
        d_state.copy_(_dev(nt.states[i]))
        launch(_stream())
        eager[i] = (d_costs.cpu().numpy(), d_res.cpu().numpy().tobytes(), eng.last_termination_steps(np.arange(K)))
    assert not np.array_equal(eager[0][0], eager[1][0]) and (eager[0][2] < H).any() and (eager[0][2] == H).any()
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
        assert np.array_equal(eng.last_termination_steps(np.arange(K)), eager[i][2])


def test_a_team_that_gives_up_reruns_with_the_same_conditions(monkeypatch):
    """BCMPC_TEAM_SPINS=-1 (the suite's hook: the team launch is skipped and reported as a team that gave up): the
    synchronous call reruns on the fallback engine, which must carry the same conditions -- its costs and steps are
    those of a split1 done engine (the layout the fallback takes at this K), bit for bit."""
    nt = net(S, A)
    K, H, seed = 37, 5, 77
    team, ref, plain = done_engine("team", K, H, True), done_engine("split1", K, H, True), plain_engine("split1", K, H, "terms")
    state = nt.states[1]
    traj, _ = plain_traj(plain, _dev(state), 0, None, seed, 0)
    T = done_cost_fn(threshold_of(traj))
    team.set_cost_terms(T)
    ref.set_cost_terms(T)
    want = ref.get_action(state, None, seed=seed, return_costs=True)
    want_t = ref.last_termination_steps(np.arange(K))
    assert (want_t < H).any() and (want_t == H).any()
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
    assert np.array_equal(team.last_termination_steps(np.arange(K)), want_t)
    # a new done_cost reaches the fallback engine that now exists
    T2 = done_cost_fn(threshold_of(traj), done_cost=-40.0)
    team.set_cost_terms(T2)
    ref.set_cost_terms(T2)
    same(rerun().costs, ref.get_action(state, None, seed=seed, return_costs=True).costs, "fallback, new done_cost")
    # a planner call reruns as a whole; the steps are those of the rerun's last iteration
    mu0, sd0 = (x[0] for x in plans(1, H, A))
    want, want_mu, want_sd = ref.cem_get_action(state, mu0, sd0, 2, 5, 0.1, seed)
    want_t = ref.last_termination_steps(np.arange(K))
    monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
    try:
        got, mu, sd = team.cem_get_action(state, mu0, sd0, 2, 5, 0.1, seed)
    finally:
        monkeypatch.delenv("BCMPC_TEAM_SPINS")
    assert (got.best_index, got.best_cost) == (want.best_index, want.best_cost)
    assert mu.tobytes() == want_mu.tobytes() and sd.tobytes() == want_sd.tobytes()
    assert np.array_equal(team.last_termination_steps(np.arange(K)), want_t)


def test_a_large_done_cost_moves_the_winner_to_the_definitions_winner():
    nt = net(S, A)
    K, H, seed = 400, 5, 777
    plain, eng = plain_engine("auto", K, H, "terms"), done_engine("auto", K, H)
    state = nt.states[0]
    traj, _ = plain_traj(plain, _dev(state), 0, None, seed, 0)
    base = plain.get_action(state, None, seed=seed, return_costs=True)
    # terminate exactly the plain winner (and everything below it in that dimension) at the last step, at a price
    thr = float(traj[H, base.best_index, DIM])
    T = done_cost_fn(thr, done_cost=1e6)
    want, t, _ = definition(T, traj)
    assert t[base.best_index] < H and (t == H).any()
    eng.set_cost_terms(T)
    got = eng.get_action(state, None, seed=seed, return_costs=True)
    same(got.costs, want, "large done_cost")
    best = int(np.argmin(want))
    assert got.best_index == best != base.best_index and t[best] == H and got.best_cost == want[best]


# ------------------------------------------------------------------ 4. refusals on a live engine
def test_refusals_by_status_code():
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import RolloutEngine
    Sr, Ar = 11, 3
    eng = RolloutEngine(Sr, Ar, 64, 2, "tanh", False, 3, 16, device=0, cost="terms")
    other = RolloutEngine(S, A, 64, 2, "tanh", False, 3, 16, device=0, cost="cheetah")
    lib = eng._lib

    def cond(kind=_lib.TERM_THRESHOLD, source=_lib.SRC_NEXT_STATE, index=0, cmp=_lib.CMP_LE, weight=0.0, param=0.7):
        c = _lib.CostTerm()
        c.kind, c.source, c.index, c.cmp, c.weight, c.param = kind, source, index, cmp, weight, param
        return c

    def arr(items):
        a = (_lib.CostTerm * max(1, len(items)))()
        for i, c in enumerate(items):
            a[i] = c
        return a
    term = cond(kind=_lib.TERM_LINEAR, source=_lib.SRC_STATE, weight=1.0, param=0.0)
    try:
        ARG, OK = _lib.ERR_ARG, _lib.OK
        assert lib.bcmpc_set_termination(other._h, arr([cond()]), 1, 0.0) == ARG            # not a terms engine
        assert b"BCMPC_COST_TERMS" in lib.bcmpc_last_error()
        assert lib.bcmpc_set_termination(eng._h, arr([cond()]), 1, 0.0) == OK               # (before any terms)
        assert lib.bcmpc_set_termination(eng._h, arr([cond()] * 33), 33, 0.0) == ARG
        assert lib.bcmpc_set_termination(eng._h, None, 1, 0.0) == ARG
        for bad in (cond(source=_lib.SRC_STATE), cond(source=_lib.SRC_ACTION), cond(kind=_lib.TERM_LINEAR),
                    cond(kind=_lib.TERM_QUADRATIC), cond(kind=_lib.TERM_DIFF, source=_lib.SRC_STATE), cond(weight=1.0),
                    cond(index=Sr), cond(index=-1), cond(cmp=4), cond(param=float("nan")), cond(param=float("inf"))):
            assert lib.bcmpc_set_termination(eng._h, arr([cond(), bad]), 2, 0.0) == ARG
            assert b"done condition 1" in lib.bcmpc_last_error()
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert lib.bcmpc_set_termination(eng._h, arr([cond()]), 1, bad) == ARG
        # the budget, in either call order: 3 conditions are set, then 30 terms do not fit, 29 do
        assert lib.bcmpc_set_termination(eng._h, arr([cond()] * 3), 3, 1.0) == OK
        assert lib.bcmpc_set_cost_terms(eng._h, arr([term] * 30), 30) == ARG
        assert lib.bcmpc_set_cost_terms(eng._h, arr([term] * 29), 29) == OK
        assert lib.bcmpc_set_termination(eng._h, arr([cond()] * 4), 4, 1.0) == ARG          # 29 + 4
        assert lib.bcmpc_set_termination(eng._h, arr([cond()] * 3), 3, 1.0) == OK
        assert eng.info()["layout"].endswith("+terms+done")
        # a refused call changes nothing: the engine still holds 29 + 3
        assert lib.bcmpc_set_cost_terms(eng._h, arr([term] * 32), 32) == ARG
        assert lib.bcmpc_set_termination(eng._h, None, 0, 0.0) == OK
        assert lib.bcmpc_set_cost_terms(eng._h, arr([term] * 32), 32) == OK
        assert lib.bcmpc_set_termination(eng._h, arr([cond()]), 1, 0.0) == ARG
        # the wrapper carries a TermCost over the same budget whatever the engine held before
        from bc_mpc_amd import cost_functions as cf
        eng.cost_terms = None
        eng.set_cost_terms(cf.TermCost([cf.linear(0, 1.0)] * 2, done=[cf.done_when(0, "<", 0.0)] * 30))
        eng.set_cost_terms(cf.TermCost([cf.linear(0, 1.0)] * 31, done=[cf.done_when(0, "<", 0.0)]))
        with pytest.raises(ValueError, match="done condition 0: index 11"):
            eng.set_cost_terms(cf.TermCost([], done=[cf.done_when(Sr, "<", 0.0)]))
        # the diagnostics' own checks
        idx, out = (ctypes.c_int64 * 1)(16), (ctypes.c_int32 * 1)()
        assert lib.bcmpc_last_termination_steps(eng._h, idx, 1, out) == ARG
        assert lib.bcmpc_last_termination_steps(other._h, idx, 1, out) == _lib.ERR_STATE
    finally:
        eng.close()
        other.close()


# ------------------------------------------------------------------ 5. controllers, Hopper-shaped
SH, AH = 11, 3


class _Box:
    def __init__(self, n):
        self.low, self.high, self.shape = -np.ones(n, np.float32), np.ones(n, np.float32), (n,)


class _Env:
    action_space = _Box(AH)
    observation_space = _Box(SH)


def hopper_cost(state):
    """Hopper's shape: progress and control cost, `not healthy` as three conditions placed around the start state
    so that some candidates of a 5-step rollout leave the band."""
    from bc_mpc_amd import cost_functions as cf
    return cf.TermCost([cf.progress(5, 0.008), cf.linear(10, 0.05)] + [cf.quadratic(j, 0.001, on="action") for j in range(AH)],
                       done=[cf.done_when(0, "<=", float(state[0]) - 0.03), cf.done_when(1, ">=", float(state[1]) + 0.45),
                             cf.done_when(1, "<=", float(state[1]) - 0.015)], done_cost=25.0)


def test_controllers_answer_what_a_hand_set_up_engine_answers():
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller
    nt = net(SH, AH)
    K, H, B = 100, 5, 4
    states = np.stack([nt.states[b % 3] + 0.001 * b for b in range(B)])
    T = hopper_cost(nt.states[0])
    seed_of = lambda s: int(np.random.RandomState(s).randint(0, 2**62, dtype=np.int64))   # noqa: E731
    one, many = nt.engine("auto", K, H, terms=T), nt.engine("auto", B * K, H, terms=T)
    try:
        kw = dict(horizon=H, cost_fn=T, num_simulated_paths=K)
        ctrl = MPCcontroller(_Env(), nt.dyn, rng="device", seed=5, **kw)
        a = ctrl.get_action(states[0])
        r = one.get_action(states[0], None, seed=seed_of(5), return_costs=True)
        steps = one.last_termination_steps(np.arange(K))
        assert (steps < H).any() and (steps == H).any(), "the conditions are vacuous on this task"
        assert ctrl._engine.info()["layout"].endswith("+terms+done")
        assert np.array_equal(a, r.first_action) and ctrl.last_index == r.best_index and ctrl.last_cost == r.best_cost
        assert ctrl.last_termination_step == steps[r.best_index] and isinstance(ctrl.last_termination_step, int)
        # rng="numpy": the reference's draw on the host, uploaded
        ctrl = MPCcontroller(_Env(), nt.dyn, **kw)
        np.random.seed(4242)
        a = ctrl.get_action(states[1])
        paths = np.random.RandomState(4242).uniform(_Env.action_space.low, _Env.action_space.high, [H, K, AH])
        r = one.get_action(states[1], paths)
        assert np.array_equal(a, paths[0, r.best_index]) and ctrl.last_cost == r.best_cost
        assert ctrl.last_termination_step == one.last_termination_steps([r.best_index])[0]
        # get_actions
        ctrl = MPCcontroller(_Env(), nt.dyn, rng="device", seed=6, **kw)
        a = ctrl.get_actions(states)
        r = many.get_actions(states, None, seed=seed_of(6))
        assert np.array_equal(a, r.first_action) and np.array_equal(ctrl.last_index, r.best_index)
        assert np.array_equal(ctrl.last_termination_step, many.last_termination_steps(r.best_index))
        # CEM and MPPI
        cem = CEMcontroller(_Env(), nt.dyn, iterations=2, n_elite=5, seed=7, **kw)
        mu0, sd0 = cem.initial_distribution()
        a = cem.get_action(states[0])
        r, mu, sd = one.cem_get_action(states[0], mu0, sd0, 2, 5, cem.alpha, seed_of(7))
        assert np.array_equal(a, r.first_action) and cem.last_cost == r.best_cost and np.array_equal(cem.last_mu, mu)
        assert cem._engine.info()["layout"].endswith("+terms+done")
        if r.best_index >= K:
            assert cem.last_termination_step == one.last_termination_steps([r.best_index - K])[0]
        else:
            assert cem.last_termination_step is None
        mp = MPPIcontroller(_Env(), nt.dyn, temperature=0.7, iterations=2, seed=9, **kw)
        mu0, sd0 = mp.initial_distribution()
        a = mp.get_action(states[0])
        r, mu, stats = one.mppi_get_action(states[0], mu0, sd0, 2, 0.7, seed_of(9))
        assert np.array_equal(a, mu[0]) and mp.last_cost == r.best_cost and mp.last_ess == float(stats.ess)
        if r.best_index >= K:
            assert mp.last_termination_step == one.last_termination_steps([r.best_index - K])[0]
        else:
            assert mp.last_termination_step is None
        # a TermCost without done: no step is published
        plain = MPCcontroller(_Env(), nt.dyn, horizon=H, cost_fn=type(T)(T.terms), num_simulated_paths=K, rng="device", seed=5)
        plain.get_action(states[0])
        assert plain.last_termination_step is None and plain._engine.info()["layout"].endswith("+terms")
    finally:
        from test_gpu_term_cost import hopper_like_terms
        one.set_cost_terms(hopper_like_terms())                         # (the shared engines go back without done)
        many.set_cost_terms(hopper_like_terms())

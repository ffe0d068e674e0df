"""Every rollout kernel against the oracle across state and action sizes (size_cases.py holds the shapes, the nets,
the inputs and the bar; expectations come from oracle/mpc_oracle.py only).

The engine takes state_dim 1..32, action_dim 1..16 with S + A <= 32; the kernels branch on both (the tile the action
input rows fall into, the action pairs of the staging, the 4-step staging ring, pp3's tile-1 partials, the reward
row, the policy rows, the team kernel's A <= 15).  SHAPES names one shape per edge; K = 130 leaves the third
64- / 32-candidate group nearly empty with a partial 16-column, H = 6 wraps the staging ring.

Per case (kernel, net, S, A), on a cost="none" (S < 18) or cost="cheetah" engine through rollout_async:
 1. the states of three action sources (explicit array, device Philox, CEM sample) against the oracle at
    size_cases' bar; row 0 exact, every entry finite, nothing written outside [H+1, K, S].  cem_rollout_async
    returns costs only: the CEM sample is rolled out as an explicit array on a cost="terms" engine (states to
    the bar) and cem_rollout_async's costs must equal that launch's bit for bit;
 2. a cost="terms" engine of the same shape whose TermCost reads state dim S - 1, next-state dim 0 and action
    dims 0 and A - 1: its costs equal trajectory_cost_fn of its own trajectory and the oracle's actions bit for bit;
 3. S >= 18: the fused cheetah cost at test_gpu_parity.assert_costs_close's bar, the record's index = argmin;
 4. (three shapes) get_actions over B = 3 environments equals the three single calls bit for bit.

What the engine refuses, and why (any other refusal fails the case):
 * kernel="team" at A = 16 -- the team kernel stages the actions in 15 slots beside a flag (engine_plan.cpp:
   action_dim <= 15).  The case asserts the refusal and runs its checks on kernel="auto", which must answer.
 * rollout_pp3 (kernel="auto" under BCMPC_SPLIT_PP=1) where bcmpc_split_pp_lds_bytes(hidden, 2, S, A) == -1 -- the
   tile-1 partials of S >= 21 do not fit the 160 KiB of LDS beside the slab.  The case asserts that the layout
   is rollout_pp3 exactly when the query is positive and runs its checks on whatever auto picked instead.
 * kernel="split4" on a relu / LayerNorm net padded to hidden 512 at A >= 13 -- the 64-candidate group's slab
   (128 KiB), layer-0 slab, column exchange and parameters leave 12,416 of the 160 KiB of LDS, and the staged actions
   take 1 KiB per action dim ("split kernel does not fit this shape"; the tanh net has no exchange and fits at
   A = 16).  As for the team kernel: the refusal is asserted, the checks run on kernel="auto".
 * CEM sampling on kernel="solo" -- rollout_impl refuses it ("CEM runs on group-kernel engines"); the case
   asserts the refusal and checks the other two sources.

Reward engines and fused policies need S >= 16.  A policy engine needs its fused cost (rollout_impl: "policy
engines need the fused cost"), which is the cheetah cost, S >= 18: the policy shapes (16, 16) and (17, 15) are
raised to S = 18, 19 with A lowered to keep S + A = 32 -- (18, 14) and (19, 13), the policy's 16-row output tile
full to its last row.
"""
import ctypes
import functools

import numpy as np
import pytest

import size_cases as sc
from conftest import envelope
from test_gpu_term_cost import same, term_total

pytestmark = pytest.mark.gpu

PAD = 3                       # rows of NaN before and after every output buffer


def _t():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(x):
    torch, dev = _t()
    return torch.from_numpy(np.array(x, dtype=np.float64, order="C", copy=True)).to(dev)


def _stream():
    torch, dev = _t()
    return torch.cuda.current_stream(dev).cuda_stream


def a_gpu_fault_stops_the_run(test):
    """A HIP error (an illegal access, a launch failure) ends the run: every later launch of the process would
    fail on the same sticky error, and nothing more should be started on a device that has just faulted."""
    @functools.wraps(test)
    def wrapped(*args, **kw):
        from bc_mpc_amd import _lib
        try:
            return test(*args, **kw)
        except Exception as e:
            if (isinstance(e, _lib.BcmpcError) and e.code == _lib.ERR_HIP) or "HIP error" in str(e):
                pytest.exit(f"GPU fault, the run stops here: {e}", returncode=3)
            raise
    return wrapped


class Padded:
    """A NaN-filled f64 device buffer of ``n`` entries with ``pad`` entries of NaN on either side."""

    def __init__(self, n, pad):
        torch, dev = _t()
        self.n, self.pad = n, pad
        self.t = torch.full((n + 2 * pad,), np.nan, dtype=torch.float64, device=dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * self.pad

    def get(self, label):
        a = self.t.cpu().numpy()
        assert np.isnan(a[:self.pad]).all() and np.isnan(a[self.pad + self.n:]).all(), f"{label}: wrote outside the buffer"
        return a[self.pad:self.pad + self.n]


def make_engine(c, kernel, cost, K=None, **kw):
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    w = c.w
    eng = RolloutEngine(c.S, c.A, c.hidden, c.L, c.act, c.ln, c.H, c.K if K is None else K, device=0, cost=cost,
                        kernel=kernel, **kw)
    eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta), c.norm, 1)
    eng.set_action_bounds(c.low, c.high)
    return eng


def sweep_terms(S, A):
    """State dim S - 1, next-state dim 0, action dims 0 and A - 1."""
    from bc_mpc_amd import cost_functions as cf
    return cf.TermCost([cf.linear(S - 1, 0.7), cf.quadratic(0, 1.3, target=0.1, on="next_state"),
                        cf.quadratic(0, 0.2, on="action"), cf.linear(A - 1, -0.4, on="action"),
                        cf.threshold(A - 1, ">=", 0.0, 3.0, on="action"), cf.progress(S - 1, 0.01)])


def create_refusal(kernel, c):
    """The message of the stated refusal of bcmpc_create for (kernel, case), None where the engine must take it."""
    if kernel == "team" and c.A > 15:
        return "team kernel"
    if kernel == "split4" and (c.act == "relu" or c.ln) and 256 < c.hidden <= 512 and c.A >= 13:
        return "split kernel does not fit this shape"
    return None


def pp3_takes(c):
    from bc_mpc_amd import _lib
    return c.L == 2 and _lib.load().bcmpc_split_pp_lds_bytes(c.hidden, 2, c.S, c.A) > 0


def launch(eng, c, src, explicit):
    """One rollout_async of source ``src`` (``explicit``: its oracle actions as an array, else drawn in the
    kernel): the trajectory [H+1, K, S], the costs and the record's index (None on a cost="none" engine)."""
    from bc_mpc_amd import _lib
    torch, dev = _t()
    K, H, S = c.K, c.H, c.S
    fused = eng.cost != "none"
    traj, costs = Padded((H + 1) * K * S, PAD * S), Padded(K, PAD)
    d_state = _dev(c.state)
    d_acts = _dev(c.acts[src]) if explicit else None
    d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev) if fused else None
    eng.rollout_async(d_state.data_ptr(), 0, d_acts.data_ptr() if explicit else None, sc.SEED, sc.OFF,
                      costs.ptr if fused else None, traj.ptr, d_res.data_ptr() if fused else None, _stream())
    got = traj.get(f"{src} trajectory").reshape(H + 1, K, S)
    eng.check_status()
    if not fused:
        return got, None, None
    index = int(d_res.cpu().numpy()[:8].view(np.int64)[0])
    return got, costs.get(f"{src} costs").copy(), index


def check_states(c, src, got, label):
    """Check 1 on one trajectory; returns the worst |got - want| / bar."""
    want = c.states[src]
    bar, spread = c.bar(src)
    assert np.array_equal(got[0], np.tile(c.state, (c.K, 1))), f"{label}: row 0 is not the tiled state"
    assert np.isfinite(got).all(), f"{label}: {int((~np.isfinite(got)).sum())} entries not finite"
    ratio = np.abs(got - want) / bar
    worst = float(ratio.max())
    print(f"[sizes] {label} {src}: worst |dstate| / bar = {worst:.3f} (reference spread {spread:.2f} base bars)")
    if worst > 1.0:
        h, k, d = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        bad = np.argwhere(ratio > 1.0)
        raise AssertionError(f"{label} {src}: {len(bad)} entries beyond the bar, worst {worst:.1f}x at step {h} "
                             f"candidate {k} dim {d} (got {got[h, k, d]!r}, want {want[h, k, d]!r}); dims off: "
                             f"{sorted(set(bad[:, 2].tolist()))}")
    return worst


def sizes_line(kernel, ran, c, worst):
    return f"[sizes-case] kernel={kernel} ran={ran} {c.net} S={c.S} A={c.A} K={c.K} H={c.H} worst={worst:.3f}"


def run_case(kernel, c, monkeypatch, refusal=create_refusal, line=sizes_line):
    """Checks 1 - 3 of the module docstring on one size_cases.Case.  ``refusal(kernel, c)``: the message of a stated
    refusal of bcmpc_create; ``line``: the case's one line of output.  Returns (the kernel that ran, the worst
    |dstate| / bar)."""
    from oracle import mpc_oracle as orc
    from test_gpu_parity import assert_costs_close
    net, S, A, K, H = c.net, c.S, c.A, c.K, c.H
    label = f"{kernel} {net} S={S} A={A} K={K} H={H}"
    name = "auto" if kernel == "pp3" else kernel
    monkeypatch.delenv("BCMPC_SPLIT_PP", raising=False)
    if kernel == "pp3":
        monkeypatch.setenv("BCMPC_SPLIT_PP", "1")
    cost = "cheetah" if c.cheetah else "none"
    refused = refusal(kernel, c)
    if refused:
        with pytest.raises(ValueError, match=refused):
            make_engine(c, kernel, cost)
        name = "auto"                                        # ... which must still answer
    eng = make_engine(c, name, cost)
    terms_eng = make_engine(c, name, "terms")
    try:
        info = eng.info()
        if kernel == "pp3":
            assert info["layout"].startswith("rollout_pp3") == pp3_takes(c), (info["layout"], pp3_takes(c))
        elif refused:
            assert info["kernel"] != kernel, info
        elif kernel != "auto":
            assert info["kernel"] == kernel, info
        T = sweep_terms(S, A)
        terms_eng.set_cost_terms(T)
        worst = 0.0
        # 1 + 3: explicit array and device Philox on the engine itself
        for src in ("explicit", "philox"):
            got, costs, index = launch(eng, c, src, explicit=src == "explicit")
            worst = max(worst, check_states(c, src, got, label))
            if c.cheetah:
                assert_costs_close(costs, c.costs[src], orc.near_threshold_mask(c.states[src]), f"{label} {src}",
                                   env=envelope(c.ln, c.L, c.hidden, H))
                assert index - sc.OFF == int(np.argmin(costs)), (index, int(np.argmin(costs)))
        # 2: the terms engine on every source; the CEM sample's states ride on its explicit launch
        term_costs = {}
        for src in sc.SOURCES:
            got, term_costs[src], _ = launch(terms_eng, c, src, explicit=src != "philox")
            worst = max(worst, check_states(c, src, got, label + " +terms"))
            same(term_costs[src], term_total(T, got, c.acts[src]), f"{label} {src}: terms vs trajectory_cost_fn")
        # 1, CEM: the sample drawn inside the rollout and the cost kernels
        d_state, d_mu, d_sd = _dev(c.state), _dev(c.mu), _dev(c.sd)
        cem_costs = Padded(K, PAD)

        def cem(e, out):
            e.cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sd.data_ptr(), sc.SEED, sc.CEM_IT, sc.OFF,
                                sc.OFF + K, out.ptr, None, False, _stream())
            got = out.get("cem costs").copy()
            e.check_status()
            return got
        if info["kernel"] == "solo":
            with pytest.raises(ValueError, match="CEM runs on group-kernel engines"):
                cem(terms_eng, cem_costs)
        else:
            same(cem(terms_eng, cem_costs), term_costs["cem"], f"{label}: cem_rollout_async vs the explicit CEM sample")
            if c.cheetah:
                assert_costs_close(cem(eng, Padded(K, PAD)), c.costs["cem"], orc.near_threshold_mask(c.states["cem"]),
                                   f"{label} cem", env=envelope(c.ln, c.L, c.hidden, H))
        print(line(kernel, info["kernel"], c, worst))
        return info["kernel"], worst
    finally:
        eng.close()
        terms_eng.close()


KERNEL_NET = [(k, n) for k, nets in sc.KERNEL_NETS.items() for n in nets]


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@pytest.mark.parametrize("kernel,net", KERNEL_NET)
@a_gpu_fault_stops_the_run
def test_rollout_matches_oracle(kernel, net, shape, monkeypatch):
    run_case(kernel, sc.case(shape[0], shape[1], net, sc.K, sc.H), monkeypatch)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@a_gpu_fault_stops_the_run
def test_pp3_partly_empty_second_group(shape, monkeypatch):
    run_case("pp3", sc.case(shape[0], shape[1], "2x500tanh", sc.K_PP, sc.H), monkeypatch)


@pytest.mark.parametrize("shape", sc.TINY_SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@pytest.mark.parametrize("kernel,net", KERNEL_NET)
@a_gpu_fault_stops_the_run
def test_one_candidate_one_step(kernel, net, shape, monkeypatch):
    run_case(kernel, sc.case(shape[0], shape[1], net, 1, 1), monkeypatch)


# ------------------------------------------------------------------ the guard against a vacuous comparison
@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@pytest.mark.parametrize("net", list(sc.NETS))
def test_a_wrong_dimension_could_not_pass(net, shape):
    """CPU only: each of the three one-dimension mutations of the oracle moves the median candidate's worst
    state by more than 10 times the cap of the bar, 1e-5 (1 + |want|)."""
    r = sc.mutation_ratios(shape[0], shape[1], net)
    print(f"[sizes-mutation] {net} S={shape[0]} A={shape[1]}: " + ", ".join(f"{k} {v:.0f}x" for k, v in r.items()))
    assert min(r.values()) > 10.0, r


# ------------------------------------------------------------------ 4. batched rollouts
@pytest.mark.parametrize("shape", sc.BATCH_SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@a_gpu_fault_stops_the_run
def test_batched_equals_single_calls(shape, monkeypatch):
    from oracle import mpc_oracle as orc
    monkeypatch.delenv("BCMPC_SPLIT_PP", raising=False)
    S, A = shape
    B = 3
    c = sc.case(S, A, "2x500tanh")
    cost = "cheetah" if c.cheetah else "terms"
    states = np.stack([orc.synthetic_state(c.norm, seed=11 + b) for b in range(B)])
    batch, single = make_engine(c, "auto", cost, K=B * c.K), make_engine(c, "auto", cost)
    try:
        assert batch.info()["kernel"] == single.info()["kernel"], (batch.info(), single.info())
        if cost == "terms":
            for e in (batch, single):
                e.set_cost_terms(sweep_terms(S, A))
        res = batch.get_actions(states, None, seed=sc.SEED, cand_offset=sc.OFF, return_costs=True)
        for b in range(B):
            one = single.get_action(states[b], None, seed=sc.SEED, cand_offset=sc.OFF + b * c.K, return_costs=True)
            same(res.costs[b], one.costs, f"S={S} A={A} environment {b}")
            assert int(res.best_index[b]) == one.best_index and res.best_cost[b] == one.best_cost
            assert np.array_equal(res.first_action[b], one.first_action)
            assert len(np.unique(one.costs)) > c.K // 2
    finally:
        batch.close()
        single.close()


# ------------------------------------------------------------------ reward engines
REWARD_SHAPES = [(16, 1), (23, 9), (24, 8), (31, 1)]
REWARD_ATOL, REWARD_RTOL, GAMMA = 1e-4, 1e-5, 0.95     # test_gpu_sweep.test_split_reward_shapes' bar


def reward_case(S, A, ln, kernel, want_kernel=None, hidden=500, K=sc.K, H=sc.H):
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc
    norm = sc.normalization(S, A, reward=True)
    w = orc.synthetic_reward_weights(S, A, hidden, ln)
    state = orc.synthetic_state(norm)
    low, high = sc.bounds(A)
    eng = RolloutEngine(S, A, hidden, 2, "tanh", ln, H, K, cost="reward", model="reward", kernel=kernel)
    try:
        assert eng.info()["kernel"] == (want_kernel or kernel), eng.info()
        eng.set_weights(MLPSpec(w.kernels, w.biases, "tanh", w.ln_gamma, w.ln_beta, model="reward"), norm, 1)
        eng.set_action_bounds(low, high)
        eng.set_discount(GAMMA)
        res = eng.get_action(state, None, seed=sc.SEED, cand_offset=sc.OFF, return_costs=True)
        ap = orc.device_rng_actions(sc.SEED, sc.OFF, K, H, low, high)
        want, _ = orc.reward_rollout(orc.NumpyRewardDynamics(w, norm), state, ap, GAMMA)
        d = np.abs(res.costs - want)
        print(f"[sizes-reward] {kernel}{' LN' if ln else ''} hidden={hidden} S={S} A={A}: max|dr|={d.max():.2e} "
              f"(bar at the worst entry {float((REWARD_ATOL + REWARD_RTOL * np.abs(want))[np.argmax(d)]):.2e})")
        assert np.isfinite(res.costs).all()
        assert (d <= REWARD_ATOL + REWARD_RTOL * np.abs(want)).all()
        assert res.best_index - sc.OFF == int(np.argmax(res.costs))
        assert np.array_equal(res.first_action, ap[0, res.best_index - sc.OFF])
    finally:
        eng.close()


@pytest.mark.parametrize("kernel", ["group4", "split2", "team"])
@pytest.mark.parametrize("shape", REWARD_SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@a_gpu_fault_stops_the_run
def test_reward_net(shape, kernel):
    """The reward row is output row S of tile 1: S = 16 its first row, 23 / 24 either side of the LayerNorm team
    variant's limit, 31 the last row."""
    reward_case(shape[0], shape[1], False, kernel)


@a_gpu_fault_stops_the_run
def test_reward_net_team_layer_norm():
    """The team kernel's LayerNorm heads carry their statistics in rows 24..27 of the exchange: S <= 23.  At
    (23, 9) it runs; at (24, 8) kernel="team" is refused with the message that says so, and kernel="auto" falls
    back to the fp32 group kernel, which answers."""
    from bc_mpc_amd.engine import RolloutEngine
    reward_case(23, 9, True, "team")
    with pytest.raises(ValueError, match="S <= 23"):
        RolloutEngine(24, 8, 500, 2, "tanh", True, sc.H, sc.K, cost="reward", model="reward", kernel="team")
    reward_case(24, 8, True, "auto", want_kernel="group4")


# ------------------------------------------------------------------ fused policy, stochastic mode
POLICY_SHAPES = [(18, 14), (19, 13), (26, 6), (31, 1)]


@pytest.mark.parametrize("kernel", ["fp32", "split2", "team"])
@pytest.mark.parametrize("shape", POLICY_SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@a_gpu_fault_stops_the_run
def test_policy_stochastic_mode_every_step(shape, kernel):
    """test_gpu_parity.test_policy_stochastic_mode_pinned_every_step's method across shapes: at every step the
    rolled-out action is mean(s_h) + exp(logstd) z_h and s_{h+1} = predict(s_h, a_h), from the device's own s_h.
    Action j is output row S - 16 + j of the policy's one 16-row tile."""
    policy_case(shape, kernel)


def policy_case(shape, kernel, policy_layers=2, policy_hidden=128, K=sc.K, H=sc.H):
    """``kernel``: "fp32" (the 2x256 relu net on the fp32 group kernel), else a kernel name for the 2x500 tanh net
    ("auto": whatever the engine picks).  Returns the kernel that ran."""
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import MLPSpec, PolicySpec, RolloutEngine
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    S, A = shape
    if kernel == "fp32":
        w, kw = orc.synthetic_weights(S, A, 256, 2, "relu", False), dict(precision="fp32")
    else:
        w, kw = orc.synthetic_weights(S, A, 500, 2, "tanh", False), dict(kernel=kernel)
    p = orc.synthetic_policy(S, A, policy_hidden, policy_layers)
    norm = sc.normalization(S, A)
    state = orc.synthetic_state(norm)
    dyn, pol = orc.NumpyDynamics(w, norm), orc.NumpyPolicy(p)
    eng = RolloutEngine(S, A, w.hidden, 2, w.activation, False, H, K, policy_hidden=policy_hidden,
                        policy_layers=policy_layers, policy_mode="stochastic", **kw)
    try:
        if kernel not in ("fp32", "auto"):
            assert eng.info()["kernel"] == kernel, eng.info()
        eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation), norm, 1)
        eng.set_policy(PolicySpec(p.kernels, p.biases, p.ob_mean, p.ob_std, p.logstd), 0.5, 1)
        traj, out, costs = Padded((H + 1) * K * S, PAD * S), Padded(H * K * A, PAD * A), Padded(K, PAD)
        d_state = _dev(state)
        d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
        eng.rollout_policy_async(d_state.data_ptr(), None, sc.SEED, sc.OFF, costs.ptr, traj.ptr, out.ptr,
                                 d_res.data_ptr(), _stream())
        tr = traj.get("trajectory").reshape(H + 1, K, S)
        acts = out.get("actions").reshape(H, K, A)
        cs = costs.get("costs")
        eng.check_status()
        assert np.array_equal(tr[0], np.tile(state, (K, 1))) and np.isfinite(tr).all() and np.isfinite(acts).all()
        sd = np.exp(p.logstd.astype(np.float64))
        worst_a = worst_s = 0.0
        for h in range(H):
            want = pol.mean(tr[h]).astype(np.float64) + sd * orc.device_rng_normals(sc.SEED, sc.OFF, K, h, A)
            da = np.abs(acts[h] - want)
            assert (da <= 1e-5 + 1e-5 * np.abs(want)).all(), (
                f"step {h}: action off by {da.max():.3e}, dims {sorted(set(np.argwhere(da > 1e-5 + 1e-5 * np.abs(want))[:, 1].tolist()))}")
            nxt = dyn.predict(tr[h], acts[h])
            ds = np.abs(tr[h + 1] - nxt)
            assert (ds <= 1e-6 * (1 + np.abs(nxt))).all(), (
                f"step {h}: state off by {ds.max():.3e}, dims {sorted(set(np.argwhere(ds > 1e-6 * (1 + np.abs(nxt)))[:, 1].tolist()))}")
            worst_a, worst_s = max(worst_a, da.max()), max(worst_s, ds.max())
        print(f"[sizes-policy] {kernel} policy {policy_layers}x{policy_hidden} S={S} A={A}: max|da|={worst_a:.2e} "
              f"max|ds|={worst_s:.2e}")
        raw = d_res.cpu().numpy()
        best = int(raw[:8].view(np.int64)[0]) - sc.OFF
        assert best == int(np.argmin(cs)) and np.array_equal(raw[16:16 + 8 * A].view(np.float64), acts[0, best])
        return eng.info()["kernel"]
    finally:
        eng.close()


# ------------------------------------------------------------------ single-pass f16
F16_SHAPES = [s for s in sc.SHAPES if s[0] >= 18]


def f16_case(S, A, K, label):
    from oracle import mpc_oracle as orc
    from test_gpu_f16 import F16_NEAR, _check, _engine
    c = sc.case(S, A, "2x500tanh", K, sc.H)
    eng = _engine(S, A, c.w, c.H, K, c.norm)         # (asserts the rollout_pp<512 layout under BCMPC_F16_PP=1)
    try:
        eng.set_action_bounds(c.low, c.high)
        for src in ("explicit", "philox"):
            res = eng.get_action(c.state, c.acts[src] if src == "explicit" else None, seed=sc.SEED,
                                 cand_offset=sc.OFF, return_costs=True)
            _check(res.costs, c.costs[src], orc.near_threshold_mask(c.states[src], F16_NEAR), c.H,
                   f"{label} S={S} A={A} {src}")
            i = res.best_index - sc.OFF
            assert i == int(np.argmin(res.costs)) and np.array_equal(res.first_action, c.acts[src][0, i])
        return eng.info()
    finally:
        eng.close()


@pytest.mark.parametrize("shape", F16_SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@a_gpu_fault_stops_the_run
def test_f16_auto(shape, monkeypatch):
    monkeypatch.delenv("BCMPC_F16_PP", raising=False)
    f16_case(shape[0], shape[1], sc.K, "auto")


@pytest.mark.parametrize("shape", F16_SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
@a_gpu_fault_stops_the_run
def test_f16_pipelined(shape, monkeypatch):
    monkeypatch.setenv("BCMPC_F16_PP", "1")
    info = f16_case(shape[0], shape[1], sc.K_PP, "pp")
    assert info["layout"].startswith("rollout_pp<512"), info

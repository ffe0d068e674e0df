"""Declarative cost terms on the GPU (csrc/term_cost.hip, BCMPC_COST_TERMS engines).

The definition is cost_functions.TermCost.__call__ (NumPy f64, term order) summed by trajectory_cost_fn; the
kernel must reproduce it BIT FOR BIT on the trajectory and actions it was given -- every comparison against
TermCost below is np.array_equal with equal NaN positions.  Only test 4 has a tolerance (two different
operation orders of the same f64 sum), derived there.  Nets: oracle.synthetic_weights, 2 x 64 tanh; the
engine shape S = 11, A = 3 is one no cheetah engine accepts.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S11, A3 = 11, 3
BIG = (1 << 32) + 12345


def _t():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(x):
    torch, dev = _t()
    return torch.from_numpy(np.array(x, dtype=np.float64, order="C", copy=True)).to(dev)


def _empty(*shape):
    torch, dev = _t()
    return torch.full(shape, np.nan, dtype=torch.float64, device=dev)


def _stream():
    torch, dev = _t()
    return torch.cuda.current_stream(dev).cuda_stream


def _record(raw, A):
    rec = raw.cpu().numpy().view(np.float64)
    return int(rec[:1].view(np.int64)[0]), float(rec[1]), rec[2:2 + A].copy()


def term_total(T, traj, acts):
    """trajectory_cost_fn(T, ...) on a [H+1, K, S] trajectory and [H, K, A] actions."""
    from bc_mpc_amd.cost_functions import trajectory_cost_fn
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(trajectory_cost_fn(T, traj[:-1], acts, traj[1:]), dtype=np.float64)


def same(got, want, label=""):
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (
        f"{label}: {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} of {got.size} differ")


class Net:
    """One shape's weights, normalisation, states and engines (shared by the tests, read-only)."""

    def __init__(self, S, A):
        from oracle import mpc_oracle as orc
        self.S, self.A = S, A
        self.w = orc.synthetic_weights(S, A, 64, 2, "tanh", False)
        self.norm = orc.synthetic_normalization(S, A)
        self.dyn = orc.NumpyDynamics(self.w, self.norm)
        self.states = np.stack([orc.synthetic_state(self.norm, seed=11 + b) for b in range(3)])
        self.states.setflags(write=False)
        self.low, self.high = -np.ones(A), np.ones(A)
        self._engines = {}

    def engine(self, kernel, K, H, cost="terms", terms=None, weights=True):
        from bc_mpc_amd.engine import MLPSpec, RolloutEngine
        key = (kernel, K, H, cost)
        if key not in self._engines:
            w = self.w
            eng = RolloutEngine(self.S, self.A, 64, 2, "tanh", False, H, K, device=0, kernel=kernel, cost=cost)
            if kernel != "auto":
                assert eng.info()["kernel"] == kernel
            if weights:
                eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation), self.norm, 1)
            self._engines[key] = eng
        eng = self._engines[key]
        if terms is not None:
            eng.set_cost_terms(terms)
        return eng


@functools.lru_cache(maxsize=None)
def net(S, A) -> Net:
    return Net(S, A)


def rich_terms(S, A, n=32):
    """n terms: every kind, source and cmp; dim S - 1 and action A - 1; thresholds on values hand_traj plants."""
    from bc_mpc_amd import cost_functions as cf
    vals = [0.2, 0.0, -0.5, 0.25]
    terms = [cf.threshold(S - 1, ">=", 0.2, 10.0), cf.threshold(S - 1, ">", 0.2, 7.0),
             cf.threshold(0, "<=", 0.0, 5.0), cf.threshold(0, "<", 0.0, 3.0),
             cf.threshold(A - 1, ">=", -0.5, 2.0, on="action"), cf.threshold(A - 1, ">", -0.5, 1.5, on="action"),
             cf.threshold(0, "<=", 0.25, 1.25, on="action"), cf.threshold(0, "<", 0.25, 0.75, on="action"),
             cf.progress(S - 1, 0.01), cf.progress(1, -0.05, 2.5),
             cf.quadratic(A - 1, 0.1, on="action"), cf.quadratic(0, 0.1, on="action"),
             cf.linear(S - 1, -0.3, on="next_state"), cf.quadratic(2, 1.5, target=0.7, on="next_state"),
             cf.linear(3, 0.01), cf.quadratic(4, 2.0, target=-1.25)]
    rs = np.random.RandomState(S * 100 + A)
    i = 0
    while len(terms) < n:
        on = ("state", "next_state", "action")[i % 3]
        idx = int(rs.randint(A if on == "action" else S))
        terms.append(cf.threshold(idx, (">=", ">", "<=", "<")[(i // 3) % 4], vals[i % 4], float(i + 1), on=on))
        i += 1
    return cf.TermCost(terms[:n])


def hand_traj(S, A, K, H, seed=0):
    """A hand-made trajectory and action array: a third of the entries exactly on the thresholds of
    rich_terms (so that >= / > and <= / < disagree), one candidate all NaN, one +inf, one -inf."""
    rs = np.random.RandomState(1000 * K + 10 * H + S + seed)
    traj = rs.standard_normal((H + 1, K, S))
    acts = rs.uniform(-1, 1, (H, K, A))
    for arr in (traj, acts):
        flat = arr.reshape(-1)
        pos = rs.choice(flat.size, flat.size // 3, replace=False)
        flat[pos] = np.resize([0.2, 0.0, -0.5, 0.25, -0.0], pos.size)
    if K >= 37:
        traj[:, 5, :], traj[:, 17, :], traj[:, 30, :] = np.nan, np.inf, -np.inf
        traj[H // 2, 9, S - 1] = np.nan                    # one NaN entry in an otherwise finite candidate
        acts[0, 11, A - 1] = np.nan
    return traj, acts


# ------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("S,A", [(5, 2), (20, 6)])
@pytest.mark.parametrize("H", [1, 7])
@pytest.mark.parametrize("K", [1, 37, 64, 65, 400])
def test_kernel_on_hand_made_trajectories(S, A, H, K):
    from bc_mpc_amd import cost_functions as cf
    nt = net(S, A)
    # (the kernel needs no weights: the engine only lends its H, S, A and action bounds)
    eng = nt.engine("auto", 64, H, weights=False)
    traj, acts = hand_traj(S, A, K, H)
    d_traj, d_acts = _dev(traj), _dev(acts)
    st = _stream()
    full = rich_terms(S, A, 32)
    no_action = cf.TermCost([t for t in full.terms if t.source != cf.ACTION][:12])
    cases = [("32 terms", full), ("0 terms", cf.TermCost()), ("9 terms", cf.TermCost(full.terms[:9])),
             ("16 terms", cf.TermCost(full.terms[:16])),
             ("12 dims", cf.TermCost([cf.linear(i, 0.5) for i in range(min(S, 12))] + [cf.linear(0, -2.0, on="action")])),
             ("no action term", no_action), ("one term", cf.TermCost([cf.progress(S - 1, 0.01)]))]
    for label, T in cases:
        eng.set_cost_terms(T)
        d_costs = _empty(K + 8)                               # (the tail must stay untouched)
        eng.trajectory_cost_async(d_traj.data_ptr(), K, d_costs.data_ptr(), d_actions=d_acts.data_ptr(), stream=st)
        got = d_costs.cpu().numpy()
        assert np.isnan(got[K:]).all(), f"{label}: wrote past K"
        want = term_total(T, traj, acts)
        same(got[:K], want, f"S={S} H={H} K={K} {label}")
        if label == "32 terms" and K >= 37:
            assert np.isnan(want[5]) and np.isnan(want[9]) and np.isnan(want[11]) and np.isfinite(want[0])
        if label == "0 terms":
            assert not got[:K].any()
    if K >= 64 and H == 7:
        # the planted values sit exactly on the thresholds: >= and > (<= and <) must disagree somewhere
        from bc_mpc_amd.cost_functions import TermCost, threshold
        ge = term_total(TermCost([threshold(S - 1, ">=", 0.2, 1.0)]), traj, acts)
        gt = term_total(TermCost([threshold(S - 1, ">", 0.2, 1.0)]), traj, acts)
        assert (ge[np.isfinite(ge)] != gt[np.isfinite(ge)]).any()


# ------------------------------------------------------------------ 2. action sources
@pytest.mark.parametrize("S,A", [(5, 2), (20, 6)])
def test_action_sources(S, A):
    from bc_mpc_amd import cost_functions as cf
    from oracle import mpc_oracle as orc
    nt = net(S, A)
    K, H, seed = 65, 7, 0x7E57C057
    T = cf.TermCost([cf.quadratic(j, 0.1, on="action") for j in range(A)]
                    + [cf.threshold(A - 1, ">=", 0.0, 3.0, on="action"), cf.linear(0, 0.5, on="action"),
                       cf.progress(S - 1, 0.01)])
    eng = nt.engine("auto", 64, H, terms=T, weights=False)
    low, high = np.linspace(-1.0, -0.5, A), np.linspace(0.75, 2.0, A)
    eng.set_action_bounds(low, high)
    try:
        traj, acts = hand_traj(S, A, K, H, seed=1)
        d_traj = _dev(traj)
        st = _stream()
        rs = np.random.RandomState(3)
        mu, sd = rs.uniform(-0.6, 0.6, (H, A)), rs.uniform(0.1, 2.0, (H, A))     # (sd 2: samples clip)
        d_mu, d_sd, d_acts = _dev(mu), _dev(sd), _dev(acts)
        sources = [
            ("explicit", dict(d_actions=d_acts.data_ptr()), acts),
            ("philox", dict(seed=seed, cand_offset=1000), orc.device_rng_actions(seed, 1000, K, H, low, high)),
            ("philox big offset", dict(seed=seed, cand_offset=BIG), orc.device_rng_actions(seed, BIG, K, H, low, high)),
            ("cem it=2", dict(seed=seed, cand_offset=1000, d_mu=d_mu.data_ptr(), d_sigma=d_sd.data_ptr(), cem_iter=2),
             orc.cem_actions(seed, 2, 1000, K, H, mu, sd, low, high)),
        ]
        for label, kw, want_acts in sources:
            d_costs = _empty(K)
            eng.trajectory_cost_async(d_traj.data_ptr(), K, d_costs.data_ptr(), stream=st, **kw)
            same(d_costs.cpu().numpy(), term_total(T, traj, want_acts), f"S={S} {label}")
        clipped = orc.cem_actions(seed, 2, 1000, K, H, mu, sd, low, high)
        assert (clipped == high).any() and (clipped == low).any()
    finally:
        eng.set_action_bounds(nt.low, nt.high)


# ------------------------------------------------------------------ 3. engine end to end, S = 11, A = 3
def hopper_like_terms():
    """A Hopper-style cost on an 11-dim state: height and pitch thresholds, forward progress, control cost."""
    from bc_mpc_amd import cost_functions as cf
    return cf.TermCost([cf.threshold(0, "<", 0.7, 10.0, on="next_state"), cf.threshold(1, ">=", 0.2, 10.0),
                        cf.threshold(1, "<=", -0.2, 10.0), cf.progress(5, 0.008), cf.linear(10, 0.05)]
                       + [cf.quadratic(j, 0.001, on="action") for j in range(A3)])


def _engine_or_skip(nt, kernel, K, H, **kw):
    try:
        return nt.engine(kernel, K, H, **kw)
    except ValueError as e:
        if kernel != "team":
            raise
        pytest.skip(f"bcmpc_create does not take this shape on the team kernel: {e}")


@pytest.mark.parametrize("kernel", ["solo", "group4", "split2", "team"])
@pytest.mark.parametrize("explicit", [False, True])
def test_engine_end_to_end_on_an_11_dim_task(kernel, explicit):
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import RolloutEngine
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    nt = net(S11, A3)
    K, H, seed, off = 37, 5, 0xC0FFEE, 2000
    with pytest.raises(ValueError, match="state_dim >= 18"):
        RolloutEngine(S11, A3, 64, 2, "tanh", False, H, K, device=0, kernel="auto", cost="cheetah")
    T = hopper_like_terms()
    eng = _engine_or_skip(nt, kernel, K, H, terms=T)
    assert eng.info()["layout"].endswith("+terms")
    state = nt.states[0]
    acts = (np.random.RandomState(7).uniform(-1, 1, (H, K, A3)) if explicit
            else orc.device_rng_actions(seed, off, K, H, nt.low, nt.high))
    d_state, d_acts = _dev(state), (_dev(acts) if explicit else None)
    d_costs, d_traj = _empty(K), _empty(H + 1, K, S11)
    d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    eng.rollout_async(d_state.data_ptr(), 0, d_acts.data_ptr() if explicit else None, seed, off, d_costs.data_ptr(),
                      d_traj.data_ptr(), d_res.data_ptr(), _stream())
    costs, traj = d_costs.cpu().numpy(), d_traj.cpu().numpy()
    eng.check_status()
    assert np.array_equal(traj[0], np.tile(state, (K, 1))) and np.isfinite(traj).all()
    # the trajectory is the model's, at the state bar of the size sweep (size_cases.state_bar: the f32 base bar
    # widened per entry by the oracle's own rounding spread)
    from size_cases import no_cost, state_bar
    _, ref_traj = orc.rollout(nt.dyn, state, acts, cost_fn=no_cost)
    bar, _ = state_bar(nt.w, nt.norm, state, acts, ref_traj, f"{kernel} S={S11} A={A3}")
    assert (np.abs(traj - ref_traj) <= bar).all(), f"worst |dstate| / bar = {np.max(np.abs(traj - ref_traj) / bar):.2f}"
    same(costs, term_total(T, traj, acts), f"{kernel} rollout_async")
    index, cost, first = _record(d_res, A3)
    best = int(np.argmin(costs))
    assert index == off + best and cost == costs[best] and np.array_equal(first, acts[0, best])
    assert len(np.unique(costs)) > K // 2
    # the synchronous call: the trajectory stays in the engine's scratch, same kernels, same bits
    res = eng.get_action(state, acts if explicit else None, seed=seed, cand_offset=off, return_costs=True)
    same(res.costs, costs, f"{kernel} get_action")
    assert res.best_index == off + best and res.best_cost == costs[best] and np.array_equal(res.first_action, acts[0, best])
    lean = eng.get_action(state, acts if explicit else None, seed=seed, cand_offset=off)
    assert lean.best_index == off + best and np.array_equal(lean.first_action, acts[0, best])


def test_terms_engine_states_and_refusals():
    from bc_mpc_amd import _lib
    from bc_mpc_amd.cost_functions import TermCost, linear
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    nt = net(S11, A3)
    eng = RolloutEngine(S11, A3, 64, 2, "tanh", False, 3, 16, device=0, cost="terms")
    try:
        eng.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, "tanh"), nt.norm, 1)
        with pytest.raises(_lib.BcmpcError, match="bcmpc_set_cost_terms has not been called"):
            eng.get_action(nt.states[0])
        d = _empty(4 * 16 * S11)
        with pytest.raises(_lib.BcmpcError, match="bcmpc_set_cost_terms has not been called"):
            eng.trajectory_cost_async(d.data_ptr(), 16, d.data_ptr())
        arr = (_lib.CostTerm * 33)()
        lib = _lib.load()
        assert lib.bcmpc_set_cost_terms(eng._h, arr, 33) == _lib.ERR_ARG
        bad = [dict(kind=4), dict(source=3), dict(cmp=4), dict(index=S11), dict(source=2, index=A3), dict(index=-1),
               dict(kind=1, source=1, param=0.01), dict(kind=1, param=0.0), dict(weight=float("inf")),
               dict(param=float("nan"))]
        for kw in bad:
            t = _lib.CostTerm(kind=0, source=0, index=0, cmp=0, weight=1.0, param=0.0)
            for k, v in kw.items():
                setattr(t, k, v)
            assert lib.bcmpc_set_cost_terms(eng._h, ctypes.byref(t), 1) == _lib.ERR_ARG, kw
        with pytest.raises(_lib.BcmpcError):                        # still none set: the bad calls left no list
            eng.get_action(nt.states[0])
        eng.set_cost_terms(TermCost([linear(0, 1.0)]))
        eng.get_action(nt.states[0])
        with pytest.raises(ValueError, match="NumPy-stream"):
            eng.get_action_numpy_stream(nt.states[0], nt.low, nt.high, 16, return_costs=True)
    finally:
        eng.close()
    # only a cost="terms" engine takes terms
    other = nt.engine("auto", 16, 3, cost="none")
    with pytest.raises(ValueError, match="BCMPC_COST_TERMS"):
        other.set_cost_terms(TermCost([linear(0, 1.0)]))


def test_a_team_that_gives_up_reruns_with_the_same_terms(monkeypatch):
    """BCMPC_TEAM_SPINS=-1 (the suite's hook: the team launch is skipped and reported as a team that gave up):
    the synchronous call reruns on the fallback engine, which must score with the same terms -- its costs are
    those of a split1 engine (the layout the fallback takes at this K), bit for bit."""
    nt = net(S11, A3)
    K, H, seed = 37, 5, 77
    T = hopper_like_terms()
    team = _engine_or_skip(nt, "team", K, H, terms=T)
    want = nt.engine("split1", K, H, terms=T).get_action(nt.states[1], None, seed=seed, return_costs=True)
    before = team.team_reruns
    monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
    got = team.get_action(nt.states[1], None, seed=seed, return_costs=True)
    monkeypatch.delenv("BCMPC_TEAM_SPINS")
    assert team.team_reruns == before + 1
    same(got.costs, want.costs, "fallback engine")
    assert got.best_index == want.best_index and np.array_equal(got.first_action, want.first_action)
    # new terms reach the fallback engine that now exists
    from bc_mpc_amd.cost_functions import TermCost, linear
    T2 = TermCost([linear(3, 1.0, on="next_state")])
    team.set_cost_terms(T2)
    want2 = nt.engine("split1", K, H, terms=T2).get_action(nt.states[1], None, seed=seed, return_costs=True)
    monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
    got2 = team.get_action(nt.states[1], None, seed=seed, return_costs=True)
    monkeypatch.delenv("BCMPC_TEAM_SPINS")
    same(got2.costs, want2.costs, "fallback engine, second list")
    assert not np.array_equal(got2.costs, got.costs)


# ------------------------------------------------------------------ 4. cheetah as terms vs the fused cost
@pytest.mark.parametrize("kernel", ["solo", "group4", "split2", "team"])
def test_cheetah_terms_against_the_fused_cheetah_cost(kernel):
    """One cheetah engine returns costs and trajectory from ONE launch; the term kernel scores that same
    trajectory.  Same states means same comparisons (no +-10 flips); what can differ is the order of the
    f64 operations of sum_h (pen_h - d_h / 0.01): at most 4 roundings per step, each <= 2^-53 relative to a
    partial sum bounded by sum_h |c_h|, i.e. <= 4 H 2^-53 (1 + sum |c_h|) ~ 2e-15 at H = 5.  The issue's bar
    |delta| <= 1e-12 (1 + sum_h |c_h|) leaves two orders of magnitude."""
    from bc_mpc_amd.cost_functions import cheetah_terms
    nt = net(20, 6)
    K, H, seed = 400, 5, 99
    T = cheetah_terms()
    fused = _engine_or_skip(nt, kernel, K, H, cost="cheetah")
    terms = nt.engine("auto", 64, H, terms=T, weights=False)
    # a state on the heading thresholds' side where penalties fire for part of the candidates
    state = nt.states[1].copy()
    state[5], state[6], state[7] = 0.2, -1e-3, 1e-3
    d_state, d_costs, d_traj = _dev(state), _empty(K), _empty(H + 1, K, 20)
    fused.rollout_async(d_state.data_ptr(), 0, None, seed, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, _stream())
    d_tc = _empty(K)
    terms.trajectory_cost_async(d_traj.data_ptr(), K, d_tc.data_ptr(), stream=_stream())
    want, got, traj = d_costs.cpu().numpy(), d_tc.cpu().numpy(), d_traj.cpu().numpy()
    fused.check_status()
    acts = np.zeros((H, K, 6))
    same(got, term_total(T, traj, acts), f"{kernel}: kernel vs TermCost")
    mag = sum(np.abs(T(traj[h], acts[h], traj[h + 1])) for h in range(H))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    delta = np.abs(got - want)
    bitwise = bool(np.array_equal(got, want))
    print(f"cheetah-as-terms vs fused [{kernel}] K={K} H={H}: bitwise={bitwise} max|delta|={delta.max():.3e} "
          f"max delta/(1+sum|c_h|)={np.max(delta / (1 + mag)):.3e}")
    assert (mag > 10).any(), "no penalty fired: the case does not exercise the thresholds"
    assert (delta <= 1e-12 * (1 + mag)).all()


# ------------------------------------------------------------------ 5. planners
ELITE = np.dtype([("cost", "<f8"), ("index", "<i8")])


def one_iteration(eng, nt, T, state, mu, sd, seed, it, off):
    """Iteration `it` of a CEM / MPPI round for the K candidates at `off`, from the single-environment
    blocks: the sampled actions rolled out as an explicit array give the trajectory; its costs must be
    TermCost's bit for bit, and cem_rollout_async (actions regenerated in both kernels) must give the same."""
    from oracle import mpc_oracle as orc
    K, H = eng.num_paths, eng.horizon
    acts = orc.cem_actions(seed, it, off, K, H, mu, sd, nt.low, nt.high)
    d_state, d_acts, d_costs, d_traj = _dev(state), _dev(acts), _empty(K), _empty(H + 1, K, nt.S)
    st = _stream()
    eng.rollout_async(d_state.data_ptr(), 0, d_acts.data_ptr(), seed, off, d_costs.data_ptr(), d_traj.data_ptr(),
                      None, st)
    costs = d_costs.cpu().numpy()
    same(costs, term_total(T, d_traj.cpu().numpy(), acts), f"it={it} off={off}: costs vs TermCost")
    d_mu, d_sd, d_c2 = _dev(mu), _dev(sd), _empty(K)
    eng.cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sd.data_ptr(), seed, it, off, off + K,
                          d_c2.data_ptr(), None, False, st)
    same(d_c2.cpu().numpy(), costs, f"it={it} off={off}: cem_rollout_async")
    eng.check_status()
    return costs, acts, d_costs


def cem_step(eng, d_costs, mu, sd, seed, it, off, E, alpha):
    torch, dev = _t()
    K, st = eng.num_paths, _stream()
    d_el = torch.zeros(E * ELITE.itemsize, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_mu, d_sd = _dev(mu), _dev(sd)
    eng.select_async(None, d_costs.data_ptr(), K, off, E, d_el.data_ptr(), d_cnt.data_ptr(), st)
    eng.cem_refit_async(d_el.data_ptr(), d_cnt.data_ptr(), seed, it, alpha, d_mu.data_ptr(), d_sd.data_ptr(), st)
    return d_mu.cpu().numpy(), d_sd.cpu().numpy()


def mppi_step(eng, d_costs, mu, sd, seed, it, off, lam):
    from bc_mpc_amd import _lib
    torch, dev = _t()
    d_mu, d_sd = _dev(mu), _dev(sd)
    d_stats = torch.zeros(ctypes.sizeof(_lib.MppiStats), dtype=torch.uint8, device=dev)
    eng.mppi_update_async(d_costs.data_ptr(), eng.num_paths, off, seed, it, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                          d_stats.data_ptr(), _stream())
    return d_mu.cpu().numpy(), d_stats.cpu().numpy().tobytes()


def plans(B, H, A):
    rs = np.random.RandomState(100 + B)
    return rs.uniform(-0.6, 0.6, (B, H, A)), rs.uniform(0.1, 0.6, (B, H, A))


@pytest.mark.parametrize("kernel", ["group4", "split2"])
def test_single_planners_on_a_terms_engine(kernel):
    nt = net(S11, A3)
    K, H, seed, iters, E, alpha, lam = 37, 5, 0x5EED5, 2, 5, 0.1, 0.7
    T = hopper_like_terms()
    eng = nt.engine(kernel, K, H, terms=T)
    state = nt.states[2]
    mu0, sd0 = (x[0] for x in plans(1, H, A3))
    for planner in ("cem", "mppi"):
        mu, sd, all_costs, all_acts = mu0, sd0, [], []
        for it in range(iters):
            costs, acts, d_costs = one_iteration(eng, nt, T, state, mu, sd, seed, it, 0)
            all_costs.append(costs)
            all_acts.append(acts)
            if planner == "cem":
                mu, sd = cem_step(eng, d_costs, mu, sd, seed, it, 0, E, alpha)
            else:
                mu, stats = mppi_step(eng, d_costs, mu, sd, seed, it, 0, lam)
        cat = np.concatenate(all_costs)
        best = int(np.argmin(cat))
        if planner == "cem":
            res, mu1, sd1 = eng.cem_get_action(state, mu0, sd0, iters, E, alpha, seed)
            assert mu1.tobytes() == mu.tobytes() and sd1.tobytes() == sd.tobytes()
        else:
            res, mu1, st1 = eng.mppi_get_action(state, mu0, sd0, iters, lam, seed)
            assert mu1.tobytes() == mu.tobytes() and bytes(st1) == stats
        assert res.best_index == best and res.best_cost == cat[best], planner
        assert np.array_equal(res.first_action, all_acts[best // K][0, best % K])


@pytest.mark.parametrize("kernel", ["group4", "split2"])
def test_batched_planners_equal_the_single_calls(kernel):
    """B = 3 environments x K = 37 candidates: environment boundaries fall inside the kernels' 64-lane
    tiles.  Environment b == the single call at cand_offset + b K on a K-candidate engine of the same
    layout, bit for bit (the contract of get_actions and of the batched planners)."""
    nt = net(S11, A3)
    B, K, H, seed, off, iters, E, alpha, lam = 3, 37, 5, 0xBA7C4, 1000, 2, 5, 0.1, 0.7
    T = hopper_like_terms()
    one = nt.engine(kernel, K, H, terms=T)
    many = nt.engine(kernel, B * K, H, terms=T)
    states = nt.states[:B]
    # random shooting
    res = many.get_actions(states, None, seed=seed, cand_offset=off, return_costs=True)
    for b in range(B):
        r1 = one.get_action(states[b], None, seed=seed, cand_offset=off + b * K, return_costs=True)
        same(res.costs[b], r1.costs, f"get_actions env {b}")
        assert res.best_index[b] == r1.best_index == off + b * K + int(np.argmin(r1.costs))
        assert res.best_cost[b] == r1.best_cost and np.array_equal(res.first_action[b], r1.first_action)
    assert len({c.tobytes() for c in res.costs}) == B
    # CEM and MPPI: every iteration's costs against the single blocks (which one_iteration holds to TermCost)
    mu0, sd0 = plans(B, H, A3)
    rc, mu_c, sd_c = many.cem_get_actions(states, mu0, sd0, iters, E, alpha, seed, cand_offset=off, return_costs=True)
    rm, mu_m, st_m = many.mppi_get_actions(states, mu0, sd0, iters, lam, seed, cand_offset=off, return_costs=True)
    for b in range(B):
        ob = off + b * K
        for planner, r, mu_out in (("cem", rc, mu_c), ("mppi", rm, mu_m)):
            mu, sd, cat, acts_all = mu0[b], sd0[b], [], []
            for it in range(iters):
                costs, acts, d_costs = one_iteration(one, nt, T, states[b], mu, sd, seed, it, ob)
                same(r.costs[it, b], costs, f"{planner} env {b} it {it}")
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


# ------------------------------------------------------------------ 6. controllers
class _Box:
    def __init__(self, n):
        self.low, self.high, self.shape = -np.ones(n, np.float32), np.ones(n, np.float32), (n,)


class _Env:
    action_space = _Box(A3)
    observation_space = _Box(S11)


def test_mpccontroller_device_terms_equal_the_host_path():
    """The same TermCost as a TermCost (device) and wrapped in a lambda (the host path: trajectory to the
    host, scored by the callable): same NumPy seed -> the same action, the same cost vector bit for bit,
    and the global stream left at the same position."""
    from bc_mpc_amd import MPCcontroller
    nt = net(S11, A3)
    T = hopper_like_terms()
    K, H = 37, 5
    out = {}
    for name, fn in (("device", T), ("host", lambda s, a, ns: T(s, a, ns))):
        ctrl = MPCcontroller(_Env(), nt.dyn, horizon=H, cost_fn=fn, num_simulated_paths=K)
        ctrl.keep_costs = True
        np.random.seed(4242)
        acts = [ctrl.get_action(nt.states[i % 3].copy()) for i in range(3)]
        st = np.random.get_state()
        out[name] = (acts, ctrl.last_costs, ctrl.last_cost, ctrl.last_index, st, ctrl._engine.cost)
        ctrl._engine.close()
    dev, host = out["device"], out["host"]
    assert (dev[5], host[5]) == ("terms", "none")
    assert all(np.array_equal(a, b) for a, b in zip(dev[0], host[0]))
    same(dev[1], host[1], "last_costs")
    assert dev[2] == host[2] and dev[3] == host[3]
    assert dev[4][2] == host[4][2] and np.array_equal(dev[4][1], host[4][1])
    ref = np.random.RandomState(4242)
    for _ in range(3):
        paths = ref.uniform(_Env.action_space.low, _Env.action_space.high, [H, K, A3])
    assert ref.get_state()[2] == dev[4][2] and np.array_equal(ref.get_state()[1], dev[4][1])
    assert np.array_equal(dev[0][2], paths[0, dev[3]])


def test_controllers_run_a_termcost_and_agree_with_the_engine():
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller
    nt = net(S11, A3)
    T = hopper_like_terms()
    K, H, B = 37, 5, 3
    states = nt.states[:B]
    seed_of = lambda s: int(np.random.RandomState(s).randint(0, 2**62, dtype=np.int64))   # noqa: E731
    one, many = nt.engine("auto", K, H, terms=T), nt.engine("auto", B * K, H, terms=T)
    # random shooting, actions drawn in the kernel
    ctrl = MPCcontroller(_Env(), nt.dyn, horizon=H, cost_fn=T, num_simulated_paths=K, rng="device", seed=5)
    a = ctrl.get_action(states[0])
    r = one.get_action(states[0], None, seed=seed_of(5))
    assert ctrl._engine.cost == "terms" and np.array_equal(a, r.first_action) and ctrl.last_index == r.best_index
    ctrl = MPCcontroller(_Env(), nt.dyn, horizon=H, cost_fn=T, num_simulated_paths=K, rng="device", seed=6)
    a = ctrl.get_actions(states)
    r = many.get_actions(states, None, seed=seed_of(6))
    assert a.shape == (B, A3) and np.array_equal(a, r.first_action) and np.array_equal(ctrl.last_index, r.best_index)
    # CEM and MPPI, single and batched
    cem = CEMcontroller(_Env(), nt.dyn, horizon=H, cost_fn=T, num_simulated_paths=K, iterations=2, n_elite=5, seed=7)
    mu0, sd0 = cem.initial_distribution()
    a = cem.get_action(states[0])
    r, mu, sd = one.cem_get_action(states[0], mu0, sd0, 2, 5, cem.alpha, seed_of(7))
    assert np.array_equal(a, r.first_action) and cem.last_cost == r.best_cost and np.array_equal(cem.last_mu, mu)
    cem = CEMcontroller(_Env(), nt.dyn, horizon=H, cost_fn=T, num_simulated_paths=K, iterations=2, n_elite=5, seed=8)
    mu0, sd0 = cem.batch_initial_distribution(B)
    a = cem.get_actions(states)
    r, mu, sd = many.cem_get_actions(states, mu0, sd0, 2, 5, cem.alpha, seed_of(8))
    assert np.array_equal(a, r.first_action) and np.array_equal(cem.last_mu, mu) and np.array_equal(cem.last_sigma, sd)
    mp = MPPIcontroller(_Env(), nt.dyn, horizon=H, cost_fn=T, num_simulated_paths=K, temperature=0.7, iterations=2, seed=9)
    mu0, sd0 = mp.initial_distribution()
    a = mp.get_action(states[0])
    r, mu, stats = one.mppi_get_action(states[0], mu0, sd0, 2, 0.7, seed_of(9))
    assert np.array_equal(a, mu[0]) and mp.last_cost == r.best_cost and mp.last_ess == float(stats.ess)
    mp = MPPIcontroller(_Env(), nt.dyn, horizon=H, cost_fn=T, num_simulated_paths=K, temperature=0.7, iterations=2, seed=10)
    mu0, sd0 = mp.batch_initial_distribution(B)
    a = mp.get_actions(states)
    r, mu, stats = many.mppi_get_actions(states, mu0, sd0, 2, 0.7, seed_of(10))
    assert np.array_equal(a, mu[:, 0]) and np.array_equal(mp.last_cost, r.best_cost)
    for c in (cem, mp):
        assert c._batch_engine.cost == "terms" and c._batch_engine.info()["layout"].endswith("+terms")


# ------------------------------------------------------------------ 7. graph capture
def test_rollout_async_on_a_terms_engine_replays_in_a_graph():
    """rollout_async (no d_traj: the engine's scratch) captured into a graph: the replay gives the eager
    launch's bits, also after the inputs change -- nothing in the chain allocates."""
    from bc_mpc_amd import _lib
    torch, dev = _t()
    nt = net(S11, A3)
    K, H, seed = 37, 5, 31337
    T = hopper_like_terms()
    eng = nt.engine("group4", K, H, terms=T)
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

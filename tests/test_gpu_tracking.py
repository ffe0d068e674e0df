"""Reference tracking on the GPU (the extended variant of csrc/term_cost.hip): per-call reference channels and action-rate terms.

The definition is cost_functions.episode_cost with ``reference`` / ``previous_action``; every comparison below is
bit for bit (np.array_equal with equal NaN positions) on the trajectory and the actions the kernel was given.
Nets: oracle.synthetic_weights, 2 x 64 tanh, S = 11, A = 3 for the engine tests.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S11, A3 = 11, 3


def _t():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(x, dtype=np.float64):
    torch, dev = _t()
    return torch.from_numpy(np.array(x, dtype=dtype, order="C", copy=True)).to(dev)


def _empty(*shape):
    torch, dev = _t()
    return torch.full(shape, np.nan, dtype=torch.float64, device=dev)


def _steps(K):
    torch, dev = _t()
    return torch.full((K,), -7, dtype=torch.int32, device=dev)


def _stream():
    torch, dev = _t()
    return torch.cuda.current_stream(dev).cuda_stream


def same(got, want, label=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (
        f"{label}: {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} of {got.size} differ")


def definition(T, traj, acts, ref=None, prev=None):
    """episode_cost for one environment: ``ref`` ``[R]`` or ``[H, R]`` (broadcast over the candidates), ``prev`` ``[A]``."""
    from bc_mpc_amd.cost_functions import episode_cost
    if ref is not None and np.ndim(ref) == 2:
        ref = np.asarray(ref)[:, None, :]
    return episode_cost(T, traj[:-1], acts, traj[1:], reference=ref, previous_action=prev)


class Net:
    """One shape's weights, normalisation, states and engines (shared by the tests, read-only)."""

    def __init__(self, S, A):
        from oracle import mpc_oracle as orc
        self.S, self.A = S, A
        self.w = orc.synthetic_weights(S, A, 64, 2, "tanh", False)
        self.norm = orc.synthetic_normalization(S, A)
        self.dyn = orc.NumpyDynamics(self.w, self.norm)
        self.states = np.stack([orc.synthetic_state(self.norm, seed=11 + b) for b in range(5)])
        self.states.setflags(write=False)
        self.low, self.high = -np.ones(A), np.ones(A)
        self._engines = {}

    def engine(self, kernel, K, H, terms=None, weights=True):
        from bc_mpc_amd.engine import MLPSpec, RolloutEngine
        key = (kernel, K, H)
        if key not in self._engines:
            eng = RolloutEngine(self.S, self.A, 64, 2, "tanh", False, H, K, device=0, kernel=kernel, cost="terms")
            if kernel != "auto":
                assert eng.info()["kernel"] == kernel
            if weights:
                eng.set_weights(MLPSpec(self.w.kernels, self.w.biases, self.w.activation), self.norm, 1)
            self._engines[key] = eng
        eng = self._engines[key]
        if terms is not None:
            eng.set_cost_terms(terms)
        return eng


@functools.lru_cache(maxsize=None)
def net(S, A) -> Net:
    return Net(S, A)


def _engine_or_skip(nt, kernel, K, H, **kw):
    """The team kernel takes this net and K (2 x 64 tanh, K = 37) on every MI355X: a refusal is a failure."""
    return nt.engine(kernel, K, H, **kw)


VALS = [0.2, 0.0, -0.5, 0.25]      # the values the hand-made data plants: thresholds sit exactly on them


def sized_cost(S, A, slots, done=False):
    """A cost that reads exactly ``slots`` slots (state dims + channels + actions), with channels, a rate term,
    referenced thresholds of every cmp and constant terms in it; ``done``: two done conditions on dims it reads."""
    from bc_mpc_amd import cost_functions as cf
    n_act = min(A, max(1, slots // 4))
    n_state = min(S, max(1, (slots - n_act) // 2))
    n_ref = slots - n_act - n_state
    assert 1 <= n_ref <= 16, (S, A, slots)
    terms = []
    for j in range(n_act):
        terms.append(cf.rate(j, 0.5 + j))
        if j % 2:
            terms.append(cf.quadratic(j, 0.1, on="action"))
    for c in range(n_ref):
        i, on = c % n_state, ("state", "next_state")[c % 2]
        if c % 3 == 0:
            terms.append(cf.quadratic(i, 1.0 + c, target=cf.ref(c), on=on))
        else:
            terms.append(cf.threshold(i, (">=", ">", "<=", "<")[c % 4], cf.ref(c), 2.0 + c, on=on))
    terms.append(cf.quadratic(A - 1 if n_act == A else 0, 0.3, target=cf.ref(0), on="action"))
    for i in range(n_state):
        terms.append(cf.threshold(i, ">=", 0.2, 1.5) if i % 2 else cf.linear(i, -0.25, on="next_state"))
    terms.append(cf.progress(0, 0.01))
    terms = terms[:32 - (2 if done else 0)]
    T = cf.TermCost(terms, done=[cf.done_when(0, ">", 1.6), cf.done_when(n_state - 1, "<", -1.8)] if done else (),
                    done_cost=3.5 if done else 0.0)
    assert T.n_slots == slots and T.n_ref == n_ref and T.uses_rate, (T.n_slots, slots, T.n_ref, n_ref)
    return T


def hand_data(S, A, K, H, R, B=1, seed=0, wild_ref=False):
    """A trajectory, actions, references ``[B, H, R]`` and previous actions ``[B, A]``: a third of the entries on
    the planted values (so >= / > and <= / < disagree on referenced thresholds), NaN / +-inf candidates, +-inf
    in channel 1 (a threshold's in the costs here) and, with ``wild_ref``, a NaN reference row and an inf target."""
    rs = np.random.RandomState(1000 * K + 10 * H + S + seed)
    traj = rs.standard_normal((H + 1, K, S))
    acts = rs.uniform(-1, 1, (H, K, A))
    ref = rs.standard_normal((B, H, R))
    prev = rs.uniform(-1, 1, (B, A))
    for arr in (traj, acts, ref, prev):
        flat = arr.reshape(-1)
        pos = rs.choice(flat.size, flat.size // 3, replace=False)
        flat[pos] = np.resize(VALS + [-0.0], pos.size)
    if K >= 37:
        traj[:, 5, :], traj[:, 17, :], traj[:, 30, :] = np.nan, np.inf, -np.inf
        acts[0, 11, A - 1] = np.nan
        acts[H - 1, 12, 0] = np.inf
    if H >= 7 and R > 1:
        ref[0, 4, 1], ref[B - 1, 5, 1] = np.inf, -np.inf
    if wild_ref:
        ref[0, 2, :] = np.nan
        ref[0, 4, 0] = np.inf
    return traj, acts, ref, prev


def run_kernel(eng, traj, acts, ref, prev, env_paths, steps=False, **kw):
    """The stream-ordered block on uploaded inputs: (costs [K], steps [K] or None); the tail must stay untouched."""
    K = traj.shape[1]
    d_traj, d_costs = _dev(traj), _empty(K + 8)
    d_acts = _dev(acts) if acts is not None else None
    d_ref = _dev(ref) if ref is not None else None
    d_prev = _dev(prev) if prev is not None else None
    d_steps = _steps(K) if steps else None
    eng.trajectory_cost_inputs_async(
        d_traj.data_ptr(), K, d_costs.data_ptr(), env_paths,
        d_ref=d_ref.data_ptr() if ref is not None else None, ref_envs=ref.shape[0] if ref is not None else 1,
        ref_steps=ref.shape[1] if ref is not None else 1,
        d_prev=d_prev.data_ptr() if prev is not None else None, prev_envs=prev.shape[0] if prev is not None else 1,
        d_actions=d_acts.data_ptr() if acts is not None else None, stream=_stream(),
        d_term_step=d_steps.data_ptr() if steps else None, **kw)
    got = d_costs.cpu().numpy()
    assert np.isnan(got[K:]).all(), "wrote past K"
    return got[:K], (d_steps.cpu().numpy() if steps else None)


# ------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("S,A", [(5, 2), (20, 6)])
@pytest.mark.parametrize("H", [1, 7, 8, 9, 17])
def test_kernel_on_hand_made_trajectories(S, A, H):
    nt = net(S, A)
    eng = nt.engine("auto", 64, H, weights=False)         # (the engine only lends its H, S, A and action bounds)
    sizes = [3, 5, 9, 17, 23] if S == 5 else [3, 5, 9, 17, 25]     # (S = 5, A = 2 has at most 5 + 2 + 16 slots)
    flips = 0
    for slots in sizes:
        for done in (False, True):
            T = sized_cost(S, A, slots, done)
            eng.set_cost_terms(T)
            for K in (1, 63, 64, 65, 130):
                traj, acts, ref, prev = hand_data(S, A, K, H, T.n_ref)
                for ref_steps in (1, H):
                    for with_prev in (False, True):
                        r = ref[:, :ref_steps]
                        p = prev if with_prev else None
                        got, steps = run_kernel(eng, traj, acts, r, p, K, steps=done)
                        want, wsteps = definition(T, traj, acts, r[0] if ref_steps > 1 else r[0, 0],
                                                  p[0] if with_prev else None)
                        label = f"S={S} H={H} K={K} slots={slots} done={done} ref_steps={ref_steps} prev={with_prev}"
                        same(got, want, label)
                        if done:
                            same(steps, wsteps, label + " steps")
                            if K >= 63 and H >= 7:
                                assert (wsteps < H).any() and (wsteps == H).any(), label
            if H >= 7 and not done:
                # the planted values sit on the referenced thresholds: >= and > must disagree somewhere
                from bc_mpc_amd import cost_functions as cf
                traj, acts, ref, prev = hand_data(S, A, 130, H, T.n_ref)
                ge = definition(cf.TermCost([cf.threshold(0, ">=", cf.ref(0), 1.0)]), traj, acts, ref[0])[0]
                gt = definition(cf.TermCost([cf.threshold(0, ">", cf.ref(0), 1.0)]), traj, acts, ref[0])[0]
                flips += int((ge != gt).sum())
    if H >= 7:
        assert flips > 0


def test_nonfinite_reference_rows_propagate():
    from bc_mpc_amd import cost_functions as cf
    S, A, K, H = 5, 2, 65, 7
    T = cf.TermCost([cf.quadratic(0, 1.0, target=cf.ref(0)), cf.threshold(1, "<=", cf.ref(1), 2.0), cf.rate(0, 1.0)])
    eng = net(S, A).engine("auto", 64, H, terms=T, weights=False)
    traj, acts, ref, prev = hand_data(S, A, K, H, 2, wild_ref=True)
    got, _ = run_kernel(eng, traj, acts, ref, prev, K)
    want, _ = definition(T, traj, acts, ref[0], prev[0])
    same(got, want)
    assert np.isnan(want).all()                            # row 2 of the reference is NaN: every candidate's cost is
    ref[0, 2, 0] = 0.25                                    # a NaN threshold value alone compares false ...
    got, _ = run_kernel(eng, traj, acts, ref, prev, K)
    want, _ = definition(T, traj, acts, ref[0], prev[0])
    same(got, want)
    assert np.isinf(want[0]) and want[0] > 0               # ... and the +inf target of row 4 gives (x - inf)^2 = inf
    ref[0, 4, 0] = -0.5
    got, _ = run_kernel(eng, traj, acts, ref, prev, K)
    want, _ = definition(T, traj, acts, ref[0], prev[0])
    same(got, want)
    assert np.isfinite(want[0])


# ------------------------------------------------------------------ 2. environment boundaries
@pytest.mark.parametrize("env_paths", [1, 50, 64, 100])
def test_environment_boundaries(env_paths):
    from bc_mpc_amd import cost_functions as cf
    S, A, H = 5, 2, 7
    T = cf.TermCost([cf.quadratic(1, 1.0, target=cf.ref(0), on="next_state"), cf.threshold(0, ">=", cf.ref(1), 4.0),
                     cf.rate(0, 2.0), cf.rate(1, 0.5), cf.linear(2, 0.1)],
                    done=[cf.done_when(3, ">", 1.7)], done_cost=2.0)
    eng = net(S, A).engine("auto", 64, H, terms=T, weights=False)
    for B in (1, 2, 3, 5):
        K = B * env_paths
        traj, acts, ref, prev = hand_data(S, A, K, H, 2, B=B, seed=B)
        ref[:, :, 0] += np.arange(B)[:, None]              # every environment's inputs differ
        prev[:, 0] = 0.1 * (1 + np.arange(B))
        got, steps = run_kernel(eng, traj, acts, ref, prev, env_paths, steps=True)
        for b in range(B):
            sl = slice(b * env_paths, (b + 1) * env_paths)
            want, wsteps = definition(T, traj[:, sl], acts[:, sl], ref[b], prev[b])
            same(got[sl], want, f"env_paths={env_paths} B={B} env {b}")
            same(steps[sl], wsteps, f"env_paths={env_paths} B={B} env {b} steps")
        if B > 1:                                          # the wrong environment would have changed the answer
            other = definition(T, traj[:, :env_paths], acts[:, :env_paths], ref[1], prev[1])[0]
            assert not np.array_equal(other, got[:env_paths], equal_nan=True)
        # one shared reference / previous action against B copies of the same data
        got1, _ = run_kernel(eng, traj, acts, ref[:1], prev[:1], env_paths)
        gotB, _ = run_kernel(eng, traj, acts, np.repeat(ref[:1], B, 0), np.repeat(prev[:1], B, 0), env_paths)
        same(got1, gotB, f"env_paths={env_paths} B={B} shared")
        same(got1, definition(T, traj, acts, ref[0], prev[0])[0], f"env_paths={env_paths} B={B} shared, definition")


# ------------------------------------------------------------------ 3. action sources for the rate term
@pytest.mark.parametrize("S,A", [(5, 2), (20, 6)])
@pytest.mark.parametrize("H", [7, 9])
def test_action_sources_for_the_rate_term(S, A, H):
    from bc_mpc_amd import cost_functions as cf
    from oracle import mpc_oracle as orc
    nt = net(S, A)
    K, seed = 65, 0x7E57C057
    T = cf.TermCost([cf.rate(j, 0.5 + j) for j in range(A)]
                    + [cf.quadratic(0, 0.1, target=cf.ref(0), on="action"), cf.progress(S - 1, 0.01)])
    eng = nt.engine("auto", 64, H, terms=T, weights=False)
    low, high = np.linspace(-1.0, -0.5, A), np.linspace(0.75, 2.0, A)
    eng.set_action_bounds(low, high)
    try:
        traj, acts, ref, prev = hand_data(S, A, K, H, 1, seed=1)
        rs = np.random.RandomState(3)
        mu, sd = rs.uniform(-0.6, 0.6, (H, A)), rs.uniform(0.1, 2.0, (H, A))
        d_mu, d_sd = _dev(mu), _dev(sd)
        sources = [
            ("explicit", acts, {}, acts),
            ("philox", None, dict(seed=seed, cand_offset=1000), orc.device_rng_actions(seed, 1000, K, H, low, high)),
            ("cem it=2", None, dict(seed=seed, cand_offset=1000, d_mu=d_mu.data_ptr(), d_sigma=d_sd.data_ptr(),
                                    cem_iter=2), orc.cem_actions(seed, 2, 1000, K, H, mu, sd, low, high)),
        ]
        for label, a, kw, want_acts in sources:
            for p in (None, prev):
                got, _ = run_kernel(eng, traj, a, ref, p, K, **kw)
                want, _ = definition(T, traj, want_acts, ref[0], None if p is None else p[0])
                same(got, want, f"S={S} H={H} {label} prev={p is not None}")
    finally:
        eng.set_action_bounds(nt.low, nt.high)


# ------------------------------------------------------------------ 3b. the two variants of the one kernel template
def _instance(n_slots):
    """<ND, PF> of launch_term_cost / launch_term_cost_x for a list of n_slots slots."""
    return (4, 8) if n_slots <= 4 else (8, 4) if n_slots <= 8 else (16, 2) if n_slots <= 16 else \
        (24, 1) if n_slots <= 24 else (32, 1)


def variant_pair(n_state, n_act, n_chan, done):
    """The same list twice: with constant thresholds / targets (the plain variant scores it) and with the first
    ``n_chan`` of those constants delivered through reference channels (the extended variant); the constants."""
    from bc_mpc_amd import cost_functions as cf
    consts, lists = [], ([], [])
    slots = [(i, "next_state" if i % 3 == 1 else "state") for i in range(n_state)] + [(j, "action") for j in range(n_act)]
    for n, (i, on) in enumerate(slots):
        v, w = VALS[n % 4], 0.5 + 0.25 * n
        for ext, terms in enumerate(lists):
            p = v
            if ext and n < n_chan:
                p = cf.ref(n)
            if n % 2:
                terms.append(cf.quadratic(i, w, target=p, on=on))
            else:
                terms.append(cf.threshold(i, (">=", ">", "<=", "<")[(n // 2) % 4], p, w, on=on))
        if n < n_chan:
            consts.append(v)
    kw = dict(done=[cf.done_when(0, ">", 1.6)], done_cost=3.5) if done else {}
    return cf.TermCost(lists[0], **kw), cf.TermCost(lists[1], **kw), np.array(consts)


@pytest.mark.parametrize("slots,n_state,n_act,n_chan", [
    (4, 1, 1, 2),        # plain  2 slots, extended  4: both <4, 8>
    (8, 3, 2, 3),        # plain  5 slots, extended  8: both <8, 4>
    (16, 7, 3, 6),       # plain 10 slots, extended 16: both <16, 2>
    (24, 13, 5, 6),      # plain 18 slots, extended 24: both <24, 1>
    (32, 20, 6, 6),      # plain 26 slots, extended 32: both <32, 1> (all of S = 20, A = 6: the channels make up 32)
])
def test_plain_and_extended_variants_agree(slots, n_state, n_act, n_chan):
    """term_cost.hip's two variants are one template: a plain list with constant thresholds and targets, and the
    same list with those constants in reference channels, give the same bits -- and the definition's.  K = 130 (two
    full waves, a two-lane tail), env_paths = 65 (a wave's lanes span two environments), H = 9 (every PF has a padded
    last trip and at least two trips); explicit and regenerated actions, with and without a done condition."""
    from oracle import mpc_oracle as orc
    S, A, K, H, seed, off = 20, 6, 130, 9, 0x5EED5, 4000
    nt = net(S, A)
    eng = nt.engine("auto", 64, H, weights=False)
    traj, acts, _, _ = hand_data(S, A, K, H, 1, seed=slots)
    d_traj, d_acts = _dev(traj), _dev(acts)
    sources = [("explicit", acts, dict(d_actions=d_acts.data_ptr()), {}),
               ("philox", orc.device_rng_actions(seed, off, K, H, nt.low, nt.high), {}, dict(seed=seed, cand_offset=off))]
    for done in (False, True):
        plain, ext, consts = variant_pair(n_state, n_act, n_chan, done)
        assert not plain.extended and ext.extended and ext.n_ref == n_chan
        assert plain.n_slots == n_state + n_act and ext.n_slots == slots
        assert _instance(plain.n_slots) == _instance(ext.n_slots)          # the same <ND, PF> on both sides
        for label, want_acts, plain_kw, kw in sources:
            want, wsteps = definition(plain, traj, want_acts)
            eng.set_cost_terms(plain)
            d_costs, d_steps = _empty(K + 8), _steps(K)
            eng.trajectory_cost_async(d_traj.data_ptr(), K, d_costs.data_ptr(), stream=_stream(),
                                      d_term_step=d_steps.data_ptr() if done else None, **plain_kw, **kw)
            got = d_costs.cpu().numpy()
            assert np.isnan(got[K:]).all(), "wrote past K"
            where = f"slots={slots} done={done} {label}"
            same(got[:K], want, where + " plain")
            if done:
                same(d_steps.cpu().numpy(), wsteps, where + " plain steps")
                assert (wsteps < H).any() and (wsteps == H).any(), where
            eng.set_cost_terms(ext)
            for ref_steps in (1, H):
                ref = np.broadcast_to(consts, (2, ref_steps, n_chan))      # every row of both environments equal
                gx, sx = run_kernel(eng, traj, acts if label == "explicit" else None, ref, None, 65, steps=done, **kw)
                same(gx, got[:K], f"{where} ref_steps={ref_steps} extended against plain")
                if done:
                    same(sx, wsteps, f"{where} ref_steps={ref_steps} extended steps")


# ------------------------------------------------------------------ 4. end to end, S = 11, A = 3
def tracking_cost(done=False):
    from bc_mpc_amd import cost_functions as cf
    return cf.TermCost([cf.quadratic(0, 4.0, target=cf.ref(0), on="next_state"),
                        cf.quadratic(5, 1.0, target=cf.ref(1), on="next_state"),
                        cf.threshold(1, ">=", cf.ref(2), 10.0), cf.progress(5, 0.008)]
                       + [cf.quadratic(j, 0.001, on="action") for j in range(A3)]
                       + [cf.rate(j, 0.05) for j in range(A3)],
                       done=[cf.done_when(0, "<", -0.4)] if done else (), done_cost=25.0 if done else 0.0)


@pytest.mark.parametrize("kernel", ["solo", "group4", "split2", "team"])
def test_engine_end_to_end(kernel):
    from bc_mpc_amd import _lib
    from oracle import mpc_oracle as orc
    torch, dev = _t()
    nt = net(S11, A3)
    K, H, seed, off = 37, 5, 0xC0FFEE, 2000
    T = tracking_cost()
    eng = _engine_or_skip(nt, kernel, K, H, terms=T)
    state = nt.states[0]
    rs = np.random.RandomState(5)
    ref_a, ref_b = rs.standard_normal((H, 3)) * 0.3, rs.standard_normal(3) * 0.3
    prev = rs.uniform(-1, 1, A3)
    acts = orc.device_rng_actions(seed, off, K, H, nt.low, nt.high)
    d_state, d_costs, d_traj = _dev(state), _empty(K), _empty(H + 1, K, S11)
    d_res = torch.zeros(ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    eng.set_cost_inputs(ref_a, prev)
    eng.rollout_async(d_state.data_ptr(), 0, None, seed, off, d_costs.data_ptr(), d_traj.data_ptr(), d_res.data_ptr(),
                      _stream())
    costs, traj = d_costs.cpu().numpy(), d_traj.cpu().numpy()
    eng.check_status()
    assert np.isfinite(traj).all()
    want_a, _ = definition(T, traj, acts, ref_a, prev)
    same(costs, want_a, f"{kernel} rollout_async")
    res = eng.get_action(state, None, seed=seed, cand_offset=off, return_costs=True)
    same(res.costs, want_a, f"{kernel} get_action")
    best = int(np.argmin(want_a))
    assert res.best_index == off + best and np.array_equal(res.first_action, acts[0, best])
    # only the reference changes between two calls: no set_cost_terms in between
    eng.set_cost_inputs(ref_b, None)
    res_b = eng.get_action(state, None, seed=seed, cand_offset=off, return_costs=True)
    want_b, _ = definition(T, traj, acts, ref_b, None)
    same(res_b.costs, want_b, f"{kernel} second reference")
    assert not np.array_equal(want_a, want_b)
    assert res_b.best_index == off + int(np.argmin(want_b))


# ------------------------------------------------------------------ 5. single planners
ELITE = np.dtype([("cost", "<f8"), ("index", "<i8")])


def one_iteration(eng, nt, T, state, mu, sd, seed, it, off, ref, prev):
    """Iteration `it` of a CEM / MPPI round for the K candidates at `off`, from the stream-ordered blocks: the
    sampled actions rolled out as an explicit array give the trajectory; its costs must be the definition's bit
    for bit, and cem_rollout_async (actions regenerated in the rollout and in the cost kernel) must give the same."""
    from oracle import mpc_oracle as orc
    K, H = eng.num_paths, eng.horizon
    acts = orc.cem_actions(seed, it, off, K, H, mu, sd, nt.low, nt.high)
    d_state, d_acts, d_costs, d_traj = _dev(state), _dev(acts), _empty(K), _empty(H + 1, K, nt.S)
    st = _stream()
    eng.rollout_async(d_state.data_ptr(), 0, d_acts.data_ptr(), seed, off, d_costs.data_ptr(), d_traj.data_ptr(),
                      None, st)
    costs = d_costs.cpu().numpy()
    same(costs, definition(T, d_traj.cpu().numpy(), acts, ref, prev)[0], f"it={it} off={off}: costs vs definition")
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


@pytest.mark.parametrize("kernel", ["group4", "split2"])
def test_single_planners_equal_the_chain_of_blocks(kernel):
    nt = net(S11, A3)
    K, H, seed, iters, E, alpha, lam = 37, 5, 0x5EED5, 2, 5, 0.1, 0.7
    T = tracking_cost(done=True)
    eng = nt.engine(kernel, K, H, terms=T)
    state = nt.states[2]
    rs = np.random.RandomState(100)
    mu0, sd0 = rs.uniform(-0.6, 0.6, (H, A3)), rs.uniform(0.1, 0.6, (H, A3))
    ref, prev = rs.standard_normal((H, 3)) * 0.3, rs.uniform(-1, 1, A3)
    eng.set_cost_inputs(ref, prev)
    _t()[0].cuda.synchronize()
    for planner in ("cem", "mppi"):
        mu, sd, all_costs, all_acts = mu0, sd0, [], []
        for it in range(iters):
            costs, acts, d_costs = one_iteration(eng, nt, T, state, mu, sd, seed, it, 0, ref, prev)
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


# ------------------------------------------------------------------ 6. the batched step
@pytest.mark.parametrize("kernel", ["group4", "split2"])
def test_batched_step_with_per_environment_inputs(kernel):
    nt = net(S11, A3)
    B, K, H, seed, off = 3, 50, 5, 4242, 700
    T = tracking_cost(done=True)
    big = nt.engine(kernel, B * K, H, terms=T)
    one = nt.engine(kernel, K, H, terms=T)
    rs = np.random.RandomState(9)
    ref = rs.standard_normal((B, H, 3)) * 0.3
    prev = rs.uniform(-1, 1, (B, A3))
    states = nt.states[:B]
    big.set_cost_inputs(ref, prev)
    got = big.get_actions(states, None, seed=seed, cand_offset=off, return_costs=True)
    for b in range(B):
        one.set_cost_inputs(ref[b], prev[b])
        want = one.get_action(states[b], None, seed=seed, cand_offset=off + b * K, return_costs=True)
        same(got.costs[b], want.costs, f"{kernel} env {b}")
        assert got.best_index[b] == want.best_index and got.best_cost[b] == want.best_cost
        assert np.array_equal(got.first_action[b], want.first_action)
    assert not np.array_equal(got.costs[0], got.costs[1])
    # a reference set for B environments does not serve a call over another number of them
    from bc_mpc_amd import _lib
    with pytest.raises(ValueError, match="environments"):
        big.get_action(states[0], None, seed=seed)
    with pytest.raises(ValueError, match="environments"):
        big.get_actions(nt.states[:2], None, seed=seed)


@pytest.mark.parametrize("planner", ["cem", "mppi"])
def test_batched_planners_with_per_environment_inputs(planner):
    nt = net(S11, A3)
    B, K, H, seed, off = 3, 50, 5, 99, 300
    T = tracking_cost()
    big = nt.engine("group4", B * K, H, terms=T)
    one = nt.engine("group4", K, H, terms=T)
    rs = np.random.RandomState(13)
    ref = rs.standard_normal((B, H, 3)) * 0.3
    prev = rs.uniform(-1, 1, (B, A3))
    mu, sd = rs.uniform(-0.3, 0.3, (B, H, A3)), rs.uniform(0.3, 0.8, (B, H, A3))
    states = nt.states[:B]
    big.set_cost_inputs(ref, prev)
    if planner == "cem":
        got, gmu, gsd = big.cem_get_actions(states, mu, sd, 2, 5, 0.1, seed, cand_offset=off, return_costs=True)
    else:
        got, gmu, _ = big.mppi_get_actions(states, mu, sd, 2, 0.7, seed, cand_offset=off, return_costs=True)
    # environment b alone: the same chain over one environment, candidates at off + b * K
    for b in range(B):
        one.set_cost_inputs(ref[b], prev[b])
        if planner == "cem":
            want, wmu, wsd = one.cem_get_actions(states[b:b + 1], mu[b:b + 1], sd[b:b + 1], 2, 5, 0.1, seed,
                                                 cand_offset=off + b * K, return_costs=True)
            same(gsd[b], wsd[0], f"cem env {b} sigma")
        else:
            want, wmu, _ = one.mppi_get_actions(states[b:b + 1], mu[b:b + 1], sd[b:b + 1], 2, 0.7, seed,
                                                cand_offset=off + b * K, return_costs=True)
        same(got.costs[:, b], want.costs[:, 0], f"{planner} env {b} costs")
        same(gmu[b], wmu[0], f"{planner} env {b} plan")
        assert got.best_cost[b] == want.best_cost[0]
        assert np.array_equal(got.first_action[b], want.first_action[0])


# ------------------------------------------------------------------ 7. controllers
class _Box:
    def __init__(self, n):
        self.low, self.high, self.shape = -np.ones(n, np.float32), np.ones(n, np.float32), (n,)


class _Env:
    action_space = _Box(A3)
    observation_space = _Box(S11)


def test_controllers_pass_the_inputs_on():
    """Every controller call with reference / previous_action is the engine call on the same seed after
    set_cost_inputs with the same arrays; rng="numpy" (the host draw uploaded) equals the definition's argmin."""
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller
    from bc_mpc_amd.cost_functions import TermCost
    nt = net(S11, A3)
    T = tracking_cost(done=True)
    K, H, B = 37, 5, 3
    states = nt.states[:B]
    rs = np.random.RandomState(17)
    ref1, refH, prev = rs.standard_normal(3) * 0.3, rs.standard_normal((H, 3)) * 0.3, rs.uniform(-1, 1, A3)
    refB, refBH, prevB = rs.standard_normal((B, 3)) * 0.3, rs.standard_normal((B, H, 3)) * 0.3, rs.uniform(-1, 1, (B, A3))
    seed_of = lambda s: int(np.random.RandomState(s).randint(0, 2**62, dtype=np.int64))   # noqa: E731
    one, many = nt.engine("auto", K, H, terms=T), nt.engine("auto", B * K, H, terms=T)
    mk = dict(horizon=H, cost_fn=TermCost(T.terms, T.done_conditions, T.done_cost), num_simulated_paths=K)
    assert mk["cost_fn"].key() == T.key()
    ctrl = MPCcontroller(_Env(), nt.dyn, rng="device", seed=5, **mk)
    ctrl.keep_costs = True
    for s, (r, p) in enumerate([(ref1, None), (refH, prev), (ref1, prev)]):
        ctrl._seed_rng = np.random.RandomState(5 + s)
        a = ctrl.get_action(states[0], reference=r, previous_action=p)
        one.set_cost_inputs(r, p)
        w = one.get_action(states[0], None, seed=seed_of(5 + s), return_costs=True)
        same(ctrl.last_costs, w.costs, f"MPC device {s}")
        assert np.array_equal(a, w.first_action) and ctrl.last_index == w.best_index
    ctrl._seed_rng = np.random.RandomState(9)
    a = ctrl.get_actions(states, reference=refBH, previous_action=prevB)
    many.set_cost_inputs(refBH, prevB)
    w = many.get_actions(states, None, seed=seed_of(9), return_costs=True)
    same(ctrl.last_costs, w.costs, "MPC get_actions")
    assert np.array_equal(a, w.first_action)
    a2 = ctrl.get_actions(states, reference=refB)           # [B, R], no previous action
    assert a2.shape == (B, A3)
    # rng="numpy": the host draw is uploaded; the costs are the definition's on the engine's own trajectory
    ctrl = MPCcontroller(_Env(), nt.dyn, **mk)
    ctrl.keep_costs = True
    np.random.seed(4242)
    a = ctrl.get_action(states[1], reference=refH, previous_action=prev)
    acts = np.random.RandomState(4242).uniform(_Env.action_space.low, _Env.action_space.high, [H, K, A3])
    one.set_cost_inputs(refH, prev)
    w = one.get_action(states[1], acts, return_costs=True)
    same(ctrl.last_costs, w.costs, "MPC numpy")
    assert np.array_equal(a, acts[0, int(np.argmin(w.costs))])
    # CEM and MPPI, single and batched
    cem = CEMcontroller(_Env(), nt.dyn, iterations=2, n_elite=5, seed=7, **mk)
    mu0, sd0 = cem.initial_distribution()
    a = cem.get_action(states[0], reference=refH, previous_action=prev)
    one.set_cost_inputs(refH, prev)
    r, mu, sd = one.cem_get_action(states[0], mu0, sd0, 2, 5, cem.alpha, seed_of(7))
    assert np.array_equal(a, r.first_action) and np.array_equal(cem.last_mu, mu)
    cem = CEMcontroller(_Env(), nt.dyn, iterations=2, n_elite=5, seed=8, **mk)
    mu0, sd0 = cem.batch_initial_distribution(B)
    a = cem.get_actions(states, reference=refBH, previous_action=prevB)
    many.set_cost_inputs(refBH, prevB)
    r, mu, sd = many.cem_get_actions(states, mu0, sd0, 2, 5, cem.alpha, seed_of(8))
    assert np.array_equal(a, r.first_action) and np.array_equal(cem.last_mu, mu)
    mp = MPPIcontroller(_Env(), nt.dyn, temperature=0.7, iterations=2, seed=10, **mk)
    mu0, sd0 = mp.batch_initial_distribution(B)
    a = mp.get_actions(states, reference=refB, previous_action=prevB)
    many.set_cost_inputs(refB[:, None, :], prevB)
    r, mu, _ = many.mppi_get_actions(states, mu0, sd0, 2, 0.7, seed_of(10))
    assert np.array_equal(a, mu[:, 0]) and np.array_equal(mp.last_mu, mu)


# ------------------------------------------------------------------ 7b. composition
def test_terminal_value_with_termination_composes():
    """A terminal value with termination, masked where the candidate died: the engine's costs are the definition's
    on its own trajectory and actions, plus weight * the engine's own values where the candidate lived."""
    from bc_mpc_amd import cost_functions as cf
    from bc_mpc_amd import value as _value
    from oracle import mpc_oracle as orc
    nt = net(S11, A3)
    K, H, seed = 64, 5, 123
    T0 = tracking_cost()
    eng = nt.engine("group4", K, H, terms=T0)
    rs = np.random.RandomState(23)
    ref, prev = rs.standard_normal((H, 3)) * 0.3, rs.uniform(-1, 1, A3)
    eng.set_cost_inputs(ref, prev)
    _t()[0].cuda.synchronize()
    acts = orc.device_rng_actions(seed, 0, K, H, nt.low, nt.high)
    d_state, d_costs, d_traj = _dev(nt.states[0]), _empty(K), _empty(H + 1, K, S11)
    # a done condition that half of the candidates meet (the trajectory does not depend on the cost)
    eng.rollout_async(d_state.data_ptr(), 0, None, seed, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, _stream())
    thr = float(np.median(d_traj.cpu().numpy()[1:, :, 0].max(axis=0)))
    T = cf.TermCost(T0.terms, done=[cf.done_when(0, ">", thr)], done_cost=25.0)
    eng.set_cost_terms(T)
    eng.set_cost_inputs(ref, prev)
    _t()[0].cuda.synchronize()
    spec = _value.ValueSpec([rs.standard_normal((S11, 16)).astype(np.float32) * 0.3,
                             rs.standard_normal((16, 1)).astype(np.float32) * 0.3],
                            [np.zeros(16, np.float32), np.zeros(1, np.float32)],
                            np.zeros(S11, np.float32), np.ones(S11, np.float32))
    try:
        eng.set_terminal_value(spec, weight=-0.5, version=1)
        eng.rollout_async(d_state.data_ptr(), 0, None, seed, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, _stream())
        costs, traj = d_costs.cpu().numpy(), d_traj.cpu().numpy()
        base, steps = definition(T, traj, acts, ref, prev)
        v = eng.last_terminal_values(np.arange(K))           # (the value kernel itself is not under test here)
        same(costs, _value.add_to_costs(base, v, -0.5, steps, H), "terminal value with termination")
        assert (steps < H).any() and (steps == H).any()
        same(costs[steps < H], base[steps < H], "a dead candidate keeps its cost")
        assert not np.array_equal(costs[steps == H], base[steps == H])
        same(eng.last_termination_steps(np.arange(K)), steps, "termination steps")
    finally:
        eng.set_terminal_value(None)


def test_correlated_noise_and_carried_elites_feed_the_rate_term():
    """noise_rho / keep_elites: the planners roll out a stored action array, and the rate term reads that array.
    Iteration 0 from the blocks (plan_sample_corr -> explicit rollout) is the definition bit for bit and is what
    the batched CEM call scores; the elites carried into iteration 1 are scored as they were."""
    nt = net(S11, A3)
    K, H, seed, E, rho = 64, 5, 777, 8, 0.6
    T = tracking_cost()
    eng = nt.engine("group4", K, H, terms=T)
    rs = np.random.RandomState(31)
    ref, prev = rs.standard_normal((H, 3)) * 0.3, rs.uniform(-1, 1, A3)
    mu0, sd0 = rs.uniform(-0.3, 0.3, (1, H, A3)), rs.uniform(0.3, 0.6, (1, H, A3))
    eng.set_cost_inputs(ref, prev)
    _t()[0].cuda.synchronize()
    state = nt.states[3]
    d_mu, d_sd, d_acts = _dev(mu0), _dev(sd0), _empty(H, K, A3)
    d_state, d_costs, d_traj = _dev(state), _empty(K), _empty(H + 1, K, S11)
    st = _stream()
    eng.plan_sample_corr_async(d_mu.data_ptr(), d_sd.data_ptr(), 1, K, seed, 0, 0, rho, d_acts.data_ptr(), stream=st)
    eng.rollout_async(d_state.data_ptr(), 0, d_acts.data_ptr(), seed, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, st)
    costs0, acts0 = d_costs.cpu().numpy(), d_acts.cpu().numpy()
    same(costs0, definition(T, d_traj.cpu().numpy(), acts0, ref, prev)[0], "stored array, iteration 0")
    res, mu, sd = eng.cem_get_actions(state[None], mu0, sd0, 2, E, 0.1, seed, return_costs=True, rho=rho,
                                      keep_elites=True)
    same(res.costs[0, 0], costs0, "cem_get_actions iteration 0")
    assert len(np.unique(costs0)) == K
    same(np.sort(res.costs[1, 0, :E]), np.sort(costs0)[:E], "carried elites keep their costs")
    # without the previous action the same array scores differently: the rate term's first step reads it
    eng.set_cost_inputs(ref, None)
    res2, _, _ = eng.cem_get_actions(state[None], mu0, sd0, 1, E, 0.1, seed, return_costs=True, rho=rho)
    same(res2.costs[0, 0], definition(T, d_traj.cpu().numpy(), acts0, ref, None)[0], "no previous action")
    assert not np.array_equal(res2.costs[0, 0], costs0)


def test_ensemble_members_get_the_same_list_and_inputs():
    """E = 2: each member's costs are its single engine's, single and batched (per-environment inputs), and the
    controllers over an EnsembleDynamicsModel pass the inputs on to every member."""
    from bc_mpc_amd import MPCcontroller
    from bc_mpc_amd.cost_functions import TermCost
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel, EnsembleEngine
    from oracle import mpc_oracle as orc
    nt = net(S11, A3)
    B, K, H, seed = 3, 37, 5, 321
    T = tracking_cost(done=True)
    rs = np.random.RandomState(29)
    ref, prev = rs.standard_normal((H, 3)) * 0.3, rs.uniform(-1, 1, A3)
    refB, prevB = rs.standard_normal((B, H, 3)) * 0.3, rs.uniform(-1, 1, (B, A3))
    ws = [nt.w, orc.synthetic_weights(S11, A3, 64, 2, "tanh", False, seed_base=2000)]
    specs = [MLPSpec(w.kernels, w.biases, w.activation) for w in ws]
    made = []

    def pair(k_total):
        ens = EnsembleEngine(2, S11, A3, 64, 2, "tanh", False, H, k_total, device=0, cost="terms")
        made.append(ens)
        one = RolloutEngine(S11, A3, 64, 2, "tanh", False, H, k_total, device=0, cost="terms",
                            kernel=ens.members[0].info()["kernel"])
        made.append(one)
        for e in (ens, one):
            e.set_cost_terms(T)
        for i, sp in enumerate(specs):
            ens.set_weights(i, sp, nt.norm, 1)
        return ens, one
    try:
        ens, one = pair(K)
        ens.set_cost_inputs(ref, prev)
        one.set_cost_inputs(ref, prev)
        got = ens.get_action(nt.states[0], None, seed=seed, return_costs=True, return_member_costs=True)
        for i, sp in enumerate(specs):
            one.set_weights(sp, nt.norm, 100 + i)
            same(got.member_costs[i], one.get_action(nt.states[0], None, seed=seed, return_costs=True).costs,
                 f"member {i}")
        assert not np.array_equal(got.member_costs[0], got.member_costs[1])
        # batched, per-environment inputs
        bens, bone = pair(B * K)
        bens.set_cost_inputs(refB, prevB)
        bone.set_cost_inputs(refB, prevB)
        states = nt.states[:B]
        gotb = bens.get_actions(states, None, seed=seed, return_costs=True, return_member_costs=True)
        for i, sp in enumerate(specs):
            bone.set_weights(sp, nt.norm, 100 + i)
            same(gotb.member_costs[i], bone.get_actions(states, None, seed=seed, return_costs=True).costs,
                 f"batched member {i}")
        # the controllers over an EnsembleDynamicsModel
        model = EnsembleDynamicsModel(_Env(), 2, 2, 64, "tanh", None, nt.norm, 32, 3, 1e-3, device=0)
        for e, w in enumerate(ws):
            model.load_weights(e, w.kernels, w.biases, w.ln_gamma, w.ln_beta)
        seed_of = lambda s: int(np.random.RandomState(s).randint(0, 2**62, dtype=np.int64))   # noqa: E731
        ctrl = MPCcontroller(_Env(), model, horizon=H, cost_fn=TermCost(T.terms, T.done_conditions, T.done_cost),
                             num_simulated_paths=K, rng="device", seed=5)
        ctrl.keep_costs = True
        a = ctrl.get_action(nt.states[0], reference=ref, previous_action=prev)
        w = ens.get_action(nt.states[0], None, seed=seed_of(5), return_costs=True)
        same(ctrl.last_costs, w.costs, "controller over an ensemble")
        assert np.array_equal(a, w.first_action)
        ctrl._seed_rng = np.random.RandomState(6)
        a = ctrl.get_actions(states, reference=refB, previous_action=prevB)
        w = bens.get_actions(states, None, seed=seed_of(6), return_costs=True)
        same(ctrl.last_costs, w.costs, "controller over an ensemble, batched")
        assert np.array_equal(a, w.first_action)
        with pytest.raises(ValueError, match="reference is for 2 environments, states for 3"):
            ctrl.get_actions(states, reference=refB[:2])
        made.extend(eng for _, eng in ctrl.__dict__.get("_ens_engines", {}).values())
    finally:
        for e in made:
            try:
                e.close()
            except Exception:
                pass


# ------------------------------------------------------------------ 8. refusals and states at the C boundary
def test_refusals_and_states():
    from bc_mpc_amd import _lib
    from bc_mpc_amd import cost_functions as cf
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    nt = net(S11, A3)
    H, K = 3, 16
    lib = _lib.load()
    eng = RolloutEngine(S11, A3, 64, 2, "tanh", False, H, K, device=0, cost="terms")
    try:
        eng.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, "tanh"), nt.norm, 1)

        def term(**kw):
            t = _lib.CostTermX(kind=3, source=0, index=0, cmp=0, weight=1.0, param=0.0, ref=-1)
            for k, v in kw.items():
                setattr(t, k, v)
            return t

        def set_x(terms, n_ref):
            arr = (_lib.CostTermX * max(1, len(terms)))(*terms)
            return lib.bcmpc_set_cost_terms_x(eng._h, arr, len(terms), n_ref)

        # argument errors leave no list behind
        bad = [([term(ref=0, kind=_lib.TERM_DIFF, param=0.01)], 1), ([term(ref=0, kind=_lib.TERM_LINEAR)], 1),
               ([term(ref=1)], 1), ([term(ref=-2)], 1), ([term(ref=0)], 17), ([term(ref=0)], -1),
               ([term(kind=_lib.TERM_RATE, source=0)], 0), ([term(kind=_lib.TERM_RATE, source=2, ref=0)], 1),
               ([term(kind=_lib.TERM_RATE, source=2, index=A3)], 0), ([term(kind=5)], 0)]
        for terms, n_ref in bad:
            assert set_x(terms, n_ref) == _lib.ERR_ARG, (terms[0].kind, terms[0].ref, n_ref)
        with pytest.raises(_lib.BcmpcError, match="bcmpc_set_cost_terms has not been called"):
            eng.get_action(nt.states[0])
        # RATE through the old setter is still refused
        old = _lib.CostTerm(kind=4, source=2, index=0, cmp=0, weight=1.0, param=0.0)
        assert lib.bcmpc_set_cost_terms(eng._h, ctypes.byref(old), 1) == _lib.ERR_ARG
        # (the slot budget: test_slot_budget_at_the_c_boundary, on a 20-dim engine)
        # a channelled list before the inputs: BCMPC_ERR_STATE with nothing launched
        T = cf.TermCost([cf.quadratic(0, 1.0, target=cf.ref(0)), cf.rate(1, 1.0)])
        eng.set_cost_terms(T)
        with pytest.raises(_lib.BcmpcError, match="bcmpc_set_cost_inputs has not been called") as ei:
            eng.get_action(nt.states[0])
        assert ei.value.code == _lib.ERR_STATE
        ref = np.zeros((1, H, 1))
        assert lib.bcmpc_set_cost_inputs(eng._h, None, 1, 1, None, 0) == _lib.ERR_ARG         # ref missing
        dp = ref.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert lib.bcmpc_set_cost_inputs(eng._h, dp, 1, 2, None, 0) == _lib.ERR_ARG           # ref_steps not in {1, H}
        assert lib.bcmpc_set_cost_inputs(eng._h, dp, 0, 1, None, 0) == _lib.ERR_ARG
        assert lib.bcmpc_set_cost_inputs(eng._h, dp, K + 1, 1, None, 0) == _lib.ERR_ARG
        with pytest.raises(_lib.BcmpcError):
            eng.get_action(nt.states[0])                                                        # still no inputs
        # ref_envs mismatch at call time
        eng.set_cost_inputs(np.zeros((2, H, 1)))
        with pytest.raises(ValueError, match="environments"):
            eng.get_action(nt.states[0])
        eng.get_actions(nt.states[:2])
        eng.set_cost_inputs(np.zeros(1))
        r1 = eng.get_action(nt.states[0], seed=3, return_costs=True)
        # budget overflow beside a held termination: 31 terms + 2 conditions
        conds = (_lib.CostTerm * 2)(*[_lib.CostTerm(kind=0, source=1, index=i, cmp=0, weight=0.0, param=5.0)
                                      for i in range(2)])
        assert lib.bcmpc_set_termination(eng._h, conds, 2, 1.0) == _lib.OK
        many = [term(ref=0)] + [term(kind=_lib.TERM_LINEAR, index=i % S11) for i in range(30)]
        assert set_x(many, 1) == _lib.ERR_ARG
        assert "done conditions" in lib.bcmpc_last_error().decode()
        assert lib.bcmpc_set_termination(eng._h, None, 0, 0.0) == _lib.OK
        # a plain list after an extended one: back to the plain instance, no inputs needed
        plain = cf.TermCost([cf.quadratic(0, 1.0), cf.linear(1, 0.5)])
        eng.set_cost_terms(plain)
        r2 = eng.get_action(nt.states[0], seed=3, return_costs=True)
        fresh = RolloutEngine(S11, A3, 64, 2, "tanh", False, H, K, device=0, cost="terms")
        try:
            fresh.set_weights(MLPSpec(nt.w.kernels, nt.w.biases, "tanh"), nt.norm, 1)
            fresh.set_cost_terms(plain)
            same(r2.costs, fresh.get_action(nt.states[0], seed=3, return_costs=True).costs, "plain after extended")
        finally:
            fresh.close()
        assert not np.array_equal(r1.costs, r2.costs)
        with pytest.raises(ValueError, match="reference channels or rate terms"):
            eng.set_cost_inputs(np.zeros(1))
    finally:
        eng.close()


def test_slot_budget_at_the_c_boundary():
    """16 quadratics, each on a state dim and a channel of its own, read 32 slots in 16 entries: they fit, and one
    more slot -- a RATE term's action, or a done condition's further dim -- does not."""
    from bc_mpc_amd import _lib
    from bc_mpc_amd import cost_functions as cf
    from bc_mpc_amd.engine import RolloutEngine
    eng = RolloutEngine(20, 6, 64, 2, "tanh", False, 7, 64, device=0, cost="terms")   # (raw lists: a private engine)
    lib = _lib.load()
    ts = [_lib.CostTermX(kind=3, source=0, index=i, cmp=0, weight=1.0, param=0.0, ref=i) for i in range(16)]
    rate = _lib.CostTermX(kind=_lib.TERM_RATE, source=2, index=0, cmp=0, weight=1.0, param=0.0, ref=-1)
    cond = _lib.CostTerm(kind=0, source=1, index=19, cmp=0, weight=0.0, param=5.0)
    held = _lib.CostTerm(kind=0, source=1, index=3, cmp=0, weight=0.0, param=5.0)
    assert lib.bcmpc_set_termination(eng._h, None, 0, 0.0) == _lib.OK
    assert lib.bcmpc_set_cost_terms_x(eng._h, (_lib.CostTermX * 17)(*ts, rate), 17, 16) == _lib.ERR_ARG
    assert "slots" in lib.bcmpc_last_error().decode()
    assert lib.bcmpc_set_cost_terms_x(eng._h, (_lib.CostTermX * 16)(*ts), 16, 16) == _lib.OK
    assert lib.bcmpc_set_termination(eng._h, ctypes.byref(held), 1, 1.0) == _lib.OK       # a dim already read
    assert lib.bcmpc_set_termination(eng._h, ctypes.byref(cond), 1, 1.0) == _lib.ERR_ARG  # the 33rd slot
    assert "slots" in lib.bcmpc_last_error().decode()
    assert lib.bcmpc_set_termination(eng._h, None, 0, 0.0) == _lib.OK
    eng.close()
    quads = [cf.quadratic(i, 1.0, target=cf.ref(i)) for i in range(16)]
    assert cf.TermCost(quads, done=[cf.done_when(3, ">", 5.0)]).n_slots == 32
    with pytest.raises(ValueError, match="slots"):
        cf.TermCost(quads + [cf.rate(0, 1.0)])
    with pytest.raises(ValueError, match="slots"):
        cf.TermCost(quads, done=[cf.done_when(19, ">", 5.0)])


# ------------------------------------------------------------------ 9. graph capture
def test_graph_replay_reads_the_new_inputs():
    torch, dev = _t()
    nt = net(S11, A3)
    K, H, seed = 64, 5, 31
    T = tracking_cost()
    eng = nt.engine("group4", K, H, terms=T)
    rs = np.random.RandomState(21)
    ref_a, ref_b = rs.standard_normal((H, 3)) * 0.3, rs.standard_normal((H, 3)) * 0.3
    prev_a, prev_b = rs.uniform(-1, 1, A3), rs.uniform(-1, 1, A3)
    state = nt.states[2]
    eng.set_cost_inputs(ref_a, prev_a)
    want_a = eng.get_action(state, None, seed=seed, return_costs=True).costs
    addr = eng.cost_input_buffers()
    assert addr[0] and addr[1]
    d_state, d_costs = _dev(state), _empty(K)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            eng.rollout_async(d_state.data_ptr(), 0, None, seed, 0, d_costs.data_ptr(), None, None,
                              torch.cuda.current_stream(dev).cuda_stream)
    g.replay()
    torch.cuda.synchronize(dev)
    same(d_costs.cpu().numpy(), want_a, "replay, first inputs")
    eng.set_cost_inputs(ref_b, prev_b)
    assert eng.cost_input_buffers() == addr                # the buffers' addresses are stable
    torch.cuda.synchronize(dev)                            # (the upload is ordered on the engine's stream)
    g.replay()
    torch.cuda.synchronize(dev)
    got_b = d_costs.cpu().numpy()
    want_b = eng.get_action(state, None, seed=seed, return_costs=True).costs
    same(got_b, want_b, "replay, new inputs")
    assert not np.array_equal(want_a, want_b)


# ------------------------------------------------------------------ 10. a team that gives up
def test_a_team_that_gives_up_reruns_with_the_same_list_and_inputs(monkeypatch):
    nt = net(S11, A3)
    K, H, seed = 37, 5, 77
    T = tracking_cost(done=True)
    team = _engine_or_skip(nt, "team", K, H, terms=T)
    ref_eng = nt.engine("split1", K, H, terms=T)
    rs = np.random.RandomState(2)
    for round_ in range(2):      # round 0: inputs set before the fallback exists; round 1: forwarded to it
        ref, prev = rs.standard_normal((H, 3)) * 0.3, rs.uniform(-1, 1, A3)
        team.set_cost_inputs(ref, prev)
        ref_eng.set_cost_inputs(ref, prev)
        want = ref_eng.get_action(nt.states[1], None, seed=seed, return_costs=True)
        before = team.team_reruns
        monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
        got = team.get_action(nt.states[1], None, seed=seed, return_costs=True)
        monkeypatch.delenv("BCMPC_TEAM_SPINS")
        assert team.team_reruns == before + 1
        same(got.costs, want.costs, f"fallback engine, round {round_}")
        assert got.best_index == want.best_index and np.array_equal(got.first_action, want.first_action)

"""Shared cases of test_gpu_state_action_sizes.py: the (state_dim, action_dim) sweep's shapes, nets, inputs and
oracle references, computed once per process and never modified.

Everything here is CPU work on oracle/mpc_oracle.py; nothing is taken from the engine.

Inputs.  Action bounds differ per dimension (low = linspace(-1, -0.5, A), high = linspace(0.75, 2, A)) and so does
the action normalisation (mean_action = linspace(-0.2, 0.3, A), std_action = linspace(0.4, 0.9, A), written over
entries 2 and 3 of synthetic_normalization's list), so that an action dimension read from the wrong slot cannot
cancel out.  Three action sources per case: an explicit array, the device Philox draw (SEED, cand_offset OFF)
and the CEM sample of iteration CEM_IT from a plan whose sigma reaches 2.0 (samples clip at both bounds).

The bar for states.  Base: |got - want| <= 1e-6 + 1e-6 |want| (test_gpu_parity.test_trajectory_states_match).
Per entry it is widened by COND_K (test_gpu_parity, 6.0) times that entry's rounding spread: the largest
deviation from ``want`` of the oracle's five other roundings of the same net (NumpyDynamicsF64 and
NumpyDynamicsChunked with 4, 4 reversed, 2 and 0 chunks, as oracle.conditioning does for costs).  The widened bar
must stay at or below 1e-5 + 1e-5 |want| on every entry -- a case whose inputs break that fails on its inputs
(state_bar asserts it), so the widening can never hide a kernel error.
"""
import functools

import numpy as np

SHAPES = [(1, 1), (5, 2), (11, 3), (15, 1), (15, 16), (16, 1), (16, 16), (17, 15), (20, 5), (21, 7), (26, 6), (29, 3),
          (31, 1)]
TINY_SHAPES = [(1, 1), (16, 16), (31, 1)]           # also run at K = 1, H = 1
BATCH_SHAPES = [(5, 2), (16, 16), (31, 1)]
K, H = 130, 6                                       # three 64- / 32-candidate groups, the last nearly empty; H wraps the 4-step ring
K_PP = 200                                          # the two-group layouts: a partly empty second group
SEED, OFF, CEM_IT = 0x51A7E5, 5, 2
SOURCES = ("explicit", "philox", "cem")

#        hidden L  act     ln
NETS = {
    "2x64tanh": (64, 2, "tanh", False),
    "2x128tanh": (128, 2, "tanh", False),
    "2x256reluLN": (256, 2, "relu", True),
    "2x500tanh": (500, 2, "tanh", False),
    "3x1000tanh": (1000, 3, "tanh", False),
    "2x512relu": (512, 2, "relu", False),
    "1x200tanhLN": (200, 1, "tanh", True),
}
KERNEL_NETS = {
    "solo": ["2x64tanh", "2x256reluLN"],
    "group4": ["2x64tanh", "2x256reluLN"],
    "group8": ["2x128tanh", "2x256reluLN"],
    "split1": ["2x500tanh", "2x256reluLN", "3x1000tanh"],
    "split2": ["2x500tanh", "2x256reluLN", "3x1000tanh"],
    "split4": ["2x500tanh", "2x512relu"],
    "team": ["2x500tanh", "2x256reluLN"],
    "pp3": ["2x500tanh"],                           # kernel="auto" under BCMPC_SPLIT_PP=1
    "auto": ["2x500tanh", "1x200tanhLN"],
}

BASE_A, BASE_R = 1e-6, 1e-6
CAP_A, CAP_R = 1e-5, 1e-5


def bounds(A):
    return np.linspace(-1.0, -0.5, A), np.linspace(0.75, 2.0, A)


def normalization(S, A, reward=False):
    from oracle import mpc_oracle as orc
    norm = orc.synthetic_normalization(S, A, reward=reward)
    norm[2] = np.linspace(-0.2, 0.3, A)
    norm[3] = np.linspace(0.4, 0.9, A)
    return norm


def net_spec(net):
    """(hidden, L, act, ln, seed_base) of a name of NETS, or of a (hidden, L, act, ln[, seed_base]) tuple given
    in its place (depth_cases.py's nets, which are not entries of NETS)."""
    t = NETS[net] if isinstance(net, str) else tuple(net)
    return t if len(t) == 5 else t + (1000,)          # (1000: synthetic_weights' own default)


def net_name(net):
    if isinstance(net, str):
        return net
    hidden, L, act, ln = net_spec(net)[:4]
    return f"{L}x{hidden}{act}{'LN' if ln else ''}"


def weights(S, A, net):
    from oracle import mpc_oracle as orc
    hidden, L, act, ln, seed_base = net_spec(net)
    return orc.synthetic_weights(S, A, hidden, L, act, ln, seed_base=seed_base)


def no_cost(state, action, next_state):
    return np.zeros(state.shape[0])


def other_roundings(w, norm):
    from oracle import mpc_oracle as orc
    return [orc.NumpyDynamicsF64(w, norm), orc.NumpyDynamicsChunked(w, norm, 4),
            orc.NumpyDynamicsChunked(w, norm, 4, reverse=True), orc.NumpyDynamicsChunked(w, norm, 2),
            orc.NumpyDynamicsChunked(w, norm, 0)]


def state_bar(w, norm, state, acts, want, label="", check=True):
    """The per-entry bar for the states ``want`` = rollout(NumpyDynamics(w, norm), state, acts) and the rounding
    spread in base bars (module docstring).  Fails when the widened bar would pass 1e-5 + 1e-5 |want| anywhere
    (``check=False``: returns it all the same, for measuring a net before it is taken)."""
    from oracle import mpc_oracle as orc
    from test_gpu_parity import COND_K
    spread = np.max([np.abs(orc.rollout(d, state, acts, no_cost)[1] - want) for d in other_roundings(w, norm)], axis=0)
    base = BASE_A + BASE_R * np.abs(want)
    bar = base + COND_K * spread
    assert not check or (bar <= CAP_A + CAP_R * np.abs(want)).all(), (
        f"{label}: the rounding spread of these inputs reaches {np.max(spread / base):.2f} base bars; the widened "
        f"bar would pass 1e-5 (1 + |want|)")
    return bar, spread / base


def action_sources(A, K, H, low=None, high=None, plan=None):
    """{source: [H, K, A] f64 actions}, the CEM plan (mu, sigma).  ``low``, ``high``: other bounds than bounds(A);
    ``plan``: a function (mu, sigma) -> (mu, sigma) applied to the plan drawn here (range_cases.py)."""
    from oracle import mpc_oracle as orc
    if low is None:
        low, high = bounds(A)
    rs = np.random.RandomState(1000 * K + 10 * H + A)
    mu, sd = rs.uniform(-0.4, 0.6, (H, A)), rs.uniform(0.1, 2.0, (H, A))
    sd[0, 0] = sd[-1, -1] = 2.0
    if plan is not None:
        mu, sd = plan(mu, sd)
    acts = {"explicit": rs.uniform(low, high, (H, K, A)),
            "philox": orc.device_rng_actions(SEED, OFF, K, H, low, high),
            "cem": orc.cem_actions(SEED, CEM_IT, OFF, K, H, mu, sd, low, high)}
    return acts, mu, sd


class Case:
    """One (S, A, net, K, H): inputs, the oracle's states and costs per action source, and the per-entry bar.
    ``net``: a name of NETS or a spec tuple (net_spec); ``self.net`` is its name either way.  ``check=False``
    builds the case even where its widened bar passes the cap (state_bar), for measuring a net before it is taken.
    ``given``: inputs that stand in for the ones built here (range_cases.py) -- a dict with any of ``w``, ``norm``,
    ``state``, ``low`` and ``high``, ``plan`` (action_sources) and ``explicit``, a function of the explicit action
    array that returns the one to use.  References, bar and cap are computed from whatever inputs result."""

    def __init__(self, S, A, net, K, H, check=True, given=None):
        from oracle import mpc_oracle as orc
        given = given or {}
        self.S, self.A, self.net, self.K, self.H = S, A, net_name(net), K, H
        self.hidden, self.L, self.act, self.ln = net_spec(net)[:4]
        self.w = given["w"] if "w" in given else weights(S, A, net)
        self.norm = given["norm"] if "norm" in given else normalization(S, A)
        self.state = np.array(given["state"], dtype=np.float64) if "state" in given else orc.synthetic_state(self.norm)
        self.low, self.high = (given["low"], given["high"]) if "low" in given else bounds(A)
        self.acts, self.mu, self.sd = action_sources(A, K, H, self.low, self.high, given.get("plan"))
        if "explicit" in given:
            self.acts["explicit"] = np.ascontiguousarray(given["explicit"](self.acts["explicit"]))
        if K >= 64:
            c = self.acts["cem"]
            assert (c == self.high).any() and (c == self.low).any(), "the CEM samples do not clip at both bounds"
        self.cheetah = S >= 18
        cost_fn = orc.cheetah_cost_fn if self.cheetah else no_cost
        self.costs, self.states = {}, {}
        dyn = orc.NumpyDynamics(self.w, self.norm)
        for src in SOURCES:
            self.costs[src], self.states[src] = orc.rollout(dyn, self.state, self.acts[src], cost_fn)
        # the five other roundings, all sources in one rollout each (candidates are independent rows)
        cat = np.ascontiguousarray(np.concatenate([self.acts[s] for s in SOURCES], axis=1))
        want = np.concatenate([self.states[s] for s in SOURCES], axis=1)
        bar, spread = state_bar(self.w, self.norm, self.state, cat, want, f"S={S} A={A} {self.net} K={K} H={H}",
                                check=check)
        self._bar = {s: bar[:, i * K:(i + 1) * K] for i, s in enumerate(SOURCES)}
        self._spread = {s: float(np.max(spread[:, i * K:(i + 1) * K])) for i, s in enumerate(SOURCES)}
        for d in (self.acts, self.costs, self.states, self._bar):
            for x in d.values():
                x.setflags(write=False)
        for x in (self.state, self.mu, self.sd, self.low, self.high):
            x.setflags(write=False)

    def bar(self, src):
        """The per-entry state bar of ``src`` ([H+1, K, S]) and the reference's own spread in base bars."""
        return self._bar[src], self._spread[src]


@functools.lru_cache(maxsize=None)
def case(S, A, net, K=K, H=H) -> Case:
    return Case(S, A, net, K, H)


# ------------------------------------------------------------------ the guard against a vacuous comparison
def mutation_ratios(S, A, net, K=K, H=3):
    """What a kernel that got one dimension wrong would show: the oracle mutated three ways (last action dim
    replaced by its neighbour, zero when A = 1; row S - 1 of layer 0's kernel zeroed; column S - 1 of the output
    kernel zeroed).  Per mutation: the median over candidates of the worst state error in units of
    1e-5 (1 + |want|)."""
    import copy
    from oracle import mpc_oracle as orc
    w, norm = weights(S, A, net), normalization(S, A)
    state = orc.synthetic_state(norm)
    low, high = bounds(A)
    acts = orc.device_rng_actions(SEED, OFF, K, H, low, high)
    _, want = orc.rollout(orc.NumpyDynamics(w, norm), state, acts, no_cost)
    unit = CAP_A * (1.0 + np.abs(want))

    def ratio(w2, acts2):
        _, got = orc.rollout(orc.NumpyDynamics(w2, norm), state, acts2, no_cost)
        return float(np.median(np.max(np.abs(got - want) / unit, axis=(0, 2))))

    a2 = acts.copy()
    a2[..., A - 1] = acts[..., A - 2] if A > 1 else 0.0
    w_in, w_out = copy.deepcopy(w), copy.deepcopy(w)
    w_in.kernels[0][S - 1, :] = 0.0
    w_out.kernels[-1][:, S - 1] = 0.0
    return {"last action dim": ratio(w, a2), "layer-0 row S-1": ratio(w_in, acts), "output column S-1": ratio(w_out, acts)}

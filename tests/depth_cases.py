"""Shared cases of test_gpu_depth_width.py and test_depth_cases.py: the network depth and width sweep's nets,
inputs, oracle references, bar and mutation guard, computed once per process and never modified.

Everything here is CPU work on oracle/mpc_oracle.py through size_cases.py's functions (bounds, normalisation, action
sources, the five other roundings, the per-entry state bar and its cap); nothing is taken from the engine.

Shape.  K = 70 (one full 64-candidate group and a partial 16-column; three 32-candidate groups), H = 3.  The depth
nets run at DEPTH_SHAPES -- (20, 6), where the fused cheetah cost is on, and (11, 3), cost "none" -- the width nets
at (20, 6).

Nets.  A net is (hidden, L, activation, LayerNorm, seed_base), named LxHIDDENact[LN] as size_cases.NETS names its own.
The depth nets reach L = 8 at every padded width (64 .. 1024) and with each activation; the width nets sit one past
a padding boundary of engine_plan.cpp's padded_hidden (65, 129, 257, 513, 769) or below one 16-row tile (1, 3, 15;
17 is 3x17reluLN).  Left out as degenerate: hidden 1 with relu or LayerNorm (a constant output, 1 distinct cost) and
2x2reluLN (71 distinct costs of 390).

Deep LayerNorm nets are ill-conditioned in the reference itself: the five other roundings of the oracle spread until
the widened bar would pass its cap 1e-5 (1 + |want|), which state_bar refuses.  The two relu + LayerNorm nets at hidden
256 and 500 therefore take the largest L <= 8 whose widened bar stays at or below RELU_LN_ROOM = 0.8 of the cap on both
DEPTH_SHAPES.  The ratio is that of the size_cases.Case the GPU tests compare against (bar_over_cap builds that very
case).  Measured at this sweep's K and H (bar / cap at (20, 6), at (11, 3)):
    hidden 256:  L = 3: 0.392 0.507  L = 4: 0.499 0.671  L = 5: 0.841 0.786  L = 6: 1.002 1.241  L = 7: 1.558 1.648
                 L = 8: 3.838 1.974
    hidden 500:  L = 3: 0.576 0.597  L = 4: 0.674 0.493  L = 5: 0.922 0.843  L = 6: 1.216 0.975  L = 7: 1.747 1.665
                 L = 8: 1.919 2.764
so the nets are 4x256reluLN (0.671) and 4x500reluLN (0.674); one layer more stands at 0.841 and 0.922, so neither choice
sits near the threshold.  The shorter horizon than the size sweep's (H = 3 against 6) is what leaves room for a
fourth layer.  test_depth_cases.py re-derives both choices.

Two nets take seed_base 1100 instead of synthetic_weights' 1000, the first of 1000, 1100, ... that passes:
 * 3x17reluLN: with 1000 its widened bar at (11, 3) is 1.36 of the cap (0.27 at (20, 6)); with 1100, 0.26 and 0.38.
 * 2x769relu: with 1000 hidden unit 768 is all but dead, mutation (d) moves the median candidate by 1.4 caps; with
   1100, by 167.

The guard against a vacuous comparison (mutation_ratios): the oracle mutated the way a kernel with a wrong layer slot
or a live pad lane would be wrong -- (a) per hidden layer l >= 1, biases[l] replaced by biases[l-1]; (b) per l >= 2,
kernels[l] replaced by kernels[l-1]; (c) LayerNorm nets, per l >= 1, gamma / beta of l replaced by those of l - 1;
(d) hidden unit hidden - 1 dropped in every layer (row hidden - 1 of kernels[1..L] zeroed).  Each must move the median
candidate's worst state by more than 10 times the cap.  A net that fails gets another seed_base, never a lower
threshold.
"""
import copy
import functools

import numpy as np

import size_cases as sc

K, H = 70, 3
DEPTH_SHAPES = [(20, 6), (11, 3)]
WIDTH_SHAPE = (20, 6)
RELU_LN_ROOM = 0.8
RELU_LN_DEPTH = {256: 4, 500: 4}                    # (module docstring; test_depth_cases.py re-derives it)

#         hidden  L  act     ln     seed_base
DEPTH_NETS = [
    (64, 4, "tanh", False, 1000),
    (64, 8, "tanh", False, 1000),
    (128, 8, "relu", False, 1000),
    (500, 4, "tanh", False, 1000),
    (512, 8, "tanh", False, 1000),
    (512, 5, "relu", False, 1000),
    (768, 4, "tanh", False, 1000),
    (1024, 8, "tanh", False, 1000),
    (64, 8, "tanh", True, 1000),
    (200, 5, "tanh", True, 1000),
    (17, 3, "relu", True, 1100),
    (256, RELU_LN_DEPTH[256], "relu", True, 1000),
    (500, RELU_LN_DEPTH[500], "relu", True, 1000),
]
WIDTH_NETS = [
    (1, 1, "tanh", False, 1000),
    (3, 2, "tanh", True, 1000),
    (15, 2, "tanh", False, 1000),
    (65, 2, "tanh", False, 1000),
    (129, 2, "relu", True, 1000),
    (257, 2, "tanh", False, 1000),
    (513, 2, "tanh", False, 1000),
    (769, 2, "relu", False, 1100),
]
NETS = {sc.net_name(n): n for n in DEPTH_NETS + WIDTH_NETS}
NET_SHAPES = ([(sc.net_name(n), s) for n in DEPTH_NETS for s in DEPTH_SHAPES] +
              [(sc.net_name(n), WIDTH_SHAPE) for n in WIDTH_NETS])


def padded(hidden):
    """engine_plan.cpp's padded_hidden."""
    return next(hp for hp in (64, 128, 256, 512, 768, 1024) if hidden <= hp)


def case(net, S, A) -> sc.Case:
    """The size_cases.Case of a net of NETS (or a spec tuple) at K, H: cached there, read-only."""
    return sc.case(S, A, NETS[net] if isinstance(net, str) else tuple(net), K, H)


def cap(want):
    return sc.CAP_A + sc.CAP_R * np.abs(want)


@functools.lru_cache(maxsize=None)
def bar_over_cap(net, S, A) -> float:
    """The largest widened bar over its cap of the very size_cases.Case the GPU tests compare against (per-source
    references, the spread of the five other roundings), built without state_bar's assertion: a net's own
    conditioning, measured before the net is taken."""
    c = sc.Case(S, A, NETS[net] if isinstance(net, str) else tuple(net), K, H, check=False)
    return max(float(np.max(c.bar(src)[0] / cap(c.states[src]))) for src in sc.SOURCES)


def distinct(c) -> dict:
    """Per action source, the number of distinct oracle costs (cheetah shapes) or distinct final states."""
    out = {}
    for src in sc.SOURCES:
        out[src] = len(np.unique(c.costs[src])) if c.cheetah else len(np.unique(c.states[src][-1], axis=0))
    return out


@functools.lru_cache(maxsize=None)
def cost_conditioning(net, S, A):
    """Cheetah shapes: per source, (the largest |cost - oracle cost| over the reference's five other roundings
    among candidates away from a penalty threshold, test_gpu_parity.assert_costs_close's tolerance there)."""
    from conftest import envelope
    from oracle import mpc_oracle as orc
    from test_gpu_parity import ATOL, RTOL
    c = case(net, S, A)
    assert c.cheetah
    out = {}
    for src in sc.SOURCES:
        spread = orc.conditioning(c.w, c.norm, c.state, c.acts[src], c.costs[src])
        keep = ~orc.near_threshold_mask(c.states[src])
        tol = np.minimum(ATOL + RTOL * np.abs(c.costs[src]), envelope(c.ln, c.L, c.hidden, H))
        i = int(np.argmax(np.where(keep, spread / tol, 0.0)))
        out[src] = (float(spread[i]), float(tol[i]))
    return out


# ------------------------------------------------------------------ the guard against a vacuous comparison
@functools.lru_cache(maxsize=None)
def mutation_ratios(net, S, A) -> dict:
    """{mutation: the median over candidates of the worst state error in units of 1e-5 (1 + |want|)} for every
    mutation (a) - (d) of the module docstring, on the device Philox actions."""
    from oracle import mpc_oracle as orc
    spec = NETS[net] if isinstance(net, str) else tuple(net)
    hidden, L, _, ln = spec[:4]
    w, norm = sc.weights(S, A, spec), sc.normalization(S, A)
    state = orc.synthetic_state(norm)
    low, high = sc.bounds(A)
    acts = orc.device_rng_actions(sc.SEED, sc.OFF, K, H, low, high)
    _, want = orc.rollout(orc.NumpyDynamics(w, norm), state, acts, sc.no_cost)
    unit = sc.CAP_A * (1.0 + np.abs(want))

    def ratio(w2):
        _, got = orc.rollout(orc.NumpyDynamics(w2, norm), state, acts, sc.no_cost)
        return float(np.median(np.max(np.abs(got - want) / unit, axis=(0, 2))))

    out = {}
    for l in range(1, L):
        m = copy.deepcopy(w)
        m.biases[l] = w.biases[l - 1]
        out[f"(a) bias {l} <- {l - 1}"] = ratio(m)
    for l in range(2, L):
        m = copy.deepcopy(w)
        m.kernels[l] = w.kernels[l - 1]
        out[f"(b) kernel {l} <- {l - 1}"] = ratio(m)
    if ln:
        for l in range(1, L):
            m = copy.deepcopy(w)
            m.ln_gamma[l], m.ln_beta[l] = w.ln_gamma[l - 1], w.ln_beta[l - 1]
            out[f"(c) LayerNorm {l} <- {l - 1}"] = ratio(m)
    m = copy.deepcopy(w)
    for l in range(1, L + 1):
        m.kernels[l][hidden - 1, :] = 0.0
    out[f"(d) unit {hidden - 1} dropped"] = ratio(m)
    return out


# ------------------------------------------------------------------ fused policy
#            layers hidden
POLICIES = [(1, 1), (1, 17), (3, 128), (8, 16), (8, 128), (2, 65)]
POLICY_SHAPE = (20, 6)
POLICY_ATOL, POLICY_RTOL = 1e-5, 1e-5               # test_policy_stochastic_mode_every_step's action bar


def policy_mean_f64(p, ob):
    """NumpyPolicy.mean restated in f64 from the same f32 observation filter input."""
    x = np.asarray(ob).astype(np.float32)
    last = np.clip((x - p.ob_mean) / p.ob_std, np.float32(-5.0), np.float32(5.0)).astype(np.float64)
    for k, b in zip(p.kernels[:-1], p.biases[:-1]):
        last = np.tanh(last @ k.astype(np.float64) + b.astype(np.float64))
    return last @ p.kernels[-1].astype(np.float64) + p.biases[-1].astype(np.float64)


@functools.lru_cache(maxsize=None)
def policy_gap(layers, hidden) -> float:
    """The largest |NumpyPolicy.mean - its f64 restatement| over the action bar, along the oracle's own stochastic
    policy rollout of the 2x500 tanh net at POLICY_SHAPE, K, H."""
    from oracle import mpc_oracle as orc
    S, A = POLICY_SHAPE
    p = orc.synthetic_policy(S, A, hidden, layers)
    norm = sc.normalization(S, A)
    dyn = orc.NumpyDynamics(orc.synthetic_weights(S, A, 500, 2, "tanh", False), norm)
    pol = orc.NumpyPolicy(p)
    s = np.tile(orc.synthetic_state(norm), (K, 1))
    sd = np.exp(p.logstd.astype(np.float64))
    worst = 0.0
    for h in range(H):
        m32, m64 = pol.mean(s).astype(np.float64), policy_mean_f64(p, s)
        worst = max(worst, float(np.max(np.abs(m32 - m64) / (POLICY_ATOL + POLICY_RTOL * np.abs(m32)))))
        s = dyn.predict(s, m32 + sd * orc.device_rng_normals(sc.SEED, sc.OFF, K, h, A))
    return worst


# ------------------------------------------------------------------ reward net widths
REWARD_WIDTHS = [65, 129, 257]
REWARD_SHAPE = (20, 6)


@functools.lru_cache(maxsize=None)
def reward_distinct(hidden) -> int:
    """Distinct oracle rewards of the reward net of width ``hidden`` at REWARD_SHAPE, K, H, on the Philox actions."""
    from oracle import mpc_oracle as orc
    S, A = REWARD_SHAPE
    norm = sc.normalization(S, A, reward=True)
    w = orc.synthetic_reward_weights(S, A, hidden, False)
    low, high = sc.bounds(A)
    ap = orc.device_rng_actions(sc.SEED, sc.OFF, K, H, low, high)
    want, _ = orc.reward_rollout(orc.NumpyRewardDynamics(w, norm), orc.synthetic_state(norm), ap, 0.95)
    return len(np.unique(want))

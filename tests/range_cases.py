"""Shared cases of test_gpu_input_range.py and test_range_cases.py: the input-magnitude sweep's regimes, their inputs,
oracle references and CPU guards, computed once per process and never modified.

Everything here is CPU work on oracle/mpc_oracle.py through size_cases.py (size_cases.Case takes the regime's inputs as
``given``; references, the per-entry bar and its cap are size_cases' own, unchanged); nothing is taken from the engine.

Why.  The size and the depth sweep share one input regime: the state within 0.5 sigma of mean_obs, std_obs in
[0.2, ~2], actions normalising to at most sqrt(3), Glorot weights.  The largest normalised layer-0 input of a candidate
is then between 1 and 3, and the split kernels (rollout_x3.h, rollout_pp.h, rollout_team.hip) branch on exactly that
number: per 16-candidate column they take max |x|, the power of two sh = 12 - e that moves it into [2^11, 2^12), clamp
sh to +-100, special-case max == 0, split into hi / lo f16 and undo the scale in the epilogue.  Across both sweeps sh
takes two values.  A regime here replaces the oracle's inputs only; shape (20, 6) and (11, 3), K = 70, H = 3 as the
depth sweep.

Regimes (FINITE; the ``far`` dimension d is 17 at S = 20 -- the one the cheetah cost differences -- and S - 1 at S = 11):
 far1        state[d] = mean_obs[d] + FAR1_SIGMA sigma.  300 sigma; 2x512relu 100 (at 300 its widened bar is 1.01 of
             the cap; at 100, 0.58).
 farall      every dimension displaced, by up to 40 sigma: state = mean_obs +- m_d sigma_d with the signs of the
             synthetic state and m_d = geomspace(0.05, 40, S) in a fixed shuffled order.  (With m_d = 40 throughout,
             layer 0 of the tanh nets saturates so far that the guards below do not hold: the last action dimension
             replaced by its neighbour moves 2x64tanh by 0.8 caps, a lost lo half moves the nets by 0.03 .. 2.2.)
 zero        state = mean_obs exactly, and the explicit array's step-0 rows of candidates 0..19 = mean_action: their
             normalised layer-0 input is exactly 0 (max == 0).  Candidates 16..19 share a 16-column with ordinary ones.
 const6-row  std_obs[3] = 1e-6 and the state of the unchanged normalisation: |x_3| ~ 1e5 .. 1e6.
 const0-row  std_obs[3] = 0, the 1e-10 floor: |x_3| ~ 1e9 .. 1e10.
             Row 3 of kernels[0] is multiplied by the exact power of two 2^-p that brings |x_3| 2^-p into [1, 2) at
             the initial state, so that the product stays O(1) and the other dimensions still matter.  Unscaled, x_3
             saturates every unit of a tanh net's layer 0 (1 distinct final state of 70); on 2x256reluLN LayerNorm
             divides everything else away (std_obs[3] = 0: 1 distinct final state; 1e-6: 70, but the last action
             dimension replaced by its neighbour moves the states by 0.02 caps); 2x512relu stands at 13.1 caps.  None
             of the unscaled cases can meet the guards below, so none is taken.
 tiny        the state within 1e-6 sigma of mean_obs, action bounds mean_action +- 1e-6 std_action, the CEM plan
             scaled into them: the step-0 column max is ~1e-6, sh ~ +32.
 dead        relu nets without LayerNorm: biases[0] shifted down by one constant so that the oracle's first hidden
             layer is all-zero at step 0 for between 8 and K - 8 candidates of the explicit and the Philox source (and
             some of the CEM sample, whose clipped actions fall there less often), a dead and a live candidate sharing
             a 16-column.  The shift is the middle of gap DEAD_GAP between neighbouring values of the candidates'
             largest layer-0 pre-activation, sorted over all three sources (dead_shift): a gap chosen on the CPU,
             among the widest of the lower half, for which all K final states stay distinct (a candidate dead at every
             step ends where every other such candidate ends).
             relu + LayerNorm is left out: next to every dead candidate sits one whose live units are ~1e-3, LayerNorm
             divides by their spread, and the widened bar passes the cap (2x256reluLN: 0.86 .. 4.3 caps, 3x17reluLN
             0.8 .. 1.3, over forty gaps no one within ROOM with the dead counts above).  A zero-variance LayerNorm
             column therefore stays unpinned.
 hot         relu nets: kernels[1] and biases[1] times 2^10, without LayerNorm 2^12 (at 2^10 2x512relu reaches 779); the
             second hidden layer's activations reach the thousands.  Without LayerNorm the output kernel is multiplied
             by the inverse power, which keeps the states those of the unscaled net (relu is homogeneous; without it
             the states grow by that power a step: 2050 caps at 2^10).
 NaN         (nan_case; its own GPU test) "action": NaN in the explicit actions at step 1 of candidates 37, 69 and 5
             (NAN_AT) -- 69 sits in the partly filled last 16-column; "state": NaN in one dimension of the initial state.

Infinite inputs are left out: the reference maps +-inf through tanh to +-1, the kernels' padded zero weights make
inf * 0, and no real state reaches f32's range.

The bar is size_cases.state_bar unchanged.  A regime x net whose widened bar exceeds ROOM = 0.8 of the cap
(depth_cases.RELU_LN_ROOM's convention) is not taken.

Guards (test_range_cases.py): K distinct final states per source; size_cases.mutation_ratios' three mutations on the
regime's inputs; and mutations of the oracle that model what a kernel would get wrong in that regime (MUTATIONS):
 clamp32     the layer-0 input clamped to +-32 (f16's range at the synthetic scale): far1, farall, const*-row.
 lostlo      the layer-0 input rounded to 11 bits below the candidate's own max |x| (a lost lo half): far1, farall.
 stale       the all-zero layer-0 inputs replaced by those of the candidate 20 places on: zero.
 revive      all-zero first-layer activations replaced by a live candidate's: dead.
Each must move the median affected candidate's worst state by more than 10 caps.
"""
import copy
import functools

import numpy as np

import depth_cases as dc
import size_cases as sc

K, H = dc.K, dc.H
SHAPES = [(20, 6), (11, 3)]
ROOM = dc.RELU_LN_ROOM
FAR1_SIGMA = {"2x512relu": 100.0}                   # every other net: 300
FAR1_DEFAULT, FARALL_SIGMA, FARALL_LOW = 300.0, 40.0, 0.05
#           (net, S): the gap of dead_shift
DEAD_GAP = {("2x512relu", 20): 50, ("2x512relu", 11): 50, ("2x64relu", 20): 42, ("2x64relu", 11): 49,
            ("2x128relu", 20): 33, ("2x128relu", 11): 32}
ZERO_CANDS = 20
HOT_EXP = {True: 10, False: 12}                     # by LayerNorm
NAN_AT = [(1, 37, 0), (1, 69, 2), (1, 5, 1)]        # (step, candidate, action dim); 69: the partly filled 16-column
NAN_STATE_DIM = 2
TINY = 1e-6

FINITE = ["far1", "farall", "zero", "const6-row", "const0-row", "tiny", "dead", "hot"]
RELU_NETS = {"2x256reluLN": (256, 2, "relu", True), "2x512relu": (512, 2, "relu", False),
             "2x64relu": (64, 2, "relu", False), "2x128relu": (128, 2, "relu", False)}

# relu nets without LayerNorm for the kernels whose size_cases.KERNEL_NETS entry has none (dead, hot, NaN)
RELU_ON = {"solo": "2x64relu", "group4": "2x64relu", "group8": "2x128relu", "split1": "2x512relu", "split2": "2x512relu",
           "split4": "2x512relu", "team": "2x512relu", "auto": "2x512relu"}


def kernel_nets(kernel, regime=None):
    """The nets ``kernel`` runs: size_cases.KERNEL_NETS' and RELU_ON's (pp3 takes the tanh net only), those of them
    that ``regime`` is taken on when one is given."""
    nets = list(sc.KERNEL_NETS[kernel])
    if kernel in RELU_ON and RELU_ON[kernel] not in nets:
        nets.append(RELU_ON[kernel])
    return [n for n in nets if regime is None or applies(regime, n)]


def spec(net):
    return RELU_NETS.get(net, net) if isinstance(net, str) else tuple(net)


def is_relu(net):
    return sc.net_spec(spec(net))[2] == "relu"


def is_ln(net):
    return sc.net_spec(spec(net))[3]


def applies(regime, net):
    """Whether ``regime`` is taken on ``net`` (module docstring)."""
    if regime == "dead":
        return is_relu(net) and not is_ln(net)
    if regime == "hot":
        return is_relu(net)
    if regime in ("const6-row", "const0-row"):
        return sc.net_name(spec(net)) != "2x512relu"
    return True


NETS = sorted({n for k in sc.KERNEL_NETS for n in kernel_nets(k)})
NET_CASES = [(r, n, s) for n in NETS for s in SHAPES for r in FINITE
             if applies(r, n) and (n in sc.NETS or r in ("dead", "hot"))]
# (kernel, net, regime, shape): the extra relu nets run the regimes that are about relu only
KERNEL_CASES = [(k, n, r, s) for k in sc.KERNEL_NETS for r in FINITE for n in kernel_nets(k, r) for s in SHAPES
                if n in sc.KERNEL_NETS[k] or r in ("dead", "hot")]
F16_REGIMES = ["far1", "farall", "zero", "const6-row", "const0-row", "tiny"]


def farall_sigmas(S):
    """Per dimension, the multiple of sigma: FARALL_LOW .. FARALL_SIGMA in geometric steps, in a fixed shuffled order."""
    return np.geomspace(FARALL_LOW, FARALL_SIGMA, S)[np.random.RandomState(240 + S).permutation(S)]


def far_dim(S):
    return 17 if S > 17 else S - 1


def _x0(w, norm, state, acts0):
    """The f32 layer-0 input of step 0 as NumpyDynamics.predict forms it."""
    from oracle import mpc_oracle as orc
    ns = (np.tile(state, (acts0.shape[0], 1)) - norm[0]) / (norm[1] + orc.NORM_EPS)
    na = (acts0 - norm[2]) / (norm[3] + orc.NORM_EPS)
    return np.concatenate([ns.astype(np.float32), na.astype(np.float32)], axis=1)


def dead_preacts(w, norm, state, acts):
    """The candidates' largest layer-0 pre-activation at step 0, sorted over all sources together."""
    return np.sort(np.concatenate([np.max(_x0(w, norm, state, a[0]) @ w.kernels[0] + w.biases[0], axis=1)
                                   for a in acts.values()]).astype(np.float64))


def dead_shift(w, norm, state, acts, gap):
    """The constant to take off biases[0]: the middle of gap ``gap`` of dead_preacts."""
    m = dead_preacts(w, norm, state, acts)
    return 0.5 * (m[gap] + m[gap + 1])


def given(name, net, S, A):
    """size_cases.Case's ``given`` of the case ``name`` (a regime, or const6-row / const0-row)."""
    from oracle import mpc_oracle as orc
    regime, _, row = name.partition("-")
    norm = sc.normalization(S, A)
    base = orc.synthetic_state(norm)
    mean, std = norm[0], norm[1]
    g = {}
    if regime == "far1":
        d = far_dim(S)
        g["state"] = base.copy()
        g["state"][d] = mean[d] + FAR1_SIGMA.get(sc.net_name(spec(net)), FAR1_DEFAULT) * std[d]
    elif regime == "farall":
        g["state"] = mean + farall_sigmas(S) * std * np.where(base >= mean, 1.0, -1.0)
    elif regime == "zero":
        g["state"] = mean.copy()

        def explicit(a):
            a = a.copy()
            a[0, :ZERO_CANDS, :] = norm[2]
            return a
        g["explicit"] = explicit
    elif regime in ("const6", "const0"):
        norm = [np.array(x, copy=True) for x in norm]
        norm[1][3] = norm[7][3] = 1e-6 if regime == "const6" else 0.0
        g["norm"], g["state"] = norm, base
        if row:                                         # (without: the unscaled row, for measuring only)
            x3 = abs((base[3] - norm[0][3]) / (norm[1][3] + orc.NORM_EPS))
            p = int(np.floor(np.log2(x3)))
            w = copy.deepcopy(sc.weights(S, A, spec(net)))
            w.kernels[0][3, :] = np.ldexp(w.kernels[0][3, :], -p)
            g["w"] = w
    elif regime == "tiny":
        z = (base - mean) / std
        g["state"] = mean + TINY * std * z / np.max(np.abs(z))
        g["low"], g["high"] = norm[2] - TINY * norm[3], norm[2] + TINY * norm[3]
        g["plan"] = lambda mu, sd: (norm[2] + TINY * norm[3] * mu, 0.5 * TINY * norm[3] * sd)
    elif regime == "dead":
        w = copy.deepcopy(sc.weights(S, A, spec(net)))
        acts, _, _ = sc.action_sources(A, K, H)
        shift = dead_shift(w, norm, base, acts, DEAD_GAP[(sc.net_name(spec(net)), S)])
        w.biases[0] = (w.biases[0] - np.float32(shift)).astype(np.float32)
        g["w"] = w
    elif regime == "hot":
        w = copy.deepcopy(sc.weights(S, A, spec(net)))
        e = HOT_EXP[bool(w.layer_norm)]
        w.kernels[1] = np.ldexp(w.kernels[1], e)
        w.biases[1] = np.ldexp(w.biases[1], e)
        if not w.layer_norm:
            w.kernels[2] = np.ldexp(w.kernels[2], -e)
        g["w"] = w
    else:
        raise ValueError(name)
    return g


@functools.lru_cache(maxsize=None)
def case(name, net, S, A, check=True, k=K) -> sc.Case:
    """The size_cases.Case of the case ``name`` on ``net`` (a name of size_cases.NETS or RELU_NETS) at K (``k``: the
    two-group layouts' K), H: read-only.  ``c.regime`` is ``name``."""
    c = sc.Case(S, A, spec(net), k, H, check=check, given=given(name, net, S, A))
    c.regime = name
    return c


def bar_over_cap(c) -> float:
    return max(float(np.max(c.bar(src)[0] / dc.cap(c.states[src]))) for src in sc.SOURCES)


def distinct(c) -> dict:
    return {src: len(np.unique(c.states[src][-1], axis=0)) for src in sc.SOURCES}


# ------------------------------------------------------------------ mutated oracles
class Mutated:
    """NumpyDynamics with a hook on the f32 layer-0 input (``x_hook``), one on the first hidden layer's activations
    before LayerNorm (``h_hook``), and ``relu``: the maximum that forms relu (np.maximum: the reference's)."""

    def __new__(cls, w, norm, x_hook=None, h_hook=None, relu=np.maximum):
        from oracle import mpc_oracle as orc

        class Dyn(orc.NumpyDynamics):
            def mlp(self, x32):
                ww = self.weights
                out = x32 if x_hook is None else x_hook(x32).astype(np.float32)
                for li in range(ww.n_layers):
                    out = out @ ww.kernels[li] + ww.biases[li]
                    out = np.tanh(out) if ww.activation == "tanh" else relu(out, np.float32(0))
                    if li == 0 and h_hook is not None:
                        out = h_hook(out)
                    if ww.layer_norm:
                        out = orc.layer_norm_tf1(out, ww.ln_gamma[li], ww.ln_beta[li])
                return (out @ ww.kernels[-1] + ww.biases[-1]).astype(np.float32, copy=False)
        return Dyn(w, norm)


def clamp32(x):
    return np.clip(x, np.float32(-32.0), np.float32(32.0))


def lostlo(x):
    mx = np.max(np.abs(x), axis=1, keepdims=True)
    q = np.exp2(np.floor(np.log2(np.where(mx > 0, mx, 1.0))) - 10.0)
    return np.round(x / q) * q


def stale(x):
    x = x.copy()
    z = np.flatnonzero(~x.any(axis=1))
    x[z] = x[(z + ZERO_CANDS) % x.shape[0]]
    return x


def revive(h):
    h = h.copy()
    z = ~h.any(axis=1)
    if z.any() and (~z).any():
        h[z] = h[np.flatnonzero(~z)[0]]
    return h


MUTATIONS = {"clamp32": (dict(x_hook=clamp32), ("far1", "farall", "const6-row", "const0-row")),
             "lostlo": (dict(x_hook=lostlo), ("far1", "farall")),
             "stale": (dict(x_hook=stale), ("zero",)),
             "revive": (dict(h_hook=revive), ("dead",))}


def _ratio(c, dyn, src, acts=None, only=None):
    """The median over candidates (``only``: a mask of those the mutation touches) of the worst state error of
    ``dyn`` in units of the cap."""
    from oracle import mpc_oracle as orc
    _, got = orc.rollout(dyn, c.state, c.acts[src] if acts is None else acts, sc.no_cost)
    per = np.max(np.abs(got - c.states[src]) / dc.cap(c.states[src]), axis=(0, 2))
    return float(np.median(per[only] if only is not None else per))


def affected(c, src):
    """The candidates a regime's own mutation touches: the zero candidates, the dead ones, else all."""
    if c.regime == "zero":
        return ~_x0(c.w, c.norm, c.state, c.acts[src][0]).any(axis=1)
    if c.regime == "dead":
        return dead_mask(c, src)
    return None


def dead_mask(c, src):
    """[K] bool: the oracle's first hidden layer is all-zero at step 0."""
    z = _x0(c.w, c.norm, c.state, c.acts[src][0]) @ c.w.kernels[0] + c.w.biases[0]
    return ~(np.maximum(z, np.float32(0)) > 0).any(axis=1)


def size_mutation_ratios(c) -> dict:
    """size_cases.mutation_ratios' three mutations on the case's own inputs (Philox actions)."""
    from oracle import mpc_oracle as orc
    S, A = c.S, c.A
    acts = c.acts["philox"]
    a2 = acts.copy()
    a2[..., A - 1] = acts[..., A - 2]
    w_in, w_out = copy.deepcopy(c.w), copy.deepcopy(c.w)
    w_in.kernels[0][S - 1, :] = 0.0
    w_out.kernels[-1][:, S - 1] = 0.0
    return {"last action dim": _ratio(c, orc.NumpyDynamics(c.w, c.norm), "philox", acts=a2),
            "layer-0 row S-1": _ratio(c, orc.NumpyDynamics(w_in, c.norm), "philox"),
            "output column S-1": _ratio(c, orc.NumpyDynamics(w_out, c.norm), "philox")}


def regime_mutation_ratios(c) -> dict:
    """The mutations of MUTATIONS that list the case's regime, on the source they bite on (zero: the explicit array)."""
    src = "explicit" if c.regime == "zero" else "philox"
    return {name: _ratio(c, Mutated(c.w, c.norm, **kw), src, only=affected(c, src))
            for name, (kw, regimes) in MUTATIONS.items() if c.regime in regimes}


# ------------------------------------------------------------------ NaN
@functools.lru_cache(maxsize=None)
def nan_case(kind, net, S, A, k=K) -> sc.Case:
    """``kind`` "action": NaN in the explicit array at NAN_AT (action dims taken modulo A); "state": NaN in dimension
    NAN_STATE_DIM of the initial state.  Built without state_bar's assertion (a NaN entry has no bar); nan_bar_ok
    checks the cap on the finite entries."""
    if kind == "action":
        def explicit(a):
            a = a.copy()
            for h, k, j in NAN_AT:
                a[h, k, j % A] = np.nan
            return a
        g = {"explicit": explicit}
    else:
        from oracle import mpc_oracle as orc
        s = orc.synthetic_state(sc.normalization(S, A))
        s[NAN_STATE_DIM] = np.nan
        g = {"state": s}
    with np.errstate(invalid="ignore"):
        c = sc.Case(S, A, spec(net), k, H, check=False, given=g)
    c.regime = "nan-" + kind
    return c


def nan_bar_ok(c, src="explicit") -> float:
    """The largest bar / cap over the finite reference entries."""
    want, bar = c.states[src], c.bar(src)[0]
    ok = np.isfinite(want)
    assert np.isfinite(bar[ok]).all()
    return float(np.max(bar[ok] / dc.cap(want[ok]))) if ok.any() else 0.0


def fmax_states(c, src="explicit"):
    """The states of a copy of the oracle whose relu is np.fmax (the device's fmaxf: NaN -> 0)."""
    from oracle import mpc_oracle as orc
    with np.errstate(invalid="ignore"):
        return orc.rollout(Mutated(c.w, c.norm, relu=np.fmax), c.state, c.acts[src], sc.no_cost)[1]

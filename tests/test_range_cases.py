"""CPU only: what test_gpu_input_range.py's comparison rests on (range_cases.py), checked without a GPU -- every
regime x net's widened state bar stays within ROOM of its cap, its K oracle final states are distinct on every action
source, the size sweep's three mutations and the regime's own could not pass, the regime's inputs are what its name
says (the zero candidates are exactly zero and share a 16-column with ordinary ones, the dead candidates likewise, the
column maxima span the exponents the split kernels branch on), and the oracle's NaN pattern is non-trivial and is lost
by a relu formed with fmax."""
import numpy as np
import pytest

import depth_cases as dc
import range_cases as rc
import size_cases as sc

IDS = [f"{r}-{n}-S{s[0]}A{s[1]}" for r, n, s in rc.NET_CASES]


@pytest.mark.parametrize("regime,net,shape", rc.NET_CASES, ids=IDS)
def test_bar_has_room_states_distinct_and_mutations_could_not_pass(regime, net, shape):
    S, A = shape
    c = rc.case(regime, net, S, A)                      # (fails on its inputs when the widened bar passes the cap)
    ratio, d = rc.bar_over_cap(c), rc.distinct(c)
    m = {**rc.size_mutation_ratios(c), **rc.regime_mutation_ratios(c)}
    print(f"[range-cpu] {regime} {net} S={S} A={A}: bar / cap = {ratio:.2f}, distinct {d}, "
          + ", ".join(f"{k} {v:.0f}x" for k, v in m.items()))
    assert ratio <= rc.ROOM
    assert min(d.values()) == rc.K, d
    assert min(m.values()) > 10.0, m
    assert all(name in m for name, (_, regimes) in rc.MUTATIONS.items() if regime in regimes)


def column_max(c, src, h=0):
    """Per candidate, max |x| of the f32 layer-0 input at step ``h`` along the oracle's own trajectory."""
    from oracle import mpc_oracle as orc
    s = c.states[src][h]
    ns = (s - c.norm[0]) / (c.norm[1] + orc.NORM_EPS)
    na = (c.acts[src][h] - c.norm[2]) / (c.norm[3] + orc.NORM_EPS)
    return np.max(np.abs(np.concatenate([ns.astype(np.float32), na.astype(np.float32)], axis=1)), axis=1)


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda v: f"S{v[0]}A{v[1]}")
def test_regimes_reach_the_exponents_they_name(shape):
    """The column scale sh = 12 - e of the step-0 input per regime, against the base inputs' 10 and 11."""
    S, A = shape
    net = "2x500tanh"
    sh = {}
    for regime in ("far1", "farall", "zero", "const6-row", "const0-row", "tiny"):
        c = rc.case(regime, net, S, A)
        mx = column_max(c, "explicit")
        e = np.floor(np.log2(mx[mx > 0])).astype(int) + 1         # mx in [2^(e-1), 2^e)
        sh[regime] = sorted(set((12 - e).tolist()))
        if regime == "zero":
            assert (mx[:rc.ZERO_CANDS] == 0).all() and (mx[rc.ZERO_CANDS:] > 0).all()
            assert rc.ZERO_CANDS % 16 != 0                          # candidates 16..19 sit beside ordinary ones
            assert (column_max(c, "explicit", 1) > 0).all() and (column_max(c, "philox") > 0).all()
    base = sc.case(S, A, net, rc.K, rc.H)
    e = np.floor(np.log2(column_max(base, "explicit"))).astype(int) + 1
    print(f"[range-cpu] S={S} A={A} sh at step 0: base {sorted(set((12 - e).tolist()))}, {sh}")
    assert max(sh["far1"]) <= 4 and max(sh["farall"]) <= 7
    assert max(sh["const6-row"]) <= -6 and max(sh["const0-row"]) <= -17
    assert min(sh["tiny"]) >= 30


DEAD = [(n, s) for r, n, s in rc.NET_CASES if r == "dead"]


@pytest.mark.parametrize("net,shape", DEAD, ids=[f"{n}-S{s[0]}A{s[1]}" for n, s in DEAD])
def test_dead_columns_are_dead_in_the_oracle(net, shape):
    """Between 8 and K - 8 candidates of the explicit and the Philox source are dead at step 0 (and at least one of
    the CEM sample), a dead and a live one share a 16-column, and no candidate is dead or alive by a rounding: the
    shift's gap is more than 1e-4, a thousand f32 roundings of a pre-activation of order 1."""
    from oracle import mpc_oracle as orc
    S, A = shape
    c = rc.case("dead", net, S, A)
    counts = {}
    for src in sc.SOURCES:
        dead = rc.dead_mask(c, src)
        counts[src] = int(dead.sum())
        if src != "cem":
            assert 8 <= counts[src] <= rc.K - 8, (src, counts)
            cols = [dead[i:i + 16] for i in range(0, rc.K, 16)]
            assert any(col.any() and not col.all() for col in cols), src
    assert counts["cem"] >= 1, counts
    w0, norm = sc.weights(S, A, rc.spec(net)), sc.normalization(S, A)
    m = rc.dead_preacts(w0, norm, orc.synthetic_state(norm), sc.action_sources(A, rc.K, rc.H)[0])
    gap = rc.DEAD_GAP[(net, S)]
    print(f"[range-cpu] dead {net} S={S}: dead at step 0 {counts}, gap {gap} is {m[gap + 1] - m[gap]:.2e} wide")
    assert m[gap + 1] - m[gap] > 1e-4


@pytest.mark.parametrize("net", ["2x256reluLN", "2x512relu"])
def test_hot_activations_reach_the_thousands(net):
    c = rc.case("hot", net, 20, 6)
    x = rc._x0(c.w, c.norm, c.state, c.acts["philox"][0])
    h0 = np.maximum(x @ c.w.kernels[0] + c.w.biases[0], 0)
    if c.ln:
        from oracle import mpc_oracle as orc
        h0 = orc.layer_norm_tf1(h0, c.w.ln_gamma[0], c.w.ln_beta[0])
    h1 = np.maximum(h0 @ c.w.kernels[1] + c.w.biases[1], 0)
    print(f"[range-cpu] hot {net}: layer-1 activations reach {h1.max():.0f}")
    assert h1.max() > 1000.0


# ------------------------------------------------------------------ what was left out, measured
@pytest.mark.parametrize("std3", [1e-6, 0.0])
@pytest.mark.parametrize("net", ["2x500tanh", "2x256reluLN"])
def test_unscaled_near_constant_observation_is_degenerate(net, std3):
    """range_cases' docstring: with row 3 of layer 0 left as it is, the case cannot meet the guards."""
    c = rc.case("const6" if std3 else "const0", net, 20, 6, False)
    d, m = rc.distinct(c), rc.size_mutation_ratios(c)
    print(f"[range-cpu] unscaled std_obs[3]={std3:g} {net}: distinct {d}, " + ", ".join(f"{k} {v:.2g}x" for k, v in m.items()))
    assert min(d.values()) == 1 or min(m.values()) < 10.0


def test_relu_at_300_sigma_and_hot_without_the_output_scale_have_no_room():
    import copy
    S, A = 20, 6
    g = rc.given("far1", "2x500tanh", S, A)             # (300 sigma)
    far = rc.bar_over_cap(sc.Case(S, A, "2x512relu", rc.K, rc.H, check=False, given=g))
    w = copy.deepcopy(rc.case("hot", "2x512relu", S, A).w)
    w.kernels[2] = np.ldexp(w.kernels[2], rc.HOT_EXP[False])
    hot = rc.bar_over_cap(sc.Case(S, A, "2x512relu", rc.K, rc.H, check=False, given={"w": w}))
    print(f"[range-cpu] 2x512relu: far1 at 300 sigma bar / cap = {far:.2f}; hot without the output kernel's inverse power = {hot:.0f}")
    assert far > rc.ROOM and hot > rc.ROOM


# ------------------------------------------------------------------ NaN
NAN_NETS = ["2x64tanh", "2x500tanh", "2x64relu", "2x512relu", "2x256reluLN"]


@pytest.mark.parametrize("net", NAN_NETS)
def test_nan_pattern_is_non_trivial_and_fmax_loses_it(net):
    """NaN in the actions: the oracle's costs are NaN for exactly the candidates of NAN_AT, from the step of the NaN
    on; np.argmin picks the first of them.  On relu nets a relu formed with fmax returns finite states instead."""
    from oracle import mpc_oracle as orc
    c = rc.nan_case("action", net, 20, 6)
    want = c.states["explicit"]
    bad = np.isnan(want).any(axis=(0, 2))
    cands = sorted(k for _, k, _ in rc.NAN_AT)
    assert np.flatnonzero(bad).tolist() == cands and not bad.all()
    assert not np.isnan(want[:2]).any() and np.isnan(want[2:, cands]).all()
    assert np.array_equal(np.isnan(c.costs["explicit"]), bad) and orc.argmin_ref(c.costs["explicit"]) == cands[0]
    assert rc.nan_bar_ok(c) <= rc.ROOM
    lost = not np.isnan(rc.fmax_states(c)).any()
    print(f"[range-cpu] NaN actions {net}: NaN candidates {cands}, argmin {cands[0]}, fmax loses the NaN: {lost}")
    assert lost == rc.is_relu(net)
    s = rc.nan_case("state", net, 20, 6)
    assert np.isnan(s.states["explicit"][1:]).all() and np.isnan(s.costs["explicit"]).all()
    assert np.isnan(s.states["explicit"][0]).sum() == rc.K
    if rc.is_relu(net):
        lost = np.isnan(rc.fmax_states(s)[1:])          # (the residual add keeps the NaN in its own dimension)
        assert lost[..., rc.NAN_STATE_DIM].all() and lost.sum() == lost[..., rc.NAN_STATE_DIM].size

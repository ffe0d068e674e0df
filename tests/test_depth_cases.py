"""CPU only: what test_gpu_depth_width.py's comparison rests on (depth_cases.py), checked without a GPU -- every
net's widened state bar stays under its cap, its oracle outputs are distinct, a wrong layer slot or a live pad lane
could not pass, the cheetah-cost bar is not already broken by the reference's own roundings, the relu + LayerNorm
depths are the deepest the cap leaves room for, and the policies' f32 reference is far inside the action bar."""
import numpy as np
import pytest

import depth_cases as dc
import size_cases as sc

NET_SHAPE_IDS = [f"{n}-S{s[0]}A{s[1]}" for n, s in dc.NET_SHAPES]


@pytest.mark.parametrize("net,shape", dc.NET_SHAPES, ids=NET_SHAPE_IDS)
def test_bar_under_its_cap_and_outputs_distinct(net, shape):
    """size_cases.Case asserts the cap itself (state_bar); here the ratio is printed, the oracle's costs (final
    states where the shape has no cheetah cost) take more than K / 2 distinct values per action source, and on
    cheetah shapes the reference's five other roundings stay inside the fused cost's bar."""
    S, A = shape
    c = dc.case(net, S, A)                              # (fails on its inputs when the widened bar passes the cap)
    worst = max(float(np.max(c.bar(src)[0] / dc.cap(c.states[src]))) for src in sc.SOURCES)
    d = dc.distinct(c)
    print(f"[depth-cpu] {net} S={S} A={A}: bar / cap = {worst:.2f}, distinct {d}")
    assert worst <= 1.0
    assert min(d.values()) > dc.K // 2, d
    if c.cheetah:
        for src, (spread, tol) in dc.cost_conditioning(net, S, A).items():
            print(f"[depth-cpu] {net} {src}: the other roundings' costs spread {spread:.1e}, bar {tol:.1e}")
            assert spread <= tol, (net, src, spread, tol)


@pytest.mark.parametrize("net,shape", dc.NET_SHAPES, ids=NET_SHAPE_IDS)
def test_a_wrong_layer_slot_could_not_pass(net, shape):
    """Every mutation (a) - (d) of depth_cases moves the median candidate's worst state by more than 10 times the
    cap of the bar, 1e-5 (1 + |want|)."""
    r = dc.mutation_ratios(net, shape[0], shape[1])
    weakest = min(r, key=r.get)
    print(f"[depth-mutation] {net} S={shape[0]} A={shape[1]}: {len(r)} mutations, weakest {weakest} {r[weakest]:.0f}x")
    assert r[weakest] > 10.0, r


@pytest.mark.parametrize("hidden", sorted(dc.RELU_LN_DEPTH))
def test_relu_layer_norm_depth_is_the_deepest_with_room(hidden):
    """RELU_LN_DEPTH[hidden] is the largest L <= 8 whose widened bar is at most RELU_LN_ROOM of the cap on both
    DEPTH_SHAPES."""
    ratio = {L: max(dc.bar_over_cap((hidden, L, "relu", True, 1000), S, A) for S, A in dc.DEPTH_SHAPES)
             for L in range(dc.RELU_LN_DEPTH[hidden], 9)}
    print(f"[depth-cpu] relu + LayerNorm hidden {hidden}: " + ", ".join(f"L={L} {r:.3f}" for L, r in ratio.items()))
    assert max(L for L, r in ratio.items() if r <= dc.RELU_LN_ROOM) == dc.RELU_LN_DEPTH[hidden], ratio
    assert dc.NETS[f"{dc.RELU_LN_DEPTH[hidden]}x{hidden}reluLN"] == (hidden, dc.RELU_LN_DEPTH[hidden], "relu", True, 1000)


@pytest.mark.parametrize("layers,hidden", dc.POLICIES, ids=lambda v: str(v))
def test_policy_reference_is_inside_a_sixth_of_the_action_bar(layers, hidden):
    gap = dc.policy_gap(layers, hidden)
    print(f"[depth-cpu] policy {layers}x{hidden}: |f32 mean - f64 mean| / bar = {gap:.3f}")
    assert gap <= 1.0 / 6.0


@pytest.mark.parametrize("hidden", dc.REWARD_WIDTHS)
def test_reward_widths_are_distinct(hidden):
    assert dc.reward_distinct(hidden) > dc.K // 2


def test_the_size_sweep_is_unchanged():
    """A spec tuple names itself as size_cases.NETS' keys do and computes what the name computes."""
    for name, spec in sc.NETS.items():
        assert sc.net_name(spec) == name and sc.net_spec(name) == spec + (1000,) == sc.net_spec(spec)
    a, b = sc.weights(5, 2, "2x64tanh"), sc.weights(5, 2, (64, 2, "tanh", False))
    assert a.digest() == b.digest()

"""Every rollout kernel against the oracle across input magnitudes (range_cases.py holds the regimes, their inputs, the
bar and the CPU guards, test_range_cases.py checks them without a GPU; test_gpu_state_action_sizes.py's run_case holds
the checks; expectations come from oracle/mpc_oracle.py only).

The size and the depth sweep keep every candidate's largest normalised layer-0 input between 1 and 3.  The split
kernels branch on that number: per 16-candidate column max |x| picks the power of two that moves the column into
[2^11, 2^12) before the hi / lo f16 split (clamped to +-100, max == 0 special-cased), the relu path scales every
activation column the same way, LayerNorm divides by a column's spread, and the fp32 kernels' tanh sees arguments it
otherwise never sees.  The regimes -- one far dimension, every dimension displaced, an all-zero column, a near-constant
observation (std_obs = 1e-6 and 0) with its layer-0 row scaled by the exact power of two that undoes it, a column of
1e-6, dead relu columns, hot relu columns, NaN -- are range_cases' docstring; so is what was left out and why.

Per case (kernel, net, regime, S, A) at K = 70, H = 3 -- run_case's checks 1 - 3 on the regime's inputs: the states of
the explicit, Philox and CEM sources at size_cases' per-entry bar, row 0 exact, everything finite, nothing written
outside the padded buffers; cost="terms" costs bit for bit against trajectory_cost_fn of the engine's own trajectory;
cem_rollout_async bit for bit against the explicit CEM sample; at S = 20 the fused cheetah cost at assert_costs_close's
bar and the record's index = argmin.  Kernels and nets are size_cases.KERNEL_NETS'; the dead and the hot regime also
run a relu net without LayerNorm on every kernel that has one (range_cases.RELU_ON).  The engine refuses none of
these shapes (test_gpu_state_action_sizes.create_refusal, asserted by run_case as in the size sweep); CEM sampling on
solo is refused and asserted there.

The single-pass f16 layouts (test_gpu_state_action_sizes.test_f16_auto, K = 70, and test_f16_pipelined, K = 200) run
the six regimes a tanh net has, at test_gpu_f16's bar.

NaN (test_nan_*): the engine promises np.argmin's rule, the first NaN wins.  With NaN in the explicit actions (step 1,
candidates 5, 37 and 69, the last in the partly filled 16-column) and with NaN in one dimension of the initial state,
on a tanh, a relu and a relu + LayerNorm net per kernel: the trajectory's and the costs' NaN pattern equal the oracle's,
the record's index is oracle.argmin_ref of the oracle's costs, and every finite entry meets the ordinary bar.

Results of the run on one MI355X (profiles/input_range.txt): every kernel ran every regime it is listed for, no case
skipped; the largest |dstate| / bar is 0.37 (split4, 2x512relu, every dimension displaced).  Two things these tests
found and the same change fixed: every kernel's relu was fmaxf, which returns 0 for a NaN (all 40 relu NaN cases failed;
now IEEE maximum, device_common.h relu_nan), and the split kernels lost a layer-0 row that sits far below the kernel's
largest entry (const6-row 1.0 - 9.2 bars, const0-row 3,000 - 71,000; now pack.cpp fold_layer0_rows).
"""
import ctypes

import numpy as np
import pytest

import range_cases as rc
import size_cases as sc
from test_gpu_state_action_sizes import (a_gpu_fault_stops_the_run, create_refusal, launch, make_engine, pp3_takes,
                                         run_case)

pytestmark = pytest.mark.gpu


def range_line(kernel, ran, c, worst):
    return f"[range-case] kernel={kernel} ran={ran} {c.net} {c.regime} S={c.S} A={c.A} worst={worst:.3f}"


@pytest.mark.parametrize("kernel,net,regime,shape", rc.KERNEL_CASES,
                         ids=[f"{k}-{n}-{r}-S{s[0]}A{s[1]}" for k, n, r, s in rc.KERNEL_CASES])
@a_gpu_fault_stops_the_run
def test_rollout_matches_oracle(kernel, net, regime, shape, monkeypatch):
    run_case(kernel, rc.case(regime, net, shape[0], shape[1]), monkeypatch, refusal=create_refusal, line=range_line)


# ------------------------------------------------------------------ single-pass f16
def f16_case(c, label):
    from oracle import mpc_oracle as orc
    from test_gpu_f16 import F16_NEAR, _check, _engine
    eng = _engine(c.S, c.A, c.w, c.H, c.K, c.norm)      # (asserts the rollout_pp<512 layout under BCMPC_F16_PP=1)
    try:
        eng.set_action_bounds(c.low, c.high)
        for src in ("explicit", "philox"):
            res = eng.get_action(c.state, c.acts[src] if src == "explicit" else None, seed=sc.SEED,
                                 cand_offset=sc.OFF, return_costs=True)
            _check(res.costs, c.costs[src], orc.near_threshold_mask(c.states[src], F16_NEAR), c.H,
                   f"{label} {c.regime} {src}")
            i = res.best_index - sc.OFF
            assert i == int(np.argmin(res.costs)) and np.array_equal(res.first_action, c.acts[src][0, i])
        return eng.info()
    finally:
        eng.close()


@pytest.mark.parametrize("regime", rc.F16_REGIMES)
@a_gpu_fault_stops_the_run
def test_f16_auto(regime, monkeypatch):
    monkeypatch.delenv("BCMPC_F16_PP", raising=False)
    f16_case(rc.case(regime, "2x500tanh", 20, 6), "auto")


@pytest.mark.parametrize("regime", rc.F16_REGIMES)
@a_gpu_fault_stops_the_run
def test_f16_pipelined(regime, monkeypatch):
    monkeypatch.setenv("BCMPC_F16_PP", "1")
    info = f16_case(rc.case(regime, "2x500tanh", 20, 6, True, sc.K_PP), "pp")
    assert info["layout"].startswith("rollout_pp<512"), info


# ------------------------------------------------------------------ NaN
def nan_nets(kernel):
    nets = [next(n for n in sc.KERNEL_NETS[kernel] if "tanh" in n)]
    if kernel != "pp3":                                 # (rollout_pp3 takes the plain tanh net only)
        nets += [rc.RELU_ON[kernel], "2x256reluLN"]
    return nets


NAN_CASES = [(k, n, kind) for k in sc.KERNEL_NETS for n in nan_nets(k) for kind in ("action", "state")]


@pytest.mark.parametrize("kernel,net,kind", NAN_CASES, ids=[f"{k}-{n}-{kind}" for k, n, kind in NAN_CASES])
@a_gpu_fault_stops_the_run
def test_nan_pattern_and_argmin_match_the_oracle(kernel, net, kind, monkeypatch):
    from oracle import mpc_oracle as orc
    from test_gpu_parity import assert_costs_close
    from conftest import envelope
    c = rc.nan_case(kind, net, 20, 6)
    assert rc.nan_bar_ok(c) <= 1.0
    monkeypatch.delenv("BCMPC_SPLIT_PP", raising=False)
    if kernel == "pp3":
        monkeypatch.setenv("BCMPC_SPLIT_PP", "1")
    eng = make_engine(c, "auto" if kernel == "pp3" else kernel, "cheetah")
    try:
        info = eng.info()
        if kernel == "pp3":
            assert info["layout"].startswith("rollout_pp3") == pp3_takes(c), info
        elif kernel != "auto":
            assert info["kernel"] == kernel, info
        got, costs, index = launch(eng, c, "explicit", explicit=True)
        want, want_costs = c.states["explicit"], c.costs["explicit"]
        label = f"{kernel} {net} NaN {kind}"
        assert np.array_equal(got[0], np.tile(c.state, (c.K, 1)), equal_nan=True), f"{label}: row 0"
        nan_g, nan_w = np.isnan(got), np.isnan(want)
        print(f"[range-nan] kernel={kernel} ran={info['kernel']} {net} {kind}: NaN entries {int(nan_g.sum())} "
              f"(oracle {int(nan_w.sum())}), NaN costs {int(np.isnan(costs).sum())} (oracle "
              f"{int(np.isnan(want_costs).sum())}), index {index - sc.OFF} (oracle {orc.argmin_ref(want_costs)})")
        assert np.array_equal(nan_g, nan_w), (
            f"{label}: the trajectory's NaN pattern differs at {np.argwhere(nan_g != nan_w)[:4].tolist()} ...")
        assert not np.isinf(got).any()
        ok = ~nan_w
        ratio = np.abs(got[ok] - want[ok]) / c.bar("explicit")[0][ok]
        assert ratio.size == 0 or ratio.max() <= 1.0, f"{label}: finite entries {ratio.max():.2f}x the bar"
        assert np.array_equal(np.isnan(costs), np.isnan(want_costs)), f"{label}: the costs' NaN pattern differs"
        fin = ~np.isnan(want_costs)
        if fin.any():
            assert_costs_close(costs[fin], want_costs[fin], orc.near_threshold_mask(want[:, fin]), label,
                               env=envelope(c.ln, c.L, c.hidden, c.H))
        assert index - sc.OFF == orc.argmin_ref(want_costs), (index - sc.OFF, orc.argmin_ref(want_costs))
    finally:
        eng.close()


@pytest.mark.parametrize("pp", [False, True], ids=["auto", "pipelined"])
@a_gpu_fault_stops_the_run
def test_f16_nan_actions(pp, monkeypatch):
    from oracle import mpc_oracle as orc
    from test_gpu_f16 import F16_NEAR, _check, _engine
    monkeypatch.delenv("BCMPC_F16_PP", raising=False)
    if pp:
        monkeypatch.setenv("BCMPC_F16_PP", "1")
    c = rc.nan_case("action", "2x500tanh", 20, 6, sc.K_PP if pp else rc.K)
    eng = _engine(c.S, c.A, c.w, c.H, c.K, c.norm)
    try:
        assert not pp or eng.info()["layout"].startswith("rollout_pp<512"), eng.info()
        eng.set_action_bounds(c.low, c.high)
        res = eng.get_action(c.state, c.acts["explicit"], seed=sc.SEED, cand_offset=sc.OFF, return_costs=True)
        want = c.costs["explicit"]
        fin = ~np.isnan(want)
        near = np.zeros(c.K, dtype=bool)
        near[fin] = orc.near_threshold_mask(c.states["explicit"][:, fin], F16_NEAR)
        _check(res.costs, want, near, c.H, f"{'pp' if pp else 'auto'} NaN actions")       # (NaN pattern first)
        assert res.best_index - sc.OFF == orc.argmin_ref(want)
    finally:
        eng.close()

"""Single-pass f16 precision (BCMPC_PREC_F16, engine precision "f16").

BASELINE configs[2] names cfg3 as "bf16 MFMA GEMM + fp32 cost accumulate".  The f16 mode is that
configuration with f16's 11-bit significand instead of bf16's 8: every dense-layer operand is rounded
once to f16 (hi part only, same power-of-two scales as the split kernel), one
v_mfma_f32_16x16x32_f16 pass, f32 accumulate; normalisation, de-normalisation, the residual, the
cheetah cost and the trajectory sum stay f64 exactly as in the split kernel.  It is NOT the fp32
tolerance of test_gpu_parity.py (the bench's `value` never uses it).  The bar here:

* per-candidate cost within F16_TOL_STEP * H of the oracle (the fixtures' reference-run costs), except
  exact +-10 flips of candidates within F16_NEAR of a penalty threshold (the f16 state error is ~100x the
  split kernel's, so the f32 bar's 1e-4 margin widens to 1e-3);
* argmin quality: the oracle cost of the f16 engine's choice is within 2 * F16_TOL_STEP * H of the
  oracle's minimum; the returned first action is the action array's row of that choice (bit-identical);
* NaN pattern identical;
* at cfg3 full size: deterministic, shard invariant (bitwise), argmin consistent with its own costs.

F16_TOL_STEP is set from the measured worst case (printed) with headroom: a 2x regression fails.
"""
import os

import numpy as np
import pytest

from conftest import Golden, golden_names

pytestmark = pytest.mark.gpu

F16_TOL_STEP = 8e-3        # |dcost| per horizon step (measured worst 3.5e-3, typical 1e-3: DESIGN.md 6.7)
F16_NEAR = 1e-3            # penalty-threshold margin of an allowed +-10 flip


def _mpc_tanh_fixtures():
    out = []
    for n in golden_names("mpc"):
        g = Golden(n)
        if g.meta["act"] == "tanh" and not g.meta["ln"] and g.meta.get("inject") != "philox":
            out.append(n)
    return out


def _engine(S, A, w, H, K, norm, kernel="auto"):
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    eng = RolloutEngine(S, A, w.hidden, w.n_layers, w.activation, False, H, K, kernel=kernel, precision="f16")
    eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation), norm, version=1)
    if os.environ.get("BCMPC_F16_PP") == "1" and K >= 128 and w.n_layers == 2 and 256 < w.hidden <= 512:
        # (the pp_kernel tests: the pipelined kernel must really be the one that runs, not a silent
        #  fallback to the single-group layouts)
        assert eng.info()["layout"].startswith("rollout_pp<512"), eng.info()["layout"]
    return eng


def _check(got, want, near, H, label):
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), f"{label}: NaN pattern differs"
    ok = ~nan_w
    tol = F16_TOL_STEP * H
    diff = np.abs(got[ok] - want[ok])
    bad = diff > tol
    if near is not None:
        flip = np.abs(diff - 10.0 * np.round(diff / 10.0)) <= tol
        bad &= ~(near[ok] & flip)
    far = diff[~(near[ok] if near is not None else np.zeros_like(bad))]     # (empty where every candidate is near)
    worst = float(far.max()) if far.size else 0.0
    print(f"[f16 {label}] max|dcost|={worst:.3e} per-step={worst / H:.3e} n={int(ok.sum())} "
          f"over_tol={int(bad.sum())}")
    assert not bad.any(), f"{label}: {int(bad.sum())} costs beyond {tol}"
    return tol


@pytest.mark.parametrize("kernel", ["auto", "split1", "split2", "split4"])
@pytest.mark.parametrize("name", _mpc_tanh_fixtures())
def test_f16_engine_vs_reference_fixture(name, kernel):
    g = Golden(name)
    if kernel == "split4" and g.meta["hidden"] <= 64:
        pytest.skip("split4 needs >= 4 waves (hidden > 64)")
    eng = _engine(g.S, g.A, g.weights, g.H, g.K, g.norm, kernel)
    assert eng.info()["kernel"] in ("split1", "split2", "split4")
    from oracle import mpc_oracle as orc
    acts = g.actions()
    res = eng.get_action(g.state, acts, return_costs=True)
    want, states = orc.rollout(orc.NumpyDynamics(g.weights, g.norm), g.state, acts)
    assert np.array_equal(want, g.costs, equal_nan=True)            # the oracle is the fixture
    tol = _check(res.costs, g.costs, orc.near_threshold_mask(states, F16_NEAR), g.H, f"{name}/{kernel}")
    i = res.best_index
    assert i == int(np.argmin(res.costs))
    assert np.array_equal(res.first_action, acts[0, i])
    if not np.isnan(g.costs).any():
        assert g.costs[i] - np.min(g.costs) <= 2 * tol, "f16 choice is not near-optimal under the oracle"
    eng.close()


@pytest.mark.parametrize("hidden,L", [(1024, 3), (768, 2), (600, 2)])
def test_f16_large_hidden_vs_oracle(hidden, L):
    from oracle import mpc_oracle as orc
    K, H = 96, 4
    w = orc.synthetic_weights(20, 6, hidden, L, "tanh", False, seed_base=77)
    norm = orc.synthetic_normalization()
    state = orc.synthetic_state(norm)
    acts = np.random.RandomState(5).uniform(-1, 1, (H, K, 6))
    eng = _engine(20, 6, w, H, K, norm)
    res = eng.get_action(state, acts, return_costs=True)
    want, states = orc.rollout(orc.NumpyDynamics(w, norm), state, acts)
    _check(res.costs, want, orc.near_threshold_mask(states, F16_NEAR), H, f"h{hidden}xL{L}")
    eng.close()


def test_f16_full_size_cfg3_properties():
    """K=65536, H=20, 2x500 tanh at full size: determinism, shard invariance (bitwise), argmin
    consistency, a 256-candidate oracle sample within the f16 bar, and the f16 costs against the
    split (f32-grade) engine's on the whole vector."""
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc
    K, H = 65536, 20
    w = orc.synthetic_weights(20, 6, 500, 2, "tanh", False)
    norm = orc.synthetic_normalization()
    state = orc.synthetic_state(norm)
    full = _engine(20, 6, w, H, K, norm)
    seed = 0xC0FFEE
    r1 = full.get_action(state, None, seed=seed, return_costs=True)
    r2 = full.get_action(state, None, seed=seed, return_costs=True)
    assert np.array_equal(r1.costs, r2.costs) and r1.best_index == r2.best_index
    assert r1.best_index == int(np.argmin(r1.costs))
    half = _engine(20, 6, w, H, K // 2, norm)
    a = half.get_action(state, None, seed=seed, cand_offset=0, return_costs=True)
    b = half.get_action(state, None, seed=seed, cand_offset=K // 2, return_costs=True)
    assert np.array_equal(np.concatenate([a.costs, b.costs]), r1.costs)
    rs = np.random.RandomState(1)
    idx = np.unique(np.concatenate([rs.choice(K, 255, replace=False), [r1.best_index]]))
    acts = orc.device_rng_actions(seed, 0, K, H, -np.ones(6), np.ones(6))[:, idx, :]
    want, states = orc.rollout(orc.NumpyDynamics(w, norm), state, acts)
    _check(r1.costs[idx], want, orc.near_threshold_mask(states, F16_NEAR), H, "cfg3-sample")
    split = RolloutEngine(20, 6, 500, 2, "tanh", False, H, K, precision="split")
    split.set_weights(MLPSpec(w.kernels, w.biases, w.activation), norm, 1)
    rs_ = split.get_action(state, None, seed=seed, return_costs=True)
    d = np.abs(r1.costs - rs_.costs)
    d = d[np.isfinite(d)]
    flip = np.abs(d - 10.0 * np.round(d / 10.0))
    print(f"[f16 vs split, cfg3 full] median|dcost|={np.median(flip):.3e} p99={np.quantile(flip, 0.99):.3e} "
          f"max={flip.max():.3e}; argmin f16={r1.best_index} split={rs_.best_index} "
          f"split cost of the f16 choice - split min = {rs_.costs[r1.best_index] - rs_.best_cost:.3e}")
    assert flip.max() <= F16_TOL_STEP * H
    assert rs_.costs[r1.best_index] - rs_.best_cost <= 2 * F16_TOL_STEP * H
    for e in (full, half, split):
        e.close()


def test_f16_argmin_agreement_cfg3_16_seeds():
    """how often the single-pass f16 engine picks the reference's argmin at cfg3 (K=65536,
    H=20, 2x500 tanh), over 16 seeds of the device actions.  bf16/f16-class GEMMs cannot promise a
    bit-exact argmin, so this is reported, with a bound on the regret.  The oracle's argmin is
    found from the split (f32-grade) engine's cost vector, which is within the fp32 envelope of the oracle:
    its top-8 candidates plus the f16 choice are re-costed by the oracle, whose argmin over them is the
    oracle's argmin whenever the split's 8th-best is more than 2e-4 above its best (asserted)."""
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc
    K, H = 65536, 20
    w = orc.synthetic_weights(20, 6, 500, 2, "tanh", False)
    norm = orc.synthetic_normalization()
    state = orc.synthetic_state(norm)
    f16 = _engine(20, 6, w, H, K, norm)
    split = RolloutEngine(20, 6, 500, 2, "tanh", False, H, K, precision="split")
    split.set_weights(MLPSpec(w.kernels, w.biases, w.activation), norm, 1)
    dyn = orc.NumpyDynamics(w, norm)
    agree, regrets = 0, []
    for seed in range(1, 17):
        rf = f16.get_action(state, None, seed=seed, return_costs=False)
        rs = split.get_action(state, None, seed=seed, return_costs=True)
        top = np.argsort(rs.costs, kind="stable")[:8]
        assert rs.costs[top[7]] - rs.costs[top[0]] > 2e-4, "the oracle argmin is not pinned by the top 8"
        idx = np.unique(np.concatenate([top, [rf.best_index]]))
        acts = orc.device_rng_actions(seed, 0, K, H, -np.ones(6), np.ones(6))[:, idx, :]
        want, _ = orc.rollout(dyn, state, acts)
        best = int(idx[int(np.argmin(want))])
        agree += int(rf.best_index == best)
        regrets.append(float(want[list(idx).index(rf.best_index)] - np.min(want)))
    print(f"[f16 argmin agreement, cfg3, 16 seeds] top-1 equal {agree}/16; oracle-cost regret of the f16 choice: "
          f"median {np.median(regrets):.3e}, max {np.max(regrets):.3e} (costs ~ -1e2..1e2; bar {2 * F16_TOL_STEP * H})")
    assert max(regrets) <= 2 * F16_TOL_STEP * H
    f16.close()
    split.close()


@pytest.fixture
def pp_kernel(monkeypatch):
    monkeypatch.setenv("BCMPC_F16_PP", "1")
    yield
    monkeypatch.delenv("BCMPC_F16_PP", raising=False)


def _pp_fixtures():
    out = []
    for n in _mpc_tanh_fixtures():
        g = Golden(n)
        if g.meta["hidden"] > 256 and g.meta["hidden"] <= 512 and g.meta["L"] == 2 and g.K >= 128:
            out.append(n)
    return out


@pytest.mark.parametrize("name", _pp_fixtures())
def test_f16_pp_vs_reference_fixture(name, pp_kernel):
    """The two-group pipelined single-pass kernel (rollout_pp, BCMPC_F16_PP=1) on the reference-run
    fixtures it takes (2-layer tanh, hidden 257..512, K >= 128): the f16 bar, NaN pattern, argmin quality."""
    test_f16_engine_vs_reference_fixture(name, "auto")


@pytest.mark.parametrize("K,H", [(128, 1), (200, 3), (1000, 15), (4096, 7)])
def test_f16_pp_ragged_vs_oracle(K, H, pp_kernel):
    """Ragged K (a partly empty second group, a partly empty column), H = 1 and an odd H: the pipelined
    kernel against the oracle on the same Philox actions (the f16 bar), and deterministic."""
    from oracle import mpc_oracle as orc
    w = orc.synthetic_weights(20, 6, 500, 2, "tanh", False, seed_base=31)
    norm = orc.synthetic_normalization()
    state = orc.synthetic_state(norm)
    eng = _engine(20, 6, w, H, K, norm)
    res = eng.get_action(state, None, seed=77, return_costs=True)
    acts = orc.device_rng_actions(77, 0, K, H, -np.ones(6), np.ones(6))
    want, states = orc.rollout(orc.NumpyDynamics(w, norm), state, acts)
    _check(res.costs, want, orc.near_threshold_mask(states, F16_NEAR), H, f"pp K{K} H{H}")
    assert res.best_index == int(np.argmin(res.costs))
    r2 = eng.get_action(state, None, seed=77, return_costs=True)
    assert np.array_equal(r2.costs, res.costs)                       # deterministic
    eng.close()


def test_f16_pp_full_size_cfg3_properties(pp_kernel):
    """cfg3 at full size on the pipelined kernel: the full-size properties of the single-group test
    (determinism, bitwise shard invariance, oracle sample, the split engine's whole cost vector)."""
    test_f16_full_size_cfg3_properties()


def test_f16_refuses_other_nets():
    from bc_mpc_amd.engine import RolloutEngine
    with pytest.raises(Exception):
        RolloutEngine(20, 6, 256, 2, "relu", True, 7, 400, precision="f16")
    with pytest.raises(Exception):
        RolloutEngine(20, 6, 500, 2, "tanh", False, 7, 400, precision="f16", kernel="team")


@pytest.mark.parametrize("dim,std", [(3, 1e-6), (9, 1e5)])
def test_f16_pp_fold_input_range(monkeypatch, dim, std):
    """rollout_pp's folded layer 0 (BCMPC_PP_FOLD, the default) converts the normalised input to f16 WITHOUT a
    power-of-two scale, clamped to +-65504: a state dim with a near-zero std_obs normalises to
    ~1e5 and saturates, one with a huge std_obs normalises below f16's normal range.  Saturation is benign
    here because the first layer's tanh saturates long before (|x W| >> 1 at x = 65504), and a subnormal
    input is off by less than 6e-8 absolute: the f16 bar holds against the oracle, which uses the unclamped
    f32 input."""
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc
    monkeypatch.setenv("BCMPC_F16_PP", "1")
    K, H = 512, 5
    w = orc.synthetic_weights(20, 6, 500, 2, "tanh", False)
    norm = [np.array(a, copy=True) for a in orc.synthetic_normalization()]
    norm[1][dim] = std                                  # std_obs
    state = orc.synthetic_state(orc.synthetic_normalization())
    eng = RolloutEngine(20, 6, 500, 2, "tanh", False, H, K, precision="f16")
    eng.set_weights(MLPSpec(w.kernels, w.biases, "tanh"), norm, 1)
    layout = eng.info()["layout"]
    assert layout.startswith("rollout_pp<512,fold"), layout
    acts = np.random.RandomState(5).uniform(-1, 1, (H, K, 6))
    x = abs((state[dim] - norm[0][dim]) / (std + 1e-10))
    assert (x > 65504) if std < 1 else (x < 6.2e-5), x
    res = eng.get_action(state, acts, return_costs=True)
    want, paths = orc.rollout(orc.NumpyDynamics(w, norm), state, acts)
    near = np.zeros(K, dtype=bool)
    for hh in range(H + 1):
        s = paths[hh]
        near |= (np.abs(s[:, 5] - 0.2) < F16_NEAR) | (np.abs(s[:, 6]) < F16_NEAR) | (np.abs(s[:, 7]) < F16_NEAR)
    _check(res.costs, want, near, H, f"pp fold, std_obs[{dim}]={std:g} (|x|={x:.3g})")
    eng.close()

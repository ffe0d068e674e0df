"""rollout_pp3: split precision (hi + lo operands, three MFMA passes) on the two-group pipelined layout --
two 64-candidate groups per workgroup, one in its hidden layer's MFMAs while the other runs its tanh /
output / f64 / layer-0 chain, over one time-shared slab.  The GPU tests force the layout with
BCMPC_SPLIT_PP=1 and hold it to the split kernel's bar against the oracle (tests/test_gpu_parity.py)."""
import numpy as np
import pytest

from conftest import Golden, envelope

LAYOUT = "rollout_pp3"
S, A, HID = 20, 6, 500
SEED = 77
SHAPES = [(1, 1), (64, 3), (128, 1), (200, 3), (1000, 15), (4096, 7)]


# ---- host side, no GPU ----
def test_layout_shape_query_without_a_device():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    f = lib.bcmpc_split_pp_lds_bytes
    total = f(HID, 2, S, A)
    # consts + biases 6,784 | slab 131,072 | partials 20,480 | action inputs 2 x 1,536 | counters 16
    assert total == 6784 + 131072 + 20480 + 2 * 1536 + 16 <= 163840
    assert f(512, 2, S, A) == total and f(497, 2, S, A) == total
    assert f(HID, 2, 20, 13) == -1 and f(HID, 2, 27, 6) == -1        # S + A > 32
    assert f(HID, 1, S, A) == -1 and f(HID, 3, S, A) == -1            # L != 2
    assert f(256, 2, S, A) == -1 and f(1000, 2, S, A) == -1           # hidden padded to 512 only
    assert f(HID, 2, 24, 6) == -1                                     # two lane rows of tile-1 partials: over 160 KiB
    assert 0 < f(HID, 2, 17, 3) <= 163840


# ---- GPU ----
_cache = {}


def _net():
    if "net" not in _cache:
        from oracle import mpc_oracle as orc
        w = orc.synthetic_weights(S, A, HID, 2, "tanh", False, seed_base=31)
        norm = orc.synthetic_normalization(S, A)
        _cache["net"] = (w, norm, orc.synthetic_state(norm))
    return _cache["net"]


def _reference(K, H):
    """Oracle costs / states / actions of the device-Philox rollout (seed 77), computed once per shape."""
    key = ("ref", K, H)
    if key not in _cache:
        from oracle import mpc_oracle as orc
        w, norm, state = _net()
        acts = orc.device_rng_actions(SEED, 0, K, H, -np.ones(A), np.ones(A))
        costs, states = orc.rollout(orc.NumpyDynamics(w, norm), state, acts)
        for arr in (acts, costs, states):
            arr.setflags(write=False)
        _cache[key] = (acts, costs, states)
    return _cache[key]


def _engine(K, H, cost="cheetah", kernel="auto", **kw):
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    w, norm, _ = _net()
    eng = RolloutEngine(S, A, HID, 2, "tanh", False, H, K, device=0, cost=cost, kernel=kernel, **kw)
    eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation), norm, 1)
    return eng


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("BCMPC_SPLIT_PP", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("K,H", SHAPES)
def test_oracle_parity(K, H, forced):
    """K = 1: one lane valid; 64: group 1 empty; 200: a partly empty group and column; H = 1: the pipeline's
    prologue and epilogue only; odd H; H = 15 / K = 4096: many steps, many workgroups."""
    from oracle import mpc_oracle as orc
    from test_gpu_parity import assert_costs_close
    _, _, state = _net()
    acts, want, states = _reference(K, H)
    eng = _engine(K, H)
    assert eng.info()["layout"].startswith(LAYOUT), eng.info()["layout"]
    assert eng.info()["kernel"] == "split4"
    r1 = eng.get_action(state, None, seed=SEED, return_costs=True)
    r2 = eng.get_action(state, None, seed=SEED, return_costs=True)
    assert r1.costs.tobytes() == r2.costs.tobytes() and r1.best_index == r2.best_index
    assert_costs_close(r1.costs, want, orc.near_threshold_mask(states), f"pp3 K={K} H={H}",
                       env=envelope(False, 2, HID, H))
    assert r1.best_index == int(np.argmin(r1.costs))
    assert np.array_equal(r1.first_action, acts[0, r1.best_index])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg1_2x500_tanh", "cfg2_2x500_tanh"])
def test_reference_fixtures(name, forced):
    from test_gpu_parity import _engine as fixture_engine, argmin_is_decidable, assert_costs_close
    g = Golden(name)
    # (the nan_candidates fixture's net, hidden 64, is outside the layout's shapes)
    eng = fixture_engine(g)
    assert eng.info()["layout"].startswith(LAYOUT), eng.info()["layout"]
    if g.meta.get("inject") == "philox":
        res = eng.get_action(g.state, None, seed=g.meta["rng_seed"], cand_offset=g.meta["cand_offset"],
                             return_costs=True)
        offset = g.meta["cand_offset"]
    else:
        res = eng.get_action(g.state, g.actions(), return_costs=True)
        offset = 0
    assert_costs_close(res.costs, g.costs, g.near, f"{name}/pp3",
                       env=envelope(g.meta["ln"], g.weights.n_layers, g.meta["hidden"], g.H), cond=g.cond)
    assert res.best_index - offset == int(np.argmin(res.costs))
    if argmin_is_decidable(g):
        assert res.best_index - offset == g.argmin
        assert np.array_equal(res.first_action, g.opt_action)
        if not np.isnan(g.costs[g.argmin]):
            assert res.best_cost == res.costs[g.argmin]
    eng.close()


@pytest.mark.gpu
def test_shard_invariance_is_bitwise(forced):
    """K = 1000 whole against the shards 0-499 and 500-999: the group and column boundaries fall differently."""
    _, _, state = _net()
    H = 15
    whole = _engine(1000, H)
    half = _engine(500, H)
    for e in (whole, half):
        assert e.info()["layout"].startswith(LAYOUT)
    r = whole.get_action(state, None, seed=SEED, return_costs=True)
    a = half.get_action(state, None, seed=SEED, cand_offset=0, return_costs=True)
    b = half.get_action(state, None, seed=SEED, cand_offset=500, return_costs=True)
    assert np.concatenate([a.costs, b.costs]).tobytes() == r.costs.tobytes()
    assert r.costs.tobytes() == _engine_costs_again(whole, state)
    whole.close()
    half.close()


def _engine_costs_again(eng, state):
    return eng.get_action(state, None, seed=SEED, return_costs=True).costs.tobytes()


@pytest.mark.gpu
def test_host_actions_equal_device_rng_bitwise(forced):
    _, _, state = _net()
    K, H = 200, 3
    acts, _, _ = _reference(K, H)
    eng = _engine(K, H)
    assert eng.info()["layout"].startswith(LAYOUT)
    dev = eng.get_action(state, None, seed=SEED, return_costs=True)
    host = eng.get_action(state, np.array(acts), return_costs=True)
    assert host.costs.tobytes() == dev.costs.tobytes()
    assert host.best_index == dev.best_index and np.array_equal(host.first_action, dev.first_action)
    eng.close()


@pytest.mark.gpu
def test_trajectory_states(forced):
    """states_paths_all from the kernel (cost "none": the trajectory output) at test_trajectory_states_match's bar."""
    import torch
    _, _, state = _net()
    K, H = 200, 3
    acts, _, want = _reference(K, H)
    eng = _engine(K, H, cost="none")
    assert eng.info()["layout"].startswith(LAYOUT)
    dev = torch.device("cuda", 0)
    st = torch.from_numpy(state).to(dev)
    act = torch.from_numpy(np.ascontiguousarray(acts)).to(dev)
    traj = torch.full((H + 1, K, S), np.nan, dtype=torch.float64, device=dev)
    eng.rollout_async(st.data_ptr(), 0, act.data_ptr(), 0, 0, None, traj.data_ptr(), None,
                      torch.cuda.current_stream(dev).cuda_stream)
    got = traj.cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(got[0], want[0])               # tiled initial state is exact
    err = np.abs(got - want)
    print(f"[pp3 traj] max|dstate|={err.max():.3e}")
    assert (err <= 1e-6 + 1e-6 * np.abs(want)).all()
    eng.close()


@pytest.mark.gpu
def test_against_rollout_x3(monkeypatch):
    """Both kernels are within one bar of the oracle, so within two of each other."""
    from test_gpu_parity import ATOL, RTOL
    _, _, state = _net()
    K, H = 4096, 20
    monkeypatch.setenv("BCMPC_SPLIT_PP", "0")
    base = _engine(K, H, kernel="split4")
    assert base.info()["layout"].startswith("rollout_x3<512,NC=4,NW=8>"), base.info()["layout"]
    monkeypatch.setenv("BCMPC_SPLIT_PP", "1")
    eng = _engine(K, H)
    assert eng.info()["layout"].startswith(LAYOUT)
    c0 = base.get_action(state, None, seed=SEED, return_costs=True).costs
    c1 = eng.get_action(state, None, seed=SEED, return_costs=True).costs
    d = np.abs(c1 - c0)
    print(f"[pp3 vs x3] max|dcost|={d.max():.3e}")
    assert (d <= 2 * (ATOL + RTOL * np.abs(c0))).all()
    base.close()
    eng.close()


@pytest.mark.gpu
def test_selection(monkeypatch):
    """Engines only, no launch: what kernel="auto" picks with the variable unset, and what stays on rollout_x3."""
    from bc_mpc_amd.engine import RolloutEngine
    monkeypatch.delenv("BCMPC_SPLIT_PP", raising=False)

    def layout(K, kernel="auto", H=20, **kw):
        args = dict(activation="tanh", layer_norm=False)
        args.update({k: kw.pop(k) for k in ("activation", "layer_norm") if k in kw})
        e = RolloutEngine(S, A, HID, 2, args["activation"], args["layer_norm"], H, K, kernel=kernel, **kw)
        name = e.info()["layout"]
        e.close()
        return name

    auto = {K: layout(K) for K in (32768, 65536)}
    assert auto[32768] == auto[65536]                    # (test_full_size_cfg3_properties compares them bitwise)
    assert auto[65536].startswith(AUTO_LAYOUT), auto
    assert layout(16384).startswith("rollout_x3<512,NC=4,NW=8>")
    # short horizons: the pipeline's two extra intervals outweigh its gain (auto from H = 14)
    assert layout(65536, H=14).startswith(AUTO_LAYOUT) and layout(65536, H=13).startswith("rollout_x3<512,NC=4,NW=8>")
    assert layout(65536, kernel="split4").startswith("rollout_x3<512,NC=4,NW=8>")
    # the nets outside the layout keep their kernels
    assert layout(65536, model="reward", cost="reward").startswith("rollout_x3<")
    assert layout(65536, policy_hidden=64, policy_layers=2).startswith("rollout_x3<")
    assert layout(65536, layer_norm=True).startswith("rollout_x3<")
    assert layout(65536, activation="relu").startswith("rollout_x3<")
    assert layout(65536, cost="terms").startswith("rollout_x3<")
    monkeypatch.setenv("BCMPC_SPLIT_PP", "0")
    assert layout(65536).startswith("rollout_x3<512,NC=4,NW=8>")
    monkeypatch.setenv("BCMPC_SPLIT_PP", "1")
    assert layout(1).startswith(LAYOUT) and layout(65536).startswith(LAYOUT)
    assert layout(65536, kernel="split4").startswith("rollout_x3<")


# what kernel="auto" selects at >= 2048 candidate columns with BCMPC_SPLIT_PP unset (the A/B)
AUTO_LAYOUT = "rollout_pp3"

"""Every rollout kernel against the oracle across network depth and width (depth_cases.py holds the nets, the inputs,
the bar and the CPU guard; test_gpu_state_action_sizes.py's run_case holds the checks; expectations come from
oracle/mpc_oracle.py only).

The engine takes n_layers 1..8 and hidden 1..1024.  Depth is no mere loop count in the kernels: every LDS carve-out
begins at param_bytes(L, HP), the host decides what fits from the same formulas, and the operand scales, the bias and
weight offsets, the LayerNorm slots and rollout_x3's resident layer-1 k-steps are all indexed by layer.  Width pads to
64 / 128 / 256 / 512 / 768 / 1024: the pad lanes of a width one past a boundary must stay zero through every layer and
out of the LayerNorm statistics.

Per case (kernel, net, S, A) at K = 70, H = 3 -- run_case's checks 1 - 3: the states of the explicit, Philox and CEM
sources at depth_cases' per-entry bar, row 0 exact, everything finite, nothing written outside the padded buffers;
cost="terms" costs bit for bit against trajectory_cost_fn of the engine's own trajectory; cem_rollout_async bit for bit
against the explicit CEM sample; at S = 20 the fused cheetah cost at assert_costs_close's bar with conftest.envelope
and the record's index = argmin.

Kernels.  Depth nets: solo (hidden <= 512), group4, group8, split1, split2, split4, auto; relu / LayerNorm nets on the
split kernels only at hidden <= 512 (beyond, split precision has no relu / LayerNorm kernel off the team kernel).
Width nets: the same, and team and pp3 (kernel="auto" under BCMPC_SPLIT_PP=1) for the 2-layer tanh nets 2x15, 2x65,
2x257 and 2x513.

What the engine refuses, and why (create_refusal; any other refusal fails the case; each is asserted with its message
and the checks then run on kernel="auto", which answered every net of the list):
 * group8 at hidden <= 64 -- four hidden tiles do not split over eight waves ("group kernel does not fit this
   shape"): 4x64tanh, 8x64tanh, 8x64tanhLN, 3x17reluLN, 1x1tanh, 2x3tanhLN, 2x15tanh.
 * split4 at hidden <= 64 -- the split kernel runs two waves there and a group holds at most one 16-candidate column
   per wave ("split kernel does not fit this shape"): the same seven nets.
 * split4 at hidden > 512 -- 768: the 64-candidate hi + lo slab alone is 192 KiB; 1024: eight tiles per wave leave
   accumulators for two columns (x3_max_nc): 4x768tanh, 8x1024tanh, 2x513tanh (padded to 768), 2x769relu.
 * split4, LDS at hidden 512 -- slab 128 KiB, layer-0 slab 8 KiB, staged actions 1 KiB per action dim, and per layer
   2 KiB of biases: 8x512tanh fits at A = 3 (162,688 B) and not at A = 6 (165,760 B of 163,840).  With LayerNorm a
   further 4 KiB of exchange and 4 KiB per layer of gamma / beta: 4x500reluLN at either shape.
 * split2 at 8x1024tanh -- two columns' slab is 128 KiB and each layer's biases 4 KiB: L <= 5.
 * team at 2x513tanh -- hidden <= 512 ("team kernel"); pp3 does not take it either (hidden 512 only) and auto runs
   split1.  pp3 takes 2x257tanh (padded to 512); 2x15tanh and 2x65tanh run the team kernel under it.
 * CEM sampling on solo -- "CEM runs on group-kernel engines", as in the size sweep.

test_deepest_net_each_layout_takes pins where the host's LDS arithmetic stops each layout, at (20, 6):
    layout                  L_max   L_max + 1
    split2, 1024 tanh         5     6: "split kernel does not fit this shape"; auto runs split1
    split4, 512 tanh          7     8: the same; auto runs split1
    split4, 512 tanh + LN     1     2: the same; auto runs split1
    split2, 512 tanh + LN     8     (9 is beyond n_layers <= 8 for every kernel, auto included)
    group4, 1024 tanh         8     "
    group8, 1024 tanh         8     "
    solo, 512 tanh            8     "
(The bytes, of 163,840: split2 at 1024 needs 141,568 + 4,096 L; split4 at 512 149,376 + 2,048 L, with LayerNorm
153,472 + 6,144 L.)  The full case runs at L_max on all seven.  With LayerNorm it runs only where the CPU bar holds at
that L, else the layout is pinned by creation and finite, distinct launches of two sources; at this K and H the bar
holds for both (1x512tanhLN 0.352 of its cap, 8x512tanhLN 0.925), so both were compared and that fallback did not
run.  Where L_max + 1 <= 8 auto also runs a K = 16,384 engine of L_max + 1 layers -- wide enough that plan_engine
tries the refused group width first and must fall back to a narrower one (6x1024tanh: split1; 8x512tanh and
2x512tanhLN: split2) -- and its first K Philox candidates meet the same oracle states at the same bar.

Fused policy, reward net: test_gpu_state_action_sizes' policy_case and reward_case, their bars unchanged, at (20, 6).
Policies (layers x hidden) 1x1, 1x17, 3x128, 8x16, 8x128, 2x65 on the fp32 group kernel and split2; both are taken from
the device's own s_h, so the depth of the dynamics net does not compound.  kernel="team" takes a 2-layer policy at
this shape and K, refuses policy_layers = 3 (PL <= 2), and auto answers it (split1).  Reward widths 65, 129, 257 on group4 and split2.

Results of the run on one MI355X (profiles/depth_width_sweep.txt): every net ran on every listed kernel or met its
stated refusal, auto answered all of them, no case skipped; the largest |dstate| / bar is 0.50 (solo, 4x500reluLN at
(20, 6)), 8x1024tanh stays at 0.11 - 0.14.
"""
import numpy as np
import pytest

import depth_cases as dc
import size_cases as sc
from test_gpu_state_action_sizes import (Padded, a_gpu_fault_stops_the_run, check_states, launch, make_engine,
                                         policy_case, pp3_takes, reward_case, run_case)

pytestmark = pytest.mark.gpu

FIT = "split kernel does not fit this shape"
PP3_TAKES = "2x257tanh"                             # padded to hidden 512; 2x15, 2x65 (team) and 2x513 (768): not
SPLIT4_LDS = {("8x512tanh", 6), ("4x500reluLN", 6), ("4x500reluLN", 3)}         # (net, A): module docstring


def create_refusal(kernel, c):
    """The message of the stated refusal of bcmpc_create for (kernel, case), None where the engine must take it."""
    hp = dc.padded(c.hidden)
    if kernel == "team" and (c.L != 2 or hp > 512):
        return "team kernel"
    if kernel == "group8" and hp == 64:
        return "group kernel does not fit this shape"
    if kernel == "split4" and (hp == 64 or hp > 512 or (c.net, c.A) in SPLIT4_LDS):
        return FIT
    if kernel == "split2" and c.net == "8x1024tanh":
        return FIT
    return None


def depth_line(kernel, ran, c, worst):
    return f"[depth-case] kernel={kernel} ran={ran} net={c.net} S={c.S} A={c.A} worst={worst:.3f}"


def kernels_of(spec, width):
    hidden, L, act, ln = spec[:4]
    plain = act == "tanh" and not ln
    ks = (["solo"] if hidden <= 512 else []) + ["group4", "group8"]
    if plain or hidden <= 512:
        ks += ["split1", "split2", "split4"]
    if width and plain and L == 2:
        ks += ["team", "pp3"]
    return ks + ["auto"]


CASES = ([(k, sc.net_name(n), s) for n in dc.DEPTH_NETS for s in dc.DEPTH_SHAPES for k in kernels_of(n, False)] +
         [(k, sc.net_name(n), dc.WIDTH_SHAPE) for n in dc.WIDTH_NETS for k in kernels_of(n, True)])


@pytest.mark.parametrize("kernel,net,shape", CASES, ids=[f"{k}-{n}-S{s[0]}A{s[1]}" for k, n, s in CASES])
@a_gpu_fault_stops_the_run
def test_rollout_matches_oracle(kernel, net, shape, monkeypatch):
    if kernel == "pp3":                                 # (run_case asserts layout == rollout_pp3 exactly when pp3_takes)
        assert pp3_takes(dc.case(net, shape[0], shape[1])) == (net == PP3_TAKES), net
    run_case(kernel, dc.case(net, shape[0], shape[1]), monkeypatch, refusal=create_refusal, line=depth_line)


# ------------------------------------------------------------------ the deepest net each layout takes
#            kernel   hidden  ln     L_max (module docstring)
LAYOUTS = [("split2", 1024, False, 5), ("split4", 512, False, 7), ("split4", 512, True, 1), ("split2", 512, True, 8),
           ("group4", 1024, False, 8), ("group8", 1024, False, 8), ("solo", 512, False, 8)]
WIDE_K = 16384                                      # 1024 16-candidate columns: auto tries 64-candidate groups first


def try_create(kernel, hidden, L, ln, S, A, K=dc.K):
    """None where bcmpc_create takes the layout, else the refusal's text."""
    from bc_mpc_amd.engine import RolloutEngine
    try:
        RolloutEngine(S, A, hidden, L, "tanh", ln, dc.H, K, device=0, cost="none", kernel=kernel).close()
    except ValueError as e:
        return str(e)
    return None


@pytest.mark.parametrize("kernel,hidden,ln,want", LAYOUTS, ids=[f"{k}-{h}{'LN' if ln else ''}" for k, h, ln, _ in LAYOUTS])
@a_gpu_fault_stops_the_run
def test_deepest_net_each_layout_takes(kernel, hidden, ln, want, monkeypatch):
    """Module docstring: L_max found from L = 8 downward, the full case at L_max (LayerNorm: where the CPU bar holds,
    else creation and finite launches), L_max + 1 refused with the fit message while auto answers it."""
    monkeypatch.delenv("BCMPC_SPLIT_PP", raising=False)
    S, A = dc.DEPTH_SHAPES[0]
    refusals = {}
    L_max = 0
    for L in range(8, 0, -1):
        refusals[L] = try_create(kernel, hidden, L, ln, S, A)
        if refusals[L] is None:
            L_max = L
            break
    print(f"[depth-lmax] kernel={kernel} hidden={hidden} ln={int(ln)} S={S} A={A} L_max={L_max}")
    assert L_max == want, (L_max, refusals)
    assert all(FIT in msg for L, msg in refusals.items() if L > L_max), refusals
    spec = (hidden, L_max, "tanh", ln, 1000)
    if not ln or dc.bar_over_cap(spec, S, A) <= 1.0:
        run_case(kernel, dc.case(spec, S, A), monkeypatch, refusal=lambda k, c: None, line=depth_line)
    else:
        w = sc.weights(S, A, spec)
        from bc_mpc_amd.engine import MLPSpec, RolloutEngine
        c = dc.case((64, 2, "tanh", False, 1000), S, A)         # (inputs only: state, bounds, the three action sources)
        eng = RolloutEngine(S, A, hidden, L_max, "tanh", ln, dc.H, dc.K, device=0, cost="none", kernel=kernel)
        try:
            assert eng.info()["kernel"] == kernel, eng.info()
            eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta), c.norm, 1)
            eng.set_action_bounds(c.low, c.high)
            for src in ("explicit", "philox"):
                got, _, _ = launch(eng, c, src, explicit=src == "explicit")
                assert np.isfinite(got).all() and np.array_equal(got[0], np.tile(c.state, (dc.K, 1)))
                assert len(np.unique(got[-1], axis=0)) > dc.K // 2
            print(f"[depth-case] kernel={kernel} ran={eng.info()['kernel']} net={sc.net_name(spec)} S={S} A={A} "
                  f"worst=nan (finite launches only: the CPU bar is {dc.bar_over_cap(spec, S, A):.2f} of its cap)")
        finally:
            eng.close()
    if L_max == 8:
        assert "n_layers must be in [1, 8]" in try_create(kernel, hidden, 9, ln, S, A)
        assert "n_layers must be in [1, 8]" in try_create("auto", hidden, 9, ln, S, A)
        return
    # L_max + 1: refused above with the fit message; auto answers, at this K ...
    deeper = (hidden, L_max + 1, "tanh", ln, 1000)
    if ln and dc.bar_over_cap(deeper, S, A) > 1.0:
        assert try_create("auto", hidden, L_max + 1, ln, S, A) is None
        return
    c = dc.case(deeper, S, A)
    ran, _ = run_case("auto", c, monkeypatch, refusal=lambda k, c: None, line=depth_line)
    assert ran != kernel, ran
    # ... and at a K where it tries the refused width first: the first K Philox candidates are the same candidates
    wide = make_engine(c, "auto", "none", K=WIDE_K)
    try:
        info = wide.info()
        assert info["kernel"].startswith("split") and int(info["kernel"][5:]) < int(kernel[5:]), info
        import torch
        dev = torch.device("cuda", 0)
        traj = Padded((dc.H + 1) * WIDE_K * S, 3 * S)
        d_state = torch.from_numpy(np.array(c.state, dtype=np.float64)).to(dev)
        wide.rollout_async(d_state.data_ptr(), 0, None, sc.SEED, sc.OFF, None, traj.ptr, None,
                           torch.cuda.current_stream(dev).cuda_stream)
        got = traj.get("wide trajectory").reshape(dc.H + 1, WIDE_K, S)
        wide.check_status()
        assert np.isfinite(got).all()
        worst = check_states(c, "philox", np.ascontiguousarray(got[:, :dc.K]), f"auto K={WIDE_K} {c.net}")
        print(f"[depth-case] kernel=auto(K={WIDE_K}) ran={info['kernel']} net={c.net} S={S} A={A} worst={worst:.3f}")
    finally:
        wide.close()


# ------------------------------------------------------------------ fused policy depth and width
@pytest.mark.parametrize("kernel", ["fp32", "split2"])
@pytest.mark.parametrize("layers,hidden", dc.POLICIES, ids=lambda v: str(v))
@a_gpu_fault_stops_the_run
def test_policy_depth_and_width(layers, hidden, kernel):
    """test_policy_stochastic_mode_every_step's method and bars per policy (depth_cases.policy_gap: the f32 reference
    is within a sixth of the action bar of its f64 restatement for each)."""
    policy_case(dc.POLICY_SHAPE, kernel, layers, hidden, K=dc.K, H=dc.H)


@a_gpu_fault_stops_the_run
def test_policy_three_layers_team_refuses_auto_answers():
    """kernel="team" takes this shape and K with a 2-layer policy and refuses the same with three (PL <= 2)."""
    from bc_mpc_amd.engine import RolloutEngine
    S, A = dc.POLICY_SHAPE
    assert policy_case(dc.POLICY_SHAPE, "team", 2, 128, K=dc.K, H=dc.H) == "team"
    with pytest.raises(ValueError, match="team kernel"):
        RolloutEngine(S, A, 500, 2, "tanh", False, dc.H, dc.K, kernel="team", policy_hidden=128, policy_layers=3,
                      policy_mode="stochastic")
    ran = policy_case(dc.POLICY_SHAPE, "auto", 3, 128, K=dc.K, H=dc.H)
    print(f"[depth-policy] team refuses policy_layers = 3; auto ran {ran}")
    assert ran != "team"


# ------------------------------------------------------------------ reward net widths
@pytest.mark.parametrize("kernel", ["group4", "split2"])
@pytest.mark.parametrize("hidden", dc.REWARD_WIDTHS)
@a_gpu_fault_stops_the_run
def test_reward_net_widths(hidden, kernel):
    """reward_case's method and bar at widths one past a padding boundary (the trunk pads to 128 / 256 / 512)."""
    reward_case(dc.REWARD_SHAPE[0], dc.REWARD_SHAPE[1], False, kernel, hidden=hidden, K=dc.K, H=dc.H)

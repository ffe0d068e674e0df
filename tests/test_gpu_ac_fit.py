"""The device actor-critic fitter (csrc/ac_fit.hip, ``ac_fit.ActorCriticFitter``, ``MlpActorCritic``) against its
definition ``bc_mpc_amd.ac_fit.run``.

Gradient-resolving parity is tests/test_fit_oracle.py's regime as is (``HP``, ``_three_and_ragged``,
``parity_terms``, ``assert_parity``): set_params, three uniform batches (one captured graph), a snapshot, three
ragged batches [B, max(1, B - 5), B] (per-step launches), a snapshot; both snapshots and all six losses against the
definition's f64 trajectory within M = 32 times the definition's own f32-vs-f64 error plus 2 ulp.  M = 32 is the
project's number for this comparison on this step structure (tests/test_gpu_fit_grads.py) and stays below the cap 64.
Set BCMPC_ACFIT_PARITY_REPORT=<file> to write every case's ratio (how profiles/ac_fit_parity.txt was made).

The shapes are the edges of the kernels' tiling (csrc/ac_fit.hip):
* width: 16-column output tiles (7: one partial tile; 16 / 17: one full tile / a second partial one); the forward
  and backward GEMMs split K over idle waves up to 8 tiles (128) and give each wave whole tiles beyond (129); weights
  stream in chunks of 32 k with four chunks in flight, so K = 129 enters a second ring pass and 256 is the cap;
* depth: 1 (no hidden-to-hidden layer, no transposed copy read but the final one), 2, 4 (the cap);
* (S, A): (1, 1), (20, 6), (31, 16) -- the gather's row width and the weight tiles' bias row at k == S, which falls
  in the first tile (1, 20) or the second (31); the value head's single output column;
* batch: row blocks of 16 (1, 15, 16, 17, 33), the parameter kernel's four batch quarters (1: three empty quarters;
  77: unequal quarters; 128), and 520: a quarter longer than the 128 rows of one load batch.
"""
import functools
import os

import numpy as np
import pytest

from oracle import mpc_oracle as orc
from test_fit_oracle import HP, _three_and_ragged, assert_parity, parity_terms, worst_ratio

pytestmark = pytest.mark.gpu

M = 32
N_ROWS = 600
RATIOS = {}
REFERENCE_REGIME = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("BCMPC_ACFIT_PARITY_REPORT")
    if path and RATIOS:
        with open(path, "w") as fh:
            for k, v in RATIOS.items():
                fh.write(f"{v:10.4f}  {k}\n")
            fh.write(f"worst {max(RATIOS.values()):.4f} over {len(RATIOS)} cases; M = {M}\n")
            for k, v in REFERENCE_REGIME.items():
                fh.write(f"reference hyperparameters, {k}: {v}\n")


def problem(head, S, A, hidden, L, n=N_ROWS, seed=5):
    """The oracle's synthetic_policy weights, observations at 1.5 sigma of its filter, targets U(-1, 1) (policy) or
    3 N(0, 1) (value)."""
    out = A if head == "policy" else 1
    w = orc.synthetic_policy(S, out, hidden, L)
    rs = np.random.RandomState(seed)
    obs = w.ob_mean.astype(np.float64) + 1.5 * w.ob_std.astype(np.float64) * rs.standard_normal((n, S))
    tgt = rs.uniform(-1, 1, (n, out)) if head == "policy" else 3.0 * rs.standard_normal((n, 1))
    params = []
    for k, b in zip(w.kernels, w.biases):
        params += [k, b]
    return params, (w.ob_mean, w.ob_std), obs, tgt


def definition_runs(head, params, flt, obs, tgt, runs, dtype, hp=HP, lrs=None, filters=None):
    """(parameter snapshot after every run, losses [steps][1]) of ac_fit.run with carried Adam state; ``lrs`` /
    ``filters``: one learning rate / filter per run."""
    from bc_mpc_amd import ac_fit
    ps = [np.asarray(p, dtype) for p in params]
    st = ac_fit.AdamState.zeros_like(ps, hp["beta1"], hp["beta2"], dtype=dtype)
    snaps, losses = [], []
    for ri, batches in enumerate(runs):
        lr = hp["lr"] if lrs is None else lrs[ri]
        cur = flt if filters is None else filters[ri]
        losses += [[x] for x in ac_fit.run(ps, st, head, cur, obs, tgt, batches, lr, hp["beta1"], hp["beta2"],
                                           hp["eps"], dtype=dtype)]
        snaps.append([p.copy() for p in ps])
    return snaps, np.array(losses, np.float64)


def device_fitter(head, params, flt, obs, tgt, hp=HP, batch_size=128):
    from bc_mpc_amd.ac_fit import ActorCriticFitter
    S, hidden = params[0].shape
    f = ActorCriticFitter(head, S, params[-1].shape[0], hidden, len(params) // 2 - 1, batch_size=batch_size,
                          beta1=hp["beta1"], beta2=hp["beta2"], epsilon=hp["eps"])
    f.set_params(params[0::2], params[1::2])
    f.set_filter(*flt)
    f.set_data(obs, tgt)
    return f


def flat(f):
    ks, bs = f.get_params()
    out = []
    for k, b in zip(ks, bs):
        out += [k, b]
    return out


def device_runs(f, runs, lr=HP["lr"], lrs=None):
    snaps, losses, graphs = [], [], []
    for ri, batches in enumerate(runs):
        losses += [[x] for x in f.run(batches, lr if lrs is None else lrs[ri])]
        graphs.append(f.graph_captures)
        snaps.append(flat(f))
    return (snaps, np.array(losses, np.float64)), graphs


@functools.lru_cache(maxsize=None)
def _case(head, S, A, hidden, L, B):
    """The problem, its two runs and the definition's f64 / f32 trajectories (computed once, read-only)."""
    params, flt, obs, tgt = problem(head, S, A, hidden, L)
    runs = _three_and_ragged(N_ROWS, B)
    ref64 = definition_runs(head, params, flt, obs, tgt, runs, np.float64)
    ref32 = definition_runs(head, params, flt, obs, tgt, runs, np.float32)
    return params, flt, obs, tgt, runs, ref64, ref32


WIDTHS = [(head, 20, 6, h, 2, 33) for head in ("policy", "value") for h in (7, 16, 17, 128, 129, 256)]
DEPTHS = [(head, 20, 6, 64, L, 33) for head in ("policy", "value") for L in (1, 2, 4)]
DIMS = [("policy", 1, 1, 64, 2, 33), ("policy", 20, 6, 64, 2, 33), ("policy", 31, 16, 64, 2, 33),
        ("value", 1, 1, 64, 2, 33), ("value", 31, 1, 64, 2, 33)]
BATCHES = [(head, 20, 6, 64, 2, B) for head in ("policy", "value") for B in (1, 15, 16, 17, 33, 77, 128)]
BATCHES.append(("policy", 20, 6, 64, 2, 520))
CASES = list(dict.fromkeys(WIDTHS + DEPTHS + DIMS + BATCHES))


@pytest.mark.parametrize("head,S,A,hidden,L,B", CASES)
def test_gradient_resolving_parity(head, S, A, hidden, L, B):
    params, flt, obs, tgt, runs, ref64, ref32 = _case(head, S, A, hidden, L, B)
    f = device_fitter(head, params, flt, obs, tgt)
    got, graphs = device_runs(f, runs)
    f.close()
    # uniform: the graph; ragged: launches (at B = 1 the second run is [1, 1, 1]: the same graph again)
    assert graphs[0] == 1 and graphs[1] == (1 if B == 1 else 0)
    terms = parity_terms(got, ref64, ref32, [3, 3])
    tag = f"{head} S{S} A{A} {hidden}x{L} B{B}"
    ratio = worst_ratio(terms)
    RATIOS[tag] = ratio
    print(f"[{tag}] worst ratio {ratio:.3g}; losses {got[1][:, 0]}")
    assert np.isfinite(got[1]).all() and ref64[1].min() > 1e-3      # far from the sqrt's singularity
    assert_parity(terms, M, tag)


@pytest.mark.parametrize("head", ["policy", "value"])
def test_reference_hyperparameters(head):
    """Adam 0.9 / 0.999 / 1e-8, lr 1e-3, B = 128, twenty steps, 20 -> 128 -> 128 -> 6 (-> 1): tests/test_gpu_fit.py's
    bars for this regime -- losses within rtol 1e-4 of the definition's f32 losses, parameters within one flipped
    Adam step (max |dw| <= 2.5 lr) with the median <= 1e-6."""
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    params, flt, obs, tgt = problem(head, 20, 6, 128, 2)
    rs = np.random.RandomState(3)
    runs = [[rs.choice(N_ROWS, 128, replace=False) for _ in range(20)]]
    want = definition_runs(head, params, flt, obs, tgt, runs, np.float32, hp)
    f = device_fitter(head, params, flt, obs, tgt, hp)
    got, _ = device_runs(f, runs, lr=hp["lr"])
    f.close()
    rel = float(np.max(np.abs(got[1] - want[1]) / want[1]))
    d = np.concatenate([np.abs(a - b).ravel() for a, b in zip(got[0][0], want[0][0])])
    REFERENCE_REGIME[head] = f"worst loss rel {rel:.3e}, params max |dw| {d.max():.3e} median {np.median(d):.3e}"
    print(f"[{head}] {REFERENCE_REGIME[head]}")
    assert np.allclose(got[1], want[1], rtol=1e-4, atol=0)
    assert d.max() <= 2.5 * hp["lr"] and np.median(d) <= 1e-6


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("head", ["policy", "value"])
def test_graph_and_launch_paths_and_two_fitters_agree_bitwise(head, monkeypatch):
    params, flt, obs, tgt, runs, _r64, _r32 = _case(head, 20, 6, 64, 2, 33)
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("BCMPC_ACFIT_GRAPH", graph)
        f = device_fitter(head, params, flt, obs, tgt)
        got, graphs = device_runs(f, runs)
        f.close()
        assert graphs == ([1, 0] if graph == "1" else [0, 0])
        out.append(got)
    snaps0, losses0 = out[0]
    for snaps, losses in out[1:]:
        assert losses.tobytes() == losses0.tobytes()
        assert _same(snaps[0], snaps0[0]) and _same(snaps[1], snaps0[1])


@pytest.mark.parametrize("head", ["policy", "value"])
def test_stale_graph_and_learning_rates(head):
    """What a captured graph holds must not outlive a change: a run after set_data grew the buffer (new addresses)
    and a run after set_filter changed (new contents at the same address) equal the definition; three runs at three
    learning rates replay one graph (the rate is read from device memory).  "Equal" is the parity bound above."""
    params, flt, obs, tgt = problem(head, 20, 6, 64, 2, n=2 * N_ROWS)
    rs = np.random.RandomState(12)
    small = [rs.choice(N_ROWS, 33, replace=False) for _ in range(3)]
    grown = [rs.choice(2 * N_ROWS, 33, replace=False) for _ in range(3)]
    flt2 = (flt[0] + np.float32(0.25), flt[1] * np.float32(1.5))
    runs = [small, small, small, grown, grown]
    lrs = [0.25, 0.125, 0.0625, 0.25, 0.25]
    filters = [flt, flt, flt, flt, flt2]
    ref64 = definition_runs(head, params, flt, obs, tgt, runs, np.float64, lrs=lrs, filters=filters)
    ref32 = definition_runs(head, params, flt, obs, tgt, runs, np.float32, lrs=lrs, filters=filters)
    f = device_fitter(head, params, flt, obs[:N_ROWS], tgt[:N_ROWS])
    snaps, losses, graphs = [], [], []
    for step, (batches, lr) in enumerate(zip(runs, lrs)):
        if step == 3:
            f.set_data(obs, tgt)
        if step == 4:
            f.set_filter(*flt2)
        losses += [[x] for x in f.run(batches, lr)]
        graphs.append(f.graph_captures)
        snaps.append(flat(f))
    f.close()
    assert graphs == [1, 1, 1, 2, 2], graphs           # no recapture per rate or filter; one for the moved buffers
    terms = parity_terms((snaps, np.array(losses, np.float64)), ref64, ref32, [3] * 5)
    print(f"[{head}] stale-graph sequence: worst ratio {worst_ratio(terms):.3g}")
    assert_parity(terms, M, f"{head} stale-graph sequence")
    # the changes matter: the definition without them is far outside the bound
    stale = definition_runs(head, params, flt, obs, tgt, runs, np.float32, lrs=[0.25] * 5)
    assert worst_ratio(parity_terms(stale, ref64, ref32, [3] * 5)) > 64


class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n), np.ones(n)


class _AcEnv:
    observation_space, action_space = _Space(20), _Space(6)


def _container(seed=3):
    from bc_mpc_amd import MlpActorCritic
    ac = MlpActorCritic(_AcEnv(), 128, 2, seed=seed)
    w = orc.synthetic_policy(20, 6, 128, 2)
    rs = np.random.RandomState(8)
    obs = w.ob_mean.astype(np.float64) + 1.5 * w.ob_std.astype(np.float64) * rs.standard_normal((300, 20))
    ac.ob_rms.update(obs)
    return ac, obs, rs.uniform(-1, 1, (300, 6)), 3.0 * rs.standard_normal(300)


def test_container_fits_equal_the_definition_and_isolate_the_heads():
    import random
    from bc_mpc_amd import ac_fit
    from bc_mpc_amd.fit import sample_batches
    ac, obs, acs, rets = _container()
    w0 = ac.get_weights()
    v0 = ac.version
    random.seed(5)
    losses = ac.fit_bc((obs, acs), 4, 64, 1e-3)
    assert ac.version == v0 + 1 and losses.dtype == np.float32 and losses.shape == (4,)
    assert _same(ac.vf_kernels + ac.vf_biases + [ac.logstd], w0["vf"][0] + w0["vf"][1] + [w0["logstd"]])
    assert not _same(ac.pol_kernels, w0["pol"][0])
    random.seed(5)
    batches = sample_batches(300, 64, 4)
    ps = []
    for k, b in zip(*w0["pol"]):
        ps += [k, b]
    st = ac_fit.AdamState.zeros_like(ps)
    want = ac_fit.run(ps, st, "policy", (ac.ob_rms.mean, ac.ob_rms.std), obs, acs, batches, 1e-3)
    assert np.allclose(losses, want, rtol=1e-4, atol=0)
    w1 = ac.get_weights()
    lv = ac.fit_value(obs, rets, 3, 50, 1e-3, rng=random.Random(2))
    assert _same(ac.pol_kernels + ac.pol_biases + [ac.logstd], w1["pol"][0] + w1["pol"][1] + [w1["logstd"]])
    assert not _same(ac.vf_kernels, w1["vf"][0])
    pv = []
    for k, b in zip(*w1["vf"]):
        pv += [k, b]
    wantv = ac_fit.run(pv, ac_fit.AdamState.zeros_like(pv), "value", (ac.ob_rms.mean, ac.ob_rms.std), obs,
                       rets[:, None], sample_batches(300, 50, 3, random.Random(2)), 1e-3)
    assert np.allclose(lv, wantv, rtol=1e-4, atol=0)
    # a filter update between two fits reaches the next fit's inputs; the Adam state carries on (second run)
    ac.ob_rms.update(obs[:40] * 3.0)
    l2 = ac.update_bc(obs[:32], acs[:32], 1e-3)
    want2 = ac_fit.run(ps, st, "policy", (ac.ob_rms.mean, ac.ob_rms.std), obs[:32], acs[:32], [np.arange(32)], 1e-3)
    assert np.allclose(l2, want2, rtol=1e-4, atol=0)
    ac.close()


def test_zero_loss_gives_nan_parameters_as_the_definition_does():
    from bc_mpc_amd import ac_fit
    ac, obs, _acs, _rets = _container()
    w = ac.get_weights()
    w["pol"] = (w["pol"][0][:-1] + [np.zeros_like(w["pol"][0][-1])], w["pol"][1])
    ac.set_weights(w)
    loss = ac.update_bc(obs[:16], np.zeros((16, 6)), 1e-3)
    assert loss[0] == 0.0
    assert all(np.isnan(k).all() for k in ac.pol_kernels) and all(np.isnan(b).all() for b in ac.pol_biases)
    ps = []
    for k, b in zip(*w["pol"]):
        ps += [k, b]
    want = ac_fit.run(ps, ac_fit.AdamState.zeros_like(ps), "policy", (ac.ob_rms.mean, ac.ob_rms.std), obs[:16],
                      np.zeros((16, 6)), [np.arange(16)], 1e-3)
    assert want[0] == 0.0 and all(np.isnan(p).all() for p in ps)
    assert not any(np.isnan(k).any() for k in ac.vf_kernels)
    ac.close()


def _engines(ctrl):
    found = [ctrl._engine] + [e for _key, e in getattr(ctrl, "_engines", {}).values()]
    return [e for e in found if e is not None]


def test_through_the_controllers():
    """CEMcontroller(policy_prior=ac, terminal_value=ac) at K = 64, H = 3: after fit_bc, fit_value and ob_rms.update
    the next call's proposal costs (closed-loop policy rollouts scored with the terminal value) are, bit for bit,
    those of a fresh controller over a copy of the container's weights, and not those of a copy of the weights
    before the change.  An untouched container uploads nothing: the engines keep the very records they hold."""
    import random
    from bc_mpc_amd import CEMcontroller, MlpActorCritic, MPCcontrollerPolicyNet, MPPIcontroller, cheetah_cost_fn
    from test_gpu_plan_batch import net
    n = net("reluln128")
    ac, obs, acs, rets = _container()
    common = dict(horizon=3, cost_fn=cheetah_cost_fn, num_simulated_paths=64, iterations=2, seed=4, warm_start=False,
                  policy_paths=8)

    def controller(container):
        return CEMcontroller(_AcEnv(), n.dyn, n_elite=6, policy_prior=container, terminal_value=container, **common)

    def costs_over(weights, seed_state):
        copy = MlpActorCritic(_AcEnv(), 128, 2, seed=99)
        copy.set_weights(weights)
        c = controller(copy)
        c._seed_rng.set_state(seed_state)
        c.get_action(n.states[0])
        return c.last_proposal_costs.copy()

    ctrl = controller(ac)
    a = ctrl.get_action(n.states[0])
    assert a.shape == (6,) and np.isfinite(a).all() and ctrl.last_proposal_costs.shape == (8,)
    for change in (lambda: ac.fit_bc((obs, acs), 3, 64, 1e-2, rng=random.Random(1)),
                   lambda: ac.fit_value(obs, rets, 3, 64, 1e-2, rng=random.Random(1)),
                   lambda: ac.ob_rms.update(obs[:50] * 2.0)):
        before, v = ac.get_weights(), ac.version
        change()
        assert ac.version == v + 1
        state = ctrl._seed_rng.get_state()
        ctrl.get_action(n.states[0])
        got = ctrl.last_proposal_costs.copy()
        assert got.tobytes() == costs_over(ac.get_weights(), state).tobytes()
        assert got.tobytes() != costs_over(before, state).tobytes()
    held = [(e, e._pol, e._value) for e in _engines(ctrl)]
    assert any(p is not None for _e, p, _v in held) and any(v is not None for _e, _p, v in held)
    v = ac.version
    ctrl.get_action(n.states[0])
    assert ac.version == v
    for e, p, val in held:
        assert e._pol is p and e._value is val
        assert p is None or p[0] == v
        assert val is None or val[0] == v
    mppi = MPPIcontroller(_AcEnv(), n.dyn, policy_prior=ac, terminal_value=ac, **common)
    assert np.isfinite(mppi.get_action(n.states[0])).all()
    pn = MPCcontrollerPolicyNet(_AcEnv(), n.dyn, ac, explore=0.1, horizon=3, cost_fn=cheetah_cost_fn,
                                num_simulated_paths=64)
    assert np.isfinite(pn.get_action(n.states[0])).all()
    ac.close()

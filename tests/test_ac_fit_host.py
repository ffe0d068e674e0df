"""CPU checks of the actor-critic fitting definition (bc_mpc_amd/ac_fit.py), of the container
(bc_mpc_amd/actor_critic.py) and of the device fitter's refusals (csrc/ac_fit_plan.cpp, no GPU needed); then
tests/test_fit_oracle.py's gradient-resolving regime applied to the definition's own f32 trajectory, broken the
ways a wrong kernel would break it: the check that tests/test_gpu_ac_fit.py's bound rejects wrong gradients."""
import random
import types
from collections import deque

import numpy as np
import pytest

from bc_mpc_amd import ac_fit
from oracle import mpc_oracle as orc
from test_fit_oracle import HP, M_CAP, _three_and_ragged, assert_parity, parity_terms, worst_ratio


def _problem(head, S, A, hidden, L, n=600, seed=5):
    """The oracle's synthetic_policy weights, observations at 1.5 sigma of its filter, targets U(-1, 1) (policy) or
    3 N(0, 1) (value): tests/test_gpu_ac_fit.py's problem."""
    out = A if head == "policy" else 1
    w = orc.synthetic_policy(S, out, hidden, L)
    rs = np.random.RandomState(seed)
    obs = w.ob_mean.astype(np.float64) + 1.5 * w.ob_std.astype(np.float64) * rs.standard_normal((n, S))
    tgt = rs.uniform(-1, 1, (n, out)) if head == "policy" else 3.0 * rs.standard_normal((n, 1))
    params = []
    for k, b in zip(w.kernels, w.biases):
        params += [k, b]
    return params, (w.ob_mean, w.ob_std), obs, tgt


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("head", ["policy", "value"])
def test_grads_match_finite_differences(head):
    params, flt, obs, tgt = _problem(head, 5, 3, 12, 2, n=7)
    ps = [p.astype(np.float64) for p in params]
    obz, t = ac_fit.batch(flt, obs, tgt, np.arange(7), np.float64)
    _, g = ac_fit.grads(ps, head, obz, t, np.float64)
    worst = 0.0
    for pi in range(len(ps)):
        for k in range(0, ps[pi].size, max(1, ps[pi].size // 7)):
            e = 1e-6
            p2 = [q.copy() for q in ps]
            p2[pi].flat[k] += e
            lp, _ = ac_fit.grads(p2, head, obz, t, np.float64)
            p2[pi].flat[k] -= 2 * e
            lm, _ = ac_fit.grads(p2, head, obz, t, np.float64)
            num = (lp - lm) / (2 * e)
            worst = max(worst, abs(num - g[pi].flat[k]) / (abs(num) + 1e-5))
    assert worst < 1e-4, worst


@pytest.mark.parametrize("head", ["policy", "value"])
def test_grads_are_the_oracles_by_the_chain_rule(head):
    """A restatement independent of the module: oracle.fit_grads is the gradient of mean((t - p)^2) over the same
    net (LayerNorm off, tanh); d sqrt(m) = dm / (2 sqrt(m)) for the policy head, dm itself for the value head."""
    params, flt, obs, tgt = _problem(head, 20, 6, 33, 2, n=19)
    ps = [p.astype(np.float64) for p in params]
    obz, t = ac_fit.batch(flt, obs, tgt, np.arange(19), np.float64)
    loss, g = ac_fit.grads(ps, head, obz, t, np.float64)
    l_mse, g_mse = orc.fit_grads(ps, 2, "tanh", False, obz, t, dtype=np.float64)
    if head == "policy":
        assert abs(loss - np.sqrt(l_mse)) <= 4 * np.spacing(loss)
        want = [x / (2.0 * np.sqrt(l_mse)) for x in g_mse]
    else:
        assert abs(loss - l_mse) <= 4 * np.spacing(loss)
        want = g_mse
    for a, b in zip(g, want):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-13 * max(1.0, np.max(np.abs(b)))


def test_observe_is_value_observe():
    from bc_mpc_amd import value
    w = orc.synthetic_policy(20, 1, 16, 2)
    spec = value.ValueSpec(w.kernels, w.biases, w.ob_mean, w.ob_std)
    rs = np.random.RandomState(2)
    ob = np.concatenate([20.0 * rs.standard_normal((50, 20)), np.full((1, 20), 1e300)])
    assert ac_fit.observe(spec, ob).tobytes() == value.observe(spec, ob).tobytes()
    assert ac_fit.observe((w.ob_mean, w.ob_std), ob).tobytes() == value.observe(spec, ob).tobytes()


def test_adam_first_step_matches_closed_form():
    """tests/test_fit_oracle.py's closed form: w' ~ w - lr sign(g); the powers advance once."""
    p = [np.array([1.0, -2.0, 0.5], np.float32)]
    g = [np.array([0.3, -4.0, 1e-3], np.float32)]
    st = ac_fit.AdamState.zeros_like(p)
    ac_fit.adam_apply(p, g, st, 1e-3)
    assert np.allclose(p[0], [1.0 - 1e-3, -2.0 + 1e-3, 0.5 - 1e-3], atol=2e-6)
    assert st.beta1_power == np.float32(0.9) * np.float32(0.9)
    po, so = [np.array([1.0, -2.0, 0.5], np.float32)], orc.AdamState.zeros_like(p)
    orc.adam_apply(po, g, so, 1e-3)
    assert po[0].tobytes() == p[0].tobytes() and so.beta2_power == st.beta2_power


def test_zero_loss_is_nan_and_the_learning_rate_is_per_run():
    params, flt, obs, _ = _problem("policy", 4, 2, 5, 1, n=6)
    params[-2][:] = 0
    params[-1][:] = 0
    ps = [p.copy() for p in params]
    st = ac_fit.AdamState.zeros_like(ps)
    losses = ac_fit.run(ps, st, "policy", flt, obs, np.zeros((6, 2)), [np.arange(6)], 1e-3)
    assert losses[0] == 0.0 and all(np.isnan(p).all() for p in ps)
    params, flt, obs, tgt = _problem("value", 4, 2, 5, 1, n=6)
    a, b = [p.copy() for p in params], [p.copy() for p in params]
    sa, sb = ac_fit.AdamState.zeros_like(a), ac_fit.AdamState.zeros_like(b)
    batches = [np.arange(6), np.arange(5)]
    la = ac_fit.run(a, sa, "value", flt, obs, tgt, batches, [0.25, 0.125], **{k: HP[k] for k in ("beta1", "beta2", "eps")})
    lb = ac_fit.run(b, sb, "value", flt, obs, tgt, batches[:1], 0.25, **{k: HP[k] for k in ("beta1", "beta2", "eps")})
    lb += ac_fit.run(b, sb, "value", flt, obs, tgt, batches[1:], 0.125, **{k: HP[k] for k in ("beta1", "beta2", "eps")})
    assert la == lb and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_limits():
    for bad in [("policy", 20, 6, 257, 2), ("policy", 20, 6, 0, 2), ("policy", 20, 6, 64, 5), ("policy", 20, 6, 64, 0),
                ("policy", 33, 6, 64, 2), ("policy", 20, 17, 64, 2), ("value", 20, 2, 64, 2), ("both", 20, 6, 64, 2)]:
        with pytest.raises(ValueError):
            ac_fit.check_shape(*bad)
    ac_fit.check_shape("policy", 32, 16, 256, 4)
    ac_fit.check_shape("value", 1, 1, 1, 1)
    with pytest.raises(ValueError):
        ac_fit.check_params("policy", [np.zeros((3, 4), np.float32), np.zeros(4, np.float32),
                                       np.zeros((5, 2), np.float32), np.zeros(2, np.float32)])


# ------------------------------------------------------------------ the bound bites
def _row_gradient(ps, head, obz, t, loss, r):
    """Row r's term of the batch sums.  The mean-squared-error gradient of that row alone is d(sum of its squared
    residuals) / out; the whole batch's gradient weighs that sum by (0.5 / loss) / (B out) (policy) or 1 / (B out)
    (value)."""
    f32 = np.float32
    B = t.shape[0]
    _, g1 = ac_fit.grads(ps, "value", obz[r:r + 1], t[r:r + 1], np.float32)
    scale = f32(0.5) / (loss * f32(B)) if head == "policy" else f32(1.0) / f32(B)
    return [(x * scale).astype(f32) for x in g1]


def _trajectory(head, params, flt, obs, tgt, runs, dtype, kind="none"):
    """ac_fit.run's loop with carried Adam state over ``runs``, the f32 gradients broken as ``kind`` says."""
    f32 = np.float32
    ps = [np.asarray(p, dtype) for p in params]
    st = ac_fit.AdamState.zeros_like(ps, HP["beta1"], HP["beta2"], dtype=dtype)
    snaps, losses, saved = [], [], None
    for ri, batches in enumerate(runs):
        for si, idx in enumerate(batches):
            obz, t = ac_fit.batch(flt, obs, tgt, idx, dtype)
            if kind == "beta_powers":                     # the powers not carried between two runs
                if (ri, si) == (0, 0):
                    saved = (st.beta1_power, st.beta2_power)
                if (ri, si) == (1, 0):
                    st.beta1_power, st.beta2_power = saved
            loss, g = ac_fit.grads(ps, head, obz, t, dtype)
            if kind == "last_row":                        # the last batch row left out of every sum
                g1 = _row_gradient(ps, head, obz, t, loss, len(idx) - 1)
                g = [(a - b).astype(f32) for a, b in zip(g, g1)]
            if kind == "column":                          # one dW column halved
                g[2] = g[2].copy()
                g[2][:, -1] *= f32(0.5)
            if kind == "scalar":                          # the policy head's 1 / (2 loss) omitted
                g = [(x * (f32(2.0) * loss)).astype(f32) for x in g]
            ac_fit.adam_apply(ps, g, st, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], dtype)
            losses.append([loss])
        snaps.append([p.copy() for p in ps])
    return snaps, np.array(losses, np.float64)


BITE_CASES = [("policy", 33, 2, 33), ("policy", 130, 2, 33), ("policy", 7, 1, 5), ("policy", 256, 4, 128),
              ("value", 33, 2, 33), ("value", 256, 4, 128)]


@pytest.mark.parametrize("head,hidden,L,B", BITE_CASES)
def test_parity_bound_bites(head, hidden, L, B):
    """The bound of tests/test_gpu_ac_fit.py at the cap M = 64 rejects every mutated f32 trajectory by a wide
    margin and accepts the unmutated one at M = 1; the policy loss stays far from the sqrt's singularity."""
    n = 600
    params, flt, obs, tgt = _problem(head, 20, 6, hidden, L, n)
    runs = _three_and_ragged(n, B)
    ref64 = _trajectory(head, params, flt, obs, tgt, runs, np.float64)
    ref32 = _trajectory(head, params, flt, obs, tgt, runs, np.float32)
    # the loop above is ac_fit.run's
    ps = [p.copy() for p in params]
    st = ac_fit.AdamState.zeros_like(ps, HP["beta1"], HP["beta2"])
    direct = []
    for batches in runs:
        direct += ac_fit.run(ps, st, head, flt, obs, tgt, batches, **HP)
    assert np.array_equal(np.array(direct, np.float64), ref32[1][:, 0])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ps, ref32[0][1]))
    assert all(p.dtype == np.float64 for p in ref64[0][1])
    if head == "policy":
        assert 0.02 < ref64[1].min() and ref64[1].max() < 2.0
    terms = parity_terms(ref32, ref64, ref32, [3, 3])
    assert worst_ratio(terms) <= 1.0
    assert_parity(terms, 1)
    kinds = ["last_row", "column", "beta_powers"] + (["scalar"] if head == "policy" else [])
    for kind in kinds:
        got = _trajectory(head, params, flt, obs, tgt, runs, np.float32, kind)
        terms = parity_terms(got, ref64, ref32, [3, 3])
        ratio = worst_ratio(terms)
        print(f"[{head} {hidden}x{L} B{B} {kind}] worst ratio {ratio:.3g}")
        assert ratio > 100 * M_CAP, (kind, ratio)
        with pytest.raises(AssertionError):
            assert_parity(terms, M_CAP)


# ------------------------------------------------------------------ the container
class _Space:
    def __init__(self, n):
        self.shape = (n,)


class _Env:
    observation_space, action_space = _Space(20), _Space(6)


def _ac(**kw):
    from bc_mpc_amd import MlpActorCritic
    return MlpActorCritic(_Env(), **kw)


def test_container_initialisation():
    ac = _ac(hid_size=48, num_hid_layers=3, seed=7)
    assert [k.shape for k in ac.pol_kernels] == [(20, 48), (48, 48), (48, 48), (48, 6)]
    assert [k.shape for k in ac.vf_kernels] == [(20, 48), (48, 48), (48, 48), (48, 1)]
    for ks, final in ((ac.pol_kernels, 0.01), (ac.vf_kernels, 1.0)):
        for i, k in enumerate(ks):
            assert k.dtype == np.float32
            assert np.allclose(np.sqrt(np.square(k.astype(np.float64)).sum(axis=0)), final if i == 3 else 1.0, rtol=1e-6)
    assert all((b == 0).all() and b.dtype == np.float32 for b in ac.pol_biases + ac.vf_biases)
    assert ac.logstd.shape == (6,) and (ac.logstd == 0).all()
    assert (ac.ob_rms.sum == 0).all() and (ac.ob_rms.sumsq == 1e-2).all() and ac.ob_rms.count == 1e-2
    same, other = _ac(hid_size=48, num_hid_layers=3, seed=7), _ac(hid_size=48, num_hid_layers=3, seed=8)
    assert same.pol_kernels[0].tobytes() == ac.pol_kernels[0].tobytes() != other.pol_kernels[0].tobytes()
    for bad in (dict(hid_size=257), dict(num_hid_layers=5), dict(hid_size=0)):
        with pytest.raises(ValueError):
            _ac(**bad)


def test_filter_formulas_are_the_tf_readers():
    """ob_rms.mean / .std against policy._tf_policy reading the same sums through a stand-in session."""
    from bc_mpc_amd import policy as bpol
    ac = _ac(hid_size=16, seed=1)
    rs = np.random.RandomState(4)
    ac.ob_rms.update(3.0 * rs.standard_normal((37, 20)) + 1.0)
    ac.ob_rms.update(rs.standard_normal(20))
    assert ac.ob_rms.count == 38.01
    p = "pi/pi"
    vals = {f"{p}/obfilter/runningsum:0": ac.ob_rms.sum, f"{p}/obfilter/runningsumsq:0": ac.ob_rms.sumsq,
            f"{p}/obfilter/count:0": np.float64(ac.ob_rms.count), f"{p}/pol/logstd:0": ac.logstd[None]}
    for i, (k, b) in enumerate(zip(ac.pol_kernels, ac.pol_biases)):
        name = "final" if i == 2 else f"fc{i + 1}"
        vals[f"{p}/pol/{name}/kernel:0"], vals[f"{p}/pol/{name}/bias:0"] = k, b
    tf = types.SimpleNamespace(global_variables=lambda: [types.SimpleNamespace(name=n) for n in vals])
    sess = types.SimpleNamespace(run=lambda fetches: [vals[v.name] for v in fetches])
    spec = bpol._tf_policy(types.SimpleNamespace(sess=sess, pi_scope="pi", num_hid_layers=2), tf=tf)
    assert spec.ob_mean.tobytes() == ac.ob_rms.mean.tobytes() and spec.ob_std.tobytes() == ac.ob_rms.std.tobytes()
    assert ac.ob_rms.mean.dtype == ac.ob_rms.std.dtype == np.float32


def test_extract_round_trip_and_version():
    from bc_mpc_amd import policy as bpol
    from bc_mpc_amd import value as bval
    ac = _ac(seed=2)
    ac.ob_rms.update(np.random.RandomState(0).standard_normal((10, 20)))
    assert ac.version == 1
    pspec, pv = bpol.extract(ac)
    vspec, vv = bval.extract(ac)
    assert pv == vv == 1 == bpol.int_version(ac)                      # the integer is trusted: no digest
    assert all(a.tobytes() == b.tobytes() for a, b in zip(pspec.kernels + pspec.biases, ac.pol_kernels + ac.pol_biases))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(list(vspec.kernels) + list(vspec.biases),
                                                         ac.vf_kernels + ac.vf_biases))
    assert pspec.ob_mean.tobytes() == vspec.ob_mean.tobytes() == ac.ob_rms.mean.tobytes()
    assert pspec.logstd.tobytes() == ac.logstd.tobytes()
    # reading, acting and extracting mutate nothing
    ac.act(np.zeros(20), stochastic=False)
    ac.act(np.zeros((3, 20)), rng=np.random.RandomState(1))
    ac.policy_spec(), ac.value_spec(), ac.get_weights()
    assert ac.version == 1
    w = ac.get_weights()
    w["logstd"] = w["logstd"] - 0.5
    ac.set_weights(w)
    assert ac.version == 2 and (ac.logstd == -0.5).all()
    ac.set_weights({"pol": w["pol"]})
    assert ac.version == 3
    ac.ob_rms.update(np.ones(20))
    assert ac.version == 4
    other = _ac(seed=3)
    other.set_weights(ac.get_weights())
    assert bpol.extract(other)[0].kernels[0].tobytes() == ac.pol_kernels[0].tobytes()
    assert other.ob_rms.mean.tobytes() == ac.ob_rms.mean.tobytes()
    with pytest.raises(ValueError):
        ac.set_weights({"pol": (w["pol"][0][:-1], w["pol"][1])})
    with pytest.raises(ValueError):
        ac.set_weights({"vf": ([np.full_like(k, np.nan) for k in w["vf"][0]], w["vf"][1])})
    assert ac.version == 4


def test_act_is_the_definitions():
    from bc_mpc_amd import value as bval
    ac = _ac(seed=5)
    rs = np.random.RandomState(6)
    ac.ob_rms.update(2.0 * rs.standard_normal((64, 20)))
    w = ac.get_weights()
    w["pol"] = ([k * np.float32(30.0) if i == 2 else k for i, k in enumerate(w["pol"][0])],
                [np.float32(0.1) * rs.standard_normal(b.shape).astype(np.float32) for b in w["pol"][1]])
    w["logstd"] = np.linspace(-1, 0, 6).astype(np.float32)
    ac.set_weights(w)
    ob = 3.0 * rs.standard_normal((9, 20))
    mean, vpred = ac.act(ob, stochastic=False)
    pol = orc.NumpyPolicy(orc.PolicyWeights(ac.pol_kernels, ac.pol_biases, ac.ob_rms.mean, ac.ob_rms.std, ac.logstd))
    assert mean.dtype == np.float32 and mean.tobytes() == pol.mean(ob).tobytes()
    assert vpred.tobytes() == bval.terminal_values(ac.value_spec(), ob).tobytes()
    one, v1 = ac.act(ob[0], stochastic=False)
    assert one.shape == (1, 6) and v1.shape == (1,) and np.allclose(one[0], mean[0], atol=1e-6)
    noisy, _ = ac.act(ob, stochastic=True, rng=np.random.RandomState(3))
    z = np.random.RandomState(3).standard_normal((9, 6)).astype(np.float32)
    assert noisy.tobytes() == (mean + np.exp(ac.logstd) * z).astype(np.float32).tobytes()


def test_fit_bc_draws_the_rows_of_databuffer_sample(monkeypatch):
    """DataBufferGeneral.sample = random.sample(deque, min(size, num)) on Python's global stream."""
    ac = _ac(hid_size=8, seed=1)
    items = deque([[np.full(20, float(i)), np.full(6, i / 50.0)] for i in range(50)])
    seen = {}

    def run(head, obs, targets, batches, lr):
        seen.update(head=head, rows=[[int(obs[i, 0]) for i in b] for b in batches], lr=lr, targets=targets)
        return np.zeros(len(batches), np.float32)
    monkeypatch.setattr(ac, "_run", run)
    for size, num in [(50, 16), (50, 64)]:
        random.seed(123)
        ref = []
        for _ in range(4):                       # data_buffer.py:45-52
            picked = random.sample(items, size) if size < num else random.sample(items, num)
            ref.append([int(b[0][0]) for b in picked])
        random.seed(123)
        ac.fit_bc(types.SimpleNamespace(buffer=items, size=size), 4, num, 1e-3)
        assert seen["rows"] == ref and seen["head"] == "policy" and seen["targets"].shape == (50, 6)
    ac.fit_value(np.stack([it[0] for it in items]), np.arange(50.0), 2, 16, 1e-3, rng=random.Random(9))
    r9 = random.Random(9)
    assert seen["rows"] == [r9.sample(range(50), 16) for _ in range(2)] and seen["targets"].shape == (50, 1)


def test_container_refuses_bad_arguments_before_any_device_work(monkeypatch):
    ac = _ac(hid_size=8, seed=1)
    monkeypatch.setattr(ac, "_fitter", lambda head: pytest.fail("device work before the checks"))
    obs, acs = np.zeros((10, 20)), np.zeros((10, 6))
    bad_obs = obs.copy()
    bad_obs[3, 2] = np.nan
    bad_acs = acs.copy()
    bad_acs[1, 1] = np.inf
    for call in (lambda: ac.fit_bc((bad_obs, acs), 2, 4, 1e-3), lambda: ac.fit_bc((obs, bad_acs), 2, 4, 1e-3),
                 lambda: ac.fit_bc((obs, acs[:, :5]), 2, 4, 1e-3), lambda: ac.fit_bc((obs[:, :19], acs), 2, 4, 1e-3),
                 lambda: ac.fit_bc((obs, acs), 2, 0, 1e-3), lambda: ac.fit_bc((obs[:0], acs[:0]), 2, 4, 1e-3),
                 lambda: ac.fit_bc(types.SimpleNamespace(buffer=deque()), 2, 4, 1e-3),
                 lambda: ac.fit_bc((obs, acs), 2, 4, float("nan")), lambda: ac.fit_bc((obs, acs, acs), 2, 4, 1e-3),
                 lambda: ac.fit_value(obs, np.zeros(9), 2, 4, 1e-3), lambda: ac.fit_value(bad_obs, np.zeros(10), 2, 4, 1e-3),
                 lambda: ac.fit_value(obs, np.zeros(10), 2, -1, 1e-3), lambda: ac.update_bc(obs, acs[:9], 1e-3),
                 lambda: ac.update_bc(bad_obs, acs, 1e-3)):
        with pytest.raises(ValueError):
            call()
    assert ac.version == 0 and not ac._fitters
    with pytest.raises(ValueError):
        ac.ob_rms.update(bad_obs)
    assert ac.version == 0


# ------------------------------------------------------------------ the device fitter's refusals (no GPU)
def test_create_refuses_before_any_device_call():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    good = dict(head="policy", state_dim=20, out_dim=6, hidden=128, n_layers=2, batch_size=128)
    for change, message in [(dict(hidden=257), "hidden outside [1, 256]"), (dict(hidden=0), "hidden outside [1, 256]"),
                            (dict(n_layers=5), "n_layers outside [1, 4]"), (dict(n_layers=0), "n_layers outside [1, 4]"),
                            (dict(state_dim=33), "state_dim outside [1, 32]"), (dict(state_dim=0), "state_dim outside"),
                            (dict(out_dim=17), "outside [1, 16]"), (dict(out_dim=0), "outside [1, 16]"),
                            (dict(head="value", out_dim=2), "value head: out_dim must be 1"),
                            (dict(batch_size=0), "batch_size must be >= 1"), (dict(head="both"), "head must be"),
                            (dict(beta1=1.0), "beta1 / beta2"), (dict(epsilon=-1.0), "epsilon")]:
        kw = dict(good, **change)
        with pytest.raises(ValueError) as err:
            ac_fit.ActorCriticFitter(**kw)
        assert message in str(err.value), (change, str(err.value))
    # ... and leaves no fitter behind: the handle stays NULL
    cfg = _lib.AcFitConfig(20, 6, 300, 2, 0, 128, 0, 0.9, 0.999, 1e-8)
    import ctypes
    h = ctypes.c_void_p(1234)
    assert lib.bcmpc_acfit_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert h.value is None
    assert lib.bcmpc_acfit_create(None, ctypes.byref(h)) == _lib.ERR_ARG
    assert lib.bcmpc_acfit_destroy(None) == _lib.OK and lib.bcmpc_acfit_is_graph(None) == 0


def test_row_kernel_lds_formula_and_its_cutoffs():
    """(2 + L) row buffers of 16 x ld words, ld = the widest of hidden / S / out rounded up to 4, plus 4; targets
    16 x 16; 16 loss partials; 16 x 256 K-split partials.  Inside the limits everything fits 160 KiB (40960 words):
    the caps give 29328 words (114.6 KiB); one past any limit is refused (-1), not sized."""
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert ac_fit.lds_words(256, 4, 32, 16) == 6 * 16 * 260 + 256 + 16 + 4096 == 29328 <= 160 * 1024 // 4
    assert ac_fit.lds_words(128, 2, 20, 6) == 4 * 16 * 132 + 4368 == 12816
    assert ac_fit.lds_words(7, 1, 31, 16) == 3 * 16 * 36 + 4368
    for hidden, L, S, out, head in [(256, 4, 32, 16, 0), (256, 4, 32, 1, 1), (128, 2, 20, 6, 0), (1, 1, 1, 1, 1),
                                    (7, 1, 31, 16, 0), (129, 3, 20, 6, 0)]:
        assert lib.bcmpc_acfit_lds_words(hidden, L, S, out, head) == ac_fit.lds_words(hidden, L, S, out)
    for hidden, L, S, out, head in [(257, 4, 32, 16, 0), (256, 5, 32, 16, 0), (256, 4, 33, 16, 0), (256, 4, 32, 17, 0),
                                    (256, 4, 32, 2, 1), (256, 4, 32, 1, 2)]:
        assert lib.bcmpc_acfit_lds_words(hidden, L, S, out, head) == -1

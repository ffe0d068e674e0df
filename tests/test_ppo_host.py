"""CPU checks of the PPO definition (bc_mpc_amd/ppo.py), of the container's PPO interface
(bc_mpc_amd/actor_critic.py) and of the device trainer's refusals (csrc/ac_ppo_plan.cpp, no GPU needed); then
tests/ppo_cases.py's regime applied to the definition's own f32 trajectory, broken the ways a wrong kernel would
break it: the check that tests/test_gpu_ac_ppo.py's bound rejects wrong gradients."""
import ctypes
import random

import numpy as np
import pytest

import ppo_cases as pc
from bc_mpc_amd import ac_fit, ppo
from test_fit_oracle import M_CAP, _three_and_ragged, assert_parity, worst_ratio


# ------------------------------------------------------------------ the definition
def _smooth_batch():
    """Rows of a trained-away policy that pass the mask guard's distance rule, with clipped rows on both sides."""
    p = pc.Problem(5, 3, 12, 2, n=40, seed=3)
    f = np.float64
    pol, vf = [x.astype(f) for x in p.pol], [x.astype(f) for x in p.vf]
    rs = np.random.RandomState(1)
    pol = [x + 0.05 * rs.standard_normal(x.shape) for x in pol]           # off the old policy
    logstd = p.logstd.astype(f) + 0.03
    obz, a, at, rt, om = ppo.batch(p.flt, p.obs, p.acs, p.atarg, p.ret, p.oldmean, np.arange(40), f)
    return p, pol, vf, logstd, obz, a, at, rt, om


def test_grads_match_finite_differences():
    p, pol, vf, logstd, obz, a, at, rt, om = _smooth_batch()
    eps, entc, f = 0.2, 0.01, np.float64
    tr = {}
    _, g = ppo.grads(pol, vf, logstd, obz, a, at, rt, om, p.logstd.astype(f), eps, entc, f, trace=tr)
    cut = ~(tr["take1"] | tr["inside"])
    assert (cut & (tr["ratio"] > tr["hi"])).any() and (cut & (tr["ratio"] < tr["lo"])).any() and (~cut).any()
    bound = np.where(at >= 0, tr["hi"], tr["lo"])
    assert np.min(np.abs(tr["ratio"] - bound) / bound) > 1e-3            # the loss is smooth around this point

    def total(flat):
        n = len(pol)
        ls = ppo.grads(flat[:n], flat[n:-1], flat[-1], obz, a, at, rt, om, p.logstd.astype(f), eps, entc, f)[0]
        return ls[0] + ls[1] + ls[2]
    flat = pol + vf + [logstd]
    worst = 0.0
    for pi in range(len(flat)):
        for k in range(0, flat[pi].size, max(1, flat[pi].size // 7)):
            e = 1e-6
            p2 = [q.copy() for q in flat]
            p2[pi].flat[k] += e
            lp = total(p2)
            p2[pi].flat[k] -= 2 * e
            lm = total(p2)
            num = (lp - lm) / (2 * e)
            worst = max(worst, abs(num - g[pi].flat[k]) / (abs(num) + 1e-5))
    assert worst < 1e-4, worst


def test_gae_by_hand_and_against_discounted_sums():
    # T = 4, an episode boundary inside (step 2 starts an episode), gamma 0.9, lam 0.8, bootstrap 0.25:
    #   t=3: delta = 1 + 0.9 * 0.25 - 0.5 = 0.725                       adv = 0.725
    #   t=2: delta = 1 + 0.9 * 0.5  - 0.5 = 0.95                        adv = 0.95 + 0.72 * 0.725 = 1.472
    #   t=1: the next step is a new episode: delta = 1 - 0.5 = 0.5      adv = 0.5
    #   t=0: delta = 0.95                                               adv = 0.95 + 0.72 * 0.5 = 1.31
    adv, ret = ppo.gae([1, 1, 1, 1], [0.5] * 4, [1, 0, 1, 0], 0.25, 0.9, 0.8)
    assert adv.dtype == np.float32 and np.allclose(adv, [1.31, 0.5, 1.472, 0.725], rtol=1e-6)
    assert np.allclose(ret, np.array([1.31, 0.5, 1.472, 0.725]) + 0.5, rtol=1e-6)
    # gamma = lam = 1: adv + v is the plain sum of rewards to the episode's end (plus the bootstrap in the last one)
    rs = np.random.RandomState(0)
    rew, v = rs.standard_normal(9), rs.standard_normal(9)
    new = np.array([1, 0, 0, 1, 0, 0, 0, 1, 0])
    adv, ret = ppo.gae(rew, v, new, 0.7, 1.0, 1.0)
    want = [rew[0:3].sum(), rew[1:3].sum(), rew[2], rew[3:7].sum(), rew[4:7].sum(), rew[5:7].sum(), rew[6],
            rew[7:9].sum() + 0.7, rew[8] + 0.7]
    assert np.allclose(ret, want, atol=1e-6)
    s = ppo.standardize(rew)
    assert abs(s.mean()) < 1e-12 and abs(s.std() - 1) < 1e-12
    with pytest.raises(ValueError):
        ppo.gae([1, 1], [0.5], [0, 0], 0.0, 0.9, 0.9)


def test_step_zero_has_ratio_one_and_kl_zero_exactly():
    p, runs, _r64, ref32, _t64, t32, _v = pc.case(20, 6, 64, 2, 33)
    assert (t32[0]["ratio"] == 1.0).all() and ref32[1][0, 3] == 0.0 and ref32[1][1, 3] > 0
    at = p.atarg[runs[0][0]].astype(np.float32)
    assert ref32[1][0, 0] == -np.mean(at, dtype=np.float32)
    assert t32[0]["take1"].all()                                         # a tie goes to the first operand


def test_run_with_bc_is_the_hand_interleaving():
    p = pc.Problem(20, 6, 33, 2)
    runs = _three_and_ragged(pc.N_ROWS, 17)
    batches, bcb = runs[0] + runs[1], _three_and_ragged(pc.N_ROWS, 17, seed=4)[0] * 2

    def fresh():
        pol, vf, ls = [x.copy() for x in p.pol], [x.copy() for x in p.vf], p.logstd.copy()
        return (pol, vf, ls, ac_fit.AdamState.zeros_like(pol + vf + [ls], 0.5, 0.75),
                ac_fit.AdamState.zeros_like(pol, 0.5, 0.75))
    pol, vf, ls, st, bst = fresh()
    bl = []
    la = ppo.run(pol, vf, ls, st, p.flt, p.obs, p.acs, p.atarg, p.ret, p.oldmean, p.logstd, batches, 0.03, 0.2, 0.01,
                 bc=(p.bc_obs, p.bc_acs, bcb, 0.02), bc_state=bst, bc_losses=bl, **pc.ADAM)
    pol2, vf2, ls2, st2, bst2 = fresh()
    lb, bl2 = [], []
    for b, bb in zip(batches, bcb):
        lb.append(ppo.run(pol2, vf2, ls2, st2, p.flt, p.obs, p.acs, p.atarg, p.ret, p.oldmean, p.logstd, [b], 0.03, 0.2,
                          0.01, **pc.ADAM)[0])
        bl2 += ac_fit.run(pol2, bst2, "policy", p.flt, p.bc_obs, p.bc_acs, [bb], 0.02, 0.5, 0.75, 0.5)
    assert np.array(la).tobytes() == np.array(lb).tobytes() and bl == bl2 and len(bl) == 6
    assert all(x.tobytes() == y.tobytes() for x, y in zip(pol + vf + [ls], pol2 + vf2 + [ls2]))
    assert st.beta1_power == st2.beta1_power and bst.beta2_power == bst2.beta2_power


def test_lds_formula():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert ppo.lds_words(128, 2, 20, 6) == ac_fit.lds_words(128, 2, 20, 6) + 416
    for hidden, L, S, A in [(256, 4, 32, 16), (128, 2, 20, 6), (1, 1, 1, 1), (7, 1, 31, 16)]:
        assert lib.bcmpc_acppo_lds_words(hidden, L, S, A) == ppo.lds_words(hidden, L, S, A) <= 160 * 1024 // 4
    for hidden, L, S, A in [(257, 4, 32, 16), (256, 5, 32, 16), (256, 4, 33, 16), (256, 4, 32, 17)]:
        assert lib.bcmpc_acppo_lds_words(hidden, L, S, A) == -1


# ------------------------------------------------------------------ the regime's inputs and the bound
@pytest.mark.parametrize("S,A,hidden,L,B", pc.CASES)
def test_every_gpu_case_passes_the_mask_guard(S, A, hidden, L, B):
    _p, _runs, ref64, ref32, t64, _t32, verdict = pc.case(S, A, hidden, L, B)
    assert verdict is None, verdict
    terms = pc.ppo_parity_terms(ref32, ref64, ref32, [3, 3], t64)
    assert worst_ratio(terms) <= 1.0
    assert_parity(terms, 1)


KINDS = ["mask", "noratio", "minus1", "noent", "stale", "last_row", "vf_last_row", "beta_powers"]
BITE_CASES = [(64, 2, 33), (128, 2, 128), (256, 4, 17), (7, 1, 1)]
BITE_SEEDS = {}


@pytest.mark.parametrize("hidden,L,B", BITE_CASES)
def test_parity_bound_bites(hidden, L, B):
    """The bound of tests/test_gpu_ac_ppo.py at the cap M = 64 rejects every mutated f32 trajectory and accepts the
    unmutated one at M = 1; the mutant loop with nothing wrong is ppo.run's."""
    p = pc.Problem(20, 6, hidden, L, seed=BITE_SEEDS.get((hidden, L, B), 5))
    runs = _three_and_ragged(pc.N_ROWS, B)
    t64, t32 = [], []
    ref64 = pc.trajectory(p, runs, np.float64, traces=t64)
    ref32 = pc.trajectory(p, runs, np.float32, traces=t32)
    assert pc.mask_guard(t32, t64, [3, 3], B) is None
    same = pc.trajectory(p, runs, np.float32, kind="unmutated")
    assert same[1].tobytes() == ref32[1].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(same[0][1], ref32[0][1]))
    assert_parity(pc.ppo_parity_terms(ref32, ref64, ref32, [3, 3], t64), 1)
    for kind in KINDS:
        if B == 1 and kind in ("last_row", "vf_last_row"):
            continue                                      # (the only row: no gradient at all, a different bug)
        got = pc.trajectory(p, runs, np.float32, kind)
        terms = pc.ppo_parity_terms(got, ref64, ref32, [3, 3], t64)
        ratio = worst_ratio(terms)
        print(f"[{hidden}x{L} B{B} {kind}] worst ratio {ratio:.3g}")
        assert ratio > M_CAP, (kind, ratio)
        with pytest.raises(AssertionError):
            assert_parity(terms, M_CAP)


def test_parity_bound_bites_on_a_stale_transposed_tile():
    """With BC interleaved, a W^T copy that is one step behind in one tile (the BC step's update not yet in it)."""
    p = pc.Problem(20, 6, 64, 2)
    runs = _three_and_ragged(pc.N_ROWS, 33)
    bc_runs = [[np.roll(b, 1) for b in run] for run in runs]
    t64 = []
    ref64 = pc.trajectory(p, runs, np.float64, bc_runs=bc_runs, traces=t64)
    ref32 = pc.trajectory(p, runs, np.float32, bc_runs=bc_runs)
    assert_parity(pc.ppo_parity_terms(ref32, ref64, ref32, [3, 3], t64), 1)
    got = pc.trajectory(p, runs, np.float32, "wt_stale", bc_runs=bc_runs)
    ratio = worst_ratio(pc.ppo_parity_terms(got, ref64, ref32, [3, 3], t64))
    print(f"[wt_stale] worst ratio {ratio:.3g}")
    assert ratio > M_CAP


# ------------------------------------------------------------------ the container
class _Space:
    def __init__(self, n):
        self.shape = (n,)


class _Env:
    observation_space, action_space = _Space(20), _Space(6)


def _ac(**kw):
    from bc_mpc_amd import MlpActorCritic
    return MlpActorCritic(_Env(), **kw)


def test_package_exports():
    import bc_mpc_amd
    assert bc_mpc_amd.gae is ppo.gae and bc_mpc_amd.standardize is ppo.standardize


def test_assign_old_eq_new_copies_and_keeps_the_version():
    ac = _ac(hid_size=8, seed=1, clip_param=0.3, entcoeff=0.02)
    assert (ac.clip_param, ac.entcoeff) == (0.3, 0.02) and (_ac().clip_param, _ac().entcoeff) == (0.2, 0.0)
    ac.ob_rms.update(np.random.RandomState(0).standard_normal((10, 20)))
    v = ac.version
    ac.assign_old_eq_new()
    assert ac.version == v
    old = ac._old
    assert old["kernels"][0].tobytes() == ac.pol_kernels[0].tobytes() and old["kernels"][0] is not ac.pol_kernels[0]
    assert old["ob_mean"].tobytes() == ac.ob_rms.mean.tobytes() and old["logstd"].tobytes() == ac.logstd.tobytes()
    ac.ob_rms.update(np.ones((5, 20)))
    ac.set_weights({"logstd": np.full(6, -1.0)})
    assert old["ob_mean"].tobytes() != ac.ob_rms.mean.tobytes() and (old["logstd"] == 0).all()


def test_container_refuses_before_any_device_work(monkeypatch):
    ac = _ac(hid_size=8, seed=1)
    monkeypatch.setattr(ac, "_make_trainer", lambda *a: pytest.fail("device work before the checks"))
    monkeypatch.setattr(ac, "_fitter", lambda head: pytest.fail("device work before the checks"))
    obs, acs, at, rt = np.zeros((10, 20)), np.zeros((10, 6)), np.zeros(10), np.zeros(10)
    with pytest.raises(ValueError, match="assign_old_eq_new"):
        ac.fit_ppo(obs, acs, at, rt, 2, 4, 1e-3)
    with pytest.raises(ValueError, match="assign_old_eq_new"):
        ac.lossandupdate_ppo(obs, acs, at, rt, 1.0, 1e-3)
    ac.assign_old_eq_new()
    bad_obs, bad_at = obs.copy(), at.copy()
    bad_obs[3, 2] = np.nan
    bad_at[1] = np.inf
    for call in (lambda: ac.fit_ppo(bad_obs, acs, at, rt, 2, 4, 1e-3), lambda: ac.fit_ppo(obs, acs, bad_at, rt, 2, 4, 1e-3),
                 lambda: ac.fit_ppo(obs, acs[:, :5], at, rt, 2, 4, 1e-3), lambda: ac.fit_ppo(obs, acs, at[:9], rt, 2, 4, 1e-3),
                 lambda: ac.fit_ppo(obs, acs, at, np.zeros(11), 2, 4, 1e-3), lambda: ac.fit_ppo(obs, acs, at, rt, 2, 0, 1e-3),
                 lambda: ac.fit_ppo(obs, acs, at, rt, -1, 4, 1e-3), lambda: ac.fit_ppo(obs, acs, at, rt, 2, 4, float("nan")),
                 lambda: ac.fit_ppo(obs, acs, at, rt, 2, 4, 1e-3, clip_param=-0.1),
                 lambda: ac.fit_ppo(obs, acs, at, rt, 2, 4, 1e-3, entcoeff=float("inf")),
                 lambda: ac.fit_ppo(obs, acs, at, rt, 2, 4, 1e-3, cur_lrmult=float("nan")),
                 lambda: ac.fit_ppo(obs, acs, at, rt, 2, 4, 1e-3, bc_data=(obs, acs)),          # no bc_learning_rate
                 lambda: ac.fit_ppo(obs, acs, at, rt, 2, 4, 1e-3, bc_data=(bad_obs, acs), bc_learning_rate=1e-3),
                 lambda: ac.fit_ppo(obs, acs, at, rt, 2, 4, 1e-3, bc_data=(obs, acs, acs), bc_learning_rate=1e-3),
                 lambda: ac.lossandupdate_ppo(obs, acs, bad_at, rt, 1.0, 1e-3),
                 lambda: ac.lossandupdate_ppo(obs, acs, at, rt, -1.0, 1e-3),
                 lambda: ac.lossandupdate_ppo(obs, acs, at, rt, 1.0, float("inf"))):
        with pytest.raises(ValueError):
            call()
    assert ac.version == 0 and not ac._fitters and ac._ppo is None


def test_fit_ppo_draws_ppo_rows_then_bc_rows_on_one_stream(monkeypatch):
    """train_mpc_ppo.py:363, 368: per epoch one DataBufferGeneral.sample over the PPO data, then one over the BC
    data, both on Python's global stream; the learning rates pass as given, cur_lrmult scales only the clip range."""
    ac = _ac(hid_size=8, seed=1)
    ac.assign_old_eq_new()
    seen = {}

    def run(data, batches, lr, eps, entcoeff, bc=None):
        seen.update(batches=[list(map(int, b)) for b in batches], lr=lr, eps=eps, entcoeff=entcoeff, bc=bc, data=data)
        return np.zeros((len(batches), 6), np.float32)
    monkeypatch.setattr(ac, "_run_ppo", run)
    obs, acs, at, rt = np.zeros((50, 20)), np.zeros((50, 6)), np.arange(50.0), np.zeros(50)
    bobs, bacs = np.zeros((30, 20)), np.zeros((30, 6))
    random.seed(123)
    want, wantb = [], []
    for _ in range(4):
        want.append(random.sample(range(50), 16))
        wantb.append(random.sample(range(30), 16))
    random.seed(123)
    ac.fit_ppo(obs, acs, at, rt, 4, 16, 3e-4, clip_param=0.2, entcoeff=0.01, cur_lrmult=0.5, bc_data=(bobs, bacs),
               bc_learning_rate=1e-3)
    (bo, ba), bb, blr = seen["bc"]
    assert seen["batches"] == want and [list(map(int, b)) for b in bb] == wantb
    assert (seen["lr"], seen["eps"], seen["entcoeff"], blr) == (3e-4, 0.1, 0.01, 1e-3) and bo.shape == (30, 20)
    assert seen["data"][2].shape == (50,) and seen["data"][2][7] == 7.0
    ac.fit_ppo(obs, acs, at, rt, 2, 64, 3e-4, rng=random.Random(9))                  # a batch larger than the data
    r9 = random.Random(9)
    assert seen["batches"] == [r9.sample(range(50), 50) for _ in range(2)] and seen["bc"] is None
    ac.lossandupdate_ppo(obs, acs, at, rt, 0.25, 1e-3)
    assert seen["batches"] == [list(range(50))] and seen["eps"] == 0.05 and seen["entcoeff"] == 0.0


# ------------------------------------------------------------------ the device trainer's refusals (no GPU)
def _cfg(head, **kw):
    from bc_mpc_amd import _lib
    d = dict(state_dim=20, out_dim=6 if head == 0 else 1, hidden=128, n_layers=2, head=head, batch_size=128, device=0,
             beta1=0.9, beta2=0.999, epsilon=1e-8)
    d.update(kw)
    return _lib.AcFitConfig(*[d[k] for k in ("state_dim", "out_dim", "hidden", "n_layers", "head", "batch_size",
                                             "device", "beta1", "beta2", "epsilon")])


def test_plan_refusals_and_messages():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    adam = _lib.AcPpoConfig(0.9, 0.999, 1e-8)

    def pair(c, pol, val):
        code = lib.bcmpc_acppo_check_pair(ctypes.byref(c), ctypes.byref(pol), ctypes.byref(val))
        return code, lib.bcmpc_acppo_last_error().decode()
    assert pair(adam, _cfg(0), _cfg(1))[0] == _lib.OK
    for c, pol, val, message in [
            (adam, _cfg(1), _cfg(1), "first fitter must be a BCMPC_ACFIT_POLICY"),
            (adam, _cfg(0), _cfg(0, out_dim=1), "second fitter must be a BCMPC_ACFIT_VALUE"),
            (adam, _cfg(0), _cfg(1, state_dim=19), "differ in state_dim"),
            (adam, _cfg(0), _cfg(1, hidden=64), "differ in hidden"),
            (adam, _cfg(0), _cfg(1, n_layers=3), "differ in n_layers"),
            (adam, _cfg(0), _cfg(1, device=1), "different devices"),
            (_lib.AcPpoConfig(1.0, 0.999, 1e-8), _cfg(0), _cfg(1), "beta1 / beta2"),
            (_lib.AcPpoConfig(0.9, 0.999, -1.0), _cfg(0), _cfg(1), "epsilon")]:
        code, text = pair(c, pol, val)
        assert code == _lib.ERR_ARG and message in text, (code, text)
    code, text = pair(adam, _cfg(0, hidden=257), _cfg(1, hidden=257))
    assert code == _lib.ERR_UNSUPPORTED and "hidden outside [1, 256]" in text
    # a run's arguments
    idx = np.array([0, 5, 9, 3], np.int64)
    sizes = np.array([2, 2], np.int32)
    ip, sp = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.bcmpc_acppo_check_run(ip, sp, 2, 10, 1e-3, 0.2, 0.0) == _lib.OK
    for n, lr, eps, entc, message in [(10, float("nan"), 0.2, 0.0, "learning_rate must be finite"),
                                      (10, 1e-3, float("inf"), 0.0, "eps"), (10, 1e-3, -0.1, 0.0, "eps"),
                                      (10, 1e-3, 0.2, float("nan"), "entcoeff must be finite"),
                                      (9, 1e-3, 0.2, 0.0, "sample index out of range")]:
        assert lib.bcmpc_acppo_check_run(ip, sp, 2, n, lr, eps, entc) == _lib.ERR_ARG
        assert message in lib.bcmpc_acppo_last_error().decode()
    sizes[1] = 0
    assert lib.bcmpc_acppo_check_run(ip, sp, 2, 10, 1e-3, 0.2, 0.0) == _lib.ERR_ARG
    # null handles are refused before any device call
    h = ctypes.c_void_p(1234)
    assert lib.bcmpc_acppo_create(ctypes.byref(adam), None, None, ctypes.byref(h)) == _lib.ERR_ARG
    assert lib.bcmpc_acppo_destroy(None) == _lib.OK and lib.bcmpc_acppo_is_graph(None) == 0
    assert lib.bcmpc_acppo_run(None, ip, sp, 2, 1e-3, 0.2, 0.0, None, None, 0.0, None, None) == _lib.ERR_ARG

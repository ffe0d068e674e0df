"""The device PPO trainer (csrc/ac_ppo.hip, ``ppo.PpoTrainer``, ``MlpActorCritic.fit_ppo``) against its definition
``bc_mpc_amd.ppo.run``.

tests/ppo_cases.py is the regime: set_params, three uniform batches (one captured graph), a snapshot, three ragged
batches [B, max(1, B - 5), B] (per-step launches), a snapshot; both snapshots (pol, vf, logstd) and all losses
against the definition's f64 trajectory within M = 32 times the definition's own f32-vs-f64 error plus 2 ulp, the
losses on the scales ``ppo_parity_terms`` states.  Every case first passes ``mask_guard`` on the CPU: the clip mask
is a discontinuity, and a parity bound means nothing across it.  Set BCMPC_ACPPO_PARITY_REPORT=<file> to write
every case's worst ratio (how profiles/ac_ppo_parity.txt was made).

The shapes are the edges of the kernels' tiling, tests/test_gpu_ac_fit.py's list for one pair of stacks.
"""
import os
import random

import numpy as np
import pytest

import ppo_cases as pc
from ppo_cases import ADAM, CLIP, ENTCOEFF, LR, M, N_ROWS
from test_fit_oracle import HP, assert_parity, parity_terms, worst_ratio

pytestmark = pytest.mark.gpu

RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("BCMPC_ACPPO_PARITY_REPORT")
    if path and RATIOS:
        with open(path, "w") as fh:
            for k, v in RATIOS.items():
                fh.write(f"{v:10.4f}  {k}\n")
            fh.write(f"worst {max(RATIOS.values()):.4f} over {len(RATIOS)} cases; M = {M}\n")


def device_trainer(p, logstd=None):
    from bc_mpc_amd.ac_fit import ActorCriticFitter
    from bc_mpc_amd.ppo import PpoTrainer
    kw = dict(beta1=HP["beta1"], beta2=HP["beta2"], epsilon=HP["eps"])
    pf = ActorCriticFitter("policy", p.S, p.A, p.hidden, p.L, **kw)
    vf = ActorCriticFitter("value", p.S, 1, p.hidden, p.L, **kw)
    pf.set_params(p.pol[0::2], p.pol[1::2])
    vf.set_params(p.vf[0::2], p.vf[1::2])
    pf.set_filter(*p.flt)
    vf.set_filter(*p.flt)
    t = PpoTrainer(pf, vf, **kw)
    t.set_logstd(p.logstd)
    t.set_old(p.pol[0::2], p.pol[1::2], p.flt[0], p.flt[1], p.logstd)
    t.set_data(p.obs, p.acs, p.atarg, p.ret)
    return t, pf, vf


def close(t, pf, vf):
    t.close()
    pf.close()
    vf.close()


def flat(f):
    ks, bs = f.get_params()
    out = []
    for k, b in zip(ks, bs):
        out += [k, b]
    return out


def snapshot(t, pf, vf):
    return flat(pf) + flat(vf) + [t.get_logstd()]


def device_runs(dev, runs, hypers=None, bc_runs=None, bc_lr=LR):
    t, pf, vf = dev
    snaps, losses, graphs = [], [], []
    for ri, batches in enumerate(runs):
        lr, eps, entc = (LR, CLIP, ENTCOEFF) if hypers is None else hypers[ri]
        if bc_runs is None:
            losses += [list(x) for x in t.run(batches, lr, eps, entc)]
        else:
            l6, lb = t.run(batches, lr, eps, entc, bc_batches=bc_runs[ri], bc_lr=bc_lr)
            losses += [list(x) + [y] for x, y in zip(l6, lb)]
        graphs.append(t.graph_captures)
        snaps.append(snapshot(t, pf, vf))
    return (snaps, np.array(losses, np.float64)), graphs


@pytest.mark.parametrize("S,A,hidden,L,B", pc.CASES)
def test_gradient_resolving_parity(S, A, hidden, L, B):
    p, runs, ref64, ref32, t64, _t32, verdict = pc.case(S, A, hidden, L, B)
    assert verdict is None, verdict                       # a condition on the inputs: another seed, not a wider bound
    dev = device_trainer(p)
    got, graphs = device_runs(dev, runs)
    close(*dev)
    # uniform: the graph; ragged: launches (at B = 1 the second run is [1, 1, 1]: the same graph again)
    assert graphs[0] == 1 and graphs[1] == (1 if B == 1 else 0)
    terms = pc.ppo_parity_terms(got, ref64, ref32, [3, 3], t64)
    tag = f"S{S} A{A} {hidden}x{L} B{B}"
    ratio = worst_ratio(terms)
    RATIOS[tag] = ratio
    worst = max(terms, key=lambda t: (t[1] - t[3]) / t[2] if t[2] > 0 and t[1] > t[3] else 0.0)
    print(f"[{tag}] worst ratio {ratio:.3g} at {worst[0]}; losses {got[1][:, 0]}")
    assert np.isfinite(got[1]).all()
    assert_parity(terms, M, tag)


def test_first_step_after_assign_old_has_kl_exactly_zero():
    """mean and oldmean come from one instruction sequence: while the parameters equal the old ones ratio == 1,
    so kl == 0.0 exactly and pol_surr == -mean(atarg) to the sum's rounding; the second step's kl is not 0."""
    p, runs, *_ = pc.case(20, 6, 64, 2, 33)
    dev = device_trainer(p)
    losses = dev[0].run(runs[0], LR, CLIP, ENTCOEFF)
    close(*dev)
    assert losses[0, 3] == 0.0 and losses[1, 3] > 0.0
    at = p.atarg[runs[0][0]].astype(np.float32).astype(np.float64)
    assert abs(losses[0, 0] + at.mean()) <= 33 * np.spacing(np.float32(np.abs(at).mean()))


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_graph_and_launch_paths_and_two_trainers_agree_bitwise(monkeypatch):
    p, runs, *_ = pc.case(20, 6, 64, 2, 33)
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("BCMPC_ACPPO_GRAPH", graph)
        dev = device_trainer(p)
        got, graphs = device_runs(dev, runs)
        close(*dev)
        assert graphs == ([1, 0] if graph == "1" else [0, 0])
        out.append(got)
    snaps0, losses0 = out[0]
    for snaps, losses in out[1:]:
        assert losses.tobytes() == losses0.tobytes()
        assert _same(snaps[0], snaps0[0]) and _same(snaps[1], snaps0[1])


def test_annealed_hyperparameters_replay_one_graph():
    """Three runs with three cur_lrmult / lr / entcoeff values replay one captured graph (they are read from
    device memory) and stay within the bound; the definition with the first values throughout is beyond the cap."""
    p, runs, *_ = pc.case(20, 6, 64, 2, 33)
    rs = np.random.RandomState(12)
    small = [rs.choice(N_ROWS, 33, replace=False) for _ in range(3)]
    three = [small, small, small]
    hypers = [(LR, CLIP * 1.0, ENTCOEFF), (LR * 0.75, CLIP * 0.75, 0.02), (LR * 0.5, CLIP * 0.5, 0.005)]
    t64, t32 = [], []
    ref64 = pc.trajectory(p, three, np.float64, hypers=hypers, traces=t64)
    ref32 = pc.trajectory(p, three, np.float32, hypers=hypers, traces=t32)
    verdict = pc.mask_guard(t32, t64, [3, 3, 3], 33)
    assert verdict is None, verdict
    dev = device_trainer(p)
    got, graphs = device_runs(dev, three, hypers=hypers)
    close(*dev)
    assert graphs == [1, 1, 1], graphs
    entc = [h[2] for h in hypers]
    terms = pc.ppo_parity_terms(got, ref64, ref32, [3, 3, 3], t64, entcoeffs=entc)
    print(f"annealed sequence: worst ratio {worst_ratio(terms):.3g}")
    assert_parity(terms, M, "annealed sequence")
    stale = pc.trajectory(p, three, np.float32, hypers=[hypers[0]] * 3)
    assert worst_ratio(pc.ppo_parity_terms(stale, ref64, ref32, [3, 3, 3], t64, entcoeffs=entc)) > 64


def test_interleaved_bc_shares_the_policy_fitters_state():
    """20 -> 64 -> 64 -> 6, B = 33, every PPO step followed by one BC step of the policy fitter in the same chain:
    both optimizers' results within the bound of ppo.run(.., bc=..); afterwards a plain BC run continues the BC
    Adam state (the beta powers carried) and a plain critic run starts from the PPO-trained critic."""
    p, runs, *_ = pc.case(20, 6, 64, 2, 33)
    rs = np.random.RandomState(21)
    bc_runs = [[rs.choice(N_ROWS, len(b), replace=False) for b in run] for run in runs]
    tail_bc = [rs.choice(N_ROWS, 33, replace=False) for _ in range(3)]
    tail_v = [rs.choice(N_ROWS, 33, replace=False) for _ in range(3)]
    t64, t32, o64, o32 = [], [], {}, {}
    ref64 = pc.trajectory(p, runs, np.float64, bc_runs=bc_runs, traces=t64, tail=(tail_bc, tail_v, o64))
    ref32 = pc.trajectory(p, runs, np.float32, bc_runs=bc_runs, traces=t32, tail=(tail_bc, tail_v, o32))
    verdict = pc.mask_guard(t32, t64, [3, 3], 33)
    assert verdict is None, verdict
    dev = device_trainer(p)
    t, pf, vf = dev
    pf.set_data(p.bc_obs, p.bc_acs)
    got, graphs = device_runs(dev, runs, bc_runs=bc_runs)
    assert graphs == [1, 0]
    terms = pc.ppo_parity_terms(got, ref64, ref32, [3, 3], t64)
    print(f"interleaved BC: worst ratio {worst_ratio(terms):.3g}; BC losses {got[1][:, 6]}")
    assert_parity(terms, M, "interleaved BC")
    lb = pf.run(tail_bc, LR)
    gb = ([flat(pf)], np.array([[x] for x in lb], np.float64))
    vf.set_data(p.obs, p.ret)
    lv = vf.run(tail_v, LR)
    gv = ([flat(vf)], np.array([[x] for x in lv], np.float64))
    close(*dev)
    for name, g in (("bc", gb), ("value", gv)):
        terms = parity_terms(g, o64[name], o32[name], [3])
        print(f"then a plain {name} run: worst ratio {worst_ratio(terms):.3g}")
        assert_parity(terms, M, f"plain {name} run after PPO")
    # ... which the BC state of a fresh optimizer would not give
    fresh = {}
    pc.trajectory(p, runs, np.float32, bc_runs=bc_runs, tail=(tail_bc, tail_v, fresh), kind="fresh_bc_tail")
    assert worst_ratio(parity_terms(fresh["bc"], o64["bc"], o32["bc"], [3])) > 64


# ------------------------------------------------------------------ the container
class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n), np.ones(n)


class _AcEnv:
    observation_space, action_space = _Space(20), _Space(6)


def _container(seed=3, **kw):
    from bc_mpc_amd import MlpActorCritic, ppo
    from oracle import mpc_oracle as orc
    ac = MlpActorCritic(_AcEnv(), 128, 2, seed=seed, **kw)
    w = orc.synthetic_policy(20, 6, 128, 2)
    rs = np.random.RandomState(8)
    obs = w.ob_mean.astype(np.float64) + 1.5 * w.ob_std.astype(np.float64) * rs.standard_normal((300, 20))
    ac.ob_rms.update(obs)
    ac.set_weights({"logstd": np.full(6, -0.5, np.float32)})
    acs = ac.act(obs, stochastic=True, rng=rs)[0].astype(np.float64)
    return ac, obs, acs, ppo.standardize(rs.standard_normal(300)), 3.0 * rs.standard_normal(300), rs


def test_fit_ppo_moves_both_stacks_and_logstd_and_is_the_definition():
    from bc_mpc_amd import ac_fit, ppo
    ac, obs, acs, atarg, ret, _rs = _container()
    with pytest.raises(ValueError):
        ac.fit_ppo(obs, acs, atarg, ret, 2, 64, 1e-3)         # no snapshot yet
    w0, v0 = ac.get_weights(), ac.version
    ac.assign_old_eq_new()
    assert ac.version == v0
    losses = ac.fit_ppo(obs, acs, atarg, ret, 4, 64, 1e-3, entcoeff=0.01, rng=random.Random(5))
    assert ac.version == v0 + 1 and losses.shape == (4, 6) and losses.dtype == np.float32
    assert losses[0, 3] == 0.0 and losses[1, 3] > 0.0
    assert not _same(ac.pol_kernels, w0["pol"][0]) and not _same(ac.vf_kernels, w0["vf"][0])
    assert not np.array_equal(ac.logstd, w0["logstd"])
    r5 = random.Random(5)
    batches = [np.asarray(r5.sample(range(300), 64)) for _ in range(4)]
    pol, vf = [], []
    for k, b in zip(*w0["pol"]):
        pol += [k, b]
    for k, b in zip(*w0["vf"]):
        vf += [k, b]
    ls = w0["logstd"].copy()
    flt = (ac.ob_rms.mean, ac.ob_rms.std)
    want = ppo.run(pol, vf, ls, ac_fit.AdamState.zeros_like(pol + vf + [ls]), flt, obs, acs, atarg, ret,
                   ppo.snapshot_old(pol, flt, obs), w0["logstd"], batches, 1e-3, 0.2, 0.01)
    # tests/test_gpu_ac_fit.py's bars at the reference's Adam (eps 1e-8 turns a gradient's rounding into a step of
    # up to lr): the losses that do not cross zero within rtol 1e-4, pol_surr on the scale of mean |atarg|, kl (second
    # order in the parameters' movement) within 1%; logstd within one flipped step per iteration
    print("fit_ppo losses", losses, "definition", want)
    assert np.allclose(losses[:, [2, 4, 5]], want[:, [2, 4, 5]], rtol=1e-4, atol=0)
    assert np.allclose(losses[:, 1], want[:, 1], rtol=1e-4, atol=0)
    assert np.allclose(losses[:, 0], want[:, 0], rtol=0, atol=1e-4 * float(np.mean(np.abs(atarg))))
    assert np.allclose(losses[:, 3], want[:, 3], rtol=1e-2, atol=0)
    assert np.allclose(ac.logstd, ls, atol=2.5 * 1e-3)
    # a later BC fit, critic fit and set_weights behave as before
    v = ac.version
    ac.fit_bc((obs, acs), 2, 64, 1e-3, rng=random.Random(1))
    ac.fit_value(obs, ret, 2, 64, 1e-3, rng=random.Random(1))
    ac.set_weights({"logstd": np.full(6, -1.0, np.float32)})
    assert ac.version == v + 3
    l2 = ac.fit_ppo(obs, acs, atarg, ret, 1, 64, 1e-3, rng=random.Random(2))
    assert np.isclose(l2[0, 4], 6 * (-1.0 + float(ppo.HALF_LOG_2PIE)), rtol=1e-6)        # the new logstd reached the trainer
    ac.close()


def test_lossandupdate_ppo_is_a_one_batch_fit_ppo():
    a, obs, acs, atarg, ret, _ = _container(clip_param=0.3, entcoeff=0.02)
    b, *_ = _container(clip_param=0.3, entcoeff=0.02)
    for ac in (a, b):
        ac.assign_old_eq_new()
    # a first step moves the policy off the old one, so that the second step's clip range and entropy matter
    la = [a.lossandupdate_ppo(obs[:64], acs[:64], atarg[:64], ret[:64], 0.5, 1e-2) for _ in range(2)]

    class Whole:
        def sample(self, population, k):
            return list(population)[:k]
    lb = [b.fit_ppo(obs[:64], acs[:64], atarg[:64], ret[:64], 1, 64, 1e-2, clip_param=0.3, entcoeff=0.02,
                    cur_lrmult=0.5, rng=Whole())[0] for _ in range(2)]
    assert np.array(la).tobytes() == np.array(lb).tobytes() and la[0].shape == (6,)
    assert _same(a.pol_kernels + a.vf_kernels + [a.logstd], b.pol_kernels + b.vf_kernels + [b.logstd])
    a.close()
    b.close()


def test_through_the_controllers():
    """tests/test_gpu_ac_fit.py's check for a PPO fit: CEMcontroller(policy_prior=ac, terminal_value=ac) at K = 64,
    H = 3 picks up the new weights -- its proposal costs equal, bit for bit, those of a fresh controller over a copy
    of the weights and differ from those before the fit; MPCcontrollerPolicyNet, which samples with logstd, gives
    another answer after logstd moved."""
    from bc_mpc_amd import CEMcontroller, MlpActorCritic, MPCcontrollerPolicyNet, cheetah_cost_fn
    from test_gpu_plan_batch import net
    n = net("reluln128")
    ac, obs, acs, atarg, ret, _rs = _container()
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

    def sampled_action(container):
        pn = MPCcontrollerPolicyNet(_AcEnv(), n.dyn, container, horizon=3, cost_fn=cheetah_cost_fn,
                                    num_simulated_paths=64, seed=7)
        np.random.seed(11)
        return np.asarray(pn.get_action(n.states[0])).copy()

    ctrl = controller(ac)
    ctrl.get_action(n.states[0])
    a0 = sampled_action(ac)
    before, v = ac.get_weights(), ac.version
    ac.assign_old_eq_new()
    ac.fit_ppo(obs, acs, atarg, ret, 3, 64, 1e-2, entcoeff=0.01, rng=random.Random(1))
    assert ac.version == v + 1
    state = ctrl._seed_rng.get_state()
    ctrl.get_action(n.states[0])
    got = ctrl.last_proposal_costs.copy()
    assert got.tobytes() == costs_over(ac.get_weights(), state).tobytes()
    assert got.tobytes() != costs_over(before, state).tobytes()
    # logstd alone: the same pol/ and vf/ with the logstd from before the fit sample differently
    w = ac.get_weights()
    assert not np.array_equal(w["logstd"], before["logstd"])
    a1 = sampled_action(ac)
    other = MlpActorCritic(_AcEnv(), 128, 2, seed=99)
    other.set_weights(dict(w, logstd=before["logstd"]))
    a2 = sampled_action(other)
    assert np.isfinite(a1).all() and not np.array_equal(a1, a2) and not np.array_equal(a1, a0)
    ac.close()

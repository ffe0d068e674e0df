"""Model ensembles on the GPU (csrc/ensemble.hip, the bcmpc_ensemble_* entry points, bc_mpc_amd/ensemble.py).

Contract: candidate k has one action sequence; member e scores it as c[e][k], bit for bit what
a single engine holding member e's weights returns; the value v[k] is ``ensemble.combine`` over c[:, k]; the
argmin, CEM's select + refit and the MPPI update run on v.

Shapes (S = 20, A = 6, bounds +-1): member e's weights are synthetic_weights(.., seed_base=1000 + 100*e).
On the CPU oracle no candidate of cases A and B is within 1e-4 of a penalty threshold and the smallest top-2
gap of v over both offsets and all three rules is 0.199 (A, offset 0, mean_std; every other >= 0.40), more
than 1000x the cost bar: every argmin assertion runs, none is skipped.  The members disagree: A/0 member
winners [5, 5, 28], rules pick 5 / 1 / 28; A/1000 [0, 5, 25] -> 5 / 10 / 21; B/0 [6, 0, 15, 3, 12] -> 7 under
every rule (no member's choice).

Cost bar: the suite's own (assert_costs_close: ATOL 1e-4, RTOL 1e-5, capped by conftest.envelope) on the
member costs, and on v for "mean" and "worst" (an average / a selection of values inside the bar stays
inside it; the spread term of "mean_std" can amplify, so v is only pinned to combine of the GPU's own member
costs there, bit for bit, like every rule).
"""
import functools
import random

import numpy as np
import pytest

from conftest import envelope
from test_gpu_parity import assert_costs_close, team_ok

pytestmark = pytest.mark.gpu

S, A = 20, 6
LOW, HIGH = -np.ones(A), np.ones(A)
RULES = [("mean", 0.0), ("mean_std", 1.0), ("worst", 0.0)]

#        hidden act    ln     H  K   E  seed
CASES = {
    "A": (64, "tanh", False, 5, 37, 3, 1234),
    "B": (128, "relu", True, 3, 17, 5, 77),
    "C": (64, "tanh", False, 1, 1, 2, 5),
}
KERNELS = ["auto", "solo", "group4", "split2", "team"]
#          (case, offset): member winners, then the winners under mean / mean_std (kappa 1) / worst
WINNERS = {("A", 0): ([5, 5, 28], [5, 1, 28]), ("A", 1000): ([0, 5, 25], [5, 10, 21]),
           ("B", 0): ([6, 0, 15, 3, 12], [7, 7, 7])}


def _bits_equal(a, b):
    """Equal bit for bit where not NaN; NaN positions equal."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), "NaN positions differ"
    assert a[~na].tobytes() == b[~nb].tobytes()


class Ref:
    """One case's inputs and its oracle composition (read-only, shared by the tests)."""

    def __init__(self, case, cand_offset):
        from bc_mpc_amd.ensemble import combine
        from oracle import mpc_oracle as orc
        self.hidden, self.act, self.ln, self.H, self.K, self.E, self.seed = CASES[case]
        self.case, self.cand_offset = case, cand_offset
        self.ws = [orc.synthetic_weights(S, A, self.hidden, 2, self.act, self.ln, seed_base=1000 + 100 * e)
                   for e in range(self.E)]
        self.norm = orc.synthetic_normalization()
        self.state = orc.synthetic_state(self.norm, seed=11)
        self.dyns = [orc.NumpyDynamics(w, self.norm) for w in self.ws]
        self.actions = orc.device_rng_actions(self.seed, cand_offset, self.K, self.H, LOW, HIGH)
        self.member_costs = np.stack([orc.rollout(d, self.state, self.actions)[0] for d in self.dyns])
        self.v = {rule: combine(self.member_costs, rule, kappa) for rule, kappa in RULES}
        for x in (self.state, self.actions, self.member_costs, *self.v.values()):
            x.setflags(write=False)
        self.env = envelope(self.ln, 2, self.hidden, self.H)

    def spec(self, e):
        from bc_mpc_amd.engine import MLPSpec
        w = self.ws[e]
        return MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta)

    def ensemble(self, kernel="auto", K=None, E=None, **kw):
        from bc_mpc_amd.ensemble import EnsembleEngine
        E = self.E if E is None else E
        ens = EnsembleEngine(E, S, A, self.hidden, 2, self.act, self.ln, self.H, self.K if K is None else K,
                             device=0, kernel=kernel, **kw)
        if kernel != "auto":
            assert ens.info()["kernel"] == kernel
        for e in range(E):
            ens.set_weights(e, self.spec(e), self.norm, 1)
        return ens

    def single(self, e, kernel="auto", K=None, **kw):
        from bc_mpc_amd.engine import RolloutEngine
        eng = RolloutEngine(S, A, self.hidden, 2, self.act, self.ln, self.H, self.K if K is None else K, device=0,
                            kernel=kernel, **kw)
        eng.set_weights(self.spec(e), self.norm, 1)
        return eng


@functools.lru_cache(maxsize=None)
def ref(case, cand_offset=0) -> Ref:
    return Ref(case, cand_offset)


def _skip_unsupported(r: Ref, kernel, K=None):
    if kernel == "team" and not team_ok(r.hidden, r.ln, 2, r.K if K is None else K, S, A):
        pytest.skip("team: the 2-layer delta net at small K (grid resident)")


def same_record(a, b, ia=None, ib=None):
    pick = lambda x, i, f: getattr(x, f) if i is None else getattr(x, f)[i]   # noqa: E731
    assert int(pick(a, ia, "best_index")) == int(pick(b, ib, "best_index"))
    ca, cb = np.float64(pick(a, ia, "best_cost")), np.float64(pick(b, ib, "best_cost"))
    assert ca.tobytes() == cb.tobytes() or (np.isnan(ca) and np.isnan(cb))
    assert np.array_equal(pick(a, ia, "first_action"), pick(b, ib, "first_action"), equal_nan=True)


def test_oracle_composition_has_the_stated_winners():
    """The reference itself: the indices the issue lists, and the gaps that make every argmin decidable."""
    for (case, off), (members, rules) in WINNERS.items():
        r = ref(case, off)
        assert [int(np.argmin(c)) for c in r.member_costs] == members
        assert [int(np.argmin(r.v[rule])) for rule, _ in RULES] == rules
        for rule, _ in RULES:
            lo2 = np.sort(r.v[rule])[:2]
            assert lo2[1] - lo2[0] >= 0.199


# ------------------------------------------------------------------ 1. the reduce kernel
def _reduce_inputs(E, K, ld, rs):
    c = np.full((E, ld), 12345.0)                        # (the padding columns are never read)
    c[:, :K] = rs.randn(E, K) * 10.0 ** rs.randint(-2, 3, size=(1, K))
    special = [np.full(E, np.nan), np.r_[np.nan, np.ones(E - 1)], np.r_[np.ones(E - 1), np.nan],
               np.r_[np.inf, np.ones(E - 1)], np.r_[-np.inf, np.ones(E - 1)], np.full(E, -0.0), np.full(E, 2.5),
               np.r_[1e308, 1e308, np.zeros(E - 2)] if E >= 2 else np.full(E, 1e308),
               np.r_[np.inf, -np.inf, np.zeros(E - 2)] if E >= 2 else np.full(E, np.inf)]
    for i, col in enumerate(special):
        if 2 + 3 * i < K:
            c[:, 2 + 3 * i] = col[:E]
    if K == 1:
        c[:, 0] = -0.0
    return c


@pytest.mark.parametrize("E", [1, 2, 3, 16])
def test_reduce_kernel_is_combine_bit_for_bit(E):
    import torch
    from bc_mpc_amd import ensemble
    r = ref("C")
    eng = r.single(0)
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(40 + E)
    st = torch.cuda.current_stream(dev).cuda_stream
    for K in (1, 63, 64, 65, 1000):
        for ld in (K, K + 3):
            c = _reduce_inputs(E, K, ld, rs)
            d_c = torch.from_numpy(c).to(dev)
            for rule, kappas in (("mean", [0.0]), ("mean_std", [0.0, 0.5, -1.0]), ("worst", [0.0])):
                for kappa in kappas:
                    d_out = torch.full((K + 2,), 777.0, dtype=torch.float64, device=dev)
                    ensemble.reduce_async(eng, d_c.data_ptr(), ld, E, K, rule, kappa, d_out.data_ptr(), st)
                    got = d_out.cpu().numpy()
                    assert got[K] == 777.0 and got[K + 1] == 777.0, "wrote past K"
                    _bits_equal(got[:K], ensemble.combine(c[:, :K], rule, kappa))
    # E = 1 returns -0.0
    d_c = torch.from_numpy(np.full((1, 5), -0.0)).to(dev)
    d_out = torch.ones(5, dtype=torch.float64, device=dev)
    for rule in ("mean", "worst"):
        ensemble.reduce_async(eng, d_c.data_ptr(), 5, 1, 5, rule, 0.0, d_out.data_ptr(), st)
        assert d_out.cpu().numpy().tobytes() == np.full(5, -0.0).tobytes()
    eng.close()


# ------------------------------------------------------------------ 2.-4. members, definition, oracle
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case,cand_offset", [("A", 0), ("A", 1000), ("B", 0), ("B", 1000), ("C", 0), ("C", 1000)])
def test_ensemble_get_action(case, cand_offset, kernel):
    from bc_mpc_amd.ensemble import combine
    r = ref(case, cand_offset)
    _skip_unsupported(r, kernel)
    ens = r.ensemble(kernel)
    layout = ens.info()["layout"]
    got = {}
    for rule, kappa in RULES:
        ens.set_rule(rule, kappa)
        for acts in (None, r.actions):
            res = ens.get_action(r.state, acts, seed=r.seed, cand_offset=cand_offset, return_member_costs=True)
            assert res.member_costs.shape == (r.E, r.K) and res.costs.shape == (r.K,)
            # 3. the call is the definition
            _bits_equal(res.costs, combine(res.member_costs, rule, kappa))
            j = res.best_index - cand_offset
            assert j == int(np.argmin(res.costs))
            assert np.float64(res.best_cost).tobytes() == res.costs[j].tobytes()
            assert np.array_equal(res.first_action, r.actions[0, j])
            # 4. oracle parity
            for e in range(r.E):
                assert_costs_close(res.member_costs[e], r.member_costs[e], None,
                                   f"{case}+{cand_offset}/{kernel}/member{e}", env=r.env)
            if rule != "mean_std":
                assert_costs_close(res.costs, r.v[rule], None, f"{case}+{cand_offset}/{kernel}/{rule}", env=r.env)
            assert j == int(np.argmin(r.v[rule]))
            if (case, cand_offset) in WINNERS:
                assert j == WINNERS[case, cand_offset][1][[x for x, _ in RULES].index(rule)]
            got[rule, acts is None] = res
        # the Philox draw and the explicit array of the same actions: the same bits
        assert np.array_equal(got[rule, True].member_costs, got[rule, False].member_costs)
        same_record(got[rule, True], got[rule, False])
        lean = ens.get_action(r.state, None, seed=r.seed, cand_offset=cand_offset)      # no cost vectors asked for
        assert lean.costs is None and lean.member_costs is None
        same_record(lean, got[rule, True])
    ens.close()
    # 2. the members are the single engines
    mc = got["mean", True].member_costs
    for e in range(r.E):
        one = r.single(e, kernel)
        assert one.info()["layout"] == layout
        for acts in (None, r.actions):
            s = one.get_action(r.state, acts, seed=r.seed, cand_offset=cand_offset, return_costs=True)
            assert np.array_equal(s.costs, mc[e]), f"member {e} differs from the single engine"
        one.close()


@pytest.mark.parametrize("kernel", ["auto", "solo"])
def test_nan_wins_and_ties_keep_the_lower_index(kernel):
    r = ref("A", 0)
    ens = r.ensemble(kernel)
    for rule, kappa in RULES:
        ens.set_rule(rule, kappa)
        acts = r.actions.copy()
        acts[0, 9, 0] = np.nan
        acts[1, 30, 2] = np.nan
        res = ens.get_action(r.state, acts, return_member_costs=True)
        assert res.best_index == 9 and np.isnan(res.best_cost)
        assert np.array_equal(res.first_action, acts[0, 9], equal_nan=True)
        assert np.isnan(res.costs).sum() == 2 and np.isnan(res.member_costs[:, [9, 30]]).all()
        best = int(np.argmin(r.v[rule]))
        acts = r.actions.copy()
        for j in (4, 33):
            acts[:, j, :] = acts[:, best, :]
        res = ens.get_action(r.state, acts, return_costs=True)
        c = res.costs
        assert c[4].tobytes() == c[33].tobytes() == c[best].tobytes() and c[4] == c.min()
        assert res.best_index == min(4, 33, best) == int(np.argmin(c))
    ens.close()


# ------------------------------------------------------------------ 5. E = 1 is the single engine
@pytest.mark.parametrize("kernel", ["auto", "solo", "group4", "split2", "team"])
def test_one_member_is_the_single_engine(kernel):
    r = ref("A", 1000)
    _skip_unsupported(r, kernel)
    ens, one = r.ensemble(kernel, E=1), r.single(0, kernel)
    for rule, kappa in (("mean", 0.0), ("worst", 0.0), ("mean_std", 0.0)):
        ens.set_rule(rule, kappa)
        for acts in (None, r.actions):
            a = ens.get_action(r.state, acts, seed=r.seed, cand_offset=1000, return_costs=True)
            b = one.get_action(r.state, acts, seed=r.seed, cand_offset=1000, return_costs=True)
            assert a.costs.tobytes() == b.costs.tobytes()
            same_record(a, b)
    ens.set_rule("mean")
    if kernel != "solo":                                  # (CEM / MPPI sample in the kernel: group layouts)
        mu0, sd0 = np.zeros((r.H, A)), np.full((r.H, A), 0.5)
        ra, ma, sa = ens.cem_get_action(r.state, mu0, sd0, 3, 5, 0.1, r.seed)
        rb, mb, sb = one.cem_get_action(r.state, mu0, sd0, 3, 5, 0.1, r.seed)
        same_record(ra, rb)
        assert ma.tobytes() == mb.tobytes() and sa.tobytes() == sb.tobytes()
        ra, ma, ta = ens.mppi_get_action(r.state, mu0, sd0, 3, 1.0, r.seed)
        rb, mb, tb = one.mppi_get_action(r.state, mu0, sd0, 3, 1.0, r.seed)
        same_record(ra, rb)
        assert ma.tobytes() == mb.tobytes() and bytes(ta) == bytes(tb)
    else:
        with pytest.raises(ValueError):
            ens.cem_get_action(r.state, np.zeros((r.H, A)), np.ones((r.H, A)), 2, 5, 0.1, 1)
    ens.close()
    one.close()


# ------------------------------------------------------------------ 6. the batched step
@pytest.mark.parametrize("kernel", ["auto", "solo", "group4", "split2"])
@pytest.mark.parametrize("case,B", [("A", 5), ("C", 4)])
def test_batch_equals_single_ensemble_calls(case, B, kernel):
    from oracle import mpc_oracle as orc
    r = ref(case, 0)
    states = np.stack([orc.synthetic_state(r.norm, seed=11 + b) for b in range(B)])
    big, one = r.ensemble(kernel, K=B * r.K), r.ensemble(kernel)
    assert big.info()["layout"] == one.info()["layout"]
    for rule, kappa in RULES:
        big.set_rule(rule, kappa)
        one.set_rule(rule, kappa)
        for off in (0, 1000):
            res = big.get_actions(states, None, seed=r.seed, cand_offset=off, return_member_costs=True)
            assert res.costs.shape == (B, r.K) and res.member_costs.shape == (r.E, B, r.K)
            for b in range(B):
                s = one.get_action(states[b], None, seed=r.seed, cand_offset=off + b * r.K, return_member_costs=True)
                assert res.costs[b].tobytes() == s.costs.tobytes()
                assert res.member_costs[:, b].tobytes() == s.member_costs.tobytes()
                same_record(res, s, b)
            lean = big.get_actions(states, None, seed=r.seed, cand_offset=off)
            assert lean.costs is None and np.array_equal(lean.best_index, res.best_index)
    # explicit actions: the kernels' [H, B*K, A] layout
    acts = orc.device_rng_actions(r.seed, 0, B * r.K, r.H, LOW, HIGH)
    a = big.get_actions(states, acts, return_member_costs=True)
    b_ = big.get_actions(states, None, seed=r.seed, return_member_costs=True)
    assert a.member_costs.tobytes() == b_.member_costs.tobytes()
    for b in range(B):
        same_record(a, b_, b, b)
    with pytest.raises(ValueError, match="multiple"):
        big.get_actions(np.zeros((3 if case == "C" else 2, S)))          # 4 % 3, 185 % 2
    big.close()
    one.close()


# ------------------------------------------------------------------ 7. CEM and MPPI over E = 3
ELITE = np.dtype([("cost", "<f8"), ("index", "<i8")])


@pytest.mark.parametrize("kernel", ["auto", "group4", "split2", "team"])
@pytest.mark.parametrize("planner", ["cem", "mppi"])
@pytest.mark.parametrize("rule,kappa", RULES)
def test_planner_equals_the_chain_composed_from_the_blocks(planner, rule, kappa, kernel):
    import torch
    from bc_mpc_amd import ensemble
    from bc_mpc_amd.engine import MPPI_STATS
    from oracle import mpc_oracle as orc
    r = ref("A", 0)
    _skip_unsupported(r, kernel)
    iters, n_elite, alpha, lam = 3, 5, 0.1, 1.0
    K, H, E = r.K, r.H, r.E
    mu0, sd0 = np.zeros((H, A)), np.full((H, A), 0.5)
    ens = r.ensemble(kernel)
    ens.set_rule(rule, kappa)
    if planner == "cem":
        res, mu, sd = ens.cem_get_action(r.state, mu0, sd0, iters, n_elite, alpha, r.seed)
    else:
        res, mu, stats = ens.mppi_get_action(r.state, mu0, sd0, iters, lam, r.seed)
    ens.close()
    # the same chain from the stream-ordered blocks on single engines
    engs = [r.single(e, kernel) for e in range(E)]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    d_state = torch.from_numpy(r.state.copy()).to(dev)
    d_mu, d_sd = torch.from_numpy(mu0.copy()).to(dev), torch.from_numpy(sd0.copy()).to(dev)
    d_mc, d_v = torch.empty((E, K), **f64), torch.empty(K, **f64)
    d_el = torch.empty(n_elite * 16, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    d_stats = torch.zeros(MPPI_STATS.itemsize, dtype=torch.uint8, device=dev)
    vs, hist = [], []
    for it in range(iters):
        hist.append((d_mu.cpu().numpy(), d_sd.cpu().numpy()))
        for e in range(E):
            engs[e].cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sd.data_ptr(), r.seed, it, 0, K,
                                      d_mc[e].data_ptr(), None, False, st)
        ensemble.reduce_async(engs[0], d_mc.data_ptr(), K, E, K, rule, kappa, d_v.data_ptr(), st)
        torch.cuda.synchronize()
        for e in range(E):
            engs[e].check_status()
        mc, v = d_mc.cpu().numpy(), d_v.cpu().numpy()
        _bits_equal(v, ensemble.combine(mc, rule, kappa))
        vs.append(v)
        if it == 0:                                      # the oracle composition of iteration 0
            acts = orc.cem_actions(r.seed, 0, 0, K, H, mu0, sd0, LOW, HIGH)
            want = np.stack([orc.rollout(d, r.state, acts)[0] for d in r.dyns])
            for e in range(E):
                assert_costs_close(mc[e], want[e], None, f"{planner}/{rule}/{kernel}/member{e}", env=r.env)
            if rule != "mean_std":
                assert_costs_close(v, ensemble.combine(want, rule, kappa), None, f"{planner}/{rule}/{kernel}/v",
                                   env=r.env)
        if planner == "cem":
            engs[0].select_async(None, d_v.data_ptr(), K, 0, n_elite, d_el.data_ptr(), d_cnt.data_ptr(), st)
            engs[0].cem_refit_async(d_el.data_ptr(), d_cnt.data_ptr(), r.seed, it, alpha, d_mu.data_ptr(),
                                    d_sd.data_ptr(), st)
        else:
            engs[0].mppi_update_async(d_v.data_ptr(), K, 0, r.seed, it, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                      d_stats.data_ptr(), st)
    torch.cuda.synchronize()
    assert mu.tobytes() == d_mu.cpu().numpy().tobytes()
    if planner == "cem":
        assert sd.tobytes() == d_sd.cpu().numpy().tobytes()
    else:
        assert bytes(stats) == d_stats.cpu().numpy().tobytes()
    flat = np.concatenate(vs)
    pos = int(np.argmin(flat))
    assert res.best_index == pos and np.float64(res.best_cost).tobytes() == flat[pos].tobytes()
    it, i = divmod(pos, K)
    assert np.array_equal(res.first_action, orc.cem_actions(r.seed, it, i, 1, 1, *hist[it], LOW, HIGH)[0, 0])
    for e in engs:
        e.close()


# ------------------------------------------------------------------ 8. cost terms
@pytest.mark.parametrize("kernel", ["solo", "group4", "split2"])
def test_cheetah_terms_ensemble_equals_the_cheetah_ensemble(kernel):
    from bc_mpc_amd import cheetah_terms
    r = ref("A", 0)
    a, b = r.ensemble(kernel), r.ensemble(kernel, cost="terms")
    with pytest.raises(Exception, match="set_cost_terms"):
        b.get_action(r.state, None, seed=r.seed)
    b.set_cost_terms(cheetah_terms())
    for rule, kappa in RULES:
        a.set_rule(rule, kappa)
        b.set_rule(rule, kappa)
        for acts in (None, r.actions):
            ra = a.get_action(r.state, acts, seed=r.seed, return_member_costs=True)
            rb = b.get_action(r.state, acts, seed=r.seed, return_member_costs=True)
            assert ra.member_costs.tobytes() == rb.member_costs.tobytes()
            assert ra.costs.tobytes() == rb.costs.tobytes()
            same_record(ra, rb)
    a.close()
    b.close()


# ------------------------------------------------------------------ 9. team give-up
def test_team_giveup_reruns_the_whole_call_on_the_fallback_layout(monkeypatch):
    from oracle import mpc_oracle as orc
    r = ref("A", 0)
    B = 5
    states = np.stack([orc.synthetic_state(r.norm, seed=11 + b) for b in range(B)])
    mu0, sd0 = np.zeros((r.H, A)), np.full((r.H, A), 0.5)
    for K, batched in ((r.K, False), (B * r.K, True)):
        team = r.ensemble("team", K=K)
        monkeypatch.setenv("BCMPC_TEAM_SPINS", "-1")
        team.set_rule("mean_std", 1.0)
        if batched:
            got = [team.get_actions(states, None, seed=r.seed, return_member_costs=True)]
        else:
            got = [team.get_action(r.state, None, seed=r.seed, return_member_costs=True),
                   team.get_action(r.state, r.actions, return_costs=True),
                   team.cem_get_action(r.state, mu0, sd0, 3, 5, 0.1, r.seed),
                   team.mppi_get_action(r.state, mu0, sd0, 3, 1.0, r.seed)]
        monkeypatch.delenv("BCMPC_TEAM_SPINS")
        assert team.team_reruns == len(got) and all(m.team_reruns == len(got) for m in team.members)
        # the fallback layout: auto without the team kernel in split precision -- one 16-candidate column per
        # workgroup at these K (capi.cpp team_fallback / bcmpc_create)
        fb = r.ensemble("split1", K=K)
        fb.set_rule("mean_std", 1.0)
        if batched:
            want = [fb.get_actions(states, None, seed=r.seed, return_member_costs=True)]
        else:
            want = [fb.get_action(r.state, None, seed=r.seed, return_member_costs=True),
                    fb.get_action(r.state, r.actions, return_costs=True),
                    fb.cem_get_action(r.state, mu0, sd0, 3, 5, 0.1, r.seed),
                    fb.mppi_get_action(r.state, mu0, sd0, 3, 1.0, r.seed)]
        fb.close()
        # the team ensemble answers normally again afterwards
        after = team.get_actions(states, None, seed=r.seed) if batched else team.get_action(r.state, None, seed=r.seed)
        assert team.team_reruns == len(got)
        assert np.array_equal(np.atleast_1d(after.best_index), np.atleast_1d(want[0].best_index))
        team.close()
        for g, w in zip(got, want):
            if isinstance(g, tuple):
                same_record(g[0], w[0])
                assert g[1].tobytes() == w[1].tobytes()
                if isinstance(g[2], np.ndarray):
                    assert g[2].tobytes() == w[2].tobytes()
                else:
                    assert bytes(g[2]) == bytes(w[2])
            elif batched:
                assert g.costs.tobytes() == w.costs.tobytes()
                assert g.member_costs.tobytes() == w.member_costs.tobytes()
                for b in range(B):
                    same_record(g, w, b, b)
            else:
                assert g.costs.tobytes() == w.costs.tobytes()
                same_record(g, w)


# ------------------------------------------------------------------ 10. graph replay
def test_reduce_replays_in_a_captured_graph():
    """The block is one kernel launch on the caller's stream: it allocates nothing and synchronises nothing,
    so it can be captured (an allocation or a synchronisation inside the capture would fail it) and replayed
    on changed inputs."""
    import torch
    from bc_mpc_amd import ensemble
    r = ref("C")
    eng = r.single(0)
    dev = torch.device("cuda", 0)
    E, K, ld = 3, 65, 68
    rs = np.random.RandomState(3)
    d_c = torch.from_numpy(rs.randn(E, ld)).to(dev)
    d_out = torch.zeros(K, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                        # warm-up launch outside the capture
        ensemble.reduce_async(eng, d_c.data_ptr(), ld, E, K, "mean_std", 0.5, d_out.data_ptr(), side.cuda_stream)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ensemble.reduce_async(eng, d_c.data_ptr(), ld, E, K, "mean_std", 0.5, d_out.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(2):
        new = rs.randn(E, ld)
        d_c.copy_(torch.from_numpy(new))
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        _bits_equal(d_out.cpu().numpy(), ensemble.combine(new[:, :K], "mean_std", 0.5))
    eng.close()


# ------------------------------------------------------------------ 11. controllers
class _Box:
    low, high = LOW, HIGH
    shape = (A,)


class _Env:
    action_space = _Box()

    class observation_space:
        shape = (S,)


def _model(r: Ref, **kw):
    """An EnsembleDynamicsModel holding the case's member weights."""
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel
    m = EnsembleDynamicsModel(_Env(), r.E, 2, r.hidden, r.act, None, r.norm, 32, 3, 1e-3, layer_norm=r.ln,
                              device=0, **kw)
    for e, w in enumerate(r.ws):
        m.load_weights(e, w.kernels, w.biases, w.ln_gamma, w.ln_beta)
    return m


def _first_seed(seed):
    return int(np.random.RandomState(seed).randint(0, 2**62, dtype=np.int64))


def test_mpc_controller_numpy_stream():
    from bc_mpc_amd import MPCcontroller, cheetah_cost_fn
    r = ref("A", 0)
    model = _model(r, diagnostics=True)
    ctrl = MPCcontroller(_Env(), model, horizon=r.H, cost_fn=cheetah_cost_fn, num_simulated_paths=r.K)
    ctrl.keep_costs = True
    np.random.seed(123)
    got = ctrl.get_action(r.state)
    after = np.random.get_state()
    np.random.seed(123)
    paths = np.random.uniform(LOW, HIGH, size=[r.H, r.K, A])               # exactly one [H, K, A] draw
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), after))
    j = int(np.argmin(ctrl.last_costs))
    assert ctrl.last_index == j and np.array_equal(got, paths[0, j])
    ens = r.ensemble("auto")
    want = ens.get_action(r.state, paths, return_member_costs=True)
    ens.close()
    assert want.best_index == j and ctrl.last_costs.tobytes() == want.costs.tobytes()
    assert ctrl.last_member_costs.tobytes() == want.member_costs[:, j].tobytes()
    assert ctrl.last_disagreement == float(np.std(want.member_costs[:, j]))
    ctrl._ens_engines["single"][1].close()


def test_controllers_agree_with_the_engine_and_follow_the_rule():
    from bc_mpc_amd import CEMcontroller, MPCcontroller, MPPIcontroller, cheetah_cost_fn
    from oracle import mpc_oracle as orc
    r = ref("A", 0)
    model = _model(r)
    ens = r.ensemble("auto")
    # rng="device": seeded so that the call draws the case's seed is not possible; the engine gets the drawn seed
    ctrl = MPCcontroller(_Env(), model, horizon=r.H, cost_fn=cheetah_cost_fn, num_simulated_paths=r.K, rng="device",
                         seed=3)
    src = np.random.RandomState(3)
    engine_obj = None
    for rule, kappa in RULES + [("mean", 0.0)]:
        model.rule, model.kappa = rule, kappa
        seed = int(src.randint(0, 2**62, dtype=np.int64))
        got = ctrl.get_action(r.state)
        ens.set_rule(rule, kappa)
        want = ens.get_action(r.state, None, seed=seed)
        assert np.array_equal(got, want.first_action) and ctrl.last_index == want.best_index
        assert ctrl.last_member_costs is None
        if engine_obj is None:
            engine_obj = ctrl._ens_engines["single"][1]
        assert ctrl._ens_engines["single"][1] is engine_obj          # the rule changes, the engines stay
    # the rule changes the winner on the case's own candidates (explicit actions = the Philox draw at seed 1234)
    ctrl2 = MPCcontroller(_Env(), model, horizon=r.H, cost_fn=cheetah_cost_fn, num_simulated_paths=r.K)
    ctrl2.sample_random_actions = lambda: r.actions.copy()
    picks = []
    for rule, kappa in RULES:
        model.rule, model.kappa = rule, kappa
        ctrl2.get_action(r.state)
        picks.append(ctrl2.last_index)
    assert picks == WINNERS["A", 0][1] == [5, 1, 28]
    model.rule, model.kappa = "mean_std", 1.0
    ens.set_rule("mean_std", 1.0)
    # get_actions
    B = 3
    states = np.stack([orc.synthetic_state(r.norm, seed=11 + b) for b in range(B)])
    model.diagnostics = True
    seed = int(src.randint(0, 2**62, dtype=np.int64))
    got = ctrl.get_actions(states)
    big = r.ensemble("auto", K=B * r.K)
    big.set_rule("mean_std", 1.0)
    want = big.get_actions(states, None, seed=seed, return_member_costs=True)
    big.close()
    assert np.array_equal(got, want.first_action) and np.array_equal(ctrl.last_index, want.best_index)
    assert ctrl.last_member_costs.shape == (B, r.E)
    for b in range(B):
        j = int(want.best_index[b]) - b * r.K
        assert ctrl.last_member_costs[b].tobytes() == want.member_costs[:, b, j].tobytes()
    model.diagnostics = False
    # CEM and MPPI
    cem = CEMcontroller(_Env(), model, horizon=r.H, cost_fn=cheetah_cost_fn, num_simulated_paths=r.K, iterations=3,
                        n_elite=5, seed=11)
    got = cem.get_action(r.state)
    mu0, sd0 = np.zeros((r.H, A)), np.full((r.H, A), 0.5)
    res, mu, sd = ens.cem_get_action(r.state, mu0, sd0, 3, 5, 0.1, _first_seed(11))
    assert np.array_equal(got, res.first_action) and cem.last_position == res.best_index
    assert cem.last_mu.tobytes() == mu.tobytes() and cem.last_sigma.tobytes() == sd.tobytes()
    mppi = MPPIcontroller(_Env(), model, horizon=r.H, cost_fn=cheetah_cost_fn, num_simulated_paths=r.K, iterations=3,
                          temperature=1.0, seed=12)
    got = mppi.get_action(r.state)
    res, mu, stats = ens.mppi_get_action(r.state, mu0, sd0, 3, 1.0, _first_seed(12))
    assert np.array_equal(got, mu[0]) and mppi.last_position == res.best_index
    assert bytes(mppi.last_stats) == bytes(stats)
    ens.close()
    for c in (ctrl, ctrl2, cem, mppi):
        for _, e in c._ens_engines.values():
            e.close()


def test_plain_model_is_unchanged():
    from bc_mpc_amd import MPCcontroller, cheetah_cost_fn
    from oracle import mpc_oracle as orc
    r = ref("A", 0)
    ctrl = MPCcontroller(_Env(), orc.NumpyDynamics(r.ws[0], r.norm), horizon=r.H, cost_fn=cheetah_cost_fn,
                         num_simulated_paths=r.K, rng="device", seed=3)
    got = ctrl.get_action(r.state)
    one = r.single(0)
    want = one.get_action(r.state, None, seed=_first_seed(3))
    one.close()
    assert np.array_equal(got, want.first_action) and ctrl.last_index == want.best_index
    assert "_ens_engines" not in ctrl.__dict__
    ctrl._engine.close()


# ------------------------------------------------------------------ 12. fit
def test_fit_members_equal_standalone_fitters():
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel, bootstrap_batches, combine, member_rng
    from bc_mpc_amd.fit import GPUFitter
    from oracle import mpc_oracle as orc
    n, bs, iters, E, lr, seed = 200, 32, 3, 3, 1e-3, 21
    rs = np.random.RandomState(5)
    norm = orc.synthetic_normalization(S, A)
    states = norm[0] + norm[1] * rs.standard_normal((n, S))
    actions = rs.uniform(-1, 1, (n, A))
    deltas = norm[8] + norm[9] * rs.standard_normal((n, S))
    model = EnsembleDynamicsModel(_Env(), E, 2, 64, "tanh", None, norm, bs, iters, lr, seed=seed, device=0)
    start = [m.mlp_spec() for m in model.members]
    py_state, np_state = random.getstate(), np.random.get_state()
    loss1, zero = model.fit((states, actions, deltas))
    after1 = [m.mlp_spec() for m in model.members]
    loss2, _ = model.fit((states, actions, deltas))
    assert random.getstate() == py_state
    assert all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), np_state))
    assert zero == 0 and np.isfinite(loss1) and np.isfinite(loss2)
    last1, last2 = [], []
    for i in range(E):
        f = GPUFitter(S, A, 64, 2, "tanh", False, bs, lr, device=0)
        f.set_params(start[i], norm)
        f.set_data(states, actions, deltas)
        rng = member_rng(seed, i)
        last1.append(f.run(bootstrap_batches(rng, n, bs, iters))[-1])
        ks, bsx, _, _ = f.get_params()
        for got, want in zip(after1[i].kernels + after1[i].biases, ks + bsx):
            assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), f"member {i} after the first fit"
        last2.append(f.run(bootstrap_batches(rng, n, bs, iters))[-1])     # the Adam slots go on
        ks, bsx, _, _ = f.get_params()
        now = model.members[i].mlp_spec()
        for got, want in zip(now.kernels + now.biases, ks + bsx):
            assert np.asarray(got).tobytes() == np.asarray(want).tobytes(), f"member {i} after the second fit"
        f.close()
    assert loss1 == float(np.mean([float(x) for x in last1])) and loss2 == float(np.mean([float(x) for x in last2]))
    k0 = [np.asarray(m.mlp_spec().kernels[0]) for m in model.members]
    assert not np.array_equal(k0[0], k0[1]) and not np.array_equal(k0[1], k0[2])
    pm = model.predict_members(states[:9], actions[:9])
    assert pm.shape == (E, 9, S) and not np.array_equal(pm[0], pm[1])
    assert model.predict(states[:9], actions[:9]).tobytes() == combine(pm, "mean").tobytes()

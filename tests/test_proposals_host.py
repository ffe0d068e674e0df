"""Proposals, the host side, no GPU: the definition (bc_mpc_amd/proposals.py) against a hand-written loop, the
argument checks, the struct's layout against the header, the controllers' refusals (each before a seed is drawn)
and that a controller without the options makes the calls it has always made.  The kernels and the engine calls are
pinned in tests/test_gpu_proposals.py."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO

S, A, H, K = 20, 6, 4, 16
NEW = {"bcmpc_cem_get_action_p": 9, "bcmpc_mppi_get_action_p": 11, "bcmpc_cem_get_actions_batch_p": 12,
       "bcmpc_mppi_get_actions_batch_p": 14, "bcmpc_plan_sample_prop_async": 19, "bcmpc_rollout_policy_batch_async": 10}


# ------------------------------------------------------------------ the definition
def _loop(actions, prop, low, high):
    """The issue's sentence, one element at a time."""
    Hh, Kk, Aa = actions.shape
    P = prop.shape[0]
    out = actions.copy()
    for p in range(P):
        for h in range(Hh):
            for j in range(Aa):
                v = prop[p][h][j]
                out[h, Kk - P + p, j] = low[j] if v < low[j] else (high[j] if v > high[j] else v)
    return out


def _odd(P, Hh, Aa, seed):
    rs = np.random.RandomState(seed)
    p = rs.uniform(-2.0, 2.0, (P, Hh, Aa))
    flat = p.reshape(-1)
    odd = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -1.0])
    flat[rs.choice(flat.size, size=max(1, flat.size // 4), replace=False)] = np.resize(odd, max(1, flat.size // 4))
    return p


@pytest.mark.parametrize("Kk,P,n_elite", [(9, 1, 0), (9, 4, 0), (9, 9, 0), (9, 4, 5), (1, 1, 0), (65, 7, 58)])
def test_inject_is_the_hand_written_loop(Kk, P, n_elite):
    from bc_mpc_amd import proposals as pp
    rs = np.random.RandomState(Kk + P)
    low, high = np.array([-1.0, 0.0, -0.5]), np.array([1.0, 1.0, 0.0])        # bounds of 0.0 on both sides
    acts = rs.uniform(-1, 1, (5, Kk, 3))
    prop = _odd(P, 5, 3, P)
    prop[0, 0] = (-0.0, -0.0, -0.0)                  # -0.0 against low = 0.0 (dim 1) and high = 0.0 (dim 2)
    got = pp.inject(acts, prop, low, high, n_elite)
    want = _loop(acts, prop, low, high)
    assert got.tobytes() == want.tobytes()
    assert got[:, :Kk - P].tobytes() == acts[:, :Kk - P].tobytes()
    assert np.signbit(got[0, Kk - P]).all()          # -0.0 kept, where np.clip answers +0.0
    assert not np.signbit(np.clip(prop[0, 0], low, high)[1])
    assert np.isnan(got[:, Kk - P:]).sum() == np.isnan(prop).sum()
    assert not np.isinf(got).any()


def test_inject_batch_and_the_argument_checks():
    from bc_mpc_amd import proposals as pp
    rs = np.random.RandomState(1)
    B, Kk, P = 3, 9, 2
    low, high = -np.ones(A), np.ones(A)
    acts = rs.uniform(-1, 1, (H, B * Kk, A))
    prop = rs.uniform(-1.5, 1.5, (B, P, H, A))
    got = pp.inject_batch(acts, prop, low, high, B)
    for b in range(B):
        assert got[:, b * Kk:(b + 1) * Kk].tobytes() == _loop(acts[:, b * Kk:(b + 1) * Kk], prop[b], low, high).tobytes()
    for bad, word in ((0, "at least one"), (Kk + 1, "do not fit")):
        with pytest.raises(ValueError, match=word):
            pp.check_count(bad, Kk)
    with pytest.raises(ValueError, match="carried"):
        pp.check_count(P, Kk, Kk - 1)
    assert pp.check_count(P, Kk, Kk - P) == P and pp.check_count(Kk, Kk) == Kk
    for bad in (np.zeros((P, H)), np.zeros((P, H + 1, A)), np.zeros((0, H, A)), np.zeros((B, P, H, A))):
        with pytest.raises(ValueError, match="proposals shape"):
            pp.as_sequences(bad, H, A)
    with pytest.raises(ValueError, match="environments"):
        pp.as_sequences(np.zeros((2, P, H, A)), H, A, 3)
    assert pp.canonical_strides(P, H, A) == (P * H * A, H * A, A)
    assert pp.policy_strides(B, P, A) == (P * A, A, B * P * A)
    pp.check_strides(B, P, H, A, *pp.canonical_strides(P, H, A))
    pp.check_strides(B, P, H, A, *pp.policy_strides(B, P, A))
    pp.check_strides(1, 1, H, A, 0, 0, A)               # (extents of 1 step over nothing)
    for bad in ((P * H * A, H * A, A - 1), (0, H * A, A), (P * H * A, A, A), (-1, H * A, A)):
        with pytest.raises(ValueError, match="alias|>= 0"):
            pp.check_strides(B, P, H, A, *bad)
    # the layouts name the same elements
    flat = np.arange(B * P * H * A, dtype=np.float64)
    canon = flat.reshape(B, P, H, A)
    pol = np.ascontiguousarray(canon.transpose(2, 0, 1, 3)).reshape(-1)
    e, q, t = pp.policy_strides(B, P, A)
    for b, p, h, j in ((0, 0, 0, 0), (2, 1, 3, 5), (1, 0, 2, 4)):
        assert pol[b * e + p * q + h * t + j] == canon[b, p, h, j]


# ------------------------------------------------------------------ bindings
def test_new_symbols_are_bound_and_the_struct_is_the_headers():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    assert lib.bcmpc_abi_version() == 5 == _lib.ABI_VERSION
    bound = {s[0]: s for s in _lib.SIGNATURES}
    for name, nargs in NEW.items():
        assert name in bound
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == bound[name][2]
        assert len(bound[name][2]) == nargs, name
    fields = ["sequences", "count", "device", "env_stride", "seq_stride", "step_stride"]
    assert [f[0] for f in _lib.Proposals._fields_] == fields
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "bcmpc.h"\nint main(void) {\n  printf("%zu", sizeof(bcmpc_proposals));\n'
    src += "".join(f'  printf(" %zu", offsetof(bcmpc_proposals, {f}));\n' for f in fields) + "  return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), c, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [ctypes.sizeof(_lib.Proposals)] + [getattr(_lib.Proposals, f).offset for f in fields]
    assert ctypes.sizeof(_lib.Proposals) == 40


def test_bad_proposals_are_argument_errors_without_hip():
    from bc_mpc_amd import _lib
    lib = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    P = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    st, mu, sd = np.zeros((1, S)), np.zeros((1, H, A)), np.ones((1, H, A))
    seqs = np.zeros((1, 2, H, A))
    out, stats = (_lib.Result * 1)(), (_lib.MppiStats * 1)()
    cem, mppi = _lib.Cem(2, 2, 0.1, 0), _lib.Mppi(1, 1.0, 0)

    def calls(q):
        r = ctypes.byref(q)
        return [lib.bcmpc_cem_get_action_p(None, P(st), ctypes.byref(cem), None, r, 0, P(mu), P(sd), out),
                lib.bcmpc_mppi_get_action_p(None, P(st), ctypes.byref(mppi), None, None, r, 0, P(mu), P(sd), out, stats),
                lib.bcmpc_cem_get_actions_batch_p(None, P(st), 1, ctypes.byref(cem), None, r, 0, 0, P(mu), P(sd), out, None),
                lib.bcmpc_mppi_get_actions_batch_p(None, P(st), 1, ctypes.byref(mppi), None, None, r, 0, 0, P(mu), P(sd),
                                                   out, stats, None)]
    for q, word in ((_lib.Proposals(seqs.ctypes.data, -1, 0, 0, 0, 0), b"count"),
                    (_lib.Proposals(None, 2, 0, 0, 0, 0), b"sequences is NULL"),
                    (_lib.Proposals(seqs.ctypes.data, 2, 7, 0, 0, 0), b"device must be"),
                    (_lib.Proposals(seqs.ctypes.data, 2, 1, 0, -A, A), b"strides must be"),
                    (_lib.Proposals(seqs.ctypes.data, 2, 0, 0, 0, 0), b"null argument")):      # (a good struct: the engine)
        for rc in calls(q):
            assert rc == _lib.ERR_ARG and word in lib.bcmpc_last_error(), (word, lib.bcmpc_last_error())
    # none: the _s / _x entry answers (here: its own null-argument refusal)
    for q in (_lib.Proposals(None, 0, 0, 0, 0, 0),):
        for rc in calls(q):
            assert rc == _lib.ERR_ARG and b"null" in lib.bcmpc_last_error()
    assert lib.bcmpc_plan_sample_prop_async(None, None, None, 1, 4, 0, 0, 0, 0.5, None, None, 0, None, 1, 0, 0, 0, None,
                                            None) == _lib.ERR_ARG
    assert lib.bcmpc_rollout_policy_batch_async(None, None, 1, None, 0, 0, None, None, None, None) == _lib.ERR_ARG


# ------------------------------------------------------------------ the engine methods
class _Recorder:
    """A stand-in for the loaded library: records the symbol every call goes to and answers BCMPC_OK."""

    def __init__(self):
        self.names = []

    def __getattr__(self, name):
        def fn(*args):
            self.names.append(name)
            return 0
        return fn


def _bare_engine(K_total=K):
    from bc_mpc_amd.engine import RolloutEngine
    eng = RolloutEngine.__new__(RolloutEngine)
    eng._lib, eng._h = _Recorder(), None
    eng.state_dim, eng.action_dim, eng.horizon, eng.num_paths = S, A, H, K_total
    return eng


def test_engine_calls_route_by_proposals():
    from bc_mpc_amd.engine import DeviceProposals
    from bc_mpc_amd.ensemble import EnsembleEngine
    eng = _bare_engine(2 * K)
    st, mu, sd = np.zeros(S), np.zeros((H, A)), np.ones((H, A))
    bst, bmu, bsd = np.zeros((2, S)), np.zeros((2, H, A)), np.ones((2, H, A))
    one, two = np.zeros((3, H, A)), np.zeros((2, 3, H, A))
    eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, proposals=None)
    eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, proposals=None)
    eng.cem_get_actions(bst, bmu, bsd, 2, 2, 0.1, 1, proposals=None)
    eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, proposals=None)
    assert eng._lib.names == ["bcmpc_cem_get_action", "bcmpc_mppi_get_action", "bcmpc_cem_get_actions_batch",
                              "bcmpc_mppi_get_actions_batch"]
    eng._lib.names.clear()
    eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, proposals=one)
    eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, rho=0.5, keep_elites=True, proposals=one)
    eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, proposals=one)
    eng.mppi_get_action(st, mu, sd, 1, 1.0, 1, control_cost=1.0, proposals=one)
    eng.cem_get_actions(bst, bmu, bsd, 2, 2, 0.1, 1, proposals=two)
    eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, rho=0.9,
                         proposals=DeviceProposals(4096, 3, 3 * A, A, 2 * 3 * A))
    assert eng._lib.names == ["bcmpc_cem_get_action_p"] * 2 + ["bcmpc_mppi_get_action_p"] * 2 + [
        "bcmpc_cem_get_actions_batch_p", "bcmpc_mppi_get_actions_batch_p"]
    eng._lib.names.clear()
    with pytest.raises(ValueError, match="proposals shape"):
        eng.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, proposals=two)
    with pytest.raises(ValueError, match="environments"):
        eng.cem_get_actions(bst, bmu, bsd, 2, 2, 0.1, 1, proposals=np.zeros((3, 3, H, A)))
    with pytest.raises(ValueError, match="do not fit"):
        eng.mppi_get_actions(bst, bmu, bsd, 1, 1.0, 1, proposals=np.zeros((2, K + 1, H, A)))
    with pytest.raises(ValueError, match="carried"):
        eng.cem_get_actions(bst, bmu, bsd, 2, 4, 0.1, 1, keep_elites=True, proposals=np.zeros((2, K - 3, H, A)))
    with pytest.raises(ValueError, match="alias"):
        eng.cem_get_actions(bst, bmu, bsd, 2, 2, 0.1, 1, proposals=DeviceProposals(4096, 3, 3 * A, A, A))
    assert eng._lib.names == []
    ens = EnsembleEngine.__new__(EnsembleEngine)
    ens._lib, ens._h = _Recorder(), None
    ens.state_dim, ens.action_dim, ens.horizon, ens.num_paths = S, A, H, K
    for call in (lambda: ens.cem_get_action(st, mu, sd, 2, 2, 0.1, 1, proposals=one),
                 lambda: ens.mppi_get_action(st, mu, sd, 1, 1.0, 1, proposals=one)):
        with pytest.raises(NotImplementedError, match="ensembles"):
            call()
    assert ens._lib.names == []


# ------------------------------------------------------------------ controllers
class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32)


class _Env:
    def __init__(self):
        self.observation_space, self.action_space = _Space(S), _Space(A)


def _delta():
    from oracle import mpc_oracle as orc
    return orc.NumpyDynamics(orc.synthetic_weights(S, A, 64, 2, "tanh", False), orc.synthetic_normalization(S, A))


def _reward():
    from oracle import mpc_oracle as orc
    return orc.NumpyRewardDynamics(orc.synthetic_reward_weights(S, A, 64), orc.synthetic_normalization(S, A, reward=True))


def _ensemble():
    from bc_mpc_amd.ensemble import EnsembleDynamicsModel
    from oracle import mpc_oracle as orc
    return EnsembleDynamicsModel(_Env(), 2, 2, 64, "tanh", None, orc.synthetic_normalization(S, A), 32, 3, 1e-3)


def _policy():
    from oracle import mpc_oracle as orc
    return orc.NumpyPolicy(orc.synthetic_policy(S, A, 64, 2))


class _FakeEngine:
    """An engine double: records its constructor arguments and every method call with its keywords."""
    log = []
    refuse_policy = None

    def __init__(self, *args, **kw):
        if kw.get("policy_hidden") and _FakeEngine.refuse_policy:
            raise ValueError(_FakeEngine.refuse_policy)
        self.args, self.kw = args, kw
        self.num_paths, self.action_dim, self.device, self.stream = args[7], args[1], 0, 0
        _FakeEngine.log.append(("create", args, tuple(sorted(kw.items()))))

    def _note(self, name, kw):
        _FakeEngine.log.append((name, tuple(sorted(kw))))

    status_errors = 0           # check_status of a policy engine raises this many times (a team that gave up)

    def set_action_bounds(self, *a): pass
    def set_weights(self, *a): pass
    def set_policy(self, *a): pass
    def close(self): pass

    def check_status(self):
        from bc_mpc_amd import _lib
        if self.kw.get("policy_hidden") and _FakeEngine.status_errors > 0:
            _FakeEngine.status_errors -= 1
            raise _lib.BcmpcError(_lib.ERR_HIP, "team kernel: a workgroup team did not meet")

    def _costs(self, it, B, kw):
        return np.zeros((it, B, self.num_paths // B)) if kw.get("return_costs") else None

    def cem_get_action(self, state, mu, sd, it, ne, alpha, seed, **kw):
        from bc_mpc_amd.engine import StepResult
        self._note("cem_get_action", kw)
        _FakeEngine.log.append(("seed", seed))
        return StepResult(0, 1.0, np.zeros(A)), np.array(mu), np.array(sd)

    def cem_get_actions(self, states, mu, sd, it, ne, alpha, seed, **kw):
        from bc_mpc_amd.engine import BatchResult
        self._note("cem_get_actions", kw)
        _FakeEngine.log.append(("seed", seed))
        B = states.shape[0]
        return BatchResult(np.zeros(B, np.int64), np.ones(B), np.zeros((B, A)), self._costs(it, B, kw)), np.array(mu), np.array(sd)

    def mppi_get_action(self, state, mu, sd, it, temp, seed, **kw):
        from bc_mpc_amd import _lib
        from bc_mpc_amd.engine import StepResult
        self._note("mppi_get_action", kw)
        _FakeEngine.log.append(("seed", seed))
        return StepResult(0, 1.0, np.zeros(A)), np.array(mu), _lib.MppiStats(1.0, 1.0, 1.0, 1)

    def mppi_get_actions(self, states, mu, sd, it, temp, seed, **kw):
        from bc_mpc_amd.engine import MPPI_STATS, BatchResult
        self._note("mppi_get_actions", kw)
        _FakeEngine.log.append(("seed", seed))
        B = states.shape[0]
        return (BatchResult(np.zeros(B, np.int64), np.ones(B), np.zeros((B, A)), self._costs(it, B, kw)), np.array(mu),
                np.zeros(B, MPPI_STATS))


@pytest.fixture
def fake_engines(monkeypatch):
    from bc_mpc_amd import controllers
    _FakeEngine.log, _FakeEngine.refuse_policy, _FakeEngine.status_errors = [], None, 0
    monkeypatch.setattr(controllers, "RolloutEngine", _FakeEngine)
    return _FakeEngine


def _make(cls, model=None, **kw):
    import bc_mpc_amd
    return getattr(bc_mpc_amd, cls)(_Env(), model if model is not None else _delta(), H, bc_mpc_amd.cheetah_cost_fn, K,
                                    seed=5, **kw)


@pytest.mark.parametrize("cls", ["CEMcontroller", "MPPIcontroller"])
def test_a_controller_without_the_options_makes_the_calls_it_made(fake_engines, cls):
    """The same engines, methods, keywords and seed draws as before: the planning engine alone, get_action through
    the single call and get_actions through the batched one with no keyword beyond the sampling / update options."""
    states = np.zeros((2, S))
    for kw in ({}, dict(policy_prior=None, policy_paths=0, policy_stochastic=False, policy_explore=0.5)):
        fake_engines.log = []
        c = _make(cls, **kw)
        c.get_action(states[0])
        c.get_action(states[0], proposals=None)
        c.get_actions(states, proposals=None)
        kind = "cem" if cls.startswith("CEM") else "mppi"
        want = np.random.RandomState(5).randint(0, 2**62, size=3, dtype=np.int64).tolist()
        calls = [e for e in fake_engines.log if e[0] not in ("create", "seed")]
        assert calls == [(f"{kind}_get_action", ()), (f"{kind}_get_action", ()), (f"{kind}_get_actions", ())]
        assert [e[1] for e in fake_engines.log if e[0] == "seed"] == want
        creates = [e for e in fake_engines.log if e[0] == "create"]
        assert len(creates) == 2 and all("policy_hidden" not in dict(e[2]) for e in creates)
        assert c.last_proposal_costs is None and c.last_best_from_proposal is None


def _seed_state(ctrl):
    return ctrl._seed_rng.get_state()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


REFUSALS = [
    # (model, constructor keywords, call keywords, world, exception, message)
    ("delta", {}, dict(proposals=np.zeros((2, H))), 1, ValueError, "proposals shape"),
    ("delta", {}, dict(proposals=np.zeros((K + 1, H, A))), 1, ValueError, "do not fit"),
    ("delta", dict(prior=True, policy_paths=K), dict(proposals=np.zeros((1, H, A))), 1, ValueError, "do not fit"),
    ("ens", {}, dict(proposals=np.zeros((2, H, A))), 1, NotImplementedError, "over an EnsembleDynamicsModel"),
    ("ens", dict(prior=True, policy_paths=2), {}, 1, NotImplementedError, "over an EnsembleDynamicsModel"),
    ("delta", {}, dict(proposals=np.zeros((2, H, A))), 2, NotImplementedError, "one rank|more than one rank"),
    ("delta", dict(prior=True, policy_paths=2), {}, 2, NotImplementedError, "one rank|more than one rank"),
    ("reward", dict(prior=True, policy_paths=2), {}, 1, ValueError, "learned-reward"),
    ("delta", dict(prior=True, policy_paths=2, refuse="policy hidden > 128 is not supported"), {}, 1, ValueError,
     "policy hidden > 128"),
]


@pytest.mark.parametrize("cls", ["CEMcontroller", "MPPIcontroller"])
@pytest.mark.parametrize("model,ckw,kw,world,exc,match", REFUSALS)
def test_refusals_come_before_a_seed_is_drawn(fake_engines, monkeypatch, cls, model, ckw, kw, world, exc, match):
    from bc_mpc_amd import distributed
    if world > 1:
        monkeypatch.setattr(distributed, "world", lambda group=None: (0, world))
    ckw = dict(ckw)
    fake_engines.refuse_policy = ckw.pop("refuse", None)
    if ckw.pop("prior", False):
        ckw["policy_prior"] = _policy()
    c = _make(cls, {"delta": _delta, "reward": _reward, "ens": _ensemble}[model](), **ckw)
    before = _seed_state(c)
    for call, arg in ((c.get_action, np.zeros(S)), (c.get_actions, np.zeros((2, S)))):
        ckw_call = dict(kw)
        if "proposals" in ckw_call and call == c.get_actions:
            ckw_call["proposals"] = np.stack([ckw_call["proposals"]] * 2)
        if model == "ens" and call == c.get_actions:
            continue                                    # (batched planners over an ensemble are refused as ever)
        with pytest.raises(exc, match=match):
            call(arg, **ckw_call)
        assert _same(before, _seed_state(c)), "a refused call drew a seed"
        assert not any(e[0].endswith(("get_action", "get_actions")) for e in fake_engines.log)


@pytest.mark.parametrize("cls", ["CEMcontroller", "MPPIcontroller"])
def test_constructor_checks(cls):
    for kw, word in ((dict(policy_paths=3), "needs a policy_prior"), (dict(policy_prior=_policy(), policy_paths=0), ">= 1"),
                     (dict(policy_prior=_policy(), policy_paths=2, policy_explore=1.5), "policy_explore")):
        with pytest.raises(ValueError, match=word):
            _make(cls, **kw)
    with pytest.raises((ValueError, TypeError, AttributeError)):       # a container policy.extract cannot read
        _make(cls, policy_prior=object(), policy_paths=2)
    c = _make(cls, policy_prior=_policy(), policy_paths=4, policy_stochastic=False, policy_explore=0.25)
    assert (c.policy_paths, c.policy_stochastic, c.policy_explore) == (4, False, 0.25)
    assert c.last_proposal_costs is None and c.last_best_from_proposal is None


@pytest.mark.parametrize("cls", ["CEMcontroller", "MPPIcontroller"])
def test_a_prior_whose_team_gave_up_is_answered_again_on_its_fallback(fake_engines, monkeypatch, cls):
    """The prior engine's status is read after the call; on a give-up the prior runs again with the SAME seed on an
    engine of a kernel that needs no resident team, and the planning call is made again with the same seed."""
    c = _make(cls, policy_prior=_policy(), policy_paths=3)
    rolled = []
    monkeypatch.setattr(c, "_prior_rollout", lambda peng, eng, states, user, pseed: rolled.append((peng, pseed)) or
                        np.zeros((states.shape[0], 3, H, A)))
    want = np.random.RandomState(5).randint(0, 2**62, size=4, dtype=np.int64).tolist()
    c.get_action(np.zeros(S))
    assert [p for _, p in rolled] == [want[1]] and "kernel" not in rolled[0][0].kw
    assert [e[1] for e in fake_engines.log if e[0] == "seed"] == [want[0]]
    assert c.last_proposal_costs.shape == (3,) and c.last_best_from_proposal is False
    fake_engines.status_errors, fake_engines.log = 1, []
    del rolled[:]
    c.get_action(np.zeros(S))
    assert [p for _, p in rolled] == [want[3], want[3]]                      # the same prior seed, twice
    assert rolled[0][0].kw.get("kernel") is None and rolled[1][0].kw["kernel"] == "split2"
    assert [e[1] for e in fake_engines.log if e[0] == "seed"] == [want[2], want[2]]      # ... and the same call
    kind = "cem" if cls.startswith("CEM") else "mppi"
    calls = [e for e in fake_engines.log if e[0].endswith("get_actions")]
    assert len(calls) == 2 and all(e[0] == f"{kind}_get_actions" and "proposals" in e[1] for e in calls)

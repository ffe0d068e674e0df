"""Reference channels and rate terms of a TermCost on the host -- no GPU needed.

cost_functions.TermCost.__call__ and episode_cost (NumPy f64) are THE definition the kernels of csrc/term_cost_x.hip
are tested against; here they are checked against a loop over plain Python floats, whose + - * are the IEEE f64
operations, one at a time.  Equality is np.array_equal(.., equal_nan=True) throughout."""
import numpy as np
import pytest

from bc_mpc_amd import cost_functions as cf

S, A, H, K, R = 6, 3, 5, 40, 4
_CMP = {cf.GE: lambda x, p: x >= p, cf.GT: lambda x, p: x > p, cf.LE: lambda x, p: x <= p, cf.LT: lambda x, p: x < p}


def py_step(T, s, a, ns, r, pa):
    """One step's cost in Python floats: s, a, ns, r, pa are lists of floats (r: the step's reference row)."""
    acc = 0.0
    for t in T.terms:
        x = (s, ns, a)[t.source][t.index]
        p = t.param if t.ref == -1 else r[t.ref]
        if t.kind == cf.THRESHOLD:
            if _CMP[t.cmp](x, p):
                acc = acc + t.weight
        elif t.kind == cf.DIFF:
            acc = acc + t.weight * ((ns[t.index] - x) / t.param)
        elif t.kind == cf.LINEAR:
            acc = acc + t.weight * x
        elif t.kind == cf.RATE:
            d = x - pa[t.index]
            acc = acc + t.weight * (d * d)
        else:
            d = x - p
            acc = acc + t.weight * (d * d)
    return acc


def py_episode(T, states, actions, next_states, ref, prev):
    """episode_cost in Python floats: ref [H, K, R] (or None), prev [K, A] or None."""
    Hn, Kn = actions.shape[:2]
    costs, steps = np.zeros(Kn), np.full(Kn, Hn, dtype=np.int32)
    for k in range(Kn):
        total = 0.0
        for h in range(Hn):
            a = [float(v) for v in actions[h, k]]
            pa = ([float(v) for v in actions[h - 1, k]] if h > 0
                  else a if prev is None else [float(v) for v in prev[k]])
            ns = [float(v) for v in next_states[h, k]]
            r = None if ref is None else [float(v) for v in ref[h, k]]
            total = total + py_step(T, [float(v) for v in states[h, k]], a, ns, r, pa)
            if any(_CMP[c.cmp](ns[c.index], c.param) for c in T.done_conditions):
                total = total + T.done_cost
                steps[k] = h
                break
        costs[k] = total
    return costs, steps


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def tracking_cost(done=False):
    return cf.TermCost(
        [cf.quadratic(0, 2.0, target=cf.ref(0)), cf.quadratic(1, 0.5, target=cf.ref(1), on="next_state"),
         cf.threshold(2, ">=", cf.ref(2), 10.0), cf.threshold(2, ">", cf.ref(2), 7.0),
         cf.threshold(3, "<=", cf.ref(3), 5.0, on="next_state"), cf.threshold(3, "<", cf.ref(3), 3.0, on="next_state"),
         cf.threshold(1, "<=", cf.ref(0), 1.5, on="action"), cf.quadratic(0, 0.1, target=cf.ref(1), on="action"),
         cf.progress(5, 0.01), cf.linear(4, -0.3), cf.quadratic(2, 0.01, on="action"), cf.threshold(0, ">=", 0.2, 4.0)]
        + [cf.rate(j, 0.25 * (j + 1)) for j in range(A)],
        done=[cf.done_when(0, ">", 1.5), cf.done_when(4, "<=", -1.6)] if done else (), done_cost=12.5 if done else 0.0)


def data(seed=0):
    """Trajectory, actions, reference [H, K, R], previous action [K, A]: a third of the entries on shared planted
    values (so the state sits exactly on the referenced thresholds), NaN and +-inf in the reference and the actions."""
    rs = np.random.RandomState(seed)
    traj = rs.standard_normal((H + 1, K, S))
    acts = rs.uniform(-1, 1, (H, K, A))
    ref = rs.standard_normal((H, K, R))
    prev = rs.uniform(-1, 1, (K, A))
    for arr in (traj, acts, ref, prev):
        flat = arr.reshape(-1)
        pos = rs.choice(flat.size, flat.size // 3, replace=False)
        flat[pos] = np.resize([0.2, 0.0, -0.5, 0.25, -0.0], pos.size)
    ref[1, 3, :], ref[2, 4, 0], ref[3, 5, 2], ref[0, 6, 3] = np.nan, np.inf, -np.inf, np.inf
    acts[0, 7, 0], acts[2, 8, 1], acts[H - 1, 9, 2] = np.nan, np.inf, -np.inf
    prev[10, 0], prev[11, 1] = np.nan, np.inf
    traj[:, 12, :] = np.nan
    return traj, acts, ref, prev


# ------------------------------------------------------------------ the definitions against a loop
@pytest.mark.parametrize("done", [False, True])
@pytest.mark.parametrize("with_prev", [False, True])
def test_episode_cost_against_python_floats(done, with_prev):
    T = tracking_cost(done)
    traj, acts, ref, prev = data(1)
    p = prev if with_prev else None
    got = cf.episode_cost(T, traj[:-1], acts, traj[1:], reference=ref, previous_action=p)
    want = py_episode(T, traj[:-1], acts, traj[1:], ref, p)
    same(got[0], want[0])
    same(got[1], want[1])
    assert np.isnan(want[0][3]) and np.isnan(want[0][12]) and np.isfinite(want[0]).sum() > K // 2
    if done:
        assert (want[1] < H).any() and (want[1] == H).any()
    # values sit exactly on the referenced thresholds: >= and > disagree somewhere
    ge = cf.episode_cost(cf.TermCost([cf.threshold(2, ">=", cf.ref(2), 1.0)]), traj[:-1], acts, traj[1:], ref)[0]
    gt = cf.episode_cost(cf.TermCost([cf.threshold(2, ">", cf.ref(2), 1.0)]), traj[:-1], acts, traj[1:], ref)[0]
    assert (ge != gt).any()


def test_step_cost_against_python_floats():
    T = tracking_cost()
    traj, acts, ref, prev = data(2)
    for h in (0, 2):
        got = T(traj[h], acts[h], traj[h + 1], reference=ref[h], previous_action=prev)
        want = [py_step(T, *[[float(v) for v in x[k]] for x in (traj[h], acts[h], traj[h + 1], ref[h], prev)])
                for k in range(K)]
        same(got, np.array(want))
    # one transition (1-D), a [R] reference for a batch, no previous action
    k = 1
    one = T(traj[0, k], acts[0, k], traj[1, k], reference=ref[0, k], previous_action=prev[k])
    assert isinstance(one, float) and one == T(traj[0], acts[0], traj[1], ref[0], prev)[k]
    same(T(traj[0], acts[0], traj[1], reference=ref[0, 0]),
         T(traj[0], acts[0], traj[1], reference=np.tile(ref[0, 0], (K, 1)), previous_action=acts[0]))


def test_reference_and_previous_action_broadcast():
    T = tracking_cost(done=True)
    traj, acts, ref, prev = data(3)
    args = (T, traj[:-1], acts, traj[1:])
    row = ref[0, 0]                                                   # [R] is that row repeated H times
    same(cf.episode_cost(*args, reference=row)[0], cf.episode_cost(*args, reference=np.tile(row, (H, K, 1)))[0])
    per_step = ref[:, :1]                                             # [H, 1, R]: one reference for every candidate
    same(cf.episode_cost(*args, reference=per_step)[0],
         cf.episode_cost(*args, reference=np.repeat(per_step, K, axis=1))[0])
    got = cf.episode_cost(*args, reference=ref)                       # no previous action is previous_action = a_0
    want = cf.episode_cost(*args, reference=ref, previous_action=acts[0])
    same(got[0], want[0])
    same(got[1], want[1])
    same(cf.episode_cost(*args, reference=ref, previous_action=prev[0])[0],
         cf.episode_cost(*args, reference=ref, previous_action=np.tile(prev[0], (K, 1)))[0])
    with pytest.raises(ValueError, match="a reference is needed"):
        cf.episode_cost(*args)
    with pytest.raises(ValueError, match="a reference is needed"):
        T(traj[0], acts[0], traj[1])
    with pytest.raises(ValueError, match="channels"):
        cf.episode_cost(*args, reference=ref[..., :3])
    with pytest.raises(ValueError, match="channels"):
        T(traj[0], acts[0], traj[1], reference=ref[0, :, :2])


def test_constant_reference_is_the_constant_target_cost():
    targets = [0.3, -0.5, 0.2, 0.25]
    def build(v):
        return cf.TermCost([cf.quadratic(0, 2.0, target=v(0)), cf.quadratic(1, 0.5, target=v(1), on="next_state"),
                            cf.threshold(2, ">=", v(2), 10.0), cf.threshold(3, "<", v(3), 3.0, on="next_state"),
                            cf.quadratic(2, 0.01, target=v(0), on="action"), cf.progress(5, 0.01)],
                           done=[cf.done_when(0, ">", 1.5)], done_cost=2.0)
    traj, acts, _, _ = data(4)
    const = cf.episode_cost(build(lambda c: targets[c]), traj[:-1], acts, traj[1:])
    chan = cf.episode_cost(build(cf.ref), traj[:-1], acts, traj[1:], reference=np.tile(targets, (H, K, 1)))
    same(chan[0], const[0])
    same(chan[1], const[1])
    same(cf.episode_cost(build(cf.ref), traj[:-1], acts, traj[1:], reference=targets)[0], const[0])


# ------------------------------------------------------------------ a plain cost is what it was
def test_a_plain_cost_is_unchanged():
    T = cf.cheetah_terms()
    assert repr(T) == ("TermCost([(0, 0, 5, 0, 10.0, 0.2), (0, 0, 6, 0, 10.0, 0.0), (0, 0, 7, 0, 10.0, 0.0), "
                       "(1, 0, 17, 0, -1.0, 0.01)])")
    key = ((0, 0, 5, 0, 10.0, 0.2), (0, 0, 6, 0, 10.0, 0.0), (0, 0, 7, 0, 10.0, 0.0), (1, 0, 17, 0, -1.0, 0.01))
    assert T.key() == key and T.key() is T.terms and hash(T.key()) == hash(key)
    assert all(type(t) is cf.Term and len(t) == 6 for t in T.terms)
    assert T.n_ref == 0 and not T.uses_rate and not T.extended
    D = cf.TermCost([cf.quadratic(1, 0.5, target=0.3), cf.linear(2, 0.1, on="action")],
                    done=[cf.done_when(0, "<=", 0.7)], done_cost=-0.0)
    assert repr(D) == ("TermCost([(3, 0, 1, 0, 0.5, 0.3), (2, 2, 2, 0, 0.1, 0.0)], done=[(0, 1, 0, 2, 0.0, 0.7)], "
                       "done_cost=-0.0)")
    assert D.key() == (((3, 0, 1, 0, 0.5, 0.3), (2, 2, 2, 0, 0.1, 0.0)), ((0, 1, 0, 2, 0.0, 0.7),), "-0x0.0p+0")
    assert not D.extended
    # positional 6-tuples are still accepted, and equal the builders' terms
    P = cf.TermCost([(3, 0, 1, 0, 0.5, 0.3), (2, 2, 2, 0, 0.1, 0.0)], done=[(0, 1, 0, 2, 0.0, 0.7)], done_cost=-0.0)
    assert P.key() == D.key() and hash(P.key()) == hash(D.key()) and P.terms == D.terms
    assert cf.Term(3, 0, 1, 0, 0.5, 0.3) == (3, 0, 1, 0, 0.5, 0.3)
    # an extended term carries its channel as a seventh entry, so its key differs from the constant's
    X = cf.TermCost([cf.quadratic(1, 0.5, target=cf.ref(2))])
    assert X.terms == ((3, 0, 1, 0, 0.5, 0.0, 2),) and X.n_ref == 3 and X.extended
    assert X.key() != cf.TermCost([cf.quadratic(1, 0.5, target=0.0)]).key()
    assert cf.TermCost([(3, 0, 1, 0, 0.5, 0.0, 2)]).key() == X.key()
    assert cf.rate(1, 0.5) == (cf.RATE, cf.ACTION, 1, 0, 0.5, 0.0) and cf.TermCost([cf.rate(1, 0.5)]).extended


# ------------------------------------------------------------------ validation
def test_validation():
    for build in (lambda: cf.progress(0, cf.ref(0)), lambda: cf.linear(0, cf.ref(0)),
                  lambda: cf.done_when(0, ">", cf.ref(0)), lambda: cf.rate(0, cf.ref(0))):
        with pytest.raises(ValueError, match="constant"):
            build()
    for bad in (16, 17, -1, 1.5):
        with pytest.raises(ValueError, match="channel"):
            cf.ref(bad)
    # hand-made tuples pass the same checks
    for t in ((cf.DIFF, 0, 0, 0, 1.0, 0.01, 0), (cf.LINEAR, 0, 0, 0, 1.0, 0.0, 0), (cf.RATE, 2, 0, 0, 1.0, 0.0, 0),
              (cf.QUADRATIC, 0, 0, 0, 1.0, 0.0, 16), (cf.QUADRATIC, 0, 0, 0, 1.0, 0.0, -2), (cf.RATE, 0, 0, 0, 1.0, 0.0)):
        with pytest.raises(ValueError):
            cf.TermCost([t])
    with pytest.raises(ValueError, match="done condition"):
        cf.TermCost([], done=[(0, 1, 0, 0, 0.0, 0.5, 1)])
    # the slot budget: 16 (dim, channel) pairs are 32 slots; one more action, or a condition on a new dim, is 33
    quads = [cf.quadratic(i, 1.0, target=cf.ref(i)) for i in range(16)]
    assert cf.TermCost(quads, done=[cf.done_when(3, ">", 5.0)]).n_slots == 32
    with pytest.raises(ValueError, match="at most 32 slots"):
        cf.TermCost(quads + [cf.rate(0, 1.0)])
    with pytest.raises(ValueError, match="at most 32 slots"):
        cf.TermCost(quads, done=[cf.done_when(19, ">", 5.0)])
    # rate indices are the action's
    T = cf.TermCost([cf.rate(2, 1.0), cf.quadratic(5, 1.0, target=cf.ref(0))])
    T.validate(6, 3)
    with pytest.raises(ValueError, match=r"term 0: index 2 outside \[0, 2\)"):
        T.validate(6, 2)
    with pytest.raises(ValueError, match=r"term 1: index 5 outside \[0, 5\)"):
        T.validate(5, 3)
    with pytest.raises(ValueError, match="negative index"):
        cf.TermCost([cf.rate(-1, 1.0)])
    assert cf.TermCost([cf.rate(0, 1.0), cf.quadratic(0, 1.0, target=cf.ref(3))]).n_ref == 4


# ------------------------------------------------------------------ controller refusals
CS, CA, CH, CK = 20, 6, 3, 8


class _Space:
    def __init__(self, n):
        self.shape = (n,)
        self.low, self.high = -np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32)


class _Env:
    def __init__(self):
        self.observation_space, self.action_space = _Space(CS), _Space(CA)


def _delta():
    from oracle import mpc_oracle as orc
    return orc.NumpyDynamics(orc.synthetic_weights(CS, CA, 64, 2, "tanh", False), orc.synthetic_normalization(CS, CA))


def _callable(s, a, ns):
    return np.zeros(s.shape[0])


COSTS = {
    "chan": lambda: cf.TermCost([cf.quadratic(0, 1.0, target=cf.ref(1)), cf.rate(0, 0.1)]),
    "chan_only": lambda: cf.TermCost([cf.quadratic(0, 1.0, target=cf.ref(1))]),
    "rate_only": lambda: cf.TermCost([cf.rate(0, 0.1)]),
    "plain": lambda: cf.TermCost([cf.linear(2, 0.1, on="action")]),
    "cheetah": lambda: __import__("bc_mpc_amd").cheetah_cost_fn,
    "callable": lambda: _callable,
}
GA, GAS = "get_action", "get_actions"
REFUSALS = [
    # (call, cost, keywords, message)
    (GA, "chan", {}, "pass reference="),
    (GAS, "chan", {}, "pass reference="),
    (GA, "plain", dict(reference=np.zeros(2)), "names no channel"),
    (GA, "cheetah", dict(reference=np.zeros(2)), "names no channel"),
    (GA, "callable", dict(reference=np.zeros(2)), "names no channel"),
    (GA, "rate_only", dict(reference=np.zeros(2)), "names no channel"),
    (GAS, "plain", dict(reference=np.zeros((2, 2))), "names no channel"),
    (GA, "chan", dict(reference=np.zeros(1)), "the reference has 1 channels, the cost names 2"),
    (GA, "chan", dict(reference=np.zeros((CH + 1, 2))), "reference must be"),
    (GA, "chan", dict(reference=np.zeros((2, CH, 2))), "reference must be"),
    (GA, "chan", dict(reference=np.float64(1.0)), "reference must be"),
    (GAS, "chan", dict(reference=np.zeros(2)), "reference must be"),
    (GAS, "chan", dict(reference=np.zeros((2, CH + 1, 2))), "reference must be"),
    (GAS, "chan", dict(reference=np.zeros((2, 1))), "the reference has 1 channels"),
    (GAS, "chan", dict(reference=np.zeros((3, 2))), "reference is for 3 environments, states for 2"),
    (GAS, "chan", dict(reference=np.zeros((2, 2)), previous_action=np.zeros((3, CA))), "previous_action is for 3"),
    (GA, "chan_only", dict(reference=np.zeros(2), previous_action=np.zeros(CA)), "needs a TermCost with rate terms"),
    (GA, "plain", dict(previous_action=np.zeros(CA)), "needs a TermCost with rate terms"),
    (GA, "cheetah", dict(previous_action=np.zeros(CA)), "needs a TermCost with rate terms"),
    (GA, "chan", dict(reference=np.zeros(2), previous_action=np.zeros(CA + 1)), "previous_action must be"),
    (GA, "chan", dict(reference=np.zeros(2), previous_action=np.zeros((1, CA))), "previous_action must be"),
    (GAS, "rate_only", dict(previous_action=np.zeros(CA)), "previous_action must be"),
]


@pytest.fixture
def no_engines(monkeypatch):
    """No refusal may get as far as constructing an engine."""
    from bc_mpc_amd import cem, controllers, ensemble, mppi

    def boom(*a, **k):
        raise AssertionError("a refused call constructed an engine")
    for mod, name in ((controllers, "RolloutEngine"), (cem, "RolloutEngine"), (mppi, "RolloutEngine"),
                      (ensemble, "EnsembleEngine")):
        if hasattr(mod, name):
            monkeypatch.setattr(mod, name, boom)


@pytest.mark.parametrize("cls", ["MPCcontroller", "CEMcontroller", "MPPIcontroller"])
@pytest.mark.parametrize("call,cost,kw,match", REFUSALS,
                         ids=[f"{c}-{k}-{i}" for i, (c, k, _, _) in enumerate(REFUSALS)])
def test_controller_refusals(no_engines, cls, call, cost, kw, match):
    import bc_mpc_amd
    extra = dict(rng="device") if cls == "MPCcontroller" else {}
    ctrl = getattr(bc_mpc_amd, cls)(_Env(), _delta(), CH, COSTS[cost](), CK, seed=1, **extra)
    arg = np.zeros(CS) if call == GA else np.zeros((2, CS))
    np.random.seed(77)
    seed_rng = ctrl._seed_rng.get_state()
    before = np.random.get_state()
    for _ in range(2):
        with pytest.raises(ValueError, match=match):
            getattr(ctrl, call)(arg, **kw)
    assert ctrl._engine is None and getattr(ctrl, "_batch_engine", None) is None
    assert not ctrl.__dict__.get("_engines") and not ctrl.__dict__.get("_ens_engines")
    for a, b in ((seed_rng, ctrl._seed_rng.get_state()), (before, np.random.get_state())):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "a refused call drew from a random stream"


def test_numpy_rng_controller_refuses_before_its_draw(no_engines):
    import bc_mpc_amd
    ctrl = bc_mpc_amd.MPCcontroller(_Env(), _delta(), CH, COSTS["chan"](), CK)      # rng="numpy"
    np.random.seed(5)
    before = np.random.get_state()
    with pytest.raises(ValueError, match="pass reference="):
        ctrl.get_action(np.zeros(CS))
    with pytest.raises(ValueError, match="names no channel"):
        bc_mpc_amd.MPCcontroller(_Env(), _delta(), CH, _callable, CK).get_action(np.zeros(CS), reference=np.zeros(2))
    assert all(np.array_equal(x, y) for x, y in zip(before, np.random.get_state()))


def test_pinned_refusals_stay(no_engines, monkeypatch):
    """The inputs do not open what is refused today: multi-rank CEM with a TermCost, MPPI on several ranks."""
    import bc_mpc_amd
    from bc_mpc_amd import distributed
    monkeypatch.setattr(distributed, "world", lambda group=None: (0, 2))
    kw = dict(reference=np.zeros(2), previous_action=np.zeros(CA))
    with pytest.raises(NotImplementedError):
        bc_mpc_amd.MPPIcontroller(_Env(), _delta(), CH, COSTS["chan"](), CK, seed=1).get_action(np.zeros(CS), **kw)
    with pytest.raises(NotImplementedError, match="multi-rank CEM with a TermCost"):
        bc_mpc_amd.CEMcontroller(_Env(), _delta(), CH, COSTS["chan"](), CK, seed=1).get_action(np.zeros(CS), **kw)

"""Cost-function objects with the reference's API (cost_functions.py:9-63).

``MPCcontroller`` receives ``cost_fn`` as an argument (controllers.py:32) and
the driver passes ``cost_functions.cheetah_cost_fn`` (train_mpc_ppo.py:515).
The rollout engine fuses that cost into the HIP kernel; these NumPy callables
exist so user code can keep importing and passing them, and so a caller can
score a trajectory the engine returns in trajectory mode.  ``is_cheetah_cost``
decides whether a given callable may be fused.
"""
from __future__ import annotations

import contextlib

import numpy as np


def cheetah_cost_fn(state, action, next_state):
    """cost_functions.py:9-52: heading penalties (+10 each) minus torso progress / 0.01."""
    if len(state.shape) > 1:
        heading_penalty_factor = 10
        scores = np.zeros((state.shape[0],))
        scores[state[:, 5] >= 0.2] += heading_penalty_factor
        scores[state[:, 6] >= 0] += heading_penalty_factor
        scores[state[:, 7] >= 0] += heading_penalty_factor
        scores -= (next_state[:, 17] - state[:, 17]) / 0.01
        return scores
    heading_penalty_factor = 10
    score = 0
    if state[5] >= 0.2:
        score += heading_penalty_factor
    if state[6] >= 0:
        score += heading_penalty_factor
    if state[7] >= 0:
        score += heading_penalty_factor
    score -= (next_state[17] - state[17]) / 0.01
    return score


cheetah_cost_fn.__bcmpc_fused__ = "cheetah"


def trajectory_cost_fn(cost_fn, states, actions, next_states):
    """cost_functions.py:59-63: sum of per-step costs over the horizon."""
    trajectory_cost = 0
    for i in range(len(actions)):
        trajectory_cost += cost_fn(states[i], actions[i], next_states[i])
    return trajectory_cost


# ---------------------------------------------------------------- declarative costs ("terms")
# The engine cannot run Python, so a cost other than the cheetah's reaches the device as a list of terms
# (include/bcmpc.h bcmpc_cost_term, csrc/term_cost.hip).  The per-step cost of (s, a, s') is acc = 0.0, then
# for each term in list order
#   threshold  if x cmp value: acc = acc + weight        (NaN compares false)
#   progress   acc = acc + weight * ((s'[index] - s[index]) / dt)
#   linear     acc = acc + weight * x
#   quadratic  d = x - target; acc = acc + weight * (d * d)
#   rate       d = a_h[index] - a_{h-1}[index]; acc = acc + weight * (d * d)
# every operation one IEEE f64 operation.  A threshold's value and a quadratic's target may be ``ref(c)``:
# channel c of the reference the CALL carries (row h of it at step h), read in place of the constant.
# TermCost.__call__ below IS that definition (NumPy f64, elementwise, term order); the kernels are tested
# against it bit for bit.
THRESHOLD, DIFF, LINEAR, QUADRATIC, RATE = range(5)
STATE, NEXT_STATE, ACTION = range(3)
GE, GT, LE, LT = range(4)
MAX_TERMS = 32
MAX_SLOTS = 32      # what the kernel loads per row: the state dims, the actions and the channels the entries name
MAX_REF = 16        # channels of a call's reference
_SOURCES = {"state": STATE, "next_state": NEXT_STATE, "action": ACTION}
_CMPS = {">=": GE, ">": GT, "<=": LE, "<": LT}
_CMP_FN = {GE: np.greater_equal, GT: np.greater, LE: np.less_equal, LT: np.less}


class Ref:
    """``ref(c)``: channel c of the call's reference, where a threshold's value or a quadratic's target stands."""
    __slots__ = ("channel",)

    def __init__(self, channel):
        c = int(channel)
        if c != channel or c < 0 or c >= MAX_REF:
            raise ValueError(f"a reference channel must be an integer in [0, {MAX_REF}), not {channel!r}")
        self.channel = c

    def __repr__(self):
        return f"ref({self.channel})"


def ref(channel) -> Ref:
    """Placeholder for "channel ``channel`` of the call's reference": ``threshold(i, op, ref(c), w)`` and
    ``quadratic(i, w, target=ref(c))`` read ``reference[h][c]`` at step h, whatever their ``on=``."""
    return Ref(channel)


def _no_ref(what, v):
    if isinstance(v, Ref):
        raise ValueError(f"{what} takes a constant: a reference channel stands only for a threshold's value or a "
                         "quadratic's target")
    return v


class Term(tuple):
    """One term: ``(kind, source, index, cmp, weight, param)`` (bcmpc_cost_term's fields); a term whose param is
    a reference channel has the channel as a seventh entry (bcmpc_cost_term_x's ``ref``)."""
    __slots__ = ()

    def __new__(cls, kind, source, index, cmp, weight, param, ref=-1):
        t = (int(kind), int(source), int(index), int(cmp), float(weight), float(param))
        return super().__new__(cls, t if ref == -1 else t + (int(ref),))

    kind = property(lambda self: self[0])
    source = property(lambda self: self[1])
    index = property(lambda self: self[2])
    cmp = property(lambda self: self[3])
    weight = property(lambda self: self[4])
    param = property(lambda self: self[5])
    ref = property(lambda self: self[6] if len(self) > 6 else -1)


def _source(on) -> int:
    if on not in _SOURCES:
        raise ValueError(f"on must be one of {sorted(_SOURCES)}, not {on!r}")
    return _SOURCES[on]


def threshold(index, op, value, weight, on="state") -> Term:
    """``+ weight`` where ``x op value`` (op one of ``>=  >  <=  <``); nothing where it is false or NaN."""
    if op not in _CMPS:
        raise ValueError(f"op must be one of {sorted(_CMPS)}, not {op!r}")
    if isinstance(value, Ref):
        return Term(THRESHOLD, _source(on), index, _CMPS[op], weight, 0.0, value.channel)
    return Term(THRESHOLD, _source(on), index, _CMPS[op], weight, value)


def progress(index, dt, weight=-1.0) -> Term:
    """``+ weight * ((next_state[index] - state[index]) / dt)``: with the default weight, forward velocity
    along ``index`` is rewarded (``cheetah_cost_fn``'s last line is ``progress(17, 0.01)``)."""
    return Term(DIFF, STATE, index, GE, _no_ref("progress", weight), _no_ref("progress", dt))


def linear(index, weight, on="state") -> Term:
    """``+ weight * x``."""
    return Term(LINEAR, _source(on), index, GE, _no_ref("linear", weight), 0.0)


def quadratic(index, weight, target=0.0, on="state") -> Term:
    """``+ weight * (x - target)**2`` (``on="action"``, target 0: one summand of ``weight * sum(a**2)``)."""
    if isinstance(target, Ref):
        return Term(QUADRATIC, _source(on), index, GE, weight, 0.0, target.channel)
    return Term(QUADRATIC, _source(on), index, GE, weight, target)


def rate(index, weight) -> Term:
    """``+ weight * (a_h[index] - a_{h-1}[index])**2``, the action-rate penalty.  ``a_{-1}`` is the call's
    ``previous_action``; a call without one takes ``a_{-1} := a_0``."""
    return Term(RATE, ACTION, index, GE, _no_ref("rate", weight), 0.0)


def done_when(index, op, value) -> Term:
    """A done condition: the episode ends at the step whose NEXT state has ``next_state[index] op value`` (op one
    of ``>=  >  <=  <``; a NaN compares false).  ``TermCost(terms, done=[...])`` combines its conditions with OR:
    Hopper's ``not healthy`` is ``done_when(0, "<=", 0.7), done_when(1, ">=", 0.2), done_when(1, "<=", -0.2)``."""
    if op not in _CMPS:
        raise ValueError(f"op must be one of {sorted(_CMPS)}, not {op!r}")
    return Term(THRESHOLD, NEXT_STATE, index, _CMPS[op], 0.0, _no_ref("done_when", value))


class TermCost:
    """A cost built from terms, with the reference's ``cost_fn(state, action, next_state)`` signature for
    1-D (one transition) and 2-D (a batch, one row each) inputs.  Passed as ``cost_fn`` to MPCcontroller,
    CEMcontroller or MPPIcontroller it is evaluated on the device (``RolloutEngine(cost="terms")``) for any
    state size; called, it evaluates the same expressions in NumPy f64 -- the definition the kernel is
    tested against.  Minimised; weights may be negative.

    ``done``: conditions built by ``done_when`` that end a candidate's episode, ``done_cost``: a finite cost
    added once at the terminating step.  Neither changes ``__call__`` (the per-step cost); ``episode_cost`` is the
    definition of what the planners then minimise.  Terms plus conditions are at most 32.

    A cost with ``ref(c)`` values or ``rate`` terms takes the call's ``reference`` / ``previous_action``
    (``__call__``, ``episode_cost``, the controllers' keywords); what its entries read per row -- state dims,
    actions and channels, each counted once -- is at most 32 slots."""

    def __init__(self, terms=(), done=(), done_cost=0.0):
        self.terms = tuple(t if isinstance(t, Term) else Term(*t) for t in terms)
        self.done_conditions = tuple(t if isinstance(t, Term) else Term(*t) for t in done)
        self.done_cost = float(done_cost)
        if len(self.terms) > MAX_TERMS:
            raise ValueError(f"a TermCost holds at most {MAX_TERMS} terms, got {len(self.terms)}")
        if len(self.terms) + len(self.done_conditions) > MAX_TERMS:
            raise ValueError(f"a TermCost holds at most {MAX_TERMS} terms and done conditions together, got "
                             f"{len(self.terms)} + {len(self.done_conditions)}")
        if not np.isfinite(self.done_cost):
            raise ValueError("done_cost must be finite")
        for i, t in enumerate(self.done_conditions):
            if t.kind != THRESHOLD or t.source != NEXT_STATE or t.cmp not in (GE, GT, LE, LT):
                raise ValueError(f"done condition {i}: not a done_when(index, op, value) condition")
            if t.ref != -1:
                raise ValueError(f"done condition {i}: a done condition compares with a constant, not a reference "
                                 "channel")
            if t.index < 0:
                raise ValueError(f"done condition {i}: negative index {t.index}")
            if not np.isfinite(t.param) or t.weight != 0.0:
                raise ValueError(f"done condition {i}: the value must be finite (and the weight 0)")
        for i, t in enumerate(self.terms):
            if t.kind not in (THRESHOLD, DIFF, LINEAR, QUADRATIC, RATE):
                raise ValueError(f"term {i}: unknown kind {t.kind}")
            if t.source not in (STATE, NEXT_STATE, ACTION):
                raise ValueError(f"term {i}: unknown source {t.source}")
            if t.kind == THRESHOLD and t.cmp not in (GE, GT, LE, LT):
                raise ValueError(f"term {i}: unknown cmp {t.cmp}")
            if t.kind == DIFF and t.source != STATE:
                raise ValueError(f"term {i}: a progress term reads the state")
            if t.index < 0:
                raise ValueError(f"term {i}: negative index {t.index}")
            if not (np.isfinite(t.weight) and np.isfinite(t.param)):
                raise ValueError(f"term {i}: weight and param must be finite")
            if t.kind == DIFF and t.param == 0.0:
                raise ValueError(f"term {i}: a progress term's dt must not be 0")
            if t.kind == RATE and t.source != ACTION:
                raise ValueError(f"term {i}: a rate term reads the action")
            if t.ref != -1:
                if t.kind not in (THRESHOLD, QUADRATIC):
                    raise ValueError(f"term {i}: a reference channel stands only for a threshold's value or a "
                                     "quadratic's target")
                if t.ref < 0 or t.ref >= MAX_REF:
                    raise ValueError(f"term {i}: reference channel {t.ref} outside [0, {MAX_REF})")
        self.n_ref = 1 + max((t.ref for t in self.terms), default=-1)
        self.uses_rate = any(t.kind == RATE for t in self.terms)
        entries = self.terms + self.done_conditions
        self.n_slots = (len({t.index for t in entries if t.source != ACTION}) +
                        len({t.index for t in entries if t.source == ACTION}) +
                        len({t.ref for t in self.terms if t.ref != -1}))
        if self.n_slots > MAX_SLOTS:
            raise ValueError(f"a TermCost reads at most {MAX_SLOTS} slots per row (state dims, actions and reference "
                             f"channels, each counted once), this one needs {self.n_slots}")

    @property
    def extended(self) -> bool:
        """Whether the cost names a reference channel or has a rate term (the engine then takes it through
        bcmpc_set_cost_terms_x and scores it with the kernel instances of csrc/term_cost_x.hip)."""
        return self.n_ref > 0 or self.uses_rate

    def key(self):
        """What identifies the cost: the terms alone without ``done`` (as before there was one), else also the
        conditions and ``done_cost`` (by its bits: -0.0 is not 0.0)."""
        if not self.done_conditions:
            return self.terms
        return (self.terms, self.done_conditions, self.done_cost.hex())

    def validate(self, state_dim: int, action_dim: int) -> None:
        """Every index inside the state / the action of this task (the engine checks the same)."""
        for i, t in enumerate(self.terms):
            lim = action_dim if t.source == ACTION else state_dim
            if t.index >= lim:
                raise ValueError(f"term {i}: index {t.index} outside [0, {lim})")
        for i, t in enumerate(self.done_conditions):
            if t.index >= state_dim:
                raise ValueError(f"done condition {i}: index {t.index} outside [0, {state_dim})")

    def done(self, next_state):
        """Whether the episode ends on reaching ``next_state`` (``[..., S]`` -> bool ``[...]``): the OR of the
        conditions, a NaN comparing false; all False without conditions."""
        ns = np.asarray(next_state, dtype=np.float64)
        out = np.zeros(ns.shape[:-1], dtype=bool)
        with np.errstate(invalid="ignore"):
            for t in self.done_conditions:
                out = out | _CMP_FN[t.cmp](ns[..., t.index], t.param)
        return out

    def __len__(self):
        return len(self.terms)

    def __repr__(self):
        if not self.done_conditions:
            return f"TermCost({list(map(tuple, self.terms))})"
        return (f"TermCost({list(map(tuple, self.terms))}, done={list(map(tuple, self.done_conditions))}, "
                f"done_cost={self.done_cost!r})")

    def _reference(self, reference, batch):
        """``reference`` broadcast to ``batch + (R,)``, or None for a cost that names no channel."""
        if self.n_ref == 0:
            return None
        if reference is None:
            raise ValueError(f"the cost names reference channels (n_ref = {self.n_ref}): a reference is needed")
        r = np.asarray(reference, dtype=np.float64)
        if r.ndim < 1 or r.shape[-1] < self.n_ref:
            raise ValueError(f"the reference has {r.shape[-1] if r.ndim else 0} channels, the cost names "
                             f"{self.n_ref}")
        return np.broadcast_to(r, tuple(batch) + (r.shape[-1],))

    def __call__(self, state, action, next_state, reference=None, previous_action=None):
        """The per-step cost.  ``reference``: broadcastable to ``[..., R]`` (needed when the cost names a channel);
        ``previous_action``: broadcastable to ``[..., A]``, the ``a_{h-1}`` of the rate terms (None: ``action``)."""
        s, a, ns = (np.asarray(x, dtype=np.float64) for x in (state, action, next_state))
        src = (s, ns, a)
        r = self._reference(reference, s.shape[:-1])
        pa = a if previous_action is None else np.broadcast_to(np.asarray(previous_action, dtype=np.float64), a.shape)
        acc = np.zeros(s.shape[:-1])
        # (a non-finite reference or action is legal data; a plain cost warns as it always did)
        with np.errstate(invalid="ignore", over="ignore") if self.extended else contextlib.nullcontext():
            for t in self.terms:
                x = src[t.source][..., t.index]
                p = t.param if t.ref == -1 else r[..., t.ref]
                if t.kind == THRESHOLD:
                    acc = np.where(_CMP_FN[t.cmp](x, p), acc + t.weight, acc)
                elif t.kind == DIFF:
                    acc = acc + t.weight * ((ns[..., t.index] - x) / t.param)
                elif t.kind == LINEAR:
                    acc = acc + t.weight * x
                elif t.kind == RATE:
                    d = x - pa[..., t.index]
                    acc = acc + t.weight * (d * d)
                else:
                    d = x - p
                    acc = acc + t.weight * (d * d)
        return acc if acc.ndim else float(acc)


def episode_cost(term_cost, states, actions, next_states, reference=None, previous_action=None):
    """THE definition of a ``TermCost`` over a horizon (csrc/term_cost.hip and csrc/term_cost_x.hip are tested
    against it bit for bit): ``states`` / ``next_states`` ``[H, K, S]``, ``actions`` ``[H, K, A]`` ->
    ``(costs [K] f64, term_step [K] int32)``.  For every candidate

        total = 0.0; t = H
        for h in 0 .. H-1:
            total = total + c_h                      # the terminating step is still paid, as gym pays it
            if term_cost.done(next_states[h]):  total = total + done_cost; t = h; break

    each operation one f64 operation in this order.  ``t == H`` exactly where the candidate never terminated.
    Without conditions this is ``trajectory_cost_fn(term_cost, ...)`` bit for bit and ``t == H`` everywhere.

    ``reference``: broadcastable to ``[H, K, R]`` -- step h reads row h, so ``[R]`` is that row repeated H times.
    ``previous_action``: broadcastable to ``[K, A]``, the rate terms' ``a_{-1}`` (None: ``actions[0]``); step h's
    ``a_{h-1}`` is ``actions[h-1]``."""
    H = len(actions)
    shape = np.shape(states)[1:-1]
    total = np.zeros(shape, dtype=np.float64)
    step = np.full(shape, H, dtype=np.int32)
    alive = np.ones(shape, dtype=bool)
    dc = np.float64(term_cost.done_cost)
    ref_rows = term_cost._reference(reference, (H,) + tuple(shape))
    acts = np.asarray(actions, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(H):
            if ref_rows is None and not term_cost.uses_rate:
                c = term_cost(states[h], actions[h], next_states[h])
            else:
                prev = acts[h - 1] if h > 0 else (acts[0] if previous_action is None else previous_action)
                c = term_cost(states[h], acts[h], next_states[h], None if ref_rows is None else ref_rows[h], prev)
            total = np.where(alive, total + c, total)
            d = alive & term_cost.done(next_states[h])
            total = np.where(d, total + dc, total)
            step = np.where(d, np.int32(h), step).astype(np.int32)
            alive = alive & ~d
    return total, step


def cheetah_terms() -> TermCost:
    """``cheetah_cost_fn`` as terms, bit for bit: ``acc + (-1.0 * q)`` is ``acc - q``."""
    return TermCost([threshold(5, ">=", 0.2, 10.0), threshold(6, ">=", 0.0, 10.0), threshold(7, ">=", 0.0, 10.0),
                     progress(17, 0.01, -1.0)])


_PROBED: dict = {}     # (cost_fn, state_dim, action_dim) -> verdict of the probe below


def is_cheetah_cost(cost_fn, state_dim: int = 20, action_dim: int = 6) -> bool:
    """True when ``cost_fn`` computes exactly cost_functions.cheetah_cost_fn.

    Our own function is recognised by its marker.  Any other callable named
    ``cheetah_cost_fn`` (e.g. the reference module's) must also reproduce the
    fused formula bit-for-bit on a probe batch that straddles every threshold.
    """
    if getattr(cost_fn, "__bcmpc_fused__", None) == "cheetah":
        return True
    if getattr(cost_fn, "__name__", "") != "cheetah_cost_fn" or state_dim < 18:
        return False
    try:
        return _PROBED[(cost_fn, state_dim, action_dim)]    # probed once per function (every env step asks)
    except (KeyError, TypeError):
        pass
    verdict = _probe(cost_fn, state_dim, action_dim)
    try:
        _PROBED[(cost_fn, state_dim, action_dim)] = verdict
    except TypeError:                                       # unhashable callable
        pass
    return verdict


def _probe(cost_fn, state_dim: int, action_dim: int) -> bool:
    rs = np.random.RandomState(20240601)
    s = rs.standard_normal((64, state_dim)) * 0.3
    s[:8, 5] = 0.2
    s[8:16, 6] = 0.0
    s[16:24, 7] = 0.0
    ns = s + rs.standard_normal((64, state_dim)) * 0.01
    a = rs.uniform(-1, 1, (64, action_dim))
    try:
        got = np.asarray(cost_fn(s, a, ns), dtype=np.float64)
    except Exception:
        return False
    want = cheetah_cost_fn(s, a, ns)
    return got.shape == want.shape and bool(np.array_equal(got, want))

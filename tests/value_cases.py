"""Shared cases of the terminal-value tests (test_terminal_value_host.py checks the definition on them,
test_gpu_terminal_value.py the kernel): nets, hand-made states and the reference figures of one case, computed
once per process and never modified.

A case is (S, hidden, L) over every K of KS.  The critic: normc-style kernels (N(0, 1) / sqrt(fan_in), so
pre-activations are O(1) and tanh is exercised on both of its branches), biases and an observation filter
with means and stds away from 0 and 1.  The states: N(0, 1) scaled into the filter's range, with planted rows
(K permitting): a NaN dimension, +inf, -inf, a value far beyond the clip, values landing exactly on +-5.
"""
import functools

import numpy as np

KS = (1, 15, 16, 17, 63, 64, 65, 400)
SS = (3, 17, 20, 32)
HIDDENS = (1, 16, 100, 128, 256)
LS = (1, 2, 4)
CASES = [(S, h, L) for S in SS for h in HIDDENS for L in LS]
RMS_FACTOR = 4.0            # bar (b): RMS(v - v_f64) <= 4 x RMS(v_seq32 - v_f64), cases with K >= 64


def make_spec(S, hidden, L, seed=0):
    from bc_mpc_amd.value import ValueSpec
    rs = np.random.RandomState(10000 * S + 10 * hidden + L + 7919 * seed)
    dims = [S] + [hidden] * L + [1]
    ks = [(rs.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L + 1)]
    bs = [(0.1 * rs.standard_normal(dims[i + 1])).astype(np.float32) for i in range(L + 1)]
    mean = rs.uniform(-0.5, 0.5, S).astype(np.float32)
    std = rs.uniform(0.5, 2.0, S).astype(np.float32)
    mean[0], std[0] = 0.0, 1.0                      # dim 0: obz == f32(state), so +-5 can be hit exactly
    return ValueSpec(ks, bs, mean, std)


def make_states(S, K, seed=0):
    rs = np.random.RandomState(1000 * K + S + 31 * seed)
    s = rs.standard_normal((K, S)) * 1.5
    if K == 1:
        s[0, S - 1] = 1e6                            # far beyond the clip
    if K >= 15:
        s[1, S // 2] = np.nan
        s[2, 0] = np.inf
        s[3, S - 1] = -np.inf
        s[4, S - 1] = -1e300                         # -> -inf in f32 -> -5
        s[5, 0], s[6, 0] = 5.0, -5.0                 # exactly on the clip
        s[7, 0], s[8, 0] = np.nextafter(np.float32(5), np.float32(6)), np.nextafter(np.float32(-5), np.float32(-6))
        s[9, :] = np.nan
    return s


class Case:
    """One (S, hidden, L, K): states, the definition's values and the figures of both bars."""

    def __init__(self, spec, S, K):
        from bc_mpc_amd import value
        self.K = K
        self.states = make_states(S, K)
        self.obz = value.observe(spec, self.states)
        self.v_def = value.terminal_values(spec, self.states)
        self.v64 = value.terminal_values_f64(spec, self.obz)
        self.bound = value.error_bound(spec, self.obz)
        self.finite = np.isfinite(self.v64)
        self.seq_rms = None
        if K >= 64:
            seq = value.terminal_values_seq32(spec, self.obz)
            assert np.array_equal(np.isfinite(seq), self.finite)
            self.seq_rms = float(np.sqrt(np.mean((seq[self.finite].astype(np.float64) - self.v64[self.finite]) ** 2)))
        for a in (self.states, self.obz, self.v_def, self.v64, self.bound):
            a.setflags(write=False)

    def check(self, v, label):
        """Both bars and the NaN pattern for an f32 evaluation ``v``; returns (worst |delta| / E_k, RMS ratio
        or None)."""
        v = np.asarray(v)
        assert v.dtype == np.float32 and v.shape == (self.K,), label
        assert np.array_equal(np.isnan(v), np.isnan(self.v_def)), f"{label}: NaN pattern"
        assert np.array_equal(np.isnan(self.v_def), ~self.finite), label
        f = self.finite
        d = np.abs(v[f].astype(np.float64) - self.v64[f])
        worst = float(np.max(d / self.bound[f])) if f.any() else 0.0
        ratio = None
        if self.seq_rms is not None:
            rms = float(np.sqrt(np.mean(d ** 2)))
            ratio = rms / self.seq_rms if self.seq_rms > 0 else (0.0 if rms == 0 else float("inf"))
        print(f"{label}: max |dv| / E_k = {worst:.3f}" + ("" if ratio is None else f", RMS ratio = {ratio:.3f} "
                                                          f"(seq32 RMS {self.seq_rms:.3e})"))
        assert (d <= self.bound[f]).all(), f"{label}: bar (a): worst |dv| / E_k = {worst}"
        if ratio is not None:
            assert ratio <= RMS_FACTOR, f"{label}: bar (b): RMS ratio {ratio}"
        return worst, ratio


@functools.lru_cache(maxsize=None)
def case(S, hidden, L):
    """(spec, {K: Case}) of one net."""
    spec = make_spec(S, hidden, L)
    return spec, {K: Case(spec, S, K) for K in KS}


def identity_like(S, d):
    """A one-layer net whose value IS obz[:, d], bit for bit, on any f32 evaluation: the hidden layer is
    2^-40 I (tanh(x) == x in f32 for |x| <= 5 * 2^-40: the cubic term is below half an ulp), the final kernel
    2^40 on neuron d and 0 elsewhere -- power-of-two scalings and additions of exact zeros only.  Holds for
    finite rows whose obz[:, d] is 0 or at least 2^-60 in magnitude (no subnormal intermediate)."""
    from bc_mpc_amd.value import ValueSpec
    rs = np.random.RandomState(77 + S)
    w0 = (np.eye(S) * 2.0 ** -40).astype(np.float32)
    wf = np.zeros((S, 1), np.float32)
    wf[d, 0] = 2.0 ** 40
    mean = rs.uniform(-0.5, 0.5, S).astype(np.float32)
    std = rs.uniform(0.5, 2.0, S).astype(np.float32)
    mean[0], std[0] = 0.0, 1.0
    return ValueSpec([w0, wf], [np.zeros(S, np.float32), np.zeros(1, np.float32)], mean, std)


def identity_states(S, K=65):
    """Finite rows for identity_like: values on, just inside and beyond the clip in every dimension."""
    rs = np.random.RandomState(5 + S)
    s = rs.standard_normal((K, S)) * 3.0
    s[0, :], s[1, :], s[2, :] = 1e6, -1e6, 0.0
    s[3, 0], s[4, 0] = 5.0, -5.0
    s[5, 0], s[6, 0] = np.nextafter(np.float32(5), np.float32(0)), np.nextafter(np.float32(-5), np.float32(0))
    s[7, :] = 1e300
    return s

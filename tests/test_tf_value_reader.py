"""The TF1 critic reader (bc_mpc_amd/value.py) against a stand-in graph that names its variables exactly as the
reference's ``ppo_bc_policy.MlpPolicy`` does (``build_network(sess, 'pi', ob)`` inside ``variable_scope('pi')``,
ppo_bc_policy.py:31-32, 56-64): ``pi/pi/vf/fc{1..L}/{kernel,bias}:0``, ``pi/pi/vf/final/{kernel,bias}:0`` and the
RunningMeanStd sums under ``pi/pi/obfilter`` -- beside ``pol/``, ``old_pi/`` and Adam slots that must not be read.
TensorFlow itself is absent here, as in tests/test_tf_readers.py."""
import sys
import types

import numpy as np
import pytest

from bc_mpc_amd import policy as bpol
from bc_mpc_amd import value as bval


class _Var:
    def __init__(self, name):
        self.name = name


class _Sess:
    def __init__(self, values):
        self.values = values
        self.fetched = []

    def run(self, fetches):
        self.fetched.append([v.name for v in fetches])
        return [self.values[v.name] for v in fetches]


@pytest.fixture
def fake_tf(monkeypatch):
    mod = types.ModuleType("tensorflow")
    mod._vars = []
    mod.global_variables = lambda: list(mod._vars)
    monkeypatch.setitem(sys.modules, "tensorflow", mod)
    return mod


def _mlp_policy_values(rs, prefix, S, A, ph, L):
    vals = {}
    dims = [S] + [ph] * L
    for i in range(L):
        for part in ("pol", "vf"):
            vals[f"{prefix}/{part}/fc{i + 1}/kernel:0"] = rs.randn(dims[i], ph).astype(np.float32)
            vals[f"{prefix}/{part}/fc{i + 1}/bias:0"] = rs.randn(ph).astype(np.float32)
            vals[f"{prefix}/{part}/fc{i + 1}/kernel/Adam:0"] = np.zeros((dims[i], ph), np.float32)
    vals[f"{prefix}/pol/final/kernel:0"] = rs.randn(ph, A).astype(np.float32)
    vals[f"{prefix}/pol/final/bias:0"] = rs.randn(A).astype(np.float32)
    vals[f"{prefix}/vf/final/kernel:0"] = rs.randn(ph, 1).astype(np.float32)
    vals[f"{prefix}/vf/final/bias:0"] = rs.randn(1).astype(np.float32)
    vals[f"{prefix}/pol/logstd:0"] = rs.randn(1, A).astype(np.float32)
    vals[f"{prefix}/obfilter/runningsum:0"] = rs.randn(S) * 50.0              # f64, as RunningMeanStd
    vals[f"{prefix}/obfilter/runningsumsq:0"] = np.abs(rs.randn(S)) * 900.0 + 500.0
    vals[f"{prefix}/obfilter/count:0"] = np.float64(377.0)
    return vals


def test_value_reader_reference_names(fake_tf):
    rs = np.random.RandomState(1)
    S, A, ph, L = 20, 6, 16, 2
    vals = _mlp_policy_values(rs, "pi/pi", S, A, ph, L)
    vals.update(_mlp_policy_values(rs, "old_pi/old_pi", S, A, ph, L))
    fake_tf._vars = [_Var(n) for n in vals]
    sess = _Sess(vals)
    pnet = types.SimpleNamespace(sess=sess, pi_scope="pi", num_hid_layers=L)
    spec, ver = bval.extract(pnet)
    p = "pi/pi"
    assert isinstance(spec, bval.ValueSpec) and (spec.n_layers, spec.hidden, spec.state_dim) == (L, ph, S)
    assert [k.shape for k in spec.kernels] == [(S, ph), (ph, ph), (ph, 1)]
    for i in range(L):
        assert np.array_equal(spec.kernels[i], vals[f"{p}/vf/fc{i + 1}/kernel:0"])
        assert np.array_equal(spec.biases[i], vals[f"{p}/vf/fc{i + 1}/bias:0"])
    assert np.array_equal(spec.kernels[L], vals[f"{p}/vf/final/kernel:0"])
    assert np.array_equal(spec.biases[L], vals[f"{p}/vf/final/bias:0"])
    # RunningMeanStd (baselines): mean = to_float(sum / count), std = sqrt(max(to_float(sumsq / count) - mean^2, 1e-2))
    cnt = vals[f"{p}/obfilter/count:0"]
    mean = (vals[f"{p}/obfilter/runningsum:0"] / cnt).astype(np.float32)
    std = np.sqrt(np.maximum((vals[f"{p}/obfilter/runningsumsq:0"] / cnt).astype(np.float32) - np.square(mean),
                             np.float32(1e-2)))
    assert np.array_equal(spec.ob_mean, mean) and np.array_equal(spec.ob_std, std.astype(np.float32))
    # ... the very filter the policy reader builds from the same graph
    pspec, _ = bpol.extract(pnet)
    assert np.array_equal(spec.ob_mean, pspec.ob_mean) and np.array_equal(spec.ob_std, pspec.ob_std)
    fetched = sess.fetched[0]
    assert all(n.startswith("pi/pi/vf/") or n.startswith("pi/pi/obfilter/") for n in fetched)
    assert not any("Adam" in n or "/pol/" in n for n in fetched)
    # the digest changes with the critic's weights, and only with them
    vals[f"{p}/pol/fc1/bias:0"] = vals[f"{p}/pol/fc1/bias:0"] + np.float32(1.0)
    assert bval.extract(pnet)[1] == ver
    vals[f"{p}/vf/final/bias:0"] = vals[f"{p}/vf/final/bias:0"] + np.float32(1.0)
    assert bval.extract(pnet)[1] != ver
    # a container's own integer version is trusted
    pnet.version = 12
    assert bval.extract(pnet)[1] == 12


def test_value_reader_accepts_a_net_built_directly_under_the_scope(fake_tf):
    vals = _mlp_policy_values(np.random.RandomState(3), "pi", 11, 3, 8, 1)
    fake_tf._vars = [_Var(n) for n in vals]
    spec, _ = bval.extract(types.SimpleNamespace(sess=_Sess(vals), pi_scope="pi", num_hid_layers=1))
    assert np.array_equal(spec.kernels[0], vals["pi/vf/fc1/kernel:0"]) and spec.n_layers == 1


def test_value_reader_rejects_missing_scope(fake_tf):
    vals = _mlp_policy_values(np.random.RandomState(2), "other/other", 20, 6, 8, 1)
    fake_tf._vars = [_Var(n) for n in vals]
    pnet = types.SimpleNamespace(sess=_Sess(vals), pi_scope="pi", num_hid_layers=1)
    with pytest.raises(KeyError, match="pi/pi/vf/fc1/kernel:0"):
        bval.extract(pnet)

"""Every controller's answers under two checkouts of the Python package, compared bitwise ("same library, different
host code": a change of bc_mpc_amd/*.py that claims the same results and the same consumption of the random streams).

usage: python tools/ctrl_bitwise.py PKG_A PKG_B [--timeout 300] [--labels A B]
           PKG_A / PKG_B: repository roots (e.g. a `git worktree` of the parent commit and this tree)

Each root runs the fixed script below in its own child process, one after the other, each under its own time limit,
with BCMPC_LIB pointing at THIS tree's libbcmpc.so.  The script drives every controller class -- single and batched,
over plain, reward and ensemble models, every ``rng`` mode -- through three consecutive calls (the repeat-call fast
paths, the warm-start plans), one change of shape (K), three more calls, and where it applies a change of gamma, of
the cost kind or of the ensemble rule.  After every call it dumps the returned action, every ``last_*`` attribute,
the controller's seed stream and the position of ``np.random``.  Exit status 1 on a mismatch."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes, sys, zlib, numpy as np
sys.path.insert(0, {root!r})
import bc_mpc_amd as pkg
from bc_mpc_amd.cost_functions import TermCost, linear, threshold
from bc_mpc_amd.ensemble import EnsembleDynamicsModel
from oracle import mpc_oracle as orc
assert pkg.__file__.startswith({root!r}), pkg.__file__
S, A, H, K, K2, B = 20, 6, 4, 40, 56, 2
saved = {{}}


class Box:
    def __init__(self, n, seed):
        self.low, self.high, self.shape = -np.ones(n, np.float32), np.ones(n, np.float32), (n,)
        self.np_random = np.random.RandomState(seed)

    def sample(self):
        return self.np_random.uniform(low=self.low, high=self.high, size=self.shape).astype(np.float32)


class Env:
    def __init__(self):
        self.action_space, self.observation_space = Box(A, 3), Box(S, 4)


norm = orc.synthetic_normalization(S, A)
rnorm = orc.synthetic_normalization(S, A, seed=5, reward=True)
# (a fused policy needs a dynamics net wider than 64: the policy-guided controllers run 2 x 128 nets)
delta = lambda h=64: orc.NumpyDynamics(orc.synthetic_weights(S, A, h, 2, "tanh", False), norm)
reward = lambda h=64: orc.NumpyRewardDynamics(orc.synthetic_reward_weights(S, A, h, False, seed_base=321), rnorm)
policy = lambda: orc.NumpyPolicy(orc.synthetic_policy(S, A, 128, 2, seed=9))
state = orc.synthetic_state(norm, seed=11)
states = np.stack([orc.synthetic_state(norm, seed=11 + b) for b in range(B)])
TERMS = TermCost([threshold(5, ">=", 0.2, 10.0), linear(2, 0.1, on="action")])


def ensemble(**kw):
    m = EnsembleDynamicsModel(Env(), 2, 2, 64, "tanh", None, norm, 32, 3, 1e-3, device=0, **kw)
    for e in range(2):
        w = orc.synthetic_weights(S, A, 64, 2, "tanh", False, seed_base=1000 + 100 * e)
        m.load_weights(e, w.kernels, w.biases, None, None)
    return m


def raw(x):
    if x is None:
        return np.frombuffer(b"None", dtype=np.uint8)
    if isinstance(x, ctypes.Structure):
        return np.frombuffer(bytes(x), dtype=np.uint8)
    if isinstance(x, (tuple, list)):
        return np.concatenate([raw(v) for v in x] + [np.zeros(0, np.uint8)])
    a = np.ascontiguousarray(np.asarray(x))
    head = np.frombuffer(f"{{a.dtype.str}}{{a.shape}}".encode(), dtype=np.uint8)
    return np.concatenate([head, a.view(np.uint8).reshape(-1)])


def stream(rs):
    st = rs.get_state() if hasattr(rs, "get_state") else None
    if st is None:
        return None
    if st[0] != "MT19937":                      # controllers._SeedStream: (RandomState state, unread seeds)
        return (stream_of(st[0]), list(st[1]))
    return stream_of(st)


def stream_of(st):
    return [zlib.crc32(np.asarray(st[1]).tobytes()), int(st[2])]


def record(tag, out, ctrl):
    saved[tag + ".return"] = raw(out)
    for k in sorted(vars(ctrl)):
        if k.startswith("last_"):
            saved[f"{{tag}}.{{k}}"] = raw(getattr(ctrl, k))
    saved[tag + ".seed_stream"] = raw(stream(getattr(ctrl, "_seed_rng", None)))
    saved[tag + ".np_random"] = raw(stream(np.random))
    saved[tag + ".env_random"] = raw(stream(ctrl.env.action_space.np_random))


def drive(tag, ctrl, calls, changes):
    # three consecutive rounds of ``calls``, then after each change in ``changes`` three more
    np.random.seed(1234)
    for phase, change in enumerate([None] + list(changes)):
        if change is not None:
            change(ctrl)
        for i in range(3):
            for name, arg in calls:
                record(f"{{tag}}|{{phase}}.{{i}}.{{name}}", getattr(ctrl, name)(arg), ctrl)
    if hasattr(ctrl, "close"):
        ctrl.close()
    print(tag, flush=True)


def set_k(c):
    if hasattr(c, "num_first_stage_actions"):
        c.num_first_stage_actions = 9
    else:
        c.num_simulated_paths = K2


def set_attr(name, value, on_model=False):
    def change(c):
        setattr(c.dyn_model if on_model else c, name, value)
    return change


ONE, BOTH = [("get_action", state)], [("get_action", state), ("get_actions", states)]
cheetah = pkg.cheetah_cost_fn
host_cost = lambda s, a, ns: np.sum(np.asarray(ns) ** 2, axis=-1) + np.asarray(a)[..., 0]
dev = dict(rng="device", seed=7)

# ---- random shooting
drive("mpc_numpy", pkg.MPCcontroller(Env(), delta(), H, cheetah, K), ONE, [set_k, set_attr("keep_costs", True)])
drive("mpc_numpy_terms", pkg.MPCcontroller(Env(), delta(), H, TERMS, K), ONE, [set_k])
drive("mpc_numpy_host_cost", pkg.MPCcontroller(Env(), delta(), H, host_cost, K), ONE, [set_k])
drive("mpc_device", pkg.MPCcontroller(Env(), delta(), H, cheetah, K, **dev), BOTH,
      [set_k, set_attr("cost_fn", TERMS), set_attr("keep_costs", True), set_attr("horizon", 3)])
drive("mpc_device_np_seeds", pkg.MPCcontroller(Env(), delta(), H, cheetah, K, rng="device"), BOTH, [set_k])
drive("mpc_ensemble_numpy", pkg.MPCcontroller(Env(), ensemble(), H, cheetah, K), ONE,
      [set_k, set_attr("rule", "worst", True)])
drive("mpc_ensemble_device", pkg.MPCcontroller(Env(), ensemble(diagnostics=True), H, cheetah, K, **dev), BOTH,
      [set_k, set_attr("rule", "mean_std", True), set_attr("kappa", 1.5, True), set_attr("cost_fn", TERMS)])
drive("reward_env", pkg.MPCcontrollerReward(Env(), reward(), H, None, K, 0.9), ONE, [set_k, set_attr("gamma", 0.5)])
drive("reward_device", pkg.MPCcontrollerReward(Env(), reward(), H, None, K, 0.9, **dev), BOTH,
      [set_k, set_attr("gamma", 0.5), set_attr("keep_costs", True)])
# ---- policy-guided
for name, self_exp in (("explore", False), ("stochastic", True)):
    drive(f"policy_{{name}}",
          pkg.MPCcontrollerPolicyNet(Env(), delta(128), policy(), 0.3, self_exp, H, cheetah, K, seed=5), ONE,
          [set_k, set_attr("explore", 0.6), set_attr("keep_costs", True)])
    drive(f"policy_reward_{{name}}",
          pkg.MPCcontrollerPolicyNetReward(Env(), reward(128), policy(), 0.3, self_exp, H, None, K, seed=5), ONE,
          [set_k])
for name, kw in (("stochastic", dict(self_exp=True)), ("mean", dict(self_exp=False)),
                 ("env", dict(random_first_stage_action=True))):
    drive(f"mcts_{{name}}", pkg.MCTScontrollerPolicyNetReward(Env(), reward(128), policy(), explore=0.3, horizon=H,
                                                            num_first_stage_actions=12, random_path_per_action=5,
                                                            seed=77, **kw), ONE, [set_k, set_attr("horizon", 3)])
# ---- the planners
for kind, cls, extra in (("cem", pkg.CEMcontroller, dict(iterations=3, n_elite=5)),
                         ("mppi", pkg.MPPIcontroller, dict(iterations=2, temperature=0.7))):
    drive(kind, cls(Env(), delta(), H, cheetah, K, seed=3, **extra), BOTH,
          [set_k, set_attr("cost_fn", TERMS), set_attr("horizon", 3), lambda c: c.reset([1]), lambda c: c.reset()])
    drive(kind + "_reward", cls(Env(), reward(), H, None, K, 0.9, seed=3, **extra), BOTH,
          [set_k, set_attr("gamma", 0.5)])
    drive(kind + "_ensemble", cls(Env(), ensemble(), H, cheetah, K, seed=3, **extra), ONE,
          [set_k, set_attr("rule", "mean_std", True), set_attr("cost_fn", TERMS)])
np.savez({path!r}, **saved)
"""


def run_child(root, path, timeout):
    env = dict(os.environ, BCMPC_LIB=os.path.join(REPO, "bc_mpc_amd", "libbcmpc.so"))
    env.pop("PYTHONPATH", None)
    code = CHILD.format(root=os.path.abspath(root), path=path)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        print(p.stdout, p.stderr)
        sys.exit(2)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pkg_a")
    ap.add_argument("pkg_b")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per package")
    ap.add_argument("--labels", nargs=2, metavar=("A", "B"), help="what the two roots are, printed beside them")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        ra, rb = (run_child(root, os.path.join(td, f"c{i}.npz"), a.timeout)
                  for i, root in enumerate((a.pkg_a, a.pkg_b)))
    print("# python tools/ctrl_bitwise.py " + " ".join(sys.argv[1:3]))
    for label, root in (("A", a.pkg_a), ("B", a.pkg_b)):
        print(f"{label}: {os.path.relpath(root, REPO)}" + (f" ({a.labels[label == 'B']})" if a.labels else ""))
    print("library: bc_mpc_amd/libbcmpc.so of this tree")
    tags = sorted({k.split("|")[0] for k in ra} | {k.split("|")[0] for k in rb})
    bad = 0
    for tag in tags:
        ka, kb = (sorted(k for k in r if k.split("|")[0] == tag) for r in (ra, rb))
        diff = sorted(set(ka) ^ set(kb)) + [k for k in ka if k in rb and ra[k].tobytes() != rb[k].tobytes()]
        calls = len({k.rsplit(".", 1)[0] for k in ka})
        print(f"{tag:26s} {calls:3d} calls {len(ka):4d} outputs {sum(ra[k].size for k in ka):8d} bytes  "
              f"byte-equal: {not diff}" + (f"  differ: {diff[:8]}" if diff else ""))
        bad += bool(diff)
    print(f"{len(tags) - bad} of {len(tags)} controllers byte-equal")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

"""Outputs of one engine configuration under two library builds, compared bitwise ("same arithmetic, different
build": a layout change that claims the same summation orders, e.g. rollout_pp's PP_QI sweep, or a change of
the host code alone).

usage: python tools/lib_bitwise.py LIB_A LIB_B [--precision f16] [--K 65536] [--H 20]
           the cost vectors of get_action at cfg3's net, Philox actions, two seeds
       python tools/lib_bitwise.py LIB_A LIB_B --entry all|NAME... [--K 2048] [--H 5] [--B 4]
           every output of the named synchronous entry points (ENTRIES below) at the 2 x 500 tanh net: records,
           costs, mu, sigma and MPPI statistics, each compared byte for byte.  The *_ln entries run get_action on
           LayerNorm nets (the host's LayerNorm packing: 2 x 256 relu + LN in split precision and in fp32, the
           reward net with LayerNorm in fp32 and on the team kernel; get_action_ln_team: the 2 x 256 relu + LN net
           on the team kernel at K = 400, the deferred LayerNorm).  get_action_policy_*: a fused-policy engine in
           fp32 (dynamics hidden 128) and in split precision (hidden 500), policy 2 x 64.  get_action_value:
           get_action with a terminal value set (value net 2 x 64).  The *_giveup entries need a team engine:
           they halve K from --K until the team grid fits the device, so they may run below --K (the layout and
           num_paths of every entry are printed)
Each build runs in its own child process (BCMPC_LIB), one after the other, under its own time limit; exit
status 1 on a mismatch."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys, numpy as np
sys.path.insert(0, {repo!r})
from bench import synthetic_problem, make_engine, WORKLOADS
wl = dict(WORKLOADS["cfg3"], K={K}, H={H})
prob = synthetic_problem(wl)
eng = make_engine(wl, prob, 0, {prec!r})
out = []
for seed in (11, 12):
    r = eng.get_action(prob["state"], None, seed=seed, return_costs=True)
    out.append(r.costs)
np.save({path!r}, np.stack(out))
print(eng.info()["layout"])
"""

# name -> (ensemble members or 0, batched, planner or None, forced team give-up[, net: NETS of the child])
ENTRIES = {
    "get_action": (0, False, None, False), "get_actions": (0, True, None, False),
    "cem": (0, False, "cem", False), "mppi": (0, False, "mppi", False),
    "cem_batch": (0, True, "cem", False), "mppi_batch": (0, True, "mppi", False),
    "ensemble_get_action": (3, False, None, False), "ensemble_get_actions": (3, True, None, False),
    "ensemble_cem": (3, False, "cem", False), "ensemble_mppi": (3, False, "mppi", False),
    "cem_giveup": (0, False, "cem", True), "mppi_giveup": (0, False, "mppi", True),
    "get_action_ln": (0, False, None, False, "ln"), "get_action_ln_fp32": (0, False, None, False, "ln_fp32"),
    "get_action_reward_ln": (0, False, None, False, "reward_ln"),
    "get_action_reward_ln_team": (0, False, None, False, "reward_ln_team"),
    "get_action_ln_team": (0, False, None, False, "ln_team"),
    "get_action_policy_fp32": (0, False, None, False, "policy_fp32"),
    "get_action_policy_split": (0, False, None, False, "policy_split"),
    "get_action_value": (0, False, None, False, "value"),
}

ENTRY_CHILD = r"""
import ctypes, os, sys, numpy as np
sys.path.insert(0, {repo!r})
from bc_mpc_amd import ensemble
from bc_mpc_amd.engine import MLPSpec, PolicySpec, RolloutEngine
from bc_mpc_amd.value import ValueSpec
from oracle import mpc_oracle as orc
S, A, HID = 20, 6, 500
K, H, B, PREC, ENTRIES, NAMES = {K}, {H}, {B}, {prec!r}, {entries!r}, {names!r}
ITERS, N_ELITE, ALPHA, LAM = 3, max(1, K // 10), 0.1, 1.0
norm = orc.synthetic_normalization(S, A)
states = np.stack([orc.synthetic_state(norm, seed=11 + b) for b in range(B)])
rs = np.random.RandomState(5)
mu0, sd0 = rs.uniform(-0.6, 0.6, (B, H, A)), rs.uniform(0.1, 0.6, (B, H, A))


# net -> (hidden, activation, LayerNorm, reward model, precision or None: PREC, kernel or None, K or None: --K
#         [, extra: "policy" a fused 2 x 64 policy, "value" a 2 x 64 terminal value])
NETS = {{"tanh": (HID, "tanh", False, False, None, None, None), "ln": (256, "relu", True, False, None, None, None),
        "ln_fp32": (256, "relu", True, False, "fp32", None, None),
        "reward_ln": (128, "tanh", True, True, None, None, None),
        "reward_ln_team": (500, "tanh", True, True, None, "team", 400),
        "ln_team": (256, "relu", True, False, None, "team", 400),
        "policy_fp32": (128, "tanh", False, False, "fp32", None, None, "policy"),
        "policy_split": (HID, "tanh", False, False, "split", None, None, "policy"),
        "value": (HID, "tanh", False, False, None, None, None, "value")}}


def spec(member, net="tanh"):
    hid, act, ln, reward = NETS[net][:4]
    if reward:
        w = orc.synthetic_reward_weights(S, A, hid, ln, seed_base=555)
        return MLPSpec(w.kernels, w.biases, "tanh", w.ln_gamma, w.ln_beta, model="reward")
    w = orc.synthetic_weights(S, A, hid, 2, act, ln, seed_base=1000 + 100 * member)
    return MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma if ln else None, w.ln_beta if ln else None)


def flat(x):
    # every output of a call as named byte strings
    if isinstance(x, tuple):
        return {{f"{{i}}.{{k}}": v for i, part in enumerate(x) for k, v in flat(part).items()}}
    if isinstance(x, np.ndarray):
        return {{"array": np.ascontiguousarray(x).view(np.uint8).reshape(-1)}}
    if isinstance(x, ctypes.Structure):
        return {{"struct": np.frombuffer(bytes(x), dtype=np.uint8)}}
    out = {{}}
    for k in ("best_index", "best_cost", "first_action", "costs", "member_costs"):
        v = getattr(x, k, None)
        if v is not None:
            out[k] = np.ascontiguousarray(np.asarray(v)).view(np.uint8).reshape(-1)
    return out


def value_spec(hidden=64, layers=2):
    rs = np.random.RandomState(77)
    dims = [S] + [hidden] * layers + [1]
    ks = [(rs.standard_normal((i, o)) / np.sqrt(i)).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
    bs = [(0.1 * rs.standard_normal(o)).astype(np.float32) for o in dims[1:]]
    return ValueSpec(ks, bs, norm[0].astype(np.float32), (norm[1] + 0.1).astype(np.float32))


def engine(members, n, kernel=None, net="tanh"):
    hid, act, ln, reward, prec, nkernel, nk = NETS[net][:7]
    extra = NETS[net][7] if len(NETS[net]) > 7 else None
    if net != "tanh":
        rnorm = orc.synthetic_normalization(seed=31, reward=True) if reward else norm
        pol = dict(policy_hidden=64, policy_layers=2, policy_mode="explore") if extra == "policy" else {{}}
        eng = RolloutEngine(S, A, hid, 2, act, ln, H, nk or n, device=0, kernel=nkernel,
                            precision=None if nkernel else (prec or PREC), cost="reward" if reward else "cheetah",
                            model="reward" if reward else "delta", **pol)
        eng.set_weights(spec(0, net), rnorm, 1)
        if reward:
            eng.set_discount(0.95)
        if extra == "policy":
            p = orc.synthetic_policy(S, A, 64, 2)
            eng.set_policy(PolicySpec(p.kernels, p.biases, p.ob_mean, p.ob_std, p.logstd), 0.25, 1)
        if extra == "value":
            eng.set_terminal_value(value_spec(), -0.5, 1)
        return eng
    if members:
        eng = ensemble.EnsembleEngine(members, S, A, HID, 2, "tanh", False, H, n, device=0, precision=PREC)
        for i in range(members):
            eng.set_weights(i, spec(i), norm, 1)
    else:
        eng = RolloutEngine(S, A, HID, 2, "tanh", False, H, n, device=0, kernel=kernel,
                            precision=None if kernel else PREC)
        eng.set_weights(spec(0), norm, 1)
    return eng


saved = {{}}
for name in NAMES:
    members, batched, planner, giveup = ENTRIES[name][:4]
    net = ENTRIES[name][4] if len(ENTRIES[name]) > 4 else "tanh"
    n = K * B if batched else K
    if giveup:
        # the largest K up to --K whose team grid the device holds
        eng = None
        while eng is None:
            try:
                eng = engine(0, n, "team")
            except ValueError:
                if n <= 64:
                    raise
                n //= 2
        os.environ["BCMPC_TEAM_SPINS"] = "-1"
    else:
        eng = engine(members, n, None, net)
    outs = []
    for seed in (11, 12):
        if planner is None and batched:
            r = eng.get_actions(states, None, seed=seed, return_costs=True, **({{"return_member_costs": True}} if members else {{}}))
        elif planner is None:
            r = eng.get_action(states[0], None, seed=seed, return_costs=True, **({{"return_member_costs": True}} if members else {{}}))
        elif planner == "cem" and batched:
            r = eng.cem_get_actions(states, mu0, sd0, ITERS, N_ELITE, ALPHA, seed, 0, True)
        elif planner == "mppi" and batched:
            r = eng.mppi_get_actions(states, mu0, sd0, ITERS, LAM, seed, 0, True)
        elif planner == "cem":
            r = eng.cem_get_action(states[0], mu0[0], sd0[0], ITERS, min(N_ELITE, n), ALPHA, seed)
        else:
            r = eng.mppi_get_action(states[0], mu0[0], sd0[0], ITERS, LAM, seed)
        outs.append(r)
    if giveup:
        del os.environ["BCMPC_TEAM_SPINS"]
        assert eng.team_reruns == 2, eng.team_reruns
    for i, r in enumerate(outs):
        for k, v in flat(r).items():
            saved[f"{{name}}|seed{{i}}.{{k}}"] = v
    print(f"{{name}}: {{eng.info()['layout']}} num_paths {{eng.num_paths}}", flush=True)
    eng.close()
np.savez({path!r}, **saved)
"""


def run_child(code, lib, timeout):
    env = dict(os.environ, BCMPC_LIB=os.path.abspath(lib))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        print(p.stdout, p.stderr)
        sys.exit(2)
    return p.stdout.strip().splitlines()


def compare_entries(a):
    names = list(ENTRIES) if a.entry == ["all"] else a.entry
    unknown = [n for n in names if n not in ENTRIES]
    if unknown:
        sys.exit(f"unknown entry {unknown}; one of {list(ENTRIES)} or all")
    res = []
    with tempfile.TemporaryDirectory() as td:
        for i, lib in enumerate((a.lib_a, a.lib_b)):
            path = os.path.join(td, f"e{i}.npz")
            code = ENTRY_CHILD.format(repo=REPO, K=a.K or 2048, H=a.H or 5, B=a.B, prec=a.precision, entries=ENTRIES,
                                      names=names, path=path)
            for line in run_child(code, lib, a.timeout):
                print(f"{lib}: {line}")
            with np.load(path) as z:
                res.append({k: z[k] for k in z.files})
    ra, rb = res
    bad = 0
    for name in names:
        keys = sorted(k for k in ra if k.startswith(name + "|"))
        assert keys and keys == sorted(k for k in rb if k.startswith(name + "|")), name
        diff = [k for k in keys if ra[k].tobytes() != rb[k].tobytes()]
        nbytes = sum(ra[k].size for k in keys)
        print(f"{name:22s} {len(keys):3d} outputs {nbytes:9d} bytes  byte-equal: {not diff}" +
              (f"  differ: {diff}" if diff else ""))
        bad += bool(diff)
    print(f"{len(names) - bad} of {len(names)} entries byte-equal")
    sys.exit(1 if bad else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--precision", default=None, help="default: f16 without --entry, the engine's own choice with it")
    ap.add_argument("--K", type=int, default=None, help="default: 65536 without --entry, 2048 with it")
    ap.add_argument("--H", type=int, default=None, help="default: 20 without --entry, 5 with it")
    ap.add_argument("--B", type=int, default=4, help="environments of the batched entries (K candidates each)")
    ap.add_argument("--entry", nargs="+", help=f"all, or of {list(ENTRIES)}")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per library")
    a = ap.parse_args()
    if a.entry:
        compare_entries(a)
    res = []
    with tempfile.TemporaryDirectory() as td:
        for i, lib in enumerate((a.lib_a, a.lib_b)):
            path = os.path.join(td, f"c{i}.npy")
            code = CHILD.format(repo=REPO, K=a.K or 65536, H=a.H or 20, prec=a.precision or "f16", path=path)
            print(f"{lib}: {run_child(code, lib, a.timeout)[-1]}")
            res.append(np.load(path))
    ca, cb = res
    same = np.array_equal(ca, cb, equal_nan=True)
    diff = np.nanmax(np.abs(ca - cb))
    print(f"bitwise equal: {same}  max |diff| {diff:.3g}  ({ca.size} costs)")
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()

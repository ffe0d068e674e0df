#!/usr/bin/env python3
"""What proposals cost the CEM and MPPI controllers, on one MI355X.

Workloads (bench.py's): ppo_defaults (2 x 256 relu + LayerNorm, K = 400, H = 7), cfg2 (2 x 500 tanh, K = 4096,
H = 20) and cfg3 (that net, K = 65,536).  Per workload and planner (CEM x 4 iterations, MPPI x 2 rounds), the
controller's get_action, host clock around the call:

  default   no proposals: the single-plan chain, as ever
  host      proposals= with P = 24 host sequences: the batched chain at one environment with plan_sample_prop as
            its sampler (what noise_rho already pays: profiles/sampling.json prices that chain) plus the upload
  prior     policy_prior= with policy_paths = 24 (2 x 128 policy, stochastic mode): the prior block on the second
            engine -- tile_states and one policy rollout of 24 candidates -- on the planning engine's stream, then
            the same chain reading the device buffer
  prior_rollout_us   the prior block alone between HIP events (median of 30 after 3)

p50 (p10, p90) per variant, the variants in alternating rounds after a prewarm and warm-up calls, so that a drift of
the shared machine falls on all of them.  These are overheads to report, not criteria.

--defaults-only times the default calls alone and --root PATH imports the package (and its own libbcmpc.so) from
another checkout; --ab-parent PATH runs this tree and that checkout as child processes in alternating rounds and
writes the A/B of the default calls (profiles/proposals_default_ab.json is a committed run).

Prints one JSON line (profiles/proposals.json is a committed run).  Needs the GPU: no fallback.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S, A, P = 20, 6, 24
ROUNDS, PREWARM_S = 4, 0.25
WORKLOADS = {   # net and shape as bench.py's WORKLOADS; timed calls per variant
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True, timed=200),
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False, timed=100),
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False, timed=32),
}
PLANNERS = {"cem_x4": ("CEMcontroller", dict(iterations=4)), "mppi_x2": ("MPPIcontroller", dict(iterations=2))}


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


class _Box:
    def __init__(self, n):
        self.low, self.high, self.shape = -np.ones(n, np.float32), np.ones(n, np.float32), (n,)


class _Env:
    def __init__(self):
        self.action_space, self.observation_space = _Box(A), _Box(S)


def time_variants(variants, state, timed):
    """{name: p50 / p10 / p90} of ``ctrl.get_action(state, **kw)`` per (name, ctrl, kw), alternating rounds."""
    t0, calls = time.perf_counter(), 0
    while time.perf_counter() - t0 < PREWARM_S or calls < 3:
        _, ctrl, kw = variants[calls % len(variants)]
        ctrl.get_action(state, **kw)
        calls += 1
    for _ in range(5):
        for _, ctrl, kw in variants:
            ctrl.get_action(state, **kw)
    ts = {name: [] for name, _, _ in variants}
    per = max(1, timed // ROUNDS)
    for _ in range(ROUNDS):
        for name, ctrl, kw in variants:
            for _ in range(per):
                t = time.perf_counter()
                ctrl.get_action(state, **kw)
                ts[name].append(time.perf_counter() - t)
    row = {"timed": per * ROUNDS, "prewarm_calls": calls}
    for name, _, _ in variants:
        row[name] = {"p50_ms": pct(ts[name], 50), "p10_ms": pct(ts[name], 10), "p90_ms": pct(ts[name], 90)}
        if name != "default" and "default" in row:
            row[name]["vs_default"] = round(row[name]["p50_ms"] / row["default"]["p50_ms"], 4)
            row[name]["over_default_us"] = round((row[name]["p50_ms"] - row["default"]["p50_ms"]) * 1e3, 2)
    return row


def prior_rollout_us(ctrl, state, reps=30):
    """Device time of the prior block alone (tile_states + the policy rollout of P candidates) between HIP events."""
    import torch
    peng = ctrl._engines["prior"][1]
    dev = torch.device("cuda", peng.device)
    st = torch.cuda.current_stream(dev).cuda_stream
    d_state = torch.from_numpy(state[None].copy()).to(dev)
    d_out = torch.empty((peng.horizon, P, A), dtype=torch.float64, device=dev)
    d_costs = torch.empty(P, dtype=torch.float64, device=dev)
    ms = []
    for i in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        peng.rollout_policy_batch_async(d_state.data_ptr(), 1, None, 77 + i, 0, d_costs.data_ptr(), None, d_out.data_ptr(), st)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    peng.check_status()
    return round(float(np.median(ms[3:])) * 1e3, 2), peng.info()["layout"]


def measure(root, workloads, defaults_only):
    sys.path.insert(0, root)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_proposals: no GPU (the measurement has no CPU fallback)")
    import bc_mpc_amd as pkg
    from oracle import mpc_oracle as orc
    assert os.path.abspath(pkg.__file__).startswith(os.path.abspath(root)), pkg.__file__
    norm = orc.synthetic_normalization(S, A)
    state = orc.synthetic_state(norm)
    policy = orc.NumpyPolicy(orc.synthetic_policy(S, A, 128, 2))
    lines = []
    for wname in workloads:
        wl = WORKLOADS[wname]
        K, H = wl["K"], wl["H"]
        dyn = orc.NumpyDynamics(orc.synthetic_weights(S, A, wl["hidden"], 2, wl["act"], wl["ln"]), norm)
        seqs = np.random.RandomState(2).uniform(-1.2, 1.2, (P, H, A))
        for pname, (cls, extra) in PLANNERS.items():
            make = lambda **kw: getattr(pkg, cls)(_Env(), dyn, H, pkg.cheetah_cost_fn, K, seed=1, **extra, **kw)   # noqa: E731
            plain = make()
            variants = [("default", plain, {})]
            if not defaults_only:
                prior = make(policy_prior=policy, policy_paths=P)
                variants += [("host", plain, dict(proposals=seqs)), ("prior", prior, {})]
            row = {"workload": wname, "planner": pname, "K": K, "H": H, "P": P}
            row.update(time_variants(variants, state, wl["timed"]))
            row["layout"] = plain._engine.info()["layout"]
            if not defaults_only:
                row["prior_rollout_us"], row["prior_layout"] = prior_rollout_us(prior, state)
                row["prior_team_reruns"] = prior._engines["prior"][1].team_reruns
            lines.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    return {"bench": "proposals" + (" (default calls only)" if defaults_only else ""), "P": P, "rounds": ROUNDS,
            "device": torch.cuda.get_device_name(0), "results": lines}


def ab_parent(parent, workloads, rounds, timeout):
    """This tree and ``parent`` (a checkout with its own built library) as child processes, alternating."""
    runs = []
    for rnd in range(1, rounds + 1):
        for tree, root in (("this", REPO), ("parent", os.path.abspath(parent))):
            env = dict(os.environ)
            env.pop("BCMPC_LIB", None)
            env.pop("PYTHONPATH", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--defaults-only", "--root", root, "--workloads",
                                *workloads], env=env, capture_output=True, text=True, timeout=timeout)
            if p.returncode != 0:
                sys.exit(f"bench_proposals: the {tree} run failed\n{p.stdout}\n{p.stderr}")
            for r in json.loads(p.stdout.strip().split("\n")[-1])["results"]:
                runs.append({"tree": tree, "round": rnd, "workload": r["workload"], "planner": r["planner"], **r["default"]})
    return {"bench": "default CEM / MPPI controller calls, this tree and its parent, alternating child processes in one "
                     "session on one MI355X", "command": "python tools/bench_proposals.py --ab-parent PARENT", "runs": runs}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--defaults-only", action="store_true")
    ap.add_argument("--root", default=REPO, help="the checkout whose package (and library) is measured")
    ap.add_argument("--ab-parent", help="a checkout of the parent commit with its library built")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process of --ab-parent")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    out = (ab_parent(args.ab_parent, args.workloads, args.ab_rounds, args.timeout) if args.ab_parent
           else measure(args.root, args.workloads, args.defaults_only))
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What reference channels and a rate term cost beside the same cost with constant targets.

Side (a), "const": two constant-target quadratics on the next state and an action quadratic -- a plain list, scored
by the plain instances of csrc/term_cost.hip.  Side (b): the same cost with both targets as reference channels plus
a rate term on the action it already reads -- an extended list, the kernel's extended variant, 5 slots against 3 --
with a reference constant over the horizon ("chan_R", [R]) and one per step ("chan_HR", [H, R]); a call of side (b)
is set_cost_inputs (one small upload) plus get_action, as a tracking controller makes it every control step.  Three
points, each in one process:

  cfg3          K = 65,536, H = 20, 2 x 500 tanh
  cfg2          K = 4,096,  H = 20, 2 x 500 tanh
  ppo_defaults  K = 400,    H = 7,  2 x 256 relu + LayerNorm

Per point: the p50 of the synchronous call of each side (a prewarm past the clock ramp, 20 warm-up calls of each
side, then 200 timed calls of each in four alternating rounds of 50, as tools/bench_term_cost.py); the cost kernel
alone between two HIP events for each side (median of 50); and, at ppo_defaults' net, the batched step
get_actions over B = 8 and B = 64 environments of 400 candidates with one shared reference against one per
environment.

Prints one JSON line (profiles/tracking.json is a committed run).  Needs the GPU: no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

S, A = 20, 6
POINTS = {
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False),
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False),
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True),
}
WARMUP, TIMED, ROUNDS = 20, 200, 4
PREWARM_S = 0.25
EVENT_REPS = 50
BATCHES = (8, 64)


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def alternate(sides):
    """p50 / p10 / p90 in ms of every side's synchronous call: prewarm, warm-up, alternating timed rounds."""
    first = next(iter(sides.values()))
    t0, calls = time.perf_counter(), 0
    while time.perf_counter() - t0 < PREWARM_S or calls < 3:
        first(1 << 40 | calls)
        calls += 1
    for fn in sides.values():
        for i in range(WARMUP):
            fn(1000 + i)
    ts = {k: [] for k in sides}
    per = TIMED // ROUNDS
    for rnd in range(ROUNDS):
        for k, fn in sides.items():
            for i in range(per):
                t = time.perf_counter()
                fn(2000 + rnd * per + i)
                ts[k].append(time.perf_counter() - t)
    return {k: {"p50_ms": pct(v, 50), "p10_ms": pct(v, 10), "p90_ms": pct(v, 90)} for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", nargs="+", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_tracking: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd.cost_functions import TermCost, quadratic, rate, ref
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    dev = torch.device("cuda", 0)
    norm = orc.synthetic_normalization(S, A)
    state = orc.synthetic_state(norm)
    targets = np.array([0.3, -0.1])
    const = TermCost([quadratic(17, 1.0, target=targets[0], on="next_state"),
                      quadratic(0, 0.5, target=targets[1], on="next_state"), quadratic(0, 0.1, on="action")])
    chan = TermCost([quadratic(17, 1.0, target=ref(0), on="next_state"),
                     quadratic(0, 0.5, target=ref(1), on="next_state"), quadratic(0, 0.1, on="action"),
                     rate(0, 0.05)])

    def engine(p, K, cost):
        w = orc.synthetic_weights(S, A, p["hidden"], 2, p["act"], p["ln"])
        spec = MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma if p["ln"] else None,
                       w.ln_beta if p["ln"] else None)
        e = RolloutEngine(S, A, p["hidden"], 2, p["act"], p["ln"], p["H"], K, device=0, cost="terms")
        e.set_weights(spec, norm, 1)
        e.set_cost_terms(cost)
        return e

    lines = []
    for name in args.points:
        p = POINTS[name]
        K, H = p["K"], p["H"]
        e_const, e_chan = engine(p, K, const), engine(p, K, chan)
        ref_r, ref_hr, prev = targets.copy(), np.tile(targets, (H, 1)), np.zeros(A)

        def call_chan(reference):
            def fn(seed):
                e_chan.set_cost_inputs(reference, prev)
                return e_chan.get_action(state, None, seed=seed)
            return fn
        timed = alternate({"const": lambda seed: e_const.get_action(state, None, seed=seed),
                           "chan_R": call_chan(ref_r), "chan_HR": call_chan(ref_hr)})

        # the cost kernels alone, between HIP events on one stream, on the trajectory of a rollout
        f64 = dict(dtype=torch.float64, device=dev)
        d_state = torch.from_numpy(np.ascontiguousarray(state)).to(dev)
        d_costs, d_traj = torch.empty(K, **f64), torch.empty((H + 1, K, S), **f64)
        st = torch.cuda.current_stream(dev).cuda_stream
        e_const.rollout_async(d_state.data_ptr(), 0, None, 5, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, st)
        d_ref = {"chan_R": torch.from_numpy(ref_r.reshape(1, 1, 2)).to(dev),
                 "chan_HR": torch.from_numpy(ref_hr.reshape(1, H, 2).copy()).to(dev)}
        d_prev = torch.from_numpy(prev.reshape(1, A)).to(dev)
        kernels = {"const": lambda: e_const.trajectory_cost_async(d_traj.data_ptr(), K, d_costs.data_ptr(), seed=5,
                                                                  stream=st)}
        for k, r in d_ref.items():
            kernels[k] = (lambda r=r: e_chan.trajectory_cost_inputs_async(
                d_traj.data_ptr(), K, d_costs.data_ptr(), K, d_ref=r.data_ptr(), ref_envs=1, ref_steps=r.shape[1],
                d_prev=d_prev.data_ptr(), prev_envs=1, seed=5, stream=st))

        def event_ms(fn):
            x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            x.record()
            fn()
            y.record()
            y.synchronize()
            return x.elapsed_time(y)
        kernel_ms = {}
        for k, fn in kernels.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            kernel_ms[k] = round(float(np.median([event_ms(fn) for _ in range(EVENT_REPS)])), 4)
        e_const.check_status()
        line = {"point": name, "K": K, "H": H, "net": f"2x{p['hidden']} {p['act']}" + (" + LayerNorm" if p["ln"] else ""),
                "layout": e_const.info()["layout"], "slots": {"const": const.n_slots, "chan": chan.n_slots},
                "call": timed, "kernel_ms": kernel_ms,
                "overhead_R_ms": round(timed["chan_R"]["p50_ms"] - timed["const"]["p50_ms"], 4),
                "overhead_HR_ms": round(timed["chan_HR"]["p50_ms"] - timed["const"]["p50_ms"], 4)}
        lines.append(line)
        e_const.close()
        e_chan.close()

    batched = []
    p = POINTS["ppo_defaults"]
    for B in BATCHES:
        K, H = p["K"], p["H"]
        e_const, e_chan = engine(p, B * K, const), engine(p, B * K, chan)
        states = np.tile(state, (B, 1))
        shared, per_env = np.tile(targets, (1, H, 1)), np.tile(targets, (B, H, 1)) + 0.01 * np.arange(B)[:, None, None]
        prev1, prevB = np.zeros((1, A)), np.zeros((B, A))

        def call(reference, prev_):
            def fn(seed):
                e_chan.set_cost_inputs(reference, prev_)
                return e_chan.get_actions(states, None, seed=seed)
            return fn
        timed = alternate({"const": lambda seed: e_const.get_actions(states, None, seed=seed),
                           "shared": call(shared, prev1), "per_env": call(per_env, prevB)})
        batched.append({"B": B, "K": K, "H": H, "call": timed})
        e_const.close()
        e_chan.close()

    out = {"bench": "tracking", "const": repr(const), "chan": repr(chan), "warmup": WARMUP, "timed": TIMED,
           "rounds": ROUNDS, "event_reps": EVENT_REPS, "device": torch.cuda.get_device_name(0), "results": lines,
           "batched_ppo_defaults": batched}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What scoring a control step with a learned terminal value costs.

A 2 x 128 tanh critic (the reference's pi/vf shape) on an engine with the fused cheetah cost, at three points,
each in one process:

  cfg3          K = 65,536, H = 20, 2 x 500 tanh
  cfg2          K = 4,096,  H = 20, 2 x 500 tanh
  ppo_defaults  K = 400,    H = 7,  2 x 256 relu + LayerNorm

Per point, on one engine layout (the plain engine's `auto` choice; the same engine object with the value set and
removed, so that nothing but the value differs):

  plain_p50_ms / value_p50_ms   p50 of the synchronous RolloutEngine.get_action (in-kernel Philox actions)
  overhead_ms                   their difference: trajectory write + terminal_value_kernel + its launch (+ the
                                argmin launch where the plain engine reduces in its rollout kernel's tail)
  value_kernel_ms               device time of terminal_value_kernel alone (terminal_value_async on the last row of
                                a rollout's trajectory, values and in-place cost add) between two HIP events, median;
                                value_gflops: 2 * K * (S*h + h*h + h) flop over that time
  composed_p50_ms               the alternative without the feature, from what a plain engine offers:
                                rollout_async with the trajectory, the trajectory to the host, value.terminal_values
                                in NumPy, the add, np.argmin (p50 of COMPOSED_REPS calls)
  same_answer                   the composed path and the engine agree on the winner

Every synchronous call ends in its own host synchronisation, so the host clock around it is its latency.  A
prewarm past the clock ramp (as bench.py's), 20 warm-up calls of each side, then 200 timed calls of each side in
four alternating rounds of 50, so that a drift of the shared machine falls on both.

Prints one JSON line (profiles/terminal_value.json is a committed run).  Needs the GPU: no fallback.
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
VH, VL = 128, 2
WEIGHT = -1.0
POINTS = {
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False),
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False),
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True),
}
WARMUP, TIMED, ROUNDS = 20, 200, 4
PREWARM_S = 0.25
EVENT_REPS = 50
COMPOSED_REPS = 10


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def critic():
    from bc_mpc_amd.value import ValueSpec
    rs = np.random.RandomState(2024)
    dims = [S] + [VH] * VL + [1]
    ks = [(rs.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(VL + 1)]
    bs = [(0.1 * rs.standard_normal(dims[i + 1])).astype(np.float32) for i in range(VL + 1)]
    return ValueSpec(ks, bs, rs.uniform(-0.5, 0.5, S).astype(np.float32), rs.uniform(0.5, 2.0, S).astype(np.float32))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", nargs="+", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_terminal_value: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd import value
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    dev = torch.device("cuda", 0)
    norm = orc.synthetic_normalization(S, A)
    state = orc.synthetic_state(norm)
    vspec = critic()
    lines = []
    for name in args.points:
        p = POINTS[name]
        K, H = p["K"], p["H"]
        w = orc.synthetic_weights(S, A, p["hidden"], 2, p["act"], p["ln"])
        spec = MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma if p["ln"] else None,
                       w.ln_beta if p["ln"] else None)
        engines = {}
        for side in ("plain", "value"):
            e = RolloutEngine(S, A, p["hidden"], 2, p["act"], p["ln"], H, K, device=0, cost="cheetah")
            e.set_weights(spec, norm, 1)
            engines[side] = e
        plain, veng = engines["plain"], engines["value"]
        veng.set_terminal_value(vspec, WEIGHT, 1)
        layouts = {k: e.info()["layout"] for k, e in engines.items()}
        assert layouts["value"] == layouts["plain"] + "+value", layouts

        f64 = dict(dtype=torch.float64, device=dev)
        d_state = torch.from_numpy(np.ascontiguousarray(state)).to(dev)
        d_costs = torch.empty(K, **f64)
        d_traj = torch.empty((H + 1, K, S), **f64)
        d_values = torch.empty(K, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev)
        st = stream.cuda_stream

        def composed(seed):
            plain.rollout_async(d_state.data_ptr(), 0, None, seed, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, st)
            traj = d_traj.cpu().numpy()                                # the whole trajectory, as a plain engine returns it
            costs = d_costs.cpu().numpy()
            total = value.add_to_costs(costs, value.terminal_values(vspec, traj[H]), WEIGHT)
            return int(np.argmin(total)), total

        best_c, total_c = composed(7)
        got = veng.get_action(state, None, seed=7, return_costs=True)
        same_answer = bool(got.best_index == best_c)
        max_dcost = float(np.max(np.abs(got.costs - total_c)))

        sides = {k: (lambda seed, e=e: e.get_action(state, None, seed=seed)) for k, e in engines.items()}
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < PREWARM_S or calls < 3:
            sides["value"](1 << 40 | calls)
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
        tc = []
        for i in range(COMPOSED_REPS + 2):
            t = time.perf_counter()
            composed(3000 + i)
            tc.append(time.perf_counter() - t)
        tc = tc[2:]

        def kernel():
            veng.terminal_value_async(d_traj[H].data_ptr(), K, d_values=d_values.data_ptr(), d_costs=d_costs.data_ptr(),
                                      stream=st)

        def event_ms(fn):
            x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            x.record()
            fn()
            y.record()
            y.synchronize()
            return x.elapsed_time(y)

        for _ in range(5):
            kernel()
        torch.cuda.synchronize()
        k_ms = float(np.median([event_ms(kernel) for _ in range(EVENT_REPS)]))
        plain.check_status()
        flop = 2.0 * K * (S * VH + (VL - 1) * VH * VH + VH)
        line = {"point": name, "K": K, "H": H, "net": f"2x{p['hidden']} {p['act']}" + (" + LayerNorm" if p["ln"] else ""),
                "critic": f"{VL}x{VH} tanh", "layout": layouts["plain"], "same_answer": same_answer,
                "composed_max_abs_dcost": max_dcost, "prewarm_calls": calls}
        for k in sides:
            line[k + "_p50_ms"] = pct(ts[k], 50)
            line[k + "_p10_ms"] = pct(ts[k], 10)
            line[k + "_p90_ms"] = pct(ts[k], 90)
        line["overhead_ms"] = round(line["value_p50_ms"] - line["plain_p50_ms"], 4)
        line["value_kernel_ms"] = round(k_ms, 4)
        line["value_gflops"] = round(flop / 1e9 / (k_ms * 1e-3), 1)
        line["composed_p50_ms"] = pct(tc, 50)
        line["traj_mb"] = round((H + 1) * K * S * 8 / 1e6, 2)
        lines.append(line)
        for e in engines.values():
            e.close()
    out = {"bench": "terminal_value", "weight": WEIGHT, "warmup": WARMUP, "timed": TIMED, "rounds": ROUNDS,
           "event_reps": EVENT_REPS, "composed_reps": COMPOSED_REPS, "device": torch.cuda.get_device_name(0),
           "results": lines}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

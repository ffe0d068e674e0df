#!/usr/bin/env python3
"""What a control step under a model ensemble costs, against composing it by hand.

For E in {1, 3, 5} members at three points, each in one process:

  ppo_defaults  K = 400,    H = 7,  2 x 256 relu + LayerNorm
  cfg2          K = 4,096,  H = 20, 2 x 500 tanh
  cfg3          K = 65,536, H = 20, 2 x 500 tanh

two ways to the same answer (rule "mean"):

  ensemble  EnsembleEngine.get_action: E rollouts, one reduce, one argmin on one stream, one synchronisation
  composed  what a user can do without the ensemble entry points: E RolloutEngine.get_action(return_costs=True)
            calls in a row on E engines (E synchronisations, E cost-vector copies), then ensemble.combine and
            np.argmin on the host

Per (point, E):

  ensemble_p50_ms / composed_p50_ms   p50 of the synchronous call (in-kernel Philox actions)
  speedup                             composed / ensemble
  single_p50_ms                       one RolloutEngine.get_action without the cost vector (the E = 1 yardstick)
  reduce_ms                           device time of ensemble_reduce_kernel alone between two HIP events, median;
                                      reduce_gbs: its E x K f64 read + K f64 write over that time
  same_answer                         both sides returned the same winner and the same values, bit for bit

A prewarm past the clock ramp, 20 warm-up calls of each side, then 200 timed calls of each side in four
alternating rounds of 50, so that a drift of the shared machine falls on both.

Prints one JSON line (profiles/ensemble.json is a committed run).  Needs the GPU: no fallback.
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
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True),
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False),
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False),
}
MEMBERS = (1, 3, 5)
WARMUP, TIMED, ROUNDS = 20, 200, 4
PREWARM_S = 0.25
EVENT_REPS = 50


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", nargs="+", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--members", nargs="+", type=int, default=list(MEMBERS))
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_ensemble: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd import ensemble
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    dev = torch.device("cuda", 0)
    norm = orc.synthetic_normalization(S, A)
    state = orc.synthetic_state(norm)
    lines = []
    for name in args.points:
        p = POINTS[name]
        K, H = p["K"], p["H"]
        for E in args.members:
            specs = []
            for e in range(E):
                w = orc.synthetic_weights(S, A, p["hidden"], 2, p["act"], p["ln"], seed_base=1000 + 100 * e)
                specs.append(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma if p["ln"] else None,
                                     w.ln_beta if p["ln"] else None))
            ens = ensemble.EnsembleEngine(E, S, A, p["hidden"], 2, p["act"], p["ln"], H, K, device=0)
            singles = []
            for e in range(E):
                ens.set_weights(e, specs[e], norm, 1)
                one = RolloutEngine(S, A, p["hidden"], 2, p["act"], p["ln"], H, K, device=0)
                one.set_weights(specs[e], norm, 1)
                singles.append(one)
            layout = ens.info()["layout"]
            assert all(one.info()["layout"] == layout for one in singles)

            def run_ensemble(seed):
                return ens.get_action(state, None, seed=seed)

            def run_composed(seed):
                costs = [one.get_action(state, None, seed=seed, return_costs=True).costs for one in singles]
                v = ensemble.combine(np.stack(costs), "mean")
                return int(np.argmin(v)), v

            def run_single(seed):
                return singles[0].get_action(state, None, seed=seed)

            got = ens.get_action(state, None, seed=7, return_costs=True)
            j, v = run_composed(7)
            same = bool(got.best_index == j and got.costs.tobytes() == v.tobytes())

            sides = {"ensemble": run_ensemble, "composed": run_composed, "single": run_single}
            t0, calls = time.perf_counter(), 0
            while time.perf_counter() - t0 < PREWARM_S or calls < 3:
                run_ensemble(1 << 40 | calls)
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

            # the reduce alone, between HIP events on one stream
            f64 = dict(dtype=torch.float64, device=dev)
            d_mc = torch.from_numpy(np.random.RandomState(E).randn(E, K)).to(dev)
            d_v = torch.empty(K, **f64)
            st = torch.cuda.current_stream(dev).cuda_stream

            def reduce():
                ens.reduce_async(d_mc.data_ptr(), K, E, K, "mean", 0.0, d_v.data_ptr(), st)

            def event_ms(fn):
                x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                x.record()
                fn()
                y.record()
                y.synchronize()
                return x.elapsed_time(y)

            for _ in range(5):
                reduce()
            torch.cuda.synchronize()
            red_ms = float(np.median([event_ms(reduce) for _ in range(EVENT_REPS)]))
            line = {"point": name, "K": K, "H": H, "E": E,
                    "net": f"2x{p['hidden']} {p['act']}" + (" + LayerNorm" if p["ln"] else ""), "layout": layout,
                    "same_answer": same, "prewarm_calls": calls}
            for k in sides:
                line[k + "_p50_ms"] = pct(ts[k], 50)
                line[k + "_p10_ms"] = pct(ts[k], 10)
                line[k + "_p90_ms"] = pct(ts[k], 90)
            line["speedup"] = round(line["composed_p50_ms"] / line["ensemble_p50_ms"], 3)
            line["reduce_ms"] = round(red_ms, 4)
            line["reduce_mb"] = round((E + 1) * K * 8 / 1e6, 3)
            line["reduce_gbs"] = round((E + 1) * K * 8 / 1e9 / (red_ms * 1e-3), 1) if red_ms > 0 else None
            lines.append(line)
            ens.close()
            for one in singles:
                one.close()
    out = {"bench": "ensemble", "rule": "mean", "warmup": WARMUP, "timed": TIMED, "rounds": ROUNDS,
           "event_reps": EVENT_REPS, "device": torch.cuda.get_device_name(0), "results": lines}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

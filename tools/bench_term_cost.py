#!/usr/bin/env python3
"""What scoring a control step with declarative cost terms costs beside the fused cheetah cost.

The same objective both ways -- cost_functions.cheetah_terms() on a cost="terms" engine against the fused
cheetah cost on an engine of the same kernel layout -- at three points, each in one process:

  cfg3          K = 65,536, H = 20, 2 x 500 tanh
  cfg2          K = 4,096,  H = 20, 2 x 500 tanh
  ppo_defaults  K = 400,    H = 7,  2 x 256 relu + LayerNorm

Per point:

  fused_p50_ms / terms_p50_ms   p50 of the synchronous RolloutEngine.get_action (in-kernel Philox actions)
  overhead_ms                   their difference: trajectory write + term_cost_kernel + its launch
  cost_ms                       device time of term_cost_kernel alone (trajectory_cost_async on the trajectory
                                of a rollout) between two HIP events, median; cost_gbs: its [H+1][K][S] f64
                                read over that time
  cost_dense_ms                 the same for a cost that reads everything: a linear term on each of the 20 state
                                dims and a quadratic one on each of the 6 actions, regenerated from Philox
                                (26 slots: the widest kernel instance, one row in flight)
  rollout_ms / rollout_traj_ms  device time of the fused engine's rollout_async without / with the
                                trajectory write (d_traj), between two HIP events, median

Every synchronous call ends in its own host synchronisation, so the host clock around it is its latency.
A prewarm past the clock ramp (as bench.py's), 20 warm-up calls of each side, then 200 timed calls of each
side in four alternating rounds of 50, so that a drift of the shared machine falls on both.

Prints one JSON line (profiles/term_cost.json is a committed run).  Needs the GPU: no fallback.
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


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", nargs="+", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_term_cost: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd.cost_functions import TermCost, cheetah_terms, linear, quadratic
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    dev = torch.device("cuda", 0)
    norm = orc.synthetic_normalization(S, A)
    state = orc.synthetic_state(norm)
    lines = []
    for name in args.points:
        p = POINTS[name]
        K, H = p["K"], p["H"]
        w = orc.synthetic_weights(S, A, p["hidden"], 2, p["act"], p["ln"])
        spec = MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma if p["ln"] else None,
                       w.ln_beta if p["ln"] else None)
        engines = {}
        for side in ("fused", "terms"):
            e = RolloutEngine(S, A, p["hidden"], 2, p["act"], p["ln"], H, K, device=0,
                              cost="cheetah" if side == "fused" else "terms")
            e.set_weights(spec, norm, 1)
            engines[side] = e
        engines["terms"].set_cost_terms(cheetah_terms())
        layouts = {k: e.info()["layout"] for k, e in engines.items()}
        assert layouts["terms"] == layouts["fused"] + "+terms", layouts
        a, b = (engines[k].get_action(state, None, seed=7, return_costs=True) for k in ("fused", "terms"))
        bitwise = bool(np.array_equal(a.costs, b.costs)) and a.best_index == b.best_index

        sides = {k: (lambda seed, e=e: e.get_action(state, None, seed=seed)) for k, e in engines.items()}
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < PREWARM_S or calls < 3:
            sides["terms"](1 << 40 | calls)
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

        # the launches alone, between HIP events on one stream
        f64 = dict(dtype=torch.float64, device=dev)
        d_state = torch.from_numpy(np.ascontiguousarray(state)).to(dev)
        d_costs, d_costs2 = torch.empty(K, **f64), torch.empty(K, **f64)
        d_traj = torch.empty((H + 1, K, S), **f64)
        st = torch.cuda.current_stream(dev).cuda_stream
        fused, terms = engines["fused"], engines["terms"]

        def rollout():
            fused.rollout_async(d_state.data_ptr(), 0, None, 5, 0, d_costs.data_ptr(), None, None, st)

        def rollout_traj():
            fused.rollout_async(d_state.data_ptr(), 0, None, 5, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, st)

        def cost():
            terms.trajectory_cost_async(d_traj.data_ptr(), K, d_costs2.data_ptr(), stream=st)

        def event_ms(fn):
            x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            x.record()
            fn()
            y.record()
            y.synchronize()
            return x.elapsed_time(y)

        for _ in range(5):
            rollout()
            rollout_traj()
            cost()
        torch.cuda.synchronize()
        r_ms = [event_ms(rollout) for _ in range(EVENT_REPS)]
        rt_ms = [event_ms(rollout_traj) for _ in range(EVENT_REPS)]
        c_ms = [event_ms(cost) for _ in range(EVENT_REPS)]
        terms.set_cost_terms(TermCost([linear(i, 0.01) for i in range(S)]
                                      + [quadratic(j, 0.1, on="action") for j in range(A)]))
        for _ in range(5):
            cost()
        torch.cuda.synchronize()
        cd_ms = [event_ms(cost) for _ in range(EVENT_REPS)]
        fused.check_status()
        cost_ms = float(np.median(c_ms))
        traj_bytes = (H + 1) * K * S * 8
        line = {"point": name, "K": K, "H": H, "net": f"2x{p['hidden']} {p['act']}" + (" + LayerNorm" if p["ln"] else ""),
                "layout": layouts["fused"], "costs_bitwise_equal_fused": bitwise, "prewarm_calls": calls}
        for k in sides:
            line[k + "_p50_ms"] = pct(ts[k], 50)
            line[k + "_p10_ms"] = pct(ts[k], 10)
            line[k + "_p90_ms"] = pct(ts[k], 90)
        line["overhead_ms"] = round(line["terms_p50_ms"] - line["fused_p50_ms"], 4)
        line["rollout_ms"] = round(float(np.median(r_ms)), 4)
        line["rollout_traj_ms"] = round(float(np.median(rt_ms)), 4)
        line["cost_ms"] = round(cost_ms, 4)
        line["cost_dense_ms"] = round(float(np.median(cd_ms)), 4)
        line["traj_mb"] = round(traj_bytes / 1e6, 2)
        line["cost_gbs"] = round(traj_bytes / 1e9 / (cost_ms * 1e-3), 1)
        lines.append(line)
        for e in engines.values():
            e.close()
    out = {"bench": "term_cost", "terms": "cheetah_terms()", "warmup": WARMUP, "timed": TIMED, "rounds": ROUNDS,
           "event_reps": EVENT_REPS, "device": torch.cuda.get_device_name(0), "results": lines}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

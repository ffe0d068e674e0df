#!/usr/bin/env python3
"""What an MPPI control step costs beside CEM and plain random shooting, and the update kernels alone.

Three points, each on one engine shape, in one process:

  cfg3          K = 65,536, H = 20, 2 x 500 tanh
  ppo_defaults  K = 400,    H = 7,  2 x 256 relu + LayerNorm
  cfg2          K = 4,096,  H = 20, 2 x 500 tanh   (the update's 64-candidate workgroups with real work each)

Per point:

  mppi_p50_ms    p50 of the synchronous RolloutEngine.mppi_get_action(iterations=1)
  cem_p50_ms     p50 of RolloutEngine.cem_get_action(iterations=1, n_elite = K / 10)
  plain_p50_ms   p50 of RolloutEngine.get_action with in-kernel (Philox) actions
  update_ms      device time of one mppi_update_async (its three launches) between two HIP events, median
  update_x20_ms  ... of 20 updates enqueued back to back between one event pair, per update
  rollout_ms     device time of one cem_rollout_async (rollout + argmin) between two HIP events, median
  update_share   update_ms / rollout_ms: the update against the rollout kernel's own time in the same run

Every synchronous call ends in its own host synchronisation, so the host clock around it is its latency.
A prewarm past the clock ramp (as bench.py's), 20 warm-up calls of each side, then 200 timed calls of each
side in four alternating rounds of 50, so that a drift of the shared machine falls on all three.

Prints one JSON line (profiles/mppi_step.json is a committed run).  Needs the GPU: no fallback.
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
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False, lam=10.0),
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True, lam=10.0),
    # below the update's 16,384-candidate threshold with real work per workgroup: 64-candidate stage-1 workgroups
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False, lam=10.0),
}
WARMUP, TIMED, ROUNDS = 20, 200, 4
PREWARM_S = 0.25
EVENT_REPS, CHAIN = 50, 20


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", nargs="+", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mppi: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    dev = torch.device("cuda", 0)
    norm = orc.synthetic_normalization(S, A)
    state = orc.synthetic_state(norm)
    lines = []
    for name in args.points:
        p = POINTS[name]
        K, H, lam = p["K"], p["H"], p["lam"]
        w = orc.synthetic_weights(S, A, p["hidden"], 2, p["act"], p["ln"])
        spec = MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma if p["ln"] else None,
                       w.ln_beta if p["ln"] else None)
        eng = RolloutEngine(S, A, p["hidden"], 2, p["act"], p["ln"], H, K, device=0)
        eng.set_weights(spec, norm, 1)
        mu0, sd0 = np.zeros((H, A)), np.full((H, A), 0.5)
        E = max(1, K // 10)

        def mppi(seed):
            return eng.mppi_get_action(state, mu0, sd0, 1, lam, seed)

        def cem(seed):
            return eng.cem_get_action(state, mu0, sd0, 1, E, 0.1, seed)

        def plain(seed):
            return eng.get_action(state, None, seed=seed)

        sides = {"mppi": mppi, "cem": cem, "plain": plain}
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < PREWARM_S or calls < 3:
            mppi(1 << 40 | calls)
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
        _, _, stats = mppi(7)

        # the launches alone, between HIP events on one stream
        f64 = dict(dtype=torch.float64, device=dev)
        d_state = torch.from_numpy(np.ascontiguousarray(state)).to(dev)
        d_mu, d_sd = torch.from_numpy(mu0.copy()).to(dev), torch.from_numpy(sd0.copy()).to(dev)
        d_costs = torch.empty(K, **f64)
        d_res = torch.zeros(64 + 8 * _lib.MAX_ACTION, dtype=torch.uint8, device=dev)
        d_stats = torch.zeros(32, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream

        def rollout():
            eng.cem_rollout_async(d_state.data_ptr(), d_mu.data_ptr(), d_sd.data_ptr(), 5, 0, 0, K,
                                  d_costs.data_ptr(), d_res.data_ptr(), False, st)

        def update():
            eng.mppi_update_async(d_costs.data_ptr(), K, 0, 5, 0, lam, d_mu.data_ptr(), d_sd.data_ptr(),
                                  d_stats.data_ptr(), st)

        def event_ms(fn, n=1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / n

        for _ in range(5):
            rollout()
            update()
        torch.cuda.synchronize()
        r_ms = [event_ms(rollout) for _ in range(EVENT_REPS)]
        d_mu.copy_(torch.from_numpy(mu0))
        u_ms = [event_ms(update) for _ in range(EVENT_REPS)]
        c_ms = [event_ms(update, CHAIN) for _ in range(EVENT_REPS)]
        eng.check_status()
        line = {"point": name, "K": K, "H": H, "net": f"2x{p['hidden']} {p['act']}" + (" + LayerNorm" if p["ln"] else ""),
                "layout": eng.info()["layout"], "lambda": lam, "n_elite": E,
                "ess": round(float(stats.ess), 1), "n_valid": int(stats.n_valid), "prewarm_calls": calls}
        for k in sides:
            line[k + "_p50_ms"] = pct(ts[k], 50)
            line[k + "_p10_ms"] = pct(ts[k], 10)
            line[k + "_p90_ms"] = pct(ts[k], 90)
        line["rollout_ms"] = round(float(np.median(r_ms)), 4)
        line["update_ms"] = round(float(np.median(u_ms)), 4)
        line["update_x20_ms"] = round(float(np.median(c_ms)), 4)
        line["update_share"] = round(float(np.median(u_ms) / np.median(r_ms)), 4)
        lines.append(line)
        eng.close()
    out = {"bench": "mppi_step", "warmup": WARMUP, "timed": TIMED, "rounds": ROUNDS, "event_reps": EVENT_REPS,
           "device": torch.cuda.get_device_name(0), "results": lines}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

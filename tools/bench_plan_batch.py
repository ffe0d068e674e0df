#!/usr/bin/env python3
"""Batched CEM / MPPI against B sequential single-environment calls, at train_mpc_ppo.py's own defaults.

Workload: the ppo_defaults net (2 x 256 relu + LayerNorm, H = 7, K = 400 candidates per environment),
B in {1, 8, 64, 256} environments; planners CEM x1, CEM x4 (E = K / 10, alpha 0.1) and MPPI x1 (lambda 1).
For each (planner, B), in one process:

  batched     p50 of the synchronous RolloutEngine.cem_get_actions / mppi_get_actions on a B*400-candidate
              engine (one plan per environment)
  sequential  p50 of B RolloutEngine.cem_get_action / mppi_get_action calls in a row on one 400-candidate engine

Both sides sample in Philox and end in the call's own host synchronisation, so the host clock around a call
is the call's latency.  Per (planner, B): a prewarm of the batched call past the clock ramp, 10 warm-up calls
of each side, then the timed calls of each side in four alternating rounds, so that a drift of the shared
machine falls on both; p10 and p90 are reported beside each p50.

Per B, the chain's launches are also timed between HIP events on the building blocks (median of 30): the
sampling kernel, the rollout (explicit actions, per-candidate states), the per-environment argmin, select +
refit and the MPPI update -- the last two in both forms, reading the stored action array and regenerating
the samples from Philox.

Prints one JSON line (profiles/plan_batch_ppo_defaults.json is a committed run).  Needs the GPU: no fallback.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

S, A, HIDDEN, H, K = 20, 6, 256, 7, 400
E, ALPHA, LAMBDA = K // 10, 0.1, 1.0
WARMUP, ROUNDS = 10, 4
PREWARM_S = 0.25
PLANNERS = [("cem", 1), ("cem", 4), ("mppi", 1)]


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def kernel_times(eng, states, mu, sd, B, reps=30):
    """Device time of each launch group of one iteration, between HIP events on torch's stream."""
    import torch
    from bc_mpc_amd import _lib
    from bc_mpc_amd.engine import MPPI_STATS
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    d_tiled = torch.from_numpy(np.repeat(states, K, axis=0)).to(dev)
    d_mu, d_sd = torch.from_numpy(mu.copy()).to(dev), torch.from_numpy(sd.copy()).to(dev)
    d_act = torch.empty((H, B * K, A), **f64)
    d_costs = torch.empty(B * K, **f64)
    d_res = torch.zeros(B * ctypes.sizeof(_lib.Result), dtype=torch.uint8, device=dev)
    d_el = torch.zeros(B * E * 16, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    d_stats = torch.zeros(B * MPPI_STATS.itemsize, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    # (the refit and the update change the plans in place: each rep restores them first, outside the events)
    steps = {
        "sample": lambda: eng.plan_sample_async(p(d_mu), p(d_sd), B, K, 1, 0, 0, p(d_act), st),
        "rollout": lambda: eng.rollout_async(p(d_tiled), S, p(d_act), 1, 0, p(d_costs), None, None, st),
        "argmin": lambda: eng.plan_argmin_async(p(d_costs), p(d_act), B, K, 0, False, p(d_res), st),
        "select": lambda: eng.select_batch_async(p(d_costs), B, K, 0, E, p(d_el), p(d_cnt), st),
        "refit_stored": lambda: eng.cem_refit_batch_async(p(d_el), p(d_cnt), B, E, 1, 0, ALPHA, p(d_mu), p(d_sd),
                                                          p(d_act), K, 0, st),
        "refit_philox": lambda: eng.cem_refit_batch_async(p(d_el), p(d_cnt), B, E, 1, 0, ALPHA, p(d_mu), p(d_sd),
                                                          None, K, 0, st),
        "mppi_update_stored": lambda: eng.mppi_update_batch_async(p(d_costs), B, K, 0, 1, 0, LAMBDA, p(d_mu), p(d_sd),
                                                                  p(d_stats), p(d_act), st),
        "mppi_update_philox": lambda: eng.mppi_update_batch_async(p(d_costs), B, K, 0, 1, 0, LAMBDA, p(d_mu),
                                                                  p(d_sd), p(d_stats), None, st),
    }
    mu_t, sd_t = torch.from_numpy(mu.copy()).to(dev), torch.from_numpy(sd.copy()).to(dev)
    out = {}
    for name, fn in steps.items():
        ms = []
        for _ in range(reps + 3):
            d_mu.copy_(mu_t)
            d_sd.copy_(sd_t)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out[name + "_us"] = round(float(np.median(ms[3:])) * 1e3, 2)
    eng.check_status()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_plan_batch: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    w = orc.synthetic_weights(S, A, HIDDEN, 2, "relu", True)
    norm = orc.synthetic_normalization(S, A)
    spec = MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta)

    def engine(k):
        e = RolloutEngine(S, A, HIDDEN, 2, "relu", True, H, k, device=0)
        e.set_weights(spec, norm, 1)
        return e

    one = engine(K)
    lines = []
    for B in args.envs:
        states = np.stack([orc.synthetic_state(norm, seed=11 + b) for b in range(B)])
        rs = np.random.RandomState(B)
        mu, sd = rs.uniform(-0.3, 0.3, (B, H, A)), np.full((B, H, A), 0.5)
        eng = engine(B * K)
        timed = 200 if B <= 8 else 80
        for planner, iters in PLANNERS:
            if planner == "cem":
                def batched(seed):
                    return eng.cem_get_actions(states, mu, sd, iters, E, ALPHA, seed)

                def sequential(seed):
                    return [one.cem_get_action(states[b], mu[b], sd[b], iters, E, ALPHA, seed) for b in range(B)]
            else:
                def batched(seed):
                    return eng.mppi_get_actions(states, mu, sd, iters, LAMBDA, seed)

                def sequential(seed):
                    return [one.mppi_get_action(states[b], mu[b], sd[b], iters, LAMBDA, seed) for b in range(B)]
            t0, calls = time.perf_counter(), 0
            while time.perf_counter() - t0 < PREWARM_S or calls < 3:
                batched(1 << 40 | calls)
                calls += 1
            for i in range(WARMUP):
                batched(1000 + i)
            for i in range(max(2, WARMUP // max(1, B // 8))):
                sequential(1000 + i)
            tb, ts = [], []
            per = timed // ROUNDS
            for rnd in range(ROUNDS):
                for i in range(per):
                    t = time.perf_counter()
                    batched(2000 + rnd * per + i)
                    tb.append(time.perf_counter() - t)
                for i in range(per):
                    t = time.perf_counter()
                    sequential(2000 + rnd * per + i)
                    ts.append(time.perf_counter() - t)
            lines.append({"planner": planner, "iterations": iters, "B": B, "K": K, "timed": timed,
                          "batched_p50_ms": pct(tb, 50), "batched_p10_ms": pct(tb, 10), "batched_p90_ms": pct(tb, 90),
                          "sequential_p50_ms": pct(ts, 50), "sequential_p10_ms": pct(ts, 10),
                          "sequential_p90_ms": pct(ts, 90), "speedup": round(pct(ts, 50) / pct(tb, 50), 2),
                          "prewarm_calls": calls})
        lines.append({"kernels": True, "B": B, "K": K, "batched_layout": eng.info()["layout"],
                      **kernel_times(eng, states, mu, sd, B)})
        eng.close()
    out = {"bench": "plan_batch_ppo_defaults", "net": "2x256 relu + LayerNorm", "H": H, "K_per_env": K, "n_elite": E,
           "alpha": ALPHA, "lambda": LAMBDA, "warmup": WARMUP, "rounds": ROUNDS,
           "sequential_layout": one.info()["layout"], "device": torch.cuda.get_device_name(0), "results": lines}
    one.close()
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What MPPI's control-cost term and the weighted sigma update cost, on one MI355X.

Workloads (bench.py's): ppo_defaults (2 x 256 relu + LayerNorm, K = 400, H = 7), cfg2 (2 x 500 tanh, K = 4096,
H = 20) and cfg3 (that net, K = 65,536).  Per workload, on the K-candidate engine:

  kernels   each new launch alone between HIP events on K columns (median of 30 after 3): mppi_control_cost, the
            sigma update's three launches together (min, partial, final), and for scale the plain update's three
            reading the stored actions (mppi_update_batch_async)
  calls     the synchronous mppi_get_action (ITERATIONS rounds, lambda 1) at the defaults and with the control
            cost only, the sigma update only, and both: p50 (p10, p90) of the host clock around the call, the
            variants in alternating rounds after a prewarm and warm-up calls, so that a drift of the shared machine
            falls on all of them.  The default call is the single-plan chain (the rollout kernel samples for
            itself); every option runs the batched chain at one environment (plan_sample, tile_states, rollout of
            the stored actions), as noise_rho does (profiles/sampling.json prices that chain), so a mode against
            the default is the chain's price plus the new launches', which "kernels" gives alone
  sigma     mean of sigma after the call per mode, from one call each on the same seed -- information on a
            synthetic net, not a criterion

Prints one JSON line (profiles/mppi_ext.json is a committed run).  Needs the GPU: no fallback.
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
LAMBDA, ITERATIONS = 1.0, 2
ROUNDS, PREWARM_S = 4, 0.25
ADAPT = dict(adapt_sigma=True, sigma_alpha=0.1, min_std=0.05)
WORKLOADS = {   # net and shape as bench.py's WORKLOADS; timed calls per variant
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True, timed=200),
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False, timed=120),
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False, timed=40),
}
VARIANTS = [("default", {}), ("control", dict(control_cost=True)), ("adapt", ADAPT),
            ("both", dict(control_cost=True, **ADAPT))]


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def kernel_times(eng, mu, sd, K, H, reps=30):
    """Device time of the new launches, each step alone between HIP events on torch's stream."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    d_mu, d_sd = torch.from_numpy(mu.copy()).to(dev), torch.from_numpy(sd.copy()).to(dev)
    d_new = torch.from_numpy(mu.copy()).to(dev)
    d_act = torch.empty((H, K, A), dtype=torch.float64, device=dev)
    d_costs = torch.from_numpy(3.0 * np.random.RandomState(0).standard_normal(K)).to(dev)
    d_scores = torch.empty(K, dtype=torch.float64, device=dev)
    d_stats = torch.zeros(32, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    eng.plan_sample_async(p(d_mu), p(d_sd), 1, K, 1, 0, 0, p(d_act), st)
    steps = {
        "mppi_control_cost": lambda: eng.mppi_control_cost_async(p(d_costs), p(d_act), 1, K, p(d_mu), p(d_sd), LAMBDA,
                                                                 p(d_scores), st),
        "mppi_sigma_update": lambda: eng.mppi_sigma_update_async(p(d_scores), p(d_act), 1, K, LAMBDA, p(d_new), p(d_sd),
                                                                 0.1, 0.05, None, st),
        "mppi_update_stored": lambda: eng.mppi_update_batch_async(p(d_scores), 1, K, 0, 1, 0, LAMBDA, p(d_new), p(d_sd),
                                                                  p(d_stats), p(d_act), st),
    }
    out = {}
    for name, fn in steps.items():
        ms = []
        for _ in range(reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out[name + "_us"] = round(float(np.median(ms[3:])) * 1e3, 2)
    return out


def call_times(eng, state, mu, sd, timed):
    """p50 / p10 / p90 per variant of the synchronous call, alternating rounds."""
    def call(kw, seed):
        return eng.mppi_get_action(state, mu, sd, ITERATIONS, LAMBDA, seed, **kw)

    t0, calls = time.perf_counter(), 0
    while time.perf_counter() - t0 < PREWARM_S or calls < 3:
        call(VARIANTS[calls % len(VARIANTS)][1], 1 << 40 | calls)
        calls += 1
    for i in range(5):
        for _, kw in VARIANTS:
            call(kw, 1000 + i)
    ts = {name: [] for name, _ in VARIANTS}
    per = max(1, timed // ROUNDS)
    for rnd in range(ROUNDS):
        for name, kw in VARIANTS:
            for i in range(per):
                t = time.perf_counter()
                call(kw, 2000 + rnd * per + i)
                ts[name].append(time.perf_counter() - t)
    row = {"iterations": ITERATIONS, "timed": per * ROUNDS, "prewarm_calls": calls}
    for name, _ in VARIANTS:
        row[name] = {"p50_ms": pct(ts[name], 50), "p10_ms": pct(ts[name], 10), "p90_ms": pct(ts[name], 90)}
        if name != "default":
            row[name]["vs_default"] = round(row[name]["p50_ms"] / row["default"]["p50_ms"], 4)
            row[name]["over_default_us"] = round((row[name]["p50_ms"] - row["default"]["p50_ms"]) * 1e3, 2)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mppi_ext: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    norm = orc.synthetic_normalization(S, A)
    state = orc.synthetic_state(norm)
    lines = []
    for wname in args.workloads:
        wl = WORKLOADS[wname]
        K, H = wl["K"], wl["H"]
        w = orc.synthetic_weights(S, A, wl["hidden"], 2, wl["act"], wl["ln"])
        eng = RolloutEngine(S, A, wl["hidden"], 2, wl["act"], wl["ln"], H, K, device=0)
        eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta), norm, 1)
        rs = np.random.RandomState(1)
        mu, sd = rs.uniform(-0.3, 0.3, (H, A)), np.full((H, A), 0.5)
        row = {"workload": wname, "K": K, "H": H, "layout": eng.info()["layout"],
               "kernels": kernel_times(eng, mu, sd, K, H), "calls": call_times(eng, state, mu, sd, wl["timed"]),
               "sigma_mean_after": {}}
        for name, kw in VARIANTS:
            out = eng.mppi_get_action(state, mu, sd, ITERATIONS, LAMBDA, 4242, **kw)
            row["sigma_mean_after"][name] = round(float(np.mean(out[3] if len(out) == 4 else sd)), 4)
        eng.check_status()
        eng.close()
        lines.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"bench": "mppi_ext", "lambda": LAMBDA, "control_cost": "True (the temperature)", "adapt": ADAPT,
           "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "results": lines}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

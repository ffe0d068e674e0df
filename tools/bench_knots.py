#!/usr/bin/env python3
"""What knot plans cost, on one MI355X.

Workloads (bench.py's): ppo_defaults (2 x 256 relu + LayerNorm, K = 400, H = 7), cfg2 (2 x 500 tanh, K = 4096,
H = 20) and cfg3 (that net, K = 65,536), one environment, M = 5 knots, linear interpolation:

  kernels   plan_sample_knots against plan_sample_corr (rho = 0.5, unchanged from before knots), each alone between
            HIP events on K columns.  The two alternate in one process: REPEATS rounds of 50 launches each after a
            prewarm, one median per round.  Reported: the median of the round medians and, as the margin, the spread
            (max - min) of plan_sample_corr's own round medians
  calls     the synchronous CEM x4 (E = K / 10, alpha 0.1) and MPPI x2 (lambda 1) single calls with knots, with
            noise_rho = 0.5 and no knots (the stored-array chain knots share) and at the defaults: p50 (p10, p90) of
            the host clock around the call, the variants in alternating rounds after a prewarm and warm-up calls
  best      the best cost of the LAST iteration with knots off and on, at equal K and seed -- recorded only: the
            net is synthetic, there is no bar

Prints one JSON line (profiles/knots.json is a committed run).  Needs the GPU: no fallback.
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
ALPHA, LAMBDA, RHO, M, KIND = 0.1, 1.0, 0.5, 5, "linear"
ROUNDS, PREWARM_S, REPEATS, REPS = 4, 0.25, 5, 50
WORKLOADS = {   # net and shape as bench.py's WORKLOADS; timed calls per variant
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True, timed=200),
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False, timed=120),
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False, timed=40),
}
VARIANTS = [("default", {}), ("rho", dict(rho=RHO)), ("knots", dict(knots=M, knot_interp=KIND))]
PLANNERS = [("cem", 4), ("mppi", 2)]


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def kernel_times(eng, K, H):
    """Device time of plan_sample_knots and plan_sample_corr, alternating, between HIP events on torch's stream."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    rs = np.random.RandomState(1)
    d_mu = torch.from_numpy(rs.uniform(-0.3, 0.3, (1, H, A))).to(dev)     # (the knot sampler reads its first M rows)
    d_sd = torch.full((1, H, A), 0.5, dtype=torch.float64, device=dev)
    d_act = torch.empty((H, K, A), dtype=torch.float64, device=dev)
    d_kn = torch.empty((M, K, A), dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    steps = {
        "plan_sample_corr": lambda: eng.plan_sample_corr_async(p(d_mu), p(d_sd), 1, K, 1, 1, 0, RHO, p(d_act), stream=st),
        "plan_sample_knots": lambda: eng.plan_sample_knots_async(p(d_mu), p(d_sd), 1, K, 1, 1, 0, RHO, M, KIND, p(d_kn),
                                                                 p(d_act), stream=st),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < PREWARM_S:
        for fn in steps.values():
            timed(fn)
    meds = {name: [] for name in steps}
    for _ in range(REPEATS):
        for name, fn in steps.items():
            meds[name].append(float(np.median([timed(fn) for _ in range(REPS)])) * 1e3)
    out = {name + "_us": round(float(np.median(v)), 2) for name, v in meds.items()}
    out.update({name + "_round_medians_us": [round(x, 2) for x in v] for name, v in meds.items()})
    out["margin_us"] = round(max(meds["plan_sample_corr"]) - min(meds["plan_sample_corr"]), 2)
    out["knots_minus_corr_us"] = round(out["plan_sample_knots_us"] - out["plan_sample_corr_us"], 2)
    return out


def plans_for(kw, mu, sd):
    return (mu[:M], sd[:M]) if "knots" in kw else (mu, sd)


def call_times(eng, planner, iters, state, mu, sd, E, timed):
    """p50 / p10 / p90 per variant of the synchronous single call, in alternating rounds."""
    def call(kw, seed):
        m, s = plans_for(kw, mu, sd)
        if planner == "cem":
            return eng.cem_get_action(state, m, s, iters, E, ALPHA, seed, **kw)
        return eng.mppi_get_action(state, m, s, iters, LAMBDA, seed, **kw)

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
    row = {"planner": planner, "iterations": iters, "timed": per * ROUNDS, "prewarm_calls": calls}
    for name, _ in VARIANTS:
        row[name] = {"p50_ms": pct(ts[name], 50), "p10_ms": pct(ts[name], 10), "p90_ms": pct(ts[name], 90)}
    for name in ("rho", "default"):
        row["knots"]["vs_" + name] = round(row["knots"]["p50_ms"] / row[name]["p50_ms"], 4)
    return row


def best_costs(eng, planner, iters, state, mu, sd, E):
    """The last iteration's best cost per variant, on one seed (the one-environment batched call returns the costs)."""
    out = {}
    for name, kw in VARIANTS:
        m, s = plans_for(kw, mu, sd)
        if planner == "cem":
            res, _, _ = eng.cem_get_actions(state[None], m[None], s[None], iters, E, ALPHA, 4242, 0, True, **kw)
        else:
            res, _, _ = eng.mppi_get_actions(state[None], m[None], s[None], iters, LAMBDA, 4242, 0, True, **kw)
        out[name] = round(float(res.costs[-1].min()), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_knots: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    norm = orc.synthetic_normalization(S, A)
    lines = []
    for wname in args.workloads:
        wl = WORKLOADS[wname]
        K, H, E = wl["K"], wl["H"], wl["K"] // 10
        w = orc.synthetic_weights(S, A, wl["hidden"], 2, wl["act"], wl["ln"])
        eng = RolloutEngine(S, A, wl["hidden"], 2, wl["act"], wl["ln"], H, K, device=0)
        eng.set_weights(MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta), norm, 1)
        state = orc.synthetic_state(norm, seed=11)
        mu, sd = np.zeros((H, A)), np.full((H, A), 0.5)
        row = {"workload": wname, "K": K, "H": H, "knots": M, "interp": KIND, "n_elite": E,
               "layout": eng.info()["layout"], "kernels": kernel_times(eng, K, H), "calls": [],
               "best_last_iteration": {}}
        for planner, iters in PLANNERS:
            row["calls"].append(call_times(eng, planner, iters, state, mu, sd, E, wl["timed"]))
            row["best_last_iteration"][planner] = best_costs(eng, planner, iters, state, mu, sd, E)
        eng.check_status()
        eng.close()
        lines.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"bench": "knots", "knots": M, "interp": KIND, "rho": RHO, "alpha": ALPHA, "lambda": LAMBDA, "rounds": ROUNDS,
           "kernel_repeats": REPEATS, "kernel_reps": REPS, "device": torch.cuda.get_device_name(0), "results": lines}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What correlated sampling noise and the CEM elite carry-over cost, on one MI355X.

Workloads (bench.py's): ppo_defaults (2 x 256 relu + LayerNorm, K = 400, H = 7), cfg2 (2 x 500 tanh, K = 4096,
H = 20) and cfg3 (that net, K = 65,536).  Per workload, single (the K-candidate engine's cem_get_action /
mppi_get_action) and batched (B environments of K candidates each, cem_get_actions / mppi_get_actions; B = 64,
cfg3: B = 4, the largest candidate count bench.py runs):

  kernels   plan_sample, plan_sample_corr (rho = 0.5), plan_sample_corr with a full keep buffer and plan_keep, each
            alone between HIP events on n_envs * K columns (median of 30 after 3)
  calls     the synchronous CEM x4 (E = K / 10, alpha 0.1) and MPPI x1 (lambda 1) calls at the defaults, at
            rho = 0.5 and (CEM) at rho = 0.5 with carry-over: p50 (p10, p90) of the host clock around the call,
            the variants in alternating rounds after a prewarm and warm-up calls, so that a drift of the shared
            machine falls on all of them
  best      the mean over the environments of the best cost of the LAST iteration, per variant, from one call
            each on the same seed -- information on a synthetic net, not a criterion

Prints one JSON line (profiles/sampling.json is a committed run).  Needs the GPU: no fallback.
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
ALPHA, LAMBDA, RHO = 0.1, 1.0, 0.5
ROUNDS, PREWARM_S = 4, 0.25
WORKLOADS = {   # net and shape as bench.py's WORKLOADS; B of the batched side; timed calls (single, batched)
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True, B=64, timed=(200, 80)),
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False, B=64, timed=(120, 40)),
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False, B=4, timed=(40, 16)),
}
VARIANTS = {"cem": [("default", {}), ("rho", dict(rho=RHO)), ("rho_keep", dict(rho=RHO, keep_elites=True))],
            "mppi": [("default", {}), ("rho", dict(rho=RHO))]}
PLANNERS = [("cem", 4), ("mppi", 1)]


def pct(ts, q):
    return round(float(np.percentile(np.asarray(ts), q) * 1e3), 4)


def kernel_times(eng, mu, sd, B, K, H, E, reps=30):
    """Device time of the sampling kernels and of plan_keep, each alone between HIP events on torch's stream."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    d_mu, d_sd = torch.from_numpy(mu.copy()).to(dev), torch.from_numpy(sd.copy()).to(dev)
    d_act = torch.empty((H, B * K, A), dtype=torch.float64, device=dev)
    d_keep = torch.zeros((B, E, H, A), dtype=torch.float64, device=dev)
    d_kc = torch.full((B,), E, dtype=torch.int32, device=dev)
    d_cnt = torch.full((B,), E, dtype=torch.int32, device=dev)
    el = np.zeros((B, E), dtype=np.dtype([("cost", "<f8"), ("index", "<i8")]))
    el["index"] = (np.arange(B)[:, None] * K + np.arange(E)[None, :] * (K // E))   # E columns spread over each K
    d_el = torch.from_numpy(el.view(np.uint8).reshape(-1).copy()).to(dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    steps = {
        "plan_sample": lambda: eng.plan_sample_async(p(d_mu), p(d_sd), B, K, 1, 1, 0, p(d_act), st),
        "plan_sample_corr": lambda: eng.plan_sample_corr_async(p(d_mu), p(d_sd), B, K, 1, 1, 0, RHO, p(d_act), stream=st),
        "plan_sample_corr_keep": lambda: eng.plan_sample_corr_async(p(d_mu), p(d_sd), B, K, 1, 1, 0, RHO, p(d_act),
                                                                    p(d_keep), p(d_kc), E, st),
        "plan_keep": lambda: eng.plan_keep_async(p(d_el), p(d_cnt), p(d_act), B, K, 0, E, p(d_keep), p(d_kc), st),
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
    assert (d_kc.cpu().numpy() == E).all()
    return out


def call_times(eng, planner, iters, states, mu, sd, E, timed, single):
    """p50 / p10 / p90 per variant of the synchronous call, alternating rounds; the last iteration's best cost."""
    def call(kw, seed, costs=False):
        if single and planner == "cem":
            return eng.cem_get_action(states[0], mu[0], sd[0], iters, E, ALPHA, seed, **kw)
        if single:
            return eng.mppi_get_action(states[0], mu[0], sd[0], iters, LAMBDA, seed, **kw)
        if planner == "cem":
            return eng.cem_get_actions(states, mu, sd, iters, E, ALPHA, seed, 0, costs, **kw)
        return eng.mppi_get_actions(states, mu, sd, iters, LAMBDA, seed, 0, costs, **kw)

    variants = VARIANTS[planner]
    t0, calls = time.perf_counter(), 0
    while time.perf_counter() - t0 < PREWARM_S or calls < 3:
        call(variants[calls % len(variants)][1], 1 << 40 | calls)
        calls += 1
    for i in range(5):
        for _, kw in variants:
            call(kw, 1000 + i)
    ts = {name: [] for name, _ in variants}
    per = max(1, timed // ROUNDS)
    for rnd in range(ROUNDS):
        for name, kw in variants:
            for i in range(per):
                t = time.perf_counter()
                call(kw, 2000 + rnd * per + i)
                ts[name].append(time.perf_counter() - t)
    row = {"planner": planner, "iterations": iters, "timed": per * ROUNDS, "prewarm_calls": calls}
    for name, _ in variants:
        row[name] = {"p50_ms": pct(ts[name], 50), "p10_ms": pct(ts[name], 10), "p90_ms": pct(ts[name], 90)}
        if name != "default":
            row[name]["vs_default"] = round(row[name]["p50_ms"] / row["default"]["p50_ms"], 4)
    return row


def best_costs(eng, planner, iters, states, mu, sd, E):
    """The mean over the environments of the last iteration's best cost, per variant, on one seed."""
    out = {}
    for name, kw in VARIANTS[planner]:
        if planner == "cem":
            res, _, _ = eng.cem_get_actions(states, mu, sd, iters, E, ALPHA, 4242, 0, True, **kw)
        else:
            res, _, _ = eng.mppi_get_actions(states, mu, sd, iters, LAMBDA, 4242, 0, True, **kw)
        out[name] = round(float(np.mean(res.costs[-1].min(axis=1))), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sampling: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    norm = orc.synthetic_normalization(S, A)
    lines = []
    for wname in args.workloads:
        wl = WORKLOADS[wname]
        K, H, E = wl["K"], wl["H"], wl["K"] // 10
        w = orc.synthetic_weights(S, A, wl["hidden"], 2, wl["act"], wl["ln"])
        spec = MLPSpec(w.kernels, w.biases, w.activation, w.ln_gamma, w.ln_beta)
        for B, single in ((1, True), (wl["B"], False)):
            eng = RolloutEngine(S, A, wl["hidden"], 2, wl["act"], wl["ln"], H, B * K, device=0)
            eng.set_weights(spec, norm, 1)
            states = np.stack([orc.synthetic_state(norm, seed=11 + b) for b in range(B)])
            rs = np.random.RandomState(B)
            mu, sd = rs.uniform(-0.3, 0.3, (B, H, A)), np.full((B, H, A), 0.5)
            row = {"workload": wname, "B": B, "K": K, "H": H, "n_elite": E, "call": "single" if single else "batched",
                   "layout": eng.info()["layout"], "kernels": kernel_times(eng, mu, sd, B, K, H, E), "calls": [],
                   "best_last_iteration": {}}
            for planner, iters in PLANNERS:
                row["calls"].append(call_times(eng, planner, iters, states, mu, sd, E, wl["timed"][0 if single else 1],
                                               single))
                row["best_last_iteration"][planner] = best_costs(eng, planner, iters, states, mu, sd, E)
            eng.check_status()
            eng.close()
            lines.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"bench": "sampling", "rho": RHO, "alpha": ALPHA, "lambda": LAMBDA, "rounds": ROUNDS,
           "device": torch.cuda.get_device_name(0), "results": lines}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

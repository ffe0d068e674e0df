#!/usr/bin/env python3
"""What episode termination (a TermCost with done conditions) costs, and what it costs those who do not use it.

Three points, each in one process, tools/bench_term_cost.py's method (a prewarm past the clock ramp, warm-up calls
of every side, then the timed calls in alternating rounds so that a drift of the shared machine falls on all
sides; p50 of the synchronous call, the kernel alone between two HIP events):

  cfg3          K = 65,536, H = 20, 2 x 500 tanh
  cfg2          K = 4,096,  H = 20, 2 x 500 tanh
  ppo_defaults  K = 400,    H = 7,  2 x 256 relu + LayerNorm

--mode plain (runs on any tree that has cost terms and a terminal value: the A/B against a parent checkout, one
process per tree, alternating; --tree names the checkout whose package is imported):

  terms_p50_ms        synchronous get_action of a cheetah_terms() engine without done
  terms_kernel_ms     term_cost_kernel alone on a rollout's trajectory (trajectory_cost_async)
  value_p50_ms        synchronous get_action of a fused-cheetah engine with a 2 x 128 critic (no step buffer)
  value_kernel_ms     terminal_value_kernel alone (terminal_value_async, values and in-place add)

--mode full (this tree) adds, on the same engines' layouts:

  done_p50_ms / done_kernel_ms   the same two figures with two done conditions added to cheetah_terms()
  done_overhead_ms, done_kernel_overhead_ms   their differences to the plain terms engine
  terminated          fraction of the candidates that terminate under the conditions
  composed_p50_ms     the alternative on an engine without the feature: rollout_async with the trajectory, the
                      trajectory to the host, cost_functions.episode_cost, np.argmin
  same_answer         the composed path and the engine agree on the winner

Prints one JSON line.  Needs the GPU: no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

S, A = 20, 6
VH, VL = 128, 2
POINTS = {
    "cfg3": dict(K=65536, H=20, hidden=500, act="tanh", ln=False),
    "cfg2": dict(K=4096, H=20, hidden=500, act="tanh", ln=False),
    "ppo_defaults": dict(K=400, H=7, hidden=256, act="relu", ln=True),
}
WARMUP, TIMED, ROUNDS = 20, 200, 4
PREWARM_S = 0.25
EVENT_REPS = 50
COMPOSED_REPS = 10
DONE_COST = 25.0


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
    ap.add_argument("--mode", default="full", choices=["plain", "full"])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose bc_mpc_amd package (and built library) is measured")
    ap.add_argument("--label", default="", help="copied into the output (which tree this is)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_termination: no GPU (the measurement has no CPU fallback)")
    from bc_mpc_amd import cost_functions as cf
    from bc_mpc_amd.engine import MLPSpec, RolloutEngine
    from oracle import mpc_oracle as orc

    full = args.mode == "full"
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

        def engine(cost):
            e = RolloutEngine(S, A, p["hidden"], 2, p["act"], p["ln"], H, K, device=0, cost=cost)
            e.set_weights(spec, norm, 1)
            return e
        engines = {"terms": engine("terms"), "value": engine("cheetah")}
        engines["terms"].set_cost_terms(cf.cheetah_terms())
        engines["value"].set_terminal_value(vspec, -1.0, 1)

        f64 = dict(dtype=torch.float64, device=dev)
        d_state = torch.from_numpy(np.ascontiguousarray(state)).to(dev)
        d_costs = torch.empty(K, **f64)
        d_traj = torch.empty((H + 1, K, S), **f64)
        d_values = torch.empty(K, dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        plain = engines["terms"]

        def composed(seed, T):
            plain.rollout_async(d_state.data_ptr(), 0, None, seed, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, st)
            traj = d_traj.cpu().numpy()                                # the whole trajectory, as a plain engine returns it
            total, t = cf.episode_cost(T, traj[:-1], np.zeros((H, 1, A)), traj[1:])
            return int(np.argmin(total)), total, t

        line = {"point": name, "K": K, "H": H, "net": f"2x{p['hidden']} {p['act']}" + (" + LayerNorm" if p["ln"] else ""),
                "layout": plain.info()["layout"]}
        plain.rollout_async(d_state.data_ptr(), 0, None, 7, 0, d_costs.data_ptr(), d_traj.data_ptr(), None, st)
        if full:
            traj = d_traj.cpu().numpy()
            T = cf.TermCost(cf.cheetah_terms().terms,
                            done=[cf.done_when(4, "<=", float(np.percentile(traj[H // 2, :, 4], 30))),
                                  cf.done_when(0, ">=", float(np.percentile(traj[H // 2, :, 0], 85)))],
                            done_cost=DONE_COST)
            engines["done"] = engine("terms")
            engines["done"].set_cost_terms(T)
            best_c, total_c, t_c = composed(7, T)
            got = engines["done"].get_action(state, None, seed=7, return_costs=True)
            line["same_answer"] = bool(got.best_index == best_c)
            line["composed_bit_equal"] = bool(np.array_equal(got.costs, total_c, equal_nan=True))
            line["terminated"] = round(float((t_c < H).mean()), 4)
            line["done_layout"] = engines["done"].info()["layout"]

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

        def event_ms(fn):
            x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            x.record()
            fn()
            y.record()
            y.synchronize()
            return x.elapsed_time(y)

        kernels = {"value": lambda: engines["value"].terminal_value_async(
            d_traj[H].data_ptr(), K, d_values=d_values.data_ptr(), d_costs=d_costs.data_ptr(), stream=st)}
        for k in ("terms", "done"):
            if k in engines:
                kernels[k] = lambda e=engines[k]: e.trajectory_cost_async(d_traj.data_ptr(), K, d_costs.data_ptr(),
                                                                          stream=st)
        kms = {k: [] for k in kernels}
        for fn in kernels.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for rnd in range(ROUNDS):                                       # alternating, as the calls above
            for k, fn in kernels.items():
                kms[k] += [event_ms(fn) for _ in range(EVENT_REPS // ROUNDS + 1)]
        plain.check_status()
        for k in sides:
            line[k + "_p50_ms"] = pct(ts[k], 50)
            line[k + "_p10_ms"] = pct(ts[k], 10)
            line[k + "_p90_ms"] = pct(ts[k], 90)
            line[k + "_kernel_ms"] = round(float(np.median(kms[k])), 4)
        if full:
            line["done_overhead_ms"] = round(line["done_p50_ms"] - line["terms_p50_ms"], 4)
            line["done_kernel_overhead_ms"] = round(line["done_kernel_ms"] - line["terms_kernel_ms"], 4)
            tc = []
            for i in range(COMPOSED_REPS + 2):
                t = time.perf_counter()
                composed(3000 + i, T)
                tc.append(time.perf_counter() - t)
            line["composed_p50_ms"] = pct(tc[2:], 50)
            line["traj_mb"] = round((H + 1) * K * S * 8 / 1e6, 2)
        line["prewarm_calls"] = calls
        lines.append(line)
        for e in engines.values():
            e.close()
    out = {"bench": "termination", "mode": args.mode, "label": args.label, "warmup": WARMUP, "timed": TIMED,
           "rounds": ROUNDS, "event_reps": EVENT_REPS, "composed_reps": COMPOSED_REPS,
           "device": torch.cuda.get_device_name(0), "results": lines}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

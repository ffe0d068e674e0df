#!/usr/bin/env python3
"""Batched control step against B sequential get_action calls, at train_mpc_ppo.py's own defaults.

Workload: the ppo_defaults net (2 x 256 relu + LayerNorm, H = 7, K = 400 candidates per environment),
B in {1, 8, 64, 256} environments.  For each B, in one process:

  batched     p50 of the synchronous RolloutEngine.get_actions(states[B, S]) on a B*400-candidate engine
  sequential  p50 of B RolloutEngine.get_action calls in a row on one 400-candidate engine (environment b at
              cand_offset b*400: the same candidates, so the same answers up to the kernel layout's rounding)

Both sides draw their actions in the kernel (Philox) and end in the call's own host synchronisation, so the
host clock around a call is the call's latency.  Per B: a prewarm of the batched call past the clock ramp (as
bench.py's prewarm), 20 warm-up calls of each side, then 200 timed calls of each side taken in four
alternating rounds of 50, so that a drift of the shared machine falls on both.  Afterwards 20 batched calls
with kernel timing on give the chain's device times (tile + rollout | argmin).

Prints one JSON line (profiles/batch_ppo_defaults.json is a committed run).  Needs the GPU: no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

S, A, HIDDEN, H, K = 20, 6, 256, 7, 400
WARMUP, TIMED, ROUNDS = 20, 200, 4
PREWARM_S = 0.25


def p50_ms(ts):
    return float(np.percentile(np.asarray(ts), 50) * 1e3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 8, 64, 256])
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_batch: no GPU (the measurement has no CPU fallback)")
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
        rows = [np.ascontiguousarray(s) for s in states]
        eng = engine(B * K)

        def batched(seed):
            return eng.get_actions(states, None, seed=seed)

        def sequential(seed):
            return [one.get_action(rows[b], None, seed=seed, cand_offset=b * K) for b in range(B)]

        # prewarm past the clock ramp with the batched call itself, then both sides' warm-up
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < PREWARM_S or calls < 3:
            batched(1 << 40 | calls)
            calls += 1
        for i in range(WARMUP):
            batched(1000 + i)
        for i in range(WARMUP):
            sequential(1000 + i)
        tb, ts = [], []
        per = TIMED // ROUNDS
        for rnd in range(ROUNDS):
            for i in range(per):
                t = time.perf_counter()
                batched(2000 + rnd * per + i)
                tb.append(time.perf_counter() - t)
            for i in range(per):
                t = time.perf_counter()
                sequential(2000 + rnd * per + i)
                ts.append(time.perf_counter() - t)
        # same candidates on both sides: the winners agree unless the two layouts' rounding reorders a near-tie
        rb, rs = batched(7), sequential(7)
        agree = int(sum(int(rb.best_index[b]) == rs[b].best_index for b in range(B)))
        eng.set_timing(True)
        km = []
        for i in range(20):
            batched(3000 + i)
            km.append(eng.last_kernel_ms())
        eng.set_timing(False)
        km = np.median(np.asarray(km), axis=0)
        line = {"B": B, "K": K, "batched_p50_ms": round(p50_ms(tb), 4), "sequential_p50_ms": round(p50_ms(ts), 4),
                "sequential_per_call_ms": round(p50_ms(ts) / B, 4),
                "speedup": round(p50_ms(ts) / p50_ms(tb), 2),
                "batched_p10_ms": round(float(np.percentile(tb, 10) * 1e3), 4),
                "batched_p90_ms": round(float(np.percentile(tb, 90) * 1e3), 4),
                "sequential_p10_ms": round(float(np.percentile(ts, 10) * 1e3), 4),
                "sequential_p90_ms": round(float(np.percentile(ts, 90) * 1e3), 4),
                "batched_rollout_kernel_ms": round(float(km[0]), 4), "batched_argmin_kernel_ms": round(float(km[1]), 4),
                "batched_layout": eng.info()["layout"], "winners_agree": agree, "prewarm_calls": calls}
        lines.append(line)
        eng.close()
    out = {"bench": "batch_ppo_defaults", "net": "2x256 relu + LayerNorm", "H": H, "K_per_env": K,
           "warmup": WARMUP, "timed": TIMED, "rounds": ROUNDS, "sequential_layout": one.info()["layout"],
           "device": torch.cuda.get_device_name(0), "results": lines}
    one.close()
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

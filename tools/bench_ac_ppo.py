"""Time the PPO trainer (csrc/ac_ppo.hip) at the reference shape and write profiles/ac_ppo.json.

train_mpc_ppo.py:355-372: 500 epochs (optim_epochs) of one PPO step and one BC step on the 20 -> 128 -> 128 -> 6
tanh policy and the 20 -> 128 -> 128 -> 1 critic.  Per batch size (128, 64: the reference's flag and function
defaults), on the graph path and on the per-step launch path, us per step and ms per 500-step epoch of

* the PPO step alone,
* the PPO + BC pair,
* the yardstick, from the SAME process: one BC step plus one critic step of the two single-head fitters
  (csrc/ac_fit.hip), each timed as its own 500-step run, their times added,
* the definition (bc_mpc_amd/ppo.py, NumPy) per PPO step on the host's BLAS threads.

Median of ``--reps`` epochs after a warm-up epoch (which also captures the graph), wall time around ``run`` with the
indices already drawn, as tools/bench_ac_fit.py measures: a run ends with the stream's synchronisation, so the
wall time of a 500-step run is the device chain's time plus one submission.

usage: python tools/bench_ac_ppo.py [--steps 500] [--reps 7] [--cpu-steps 50] [--out profiles/ac_ppo.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps):
    fn()                                                  # warm-up (and the capture)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-steps", type=int, default=50)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ac_ppo.json"))
    args = ap.parse_args()
    import torch  # noqa: F401  (single HIP runtime)
    from bc_mpc_amd import ac_fit, ppo
    from oracle import mpc_oracle as orc
    S, A, h, L, lr, eps, entc = 20, 6, 128, 2, 3e-4, 0.2, 0.0
    rs = np.random.RandomState(5)
    wp, wv = orc.synthetic_policy(S, A, h, L), orc.synthetic_policy(S, 1, h, L, seed=2025)
    flt = (wp.ob_mean, wp.ob_std)
    n = args.rows
    obs = wp.ob_mean.astype(np.float64) + 1.5 * wp.ob_std.astype(np.float64) * rs.standard_normal((n, S))
    pol, vf = [], []
    for k, b in zip(wp.kernels, wp.biases):
        pol += [k, b]
    for k, b in zip(wv.kernels, wv.biases):
        vf += [k, b]
    logstd = np.full(A, -0.5, np.float32)
    oldmean = ppo.snapshot_old(pol, flt, obs)
    acs = oldmean.astype(np.float64) + np.exp(-0.5) * rs.standard_normal((n, A))
    atarg, ret = ppo.standardize(rs.standard_normal(n)), 3.0 * rs.standard_normal(n)
    bc_acs = rs.uniform(-1, 1, (n, A))
    results = []
    for B in (128, 64):
        batches = [rs.choice(n, B, replace=False) for _ in range(args.steps)]
        bcb = [rs.choice(n, B, replace=False) for _ in range(args.steps)]
        rec = {"shape": f"{S}->{h}x{L}->{A} + {S}->{h}x{L}->1 tanh", "batch": B, "steps": args.steps}
        for path, env in (("graph", "1"), ("launch", "0")):
            os.environ["BCMPC_ACPPO_GRAPH"] = os.environ["BCMPC_ACFIT_GRAPH"] = env
            pf = ac_fit.ActorCriticFitter("policy", S, A, h, L, batch_size=B)
            vfit = ac_fit.ActorCriticFitter("value", S, 1, h, L, batch_size=B)
            pf.set_params(pol[0::2], pol[1::2])
            vfit.set_params(vf[0::2], vf[1::2])
            pf.set_filter(*flt)
            vfit.set_filter(*flt)
            pf.set_data(obs, bc_acs)
            vfit.set_data(obs, ret)
            # the yardstick first, on the untrained weights: the parent's two single-head steps
            t_bc = timed(lambda: pf.run(bcb, lr), args.reps)
            t_v = timed(lambda: vfit.run(batches, lr), args.reps)
            assert (pf.graph_captures == 1) == (path == "graph")
            pf.set_params(pol[0::2], pol[1::2])
            vfit.set_params(vf[0::2], vf[1::2])
            t = ppo.PpoTrainer(pf, vfit)
            t.set_logstd(logstd)
            t.set_old(pol[0::2], pol[1::2], flt[0], flt[1], logstd)
            t.set_data(obs, acs, atarg, ret)
            t_ppo = timed(lambda: t.run(batches, lr, eps, entc), args.reps)
            assert (t.graph_captures >= 1) == (path == "graph")
            t_pair = timed(lambda: t.run(batches, lr, eps, entc, bc_batches=bcb, bc_lr=lr), args.reps)
            t.close()
            pf.close()
            vfit.close()
            for name, tm in (("ppo", t_ppo), ("ppo_bc_pair", t_pair), ("bc_alone", t_bc), ("critic_alone", t_v)):
                rec[f"{path}_{name}_us_per_step"] = tm[0] / args.steps * 1e6
                rec[f"{path}_{name}_ms_per_epoch_min_max"] = [tm[1] * 1e3, tm[2] * 1e3]
            rec[f"{path}_yardstick_bc_plus_critic_us_per_step"] = (t_bc[0] + t_v[0]) / args.steps * 1e6
        os.environ.pop("BCMPC_ACPPO_GRAPH", None)
        os.environ.pop("BCMPC_ACFIT_GRAPH", None)
        p2, v2, ls = [x.copy() for x in pol], [x.copy() for x in vf], logstd.copy()
        st = ac_fit.AdamState.zeros_like(p2 + v2 + [ls])
        ppo.run(p2, v2, ls, st, flt, obs, acs, atarg, ret, oldmean, logstd, batches[:5], lr, eps, entc)
        t0 = time.perf_counter()
        ppo.run(p2, v2, ls, st, flt, obs, acs, atarg, ret, oldmean, logstd, batches[:args.cpu_steps], lr, eps, entc)
        rec["definition_us_per_step"] = (time.perf_counter() - t0) / args.cpu_steps * 1e6
        rec["definition_threads"] = os.environ.get("OMP_NUM_THREADS", "default")
        results.append(rec)
        print(json.dumps(rec))
    doc = {"metric": "PPO trainer: clipped-surrogate step time against one BC step plus one critic step",
           "reps": args.reps, "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
